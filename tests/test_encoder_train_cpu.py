"""Spatial autoencoder training, host side: calculate_R2, get_model's parameter schema, and the fixtures themselves against the CPU oracle."""
import numpy as np
import pytest
import torch

from oracle import sea_oracle as O
from tests.conftest import load_golden

FIXTURES = ("encoder_train_cyl_small", "encoder_train_three_groups")


def grad_err(a, b, floor=1e-4):
    """rel-L2 with an absolute floor on the denominator (for gradients that are zero by construction)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), floor))


def fixture_config(z):
    n_inp, hidden, layers, E, H, B, P = (int(v) for v in z["meta"])
    fg = [int(v) for v in z["field_groups"]]
    groups, f = [], 0
    for g in range(max(fg) + 1):
        n = fg.count(g)
        groups.append(list(range(f, f + n)))
        f += n
    return dict(field_groups=groups, n_inp=n_inp, MLP_hidden=hidden, num_layers=layers, embed_dim=E, n_heads=H, block_size=P, src_len=0,
                variational=False, dropout=0.0, learning_rate=1e-3, epoch_num=1), B, P


def test_calculate_r2_matches_formula():
    from sea_amd.utils.train_utils import calculate_R2

    g = torch.Generator().manual_seed(0)
    y = torch.randn(4, 5, 3, generator=g, dtype=torch.float64)
    p = y + 0.3 * torch.randn(4, 5, 3, generator=g, dtype=torch.float64)
    yn, pn = y.numpy().ravel(), p.numpy().ravel()
    want = 1.0 - ((pn - yn) ** 2).sum() / ((yn - yn.mean()) ** 2).sum()
    assert abs(float(calculate_R2(p, y)) - want) < 1e-12
    assert float(calculate_R2(y, y)) == 1.0


@pytest.mark.parametrize("name", FIXTURES)
def test_get_model_parameter_names_match_reference(name):
    from sea_amd.train.train_encoder import get_model

    z = load_golden(name)
    cfg, _, _ = fixture_config(z)
    model, loss_fn, opt = get_model(cfg, torch.device("cpu"))
    want = sorted(k[len("init."):] for k in z.files if k.startswith("init."))
    assert sorted(k for k, _ in model.named_parameters()) == want
    for k, p in model.named_parameters():
        assert tuple(p.shape) == z["init." + k].shape, k
    assert "encode.spatial_pos_encoder.pe" in model.state_dict()


def test_train_encoder_needs_loaders():
    from sea_amd.train.train_encoder import train

    with pytest.raises(RuntimeError, match="loaders"):
        train(dict(device="cpu"), None)


def _oracle_loss_and_grads(z):
    cfg, B, P = fixture_config(z)
    p = {k[len("init."):]: torch.from_numpy(z["init." + k[len("init."):]]).double().requires_grad_(True) for k in z.files if k.startswith("init.")}
    x = torch.from_numpy(z["x"]).double()
    x[x == -9999] = 0.0
    enc = {k[len("encode."):]: v for k, v in p.items() if k.startswith("encode.")}
    zlat = O.encode(x, enc, cfg["field_groups"], cfg["n_heads"], cfg["num_layers"])
    out = O.decode(zlat, p, cfg["field_groups"], pre="decode.decoders.")
    loss = ((out - x) ** 2).mean()
    loss.backward()
    return x, loss, {k: v.grad for k, v in p.items()}


@pytest.mark.parametrize("name", FIXTURES)
def test_oracle_reproduces_fixture_gradients(name):
    """Pins the fixtures (reference autograd) to the oracle's formulas, not the feature."""
    z = load_golden(name)
    x, loss, grads = _oracle_loss_and_grads(z)
    assert np.abs(x.numpy() - z["x_masked"]).max() == 0.0
    assert abs(float(loss.detach()) - float(z["loss"])) <= 1e-6 * abs(float(z["loss"]))
    for k, g in grads.items():   # attn_1.k.bias has a zero gradient (softmax is shift-invariant): an absolute floor
        assert grad_err(g.numpy(), z["grad." + k]) < 1e-5, k


def _enc_block_lib():
    from sea_amd import build, _native

    build.build(verbose=False)
    return _native


def test_encoder_block_entry_points_refuse_bad_arguments():
    """sea_encoder_block_fwd / _bwd validate on the host: -1 with a message for null or oversized arguments, -3 for fp32 and unsupported shapes."""
    import ctypes as C

    N = _enc_block_lib()
    L = N.lib()
    for fn in (L.sea_encoder_block_fwd, L.sea_encoder_block_bwd):
        assert fn(None, N.SEA_BF16, None) == -1
        assert b"null params" in L.sea_last_error()
        p = N.SeaEncBlock()
        p.B, p.P, p.W, p.H, p.eps = 4, 81, 32, 8, 1e-5
        assert fn(C.byref(p), N.SEA_BF16, None) == -1          # null operands
        assert b"null pointer" in L.sea_last_error()
        fake = 1 << 40
        for k in ("Zin", "Zout", "wqkv", "bqkv", "wo", "w1", "b1", "lnw", "lnb", "w2", "b2", "g1", "g2", "dZout", "n1", "dqkv", "att", "dz1", "n2",
                  "dh", "hg", "dz2", "u1", "u2", "u3w", "u3b", "ws"):
            setattr(p, k, fake)
        p.dZin = fake + 4096
        p.ws_floats = L.sea_encoder_block_ws_floats(4, 81, 32) - 1      # one float short
        assert fn(C.byref(p), N.SEA_BF16, None) == -1
        assert b"workspace" in L.sea_last_error()
        p.ws_floats += 1
        p.B = 1 << 20                                                     # more snapshots than the grid holds
        assert fn(C.byref(p), N.SEA_BF16, None) == -1
        p.B = 4
        assert fn(C.byref(p), N.SEA_F32, None) == -3                    # fp32: compose instead
        for W, H, P in ((48, 8, 81), (32, 4, 81), (64, 8, 129)):
            p.W, p.H, p.P = W, H, P
            assert fn(C.byref(p), N.SEA_BF16, None) == -3, (W, H, P)
            assert b"unsupported" in L.sea_last_error()
        p.W, p.H, p.P = 32, 8, 81
    assert L.sea_encoder_block_ws_floats(2, 81, 48) == 0


def test_encoder_block_supported_shapes():
    import torch as T

    from sea_amd import ops

    assert ops.encoder_block_supported(T.bfloat16, 32, 8, 81) and ops.encoder_block_supported(T.bfloat16, 64, 8, 128)
    assert not ops.encoder_block_supported(T.float32, 32, 8, 81)
    assert not ops.encoder_block_supported(T.bfloat16, 48, 6, 81)
    assert not ops.encoder_block_supported(T.bfloat16, 64, 8, 129)
