"""Spatial autoencoder training on the MI355X: SpatialModel forward under grad + loss.backward() + the fused AdamW, against the reference's own
autograd (fixtures of tests/golden/make_encoder_train_fixtures.py) and the CPU oracle in fp64."""
import copy

import numpy as np
import pytest
import torch

from oracle import sea_oracle as O
from tests.conftest import load_golden, rel_l2
from tests.test_encoder_train_cpu import FIXTURES, fixture_config

pytestmark = pytest.mark.gpu


def _errs(got, want):
    """Per-parameter rel-L2; a parameter whose reference gradient is zero by construction (attn_1.k.bias: softmax is shift-invariant) is measured
    against the median gradient norm instead."""
    med = float(np.median([np.linalg.norm(np.asarray(w, np.float64)) for w in want.values()]))
    out = {}
    for k, w in want.items():
        w = np.asarray(w, np.float64)
        g = np.asarray(got[k], np.float64)
        out[k] = float(np.linalg.norm(g - w) / max(np.linalg.norm(w), 1e-3 * med))
    return out


def _model(cfg, params, dtype):
    from sea_amd.models.encoder_decoder import SpatialModel

    m = SpatialModel(cfg["field_groups"], cfg["n_inp"], cfg["MLP_hidden"], cfg["num_layers"], cfg["embed_dim"], cfg["n_heads"], cfg["block_size"], 0,
                     dropout=0.0)
    with torch.no_grad():
        for k, p in m.named_parameters():
            p.copy_(torch.as_tensor(np.asarray(params[k])))
    return m.set_compute_dtype(dtype).to("cuda:0").train()


def _loss_backward(m, x):
    from sea_amd.utils.train_utils import SeaMSELoss

    xd = x.clone().cuda()
    out = m(xd)
    loss = SeaMSELoss()(out, xd)
    loss.backward()
    return float(loss.detach()), xd


def _grads(m):
    return {k: p.grad.detach().cpu().numpy() for k, p in m.named_parameters()}


@pytest.mark.parametrize("name", FIXTURES)
@pytest.mark.parametrize("dtype,tol", [("fp32", 1e-4), ("bf16", 3e-2)])
def test_gradients_and_adamw_match_reference(name, dtype, tol):
    from sea_amd.utils.train_utils import initialize_optimizer

    z = load_golden(name)
    cfg, _, _ = fixture_config(z)
    init = {k[len("init."):]: z[k] for k in z.files if k.startswith("init.")}
    m = _model(cfg, init, dtype)
    x = torch.from_numpy(z["x"])
    loss, xd = _loss_backward(m, x)
    assert np.array_equal(xd.cpu().numpy(), z["x_masked"]), "the input is masked in place, as the reference's loop relies on"
    assert abs(loss - float(z["loss"])) <= tol * abs(float(z["loss"]))
    errs = _errs(_grads(m), {k: z["grad." + k] for k in init})
    bad = {k: e for k, e in errs.items() if not e <= tol}
    assert not bad, bad

    m = _model(cfg, init, dtype)
    opt = initialize_optimizer(m, dict(learning_rate=float(z["lr"])))
    for _ in range(int(z["steps"])):
        opt.zero_grad()
        _loss_backward(m, x)
        opt.step()
    after = {k: p.detach().cpu().numpy() for k, p in m.named_parameters()}
    # relative to the parameter change, not the parameter: three steps of lr 1e-3 move every weight by ~3e-3.  attn_1.k.bias is left out here:
    # its gradient is zero up to round-off, and Adam's normalised step turns round-off into a full-size step of either sign (on both sides)
    live = [k for k in init if not k.endswith("attn_1.k.bias")]
    moved = {k: after[k] - init[k] for k in live}
    want = {k: z["after3." + k] - init[k] for k in live}
    errs = _errs(moved, want)
    bad = {k: e for k, e in errs.items() if not e <= (1e-3 if dtype == "fp32" else 0.2)}
    assert not bad, bad
    for k in live:
        assert rel_l2(after[k], z["after3." + k]) < (1e-5 if dtype == "fp32" else 1e-2), k
    for k in set(init) - set(live):   # an Adam step moves a parameter by at most ~lr per step
        assert np.abs(after[k] - init[k]).max() <= 1.01 * float(z["lr"]) * int(z["steps"]), k


def _oracle_grads(cfg, params, x):
    p = {k: torch.as_tensor(np.asarray(v)).double().requires_grad_(True) for k, v in params.items()}
    xr = x.double().clone()
    xr[xr == -9999] = 0.0
    enc = {k[len("encode."):]: v for k, v in p.items() if k.startswith("encode.")}
    out = O.decode(O.encode(xr, enc, cfg["field_groups"], cfg["n_heads"], cfg["num_layers"]), p, cfg["field_groups"], pre="decode.decoders.")
    loss = ((out - xr) ** 2).mean()
    loss.backward()
    return float(loss.detach()), {k: v.grad.numpy() for k, v in p.items()}


def _shipped(E, hidden, n_inp=40, seed=0):
    from sea_amd.models.encoder_decoder import SpatialModel

    cfg = dict(field_groups=[[0, 1], [2]], n_inp=n_inp, MLP_hidden=hidden, num_layers=12, embed_dim=E, n_heads=8, block_size=81)
    torch.manual_seed(seed)
    m = SpatialModel(cfg["field_groups"], n_inp, hidden, 12, E, 8, 81, 0, dropout=0.0)
    with torch.no_grad():   # non-trivial LayerNorm parameters and biases
        for k, p in m.named_parameters():
            if k.endswith("bias") or "ln" in k or "layers.1" in k:
                p.add_(0.1 * torch.randn_like(p))
    params = {k: p.detach().clone().numpy() for k, p in m.named_parameters()}
    return cfg, params


@pytest.mark.parametrize("E,hidden", [(16, 480), (32, 624)])
def test_shipped_widths_bf16_against_oracle(E, hidden):
    """The shipped spatial configs (W = 32 with head dim 4 padded to 8, W = 64 with head dim 8; 12 layers, 81 patches), 3 snapshots, bf16 gradients
    against fp64 autograd of the oracle.  Stated tolerance: 5e-2 rel-L2 per parameter (bf16 operands through 12 layers and back)."""
    cfg, params = _shipped(E, hidden)
    rng = np.random.Generator(np.random.PCG64(E))
    x = torch.from_numpy(rng.standard_normal((3, 81, 3, cfg["n_inp"])).astype(np.float32))
    x[0, :4, 1, :7] = -9999.0
    ref_loss, ref = _oracle_grads(cfg, params, x)
    m = _model(cfg, params, "bf16")
    loss, _ = _loss_backward(m, x)
    assert abs(loss - ref_loss) < 2e-2 * ref_loss
    errs = _errs(_grads(m), ref)
    bad = {k: e for k, e in errs.items() if not e <= 5e-2}
    assert not bad, (bad, max(errs.values()))


def test_gradients_accumulate_until_zero_grad():
    z = load_golden("encoder_train_cyl_small")
    cfg, _, _ = fixture_config(z)
    init = {k[len("init."):]: z[k] for k in z.files if k.startswith("init.")}
    m = _model(cfg, init, "fp32")
    x = torch.from_numpy(z["x"])
    _loss_backward(m, x)
    one = _grads(m)
    _loss_backward(m, x)
    two = _grads(m)
    for k in ("encode.blocks.1.mlp_1.layers.0.weight", "encode.blocks.1.mlp_1.layers.3.weight", "encode.blocks.0.attn_1.q.weight",
              "encode.blocks.0.attn_1.k.weight", "encode.blocks.0.attn_1.v.weight", "decode.decoders.0.layer2.weight", "encode.encoders.1.layer1.weight"):
        assert rel_l2(two[k], 2 * one[k]) < 1e-5, k
    from sea_amd.utils.train_utils import initialize_optimizer

    opt = initialize_optimizer(m, dict(learning_rate=1e-3))
    opt.zero_grad()
    assert all(p.grad is None for p in m.parameters())
    _loss_backward(m, x)
    again = _grads(m)
    assert rel_l2(again["encode.blocks.0.attn_1.v.weight"], one["encode.blocks.0.attn_1.v.weight"]) < 1e-5


@pytest.mark.parametrize("dtype,tol", [("fp32", 1e-4), ("bf16", 3e-2)])
def test_inference_after_step_uses_updated_weights(dtype, tol):
    """The encoder's / decoder's activation-dtype packs are keyed on tensor versions, which a raw-pointer AdamW write does not bump: after
    optimizer.step() a no_grad forward must still see the new parameters."""
    from sea_amd.utils.train_utils import initialize_optimizer

    z = load_golden("encoder_train_three_groups")
    cfg, _, _ = fixture_config(z)
    init = {k[len("init."):]: z[k] for k in z.files if k.startswith("init.")}
    m = _model(cfg, init, dtype)
    x = torch.from_numpy(z["x"])
    with torch.no_grad():
        before = m.eval()(x.clone().cuda()).cpu()   # builds the packs
    m.train()
    opt = initialize_optimizer(m, dict(learning_rate=1e-2))
    opt.zero_grad()
    _loss_backward(m, x)
    opt.step()
    new = {k: p.detach().cpu().double() for k, p in m.named_parameters()}
    xr = x.double().clone()
    xr[xr == -9999] = 0.0
    enc = {k[len("encode."):]: v for k, v in new.items() if k.startswith("encode.")}
    ref = O.decode(O.encode(xr, enc, cfg["field_groups"], cfg["n_heads"], cfg["num_layers"]), new, cfg["field_groups"], pre="decode.decoders.")
    with torch.no_grad():
        after = m.eval()(x.clone().cuda()).cpu()
    assert rel_l2(after.numpy(), ref.numpy()) < tol
    assert rel_l2(before.numpy(), ref.numpy()) > 10 * tol   # the step did move the output


class _Tracker:
    def __init__(self):
        self.records, self.finished, self.logged = [], False, False

    def log_model(self, model, criterion, optimizer):
        self.logged = True

    def record_error(self, phase, epoch, metrics):
        self.records.append((phase, epoch, dict(metrics)))

    def finish(self):
        self.finished = True


def test_train_loop_checkpoint_and_latents(tmp_path):
    from sea_amd.models.encoder_decoder import SpatialModel
    from sea_amd.train.train_encoder import train

    rng = np.random.Generator(np.random.PCG64(5))
    base = rng.standard_normal((1, 9, 3, 12)).astype(np.float32)
    data = [torch.from_numpy(base + 0.1 * rng.standard_normal((4, 9, 3, 12)).astype(np.float32)) for _ in range(3)]
    data[0][0, 0, 0, :3] = -9999.0
    val = [torch.from_numpy(base + 0.1 * rng.standard_normal((4, 9, 3, 12)).astype(np.float32))]
    cfg = dict(field_groups=[[0, 1], [2]], n_inp=12, MLP_hidden=32, num_layers=2, embed_dim=16, n_heads=8, block_size=9, src_len=0,
               variational=False, dropout=0.0, learning_rate=1e-3, epoch_num=3, validation_interval=1, device="cuda:0", save_dir=str(tmp_path),
               case_name="tiny", run_name="t", loaders=(data, val, None))
    tr = _Tracker()
    torch.manual_seed(0)
    model = train(cfg, tr)
    assert tr.logged and tr.finished
    train_losses = [r[2]["Loss"] for r in tr.records if r[0] == "train"]
    assert len(train_losses) == 3 and train_losses[-1] < train_losses[0], train_losses
    assert [r[1] for r in tr.records if r[0] == "val"] == [1, 2, 3]
    path = tmp_path / "encoder_decoder_tiny_t.pt"
    assert path.exists()
    sd = torch.load(path, map_location="cpu")
    fresh = SpatialModel(cfg["field_groups"], 12, 32, 2, 16, 8, 9, 0, dropout=0.0)
    fresh.load_state_dict(sd, strict=True)
    fresh = fresh.to("cuda:0").eval()
    model.eval()
    xv = val[0].cuda()
    with torch.no_grad():
        a, b = fresh.encode(xv), model.encode(xv)
    val_losses = [r[2]["Loss"] for r in tr.records if r[0] == "val"]
    assert min(val_losses) == val_losses[-1], val_losses   # the last epoch is the best: the checkpoint holds the trained parameters
    assert torch.equal(a, b)


def test_dropout_refused_and_inference_untouched():
    from sea_amd.models.encoder_decoder import SpatialModel
    from sea_amd.utils.train_utils import initialize_optimizer

    md = SpatialModel([[0, 1], [2]], 12, 32, 1, 16, 8, 9, 0, dropout=0.1).to("cuda:0").train()
    with pytest.raises(NotImplementedError, match="0.0"):
        md(torch.zeros(2, 9, 3, 12, device="cuda:0"))
    torch.manual_seed(1)
    m = SpatialModel([[0, 1], [2]], 12, 32, 2, 16, 8, 9, 0, dropout=0.0).set_compute_dtype("bf16").to("cuda:0")
    x = torch.randn(3, 9, 3, 12, device="cuda:0")
    with torch.no_grad():
        before = m(x.clone())
    c = copy.deepcopy(m).train()
    opt = initialize_optimizer(c, dict(learning_rate=1e-3))
    opt.zero_grad()
    _loss_backward(c, x.cpu())
    opt.step()
    with torch.no_grad():
        after = m(x.clone())
        trained = c(x.clone())
    assert torch.equal(before, after)
    assert not torch.equal(before, trained)


def _fused_vs_composed_case(E, hidden, B):
    cfg, params = _shipped(E, hidden, n_inp=40, seed=E + B)
    rng = np.random.Generator(np.random.PCG64(100 + B))
    x = torch.from_numpy(rng.standard_normal((B, 81, 3, cfg["n_inp"])).astype(np.float32))
    x[0, :3, 0, :5] = -9999.0
    return cfg, params, x


@pytest.mark.parametrize("E,hidden", [(16, 480), (32, 624)])
@pytest.mark.parametrize("B", [1, 3, 5])
def test_fused_blocks_match_composed(E, hidden, B, monkeypatch):
    """bf16 at both shipped widths, snapshot counts 1 / 3 / 5: the fused EncoderBlock launches (sea_encoder_block_fwd / _bwd) against the composed form
    (the default; SEA_PLAN=enc=fused selects the fused form).  Stated tolerance: loss 1e-2 relative, every gradient 1e-1 rel-L2 — each form is held within 5e-2 of fp64 autograd
    (test_shipped_widths_bf16_against_oracle, test_fused_gradients_against_oracle), so two bf16 forms may differ by the sum; the small q / k gradients
    (through the softmax) come closest to it, at one snapshot.  The fused block keeps its intermediates in fp32, the composed one rounds them to
    bf16 between launches."""
    cfg, params, x = _fused_vs_composed_case(E, hidden, B)
    monkeypatch.setenv("SEA_PLAN", "enc=composed")
    mc = _model(cfg, params, "bf16")
    lc, _ = _loss_backward(mc, x)
    gc = _grads(mc)
    assert mc.engine().launches > 0
    monkeypatch.setenv("SEA_PLAN", "enc=fused")
    mf = _model(cfg, params, "bf16")
    lf, _ = _loss_backward(mf, x)
    gf = _grads(mf)
    # 12 blocks: one forward launch each, two backward launches each, plus the same down-scale / final norm / decoder launches as composed
    assert mf.engine().launches < mc.engine().launches - 12 * 10
    assert abs(lf - lc) <= 1e-2 * lc, (lf, lc)
    errs = _errs(gf, gc)
    bad = {k: e for k, e in errs.items() if not e <= 1e-1}
    assert not bad, (bad, max(errs.values()))
    assert np.median(list(errs.values())) < 1e-2


def test_fused_block_launch_counts(monkeypatch):
    """The fused form issues exactly 1 launch per block forward and 2 per block backward."""
    cfg, params, x = _fused_vs_composed_case(16, 480, 2)
    counts = {}
    for form in ("composed", "fused"):
        monkeypatch.setenv("SEA_PLAN", f"enc={form}")
        m = _model(cfg, params, "bf16")
        eng = m.engine()
        a = eng.launches
        xd = x.clone().cuda()
        out = m(xd)
        b = eng.launches
        from sea_amd.utils.train_utils import SeaMSELoss

        SeaMSELoss()(out, xd).backward()
        counts[form] = (b - a, eng.launches - b)
    (cf, cb), (ff, fb) = counts["composed"], counts["fused"]
    assert cf - ff == 12 * (8 - 1), counts     # composed: 8 launches per block forward (norm, qkv, attention, proj, norm, fc1, norm+gelu, fc2)
    assert cb - fb > 12 * (10 - 2), counts


def test_fused_gradients_against_oracle(monkeypatch):
    """The fused blocks (SEA_PLAN=enc=fused) through the full model at W = 64 against fp64 oracle autograd."""
    monkeypatch.setenv("SEA_PLAN", "enc=fused")
    cfg, params = _shipped(32, 624, seed=3)
    rng = np.random.Generator(np.random.PCG64(77))
    x = torch.from_numpy(rng.standard_normal((2, 81, 3, cfg["n_inp"])).astype(np.float32))
    ref_loss, ref = _oracle_grads(cfg, params, x)
    m = _model(cfg, params, "bf16")
    loss, _ = _loss_backward(m, x)
    assert m.engine().launches > 0
    assert abs(loss - ref_loss) < 2e-2 * ref_loss
    errs = _errs(_grads(m), ref)
    bad = {k: e for k, e in errs.items() if not e <= 5e-2}
    assert not bad, (bad, max(errs.values()))
