"""Decoded-field loss (sea_decode_mse, Decode.mse_loss, FieldSpaceLoss) without a GPU: the contract restated in fp64 reproduces what the
reference's Decode + F.mse_loss give (tests/golden/decode_mse_*.npz, written by tests/golden/make_decode_mse_fixtures.py), the entry point is
exported and checks its arguments before touching a device, and the Python layers refuse malformed arguments, CPU tensors and a trainable decoder.

`restate` below is the reference every GPU test of tests/test_decode_loss_gpu.py compares with."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


# ------------------------------------------------------------------------------------------------ the contract, in fp64
def restate(w1, w2, b2, field_groups, z, target, counts=None):
    """include/sea_hip.h, sea_decode_mse, with the two small ends around it, in fp64 and without autograd.
    w1[g] [S, D], w2[g] [n_g * C, S], b2[g] [n_g * C]; z [B, P, G, D]; target [B, P, F, >= C]; counts: P integers or None.
    Returns (loss, dz [B, P, G, D], dH list of [M, S])."""
    f64 = torch.float64
    B, P, G, D = z.shape
    M = B * P
    n_f = [len(g) for g in field_groups]
    C_ = w2[0].shape[0] // n_f[0]
    zz = z.detach().to(f64).reshape(M, G, D)
    tgt = target.detach().to(f64)[..., :C_].reshape(M, sum(n_f), C_)
    if counts is None:
        valid = torch.ones(M, 1, C_, dtype=torch.bool)
        n = M * sum(n_f) * C_
    else:
        cnt = torch.as_tensor(counts).clamp(0, C_)
        valid = (torch.arange(C_) < cnt[torch.arange(M) % P, None]).view(M, 1, C_)
        n = B * sum(n_f) * int(cnt.sum())
    loss = torch.zeros((), dtype=f64)
    resid, pres = [], []
    f0 = 0
    for g in range(G):
        pre = zz[:, g] @ w1[g].to(f64).t()
        H = 0.5 * pre * (1.0 + torch.erf(pre / math.sqrt(2.0)))
        Y = (H @ w2[g].to(f64).t() + b2[g].to(f64)).view(M, n_f[g], C_)
        Dm = torch.where(valid, Y - tgt[:, f0:f0 + n_f[g]], torch.zeros((), dtype=f64))
        loss = loss + (Dm * Dm).sum() / n
        resid.append(Dm)
        pres.append(pre)
        f0 += n_f[g]
    dz = torch.empty(M, G, D, dtype=f64)
    dHs = []
    for g in range(G):
        dH = (2.0 / n) * resid[g].reshape(M, -1) @ w2[g].to(f64)
        pre = pres[g]
        gelu_grad = 0.5 * (1.0 + torch.erf(pre / math.sqrt(2.0))) + pre * torch.exp(-0.5 * pre * pre) / math.sqrt(2.0 * math.pi)
        dz[:, g] = (dH * gelu_grad) @ w1[g].to(f64)
        dHs.append(dH)
    return loss, dz.view(B, P, G, D), dHs


def load_fixture(name):
    d = np.load(os.path.join(GOLDEN, name + ".npz"))
    meta = [int(v) for v in d["meta"]]
    n_inp, hidden, D, B, P = meta[:5]
    groups, cur = [], []
    for v in meta[5:]:
        if v < 0:
            groups.append(cur)
            cur = []
        else:
            cur.append(v)
    t = lambda k: torch.from_numpy(d[k])  # noqa: E731
    G = len(groups)
    return dict(groups=groups, n_inp=n_inp, hidden=hidden, D=D, B=B, P=P, w1=[t(f"w1.{g}") for g in range(G)], w2=[t(f"w2.{g}") for g in range(G)],
                b2=[t(f"b2.{g}") for g in range(G)], z=t("z"), target=t("target"), counts=t("counts"), loss=t("loss"), dz=t("dz"),
                loss_masked=t("loss_masked"), dz_masked=t("dz_masked"))


def rel(a, b):
    a, b = a.double().reshape(-1), b.double().reshape(-1)
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


@pytest.mark.parametrize("name", ["decode_mse_a", "decode_mse_b"])
@pytest.mark.parametrize("masked", [False, True])
def test_restatement_reproduces_the_reference(name, masked):
    fx = load_fixture(name)
    loss, dz, _ = restate(fx["w1"], fx["w2"], fx["b2"], fx["groups"], fx["z"], fx["target"], fx["counts"] if masked else None)
    ref_loss, ref_dz = (fx["loss_masked"], fx["dz_masked"]) if masked else (fx["loss"], fx["dz"])
    assert rel(loss, ref_loss) <= 1e-9
    assert rel(dz, ref_dz) <= 1e-9
    if masked:   # a patch without valid slots gets no gradient
        empty = [p for p, c in enumerate(fx["counts"].tolist()) if c == 0]
        assert empty and float(dz[:, empty].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ the entry point, without a GPU
@pytest.fixture(scope="module")
def lib():
    from sea_amd import build, _native

    build.build(verbose=False)
    return _native.lib()


def _table(n_groups=2):
    """A well-formed argument table over made-up (aligned, never dereferenced) addresses: every test below breaks exactly one thing, so the checks
    refuse it before anything could be launched."""
    from sea_amd import _native as N

    g = (N.SeaDecodeMseGroup * N.DECODE_MSE_MAX_GROUPS)()
    for i in range(n_groups):
        base = 0x10000 * (i + 1)
        g[i].H, g[i].W2, g[i].bias, g[i].dH, g[i].Z = base, base + 0x1000, base + 0x2000, base + 0x3000, base + 0x4000
        g[i].ldh = g[i].ldw = g[i].lddh = g[i].ldz = 40
        g[i].n_fields, g[i].field0 = 1 + i, i
    p = N.SeaDecodeMse()
    p.target, p.counts, p.loss, p.partial = 0x100000, 0x200000, 0x300000, 0x400000
    p.ld_row, p.ld_field = 48, 16
    p.M, p.S, p.C, p.Cp, p.P, p.n_partial_cap = 18, 40, 12, 32, 9, 2
    p.inv_n, p.grad_scale = 1.0 / (18 * 3 * 12), 1.0
    return g, p


def test_symbol_and_layout(lib):
    from sea_amd import _native as N

    assert hasattr(lib, "sea_decode_mse") and "sea_decode_mse" in N.EXPORTED_SYMBOLS
    assert C.sizeof(N.SeaDecodeMseGroup) == 64 and C.sizeof(N.SeaDecodeMse) == 80   # include/sea_hip.h states both
    assert lib.sea_abi_version() == 8
    # the library reads the fields where the binding writes them: its messages quote the values back
    g, p = _table()
    p.n_partial_cap = 1
    assert lib.sea_decode_mse(g, 2, C.byref(p), N.SEA_BF16, None) == -1
    assert b"partial workspace of 1 floats is too small: 2 needed" in lib.sea_last_error()
    g, p = _table()
    g[1].n_fields, g[1].field0 = 0, 7
    assert lib.sea_decode_mse(g, 2, C.byref(p), N.SEA_BF16, None) == -1
    assert b"group 1: n_fields=0, field0=7" in lib.sea_last_error()
    g, p = _table()
    p.ld_row, p.ld_field = 50, 16
    assert lib.sea_decode_mse(g, 2, C.byref(p), N.SEA_BF16, None) == -1
    assert b"ld_row=50, ld_field=16" in lib.sea_last_error()


def _break(what):
    g, p = _table()
    n = 2
    if what == "null group pointer":
        g[1].W2 = None
    elif what == "null target":
        p.target = None
    elif what == "null loss":
        p.loss = None
    elif what == "null partial":
        p.partial = None
    elif what == "M < 1":
        p.M = 0
    elif what == "S % 8":
        p.S = 36
    elif what == "field stride":
        p.ld_field = 14
    elif what == "row stride":
        p.ld_row = 46
    elif what == "C > Cp":
        p.C = 33
    elif what == "P < 1":
        p.P = 0
    elif what == "M % P":
        p.P = 4
    elif what == "too many groups":
        n = 17
    elif what == "no groups":
        n = 0
    elif what == "misaligned operand":
        g[0].H = 0x10008
    elif what == "short row stride":
        g[1].ldw = 32
    elif what == "misaligned target":
        p.target = 0x100004
    return g, n, p


@pytest.mark.parametrize("what", ["null group pointer", "null target", "null loss", "null partial", "M < 1", "S % 8", "field stride", "row stride", "C > Cp", "P < 1",
                                  "M % P", "too many groups", "no groups", "misaligned operand", "short row stride", "misaligned target"])
def test_bad_arguments_are_refused_without_a_device(lib, what):
    from sea_amd import _native as N

    g, n, p = _break(what)
    assert lib.sea_decode_mse(g, n, C.byref(p), N.SEA_BF16, None) == -1, what
    msg = lib.sea_last_error()
    assert b"sea_decode_mse" in msg
    if what in ("null group pointer", "short row stride"):
        assert b"group 1" in msg
    if what == "misaligned operand":
        assert b"group 0" in msg


def test_unsupported_forms_and_null_tables(lib):
    from sea_amd import _native as N

    g, p = _table()
    assert lib.sea_decode_mse(g, 2, C.byref(p), N.SEA_F32, None) == -3   # fp32: unsupported, not an argument error
    assert b"sea_decode_mse" in lib.sea_last_error() and b"bf16 only" in lib.sea_last_error()
    g, p = _table()
    p.S = 648
    for i in range(2):
        g[i].ldh = g[i].ldw = g[i].lddh = g[i].ldz = 648
    assert lib.sea_decode_mse(g, 2, C.byref(p), N.SEA_BF16, None) == -3 and b"S=648" in lib.sea_last_error()
    assert lib.sea_decode_mse(None, 1, C.byref(p), N.SEA_BF16, None) == -1
    assert lib.sea_decode_mse(g, 1, None, N.SEA_BF16, None) == -1
    assert lib.sea_decode_mse(g, 2, C.byref(p), 7, None) == -1
    # M % P matters only with counts
    g, p = _table()
    p.P, p.counts, p.M = 4, None, 0
    assert lib.sea_decode_mse(g, 2, C.byref(p), N.SEA_BF16, None) == -1 and b"M=0" in lib.sea_last_error()


# ------------------------------------------------------------------------------------------------ ops.decode_mse on the host
def _ops_args(M=18, S=40, C_=12, Cp=32, n_f=(2, 1), P=9, dtype=torch.bfloat16):
    groups = [dict(H=torch.zeros(M, S, dtype=dtype), W2=torch.zeros(n * Cp, S, dtype=dtype), bias=torch.zeros(n * Cp), dH=torch.zeros(M, S, dtype=dtype),
                   Z=torch.zeros(M, S, dtype=dtype)) for n in n_f]
    return dict(groups=groups, target=torch.zeros(M, sum(n_f), C_), C_=C_, Cp=Cp, inv_n=1.0 / (M * sum(n_f) * C_), counts=torch.zeros(P, dtype=torch.int32), n_patches=P)


def test_ops_decode_mse_refuses_cpu_tensors_and_malformed_arguments():
    from sea_amd import ops

    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.decode_mse(**_ops_args())

    def bad(match, **change):
        a = _ops_args()
        for k, v in change.items():
            if callable(v):
                v(a)
            else:
                a[k] = v
        with pytest.raises(ValueError, match=match):
            ops.decode_mse(**a)

    bad("bf16 only", dtype=torch.float32)
    bad("groups", groups=[])
    bad("groups", groups=_ops_args()["groups"] * 9)
    bad("Cp", Cp=48)
    bad("Cp", C_=33)
    bad("multiple of 8", f=lambda a: a["groups"][0].update(H=torch.zeros(18, 36, dtype=torch.bfloat16)))
    bad("multiple of 8", f=lambda a: [g.update({k: torch.zeros(g[k].shape[0], 648, dtype=torch.bfloat16) for k in ("H", "W2", "dH", "Z")}) for g in a["groups"]])
    bad("group 1: dH", f=lambda a: a["groups"][1].update(dH=torch.zeros(17, 40, dtype=torch.bfloat16)))
    bad("group 0: Z", f=lambda a: a["groups"][0].update(Z=torch.zeros(18, 40)))
    bad("unit inner stride", f=lambda a: a["groups"][0].update(H=torch.zeros(40, 18, dtype=torch.bfloat16).t()))
    bad("row stride", f=lambda a: a["groups"][1].update(H=torch.zeros(18, 44, dtype=torch.bfloat16)[:, :40]))
    bad("16-byte", f=lambda a: a["groups"][1].update(H=torch.zeros(18 * 40 + 4, dtype=torch.bfloat16)[4:].view(18, 40)))
    bad("not a multiple of Cp", f=lambda a: a["groups"][0].update(W2=torch.zeros(40, 40, dtype=torch.bfloat16)))
    bad("bias", f=lambda a: a["groups"][0].update(bias=torch.zeros(64, dtype=torch.float64)))
    bad("bias", f=lambda a: a["groups"][0].update(bias=torch.zeros(32)))
    bad("target must be float32", target=torch.zeros(18, 3, 12, dtype=torch.float64))
    bad("target must be float32", target=torch.zeros(18, 2, 12))
    bad("target must be float32", target=torch.zeros(18, 3, 8))
    bad("multiples of 4", target=torch.zeros(18, 3, 13)[..., :12])
    bad("multiples of 4", target=torch.zeros(18 * 36 + 1)[1:].view(18, 3, 12))
    bad("n_patches", n_patches=0, counts=None)
    bad("counts", counts=torch.zeros(9, dtype=torch.int64))
    bad("counts", counts=torch.zeros(8, dtype=torch.int32))
    bad("not a multiple of", n_patches=4, counts=torch.zeros(4, dtype=torch.int32))
    bad("inv_n", inv_n=0.0)


# ------------------------------------------------------------------------------------------------ Decode.mse_loss / FieldSpaceLoss on the host
def _decoder(frozen=True):
    from sea_amd.models.encoder_decoder import Decode

    dec = Decode([[0, 1], [2]], 12, 40, 16)
    return dec.requires_grad_(False) if frozen else dec


def test_mse_loss_refuses_cpu_tensors_and_malformed_arguments():
    dec = _decoder().set_compute_dtype("bf16")
    z, tgt = torch.zeros(2, 9, 2, 16), torch.zeros(2, 9, 3, 12)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        dec.mse_loss(z, tgt)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        dec.mse_loss(z, tgt, counts=[0, 1, 11, 12, 5, 12, 3, 7, 12], fused=False)
    for bad_z in (torch.zeros(2, 9, 2, 8), torch.zeros(2, 9, 3, 16), torch.zeros(18, 2, 16)):
        with pytest.raises(ValueError, match="z must be"):
            dec.mse_loss(bad_z, tgt)
    for bad_t in (torch.zeros(2, 9, 3, 11), torch.zeros(2, 9, 2, 12), torch.zeros(2, 8, 3, 12), torch.zeros(18, 3, 12)):
        with pytest.raises(ValueError, match="target must be"):
            dec.mse_loss(z, bad_t)
    with pytest.raises(ValueError, match="float32"):
        dec.mse_loss(z, tgt.double())
    with pytest.raises(ValueError, match="target must not require grad"):
        dec.mse_loss(z, tgt.clone().requires_grad_(True))
    with pytest.raises(ValueError, match="counts must be 9 integers"):
        dec.mse_loss(z, tgt, counts=[1, 2, 3])
    with pytest.raises(ValueError, match="counts must be 9 integers"):
        dec.mse_loss(z, tgt, counts=torch.ones(9))
    with pytest.raises(ValueError, match=r"counts must lie in \[0, n_inp = 12\]"):
        dec.mse_loss(z, tgt, counts=[0, 1, 13, 12, 5, 12, 3, 7, 12])
    with pytest.raises(ValueError, match="no valid element"):
        dec.mse_loss(z, tgt, counts=[0] * 9)
    with pytest.raises(ValueError, match="bf16 only"):
        _decoder().mse_loss(z, tgt, fused=True)   # fp32 compute dtype has no fused form


def test_trainable_decoder_is_refused():
    dec = _decoder(frozen=False)
    z, tgt = torch.zeros(2, 9, 2, 16, requires_grad=True), torch.zeros(2, 9, 3, 12)
    with pytest.raises(ValueError, match=r"requires_grad_\(False\).*SpatialModel"):
        dec.mse_loss(z, tgt)
    with torch.no_grad():   # nothing to drop without grad mode: the call proceeds to the device check
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            dec.mse_loss(z, tgt)


def test_field_space_loss_checks_its_arguments():
    from sea_amd.train.train_temporal import _loss_fn
    from sea_amd.utils.train_utils import FieldSpaceLoss, SeaMSELoss

    dec = _decoder()
    with pytest.raises(ValueError, match="layout"):
        FieldSpaceLoss(dec, 9, layout="PBFC")
    with pytest.raises(ValueError, match="n_patches"):
        FieldSpaceLoss(dec, 0)
    loss = FieldSpaceLoss(dec, 9)
    assert list(loss.parameters()) == []   # the decoder is an operand, not a sub-module
    with pytest.raises(ValueError, match="output must be"):
        loss(torch.zeros(1, 4, 2, 9 * 16 + 1), torch.zeros(1, 4, 9, 3, 12))
    with pytest.raises(ValueError, match="target fields must be"):
        loss(torch.zeros(1, 4, 2, 9 * 16), torch.zeros(1, 4, 8, 3, 12))
    with pytest.raises(ValueError, match="target must be"):   # the reference's layout given without naming it
        loss(torch.zeros(1, 4, 2, 9 * 16), torch.zeros(1, 4, 9, 12, 3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        loss(torch.zeros(1, 4, 2, 9 * 16), torch.zeros(1, 4, 9, 12, 3), layout="BPCF")
    assert isinstance(_loss_fn({}), SeaMSELoss)
    assert isinstance(_loss_fn({"loss_space": "field", "decoder": dec, "n_patches": 9}), FieldSpaceLoss)
    with pytest.raises(ValueError, match="loss_space"):
        _loss_fn({"loss_space": "pixels"})
    with pytest.raises(ValueError, match="decoder"):
        _loss_fn({"loss_space": "field"})
