"""The forecast of an ensemble (sea_decode_member_moments, Decode.member_moments, EnsembleFields, unpatch_spread) without a GPU: the contract of
include/sea_hip.h restated in fp64 and tied to the reference-generated goldens through `restate_member_sse`, the weight rules of EnsembleFields
restated in fp64, the entry point's symbol, struct layout and argument checks, and the refusals of the Python layers.

`restate_member_moments` and `restate_weights` are what tests/test_ensemble_moments_gpu.py compares with."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from tests.test_decode_loss_cpu import load_fixture, rel
from tests.test_ensemble_cpu import restate_member_sse


# ------------------------------------------------------------------------------------------------ the contracts, in fp64
def restate_member_moments(w1, w2, b2, groups, z, members, weights=None, counts=None, unbiased=False):
    """include/sea_hip.h, sea_decode_member_moments, with the first decoder layer in front of it, in fp64.
    w1[g] [S, D], w2[g] [n_g * C, S], b2[g] [n_g * C]; z [Bm, P, G, D]; weights: [Bm] normalised per history, or None (1 / members); a member with
    weight <= 0 (or NaN) is passed over; counts: P integers or None.  Returns (mean [B, P, F, C], var [B, P, F, C], Y [Bm, P, F, C]) in float64;
    invalid cells are 0 in mean and var."""
    f64 = torch.float64
    Bm, P, G, D = z.shape
    assert Bm % members == 0
    B = Bm // members
    n_f = [len(g) for g in groups]
    C_ = w2[0].shape[0] // n_f[0]
    ys = []
    for g in range(G):
        pre = z[:, :, g].detach().to(f64) @ w1[g].to(f64).t()
        H = 0.5 * pre * (1.0 + torch.erf(pre / math.sqrt(2.0)))
        ys.append((H @ w2[g].to(f64).t() + b2[g].to(f64)).view(Bm, P, n_f[g], C_))
    Y = torch.cat(ys, 2)
    w = torch.full((Bm,), 1.0 / members, dtype=f64) if weights is None else torch.as_tensor(weights).detach().to(f64).reshape(Bm)
    w = w.view(B, members, 1, 1, 1)
    live = w > 0
    zero = torch.zeros((), dtype=f64)
    y = Y.view(B, members, P, sum(n_f), C_)
    W = torch.where(live, w, zero).sum(1)
    mean = torch.where(W > 0, (w * torch.where(live, y, zero)).sum(1) / W.clamp_min(1e-300), zero)
    d = torch.where(live, y - mean.unsqueeze(1), zero)
    var = (w * d * d).sum(1)
    if unbiased:
        den = 1.0 - (torch.where(live, w, zero) ** 2).sum(1)
        var = var * torch.where(den > 0, 1.0 / den.clamp_min(1e-300), zero)
    if counts is not None:
        cnt = torch.as_tensor(counts).clamp(0, C_)
        valid = (torch.arange(C_) < cnt[:, None]).view(1, P, 1, C_)
        mean, var = torch.where(valid, mean, zero), torch.where(valid, var, zero)
    return mean, var, Y


def restate_weights(logw, members):
    """EnsembleFields' weights in numpy fp64: a NaN or infinite log-weight is a dead member (weight 0), the maximum over the live members is
    subtracted, a history without a live member gets equal weights.  logw [B * members] -> float64 [B * members]."""
    lw = np.asarray(logw, dtype=np.float32).astype(np.float64).reshape(-1, members)
    out = np.empty_like(lw)
    for b in range(lw.shape[0]):
        live = np.isfinite(lw[b])
        if not live.any():
            out[b] = 1.0 / members
            continue
        mx = lw[b][live].max()
        w = np.where(live, np.exp(np.where(live, lw[b], mx) - mx), 0.0)
        out[b] = w / w.sum()
    return out.reshape(-1)


@pytest.mark.parametrize("name", ["decode_mse_a", "decode_mse_b"])
def test_moments_restatement_decodes_what_the_reference_restatement_decodes(name):
    fx = load_fixture(name)
    args = (fx["w1"], fx["w2"], fx["b2"], fx["groups"], fx["z"])
    mean, var, Y = restate_member_moments(*args, 1)
    n_fields = sum(len(g) for g in fx["groups"])
    assert Y.shape == (fx["B"], fx["P"], n_fields, fx["n_inp"])
    # the decode of restate_member_sse (which reproduces the reference's loss): against a zero observation its score is sum Y^2; against Y itself it is 0
    sse0 = restate_member_sse(fx["w1"], fx["w2"], fx["b2"], fx["groups"], fx["z"], torch.zeros(fx["B"], fx["P"], n_fields, fx["n_inp"]), None, 1)
    assert rel((Y * Y).sum(dim=(1, 3)), sse0) <= 1e-12
    assert float(restate_member_sse(fx["w1"], fx["w2"], fx["b2"], fx["groups"], fx["z"], Y, None, 1).max()) == 0.0
    # one member per history: its own field, variance 0
    assert torch.equal(mean, Y) and float(var.abs().max()) == 0.0
    # uniform weights over the whole batch as one history
    Bm = fx["B"]
    mean, var, _ = restate_member_moments(*args, Bm)
    assert rel(mean[0], Y.mean(0)) <= 1e-13 and rel(var[0], Y.var(0, unbiased=False)) <= 1e-12
    _, var_u, _ = restate_member_moments(*args, Bm, unbiased=True)
    assert rel(var_u[0], Y.var(0, unbiased=True)) <= 1e-12
    # all the weight on one member: that member's field, variance exactly 0 — biased or not — whatever the dead members hold
    w = torch.zeros(Bm)
    w[Bm - 1] = 1.0
    zn = fx["z"].clone()
    zn[:Bm - 1] = float("nan")
    for unb in (False, True):
        mean, var, _ = restate_member_moments(fx["w1"], fx["w2"], fx["b2"], fx["groups"], zn, Bm, weights=w, unbiased=unb)
        assert torch.equal(mean[0], Y[Bm - 1]) and float(var.abs().max()) == 0.0
    # counts: invalid cells are 0 in both
    mean, var, _ = restate_member_moments(*args, Bm, counts=fx["counts"])
    for p, n in enumerate(fx["counts"].tolist()):
        assert float(mean[:, p, :, n:].abs().max() if n < fx["n_inp"] else 0.0) == 0.0 and float(var[:, p, :, n:].abs().max() if n < fx["n_inp"] else 0.0) == 0.0
        if n:
            assert torch.equal(mean[0, p, :, :n], restate_member_moments(*args, Bm)[0][0, p, :, :n])


def test_weight_restatement_and_the_tensor_ops_agree_on_the_rules():
    from sea_amd.ensemble import normalised_weights

    nan, inf = float("nan"), float("inf")
    g = torch.Generator().manual_seed(8)
    lw = 3 * torch.randn(5, 7, generator=g)
    lw[0, [1, 4]] = torch.tensor([nan, -inf])
    lw[1] = torch.tensor([nan, inf, -inf, nan, inf, -inf, nan])        # no live member
    lw[2, :6] = -inf                                                   # one live member
    lw[3] += 500.0                                                     # exp would overflow without the maximum
    lw[4, 0] = inf                                                     # +inf is dead too, as in the resampler
    ref = restate_weights(lw.reshape(-1), 7).reshape(5, 7)
    assert np.allclose(ref.sum(1), 1.0, atol=1e-12)
    assert ref[0, 1] == 0.0 and ref[0, 4] == 0.0 and np.all(ref[1] == 1.0 / 7) and ref[2].tolist() == [0.0] * 6 + [1.0] and ref[4, 0] == 0.0
    assert np.all(np.isfinite(ref))
    got = normalised_weights(lw.reshape(-1), 7)
    assert got.dtype == torch.float32 and got.shape == (35,)
    assert np.allclose(got.numpy().astype(np.float64), ref.reshape(-1), rtol=1e-6, atol=1e-9)
    assert np.array_equal(got.numpy() == 0.0, ref.reshape(-1) == 0.0)      # dead members: exactly 0, and nobody else
    assert got.view(5, 7)[2].tolist() == [0.0] * 6 + [1.0]
    # the normalised log-weights the resampler hands back (dead members -inf) give the same weights
    out = torch.log(torch.as_tensor(ref[0])).float()
    assert np.allclose(normalised_weights(out, 7).numpy(), ref[0], rtol=1e-5, atol=1e-8)
    assert torch.equal(normalised_weights(torch.zeros(6), 3), torch.full((6,), 1.0 / 3))


# ------------------------------------------------------------------------------------------------ the entry point, without a GPU
@pytest.fixture(scope="module")
def lib():
    from sea_amd import build, _native

    build.build(verbose=False)
    return _native.lib()


def _table(n_groups=2):
    """A well-formed sea_decode_member_moments table over made-up (aligned, never dereferenced) addresses: shape a with two members per history."""
    from sea_amd import _native as N

    g = (N.SeaDecodeMseGroup * N.DECODE_MSE_MAX_GROUPS)()
    for i in range(n_groups):
        base = 0x10000 * (i + 1)
        g[i].H, g[i].W2, g[i].bias, g[i].dH, g[i].Z = base, base + 0x1000, base + 0x2000, None, None
        g[i].ldh = g[i].ldw = 40
        g[i].n_fields, g[i].field0 = (2, 0) if i == 0 else (1, 2)
    p = N.SeaDecodeMemberMoments()
    p.w, p.var_scale, p.counts, p.mean, p.var, p.work = 0x100000, 0x110000, 0x200000, 0x300000, 0x400000, None
    p.work_cap = 0
    p.M, p.S, p.C, p.Cp, p.P, p.members, p.n_fields_total, p.ld = 36, 40, 12, 32, 9, 2, 3, 32
    return g, p


def _large(p, members=130):
    """The same table with an ensemble above 128 members: M = 9 * members rows of one history, two chunks, a workspace of exactly the needed size."""
    p.members, p.M = members, 9 * members
    p.work, p.work_cap = 0x500000, 2 * (2 * 9 * 3 * 32 + 9)
    return p


def test_symbol_and_struct_layout(lib):
    from sea_amd import _native as N

    assert hasattr(lib, "sea_decode_member_moments") and "sea_decode_member_moments" in N.EXPORTED_SYMBOLS
    assert C.sizeof(N.SeaDecodeMemberMoments) == 88                 # include/sea_hip.h states it
    assert N.SeaDecodeMemberMoments.ld.offset == 84 and N.SeaDecodeMemberMoments.work_cap.offset == 48 and N.SeaDecodeMemberMoments.M.offset == 56
    assert N.MEMBER_MOMENTS_CHUNK == 128 and lib.sea_abi_version() == 8
    # the library reads the fields where the binding writes them: its messages quote the values back
    g, p = _table()
    p.members = 5
    assert lib.sea_decode_member_moments(g, 2, C.byref(p), N.SEA_BF16, None) == -1
    assert b"M=36 is not a multiple of P * members = 9 * 5" in lib.sea_last_error()
    g, p = _table()
    p.ld = 10
    assert lib.sea_decode_member_moments(g, 2, C.byref(p), N.SEA_BF16, None) == -1
    assert b"ld=10 must cover C=12" in lib.sea_last_error()
    g, p = _table()
    _large(p).work_cap -= 1
    assert lib.sea_decode_member_moments(g, 2, C.byref(p), N.SEA_BF16, None) == -1
    assert b"workspace of 3473 floats is too small: 3474 needed" in lib.sea_last_error() and b"members=130" in lib.sea_last_error()
    g, p = _table()
    g[1].n_fields, g[1].field0 = 2, 2
    assert lib.sea_decode_member_moments(g, 2, C.byref(p), N.SEA_BF16, None) == -1
    assert b"group 1: n_fields=2, field0=2 outside the 3 fields" in lib.sea_last_error()


def _break(what):
    g, p = _table()
    n = 2
    if what == "null group pointer":
        g[1].W2 = None
    elif what == "null mean":
        p.mean = None
    elif what == "null var":
        p.var = None
    elif what == "members = 0":
        p.members = 0
    elif what == "M % (P members)":
        p.M = 27
    elif what == "M < 1":
        p.M = 0
    elif what == "S % 8":
        p.S = 36
    elif what == "C > Cp":
        p.C = 33
    elif what == "P < 1":
        p.P = 0
    elif what == "ld < C":
        p.ld = 8
    elif what == "ld % 4":
        p.ld = 14
    elif what == "misaligned operand":
        g[0].H = 0x10008
    elif what == "misaligned mean":
        p.mean = 0x300008
    elif what == "misaligned var":
        p.var = 0x400004
    elif what == "misaligned weights":
        p.w = 0x100002
    elif what == "misaligned var_scale":
        p.var_scale = 0x110001
    elif what == "misaligned counts":
        p.counts = 0x200002
    elif what == "short row stride":
        g[1].ldw = 32
    elif what == "row stride % 8":
        g[0].ldh = 44
    elif what == "overlapping fields":
        g[1].field0 = 1
    elif what == "uncovered field":
        p.n_fields_total = 4
    elif what == "no fields":
        p.n_fields_total = 0
    elif what == "too many groups":
        n = 17
    elif what == "no groups":
        n = 0
    elif what == "no workspace above 128 members":
        _large(p).work = None
    elif what == "small workspace above 128 members":
        _large(p, 257).work_cap = 3 * (2 * 9 * 3 * 32 + 9) - 1
    elif what == "misaligned workspace":
        _large(p).work = 0x500002
    return g, n, p


WHATS = ["null group pointer", "null mean", "null var", "members = 0", "M % (P members)", "M < 1", "S % 8", "C > Cp", "P < 1", "ld < C", "ld % 4",
         "misaligned operand", "misaligned mean", "misaligned var", "misaligned weights", "misaligned var_scale", "misaligned counts", "short row stride",
         "row stride % 8", "overlapping fields", "uncovered field", "no fields", "too many groups", "no groups", "no workspace above 128 members",
         "small workspace above 128 members", "misaligned workspace"]


@pytest.mark.parametrize("what", WHATS)
def test_member_moments_refuses_bad_arguments_without_a_device(lib, what):
    from sea_amd import _native as N

    g, n, p = _break(what)
    assert lib.sea_decode_member_moments(g, n, C.byref(p), N.SEA_BF16, None) == -1, what
    msg = lib.sea_last_error()
    assert b"sea_decode_member_moments" in msg
    if what in ("null group pointer", "short row stride", "overlapping fields"):
        assert b"group 1" in msg
    if what in ("misaligned operand", "row stride % 8"):
        assert b"group 0" in msg
    if "workspace" in what and "misaligned" not in what:
        assert b"workspace" in msg and b"too small" in msg


def test_member_moments_unsupported_forms_and_null_tables(lib):
    from sea_amd import _native as N

    g, p = _table()
    assert lib.sea_decode_member_moments(g, 2, C.byref(p), N.SEA_F32, None) == -3   # fp32: unsupported, not an argument error
    assert b"sea_decode_member_moments" in lib.sea_last_error() and b"bf16 only" in lib.sea_last_error()
    g, p = _table()
    p.S = 648
    for i in range(2):
        g[i].ldh = g[i].ldw = 648
    assert lib.sea_decode_member_moments(g, 2, C.byref(p), N.SEA_BF16, None) == -3 and b"S=648" in lib.sea_last_error()
    assert lib.sea_decode_member_moments(None, 1, C.byref(p), N.SEA_BF16, None) == -1
    assert lib.sea_decode_member_moments(g, 1, None, N.SEA_BF16, None) == -1
    assert lib.sea_decode_member_moments(g, 2, C.byref(p), 7, None) == -1
    g, p = _table()   # w, var_scale, counts and (up to 128 members) work may be NULL: a well-formed table fails only at the launch, which this test never reaches
    p.w = p.var_scale = p.counts = None
    p.M = 0
    assert lib.sea_decode_member_moments(g, 2, C.byref(p), N.SEA_BF16, None) == -1 and b"M=0" in lib.sea_last_error()


# ------------------------------------------------------------------------------------------------ ops on the host
def _ops_args(M=36, S=40, C_=12, Cp=32, n_f=(2, 1), P=9, members=2, dtype=torch.bfloat16):
    groups = [dict(H=torch.zeros(M, S, dtype=dtype), W2=torch.zeros(n * Cp, S, dtype=dtype), bias=torch.zeros(n * Cp)) for n in n_f]
    return dict(groups=groups, C_=C_, Cp=Cp, n_patches=P, members=members, weights=torch.full((M // P,), 0.5), var_scale=torch.ones(M // (P * members)),
                counts=torch.zeros(P, dtype=torch.int32))


def test_ops_refuse_cpu_tensors_and_malformed_arguments():
    from sea_amd import ops

    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.decode_member_moments(**_ops_args())

    def bad(match, **change):
        a = _ops_args()
        for k, v in change.items():
            if callable(v):
                v(a)
            else:
                a[k] = v
        with pytest.raises(ValueError, match=match):
            ops.decode_member_moments(**a)

    bad("bf16 only", dtype=torch.float32)
    bad("groups", groups=[])
    bad("Cp", Cp=48)
    bad("ld = 10", ld=10)
    bad("ld = 14", ld=14)
    bad("multiple of 8", f=lambda a: a["groups"][0].update(H=torch.zeros(36, 36, dtype=torch.bfloat16)))
    bad("must be positive", members=0)
    bad("must be positive", n_patches=0)
    bad("not a multiple of n_patches \\* members", members=8)
    bad("group 1: H", f=lambda a: a["groups"][1].update(H=torch.zeros(35, 40, dtype=torch.bfloat16)))
    bad("unit inner stride", f=lambda a: a["groups"][0].update(H=torch.zeros(40, 36, dtype=torch.bfloat16).t()))
    bad("not a multiple of Cp", f=lambda a: a["groups"][0].update(W2=torch.zeros(40, 40, dtype=torch.bfloat16)))
    bad("bias", f=lambda a: a["groups"][0].update(bias=torch.zeros(32)))
    bad("weights must be", weights=torch.zeros(2))                        # one per history instead of one per member
    bad("weights must be", weights=torch.zeros(4, dtype=torch.float64))
    bad("weights must be", weights=torch.zeros(2, 2))
    bad("weights must be", weights=[0.5] * 4)
    bad("var_scale must be", var_scale=torch.ones(4))
    bad("counts", counts=torch.zeros(9, dtype=torch.int64))


# ------------------------------------------------------------------------------------------------ the Python layers on the host
def _decoder():
    from sea_amd.models.encoder_decoder import Decode

    return Decode([[0, 1], [2]], 12, 40, 16).requires_grad_(False)


def test_member_moments_refuses_cpu_tensors_and_malformed_arguments():
    dec = _decoder().set_compute_dtype("bf16")
    z = torch.zeros(4, 9, 2, 16)
    for kw in (dict(), dict(fused=False), dict(weights=torch.full((4,), 0.5), unbiased=True), dict(counts=[0] * 9)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            dec.member_moments(z, 2, **kw)
    for bad_z in (torch.zeros(4, 9, 2, 8), torch.zeros(4, 9, 3, 16), torch.zeros(36, 2, 16)):
        with pytest.raises(ValueError, match="z must be"):
            dec.member_moments(bad_z, 2)
    for m in (0, 3, -1, 2.0, True):
        with pytest.raises(ValueError, match="members"):
            dec.member_moments(z, m)
    for bad_w in (torch.zeros(2), torch.zeros(2, 2), torch.zeros(5), [0.5] * 4):
        with pytest.raises(ValueError, match=r"weights must be None or a \[4\] tensor"):
            dec.member_moments(z, 2, weights=bad_w)
    with pytest.raises(ValueError, match="weights must be float32"):
        dec.member_moments(z, 2, weights=torch.zeros(4, dtype=torch.float64))
    with pytest.raises(ValueError, match="weights must be float32 on cpu"):      # the wrong device (a meta tensor stands for it here)
        dec.member_moments(z, 2, weights=torch.zeros(4, device="meta"))
    with pytest.raises(ValueError, match="Decode.member_moments: counts must be 9 integers"):
        dec.member_moments(z, 2, counts=[1, 2, 3])
    with pytest.raises(ValueError, match=r"counts must lie in \[0, n_inp = 12\]"):
        dec.member_moments(z, 2, counts=[0, 1, 13, 12, 5, 12, 3, 7, 12])
    with pytest.raises(ValueError, match="bf16 only"):
        _decoder().member_moments(z, 2, fused=True)


def test_ensemble_fields_checks_its_arguments():
    from sea_amd.ensemble import EnsembleFields as EF
    from sea_amd.utils import train_utils

    assert train_utils.EnsembleFields is EF
    dec = _decoder()
    with pytest.raises(ValueError, match="layout"):
        EF(dec, 9, 2, layout="PBFC")
    with pytest.raises(ValueError, match="n_patches"):
        EF(dec, 0, 2)
    for m in (0, -2, 2.0, True):
        with pytest.raises(ValueError, match="members"):
            EF(dec, 9, m)
    ef = EF(dec, 9, 2)
    y = torch.zeros(4, 2, 9 * 16)
    with pytest.raises(ValueError, match="y must be"):
        ef(torch.zeros(4, 2, 9 * 16 + 1))
    with pytest.raises(ValueError, match="y must be"):
        ef(torch.zeros(1, 4, 2, 9 * 16))
    with pytest.raises(ValueError, match="not a multiple of members"):
        ef(torch.zeros(5, 2, 9 * 16))
    with pytest.raises(ValueError, match="layout"):
        ef(y, layout="FC")
    for bad in (torch.zeros(3), torch.zeros(4, dtype=torch.int64), torch.zeros(4, 1), [0.0] * 4):
        with pytest.raises(ValueError, match="logw must be"):
            ef(y, logw=bad)
    with pytest.raises(ValueError, match="logw is on meta"):
        ef(y, logw=torch.zeros(4, device="meta"))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ef(y)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ef(y, logw=torch.zeros(2, 2), unbiased=True, layout="BPCF")


def test_unpatch_spread_refuses_cpu_tensors_and_needs_a_partition():
    from sea_amd.utils.data_processors import MeshProcessor, MeshUnpatcher

    assert callable(MeshUnpatcher.unpatch_spread)
    mp = MeshProcessor(dict(dimension="2D", field_groups=[[0, 1], [2]], m=3, n=4), torch.zeros(2, 5), device="cpu")
    with pytest.raises(ValueError, match="patchify_and_scale first"):
        mp.unpatch_spread(torch.zeros(1, 6, 3, 4))
