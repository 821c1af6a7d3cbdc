"""Ensemble weighting and resampling (sea_decode_member_sse, sea_resample_systematic, Decode.member_sse, sea_amd/ensemble.py) without a GPU: the two
contracts restated in fp64, the restatement of the first tied to the reference-generated goldens (tests/golden/decode_mse_*.npz), the properties of
the second, the condition under which the GPU test may compare resampling indices exactly, the entry points' argument checks and those of the
Python layers.

`restate_member_sse`, `restate_resample`, `resample_inputs` and `extra_resample_cases` are what tests/test_ensemble_gpu.py compares with."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from tests.test_decode_loss_cpu import load_fixture, rel

RESAMPLE_N = (1, 2, 63, 64, 65, 257, 4096)
MARGIN = 1e-9   # an fp64 scan of 4096 terms in any order errs by about 5e-13 (relative to W): thresholds this far from every c_i select the same member


# ------------------------------------------------------------------------------------------------ the contracts, in fp64
def restate_member_sse(w1, w2, b2, groups, z, target, counts, members):
    """include/sea_hip.h, sea_decode_member_sse, with the first decoder layer in front of it, in fp64.
    w1[g] [S, D], w2[g] [n_g * C, S], b2[g] [n_g * C]; z [Bm, P, G, D]; target [Bm / members, P, F, >= C]; counts: P integers or None.
    Returns sse [Bm, F] (float64)."""
    f64 = torch.float64
    Bm, P, G, D = z.shape
    n_f = [len(g) for g in groups]
    C_ = w2[0].shape[0] // n_f[0]
    assert Bm % members == 0 and target.shape[0] == Bm // members
    tgt = target.detach().to(f64)[..., :C_].repeat_interleave(members, dim=0)           # [Bm, P, F, C]: the members of a history share its observation
    if counts is None:
        valid = torch.ones(1, P, 1, C_, dtype=torch.bool)
    else:
        cnt = torch.as_tensor(counts).clamp(0, C_)
        valid = (torch.arange(C_) < cnt[:, None]).view(1, P, 1, C_)
    out, f0 = torch.empty(Bm, sum(n_f), dtype=f64), 0
    for g in range(G):
        pre = z[:, :, g].detach().to(f64) @ w1[g].to(f64).t()
        H = 0.5 * pre * (1.0 + torch.erf(pre / math.sqrt(2.0)))
        Y = (H @ w2[g].to(f64).t() + b2[g].to(f64)).view(Bm, P, n_f[g], C_)
        d = torch.where(valid, Y - tgt[:, :, f0:f0 + n_f[g]], torch.zeros((), dtype=f64))
        out[:, f0:f0 + n_f[g]] = (d * d).sum(dim=(1, 3))
        f0 += n_f[g]
    return out


def _weights_of(logw_row):
    lw = np.asarray(logw_row, dtype=np.float64)
    live = np.isfinite(lw)
    if not live.any():
        return live, None, None
    mx = lw[live].max()
    w = np.where(live, np.exp(np.where(live, lw, mx) - mx), 0.0)
    return live, mx, w


def restate_resample(logw, u, n, ess_frac):
    """include/sea_hip.h, sea_resample_systematic, in numpy fp64.  logw [G * n] or [G, n], u [G].  Returns (index int64 [G * n], logw_out float64 [G * n],
    ess float64 [G], resampled int64 [G])."""
    logw = np.asarray(logw, dtype=np.float32).reshape(-1, n)
    u = np.asarray(u, dtype=np.float32).astype(np.float64)
    G = logw.shape[0]
    index, out, ess, res = np.empty((G, n), np.int64), np.empty((G, n), np.float64), np.zeros(G), np.zeros(G, np.int64)
    for g in range(G):
        live, mx, w = _weights_of(logw[g])
        ident = g * n + np.arange(n)
        if mx is None:
            index[g], out[g], ess[g], res[g] = ident, 0.0, 0.0, -1
            continue
        c = np.cumsum(w)
        W = c[-1]
        ess[g] = W * W / np.sum(w * w)
        if ess_frac < 0 or ess[g] < float(ess_frac) * n:
            thr = (np.arange(n) + u[g]) / n * W
            pick = np.searchsorted(c, thr, side="right")                 # min{ i : c_i > thr }
            index[g] = g * n + np.minimum(pick, np.nonzero(live)[0].max())
            out[g], res[g] = 0.0, 1
        else:
            with np.errstate(invalid="ignore"):
                index[g], res[g] = ident, 0
                out[g] = np.where(live, logw[g].astype(np.float64) - mx - np.log(W), -np.inf)
    return index.reshape(-1), out.reshape(-1), ess, res


def margin(logw, u, n):
    """min over histories, i, j of |c_i - (j + u) / n * W| / W: how far every search threshold stays from every cumulative weight (histories without a
    live member have no search and are left out)."""
    logw = np.asarray(logw, dtype=np.float32).reshape(-1, n)
    u = np.asarray(u, dtype=np.float32).astype(np.float64)
    best = np.inf
    for g in range(logw.shape[0]):
        _, mx, w = _weights_of(logw[g])
        if mx is None:
            continue
        c = np.cumsum(w)
        thr = (np.arange(n) + u[g]) / n * c[-1]
        pos = np.clip(np.searchsorted(c, thr), 1, n - 1) if n > 1 else np.zeros(n, np.int64)
        near = np.minimum(np.abs(c[pos] - thr), np.abs(c[pos - 1] - thr)) if n > 1 else np.abs(c[0] - thr)
        best = min(best, float(near.min() / c[-1]))
    return best


def resample_inputs(n):
    """The issue's inputs for n members: three histories."""
    g = torch.Generator().manual_seed(1000 + n)
    logw = 3 * torch.randn(3, n, generator=g)
    u = torch.rand(3, generator=g)
    return logw, u


def extra_resample_cases():
    """name -> (logw [G, n], u [G], ess_threshold or None): the further launches of the GPU test.  Each passes the margin condition below."""
    g = torch.Generator().manual_seed(77)
    nan, inf = float("nan"), float("inf")
    cases = {}
    cases["one history"] = (3 * torch.randn(1, 17, generator=g), torch.rand(1, generator=g), None)
    one = torch.full((2, 33), -1e4)
    one[0, 5], one[1, 32] = 0.0, 2.0
    cases["all mass on one member"] = (one, torch.tensor([0.25, 0.75]), None)
    dead = 2 * torch.randn(3, 40, generator=g)
    dead[0, [0, 7, 39]] = torch.tensor([nan, inf, -inf])
    dead[1, 20:] = -inf
    dead[2, :39] = nan
    cases["dead members"] = (dead, torch.rand(3, generator=g), None)
    alld = 2 * torch.randn(3, 9, generator=g)
    alld[1] = torch.tensor([nan, inf, -inf] * 3)
    cases["an all-dead history"] = (alld, torch.rand(3, generator=g), None)
    mixed = torch.stack([0.1 * torch.randn(64, generator=g), 4 * torch.randn(64, generator=g)])
    cases["ess gate"] = (mixed, torch.rand(2, generator=g), 0.5)
    cases["uniform"] = (torch.zeros(2, 50), torch.tensor([0.5, 0.5]), None)
    return cases


# ------------------------------------------------------------------------------------------------ restatements
@pytest.mark.parametrize("name", ["decode_mse_a", "decode_mse_b"])
def test_member_sse_restatement_reproduces_the_reference(name):
    fx = load_fixture(name)
    n_fields = sum(len(g) for g in fx["groups"])
    for counts, ref in ((None, fx["loss"]), (fx["counts"], fx["loss_masked"])):
        sse = restate_member_sse(fx["w1"], fx["w2"], fx["b2"], fx["groups"], fx["z"], fx["target"], counts, 1)
        assert sse.shape == (fx["B"], n_fields)
        per = fx["P"] * fx["n_inp"] if counts is None else int(torch.as_tensor(counts).sum())
        assert rel(sse.sum() / (fx["B"] * n_fields * per), ref) <= 1e-9
    # members: the k members of a history read the same observation
    z2 = fx["z"].repeat_interleave(2, dim=0)
    twice = restate_member_sse(fx["w1"], fx["w2"], fx["b2"], fx["groups"], z2, fx["target"], fx["counts"], 2)
    assert torch.equal(twice[0::2], sse) and torch.equal(twice[1::2], sse)


@pytest.mark.parametrize("n", RESAMPLE_N)
def test_resample_restatement_properties_and_margin(n):
    logw, u = resample_inputs(n)
    assert margin(logw, u, n) >= MARGIN
    index, out, ess, res = restate_resample(logw, u, n, -1.0)
    assert res.tolist() == [1, 1, 1] and np.all(out == 0.0)
    for g in range(3):
        idx = index[g * n:(g + 1) * n] - g * n
        assert idx.min() >= 0 and idx.max() < n and np.all(np.diff(idx) >= 0)
        _, _, w = _weights_of(logw[g].numpy())
        npi = n * w / w.sum()
        copies = np.bincount(idx, minlength=n)
        assert np.all(copies >= np.floor(npi - 1e-9)) and np.all(copies <= np.ceil(npi + 1e-9))
        assert 1.0 - 1e-12 <= ess[g] <= n + 1e-9


def test_extra_resample_cases_keep_the_margin_and_the_rules():
    cases = extra_resample_cases()
    for name, (logw, u, thr) in cases.items():
        assert margin(logw, u, logw.shape[1]) >= MARGIN, name
    logw, u, _ = cases["dead members"]
    n = logw.shape[1]
    index, out, ess, res = restate_resample(logw, u, n, -1.0)
    picked = index.reshape(3, n) - np.arange(3)[:, None] * n
    assert not np.isin(picked[0], [0, 7, 39]).any() and picked[1].max() < 20 and np.all(picked[2] == 39)
    assert abs(ess[2] - 1.0) <= 1e-12
    logw, u, _ = cases["an all-dead history"]
    n = logw.shape[1]
    index, out, ess, res = restate_resample(logw, u, n, -1.0)
    assert res.tolist() == [1, -1, 1] and ess[1] == 0.0 and np.all(out == 0.0)
    assert index[n:2 * n].tolist() == list(range(n, 2 * n))
    logw, u, thr = cases["ess gate"]
    n = logw.shape[1]
    index, out, ess, res = restate_resample(logw, u, n, thr)
    assert res.tolist() == [0, 1] and ess[0] > 0.9 * n and ess[1] < 0.25 * n
    assert index[:n].tolist() == list(range(n)) and abs(np.exp(out[:n]).sum() - 1.0) <= 1e-12 and np.all(out[n:] == 0.0)
    logw, u, _ = cases["uniform"]
    index, _, ess, _ = restate_resample(logw, u, 50, -1.0)
    assert index.tolist() == list(range(100)) and np.allclose(ess, 50.0)
    logw, u, _ = cases["all mass on one member"]
    index, _, ess, _ = restate_resample(logw, u, 33, -1.0)
    assert np.all(index[:33] == 5) and np.all(index[33:] == 33 + 32) and np.allclose(ess, 1.0)
    # a dead member keeps -inf where the history is not resampled
    lw = torch.tensor([[0.0, float("nan"), 0.0, 0.0]])
    index, out, ess, res = restate_resample(lw, torch.tensor([0.5]), 4, 0.5)
    assert res.tolist() == [0] and out[1] == -np.inf and np.allclose(out[[0, 2, 3]], -math.log(3.0)) and abs(ess[0] - 3.0) <= 1e-12


# ------------------------------------------------------------------------------------------------ the entry points, without a GPU
@pytest.fixture(scope="module")
def lib():
    from sea_amd import build, _native

    build.build(verbose=False)
    return _native.lib()


def _table(n_groups=2):
    """A well-formed sea_decode_member_sse table over made-up (aligned, never dereferenced) addresses: shape a with two members per history."""
    from sea_amd import _native as N

    g = (N.SeaDecodeMseGroup * N.DECODE_MSE_MAX_GROUPS)()
    for i in range(n_groups):
        base = 0x10000 * (i + 1)
        g[i].H, g[i].W2, g[i].bias, g[i].dH, g[i].Z = base, base + 0x1000, base + 0x2000, None, None
        g[i].ldh = g[i].ldw = 40
        g[i].n_fields, g[i].field0 = (2, 0) if i == 0 else (1, 2)
    p = N.SeaDecodeMemberSse()
    p.target, p.counts, p.sse, p.work = 0x100000, 0x200000, 0x300000, 0x400000
    p.ld_row, p.ld_field, p.work_cap = 48, 16, 36 * 3
    p.M, p.S, p.C, p.Cp, p.P, p.members, p.n_fields_total = 36, 40, 12, 32, 9, 2, 3
    return g, p


def test_symbols_and_struct_layout(lib):
    from sea_amd import _native as N

    for name in ("sea_decode_member_sse", "sea_resample_systematic"):
        assert hasattr(lib, name) and name in N.EXPORTED_SYMBOLS
    assert C.sizeof(N.SeaDecodeMemberSse) == 88                     # include/sea_hip.h states it
    assert N.SeaDecodeMemberSse not in N.ABI_STRUCTS and len(N.ABI_STRUCTS) == 33 and N.ABI_STRUCTS[-1] is N.SeaKvFork
    assert lib.sea_abi_version() == 8
    # the library reads the fields where the binding writes them: its messages quote the values back
    g, p = _table()
    p.work_cap = 107
    assert lib.sea_decode_member_sse(g, 2, C.byref(p), N.SEA_BF16, None) == -1
    assert b"workspace of 107 floats is too small: 108 needed" in lib.sea_last_error()
    g, p = _table()
    p.members = 5
    assert lib.sea_decode_member_sse(g, 2, C.byref(p), N.SEA_BF16, None) == -1
    assert b"M=36 is not a multiple of P * members = 9 * 5" in lib.sea_last_error()
    g, p = _table()
    g[1].n_fields, g[1].field0 = 2, 2
    assert lib.sea_decode_member_sse(g, 2, C.byref(p), N.SEA_BF16, None) == -1
    assert b"group 1: n_fields=2, field0=2 outside the 3 fields" in lib.sea_last_error()
    g, p = _table()
    p.ld_row, p.ld_field = 50, 16
    assert lib.sea_decode_member_sse(g, 2, C.byref(p), N.SEA_BF16, None) == -1
    assert b"ld_row=50, ld_field=16" in lib.sea_last_error()


def _break(what):
    g, p = _table()
    n = 2
    if what == "null group pointer":
        g[1].W2 = None
    elif what == "null target":
        p.target = None
    elif what == "null sse":
        p.sse = None
    elif what == "null work":
        p.work = None
    elif what == "members = 0":
        p.members = 0
    elif what == "M % (P members)":
        p.M, p.work_cap = 27, 27 * 3
    elif what == "small workspace":
        p.work_cap = 36 * 3 - 1
    elif what == "M < 1":
        p.M = 0
    elif what == "S % 8":
        p.S = 36
    elif what == "C > Cp":
        p.C = 33
    elif what == "P < 1":
        p.P = 0
    elif what == "field stride":
        p.ld_field = 14
    elif what == "misaligned operand":
        g[0].H = 0x10008
    elif what == "short row stride":
        g[1].ldw = 32
    elif what == "overlapping fields":
        g[1].field0 = 1
    elif what == "uncovered field":
        p.n_fields_total, p.work_cap = 4, 36 * 4
    elif what == "too many groups":
        n = 17
    elif what == "no groups":
        n = 0
    return g, n, p


@pytest.mark.parametrize("what", ["null group pointer", "null target", "null sse", "null work", "members = 0", "M % (P members)", "small workspace", "M < 1", "S % 8",
                                  "C > Cp", "P < 1", "field stride", "misaligned operand", "short row stride", "overlapping fields", "uncovered field",
                                  "too many groups", "no groups"])
def test_member_sse_refuses_bad_arguments_without_a_device(lib, what):
    from sea_amd import _native as N

    g, n, p = _break(what)
    assert lib.sea_decode_member_sse(g, n, C.byref(p), N.SEA_BF16, None) == -1, what
    msg = lib.sea_last_error()
    assert b"sea_decode_member_sse" in msg
    if what in ("null group pointer", "short row stride", "overlapping fields"):
        assert b"group 1" in msg
    if what == "misaligned operand":
        assert b"group 0" in msg


def test_member_sse_unsupported_forms_and_null_tables(lib):
    from sea_amd import _native as N

    g, p = _table()
    assert lib.sea_decode_member_sse(g, 2, C.byref(p), N.SEA_F32, None) == -3   # fp32: unsupported, not an argument error
    assert b"sea_decode_member_sse" in lib.sea_last_error() and b"bf16 only" in lib.sea_last_error()
    g, p = _table()
    p.S = 648
    for i in range(2):
        g[i].ldh = g[i].ldw = 648
    assert lib.sea_decode_member_sse(g, 2, C.byref(p), N.SEA_BF16, None) == -3 and b"S=648" in lib.sea_last_error()
    assert lib.sea_decode_member_sse(None, 1, C.byref(p), N.SEA_BF16, None) == -1
    assert lib.sea_decode_member_sse(g, 1, None, N.SEA_BF16, None) == -1
    assert lib.sea_decode_member_sse(g, 2, C.byref(p), 7, None) == -1
    g, p = _table()   # dH and Z are not read: NULL above; counts may be NULL too — a well-formed table fails only at the launch, which this test never reaches
    p.counts = None
    p.M = 0
    assert lib.sea_decode_member_sse(g, 2, C.byref(p), N.SEA_BF16, None) == -1 and b"M=0" in lib.sea_last_error()


def test_resample_refuses_bad_arguments_without_a_device(lib):
    a = [0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000]   # logw, u, index, logw_out, ess, resampled: aligned, never dereferenced

    def call(ptrs=a, frac=-1.0, G=3, n=64):
        logw, u, index, out, ess, res = ptrs
        return lib.sea_resample_systematic(logw, u, frac, G, n, index, out, ess, res, None)

    for i in range(6):
        ptrs = list(a)
        ptrs[i] = None
        assert call(ptrs) == -1 and b"sea_resample_systematic: null pointer" in lib.sea_last_error()
    assert call(n=0) == -1 and b"sea_resample_systematic: n=0" in lib.sea_last_error()
    assert call(G=0) == -1 and b"sea_resample_systematic: G=0" in lib.sea_last_error()
    assert call(n=-5) == -1 and call(G=-1) == -1
    assert call(frac=float("nan")) == -1 and b"NaN" in lib.sea_last_error()
    assert call(ptrs=[0x1002] + a[1:]) == -1 and b"misaligned" in lib.sea_last_error()
    assert call(n=4097) == -3 and b"n=4097" in lib.sea_last_error() and b"unsupported" in lib.sea_last_error()
    assert call(G=1 << 20, n=4096) == -1 and b"int32" in lib.sea_last_error()


# ------------------------------------------------------------------------------------------------ ops on the host
def _ops_args(M=36, S=40, C_=12, Cp=32, n_f=(2, 1), P=9, members=2, dtype=torch.bfloat16):
    groups = [dict(H=torch.zeros(M, S, dtype=dtype), W2=torch.zeros(n * Cp, S, dtype=dtype), bias=torch.zeros(n * Cp)) for n in n_f]
    return dict(groups=groups, target=torch.zeros(M // members, sum(n_f), C_), C_=C_, Cp=Cp, n_patches=P, members=members, counts=torch.zeros(P, dtype=torch.int32))


def test_ops_refuse_cpu_tensors_and_malformed_arguments():
    from sea_amd import ops

    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.decode_member_sse(**_ops_args())

    def bad(match, **change):
        a = _ops_args()
        for k, v in change.items():
            if callable(v):
                v(a)
            else:
                a[k] = v
        with pytest.raises(ValueError, match=match):
            ops.decode_member_sse(**a)

    bad("bf16 only", dtype=torch.float32)
    bad("groups", groups=[])
    bad("Cp", Cp=48)
    bad("multiple of 8", f=lambda a: a["groups"][0].update(H=torch.zeros(36, 36, dtype=torch.bfloat16)))
    bad("must be positive", members=0)
    bad("must be positive", n_patches=0)
    bad("not a multiple of n_patches \\* members", members=8)
    bad("group 1: H", f=lambda a: a["groups"][1].update(H=torch.zeros(35, 40, dtype=torch.bfloat16)))
    bad("unit inner stride", f=lambda a: a["groups"][0].update(H=torch.zeros(40, 36, dtype=torch.bfloat16).t()))
    bad("not a multiple of Cp", f=lambda a: a["groups"][0].update(W2=torch.zeros(40, 40, dtype=torch.bfloat16)))
    bad("bias", f=lambda a: a["groups"][0].update(bias=torch.zeros(32)))
    bad("target must be float32", target=torch.zeros(36, 3, 12))          # one row per member: members = 2 wants 18
    bad("target must be float32", target=torch.zeros(18, 3, 12, dtype=torch.float64))
    bad("multiples of 4", target=torch.zeros(18, 3, 13)[..., :12])
    bad("counts", counts=torch.zeros(9, dtype=torch.int64))

    lw, u = torch.zeros(12), torch.zeros(3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.resample_systematic(lw, u, 4)
    for kw, match in ((dict(logw=lw, u=u, members=0), "members"), (dict(logw=lw, u=u, members=4097), "members"), (dict(logw=lw, u=u, members=5), "logw must be"),
                      (dict(logw=lw.double(), u=u, members=4), "logw must be"), (dict(logw=lw, u=torch.zeros(4), members=4), "u must be"),
                      (dict(logw=lw, u=u, members=4, ess_frac=float("nan")), "NaN")):
        with pytest.raises(ValueError, match=match):
            ops.resample_systematic(**kw)


# ------------------------------------------------------------------------------------------------ the Python layers on the host
def _decoder():
    from sea_amd.models.encoder_decoder import Decode

    return Decode([[0, 1], [2]], 12, 40, 16).requires_grad_(False)


def test_member_sse_refuses_cpu_tensors_and_malformed_arguments():
    dec = _decoder().set_compute_dtype("bf16")
    z, tgt = torch.zeros(4, 9, 2, 16), torch.zeros(2, 9, 3, 12)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        dec.member_sse(z, tgt, members=2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        dec.member_sse(z, tgt, members=2, counts=[0] * 9, fused=False)    # counts without a valid element are accepted: every score is 0
    for bad_z in (torch.zeros(4, 9, 2, 8), torch.zeros(4, 9, 3, 16), torch.zeros(36, 2, 16)):
        with pytest.raises(ValueError, match="z must be"):
            dec.member_sse(bad_z, tgt, members=2)
    for m in (0, 3, -1, 2.0, True):
        with pytest.raises(ValueError, match="members"):
            dec.member_sse(z, tgt, members=m)
    for bad_t in (torch.zeros(4, 9, 3, 12), torch.zeros(2, 9, 3, 11), torch.zeros(2, 9, 2, 12), torch.zeros(2, 8, 3, 12), torch.zeros(18, 3, 12)):
        with pytest.raises(ValueError, match="target must be"):
            dec.member_sse(z, bad_t, members=2)
    with pytest.raises(ValueError, match="float32"):
        dec.member_sse(z, tgt.double(), members=2)
    with pytest.raises(ValueError, match="Decode.member_sse: counts must be 9 integers"):      # the message names the function that was called
        dec.member_sse(z, tgt, members=2, counts=[1, 2, 3])
    with pytest.raises(ValueError, match=r"counts must lie in \[0, n_inp = 12\]"):
        dec.member_sse(z, tgt, members=2, counts=[0, 1, 13, 12, 5, 12, 3, 7, 12])
    with pytest.raises(ValueError, match="bf16 only"):
        _decoder().member_sse(z, tgt, members=2, fused=True)
    # the counts cache does not let mse_loss accept what member_sse accepted
    empty = [0] * 9
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        dec.member_sse(z, tgt, members=2, counts=empty)
    with pytest.raises(ValueError, match="no valid element"):
        dec.mse_loss(torch.zeros(2, 9, 2, 16), tgt, counts=empty)


def test_field_likelihood_and_systematic_resample_check_their_arguments():
    from sea_amd.ensemble import FieldLikelihood as FL, systematic_resample as sr
    from sea_amd.utils import train_utils

    assert train_utils.FieldLikelihood is FL and train_utils.systematic_resample is sr
    dec = _decoder()
    with pytest.raises(ValueError, match="layout"):
        FL(dec, 9, 2, layout="PBFC")
    with pytest.raises(ValueError, match="n_patches"):
        FL(dec, 0, 2)
    with pytest.raises(ValueError, match="members"):
        FL(dec, 9, 0)
    for sigma in (0.0, -1.0, float("nan"), float("inf"), [1.0, 2.0], [1.0, 0.0, 1.0], torch.ones(2, 3)):
        with pytest.raises(ValueError, match="sigma"):
            FL(dec, 9, 2, sigma=sigma)
    like = FL(dec, 9, 2, sigma=[0.5, 1.0, 2.0])
    assert like._scale_host == [-2.0, -0.5, -0.125] and FL(dec, 9, 2, sigma=2)._scale_host == [-0.125] * 3
    with pytest.raises(ValueError, match="y must be"):
        like(torch.zeros(4, 2, 9 * 16 + 1), torch.zeros(2, 9, 3, 12))
    with pytest.raises(ValueError, match="y must be"):
        like(torch.zeros(1, 4, 2, 9 * 16), torch.zeros(2, 9, 3, 12))
    with pytest.raises(ValueError, match="not a multiple of members"):
        like(torch.zeros(5, 2, 9 * 16), torch.zeros(2, 9, 3, 12))
    with pytest.raises(ValueError, match="observation must be"):
        like(torch.zeros(4, 2, 9 * 16), torch.zeros(4, 9, 3, 12))
    with pytest.raises(ValueError, match="target must be"):              # the reference's layout given without naming it
        like(torch.zeros(4, 2, 9 * 16), torch.zeros(2, 9, 12, 3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        like(torch.zeros(4, 2, 9 * 16), torch.zeros(2, 9, 12, 3), layout="BPCF")

    lw = torch.zeros(12)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        sr(lw, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        sr(lw.view(3, 4), 4, u=torch.zeros(3), ess_threshold=0.5, prior=torch.zeros(12))
    for kw, match in ((dict(members=0), "members"), (dict(members=4097), "members"), (dict(members=5), "logw must be"), (dict(members=4, u=torch.zeros(4)), "u must be"),
                      (dict(members=4, u=torch.zeros(3, dtype=torch.float64)), "u must be"), (dict(members=4, ess_threshold=1.5), "ess_threshold"),
                      (dict(members=4, ess_threshold=-0.1), "ess_threshold"), (dict(members=4, prior=torch.zeros(11)), "prior")):
        with pytest.raises(ValueError, match=match):
            sr(lw, **kw)
    with pytest.raises(ValueError, match="logw must be"):
        sr(torch.zeros(12, dtype=torch.int64), 4)
    with pytest.raises(ValueError, match="logw must be"):
        sr(lw.view(4, 3), 4)
