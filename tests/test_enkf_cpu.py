"""The ensemble Kalman analysis (sea_enkf_transform, sea_ensemble_mix, SensorKalman, gaspari_cohn, MeshUnpatcher.sensor_taper) without a GPU: the
formulas of include/sea_hip.h restated in fp64 (`restate_enkf`, `restate_mix`) and held against the state-space Kalman formulas for a linear
observation operator, the neutrality of a reading without weight, the conditioning of every input the GPU test uses (cond(I + C) <= 1e4, met by
scaling the precisions), the error that bf16-rounded decoder operands alone put into the increment (the envelope of the GPU test), the entry points'
argument checks through the built library, and the localisation helpers.

Every input of tests/test_enkf_gpu.py is generated here (`transform_case`, `mix_case`, `kalman_case`), once, and never modified."""
import ctypes as C
import functools
import math

import pytest
import torch

from tests.test_decode_loss_cpu import rel
from tests.test_sensor_cpu import SPLITS, host_case, make_decoder, restate_sensor, sensor_obs, sensor_precision, sensor_sets

F64 = torch.float64
COND_MAX = 1e4


# ------------------------------------------------------------------------------------------------ the contract, in fp64
def restate_enkf(pred, obs, prec, taper, members, rho, alpha):
    """include/sea_hip.h, sea_enkf_transform, in fp64, problem by problem, with torch.linalg.inv (no Cholesky: another route to W).  pred [B * N, K],
    obs [B, K], prec None / [K] / [B, K], taper None / [Ld, K].  Returns (D [B, Ld, N, N] float64, status [B, Ld] int64, cond [B, Ld] of I + C)."""
    n = members
    B, K = obs.shape
    Ld = 1 if taper is None else taper.shape[0]
    D = torch.zeros(B, Ld, n, n, dtype=F64)
    status = torch.zeros(B, Ld, dtype=torch.int64)
    cond = torch.ones(B, Ld, dtype=F64)
    eye = torch.eye(n, dtype=F64)
    Pi = eye - 1.0 / n
    for b in range(B):
        p = pred[b * n:(b + 1) * n].to(F64)                          # [N, K]
        w = torch.ones(K, dtype=F64) if prec is None else (prec if prec.dim() == 1 else prec[b]).to(F64)
        w = torch.where(w > 0, w, torch.zeros((), dtype=F64))
        for d in range(Ld):
            wd = w if taper is None else w * torch.where(taper[d] > 0, taper[d].to(F64), torch.zeros((), dtype=F64))
            live = wd > 0
            status[b, d] = int(live.sum())
            pl, ol, wl = p[:, live], obs[b].to(F64)[live], wd[live]  # a reading without weight never enters
            if not (bool(torch.isfinite(pl).all()) and bool(torch.isfinite(ol).all()) and bool(torch.isfinite(wl).all())):
                status[b, d] = -1
                continue
            ybar = pl.mean(0)
            S = rho * (pl - ybar) * (wl / (n - 1)).sqrt()
            dl = wl.sqrt() * (ol - ybar)
            M = eye + S @ S.t()
            cond[b, d] = torch.linalg.cond(M)
            W = torch.linalg.inv(M)
            G = (W @ (S @ dl)).unsqueeze(1).expand(n, n) / math.sqrt(n - 1) - alpha * (eye - W)
            D[b, d] = (rho - 1.0) * Pi + rho * (G - G.mean(0, keepdim=True))
    return D, status, cond


def restate_mix(y, D, n_patches):
    """sea_ensemble_mix's increment in fp64: inc[b N + j, g, p, :] = sum_i D[b, dom(p), i, j] y[b N + i, g, p, :]; y [Bm, G, P * Dl], D [B, Ld, N, N]."""
    B, Ld, n, _ = D.shape
    Bm, G, E = y.shape
    yy = y.to(F64).view(B, n, G, n_patches, E // n_patches)
    Dd = D.to(F64).expand(B, n_patches, n, n) if Ld == 1 else D.to(F64)
    return torch.einsum("bpij,bigpe->bjgpe", Dd, yy).reshape(Bm, G, E)


# ------------------------------------------------------------------------------------------------ the inputs of the GPU test
T_N, T_K, T_B, T_LD = (2, 3, 5, 33, 64, 128), (1, 7, 33, 257), (1, 3), (1, 4)


@functools.lru_cache(maxsize=None)
def transform_case(n, K, B, Ld, with_prec):
    """Random normal predictions and readings (float32); with_prec: precisions in [0.25, 2], a tenth of the readings missing (precision 0, the reading
    NaN); Ld = 4: a taper in [0, 1] with a third of its entries 0 and domain 1 all zero.  Returns dict(pred, obs, prec, taper, rho, alpha)."""
    g = torch.Generator().manual_seed(100000 + 1000 * n + 10 * K + 3 * B + Ld + (500 if with_prec else 0))
    pred, obs = torch.randn(B * n, K, generator=g), torch.randn(B, K, generator=g)
    prec = None
    if with_prec:
        prec = 0.25 + 1.75 * torch.rand(B, K, generator=g)
        miss = torch.rand(B, K, generator=g) < 0.1
        prec[miss] = 0.0
        obs[miss] = float("nan")
    taper = None
    if Ld > 1:
        taper = torch.rand(Ld, K, generator=g)
        taper[torch.rand(Ld, K, generator=g) < 1.0 / 3.0] = 0.0
        taper[1] = 0.0
    return dict(pred=pred, obs=obs, prec=prec, taper=taper, rho=1.1 if (n + K) % 2 else 1.0, alpha=0.5 if K % 2 else 0.8)


def transform_cases(n):
    return [(K, B, Ld, wp) for K in T_K for B in T_B for Ld in T_LD for wp in (False, True)]


# (name, members, histories, n_groups, n_patches, Dl, Ld, dtype): shape a of tests/test_decode_loss_gpu.py (two groups, nine patches) with two members,
# 33 members of one history, 5 members of 7 histories, 128 members; one domain and P domains; a column count that is no multiple of 64
MIX_CASES = (("a2", 2, 1, 2, 9, 16, 1), ("a2_local", 2, 1, 2, 9, 16, 9), ("n33", 33, 1, 3, 4, 48, 1), ("n5_local", 5, 7, 1, 3, 50, 3),
             ("n128", 128, 1, 2, 2, 24, 1), ("n128_local", 128, 1, 2, 2, 24, 2))


@functools.lru_cache(maxsize=None)
def mix_case(name):
    """(y float32 [Bm, G, P * Dl], D float32 [B, Ld, N, N], n_patches): random normal states, D with entries of size 1 / sqrt(N)."""
    _, n, B, G, P, Dl, Ld = next(c for c in MIX_CASES if c[0] == name)
    g = torch.Generator().manual_seed(4000 + n + 7 * B + Ld)
    if name.startswith("a2"):
        Dl = host_case("a")["D"]
    return torch.randn(B * n, G, P * Dl, generator=g), torch.randn(B, Ld, n, n, generator=g) / math.sqrt(n), P


E2E_SETS = {"a": ("segments", "last"), "b": ("segments", "last"), "c": ("s31_32", "s33_70")}   # "last" of a and "segments" of b leave a group unobserved
E2E_PRECISION_SCALE = {"a": 1.0, "b": 1.0, "c": 1.0}   # multiplies tests/test_sensor_cpu.py's precisions so that cond(I + C) <= 1e4 on every input below


def kalman_cases():
    return [(name, s, m, h, local) for name in ("a", "b", "c") for s in E2E_SETS[name] for m, h in SPLITS[name] if m >= 2 for local in (False, True)]


@functools.lru_cache(maxsize=None)
def kalman_case(name, set_name, members, hist, local, dtype="bf16"):
    """An end-to-end input: the shape's states as y [Bm, G, P * D] in the act dtype (bf16: rounded once, here — the state as the session hands it over),
    the set's readings, the scaled precisions, a taper [P, K] (local) or None, and the fp64 restatement of the whole chain from the exact decoder:
    dict(y, z, patch, cell, field, obs, prec, taper, rho, alpha, pred, D, status, cond, inc)."""
    c = host_case(name)
    patch, cell, field = sensor_sets(name)[set_name]
    Bm, P, G, D_ = c["z"].shape
    y = c["z"].permute(0, 2, 1, 3).reshape(Bm, G, P * D_).contiguous()
    y = y.to(torch.bfloat16) if dtype == "bf16" else y.clone()
    z = y.to(F64).view(Bm, G, P, D_).permute(0, 2, 1, 3)
    obs = sensor_obs(name, set_name, hist)
    prec = sensor_precision(name, set_name, hist) * E2E_PRECISION_SCALE[name]
    taper = None
    if local:
        g = torch.Generator().manual_seed(77 + len(patch) + members)
        taper = torch.rand(P, len(patch), generator=g)
        taper[torch.rand(P, len(patch), generator=g) < 0.3] = 0.0
    rho, alpha = (1.05, 0.5) if members % 2 else (1.0, 0.5)
    _, pred = restate_sensor(c["w1"], c["w2"], c["b2"], c["groups"], z, patch, cell, field, obs, prec, members)
    D, status, cond = restate_enkf(pred, obs, prec, taper, members, rho, alpha)
    return dict(y=y, z=z, patch=patch, cell=cell, field=field, obs=obs, prec=prec, taper=taper, rho=rho, alpha=alpha, pred=pred, D=D, status=status,
                cond=cond, inc=restate_mix(y, D, P))


@functools.lru_cache(maxsize=None)
def bf16_envelope():
    """The largest relative L2 error of the increment, over the end-to-end inputs, that decoder operands rounded to bf16 cause on their own (the
    predictions of restate_sensor(round_bf16=True) against the exact ones, both pushed through restate_enkf and restate_mix)."""
    worst = 0.0
    for name, set_name, members, hist, local in kalman_cases():
        k = kalman_case(name, set_name, members, hist, local)
        c = host_case(name)
        _, pred_r = restate_sensor(c["w1"], c["w2"], c["b2"], c["groups"], k["z"], k["patch"], k["cell"], k["field"], k["obs"], k["prec"], members, round_bf16=True)
        D_r, _, _ = restate_enkf(pred_r, k["obs"], k["prec"], k["taper"], members, k["rho"], k["alpha"])
        e = rel(restate_mix(k["y"], D_r, c["P"]), k["inc"])
        print(f"enkf shape {name} set {set_name} members {members} x {hist} local {local}: bf16 operands e(inc) {e:.3e} e(pred) {rel(pred_r, k['pred']):.3e} "
              f"cond {float(k['cond'].max()):.3e}")
        worst = max(worst, e)
    print(f"enkf bf16 envelope: {worst:.3e}")
    return worst


# ------------------------------------------------------------------------------------------------ the restatement against the state-space formulas
@pytest.mark.parametrize("n", [2, 5, 64])
@pytest.mark.parametrize("rho", [1.0, 1.1])
def test_ensemble_space_transform_is_the_state_space_analysis(n, rho):
    g = torch.Generator().manual_seed(31 * n + int(10 * rho))
    n_state, K = 40, 23
    for alpha in (0.5, 0.0, 1.0):
        X = torch.randn(n_state, n, generator=g, dtype=F64)
        H = torch.randn(K, n_state, generator=g, dtype=F64) / math.sqrt(n_state)
        obs = torch.randn(1, K, generator=g, dtype=F64)
        prec = 0.25 + 2.0 * torch.rand(K, generator=g, dtype=F64)
        prec[torch.rand(K, generator=g) < 0.25] = 0.0                # missing readings
        prec[0] = 1.0
        pred = (H @ X).t().contiguous()                              # [N, K]
        D, status, _ = restate_enkf(pred, obs, prec, None, n, rho, alpha)
        D = D[0, 0]
        assert int(status[0, 0]) == int((prec > 0).sum())
        assert float(D.sum(0).abs().max()) <= 1e-12                 # every column of D sums to 0 over i
        Xa = X + X @ D
        live = prec > 0
        Hl, R = H[live], torch.diag(1.0 / prec[live])
        xbar = X.mean(1, keepdim=True)
        A = rho * (X - xbar)                                         # the inflated forecast anomalies
        Pf = A @ A.t() / (n - 1)
        Kg = Pf @ Hl.t() @ torch.linalg.inv(Hl @ Pf @ Hl.t() + R)
        mean_a = xbar[:, 0] + Kg @ (obs[0, live] - Hl @ xbar[:, 0])
        anom_a = A - alpha * Kg @ Hl @ A
        assert float((Xa.mean(1) - mean_a).abs().max()) <= 1e-10, (n, rho, alpha)
        assert float((Xa - Xa.mean(1, keepdim=True) - anom_a).abs().max()) <= 1e-10, (n, rho, alpha)
        if alpha == 0.0:                                             # the anomalies are the (inflated) forecast's
            assert float((Xa - Xa.mean(1, keepdim=True) - A).abs().max()) <= 1e-10


def test_a_reading_without_weight_is_neutral():
    g = torch.Generator().manual_seed(5)
    n, K, B = 7, 19, 2
    pred, obs = torch.randn(B * n, K, generator=g), torch.randn(B, K, generator=g)
    D0, status, _ = restate_enkf(pred, obs, torch.zeros(K), None, n, 1.0, 0.5)
    assert torch.equal(D0, torch.zeros_like(D0)) and torch.equal(status, torch.zeros_like(status))      # no live reading, rho = 1: exactly no update
    Dt, _, _ = restate_enkf(pred, obs, None, torch.zeros(3, K), n, 1.0, 0.5)
    assert torch.equal(Dt, torch.zeros_like(Dt))
    prec = 0.5 + torch.rand(B, K, generator=g)
    prec[:, ::3] = 0.0
    base, s0, _ = restate_enkf(pred, obs, prec, None, n, 1.1, 0.5)
    for junk in (float("nan"), float("inf"), 3e38):
        o = obs.clone()
        o[prec == 0] = junk
        got, s1, _ = restate_enkf(pred, o, prec, None, n, 1.1, 0.5)
        assert torch.equal(got, base) and torch.equal(s0, s1) and bool(torch.isfinite(got).all())
    o = obs.clone()
    o[1, 1] = float("nan")                                           # a live reading that is not finite: no update for that history alone
    got, s1, _ = restate_enkf(pred, o, prec, None, n, 1.1, 0.5)
    assert int(s1[1, 0]) == -1 and torch.equal(got[1], torch.zeros_like(got[1])) and torch.equal(got[0], base[0])


def test_restate_mix_is_the_member_sum():
    y, D, P = mix_case("n5_local")
    inc = restate_mix(y, D, P)
    n, Dl = 5, y.shape[2] // P
    b, j, p = 3, 2, 1
    want = sum(float(D[b, p, i, j]) * y[b * n + i, 0, p * Dl:(p + 1) * Dl].double() for i in range(n))
    assert float((inc[b * n + j, 0, p * Dl:(p + 1) * Dl] - want).abs().max()) <= 1e-12
    assert torch.equal(restate_mix(y, torch.zeros_like(D), P), torch.zeros_like(inc))


# ------------------------------------------------------------------------------------------------ conditioning of the GPU test's inputs
@pytest.mark.parametrize("n", T_N)
def test_transform_inputs_are_well_conditioned(n):
    worst = 0.0
    for K, B, Ld, wp in transform_cases(n):
        t = transform_case(n, K, B, Ld, wp)
        _, status, cond = restate_enkf(t["pred"], t["obs"], t["prec"], t["taper"], n, t["rho"], t["alpha"])
        worst = max(worst, float(cond.max()))
        assert float(cond.max()) <= COND_MAX, (K, B, Ld, wp, float(cond.max()))
        assert int(status.min()) >= 0 and (Ld == 1 or int(status[:, 1].max()) == 0)
    print(f"enkf transform inputs N = {n}: largest cond(I + C) {worst:.3e}")


def test_end_to_end_inputs_are_well_conditioned_and_the_bf16_envelope():
    for name, set_name, members, hist, local in kalman_cases():
        k = kalman_case(name, set_name, members, hist, local)
        assert float(k["cond"].max()) <= COND_MAX, (name, set_name, members, hist, local, float(k["cond"].max()))
        assert int(k["status"].min()) >= 0 and float(k["inc"].abs().max()) > 0
    env = bf16_envelope()
    assert 0 < env < 1.0                                             # rounded operands leave the increment recognisable: the GPU bound 2 * envelope means something


# ------------------------------------------------------------------------------------------------ the entry points, without a GPU
@pytest.fixture(scope="module")
def lib():
    from sea_amd import build, _native

    build.build(verbose=False)
    return _native.lib()


def _transform_table():
    from sea_amd import _native as N

    p = N.SeaEnkfTransform()
    p.pred, p.obs, p.prec, p.taper, p.D, p.status = 0x100000, 0x110000, 0x120000, 0x130000, 0x140000, 0x150000   # made-up, aligned, never dereferenced
    p.ld_pred, p.ld_obs, p.ld_prec, p.ld_taper = 40, 40, 0, 40
    p.rho, p.alpha = 1.0, 0.5
    p.B, p.N, p.K, p.Ld = 2, 8, 40, 3
    return p


def _mix_table():
    from sea_amd import _native as N

    p = N.SeaEnsembleMix()
    p.y, p.D, p.out, p.inc = 0x100000, 0x200000, 0x300000, 0x400000
    p.Bm, p.N, p.G, p.P, p.Dl, p.Ld = 16, 8, 2, 4, 16, 4
    return p


def test_symbols_and_struct_layouts(lib):
    from sea_amd import _native as N

    for name in ("sea_enkf_transform", "sea_ensemble_mix"):
        assert hasattr(lib, name) and name in N.EXPORTED_SYMBOLS
    assert C.sizeof(N.SeaEnkfTransform) == 112 and C.sizeof(N.SeaEnsembleMix) == 56          # include/sea_hip.h states them
    assert N.SeaEnkfTransform.ld_pred.offset == 48 and N.SeaEnkfTransform.rho.offset == 80 and N.SeaEnkfTransform.B.offset == 96 and N.SeaEnkfTransform.Ld.offset == 108
    assert N.SeaEnsembleMix.Bm.offset == 32 and N.SeaEnsembleMix.Ld.offset == 52
    assert lib.sea_abi_version() == 8 and len(N.ABI_STRUCTS) == 33 and N.ABI_STRUCTS[-1] is N.SeaKvFork and N.ENKF_MAX_N == 128
    # the library reads the fields where the binding writes them: its messages quote the values back
    p = _transform_table()
    p.N = 1
    assert lib.sea_enkf_transform(C.byref(p), None) == -1 and b"N=1" in lib.sea_last_error()
    p = _transform_table()
    p.ld_taper = 39
    assert lib.sea_enkf_transform(C.byref(p), None) == -1 and b"ld_taper=39 must cover K=40" in lib.sea_last_error()
    p = _transform_table()
    p.rho = 0.5
    assert lib.sea_enkf_transform(C.byref(p), None) == -1 and b"rho=0.5" in lib.sea_last_error()
    p = _mix_table()
    p.Ld = 3
    assert lib.sea_ensemble_mix(C.byref(p), N.SEA_BF16, None) == -1 and b"Ld=3 must be 1 or P=4" in lib.sea_last_error()
    p = _mix_table()
    p.Bm = 12
    assert lib.sea_ensemble_mix(C.byref(p), N.SEA_F32, None) == -1 and b"Bm=12 must be a positive multiple of N=8" in lib.sea_last_error()


T_BREAKS = {"null pred": ("pred", None), "null obs": ("obs", None), "null D": ("D", None), "null status": ("status", None), "misaligned pred": ("pred", 0x100002),
            "misaligned taper": ("taper", 0x130001), "N = 1": ("N", 1), "N = 0": ("N", 0), "K = 0": ("K", 0), "B = 0": ("B", 0), "Ld = 0": ("Ld", 0),
            "domains without a taper": ("taper", None), "ld_pred short": ("ld_pred", 39), "ld_obs short": ("ld_obs", 8), "ld_prec short": ("ld_prec", 39),
            "rho below 1": ("rho", 0.99), "rho nan": ("rho", float("nan")), "rho inf": ("rho", float("inf")), "alpha above 1": ("alpha", 1.5),
            "alpha negative": ("alpha", -0.1)}


@pytest.mark.parametrize("what", sorted(T_BREAKS))
def test_transform_refuses_bad_arguments_without_a_device(lib, what):
    p = _transform_table()
    setattr(p, *T_BREAKS[what])
    assert lib.sea_enkf_transform(C.byref(p), None) == -1, what
    assert b"sea_enkf_transform" in lib.sea_last_error()


M_BREAKS = {"null y": ("y", None), "null D": ("D", None), "misaligned y": ("y", 0x100001), "misaligned inc": ("inc", 0x400002), "N = 1": ("N", 1),
            "Bm not a multiple": ("Bm", 12), "G = 0": ("G", 0), "P = 0": ("P", 0), "Dl = 0": ("Dl", 0), "Ld = 2": ("Ld", 2), "Ld = 0": ("Ld", 0),
            "out is y": ("out", 0x100000), "out overlaps y": ("out", 0x100040)}


@pytest.mark.parametrize("what", sorted(M_BREAKS) + ["neither out nor inc", "bad dtype"])
def test_mix_refuses_bad_arguments_without_a_device(lib, what):
    from sea_amd import _native as N

    p = _mix_table()
    dt = N.SEA_BF16
    if what in M_BREAKS:
        setattr(p, *M_BREAKS[what])
    elif what == "neither out nor inc":
        p.out = p.inc = None
    else:
        dt = 5
    assert lib.sea_ensemble_mix(C.byref(p), dt, None) == -1, what
    assert b"sea_ensemble_mix" in lib.sea_last_error()


def test_unsupported_sizes_and_null_tables(lib):
    from sea_amd import _native as N

    p = _transform_table()
    p.N = 129
    assert lib.sea_enkf_transform(C.byref(p), None) == -3 and b"sea_enkf_transform" in lib.sea_last_error() and b"N=129" in lib.sea_last_error()
    p = _mix_table()
    p.N, p.Bm = 129, 258
    assert lib.sea_ensemble_mix(C.byref(p), N.SEA_BF16, None) == -3 and b"sea_ensemble_mix" in lib.sea_last_error() and b"N=129" in lib.sea_last_error()
    assert lib.sea_enkf_transform(None, None) == -1 and b"sea_enkf_transform" in lib.sea_last_error()
    assert lib.sea_ensemble_mix(None, N.SEA_BF16, None) == -1 and b"sea_ensemble_mix" in lib.sea_last_error()
    # prec, taper (one domain), out or inc may be NULL: such tables pass the pointer checks and fail only at the last check, which this test breaks
    p = _transform_table()
    p.prec = p.taper = None
    p.Ld, p.alpha = 1, 2.0
    assert lib.sea_enkf_transform(C.byref(p), None) == -1 and b"alpha=2" in lib.sea_last_error()
    for drop in ("out", "inc"):
        p = _mix_table()
        setattr(p, drop, None)
        p.N, p.Bm = 129, 258
        assert lib.sea_ensemble_mix(C.byref(p), N.SEA_F32, None) == -3


# ------------------------------------------------------------------------------------------------ refusals of the Python layers
def test_python_layers_refuse_before_a_device_is_touched():
    from sea_amd import ops
    from sea_amd.ensemble import SensorKalman, SensorSet
    from sea_amd.utils.train_utils import SensorKalman as SK2, gaspari_cohn as gc2
    from sea_amd.ensemble import gaspari_cohn

    assert SK2 is SensorKalman and gc2 is gaspari_cohn
    c = host_case("a")
    dec = make_decoder("a").set_compute_dtype("bf16")
    P, D_, G = c["P"], c["D"], len(c["groups"])
    s = SensorSet(dec, P, [0, 1, 8], [3, 4, 11], [0, 2, 1])
    for members in (1, 129, 0, True, 2.0):
        with pytest.raises(ValueError):
            SensorKalman(dec, P, members, s)
    for kw in (dict(inflation=0.9), dict(inflation=float("inf")), dict(anomaly_gain=-0.1), dict(anomaly_gain=1.1), dict(taper=torch.ones(P, 4)),
               dict(taper=torch.ones(P + 1, 3)), dict(taper=torch.full((P, 3), 2.0)), dict(taper=torch.ones(3)), dict(sigma=-1.0), dict(sensors=None)):
        args = dict(sensors=s)
        args.update(kw)
        with pytest.raises(ValueError):
            SensorKalman(dec, P, 2, **args)
    ka = SensorKalman(dec, P, 2, s, sigma=[0.5, 1.0, 2.0], inflation=1.05, taper=torch.ones(P, 3))
    assert ka._like._prec_host == [4.0, 0.25, 1.0]                  # SensorLikelihood's folding
    y, obs = torch.zeros(4, G, P * D_), torch.zeros(2, 3)
    for yy, oo, pp in ((torch.zeros(3, G, P * D_), obs, None), (torch.zeros(4, G, P * D_ + 1), obs, None), (y, torch.zeros(2, 2), None), (y, obs.double(), None),
                       (y, obs, torch.tensor([1.0, -2.0, 1.0]))):
        with pytest.raises(ValueError):
            ka.analyse(yy, oo, pp)
    with pytest.raises(RuntimeError, match="MI355X"):
        ka.analyse(y, obs)
    pred = torch.zeros(4, 3)
    with pytest.raises(RuntimeError, match="MI355X"):
        ops.enkf_transform(pred, obs, 2)
    for kw in (dict(members=1), dict(members=129), dict(pred=torch.zeros(4, 4)), dict(pred=pred.double()), dict(prec=torch.ones(4)), dict(taper=torch.ones(2, 4)),
               dict(rho=0.5), dict(alpha=1.5), dict(obs=torch.zeros(6))):
        args = dict(pred=pred, obs=obs, members=2)
        args.update(kw)
        with pytest.raises(ValueError):
            ops.enkf_transform(**args)
    Dm = torch.zeros(2, 1, 2, 2)
    with pytest.raises(RuntimeError, match="MI355X"):
        ops.ensemble_mix(y, Dm, P)
    for yy, dd, kw in ((y, torch.zeros(2, 2, 2, 2), {}), (y, torch.zeros(1, 1, 2, 2), {}), (y, torch.zeros(2, 1, 2, 3), {}), (y.double(), Dm, {}), (y[:, :, ::2], Dm, {}),
                       (y, Dm, dict(output=False)), (y, Dm.double(), {})):
        with pytest.raises(ValueError):
            ops.ensemble_mix(yy, dd, P, **kw)


# ------------------------------------------------------------------------------------------------ localisation helpers
def test_gaspari_cohn():
    from sea_amd.ensemble import gaspari_cohn

    c = 2.5
    r = torch.linspace(0.0, 3.0 * c, 601, dtype=F64)
    t = gaspari_cohn(r, c)
    assert t.dtype == F64 and float(t[0]) == 1.0 and bool((t[r >= 2 * c] == 0).all()) and bool((t >= 0).all()) and bool((t <= 1).all())
    assert bool((t[1:] <= t[:-1]).all()) and bool((t[1:][r[1:] < 2 * c] < t[:-1][r[1:] < 2 * c]).all())         # monotone, strictly inside the support
    inner = lambda z: -z ** 5 / 4 + z ** 4 / 2 + 5 * z ** 3 / 8 - 5 * z ** 2 / 3 + 1                             # noqa: E731
    outer = lambda z: z ** 5 / 12 - z ** 4 / 2 + 5 * z ** 3 / 8 + 5 * z ** 2 / 3 - 5 * z + 4 - 2 / (3 * z)      # noqa: E731
    got = gaspari_cohn(torch.tensor([c / 2, c, 1.5 * c, -c / 2], dtype=F64), c)
    want = torch.tensor([inner(0.5), inner(1.0), outer(1.5), inner(0.5)], dtype=F64)
    assert float((got - want).abs().max()) <= 1e-14 and abs(inner(1.0) - outer(1.0)) <= 1e-15 and abs(float(want[1]) - 5.0 / 24.0) <= 1e-15
    assert gaspari_cohn(torch.tensor([0.0, 1.0, 5.0]), 1.0).dtype == torch.float32
    for bad in (0.0, -1.0, float("nan"), True, None):
        with pytest.raises(ValueError):
            gaspari_cohn(r, bad)


def test_sensor_taper_on_the_synthetic_mesh():
    from sea_amd.ensemble import SensorSet, gaspari_cohn
    from sea_amd.models.encoder_decoder import Decode
    from sea_amd.utils.data_processors import DataPartitioner2D, MeshProcessor, MeshUnpatcher
    from tests.conftest import load_golden

    gld = load_golden("unpatch_5x5")
    m, n = (int(v) for v in gld["mn"])
    xy = torch.from_numpy(gld["xy"]).clone()
    imap0 = torch.from_numpy(gld["index_map"])
    # the first point of patch 7 moves to the mean of the patch's other points: it then sits at the patch's centroid (and stays in the cell, which is convex)
    row = imap0[7][imap0[7] >= 0]
    q, others = int(row[0]), row[1:]
    xy[:, q] = xy[:, others].mean(1)
    part = DataPartitioner2D(xy[0], xy[1], m=m, n=n, device="cpu")
    P, C_ = part.padded_index_map.shape
    assert int(part.point_slot[q]) // C_ == 7
    groups = [[0, 1], [2]]
    mesh = MeshUnpatcher(part, groups)
    dec = Decode(groups, C_, 16, 8)
    points = [q, int(imap0[0, 0]), int(imap0[24, 0]), int(imap0[12, 3])]
    s = mesh.sensor_set(dec, points, [0, 2, 1, 0])
    radius = 0.3 * float(xy[0].max() - xy[0].min())
    t = mesh.sensor_taper(s, radius)
    assert t.shape == (P, 4) and t.dtype == torch.float32 and bool((t >= 0).all()) and bool((t <= 1).all())
    assert abs(float(t[7, 0]) - 1.0) <= 1e-6                                          # a sensor at the patch's centroid
    idx = part.padded_index_map.long()
    for p in (0, 7, 24):                                                              # the definition, patch by patch
        cen = part.full_coords[idx[p][idx[p] >= 0]].mean(0)
        dist = (part.full_coords[torch.tensor(points)] - cen).norm(dim=1)
        assert float((t[p] - gaspari_cohn(dist, radius)).abs().max()) <= 1e-6
    assert float(t[0, 2]) == 0.0 and float(t[24, 1]) == 0.0                           # opposite corners are beyond 2 * radius
    with pytest.raises(ValueError):
        mesh.sensor_taper(SensorSet(dec, P, [0], [0], [0]), radius)                   # built without points
    with pytest.raises(ValueError):
        mesh.sensor_taper(s, 0.0)
    proc = MeshProcessor(dict(dimension="2D", field_groups=groups, m=m, n=n), xy, device="cpu")
    with pytest.raises(ValueError, match="patchify_and_scale first"):
        proc.sensor_taper(s, radius)
