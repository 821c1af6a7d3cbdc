"""Threshold scores of an ensemble on the device: sea_decode_member_brier through ops.decode_member_brier, Decode.member_brier and
FieldThresholdVerification; sea_ensemble_brier through ops.ensemble_brier and SensorThresholdVerification.

Reference: `restate_field_brier` / `restate_brier` of tests/test_brier_cpu.py, the fp64 restatement of the definitions in include/sea_hip.h.
  kernel      on EXACT operands (tests/test_field_verify_gpu.exact_case: decoded values, readings and thresholds are multiples of 0.25, so x == thr and
              y == thr occur and the restatement sees the kernel's values): hist, hits, status and the three counts in sums EQUAL; the f32 maps within
              1e-6 max(1, max |ref|) (the project's bound for fp64 values stored as f32); the two fp64 sums within SUMS_TOL max(1, max |ref|), the
              figure tests/test_field_verify_gpu.py derives for longer, cancelling sums over the same cells (these have non-negative terms only)
  bits        the prob map against ops.decode_member_quantiles' exceed map (equal weights); the field launch against ops.ensemble_brier on the same
              values; two runs; a history alone against the batch
  random      bf16 operands: against the fp64 restatement on the cells where no live member's fp64 value lies within g = S 2^-22 (sum_s |h_s| |W2_cs| +
              |b_c|) of the threshold — the fp32-accumulation bound of the decode: S products, each within 2^-24 relative of its exact value after the
              fp32 add, summed in any order, with a factor 4 for the two accumulators and the bias — m equal and p within 1e-6; the excluded share is
              computed from the restatement before the device is touched and is at most 1 %."""
import functools

import pytest
import torch

from tests.test_brier_cpu import restate_brier, restate_field_brier
from tests.test_decode_loss_gpu import DEV, TOL_F32, case, decoder
from tests.test_field_enkf_cpu import decode_members, field_states
from tests.test_field_verify_cpu import field_logw
from tests.test_field_verify_gpu import SUMS_TOL, X_B, X_C, X_COUNTS, X_CP, X_F, X_MEMBERS, X_P, decode_exact, dev, exact_case
from tests.test_verify_cpu import close
from tests.test_verify_gpu import same_bits

pytestmark = pytest.mark.gpu

F64 = torch.float64
MAPS = ("prob", "brier")
THR_POOL = (0.0, -1.0, 0.25, 1.0, -2.5, 2.0, 0.5, -0.25)   # multiples of 0.25 inside the decoded values' and the readings' range


def thresholds(T):
    """[T, X_F]: field f takes the pool's values shifted by 0.25 f."""
    return torch.tensor([[THR_POOL[t] + 0.25 * f for f in range(X_F)] for t in range(T)], dtype=torch.float32)


def run_brier(t, n, thr, accumulate=False, out=None, maps=MAPS, H=None, bias=None, obs=None, logw="case", hist=None):
    """ops.decode_member_brier on an exact case (hist: that history alone)."""
    from sea_amd import ops

    P = X_P
    H = t["H"] if H is None else H
    obs, prec = t["obs"] if obs is None else obs, t["prec"]
    logw = t["logw"] if isinstance(logw, str) else logw
    if hist is not None:
        H, obs = H[hist * n * P:(hist + 1) * n * P], obs[hist * P:(hist + 1) * P]
        prec = None if prec is None else prec[hist * P:(hist + 1) * P]
        logw = None if logw is None else logw[hist * n:(hist + 1) * n]
    grp = [dict(H=H.to(DEV).to(torch.bfloat16), W2=t["W2"].to(DEV).to(torch.bfloat16), bias=(t["bias"] if bias is None else bias).to(DEV))]
    return ops.decode_member_brier(grp, obs.to(DEV), t["C"], t["Cp"], P, n, thr.to(DEV), prec=dev(prec), counts=t["counts"].to(DEV), logw=dev(logw),
                                   accumulate=accumulate, maps=maps, out=out)


def prefilled(B, n, T, fill, width=X_C):
    """Output buffers that hold NaN (or `fill`) and -7: every element has to be written."""
    out = {k: torch.full((T, B, X_P, X_F, width), fill, device=DEV) for k in MAPS}
    out.update(sums=torch.full((B, X_F, T, 5), fill, device=DEV, dtype=F64), hist=torch.full((B, X_F, T, n + 1), -7, device=DEV, dtype=torch.int64),
               hits=torch.full((B, X_F, T, n + 1), -7, device=DEV, dtype=torch.int64), status=torch.full((B,), -7, device=DEV, dtype=torch.int32))
    return out


def check_exact(got, ref, tag):
    """The kernel's bounds (the module docstring); returns the largest error / bound of the f32 maps and of the fp64 sums."""
    got = {k: v.cpu() for k, v in got.items()}
    assert torch.equal(got["hist"], ref["hist"]) and torch.equal(got["hits"], ref["hits"]) and torch.equal(got["status"].long(), ref["status"]), tag
    for j in (0, 3, 4):
        assert torch.equal(got["sums"][..., j], ref["sums"][..., j]), tag + ("sums", j)
    w32, w64 = 0.0, 0.0
    for k in MAPS:
        ok, ratio = close(got[k], ref[k], 1e-6)
        w32 = max(w32, ratio)
        assert ok, tag + (k, ratio)
    for j in (1, 2):
        ok, ratio = close(got["sums"][..., j], ref["sums"][..., j], SUMS_TOL)
        w64 = max(w64, ratio)
        assert ok, tag + ("sums", j, ratio)
    return w32, w64


@functools.lru_cache(maxsize=None)
def exact_reference(n, counts, wp, wl, T, C_=X_C, Cp=X_CP):
    t = exact_case(n, counts, wp, wl, C_, Cp)
    return restate_field_brier(t["Y"], t["obs"].view(X_B, X_P, X_F, C_), t["w"], t["logw"], n, thresholds(T))


# ------------------------------------------------------------------------------------------------ 1: the kernel on exact operands
@pytest.mark.parametrize("n", X_MEMBERS)
def test_kernel_against_fp64_on_exact_operands(n):
    worst32, worst64, cases, ties = 0.0, 0.0, 0, 0
    for counts in X_COUNTS:
        for wp in (False, True):
            for wl in (False, True):
                t = exact_case(n, counts, wp, wl)
                for T in (1, 3, 8):
                    thr = thresholds(T)
                    ref = exact_reference(n, counts, wp, wl, T)
                    out = prefilled(X_B, n, T, float("nan"), X_C + 3)
                    got = run_brier(t, n, thr, out=out)
                    assert all(got[k].data_ptr() == out[k].data_ptr() for k in out)
                    assert all(float(got[k][..., X_C:].abs().max()) == 0.0 for k in MAPS)          # the pad columns are dead cells: written, 0
                    a, b = check_exact({k: v[..., :X_C] if k in MAPS else v for k, v in got.items()}, ref, (n, counts, wp, wl, T))
                    worst32, worst64, cases = max(worst32, a), max(worst64, b), cases + 1
                    live = (t["w"] > 0).unsqueeze(0)
                    tf = thr.to(F64).view(T, 1, 1, X_F, 1)
                    ties += int(((t["obs"].view(X_B, X_P, X_F, X_C).to(F64).unsqueeze(0) == tf) & live).sum()) + int((t["Y"].view(X_B, n, X_P, X_F, X_C)[:, 0].unsqueeze(0) == tf).sum())
                if wl and n >= 2:
                    assert int(exact_reference(n, counts, wp, wl, 1)["status"][0]) == n - 1       # the dead member is not counted
    assert ties > 0                                                                               # x == thr and y == thr occur: strictness is tested
    print(f"brier N = {n}: largest error / bound over {cases} cases: f32 maps {worst32:.3e} (bound 1e-6), fp64 sums {worst64:.3e} (bound {SUMS_TOL:.1e})")


# ------------------------------------------------------------------------------------------------ 2: a field wider than one chunk of tiles
def test_a_field_wider_than_one_chunk_of_tiles():
    """530 columns in 544 are 17 tiles: a workgroup scores 16, so a field has two chunks whose partials the finish launch adds in order; counts 513
    leave the second chunk ONE valid column, counts 512 none (it leaves at once)."""
    n, C_, Cp, T = 5, 530, 544, 3
    for counts in ((C_, 513), (512, 1)):
        t = exact_case(n, counts, True, True, C_, Cp)
        ref = exact_reference(n, counts, True, True, T, C_, Cp)
        got = run_brier(t, n, thresholds(T), out=prefilled(X_B, n, T, float("nan"), C_ + 3))
        assert all(float(got[k][..., C_:].abs().max()) == 0.0 for k in MAPS)
        a, b = check_exact({k: v[..., :C_] if k in MAPS else v for k, v in got.items()}, ref, (counts,))
        print(f"brier wide {counts}: largest error / bound: f32 maps {a:.3e} (bound 1e-6), fp64 sums {b:.3e} (bound {SUMS_TOL:.1e})")
        assert same_bits(run_brier(t, n, thresholds(T), out=prefilled(X_B, n, T, 7.0, C_ + 3)), got)
        alone = run_brier(t, n, thresholds(T), hist=1)
        assert same_bits({k: v[:, 0] if k in MAPS else v[0] for k, v in alone.items()}, {k: v[:, 1, ..., :C_] if k in MAPS else v[1] for k, v in got.items()})


# ------------------------------------------------------------------------------------------------ 3: the bits of the exceedance maps
@pytest.mark.parametrize("n", [1, 5, 64, 65, 128])
def test_equal_weights_give_the_bits_of_the_quantile_launch(n):
    from sea_amd import ops

    T = 3
    for counts in X_COUNTS:
        t = exact_case(n, counts, False, False)                                           # every valid cell is live: the quantile launch knows no readings
        got = run_brier(t, n, thresholds(T), maps=("prob",))
        grp = [dict(H=t["H"].to(DEV).to(torch.bfloat16), W2=t["W2"].to(DEV).to(torch.bfloat16), bias=t["bias"].to(DEV))]
        q = ops.decode_member_quantiles(grp, t["C"], t["Cp"], X_P, n, thr=thresholds(T).to(DEV), counts=t["counts"].to(DEV))
        assert same_bits(dict(prob=got["prob"]), dict(prob=q["exceed"])), (n, counts)
        assert "brier" not in got
    # random operands: the two launches share their decode, so the bits agree on inexact values too
    k = random_case(n, False)
    got = run_random(k, n, maps=("prob",))
    grp = [dict(H=k["H"].to(DEV), W2=k["W2"].to(DEV), bias=k["bias"].to(DEV))]
    q = ops.decode_member_quantiles(grp, R_C, R_CP, R_P, n, thr=k["thr"].to(DEV))
    assert same_bits(dict(prob=got["prob"]), dict(prob=q["exceed"])), n


# ------------------------------------------------------------------------------------------------ 4: against the sensor kernel
@pytest.mark.parametrize("n", [2, 17, 64, 128])
def test_cells_are_scored_as_sensors(n):
    """ops.ensemble_brier on the same exact values with every cell a sensor, (patch, field, cell) order, a threshold per sensor: the f32 maps have equal
    BITS (one device function scores a cell and a sensor), status equal, and its histograms are the field launch's added over the fields."""
    from sea_amd import ops

    B, P, F, C_, T = X_B, X_P, X_F, X_C, 3
    K = P * F * C_
    thr = thresholds(T)
    tk = thr.view(T, 1, F, 1).expand(T, P, F, C_).reshape(T, K).contiguous()
    for counts, wp, wl in ((X_COUNTS[0], True, True), (X_COUNTS[0], False, False), (X_COUNTS[1], True, False)):
        t = exact_case(n, counts, wp, wl)
        got = run_brier(t, n, thr)
        pred = t["Y"].reshape(B * n, K).to(torch.float32).to(DEV)
        out = dict(prob=torch.full((T, B, K), float("nan"), device=DEV), brier=torch.full((T, B, K), float("nan"), device=DEV))
        s = ops.ensemble_brier(pred, t["obs"].reshape(B, K).to(DEV), n, tk.to(DEV), prec=t["w"].reshape(B, K).to(torch.float32).to(DEV), logw=dev(t["logw"]), out=out)
        assert torch.equal(got["status"], s["status"]) and s["prob"].data_ptr() == out["prob"].data_ptr()
        assert same_bits({k: got[k].reshape(T, B, K) for k in MAPS}, {k: s[k] for k in MAPS}), (n, counts, wp, wl)
        assert torch.equal(got["hist"].sum(1), s["hist"]) and torch.equal(got["hits"].sum(1), s["hits"])
        for j in (0, 3, 4):
            assert torch.equal(got["sums"].sum(1)[..., j], s["sums"][..., j])
        for j in (1, 2):
            ok, ratio = close(got["sums"].sum(1)[..., j].cpu(), s["sums"][..., j].cpu(), SUMS_TOL)
            assert ok, (n, counts, wp, wl, j, ratio)
        ref = restate_brier(t["Y"].reshape(B * n, K), t["obs"].reshape(B, K), t["w"].reshape(B, K), t["logw"], n, tk)
        sc = {k: v.cpu() for k, v in s.items()}
        assert torch.equal(sc["hist"], ref["hist"]) and torch.equal(sc["hits"], ref["hits"])


@pytest.mark.parametrize("K", [1, 15, 16, 17, 100])
def test_sensor_kernel_at_tile_edges(K):
    """16 sensors per workgroup: one sensor, a tile less one, a tile, a tile and one, several tiles with a tail; [K] and [B, K] precisions."""
    from sea_amd import ops
    from tests.test_brier_cpu import sensor_case

    for n, wp, wl in ((5, True, True), (65, False, False), (128, True, False)):
        t = sensor_case(n, 3, K, 2, wp, wl)
        ref = restate_brier(t["pred"], t["obs"], t["prec"], t["logw"], n, t["thr"])
        got = ops.ensemble_brier(t["pred"].to(DEV), t["obs"].to(DEV), n, t["thr"].to(DEV), prec=dev(t["prec"]), logw=dev(t["logw"]))
        got = {k: v.cpu() for k, v in got.items()}
        assert torch.equal(got["hist"], ref["hist"]) and torch.equal(got["hits"], ref["hits"]) and torch.equal(got["status"].long(), ref["status"])
        for j in (0, 3, 4):
            assert torch.equal(got["sums"][..., j], ref["sums"][..., j])
        for k, tol in (("prob", 1e-6), ("brier", 1e-6)):
            assert close(got[k], ref[k], tol)[0], (K, n, k)
        for j in (1, 2):
            assert close(got["sums"][..., j], ref["sums"][..., j], SUMS_TOL)[0], (K, n, j)
        if wp:
            one = ops.ensemble_brier(t["pred"].to(DEV), t["obs"].to(DEV), n, t["thr"].to(DEV), prec=t["prec"][1].contiguous().to(DEV), logw=dev(t["logw"]))
            assert same_bits({k: v[1] if k not in MAPS else v[:, 1] for k, v in one.items()}, {k: v[1].to(DEV) if k not in MAPS else v[:, 1].to(DEV) for k, v in got.items()})


# ------------------------------------------------------------------------------------------------ 5: special cases
@pytest.mark.parametrize("n,wl", [(5, False), (5, True), (128, True)])
def test_a_value_that_is_not_finite_marks_its_cell_alone(n, wl):
    t = exact_case(n, X_COUNTS[0], True, wl)
    T = 3
    thr = thresholds(T)
    clean = run_brier(t, n, thr)
    f0, c0 = 1, 7
    bias = t["bias"].clone()
    bias[f0 * X_CP + c0] = float("inf")                                                   # every member's value at column c0 of field f0 is +inf
    d = decode_exact(t["H"], t["W2"], bias, t["prec"], X_COUNTS[0], n)
    ref = restate_field_brier(d["Y"], t["obs"].view(X_B, X_P, X_F, X_C), t["w"], t["logw"], n, thr)
    got = run_brier(t, n, thr, out=prefilled(X_B, n, T, 7.0), bias=bias)
    check_exact(got, ref, (n, wl))
    live = t["w"][:, :, f0, c0] > 0                                                       # [B, P]
    assert int(live.sum()) > 0
    for k in MAPS:
        cell = got[k][:, :, :, f0, c0].cpu()
        assert bool(torch.isnan(cell[:, live]).all()) and float(cell[:, ~live].abs().sum()) == 0.0
        other = got[k].clone()
        other[:, :, :, f0, c0] = clean[k][:, :, :, f0, c0]
        assert same_bits({k: other}, {k: clean[k]})                                       # no other cell sees it
    assert torch.equal(got["sums"][:, f0, :, 4].cpu(), live.sum(1).to(F64).view(X_B, 1).expand(X_B, T)) and float(got["sums"][:, 1 - f0, :, 4].abs().max()) == 0.0
    assert torch.equal(got["sums"][:, f0, :, 0].cpu(), clean["sums"][:, f0, :, 0].cpu() - live.sum(1).to(F64).view(X_B, 1))
    if wl:                                                                                # NaN in the hidden row of the DEAD member reaches nothing
        H = t["H"].clone()
        H[(n + 2) * X_P:(n + 3) * X_P] = float("nan")
        assert same_bits(run_brier(t, n, thr, H=H), clean)


def test_an_invalid_history_is_left_out_and_accumulate_adds():
    n, T = 17, 3
    thr = thresholds(T)
    t = exact_case(n, X_COUNTS[0], True, True)
    clean = run_brier(t, n, thr)
    for badv in (float("nan"), float("inf")):
        logw = t["logw"].clone()
        logw[n + 3] = badv
        got = run_brier(t, n, thr, out=prefilled(X_B, n, T, float("nan")), logw=logw)
        assert got["status"].tolist() == [n - 1, -1]
        assert all(float(got[k][:, 1].abs().max()) == 0.0 for k in MAPS) and float(got["sums"][1].abs().max()) == 0.0
        assert int(got["hist"][1].abs().sum()) == 0 and int(got["hits"][1].abs().sum()) == 0
        assert same_bits({k: v[:, 0] if k in MAPS else v[0] for k, v in got.items()}, {k: v[:, 0] if k in MAPS else v[0] for k, v in clean.items()})
        acc = {k: clean[k].clone() for k in ("sums", "hist", "hits")}
        run_brier(t, n, thr, accumulate=True, out=acc, maps=(), logw=logw)              # nothing is added for history 1
        assert same_bits({k: v[1] for k, v in acc.items()}, {k: clean[k][1] for k in acc})
    none = torch.full_like(t["logw"], float("-inf"))
    assert run_brier(t, n, thr, logw=none)["status"].tolist() == [-1, -1]
    # accumulate: the sum of two calls — integers exact, the fp64 sums the single calls' sums added in fp64
    obs2 = t["obs"] + 0.5
    second = run_brier(t, n, thr, obs=obs2)
    acc = {k: clean[k].clone() for k in ("sums", "hist", "hits")}
    both = run_brier(t, n, thr, obs=obs2, accumulate=True, out=acc, maps=("brier",))
    assert both["sums"].data_ptr() == acc["sums"].data_ptr() and "prob" not in both
    assert torch.equal(both["hist"], clean["hist"] + second["hist"]) and torch.equal(both["hits"], clean["hits"] + second["hits"])
    assert same_bits(dict(sums=both["sums"], brier=both["brier"]), dict(sums=clean["sums"] + second["sums"], brier=second["brier"]))
    assert not torch.equal(second["hits"], clean["hits"])


# ------------------------------------------------------------------------------------------------ 6: reproducibility
@pytest.mark.parametrize("n", [5, 65])
def test_two_runs_and_a_history_alone_give_the_same_bits(n):
    T = 8
    for counts, wp, wl in ((X_COUNTS[0], True, True), (X_COUNTS[1], False, False)):
        t = exact_case(n, counts, wp, wl)
        a, b = run_brier(t, n, thresholds(T)), run_brier(t, n, thresholds(T), out=prefilled(X_B, n, T, 3.0))
        assert same_bits(a, b)
        for h in range(X_B):
            alone = run_brier(t, n, thresholds(T), hist=h)
            assert same_bits({k: v[:, 0] if k in MAPS else v[0] for k, v in alone.items()}, {k: v[:, h] if k in MAPS else v[h] for k, v in a.items()}), (n, h)
    k = random_case(n, True)
    assert same_bits(run_random(k, n), run_random(k, n))


# ------------------------------------------------------------------------------------------------ 7: random bf16 operands
R_B, R_P, R_F, R_C, R_CP, R_S = 2, 2, 2, 40, 64, 72
R_THR = ((-0.55, 0.35, 1.15), (-0.85, 0.05, 0.65))   # per field; between the multiples of 2^-k that bf16 products like to land on


@functools.lru_cache(maxsize=None)
def random_case(n, with_logw, seed=11):
    """bf16-representable H, W2 and an f32 bias; Y, the decode in fp64; g, the band of the module docstring; thr [T, F]."""
    gen = torch.Generator().manual_seed(seed + 10 * n + with_logw)
    M = R_B * n * R_P
    H = torch.randn(M, R_S, generator=gen).to(torch.bfloat16)
    W2 = torch.zeros(R_F * R_CP, R_S)
    W2.view(R_F, R_CP, R_S)[:, :R_C] = 0.12 * torch.randn(R_F, R_C, R_S, generator=gen)
    W2 = W2.to(torch.bfloat16)
    bias = torch.zeros(R_F * R_CP)
    bias.view(R_F, R_CP)[:, :R_C] = 0.3 * torch.randn(R_F, R_C, generator=gen)
    Y = (H.double() @ W2.double().t() + bias.double()).view(R_B * n, R_P, R_F, R_CP)[..., :R_C].contiguous()
    g = R_S * 2.0 ** -22 * ((H.double().abs() @ W2.double().abs().t()) + bias.double().abs()).view(R_B * n, R_P, R_F, R_CP)[..., :R_C]
    obs = torch.randn(R_B * R_P, R_F, R_C, generator=gen)
    thr = torch.tensor(R_THR, dtype=torch.float32).t().contiguous()                       # [T, F]
    return dict(H=H, W2=W2, bias=bias, Y=Y, g=g, obs=obs, thr=thr, logw=field_logw(n, R_B, 40 + n) if with_logw else None)


def run_random(k, n, maps=MAPS):
    from sea_amd import ops

    grp = [dict(H=k["H"].to(DEV), W2=k["W2"].to(DEV), bias=k["bias"].to(DEV))]
    return ops.decode_member_brier(grp, k["obs"].to(DEV), R_C, R_CP, R_P, n, k["thr"].to(DEV), logw=dev(k["logw"]), maps=maps)


@pytest.mark.parametrize("n,wl", [(5, False), (17, True), (64, False), (65, True), (128, False)])
def test_random_operands_away_from_the_thresholds(n, wl):
    k = random_case(n, wl)
    T = k["thr"].shape[0]
    B, P, F, C_ = R_B, R_P, R_F, R_C
    w = torch.ones(B, P, F, C_, dtype=F64)
    ref = restate_field_brier(k["Y"], k["obs"].view(B, P, F, C_), w, k["logw"], n, k["thr"])
    # the excluded cells, from the restatement alone: a live member within g of the threshold (a dead member's value reaches nothing)
    alive = torch.ones(B, n, dtype=torch.bool) if k["logw"] is None else (k["logw"].view(B, n) != float("-inf"))
    near = ((k["Y"].unsqueeze(0) - k["thr"].to(F64).view(T, 1, 1, F, 1)).abs() <= k["g"].unsqueeze(0)).view(T, B, n, P, F, C_)
    excluded = (near & alive.view(1, B, n, 1, 1, 1)).any(2)                                # [T, B, P, F, C]
    share = float(excluded.double().mean())
    print(f"brier random N = {n}: excluded share {share:.4%} (band g <= {float(k['g'].max()):.2e})")
    assert share <= 0.01
    got = {kk: v.cpu() for kk, v in run_random(k, n).items()}
    keep = ~excluded
    err = (got["prob"].to(F64) - ref["prob"])[keep].abs().max()
    assert float(err) <= 1e-6, float(err)
    if not wl:                                                                            # equal weights: p = m / L, so m is read from the map
        m = (got["prob"].to(F64) * n).round().long()
        assert torch.equal(m[keep], ref["m"][keep])
    ok, ratio = close(got["brier"][keep], ref["brier"][keep], 1e-6)
    assert ok, ratio
    # the sums are those of the kernel's own maps (every cell is live here)
    count = float(P * C_)
    own = torch.stack([got["brier"].to(F64).sum((2, 4)), got["prob"].to(F64).sum((2, 4))], -1).permute(1, 2, 0, 3)   # [B, F, T, 2]
    assert float((got["sums"][..., 1:3] - own).abs().max()) <= 1e-6 * count
    assert torch.equal(got["sums"][..., 0], torch.full((B, F, T), count, dtype=F64)) and torch.equal(got["hist"].sum(-1), torch.full((B, F, T), int(count)))
    print(f"brier random N = {n}: p error {float(err):.3e} (bound 1e-6), sums against the maps {float((got['sums'][..., 1:3] - own).abs().max()) / (1e-6 * count):.3e} of the bound")


# ------------------------------------------------------------------------------------------------ 8: the classes
def class_inputs(name, members, hist, dtype, seed=5):
    c = case(name)
    P, C_ = c["P"], c["n_inp"]
    F = sum(len(g) for g in c["groups"])
    y, z = field_states(name, members, hist, dtype)
    gen = torch.Generator().manual_seed(seed)
    Y = decode_members(name, z)                                                           # float64 [Bm, P, F, C]
    obs = (Y.view(hist, members, P, F, C_).mean(1) + 0.5 * torch.randn(hist, P, F, C_, generator=gen, dtype=F64)).to(torch.float32)
    prec = 0.25 + torch.rand(hist, P, F, C_, generator=gen)
    prec[torch.rand(hist, P, F, C_, generator=gen) < 0.1] = 0.0
    q = torch.quantile(Y.transpose(2, 3).reshape(-1, F), torch.tensor([0.3, 0.7], dtype=F64), dim=0)   # [2, F]: thresholds inside each field's range
    return dict(y=y, z=z, Y=Y, obs=obs, prec=prec, thr=q.to(torch.float32).contiguous(), counts=[C_, 1, C_ - 1, 0, C_, C_, 3, C_, C_][:P], P=P, F=F, C=C_)


def test_field_class_fused_gives_the_bits_of_the_ops_call():
    from sea_amd import ops
    from sea_amd.ensemble import FieldThresholdVerification, ThresholdScores

    name, n, hist = "a", 5, 3
    k = class_inputs(name, n, hist, "bf16")
    dec = decoder(name, "bf16")
    P, F, C_ = k["P"], k["F"], k["C"]
    logw = field_logw(n, hist, 3)
    v = FieldThresholdVerification(dec, P, n, k["thr"], counts=k["counts"], fused=True)
    s = v(k["y"].to(DEV), k["obs"].to(DEV), k["prec"].to(DEV), logw=logw.to(DEV), maps=MAPS)
    assert isinstance(s, ThresholdScores) and s.weighted and tuple(s.prob.shape) == (2, hist, P, F, C_) and tuple(s.brier.shape) == (hist, F, 2)
    # the same first-layer rows, then the ops-level call
    c = case(name)
    G, D = len(c["groups"]), c["D"]
    M = hist * n * P
    z = k["y"].to(DEV).reshape(hist * n, G, P, D).permute(0, 2, 1, 3)
    zf = z.to(torch.float32).contiguous().view(M, G * D)
    za = torch.empty(M, G * D, device=DEV, dtype=torch.bfloat16)
    ops.convert(zf, za)
    W1, W2 = dec._weights(torch.bfloat16)
    hid = [torch.empty(M, c["hidden"], device=DEV, dtype=torch.bfloat16) for _ in range(G)]
    ops.gemm_grouped([dict(A=za[:, g * D:(g + 1) * D], W=W1[g], Cact=hid[g], act=1) for g in range(G)], torch.bfloat16)
    r = ops.decode_member_brier([dict(H=hid[g], W2=W2[g], bias=dec._shadow[3][g]) for g in range(G)], k["obs"].to(DEV).view(hist * P, F, C_), C_, dec._n_inp_p, P, n,
                                k["thr"].to(DEV), prec=k["prec"].to(DEV).view(hist * P, F, C_), counts=torch.tensor(k["counts"], dtype=torch.int32, device=DEV), logw=logw.to(DEV))
    assert same_bits(dict(prob=s.prob, brier=s.brier_map, sums=s.sums, hist=s.hist, hits=s.hits, status=s.status), r)
    with pytest.raises(ValueError, match="equal weights only"):
        s.reliability
    # equal weights on the device result: the decomposition is exact; into= adds in place
    e = v(k["y"].to(DEV), k["obs"].to(DEV), k["prec"].to(DEV))
    assert e.prob is None and e.brier_map is None and not e.weighted
    assert float((e.reliability - e.resolution + e.uncertainty - e.brier).abs().max()) <= 1e-12
    sums0, hist0 = e.sums.clone(), e.hist.clone()
    e2 = v(k["y"].to(DEV), k["obs"].to(DEV), k["prec"].to(DEV), into=e)
    assert e2.sums.data_ptr() == e.sums.data_ptr() and torch.equal(e2.hist, 2 * hist0) and same_bits(dict(sums=e2.sums), dict(sums=sums0 + sums0))
    assert float((e2.reliability - e2.resolution + e2.uncertainty - e2.brier).abs().max()) <= 1e-12
    # nothing is read back and nothing uploaded after the first call: the calls and every derived score run with synchronisation forbidden
    yd, od, pd, ld_ = k["y"].to(DEV), k["obs"].to(DEV), k["prec"].to(DEV), logw.to(DEV)
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        q = v(yd, od, pd, logw=ld_, maps=MAPS)
        q1 = v(yd, od, pd, into=v(yd, od, pd))
        kept = (q.brier, q.brier_skill, q.roc_area, q.roc(), q1.reliability, q1.resolution, q1.uncertainty, q1.reliability_curve(), q1.base_rate, q1.mean_probability)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert same_bits(dict(sums=q.sums, prob=q.prob), dict(sums=s.sums, prob=s.prob)) and len(kept) == 10


def test_field_class_composed_fp32_against_the_restatement():
    from sea_amd.ensemble import FieldThresholdVerification
    from tests.test_field_enkf_cpu import field_weights

    name, n, hist = "a", 5, 3
    k = class_inputs(name, n, hist, "fp32")
    P, F, C_ = k["P"], k["F"], k["C"]
    T = k["thr"].shape[0]
    w = field_weights((hist, P, F, C_), None, k["prec"], k["counts"])
    ref = restate_field_brier(k["Y"], k["obs"], w, None, n, k["thr"])
    g = TOL_F32 * float(k["Y"].abs().max())
    near = ((k["Y"].unsqueeze(0) - k["thr"].to(F64).view(T, 1, 1, F, 1)).abs() <= g).view(T, hist, n, P, F, C_).any(2)
    share = float(near.double().mean())
    print(f"brier composed fp32: excluded share {share:.4%} (band {g:.2e})")
    assert share <= 0.01
    v = FieldThresholdVerification(decoder(name, "fp32"), P, n, k["thr"], counts=k["counts"], fused=False)
    s = v(k["y"].to(DEV), k["obs"].to(DEV), k["prec"].to(DEV), maps=("prob",))
    keep = ~near
    prob = s.prob.cpu().to(F64)
    assert float((prob - ref["prob"])[keep].abs().max()) <= 1e-6
    assert torch.equal((prob * n).round().long()[keep & (w > 0).unsqueeze(0)], ref["m"][keep & (w > 0).unsqueeze(0)])
    assert torch.equal(s.sums[..., 0].cpu(), ref["sums"][..., 0]) and s.status.tolist() == [n] * hist
    assert FieldThresholdVerification(decoder(name, "bf16"), P, n, k["thr"])._fused_for(k["y"]) is False          # 135 rows: below the measured sizes
    assert FieldThresholdVerification(decoder(name, "bf16"), P, n, k["thr"])._fused_for(torch.zeros(4096 // P + 1, 1, 1)) is True
    assert FieldThresholdVerification(decoder(name, "fp32"), P, n, k["thr"])._fused_for(torch.zeros(4096, 1, 1)) is False


def test_sensor_class_scores_the_kalman_predictions_without_decoding_twice():
    from sea_amd.ensemble import SensorKalman, SensorSet, SensorThresholdVerification

    name, n, hist = "a", 8, 2
    k = class_inputs(name, n, hist, "bf16", seed=9)
    dec = decoder(name, "bf16")
    c = case(name)
    P, C_ = k["P"], k["C"]
    gen = torch.Generator().manual_seed(2)
    K = 37
    flat = [f for g in c["groups"] for f in g]
    patch, cell, field = torch.randint(0, P, (K,), generator=gen).tolist(), torch.randint(0, C_, (K,), generator=gen).tolist(), [flat[i] for i in torch.randint(0, len(flat), (K,), generator=gen).tolist()]
    s = SensorSet(dec, P, patch, cell, field)
    obs = torch.randn(hist, K, generator=gen)
    prec = 0.5 + torch.rand(hist, K, generator=gen)
    prec[torch.rand(hist, K, generator=gen) < 0.2] = 0.0
    logw = field_logw(n, hist, 8)
    y, obs_d, prec_d = k["y"].to(DEV), obs.to(DEV), prec.to(DEV)
    _, _, pred = SensorKalman(dec, P, n, s).transform(y, obs_d, prec_d)
    sv = SensorThresholdVerification(dec, P, n, s, k["thr"])
    assert sv._fused_for(y.device) and not sv._fused_for(torch.device("cpu"))
    for lw in (None, logw.to(DEV)):
        a, b = sv.from_predictions(pred, obs_d, prec_d, logw=lw, maps=MAPS), sv(y, obs_d, prec_d, logw=lw, maps=MAPS)
        assert same_bits(dict(prob=a.prob, brier=a.brier_map, sums=a.sums, hist=a.hist, hits=a.hits, status=a.status),
                         dict(prob=b.prob, brier=b.brier_map, sums=b.sums, hist=b.hist, hits=b.hits, status=b.status))
        assert tuple(a.brier.shape) == (hist, 2) and torch.equal(a.count.cpu(), (prec > 0).sum(1).to(F64).view(hist, 1).expand(hist, 2))
        ref = restate_brier(pred.cpu(), obs, prec, None if lw is None else logw, n, sv.thresholds)
        assert torch.equal(a.hist.cpu(), ref["hist"]) and torch.equal(a.hits.cpu(), ref["hits"]) and close(a.prob.cpu(), ref["prob"], 1e-6)[0]
        cpu = sv.from_predictions(pred.cpu(), obs, prec, logw=None if lw is None else logw)   # CPU tensors: the composed path
        assert torch.equal(cpu.hist, ref["hist"]) and close(cpu.sums[..., 1], a.sums[..., 1].cpu(), SUMS_TOL)[0]
    e = sv.from_predictions(pred, obs_d, prec_d)
    assert float((e.reliability - e.resolution + e.uncertainty - e.brier).abs().max()) <= 1e-12
    lw_d = logw.to(DEV)
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")                                              # nothing is read back, nothing uploaded: the tables went up with the set
    try:
        total = sv(y, obs_d, prec_d, into=sv.from_predictions(pred, obs_d, prec_d))
        w = sv.from_predictions(pred, obs_d, prec_d, logw=lw_d, maps=MAPS)
        kept = (total.brier, total.reliability, total.roc_area, w.brier_skill, w.roc())
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert torch.equal(total.hist, 2 * e.hist) and torch.equal(total.hits, 2 * e.hits) and len(kept) == 5
