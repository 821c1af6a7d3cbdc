"""Threshold scores of an ensemble (Brier score, reliability / resolution / uncertainty, reliability diagram, ROC), on the host: `restate_brier`, an fp64
restatement written from the definitions of include/sea_hip.h (sea_decode_member_brier, sea_ensemble_brier), against a brute-force Python loop; the
composed paths of sea_amd.ensemble against the restatement; ThresholdScores' derived properties (the decomposition is exact for equal weights; a perfect
forecast has ROC area 1, one whose bins all have the same hit fraction 0.5); the argument checks of the Python layers; the struct layouts and the argument
checks of the two entry points without a device."""
import ctypes as C
import functools

import pytest
import torch

from tests.test_field_enkf_cpu import as_sensors
from tests.test_field_verify_cpu import field_logw
from tests.test_sensor_cpu import host_case, make_decoder
from tests.test_verify_cpu import close

F64 = torch.float64


# ------------------------------------------------------------------------------------------------ the contract, in fp64
def restate_brier(pred, obs, prec, logw, n, thr):
    """The definitions, member by member: pred [B * n, K], obs [B, K], prec None / [K] / [B, K], logw None / [B * n], thr [T, K] (or [T, B, K]) — any
    float dtype, compared in float64 (exact for float32 inputs).  Returns float64 prob, brier [T, B, K] (0 at a dead reading and in an unscored history,
    NaN at a bad one), m int64 [T, B, K] (-1: in no bin), sums [B, T, 5], hist, hits int64 [B, T, n + 1], status int64 [B]."""
    B, K = obs.shape
    x, y = pred.to(F64).view(B, n, K), obs.to(F64)
    t = thr.to(F64)
    T = t.shape[0]
    t = t.view(T, 1, K).expand(T, B, K) if t.dim() == 2 else t
    lw = torch.zeros(B, n, dtype=F64) if logw is None else logw.to(F64).view(B, n)
    p_ = torch.ones(B, K, dtype=F64) if prec is None else prec.to(F64).expand(B, K)
    prob, brier = torch.zeros(T, B, K, dtype=F64), torch.zeros(T, B, K, dtype=F64)
    m_out = torch.full((T, B, K), -1, dtype=torch.int64)
    sums = torch.zeros(B, T, 5, dtype=F64)
    hist, hits = torch.zeros(B, T, n + 1, dtype=torch.int64), torch.zeros(B, T, n + 1, dtype=torch.int64)
    status = torch.zeros(B, dtype=torch.int64)
    for b in range(B):
        l = lw[b]
        if bool((torch.isnan(l) | (l == float("inf"))).any()) or not bool(torch.isfinite(l).any()):
            status[b] = -1
            continue
        alive = l != float("-inf")
        status[b] = int(alive.sum())
        mx = l.max()
        e = [float(torch.exp(l[j] - mx)) if bool(alive[j]) else 0.0 for j in range(n)]
        W = 0.0
        for j in range(n):
            W += e[j]
        live = p_[b] > 0
        fin = torch.isfinite(y[b]) & torch.isfinite(p_[b])
        for j in range(n):
            if bool(alive[j]):
                fin = fin & torch.isfinite(x[b, j])
        good, bad = live & fin, live & ~fin
        for q in range(T):
            num, m = torch.zeros(K, dtype=F64), torch.zeros(K, dtype=torch.int64)
            for j in range(n):
                if bool(alive[j]):
                    over = x[b, j] > t[q, b]
                    num = num + torch.where(over, torch.full((), e[j], dtype=F64), torch.zeros((), dtype=F64))
                    m = m + over.long()
            p = num / W
            o = y[b] > t[q, b]
            d2 = (p - o.to(F64)) ** 2
            prob[q, b] = torch.where(bad, torch.full((), float("nan"), dtype=F64), torch.where(good, p, torch.zeros((), dtype=F64)))
            brier[q, b] = torch.where(bad, torch.full((), float("nan"), dtype=F64), torch.where(good, d2, torch.zeros((), dtype=F64)))
            m_out[q, b] = torch.where(good, m, torch.full((), -1, dtype=torch.int64))
            sums[b, q] = torch.stack([good.sum().to(F64), d2[good].sum(), p[good].sum(), (good & o).sum().to(F64), bad.sum().to(F64)])
            hist[b, q] = torch.bincount(m[good], minlength=n + 1)
            hits[b, q] = torch.bincount(m[good & o], minlength=n + 1)
    return dict(prob=prob, brier=brier, m=m_out, sums=sums, hist=hist, hits=hits, status=status)


def restate_field_brier(Y, obs, w, logw, n, thr):
    """sea_decode_member_brier from the decoded members: restate_brier with every cell a sensor, field by field.  Y [B * n, P, F, C], obs [B, P, F, >= C],
    w [B, P, F, C] (0: dead), logw None / [B * n], thr [T, F].  Returns prob, brier, m [T, B, P, F, C], sums [B, F, T, 5], hist, hits [B, F, T, n + 1],
    status [B]."""
    Bm, P, F, C_ = Y.shape
    B, T = Bm // n, thr.shape[0]
    out = dict(prob=torch.zeros(T, B, P, F, C_, dtype=F64), brier=torch.zeros(T, B, P, F, C_, dtype=F64), m=torch.zeros(T, B, P, F, C_, dtype=torch.int64))
    sums = torch.zeros(B, F, T, 5, dtype=F64)
    hist, hits = torch.zeros(B, F, T, n + 1, dtype=torch.int64), torch.zeros(B, F, T, n + 1, dtype=torch.int64)
    for f in range(F):
        pred, o, p, _ = as_sensors(Y[:, :, f:f + 1], obs[:, :, f:f + 1], w[:, :, f:f + 1], None)
        r = restate_brier(pred, o, p, logw, n, thr[:, f:f + 1].expand(T, P * C_))
        for k in ("prob", "brier", "m"):
            out[k][:, :, :, f] = r[k].view(T, B, P, C_)
        sums[:, f], hist[:, f], hits[:, f], status = r["sums"], r["hist"], r["hits"], r["status"]
    return dict(out, sums=sums, hist=hist, hits=hits, status=status)


def scores_of(r, thr, weighted=False):
    from sea_amd.ensemble import ThresholdScores

    return ThresholdScores(prob=r.get("prob"), brier_map=r.get("brier"), sums=r["sums"], hist=r["hist"], hits=r["hits"], status=r["status"], thresholds=thr, weighted=weighted)


@functools.lru_cache(maxsize=None)
def sensor_case(n, B, K, T, with_prec, with_logw, seed=0):
    """Predictions, readings and per-sensor thresholds that are multiples of 0.25 (x == thr and y == thr occur), a tenth of the readings dead (obs NaN)."""
    g = torch.Generator().manual_seed(5000 + 64 * n + 8 * K + 4 * T + 2 * with_prec + with_logw + seed)
    pred = torch.randint(-8, 9, (B * n, K), generator=g).float() / 4
    obs = torch.randint(-8, 9, (B, K), generator=g).float() / 4
    thr = torch.randint(-6, 7, (T, K), generator=g).float() / 4
    prec = None
    if with_prec:
        prec = 0.25 + 1.75 * torch.rand(B, K, generator=g)
        miss = torch.rand(B, K, generator=g) < 0.1
        prec[miss] = 0.0
        obs[miss] = float("nan")
    return dict(pred=pred, obs=obs, thr=thr, prec=prec, logw=field_logw(n, B, 77 + n) if with_logw else None)


# ------------------------------------------------------------------------------------------------ the restatement against a brute-force loop
def test_restatement_against_a_python_loop():
    import math

    n, B, K, T = 3, 2, 19, 2
    t = sensor_case(n, B, K, T, True, True)
    pred, obs, thr, prec, logw = t["pred"].tolist(), t["obs"].tolist(), t["thr"].tolist(), t["prec"].tolist(), t["logw"].tolist()
    r = restate_brier(t["pred"], t["obs"], t["prec"], t["logw"], n, t["thr"])
    ties_x = ties_y = 0
    for b in range(B):
        lw = logw[b * n:(b + 1) * n]
        mx = max(lw)
        e = [0.0 if v == -math.inf else math.exp(v - mx) for v in lw]
        W = sum(e)
        assert int(r["status"][b]) == sum(v != -math.inf for v in lw)
        for q in range(T):
            cnt = sb = sp = so = 0.0
            hist, hits = [0] * (n + 1), [0] * (n + 1)
            for k in range(K):
                if not prec[b][k] > 0:
                    assert float(r["prob"][q, b, k]) == 0.0 and int(r["m"][q, b, k]) == -1
                    continue
                m = sum(1 for j in range(n) if e[j] > 0 and pred[b * n + j][k] > thr[q][k])
                p = sum(e[j] for j in range(n) if e[j] > 0 and pred[b * n + j][k] > thr[q][k]) / W
                o = 1.0 if obs[b][k] > thr[q][k] else 0.0
                ties_x += sum(pred[b * n + j][k] == thr[q][k] for j in range(n))
                ties_y += obs[b][k] == thr[q][k]
                cnt, sb, sp, so = cnt + 1, sb + (p - o) ** 2, sp + p, so + o
                hist[m] += 1
                hits[m] += int(o)
                assert abs(float(r["prob"][q, b, k]) - p) <= 1e-15 and abs(float(r["brier"][q, b, k]) - (p - o) ** 2) <= 1e-15 and int(r["m"][q, b, k]) == m
            assert r["hist"][b, q].tolist() == hist and r["hits"][b, q].tolist() == hits
            assert float(r["sums"][b, q, 0]) == cnt and float(r["sums"][b, q, 3]) == so and float(r["sums"][b, q, 4]) == 0.0
            assert abs(float(r["sums"][b, q, 1]) - sb) <= 1e-13 and abs(float(r["sums"][b, q, 2]) - sp) <= 1e-13
    assert ties_x > 0 and ties_y > 0                                                      # strictness is exercised


def test_restatement_special_cases():
    n = 4
    pred = torch.tensor([[0.5], [1.5], [float("inf")], [2.5]]).repeat(2, 1)              # history 1: the member with Inf is dead
    obs, thr = torch.tensor([[1.0], [1.0]]), torch.tensor([[1.0], [float("nan")]])
    logw = torch.zeros(2, n)
    logw[1, 2] = float("-inf")
    r = restate_brier(pred, obs, None, logw.reshape(-1), n, thr)
    assert bool(torch.isnan(r["prob"][:, 0]).all()) and r["sums"][0, :, 4].tolist() == [1.0, 1.0] and float(r["sums"][0, :, :4].abs().max()) == 0.0
    assert float(r["prob"][0, 1, 0]) == 2.0 / 3.0 and int(r["m"][0, 1, 0]) == 2 and r["status"].tolist() == [4, 3]
    assert float(r["prob"][1, 1, 0]) == 0.0 and int(r["m"][1, 1, 0]) == 0 and float(r["sums"][1, 1, 3]) == 0.0   # a NaN threshold: every comparison false
    logw[0, 0] = float("nan")
    r = restate_brier(pred, obs, None, logw.reshape(-1), n, thr)
    assert int(r["status"][0]) == -1 and float(r["sums"][0].abs().max()) == 0.0 and int(r["hist"][0].sum()) == 0 and float(r["prob"][:, 0].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ the composed paths
def check_against(got, ref, tol, tag, maps=("prob", "brier")):
    assert torch.equal(got["hist"], ref["hist"]) and torch.equal(got["hits"], ref["hits"]) and torch.equal(got["status"].long(), ref["status"]), tag
    for j in (0, 3, 4):
        assert torch.equal(got["sums"][..., j], ref["sums"][..., j]), tag + (j,)
    for j in (1, 2):
        ok, ratio = close(got["sums"][..., j], ref["sums"][..., j], tol)
        assert ok, tag + ("sums", j, ratio)
    for k in maps:
        ok, ratio = close(got[k], ref[k], tol)
        assert ok, tag + (k, ratio)


@pytest.mark.parametrize("n", [1, 2, 5, 130])
def test_composed_sensor_path_equals_the_restatement(n):
    from sea_amd.ensemble import _composed_brier

    for wp in (False, True):
        for wl in (False, True):
            t = sensor_case(n, 2, 23, 3, wp, wl)
            ref = restate_brier(t["pred"], t["obs"], t["prec"], t["logw"], n, t["thr"])
            got = _composed_brier(t["pred"], t["obs"], t["prec"], t["logw"], n, t["thr"], out_dtype=F64)
            check_against(got, ref, 1e-12, (n, wp, wl))
    # a live member's Inf marks its reading alone; invalid log-weights leave a history out
    t = sensor_case(n, 2, 23, 3, True, True)
    pred, logw = t["pred"].clone(), t["logw"].clone()
    pred[0, 5] = float("inf")
    logw[n] = float("nan")
    ref = restate_brier(pred, t["obs"], t["prec"], logw, n, t["thr"])
    check_against(_composed_brier(pred, t["obs"], t["prec"], logw, n, t["thr"], out_dtype=F64), ref, 1e-12, (n, "special"))
    assert int(ref["status"][1]) == -1


@pytest.mark.parametrize("n", [2, 5])
def test_composed_field_path_equals_the_restatement(n):
    from sea_amd.ensemble import _composed_field_brier

    B, P, F, C_, T = 2, 3, 2, 9, 3
    g = torch.Generator().manual_seed(31 + n)
    Y = torch.randint(-8, 9, (B * n, P, F, C_), generator=g).float() / 4
    obs = torch.randint(-8, 9, (B, P, F, C_ + 2), generator=g).float() / 4
    w = 0.25 + torch.rand(B, P, F, C_, generator=g)
    w[torch.rand(B, P, F, C_, generator=g) < 0.15] = 0.0
    w[:, 1, :, 4:] = 0.0                                                                  # counts
    thr = torch.randint(-4, 5, (T, F), generator=g).float() / 4
    for logw in (None, field_logw(n, B, 5)):
        ref = restate_field_brier(Y, obs, w, logw, n, thr)
        got = _composed_field_brier(Y, obs, w, logw, n, thr, out_dtype=F64)
        check_against(got, ref, 1e-12, (n, logw is None))
        assert set(_composed_field_brier(Y, obs, w, logw, n, thr, maps=("prob",))) == {"prob", "sums", "hist", "hits", "status"}


# ------------------------------------------------------------------------------------------------ the derived scores
def test_decomposition_is_exact_for_equal_weights_and_refused_for_weighted_results():
    from sea_amd.ensemble import _composed_brier

    n = 5
    t = sensor_case(n, 3, 200, 3, True, False, seed=3)
    s = scores_of(_composed_brier(t["pred"], t["obs"], t["prec"], None, n, t["thr"]), t["thr"])
    assert tuple(s.brier.shape) == (3, 3) and s.brier.dtype == F64
    assert float((s.reliability - s.resolution + s.uncertainty - s.brier).abs().max()) <= 1e-12
    assert float(s.brier.min()) > 0.0 and float(s.resolution.min()) > 0.0
    assert float((s.brier_skill - (1.0 - s.brier / s.uncertainty)).abs().max()) == 0.0
    assert torch.equal(s.count, s.hist.sum(-1).to(F64)) and float((s.base_rate * s.count - s.hits.sum(-1).to(F64)).abs().max()) <= 1e-12 * 200
    prob, freq, cells = s.reliability_curve()
    assert tuple(prob.shape) == (3, 3, n + 1) and prob[0, 0].tolist() == [k / n for k in range(n + 1)] and torch.equal(cells, s.hist.to(F64))
    assert float(((prob * cells).sum(-1) / s.count - s.mean_probability).abs().max()) <= 1e-12   # p = m / L in every bin
    w = scores_of(_composed_brier(t["pred"], t["obs"], t["prec"], field_logw(n, 3, 1), n, t["thr"]), t["thr"], weighted=True)
    for fn in (lambda: w.reliability, lambda: w.resolution, w.reliability_curve):
        with pytest.raises(ValueError, match="equal weights only"):
            fn()
    assert bool(torch.isfinite(w.brier).all()) and bool(torch.isfinite(w.brier_skill).all()) and bool(torch.isfinite(w.roc_area).all())
    # a field without a live good reading: NaN
    e = scores_of(_composed_brier(t["pred"], t["obs"], torch.zeros(200), None, n, t["thr"]), t["thr"])
    assert bool(torch.isnan(e.brier).all()) and bool(torch.isnan(e.reliability).all()) and bool(torch.isnan(e.roc_area).all())


def test_roc_of_a_perfect_and_of_an_independent_forecast():
    from sea_amd.ensemble import _composed_brier

    # perfect: every member is above the threshold where the reading is, and below where it is not
    n, K = 4, 10
    up = torch.arange(K) % 3 == 0
    obs = torch.where(up, torch.tensor(1.0), torch.tensor(-1.0)).view(1, K)
    pred = (obs + 0.25 * torch.arange(n).view(n, 1).float() * obs.sign())
    s = scores_of(_composed_brier(pred, obs, None, None, n, torch.zeros(1, K)), torch.zeros(1, K))
    assert float(s.roc_area) == 1.0 and float(s.brier) == 0.0 and float(s.brier_skill) == 1.0
    hr, far = s.roc()
    assert hr[0, 0].tolist() == [1.0] * (n + 1) + [0.0] and far[0, 0].tolist() == [1.0] + [0.0] * (n + 1)
    # independent BY CONSTRUCTION: two members, bins m = 0, 1, 2, and in every bin one reading of four is above the threshold
    members = torch.tensor([[-1.0, -1.0], [-1.0, 1.0], [1.0, 1.0]])                       # the three bins
    pred = members.repeat_interleave(4, 0).t().contiguous()                               # [2, 12]
    obs = torch.tensor([1.0, -1.0, -1.0, -1.0]).repeat(3).view(1, 12)
    s = scores_of(_composed_brier(pred, obs, None, None, 2, torch.zeros(1, 12)), torch.zeros(1, 12))
    assert s.hist[0, 0].tolist() == [4, 4, 4] and s.hits[0, 0].tolist() == [1, 1, 1]
    assert abs(float(s.roc_area) - 0.5) <= 1e-15 and abs(float(s.resolution)) <= 1e-15
    hr, far = s.roc()
    assert torch.equal(hr, far) and hr[0, 0].tolist() == [1.0, 2.0 / 3.0, 1.0 / 3.0, 0.0]


# ------------------------------------------------------------------------------------------------ refusals of the Python layers
def test_python_layers_refuse_before_a_device_is_touched():
    from sea_amd import _native as N
    from sea_amd import ops
    from sea_amd.ensemble import FieldThresholdVerification, SensorSet, SensorThresholdVerification, ThresholdScores
    from sea_amd.utils.train_utils import FieldThresholdVerification as F2, SensorThresholdVerification as S2

    assert F2 is FieldThresholdVerification and S2 is SensorThresholdVerification and N.BRIER_MAX_N == 128 and N.BRIER_MAX_T == 8 and N.BRIER_SUMS == 5
    c = host_case("a")
    dec = make_decoder("a").set_compute_dtype("bf16")
    P, D_, G, C_ = c["P"], c["D"], len(c["groups"]), c["n_inp"]
    F = sum(len(g) for g in c["groups"])
    for members in (0, -1, True, 2.0):
        with pytest.raises(ValueError):
            FieldThresholdVerification(dec, P, members, [0.5])
    for thr in ([], [float("nan")], [float("inf")], [0.0] * 9, [[0.0] * (F + 1)], torch.zeros(2, 2, 2), torch.zeros(2, dtype=torch.int64), "half", None):
        with pytest.raises(ValueError):
            FieldThresholdVerification(dec, P, 2, thr)
        with pytest.raises(ValueError):
            SensorThresholdVerification(dec, P, 2, SensorSet(dec, P, [0, 1, 8], [3, 4, 11], [0, 2, 1]), thr)
    for kw in (dict(layout="PBFC"), dict(fused="yes"), dict(n_patches=0)):
        args = dict(decoder=dec, n_patches=P, members=2, thresholds=[0.5])
        args.update(kw)
        with pytest.raises(ValueError):
            FieldThresholdVerification(**args)
    with pytest.raises(ValueError, match="up to 128"):
        FieldThresholdVerification(dec, P, 129, [0.5], fused=True)
    FieldThresholdVerification(dec, P, 129, [0.5])                                          # the composed path carries any member count
    v = FieldThresholdVerification(dec, P, 2, [[0.5] * F, [1.0] * F], fused=True)
    assert tuple(v.thresholds.shape) == (2, F) and tuple(FieldThresholdVerification(dec, P, 2, [0.25, 0.5, 0.75]).thresholds.shape) == (3, F)
    y, obs = torch.zeros(4, G, P * D_), torch.zeros(2, P, F, C_)
    for yy, oo, pp in ((torch.zeros(3, G, P * D_), obs, None), (torch.zeros(4, G, P * D_ + 1), obs, None), (y, torch.zeros(2, P + 1, F, C_), None), (y, obs.double(), None),
                       (y, obs[0], None), (y, obs, torch.ones(2, P, F, C_ + 1)), (y, obs, -torch.ones(2, P, F, C_)), (y, obs, torch.ones(2, P, F, C_).double())):
        with pytest.raises(ValueError):
            v(yy, oo, pp)
    z64, i64 = torch.zeros(2, F, 2, 5, dtype=F64), torch.zeros(2, F, 2, 3, dtype=torch.int64)
    good_into = ThresholdScores(None, None, z64, i64, i64.clone(), torch.zeros(2, dtype=torch.int32), v.thresholds)
    for kw in (dict(logw=torch.zeros(3)), dict(logw=torch.zeros(4, dtype=torch.int64)), dict(logw=torch.zeros(4, 1)), dict(maps=("prob", "prob")), dict(maps=("crps",)),
               dict(into=dict(sums=z64, hist=i64, hits=i64)), dict(into=ThresholdScores(None, None, z64.float(), i64, i64, good_into.status, v.thresholds)),
               dict(into=ThresholdScores(None, None, z64, i64, torch.zeros(2, F, 2, 4, dtype=torch.int64), good_into.status, v.thresholds)),
               dict(into=ThresholdScores(None, None, torch.zeros(2, F, 3, 5, dtype=F64), i64, i64, good_into.status, v.thresholds))):
        with pytest.raises(ValueError):
            v(y, obs, **kw)
    with pytest.raises(RuntimeError, match="MI355X"):
        v(y, obs, logw=torch.zeros(2, 2), into=good_into, maps=("brier",))
    # Decode.member_brier
    z, thr = torch.zeros(4, P, G, D_), torch.zeros(2, F)
    for kw in (dict(members=0), dict(members=3), dict(obs=torch.zeros(2, P, F, C_ - 1)), dict(obs=obs.double()), dict(precision=torch.ones(2, P, F, C_ + 4)),
               dict(field_precision=torch.ones(F + 1)), dict(z=torch.zeros(4, P, G + 1, D_)), dict(logw=torch.zeros(5)), dict(logw=torch.zeros(4, dtype=F64)),
               dict(maps=("prob", "nope")), dict(into=dict(sums=z64, hist=i64)), dict(thresholds=torch.zeros(9, F)), dict(thresholds=torch.zeros(2, F + 1)),
               dict(thresholds=torch.full((2, F), float("nan"))), dict(thresholds=[0.5]), dict(thresholds=thr.double())):
        args = dict(z=z, obs=obs, members=2, thresholds=thr)
        args.update(kw)
        with pytest.raises(ValueError):
            dec.member_brier(**args)
    with pytest.raises(ValueError, match="bf16 only"):
        make_decoder("a").member_brier(z, obs, 2, thr, fused=True)
    with pytest.raises(ValueError, match="up to 128"):
        dec.member_brier(torch.zeros(129, P, G, D_), obs[:1], 129, thr, fused=True)
    with pytest.raises(RuntimeError, match="MI355X"):
        dec.member_brier(z, obs, 2, thr, fused=True)
    # the sensor class: its checks, and CPU tensors through the composed path
    s = SensorSet(dec, P, [0, 1, 8], [3, 4, 11], [0, 2, 1])
    with pytest.raises(ValueError):
        SensorThresholdVerification(dec, P, 2, "sensors", [0.5])
    with pytest.raises(ValueError, match="up to 128"):
        SensorThresholdVerification(dec, P, 129, s, [0.5], fused=True)
    sv = SensorThresholdVerification(dec, P, 2, s, [[0.0, 1.0, 2.0][:F], [3.0, 4.0, 5.0][:F]])
    assert sv.thresholds.tolist() == [[0.0, 2.0, 1.0], [3.0, 5.0, 4.0]]                     # [T, K] through the set's field index
    pred, ob = torch.randn(4, 3), torch.randn(2, 3)
    for pp, oo, kw in ((pred[:3], ob, {}), (pred.double(), ob, {}), (pred[:, :2], ob, {}), (pred, ob[:1], {}), (pred, ob.double(), {}), (pred, ob, dict(precision=-torch.ones(3))),
                       (pred, ob, dict(logw=torch.zeros(3))), (pred, ob, dict(maps=("rank",))), (pred, ob, dict(into=good_into))):
        with pytest.raises(ValueError):
            sv.from_predictions(pp, oo, **kw)
    for yy in (torch.zeros(3, G, P * D_), torch.zeros(4, G, P * D_ + 1)):
        with pytest.raises(ValueError):
            sv(yy, ob)
    r = sv.from_predictions(pred, ob, logw=torch.zeros(2, 2), maps=("prob",))
    ref = restate_brier(pred, ob, None, torch.zeros(4), 2, sv.thresholds)
    check_against(dict(prob=r.prob, sums=r.sums, hist=r.hist, hits=r.hits, status=r.status), ref, 1e-6, ("cpu",), maps=("prob",))
    assert r.brier_map is None and r.weighted and tuple(r.brier.shape) == (2, 2)
    again = sv.from_predictions(pred, ob, into=r)
    assert again.sums is r.sums and again.weighted and int(again.hist.sum()) == 2 * 2 * 3 * 2
    with pytest.raises(RuntimeError, match="MI355X"):
        SensorThresholdVerification(dec, P, 2, s, [0.5], fused=True).from_predictions(pred, ob)
    # ops.decode_member_brier / ops.ensemble_brier: their own tables of refusals on host tensors, then the device
    S, Cp = 40, 64
    M = 2 * 2 * P
    grp = [dict(H=torch.zeros(M, S, dtype=torch.bfloat16), W2=torch.zeros(F * Cp, S, dtype=torch.bfloat16), bias=torch.zeros(F * Cp))]
    o3, th = torch.zeros(2 * P, F, 40), torch.zeros(2, F)
    base = dict(groups=grp, obs=o3, C_=40, Cp=Cp, n_patches=P, members=2, thr=th)
    for kw in (dict(members=0), dict(members=129), dict(members=3), dict(Cp=48), dict(C_=65), dict(obs=o3.double()), dict(obs=o3[:, :, :39]), dict(prec=o3[:-1]),
               dict(prec_field=torch.ones(F + 1)), dict(counts=torch.zeros(P, dtype=torch.int64)), dict(logw=torch.zeros(5)), dict(maps=("prob", "median")),
               dict(thr=torch.zeros(9, F)), dict(thr=torch.zeros(2, F + 1)), dict(thr=th.double()), dict(thr=torch.full((2, F), float("inf"))),
               dict(out=dict(prob=torch.zeros(2, 2, P, F, 39))), dict(out=dict(prob=torch.zeros(2, 2, P, F, 40), brier=torch.zeros(2, 2, P, F, 48))),
               dict(out=dict(sums=torch.zeros(2, F, 2, 5))), dict(out=dict(crps=torch.zeros(2))), dict(accumulate=True),
               dict(accumulate=True, out=dict(sums=torch.zeros(2, F, 2, 5, dtype=F64), hist=torch.zeros(2, F, 2, 3, dtype=torch.int64))), dict(dtype=torch.float32), dict(groups=[])):
        args = dict(base)
        args.update(kw)
        with pytest.raises(ValueError):
            ops.decode_member_brier(**args)
    with pytest.raises(RuntimeError, match="MI355X"):
        ops.decode_member_brier(**base)
    base = dict(pred=torch.zeros(4, 3), obs=torch.zeros(2, 3), members=2, thr=torch.zeros(2, 3))
    for kw in (dict(members=0), dict(members=129), dict(pred=torch.zeros(5, 3)), dict(obs=torch.zeros(2, 3).double()), dict(thr=torch.zeros(2, 4)), dict(thr=torch.zeros(9, 3)),
               dict(thr=torch.full((1, 3), float("nan"))), dict(prec=torch.ones(4)), dict(prec=-torch.ones(3)), dict(logw=torch.zeros(3)), dict(maps=("pit",)),
               dict(out=dict(prob=torch.zeros(2, 2, 2))), dict(out=dict(hits=torch.zeros(2, 2, 3))), dict(accumulate=True)):
        args = dict(base)
        args.update(kw)
        with pytest.raises(ValueError):
            ops.ensemble_brier(**args)
    with pytest.raises(RuntimeError, match="MI355X"):
        ops.ensemble_brier(**base)


# ------------------------------------------------------------------------------------------------ the entry points without a device
@pytest.fixture(scope="module")
def lib():
    from sea_amd import build, _native

    build.build(verbose=False)
    return _native.lib()


def _field_tables(n_groups=2):
    """A well-formed sea_decode_member_brier table over made-up (aligned, never dereferenced) addresses: 4 members of 2 histories, 9 patches, 3 fields, 2 thresholds."""
    from sea_amd import _native as N

    arr, p = (N.SeaDecodeMseGroup * n_groups)(), N.SeaDecodeMemberBrier()
    for g in range(n_groups):
        arr[g].H, arr[g].W2, arr[g].bias = 0x100000 + 0x10000 * g, 0x200000 + 0x10000 * g, 0x300000 + 0x10000 * g
        arr[g].ldh, arr[g].ldw, arr[g].n_fields, arr[g].field0 = 40, 40, 2 if g == 0 else 1, 0 if g == 0 else 2
    p.obs, p.prec_field, p.prec, p.counts, p.logw, p.thr = 0x400000, 0x410000, 0x420000, 0x430000, 0x440000, 0x450000
    p.prob, p.brier = 0x500000, 0x510000
    p.sums, p.hist, p.hits, p.status, p.work = 0x600000, 0x610000, 0x630000, 0x620000, 0x700000
    p.ld_row, p.ld_field, p.ld_prow, p.ld_pfield, p.ld_out, p.ld_map = 3 * 24, 24, 3 * 24, 24, 21, 2 * 9 * 3 * 21
    p.M, p.S, p.C, p.Cp, p.P, p.members, p.n_fields_total, p.n_thr, p.accumulate = 2 * 4 * 9, 40, 21, 32, 9, 4, 3, 2, 0
    p.work_bytes = 2 * 9 * 3 * (10 + 10) * 8
    return arr, p


def _sensor_table():
    """A well-formed sea_ensemble_brier table: 2 histories of 4 members, 21 sensors, 3 thresholds."""
    from sea_amd import _native as N

    p = N.SeaEnsembleBrier()
    p.pred, p.obs, p.prec, p.logw, p.thr, p.prob, p.brier = 0x100000, 0x110000, 0x120000, 0x130000, 0x140000, 0x150000, 0x160000
    p.sums, p.hist, p.hits, p.status, p.work = 0x200000, 0x210000, 0x220000, 0x230000, 0x300000
    p.ld_pred, p.ld_obs, p.ld_prec, p.ld_thr, p.ld_out, p.ld_map = 24, 24, 24, 24, 21, 42
    p.B, p.N, p.K, p.n_thr, p.accumulate = 2, 4, 21, 3, 0
    p.work_bytes = 2 * 2 * (15 + 15) * 8
    return p


def test_symbols_struct_layouts_and_workspaces(lib):
    from sea_amd import _native as N

    for name in ("sea_decode_member_brier", "sea_decode_member_brier_ws_bytes", "sea_ensemble_brier", "sea_ensemble_brier_ws_bytes"):
        assert hasattr(lib, name) and name in N.EXPORTED_SYMBOLS
    T, E = N.SeaDecodeMemberBrier, N.SeaEnsembleBrier
    assert C.sizeof(T) == 200 and C.sizeof(E) == 176                                       # include/sea_hip.h states them
    assert T.thr.offset == 40 and T.hits.offset == 80 and T.work.offset == 96 and T.ld_row.offset == 104 and T.ld_map.offset == 144 and T.M.offset == 160
    assert T.n_thr.offset == 188 and T.accumulate.offset == 192 and E.thr.offset == 32 and E.work.offset == 88 and E.ld_thr.offset == 120 and E.B.offset == 152
    assert lib.sea_abi_version() == 8 and len(N.ABI_STRUCTS) == 33 and N.ABI_STRUCTS[-1] is N.SeaKvFork and T not in N.ABI_STRUCTS and E not in N.ABI_STRUCTS
    # per (history, patch, chunk of 512 columns, field): 5 T sums and 2 T (members + 1) int32 bins — sized by the call's T and members
    assert lib.sea_decode_member_brier_ws_bytes(2, 9, 3, 4, 32, 2) == 2 * 9 * 3 * 20 * 8 and lib.sea_decode_member_brier_ws_bytes(1, 1, 1, 128, 512, 8) == (40 + 8 * 129) * 8
    assert lib.sea_decode_member_brier_ws_bytes(1, 1, 1, 1, 544, 1) == 2 * (5 + 2) * 8 and lib.sea_ensemble_brier_ws_bytes(2, 4, 21, 3) == 2 * 2 * 30 * 8
    for bad in ((0, 9, 3, 4, 32, 1), (65536, 9, 3, 4, 32, 1), (2, 0, 3, 4, 32, 1), (2, 9, 0, 4, 32, 1), (2, 9, 3, 0, 32, 1), (2, 9, 3, 129, 32, 1), (2, 9, 3, 4, 40, 1),
                (2, 9, 3, 4, 32, 0), (2, 9, 3, 4, 32, 9)):
        assert lib.sea_decode_member_brier_ws_bytes(*bad) == -1, bad
    for bad in ((0, 4, 21, 1), (2, 0, 21, 1), (2, 129, 21, 1), (2, 4, 0, 1), (2, 4, 21, 0), (2, 4, 21, 9)):
        assert lib.sea_ensemble_brier_ws_bytes(*bad) == -1, bad
    # the library reads the fields where the binding writes them: its messages quote the values back
    for field, value, msg in (("members", 0, b"members=0"), ("ld_pfield", 20, b"ld_pfield=20 must cover C=21"), ("M", 71, b"M=71 is not a multiple of P * members = 9 * 4"),
                              ("ld_out", 20, b"ld_out=20 must cover C=21"), ("n_thr", 9, b"n_thr=9 outside 1..8"), ("accumulate", 3, b"accumulate=3"),
                              ("work_bytes", 8639, b"work_bytes=8639 below the 8640")):
        arr, p = _field_tables()
        setattr(p, field, value)
        assert lib.sea_decode_member_brier(arr, 2, C.byref(p), N.SEA_BF16, None) == -1 and msg in lib.sea_last_error(), (field, lib.sea_last_error())
    for field, value, msg in (("N", 0, b"N=0"), ("ld_thr", 20, b"ld_thr=20"), ("n_thr", 0, b"n_thr=0"), ("work_bytes", 959, b"work_bytes=959 below the 960")):
        p = _sensor_table()
        setattr(p, field, value)
        assert lib.sea_ensemble_brier(C.byref(p), None) == -1 and msg in lib.sea_last_error(), (field, lib.sea_last_error())


FIELD_BREAKS = {"null obs": ("obs", None), "null thr": ("thr", None), "null sums": ("sums", None), "null hist": ("hist", None), "null hits": ("hits", None),
                "null status": ("status", None), "null work": ("work", None), "misaligned obs": ("obs", 0x400002), "misaligned prec": ("prec", 0x420001),
                "misaligned prec_field": ("prec_field", 0x410003), "misaligned counts": ("counts", 0x430002), "misaligned logw": ("logw", 0x440001),
                "misaligned thr": ("thr", 0x450002), "misaligned prob": ("prob", 0x500002), "misaligned brier": ("brier", 0x510001), "misaligned sums": ("sums", 0x600004),
                "misaligned hist": ("hist", 0x610004), "misaligned hits": ("hits", 0x630004), "misaligned status": ("status", 0x620002), "misaligned work": ("work", 0x700004),
                "members = 0": ("members", 0), "M = 0": ("M", 0), "M not a multiple": ("M", 70), "S odd": ("S", 36), "Cp = 40": ("Cp", 40), "C above Cp": ("C", 33),
                "C = 0": ("C", 0), "P = 0": ("P", 0), "ld_field short": ("ld_field", 20), "ld_row negative": ("ld_row", -1), "ld_pfield short": ("ld_pfield", 20),
                "ld_out short": ("ld_out", 20), "ld_map short": ("ld_map", 2 * 9 * 3 * 21 - 1), "fields": ("n_fields_total", 4), "n_thr = 0": ("n_thr", 0),
                "n_thr = 9": ("n_thr", 9), "accumulate = -1": ("accumulate", -1), "workspace one byte short": ("work_bytes", 2 * 9 * 3 * 20 * 8 - 1)}


@pytest.mark.parametrize("what", sorted(FIELD_BREAKS) + ["bad dtype", "no groups", "too many groups", "group null", "group misaligned", "group overlap", "group missing", "ldh short"])
def test_member_brier_refuses_bad_arguments_without_a_device(lib, what):
    from sea_amd import _native as N

    arr, p = _field_tables()
    dt, ng = N.SEA_BF16, 2
    if what in FIELD_BREAKS:
        setattr(p, *FIELD_BREAKS[what])
    elif what == "bad dtype":
        dt = 5
    elif what == "no groups":
        ng = 0
    elif what == "too many groups":
        ng = N.DECODE_MSE_MAX_GROUPS + 1
    elif what == "group null":
        arr[1].W2 = None
    elif what == "group misaligned":
        arr[0].bias = 0x300008
    elif what == "group overlap":
        arr[1].field0 = 1
    elif what == "group missing":
        ng = 1
    else:
        arr[0].ldh = 32
    assert lib.sea_decode_member_brier(arr, ng, C.byref(p), dt, None) == -1, what
    assert b"sea_decode_member_brier" in lib.sea_last_error()


SENSOR_BREAKS = {"null pred": ("pred", None), "null obs": ("obs", None), "null thr": ("thr", None), "null sums": ("sums", None), "null hist": ("hist", None),
                 "null hits": ("hits", None), "null status": ("status", None), "null work": ("work", None), "misaligned pred": ("pred", 0x100002),
                 "misaligned thr": ("thr", 0x140001), "misaligned prob": ("prob", 0x150002), "misaligned hits": ("hits", 0x220004), "misaligned work": ("work", 0x300004),
                 "B = 0": ("B", 0), "B too large": ("B", 65536), "N = 0": ("N", 0), "K = 0": ("K", 0), "n_thr = 0": ("n_thr", 0), "n_thr = 9": ("n_thr", 9),
                 "ld_pred short": ("ld_pred", 20), "ld_obs short": ("ld_obs", 20), "ld_thr short": ("ld_thr", 20), "ld_prec short": ("ld_prec", 20),
                 "ld_out short": ("ld_out", 20), "ld_map short": ("ld_map", 41), "accumulate = 2": ("accumulate", 2), "workspace one byte short": ("work_bytes", 959)}


@pytest.mark.parametrize("what", sorted(SENSOR_BREAKS))
def test_ensemble_brier_refuses_bad_arguments_without_a_device(lib, what):
    p = _sensor_table()
    setattr(p, *SENSOR_BREAKS[what])
    assert lib.sea_ensemble_brier(C.byref(p), None) == -1, what
    assert b"sea_ensemble_brier" in lib.sea_last_error()


def test_unsupported_forms_and_null_tables(lib):
    from sea_amd import _native as N

    arr, p = _field_tables()
    assert lib.sea_decode_member_brier(arr, 2, C.byref(p), N.SEA_F32, None) == -3 and b"sea_decode_member_brier" in lib.sea_last_error()
    arr, p = _field_tables()
    p.S = 648
    for g in range(2):
        arr[g].ldh = arr[g].ldw = 648
    assert lib.sea_decode_member_brier(arr, 2, C.byref(p), N.SEA_BF16, None) == -3 and b"S=648" in lib.sea_last_error()
    arr, p = _field_tables()
    p.members, p.M = 129, 2 * 129 * 9
    assert lib.sea_decode_member_brier(arr, 2, C.byref(p), N.SEA_BF16, None) == -3 and b"members=129" in lib.sea_last_error()
    assert lib.sea_decode_member_brier(None, 2, C.byref(p), N.SEA_BF16, None) == -1 and lib.sea_decode_member_brier(arr, 2, None, N.SEA_BF16, None) == -1
    # prec_field, prec, counts, logw and both maps may be NULL: such a table passes the pointer checks and fails only at the check this test breaks
    arr, p = _field_tables()
    p.prec_field = p.prec = p.counts = p.logw = p.prob = p.brier = None
    p.ld_out, p.ld_map, p.ld_pfield, p.work_bytes = 0, 0, 0, 7
    assert lib.sea_decode_member_brier(arr, 2, C.byref(p), N.SEA_BF16, None) == -1 and b"work_bytes=7" in lib.sea_last_error()
    p = _sensor_table()
    p.N = 129
    assert lib.sea_ensemble_brier(C.byref(p), None) == -3 and b"N=129" in lib.sea_last_error()
    assert lib.sea_ensemble_brier(None, None) == -1 and b"sea_ensemble_brier" in lib.sea_last_error()
    p = _sensor_table()
    p.prec = p.logw = p.prob = p.brier = None
    p.ld_out, p.ld_map, p.ld_prec, p.work_bytes = 0, 0, 0, 7
    assert lib.sea_ensemble_brier(C.byref(p), None) == -1 and b"work_bytes=7" in lib.sea_last_error()
