"""Verification of an ensemble at the sensors (sea_ensemble_verify, ops.ensemble_verify, SensorVerification, EnsembleScores) without a GPU: the formulas
of include/sea_hip.h restated in fp64 from the definitions (`restate_verify`: the double sum over member pairs, no sort) and held against closed forms;
the composed path (fused=False, fp64 torch ops with a sort and a cumulative sum) held against the restatement; accumulation over calls; the entry
point's argument checks through the built library; the refusals of the Python layers.

Every input of tests/test_verify_gpu.py is generated here (`verify_case`), once, and never modified; `reference` computes each restatement once.
Predictions and readings are multiples of 0.25, so ties between members and between a member and the reading really occur (asserted)."""
import ctypes as C
import functools

import pytest
import torch

from tests.test_sensor_cpu import host_case, make_decoder

F64 = torch.float64
FLOATS = ("mean", "spread", "crps", "pit")
V_N, V_K, V_B = (1, 2, 5, 33, 64, 65, 128, 200), (1, 63, 65, 257), (1, 3)
DOMINANT = 6.0   # the log-weight lead of the dominant member: it keeps 1 - sum w^2 >= 1e-2, so the cancellation in it costs two digits of sixteen


# ------------------------------------------------------------------------------------------------ the contract, in fp64
def restate_verify(pred, obs, prec, logw, n, unbiased):
    """include/sea_hip.h, sea_ensemble_verify, in fp64, history by history, from the definitions: the member-pair term of the CRPS is the double sum.
    pred [B * n, K], obs [B, K], prec None / [K] / [B, K], logw None / [B * n].  Returns a dict of float64 mean, spread, crps, pit [B, K], int64 rank
    [B, K], float64 sums [B, 8], int64 hist [B, n + 1], int64 status [B]."""
    B, K = obs.shape
    out = {k: torch.zeros(B, K, dtype=F64) for k in FLOATS}
    rank = torch.full((B, K), -1, dtype=torch.int64)
    sums, hist, status = torch.zeros(B, 8, dtype=F64), torch.zeros(B, n + 1, dtype=torch.int64), torch.zeros(B, dtype=torch.int64)
    for b in range(B):
        lw = torch.zeros(n, dtype=F64) if logw is None else logw[b * n:(b + 1) * n].to(F64)
        if bool(torch.isnan(lw).any()) or bool((lw == float("inf")).any()) or not bool(torch.isfinite(lw).any()):
            status[b] = -1
            continue
        alive = lw != float("-inf")
        status[b] = int(alive.sum())
        e = (lw[alive] - lw[alive].max()).exp()
        w = e / e.sum()                                               # [L]
        c = 1.0 - float((w * w).sum()) if unbiased else 1.0
        x = pred[b * n:(b + 1) * n].to(F64)[alive]                    # [L, K]: a dead member never enters
        y = obs[b].to(F64)
        p = torch.ones(K, dtype=F64) if prec is None else (prec if prec.dim() == 1 else prec[b]).to(F64)
        live = p > 0
        good = live & torch.isfinite(y) & torch.isfinite(p) & torch.isfinite(x).all(0)
        bad = live & ~good
        for k in FLOATS:
            out[k][b, bad] = float("nan")
        rank[b, bad] = -2
        sums[b, 6] = int(bad.sum())
        if not bool(good.any()):
            continue
        xg, yg, pg = x[:, good], y[good], p[good]
        wc = w.unsqueeze(1)
        mean = (wc * xg).sum(0)
        var = (wc * (xg - mean) ** 2).sum(0)
        sp2 = var / c if c > 0 else torch.zeros_like(var)
        pairs = (w.view(-1, 1, 1) * w.view(1, -1, 1) * (xg.unsqueeze(1) - xg.unsqueeze(0)).abs()).sum((0, 1))
        crps = (wc * (xg - yg).abs()).sum(0) - (pairs / (2.0 * c) if c > 0 else torch.zeros_like(pairs))
        pit = (wc * (xg < yg)).sum(0) + 0.5 * (wc * (xg == yg)).sum(0)
        rk = (xg < yg).sum(0)
        out["mean"][b, good], out["spread"][b, good], out["crps"][b, good], out["pit"][b, good] = mean, sp2.sqrt(), crps, pit
        rank[b, good] = rk
        err = yg - mean
        sums[b, 0], sums[b, 1], sums[b, 2], sums[b, 3] = int(good.sum()), crps.sum(), (err * err).sum(), sp2.sum()
        sums[b, 4], sums[b, 5], sums[b, 7] = (err * err / (sp2 + 1.0 / pg)).sum(), (mean - yg).sum(), (1.0 / pg).sum()
        hist[b] = torch.bincount(rk, minlength=n + 1)
    return dict(out, rank=rank, sums=sums, hist=hist, status=status)


# ------------------------------------------------------------------------------------------------ the inputs of the GPU test
@functools.lru_cache(maxsize=None)
def verify_case(n, K, B, with_prec, with_logw):
    """Normal predictions and readings rounded to multiples of 0.25 (float32); with_prec: precisions in [0.25, 2], a tenth of the readings dead
    (precision 0, the reading NaN); with_logw: normal log-weights, in history b member b % n leads by DOMINANT and, from two members on, member
    (b + 1) % n is dead (-inf): two members leave ONE live member, the c = 0 selects.  Returns dict(pred, obs, prec, logw, unbiased)."""
    g = torch.Generator().manual_seed(200000 + 1000 * n + 10 * K + 3 * B + (500 if with_prec else 0) + (250 if with_logw else 0))
    pred, obs = (torch.randn(B * n, K, generator=g) * 4).round() / 4, (torch.randn(B, K, generator=g) * 4).round() / 4
    prec = None
    if with_prec:
        prec = 0.25 + 1.75 * torch.rand(B, K, generator=g)
        miss = torch.rand(B, K, generator=g) < 0.1
        prec[miss] = 0.0
        obs[miss] = float("nan")
    logw = None
    if with_logw:
        logw = torch.randn(B, n, generator=g)
        for b in range(B):
            logw[b, b % n] = float(logw[b].max()) + DOMINANT
            if n >= 2:
                logw[b, (b + 1) % n] = float("-inf")
        logw = logw.reshape(-1).contiguous()
    return dict(pred=pred, obs=obs, prec=prec, logw=logw, unbiased=bool((n + K + B) % 2))


def verify_cases(n):
    return [(K, B, wp, wl) for K in V_K for B in V_B for wp in (False, True) for wl in (False, True)]


@functools.lru_cache(maxsize=None)
def reference(n, K, B, with_prec, with_logw):
    t = verify_case(n, K, B, with_prec, with_logw)
    return restate_verify(t["pred"], t["obs"], t["prec"], t["logw"], n, t["unbiased"])


@functools.lru_cache(maxsize=None)
def _sensor_set(K):
    from sea_amd.ensemble import SensorSet

    c = host_case("a")
    dec = make_decoder("a")
    fields = [f for g in c["groups"] for f in g]
    return dec, SensorSet(dec, c["P"], [k % c["P"] for k in range(K)], [(7 * k) % c["n_inp"] for k in range(K)], [fields[k % len(fields)] for k in range(K)])


def verifier(n, K, fused=False, unbiased=True, sigma=None):
    """A SensorVerification over K made-up sensors of shape a's decoder (from_predictions never decodes)."""
    from sea_amd.ensemble import SensorVerification

    dec, s = _sensor_set(K)
    return SensorVerification(dec, host_case("a")["P"], n, s, sigma=sigma, unbiased=unbiased, fused=fused)


def close(got, ref, tol):
    """max |got - ref| <= tol * max(1, max |ref|), NaN where and only where the reference has it."""
    got, ref = got.to(F64), ref.to(F64)
    nan = torch.isnan(ref)
    if not torch.equal(torch.isnan(got), nan):
        return False, float("inf")
    if bool(nan.all()):
        return True, 0.0
    err = float((got[~nan] - ref[~nan]).abs().max())
    bound = tol * max(1.0, float(ref[~nan].abs().max()))
    return err <= bound, err / bound


# ------------------------------------------------------------------------------------------------ the restatement against closed forms
@pytest.mark.parametrize("unbiased", [False, True])
def test_restatement_closed_forms(unbiased):
    x, y = torch.tensor([[1.5, -2.0, 0.25]]), torch.tensor([[0.5, -2.0, 4.0]])
    r = restate_verify(x, y, None, None, 1, unbiased)                # one member: crps = |x - y|, spread = 0
    assert torch.equal(r["crps"], (x - y).abs().to(F64)) and torch.equal(r["spread"], torch.zeros(1, 3, dtype=F64)) and torch.equal(r["mean"], x.to(F64))
    assert r["rank"].tolist() == [[0, 0, 1]] and r["pit"].tolist() == [[0.0, 0.5, 1.0]] and int(r["status"][0]) == 1
    assert r["hist"].tolist() == [[2, 1]] and float(r["sums"][0, 0]) == 3.0 and float(r["sums"][0, 1]) == 1.0 + 0.0 + 3.75
    # two equal-weight members a < b: E|X - y| - E|X - X'| / (2 c) with E|X - X'| = (b - a) / 2 and c = 1 / 2 (fair) or 1
    a, bb = -1.0, 2.0
    pair = (bb - a) / 2.0 / (2.0 * (0.5 if unbiased else 1.0))
    x2 = torch.tensor([[a] * 3, [bb] * 3])
    y2 = torch.tensor([[0.5, -3.0, 2.0]])                            # between, outside, on the upper member
    r = restate_verify(x2, y2, None, None, 2, unbiased)
    want = torch.tensor([[(0.5 - a) / 2 + (bb - 0.5) / 2 - pair, ((a + 3.0) + (bb + 3.0)) / 2 - pair, (2.0 - a) / 2 - pair]], dtype=F64)
    assert float((r["crps"] - want).abs().max()) <= 1e-15
    assert r["rank"].tolist() == [[1, 0, 1]] and r["pit"].tolist() == [[0.5, 0.0, 0.75]]
    spread = (bb - a) / 2.0 * (2.0 ** 0.5 if unbiased else 1.0)
    assert float((r["spread"] - spread).abs().max()) <= 1e-15 and float((r["mean"] - (a + bb) / 2).abs().max()) == 0.0
    # every member on the reading
    r = restate_verify(torch.full((7, 4), 0.75), torch.full((1, 4), 0.75), None, None, 7, unbiased)
    assert torch.equal(r["crps"], torch.zeros(1, 4, dtype=F64)) and float((r["pit"] - 0.5).abs().max()) <= 1e-15 and int(r["rank"].abs().max()) == 0
    assert r["hist"][0].tolist() == [4] + [0] * 7
    # log-weights that kill all but one member reproduce N = 1
    g = torch.Generator().manual_seed(3)
    x5, y5 = torch.randn(5, 6, generator=g), torch.randn(1, 6, generator=g)
    lw = torch.full((5,), float("-inf"))
    lw[3] = -2.5
    r5, r1 = restate_verify(x5, y5, None, lw, 5, unbiased), restate_verify(x5[3:4], y5, None, None, 1, unbiased)
    for k in FLOATS + ("rank",):
        assert torch.equal(r5[k], r1[k]), k
    assert int(r5["status"][0]) == 1 and torch.equal(r5["sums"], r1["sums"]) and torch.equal(r5["hist"][0, :2], r1["hist"][0])
    # equal log-weights reproduce None
    ra, rb = restate_verify(x5, y5, None, torch.full((5,), 1.75), 5, unbiased), restate_verify(x5, y5, None, None, 5, unbiased)
    for k in FLOATS + ("sums",):
        assert float((ra[k] - rb[k]).abs().max()) <= 1e-15, k
    assert torch.equal(ra["rank"], rb["rank"]) and torch.equal(ra["hist"], rb["hist"])


def test_restatement_dead_and_bad_sensors_and_unscored_histories():
    g = torch.Generator().manual_seed(4)
    n, K, B = 4, 9, 3
    x, y = torch.randn(B * n, K, generator=g), torch.randn(B, K, generator=g)
    prec = 0.5 + torch.rand(B, K, generator=g)
    prec[:, ::4] = 0.0
    base = restate_verify(x, y, prec, None, n, True)
    assert bool((base["rank"][:, ::4] == -1).all()) and float(base["crps"][:, ::4].abs().max()) == 0.0
    assert base["sums"][:, 0].tolist() == [6.0] * B and base["hist"].sum(1).tolist() == [6] * B
    for junk in (float("nan"), float("inf"), 3e38):                  # a reading without weight is neutral whatever it and the predictions hold
        xx, yy = x.clone(), y.clone()
        yy[:, ::4] = junk
        xx[:, ::4] = junk
        got = restate_verify(xx, yy, prec, None, n, True)
        for k in base:
            assert torch.equal(got[k], base[k]), (junk, k)
    xx = x.clone()
    xx[1 * n + 2, 1] = float("nan")                                  # a live member's prediction at a live sensor: that sensor alone is bad
    got = restate_verify(xx, y, prec, None, n, True)
    assert int(got["rank"][1, 1]) == -2 and bool(torch.isnan(got["crps"][1, 1])) and float(got["sums"][1, 6]) == 1.0 and float(got["sums"][1, 0]) == 5.0
    keep = torch.ones(B, K, dtype=torch.bool)
    keep[1, 1] = False
    for k in FLOATS + ("rank",):
        assert torch.equal(got[k][keep], base[k][keep]), k
    assert torch.equal(got["sums"][[0, 2]], base["sums"][[0, 2]]) and torch.equal(got["hist"][[0, 2]], base["hist"][[0, 2]])
    lw = torch.zeros(B * n)
    lw[n + 1] = float("nan")                                         # a history whose log-weights hold a NaN is not scored; the others do not move
    got = restate_verify(x, y, prec, lw, n, True)
    assert got["status"].tolist() == [4, -1, 4] and float(got["sums"][1].abs().max()) == 0.0 and bool((got["rank"][1] == -1).all())
    for k in FLOATS:
        assert float((got[k][[0, 2]] - base[k][[0, 2]]).abs().max()) <= 1e-15 and float(got[k][1].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ the composed path against the restatement
def _ties(t, n):
    x, y = t["pred"].view(-1, n, t["pred"].shape[1]), t["obs"]
    srt = x.sort(dim=1).values
    return bool((srt[:, 1:] == srt[:, :-1]).any()) if n > 1 else False, bool((x == y.unsqueeze(1)).any())


@pytest.mark.parametrize("n", V_N)
def test_composed_path_against_the_restatement(n):
    from sea_amd.ensemble import _composed_verify

    worst, member_ties, reading_ties = 0.0, False, False
    for K, B, wp, wl in verify_cases(n):
        t, ref = verify_case(n, K, B, wp, wl), reference(n, K, B, wp, wl)
        a, bb = _ties(t, n)
        member_ties, reading_ties = member_ties or a, reading_ties or bb
        exact = _composed_verify(t["pred"], t["obs"], t["prec"], t["logw"], n, t["unbiased"], out_dtype=F64)
        got = verifier(n, K, fused=False, unbiased=t["unbiased"]).from_predictions(t["pred"], t["obs"], t["prec"], t["logw"])
        for k in FLOATS:
            ok, ratio = close(exact[k], ref[k], 1e-12)
            worst = max(worst, ratio)
            assert ok, (K, B, wp, wl, k, ratio)
            assert getattr(got, k).dtype == torch.float32 and torch.equal(getattr(got, k), exact[k].to(torch.float32)), (K, B, wp, wl, k)
        for j in range(8):
            ok, ratio = close(got.sums[:, j], ref["sums"][:, j], 1e-12)
            worst = max(worst, ratio)
            assert ok, (K, B, wp, wl, "sums", j, ratio)
        assert got.rank.dtype == torch.int32 and torch.equal(got.rank.long(), ref["rank"]), (K, B, wp, wl)
        assert got.hist.dtype == torch.int64 and torch.equal(got.hist, ref["hist"]) and torch.equal(got.status.long(), ref["status"]), (K, B, wp, wl)
        assert torch.equal(got.sums[:, 0], ref["sums"][:, 0]) and torch.equal(got.hist.sum(1).double(), ref["sums"][:, 0])
    assert reading_ties and (member_ties or n == 1)
    print(f"verify composed N = {n}: largest error / bound over {len(verify_cases(n))} cases {worst:.3e}")


def test_composed_path_bad_sensors_and_unscored_histories():
    g = torch.Generator().manual_seed(6)
    n, K, B = 5, 70, 3
    x, y = (torch.randn(B * n, K, generator=g) * 4).round() / 4, (torch.randn(B, K, generator=g) * 4).round() / 4
    prec = 0.5 + torch.rand(K, generator=g)
    prec[::5] = 0.0
    x[2, 0], y[0, 5] = float("nan"), 3e38                            # dead readings
    x[n + 1, 3], y[2, 66] = float("nan"), float("inf")               # bad sensors
    lw = torch.randn(B * n, generator=g)
    lw[2 * n + 4] = float("-inf")
    x[2 * n + 4, 7] = float("nan")                                   # a dead member's prediction reaches nothing
    ver = verifier(n, K, fused=False)
    for logw in (lw, torch.cat([lw[:n], torch.full((n,), float("nan")), lw[2 * n:]]), torch.cat([torch.full((n,), float("-inf")), lw[n:]])):
        ref, got = restate_verify(x, y, prec, logw, n, True), ver.from_predictions(x, y, prec, logw)
        for k in FLOATS:
            ok, ratio = close(getattr(got, k), ref[k], 1e-6)         # float32 outputs
            assert ok, (k, ratio)
        ok, ratio = close(got.sums, ref["sums"], 1e-12)
        assert ok and torch.equal(got.rank.long(), ref["rank"]) and torch.equal(got.hist, ref["hist"]) and torch.equal(got.status.long(), ref["status"])
    assert ref["status"].tolist() == [-1, 5, 4] and int(ref["rank"][2, 66]) == -2 and float(ref["sums"][2, 6]) == 1.0


def test_accumulation_is_the_concatenated_sensors():
    n, B, K1, K2 = 33, 3, 63, 65
    t1, t2 = verify_case(n, K1, B, True, True), verify_case(n, K2, B, True, True)
    lw = t1["logw"]
    first = verifier(n, K1).from_predictions(t1["pred"], t1["obs"], t1["prec"], lw)
    sums1, hist1 = first.sums.clone(), first.hist.clone()
    second = verifier(n, K2).from_predictions(t2["pred"], t2["obs"], t2["prec"], lw, into=first)
    assert second.sums.data_ptr() == first.sums.data_ptr() and second.hist.data_ptr() == first.hist.data_ptr()      # added in place
    assert second.crps.shape == (B, K2) and not torch.equal(first.sums, sums1)
    whole = verifier(n, K1 + K2).from_predictions(torch.cat([t1["pred"], t2["pred"]], 1), torch.cat([t1["obs"], t2["obs"]], 1), torch.cat([t1["prec"], t2["prec"]], 1), lw)
    ok, ratio = close(second.sums, whole.sums, 1e-12)
    assert ok, ratio
    assert torch.equal(second.hist, whole.hist) and torch.equal(second.hist, hist1 + verifier(n, K2).from_predictions(t2["pred"], t2["obs"], t2["prec"], lw).hist)
    assert torch.equal(second.sums[:, 0], whole.sums[:, 0]) and torch.equal(whole.crps[:, K1:], second.crps)


def test_derived_scores():
    n, K, B = 64, 257, 3
    t, ref = verify_case(n, K, B, True, False), reference(n, K, B, True, False)
    s = verifier(n, K, unbiased=t["unbiased"]).from_predictions(t["pred"], t["obs"], t["prec"])
    cnt = ref["sums"][:, 0]
    live = t["prec"] > 0
    err2 = torch.where(live, (t["obs"].double() - ref["mean"]) ** 2, torch.zeros((), dtype=F64)).sum(1)
    for got, want in ((s.count, cnt), (s.mean_crps, ref["crps"].sum(1) / cnt), (s.rmse, (err2 / cnt).sqrt()), (s.mean_spread, ((ref["spread"] ** 2).sum(1) / cnt).sqrt()),
                      (s.spread_skill, ((ref["spread"] ** 2).sum(1) / err2).sqrt()), (s.consistency, ref["sums"][:, 4] / cnt), (s.bias, ref["sums"][:, 5] / cnt),
                      (s.suggested_inflation, ((err2 - ref["sums"][:, 7]) / ref["sums"][:, 3]).clamp_min(1.0).sqrt())):
        assert got.dtype == F64 and got.shape == (B,) and float((got - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))
    assert bool((s.suggested_inflation >= 1.0).all())
    # sigma folds into the precision as SensorLikelihood folds it: 1 / sigma^2 per sensor
    s2 = verifier(n, K, unbiased=t["unbiased"], sigma=2.0).from_predictions(t["pred"], t["obs"], t["prec"])
    assert float((s2.sums[:, 7] - 4.0 * s.sums[:, 7]).abs().max()) <= 1e-9 and torch.equal(s2.crps, s.crps)


# ------------------------------------------------------------------------------------------------ the entry point, without a GPU
@pytest.fixture(scope="module")
def lib():
    from sea_amd import build, _native

    build.build(verbose=False)
    return _native.lib()


def _table():
    from sea_amd import _native as N

    p = N.SeaEnsembleVerify()
    p.pred, p.obs, p.prec, p.logw = 0x100000, 0x110000, 0x120000, 0x130000                       # made-up, aligned, never dereferenced
    p.mean, p.spread, p.crps, p.pit, p.rank = 0x140000, 0x150000, 0x160000, 0x170000, 0x180000
    p.sums, p.hist, p.status, p.work = 0x190000, 0x1a0000, 0x1b0000, 0x1c0000
    p.ld_pred, p.ld_obs, p.ld_prec, p.ld_out, p.work_bytes = 40, 40, 0, 40, 1 << 20
    p.B, p.N, p.K, p.unbiased, p.accumulate = 2, 8, 40, 1, 0
    return p


def test_symbols_and_struct_layout(lib):
    from sea_amd import _native as N

    for name in ("sea_ensemble_verify", "sea_ensemble_verify_ws_bytes"):
        assert hasattr(lib, name) and name in N.EXPORTED_SYMBOLS
    assert C.sizeof(N.SeaEnsembleVerify) == 168                      # include/sea_hip.h states it
    assert N.SeaEnsembleVerify.sums.offset == 72 and N.SeaEnsembleVerify.ld_pred.offset == 104 and N.SeaEnsembleVerify.work_bytes.offset == 136
    assert N.SeaEnsembleVerify.B.offset == 144 and N.SeaEnsembleVerify.accumulate.offset == 160
    assert lib.sea_abi_version() == 8 and len(N.ABI_STRUCTS) == 33 and N.ABI_STRUCTS[-1] is N.SeaKvFork and N.VERIFY_MAX_N == 128
    # the workspace: per (history, tile of 16 sensors) 8 fp64 sums and N + 1 int32 bins, in 8-byte words
    assert lib.sea_ensemble_verify_ws_bytes(2, 8, 40) == 2 * 3 * (8 + 5) * 8 and lib.sea_ensemble_verify_ws_bytes(3, 128, 130) == 3 * 9 * (8 + 65) * 8
    assert lib.sea_ensemble_verify_ws_bytes(1, 129, 4) == -1 and lib.sea_ensemble_verify_ws_bytes(0, 4, 4) == -1
    # the library reads the fields where the binding writes them: its messages quote the values back
    p = _table()
    p.ld_prec = 39
    assert lib.sea_ensemble_verify(C.byref(p), None) == -1 and b"ld_prec=39 must be 0" in lib.sea_last_error()
    p = _table()
    p.work_bytes = 623
    assert lib.sea_ensemble_verify(C.byref(p), None) == -1 and b"work_bytes=623 below the 624" in lib.sea_last_error()
    p = _table()
    p.accumulate = 2
    assert lib.sea_ensemble_verify(C.byref(p), None) == -1 and b"accumulate=2" in lib.sea_last_error()


BREAKS = {"null pred": ("pred", None), "null obs": ("obs", None), "null sums": ("sums", None), "null hist": ("hist", None), "null status": ("status", None),
          "null work": ("work", None), "misaligned pred": ("pred", 0x100002), "misaligned logw": ("logw", 0x130001), "misaligned rank": ("rank", 0x180002),
          "misaligned sums": ("sums", 0x190004), "misaligned hist": ("hist", 0x1a0004), "misaligned work": ("work", 0x1c0004), "B = 0": ("B", 0),
          "B = 65536": ("B", 65536), "N = 0": ("N", 0), "K = 0": ("K", 0), "ld_pred short": ("ld_pred", 39), "ld_obs short": ("ld_obs", 8),
          "ld_prec short": ("ld_prec", 39), "ld_out short": ("ld_out", 39), "unbiased = 2": ("unbiased", 2), "accumulate = -1": ("accumulate", -1),
          "work too small": ("work_bytes", 616)}


@pytest.mark.parametrize("what", sorted(BREAKS))
def test_verify_refuses_bad_arguments_without_a_device(lib, what):
    p = _table()
    setattr(p, *BREAKS[what])
    assert lib.sea_ensemble_verify(C.byref(p), None) == -1, what
    assert b"sea_ensemble_verify" in lib.sea_last_error()


def test_unsupported_sizes_and_null_tables(lib):
    p = _table()
    p.N = 129
    assert lib.sea_ensemble_verify(C.byref(p), None) == -3 and b"sea_ensemble_verify" in lib.sea_last_error() and b"N=129" in lib.sea_last_error()
    assert lib.sea_ensemble_verify(None, None) == -1 and b"sea_ensemble_verify" in lib.sea_last_error()
    # prec, logw and the per-sensor outputs may be NULL: such a table passes the pointer checks and fails only at the last check, which this test breaks
    p = _table()
    p.prec = p.logw = p.mean = p.spread = p.crps = p.pit = p.rank = None
    p.ld_out, p.work_bytes = 0, 8
    assert lib.sea_ensemble_verify(C.byref(p), None) == -1 and b"work_bytes=8" in lib.sea_last_error()


# ------------------------------------------------------------------------------------------------ refusals of the Python layers
def test_python_layers_refuse_before_a_device_is_touched():
    from sea_amd import ops
    from sea_amd.ensemble import EnsembleScores, SensorSet, SensorVerification
    from sea_amd.utils.train_utils import EnsembleScores as ES2, SensorVerification as SV2

    assert SV2 is SensorVerification and ES2 is EnsembleScores
    c = host_case("a")
    dec = make_decoder("a").set_compute_dtype("bf16")
    P, D_, G = c["P"], c["D"], len(c["groups"])
    s = SensorSet(dec, P, [0, 1, 8], [3, 4, 11], [0, 2, 1])
    for members in (0, True, 2.0, -1):
        with pytest.raises(ValueError):
            SensorVerification(dec, P, members, s)
    for kw in (dict(fused=True, members=129), dict(fused=1), dict(sigma=-1.0), dict(sensors=None)):
        args = dict(members=2, sensors=s)
        args.update(kw)
        with pytest.raises(ValueError):
            SensorVerification(dec, P, **args)
    assert SensorVerification(dec, P, 200, s)._fused_for(torch.device("cuda", 0)) is False               # above 128 members: the composed path
    assert SensorVerification(dec, P, 128, s)._fused_for(torch.device("cuda", 0)) is True
    ver = SensorVerification(dec, P, 2, s, sigma=[0.5, 1.0, 2.0])
    assert ver._like._prec_host == [4.0, 0.25, 1.0]                  # SensorLikelihood's folding
    pred, obs = torch.zeros(4, 3), torch.zeros(2, 3)
    ok = ver.from_predictions(pred, obs)                             # CPU tensors: the composed path
    assert ok.sums.tolist()[0] == [3.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.25 + 4.0 + 1.0]
    for pp, oo, kw in ((torch.zeros(3, 3), obs, {}), (torch.zeros(4, 4), obs, {}), (pred.double(), obs, {}), (pred, torch.zeros(2, 2), {}), (pred, obs.double(), {}),
                       (pred, obs, dict(precision=torch.tensor([1.0, -2.0, 1.0]))), (pred, obs, dict(logw=torch.zeros(3))), (pred, obs, dict(logw=torch.zeros(4, dtype=torch.int64))),
                       (pred, obs, dict(into=ok.sums)), (pred, obs, dict(into=SensorVerification(dec, P, 4, s).from_predictions(pred, obs[:1])))):
        with pytest.raises(ValueError):
            ver.from_predictions(pp, oo, **kw)
    y = torch.zeros(4, G, P * D_)
    for yy in (torch.zeros(3, G, P * D_), torch.zeros(4, G, P * D_ + 1)):
        with pytest.raises(ValueError):
            ver(yy, obs)
    with pytest.raises(RuntimeError, match="MI355X"):
        SensorVerification(dec, P, 2, s, fused=True).from_predictions(pred, obs)
    with pytest.raises(RuntimeError, match="MI355X"):
        ops.ensemble_verify(pred, obs, 2)
    for kw in (dict(members=0), dict(members=129), dict(pred=torch.zeros(4, 4)), dict(pred=pred.double()), dict(prec=torch.ones(4)), dict(prec=torch.tensor([1.0, float("nan"), 1.0])),
               dict(logw=torch.zeros(3)), dict(obs=torch.zeros(6)), dict(accumulate=True), dict(out=dict(sums=torch.zeros(2, 8))), dict(out=dict(other=pred)),
               dict(accumulate=True, out=dict(sums=torch.zeros(2, 8, dtype=F64)))):
        args = dict(pred=pred, obs=obs, members=2)
        args.update(kw)
        with pytest.raises(ValueError):
            ops.ensemble_verify(**args)
