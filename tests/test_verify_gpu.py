"""Verification of an ensemble at the sensors on the device: sea_ensemble_verify through ops.ensemble_verify, SensorVerification end to end and on a
rollout session.

Reference: the fp64 restatement `restate_verify` of tests/test_verify_cpu.py (the double sum over member pairs), which that file holds against closed
forms; every input comes from that file, and each restatement is computed once there (`reference`).
  kernel      on the SAME fp32 predictions: rank, hist, status and the two counts in sums exact; the f32 outputs within 1e-6 max(1, max |ref|) — the
              arithmetic is fp64 over at most 128 + 64 terms, the margin covers the fp32 store (6e-8 relative) and nothing else; the fp64 sums within
              1e-10 max(1, |ref|): fp64 rounding over at most 385 terms, three digits left for the cancellation between the CRPS's two terms; exact
              bits where the contract promises them
  end to end  bf16 fused: e <= 2 e_c + 1e-6 for mean, spread, crps and the derived means (e_c: fused=False on the same inputs; the factor 2 covers
              summation order on top of bf16 operand rounding); fp32: e <= 1e-4; rank and pit are discontinuous in the predictions and are compared on
              the same predictions only"""
import functools

import pytest
import torch

from tests.test_decode_loss_cpu import rel
from tests.test_decode_loss_gpu import DEV, TOL_F32, case, decoder
from tests.test_enkf_cpu import E2E_SETS
from tests.test_sensor_cpu import SPLITS, _draw, host_case, restate_sensor, sensor_obs, sensor_precision, sensor_sets
from tests.test_verify_cpu import FLOATS, V_N, close, reference, restate_verify, verify_case, verify_cases

pytestmark = pytest.mark.gpu

F64 = torch.float64


def dev(t):
    return None if t is None else t.to(DEV)


def run_verify(t, n, accumulate=False, out=None):
    from sea_amd import ops

    return ops.ensemble_verify(dev(t["pred"]), dev(t["obs"]), n, prec=dev(t["prec"]), logw=dev(t["logw"]), unbiased=t["unbiased"], accumulate=accumulate, out=out)


def prefilled(B, K, n):
    """Output buffers that hold NaN or -7: every element has to be written."""
    out = {k: torch.full((B, K), float("nan"), device=DEV) for k in FLOATS}
    out.update(rank=torch.full((B, K), -7, device=DEV, dtype=torch.int32), sums=torch.full((B, 8), float("nan"), device=DEV, dtype=F64),
               hist=torch.full((B, n + 1), -7, device=DEV, dtype=torch.int64), status=torch.full((B,), -7, device=DEV, dtype=torch.int32))
    return out


def same_bits(a, b, keys=None):
    """Equal bits, NaN included (torch.equal takes NaN != NaN)."""
    for k in (a.keys() if keys is None else keys):
        x, y = a[k], b[k]
        if x.is_floating_point():
            x, y = x.view(torch.int32 if x.dtype == torch.float32 else torch.int64), y.view(torch.int32 if y.dtype == torch.float32 else torch.int64)
        if not torch.equal(x, y):
            return False
    return True


# ------------------------------------------------------------------------------------------------ the kernel
@pytest.mark.parametrize("n", [n for n in V_N if n <= 128])
def test_verify_against_fp64_on_the_same_predictions(n):
    worst_f32, worst_f64 = 0.0, 0.0
    for K, B, wp, wl in verify_cases(n):
        t, ref = verify_case(n, K, B, wp, wl), reference(n, K, B, wp, wl)
        out = prefilled(B, K, n)
        got = run_verify(t, n, out=out)
        assert all(got[k].data_ptr() == out[k].data_ptr() for k in out)
        got = {k: v.cpu() for k, v in got.items()}
        assert torch.equal(got["rank"].long(), ref["rank"]), (K, B, wp, wl)
        assert torch.equal(got["hist"], ref["hist"]) and torch.equal(got["status"].long(), ref["status"]), (K, B, wp, wl)
        assert torch.equal(got["sums"][:, 0], ref["sums"][:, 0]) and torch.equal(got["sums"][:, 6], ref["sums"][:, 6]), (K, B, wp, wl)
        for k in FLOATS:
            ok, ratio = close(got[k], ref[k], 1e-6)
            worst_f32 = max(worst_f32, ratio)
            assert ok, (K, B, wp, wl, k, ratio)
        for j in range(8):
            ok, ratio = close(got["sums"][:, j], ref["sums"][:, j], 1e-10)
            worst_f64 = max(worst_f64, ratio)
            assert ok, (K, B, wp, wl, "sums", j, ratio)
    print(f"verify N = {n}: largest error / bound over {len(verify_cases(n))} cases: f32 outputs {worst_f32:.3e} (bound 1e-6), fp64 sums {worst_f64:.3e} (bound 1e-10)")


def test_more_tiles_than_the_finish_launch_holds_at_once():
    """4101 sensors are 257 tiles of 16: the finish launch adds them in two chunks (256 tiles' partial sums at a time)."""
    n, K, B = 5, 4101, 2
    g = torch.Generator().manual_seed(77)
    t = dict(pred=(torch.randn(B * n, K, generator=g) * 4).round() / 4, obs=(torch.randn(B, K, generator=g) * 4).round() / 4,
             prec=0.25 + torch.rand(B, K, generator=g), logw=torch.randn(B * n, generator=g), unbiased=True)
    t["prec"][:, ::9] = 0.0
    ref = restate_verify(t["pred"], t["obs"], t["prec"], t["logw"], n, True)
    got = {k: v.cpu() for k, v in run_verify(t, n, out=prefilled(B, K, n)).items()}
    assert torch.equal(got["rank"].long(), ref["rank"]) and torch.equal(got["hist"], ref["hist"]) and torch.equal(got["status"].long(), ref["status"])
    assert torch.equal(got["sums"][:, 0], ref["sums"][:, 0]) and float(got["sums"][:, 6].abs().max()) == 0.0
    for k in FLOATS:
        ok, ratio = close(got[k], ref[k], 1e-6)
        assert ok, (k, ratio)
    for j in range(8):                                                               # 1e-10: fp64 rounding over 4101 terms is below 1e-12 relative
        ok, ratio = close(got["sums"][:, j], ref["sums"][:, j], 1e-10)
        assert ok, (j, ratio)


def test_the_form_taken_is_noted():
    import ctypes as C

    from sea_amd import _native as N

    for n, lanes in ((5, 1), (64, 1), (65, 2), (128, 2)):
        run_verify(verify_case(n, 65, 1, False, False), n)
        a, b = C.c_int(0), C.c_int(0)
        name = N.lib().sea_last_form(C.byref(a), C.byref(b))
        assert name == b"verify" and a.value == lanes and b.value == 16 * (n | 1) * 4, (n, name, a.value, b.value)


@pytest.mark.parametrize("n", [5, 64, 128])
def test_verify_bits(n):
    """Two runs give the same bits; a history alone reproduces its rows and sums; the first 64 and the last 66 sensors, run as launches of their own,
    reproduce the per-sensor bits, and so do the first 37 and the last 93 (a cut inside a tile); junk at dead readings changes nothing; a NaN in one live member's prediction spoils that sensor alone; a NaN in one
    history's log-weights leaves the other histories' bits; accumulating twice doubles sums and hist exactly."""
    K, B = 130, 3
    t = dict(verify_case(n, 257, B, True, True))
    t.update(pred=t["pred"][:, :K].contiguous(), obs=t["obs"][:, :K].contiguous(), prec=t["prec"][:, :K].contiguous())
    per_sensor = FLOATS + ("rank",)
    base = run_verify(t, n)
    assert same_bits(base, run_verify(t, n))
    assert int(base["status"].min()) > 0 and int((base["rank"] == -1).sum()) == int((t["prec"] == 0).sum()) > 0
    for b in range(B):
        one = dict(t, pred=t["pred"][b * n:(b + 1) * n], obs=t["obs"][b:b + 1], prec=t["prec"][b:b + 1], logw=t["logw"][b * n:(b + 1) * n])
        r = run_verify(one, n)
        assert same_bits({k: v[0] for k, v in r.items()}, {k: v[b] for k, v in base.items()}), b
    for lo, hi in ((0, 64), (64, 130), (0, 37), (37, 130)):                           # a sensor's bits do not depend on K or on its place in a tile (37: no multiple of the tile)
        part = dict(t, pred=t["pred"][:, lo:hi].contiguous(), obs=t["obs"][:, lo:hi].contiguous(), prec=t["prec"][:, lo:hi].contiguous())
        r = run_verify(part, n)
        assert same_bits(r, {k: base[k][:, lo:hi] for k in per_sensor}, per_sensor), (lo, hi)
    dead = t["prec"] == 0
    for junk in (3e38, float("nan")):
        obs, pred = t["obs"].clone(), t["pred"].clone()
        obs[dead] = junk
        pred.view(B, n, K)[dead.unsqueeze(1).expand(B, n, K)] = junk
        assert same_bits(run_verify(dict(t, obs=obs, pred=pred), n), base), junk
    # a live member's prediction that is NaN at one live sensor
    live_members = torch.nonzero(t["logw"].view(B, n)[1] != float("-inf")).view(-1)
    j, k = int(live_members[len(live_members) // 2]), int(torch.nonzero(~dead[1])[70])
    pred = t["pred"].clone()
    pred[1 * n + j, k] = float("nan")
    r = run_verify(dict(t, pred=pred), n)
    assert int(r["rank"][1, k]) == -2 and all(bool(torch.isnan(r[f][1, k])) for f in FLOATS)
    assert float(r["sums"][1, 6]) == float(base["sums"][1, 6]) + 1.0 and float(r["sums"][1, 0]) == float(base["sums"][1, 0]) - 1.0
    keep = torch.ones(B, K, dtype=torch.bool, device=DEV)
    keep[1, k] = False
    assert same_bits({f: r[f][keep] for f in per_sensor}, {f: base[f][keep] for f in per_sensor})
    assert same_bits({f: r[f][[0, 2]] for f in r}, {f: base[f][[0, 2]] for f in base})
    # the same NaN under a DEAD member reaches nothing
    dead_members = torch.nonzero(t["logw"].view(B, n)[1] == float("-inf")).view(-1)
    if len(dead_members):
        pred = t["pred"].clone()
        pred[1 * n + int(dead_members[0]), k] = float("nan")
        assert same_bits(run_verify(dict(t, pred=pred), n), base)
    # a history whose log-weights hold a NaN is not scored
    logw = t["logw"].clone()
    logw[2 * n + n // 2] = float("nan")
    r = run_verify(dict(t, logw=logw), n)
    assert r["status"].tolist()[2] == -1 and r["status"].tolist()[:2] == base["status"].tolist()[:2]
    assert all(float(r[f][2].abs().max()) == 0.0 for f in FLOATS) and bool((r["rank"][2] == -1).all())
    assert float(r["sums"][2].abs().max()) == 0.0 and int(r["hist"][2].abs().max()) == 0
    assert same_bits({f: r[f][:2] for f in r}, {f: base[f][:2] for f in base})
    # accumulate twice on the same inputs: exactly doubled sums and hist
    acc = dict(sums=torch.zeros(B, 8, device=DEV, dtype=F64), hist=torch.zeros(B, n + 1, device=DEV, dtype=torch.int64))
    r1 = run_verify(t, n, accumulate=True, out=acc)
    assert same_bits({k: r1[k] for k in ("sums", "hist")}, {k: base[k] for k in ("sums", "hist")})
    r2 = run_verify(t, n, accumulate=True, out=acc)
    assert r2["sums"].data_ptr() == acc["sums"].data_ptr() and torch.equal(r2["sums"], 2.0 * base["sums"]) and torch.equal(r2["hist"], 2 * base["hist"])


def test_no_scored_sensor_and_null_outputs():
    import ctypes as C

    from sea_amd import _native as N, ops

    n, K, B = 33, 65, 3
    t = verify_case(n, K, B, True, True)
    r = run_verify(dict(t, prec=torch.zeros(B, K)), n)
    assert float(r["sums"].abs().max()) == 0.0 and int(r["hist"].abs().max()) == 0 and bool((r["rank"] == -1).all()) and int(r["status"].min()) == n - 1
    base = run_verify(t, n)
    pred, obs, prec, logw = dev(t["pred"]), dev(t["obs"]), dev(t["prec"]), dev(t["logw"])
    out = prefilled(B, K, n)
    work = torch.empty(int(N.lib().sea_ensemble_verify_ws_bytes(B, n, K)), device=DEV, dtype=torch.uint8)
    tab = N.SeaEnsembleVerify()
    ops.fill_ensemble_verify(tab, pred, obs, prec, logw, n, t["unbiased"], False, None, None, out["crps"], None, None, out["sums"], out["hist"], out["status"], work)
    N.check(N.lib().sea_ensemble_verify(C.byref(tab), N.stream_ptr()), "sea_ensemble_verify")
    assert same_bits(out, base, ("crps", "sums", "hist", "status")) and bool(torch.isnan(out["mean"]).all()) and bool((out["rank"] == -7).all())


# ------------------------------------------------------------------------------------------------ end to end
@functools.lru_cache(maxsize=None)
def _decoder(name, dtype):
    return decoder(name, dtype)


def e2e_cases():
    return [(name, s, m, h) for name in ("a", "b", "c") for s in E2E_SETS[name] for m, h in SPLITS[name]]


@functools.lru_cache(maxsize=None)
def e2e_case(name, set_name, members, hist, dtype="bf16"):
    """The shape's states as y [Bm, G, P * D] in the act dtype, the set's readings and precisions, log-weights, and the fp64 restatement of the whole
    chain from the exact decoder (restate_sensor, then restate_verify)."""
    c = host_case(name)
    patch, cell, field = sensor_sets(name)[set_name]
    Bm, P, G, D_ = c["z"].shape
    y = c["z"].permute(0, 2, 1, 3).reshape(Bm, G, P * D_).contiguous()
    y = y.to(torch.bfloat16) if dtype == "bf16" else y.clone()
    z = y.to(F64).view(Bm, G, P, D_).permute(0, 2, 1, 3)
    obs, prec = sensor_obs(name, set_name, hist), sensor_precision(name, set_name, hist)
    logw = torch.randn(Bm, generator=torch.Generator().manual_seed(55 + members + hist)) if members % 2 else None
    _, pred = restate_sensor(c["w1"], c["w2"], c["b2"], c["groups"], z, patch, cell, field, obs, prec, members)
    return dict(y=y, patch=patch, cell=cell, field=field, obs=obs, prec=prec, logw=logw, ref=restate_verify(pred, obs, prec, logw, members, True))


def _verifier(name, k, members, dtype, fused):
    from sea_amd.ensemble import SensorSet, SensorVerification

    dec = _decoder(name, dtype)
    s = SensorSet(dec, case(name)["P"], k["patch"], k["cell"], k["field"])
    return SensorVerification(dec, case(name)["P"], members, s, fused=fused)


def _errors(s, ref):
    """Relative L2 errors of the continuous per-sensor outputs, and the largest relative error of the derived means, against the restatement."""
    cnt = ref["sums"][:, 0]
    derived = ((s.mean_crps, ref["sums"][:, 1] / cnt), (s.rmse, (ref["sums"][:, 2] / cnt).sqrt()), (s.mean_spread, (ref["sums"][:, 3] / cnt).sqrt()),
               (s.consistency, ref["sums"][:, 4] / cnt))
    e = {k: rel(getattr(s, k).cpu(), ref[k]) for k in ("mean", "spread", "crps")}
    e["derived"] = max(float(((got.cpu() - want).abs() / want.abs().clamp_min(1e-300)).max()) for got, want in derived)
    return e


@pytest.mark.parametrize("name,set_name,members,hist", e2e_cases())
def test_verification_bf16_against_fp64(name, set_name, members, hist):
    k = e2e_case(name, set_name, members, hist)
    y, obs, prec, logw = k["y"].to(DEV), k["obs"].to(DEV), k["prec"].to(DEV), dev(k["logw"])
    s = _verifier(name, k, members, "bf16", None)(y, obs, prec, logw)
    s_c = _verifier(name, k, members, "bf16", False)(y, obs, prec, logw)
    assert s.crps.dtype == torch.float32 and s.crps.shape == obs.shape and s.sums.dtype == F64 and s.hist.shape == (hist, members + 1)
    assert torch.equal(s.status.cpu().long(), k["ref"]["status"]) and torch.equal(s.sums[:, 0].cpu(), k["ref"]["sums"][:, 0])
    assert torch.equal(s.hist.sum(1).cpu().double(), k["ref"]["sums"][:, 0]) and torch.equal((s.rank == -1).cpu(), k["prec"] == 0)
    e, e_c = _errors(s, k["ref"]), _errors(s_c, k["ref"])
    print(f"verify shape {name} set {set_name} members {members} x {hist}: fused " + " ".join(f"{q} {v:.3e}" for q, v in e.items())
          + "; composed " + " ".join(f"{q} {v:.3e}" for q, v in e_c.items()))
    for q in e:
        assert e[q] <= 2 * e_c[q] + 1e-6, (q, e[q], e_c[q])


@pytest.mark.parametrize("name,set_name,members,hist", e2e_cases())
def test_verification_fp32_against_fp64(name, set_name, members, hist):
    k = e2e_case(name, set_name, members, hist, "fp32")
    s = _verifier(name, k, members, "fp32", None)(k["y"].to(DEV), k["obs"].to(DEV), k["prec"].to(DEV), dev(k["logw"]))
    e = _errors(s, k["ref"])
    print(f"verify fp32 shape {name} set {set_name} members {members} x {hist}: " + " ".join(f"{q} {v:.3e}" for q, v in e.items()))
    for q in e:
        assert e[q] <= TOL_F32, (q, e[q])


# ------------------------------------------------------------------------------------------------ on a rollout session
def test_verification_on_a_rollout_session():
    """open_rollout -> fork(n) -> step -> transform -> from_predictions (the forecast's scores) -> analyse -> __call__ (the analysis' scores): nothing is
    read back, the analysis' rmse at the sensors is below the forecast's, the histogram holds every live sensor, and into= aggregates the two."""
    from sea_amd.ensemble import SensorKalman, SensorSet, SensorVerification
    from oracle.recipe import recipe_inputs
    from tests.test_input_grad_gpu import cfg_of
    from tests.test_model_gpu import build
    from tests.test_rollout_session_gpu import open_on

    c = case("a")
    P, D_, n_mem, B, k = 4, c["D"], 8, 2, 3
    G = len(c["groups"])
    cfg = cfg_of(1, P * D_, 4, G)
    m = build(cfg, "bf16")
    x, _, ib = recipe_inputs(B, k + 4, cfg, seed=9)
    dec = decoder("a", "bf16")
    g = torch.Generator().manual_seed(21)
    patch, cell, field = _draw(g, c["groups"], c["n_inp"], [(0, 0, 5), (0, 3, 33), (1, 2, 4)])
    K = len(patch)
    base = 0.5 + torch.rand(B, K, generator=g)
    base[torch.rand(B, K, generator=g) < 0.2] = 0.0
    conds = torch.rand(B * n_mem, 1, generator=g).to(DEV)

    ens = open_on(m, x, ib, k).fork(n_mem)
    y = ens.step(conds)
    s = SensorSet(dec, P, patch, cell, field)
    ka = SensorKalman(dec, P, n_mem, s)
    ver = SensorVerification(dec, P, n_mem, s)
    # the fixture of tests/test_enkf_gpu.py's session test: the readings are member 0's predictions (a truth inside the ensemble's span), the precisions
    # scaled so that trace(C) = 50 per history
    _, _, pred0 = ka.transform(y, torch.zeros(B, K, device=DEV), None)
    pred0 = pred0.cpu().double().view(B, n_mem, K)
    obs = pred0[:, 0].to(torch.float32)
    anom = pred0 - pred0.mean(1, keepdim=True)
    trace = (base.double() * (anom * anom).sum(1) / (n_mem - 1)).sum(1, keepdim=True)
    assert bool((trace > 0).all())
    prec = (base.double() * 50.0 / trace).to(torch.float32)
    obs_d, prec_d = obs.to(DEV), prec.to(DEV)
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")                                              # nothing is read back, nothing uploaded: the tables went up with the set
    try:
        _, _, pred = ka.transform(y, obs_d, prec_d)
        forecast = ver.from_predictions(pred, obs_d, prec_d)
        ya = ka.analyse(y, obs_d, prec_d)
        analysis = ver(ya, obs_d, prec_d)
        rmse_f, rmse_a, ratio, infl = forecast.rmse, analysis.rmse, forecast.spread_skill, forecast.suggested_inflation
        total = ver(ya, obs_d, prec_d, into=ver.from_predictions(pred, obs_d, prec_d))
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    live = (prec > 0).sum(1)
    print(f"verify session: rmse forecast {rmse_f.tolist()} analysis {rmse_a.tolist()}; forecast spread / skill {ratio.tolist()}; suggested inflation {infl.tolist()}")
    assert bool((rmse_a < rmse_f).all()) and bool(torch.isfinite(ratio).all()) and bool((infl >= 1.0).all())
    for sc in (forecast, analysis):
        assert torch.equal(sc.hist.sum(1).cpu(), live) and torch.equal(sc.sums[:, 0].cpu(), live.double()) and sc.status.tolist() == [n_mem] * B
    assert torch.equal(total.hist, forecast.hist + analysis.hist) and torch.equal(total.sums, forecast.sums + analysis.sums)
