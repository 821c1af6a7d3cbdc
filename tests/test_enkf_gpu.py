"""The ensemble Kalman analysis on the device: sea_enkf_transform and sea_ensemble_mix through ops, SensorKalman end to end and on a rollout session.

Reference: the fp64 restatements `restate_enkf` / `restate_mix` of tests/test_enkf_cpu.py, which that file holds against the state-space Kalman
formulas; every input comes from that file, where cond(I + C) <= 1e4 is asserted for each.
  transform  on the SAME fp32 predictions: max |D - D_ref| <= 1e-6 max(1, max |D_ref|) — D is stored in fp32 (6e-8 relative); the fp64 Cholesky inverse at
             cond <= 1e4 and N <= 128 contributes about N eps cond ~ 1e-10: the margin covers the fp32 store only; status is the live count; exact bits
             where the contract promises them
  mix        the fp32 increment within 1e-5 relative L2 (fp32 accumulation of N terms); out = (y + inc) rounded to y's dtype, bit for bit
  end to end bf16 fused: e <= 2 e_c + 1e-6 (e_c: fused=False on the same inputs) and e <= 2 x the bf16-operand envelope of tests/test_enkf_cpu.py (the margin
             of 2 covers summation order on top of operand rounding); fp32: e <= 1e-4"""
import functools

import pytest
import torch

from tests.test_decode_loss_cpu import rel
from tests.test_decode_loss_gpu import DEV, TOL_F32, case, decoder
from tests.test_enkf_cpu import MIX_CASES, T_N, bf16_envelope, kalman_case, kalman_cases, mix_case, restate_enkf, restate_mix, transform_case, transform_cases
from tests.test_sensor_cpu import _draw, restate_sensor

pytestmark = pytest.mark.gpu


def dev(t):
    return None if t is None else t.to(DEV)


def run_transform(t, n, out=None):
    from sea_amd import ops

    return ops.enkf_transform(dev(t["pred"]), dev(t["obs"]), n, prec=dev(t["prec"]), taper=dev(t["taper"]), rho=t["rho"], alpha=t["alpha"], out=out)


# ------------------------------------------------------------------------------------------------ the transform kernel
@pytest.mark.parametrize("n", T_N)
def test_transform_against_fp64_on_the_same_predictions(n):
    worst = 0.0
    for K, B, Ld, wp in transform_cases(n):
        t = transform_case(n, K, B, Ld, wp)
        D_ref, s_ref, _ = restate_enkf(t["pred"], t["obs"], t["prec"], t["taper"], n, t["rho"], t["alpha"])
        out = torch.full((B, Ld, n, n), float("nan"), device=DEV)
        D, status = run_transform(t, n, out=out)
        assert D.data_ptr() == out.data_ptr() and D.dtype == torch.float32 and status.dtype == torch.int32 and status.shape == (B, Ld)
        D, status = D.cpu(), status.cpu()
        assert bool(torch.isfinite(D).all()), (K, B, Ld, wp)                         # every element was written
        err = float((D.double() - D_ref).abs().max())
        bound = 1e-6 * max(1.0, float(D_ref.abs().max()))
        worst = max(worst, err / bound)
        assert err <= bound, (K, B, Ld, wp, err, bound)
        assert torch.equal(status.long(), s_ref), (K, B, Ld, wp)
        if Ld > 1:                                                                   # a domain whose taper is all zero: exactly (rho - 1) Pi, rounded to fp32
            Pi = torch.eye(n, dtype=torch.float64) - 1.0 / n
            assert torch.equal(D[:, 1], ((t["rho"] - 1.0) * Pi).to(torch.float32).expand(B, n, n)), (K, B, wp)
    print(f"enkf transform N = {n}: largest max|D - D_ref| / bound over {len(transform_cases(n))} cases {worst:.3e}")


@pytest.mark.parametrize("n", [5, 64, 128])
def test_transform_bits(n):
    """Two runs give the same bits; a history's D is that of a launch holding the history alone, and so is a domain's; a NaN in one member's prediction in
    one history gives that history status -1 and D = 0 and changes no bit of any other."""
    K, B, Ld = 33, 3, 4
    t = transform_case(n, K, B, Ld, True)
    D, status = run_transform(t, n)
    D2, status2 = run_transform(t, n)
    assert torch.equal(D, D2) and torch.equal(status, status2)
    for b in range(B):
        one = dict(t, pred=t["pred"][b * n:(b + 1) * n], obs=t["obs"][b:b + 1], prec=t["prec"][b:b + 1])
        Db, sb = run_transform(one, n)
        assert torch.equal(Db[0], D[b]) and torch.equal(sb[0], status[b]), b
    for d in range(Ld):
        one = dict(t, taper=t["taper"][d:d + 1].contiguous())
        Dd, sd = run_transform(one, n)
        assert torch.equal(Dd[:, 0], D[:, d]) and torch.equal(sd[:, 0], status[:, d]), d
    pred = t["pred"].clone()
    live = int(torch.nonzero((t["prec"][1] > 0) & (t["taper"][0] > 0))[0])
    pred[1 * n + n // 2, live] = float("nan")
    Dn, sn = run_transform(dict(t, pred=pred), n)
    for d in range(Ld):
        hit = bool((t["prec"][1, live] > 0) and (t["taper"][d, live] > 0))           # the sensor is live in this domain
        assert int(sn[1, d]) == (-1 if hit else int(status[1, d]))
        assert torch.equal(Dn[1, d], torch.zeros_like(Dn[1, d]) if hit else D[1, d])
    assert int(sn[1, 0]) == -1
    assert torch.equal(Dn[0], D[0]) and torch.equal(Dn[2], D[2]) and torch.equal(sn[0], status[0]) and torch.equal(sn[2], status[2])
    # a reading without weight is neutral whatever it holds
    obs = t["obs"].clone()
    obs[t["prec"] == 0] = 3e38
    Dj, sj = run_transform(dict(t, obs=obs), n)
    assert torch.equal(Dj, D) and torch.equal(sj, status)


def test_no_live_reading_is_no_update():
    n, K, B = 33, 7, 3
    t = dict(transform_case(n, K, B, 1, True), rho=1.0)
    D, status = run_transform(dict(t, prec=torch.zeros(B, K)), n)
    assert torch.equal(D, torch.zeros_like(D)) and torch.equal(status, torch.zeros_like(status))
    D, status = run_transform(dict(t, prec=torch.full((B, K), float("inf"))), n)      # a live weight that is not finite
    assert torch.equal(D, torch.zeros_like(D)) and bool((status == -1).all())


# ------------------------------------------------------------------------------------------------ the mix kernel
@pytest.mark.parametrize("name", [c[0] for c in MIX_CASES])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_mix_against_fp64(name, dtype):
    from sea_amd import ops

    y_host, D_host, P = mix_case(name)
    y = y_host.to(dtype).to(DEV)
    D = D_host.to(DEV)
    ref = restate_mix(y.cpu(), D_host, P)
    out, inc = ops.ensemble_mix(y, D, P, output=True, increment=True)
    assert out.dtype == dtype and inc.dtype == torch.float32 and out.shape == inc.shape == y.shape and out.data_ptr() != y.data_ptr()
    e = rel(inc.cpu(), ref)
    print(f"enkf mix {name} {dtype}: e(inc) {e:.3e}")
    assert bool(torch.isfinite(inc).all()) and e <= 1e-5, e
    assert torch.equal(out, (y.float() + inc).to(dtype))
    assert torch.equal(ops.ensemble_mix(y, D, P), out) and torch.equal(ops.ensemble_mix(y, D, P, output=False, increment=True), inc)
    assert torch.equal(ops.ensemble_mix(y, torch.zeros_like(D), P), y)               # D = 0: the bits of y


def test_mix_writes_every_element_of_prefilled_outputs():
    import ctypes as C

    from sea_amd import _native as N, ops

    y_host, D_host, P = mix_case("n5_local")
    y, D = y_host.to(torch.bfloat16).to(DEV), D_host.to(DEV)
    out = torch.full_like(y, float("nan"))
    inc = torch.full(y.shape, float("nan"), device=DEV)
    tab = N.SeaEnsembleMix()
    ops.fill_ensemble_mix(tab, y, D, out, inc, D.shape[2], P)
    N.check(N.lib().sea_ensemble_mix(C.byref(tab), N.SEA_BF16, N.stream_ptr()), "sea_ensemble_mix")
    assert bool(torch.isfinite(out.float()).all()) and bool(torch.isfinite(inc).all())
    want_out, want_inc = ops.ensemble_mix(y, D, P, output=True, increment=True)
    assert torch.equal(out, want_out) and torch.equal(inc, want_inc)


# ------------------------------------------------------------------------------------------------ end to end
@functools.lru_cache(maxsize=None)
def _decoder(name, dtype):
    return decoder(name, dtype)


def _kalman(name, k, members, dtype, fused):
    from sea_amd.ensemble import SensorKalman, SensorSet

    dec = _decoder(name, dtype)
    s = SensorSet(dec, case(name)["P"], k["patch"], k["cell"], k["field"])
    return SensorKalman(dec, case(name)["P"], members, s, inflation=k["rho"], anomaly_gain=k["alpha"], taper=k["taper"], fused=fused)


@pytest.mark.parametrize("name,set_name,members,hist,local", kalman_cases())
def test_analyse_bf16_against_fp64(name, set_name, members, hist, local):
    from sea_amd import ops

    k = kalman_case(name, set_name, members, hist, local)
    y, obs, prec = k["y"].to(DEV), k["obs"].to(DEV), k["prec"].to(DEV)
    ka = _kalman(name, k, members, "bf16", None)
    ya, inc = ka.analyse(y, obs, prec, increment=True)
    yc, inc_c = _kalman(name, k, members, "bf16", False).analyse(y, obs, prec, increment=True)
    assert ya.dtype == y.dtype and ya.shape == y.shape and inc.dtype == torch.float32 and yc.dtype == y.dtype
    e, e_c, env = rel(inc.cpu(), k["inc"]), rel(inc_c.cpu(), k["inc"]), bf16_envelope()
    print(f"enkf analyse shape {name} set {set_name} members {members} x {hist} local {local}: fused e {e:.3e}; composed e_c {e_c:.3e}; envelope {env:.3e}")
    assert e <= 2 * e_c + 1e-6, (e, e_c)
    assert e <= 2 * env, (e, env)
    # analyse is transform + ensemble_mix, bit for bit
    D, status, pred = ka.transform(y, obs, prec)
    assert torch.equal(status.cpu().long(), k["status"]) and pred.shape == (y.shape[0], len(k["patch"]))
    out, inc2 = ops.ensemble_mix(y, D, case(name)["P"], output=True, increment=True)
    assert torch.equal(out, ya) and torch.equal(inc2, inc) and torch.equal(ka.analyse(y, obs, prec), ya)


@pytest.mark.parametrize("name,set_name,members,hist,local", kalman_cases())
def test_analyse_fp32_against_fp64(name, set_name, members, hist, local):
    k = kalman_case(name, set_name, members, hist, local, "fp32")
    y, obs, prec = k["y"].to(DEV), k["obs"].to(DEV), k["prec"].to(DEV)
    ya, inc = _kalman(name, k, members, "fp32", None).analyse(y, obs, prec, increment=True)
    e = rel(inc.cpu(), k["inc"])
    print(f"enkf analyse fp32 shape {name} set {set_name} members {members} x {hist} local {local}: e {e:.3e}")
    assert ya.dtype == torch.float32 and e <= TOL_F32, e
    assert torch.equal(ya, y + inc)


# ------------------------------------------------------------------------------------------------ on a rollout session
def test_analysis_on_a_rollout_session():
    """open_rollout -> fork(n) -> step -> analyse -> step(c, state=y_a): nothing is read back, shapes and dtype are kept, and the precision-weighted misfit
    of the ensemble-mean prediction drops."""
    from sea_amd.ensemble import SensorKalman, SensorSet
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
    conds2 = torch.rand(B * n_mem, 1, generator=g).to(DEV)

    ens = open_on(m, x, ib, k).fork(n_mem)
    y = ens.step(conds)                                                                   # [16, 2, 64]

    # the CPU side of the fixture, from the fp64 restatement: the readings are member 0's exact predictions (a truth inside the ensemble's span), the
    # precisions are scaled so that trace(C) = 50 per history (cond(I + C) <= 51), and the restated analysis must lower the misfit by at least 10 %
    relayout = lambda t: t.reshape(B * n_mem, G, P, D_).permute(0, 2, 1, 3)              # noqa: E731
    predict = lambda yy: restate_sensor(c["w1"], c["w2"], c["b2"], c["groups"], relayout(yy.double()), patch, cell, field, torch.zeros(B, K), None, n_mem)[1]   # noqa: E731
    y_host = y.detach().cpu()
    pred0 = predict(y_host).view(B, n_mem, K)
    obs = pred0[:, 0].to(torch.float32)
    anom = pred0 - pred0.mean(1, keepdim=True)
    trace = (base.double() * (anom * anom).sum(1) / (n_mem - 1)).sum(1, keepdim=True)
    assert bool((trace > 0).all())
    prec = (base.double() * 50.0 / trace).to(torch.float32)
    misfit = lambda pp: float((prec.double() * (pp.view(B, n_mem, K).mean(1) - obs.double()) ** 2).sum())   # noqa: E731
    D_ref, s_ref, cond = restate_enkf(pred0.view(B * n_mem, K), obs, prec, None, n_mem, 1.0, 0.5)
    y_ref = y_host.double() + restate_mix(y_host, D_ref, P)
    before, after_ref = misfit(pred0), misfit(predict(y_ref))
    print(f"enkf session: restated misfit of the ensemble mean {before:.4f} -> {after_ref:.4f}; cond(I + C) {float(cond.max()):.2f}")
    assert float(cond.max()) <= 1e4 and int(s_ref.min()) > 0 and after_ref <= 0.9 * before

    s = SensorSet(dec, P, patch, cell, field)
    ka = SensorKalman(dec, P, n_mem, s)
    obs_d, prec_d = obs.to(DEV), prec.to(DEV)
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")                                              # nothing is read back, nothing uploaded: the tables went up with the set
    try:
        ya = ka.analyse(y, obs_d, prec_d)
        D, status, _ = ka.transform(y, obs_d, prec_d)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert ya.shape == y.shape and ya.dtype == y.dtype and bool(torch.isfinite(ya.float()).all())
    assert torch.equal(status.cpu().long(), s_ref) and bool(torch.isfinite(D).all())
    after = misfit(predict(ya.detach().cpu()))
    print(f"enkf session: misfit after the analysis on the device {after:.4f}")
    assert after < before
    y2 = ens.step(conds2, state=ya)                                                       # the session takes the analysed state
    assert y2.shape == y.shape and y2.dtype == y.dtype and bool(torch.isfinite(y2.float()).all())
