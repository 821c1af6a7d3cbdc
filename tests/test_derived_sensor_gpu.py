"""Sensors that read a derived quantity on the device: sea_decode_derived_sensor_sse / _grad through Decode.sensor_sse, Decode.sensor_loss and the
consumers of a DerivedSensorSet (SensorLikelihood, SensorKalman, SensorVerification, SensorThresholdVerification).

References.  (1) The plain launch: the prediction of a derived reading is numpy-float32 dv_value arithmetic (every operation rounded once, numpy's
correctly rounded float32 root) on sea_decode_sensor_sse's predictions of its two component sensors, BIT FOR BIT — a gathered column's dot product
does not depend on its position in a tile.  (2) The fp64 restatement `restate_derived_sensor` of tests/test_derived_sensor_cpu.py, held there against
torch.autograd: with e the relative L2 error of the fused path and e_c that of the composed bf16 path (Decode.forward, a gather of both sources,
_composed_derived's float32 arithmetic, autograd), e <= 2e-2 and e <= 2 e_c + 1e-6 for wsse, pred and dz (tests/test_decode_loss_gpu.py's constants
and rule); fp32 composed: e <= 1e-4.  That file asserts that the roundings no bf16 path can avoid stay below 1e-2 on every input used here and
that no speed of the gradient inputs is near zero.

Shapes a and c of tests/test_decode_loss_gpu.py (b: plain-only), the sets of tests/test_derived_sensor_cpu.py, the splits of tests/test_sensor_cpu.py."""
import functools

import numpy as np
import pytest
import torch

from tests.test_decode_loss_cpu import rel
from tests.test_decode_loss_gpu import DEV, TOL_BF16, TOL_F32, case, decoder
from tests.test_derived_sensor_cpu import (_components, derived_obs, derived_precision, derived_sets, make_set, readings_of,
                                           restate_derived_sensor)
from tests.test_sensor_cpu import BIG, SPLITS, big_states, sensor_obs, sensor_sets

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def reference(name, set_name, members, hist, with_precision):
    c = case(name)
    patch, cell, reading = derived_sets(name)[set_name]
    prec = derived_precision(name, set_name, hist) if with_precision else None
    return restate_derived_sensor(c["w1"], c["w2"], c["b2"], c["groups"], c["z"], patch, cell, reading, derived_obs(name, set_name, hist), prec, members)


def loss_and_grad(dec, z_host, s, obs, prec, members, fused):
    """(wsse, pred, z.grad) of sum(wsse) on the device."""
    z = z_host.to(DEV).requires_grad_(True)
    wsse, pred = dec.sensor_loss(z, s, obs, precision=prec, members=members, fused=fused, predictions=True)
    assert wsse.dtype == pred.dtype == torch.float32 and wsse.shape == (z.shape[0],) and pred.shape == (z.shape[0], s.K)
    assert wsse.requires_grad and not pred.requires_grad
    wsse.sum().backward()
    return wsse.detach(), pred.detach(), z.grad.detach()


def check(name, what, got, comp, ref):
    for label, g, cc, r in (("wsse", got[0], comp[0], ref[0]), ("pred", got[1], comp[1], ref[1]), ("dz", got[2], comp[2], ref[2])):
        e, e_c = rel(g.cpu(), r), rel(cc.cpu(), r)
        print(f"derived_sensor shape {name} {what} {label}: fused e {e:.3e}; composed e_c {e_c:.3e}")
        assert e <= TOL_BF16, (what, label, e)
        assert e <= 2 * e_c + 1e-6, (what, label, e, e_c)


def numpy_dv(ya, yb, reading):
    """dv_value in numpy float32 on the component predictions ya, yb float32 [Bm, K]: every operation rounded once, numpy's float32 root."""
    _, _, op, sa, ha, sb, hb = _components(reading)
    f = lambda t: t.numpy().astype(np.float32)   # noqa: E731
    a = ya * f(sa) + f(ha)
    b = yb * f(sb) + f(hb)
    q = a * a + b * b
    opn = op.numpy()
    out = np.where(opn < 0, ya, np.where(opn == 2, a - b, np.where(opn == 1, q * np.float32(0.5), np.sqrt(q))))
    assert out.dtype == np.float32
    return out


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


# ------------------------------------------------------------------------------------------------ against the plain launch, bit for bit
@pytest.mark.parametrize("hidden", [40, 256, 384, 512, 624])
def test_predictions_are_dv_value_of_the_plain_launch_bit_for_bit(hidden):
    """One hidden width per SP form (128, 256, 384, 512, 640), 130 members (26 x 5: three row tiles, a history boundary inside a tile), segments of 1, 17
    and 35 readings: pred of a derived reading is numpy-float32 dv_value of the PLAIN launch's predictions of its two component sensors; a plain
    reading inside the derived set has the plain launch's bits; the gradient entry point writes the same wsse and pred."""
    from sea_amd.ensemble import DerivedSensorSet, SensorSet
    from sea_amd.models.encoder_decoder import Decode
    from tests.test_derived_sensor_cpu import _draw_readings

    groups, C_, D, P = [[0, 1], [2]], 12, 8, 4
    g = torch.Generator().manual_seed(1000 + hidden)
    torch.manual_seed(hidden)
    dec = Decode(groups, C_, hidden, D).requires_grad_(False).set_compute_dtype("bf16").to(DEV)
    members, hist = BIG["members"], BIG["hist"]
    z = torch.randn(members * hist, P, len(groups), D, generator=g).to(DEV)
    patch, cell, reading = _draw_readings(g, groups, C_, [(0, 0, 1), (0, 1, 17), (0, 3, 35), (1, 1, 3), (1, 2, 1)])
    K = len(patch)
    s = DerivedSensorSet(dec, P, patch, cell, readings_of(reading))
    fa, fb, op, *_ = _components(reading)
    comp = SensorSet(dec, P, patch * 2, cell * 2, fa + fb)                      # the 2 K component sensors: sources a, then sources b
    obs = (1.0 + torch.randn(hist, K, generator=g)).to(DEV)
    prec = (0.25 + torch.rand(hist, K, generator=g)).to(DEV)
    wsse, pred = dec.sensor_sse(z, s, obs, precision=prec, members=members, fused=True, predictions=True)
    _, pc = dec.sensor_sse(z, comp, torch.zeros(hist, 2 * K, device=DEV), members=members, fused=True, predictions=True)
    pc = pc.cpu().numpy()
    want = numpy_dv(pc[:, :K], pc[:, K:], reading)
    got = pred.cpu().numpy()
    plain = (op < 0).numpy()
    assert plain.sum() >= 5 and {int(o) for o in op} == {-1, 0, 1, 2}
    assert same_bits(got[:, plain], pc[:, :K][:, plain])                           # a plain reading: the plain launch's bits
    bad = int((got.view(np.uint32) != want.view(np.uint32)).sum())
    print(f"derived_sensor hidden {hidden}: {got.size} predictions, {bad} differ from numpy dv_value of the plain launch")
    assert bad == 0
    # the score from those predictions, in fp64, bounds nothing new — but the gradient entry point must give the same bits
    zz = z.clone().requires_grad_(True)
    w2, p2 = dec.sensor_loss(zz, s, obs, precision=prec, members=members, fused=True, predictions=True)
    assert torch.equal(w2.detach(), wsse) and torch.equal(p2, pred)
    o = obs.repeat_interleave(members, 0).double().cpu()
    w = prec.repeat_interleave(members, 0).double().cpu()
    assert rel(wsse.cpu(), (w * (torch.from_numpy(want).double() - o) ** 2).sum(1)) <= 1e-5


# ------------------------------------------------------------------------------------------------ against fp64
@pytest.mark.parametrize("name", ["a", "c"])
def test_fused_score_predictions_and_gradient_against_fp64(name):
    from sea_amd import ops

    c = case(name)
    dec = decoder(name, "bf16")
    for set_name in derived_sets(name):
        s = make_set(dec, name, set_name)
        for members, hist in SPLITS[name]:
            obs = derived_obs(name, set_name, hist).to(DEV)
            for with_prec in (False, True):
                prec = derived_precision(name, set_name, hist).to(DEV) if with_prec else None
                got = loss_and_grad(dec, c["z"], s, obs, prec, members, fused=True)
                comp = loss_and_grad(dec, c["z"], s, obs, prec, members, fused=False)
                check(name, f"set {set_name} members {members} x {hist} precision {with_prec}", got, comp, reference(name, set_name, members, hist, with_prec))
                # the score-only entry point: the same wsse and pred, bit for bit; fused=None is the fused path for this set
                score = dec.sensor_sse(c["z"].to(DEV), s, obs, precision=prec, members=members, fused=True, predictions=True)
                assert ops.last_form()[0] == "derived_sensor_sse.rows64"
                assert torch.equal(score[0], got[0]) and torch.equal(score[1], got[1])
                auto = dec.sensor_sse(c["z"].to(DEV), s, obs, precision=prec, members=members)
                assert torch.equal(auto, got[0])
        members, hist = SPLITS[name][-1]
        obs, prec = derived_obs(name, set_name, hist).to(DEV), derived_precision(name, set_name, hist).to(DEV)
        want = loss_and_grad(dec, c["z"], s, obs, prec, members, fused=True)
        z = c["z"].to(DEV).requires_grad_(True)
        w = dec.sensor_loss(z, s, obs, precision=prec, members=members)               # fused=None, no predictions: the same bits
        w.sum().backward()
        assert torch.equal(w.detach(), want[0]) and torch.equal(z.grad, want[2])


@pytest.mark.parametrize("name", ["a", "c"])
def test_fp32_composed_path_against_fp64(name):
    c = case(name)
    dec = decoder(name, "fp32")
    for set_name in derived_sets(name):
        s = make_set(dec, name, set_name)
        members, hist = SPLITS[name][0]
        for with_prec in (False, True):
            prec = derived_precision(name, set_name, hist).to(DEV) if with_prec else None
            wsse, pred, dz = loss_and_grad(dec, c["z"], s, derived_obs(name, set_name, hist).to(DEV), prec, members, fused=None)
            ref = reference(name, set_name, members, hist, with_prec)
            e_w, e_p, e_g = rel(wsse.cpu(), ref[0]), rel(pred.cpu(), ref[1]), rel(dz.cpu(), ref[2])
            print(f"derived_sensor shape {name} set {set_name} precision {with_prec}: fp32 e(wsse) {e_w:.3e} e(pred) {e_p:.3e} e(dz) {e_g:.3e}")
            assert e_w <= TOL_F32 and e_p <= TOL_F32 and e_g <= TOL_F32
            sse = dec.sensor_sse(c["z"].to(DEV), s, derived_obs(name, set_name, hist).to(DEV), precision=prec, members=members, predictions=True)
            assert rel(sse[0].cpu(), ref[0]) <= TOL_F32 and rel(sse[1].cpu(), ref[1]) <= TOL_F32


def test_more_than_one_row_tile_against_fp64():
    """130 members (shape a's two states repeated, 26 x 5): three row tiles per (patch, group), a history boundary inside a tile."""
    c = case("a")
    dec = decoder("a", "bf16")
    members, hist = BIG["members"], BIG["hist"]
    z_host = big_states()
    for set_name in derived_sets("a"):
        patch, cell, reading = derived_sets("a")[set_name]
        s = make_set(dec, "a", set_name)
        obs, prec = derived_obs("a", set_name, hist), derived_precision("a", set_name, hist)
        ref = restate_derived_sensor(c["w1"], c["w2"], c["b2"], c["groups"], z_host, patch, cell, reading, obs, prec, members)
        got = loss_and_grad(dec, z_host, s, obs.to(DEV), prec.to(DEV), members, fused=True)
        comp = loss_and_grad(dec, z_host, s, obs.to(DEV), prec.to(DEV), members, fused=False)
        check("a", f"130 rows set {set_name}", got, comp, ref)
        for bm in (0, 63, 64, 77, 78, 129):                                              # a member alone against its history's readings: the same bits
            b = bm // members
            alone = loss_and_grad(dec, z_host[bm:bm + 1], s, obs[b:b + 1].to(DEV), prec[b:b + 1].to(DEV), 1, fused=True)
            assert torch.equal(alone[2][0], got[2][bm]) and torch.equal(alone[0], got[0][bm:bm + 1]) and torch.equal(alone[1][0], got[1][bm]), (set_name, bm)


# ------------------------------------------------------------------------------------------------ the other properties
@pytest.mark.parametrize("name", ["a", "c"])
def test_bits_do_not_depend_on_the_run_the_members_or_the_histories(name):
    from sea_amd import ops

    c = case(name)
    dec = decoder(name, "bf16")
    for set_name in derived_sets(name):
        s = make_set(dec, name, set_name)
        for members, hist in SPLITS[name]:
            obs, prec = derived_obs(name, set_name, hist).to(DEV), derived_precision(name, set_name, hist).to(DEV)
            a = loss_and_grad(dec, c["z"], s, obs, prec, members, fused=True)
            b = loss_and_grad(dec, c["z"], s, obs, prec, members, fused=True)
            assert all(torch.equal(x, y) for x, y in zip(a, b))                          # two runs are equal
            one = loss_and_grad(dec, c["z"], s, obs.repeat_interleave(members, dim=0), prec.repeat_interleave(members, dim=0), 1, fused=True)
            assert all(torch.equal(x, y) for x, y in zip(a, one)), (set_name, members, hist)
            for h in sorted({0, hist - 1}):                                              # a history alone equals the same history in company
                rows = slice(h * members, (h + 1) * members)
                alone = loss_and_grad(dec, c["z"][rows], s, obs[h:h + 1], prec[h:h + 1], members, fused=True)
                assert all(torch.equal(x, y[rows]) for x, y in zip(alone, a)), (set_name, members, hist, h)
    # the entry point itself, on the last set and split: every element of dH and of pred is written (no NaN of the fill survives)
    z = c["z"].to(DEV)
    T = s.tables(z.device)
    hid, pre = dec._first_layer(z.index_select(1, T["patches"]).permute(1, 0, 2, 3), torch.bfloat16)
    _, W2 = dec._weights(torch.bfloat16)
    dpre = [torch.full_like(h, float("nan")) for h in hid]
    _, pred = ops.decode_derived_sensor_grad([dict(H=hid[g], W2=W2[g], bias=dec._shadow[3][g], dH=dpre[g], Z=pre[g]) for g in range(len(hid))],
                                             obs.index_select(1, T["perm"]), T["live"], T["wrow"], T["seg"], T["op"], T["scale"], T["shift"], dec._n_inp_p,
                                             members=members, predictions=True)
    assert ops.last_form()[0] == "derived_sensor_grad.rows64"
    assert all(bool(torch.isfinite(d.float()).all()) for d in dpre) and bool(torch.isfinite(pred).all())
    assert torch.equal(pred[:, 0::2], pred[:, 1::2])                                     # pred[2 i] = pred[2 i + 1] = x


def test_neutral_readings_exact_zeros_and_a_zero_speed():
    from sea_amd.ensemble import DerivedField, DerivedSensorSet

    name = "a"
    c = case(name)
    dec = decoder(name, "bf16")
    groups, P = c["groups"], c["P"]
    members, hist = SPLITS[name][0]
    # dH is exactly 0 at unobserved patches and groups
    for set_name in ("g0", "one", "segments"):
        patch, cell, reading = derived_sets(name)[set_name]
        s = make_set(dec, name, set_name)
        fa = _components(reading)[0]
        _, _, dz = loss_and_grad(dec, c["z"], s, derived_obs(name, set_name, hist).to(DEV), None, members, fused=True)
        seen = {(0 if f < 2 else 1, p) for p, f in zip(patch, fa)}
        n_zero = 0
        for g in range(len(groups)):
            for p in range(P):
                if (g, p) not in seen:
                    assert float(dz[:, p, g].abs().max()) == 0.0, (set_name, g, p)
                    n_zero += 1
                else:
                    assert float(dz[:, p, g].abs().max()) > 0.0
        assert n_zero >= 1 and bool(torch.isfinite(dz).all())
    # a precision 0, or NaN / Inf in obs under precision 0, changes no bit of the score or of the gradient
    set_name = "segments"
    s = make_set(dec, name, set_name)
    obs, wd = derived_obs(name, set_name, hist).to(DEV), derived_precision(name, set_name, hist).to(DEV)
    dead = wd == 0
    n_dead = int(dead.sum())
    assert n_dead >= 8
    base = loss_and_grad(dec, c["z"], s, obs, wd, members, fused=True)
    dirty = obs.clone()
    dirty[dead] = torch.tensor([float("nan"), float("inf"), -float("inf"), 3e38], device=DEV).repeat(n_dead // 4 + 1)[:n_dead]
    got = loss_and_grad(dec, c["z"], s, dirty, wd, members, fused=True)
    assert torch.equal(got[0], base[0]) and torch.equal(got[2], base[2]) and bool(torch.isfinite(got[2]).all())
    sse = dec.sensor_sse(c["z"].to(DEV), s, dirty, precision=wd, members=members, fused=True)
    assert torch.equal(sse, base[0])
    comp = loss_and_grad(dec, c["z"], s, dirty, wd, members, fused=False)
    assert bool(torch.isfinite(comp[2]).all()) and rel(comp[2].cpu(), reference(name, set_name, members, hist, True)[2]) <= TOL_BF16
    zero = loss_and_grad(dec, c["z"], s, dirty, torch.zeros_like(wd), members, fused=True)
    assert float(zero[0].abs().max()) == 0.0 and float(zero[2].abs().max()) == 0.0
    # x = 0 at a magnitude reading (zero scales and shifts): a finite contribution to the score, exactly none to the gradient
    s0 = DerivedSensorSet(dec, P, [3, 3], [5, 5], [DerivedField("magnitude", 0, 1, 0.0, 0.0, 0.0, 0.0), 2])
    o0 = torch.ones(hist, 2, device=DEV)
    for fused in (True, False):
        wsse, pred, dz = loss_and_grad(dec, c["z"], s0, o0, None, members, fused=fused)
        assert float(pred[:, 0].abs().max()) == 0.0 and bool(torch.isfinite(wsse).all()) and bool(torch.isfinite(dz).all())
        assert float(dz[:, 3, 0].abs().max()) == 0.0 and float(dz[:, 3, 1].abs().max()) > 0.0, fused
    only = DerivedSensorSet(dec, P, [3], [5], [DerivedField("magnitude", 0, 1, 0.0, 0.0, 0.0, 0.0)])
    wsse, pred, dz = loss_and_grad(dec, c["z"], only, o0[:, :1].contiguous(), None, members, fused=True)
    assert torch.equal(wsse, torch.ones_like(wsse)) and float(dz.abs().max()) == 0.0


def test_plain_only_set_and_cross_group_readings_on_shape_b():
    """Three one-field groups: a plain-only DerivedSensorSet has the bits of the SensorSet on the same sensors; a derived reading pairs two groups
    there, so fused=True is refused and fused=None takes the composed path."""
    from sea_amd.ensemble import DerivedField, DerivedSensorSet, SensorSet

    name = "b"
    c = case(name)
    dec = decoder(name, "bf16")
    patch, cell, field = sensor_sets(name)["segments"]
    members, hist = SPLITS[name][0]
    obs = sensor_obs(name, "segments", hist).to(DEV)
    plain, ds = SensorSet(dec, c["P"], patch, cell, field), DerivedSensorSet(dec, c["P"], patch, cell, list(field))
    z = c["z"].to(DEV)
    a = dec.sensor_sse(z, plain, obs, members=members, fused=True, predictions=True)
    b = dec.sensor_sse(z, ds, obs, members=members, fused=True, predictions=True)
    assert torch.equal(a[1], b[1]) and rel(b[0].cpu(), a[0].cpu()) <= 1e-5           # the same predictions; the sum runs over other tiles
    ga = loss_and_grad(dec, c["z"], ds, obs, None, members, fused=True)
    gp = loss_and_grad(dec, c["z"], plain, obs, None, members, fused=True)
    assert torch.equal(ga[1], gp[1]) and rel(ga[2].cpu(), gp[2].cpu()) <= TOL_BF16
    cross = DerivedSensorSet(dec, c["P"], [0, 1, 3], [3, 4, c["n_inp"] - 1], [DerivedField("magnitude", 0, 1, 0.5, 3.0, 0.5, -3.0), 2,
                                                                              DerivedField("difference", 2, 0)])
    o3 = torch.ones(hist, 3, device=DEV)
    for fn in (dec.sensor_sse, dec.sensor_loss):
        with pytest.raises(ValueError, match="different decoder groups"):
            fn(z, cross, o3, members=members, fused=True)
    got = loss_and_grad(dec, c["z"], cross, o3, None, members, fused=None)             # the composed path
    reading = [("magnitude", 0, 1, 0.5, 3.0, 0.5, -3.0), 2, ("difference", 2, 0, 1.0, 0.0, 1.0, 0.0)]
    ref = restate_derived_sensor(c["w1"], c["w2"], c["b2"], c["groups"], c["z"], [0, 1, 3], [3, 4, c["n_inp"] - 1], reading, torch.ones(hist, 3), None, members)
    assert all(rel(g.cpu(), r) <= TOL_BF16 for g, r in zip(got, ref))


# ------------------------------------------------------------------------------------------------ end to end on a forked rollout session
def test_a_mixed_rig_on_a_forked_rollout_session():
    """Pressure-tap-like plain readings plus speed, energy and difference probes on a forked RolloutSession: weight and resample; the Kalman analysis
    against _composed_transform / _composed_mix on the same predictions (the bound of tests/test_enkf_gpu.py for D on given predictions); verification
    from predictions equals the call; a small nudge raises every member's own log-weight."""
    from sea_amd.ensemble import (DerivedSensorSet, SensorKalman, SensorLikelihood, SensorThresholdVerification, SensorVerification, _composed_mix,
                                  _composed_transform, systematic_resample)
    from oracle.recipe import recipe_inputs
    from tests.test_derived_sensor_cpu import _draw_readings
    from tests.test_input_grad_gpu import cfg_of
    from tests.test_model_gpu import build
    from tests.test_rollout_session_gpu import open_on

    c = case("a")
    P, D, n_mem, B, k = 4, c["D"], 8, 2, 3
    G = len(c["groups"])
    cfg = cfg_of(1, P * D, 4, G)
    m = build(cfg, "bf16")
    x, _, ib = recipe_inputs(B, k + 4, cfg, seed=9)
    dec = decoder("a", "bf16")
    g = torch.Generator().manual_seed(31)
    patch, cell, reading = _draw_readings(g, c["groups"], c["n_inp"], [(0, 0, 5), (0, 3, 17), (1, 2, 4)])
    K = len(patch)
    assert {-1, 0, 1, 2} == {int(o) for o in _components(reading)[2]}
    prec = 0.5 + torch.rand(B, K, generator=g)
    prec[torch.rand(B, K, generator=g) < 0.2] = 0.0
    prec[:, 0] = 1.0
    conds = torch.rand(B * n_mem, 1, generator=g).to(DEV)
    conds2 = torch.rand(B * n_mem, 1, generator=g).to(DEV)
    s = DerivedSensorSet(dec, P, patch, cell, readings_of(reading))

    ens = open_on(m, x, ib, k).fork(n_mem)
    y = ens.step(conds)                                                                   # [16, 2, 64]
    relayout = lambda t: t.reshape(B * n_mem, G, P, D).permute(0, 2, 1, 3)              # noqa: E731
    restate = lambda zz, o: restate_derived_sensor(c["w1"], c["w2"], c["b2"], c["groups"], zz, patch, cell, reading, o, prec, n_mem)   # noqa: E731
    z0 = relayout(y.detach().cpu().double())
    pred0 = restate(z0, torch.zeros(B, K))[1].view(B, n_mem, K)
    obs = (pred0[:, 0] + 0.05 * torch.randn(B, K, generator=g).double()).to(torch.float32)   # member 0's readings plus noise: a truth inside the span
    obs_d, prec_d = obs.to(DEV), prec.to(DEV)

    # weight -> resample
    like = SensorLikelihood(dec, P, n_mem, s, sigma=0.5)
    logw = like(y, obs_d, prec_d)
    w_ref = restate(z0, obs)[0]
    e = rel(logw.cpu(), -0.5 * w_ref / 0.25)
    print(f"derived_sensor session: log-weights against fp64 {e:.3e}")
    assert e <= TOL_BF16
    idx, _, ess, resampled = systematic_resample(logw, n_mem, u=torch.full((B,), 0.5, device=DEV))
    assert idx.shape[0] == B * n_mem and bool(((idx // n_mem) == torch.arange(B, device=DEV).repeat_interleave(n_mem)).all())
    assert bool((resampled == 1).all()) and bool((ess >= 1).all()) and bool((ess <= n_mem).all())

    # verification: from_predictions(pred) equals __call__
    _, pred = dec.sensor_sse(relayout(y), s, obs_d, precision=prec_d, members=n_mem, predictions=True)
    ver = SensorVerification(dec, P, n_mem, s, sigma=0.5)
    sc_a, sc_b = ver(y, obs_d, prec_d), ver.from_predictions(pred, obs_d, prec_d)
    assert torch.equal(sc_a.sums, sc_b.sums) and torch.equal(sc_a.hist, sc_b.hist) and bool(torch.isfinite(sc_a.mean_crps).all())
    thr = SensorThresholdVerification(dec, P, n_mem, s, [0.5, 2.0])
    br_a, br_b = thr(y, obs_d, prec_d), thr.from_predictions(pred, obs_d, prec_d)
    assert torch.equal(br_a.sums, br_b.sums) and bool(torch.isfinite(br_a.brier).all())

    # Kalman analysis against the composed transform and mix on the same predictions
    ka = SensorKalman(dec, P, n_mem, s, sigma=0.5)
    D_, status, kpred = ka.transform(y, obs_d, prec_d)
    assert torch.equal(kpred, pred)
    D_ref, s_ref = _composed_transform(pred, obs_d, prec_d * 4.0, None, n_mem, 1.0, 0.5)
    err, bound = float((D_.double() - D_ref.double()).abs().max()), 1e-6 * max(1.0, float(D_ref.abs().max()))
    print(f"derived_sensor session: max |D - D_composed| {err:.3e} (bound {bound:.3e})")
    assert err <= bound and torch.equal(status.long().cpu().view(-1), s_ref.long().cpu().view(-1))
    ya = ka.analyse(y, obs_d, prec_d)
    ya_ref = y.float() + _composed_mix(y, D_ref, P)
    assert ya.shape == y.shape and ya.dtype == y.dtype and rel(ya.float().cpu(), ya_ref.cpu()) <= TOL_BF16
    # ... and with a taper [P, K] (one domain per patch; patch 1 sees no reading: no update there), the same bound on the same predictions
    taper = torch.rand(P, K, generator=torch.Generator().manual_seed(32))
    taper[1] = 0.0
    kt = SensorKalman(dec, P, n_mem, s, sigma=0.5, taper=taper)
    Dt, st, tpred = kt.transform(y, obs_d, prec_d)
    Dt_ref, st_ref = _composed_transform(pred, obs_d, prec_d * 4.0, taper.to(DEV), n_mem, 1.0, 0.5)
    err_t, bound_t = float((Dt.double() - Dt_ref.double()).abs().max()), 1e-6 * max(1.0, float(Dt_ref.abs().max()))
    print(f"derived_sensor session: with a taper max |D - D_composed| {err_t:.3e} (bound {bound_t:.3e})")
    assert torch.equal(tpred, pred) and tuple(Dt.shape) == (B, P, n_mem, n_mem) and err_t <= bound_t and torch.equal(st.long().cpu(), st_ref.long().cpu())
    assert int(st[:, 1].abs().max()) == 0 and int(st[:, 0].min()) > 0
    yat = kt.analyse(y, obs_d, prec_d)
    assert yat.shape == y.shape and rel(yat.float().cpu(), (y.float() + _composed_mix(y, Dt_ref, P)).cpu()) <= TOL_BF16

    # nudge: a small step raises every member's own log-weight (the rate halved on the host, from the restatement, until every member gains)
    _, _, dz0 = restate(z0, obs)
    w0 = restate(z0, obs)[0]
    rate = 0.25
    while rate > 1e-7 and not bool((restate(z0 + rate * (-0.5 * dz0) / 0.25, obs)[0] < w0).all()):
        rate *= 0.5
    assert rate > 1e-7
    rate *= 0.5
    y1 = like.nudge(y, obs_d, prec_d, rate=rate)
    lw0, grad = like.score_and_grad(y, obs_d, prec_d)
    # the session's states are not the fixture's (larger, and squared by the energy readings): the gradient is held to the composed bf16 path by the
    # usual rule and to twice the envelope of the roundings no bf16 path can avoid ON THESE inputs (tests/test_enkf_gpu.py's rule for its session)
    g_ref = (-0.5 * dz0 / 0.25).permute(0, 2, 1, 3).reshape(y.shape)
    env = rel(restate_derived_sensor(c["w1"], c["w2"], c["b2"], c["groups"], z0, patch, cell, reading, obs, prec, n_mem, round_bf16=True)[2], dz0)
    _, grad_c = SensorLikelihood(dec, P, n_mem, s, sigma=0.5, fused=False).score_and_grad(y, obs_d, prec_d)
    e, e_c = rel(grad.cpu(), g_ref), rel(grad_c.cpu(), g_ref)
    print(f"derived_sensor session: dlogw/dy fused e {e:.3e}; composed e_c {e_c:.3e}; bf16 rounding envelope {env:.3e}")
    assert torch.equal(lw0, logw) and e <= 2 * e_c + 1e-6 and e <= 2 * env, (e, e_c, env)
    dec32 = decoder("a", "fp32")
    s32 = DerivedSensorSet(dec32, P, patch, cell, readings_of(reading))
    score = lambda t: -0.5 * dec32.sensor_sse(relayout(t.float()), s32, obs_d, precision=prec_d * 4.0, members=n_mem, fused=False)   # noqa: E731
    before, after = score(y), score(y1)
    print(f"derived_sensor session: nudge at rate {rate:g}: log-weights rise by {float((after - before).min()):.3e} .. {float((after - before).max()):.3e}")
    assert bool((after > before).all())
    ens.resample(idx)                                                                     # the session takes the resampled, nudged states
    y2 = ens.step(conds2, state=y1.index_select(0, idx.long()))
    assert y2.shape == y.shape and bool(torch.isfinite(y2.float()).all())
    ens.close()
