"""The latent gradient of the sparse-sensor score on the device: sea_decode_sensor_grad through Decode.sensor_loss, SensorLikelihood.score_and_grad and
SensorLikelihood.nudge.

Reference: the fp64 restatement `restate_sensor_grad` of tests/test_sensor_grad_cpu.py, which that file holds against torch.autograd and ties to the
reference-generated goldens.  Let e be the relative L2 error of the fused path against it and e_c that of the composed bf16 path (Decode.forward
under autograd, a gather, torch reductions) on the same inputs, for the scores wsse [Bm], the predictions pred [Bm, K] and the gradient dz [Bm, P,
G, D]: e <= 2e-2 (the bf16 decode tolerance) and e <= 2 e_c + 1e-6 (tests/test_decode_loss_gpu.py's constants and rule); fp32
(composed): e <= 1e-4.  tests/test_sensor_grad_cpu.py asserts that the roundings no bf16 path can avoid stay below 1e-2 on every input used here.

Shapes a, b, c of tests/test_decode_loss_gpu.py; sensor sets, readings, precisions and (members, histories) splits of tests/test_sensor_cpu.py."""
import functools

import pytest
import torch

from tests.test_decode_loss_cpu import rel
from tests.test_decode_loss_gpu import DEV, TOL_BF16, TOL_F32, case, decoder, device_target
from tests.test_sensor_cpu import BIG, SPLITS, _draw, big_states, sensor_obs, sensor_precision, sensor_sets
from tests.test_sensor_grad_cpu import restate_sensor_grad

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def reference(name, set_name, members, hist, with_precision):
    c = case(name)
    patch, cell, field = sensor_sets(name)[set_name]
    prec = sensor_precision(name, set_name, hist) if with_precision else None
    return restate_sensor_grad(c["w1"], c["w2"], c["b2"], c["groups"], c["z"], patch, cell, field, sensor_obs(name, set_name, hist), prec, members)


def sensor_set(dec, name, set_name):
    from sea_amd.ensemble import SensorSet

    return SensorSet(dec, case(name)["P"], *sensor_sets(name)[set_name])


def loss_and_grad(dec, z_host, s, obs, prec, members, fused, upstream=None):
    """(wsse, pred, z.grad) of sum(wsse) — or of sum(wsse * upstream) — on the device."""
    z = z_host.to(DEV).requires_grad_(True)
    wsse, pred = dec.sensor_loss(z, s, obs, precision=prec, members=members, fused=fused, predictions=True)
    assert wsse.dtype == pred.dtype == torch.float32 and wsse.shape == (z.shape[0],) and pred.shape == (z.shape[0], s.K)
    assert wsse.requires_grad and not pred.requires_grad
    (wsse.sum() if upstream is None else (wsse * upstream).sum()).backward()
    assert z.grad.shape == z.shape and z.grad.dtype == z.dtype
    return wsse.detach(), pred.detach(), z.grad.detach()


def check(name, what, got, comp, ref):
    for label, g, cc, r in (("wsse", got[0], comp[0], ref[0]), ("pred", got[1], comp[1], ref[1]), ("dz", got[2], comp[2], ref[2])):
        e, e_c = rel(g.cpu(), r), rel(cc.cpu(), r)
        print(f"sensor_loss shape {name} {what} {label}: fused e {e:.3e}; composed e_c {e_c:.3e}")
        assert e <= TOL_BF16, (what, label, e)
        assert e <= 2 * e_c + 1e-6, (what, label, e, e_c)


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_fused_sensor_loss_and_gradient_against_fp64(name):
    c = case(name)
    dec = decoder(name, "bf16")
    for set_name in sensor_sets(name):
        s = sensor_set(dec, name, set_name)
        for members, hist in SPLITS[name]:
            obs = sensor_obs(name, set_name, hist).to(DEV)
            for with_prec in (False, True):
                prec = sensor_precision(name, set_name, hist).to(DEV) if with_prec else None
                got = loss_and_grad(dec, c["z"], s, obs, prec, members, fused=True)
                comp = loss_and_grad(dec, c["z"], s, obs, prec, members, fused=False)
                check(name, f"set {set_name} members {members} x {hist} precision {with_prec}", got, comp, reference(name, set_name, members, hist, with_prec))
        # fused=None is the fused path in bf16, and without the predictions the score and the gradient are the same bits (last split, with precision)
        members, hist = SPLITS[name][-1]
        obs, prec = sensor_obs(name, set_name, hist).to(DEV), sensor_precision(name, set_name, hist).to(DEV)
        want = loss_and_grad(dec, c["z"], s, obs, prec, members, fused=True)
        z = c["z"].to(DEV).requires_grad_(True)
        w = dec.sensor_loss(z, s, obs, precision=prec, members=members)
        w.sum().backward()
        assert torch.equal(w.detach(), want[0]) and torch.equal(z.grad, want[2])


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_fp32_composed_sensor_loss_against_fp64(name):
    c = case(name)
    dec = decoder(name, "fp32")
    for set_name in sensor_sets(name):
        s = sensor_set(dec, name, set_name)
        members, hist = SPLITS[name][0]
        for with_prec in (False, True):
            prec = sensor_precision(name, set_name, hist).to(DEV) if with_prec else None
            wsse, pred, dz = loss_and_grad(dec, c["z"], s, sensor_obs(name, set_name, hist).to(DEV), prec, members, fused=None)
            ref = reference(name, set_name, members, hist, with_prec)
            e_w, e_p, e_g = rel(wsse.cpu(), ref[0]), rel(pred.cpu(), ref[1]), rel(dz.cpu(), ref[2])
            print(f"sensor_loss shape {name} set {set_name} precision {with_prec}: fp32 e(wsse) {e_w:.3e} e(pred) {e_p:.3e} e(dz) {e_g:.3e}")
            assert e_w <= TOL_F32 and e_p <= TOL_F32 and e_g <= TOL_F32


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_score_and_predictions_are_the_bits_of_sensor_sse(name):
    from sea_amd.ensemble import SensorLikelihood

    c = case(name)
    dec = decoder(name, "bf16")
    z = c["z"].to(DEV)
    P, G, D = c["P"], len(c["groups"]), c["D"]
    for set_name in sensor_sets(name):
        s = sensor_set(dec, name, set_name)
        for members, hist in SPLITS[name]:
            obs = sensor_obs(name, set_name, hist).to(DEV)
            for prec in (None, sensor_precision(name, set_name, hist).to(DEV)):
                score = dec.sensor_sse(z, s, obs, precision=prec, members=members, fused=True, predictions=True)
                got = dec.sensor_loss(z.clone().requires_grad_(True), s, obs, precision=prec, members=members, fused=True, predictions=True)
                assert torch.equal(got[0].detach(), score[0]) and torch.equal(got[1], score[1]), (set_name, members, hist)
                with torch.no_grad():   # no gradient wanted: the same launch, the same bits
                    ng = dec.sensor_loss(z, s, obs, precision=prec, members=members, fused=True)
                assert torch.equal(ng, score[0]) and not ng.requires_grad
        members, hist = SPLITS[name][0]
        y = z.permute(0, 2, 1, 3).reshape(z.shape[0], G, P * D).contiguous()            # the layout RolloutSession.step returns
        sigma = [0.5 + 0.25 * f for f in range(sum(len(g) for g in c["groups"]))]
        like = SensorLikelihood(dec, P, members, s, sigma=sigma)
        obs, prec = sensor_obs(name, set_name, hist).to(DEV), sensor_precision(name, set_name, hist).to(DEV)
        logw, grad = like.score_and_grad(y, obs, prec)
        assert torch.equal(logw, like(y, obs, prec)) and grad.shape == y.shape and grad.dtype == torch.float32 and not grad.requires_grad
        # the gradient in y's layout is -0.5 dz of sensor_loss with the folded precision
        zz = z.clone().requires_grad_(True)
        dec.sensor_loss(zz, s, obs, precision=prec * like._sigma_precision(torch.device(DEV)), members=members, fused=True).sum().backward()
        assert torch.equal(grad, (-0.5 * zz.grad).permute(0, 2, 1, 3).reshape(y.shape))


@pytest.mark.parametrize("name", ["a", "b"])
def test_exact_zeros_neutral_readings_and_the_upstream_gradient(name):
    c = case(name)
    dec = decoder(name, "bf16")
    groups, P = c["groups"], c["P"]
    grp_of = {f: g for g, grp in enumerate(groups) for f in grp}
    members, hist = SPLITS[name][0]
    for set_name in ("last", "one", "segments"):
        patch, cell, field = sensor_sets(name)[set_name]
        s = sensor_set(dec, name, set_name)
        obs = sensor_obs(name, set_name, hist).to(DEV)
        _, _, dz = loss_and_grad(dec, c["z"], s, obs, None, members, fused=True)
        _, _, dz_c = loss_and_grad(dec, c["z"], s, obs, None, members, fused=False)
        seen = {(grp_of[f], p) for p, f in zip(patch, field)}
        n_zero = 0
        for g in range(len(groups)):
            for p in range(P):
                if (g, p) not in seen:
                    assert float(dz[:, p, g].abs().max()) == 0.0 and float(dz_c[:, p, g].abs().max()) == 0.0, (set_name, g, p)
                    n_zero += 1
                else:
                    assert float(dz[:, p, g].abs().max()) > 0.0
        assert n_zero >= 1 and bool(torch.isfinite(dz).all())
    # readings without weight: NaN / Inf there change no bit of the score or of the gradient
    set_name = "segments"
    s = sensor_set(dec, name, set_name)
    obs, wd = sensor_obs(name, set_name, hist).to(DEV), sensor_precision(name, set_name, hist).to(DEV)
    dead = wd == 0
    n_dead = int(dead.sum())
    assert n_dead >= 8
    base = loss_and_grad(dec, c["z"], s, obs, wd, members, fused=True)
    dirty = obs.clone()
    dirty[dead] = torch.tensor([float("nan"), float("inf"), -float("inf"), 3e38], device=DEV).repeat(n_dead // 4 + 1)[:n_dead]
    got = loss_and_grad(dec, c["z"], s, dirty, wd, members, fused=True)
    assert torch.equal(got[0], base[0]) and torch.equal(got[2], base[2]) and bool(torch.isfinite(got[2]).all())
    comp = loss_and_grad(dec, c["z"], s, dirty, wd, members, fused=False)
    assert bool(torch.isfinite(comp[2]).all()) and rel(comp[2].cpu(), reference(name, set_name, members, hist, True)[2]) <= TOL_BF16
    # ... and equal the call on the set without those sensors (one history: a [K] subset is one set for every row)
    if hist == 1:
        from sea_amd.ensemble import SensorSet

        keep = [k for k in range(s.K) if float(wd[0, k]) > 0]
        patch, cell, field = sensor_sets(name)[set_name]
        sub = SensorSet(dec, P, [patch[k] for k in keep], [cell[k] for k in keep], [field[k] for k in keep])
        kk = torch.tensor(keep, device=DEV)
        lean = loss_and_grad(dec, c["z"], sub, obs[:, kk].contiguous(), wd[:, kk].contiguous(), members, fused=True)
        assert rel(lean[2].cpu(), base[2].cpu()) <= TOL_BF16 and rel(lean[0].cpu(), base[0].cpu()) <= 1e-5   # other tiles, another summation order: not the same bits
    zero = loss_and_grad(dec, c["z"], s, dirty, torch.zeros_like(wd), members, fused=True)
    assert float(zero[0].abs().max()) == 0.0 and float(zero[2].abs().max()) == 0.0
    # a non-uniform upstream gradient scales every member's dz: the bits of the unit-gradient result times c[bm]
    cvec = torch.randn(c["z"].shape[0], generator=torch.Generator().manual_seed(5)).to(DEV)
    scaled = loss_and_grad(dec, c["z"], s, obs, wd, members, fused=True, upstream=cvec)
    assert torch.equal(scaled[0], base[0]) and torch.equal(scaled[2], base[2] * cvec.view(-1, 1, 1, 1))


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_bits_do_not_depend_on_the_run_the_members_or_the_histories(name):
    from sea_amd import ops

    c = case(name)
    dec = decoder(name, "bf16")
    for set_name in sensor_sets(name):
        s = sensor_set(dec, name, set_name)
        for members, hist in SPLITS[name]:
            obs = sensor_obs(name, set_name, hist).to(DEV)
            prec = sensor_precision(name, set_name, hist).to(DEV)
            a = loss_and_grad(dec, c["z"], s, obs, prec, members, fused=True)
            b = loss_and_grad(dec, c["z"], s, obs, prec, members, fused=True)
            assert all(torch.equal(x, y) for x, y in zip(a, b))
            # every member alone against its history's readings
            one = loss_and_grad(dec, c["z"], s, obs.repeat_interleave(members, dim=0), prec.repeat_interleave(members, dim=0), 1, fused=True)
            assert all(torch.equal(x, y) for x, y in zip(a, one)), (set_name, members, hist)
            # a history on its own: (members, 1) against one of `hist` histories
            for h in sorted({0, hist - 1}):
                rows = slice(h * members, (h + 1) * members)
                alone = loss_and_grad(dec, c["z"][rows], s, obs[h:h + 1], prec[h:h + 1], members, fused=True)
                assert all(torch.equal(x, y[rows]) for x, y in zip(alone, a)), (set_name, members, hist, h)
    # the entry point itself, on the last set and split: the form it notes, and every element of dH written (no NaN of the fill survives)
    z = c["z"].to(DEV)
    T = s.tables(z.device)
    hid, pre = dec._first_layer(z.index_select(1, T["patches"]).permute(1, 0, 2, 3), torch.bfloat16)
    _, W2 = dec._weights(torch.bfloat16)
    dpre = [torch.full_like(h, float("nan")) for h in hid]
    ops.decode_sensor_grad([dict(H=hid[g], W2=W2[g], bias=dec._shadow[3][g], dH=dpre[g], Z=pre[g]) for g in range(len(hid))], obs.index_select(1, T["perm"]), T["live"],
                           T["wrow"], T["seg"], dec._n_inp_p, members=members)
    assert ops.last_form()[0] == "sensor_grad.rows64"
    assert all(bool(torch.isfinite(d.float()).all()) for d in dpre)


def test_more_than_one_row_tile():
    """130 members (shape a's two states repeated 65 times, 26 members x 5 histories): three 64-member row tiles per (patch, group), the last with two
    rows, a history boundary inside a tile.  The fused path is held against fp64 with the bounds above; member 0's dz equals its dz in the 2-member call."""
    c = case("a")
    dec = decoder("a", "bf16")
    members, hist = BIG["members"], BIG["hist"]
    z_host = big_states()
    for set_name in sensor_sets("a"):
        patch, cell, field = sensor_sets("a")[set_name]
        s = sensor_set(dec, "a", set_name)
        obs, prec = sensor_obs("a", set_name, hist), sensor_precision("a", set_name, hist)
        ref = restate_sensor_grad(c["w1"], c["w2"], c["b2"], c["groups"], z_host, patch, cell, field, obs, prec, members)
        got = loss_and_grad(dec, z_host, s, obs.to(DEV), prec.to(DEV), members, fused=True)
        comp = loss_and_grad(dec, z_host, s, obs.to(DEV), prec.to(DEV), members, fused=False)
        assert got[2].shape == (130,) + tuple(c["z"].shape[1:])
        check("a", f"130 rows set {set_name}", got, comp, ref)
        two = loss_and_grad(dec, c["z"], s, obs[:1].to(DEV), prec[:1].to(DEV), 2, fused=True)
        assert torch.equal(got[2][0], two[2][0]) and torch.equal(got[2][1], two[2][1]) and torch.equal(got[0][:2], two[0])
        for bm in (63, 64, 77, 78, 128, 129):                                              # a member alone against its history's readings: the same bits
            b = bm // members
            alone = loss_and_grad(dec, z_host[bm:bm + 1], s, obs[b:b + 1].to(DEV), prec[b:b + 1].to(DEV), 1, fused=True)
            assert torch.equal(alone[2][0], got[2][bm]) and torch.equal(alone[0], got[0][bm:bm + 1]), (set_name, bm)


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_every_cell_as_sensors_is_the_dense_launch(name):
    """All valid cells of all fields as sensors, unit precision, members = 1, readings = the dense target: d sum(wsse) / dz / n against
    Decode.mse_loss(fused=True)'s gradient.  The two launches round different residual tiles: the bound is TOL_BF16, not bit equality."""
    from sea_amd.ensemble import SensorSet

    c = case(name)
    dec = decoder(name, "bf16")
    tgt = device_target(name)
    P, C_, B = c["P"], c["n_inp"], c["B"]
    fields = [f for g in c["groups"] for f in g]
    for counts in (None, c["counts"]):
        patch, cell, field, col = [], [], [], []
        for p in range(P):
            for j, f in enumerate(fields):
                for cc in range(C_ if counts is None else counts[p]):
                    patch.append(p), cell.append(cc), field.append(f), col.append(j)
        n = B * len(patch)
        s = SensorSet(dec, P, patch, cell, field)
        obs = c["target"][:, torch.tensor(patch), torch.tensor(col), torch.tensor(cell)].contiguous().to(DEV)      # [B, K]: members = 1
        wsse, _, dz = loss_and_grad(dec, c["z"], s, obs, None, 1, fused=True)
        z = c["z"].to(DEV).requires_grad_(True)
        loss = dec.mse_loss(z, tgt, counts=counts, fused=True)
        loss.backward()
        e_g, e_l = rel(dz.cpu() / n, z.grad.cpu()), rel(wsse.sum().cpu() / n, loss.detach().cpu())
        print(f"sensor_loss shape {name} counts {counts is not None}: every cell as a sensor against the dense launch e(dz) {e_g:.3e} e(loss) {e_l:.3e}")
        assert e_g <= TOL_BF16 and e_l <= TOL_BF16


def test_nudge_on_a_rollout_session():
    """One gradient step on the log-likelihood of the readings lowers the score, and the session takes the nudged state."""
    from sea_amd.ensemble import SensorLikelihood, SensorSet
    from oracle.recipe import recipe_inputs
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
    g = torch.Generator().manual_seed(12)
    patch, cell, field = _draw(g, c["groups"], c["n_inp"], [(0, 0, 5), (0, 3, 33), (1, 2, 4)])
    K = len(patch)
    obs = torch.randn(B, K, generator=g)
    prec = 0.5 + torch.rand(B, K, generator=g)
    prec[torch.rand(B, K, generator=g) < 0.2] = 0.0
    conds = torch.rand(B * n_mem, 1, generator=g).to(DEV)
    conds2 = torch.rand(B * n_mem, 1, generator=g).to(DEV)

    ens = open_on(m, x, ib, k).fork(n_mem)
    y = ens.step(conds)                                                                   # [16, 2, 64]
    s = SensorSet(dec, P, patch, cell, field)
    like = SensorLikelihood(dec, P, n_mem, s)
    obs_d, prec_d = obs.to(DEV), prec.to(DEV)

    # the step length, on the host, from the fp64 restatement: halved until one step lowers the restated sum(wsse) by at least 10 %
    relayout = lambda t: t.reshape(B * n_mem, G, P, D).permute(0, 2, 1, 3)              # noqa: E731
    restate = lambda zz: restate_sensor_grad(c["w1"], c["w2"], c["b2"], c["groups"], zz, patch, cell, field, obs, prec, n_mem)   # noqa: E731
    z0 = relayout(y.detach().cpu().double())
    w0, _, dz0 = restate(z0)
    rate = 1.0
    while rate > 1e-6 and float(restate(z0 + rate * (-0.5 * dz0))[0].sum()) > 0.9 * float(w0.sum()):
        rate *= 0.5
    after = float(restate(z0 + rate * (-0.5 * dz0))[0].sum())
    print(f"nudge: rate {rate:g} lowers the restated sum(wsse) from {float(w0.sum()):.4f} to {after:.4f}")
    assert rate > 1e-6 and after <= 0.9 * float(w0.sum())

    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")                                              # nothing is read back, nothing uploaded: the tables went up with the set
    try:
        logw, grad = like.score_and_grad(y, obs_d, prec_d)
        y1 = like.nudge(y, obs_d, prec_d, rate=rate)
        y1v = like.nudge(y, obs_d, prec_d, rate=torch.full((B * n_mem,), rate, device=DEV))
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert y1.shape == y.shape and y1.dtype == y.dtype and torch.equal(y1, y1v) and torch.equal(logw, like(y, obs_d, prec_d))
    assert rel(grad.cpu(), (-0.5 * dz0).permute(0, 2, 1, 3).reshape(y.shape)) <= TOL_BF16
    assert torch.equal(y1, (y.float() + rate * grad).to(y.dtype))
    dec32 = decoder("a", "fp32")
    s32 = SensorSet(dec32, P, patch, cell, field)
    score = lambda t: float(dec32.sensor_sse(relayout(t.float()), s32, obs_d, precision=prec_d, members=n_mem, fused=False).sum())   # noqa: E731
    before, nudged = score(y), score(y1)
    print(f"nudge: fp32 composed sum(wsse) {before:.4f} -> {nudged:.4f} on the device")
    assert nudged < before
    y2 = ens.step(conds2, state=y1)                                                       # the session takes the corrected state
    assert y2.shape == y.shape and bool(torch.isfinite(y2.float()).all())
    ens.close()
