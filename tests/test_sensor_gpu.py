"""Scoring ensemble members against sparse sensor observations on the device: sea_decode_sensor_sse through Decode.sensor_sse and SensorLikelihood.

Reference: the fp64 restatement `restate_sensor` of tests/test_sensor_cpu.py, which that file ties to the reference-generated goldens.  Let e be the
relative L2 error of the fused path against it and e_c that of the composed bf16 path (forward(), a gather, torch reductions) on the same inputs, for
the scores wsse [Bm] and for the predictions pred [Bm, K] (a sum hides index mistakes): e <= 2e-2 (the bf16 decode tolerance) and
e <= 2 e_c + 1e-6 (both paths make the same roundings and differ in summation order only); fp32 (composed): e <= 1e-4.  tests/test_sensor_cpu.py asserts
that the bf16 rounding of the operands alone stays below 1e-2 on every input used here.

Shapes a, b, c of tests/test_decode_loss_gpu.py with the (members, histories) splits of tests/test_ensemble_gpu.py; the sensor sets, readings and
precisions of tests/test_sensor_cpu.py (segments of 0, 1, 31, 32, 33 and 70 sensors, an unobserved group, the last group only, cell C - 1, second
fields of a group, K = 1; readings random normal, independent of the decoded values)."""
import functools

import pytest
import torch

from tests.test_decode_loss_cpu import rel
from tests.test_decode_loss_gpu import DEV, TOL_BF16, TOL_F32, case, decoder
from tests.test_ensemble_gpu import SPLITS
from tests.test_sensor_cpu import BIG, _draw, big_states, restate_sensor, sensor_obs, sensor_precision, sensor_sets

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def reference(name, set_name, members, hist, with_precision):
    c = case(name)
    patch, cell, field = sensor_sets(name)[set_name]
    prec = sensor_precision(name, set_name, hist) if with_precision else None
    return restate_sensor(c["w1"], c["w2"], c["b2"], c["groups"], c["z"], patch, cell, field, sensor_obs(name, set_name, hist), prec, members)


def sensor_set(dec, name, set_name):
    from sea_amd.ensemble import SensorSet

    return SensorSet(dec, case(name)["P"], *sensor_sets(name)[set_name])


def check(name, what, got, comp, ref):
    for label, g, cc, r in (("wsse", got[0], comp[0], ref[0]), ("pred", got[1], comp[1], ref[1])):
        e, e_c = rel(g.cpu(), r), rel(cc.cpu(), r)
        print(f"sensor_sse shape {name} {what} {label}: fused e {e:.3e}; composed e_c {e_c:.3e}")
        assert e <= TOL_BF16, (what, label, e)
        assert e <= 2 * e_c + 1e-6, (what, label, e, e_c)


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_fused_sensor_sse_against_fp64(name):
    c = case(name)
    dec = decoder(name, "bf16")
    z = c["z"].to(DEV)
    for set_name in sensor_sets(name):
        s = sensor_set(dec, name, set_name)
        for members, hist in SPLITS[name]:
            obs = sensor_obs(name, set_name, hist).to(DEV)
            for with_prec in (False, True):
                prec = sensor_precision(name, set_name, hist).to(DEV) if with_prec else None
                got = dec.sensor_sse(z, s, obs, precision=prec, members=members, fused=True, predictions=True)
                comp = dec.sensor_sse(z, s, obs, precision=prec, members=members, fused=False, predictions=True)
                assert got[0].shape == (c["B"],) and got[1].shape == (c["B"], s.K) and got[0].dtype == got[1].dtype == torch.float32
                assert not got[0].requires_grad and got[0].grad_fn is None
                check(name, f"set {set_name} members {members} x {hist} precision {with_prec}", got, comp, reference(name, set_name, members, hist, with_prec))
                dflt = dec.sensor_sse(z, s, obs, precision=prec, members=members, predictions=True)              # fused=None: the fused path in bf16
                assert torch.equal(dflt[0], got[0]) and torch.equal(dflt[1], got[1])
                assert torch.equal(dec.sensor_sse(z, s, obs, precision=prec, members=members, fused=True), got[0])   # without the predictions: the same score


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_fp32_composed_sensor_sse_against_fp64(name):
    c = case(name)
    dec = decoder(name, "fp32")
    z = c["z"].to(DEV)
    for set_name in sensor_sets(name):
        s = sensor_set(dec, name, set_name)
        members, hist = SPLITS[name][0]
        for with_prec in (False, True):
            prec = sensor_precision(name, set_name, hist).to(DEV) if with_prec else None
            wsse, pred = dec.sensor_sse(z, s, sensor_obs(name, set_name, hist).to(DEV), precision=prec, members=members, predictions=True)
            ref = reference(name, set_name, members, hist, with_prec)
            e_w, e_p = rel(wsse.cpu(), ref[0]), rel(pred.cpu(), ref[1])
            print(f"sensor_sse shape {name} set {set_name} precision {with_prec}: fp32 e(wsse) {e_w:.3e} e(pred) {e_p:.3e}")
            assert e_w <= TOL_F32 and e_p <= TOL_F32


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_precision_forms_and_missing_readings(name):
    c = case(name)
    dec = decoder(name, "bf16")
    z = c["z"].to(DEV)
    set_name = next(iter(sensor_sets(name)))
    s = sensor_set(dec, name, set_name)
    members, hist = SPLITS[name][0]
    obs = sensor_obs(name, set_name, hist).to(DEV)
    w = sensor_precision(name, set_name, hist)
    w1 = w[:1].expand(hist, -1).contiguous().to(DEV)                                       # the same row for every history: [B, K] against [K]
    a = dec.sensor_sse(z, s, obs, precision=w1, members=members, fused=True)
    b = dec.sensor_sse(z, s, obs, precision=w1[0].contiguous(), members=members, fused=True)
    assert torch.equal(a, b)
    # missing readings: precision 0, whatever the reading holds
    wd = w.to(DEV)
    dead = wd == 0
    assert int(dead.sum()) >= 8
    base = dec.sensor_sse(z, s, obs, precision=wd, members=members, fused=True)
    dirty = obs.clone()
    dirty[dead] = torch.tensor([float("nan"), float("inf"), -float("inf"), 3e38], device=DEV).repeat(int(dead.sum()) // 4 + 1)[:int(dead.sum())]
    got = dec.sensor_sse(z, s, dirty, precision=wd, members=members, fused=True)
    assert torch.equal(got, base) and bool(torch.isfinite(got).all())
    assert torch.equal(dec.sensor_sse(z, s, dirty, precision=wd, members=members, fused=False), dec.sensor_sse(z, s, obs, precision=wd, members=members, fused=False))
    assert rel(got.cpu(), reference(name, set_name, members, hist, True)[0]) <= TOL_BF16
    zero = dec.sensor_sse(z, s, dirty, precision=torch.zeros_like(wd), members=members, fused=True)
    assert float(zero.abs().max()) == 0.0
    assert float(dec.sensor_sse(z, s, dirty, precision=torch.zeros_like(wd), members=members, fused=False).abs().max()) == 0.0


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_every_cell_of_a_field_equals_the_dense_score(name):
    """Sensors = every cell of one field, unit precision, readings = the dense observation there: the dense launch's column of that field."""
    from sea_amd.ensemble import SensorSet
    from tests.test_decode_loss_gpu import device_target

    c = case(name)
    dec = decoder(name, "bf16")
    z, tgt = c["z"].to(DEV), device_target(name)
    members, hist = SPLITS[name][0]
    P, C_ = c["P"], c["n_inp"]
    fields = [f for g in c["groups"] for f in g]
    dense = dec.member_sse(z, tgt[:hist], members=members, fused=True)
    for col, f in ((len(fields) - 1, fields[-1]), (0, fields[0])):
        patch = [p for p in range(P) for _ in range(C_)]
        cell = [i for _ in range(P) for i in range(C_)]
        s = SensorSet(dec, P, patch, cell, [f] * len(patch))
        obs = c["target"][:hist, :, col, :C_].reshape(hist, P * C_).contiguous()
        got = dec.sensor_sse(z, s, obs.to(DEV), members=members, fused=True)
        ref, _ = restate_sensor(c["w1"], c["w2"], c["b2"], c["groups"], c["z"], patch, cell, [f] * len(patch), obs, None, members)
        e_c = rel(dec.sensor_sse(z, s, obs.to(DEV), members=members, fused=False).cpu(), ref)
        diff = rel(got.cpu(), dense[:, col].cpu())
        print(f"sensor_sse shape {name} field {f}: against the dense score {diff:.3e}; composed e_c {e_c:.3e}")
        assert diff <= 2 * e_c + 1e-6


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_bits_do_not_depend_on_the_run_the_members_or_the_histories(name):
    from sea_amd import ops

    c = case(name)
    dec = decoder(name, "bf16")
    z = c["z"].to(DEV)
    for set_name in sensor_sets(name):
        s = sensor_set(dec, name, set_name)
        for members, hist in SPLITS[name]:
            obs = sensor_obs(name, set_name, hist).to(DEV)
            prec = sensor_precision(name, set_name, hist).to(DEV)
            a = dec.sensor_sse(z, s, obs, precision=prec, members=members, fused=True, predictions=True)
            assert ops.last_form()[0] == "sensor_sse.rows64"
            b = dec.sensor_sse(z, s, obs, precision=prec, members=members, fused=True, predictions=True)
            assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
            # every member scored alone against its history's readings
            one = dec.sensor_sse(z, s, obs.repeat_interleave(members, dim=0), precision=prec.repeat_interleave(members, dim=0), members=1, fused=True, predictions=True)
            assert torch.equal(a[0], one[0]) and torch.equal(a[1], one[1])
            # a history on its own: (members, 1) against one of `hist` histories
            for h in sorted({0, hist - 1}):
                rows = slice(h * members, (h + 1) * members)
                alone = dec.sensor_sse(z[rows], s, obs[h:h + 1], precision=prec[h:h + 1], members=members, fused=True, predictions=True)
                assert torch.equal(alone[0], a[0][rows]) and torch.equal(alone[1], a[1][rows]), (set_name, members, hist, h)


def test_more_than_one_row_tile():
    """130 members (shape a's two states repeated 65 times, members = 26 x 5 histories: 26 does not divide 64): three 64-member row tiles per (patch,
    group), the last with two rows, a history boundary inside a tile, and the finish launch's rows beyond the first.  Every member is a copy of one of
    two states, so its prediction row must be the bits of that state scored alone; the scores are held against the fp64 restatement."""
    c = case("a")
    dec = decoder("a", "bf16")
    members, hist, rep = BIG["members"], BIG["hist"], BIG["rep"]
    z_host = big_states()                                                                 # [130, P, G, D]: rows 0, 2, 4, .. are state 0
    z = z_host.to(DEV)
    for set_name in sensor_sets("a"):
        patch, cell, field = sensor_sets("a")[set_name]
        s = sensor_set(dec, "a", set_name)
        obs, prec = sensor_obs("a", set_name, hist), sensor_precision("a", set_name, hist)
        ref = restate_sensor(c["w1"], c["w2"], c["b2"], c["groups"], z_host, patch, cell, field, obs, prec, members)
        got = dec.sensor_sse(z, s, obs.to(DEV), precision=prec.to(DEV), members=members, fused=True, predictions=True)
        comp = dec.sensor_sse(z, s, obs.to(DEV), precision=prec.to(DEV), members=members, fused=False, predictions=True)
        assert got[0].shape == (130,) and got[1].shape == (130, s.K)
        check("a", f"130 rows set {set_name}", got, comp, ref)
        two = dec.sensor_sse(c["z"].to(DEV), s, obs[:1].to(DEV), members=2, fused=True, predictions=True)[1]
        assert torch.equal(got[1], two.repeat(rep, 1))                                    # row arithmetic does not depend on the tile
        for bm in (0, 63, 64, 77, 78, 128, 129):                                          # a member alone against its history's readings: the same bits
            b = bm // members
            alone = dec.sensor_sse(z[bm:bm + 1], s, obs[b:b + 1].to(DEV), precision=prec[b:b + 1].to(DEV), members=1, fused=True)
            assert torch.equal(alone, got[0][bm:bm + 1]), (set_name, bm)


def test_sensor_set_scaling_is_what_patchify_writes():
    from sea_amd.models.encoder_decoder import Decode
    from sea_amd.utils.data_processors import DataPartitioner2D, MeshUnpatcher, MinMaxScaler

    g = torch.Generator().manual_seed(3)
    n_pts = 57
    x, y = torch.rand(n_pts, generator=g), torch.rand(n_pts, generator=g)
    part = DataPartitioner2D(x, y, m=4, n=3, device=DEV)
    groups = [[0, 1], [2]]
    data = torch.randn(5, n_pts, 3, generator=g) * torch.tensor([1.0, 10.0, 0.1]) + torch.tensor([0.0, 5.0, -1.0])
    scalers = [MinMaxScaler((-1, 1)), MinMaxScaler((0, 2))]
    for sc, grp in zip(scalers, groups):
        sc.fit(data[:, :, grp])
    mesh = MeshUnpatcher(part, groups, scalers)
    dec = Decode(groups, part.padded_index_map.shape[1], 16, 8).to(DEV)
    points = torch.randperm(n_pts, generator=g)[:20].tolist()
    fields = [int(v) for v in torch.randint(3, (20,), generator=g)]
    s = mesh.sensor_set(dec, points, fields)
    cells = mesh.patchify_and_scale(data.to(DEV), layout="BPFC")                           # [T, P, F, C]
    want = cells[:, torch.tensor(s.patch), torch.tensor(fields), torch.tensor(s.cell)]
    got = s.scale_values(data[:, torch.tensor(points), torch.tensor(fields)].to(DEV))
    assert torch.allclose(got, want, rtol=1e-6, atol=1e-6)                                 # the same float32 coefficients; a fused multiply-add may differ by an ulp


# ------------------------------------------------------------------------------------------------ end to end
def test_sensor_observation_cycle_on_a_rollout_session():
    """fork, step, weigh on sparse sensor readings, resample on the device, step again: the weights are those of the fp64 restatement on the returned
    states, the int32 index goes into resample as it is, and a SensorLikelihood call does not synchronise."""
    from sea_amd.ensemble import SensorLikelihood, SensorSet, systematic_resample
    from oracle.recipe import recipe_inputs
    from tests.test_input_grad_gpu import cfg_of
    from tests.test_model_gpu import build
    from tests.test_rollout_session_gpu import open_on

    c = case("a")
    P, D, n_mem, B, k = 4, c["D"], 8, 2, 3
    cfg = cfg_of(1, P * D, 4, len(c["groups"]))
    m = build(cfg, "bf16")
    x, _, ib = recipe_inputs(B, k + 4, cfg, seed=9)
    dec = decoder("a", "bf16")
    g = torch.Generator().manual_seed(12)
    patch, cell, field = _draw(g, c["groups"], c["n_inp"], [(0, 0, 5), (0, 3, 33), (1, 2, 4)])
    K = len(patch)
    obs = torch.randn(B, K, generator=g)
    prec = 0.5 + torch.rand(B, K, generator=g)
    prec[torch.rand(B, K, generator=g) < 0.2] = 0.0
    sigma = [0.5, 1.0, 2.0]
    conds = torch.rand(B * n_mem, 1, generator=g).to(DEV)
    conds2 = torch.rand(B * n_mem, 1, generator=g).to(DEV)
    u = torch.rand(B, generator=g).to(DEV)

    ens = open_on(m, x, ib, k).fork(n_mem)
    y = ens.step(conds)                                                                   # [16, 2, 64]
    s = SensorSet(dec, P, patch, cell, field)                                             # uploads its tables
    like = SensorLikelihood(dec, P, n_mem, s, sigma=sigma)                                # fused=None: the fused launch in bf16
    obs_d, prec_d = obs.to(DEV), prec.to(DEV)
    logw = like(y, obs_d, prec_d)
    assert logw.shape == (B * n_mem,) and logw.dtype == torch.float32 and logw.is_cuda
    z = y.cpu().reshape(B * n_mem, len(c["groups"]), P, D).permute(0, 2, 1, 3)
    fpos = torch.tensor([[f for grp in c["groups"] for f in grp].index(f) for f in field])
    w_ref = prec.double() / torch.tensor(sigma, dtype=torch.float64)[fpos] ** 2
    ref = -0.5 * restate_sensor(c["w1"], c["w2"], c["b2"], c["groups"], z, patch, cell, field, obs, w_ref, n_mem)[0]
    comp = SensorLikelihood(dec, P, n_mem, s, sigma=sigma, fused=False)(y, obs_d, prec_d)
    e, e_c = rel(logw.cpu(), ref), rel(comp.cpu(), ref)
    print(f"sensor observation cycle: log-weights fused e {e:.3e}, composed e_c {e_c:.3e}")
    assert e <= TOL_BF16 and e <= 2 * e_c + 1e-6
    assert torch.equal(SensorLikelihood(dec, P, n_mem, s, sigma=sigma, fused=True)(y, obs_d, prec_d), logw)

    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        logw2 = like(y, obs_d, prec_d)
        wsse2, pred2 = dec.sensor_sse(y.reshape(B * n_mem, len(c["groups"]), P, D).permute(0, 2, 1, 3), s, obs_d, precision=prec_d[0].contiguous(), members=n_mem,
                                      predictions=True)
        index, logw_out, ess, resampled = systematic_resample(logw2, n_mem, u=u)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert torch.equal(logw2, logw) and pred2.shape == (B * n_mem, K)
    assert index.dtype == torch.int32 and index.is_cuda and resampled.tolist() == [1, 1]
    idx = index.view(B, n_mem).cpu()
    assert bool((idx // n_mem == torch.arange(B).view(B, 1)).all()) and bool((idx[:, 1:] >= idx[:, :-1]).all())

    before = ens.states()
    ens.resample(index)                                                                   # the device index goes in as it is
    assert torch.equal(ens.states(), before[index.long()])
    y2 = ens.step(conds2)
    assert y2.shape == y.shape and bool(torch.isfinite(like(y2, obs_d, prec_d)).all())
    ens.close()
