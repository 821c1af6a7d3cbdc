"""Scoring ensemble members against sparse sensor observations (sea_decode_sensor_sse, Decode.sensor_sse, SensorSet, SensorLikelihood,
MeshUnpatcher.sensor_set) without a GPU: the contract restated in fp64 and tied to the reference-generated goldens through the dense restatement
of tests/test_ensemble_cpu.py, the launch tables a SensorSet builds, the condition under which the GPU test's bound is meaningful (bf16-rounded
operands stay within half of it), the entry point's argument checks and those of the Python layers, and the mesh-side constructor.

`restate_sensor`, `sensor_sets`, `sensor_obs` and `sensor_precision` are what tests/test_sensor_gpu.py compares with.

Sensor sets (fixed seed, defined once, here).  Per shape of tests/test_decode_loss_gpu.py they cover (group, patch) segments with 0, 1, 31, 32,
33 and >= 70 sensors (70 by duplicates where a patch has fewer (field, cell) pairs), cell C - 1, K = 1, a given order that is not the sorted one
and, where the shape allows it, an unobserved group, a set on the last group only and fields that are not the first of their group (the padded
width Cp, not C, separates the rows of two fields: shape a has C 12 against Cp 32):
  a  groups [[0, 1], [2]], P 9:  "segments" (group 0: patches 0 - 5 hold 0, 1, 31, 32, 33, 70; group 1: a few in patches 1 and 6), "last" (field
     2 only: group 0 unobserved), "one" (K = 1: field 1, cell C - 1, the last patch)
  b  groups [[0], [1], [2]], P 4 (one field per group: no second field exists):  "segments" (group 0: 0, 1, 31, 32; group 1: 33, 70, 0, 5;
     group 2: unobserved), "last" (group 2 only), "one"
  c  one group [[0, 1]], P 2, hidden 624 (no second group exists):  "s31_32", "s33_70", "one"
"""
import ctypes as C
import functools
import math

import pytest
import torch

from tests.test_decode_loss_cpu import load_fixture, rel
from tests.test_ensemble_cpu import restate_member_sse

SHAPES = ("a", "b", "c")
SPLITS = {"a": ((2, 1), (1, 2)), "b": ((11, 3), (33, 1), (1, 33)), "c": ((5, 7), (35, 1))}   # (members, histories): tests/test_ensemble_gpu.py::SPLITS


def host_case(name):
    """The inputs of a shape: tests/test_decode_loss_gpu.case (that module is a GPU test file but builds its cases on the host)."""
    from tests.test_decode_loss_gpu import case

    return case(name)


# ------------------------------------------------------------------------------------------------ the contract, in fp64
def _bf16(t):
    return t.to(torch.float32).to(torch.bfloat16).to(torch.float64)


def restate_sensor(w1, w2, b2, groups, z, patch, cell, field, obs, precision, members, round_bf16=False):
    """include/sea_hip.h, sea_decode_sensor_sse, with the first decoder layer in front of it, in fp64 (exact GELU, as tests/test_decode_loss_cpu.restate
    decodes).  w1[g] [S, D], w2[g] [n_g * C, S], b2[g] [n_g * C]; z [Bm, P, G, D]; patch, cell, field: K integers; obs [Bm / members, K]; precision None,
    [K] or [Bm / members, K].  round_bf16: z, W1, the hidden rows and W2 are rounded to bf16 first (what the bf16 paths compute with).
    Returns (wsse [Bm], pred [Bm, K]) in float64."""
    f64 = torch.float64
    Bm, P, G, D = z.shape
    n_f = [len(g) for g in groups]
    C_ = w2[0].shape[0] // n_f[0]
    rnd = _bf16 if round_bf16 else (lambda t: t.detach().to(f64))
    flat = [f for g in groups for f in g]
    Y = torch.empty(Bm, P, sum(n_f), C_, dtype=f64)
    f0 = 0
    for g in range(G):
        pre = rnd(z[:, :, g]) @ rnd(w1[g]).t()
        H = 0.5 * pre * (1.0 + torch.erf(pre / math.sqrt(2.0)))
        if round_bf16:
            H = _bf16(H)
        Y[:, :, f0:f0 + n_f[g]] = (H @ rnd(w2[g]).t() + b2[g].to(f64)).view(Bm, P, n_f[g], C_)
        f0 += n_f[g]
    pos = torch.tensor([flat.index(f) for f in field])
    pred = Y[:, torch.tensor(patch), pos, torch.tensor(cell)]                       # [Bm, K]
    B, K = Bm // members, len(patch)
    assert Bm % members == 0 and tuple(obs.shape) == (B, K)
    o = obs.to(f64).repeat_interleave(members, dim=0)
    w = torch.ones(B, K, dtype=f64) if precision is None else precision.to(f64).expand(B, K)
    w = w.repeat_interleave(members, dim=0)
    live = w > 0
    d = torch.where(live, pred - o, torch.zeros((), dtype=f64))
    return (torch.where(live, w, torch.zeros((), dtype=f64)) * d * d).sum(1), pred


# ------------------------------------------------------------------------------------------------ the sensor sets of the GPU test
def _draw(g, groups, C_, segments):
    """segments: (group, patch, count) -> sensors drawn with replacement from the group's (field, cell) pairs; the first of a segment sits at cell
    C - 1 of the group's last field."""
    patch, cell, field = [], [], []
    for grp, p, n in segments:
        for i in range(n):
            if i == 0:
                f, c = groups[grp][-1], C_ - 1
            else:
                f = groups[grp][int(torch.randint(len(groups[grp]), (1,), generator=g))]
                c = int(torch.randint(C_, (1,), generator=g))
            patch.append(p), cell.append(c), field.append(f)
    order = torch.randperm(len(patch), generator=g).tolist()                       # the given order is not the sorted one
    return [patch[i] for i in order], [cell[i] for i in order], [field[i] for i in order]


@functools.lru_cache(maxsize=None)
def sensor_sets(name):
    """name of a shape -> {set name: (patch, cell, field)}; computed once, never modified."""
    c = host_case(name)
    groups, C_, P = c["groups"], c["n_inp"], c["P"]
    g = torch.Generator().manual_seed({"a": 101, "b": 102, "c": 103}[name])
    last = len(groups) - 1
    if name == "a":
        return {"segments": _draw(g, groups, C_, [(0, 1, 1), (0, 2, 31), (0, 3, 32), (0, 4, 33), (0, 5, 70), (1, 1, 3), (1, 6, 2)]),
                "last": _draw(g, groups, C_, [(last, 2, 5), (last, 8, 7)]),
                "one": ([P - 1], [C_ - 1], [1])}
    if name == "b":
        return {"segments": _draw(g, groups, C_, [(0, 1, 1), (0, 2, 31), (0, 3, 32), (1, 0, 33), (1, 1, 70), (1, 3, 5)]),
                "last": _draw(g, groups, C_, [(last, 0, 4), (last, 3, 9)]),
                "one": ([P - 1], [C_ - 1], [groups[last][0]])}
    return {"s31_32": _draw(g, groups, C_, [(0, 0, 31), (0, 1, 32)]),
            "s33_70": _draw(g, groups, C_, [(0, 0, 33), (0, 1, 70)]),
            "one": ([P - 1], [C_ - 1], [1])}


@functools.lru_cache(maxsize=None)
def sensor_obs(name, set_name, hist):
    """Readings [hist, K]: random normal, independent of the decoded values."""
    K = len(sensor_sets(name)[set_name][0])
    g = torch.Generator().manual_seed(7000 + 13 * hist + len(set_name) + ord(name))
    return torch.randn(hist, K, generator=g)


@functools.lru_cache(maxsize=None)
def sensor_precision(name, set_name, hist):
    """A precision per history and sensor [hist, K] in [0.25, 4], about a quarter of the entries exactly 0 (missing readings); K = 1 keeps its reading."""
    K = len(sensor_sets(name)[set_name][0])
    g = torch.Generator().manual_seed(9000 + 17 * hist + len(set_name) + ord(name))
    w = 0.25 + 3.75 * torch.rand(hist, K, generator=g)
    if K > 1:
        w[torch.rand(hist, K, generator=g) < 0.25] = 0.0
        w[:, 0] = 1.5
    return w


BIG = dict(members=26, hist=5, rep=65)   # tests/test_sensor_gpu.py::test_more_than_one_row_tile: shape a's two states repeated to 130 members


def big_states():
    return host_case("a")["z"].repeat(BIG["rep"], 1, 1, 1)


def every_set():
    return [(name, s) for name in SHAPES for s in sensor_sets(name)]


def make_decoder(name):
    from sea_amd.models.encoder_decoder import Decode

    c = host_case(name)
    return Decode(c["groups"], c["n_inp"], c["hidden"], c["D"])


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("name", ["decode_mse_a", "decode_mse_b"])
def test_sensor_restatement_with_every_valid_cell_is_the_dense_restatement(name):
    """Every valid cell of every field as a sensor, unit precision: the sum over the sensors is the dense score summed over the fields, which
    tests/test_ensemble_cpu.py ties to the reference-generated goldens."""
    fx = load_fixture(name)
    C_, P = fx["n_inp"], fx["P"]
    fields = [f for g in fx["groups"] for f in g]
    for counts in (None, fx["counts"].tolist()):
        for members in (1, 2):
            z = fx["z"] if members == 1 else fx["z"].repeat_interleave(2, dim=0)
            patch, cell, field = [], [], []
            for p in range(P):
                for f in fields:
                    for c in range(C_ if counts is None else counts[p]):
                        patch.append(p), cell.append(c), field.append(f)
            tgt = fx["target"].to(torch.float64)
            obs = tgt[:, torch.tensor(patch), torch.tensor(field), torch.tensor(cell)]
            wsse, pred = restate_sensor(fx["w1"], fx["w2"], fx["b2"], fx["groups"], z, patch, cell, field, obs, None, members)
            dense = restate_member_sse(fx["w1"], fx["w2"], fx["b2"], fx["groups"], z, fx["target"], counts, members).sum(1)
            assert pred.shape == (z.shape[0], len(patch))
            assert rel(wsse, dense) <= 1e-12, (counts is None, members)


def test_zero_precision_is_neutral_in_the_restatement():
    c = host_case("a")
    patch, cell, field = sensor_sets("a")["segments"]
    obs, w = sensor_obs("a", "segments", 1).clone(), sensor_precision("a", "segments", 1)
    base, _ = restate_sensor(c["w1"], c["w2"], c["b2"], c["groups"], c["z"], patch, cell, field, obs, w, 2)
    obs[w == 0] = float("nan")
    got, _ = restate_sensor(c["w1"], c["w2"], c["b2"], c["groups"], c["z"], patch, cell, field, obs, w, 2)
    assert int((w == 0).sum()) > 10 and torch.equal(base, got) and bool(torch.isfinite(got).all())
    assert torch.equal(restate_sensor(c["w1"], c["w2"], c["b2"], c["groups"], c["z"], patch, cell, field, obs, w[0], 2)[0], got)   # [K] against [B, K]


# ------------------------------------------------------------------------------------------------ the launch tables
@pytest.mark.parametrize("name,set_name", every_set())
def test_launch_tables(name, set_name):
    from sea_amd import _native as N
    from sea_amd.ensemble import SensorSet

    c = host_case(name)
    dec = make_decoder(name)
    patch, cell, field = sensor_sets(name)[set_name]
    s = SensorSet(dec, c["P"], patch, cell, field)
    K, G, Cp, C_ = len(patch), len(c["groups"]), dec._n_inp_p, c["n_inp"]
    grp_of = {f: g for g, grp in enumerate(c["groups"]) for f in grp}
    assert s.K == K and s.K_pad == len(s.perm) == len(s.wrow) == len(s.live) and s.K_pad % N.SENSOR_TILE == 0 and s.K_pad >= N.SENSOR_TILE
    assert s.patches == sorted(set(patch)) and s.Q == len(s.patches) and len(s.seg) == G and all(len(r) == s.Q + 1 for r in s.seg)
    # perm over the live entries is a permutation of range(K); pad entries point at sensor 0 with row 0
    assert sorted(k for k, l in zip(s.perm, s.live) if l) == list(range(K))
    assert all(k == 0 and w == 0 for k, w, l in zip(s.perm, s.wrow, s.live) if not l)
    assert all(s.perm[s.inv[k]] == k and s.live[s.inv[k]] == 1 for k in range(K))
    # the segments: CSR over (group, patch), multiples of 32, contiguous; the live entries of a segment are exactly the group's sensors of that patch in the given order
    flat = [v for r in s.seg for v in r]
    assert flat[0] == 0 and flat[-1] == s.K_pad and all(a <= b for a, b in zip(flat, flat[1:]))
    for g in range(G):
        assert g == 0 or s.seg[g][0] == s.seg[g - 1][-1]
        for qi, p in enumerate(s.patches):
            a, b = s.seg[g][qi], s.seg[g][qi + 1]
            want = [k for k in range(K) if grp_of[field[k]] == g and patch[k] == p]
            assert (b - a) % N.SENSOR_TILE == 0 and b - a == -(-len(want) // N.SENSOR_TILE) * N.SENSOR_TILE
            assert [k for k, l in zip(s.perm[a:b], s.live[a:b]) if l] == want and s.live[a:b] == [1] * len(want) + [0] * (b - a - len(want))
            for i, k in enumerate(want):   # the PADDED width separates the fields of a group
                assert s.wrow[a + i] == c["groups"][g].index(field[k]) * Cp + cell[k]
    if Cp != C_ and any(c["groups"][grp_of[f]].index(f) > 0 for f in field):
        assert any(w >= Cp for w in s.wrow)                                       # a second field sits beyond Cp, not beyond C
    assert s.matches(dec, c["P"]) and not s.matches(dec, c["P"] + 1)


def test_the_sets_cover_what_the_gpu_test_needs():
    from sea_amd.ensemble import SensorSet

    for name in SHAPES:
        c = host_case(name)
        dec = make_decoder(name)
        sizes, empty_groups, cells, second_fields = set(), 0, set(), 0
        for set_name, (patch, cell, field) in sensor_sets(name).items():
            s = SensorSet(dec, c["P"], patch, cell, field)
            for g in range(len(s.seg)):
                n_g = 0
                for qi in range(s.Q):
                    n = sum(s.live[s.seg[g][qi]:s.seg[g][qi + 1]])
                    sizes.add(n if n < 70 else 70)
                    n_g += n
                empty_groups += n_g == 0
            cells |= set(cell)
            second_fields += sum(1 for f in field if any(f in grp and grp.index(f) > 0 for grp in c["groups"]))
            if set_name == "last":
                assert {f for f in field} <= set(c["groups"][-1])
        assert {1, 31, 32, 33, 70} <= sizes and (0 in sizes or len(c["groups"]) == 1), (name, sizes)
        assert c["n_inp"] - 1 in cells and any(len(v[0]) == 1 for v in sensor_sets(name).values())
        assert empty_groups >= 1 or len(c["groups"]) == 1
        assert second_fields >= 1 or all(len(g) == 1 for g in c["groups"])


@pytest.mark.parametrize("name,set_name", every_set())
def test_bf16_rounded_operands_stay_within_half_the_gpu_bound(name, set_name):
    """The GPU test allows 2e-2 against the fp64 restatement; what the bf16 paths cannot avoid — operands rounded to bf16 — must stay below half of it
    on every set and split, or the bound would measure the inputs and not the kernel."""
    c = host_case(name)
    patch, cell, field = sensor_sets(name)[set_name]
    for members, hist in SPLITS[name]:
        for prec in (None, sensor_precision(name, set_name, hist)):
            obs = sensor_obs(name, set_name, hist)
            ref = restate_sensor(c["w1"], c["w2"], c["b2"], c["groups"], c["z"], patch, cell, field, obs, prec, members)
            rnd = restate_sensor(c["w1"], c["w2"], c["b2"], c["groups"], c["z"], patch, cell, field, obs, prec, members, round_bf16=True)
            e_w, e_p = rel(rnd[0], ref[0]), rel(rnd[1], ref[1])
            print(f"sensor shape {name} set {set_name} members {members} x {hist} precision {prec is not None}: bf16 operands e(wsse) {e_w:.3e} e(pred) {e_p:.3e}")
            assert e_w <= 1e-2 and e_p <= 1e-2, (members, hist, e_w, e_p)


def test_bf16_rounded_operands_stay_within_half_the_gpu_bound_at_130_members():
    c = host_case("a")
    z = big_states()
    for set_name, (patch, cell, field) in sensor_sets("a").items():
        obs, prec = sensor_obs("a", set_name, BIG["hist"]), sensor_precision("a", set_name, BIG["hist"])
        ref = restate_sensor(c["w1"], c["w2"], c["b2"], c["groups"], z, patch, cell, field, obs, prec, BIG["members"])
        rnd = restate_sensor(c["w1"], c["w2"], c["b2"], c["groups"], z, patch, cell, field, obs, prec, BIG["members"], round_bf16=True)
        e_w, e_p = rel(rnd[0], ref[0]), rel(rnd[1], ref[1])
        print(f"sensor shape a set {set_name} 130 members: bf16 operands e(wsse) {e_w:.3e} e(pred) {e_p:.3e}")
        assert e_w <= 1e-2 and e_p <= 1e-2, (set_name, e_w, e_p)


# ------------------------------------------------------------------------------------------------ refusals of the Python layers
def test_sensor_set_refuses_bad_inputs():
    from sea_amd.ensemble import SensorSet

    dec = make_decoder("a")   # groups [[0, 1], [2]], n_inp 12
    ok = ([0, 1], [3, 4], [0, 2])
    SensorSet(dec, 9, *ok)
    SensorSet(dec, 9, torch.tensor(ok[0]), torch.tensor(ok[1], dtype=torch.int32), ok[2])
    SensorSet(dec, 9, [1, 1], [3, 3], [0, 0])                                         # duplicates: two instruments at one point
    bad = [dict(patch=[0, 9]), dict(patch=[-1, 0]), dict(cell=[3, 12]), dict(cell=[-1, 0]), dict(field=[0, 3]), dict(field=[0, -1]),
           dict(patch=[True, False]), dict(cell=[1.0, 2.0]), dict(patch=torch.tensor([0.0, 1.0])), dict(patch=torch.tensor([True, False])),
           dict(patch=[]), dict(patch=[], cell=[], field=[]), dict(patch=[[0], [1, 2]]), dict(patch=[0, 1, 2]), dict(field=[0]),
           dict(patch=torch.zeros(2, 1, dtype=torch.int64)), dict(patch=3), dict(cell=None)]
    for kw in bad:
        args = dict(patch=ok[0], cell=ok[1], field=ok[2])
        args.update(kw)
        with pytest.raises(ValueError):
            SensorSet(dec, 9, **args)
    for n in (0, -1, True, 2.0):
        with pytest.raises(ValueError):
            SensorSet(dec, n, *ok)


def test_sensor_sse_and_likelihood_refuse_before_a_device_is_touched():
    from sea_amd.ensemble import SensorLikelihood, SensorSet
    from sea_amd.utils.train_utils import SensorLikelihood as SL2, SensorSet as SS2

    assert SL2 is SensorLikelihood and SS2 is SensorSet
    c = host_case("a")
    dec = make_decoder("a").set_compute_dtype("bf16")
    P, D, G = c["P"], c["D"], len(c["groups"])
    s = SensorSet(dec, P, [0, 1, 8], [3, 4, 11], [0, 2, 1])
    z, obs = torch.zeros(4, P, G, D), torch.zeros(2, 3)
    bad = [dict(z=torch.zeros(4, P, G)), dict(z=torch.zeros(4, P, G + 1, D)), dict(members=3), dict(members=0), dict(members=True),
           dict(obs=torch.zeros(2, 4)), dict(obs=torch.zeros(4, 3)), dict(obs=torch.zeros(2, 3, dtype=torch.float64)), dict(obs=torch.zeros(6)), dict(obs=[0.0] * 3),
           dict(precision=torch.ones(4)), dict(precision=torch.ones(3, dtype=torch.float64)), dict(precision=torch.ones(4, 3)),
           dict(precision=torch.tensor([1.0, -1.0, 1.0])), dict(precision=torch.tensor([1.0, float("nan"), 1.0])), dict(precision=torch.tensor([[1.0, float("inf"), 1.0]] * 2)),
           dict(precision=[1.0, 1.0, 1.0]), dict(sensors=None), dict(sensors=([0], [0], [0])),
           dict(sensors=SensorSet(dec, P + 1, [0], [0], [0])),                                                       # another n_patches
           dict(sensors=SensorSet(make_decoder("b"), P, [0], [0], [0])),                                             # another n_inp and grouping
           dict(obs=torch.zeros(2, 3, device="meta"))]
    for kw in bad:
        args = dict(z=z, sensors=s, obs=obs, precision=None, members=2)
        args.update(kw)
        zz = args.pop("z")
        with pytest.raises(ValueError):
            dec.sensor_sse(zz, **args)
    with pytest.raises(ValueError):
        make_decoder("a").sensor_sse(z, s, obs, members=2, fused=True)                                               # fp32: no fused launch
    with pytest.raises(RuntimeError, match="MI355X"):                                                                # well-formed, but on the host
        dec.sensor_sse(z, s, obs, members=2)
    with pytest.raises(RuntimeError, match="MI355X"):
        make_decoder("a").sensor_sse(z, s, obs, precision=torch.ones(2, 3), members=2, predictions=True)

    y = torch.zeros(4, G, P * D)
    like = SensorLikelihood(dec, P, 2, s, sigma=[0.5, 1.0, 2.0])
    assert like._prec_host == [4.0, 0.25, 1.0]                                                                       # per field, at the sensors' fields 0, 2, 1
    assert SensorLikelihood(dec, P, 2, s, sigma=2.0)._prec_host == [0.25] * 3 and SensorLikelihood(dec, P, 2, s)._prec_host is None
    s4 = SensorSet(dec, P, [0, 1, 8, 8], [3, 4, 11, 0], [0, 2, 1, 1])
    assert SensorLikelihood(dec, P, 2, s4, sigma=torch.tensor([1.0, 2.0, 4.0, 0.5]))._prec_host == [1.0, 0.25, 0.0625, 4.0]   # per sensor
    for sig in (0.0, -1.0, float("nan"), [1.0, 2.0], [1.0, 0.0, 1.0], torch.ones(2, 3)):
        with pytest.raises(ValueError):
            SensorLikelihood(dec, P, 2, s, sigma=sig)
    for kw in (dict(n_patches=P + 1), dict(n_patches=0), dict(members=0), dict(members=1.0), dict(sensors=None)):
        args = dict(n_patches=P, members=2, sensors=s)
        args.update(kw)
        with pytest.raises(ValueError):
            SensorLikelihood(dec, **args)
    for yy, oo, pp in ((torch.zeros(4, G, P * D + 1), obs, None), (torch.zeros(3, G, P * D), obs, None), (torch.zeros(4, P * D), obs, None), (y, torch.zeros(2, 2), None),
                       (y, obs, torch.tensor([1.0, -2.0, 1.0])), (y, obs.double(), None)):
        with pytest.raises(ValueError):
            like(yy, oo, pp)
    with pytest.raises(RuntimeError, match="MI355X"):
        like(y, obs, torch.ones(3))


def test_ops_refuse_malformed_operands_on_the_host():
    from sea_amd import ops

    def args(**kw):
        Q, Bm, S, Cp, K_pad = 2, 4, 40, 32, 64
        a = dict(groups=[dict(H=torch.zeros(Q * Bm, S, dtype=torch.bfloat16), W2=torch.zeros(n * Cp, S, dtype=torch.bfloat16), bias=torch.zeros(n * Cp)) for n in (2, 1)],
                 obs=torch.zeros(2, K_pad), live=torch.zeros(K_pad, dtype=torch.int32), wrow=torch.zeros(K_pad, dtype=torch.int32),
                 seg=torch.zeros(2, Q + 1, dtype=torch.int32), Cp=Cp, members=2, prec=None)
        a.update(kw)
        return a

    with pytest.raises(RuntimeError, match="MI355X"):
        ops.decode_sensor_sse(**args())
    with pytest.raises(RuntimeError, match="MI355X"):
        ops.decode_sensor_sse(**args(prec=torch.ones(2, 64), predictions=True))
    bad = [dict(dtype=torch.float32), dict(groups=[]), dict(Cp=12), dict(seg=torch.zeros(2, 3, dtype=torch.int64)), dict(seg=torch.zeros(3, 3, dtype=torch.int32)),
           dict(seg=torch.zeros(2, 1, dtype=torch.int32)), dict(live=torch.zeros(64, dtype=torch.int64)), dict(wrow=torch.zeros(32, dtype=torch.int32)),
           dict(live=torch.zeros(48, dtype=torch.int32), wrow=torch.zeros(48, dtype=torch.int32)), dict(members=3), dict(members=0),
           dict(obs=torch.zeros(2, 32)), dict(obs=torch.zeros(4, 64)), dict(obs=torch.zeros(2, 64, dtype=torch.float64)), dict(obs=torch.zeros(2, 128)[:, ::2]),
           dict(prec=torch.ones(32)), dict(prec=torch.ones(4, 64)), dict(prec=torch.ones(64, dtype=torch.float64)), dict(prec=torch.ones(65)[1:]),
           dict(seg=torch.zeros(2, 4, dtype=torch.int32))]                         # Q = 3 does not divide the 8 hidden rows
    for kw in bad:
        with pytest.raises(ValueError):
            ops.decode_sensor_sse(**args(**kw))
    a = args()
    a["groups"][1]["H"] = torch.zeros(8, 48, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="group 1"):
        ops.decode_sensor_sse(**a)
    a = args()
    a["groups"][0]["bias"] = torch.zeros(65)[1:]
    with pytest.raises(ValueError, match="group 0"):
        ops.decode_sensor_sse(**a)


# ------------------------------------------------------------------------------------------------ the entry point, without a GPU
@pytest.fixture(scope="module")
def lib():
    from sea_amd import build, _native

    build.build(verbose=False)
    return _native.lib()


def _table(n_groups=2):
    """A well-formed sea_decode_sensor_sse table over made-up (aligned, never dereferenced) addresses: shape a, 4 members, 3 observed patches."""
    from sea_amd import _native as N

    g = (N.SeaDecodeMseGroup * N.DECODE_MSE_MAX_GROUPS)()
    for i in range(n_groups):
        base = 0x10000 * (i + 1)
        g[i].H, g[i].W2, g[i].bias, g[i].dH, g[i].Z = base, base + 0x1000, base + 0x2000, None, None
        g[i].ldh = g[i].ldw = 40
        g[i].n_fields, g[i].field0 = (2, 0) if i == 0 else (1, 2)
    p = N.SeaDecodeSensorSse()
    p.obs, p.prec, p.live, p.wrow, p.seg, p.wsse, p.pred, p.work = 0x100000, 0x110000, 0x120004, 0x130004, 0x140004, 0x150004, 0x160000, 0x170004
    p.ld_obs, p.ld_prec, p.work_cap = 128, 0, 3 * 2 * 4
    p.Bm, p.members, p.S, p.Cp, p.Q, p.K_pad = 4, 2, 40, 32, 3, 128
    return g, p


def test_symbol_and_struct_layout(lib):
    from sea_amd import _native as N

    assert hasattr(lib, "sea_decode_sensor_sse") and "sea_decode_sensor_sse" in N.EXPORTED_SYMBOLS
    assert C.sizeof(N.SeaDecodeSensorSse) == 112                    # include/sea_hip.h states it
    assert N.SeaDecodeSensorSse.ld_obs.offset == 64 and N.SeaDecodeSensorSse.Bm.offset == 88 and N.SeaDecodeSensorSse.K_pad.offset == 108
    assert N.SENSOR_TILE == 32 and lib.sea_abi_version() == 8 and len(N.ABI_STRUCTS) == 33 and N.ABI_STRUCTS[-1] is N.SeaKvFork
    # the library reads the fields where the binding writes them: its messages quote the values back
    call = lambda g, p, n=2, dt=N.SEA_BF16: lib.sea_decode_sensor_sse(g, n, C.byref(p), dt, None)   # noqa: E731
    g, p = _table()
    p.members = 3
    assert call(g, p) == -1 and b"Bm=4 must be a positive multiple of members=3" in lib.sea_last_error()
    g, p = _table()
    p.K_pad = 31
    assert call(g, p) == -1 and b"K_pad=31" in lib.sea_last_error()
    g, p = _table()
    p.work_cap -= 1
    assert call(g, p) == -1 and b"workspace of 23 floats is too small: 24 needed" in lib.sea_last_error()
    g, p = _table()
    p.ld_obs = 96
    assert call(g, p) == -1 and b"ld_obs=96 must cover K_pad=128" in lib.sea_last_error()
    g, p = _table()
    p.ld_prec = 130
    assert call(g, p) == -1 and b"ld_prec=130" in lib.sea_last_error()
    g, p = _table()
    p.Q = 0
    assert call(g, p) == -1 and b"Q=0" in lib.sea_last_error()
    g, p = _table()
    p.Cp = 48
    assert call(g, p) == -1 and b"Cp=48" in lib.sea_last_error()
    g, p = _table()
    p.S = 36
    assert call(g, p) == -1 and b"S=36" in lib.sea_last_error()


BREAKS = {"null obs": ("obs", None), "null live": ("live", None), "null wrow": ("wrow", None), "null seg": ("seg", None), "null wsse": ("wsse", None),
          "null work": ("work", None), "misaligned obs": ("obs", 0x100008), "misaligned prec": ("prec", 0x110004), "misaligned pred": ("pred", 0x160008),
          "misaligned live": ("live", 0x120002), "misaligned wrow": ("wrow", 0x130001), "misaligned seg": ("seg", 0x140002), "misaligned wsse": ("wsse", 0x150002),
          "misaligned work": ("work", 0x170001), "K_pad = 0": ("K_pad", 0), "K_pad = 48": ("K_pad", 48), "Bm = 0": ("Bm", 0), "members = 0": ("members", 0),
          "S = 0": ("S", 0), "Cp = 0": ("Cp", 0), "Q too large": ("Q", 65536), "ld_obs % 4": ("ld_obs", 130), "ld_prec short": ("ld_prec", 64)}


@pytest.mark.parametrize("what", sorted(BREAKS) + ["null group pointer", "misaligned operand", "short row stride", "row stride % 8", "no groups", "too many groups"])
def test_sensor_sse_refuses_bad_arguments_without_a_device(lib, what):
    from sea_amd import _native as N

    g, p = _table()
    n = 2
    if what in BREAKS:
        setattr(p, *BREAKS[what])
    elif what == "null group pointer":
        g[1].bias = None
    elif what == "misaligned operand":
        g[0].W2 = 0x11008
    elif what == "short row stride":
        g[1].ldh = 32
    elif what == "row stride % 8":
        g[0].ldw = 44
    elif what == "no groups":
        n = 0
    else:
        n = 17
    assert lib.sea_decode_sensor_sse(g, n, C.byref(p), N.SEA_BF16, None) == -1, what
    msg = lib.sea_last_error()
    assert b"sea_decode_sensor_sse" in msg
    if what in ("null group pointer", "short row stride"):
        assert b"group 1" in msg
    if what in ("misaligned operand", "row stride % 8"):
        assert b"group 0" in msg


def test_sensor_sse_unsupported_forms_and_null_tables(lib):
    from sea_amd import _native as N

    g, p = _table()
    assert lib.sea_decode_sensor_sse(g, 2, C.byref(p), N.SEA_F32, None) == -3   # fp32: unsupported, not an argument error
    assert b"sea_decode_sensor_sse" in lib.sea_last_error() and b"bf16 only" in lib.sea_last_error()
    g, p = _table()
    p.S = 648
    for i in range(2):
        g[i].ldh = g[i].ldw = 648
    assert lib.sea_decode_sensor_sse(g, 2, C.byref(p), N.SEA_BF16, None) == -3 and b"S=648" in lib.sea_last_error()
    assert lib.sea_decode_sensor_sse(None, 1, C.byref(p), N.SEA_BF16, None) == -1
    assert lib.sea_decode_sensor_sse(g, 1, None, N.SEA_BF16, None) == -1
    assert lib.sea_decode_sensor_sse(g, 2, C.byref(p), 7, None) == -1
    g, p = _table()   # prec and pred may be NULL: such a table passes the pointer and alignment checks and fails only at the last check, which this test breaks
    p.prec = p.pred = None
    p.work_cap -= 1
    assert lib.sea_decode_sensor_sse(g, 2, C.byref(p), N.SEA_BF16, None) == -1 and b"workspace of 23 floats is too small" in lib.sea_last_error()


# ------------------------------------------------------------------------------------------------ sensors on a mesh
def test_sensor_set_on_a_synthetic_partitioner():
    from sea_amd.models.encoder_decoder import Decode
    from sea_amd.utils.data_processors import DataPartitioner2D, MeshProcessor, MeshUnpatcher, MinMaxScaler

    g = torch.Generator().manual_seed(3)
    n_pts = 57
    x, y = torch.rand(n_pts, generator=g), torch.rand(n_pts, generator=g)
    part = DataPartitioner2D(x, y, m=4, n=3, device="cpu")                         # 3 x 2 cells
    P, C_ = part.padded_index_map.shape
    groups = [[0, 1], [2]]
    data = torch.randn(5, n_pts, 3, generator=g) * torch.tensor([1.0, 10.0, 0.1]) + torch.tensor([0.0, 5.0, -1.0])
    scalers = [MinMaxScaler((-1, 1)), MinMaxScaler((0, 2))]
    for sc, grp in zip(scalers, groups):
        sc.fit(data[:, :, grp])
    mesh = MeshUnpatcher(part, groups, scalers)
    dec = Decode(groups, C_, 16, 8)
    points = torch.randperm(n_pts, generator=g)[:20].tolist() + [0, 0]
    fields = [int(v) for v in torch.randint(3, (22,), generator=g)]
    s = mesh.sensor_set(dec, points, fields)
    assert s.K == 22 and s.n_patches == P and s.matches(dec, P) and s.field == fields
    imap = part.padded_index_map
    for k, pt in enumerate(points):                                                # the point sits where padded_index_map puts it
        assert int(imap[s.patch[k], s.cell[k]]) == pt
    # scale_values: the column patchify_and_scale writes at the sensor's slot — the forward affine of the field's group, in float32
    snap = data[2]
    v = snap[torch.tensor(points), torch.tensor(fields)]
    a, b = mesh._forward_coefficients()
    want = torch.stack([v[k] * torch.tensor(a[f], dtype=torch.float32) + torch.tensor(b[f], dtype=torch.float32) for k, f in enumerate(fields)])
    assert torch.equal(s.scale_values(v), want)
    for k, f in enumerate(fields):                                                 # and that is the reference scaler's transform
        grp = 0 if f < 2 else 1
        assert abs(float(want[k]) - float(scalers[grp].transform(v[k]))) <= 1e-5
    assert torch.equal(s.scale_values(torch.stack([v, v]))[1], want)
    sig = torch.rand(22, generator=g)
    assert torch.equal(s.scale_sigma(sig), sig * torch.tensor([abs(a[f]) for f in fields], dtype=torch.float32))
    # refusals
    for pts, fl in (([n_pts], [0]), ([-1], [0]), ([0], [3]), ([0, 1], [0]), ([0.5], [0]), ([], [])):
        with pytest.raises(ValueError):
            mesh.sensor_set(dec, pts, fl)
    with pytest.raises(ValueError):
        mesh.sensor_set(Decode(groups, C_ - 1, 16, 8), [int(imap[0, 0])], [0])    # a decoder narrower than the mesh's patches, even for a point in cell 0
    wide = mesh.sensor_set(Decode(groups, C_ + 3, 16, 8), points, fields)          # a wider (padded) cell is the decoder's business
    assert wide.patch == s.patch and wide.cell == s.cell and wide.points == points and s.points == points
    from sea_amd.ensemble import SensorSet

    with pytest.raises(ValueError):
        SensorSet(dec, P, [0], [0], [0]).scale_values(torch.zeros(1))              # built without a mesh: no scaling to apply
    with pytest.raises(ValueError):
        s.scale_values(torch.zeros(21))
    proc = MeshProcessor(dict(dimension="2D", field_groups=groups, m=4, n=3), torch.stack([x, y]), device="cpu")
    with pytest.raises(ValueError, match="patchify_and_scale first"):
        proc.sensor_set(dec, [0], [0])
