"""Sensors that read a derived quantity (sea_decode_derived_sensor_sse / _grad, DerivedSensorSet and its consumers, MeshUnpatcher.derived_sensor_set)
without a GPU: the contract restated in fp64 (`restate_derived_sensor`: score, predictions and dz, built on the decode of tests/test_sensor_cpu.py's
restate_sensor and tests/test_sensor_grad_cpu.py's forward, the derivative held against torch.autograd), the pair tables a DerivedSensorSet builds,
every refusal before a device is touched, both symbols through ctypes, the composed float32 arithmetic against numpy float32 bit for bit, and the
conditions under which the GPU test's bounds are meaningful (the roundings no bf16 path can avoid stay below 1e-2; no magnitude reading of the
gradient inputs sits near a zero speed, where the derivative is ill-conditioned).

`restate_derived_sensor`, `derived_sets`, `derived_obs`, `derived_precision` and `readings_of` are what tests/test_derived_sensor_gpu.py compares with.

Sets (fixed seeds, defined once, here).  A reading is a field id (plain) or a tuple (op, a, b, scale_a, shift_a, scale_b, shift_b).  Per shape of
tests/test_decode_loss_gpu.py, (group, patch) segments of 1, 15, 16, 17 and 35 READINGS (one pair; a tile less one; one tile; a tile plus one; more than
two tiles), all three ops and plain readings mixed, the first reading of every segment at cell C - 1, a shuffled given order:
  a  groups [[0, 1], [2]], P 9:  "segments" (group 0: patches 1 - 5 hold 1, 15, 16, 17, 35; group 1, plain only: 3 in patch 1, 2 in patch 6), "g0"
     (group 0 only: group 1 unobserved), "one" (K = 1: a speed at cell C - 1 of the last patch)
  c  one group [[0, 1]], P 2, hidden 624:  "s15_16", "s17_35", "one"
  b  three one-field groups: no derived reading can be paired there; the plain-only set is tests/test_sensor_cpu.py's "segments".
The shifts keep every speed well away from 0 (asserted below): a' = y_a scale_a + shift_a with |shift| in [2.5, 3.5] and |scale| in [0.4, 0.8]."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests.test_decode_loss_cpu import rel
from tests.test_sensor_cpu import BIG, SPLITS, _bf16, _table, big_states, host_case, make_decoder, restate_sensor, sensor_sets
from tests.test_sensor_grad_cpu import _forward

OPS = ("magnitude", "energy", "difference")
SHAPES = ("a", "c")
SEGMENT_SIZES = (1, 15, 16, 17, 35)


# ------------------------------------------------------------------------------------------------ the sets of the GPU test
def _draw_readings(g, groups, C_, segments):
    """segments: (group, patch, count) -> readings: in a group with two fields a cycle of magnitude, energy, difference and plain readings with drawn
    coefficients, in a one-field group plain readings; the first of a segment sits at cell C - 1; the given order is shuffled."""
    patch, cell, reading = [], [], []
    n = 0
    for grp, p, cnt in segments:
        flds = groups[grp]
        for i in range(cnt):
            c = C_ - 1 if i == 0 else int(torch.randint(C_, (1,), generator=g))
            kind = n % 4 if len(flds) >= 2 else 3
            n += 1
            if kind == 3:
                r = flds[int(torch.randint(len(flds), (1,), generator=g))]
            else:
                a, b = (flds[0], flds[1]) if int(torch.randint(2, (1,), generator=g)) else (flds[1], flds[0])
                u = torch.rand(6, generator=g).tolist()
                sgn = lambda v: 1.0 if v < 0.5 else -1.0   # noqa: E731
                # coefficients that are float32 values: the set, the restatement and the launch see the same numbers
                f32 = lambda v: float(torch.tensor(v, dtype=torch.float32))   # noqa: E731
                r = (OPS[kind], a, b, f32(sgn(u[0]) * (0.4 + 0.4 * u[1])), f32(sgn(u[2]) * (2.5 + u[3])), f32(0.4 + 0.4 * u[4]), f32(-(2.5 + u[5])))
            patch.append(p), cell.append(c), reading.append(r)
    order = torch.randperm(len(patch), generator=g).tolist()
    return [patch[i] for i in order], [cell[i] for i in order], [reading[i] for i in order]


@functools.lru_cache(maxsize=None)
def derived_sets(name):
    """name of a shape -> {set name: (patch, cell, reading)}; computed once, never modified."""
    c = host_case(name)
    groups, C_, P = c["groups"], c["n_inp"], c["P"]
    g = torch.Generator().manual_seed({"a": 201, "c": 203}[name])
    one = ([P - 1], [C_ - 1], [("magnitude", 0, 1, 0.75, 3.0, -0.5, -2.75)])
    if name == "a":
        return {"segments": _draw_readings(g, groups, C_, [(0, 1, 1), (0, 2, 15), (0, 3, 16), (0, 4, 17), (0, 5, 35), (1, 1, 3), (1, 6, 2)]),
                "g0": _draw_readings(g, groups, C_, [(0, 0, 4), (0, 8, 18)]),
                "one": one}
    return {"s15_16": _draw_readings(g, groups, C_, [(0, 0, 15), (0, 1, 16)]),
            "s17_35": _draw_readings(g, groups, C_, [(0, 0, 17), (0, 1, 35)]),
            "one": one}


def readings_of(reading):
    """The tuples of a set as what DerivedSensorSet takes: field ids and DerivedField."""
    from sea_amd.ensemble import DerivedField

    return [r if isinstance(r, int) else DerivedField(r[0], r[1], r[2], scale_a=r[3], shift_a=r[4], scale_b=r[5], shift_b=r[6]) for r in reading]


def make_set(dec, name, set_name):
    from sea_amd.ensemble import DerivedSensorSet

    patch, cell, reading = derived_sets(name)[set_name]
    return DerivedSensorSet(dec, host_case(name)["P"], patch, cell, readings_of(reading))


@functools.lru_cache(maxsize=None)
def derived_obs(name, set_name, hist):
    """Readings [hist, K]: random normal around 1, independent of the decoded values."""
    K = len(derived_sets(name)[set_name][0])
    g = torch.Generator().manual_seed(17000 + 13 * hist + len(set_name) + ord(name))
    return 1.0 + torch.randn(hist, K, generator=g)


@functools.lru_cache(maxsize=None)
def derived_precision(name, set_name, hist):
    """A precision per history and reading [hist, K] in [0.25, 4], about a quarter exactly 0 (missing readings); reading 0 keeps its weight."""
    K = len(derived_sets(name)[set_name][0])
    g = torch.Generator().manual_seed(19000 + 17 * hist + len(set_name) + ord(name))
    w = 0.25 + 3.75 * torch.rand(hist, K, generator=g)
    if K > 1:
        w[torch.rand(hist, K, generator=g) < 0.25] = 0.0
    w[:, 0] = 1.5
    return w


def every_set():
    return [(name, s) for name in SHAPES for s in derived_sets(name)]


# ------------------------------------------------------------------------------------------------ the contract, in fp64
def _components(reading):
    """(field a, field b, op code, sa, ha, sb, hb) per reading; a plain reading has op -1 and b = a."""
    fa = [r if isinstance(r, int) else r[1] for r in reading]
    fb = [r if isinstance(r, int) else r[2] for r in reading]
    op = torch.tensor([-1 if isinstance(r, int) else OPS.index(r[0]) for r in reading])
    co = torch.tensor([[1.0, 0.0, 1.0, 0.0] if isinstance(r, int) else list(r[3:7]) for r in reading], dtype=torch.float64)
    return fa, fb, op, co[:, 0], co[:, 1], co[:, 2], co[:, 3]


def _derived_value(ya, yb, op, sa, ha, sb, hb):
    """x and its two partial derivatives from the decoded source values, in the tensors' dtype (fp64): include/sea_hip.h, sea_decode_derived_sensor_grad."""
    a, b = ya * sa + ha, yb * sb + hb
    q = a * a + b * b
    zero, one = torch.zeros_like(q), torch.ones_like(q)
    pos = q > 0
    mag = torch.where(pos, torch.sqrt(torch.where(pos, q, one)), zero)
    safe = torch.where(pos, mag, one)
    x = torch.where(op < 0, ya, torch.where(op == 2, a - b, torch.where(op == 1, 0.5 * q, mag)))
    ga = torch.where(op < 0, one, torch.where(op == 2, sa * one, torch.where(op == 1, a * sa, torch.where(pos, a * sa / safe, zero))))
    gb = torch.where(op < 0, zero, torch.where(op == 2, -sb * one, torch.where(op == 1, b * sb, torch.where(pos, b * sb / safe, zero))))
    return x, ga, gb


def restate_derived_sensor(w1, w2, b2, groups, z, patch, cell, reading, obs, precision, members, round_bf16=False, autograd=False):
    """include/sea_hip.h, sea_decode_derived_sensor_sse / _grad, with the first decoder layer in front and its data gradient behind, in fp64.  The decode
    is tests/test_sensor_grad_cpu._forward on the 2 K component sensors (sources a, then sources b): exactly restate_sensor's values.  round_bf16: z, W1,
    the hidden rows and W2 are rounded to bf16 first and the two weighted residuals of a reading once each (what the fused launch computes with).
    autograd=True: dz by torch.autograd through the same forward instead of the written-out backward.
    Returns (wsse [Bm], pred [Bm, K], dz [Bm, P, G, D]) in float64."""
    import math

    f64 = torch.float64
    Bm, P, G, D = z.shape
    K = len(patch)
    fa, fb, op, sa, ha, sb, hb = _components(reading)
    assert [f for g in groups for f in g] == list(range(sum(len(g) for g in groups)))   # field ids are output positions in these shapes
    rnd = _bf16 if round_bf16 else (lambda t: t.to(f64))
    zz = z.detach().to(f64).requires_grad_(True) if autograd else z.detach()
    comp = _forward(w1, w2, b2, groups, zz, list(patch) * 2, list(cell) * 2, fa + fb, torch.zeros(Bm // members, 2 * K), None, members, rnd, round_bf16)
    y, pres, pos = comp[1], comp[4], comp[5]
    ya, yb = y[:, :K], y[:, K:]
    x, ga, gb = _derived_value(ya, yb, op, sa, ha, sb, hb)
    B = Bm // members
    assert tuple(obs.shape) == (B, K)
    o = obs.to(f64).repeat_interleave(members, dim=0)
    w = (torch.ones(B, K, dtype=f64) if precision is None else precision.to(f64).expand(B, K)).repeat_interleave(members, dim=0)
    live = w > 0
    d = torch.where(live, x - o, torch.zeros((), dtype=f64))
    w = torch.where(live, w, torch.zeros((), dtype=f64))
    wsse = (w * d * d).sum(1)
    if autograd:
        (dz,) = torch.autograd.grad(wsse.sum(), zz)
        return wsse.detach(), x.detach(), dz
    ra, rb = w * d * ga, w * d * gb
    if round_bf16:
        ra, rb = _bf16(ra), _bf16(rb)
    n_f = [len(g) for g in groups]
    C_ = w2[0].shape[0] // n_f[0]
    dY = torch.zeros(Bm, P, sum(n_f), C_, dtype=f64)
    bm = torch.arange(Bm).view(Bm, 1).expand(Bm, 2 * K)
    dY.index_put_((bm, torch.tensor(list(patch) * 2).expand(Bm, 2 * K), pos.expand(Bm, 2 * K), torch.tensor(list(cell) * 2).expand(Bm, 2 * K)),
                  2.0 * torch.cat([ra, rb], dim=1), accumulate=True)
    dz = torch.empty(Bm, P, G, D, dtype=f64)
    f0 = 0
    for g in range(G):
        dH = dY[:, :, f0:f0 + n_f[g]].reshape(Bm, P, n_f[g] * C_) @ rnd(w2[g])
        pre = pres[g]
        gelu_grad = 0.5 * (1.0 + torch.erf(pre / math.sqrt(2.0))) + pre * torch.exp(-0.5 * pre * pre) / math.sqrt(2.0 * math.pi)
        dz[:, :, g] = (dH * gelu_grad) @ rnd(w1[g])
        f0 += n_f[g]
    return wsse, x, dz


def _args(name, set_name, members, hist, with_prec, z=None):
    c = host_case(name)
    patch, cell, reading = derived_sets(name)[set_name]
    prec = derived_precision(name, set_name, hist) if with_prec else None
    return (c["w1"], c["w2"], c["b2"], c["groups"], c["z"] if z is None else z, patch, cell, reading, derived_obs(name, set_name, hist), prec, members)


@pytest.mark.parametrize("name,set_name", every_set())
def test_restated_backward_is_autograd_and_plain_readings_are_restate_sensor(name, set_name):
    c = host_case(name)
    patch, cell, reading = derived_sets(name)[set_name]
    members, hist = SPLITS[name][0]
    for with_prec in (False, True):
        args = _args(name, set_name, members, hist, with_prec)
        wsse, pred, dz = restate_derived_sensor(*args)
        w_a, p_a, dz_a = restate_derived_sensor(*args, autograd=True)
        e = rel(dz, dz_a)
        print(f"derived sensor shape {name} set {set_name} precision {with_prec}: written-out backward against autograd {e:.3e}")
        assert torch.equal(wsse, w_a) and torch.equal(pred, p_a) and e <= 1e-10
    plain = [k for k, r in enumerate(reading) if isinstance(r, int)]
    if plain:
        ref = restate_sensor(c["w1"], c["w2"], c["b2"], c["groups"], c["z"], [patch[k] for k in plain], [cell[k] for k in plain], [reading[k] for k in plain],
                             torch.zeros(hist, len(plain)), None, members)[1]
        assert torch.equal(pred[:, plain], ref)


def test_a_zero_speed_has_a_zero_finite_gradient_in_the_restatement():
    c = host_case("a")
    reading = [("magnitude", 0, 1, 0.0, 0.0, 0.0, 0.0), 2]
    wsse, pred, dz = restate_derived_sensor(c["w1"], c["w2"], c["b2"], c["groups"], c["z"], [3, 3], [5, 5], reading, torch.ones(1, 2), None, 2)
    assert float(pred[:, 0].abs().max()) == 0.0 and bool(torch.isfinite(dz).all()) and float(dz[:, 3, 0].abs().max()) == 0.0 and float(dz[:, 3, 1].abs().max()) > 0
    _, _, dz_a = restate_derived_sensor(c["w1"], c["w2"], c["b2"], c["groups"], c["z"], [3, 3], [5, 5], reading, torch.ones(1, 2), None, 2, autograd=True)
    assert torch.equal(dz, dz_a) or rel(dz, dz_a) <= 1e-12


# ------------------------------------------------------------------------------------------------ the conditions behind the GPU test's bounds
def _rounding_errors(args):
    ref = restate_derived_sensor(*args)
    rnd = restate_derived_sensor(*args, round_bf16=True)
    return rel(rnd[0], ref[0]), rel(rnd[1], ref[1]), rel(rnd[2], ref[2])


@pytest.mark.parametrize("name,set_name", every_set())
def test_bf16_rounding_stays_below_half_the_gpu_bound(name, set_name):
    """The GPU test allows 2e-2 against the fp64 restatement; what no bf16 path can avoid — z, W1, the hidden rows and W2 rounded to bf16, the two
    weighted residuals rounded once — must stay below 1e-2 on every input used there (tests/test_sensor_grad_cpu.py's rule)."""
    for members, hist in SPLITS[name]:
        for with_prec in (False, True):
            e_w, e_p, e_g = _rounding_errors(_args(name, set_name, members, hist, with_prec))
            print(f"derived sensor shape {name} set {set_name} members {members} x {hist} precision {with_prec}: bf16 roundings e(wsse) {e_w:.3e} e(pred) {e_p:.3e} e(dz) {e_g:.3e}")
            assert e_w <= 1e-2 and e_p <= 1e-2 and e_g <= 1e-2, (members, hist, e_w, e_p, e_g)


def test_bf16_rounding_stays_below_half_the_gpu_bound_at_130_members():
    for set_name in derived_sets("a"):
        e_w, e_p, e_g = _rounding_errors(_args("a", set_name, BIG["members"], BIG["hist"], True, z=big_states()))
        print(f"derived sensor shape a set {set_name} 130 members: bf16 roundings e(wsse) {e_w:.3e} e(pred) {e_p:.3e} e(dz) {e_g:.3e}")
        assert e_w <= 1e-2 and e_p <= 1e-2 and e_g <= 1e-2, (set_name, e_w, e_p, e_g)


@pytest.mark.parametrize("name,set_name", every_set())
def test_no_speed_of_the_gradient_inputs_is_near_zero(name, set_name):
    """The derivative of |u| is ill-conditioned at |u| -> 0: the fp64 speed at every magnitude reading of the gradient inputs is at least 0.25."""
    reading = derived_sets(name)[set_name][2]
    mags = [k for k, r in enumerate(reading) if not isinstance(r, int) and r[0] == "magnitude"]
    assert mags or set_name != "one"
    for z in ([None, big_states()] if name == "a" else [None]):
        members, hist = (BIG["members"], BIG["hist"]) if z is not None else SPLITS[name][0]
        pred = restate_derived_sensor(*_args(name, set_name, members, hist, False, z=z))[1]
        if mags:
            lo = float(pred[:, mags].min())
            print(f"derived sensor shape {name} set {set_name}: smallest fp64 speed {lo:.3f} over {len(mags)} magnitude readings")
            assert lo >= 0.25


def test_the_sets_cover_what_the_gpu_test_needs():
    for name in SHAPES:
        c = host_case(name)
        dec = make_decoder(name)
        sizes, ops_seen, plain, empty_groups, cells, ks = set(), set(), 0, 0, set(), set()
        for set_name, (patch, cell, reading) in derived_sets(name).items():
            s = make_set(dec, name, set_name)
            ks.add(s.K)
            for g in range(len(s.seg)):
                n_g = 0
                for qi in range(s.Q):
                    n = sum(s.live[s.seg[g][qi]:s.seg[g][qi + 1]])
                    sizes.add(n)
                    n_g += n
                empty_groups += n_g == 0
            cells |= set(cell)
            ops_seen |= {r[0] for r in reading if not isinstance(r, int)}
            plain += sum(isinstance(r, int) for r in reading)
            assert sorted(zip(patch, cell)) != list(zip(patch, cell)) or s.K == 1          # the given order is not the sorted one
        assert set(SEGMENT_SIZES) <= sizes and ops_seen == set(OPS) and plain >= 5 and c["n_inp"] - 1 in cells and 1 in ks, (name, sizes)
        assert empty_groups >= 1 or len(c["groups"]) == 1


# ------------------------------------------------------------------------------------------------ the pair tables
def _plain_only_b():
    from sea_amd.ensemble import DerivedSensorSet

    c = host_case("b")
    patch, cell, field = sensor_sets("b")["segments"]
    return DerivedSensorSet(make_decoder("b"), c["P"], patch, cell, field), (patch, cell, list(field))


@pytest.mark.parametrize("name,set_name", every_set() + [("b", "segments")])
def test_pair_tables(name, set_name):
    from sea_amd import _native as N
    from sea_amd.ensemble import SensorSet

    c = host_case(name)
    dec = make_decoder(name)
    if name == "b":
        s, (patch, cell, reading) = _plain_only_b()
    else:
        patch, cell, reading = derived_sets(name)[set_name]
        s = make_set(dec, name, set_name)
    assert isinstance(s, SensorSet) and s.fusable
    K, G, Cp, T = len(patch), len(c["groups"]), dec._n_inp_p, N.SENSOR_TILE
    fa, fb, op, sa, ha, sb, hb = _components(reading)
    grp_of = {f: g for g, grp in enumerate(c["groups"]) for f in grp}
    row = lambda f, cc: c["groups"][grp_of[f]].index(f) * Cp + cc   # noqa: E731
    tabs = (s.perm, s.wrow, s.live, s.op, s.scale, s.shift)
    assert s.K == K and all(len(t) == s.K_pad for t in tabs) and s.K_pad % T == 0 and s.K_pad >= T
    assert s.patches == sorted(set(patch)) and s.Q == len(s.patches) and len(s.seg) == G and all(len(r) == s.Q + 1 for r in s.seg)
    flat = [v for r in s.seg for v in r]
    assert flat[0] == 0 and flat[-1] == s.K_pad and all(a <= b and (b - a) % T == 0 for a, b in zip(flat, flat[1:]))       # steps of 32
    assert sum(s.live) == K and all(s.live[i] == 0 and s.op[i] == -1 for i in range(1, s.K_pad, 2))                        # the second entry of a pair: never live, no op
    for g in range(G):
        for qi, p in enumerate(s.patches):
            a, b = s.seg[g][qi], s.seg[g][qi + 1]
            want = [k for k in range(K) if grp_of[fa[k]] == g and patch[k] == p]
            assert b - a == -(-2 * len(want) // T) * T                                                                     # 16 readings per tile
            for i, k in enumerate(want):                                                                                   # pairs adjacent, in the given order
                e = a + 2 * i
                assert e % 2 == 0 and s.perm[e] == s.perm[e + 1] == k and s.live[e] == 1 and s.inv[k] == e
                assert s.wrow[e] == row(fa[k], cell[k]) and s.op[e] == int(op[k])
                if int(op[k]) < 0:                                                                                         # plain: op -1, the second row is row 0
                    assert s.wrow[e + 1] == 0 and (s.scale[e], s.shift[e], s.scale[e + 1], s.shift[e + 1]) == (1.0, 0.0, 1.0, 0.0)
                else:
                    assert s.wrow[e + 1] == row(fb[k], cell[k]) and grp_of[fb[k]] == g
                    assert (s.scale[e], s.shift[e], s.scale[e + 1], s.shift[e + 1]) == (float(sa[k]), float(ha[k]), float(sb[k]), float(hb[k]))
            for e in range(a + 2 * len(want), b):                                                                          # pad entries
                assert (s.perm[e], s.wrow[e], s.live[e], s.op[e], s.scale[e], s.shift[e]) == (0, 0, 0, -1, 1.0, 0.0)
    assert sorted(s.inv) == sorted(set(s.inv)) and [s.perm[e] for e in s.inv] == list(range(K))                            # the inv round trip
    assert s.matches(dec, c["P"]) and not s.matches(dec, c["P"] + 1)
    t = s.tables("cpu")
    assert t["op"].dtype == torch.int32 and t["scale"].dtype == t["shift"].dtype == torch.float32 and t["inv"].tolist() == s.inv and t["op"].tolist() == s.op
    if name == "b":                                                                  # SensorSet itself is untouched: the same segments at twice the length
        plain = SensorSet(dec, c["P"], patch, cell, reading)
        assert plain.patches == s.patches and [k for k, l in zip(plain.perm, plain.live) if l] == [k for k, l in zip(s.perm, s.live) if l]


# ------------------------------------------------------------------------------------------------ the composed float32 arithmetic
def test_composed_readings_are_numpy_float32_arithmetic_bit_for_bit():
    """DerivedSensorSet.composed_predictions on CPU tensors against numpy float32 arithmetic, every operation rounded once, numpy's float32 root
    (correctly rounded), as tests/test_derived_fields_cpu.py holds _composed_derived."""
    for name, set_name in every_set():
        c = host_case(name)
        s = make_set(make_decoder(name), name, set_name)
        patch, cell, reading = derived_sets(name)[set_name]
        fa, fb, op, sa, ha, sb, hb = _components(reading)
        g = torch.Generator().manual_seed(5)
        Y = torch.randn(7, c["P"], sum(len(gr) for gr in c["groups"]), c["n_inp"], generator=g) * 3.0
        Y[0] = 0.0
        got = s.composed_predictions(Y)
        y = Y.numpy()
        ya, yb = y[:, patch, fa, cell], y[:, patch, fb, cell]
        f = lambda t: t.numpy().astype(np.float32)   # noqa: E731
        a = ya * f(sa) + f(ha)
        b = yb * f(sb) + f(hb)
        q = a * a + b * b
        assert a.dtype == b.dtype == q.dtype == np.float32
        opn = op.numpy()
        want = np.where(opn < 0, ya, np.where(opn == 2, a - b, np.where(opn == 1, q * np.float32(0.5), np.sqrt(q))))
        assert got.dtype == torch.float32 and got.shape == (7, s.K) and np.array_equal(got.numpy().view(np.uint32), want.astype(np.float32).view(np.uint32))
    # a zero speed: the value 0 and a zero, finite gradient through the composed arithmetic
    from sea_amd.ensemble import DerivedField, DerivedSensorSet

    s0 = DerivedSensorSet(make_decoder("a"), 9, [3], [5], [DerivedField("magnitude", 0, 1)])
    Y = torch.zeros(2, 9, 3, 12, requires_grad=True)
    x = s0.composed_predictions(Y)
    x.sum().backward()
    assert float(x.detach().abs().max()) == 0.0 and float(Y.grad.abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ refusals of the Python layers
def test_the_set_refuses_bad_inputs():
    from sea_amd.ensemble import DerivedField, DerivedSensorSet, SensorSet

    dec = make_decoder("a")   # groups [[0, 1], [2]], n_inp 12
    sp = DerivedField("magnitude", 0, 1)
    ok = dict(patch=[0, 1, 8], cell=[3, 4, 11], reading=[0, sp, 2])
    s = DerivedSensorSet(dec, 9, **ok)
    assert s.K == 3 and s.fusable and s.plain == [True, False, True] and s.field == [0, None, 2] and s.out_field == [0, None, 2]
    DerivedSensorSet(dec, 9, torch.tensor([0, 1]), torch.tensor([3, 4], dtype=torch.int32), torch.tensor([0, 2]))       # plain readings as a tensor
    DerivedSensorSet(dec, 9, [1, 1], [3, 3], [sp, sp])                                                               # duplicates
    bad = [dict(patch=[0, 1, 9]), dict(patch=[-1, 0, 0]), dict(cell=[3, 4, 12]), dict(cell=[-1, 0, 0]), dict(reading=[0, sp, 3]), dict(reading=[0, sp, -1]),
           dict(reading=[0, sp, True]), dict(reading=[0, sp, 1.0]), dict(reading=[0, sp, "magnitude"]), dict(reading=[0, sp, ("magnitude", 0, 1)]),
           dict(reading=[0, sp]), dict(reading=3), dict(reading=None), dict(reading=[0, DerivedField("energy", 0, 3), 2]), dict(patch=[]),
           dict(patch=[0, 1]), dict(cell=[1.0, 2.0, 3.0]), dict(patch=[True, False, True])]
    for kw in bad:
        args = dict(ok)
        args.update(kw)
        with pytest.raises(ValueError):
            DerivedSensorSet(dec, 9, **args)
    for n in (0, -1, True, 2.0):
        with pytest.raises(ValueError):
            DerivedSensorSet(dec, n, **ok)
    for kw in (dict(affine=([1.0], [0.0])), dict(points=[0, 1])):
        with pytest.raises(ValueError):
            DerivedSensorSet(dec, 9, **ok, **kw)
    with pytest.raises(ValueError, match="not built from a mesh"):
        s.scale_values(torch.zeros(3))
    # sources in different groups: accepted, not fusable, no launch tables
    x = DerivedSensorSet(dec, 9, [0, 1], [3, 4], [DerivedField("difference", 0, 2), 1])
    assert not x.fusable and x.K_pad is None and x.K == 2 and x.Q == 2 and x.patches == [0, 1] and "wrow" not in x.tables("cpu")
    # SensorSet is what it was
    p = SensorSet(dec, 9, [0, 1, 8], [3, 4, 11], [0, 1, 2])
    assert not hasattr(p, "op") and p.K_pad == 96 and set(p.tables("cpu")) == {"perm", "wrow", "live", "seg", "patches", "inv", "patch", "cell", "out_field"}


def test_the_consumers_refuse_before_a_device_is_touched():
    from sea_amd.ensemble import (DerivedField, DerivedSensorSet, SensorKalman, SensorLikelihood, SensorThresholdVerification, SensorVerification)

    c = host_case("a")
    dec = make_decoder("a").requires_grad_(False).set_compute_dtype("bf16")        # sensor_loss takes a frozen decoder
    P, D, G = c["P"], c["D"], len(c["groups"])
    sp = DerivedField("magnitude", 0, 1, 2.0, 0.5, 3.0, -1.0)
    s = DerivedSensorSet(dec, P, [0, 1, 8], [3, 4, 11], [0, sp, 2])
    cross = DerivedSensorSet(dec, P, [0, 1, 8], [3, 4, 11], [0, DerivedField("difference", 1, 2), 2])
    z, obs = torch.zeros(4, P, G, D), torch.zeros(2, 3)
    bad = [dict(z=torch.zeros(4, P, G)), dict(members=3), dict(obs=torch.zeros(2, 4)), dict(obs=torch.zeros(2, 6)), dict(obs=torch.zeros(2, 3, dtype=torch.float64)),
           dict(precision=torch.ones(4)), dict(precision=torch.tensor([1.0, -1.0, 1.0])), dict(sensors=DerivedSensorSet(dec, P + 1, [0], [0], [sp])),
           dict(sensors=cross, fused=True)]
    for fn in (dec.sensor_sse, dec.sensor_loss):
        for kw in bad:
            args = dict(z=z, sensors=s, obs=obs, precision=None, members=2)
            args.update(kw)
            zz = args.pop("z")
            with pytest.raises(ValueError):
                fn(zz, **args)
        with pytest.raises(ValueError, match="different decoder groups"):
            fn(z, cross, obs, members=2, fused=True)
        with pytest.raises(ValueError, match="bf16 only"):
            getattr(make_decoder("a").requires_grad_(False), fn.__name__)(z, s, obs, members=2, fused=True)
        with pytest.raises(RuntimeError, match="MI355X"):                                                              # well-formed, but on the host
            fn(z, s, obs, members=2)
        with pytest.raises(RuntimeError, match="MI355X"):                                                              # fused=None: the composed path for this set
            fn(z, cross, obs, members=2)
    # sigma: a number or K numbers; the per-field form is refused for this set (here K == n_fields == 3: three numbers are per READING)
    assert SensorLikelihood(dec, P, 2, s, sigma=2.0)._prec_host == [0.25] * 3 and SensorLikelihood(dec, P, 2, s)._prec_host is None
    assert SensorLikelihood(dec, P, 2, s, sigma=[0.5, 1.0, 2.0])._prec_host == [4.0, 1.0, 0.25]
    s4 = DerivedSensorSet(dec, P, [0, 1, 8, 8], [3, 4, 11, 0], [0, sp, 2, sp])
    assert SensorLikelihood(dec, P, 2, s4, sigma=[1.0, 2.0, 4.0, 0.5])._prec_host == [1.0, 0.25, 0.0625, 4.0]
    for cls, kw in ((SensorLikelihood, {}), (SensorKalman, {}), (SensorVerification, {})):
        with pytest.raises(ValueError, match="one per reading"):
            cls(dec, P, 2, s4, sigma=[1.0, 2.0, 3.0], **kw)                                                            # n_fields numbers: refused
        for sig in (0.0, -1.0, [1.0, 2.0], torch.ones(2, 4)):
            with pytest.raises(ValueError):
                cls(dec, P, 2, s4, sigma=sig, **kw)
        with pytest.raises(ValueError):
            cls(dec, P + 1, 2, s4, **kw)
    # thresholds of the exceedance verification: [T] or [T, K] (one column per reading)
    assert tuple(SensorThresholdVerification(dec, P, 2, s4, [0.5, 1.0]).thresholds.shape) == (2, 4)
    assert tuple(SensorThresholdVerification(dec, P, 2, s4, torch.ones(2, 4)).thresholds.shape) == (2, 4)
    with pytest.raises(ValueError):
        SensorThresholdVerification(dec, P, 2, s4, torch.ones(2, 3))                                                   # n_fields columns: refused for this set
    y = torch.zeros(4, G, P * D)
    like = SensorLikelihood(dec, P, 2, s)
    for yy, oo, pp in ((torch.zeros(3, G, P * D), obs, None), (y, torch.zeros(2, 2), None), (y, obs, torch.tensor([1.0, -2.0, 1.0]))):
        with pytest.raises(ValueError):
            like(yy, oo, pp)
        with pytest.raises(ValueError):
            like.score_and_grad(yy, oo, pp)
    with pytest.raises(ValueError, match="different decoder groups"):
        SensorLikelihood(dec, P, 2, cross, fused=True).score_and_grad(y, obs)
    with pytest.raises(RuntimeError, match="MI355X"):
        like(y, obs, torch.ones(3))
    with pytest.raises(RuntimeError, match="MI355X"):
        like.score_and_grad(y, obs)
    with pytest.raises(ValueError):
        SensorKalman(dec, P, 2, s, taper=torch.ones(P, 4))                                                             # one column per reading: K = 3


def test_ops_refuse_malformed_tables_on_the_host():
    from sea_amd import ops

    def args(**kw):
        Q, Bm, S, Cp, K_pad = 2, 4, 40, 32, 64
        a = dict(groups=[dict(H=torch.zeros(Q * Bm, S, dtype=torch.bfloat16), W2=torch.zeros(n * Cp, S, dtype=torch.bfloat16), bias=torch.zeros(n * Cp),
                              dH=torch.zeros(Q * Bm, S, dtype=torch.bfloat16)) for n in (2, 1)],
                 obs=torch.zeros(2, K_pad), live=torch.zeros(K_pad, dtype=torch.int32), wrow=torch.zeros(K_pad, dtype=torch.int32),
                 seg=torch.zeros(2, Q + 1, dtype=torch.int32), op=torch.full((K_pad,), -1, dtype=torch.int32), scale=torch.ones(K_pad), shift=torch.zeros(K_pad),
                 Cp=Cp, members=2, prec=None)
        a.update(kw)
        return a

    for fn in (ops.decode_derived_sensor_sse, ops.decode_derived_sensor_grad):
        with pytest.raises(RuntimeError, match="MI355X"):
            fn(**args())
        bad = [dict(op=torch.zeros(64, dtype=torch.int64)), dict(op=torch.zeros(32, dtype=torch.int32)), dict(scale=torch.ones(64, dtype=torch.float64)),
               dict(shift=torch.zeros(128)[::2]), dict(scale=torch.ones(65)[1:]), dict(shift=None), dict(op=torch.zeros(2, 32, dtype=torch.int32)),
               dict(dtype=torch.float32), dict(Cp=12), dict(members=3), dict(obs=torch.zeros(2, 32)), dict(prec=torch.ones(32)), dict(live=torch.zeros(64, dtype=torch.int64))]
        for kw in bad:
            with pytest.raises(ValueError, match=fn.__name__):
                fn(**args(**kw))
    with pytest.raises(ValueError, match="grad_scale"):
        ops.decode_derived_sensor_grad(**args(grad_scale=float("inf")))


# ------------------------------------------------------------------------------------------------ the entry points, without a GPU
@pytest.fixture(scope="module")
def lib():
    from sea_amd import build, _native

    build.build(verbose=False)
    return _native.lib()


def _tables():
    from sea_amd import _native as N

    t = N.SeaDerivedSensorTables()
    t.op, t.scale, t.shift = 0x200000, 0x210000, 0x220000
    return t


def _grad_table():
    """tests/test_sensor_cpu._table as a SeaDecodeSensorGrad table with dH given."""
    from sea_amd import _native as N

    g, p = _table()
    for i in range(2):
        g[i].dH, g[i].lddh = 0x10000 * (i + 1) + 0x3000, 40
    q = N.SeaDecodeSensorGrad()
    for name, _ in N.SeaDecodeSensorSse._fields_:
        setattr(q, name, getattr(p, name))
    q.grad_scale = 1.0
    return g, q


ENTRY = {"sse": ("sea_decode_derived_sensor_sse", _table), "grad": ("sea_decode_derived_sensor_grad", _grad_table)}


def test_symbols_struct_size_and_unchanged_struct_sizes(lib):
    from sea_amd import _native as N

    assert C.sizeof(N.SeaDerivedSensorTables) == 24                  # include/sea_hip.h states it
    assert N.SeaDerivedSensorTables.op.offset == 0 and N.SeaDerivedSensorTables.scale.offset == 8 and N.SeaDerivedSensorTables.shift.offset == 16
    for sym, _ in ENTRY.values():
        assert hasattr(lib, sym) and sym in N.EXPORTED_SYMBOLS
    assert lib.sea_abi_version() == 8 and len(N.ABI_STRUCTS) == 33 and N.ABI_STRUCTS[-1] is N.SeaKvFork and N.SeaDerivedSensorTables not in N.ABI_STRUCTS
    out = (C.c_int * 64)()
    n = lib.sea_struct_sizes(out, 64)
    assert n == 33 and [out[i] for i in range(n)] == [C.sizeof(s) for s in N.ABI_STRUCTS]          # sea_struct_sizes() is what it was
    # the library reads the fields where the binding writes them
    for which, (sym, make) in ENTRY.items():
        fn = getattr(lib, sym)
        g, p = make()
        p.members = 3
        assert fn(g, 2, C.byref(p), C.byref(_tables()), N.SEA_BF16, None) == -1 and b"Bm=4 must be a positive multiple of members=3" in lib.sea_last_error()
        g, p = make()
        p.work_cap -= 1
        assert fn(g, 2, C.byref(p), C.byref(_tables()), N.SEA_BF16, None) == -1 and b"workspace of 23 floats is too small: 24 needed" in lib.sea_last_error()
        assert sym.encode() in lib.sea_last_error()


TABLE_BREAKS = {"null op": ("op", None), "null scale": ("scale", None), "null shift": ("shift", None), "misaligned op": ("op", 0x200004),
                "misaligned scale": ("scale", 0x210008), "misaligned shift": ("shift", 0x220002)}
PLAIN_BREAKS = {"null obs": ("obs", None), "null live": ("live", None), "null wrow": ("wrow", None), "null seg": ("seg", None), "null wsse": ("wsse", None),
                "null work": ("work", None), "misaligned obs": ("obs", 0x100008), "misaligned prec": ("prec", 0x110004), "misaligned pred": ("pred", 0x160008),
                "misaligned live": ("live", 0x120002), "misaligned seg": ("seg", 0x140002), "K_pad = 48": ("K_pad", 48), "Bm = 0": ("Bm", 0), "S = 36": ("S", 36),
                "Cp = 48": ("Cp", 48), "Q too large": ("Q", 65536), "ld_obs % 4": ("ld_obs", 130), "ld_prec short": ("ld_prec", 64)}


@pytest.mark.parametrize("which", sorted(ENTRY))
@pytest.mark.parametrize("what", sorted(TABLE_BREAKS) + sorted(PLAIN_BREAKS) + ["null tables", "null p", "null groups", "null group pointer", "misaligned operand",
                                                                                   "short row stride", "no groups", "too many groups", "bad dtype"])
def test_the_entry_points_refuse_bad_arguments_without_a_device(lib, which, what):
    from sea_amd import _native as N

    sym, make = ENTRY[which]
    fn = getattr(lib, sym)
    g, p = make()
    t = _tables()
    n, dt, pa, ta, ga = 2, N.SEA_BF16, C.byref(p), C.byref(t), g
    if what in TABLE_BREAKS:
        setattr(t, *TABLE_BREAKS[what])
    elif what in PLAIN_BREAKS:
        setattr(p, *PLAIN_BREAKS[what])
    elif what == "null tables":
        ta = None
    elif what == "null p":
        pa = None
    elif what == "null groups":
        ga = None
    elif what == "null group pointer":
        g[1].bias = None
    elif what == "misaligned operand":
        g[0].W2 = 0x11008
    elif what == "short row stride":
        g[1].ldh = 32
    elif what == "no groups":
        n = 0
    elif what == "too many groups":
        n = 17
    else:
        dt = 7
    assert fn(ga, n, pa, ta, dt, None) == -1, what
    msg = lib.sea_last_error()
    assert sym.encode() in msg
    if what in TABLE_BREAKS:
        assert b"op, scale" in msg and (b"null" in msg) == what.startswith("null")
    if what in ("null group pointer", "short row stride"):
        assert b"group 1" in msg
    if what == "misaligned operand":
        assert b"group 0" in msg


def test_gradient_only_refusals_and_unsupported_forms(lib):
    from sea_amd import _native as N

    sym, make = ENTRY["grad"]
    fn = getattr(lib, sym)
    for brk, frag in (("dH", b"group 0"), ("lddh", b"lddh=32"), ("Z", b"group 0"), ("grad_scale", b"grad_scale must be finite")):
        g, p = make()
        if brk == "dH":
            g[0].dH = None
        elif brk == "lddh":
            g[0].lddh = 32
        elif brk == "Z":
            g[0].Z, g[0].ldz = 0x19008, 40
        else:
            p.grad_scale = float("nan")
        assert fn(g, 2, C.byref(p), C.byref(_tables()), N.SEA_BF16, None) == -1 and frag in lib.sea_last_error() and sym.encode() in lib.sea_last_error(), brk
    for which, (sym, make) in ENTRY.items():
        fn = getattr(lib, sym)
        g, p = make()
        assert fn(g, 2, C.byref(p), C.byref(_tables()), N.SEA_F32, None) == -3 and b"bf16 only" in lib.sea_last_error() and sym.encode() in lib.sea_last_error()
        g, p = make()
        p.S = 648
        for i in range(2):
            g[i].ldh = g[i].ldw = g[i].lddh = 648
        assert fn(g, 2, C.byref(p), C.byref(_tables()), N.SEA_BF16, None) == -3 and b"S=648" in lib.sea_last_error()
        g, p = make()   # prec and pred may be NULL: the table then fails only at the last check, which this breaks
        p.prec = p.pred = None
        p.work_cap -= 1
        assert fn(g, 2, C.byref(p), C.byref(_tables()), N.SEA_BF16, None) == -1 and b"workspace of 23 floats is too small" in lib.sea_last_error()


# ------------------------------------------------------------------------------------------------ sensors on a mesh
def test_derived_sensor_set_on_a_synthetic_partitioner():
    from sea_amd.ensemble import DerivedField, DerivedSensorSet
    from sea_amd.models.encoder_decoder import Decode
    from sea_amd.utils.data_processors import DataPartitioner2D, MeshProcessor, MeshUnpatcher, MinMaxScaler

    g = torch.Generator().manual_seed(3)   # the partitioner of tests/test_sensor_cpu.py::test_sensor_set_on_a_synthetic_partitioner
    n_pts = 57
    x, y = torch.rand(n_pts, generator=g), torch.rand(n_pts, generator=g)
    part = DataPartitioner2D(x, y, m=4, n=3, device="cpu")
    P, C_ = part.padded_index_map.shape
    groups = [[0, 1], [2]]
    data = torch.randn(5, n_pts, 3, generator=g) * torch.tensor([1.0, 10.0, 0.1]) + torch.tensor([0.0, 5.0, -1.0])
    scalers = [MinMaxScaler((-1, 1)), MinMaxScaler((0, 2))]
    for sc, grp in zip(scalers, groups):
        sc.fit(data[:, :, grp])
    mesh = MeshUnpatcher(part, groups, scalers)
    dec = Decode(groups, C_, 16, 8)
    points = torch.randperm(n_pts, generator=g)[:10].tolist() + [0, 0]
    readings = [2, ("magnitude", 0, 1), 0, ("difference", 1, 0, "tap"), ("energy", 0, 1), 1, ("magnitude", 1, 0), 2, 2, ("difference", 0, 2), 0, ("magnitude", 0, 1)]
    s = mesh.derived_sensor_set(dec, points, readings)
    assert isinstance(s, DerivedSensorSet) and s.K == 12 and s.n_patches == P and s.matches(dec, P) and s.points == points
    assert not s.fusable                                                            # reading 9 pairs fields of two groups
    imap = part.padded_index_map
    for k, pt in enumerate(points):
        assert int(imap[s.patch[k], s.cell[k]]) == pt
    dfs = mesh.derived_fields([r for r in readings if isinstance(r, tuple)])        # derived readings carry the INVERSE affine of their sources
    assert [r for r in s.reading if isinstance(r, DerivedField)] == dfs and dfs[1].name == "tap"
    a, b = mesh._forward_coefficients()                                             # plain readings the forward affine; derived ones pass through
    v = torch.randn(12, generator=g)
    want = torch.stack([v[k] * torch.tensor(a[r], dtype=torch.float32) + torch.tensor(b[r], dtype=torch.float32) if isinstance(r, int) else v[k]
                        for k, r in enumerate(readings)])
    assert torch.equal(s.scale_values(v), want)
    sig = torch.rand(12, generator=g)
    assert torch.equal(s.scale_sigma(sig), sig * torch.tensor([abs(a[r]) if isinstance(r, int) else 1.0 for r in readings], dtype=torch.float32))
    as_np = mesh.derived_sensor_set(dec, points[:3], [np.int64(2), ("magnitude", 0, 1), torch.tensor(0)])   # field ids as DerivedSensorSet itself takes them
    assert as_np.field == [2, None, 0] and as_np.plain == [True, False, True]
    fus = mesh.derived_sensor_set(dec, points[:9], readings[:9])
    assert fus.fusable and fus.K_pad % 32 == 0
    taper = mesh.sensor_taper(fus, 0.5)                                             # the set carries its mesh points: sensor_taper keeps working
    assert tuple(taper.shape) == (P, 9) and torch.equal(taper, mesh.sensor_taper(mesh.sensor_set(dec, points[:9], [0] * 9), 0.5))
    for pts, rd in (([n_pts], [0]), ([-1], [0]), ([0], [3]), ([0, 1], [0]), ([0], [("magnitude", 0, 3)]), ([0], [("speed", 0, 1)]), ([0], [("magnitude", 0)]),
                    ([0], [0.5]), ([0], [True]), ([], []), ([0], 0)):
        with pytest.raises(ValueError):
            mesh.derived_sensor_set(dec, pts, rd)
    with pytest.raises(ValueError):
        mesh.derived_sensor_set(Decode(groups, C_ - 1, 16, 8), [int(imap[0, 0])], [0])
    proc = MeshProcessor(dict(dimension="2D", field_groups=groups, m=4, n=3), torch.stack([x, y]), device="cpu")
    with pytest.raises(ValueError, match="patchify_and_scale first"):
        proc.derived_sensor_set(dec, [0], [0])
