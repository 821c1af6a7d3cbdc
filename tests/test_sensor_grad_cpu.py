"""The latent gradient of the sparse-sensor score (sea_decode_sensor_grad, Decode.sensor_loss, SensorLikelihood.score_and_grad / nudge) without a
GPU: the contract restated in fp64 with its backward written out (`restate_sensor_grad`), checked against torch.autograd on a differentiable fp64
copy of the forward and tied to the reference-generated goldens (every valid cell as a sensor is the dense loss and its dz), the neutrality of
readings without weight, the condition under which the GPU test's bound is meaningful (bf16-rounded operands and the once-rounded weighted
residual stay within half of it), the entry point's argument checks and the refusals of the Python layers.

`restate_sensor_grad` is what tests/test_sensor_grad_gpu.py compares with.  Shapes, sensor sets, readings and precisions are those of
tests/test_sensor_cpu.py.  GRAD_SETS lists the sets the gradient tests use: every set of every shape (none had to be dropped: the figures
test_bf16_rounding_stays_within_half_the_gpu_bound prints are all below TOL_BF16 / 2)."""
import ctypes as C
import math

import pytest
import torch

from tests.test_decode_loss_cpu import load_fixture, rel
from tests.test_sensor_cpu import BIG, SHAPES, SPLITS, _bf16, big_states, host_case, make_decoder, restate_sensor, sensor_obs, sensor_precision, sensor_sets

TOL_BF16 = 2e-2   # tests/test_decode_loss_gpu.py::TOL_BF16 (that module is imported lazily: see host_case)
GRAD_SETS = [(name, s) for name in SHAPES for s in sensor_sets(name)]


# ------------------------------------------------------------------------------------------------ the contract, in fp64
def _forward(w1, w2, b2, groups, z, patch, cell, field, obs, precision, members, rnd, round_h):
    """restate_sensor's forward, expression by expression, on tensors that may carry a graph: (wsse, pred, w, d, pres)."""
    f64 = torch.float64
    Bm, P, G, D = z.shape
    n_f = [len(g) for g in groups]
    C_ = w2[0].shape[0] // n_f[0]
    flat = [f for g in groups for f in g]
    Ys, pres = [], []
    for g in range(G):
        pre = rnd(z[:, :, g]) @ rnd(w1[g]).t()
        H = 0.5 * pre * (1.0 + torch.erf(pre / math.sqrt(2.0)))
        if round_h:
            H = _bf16(H)
        Ys.append((H @ rnd(w2[g]).t() + b2[g].to(f64)).view(Bm, P, n_f[g], C_))
        pres.append(pre)
    Y = torch.cat(Ys, dim=2)
    pos = torch.tensor([flat.index(f) for f in field])
    pred = Y[:, torch.tensor(patch), pos, torch.tensor(cell)]
    B, K = Bm // members, len(patch)
    assert Bm % members == 0 and tuple(obs.shape) == (B, K)
    o = obs.to(f64).repeat_interleave(members, dim=0)
    w = torch.ones(B, K, dtype=f64) if precision is None else precision.to(f64).expand(B, K)
    w = w.repeat_interleave(members, dim=0)
    live = w > 0
    d = torch.where(live, pred - o, torch.zeros((), dtype=f64))
    w = torch.where(live, w, torch.zeros((), dtype=f64))
    return (w * d * d).sum(1), pred, w, d, pres, pos


def restate_sensor_grad(w1, w2, b2, groups, z, patch, cell, field, obs, precision, members, round_bf16=False):
    """include/sea_hip.h, sea_decode_sensor_grad, with the first decoder layer in front of it and its data gradient behind it, in fp64, the backward
    written out (no autograd).  Arguments as tests/test_sensor_cpu.restate_sensor.  round_bf16: z, W1, the hidden rows and W2 are rounded to bf16 first
    and the weighted residual r = w d once between the two products (what the fused launch computes with).
    Returns (wsse [Bm], pred [Bm, K], dz [Bm, P, G, D]) in float64: dz[bm] = d wsse[bm] / d z[bm]."""
    f64 = torch.float64
    Bm, P, G, D = z.shape
    n_f = [len(g) for g in groups]
    C_ = w2[0].shape[0] // n_f[0]
    rnd = _bf16 if round_bf16 else (lambda t: t.detach().to(f64))
    wsse, pred, w, d, pres, pos = _forward(w1, w2, b2, groups, z.detach(), patch, cell, field, obs, precision, members, rnd, round_bf16)
    r = w * d                                                                           # [Bm, K]
    if round_bf16:
        r = _bf16(r)
    dY = torch.zeros(Bm, P, sum(n_f), C_, dtype=f64)
    K = len(patch)
    bm = torch.arange(Bm).view(Bm, 1).expand(Bm, K)
    dY.index_put_((bm, torch.tensor(patch).expand(Bm, K), pos.expand(Bm, K), torch.tensor(cell).expand(Bm, K)), 2.0 * r, accumulate=True)   # duplicates add
    dz = torch.empty(Bm, P, G, D, dtype=f64)
    f0 = 0
    for g in range(G):
        dH = dY[:, :, f0:f0 + n_f[g]].reshape(Bm, P, n_f[g] * C_) @ rnd(w2[g])
        pre = pres[g]
        gelu_grad = 0.5 * (1.0 + torch.erf(pre / math.sqrt(2.0))) + pre * torch.exp(-0.5 * pre * pre) / math.sqrt(2.0 * math.pi)
        dz[:, :, g] = (dH * gelu_grad) @ rnd(w1[g])
        f0 += n_f[g]
    return wsse, pred, dz


def autograd_sensor_grad(w1, w2, b2, groups, z, patch, cell, field, obs, precision, members):
    """The same forward as a differentiable fp64 graph; dz by torch.autograd."""
    zz = z.detach().to(torch.float64).requires_grad_(True)
    wsse = _forward(w1, w2, b2, groups, zz, patch, cell, field, obs, precision, members, lambda t: t.to(torch.float64), False)[0]
    (dz,) = torch.autograd.grad(wsse.sum(), zz)
    return wsse.detach(), dz


@pytest.mark.parametrize("name,set_name", GRAD_SETS)
def test_restated_backward_is_autograd_and_the_forward_is_restate_sensor(name, set_name):
    c = host_case(name)
    patch, cell, field = sensor_sets(name)[set_name]
    for members, hist in SPLITS[name]:
        obs = sensor_obs(name, set_name, hist)
        for prec in (None, sensor_precision(name, set_name, hist)):
            args = (c["w1"], c["w2"], c["b2"], c["groups"], c["z"], patch, cell, field, obs, prec, members)
            wsse, pred, dz = restate_sensor_grad(*args)
            ref_w, ref_p = restate_sensor(*args)
            assert torch.equal(wsse, ref_w) and torch.equal(pred, ref_p)
            _, dz_a = autograd_sensor_grad(*args)
            e = rel(dz, dz_a)
            print(f"sensor_grad shape {name} set {set_name} members {members} x {hist} precision {prec is not None}: written-out backward against autograd {e:.3e}")
            assert e <= 1e-10, (members, hist, e)
            w_r, p_r = restate_sensor(*args, round_bf16=True)
            got = restate_sensor_grad(*args, round_bf16=True)
            assert torch.equal(got[0], w_r) and torch.equal(got[1], p_r)


@pytest.mark.parametrize("name", ["decode_mse_a", "decode_mse_b"])
def test_every_valid_cell_as_a_sensor_is_the_reference_loss_and_gradient(name):
    """Every valid cell of every field as a sensor, unit precision, members = 1, readings = the golden target there: sum(wsse) / n is the
    reference's loss and d sum(wsse) / dz / n its dz (tests/golden/decode_mse_*.npz), with the tolerance tests/test_decode_loss_cpu.py uses."""
    fx = load_fixture(name)
    C_, P, B = fx["n_inp"], fx["P"], fx["B"]
    fields = [f for g in fx["groups"] for f in g]
    for counts, ref_loss, ref_dz in ((None, fx["loss"], fx["dz"]), (fx["counts"].tolist(), fx["loss_masked"], fx["dz_masked"])):
        patch, cell, field = [], [], []
        for p in range(P):
            for f in fields:
                for cc in range(C_ if counts is None else counts[p]):
                    patch.append(p), cell.append(cc), field.append(f)
        n = B * len(patch)
        obs = fx["target"].to(torch.float64)[:, torch.tensor(patch), torch.tensor(field), torch.tensor(cell)]
        wsse, _, dz = restate_sensor_grad(fx["w1"], fx["w2"], fx["b2"], fx["groups"], fx["z"], patch, cell, field, obs, None, 1)
        assert rel(wsse.sum() / n, ref_loss) <= 1e-9
        assert rel(dz / n, ref_dz) <= 1e-9


def test_neutrality_duplicates_and_exact_zeros_in_the_restatement():
    c = host_case("a")
    groups, P = c["groups"], c["P"]
    patch, cell, field = sensor_sets("a")["segments"]
    obs, w = sensor_obs("a", "segments", 1).clone(), sensor_precision("a", "segments", 1)
    args = lambda o, ww: (c["w1"], c["w2"], c["b2"], groups, c["z"], patch, cell, field, o, ww, 2)   # noqa: E731
    base = restate_sensor_grad(*args(obs, w))
    dirty = obs.clone()
    dirty[w == 0] = float("nan")
    got = restate_sensor_grad(*args(dirty, w))
    assert int((w == 0).sum()) > 10 and torch.equal(base[0], got[0]) and torch.equal(base[2], got[2]) and bool(torch.isfinite(got[2]).all())
    # a sensor with precision 0 contributes exactly 0: the set without those sensors gives the same gradient
    keep = [k for k in range(len(patch)) if float(w[0, k]) > 0]
    sub = restate_sensor_grad(c["w1"], c["w2"], c["b2"], groups, c["z"], [patch[k] for k in keep], [cell[k] for k in keep], [field[k] for k in keep],
                              obs[:, keep], w[:, keep], 2)
    assert rel(sub[2], base[2]) <= 1e-14 and rel(sub[0], base[0]) <= 1e-14
    only_dead = restate_sensor_grad(*args(dirty, torch.zeros_like(w)))
    assert float(only_dead[2].abs().max()) == 0.0 and float(only_dead[0].abs().max()) == 0.0
    # duplicates add: a sensor given twice is the sensor with twice the precision
    one = ([3], [5], [1], torch.tensor([[0.25]]))
    a = restate_sensor_grad(c["w1"], c["w2"], c["b2"], groups, c["z"], one[0] * 2, one[1] * 2, one[2] * 2, one[3].repeat(1, 2), None, 2)
    b = restate_sensor_grad(c["w1"], c["w2"], c["b2"], groups, c["z"], *one[:3], one[3], torch.tensor([2.0]), 2)
    assert rel(a[2], b[2]) <= 1e-14 and rel(a[0], b[0]) <= 1e-14 and float(b[2].abs().max()) > 0
    # exact zeros: unobserved patches, and the slice of a group without sensors
    dz = base[2]
    grp_of = {f: g for g, grp in enumerate(groups) for f in grp}
    seen = {(grp_of[f], p) for k, (p, f) in enumerate(zip(patch, field)) if float(w[0, k]) > 0}   # pairs with a reading that has weight
    n_zero = 0
    for g in range(len(groups)):
        for p in range(P):
            if (g, p) not in seen:
                assert float(dz[:, p, g].abs().max()) == 0.0
                n_zero += 1
            else:
                assert float(dz[:, p, g].abs().max()) > 0
    assert n_zero >= 3
    last = restate_sensor_grad(c["w1"], c["w2"], c["b2"], groups, c["z"], *sensor_sets("a")["last"], sensor_obs("a", "last", 1), None, 2)[2]
    assert float(last[:, :, 0].abs().max()) == 0.0 and float(last[:, :, 1].abs().max()) > 0      # group 0 is unobserved in "last"


def _rounding_errors(c, z, patch, cell, field, obs, prec, members):
    args = (c["w1"], c["w2"], c["b2"], c["groups"], z, patch, cell, field, obs, prec, members)
    ref = restate_sensor_grad(*args)
    rnd = restate_sensor_grad(*args, round_bf16=True)
    return rel(rnd[0], ref[0]), rel(rnd[1], ref[1]), rel(rnd[2], ref[2])


@pytest.mark.parametrize("name,set_name", GRAD_SETS)
def test_bf16_rounding_stays_within_half_the_gpu_bound(name, set_name):
    """The GPU test allows TOL_BF16 = 2e-2 against the fp64 restatement; what the bf16 paths cannot avoid — z, W1, the hidden rows and W2 rounded to bf16, and
    the weighted residual rounded once — must stay below half of it for the gradient too, or the bound would measure the inputs and not the kernel."""
    c = host_case(name)
    patch, cell, field = sensor_sets(name)[set_name]
    for members, hist in SPLITS[name]:
        for prec in (None, sensor_precision(name, set_name, hist)):
            e_w, e_p, e_g = _rounding_errors(c, c["z"], patch, cell, field, sensor_obs(name, set_name, hist), prec, members)
            print(f"sensor_grad shape {name} set {set_name} members {members} x {hist} precision {prec is not None}: bf16 operands e(wsse) {e_w:.3e} e(pred) {e_p:.3e} e(dz) {e_g:.3e}")
            assert e_g <= TOL_BF16 / 2 and e_w <= TOL_BF16 / 2, (members, hist, e_w, e_g)


def test_bf16_rounding_stays_within_half_the_gpu_bound_at_130_members():
    c = host_case("a")
    for set_name, (patch, cell, field) in sensor_sets("a").items():
        e_w, e_p, e_g = _rounding_errors(c, big_states(), patch, cell, field, sensor_obs("a", set_name, BIG["hist"]), sensor_precision("a", set_name, BIG["hist"]),
                                         BIG["members"])
        print(f"sensor_grad shape a set {set_name} 130 members: bf16 operands e(wsse) {e_w:.3e} e(dz) {e_g:.3e}")
        assert e_g <= TOL_BF16 / 2 and e_w <= TOL_BF16 / 2, (set_name, e_w, e_g)


# ------------------------------------------------------------------------------------------------ the entry point, without a GPU
@pytest.fixture(scope="module")
def lib():
    from sea_amd import build, _native

    build.build(verbose=False)
    return _native.lib()


def _table(n_groups=2):
    """A well-formed sea_decode_sensor_grad table over made-up (aligned, never dereferenced) addresses: shape a, 4 members, 3 observed patches."""
    from sea_amd import _native as N

    g = (N.SeaDecodeMseGroup * N.DECODE_MSE_MAX_GROUPS)()
    for i in range(n_groups):
        base = 0x10000 * (i + 1)
        g[i].H, g[i].W2, g[i].bias, g[i].dH, g[i].Z = base, base + 0x1000, base + 0x2000, base + 0x3000, base + 0x4000
        g[i].ldh = g[i].ldw = g[i].lddh = g[i].ldz = 40
        g[i].n_fields, g[i].field0 = (2, 0) if i == 0 else (1, 2)
    p = N.SeaDecodeSensorGrad()
    p.obs, p.prec, p.live, p.wrow, p.seg, p.wsse, p.pred, p.work = 0x100000, 0x110000, 0x120004, 0x130004, 0x140004, 0x150004, 0x160000, 0x170004
    p.ld_obs, p.ld_prec, p.work_cap = 128, 0, 3 * 2 * 4
    p.Bm, p.members, p.S, p.Cp, p.Q, p.K_pad = 4, 2, 40, 32, 3, 128
    p.grad_scale = 1.0
    return g, p


def test_symbol_and_struct_layout(lib):
    from sea_amd import _native as N

    assert hasattr(lib, "sea_decode_sensor_grad") and "sea_decode_sensor_grad" in N.EXPORTED_SYMBOLS
    assert C.sizeof(N.SeaDecodeSensorGrad) == 120                   # include/sea_hip.h states it
    for name, _ in N.SeaDecodeSensorSse._fields_:                   # the fields of SeaDecodeSensorSse where they are there, then grad_scale
        assert getattr(N.SeaDecodeSensorGrad, name).offset == getattr(N.SeaDecodeSensorSse, name).offset
    assert N.SeaDecodeSensorGrad.grad_scale.offset == 112
    assert lib.sea_abi_version() == 8 and len(N.ABI_STRUCTS) == 33 and N.ABI_STRUCTS[-1] is N.SeaKvFork
    # the library reads the fields where the binding writes them: its messages quote the values back
    call = lambda g, p, n=2, dt=N.SEA_BF16: lib.sea_decode_sensor_grad(g, n, C.byref(p), dt, None)   # noqa: E731
    g, p = _table()
    p.members = 3
    assert call(g, p) == -1 and b"Bm=4 must be a positive multiple of members=3" in lib.sea_last_error()
    g, p = _table()
    p.work_cap -= 1   # the LAST check: a table that is well formed up to the launch reaches it, and only it refuses
    assert call(g, p) == -1 and b"sea_decode_sensor_grad: workspace of 23 floats is too small: 24 needed" in lib.sea_last_error()
    g, p = _table()
    p.prec = p.pred = None
    for i in range(2):
        g[i].Z, g[i].ldz = None, 0                                   # Z is nullable, and its stride is then not looked at
    p.work_cap -= 1
    assert call(g, p) == -1 and b"workspace of 23 floats is too small" in lib.sea_last_error()
    g, p = _table()
    g[1].lddh, g[1].ldz = 48, 56
    g[1].ldh = 32
    assert call(g, p) == -1 and b"group 1: row strides ldh=32 ldw=40" in lib.sea_last_error()
    g, p = _table()
    g[1].lddh, g[1].ldz = 36, 56
    assert call(g, p) == -1 and b"group 1: row strides lddh=36 ldz=56" in lib.sea_last_error()


GROUP_BREAKS = {"null dH": (1, "dH", None), "misaligned dH": (0, "dH", 0x13008), "misaligned Z": (1, "Z", 0x24004), "lddh < S": (1, "lddh", 32),
                "lddh % 8": (0, "lddh", 44), "ldz < S": (0, "ldz", 32), "ldz % 8": (1, "ldz", 44), "null H": (0, "H", None), "misaligned W2": (1, "W2", 0x21008),
                "ldh % 8": (0, "ldh", 44), "n_fields = 0": (1, "n_fields", 0)}
PARAM_BREAKS = {"grad_scale = inf": ("grad_scale", float("inf")), "grad_scale = -inf": ("grad_scale", -float("inf")), "grad_scale = nan": ("grad_scale", float("nan")),
                "null obs": ("obs", None), "null work": ("work", None), "misaligned pred": ("pred", 0x160008), "misaligned seg": ("seg", 0x140002),
                "K_pad = 48": ("K_pad", 48), "Bm = 0": ("Bm", 0), "members = 0": ("members", 0), "S = 36": ("S", 36), "Cp = 48": ("Cp", 48), "Q too large": ("Q", 65536),
                "ld_obs % 4": ("ld_obs", 130), "ld_prec short": ("ld_prec", 64)}


@pytest.mark.parametrize("what", sorted(GROUP_BREAKS) + sorted(PARAM_BREAKS) + ["no groups", "too many groups"])
def test_sensor_grad_refuses_bad_arguments_without_a_device(lib, what):
    from sea_amd import _native as N

    g, p = _table()
    n = 2
    if what in GROUP_BREAKS:
        i, field, value = GROUP_BREAKS[what]
        setattr(g[i], field, value)
    elif what in PARAM_BREAKS:
        setattr(p, *PARAM_BREAKS[what])
    else:
        n = 0 if what == "no groups" else 17
    assert lib.sea_decode_sensor_grad(g, n, C.byref(p), N.SEA_BF16, None) == -1, what
    msg = lib.sea_last_error()
    assert b"sea_decode_sensor_grad" in msg
    if what in GROUP_BREAKS:
        assert b"group %d" % GROUP_BREAKS[what][0] in msg, msg
    if what.startswith("grad_scale"):
        assert b"grad_scale" in msg


def test_sensor_grad_unsupported_forms_and_null_tables(lib):
    from sea_amd import _native as N

    g, p = _table()
    assert lib.sea_decode_sensor_grad(g, 2, C.byref(p), N.SEA_F32, None) == -3   # fp32: unsupported, not an argument error
    assert b"sea_decode_sensor_grad" in lib.sea_last_error() and b"bf16 only" in lib.sea_last_error()
    g, p = _table()
    p.S = 648
    for i in range(2):
        g[i].ldh = g[i].ldw = g[i].lddh = g[i].ldz = 648
    assert lib.sea_decode_sensor_grad(g, 2, C.byref(p), N.SEA_BF16, None) == -3 and b"S=648" in lib.sea_last_error()
    assert lib.sea_decode_sensor_grad(None, 1, C.byref(p), N.SEA_BF16, None) == -1
    assert lib.sea_decode_sensor_grad(g, 1, None, N.SEA_BF16, None) == -1
    assert lib.sea_decode_sensor_grad(g, 2, C.byref(p), 7, None) == -1


# ------------------------------------------------------------------------------------------------ refusals of the Python layers
def test_ops_decode_sensor_grad_refuses_malformed_operands_on_the_host():
    from sea_amd import ops

    def args(**kw):
        Q, Bm, S, Cp, K_pad = 2, 4, 40, 32, 64
        bf = lambda *s: torch.zeros(*s, dtype=torch.bfloat16)   # noqa: E731
        a = dict(groups=[dict(H=bf(Q * Bm, S), W2=bf(n * Cp, S), bias=torch.zeros(n * Cp), dH=bf(Q * Bm, S), Z=bf(Q * Bm, S)) for n in (2, 1)],
                 obs=torch.zeros(2, K_pad), live=torch.zeros(K_pad, dtype=torch.int32), wrow=torch.zeros(K_pad, dtype=torch.int32),
                 seg=torch.zeros(2, Q + 1, dtype=torch.int32), Cp=Cp, members=2, prec=None)
        a.update(kw)
        return a

    with pytest.raises(RuntimeError, match="MI355X"):
        ops.decode_sensor_grad(**args())
    a = args()
    del a["groups"][0]["Z"]                                          # Z is optional per group
    with pytest.raises(RuntimeError, match="MI355X"):
        ops.decode_sensor_grad(**a)
    for kw in (dict(dtype=torch.float32), dict(groups=[]), dict(Cp=12), dict(members=3), dict(obs=torch.zeros(2, 32)), dict(prec=torch.ones(32)),
               dict(grad_scale=float("inf")), dict(grad_scale=float("nan")), dict(grad_scale="1"), dict(seg=torch.zeros(2, 4, dtype=torch.int32))):
        with pytest.raises(ValueError):
            ops.decode_sensor_grad(**args(**kw))
    for name, bad, grp in (("dH", torch.zeros(8, 40), 1), ("dH", torch.zeros(7, 40, dtype=torch.bfloat16), 0), ("dH", torch.zeros(8, 48, dtype=torch.bfloat16), 1),
                           ("dH", torch.zeros(8, 44, dtype=torch.bfloat16)[:, :40], 0), ("dH", torch.zeros(8 * 40 + 4, dtype=torch.bfloat16)[4:].view(8, 40), 1),
                           ("dH", torch.zeros(8, 80, dtype=torch.bfloat16)[:, ::2], 0), ("dH", None, 1),
                           ("Z", torch.zeros(8, 40), 0), ("Z", torch.zeros(9, 40, dtype=torch.bfloat16), 1), ("Z", torch.zeros(8, 44, dtype=torch.bfloat16)[:, :40], 1)):
        a = args()
        a["groups"][grp][name] = bad
        with pytest.raises(ValueError, match=f"group {grp}: {name}"):
            ops.decode_sensor_grad(**a)


def test_sensor_loss_score_and_grad_and_nudge_refuse_before_a_device_is_touched():
    from sea_amd.ensemble import SensorLikelihood, SensorSet

    c = host_case("a")
    dec = make_decoder("a").set_compute_dtype("bf16").requires_grad_(False)
    P, D, G = c["P"], c["D"], len(c["groups"])
    s = SensorSet(dec, P, [0, 1, 8], [3, 4, 11], [0, 2, 1])
    z, obs = torch.zeros(4, P, G, D, requires_grad=True), torch.zeros(2, 3)
    bad = [dict(z=torch.zeros(4, P, G)), dict(members=3), dict(members=True), dict(obs=torch.zeros(2, 4)), dict(obs=torch.zeros(2, 3, dtype=torch.float64)),
           dict(obs=torch.zeros(2, 3, requires_grad=True)), dict(precision=torch.ones(3, requires_grad=True)),
           dict(precision=torch.tensor([1.0, -1.0, 1.0])), dict(sensors=None),
           dict(sensors=SensorSet(dec, P + 1, [0], [0], [0])),                                                       # another n_patches
           dict(sensors=SensorSet(make_decoder("b"), P, [0], [0], [0])),                                             # another n_inp and grouping
           dict(obs=torch.zeros(2, 3, device="meta"))]
    for kw in bad:
        args = dict(z=z, sensors=s, obs=obs, precision=None, members=2)
        args.update(kw)
        zz = args.pop("z")
        with pytest.raises(ValueError):
            dec.sensor_loss(zz, **args)
    trainable = make_decoder("a").set_compute_dtype("bf16")                                                          # its parameters require grad
    with pytest.raises(ValueError, match="frozen observation operator"):
        trainable.sensor_loss(z, s, obs, members=2)
    with pytest.raises(ValueError, match="bf16 only"):
        make_decoder("a").requires_grad_(False).sensor_loss(z, s, obs, members=2, fused=True)                        # fp32: no fused launch
    with pytest.raises(RuntimeError, match="MI355X"):                                                                # well-formed, but on the host
        dec.sensor_loss(z, s, obs, members=2)
    with pytest.raises(RuntimeError, match="MI355X"):
        make_decoder("a").requires_grad_(False).sensor_loss(z, s, obs, precision=torch.ones(2, 3), members=2, predictions=True)

    y = torch.zeros(4, G, P * D)
    like = SensorLikelihood(dec, P, 2, s, sigma=[0.5, 1.0, 2.0])
    for yy, oo, pp in ((torch.zeros(4, G, P * D + 1), obs, None), (torch.zeros(3, G, P * D), obs, None), (y, torch.zeros(2, 2), None), (y, obs.double(), None),
                       (y, obs, torch.tensor([1.0, -2.0, 1.0]))):
        with pytest.raises(ValueError):
            like.score_and_grad(yy, oo, pp)
        with pytest.raises(ValueError):
            like.nudge(yy, oo, pp)
    with pytest.raises(ValueError, match="bf16 only"):
        SensorLikelihood(make_decoder("a").requires_grad_(False), P, 2, s, fused=True).score_and_grad(y, obs)
    for rate in (torch.ones(3), torch.ones(4, 1), torch.ones(4, dtype=torch.float64), torch.ones(4, device="meta"), torch.ones(()), float("nan"), float("inf"), "1", True, None):
        with pytest.raises(ValueError, match="rate"):
            like.nudge(y, obs, rate=rate)
    with pytest.raises(RuntimeError, match="MI355X"):
        like.score_and_grad(y, obs, torch.ones(3))
    with pytest.raises(RuntimeError, match="MI355X"):
        like.nudge(y, obs, rate=torch.ones(4))
    with pytest.raises(RuntimeError, match="MI355X"):
        like.nudge(y, obs, rate=0.5)
