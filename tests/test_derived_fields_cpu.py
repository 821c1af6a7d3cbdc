"""Derived fields (|u|, energy, differences) of an ensemble, on the host: the composed arithmetic against a plain float32 loop; DerivedField's
refusals; the composed DerivedQuantiles / DerivedThresholdVerification against the restatements of the member launches applied to the derived values;
the two forms of the observation; MeshUnpatcher.derived_fields; and sea_decode_derived_quantiles / sea_decode_derived_brier through ctypes without a
device (the symbols, the struct's size, every refusal with its message, the unsupported forms)."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.test_brier_cpu import _field_tables, restate_field_brier
from tests.test_ensemble_quantiles_cpu import _tables, restate_quantiles, same
from tests.test_field_verify_cpu import field_logw
from tests.test_sensor_cpu import make_decoder
from tests.test_verify_cpu import close

F64 = torch.float64


def three(sa=0.5, ha=0.25, sb=2.0, hb=-0.5):
    from sea_amd.ensemble import DerivedField

    return [DerivedField("magnitude", 0, 1, sa, ha, sb, hb), DerivedField("energy", 0, 1, sa, ha, sb, hb), DerivedField("difference", 1, 0, sa, ha, sb, hb)]


# ------------------------------------------------------------------------------------------------ the arithmetic
def test_composed_derived_against_a_float32_loop():
    from sea_amd.ensemble import _composed_derived

    g = torch.Generator().manual_seed(5)
    Y = torch.randn(2, 3, 2, 3, 7, generator=g) * 3
    derived = three(1.5, -0.25, 0.75, 0.5)
    got = _composed_derived(Y, derived)
    assert got.dtype == torch.float32 and got.shape == (2, 3, 2, 3, 7)
    f32 = np.float32
    y = Y.numpy()
    for i, d in enumerate(derived):
        for idx in np.ndindex(2, 3, 2, 7):
            b_, j, p, c = idx
            a = f32(f32(y[b_, j, p, d.a, c] * f32(d.scale_a)) + f32(d.shift_a))
            b = f32(f32(y[b_, j, p, d.b, c] * f32(d.scale_b)) + f32(d.shift_b))
            if d.op == "difference":
                want = f32(a - b)
            else:
                q = f32(f32(a * a) + f32(b * b))
                want = f32(f32(0.5) * q) if d.op == "energy" else np.sqrt(q, dtype=f32)
            assert got[b_, j, p, i, c].numpy().tobytes() == f32(want).tobytes(), (d.op, idx)
    # a tensor long enough for torch's vectorised loops, against numpy's float32 arithmetic (its root is correctly rounded; torch.sqrt's float32 one is not always)
    big = torch.randn(3, 2, 1 << 16, generator=g) * 3
    yb = big.numpy()
    for i, d in enumerate(derived):
        a, b = yb[:, d.a] * f32(d.scale_a) + f32(d.shift_a), yb[:, d.b] * f32(d.scale_b) + f32(d.shift_b)
        want = a - b if d.op == "difference" else (f32(0.5) * (a * a + b * b) if d.op == "energy" else np.sqrt(a * a + b * b))
        assert want.dtype == f32 and _composed_derived(big, derived)[:, i].numpy().tobytes() == want.tobytes(), d.op
    # bf16 members are converted first; an observation [B, P, F, C] goes through the same ops
    assert torch.equal(_composed_derived(Y.to(torch.bfloat16), derived), _composed_derived(Y.to(torch.bfloat16).float(), derived))
    assert torch.equal(_composed_derived(Y[:, 0], derived), got[:, 0])


def test_derived_field_refusals():
    from sea_amd.ensemble import DerivedField, DerivedQuantiles

    d = DerivedField("magnitude", 0, 1, 0.5, 0.25, name="speed")
    assert (d.op, d.a, d.b, d.scale_a, d.shift_a, d.scale_b, d.shift_b, d.name) == ("magnitude", 0, 1, 0.5, 0.25, 1.0, 0.0, "speed")
    assert d == DerivedField("magnitude", 0, 1, 0.5, 0.25, name="speed") and len({d, DerivedField("magnitude", 0, 1, 0.5, 0.25, name="speed")}) == 1
    with pytest.raises(AttributeError):
        d.a = 2
    for bad in (dict(op="hypot"), dict(a=1), dict(a=-1), dict(b=True), dict(scale_a=float("inf")), dict(shift_b=float("nan")), dict(scale_b=1e39), dict(shift_a="x")):
        kw = dict(op="energy", a=0, b=1)
        kw.update(bad)
        with pytest.raises(ValueError, match="DerivedField"):
            DerivedField(**kw)
    dec = make_decoder("decode_mse_a")
    n_fields = sum(len(g) for g in dec.field_groups)
    with pytest.raises(ValueError, match="outside"):
        DerivedQuantiles(dec, 2, 2, [DerivedField("energy", 0, n_fields)])
    for kw in (dict(derived=[]), dict(derived=[("magnitude", 0, 1)]), dict(levels=(), thresholds=None), dict(thresholds=[[1.0, 2.0]]), dict(layout="FC"), dict(fused=1),
               dict(members=129, fused=True)):
        args = dict(decoder=dec, n_patches=2, members=2, derived=[DerivedField("energy", 0, 1)])
        args.update(kw)
        with pytest.raises(ValueError, match="DerivedQuantiles"):
            DerivedQuantiles(**args)


# ------------------------------------------------------------------------------------------------ the composed classes against the restatements
def members_case(n, seed, dec, P=2, B=2):
    F, C_ = sum(len(g) for g in dec.field_groups), dec.n_inp
    g = torch.Generator().manual_seed(seed)
    Y = (torch.randn(B, n, P, F, C_, generator=g) * 2).round() / 4       # multiples of 0.25: ties occur, and with dyadic coefficients every op is exact
    obs = (torch.randn(B, P, F, C_ + 3, generator=g) * 2).round() / 4
    prec = (torch.rand(B, P, F, C_ + 3, generator=g) > 0.2).float() * (0.5 + torch.rand(B, P, F, C_ + 3, generator=g))
    return Y, obs, prec


@pytest.mark.parametrize("n", [1, 2, 5])
def test_composed_classes_equal_the_restatements_on_the_derived_values(n):
    from sea_amd.ensemble import DerivedQuantiles, DerivedThresholdVerification, _composed_derived, _field_cell_weights, normalised_weights

    dec = make_decoder("decode_mse_a")
    P, B = 2, 2
    C_ = dec.n_inp
    Y, obs, prec = members_case(n, 40 + n, dec, P, B)
    derived = three()
    X = _composed_derived(Y, derived)
    counts = [C_, max(C_ - 3, 0)]
    levels = (0.0, 0.3, 0.5, 1.0)
    thr = torch.tensor([[0.75, 0.25, -0.5], [1.5, 1.0, 0.25]])
    for logw in (None, field_logw(n, B, 7)):
        w = None if logw is None else normalised_weights(logw, n).view(B, n)
        ref = restate_quantiles(X, w, levels, thr)
        valid = (torch.arange(C_) < torch.tensor(counts)[:, None]).view(1, 1, P, 1, C_)
        q, e = DerivedQuantiles(dec, P, n, derived, levels=levels, thresholds=thr, counts=counts).from_fields(Y, logw)
        assert same(q, torch.where(valid, ref["quant"], torch.zeros(()))), (n, logw is None)
        assert close(e.to(F64), torch.where(valid, ref["exceed"], torch.zeros((), dtype=F64)), 1e-6)[0], (n, logw is None)
        qt, et = DerivedQuantiles(dec, P, n, derived, levels=levels, thresholds=thr, counts=counts, layout="BPCF").from_fields(Y, logw)
        assert torch.equal(qt.permute(0, 1, 2, 4, 3).isnan(), q.isnan()) and et.shape == e.permute(0, 1, 2, 4, 3).shape

        ver = DerivedThresholdVerification(dec, P, n, derived, thr, counts=counts, observed="fields")
        s = ver.from_fields(Y, obs, precision=prec, logw=logw, maps=("prob", "brier"))
        on = (prec > 0).float()
        pd = torch.stack([on[:, :, d.a] * on[:, :, d.b] for d in derived], dim=2)
        wd = _field_cell_weights((B, P, len(derived), C_), None, pd, torch.tensor(counts), torch.device("cpu"))
        r = restate_field_brier(X.view(B * n, P, len(derived), C_), _composed_derived(obs, derived), wd, logw, n, thr)
        assert torch.equal(s.hist, r["hist"]) and torch.equal(s.hits, r["hits"]) and torch.equal(s.status.long(), r["status"].long())
        assert close(s.sums, r["sums"], 1e-12)[0] and close(s.prob.to(F64), r["prob"], 1e-6)[0] and close(s.brier_map.to(F64), r["brier"], 1e-6)[0]
        # the two forms of the observation agree when the second is fed the first's derived observation
        s2 = DerivedThresholdVerification(dec, P, n, derived, thr, counts=counts, observed="derived").from_fields(
            Y, _composed_derived(obs, derived), precision=pd, logw=logw, maps=("prob", "brier"))
        for k in ("sums", "hist", "hits", "status", "prob", "brier_map"):
            assert same(getattr(s, k).to(F64), getattr(s2, k).to(F64)), k
        # into= accumulates
        s3 = ver.from_fields(Y, obs, precision=prec, logw=logw, into=s2)
        assert s3.sums is s2.sums and torch.equal(s3.hist, 2 * r["hist"])
    with pytest.raises(ValueError, match="observed"):
        DerivedThresholdVerification(dec, P, n, derived, thr, observed="both")
    with pytest.raises(ValueError, match="finite"):
        DerivedThresholdVerification(dec, P, n, derived, [float("nan")])
    with pytest.raises(ValueError, match="must carry"):
        DerivedThresholdVerification(dec, P, n, derived, thr, observed="derived").from_fields(Y, obs[:, :, :1])


# ------------------------------------------------------------------------------------------------ the mesh's coefficients
def test_mesh_derived_fields_carry_the_inverse_scaling():
    from sea_amd.ensemble import _composed_derived
    from sea_amd.utils.data_processors import DataPartitioner2D, MeshUnpatcher, MinMaxScaler

    g = torch.Generator().manual_seed(3)
    n_pts = 57
    part = DataPartitioner2D(torch.rand(n_pts, generator=g), torch.rand(n_pts, generator=g), m=4, n=3, device="cpu")
    groups = [[0, 1], [2]]
    data = torch.randn(5, n_pts, 3, generator=g) * torch.tensor([1.0, 10.0, 0.1]) + torch.tensor([0.0, 5.0, -1.0])
    scalers = [MinMaxScaler((-1, 1)), MinMaxScaler((0, 2))]
    for sc, grp in zip(scalers, groups):
        sc.fit(data[:, :, grp])
    mesh = MeshUnpatcher(part, groups, scalers)
    speed, diff = mesh.derived_fields([("magnitude", 0, 1), ("difference", 2, 0, "p - u")])
    assert (speed.op, speed.a, speed.b, diff.name) == ("magnitude", 0, 1, "p - u")
    scaled = torch.stack([scalers[0].transform(data[..., 0]), scalers[0].transform(data[..., 1]), scalers[1].transform(data[..., 2])], dim=1)   # [T, F, N]
    got = _composed_derived(scaled, [speed, diff])                                                                                               # [T, 2, N]
    phys = [data[..., f].double() for f in range(3)]                     # the inverse-scaled fields are the data the scalers were fitted to
    # float32 rounding: each value goes through the forward scaling, then a multiply, an add, a square, a sum and a root — a few 2^-24 relative of the
    # largest term (the group's range, which the scaled value's rounding is blown back up to)
    tol = 16 * 2.0 ** -24 * max(float(t.abs().max()) for t in phys)
    assert float((got[:, 0].double() - torch.hypot(phys[0], phys[1])).abs().max()) <= tol
    assert float((got[:, 1].double() - (phys[2] - phys[0])).abs().max()) <= tol
    for bad in ([("magnitude", 0, 3)], [("magnitude", 0)], [("magnitude", 1, 1)], ["magnitude"]):
        with pytest.raises(ValueError):
            mesh.derived_fields(bad)


# ------------------------------------------------------------------------------------------------ the entry points without a device
@pytest.fixture(scope="module")
def lib():
    from sea_amd import build, _native

    build.build(verbose=False)
    return _native.lib()


def derived_table(*rows):
    from sea_amd import _native as N

    rows = rows or ((0, 0, 1, 0.5, 0.25, 1.0, 0.0), (2, 1, 0, 1.0, 0.0, 1.0, 0.0))
    tab = (N.SeaDerivedField * len(rows))()
    for t, (op, a, b, sa, ha, sb, hb) in zip(tab, rows):
        t.op, t.a, t.b, t.scale_a, t.shift_a, t.scale_b, t.shift_b = op, a, b, sa, ha, sb, hb
    return tab


def tables(which):
    """Well-formed tables of the member entry points (3 source fields in groups [0, 1] and [2]) with their maps sized for 2 derived fields."""
    arr, p = _tables() if which == "quantiles" else _field_tables()
    if which == "quantiles":
        p.ld_map = 2 * 9 * 2 * 21
    else:
        p.ld_map, p.ld_row, p.ld_prow, p.work_bytes = 2 * 9 * 2 * 21, 2 * 24, 2 * 24, 2 * 9 * 2 * 20 * 8
    return arr, p


def call(lib, which, arr, ng, tab, nd, p, dt):
    fn = lib.sea_decode_derived_quantiles if which == "quantiles" else lib.sea_decode_derived_brier
    return fn(arr, ng, tab, nd, None if p is None else C.byref(p), dt, None)


INF, NAN = float("inf"), float("nan")
REFUSED = {"unknown op": (((3, 0, 1, 1.0, 0.0, 1.0, 0.0),), b"derived field 0: unknown op 3"),
           "negative op": (((0, 0, 1, 1.0, 0.0, 1.0, 0.0), (-1, 0, 1, 1.0, 0.0, 1.0, 0.0)), b"derived field 1: unknown op -1"),
           "a outside": (((0, 3, 1, 1.0, 0.0, 1.0, 0.0),), b"derived field 0: sources a=3, b=1 outside the 3 fields"),
           "b negative": (((1, 0, -1, 1.0, 0.0, 1.0, 0.0),), b"derived field 0: sources a=0, b=-1 outside the 3 fields"),
           "a == b": (((0, 0, 1, 1.0, 0.0, 1.0, 0.0), (2, 1, 1, 1.0, 0.0, 1.0, 0.0)), b"derived field 1: a == b = 1"),
           "scale inf": (((0, 0, 1, INF, 0.0, 1.0, 0.0),), b"derived field 0: a coefficient is not finite"),
           "shift nan": (((0, 0, 1, 1.0, 0.0, 1.0, NAN),), b"derived field 0: a coefficient is not finite")}


@pytest.mark.parametrize("which", ["quantiles", "brier"])
def test_symbols_struct_size_and_refusals_without_a_device(lib, which):
    from sea_amd import _native as N

    name = f"sea_decode_derived_{which}".encode()
    assert hasattr(lib, name.decode()) and name.decode() in N.EXPORTED_SYMBOLS
    assert C.sizeof(N.SeaDerivedField) == 32 and N.SeaDerivedField.scale_a.offset == 16 and N.SeaDerivedField not in N.ABI_STRUCTS and lib.sea_abi_version() == 8
    assert N.DERIVED_MAX == 8 and N.DERIVED_OPS == {"magnitude": 0, "energy": 1, "difference": 2}
    for what, (rows, msg) in REFUSED.items():
        arr, p = tables(which)
        assert call(lib, which, arr, 2, derived_table(*rows), len(rows), p, N.SEA_BF16) == -1, what
        assert msg in lib.sea_last_error() and name in lib.sea_last_error(), (what, lib.sea_last_error())
    for nd in (0, 9, -1):
        arr, p = tables(which)
        assert call(lib, which, arr, 2, derived_table(), nd, p, N.SEA_BF16) == -1 and f"n_derived={nd} outside 1..8".encode() in lib.sea_last_error()
    # what the member entry points refuse, under this entry point's name
    for field, value, msg in (("members", 0, b"members=0"), ("M", 71, b"M=71 is not a multiple of P * members = 9 * 4"), ("S", 36, b"S=36"), ("Cp", 40, b"Cp=40"),
                              ("C", 33, b"C=33"), ("n_fields_total", 4, b"cover 3 of the 4 fields"), ("ld_map", 2 * 9 * 2 * 21 - 1, b"ld_map=755")):
        arr, p = tables(which)
        setattr(p, field, value)
        assert call(lib, which, arr, 2, derived_table(), 2, p, N.SEA_BF16) == -1 and msg in lib.sea_last_error() and name in lib.sea_last_error(), (field, lib.sea_last_error())
    arr, p = tables(which)
    arr[1].W2 = None
    assert call(lib, which, arr, 2, derived_table(), 2, p, N.SEA_BF16) == -1 and b"group 1: null pointer" in lib.sea_last_error()
    arr, p = tables(which)
    assert call(lib, which, arr, 2, derived_table(), 2, p, 5) == -1 and b"bad dtype 5" in lib.sea_last_error()
    assert call(lib, which, None, 2, derived_table(), 2, p, N.SEA_BF16) == -1 and call(lib, which, arr, 2, None, 2, p, N.SEA_BF16) == -1
    assert call(lib, which, arr, 2, derived_table(), 2, None, N.SEA_BF16) == -1 and b"null argument table" in lib.sea_last_error()
    if which == "brier":
        arr, p = tables(which)
        p.work_bytes -= 1
        assert call(lib, which, arr, 2, derived_table(), 2, p, N.SEA_BF16) == -1 and b"work_bytes=5759 below the 5760" in lib.sea_last_error()
    else:
        arr, p = tables(which)
        p.level[1] = 1.5
        assert call(lib, which, arr, 2, derived_table(), 2, p, N.SEA_BF16) == -1 and b"level[1]=1.5" in lib.sea_last_error()


@pytest.mark.parametrize("which", ["quantiles", "brier"])
def test_unsupported_forms_without_a_device(lib, which):
    from sea_amd import _native as N

    name = f"sea_decode_derived_{which}".encode()
    arr, p = tables(which)
    cross = derived_table((0, 0, 1, 1.0, 0.0, 1.0, 0.0), (2, 2, 1, 1.0, 0.0, 1.0, 0.0))
    assert call(lib, which, arr, 2, cross, 2, p, N.SEA_BF16) == -3
    assert b"derived field 1: its sources a=2 and b=1 lie in different groups" in lib.sea_last_error() and name in lib.sea_last_error()
    arr, p = tables(which)
    assert call(lib, which, arr, 2, derived_table(), 2, p, N.SEA_F32) == -3 and b"bf16 only" in lib.sea_last_error()
    arr, p = tables(which)
    p.S = 648
    for g in range(2):
        arr[g].ldh = arr[g].ldw = 648
    assert call(lib, which, arr, 2, derived_table(), 2, p, N.SEA_BF16) == -3 and b"S=648" in lib.sea_last_error()
    arr, p = tables(which)
    p.members, p.M = 129, 2 * 129 * 9
    assert call(lib, which, arr, 2, derived_table(), 2, p, N.SEA_BF16) == -3 and b"members=129" in lib.sea_last_error()
    # a refused table with a bad derived field is -1, not -3: the checks come first
    arr, p = tables(which)
    p.members, p.M = 129, 2 * 129 * 9
    assert call(lib, which, arr, 2, derived_table((0, 1, 1, 1.0, 0.0, 1.0, 0.0)), 1, p, N.SEA_BF16) == -1
