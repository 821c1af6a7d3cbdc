"""Quantile and exceedance-probability maps of an ensemble, on the host: the fp64 restatement `restate_quantiles` written from the definitions in
include/sea_hip.h (sea_decode_member_quantiles) — below_i as a loop over j ascending, no sort — against the composed path `_composed_quantiles` (a
stable sort and cumulative weights) and numpy's method="inverted_cdf"; the properties of the definition; the refusals of the Python layers and of the
entry point without a device; the struct's size; MeshUnpatcher.scale_thresholds."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from tests.test_field_verify_cpu import field_logw
from tests.test_sensor_cpu import host_case, make_decoder
from tests.test_verify_cpu import restate_verify

F64 = torch.float64
INF = float("inf")


# ------------------------------------------------------------------------------------------------ the contract, in fp64
def restate_quantiles(Y, w, levels, thr):
    """include/sea_hip.h, sea_decode_member_quantiles, history by history from the definitions.  Y [B, n, P, F, C] (compared in the dtype given), w None
    (equal weights: 1 each) or float32 [B, n], levels numbers in [0, 1] (rounded to float32 first, as the launch carries them), thr None or [T, F].
    below_i is accumulated in fp64 over j ASCENDING, W is one fp64 chain over j ascending, tau * W one fp64 product: the sums have the kernel's order,
    so every decision cum_i >= tau W has the kernel's operands.  Returns dict(quant [Q, B, P, F, C] in Y's dtype or None, exceed float64 [T, B, P, F, C]
    or None, margin: the smallest NON-ZERO |cum_i - tau W| / W over the live members, cells and levels — how far the nearest decision that is not an
    exact tie is from flipping)."""
    B, n, P, F, C_ = Y.shape
    Q, T = len(levels), 0 if thr is None else thr.shape[0]
    quant = torch.zeros(Q, B, P, F, C_, dtype=Y.dtype) if Q else None
    exceed = torch.zeros(T, B, P, F, C_, dtype=F64) if T else None
    taus = [float(np.float32(v)) for v in levels]
    margin = INF
    idx = torch.arange(n).view(n, 1)
    for b in range(B):
        wb = torch.ones(n, dtype=F64) if w is None else w[b].to(F64)
        live = wb > 0                                                      # false for NaN
        wb = torch.where(live, wb, torch.zeros((), dtype=F64))
        if not bool(live.any()):
            continue                                                       # zeros everywhere
        W = 0.0
        for j in range(n):
            W = W + float(wb[j])
        x = Y[b].reshape(n, P * F * C_)
        lv = live.view(n, 1)
        bad = (lv & ~torch.isfinite(x)).any(0)
        if Q:
            below = torch.zeros(n, P * F * C_, dtype=F64)
            for j in range(n):
                lower = (x[j] < x) | ((x[j] == x) & (j < idx))
                below = below + torch.where(lower, wb[j], torch.zeros((), dtype=F64))
            cum = below + wb.view(n, 1)
            hi = torch.where(lv, x, torch.full((), -INF, dtype=x.dtype)).amax(0)
            for k, tau in enumerate(taus):
                tw = tau * W
                ok = lv & (cum >= tw)
                q = torch.where(ok, x, torch.full((), INF, dtype=x.dtype)).amin(0)
                q = torch.where(ok.any(0), q, hi)
                q[bad] = float("nan")
                quant[k, b] = q.view(P, F, C_)
                gap = (cum - tw).abs()[lv.expand_as(cum) & ~bad.view(1, -1).expand_as(cum)]
                gap = gap[gap > 0]
                if gap.numel():
                    margin = min(margin, float(gap.min()) / W)
        for t in range(T):
            th = thr[t].to(x.dtype).view(1, 1, F, 1)
            xv = x.view(n, P, F, C_)
            e = torch.where(lv.view(n, 1, 1, 1) & (xv > th), wb.view(n, 1, 1, 1), torch.zeros((), dtype=F64)).sum(0) / W
            e = torch.where(bad.view(P, F, C_) | torch.isnan(th[0]).expand(P, F, C_), torch.full((), float("nan"), dtype=F64), e)
            exceed[t, b] = e
    return dict(quant=quant, exceed=exceed, margin=margin)


def same(a, b):
    """Equal bits up to the sign of zero, NaN where and only where the other has it."""
    return a.shape == b.shape and torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a, nan=7.5), torch.nan_to_num(b, nan=7.5))


def composed(Y, w, levels, thr):
    from sea_amd.ensemble import _composed_quantiles

    return _composed_quantiles(Y, w, levels, thr)


def draw(n, B, seed, tied, P=2, F=2, C_=9):
    g = torch.Generator().manual_seed(seed)
    Y = torch.randn(B, n, P, F, C_, generator=g)
    if tied:
        Y = (Y * 2).round() / 4                                            # multiples of 0.25: ties occur
    w = torch.rand(B, n, generator=g)
    w = (w / w.sum(1, keepdim=True)).to(torch.float32)
    thr = torch.tensor([[-0.25, 0.25], [0.5, float("nan")]])
    return Y, w, thr


LEVELS = (0.0, 0.05, 0.25, 0.5, 0.9, 1.0)


@pytest.mark.parametrize("n", [1, 2, 5, 17, 64])
@pytest.mark.parametrize("tied", [False, True])
def test_restatement_equals_the_composed_path_and_numpy(n, tied):
    Y, w, thr = draw(n, 3, 100 + n + tied, tied)
    for weights in (None, w):
        r = restate_quantiles(Y, weights, LEVELS, thr)
        q, e = composed(Y, weights, LEVELS, thr)
        assert r["margin"] > 1e-12                                         # every decision is an exact tie or far from one: the sort's sums decide alike
        assert same(q, r["quant"]) and q.dtype == Y.dtype
        assert torch.equal(torch.isnan(e), torch.isnan(r["exceed"])) and float((torch.nan_to_num(e).double() - torch.nan_to_num(r["exceed"])).abs().max()) <= 1e-6
        assert bool(torch.isnan(e[1, :, :, 1]).all()) and not bool(torch.isnan(e[0]).any())     # a NaN threshold marks its own map and field only
    dyadic = (0.0, 0.25, 0.5, 0.75, 1.0)                                   # float32-exact levels: the launch's rounding of the level changes nothing
    try:
        want = np.quantile(Y.numpy(), dyadic, axis=1, method="inverted_cdf")
    except TypeError:
        want = None                                                        # a numpy without the method: this one assertion is passed over
    if want is not None:
        assert np.array_equal(restate_quantiles(Y, None, dyadic, None)["quant"].numpy(), want)
        assert np.array_equal(composed(Y, None, dyadic, None)[0].numpy(), want)


@pytest.mark.parametrize("n", [2, 5, 33])
def test_properties_of_the_definition(n):
    Y, w, _ = draw(n, 2, 300 + n, True)
    w = w.clone()
    w[:, 1] = 0.0                                                          # a dead member
    fine = tuple(k / 7 for k in range(8))
    for fn in (lambda *a: restate_quantiles(*a)["quant"], lambda *a: composed(*a)[0]):
        q = fn(Y, w, fine, None)
        assert bool((q[1:] >= q[:-1]).all())                               # monotone in tau
        live = (w > 0).view(2, n, 1, 1, 1)
        assert torch.equal(q[0], torch.where(live, Y, torch.full((), INF)).amin(1)) and torch.equal(q[-1], torch.where(live, Y, torch.full((), -INF)).amax(1))
        Yn = Y.clone()
        Yn[:, 1] = float("nan")                                            # NaN in the dead member changes nothing
        assert same(fn(Yn, w, fine, None), q)
        one = torch.zeros(2, n)
        one[0, 0], one[1, n - 1] = 0.5, 2.0                                # all the weight on one member: its value at every level
        q1 = fn(Y, one, fine, None)
        assert torch.equal(q1[:, 0], Y[0, 0].expand(8, -1, -1, -1)) and torch.equal(q1[:, 1], Y[1, n - 1].expand(8, -1, -1, -1))
    for fn in (lambda *a: restate_quantiles(*a), lambda *a: dict(zip(("quant", "exceed"), composed(*a)))):
        Yb = Y.clone()
        Yb[0, 0, 1, 0, 3] = INF                                            # a live member's value is not finite: NaN in that cell's maps, nowhere else
        r = fn(Yb, w, (0.5,), torch.zeros(1, 2))
        mark = torch.zeros(2, 2, 2, 9, dtype=torch.bool)
        mark[0, 1, 0, 3] = True
        assert torch.equal(torch.isnan(r["quant"][0]), mark) and torch.equal(torch.isnan(r["exceed"][0]), mark)
        r = fn(Y, torch.zeros(2, n), (0.5,), torch.zeros(1, 2))            # no live member: zeros
        assert float(r["quant"].abs().max()) == 0.0 and float(r["exceed"].abs().max()) == 0.0


@pytest.mark.parametrize("n", [2, 5, 33])
def test_exceedance_is_one_minus_pit_away_from_ties(n):
    from sea_amd.ensemble import normalised_weights

    B, K = 3, 40
    g = torch.Generator().manual_seed(500 + n)
    pred = torch.randn(B * n, K, generator=g)
    thr_cells = (torch.randn(B, K, generator=g) * 4).round() / 4          # never a decoded value: no ties
    for logw in (None, field_logw(n, B, 70 + n)):
        pit = restate_verify(pred, thr_cells, None, logw, n, False)["pit"]
        w = None if logw is None else normalised_weights(logw, n).view(B, n)
        for b in range(B):                                                 # a history and a threshold at a time: thr is per field, so every cell is a field
            for k in range(0, K, 7):
                Yk = pred[b * n:(b + 1) * n, k].view(1, n, 1, 1, 1)
                wk = None if w is None else w[b:b + 1]
                for fn in (lambda *a: restate_quantiles(*a)["exceed"], lambda *a: composed(*a)[1]):
                    e = fn(Yk, wk, (), thr_cells[b, k].view(1, 1))
                    assert abs(float(e) - (1.0 - float(pit[b, k]))) <= 1e-6, (n, b, k)


# ------------------------------------------------------------------------------------------------ the Python layers
def test_python_layers_refuse_before_a_device_is_touched():
    from sea_amd import _native as N, ops
    from sea_amd.ensemble import EnsembleQuantiles
    from sea_amd.utils.train_utils import EnsembleQuantiles as EQ2

    c = host_case("a")
    dec = make_decoder("a")
    P, G, D_ = c["P"], len(c["groups"]), c["D"]
    F = sum(len(g) for g in c["groups"])
    assert EQ2 is EnsembleQuantiles and N.QUANTILE_MAX_LEVELS == 8 and N.QUANTILE_MAX_N == 128
    for kw in (dict(levels=(0.5, 1.5)), dict(levels=(-0.1,)), dict(levels=(float("nan"),)), dict(levels=tuple(k / 9 for k in range(9))), dict(levels=(), thresholds=None),
               dict(thresholds=torch.zeros(2, F + 1)), dict(thresholds=torch.zeros(9)), dict(thresholds=torch.zeros(1, F, 1)), dict(layout="PBFC"), dict(fused=1),
               dict(levels="median")):
        with pytest.raises(ValueError):
            EnsembleQuantiles(dec, P, 2, **kw)
    with pytest.raises(ValueError):
        EnsembleQuantiles(dec, 0, 2)
    with pytest.raises(ValueError):
        EnsembleQuantiles(dec, P, 129, fused=True)
    EnsembleQuantiles(dec, P, 129)                                          # the composed path carries any member count
    q = EnsembleQuantiles(dec, P, 2, levels=(0, 0.5, 1), thresholds=[0.5, 1.0])
    assert q.levels == (0.0, 0.5, 1.0) and tuple(q._thresholds_on(torch.device("cpu")).shape) == (2, F)
    assert EnsembleQuantiles(dec, P, 2, levels=(), thresholds=torch.zeros(3, F))._thresholds_on(torch.device("cpu")).shape == (3, F)
    y = torch.zeros(4, G, P * D_)
    for bad_y, lw in ((torch.zeros(4, G, P * D_ + 1), None), (torch.zeros(3, G, P * D_), None), (y, torch.zeros(3)), (y, torch.zeros(2, 3)), (y, torch.zeros(4, dtype=torch.int64)),
                      (y, torch.zeros(4, device="meta"))):
        with pytest.raises(ValueError):
            q(bad_y, lw)
    with pytest.raises(RuntimeError, match="MI355X"):
        q(y, torch.zeros(4))
    z = torch.zeros(4, P, G, D_)
    for kw in (dict(levels=(1.5,)), dict(levels=()), dict(levels=(0.5,), thresholds=torch.zeros(1, F + 1)), dict(levels=(0.5,), thresholds=torch.zeros(1, F, dtype=F64)),
               dict(levels=(0.5,), weights=torch.zeros(3)), dict(levels=(0.5,), weights=torch.zeros(4, dtype=F64)), dict(levels=(0.5,), fused=True)):
        with pytest.raises(ValueError):                                    # fused=True: this decoder computes in fp32
            dec.member_quantiles(z, 2, **kw)
    with pytest.raises(ValueError):
        dec.member_quantiles(z, 3, levels=(0.5,))
    with pytest.raises(RuntimeError, match="MI355X"):
        dec.member_quantiles(z, 2, levels=(0.5,))
    bf = torch.bfloat16
    base = dict(groups=[dict(H=torch.zeros(2 * 4 * 9, 40, dtype=bf), W2=torch.zeros(3 * 32, 40, dtype=bf), bias=torch.zeros(3 * 32))], C_=21, Cp=32, n_patches=9,
                members=4, levels=(0.5,), thr=torch.zeros(2, 3))
    for kw in (dict(levels=(1.5,)), dict(levels=(), thr=None), dict(members=129), dict(members=5), dict(dtype=torch.float32), dict(thr=torch.zeros(2, 4)), dict(thr=torch.zeros(9, 3)),
               dict(w=torch.zeros(7)), dict(counts=torch.zeros(9, dtype=torch.int64)), dict(out=dict(quant=torch.zeros(1, 2, 9, 3, 20))), dict(out=dict(mean=torch.zeros(1))),
               dict(groups=[dict(H=torch.zeros(72, 648, dtype=bf), W2=torch.zeros(96, 648, dtype=bf), bias=torch.zeros(96))]),
               dict(groups=[dict(H=torch.zeros(72, 40), W2=torch.zeros(96, 40), bias=torch.zeros(96))]), dict(groups=[])):
        args = dict(base)
        args.update(kw)
        with pytest.raises(ValueError):
            ops.decode_member_quantiles(**args)
    with pytest.raises(RuntimeError, match="MI355X"):
        ops.decode_member_quantiles(**base)


def test_scale_thresholds_round_trips_against_the_scaler():
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
    thr = torch.tensor([[0.5, 7.0, -1.05], [-2.0, 0.0, -0.9]])
    got = mesh.scale_thresholds(thr)
    want = torch.stack([scalers[0].transform(thr[:, 0]), scalers[0].transform(thr[:, 1]), scalers[1].transform(thr[:, 2])], dim=1)
    assert got.dtype == torch.float32 and got.shape == (2, 3) and float((got - want).abs().max()) <= 4e-6 * float(want.abs().max())
    assert torch.equal(mesh.scale_thresholds(thr.tolist()), got)
    assert torch.equal(mesh.scale_thresholds([0.5, -2.0]), mesh.scale_thresholds(torch.tensor([[0.5] * 3, [-2.0] * 3])))
    a, _ = mesh._forward_coefficients()
    assert all(v > 0 for v in a)                                           # an increasing map keeps the sense of ">"
    x = data[0, :, 1]
    assert torch.equal(x > 7.0, scalers[0].transform(x) > got[0, 1]) or int(((x > 7.0) != (scalers[0].transform(x) > got[0, 1])).sum()) <= 1
    with pytest.raises(ValueError):
        mesh.scale_thresholds(torch.zeros(2, 4))
    down = MinMaxScaler((1, -1))
    down.min_val, down.max_val = torch.tensor(0.5), torch.tensor(2.0)
    with pytest.raises(ValueError, match="not increasing"):
        MeshUnpatcher(part, groups, [scalers[0], down]).scale_thresholds(thr)


# ------------------------------------------------------------------------------------------------ the entry point without a device
@pytest.fixture(scope="module")
def lib():
    from sea_amd import build, _native

    build.build(verbose=False)
    return _native.lib()


def _tables(n_groups=2):
    """A well-formed sea_decode_member_quantiles table over made-up (aligned, never dereferenced) addresses: 4 members of 2 histories, 9 patches, 3 fields."""
    from sea_amd import _native as N

    arr, p = (N.SeaDecodeMseGroup * n_groups)(), N.SeaDecodeMemberQuantiles()
    for g in range(n_groups):
        arr[g].H, arr[g].W2, arr[g].bias = 0x100000 + 0x10000 * g, 0x200000 + 0x10000 * g, 0x300000 + 0x10000 * g
        arr[g].ldh, arr[g].ldw, arr[g].n_fields, arr[g].field0 = 40, 40, 2 if g == 0 else 1, 0 if g == 0 else 2
    p.w, p.counts, p.thr, p.quant, p.exceed = 0x400000, 0x410000, 0x420000, 0x500000, 0x600000
    p.level[0], p.level[1], p.n_levels, p.n_thr = 0.5, 1.0, 2, 1
    p.ld, p.ld_map = 21, 2 * 9 * 3 * 21
    p.M, p.S, p.C, p.Cp, p.P, p.members, p.n_fields_total = 2 * 4 * 9, 40, 21, 32, 9, 4, 3
    return arr, p


def test_symbol_struct_size_and_refusals(lib):
    from sea_amd import _native as N

    assert hasattr(lib, "sea_decode_member_quantiles") and "sea_decode_member_quantiles" in N.EXPORTED_SYMBOLS
    T = N.SeaDecodeMemberQuantiles
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "sea_hip.h")).read()
    stated = int(re.search(r"sizeof\(SeaDecodeMemberQuantiles\) is (\d+)", header).group(1))
    assert C.sizeof(T) == stated == 128 and T.level.offset == 40 and T.ld.offset == 72 and T.n_levels.offset == 88 and T.n_fields_total.offset == 120
    assert int(re.search(r"#define SEA_QUANTILE_MAX_LEVELS (\d+)", header).group(1)) == N.QUANTILE_MAX_LEVELS
    assert lib.sea_abi_version() == 8 and len(N.ABI_STRUCTS) == 33 and T not in N.ABI_STRUCTS
    call = lambda arr, p, dt=N.SEA_BF16: lib.sea_decode_member_quantiles(arr, 2, C.byref(p), dt, None)   # noqa: E731
    # the library reads the fields where the binding writes them: its messages quote the values back
    for field, value, msg in (("members", 0, b"members=0"), ("ld", 20, b"ld=20 must cover C=21"), ("ld_map", 1133, b"ld_map=1133"), ("M", 71, b"M=71 is not a multiple"),
                              ("n_levels", 9, b"n_levels=9"), ("n_thr", -1, b"n_thr=-1"), ("quant", None, b"null pointer"), ("thr", None, b"null pointer"),
                              ("exceed", 0x600002, b"misaligned"), ("Cp", 40, b"Cp=40"), ("S", 36, b"S=36")):
        arr, p = _tables()
        setattr(p, field, value)
        assert call(arr, p) == -1 and msg in lib.sea_last_error() and b"sea_decode_member_quantiles" in lib.sea_last_error(), (field, lib.sea_last_error())
    for bad in (1.5, -0.25, float("nan"), float("inf")):
        arr, p = _tables()
        p.level[1] = bad
        assert call(arr, p) == -1 and b"sea_decode_member_quantiles: level[1]" in lib.sea_last_error(), bad
    arr, p = _tables()
    p.n_levels = p.n_thr = 0
    assert call(arr, p) == -1 and b"not both be 0" in lib.sea_last_error()
    arr, p = _tables()
    arr[1].field0 = 1
    assert call(arr, p) == -1 and b"group 1" in lib.sea_last_error()
    arr, p = _tables()
    assert call(arr, p, N.SEA_F32) == -3 and b"sea_decode_member_quantiles" in lib.sea_last_error()
    arr, p = _tables()
    p.S = 648
    for g in range(2):
        arr[g].ldh = arr[g].ldw = 648
    assert call(arr, p) == -3 and b"S=648" in lib.sea_last_error()
    arr, p = _tables()
    p.members, p.M = 129, 2 * 129 * 9
    assert call(arr, p) == -3 and b"members=129" in lib.sea_last_error()
    assert lib.sea_decode_member_quantiles(None, 2, C.byref(p), N.SEA_BF16, None) == -1 and lib.sea_decode_member_quantiles(arr, 2, None, N.SEA_BF16, None) == -1
