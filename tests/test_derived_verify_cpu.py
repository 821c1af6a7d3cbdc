"""CRPS, rank and spread verification of DERIVED fields (|u|, energy, differences), on the host: the composed DerivedVerification against the fp64
restatement `restate_field_verify` (tests/test_field_verify_cpu.py) applied to `_composed_derived`'s float32 values; the two forms of the observation;
into= semantics; the refusals of the Python layers; and sea_decode_derived_verify through ctypes without a device (the symbol, every refusal with its
message, the unsupported forms)."""
import ctypes as C

import pytest
import torch

from tests.test_derived_fields_cpu import REFUSED, derived_table, members_case, three
from tests.test_field_verify_cpu import MAPS, _tables, check_against, field_logw, restate_field_verify
from tests.test_sensor_cpu import make_decoder
from tests.test_verify_cpu import close

F64 = torch.float64
SIGMA = (0.5, 2.0, 1.0)                                                    # one per derived field of three(): 1 / sigma^2 = 4, 0.25, 1 are exact


def reference(Y, x_obs, pd, counts, sigma, logw, n, unbiased, derived):
    """restate_field_verify on _composed_derived's float32 values; the weight of a cell is the f32 product (1 / sigma_d^2) * precision, 0 beyond counts."""
    from sea_amd.ensemble import _composed_derived

    B, _, P, _, C_ = Y.shape
    nd = len(derived)
    X = _composed_derived(Y, derived).view(B * n, P, nd, C_)
    w32 = torch.ones(B, P, nd, C_)
    if sigma is not None:
        w32 = w32 * torch.tensor([1.0 / (s * s) for s in sigma], dtype=torch.float32).view(1, 1, nd, 1)
    if pd is not None:
        w32 = w32 * torch.where(pd[..., :C_] > 0, pd[..., :C_], torch.zeros(()))
    valid = (torch.arange(C_) < torch.tensor(counts)[:, None]).view(1, P, 1, C_)
    w = torch.where(valid, w32.to(F64), torch.zeros((), dtype=F64))
    return restate_field_verify(X.to(F64), x_obs.to(F64), w, logw, n, unbiased)


def as_dict(s):
    return {k: getattr(s, k) for k in MAPS + ("sums", "hist", "status") if getattr(s, k) is not None}


# ------------------------------------------------------------------------------------------------ the composed path
@pytest.mark.parametrize("n", [1, 2, 5])
def test_composed_path_against_the_restatement_on_the_derived_values(n):
    """All three ops on members that are multiples of 0.25 (ties with the readings occur): ranks, histograms, status and counts equal, the f32 maps
    within 1e-6 max(1, max |ref|), the fp64 sums within 1e-10 max(1, max |ref|) — check_against's bounds, on a few dozen cells per derived field."""
    from sea_amd.ensemble import DerivedVerification, FieldScores, _composed_derived

    dec = make_decoder("decode_mse_a")
    P, B = 2, 2
    C_ = dec.n_inp
    Y, obs, prec = members_case(n, 140 + n, dec, P, B)
    derived = three()
    counts = [C_, max(C_ - 3, 0)]
    x_obs = _composed_derived(obs, derived)
    on = (prec > 0).float()
    pd = torch.stack([on[:, :, d.a] * on[:, :, d.b] for d in derived], dim=2)
    assert 0 < int((pd == 0).sum()) < pd.numel()                           # the source precision map is gappy
    for logw in (None, field_logw(n, B, 11)):
        for unbiased in (True, False):
            for sigma in (None, SIGMA):
                tag = (n, logw is None, unbiased, sigma)
                ver = DerivedVerification(dec, P, n, derived, counts=counts, sigma=sigma, unbiased=unbiased, observed="fields")
                s = ver.from_fields(Y, obs, precision=prec, logw=logw)
                assert isinstance(s, FieldScores) and s.sums.shape == (B, 3, 8) and s.hist.shape == (B, 3, n + 1) and s.crps.shape == (B, P, 3, C_)
                check_against(as_dict(s), reference(Y, x_obs, pd, counts, sigma, logw, n, unbiased, derived), n, tag=tag)
                # observed="derived": readings of the derived quantity with their own precision map, weight precision / sigma_d^2
                pmap = pd * (0.5 + torch.rand(pd.shape, generator=torch.Generator().manual_seed(3)))
                s2 = DerivedVerification(dec, P, n, derived, counts=counts, sigma=sigma, unbiased=unbiased, observed="derived").from_fields(
                    Y, x_obs, precision=pmap, logw=logw)
                check_against(as_dict(s2), reference(Y, x_obs, pmap, counts, sigma, logw, n, unbiased, derived), n, tag=tag + ("derived",))
                # the two forms agree when the second is fed the first's derived observation and liveness
                s3 = DerivedVerification(dec, P, n, derived, counts=counts, sigma=sigma, unbiased=unbiased, observed="derived").from_fields(
                    Y, x_obs, precision=pd, logw=logw)
                assert all(torch.equal(getattr(s, k), getattr(s3, k)) for k in ("rank", "hist", "status")) and torch.equal(s.sums.isnan(), s3.sums.isnan())
                assert torch.equal(torch.nan_to_num(s.sums), torch.nan_to_num(s3.sums)) and torch.equal(torch.nan_to_num(s.crps), torch.nan_to_num(s3.crps))
    # without a precision map every valid cell is live; "BPCF" observations give the same scores; a maps subset leaves the others None
    ver = DerivedVerification(dec, P, n, derived, counts=counts, sigma=SIGMA)
    s = ver.from_fields(Y, obs[..., :C_].contiguous())
    check_against(as_dict(s), reference(Y, x_obs, None, counts, SIGMA, None, n, True, derived), n, tag=(n, "no precision"))
    t = DerivedVerification(dec, P, n, derived, counts=counts, sigma=SIGMA, layout="BPCF").from_fields(Y, obs.permute(0, 1, 3, 2).contiguous(), maps=("crps", "rank"))
    assert t.mean is None and t.spread is None and t.pit is None and torch.equal(t.rank, s.rank) and torch.equal(t.sums, s.sums)
    assert torch.equal(torch.nan_to_num(t.crps), torch.nan_to_num(s.crps))
    none = ver.from_fields(Y, obs, maps=())
    assert all(getattr(none, k) is None for k in MAPS) and torch.equal(none.hist, s.hist)
    # FieldScores' expressions work with n_derived for n_fields
    assert s.rmse.shape == (B, 3) and s.suggested_inflation.shape == (B, 3) and s.pooled().sums.shape == (B, 8)


def test_into_over_two_snapshots_is_one_call_over_both():
    """into= adds a second snapshot's sums and histograms onto the first result's tensors, in place: they are those of one call whose patches are both
    snapshots' patches (integers equal; the fp64 sums within 1e-12, two orders of adding a few dozen terms)."""
    from sea_amd.ensemble import DerivedVerification

    dec = make_decoder("decode_mse_a")
    n, P, B = 5, 2, 2
    C_ = dec.n_inp
    derived = three()
    Y1, o1, p1 = members_case(n, 71, dec, P, B)
    Y2, o2, p2 = members_case(n, 72, dec, P, B)
    logw = field_logw(n, B, 13)
    ver = DerivedVerification(dec, P, n, derived, sigma=SIGMA)
    first = ver.from_fields(Y1, o1, precision=p1, logw=logw)
    h1, s1 = first.hist.clone(), first.sums.clone()
    both = ver.from_fields(Y2, o2, precision=p2, logw=logw, into=first, maps=("rank",))
    assert both.sums is first.sums and both.hist is first.hist and both.crps is None and both.rank is not None
    second = ver.from_fields(Y2, o2, precision=p2, logw=logw)
    assert torch.equal(both.hist, h1 + second.hist) and torch.equal(both.sums, s1 + second.sums)
    one = DerivedVerification(dec, 2 * P, n, derived, sigma=SIGMA).from_fields(torch.cat([Y1, Y2], 2), torch.cat([o1, o2], 1), precision=torch.cat([p1, p2], 1), logw=logw)
    assert torch.equal(both.hist, one.hist) and torch.equal(both.sums[..., 0], one.sums[..., 0]) and torch.equal(both.sums[..., 6], one.sums[..., 6])
    for j in range(8):
        ok, ratio = close(both.sums[..., j], one.sums[..., j], 1e-12)
        assert ok, (j, ratio)


# ------------------------------------------------------------------------------------------------ refusals of the Python layers
def test_python_layers_refuse_before_a_device_is_touched():
    from sea_amd import _native as N
    from sea_amd import ops
    from sea_amd.ensemble import DerivedField, DerivedVerification, FieldScores
    from sea_amd.utils.train_utils import DerivedVerification as DV2

    assert DV2 is DerivedVerification
    dec = make_decoder("decode_mse_a").set_compute_dtype("bf16")
    P, n, B = 2, 2, 2
    G, D_, C_ = dec.num_groups, dec.embed_dim, dec.n_inp
    F = sum(len(g) for g in dec.field_groups)
    derived = three()
    nd = len(derived)
    for kw in (dict(observed="both"), dict(sigma=-1.0), dict(sigma=[1.0, 2.0]), dict(sigma=float("nan")), dict(layout="PBFC"), dict(fused="yes"), dict(members=0),
               dict(members=True), dict(n_patches=0), dict(derived=[]), dict(derived=[("magnitude", 0, 1)]), dict(derived=[DerivedField("energy", 0, F)]),
               dict(members=129, fused=True), dict(derived=three() * 3, fused=True)):
        args = dict(decoder=dec, n_patches=P, members=n, derived=derived)
        args.update(kw)
        with pytest.raises(ValueError, match="DerivedVerification"):
            DerivedVerification(**args)
    DerivedVerification(dec, P, 129, derived)                               # the composed path carries any member count
    v = DerivedVerification(dec, P, n, derived, sigma=SIGMA, fused=True)
    assert v._prec_host == [4.0, 0.25, 1.0] and v.verify.__func__ is DerivedVerification.__call__
    y, obs = torch.zeros(B * n, G, P * D_), torch.zeros(B, P, F, C_)
    for yy, oo, pp in ((torch.zeros(3, G, P * D_), obs, None), (torch.zeros(4, G, P * D_ + 1), obs, None), (y, torch.zeros(B, P + 1, F, C_), None), (y, obs.double(), None),
                       (y, obs[0], None), (y, obs, torch.ones(B, P, F, C_ + 1)), (y, obs, -torch.ones(B, P, F, C_)), (y, obs, torch.ones(B, P, F, C_).double()),
                       (y, torch.zeros(B, P, nd + F, C_), None)):
        with pytest.raises(ValueError, match="DerivedVerification"):
            v(yy, oo, pp)
    with pytest.raises(ValueError, match="must carry"):
        DerivedVerification(dec, P, n, derived, observed="derived", fused=True)(y, torch.zeros(B, P, nd + 1, C_))
    good_into = FieldScores(None, None, None, None, None, torch.zeros(B, nd, 8, dtype=F64), torch.zeros(B, nd, n + 1, dtype=torch.int64), torch.zeros(B, dtype=torch.int32))
    bad = (dict(logw=torch.zeros(3)), dict(logw=torch.zeros(4, dtype=torch.int64)), dict(logw=torch.zeros(4, 1)), dict(maps=("crps", "crps")), dict(maps=("skill",)),
           dict(into=dict(sums=good_into.sums, hist=good_into.hist)),
           dict(into=FieldScores(None, None, None, None, None, torch.zeros(B, nd, 8), good_into.hist, good_into.status)),
           dict(into=FieldScores(None, None, None, None, None, torch.zeros(B, F, 8, dtype=F64) if F != nd else torch.zeros(B, nd + 1, 8, dtype=F64), good_into.hist, good_into.status)),
           dict(into=FieldScores(None, None, None, None, None, good_into.sums, torch.zeros(B, nd, n + 2, dtype=torch.int64), good_into.status)))
    for kw in bad:
        with pytest.raises(ValueError, match="DerivedVerification"):
            v(y, obs, **kw)
        with pytest.raises(ValueError, match="DerivedVerification"):
            v.from_fields(torch.zeros(B, n, P, F, C_), obs, **kw)
    with pytest.raises(ValueError, match="DerivedVerification: Y must be"):
        v.from_fields(torch.zeros(B, n + 1, P, F, C_), obs)
    with pytest.raises(RuntimeError, match="MI355X"):
        v(y, obs, logw=torch.zeros(B, n), into=good_into, maps=())
    # Decode.member_derived_verify: its own table of refusals on host tensors, then the device
    z, xo = torch.zeros(B * n, P, G, D_), torch.zeros(B, P, nd, C_)
    for kw in (dict(members=0), dict(members=3), dict(obs=torch.zeros(B, P, nd, C_ - 1)), dict(obs=xo.double()), dict(obs=torch.zeros(B, P, nd + 1, C_)),
               dict(precision=torch.ones(B, P, nd, C_ + 4)), dict(field_precision=torch.ones(nd + 1)), dict(z=torch.zeros(B * n, P, G + 1, D_)), dict(logw=torch.zeros(5)),
               dict(logw=torch.zeros(B * n, dtype=F64)), dict(maps=("rank", "nope")), dict(into=dict(sums=torch.zeros(B, nd, 8, dtype=F64))),
               dict(derived=[DerivedField("energy", 0, F)]), dict(derived=[]), dict(derived=three() * 3, fused=True)):
        args = dict(z=z, obs=xo, members=n, derived=derived)
        args.update(kw)
        with pytest.raises(ValueError, match="member_derived_verify"):
            dec.member_derived_verify(**args)
    with pytest.raises(ValueError, match="bf16 only"):
        make_decoder("decode_mse_a").member_derived_verify(z, xo, n, derived, fused=True)
    with pytest.raises(ValueError, match="up to 128"):
        dec.member_derived_verify(torch.zeros(129, P, G, D_), xo[:1], 129, derived, fused=True)
    with pytest.raises(RuntimeError, match="MI355X"):
        dec.member_derived_verify(z, xo, n, derived, fused=True)
    # ops.decode_derived_verify: its own table of refusals on host tensors, then the device
    S, Cp = 40, 64
    M = B * n * P
    grp = [dict(H=torch.zeros(M, S, dtype=torch.bfloat16), W2=torch.zeros(2 * Cp, S, dtype=torch.bfloat16), bias=torch.zeros(2 * Cp))]
    o3 = torch.zeros(B * P, nd, 40)
    base = dict(groups=grp, derived=derived, obs=o3, C_=40, Cp=Cp, n_patches=P, members=n)
    for kw in (dict(members=0), dict(members=129), dict(members=3), dict(Cp=48), dict(C_=65), dict(obs=o3.double()), dict(obs=o3[:, :, :39]), dict(obs=o3[:, :2]),
               dict(prec=o3[:-1]), dict(prec_field=torch.ones(nd + 1)), dict(counts=torch.zeros(P, dtype=torch.int64)), dict(logw=torch.zeros(5)),
               dict(maps=("mean", "median")), dict(out=dict(crps=torch.zeros(B, P, nd, 39))), dict(out=dict(crps=torch.zeros(B, P, nd, 40), pit=torch.zeros(B, P, nd, 48))),
               dict(out=dict(sums=torch.zeros(B, nd, 8))), dict(out=dict(sums=torch.zeros(B, 2, 8, dtype=F64))), dict(out=dict(gram=torch.zeros(2))), dict(accumulate=True),
               dict(dtype=torch.float32), dict(groups=[]), dict(derived=[]), dict(derived=three() * 3), dict(derived=[DerivedField("energy", 0, 2)])):
        args = dict(base)
        args.update(kw)
        with pytest.raises(ValueError, match="decode_derived_verify"):
            ops.decode_derived_verify(**args)
    with pytest.raises(RuntimeError, match="MI355X"):
        ops.decode_derived_verify(**base)
    assert N.FIELD_VERIFY_MAX_N == 128 and N.DERIVED_MAX == 8


# ------------------------------------------------------------------------------------------------ the entry point without a device
NAME = b"sea_decode_derived_verify"


@pytest.fixture(scope="module")
def lib():
    from sea_amd import build, _native

    build.build(verbose=False)
    return _native.lib()


def tables():
    """sea_decode_member_verify's well-formed table (3 source fields in groups [0, 1] and [2], 4 members of 2 histories, 9 patches) with obs, prec, the maps
    and the workspace sized for 2 derived fields."""
    arr, p = _tables()
    p.ld_row, p.ld_prow, p.work_bytes = 2 * 24, 2 * 24, 2 * 9 * 2 * (8 + 3) * 8
    return arr, p


def call(lib, arr, ng, tab, nd, p, dt):
    return lib.sea_decode_derived_verify(arr, ng, tab, nd, None if p is None else C.byref(p), dt, None)


def test_symbol_and_refusals_without_a_device(lib):
    from sea_amd import _native as N

    assert hasattr(lib, NAME.decode()) and NAME.decode() in N.EXPORTED_SYMBOLS and lib.sea_abi_version() == 8
    for what, (rows, msg) in REFUSED.items():                               # an unknown op, a source out of range, a == b, a coefficient that is not finite
        arr, p = tables()
        assert call(lib, arr, 2, derived_table(*rows), len(rows), p, N.SEA_BF16) == -1, what
        assert msg in lib.sea_last_error() and NAME in lib.sea_last_error(), (what, lib.sea_last_error())
    for nd in (0, 9, -1):
        arr, p = tables()
        assert call(lib, arr, 2, derived_table(), nd, p, N.SEA_BF16) == -1 and NAME + f": n_derived={nd} outside 1..8".encode() in lib.sea_last_error()
    for field in ("obs", "sums", "hist", "status", "work"):
        arr, p = tables()
        setattr(p, field, None)
        assert call(lib, arr, 2, derived_table(), 2, p, N.SEA_BF16) == -1 and NAME + b": null pointer" in lib.sea_last_error(), field
    arr, p = tables()
    p.work_bytes -= 1
    assert call(lib, arr, 2, derived_table(), 2, p, N.SEA_BF16) == -1
    assert NAME + b": work_bytes=3167 below the 3168 that sea_decode_member_verify_ws_bytes(B=2, P=9, n_derived=2, members=4, Cp=32)" in lib.sea_last_error()
    # what sea_decode_member_verify refuses, under this entry point's name
    for field, value, msg in (("members", 0, b"members=0"), ("M", 71, b"M=71 is not a multiple of P * members = 9 * 4"), ("S", 36, b"S=36"), ("Cp", 40, b"Cp=40"),
                              ("C", 33, b"C=33"), ("n_fields_total", 4, b"cover 3 of the 4 fields"), ("ld_field", 20, b"ld_field=20 must cover C=21"),
                              ("ld_pfield", 20, b"ld_pfield=20 must cover C=21"), ("ld_out", 20, b"ld_out=20 must cover C=21"), ("unbiased", 2, b"unbiased=2 and accumulate=0"),
                              ("accumulate", -1, b"unbiased=1 and accumulate=-1"), ("obs", 0x400002, b"misaligned"), ("sums", 0x600004, b"misaligned"),
                              ("rank", 0x540002, b"misaligned"), ("work", 0x700004, b"misaligned")):
        arr, p = tables()
        setattr(p, field, value)
        assert call(lib, arr, 2, derived_table(), 2, p, N.SEA_BF16) == -1 and msg in lib.sea_last_error() and NAME in lib.sea_last_error(), (field, lib.sea_last_error())
    arr, p = tables()
    arr[1].W2 = None
    assert call(lib, arr, 2, derived_table(), 2, p, N.SEA_BF16) == -1 and NAME + b": group 1: null pointer" in lib.sea_last_error()
    arr, p = tables()
    assert call(lib, arr, 2, derived_table(), 2, p, 5) == -1 and NAME + b": bad dtype 5" in lib.sea_last_error()
    assert call(lib, arr, 0, derived_table(), 2, p, N.SEA_BF16) == -1 and NAME + b": n_groups=0" in lib.sea_last_error()
    assert call(lib, None, 2, derived_table(), 2, p, N.SEA_BF16) == -1 and call(lib, arr, 2, None, 2, p, N.SEA_BF16) == -1
    assert call(lib, arr, 2, derived_table(), 2, None, N.SEA_BF16) == -1 and NAME + b": null argument table" in lib.sea_last_error()
    # prec_field, prec, counts, logw and every map may be NULL: such a table passes the pointer checks and fails only at the check this test breaks
    arr, p = tables()
    p.prec_field = p.prec = p.counts = p.logw = p.mean = p.spread = p.crps = p.pit = p.rank = None
    p.ld_out, p.ld_pfield, p.work_bytes = 0, 0, 7
    assert call(lib, arr, 2, derived_table(), 2, p, N.SEA_BF16) == -1 and NAME + b": work_bytes=7" in lib.sea_last_error()


def test_unsupported_forms_without_a_device(lib):
    from sea_amd import _native as N

    arr, p = tables()
    cross = derived_table((0, 0, 1, 1.0, 0.0, 1.0, 0.0), (2, 2, 1, 1.0, 0.0, 1.0, 0.0))
    assert call(lib, arr, 2, cross, 2, p, N.SEA_BF16) == -3
    assert b"derived field 1: its sources a=2 and b=1 lie in different groups" in lib.sea_last_error() and NAME in lib.sea_last_error()
    arr, p = tables()
    assert call(lib, arr, 2, derived_table(), 2, p, N.SEA_F32) == -3 and b"bf16 only" in lib.sea_last_error() and NAME in lib.sea_last_error()
    arr, p = tables()
    p.S = 648
    for g in range(2):
        arr[g].ldh = arr[g].ldw = 648
    assert call(lib, arr, 2, derived_table(), 2, p, N.SEA_BF16) == -3 and b"S=648" in lib.sea_last_error() and NAME in lib.sea_last_error()
    arr, p = tables()
    p.members, p.M = 129, 2 * 129 * 9
    assert call(lib, arr, 2, derived_table(), 2, p, N.SEA_BF16) == -3 and b"members=129" in lib.sea_last_error() and NAME in lib.sea_last_error()
    # a refused table with a bad derived field is -1, not -3: the checks come first
    arr, p = tables()
    p.members, p.M = 129, 2 * 129 * 9
    assert call(lib, arr, 2, derived_table((0, 1, 1, 1.0, 0.0, 1.0, 0.0)), 1, p, N.SEA_BF16) == -1
