"""Verification of an ensemble against a dense snapshot, on the host: the composed path (every cell a sensor of _composed_verify, every (history,
field) a history of it) against the fp64 restatement `restate_verify` of tests/test_verify_cpu.py on `as_sensors(...)` of tests/test_field_enkf_cpu.py's
inputs; FieldScores' derived properties; into= semantics; the struct layout and the argument checks of sea_decode_member_verify without a device; the
refusals of the Python layers."""
import ctypes as C
import dataclasses
import functools

import pytest
import torch

from tests.test_field_enkf_cpu import F64, as_sensors, decoded, field_weights, ragged_counts
from tests.test_sensor_cpu import host_case, make_decoder
from tests.test_verify_cpu import DOMINANT, FLOATS, close, restate_verify

MAPS = FLOATS + ("rank",)


# ------------------------------------------------------------------------------------------------ the contract, in fp64
def restate_field_verify(Y, obs, w, logw, n, unbiased):
    """sea_decode_member_verify from the decoded members: restate_verify with every cell a sensor, field by field.  Y [B * n, P, F, C], obs [B, P, F,
    >= C], w [B, P, F, C] (0: dead), logw None / [B * n].  Returns the maps [B, P, F, C], sums [B, F, 8], hist [B, F, n + 1], status [B]."""
    Bm, P, F, C_ = Y.shape
    B = Bm // n
    out = {k: torch.zeros(B, P, F, C_, dtype=F64) for k in FLOATS}
    out["rank"] = torch.zeros(B, P, F, C_, dtype=torch.int64)
    sums, hist = torch.zeros(B, F, 8, dtype=F64), torch.zeros(B, F, n + 1, dtype=torch.int64)
    for f in range(F):
        pred, o, p, _ = as_sensors(Y[:, :, f:f + 1], obs[:, :, f:f + 1], w[:, :, f:f + 1], None)
        r = restate_verify(pred, o, p, logw, n, unbiased)
        for k in MAPS:
            out[k][:, :, f] = r[k].view(B, P, C_)
        sums[:, f], hist[:, f], status = r["sums"], r["hist"], r["status"]
    return dict(out, sums=sums, hist=hist, status=status)


def field_logw(n, B, seed):
    """verify_case's log-weights: normal, in history b member b % n leads by DOMINANT and, from two members on, member (b + 1) % n is dead."""
    g = torch.Generator().manual_seed(seed)
    logw = torch.randn(B, n, generator=g)
    for b in range(B):
        logw[b, b % n] = float(logw[b].max()) + DOMINANT
        if n >= 2:
            logw[b, (b + 1) % n] = float("-inf")
    return logw.reshape(-1).contiguous()


@functools.lru_cache(maxsize=None)
def verify_field_case(name, members, hist, with_counts, with_prec, with_logw, dtype="bf16"):
    """An end-to-end input on test_field_enkf_cpu's states and its fp64 restatement on the fp64-decoded values: dict(Y, obs, prec, counts, sigma, w, logw,
    unbiased, ref).  obs: the member mean plus unit normal noise; with_prec: a map in [0.25, 2] with a tenth of the cells dead (precision 0, obs NaN)."""
    c = host_case(name)
    P, C_ = c["P"], c["n_inp"]
    F = sum(len(g) for g in c["groups"])
    g = torch.Generator().manual_seed(81000 + 100 * members + 10 * hist + 4 * with_counts + 2 * with_prec + with_logw + ord(name))
    Y = decoded(name, members, hist, dtype)
    obs = Y.view(hist, members, P, F, C_).mean(1).to(torch.float32) + torch.randn(hist, P, F, C_, generator=g)
    prec = None
    if with_prec:
        prec = 0.25 + 1.75 * torch.rand(hist, P, F, C_, generator=g)
        miss = torch.rand(hist, P, F, C_, generator=g) < 0.1
        prec[miss] = 0.0
        obs[miss] = float("nan")
    counts = ragged_counts(name, members) if with_counts else None
    sigma = 0.5
    logw = field_logw(members, hist, 5 * members + hist) if with_logw else None
    w32 = torch.full((hist, P, F, C_), 1.0 / sigma ** 2, dtype=torch.float32)
    if prec is not None:   # the weight is an fp32 product (include/sea_hip.h): 1 / w enters two sums
        w32 = w32 * torch.where(prec > 0, prec, torch.zeros(()))
    w = field_weights((hist, P, F, C_), None, None, counts) * w32.to(F64)
    unbiased = bool((members + hist) % 2)
    return dict(Y=Y, obs=obs, prec=prec, counts=counts, sigma=sigma, w=w, logw=logw, unbiased=unbiased, ref=restate_field_verify(Y, obs, w, logw, members, unbiased))


def composed(k, n, maps=MAPS):
    from sea_amd.ensemble import _composed_field_verify, _field_cell_weights

    B, P, F, C_ = k["obs"].shape
    pf = torch.full((F,), 1.0 / k["sigma"] ** 2, dtype=torch.float32)
    cnt = None if k["counts"] is None else torch.tensor(k["counts"], dtype=torch.int32)
    w = _field_cell_weights((B, P, F, C_), pf, k["prec"], cnt, torch.device("cpu"))
    return _composed_field_verify(k["Y"].to(torch.float32), k["obs"], w, k["logw"], n, k["unbiased"], maps=maps)


def check_against(got, ref, n, tol_f32=1e-6, tol_f64=1e-10, tag=()):
    assert torch.equal(got["rank"].long(), ref["rank"]), tag
    assert torch.equal(got["hist"], ref["hist"]) and torch.equal(got["status"].long(), ref["status"]), tag
    assert torch.equal(got["sums"][..., 0], ref["sums"][..., 0]) and torch.equal(got["sums"][..., 6], ref["sums"][..., 6]), tag
    worst = 0.0
    for k in FLOATS:
        ok, ratio = close(got[k], ref[k], tol_f32)
        assert ok, tag + (k, ratio)
        worst = max(worst, ratio)
    for j in range(8):
        ok, ratio = close(got["sums"][..., j], ref["sums"][..., j], tol_f64)
        assert ok, tag + ("sums", j, ratio)
    return worst


# ------------------------------------------------------------------------------------------------ the composed path
@pytest.mark.parametrize("name,members,hist", [("a", 2, 3), ("a", 5, 1), ("a", 17, 3), ("b", 11, 3), ("c", 5, 7)])
def test_composed_path_against_the_restatement(name, members, hist):
    """On the SAME decoded values (fp64-decoded, rounded to fp32 for both): ranks, histograms, status and counts equal; the f32 maps within 1e-6
    max(1, max |ref|) (fp64 arithmetic plus the fp32 store); the fp64 sums within 1e-10 max(1, max |ref|) — test_verify_cpu's bounds: a field of these
    shapes has at most a few hundred cells."""
    from sea_amd.ensemble import FieldScores

    for cnt in (False, True):
        for wp in (False, True):
            for wl in (False, True):
                k = dict(verify_field_case(name, members, hist, cnt, wp, wl))
                k["Y"] = k["Y"].to(torch.float32).to(F64)
                ref = restate_field_verify(k["Y"], k["obs"], k["w"], k["logw"], members, k["unbiased"])
                got = composed(k, members)
                B, P, F, C_ = k["obs"].shape
                assert got["sums"].shape == (B, F, 8) and got["hist"].shape == (B, F, members + 1) and got["status"].shape == (B,)
                assert all(got[m].shape == (B, P, F, C_) for m in MAPS)
                check_against(got, ref, members, tag=(name, members, hist, cnt, wp, wl))
                # pooled(): the fields added up are the restatement with every cell of every field a sensor
                s = FieldScores(**{m: got[m] for m in MAPS}, sums=got["sums"], hist=got["hist"], status=got["status"]).pooled()
                pred, o, p, _ = as_sensors(k["Y"], k["obs"], k["w"], None)
                allc = restate_verify(pred, o, p, k["logw"], members, k["unbiased"])
                assert torch.equal(s.hist, allc["hist"]) and torch.equal(s.sums[:, 0], allc["sums"][:, 0]) and s.sums.shape == (B, 8)
                for j in range(8):
                    ok, ratio = close(s.sums[:, j], allc["sums"][:, j], 1e-10)
                    assert ok, (name, members, cnt, wp, wl, j, ratio)
                if bool((allc["sums"][:, 0] > 0).all()):
                    assert torch.allclose(s.mean_crps, allc["sums"][:, 1] / allc["sums"][:, 0], rtol=1e-9, atol=0)


def test_composed_path_maps_subset_bad_cells_and_unscored_histories():
    name, n, hist = "a", 5, 3
    k = dict(verify_field_case(name, n, hist, True, True, True))
    got = composed(k, n, maps=("crps", "rank"))
    assert set(got) == {"crps", "rank", "sums", "hist", "status"}
    # a NaN value of a live member makes its history's live cells bad; of a dead member, nothing
    Y = k["Y"].clone()
    dead = [j for j in range(n) if k["logw"][n + j] == float("-inf")][0]
    live = [j for j in range(n) if j != dead][0]
    Y[n + dead] = float("nan")
    k2 = dict(k, Y=Y)
    same = composed(k2, n)
    base = composed(k, n)
    assert torch.equal(same["rank"], base["rank"]) and torch.equal(same["sums"], base["sums"])
    Y[n + live] = float("nan")
    bad = composed(dict(k, Y=Y), n)
    w1 = k["w"][1] > 0
    assert torch.equal(bad["rank"][1][w1], torch.full_like(bad["rank"][1][w1], -2)) and bool(torch.isnan(bad["crps"][1][w1]).all())
    assert torch.equal(bad["rank"][1][~w1], torch.full_like(bad["rank"][1][~w1], -1)) and float(bad["crps"][1][~w1].abs().max()) == 0.0
    assert torch.equal(bad["sums"][1, :, 6], w1.sum((0, 2)).to(F64)) and float(bad["sums"][1, :, :6].abs().max()) == 0.0 and int(bad["hist"][1].sum()) == 0
    assert torch.equal(bad["rank"][0], base["rank"][0]) and torch.equal(bad["sums"][0], base["sums"][0]) and torch.equal(bad["sums"][2], base["sums"][2])
    # invalid log-weights: the history is not scored
    lw = k["logw"].clone()
    lw[2 * n] = float("nan")
    un = composed(dict(k, logw=lw), n)
    assert un["status"].tolist() == [base["status"][0].item(), base["status"][1].item(), -1]
    assert float(un["sums"][2].abs().max()) == 0.0 and int(un["hist"][2].sum()) == 0 and bool((un["rank"][2] == -1).all()) and float(un["crps"][2].abs().max()) == 0.0
    assert torch.equal(un["sums"][:2], base["sums"][:2])


# ------------------------------------------------------------------------------------------------ FieldScores
def test_derived_scores_on_hand_made_sums():
    from sea_amd.ensemble import EnsembleScores, FieldScores

    sums = torch.tensor([[[4.0, 2.0, 16.0, 4.0, 6.0, -2.0, 1.0, 8.0], [2.0, 1.0, 2.0, 8.0, 1.0, 1.0, 0.0, 1.0]],
                         [[0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 3.0, 0.0], [1.0, 0.5, 9.0, 1.0, 2.0, 3.0, 0.0, 5.0]]], dtype=F64)
    hist = torch.arange(2 * 2 * 4).view(2, 2, 4)
    s = FieldScores(crps=None, pit=None, rank=None, mean=None, spread=None, sums=sums, hist=hist, status=torch.tensor([3, 3], dtype=torch.int32))
    assert s.count.tolist() == [[4.0, 2.0], [0.0, 1.0]]
    assert s.mean_crps[0].tolist() == [0.5, 0.5] and s.rmse[0].tolist() == [2.0, 1.0] and s.mean_spread[0].tolist() == [1.0, 2.0]
    assert s.spread_skill[0].tolist() == [0.5, 2.0] and s.consistency[0].tolist() == [1.5, 0.5] and s.bias[0].tolist() == [-0.5, 0.5]
    assert s.suggested_inflation[0].tolist() == pytest.approx([2.0 ** 0.5, 1.0], rel=1e-15) and s.suggested_inflation[1, 1].item() == 2.0
    assert bool(torch.isnan(s.rmse[1, 0])) and bool(torch.isnan(s.mean_crps[1, 0]))            # a field without a live good cell
    p = s.pooled()
    assert isinstance(p, EnsembleScores) and torch.equal(p.sums, sums.sum(1)) and torch.equal(p.hist, hist.sum(1)) and p.status is s.status
    assert p.rmse.tolist() == pytest.approx([(18.0 / 6.0) ** 0.5, 3.0], rel=1e-15) and p.mean_crps.tolist() == [0.5, 0.5]
    with pytest.raises(dataclasses.FrozenInstanceError):
        s.sums = sums


def test_into_over_two_snapshots_is_one_call_over_both():
    """The sums and histograms of two snapshots added up (what into= does: in place, onto the earlier object's tensors) are those of one call whose
    patches are both snapshots' patches."""
    name, n, hist = "a", 5, 3
    k1, k2 = verify_field_case(name, n, hist, True, True, True), verify_field_case(name, n, hist, False, True, True)
    a, b = composed(k1, n), composed(k2, n)
    both = dict(k1, Y=torch.cat([k1["Y"], k2["Y"]], 1), obs=torch.cat([k1["obs"], k2["obs"]], 1), prec=torch.cat([k1["prec"], k2["prec"]], 1),
                counts=list(k1["counts"]) + [host_case(name)["n_inp"]] * host_case(name)["P"])
    one = composed(both, n)
    sums, hist = a["sums"].clone(), a["hist"].clone()
    s2, h2 = sums.add_(b["sums"]), hist.add_(b["hist"])
    assert s2 is sums and h2 is hist
    assert torch.equal(hist, one["hist"]) and torch.equal(sums[..., 0], one["sums"][..., 0])
    for j in range(8):
        ok, ratio = close(sums[..., j], one["sums"][..., j], 1e-12)
        assert ok, (j, ratio)


# ------------------------------------------------------------------------------------------------ refusals of the Python layers
def test_python_layers_refuse_before_a_device_is_touched():
    from sea_amd import _native as N
    from sea_amd import ops
    from sea_amd.ensemble import FieldScores, FieldVerification
    from sea_amd.utils.train_utils import FieldScores as FS2, FieldVerification as FV2

    assert FV2 is FieldVerification and FS2 is FieldScores and N.FIELD_VERIFY_MAX_N == 128
    c = host_case("a")
    dec = make_decoder("a").set_compute_dtype("bf16")
    P, D_, G, C_ = c["P"], c["D"], len(c["groups"]), c["n_inp"]
    F = sum(len(g) for g in c["groups"])
    for members in (0, -1, True, 2.0):
        with pytest.raises(ValueError):
            FieldVerification(dec, P, members)
    for kw in (dict(sigma=-1.0), dict(sigma=[1.0, 2.0]), dict(layout="PBFC"), dict(fused="yes")):
        with pytest.raises(ValueError):
            FieldVerification(dec, P, 2, **kw)
    with pytest.raises(ValueError):
        FieldVerification(dec, 0, 2)
    with pytest.raises(ValueError, match="up to 128"):
        FieldVerification(dec, P, 129, fused=True)
    FieldVerification(dec, P, 129)                                                        # the composed path carries any member count
    v = FieldVerification(dec, P, 2, sigma=[0.5, 1.0, 2.0][:F] if F <= 3 else 1.0, fused=True)
    if F == 3:
        assert v._prec_host == [4.0, 1.0, 0.25]
    y, obs = torch.zeros(4, G, P * D_), torch.zeros(2, P, F, C_)
    for yy, oo, pp in ((torch.zeros(3, G, P * D_), obs, None), (torch.zeros(4, G, P * D_ + 1), obs, None), (y, torch.zeros(2, P + 1, F, C_), None), (y, obs.double(), None),
                       (y, obs[0], None), (y, obs, torch.ones(2, P, F, C_ + 1)), (y, obs, -torch.ones(2, P, F, C_)), (y, obs, torch.ones(2, P, F, C_).double())):
        with pytest.raises(ValueError):
            v(yy, oo, pp)
    good_into = FieldScores(None, None, None, None, None, torch.zeros(2, F, 8, dtype=F64), torch.zeros(2, F, 3, dtype=torch.int64), torch.zeros(2, dtype=torch.int32))
    for kw in (dict(logw=torch.zeros(3)), dict(logw=torch.zeros(4, dtype=torch.int64)), dict(logw=torch.zeros(4, 1)), dict(maps=("crps", "crps")), dict(maps=("skill",)),
               dict(into=dict(sums=good_into.sums, hist=good_into.hist)),
               dict(into=FieldScores(None, None, None, None, None, torch.zeros(2, F, 8), good_into.hist, good_into.status)),
               dict(into=FieldScores(None, None, None, None, None, good_into.sums, torch.zeros(2, F, 4, dtype=torch.int64), good_into.status))):
        with pytest.raises(ValueError):
            v(y, obs, **kw)
    with pytest.raises(RuntimeError, match="MI355X"):
        v(y, obs, logw=torch.zeros(2, 2), into=good_into, maps=())
    z = torch.zeros(4, P, G, D_)
    for kw in (dict(members=0), dict(members=3), dict(obs=torch.zeros(2, P, F, C_ - 1)), dict(obs=obs.double()), dict(precision=torch.ones(2, P, F, C_ + 4)),
               dict(field_precision=torch.ones(F + 1)), dict(z=torch.zeros(4, P, G + 1, D_)), dict(logw=torch.zeros(5)), dict(logw=torch.zeros(4, dtype=F64)),
               dict(maps=("rank", "nope")), dict(into=dict(sums=torch.zeros(2, F, 8, dtype=F64))), dict(members=4, z=torch.zeros(4 * 129, P, G, D_)[:0])):
        args = dict(z=z, obs=obs, members=2)
        args.update(kw)
        with pytest.raises(ValueError):
            dec.member_verify(**args)
    with pytest.raises(ValueError, match="bf16 only"):
        make_decoder("a").member_verify(z, obs, 2, fused=True)
    with pytest.raises(ValueError, match="up to 128"):
        dec.member_verify(torch.zeros(129, P, G, D_), obs[:1], 129, fused=True)
    with pytest.raises(RuntimeError, match="MI355X"):
        dec.member_verify(z, obs, 2, fused=True)
    # ops.decode_member_verify: its own table of refusals on host tensors, then the device
    S, Cp = 40, 64
    M = 2 * 2 * P
    grp = [dict(H=torch.zeros(M, S, dtype=torch.bfloat16), W2=torch.zeros(F * Cp, S, dtype=torch.bfloat16), bias=torch.zeros(F * Cp))]
    o3 = torch.zeros(2 * P, F, 40)
    base = dict(groups=grp, obs=o3, C_=40, Cp=Cp, n_patches=P, members=2)
    for kw in (dict(members=0), dict(members=129), dict(members=3), dict(Cp=48), dict(C_=65), dict(obs=o3.double()), dict(obs=o3[:, :, :39]), dict(prec=o3[:-1]),
               dict(prec_field=torch.ones(F + 1)), dict(counts=torch.zeros(P, dtype=torch.int64)), dict(logw=torch.zeros(5)), dict(maps=("mean", "median")),
               dict(out=dict(crps=torch.zeros(2, P, F, 39))), dict(out=dict(crps=torch.zeros(2, P, F, 40), pit=torch.zeros(2, P, F, 48))),
               dict(out=dict(sums=torch.zeros(2, F, 8))), dict(out=dict(gram=torch.zeros(2))), dict(accumulate=True), dict(dtype=torch.float32), dict(groups=[])):
        args = dict(base)
        args.update(kw)
        with pytest.raises(ValueError):
            ops.decode_member_verify(**args)
    with pytest.raises(RuntimeError, match="MI355X"):
        ops.decode_member_verify(**base)


# ------------------------------------------------------------------------------------------------ the entry points without a device
@pytest.fixture(scope="module")
def lib():
    from sea_amd import build, _native

    build.build(verbose=False)
    return _native.lib()


def _tables(n_groups=2):
    """A well-formed sea_decode_member_verify table over made-up (aligned, never dereferenced) addresses: 4 members of 2 histories, 9 patches, 3 fields."""
    from sea_amd import _native as N

    arr, p = (N.SeaDecodeMseGroup * n_groups)(), N.SeaDecodeMemberVerify()
    for g in range(n_groups):
        arr[g].H, arr[g].W2, arr[g].bias = 0x100000 + 0x10000 * g, 0x200000 + 0x10000 * g, 0x300000 + 0x10000 * g
        arr[g].ldh, arr[g].ldw, arr[g].n_fields, arr[g].field0 = 40, 40, 2 if g == 0 else 1, 0 if g == 0 else 2
    p.obs, p.prec_field, p.prec, p.counts, p.logw = 0x400000, 0x410000, 0x420000, 0x430000, 0x440000
    p.mean, p.spread, p.crps, p.pit, p.rank = 0x500000, 0x510000, 0x520000, 0x530000, 0x540000
    p.sums, p.hist, p.status, p.work = 0x600000, 0x610000, 0x620000, 0x700000
    p.ld_row, p.ld_field, p.ld_prow, p.ld_pfield, p.ld_out = 3 * 24, 24, 3 * 24, 24, 21
    p.M, p.S, p.C, p.Cp, p.P, p.members, p.n_fields_total, p.unbiased, p.accumulate = 2 * 4 * 9, 40, 21, 32, 9, 4, 3, 1, 0
    p.work_bytes = 2 * 9 * 3 * (8 + 3) * 8
    return arr, p


def test_symbols_and_struct_layout(lib):
    from sea_amd import _native as N

    for name in ("sea_decode_member_verify", "sea_decode_member_verify_ws_bytes"):
        assert hasattr(lib, name) and name in N.EXPORTED_SYMBOLS
    T = N.SeaDecodeMemberVerify
    assert C.sizeof(T) == 200                                                               # include/sea_hip.h states it
    assert T.logw.offset == 32 and T.rank.offset == 72 and T.work.offset == 104 and T.ld_row.offset == 112 and T.ld_out.offset == 144 and T.work_bytes.offset == 152
    assert T.M.offset == 160 and T.members.offset == 180 and T.unbiased.offset == 188 and T.accumulate.offset == 192
    assert lib.sea_abi_version() == 8 and len(N.ABI_STRUCTS) == 33 and N.ABI_STRUCTS[-1] is N.SeaKvFork and T not in N.ABI_STRUCTS
    # 8 sums and members + 1 int32 bins, in 8-byte words, per (history, patch, field)
    # ... and chunk of 16 tiles (512 columns) of a field
    assert lib.sea_decode_member_verify_ws_bytes(2, 9, 3, 4, 32) == 2 * 9 * 3 * (8 + 3) * 8 and lib.sea_decode_member_verify_ws_bytes(1, 1, 1, 128, 512) == (8 + 65) * 8
    assert lib.sea_decode_member_verify_ws_bytes(1, 1, 1, 1, 544) == 2 * (8 + 1) * 8 and lib.sea_decode_member_verify_ws_bytes(1, 2, 3, 1, 1632) == 2 * 4 * 3 * 9 * 8
    for bad in ((0, 9, 3, 4, 32), (65536, 9, 3, 4, 32), (2, 0, 3, 4, 32), (2, 9, 0, 4, 32), (2, 9, 3, 0, 32), (2, 9, 3, 129, 32), (2, 9, 3, 4, 0), (2, 9, 3, 4, 40)):
        assert lib.sea_decode_member_verify_ws_bytes(*bad) == -1, bad
    # the library reads the fields where the binding writes them: its messages quote the values back
    for field, value, msg in (("members", 0, b"members=0"), ("ld_pfield", 20, b"ld_pfield=20 must cover C=21"), ("M", 71, b"M=71 is not a multiple of P * members = 9 * 4"),
                              ("ld_out", 20, b"ld_out=20 must cover C=21"), ("unbiased", 2, b"unbiased=2 and accumulate=0"), ("accumulate", 3, b"unbiased=1 and accumulate=3"),
                              ("work_bytes", 4751, b"work_bytes=4751 below the 4752")):
        arr, p = _tables()
        setattr(p, field, value)
        assert lib.sea_decode_member_verify(arr, 2, C.byref(p), N.SEA_BF16, None) == -1 and msg in lib.sea_last_error(), (field, lib.sea_last_error())


BREAKS = {"null obs": ("obs", None), "null sums": ("sums", None), "null hist": ("hist", None), "null status": ("status", None), "null work": ("work", None),
          "misaligned obs": ("obs", 0x400002), "misaligned prec": ("prec", 0x420001), "misaligned prec_field": ("prec_field", 0x410003), "misaligned counts": ("counts", 0x430002),
          "misaligned logw": ("logw", 0x440001), "misaligned mean": ("mean", 0x500002), "misaligned spread": ("spread", 0x510001), "misaligned crps": ("crps", 0x520003),
          "misaligned pit": ("pit", 0x530002), "misaligned rank": ("rank", 0x540002), "misaligned sums": ("sums", 0x600004), "misaligned hist": ("hist", 0x610004),
          "misaligned status": ("status", 0x620002), "misaligned work": ("work", 0x700004), "members = 0": ("members", 0), "M = 0": ("M", 0), "M not a multiple": ("M", 70),
          "S odd": ("S", 36), "Cp = 40": ("Cp", 40), "C above Cp": ("C", 33), "C = 0": ("C", 0), "P = 0": ("P", 0), "ld_field short": ("ld_field", 20),
          "ld_row negative": ("ld_row", -1), "ld_pfield short": ("ld_pfield", 20), "ld_out short": ("ld_out", 20), "fields": ("n_fields_total", 4),
          "unbiased = 2": ("unbiased", 2), "accumulate = -1": ("accumulate", -1), "workspace one byte short": ("work_bytes", 2 * 9 * 3 * 11 * 8 - 1)}


@pytest.mark.parametrize("what", sorted(BREAKS) + ["bad dtype", "no groups", "too many groups", "group null", "group misaligned", "group overlap", "group missing", "ldh short"])
def test_member_verify_refuses_bad_arguments_without_a_device(lib, what):
    from sea_amd import _native as N

    arr, p = _tables()
    dt, ng = N.SEA_BF16, 2
    if what in BREAKS:
        setattr(p, *BREAKS[what])
    elif what == "bad dtype":
        dt = 5
    elif what == "no groups":
        ng = 0
    elif what == "too many groups":
        ng = N.DECODE_MSE_MAX_GROUPS + 1
    elif what == "group null":
        arr[1].W2 = None
    elif what == "group misaligned":
        arr[0].bias = 0x300008
    elif what == "group overlap":
        arr[1].field0 = 1
    elif what == "group missing":
        ng = 1
    else:
        arr[0].ldh = 32
    assert lib.sea_decode_member_verify(arr, ng, C.byref(p), dt, None) == -1, what
    assert b"sea_decode_member_verify" in lib.sea_last_error()


def test_unsupported_forms_and_null_tables(lib):
    from sea_amd import _native as N

    arr, p = _tables()
    assert lib.sea_decode_member_verify(arr, 2, C.byref(p), N.SEA_F32, None) == -3 and b"sea_decode_member_verify" in lib.sea_last_error()
    arr, p = _tables()
    p.S = 648
    for g in range(2):
        arr[g].ldh = arr[g].ldw = 648
    assert lib.sea_decode_member_verify(arr, 2, C.byref(p), N.SEA_BF16, None) == -3 and b"S=648" in lib.sea_last_error()
    arr, p = _tables()
    p.members, p.M = 129, 2 * 129 * 9
    assert lib.sea_decode_member_verify(arr, 2, C.byref(p), N.SEA_BF16, None) == -3 and b"members=129" in lib.sea_last_error()
    assert lib.sea_decode_member_verify(None, 2, C.byref(p), N.SEA_BF16, None) == -1 and lib.sea_decode_member_verify(arr, 2, None, N.SEA_BF16, None) == -1
    # prec_field, prec, counts, logw and every map may be NULL: such a table passes the pointer checks and fails only at the check this test breaks
    arr, p = _tables()
    p.prec_field = p.prec = p.counts = p.logw = p.mean = p.spread = p.crps = p.pit = p.rank = None
    p.ld_out, p.ld_pfield, p.work_bytes = 0, 0, 7
    assert lib.sea_decode_member_verify(arr, 2, C.byref(p), N.SEA_BF16, None) == -1 and b"work_bytes=7" in lib.sea_last_error()
