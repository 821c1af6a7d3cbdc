"""CRPS, rank and spread verification of DERIVED fields on the device: sea_decode_derived_verify through ops.decode_derived_verify,
Decode.member_derived_verify and DerivedVerification end to end, on a rollout session and on the mesh.

Reference: `restate_field_verify` (tests/test_field_verify_cpu.py) applied to `_composed_derived`'s float32 values (tests/test_derived_fields_cpu.py ties
that function to a plain float32 loop and numpy's root).
  kernel      on EXACT operands (tests/test_field_verify_gpu.exact_case; dyadic coefficients: the affine steps, the squares and their sums are exact in
              float32; readings that are multiples of 0.25, so ties with energy and difference values occur): rank, hist, status and the two counts in
              sums EQUAL; the f32 maps within 1e-6 max(1, max |ref|); the fp64 sums within tests/test_field_verify_gpu.SUMS_TOL max(1, max |ref|) — the
              same cell and term counts as that test (2 patches x 40 cells, at most 128 + 64 terms per cell), so its derivation applies; against
              ops.ensemble_verify on the derived values: equal bits per cell; difference(a, 0) against ops.decode_member_verify: equal bits
  decode      random bf16 operands in every hidden-width form: rank and hist equal the restatement on _composed_derived of the member launch's own
              decoded values, maps within 1e-6
  end to end  bf16 fused: e <= 2 e_c + 1e-6 for the mean, spread and crps maps and the per-field rmse, mean_spread and mean_crps (e: against the fp64
              restatement on fp64-decoded values; e_c: fused=False on the same inputs — the project's rule); rank and pit are discontinuous in the
              decoded values and are compared on equal values only (the kernel tests)"""
import functools

import pytest
import torch

from tests.test_decode_loss_cpu import rel
from tests.test_decode_loss_gpu import DEV, case, decoder
from tests.test_derived_fields_gpu import ND, R_COEFF, derived3, derived64, groups_of, member_values, values
from tests.test_ensemble_quantiles_gpu import random_case
from tests.test_field_enkf_cpu import field_case, field_cases
from tests.test_field_verify_cpu import MAPS, restate_field_verify
from tests.test_field_verify_gpu import SUMS_TOL, X_B, X_C, X_COUNTS, X_CP, X_F, X_MEMBERS, X_P, check_exact, dev, exact_case
from tests.test_verify_cpu import FLOATS, close
from tests.test_verify_gpu import same_bits

pytestmark = pytest.mark.gpu

F64 = torch.float64
OUT = MAPS + ("sums", "hist", "status")


# ------------------------------------------------------------------------------------------------ exact operands
@functools.lru_cache(maxsize=None)
def derived_case(n, counts, with_prec, with_logw, C_=X_C, Cp=X_CP):
    """exact_case's operands with READINGS OF THE DERIVED QUANTITIES: dict(t, H (the dead members' hidden rows NaN), obs [B P, 3, C] multiples of 0.25,
    prec [B P, 3, C] or None (precisions in [0.25, 2], a tenth of the cells dead: precision 0, obs NaN there), logw, X float64 [B n, P, 3, C] —
    _composed_derived's float32 values of the exact members — and w [B, P, 3, C] float64 the cells' weights)."""
    t = exact_case(n, counts, with_prec, with_logw, C_, Cp)
    g = torch.Generator().manual_seed(5100 + 16 * n + 4 * counts[0] + 2 * with_prec + with_logw)
    B, P = X_B, X_P
    obs = torch.randint(-6, 17, (B * P, ND, C_), generator=g).float() / 4
    prec = None
    if with_prec:
        prec = 0.25 + 1.75 * torch.rand(B * P, ND, C_, generator=g)
        miss = torch.rand(B * P, ND, C_, generator=g) < 0.1
        prec[miss] = 0.0
        obs[miss] = float("nan")
    w = torch.ones(B, P, ND, C_, dtype=F64) if prec is None else prec.view(B, P, ND, C_).to(F64)
    w = torch.where((torch.arange(C_) < torch.tensor(counts)[:, None]).view(1, P, 1, C_), w, torch.zeros((), dtype=F64))
    H = t["H"]
    if t["logw"] is not None:
        H = H.clone()
        for m in range(B * n):
            if float(t["logw"][m]) == float("-inf"):
                H[m * P:(m + 1) * P] = float("nan")
    X = values(t["Y"], n, derived3()).reshape(B * n, P, ND, C_).to(F64)
    return dict(t=t, H=H, obs=obs, prec=prec, logw=t["logw"], X=X, w=w, C=C_, Cp=Cp)


def run(k, n, unbiased=True, accumulate=False, out=None, maps=MAPS, H=None, hist=None, derived=None, cols=None, logw="case", bias=None):
    """ops.decode_derived_verify on a derived case (hist: that history alone; cols: the columns of obs / prec that go with `derived`)."""
    from sea_amd import ops

    t, P = k["t"], X_P
    H = k["H"] if H is None else H
    obs, prec = k["obs"], k["prec"]
    logw = k["logw"] if isinstance(logw, str) else logw
    if cols is not None:
        obs, prec = obs[:, list(cols)].contiguous(), None if prec is None else prec[:, list(cols)].contiguous()
    if hist is not None:
        H, obs = H[hist * n * P:(hist + 1) * n * P], obs[hist * P:(hist + 1) * P]
        prec = None if prec is None else prec[hist * P:(hist + 1) * P]
        logw = None if logw is None else logw[hist * n:(hist + 1) * n]
    grp = groups_of(t, H)
    if bias is not None:
        grp[0]["bias"] = bias.to(DEV)
    return ops.decode_derived_verify(grp, derived3() if derived is None else derived, obs.to(DEV), k["C"], k["Cp"], P, n, prec=dev(prec), counts=t["counts"].to(DEV),
                                     logw=dev(logw), unbiased=unbiased, accumulate=accumulate, maps=maps, out=out)


def prefilled(B, n, fill, width=X_C, nd=ND):
    """Output buffers that hold NaN or -7: every element has to be written."""
    out = {k: torch.full((B, X_P, nd, width), fill, device=DEV) for k in FLOATS}
    out.update(rank=torch.full((B, X_P, nd, width), -7, device=DEV, dtype=torch.int32), sums=torch.full((B, nd, 8), fill, device=DEV, dtype=F64),
               hist=torch.full((B, nd, n + 1), -7, device=DEV, dtype=torch.int64), status=torch.full((B,), -7, device=DEV, dtype=torch.int32))
    return out


def reference(k, n, unbiased, X=None):
    return restate_field_verify(k["X"] if X is None else X, k["obs"].view(X_B, X_P, ND, -1), k["w"], k["logw"], n, unbiased)


def written(got):
    """No prefilled -7 is left: rank >= -2, histogram bins and status are counts (or -1)."""
    return bool((got["rank"] >= -2).all()) and bool((got["hist"] >= 0).all()) and bool((got["status"] >= -1).all())


# ------------------------------------------------------------------------------------------------ 1: the kernel on exact operands
@pytest.mark.parametrize("n", X_MEMBERS)
def test_kernel_against_fp64_on_exact_operands(n):
    from sea_amd import ops

    worst32, worst64, cases, ties = 0.0, 0.0, 0, 0
    for counts in X_COUNTS:
        for wp, wl in ((False, False), (True, True)):
            k = derived_case(n, counts, wp, wl)
            live = (k["w"] > 0).view(X_B, 1, X_P, ND, X_C)
            ties += int(((k["X"].view(X_B, n, X_P, ND, X_C) == k["obs"].view(X_B, 1, X_P, ND, X_C).to(F64)) & live)[:, :, :, 1:].sum())
            for unbiased in (True, False):
                ref = reference(k, n, unbiased)
                out = prefilled(X_B, n, float("nan"))
                got = run(k, n, unbiased, out=out)
                assert ops.last_form()[:2] == ("decode.derived_verify", 128) and all(got[m].data_ptr() == out[m].data_ptr() for m in out)
                assert written(got) and not bool(torch.isnan(got["sums"]).any())
                a, b = check_exact(got, ref, (n, counts, wp, wl, unbiased))
                worst32, worst64, cases = max(worst32, a), max(worst64, b), cases + 1
            if wl and n >= 2:
                assert int(ref["status"][0]) == n - 1                           # the dead member (its hidden rows NaN) is not counted and reaches nothing
    if n >= 5:
        assert ties > 0                                                       # a member's energy or difference EQUALS the reading: the rank's strictness is tested
    print(f"derived verify N = {n}: rank, hist, status, counts equal ({ties} ties of a member with the reading); largest error / bound over {cases} cases: "
          f"f32 maps {worst32:.3e} (bound 1e-6), fp64 sums {worst64:.3e} (bound {SUMS_TOL:.1e})")


# ------------------------------------------------------------------------------------------------ 2: against the sensor kernel
@pytest.mark.parametrize("n", [2, 17, 64, 128])
def test_derived_cells_are_scored_as_sensors(n):
    """ops.ensemble_verify on the same derived values as a prediction matrix, every cell a sensor in (patch, derived field, cell) order: the f32 maps and
    the ranks have equal BITS (one device function scores a derived cell and a sensor), status equal; hist and the counts pooled over the derived fields
    equal, the pooled sums within the sums bound (another order of adding)."""
    from sea_amd import ops

    B, P, C_ = X_B, X_P, X_C
    for counts, wp, wl in ((X_COUNTS[0], True, True), (X_COUNTS[0], False, False), (X_COUNTS[1], True, False)):
        k = derived_case(n, counts, wp, wl)
        got = run(k, n, True)
        pred = k["X"].reshape(B * n, P * ND * C_).to(torch.float32).to(DEV)
        s = ops.ensemble_verify(pred, k["obs"].reshape(B, P * ND * C_).to(DEV), n, prec=k["w"].reshape(B, P * ND * C_).to(torch.float32).to(DEV), logw=dev(k["logw"]),
                                unbiased=True)
        assert torch.equal(got["status"], s["status"])
        assert same_bits({m: got[m].reshape(B, -1) for m in MAPS}, {m: s[m] for m in MAPS}), (n, counts, wp, wl)
        assert torch.equal(got["hist"].sum(1), s["hist"]) and torch.equal(got["sums"].sum(1)[:, 0], s["sums"][:, 0]) and torch.equal(got["sums"].sum(1)[:, 6], s["sums"][:, 6])
        for j in range(8):
            ok, ratio = close(got["sums"].sum(1)[:, j].cpu(), s["sums"][:, j].cpu(), SUMS_TOL)
            assert ok, (n, counts, wp, wl, j, ratio)


# ------------------------------------------------------------------------------------------------ 3: a zero source b
@pytest.mark.parametrize("S", [40, 640])
def test_a_zero_source_gives_the_member_launch_bits(S):
    """difference(a, b) with scale_a = 1, shift_a = 0 and a source b whose weights and bias are zero: x = y_a - 0 = y_a, so the maps are the member launch's
    maps of field a bit for bit, and so are the sums and the histogram."""
    from sea_amd import ops
    from sea_amd.ensemble import DerivedField

    r = dict(random_case(S))
    W2, bias = r["W2"].clone(), r["bias"].clone()
    W2.view(r["F"], r["Cp"], S)[1] = 0.0
    bias.view(r["F"], r["Cp"])[1] = 0.0
    n, B, P, F, C_ = r["n"], r["B"], r["P"], r["F"], r["C"]
    g = torch.Generator().manual_seed(31 + S)
    obs = torch.randn(B * P, F, C_, generator=g)
    prec = (torch.rand(B * P, F, C_, generator=g) > 0.15).float() * (0.5 + torch.rand(B * P, F, C_, generator=g))
    logw = torch.tensor([0.3, -0.2, 0.1, 0.0, float("-inf"), 0.7])
    counts = torch.tensor([C_ - 7], dtype=torch.int32).to(DEV)
    grp = [dict(H=r["H"].to(DEV).to(torch.bfloat16), W2=W2.to(DEV).to(torch.bfloat16), bias=bias.to(DEV))]
    want = ops.decode_member_verify(grp, obs.to(DEV), C_, r["Cp"], P, n, prec=prec.to(DEV), counts=counts, logw=logw.to(DEV))
    got = ops.decode_derived_verify(grp, [DerivedField("difference", 0, 1)], obs[:, :1].contiguous().to(DEV), C_, r["Cp"], P, n, prec=prec[:, :1].contiguous().to(DEV),
                                    counts=counts, logw=logw.to(DEV))
    assert ops.last_form()[:2] == ("decode.derived_verify", 128 * ((S + 127) // 128))
    assert same_bits({m: got[m][:, :, 0] for m in MAPS}, {m: want[m][:, :, 0] for m in MAPS}), S
    assert same_bits(dict(s=got["sums"][:, 0]), dict(s=want["sums"][:, 0])) and torch.equal(got["hist"][:, 0], want["hist"][:, 0]) and torch.equal(got["status"], want["status"])
    assert float(got["sums"][:, 0, 0].sum()) > 0


# ------------------------------------------------------------------------------------------------ 4: every hidden-width form
@pytest.mark.parametrize("S", [72, 128, 256, 384, 512, 640])
def test_every_hidden_width_form(S):
    """Each SP the dispatcher instantiates at its widest S (and S = 72, no multiple of 32), random bf16-exact operands, coefficients that are not dyadic:
    rank and hist equal the restatement on _composed_derived of the member launch's own decoded values, the maps within 1e-6.  Every form is built
    without scratch, so none is refused."""
    from sea_amd import ops
    from sea_amd.ensemble import _composed_derived

    r = random_case(S)
    n, B, P, C_ = r["n"], r["B"], r["P"], r["C"]
    derived = derived3(*R_COEFF)
    X = _composed_derived(member_values(r), derived).view(B * n, P, ND, C_)
    g = torch.Generator().manual_seed(77 + S)
    obs = X.view(B, n, P, ND, C_).mean(1) + torch.randn(B, P, ND, C_, generator=g)
    prec = (torch.rand(B, P, ND, C_, generator=g) > 0.1).float() * (0.5 + torch.rand(B, P, ND, C_, generator=g))
    logw = torch.tensor([0.3, -0.2, 0.1, 0.0, float("-inf"), 0.7])
    ref = restate_field_verify(X.to(F64), obs.to(F64), prec.to(F64), logw, n, True)
    gap = (X.view(B, n, P, ND, C_).to(F64) - obs.to(F64).unsqueeze(1)).abs().min()
    assert float(gap) > 0.0                                                  # no member equals a reading: the ranks are decided
    grp = [dict(H=r["H"].to(DEV).to(torch.bfloat16), W2=r["W2"].to(DEV).to(torch.bfloat16), bias=r["bias"].to(DEV))]
    got = ops.decode_derived_verify(grp, derived, obs.view(B * P, ND, C_).to(DEV), C_, r["Cp"], P, n, prec=prec.view(B * P, ND, C_).to(DEV), logw=logw.to(DEV))
    assert ops.last_form()[:2] == ("decode.derived_verify", 128 * ((S + 127) // 128))
    got = {m: v.cpu() for m, v in got.items()}
    assert torch.equal(got["rank"].long(), ref["rank"]) and torch.equal(got["hist"], ref["hist"]) and torch.equal(got["status"].long(), ref["status"])
    worst = 0.0
    for m in FLOATS:
        ok, ratio = close(got[m], ref[m], 1e-6)
        assert ok, (S, m, ratio)
        worst = max(worst, ratio)
    print(f"derived verify form S = {S}: rank and hist equal against the member launch's values for all three ops; maps error / bound {worst:.3e} (bound 1e-6)")


# ------------------------------------------------------------------------------------------------ 5: more than one chunk of tiles
def test_a_field_wider_than_one_chunk_of_tiles():
    """530 columns in 544 are 17 tiles: a workgroup scores 16, so a derived field has two chunks whose partials the finish launch adds in order; counts 513
    leave the second chunk ONE valid column, counts 512 none (it leaves at once), and the columns from 513 on are dead cells of the maps."""
    n, C_, Cp = 5, 530, 544
    for counts in ((C_, 513), (512, 1)):
        k = derived_case(n, counts, True, True, C_, Cp)
        ref = reference(k, n, True)
        got = run(k, n, True, out=prefilled(X_B, n, float("nan"), C_ + 3))
        assert all(float(got[m][..., C_:].abs().max()) == 0.0 for m in FLOATS) and bool((got["rank"][..., C_:] == -1).all())
        a, b = check_exact({m: v[..., :C_] if m in MAPS else v for m, v in got.items()}, ref, (counts,))
        assert same_bits(run(k, n, True, out=prefilled(X_B, n, 7.0, C_ + 3)), got)
        alone = run(k, n, True, hist=1)
        assert same_bits({m: v[0] for m, v in alone.items()}, {m: v[1][..., :C_] if m in MAPS else v[1] for m, v in got.items()})
        print(f"derived verify chunks counts {counts}: error / bound f32 maps {a:.3e}, fp64 sums {b:.3e}")


# ------------------------------------------------------------------------------------------------ 6: special calls and cells
@pytest.mark.parametrize("n", [5, 128])
def test_special_calls_and_cells(n):
    k = derived_case(n, X_COUNTS[0], True, True)                             # obs is NaN at its dead cells: it is never read there
    want = run(k, n, True)
    live = (k["w"] > 0)
    assert not bool(torch.isnan(want["sums"]).any()) and all(not bool(torch.isnan(want[m]).any()) for m in FLOATS)
    assert torch.equal((want["rank"] == -1).cpu(), ~live) and all(float(want[m].cpu()[~live].abs().max()) == 0.0 for m in FLOATS)
    # Inf in source field 0 at column 3: x is +inf (magnitude, energy) or -inf (difference) for every member — a BAD cell where it is live
    bias = k["t"]["bias"].clone()
    bias.view(X_F, X_CP)[0, 3] = float("inf")
    Y = k["t"]["Y"].clone()
    Y[:, :, 0, 3] = float("inf")
    X = values(Y, n, derived3()).reshape(X_B * n, X_P, ND, X_C).to(F64)
    assert not bool(torch.isfinite(X[..., 3]).any())
    got = run(k, n, True, out=prefilled(X_B, n, 7.0), bias=bias)
    check_exact(got, reference(k, n, True, X=X), (n, "inf"))
    bad = torch.zeros_like(live)
    bad[..., 3] = live[..., 3]
    assert int(bad.sum()) > 0 and torch.equal((got["rank"] == -2).cpu(), bad) and all(torch.equal(torch.isnan(got[m]).cpu(), bad) for m in FLOATS)
    assert torch.equal(got["sums"][..., 6].cpu(), bad.sum((1, 3)).to(F64)) and torch.equal(got["sums"][..., 0].cpu(), (live & ~bad).sum((1, 3)).to(F64))
    assert torch.equal(got["hist"].sum(2).cpu(), (live & ~bad).sum((1, 3)))
    keep = ~bad.to(DEV)
    assert same_bits({m: got[m][keep] for m in MAPS}, {m: want[m][keep] for m in MAPS})          # the other cells do not see it
    dead3 = dict(k, prec=k["prec"].clone())
    dead3["prec"][:, :, 3] = 0.0                                             # the same column dead instead of bad: the sums but entry 6 have the same bits
    off = run(dead3, n, True)
    assert same_bits(dict(s=got["sums"][..., [0, 1, 2, 3, 4, 5, 7]]), dict(s=off["sums"][..., [0, 1, 2, 3, 4, 5, 7]])) and torch.equal(got["hist"], off["hist"])
    # invalid log-weights: history 1 is not scored — status -1, maps 0 / -1, nothing added — and history 0 is untouched
    lw = k["logw"].clone()
    lw[n] = float("inf")
    got = run(k, n, True, out=prefilled(X_B, n, float("nan")), logw=lw)
    assert got["status"].tolist() == [want["status"][0].item(), -1] and same_bits({m: v[0] for m, v in got.items()}, {m: v[0] for m, v in want.items()})
    assert all(float(got[m][1].abs().max()) == 0.0 for m in FLOATS + ("sums", "hist")) and bool((got["rank"][1] == -1).all())
    acc = run(k, n, True, accumulate=True, out=dict(sums=want["sums"].clone(), hist=want["hist"].clone()), logw=lw)
    assert same_bits(dict(s=acc["sums"][1]), dict(s=want["sums"][1])) and torch.equal(acc["hist"][1], want["hist"][1])
    # accumulate = the sum of two calls, in the calls' order
    k2 = derived_case(n, X_COUNTS[0], False, True)
    other = run(k2, n, True)
    acc = run(k2, n, True, accumulate=True, out=dict(sums=want["sums"].clone(), hist=want["hist"].clone()))
    assert torch.equal(acc["hist"], want["hist"] + other["hist"]) and same_bits(dict(s=acc["sums"]), dict(s=want["sums"] + other["sums"]))
    assert same_bits(acc, other, keys=MAPS + ("status",))
    # maps=() writes sums only; a subset leaves the others out
    for maps in ((), ("rank",), ("crps", "pit")):
        sub = run(k, n, True, maps=maps)
        assert set(sub) == set(maps) | {"sums", "hist", "status"} and same_bits(sub, want, keys=sub.keys()), (n, maps)


# ------------------------------------------------------------------------------------------------ 7: bits
@pytest.mark.parametrize("n", [5, 64, 128])
def test_two_runs_a_history_alone_and_the_company_of_other_derived_fields(n):
    for counts in X_COUNTS:
        k = derived_case(n, counts, True, True)
        want = run(k, n, True)
        assert same_bits(run(k, n, True, out=prefilled(X_B, n, -7.0, X_C + 9)), {m: v for m, v in want.items()}, keys=("sums", "hist", "status"))
        assert same_bits(run(k, n, True), want)                               # two runs, the same bits
        for h in range(X_B):                                                 # a history alone reproduces its own outputs
            alone = run(k, n, True, hist=h)
            assert same_bits({m: v[0] for m, v in alone.items()}, {m: v[h] for m, v in want.items()}), (n, counts, h)
        for order in ((0,), (2, 1, 0), (1, 1, 2, 0, 0, 1, 2, 0)):             # alone, reversed, and a full table of eight
            got = run(k, n, True, derived=tuple(derived3()[i] for i in order), cols=order)
            for slot, i in enumerate(order):
                assert same_bits({m: got[m][:, :, slot] for m in MAPS}, {m: want[m][:, :, i] for m in MAPS}), (n, counts, order, slot)
                assert same_bits(dict(s=got["sums"][:, slot]), dict(s=want["sums"][:, i])) and torch.equal(got["hist"][:, slot], want["hist"][:, i])
            assert torch.equal(got["status"], want["status"])


# ------------------------------------------------------------------------------------------------ 8: end to end
CASES = [c for c in field_cases() if not c[5]]
BY_SHAPE = {name: [c for c in CASES if c[0] == name] for name in ("a", "c")}
E2E_SIGMA = (0.5, 2.0)


def e2e_errors(s, ref):
    """Relative L2 errors of the continuous maps, and the largest relative error of rmse, mean_spread and mean_crps over the derived fields with a live cell."""
    cnt = ref["sums"][..., 0]
    on = cnt > 0
    means = ((s.mean_crps, ref["sums"][..., 1] / cnt), (s.rmse, (ref["sums"][..., 2] / cnt).sqrt()), (s.mean_spread, (ref["sums"][..., 3] / cnt).sqrt()))
    e = {q: rel(getattr(s, q).cpu(), ref[q]) for q in ("mean", "spread", "crps")}
    e["per-field"] = max(float(((got.cpu()[on] - want[on]).abs() / want[on].abs().clamp_min(1e-300)).max()) for got, want in means) if bool(on.any()) else 0.0
    return e


@pytest.mark.parametrize("name", ["a", "c"])
def test_derived_verification_bf16_against_fp64(name):
    """Decoders "a" (fields [[0, 1], [2]]) and "c" (fields [[0, 1]], hidden 624), observed="fields" with the cases' gappy precision maps and counts."""
    from sea_amd.ensemble import DerivedField, DerivedVerification, _composed_derived

    derived = (DerivedField("magnitude", 0, 1, *R_COEFF), DerivedField("difference", 1, 0, *R_COEFF))
    nd = len(derived)
    P = case(name)["P"]
    worst = {}
    for case_ in BY_SHAPE[name]:
        _, members, hist, cnt, wp, local = case_
        k = field_case(*case_)
        logw = torch.randn(hist * members, generator=torch.Generator().manual_seed(66 + members + hist)) if members % 2 else None
        F, C_ = k["obs"].shape[2:]
        X, _ = derived64(k["Y"].view(hist, members, P, F, C_), torch.zeros(hist, members, P, F, C_, dtype=F64), derived)
        x_obs = _composed_derived(k["obs"], derived).to(F64)
        on = torch.ones(hist, P, F, C_) if k["prec"] is None else (k["prec"] > 0).float()
        w = torch.stack([on[:, :, d.a] * on[:, :, d.b] for d in derived], dim=2).to(F64) * torch.tensor([1.0 / (s * s) for s in E2E_SIGMA], dtype=F64).view(1, 1, nd, 1)
        if k["counts"] is not None:
            w = torch.where((torch.arange(C_) < torch.tensor(k["counts"])[:, None]).view(1, P, 1, C_), w, torch.zeros((), dtype=F64))
        ref = restate_field_verify(X.view(hist * members, P, nd, C_), x_obs, w, logw, members, True)
        y, obs, prec, lw = k["y"].to(DEV), k["obs"].to(DEV), dev(k["prec"]), dev(logw)
        s = DerivedVerification(decoder(name, "bf16"), P, members, derived, counts=k["counts"], sigma=E2E_SIGMA, fused=True)(y, obs, prec, lw)
        s_c = DerivedVerification(decoder(name, "bf16"), P, members, derived, counts=k["counts"], sigma=E2E_SIGMA, fused=False)(y, obs, prec, lw)
        assert s.crps.dtype == torch.float32 and s.crps.shape == (hist, P, nd, C_) and s.rank.dtype == torch.int32 and s.sums.dtype == F64
        assert s.sums.shape == (hist, nd, 8) and s.hist.shape == (hist, nd, members + 1) and s.status.shape == (hist,)
        for t in (s, s_c):
            assert torch.equal(t.status.cpu().long(), ref["status"]) and torch.equal(t.sums[..., 0].cpu(), ref["sums"][..., 0])
            assert torch.equal(t.hist.sum(2).cpu().double(), ref["sums"][..., 0]) and torch.equal((t.rank == -1).cpu(), w == 0)
        if float(ref["sums"][..., 0].sum()) == 0.0:
            assert all(float(getattr(s, q).abs().max()) == 0.0 for q in FLOATS)
            continue
        e, e_c = e2e_errors(s, ref), e2e_errors(s_c, ref)
        print(f"derived verify {name} members {members} x {hist} counts {cnt} prec {wp}: fused " + " ".join(f"{q} {v:.3e}" for q, v in e.items())
              + "; composed " + " ".join(f"{q} {v:.3e}" for q, v in e_c.items()))
        for q in e:
            assert e[q] <= 2 * e_c[q] + 1e-6, (members, hist, cnt, wp, q, e[q], e_c[q])
            worst[q] = max(worst.get(q, 0.0), e[q])
            worst["composed " + q] = max(worst.get("composed " + q, 0.0), e_c[q])
    print(f"derived verify shape {name} worst: " + " ".join(f"{q} {v:.3e}" for q, v in worst.items()) + " (rule: fused <= 2 composed + 1e-6)")


# ------------------------------------------------------------------------------------------------ 9: a rollout session; the mesh
def test_derived_verification_around_an_analysis_on_a_rollout_session():
    """open_rollout -> fork(n + 1) -> step: the first n members of a history are the ensemble, the last one is the truth (drawn like the members).
    DerivedVerification of the speed (observed="fields": the truth's snapshot of the source fields, a gappy precision map) around a FieldKalman.analyse:
    nothing is read back or uploaded in a warm call, every live derived cell is in a histogram, a derived cell is live only where both sources are, and
    into= adds the two cycles up."""
    from oracle.recipe import recipe_inputs
    from sea_amd.ensemble import DerivedField, DerivedVerification, FieldKalman
    from tests.test_field_enkf_cpu import decode_members
    from tests.test_input_grad_gpu import cfg_of
    from tests.test_model_gpu import build
    from tests.test_rollout_session_gpu import open_on

    c = case("a")
    P, D_, n_mem, B, kk = 4, c["D"], 8, 2, 3
    G, C_ = len(c["groups"]), c["n_inp"]
    F = sum(len(g) for g in c["groups"])
    cfg = cfg_of(1, P * D_, 4, G)
    m = build(cfg, "bf16")
    x, _, ib = recipe_inputs(B, kk + 4, cfg, seed=9)
    dec = decoder("a", "bf16")
    g = torch.Generator().manual_seed(22)
    conds = torch.rand(B * (n_mem + 1), 1, generator=g).to(DEV)
    counts = [C_, C_ - 1, 1, C_]
    y_all = open_on(m, x, ib, kk).fork(n_mem + 1).step(conds)
    E = y_all.shape[-1]
    y = y_all.view(B, n_mem + 1, G, E)[:, :n_mem].reshape(B * n_mem, G, E).contiguous()
    truth = decode_members("a", y_all.view(B, n_mem + 1, G, E)[:, n_mem].detach().cpu().double().reshape(-1, G, P, D_).permute(0, 2, 1, 3))   # [B, P, F, C]
    prec = 0.5 + torch.rand(B, P, F, C_, generator=g)
    prec[torch.rand(B, P, F, C_, generator=g) < 0.2] = 0.0
    obs = (truth + 0.05 * torch.randn(B, P, F, C_, generator=g)).to(torch.float32)
    obs[prec == 0] = float("nan")
    derived = [DerivedField("magnitude", 0, 1, 2.0, 0.5, 2.0, -0.5, name="speed")]
    valid = (torch.arange(C_) < torch.tensor(counts)[:, None]).view(1, P, 1, C_)
    live = ((prec[:, :, 0:1] > 0) & (prec[:, :, 1:2] > 0)) & valid                      # [B, P, 1, C]
    ka = FieldKalman(dec, P, n_mem, counts=counts, fused=True)
    ver = DerivedVerification(dec, P, n_mem, derived, counts=counts, sigma=0.1, fused=True)
    obs_d, prec_d = obs.to(DEV), prec.to(DEV)
    ver(y, obs_d, prec_d)                                                              # the first call on a device uploads the counts and the precision
    ka.transform(y, torch.nan_to_num(obs_d), prec_d)
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        forecast = ver(y, obs_d, prec_d)
        ya = ka.analyse(y, torch.nan_to_num(obs_d), prec_d)
        analysis = ver(ya, obs_d, prec_d)
        infl, crps_f, crps_a = forecast.suggested_inflation, forecast.pooled().mean_crps, analysis.pooled().mean_crps
        total = ver(ya, obs_d, prec_d, into=ver(y, obs_d, prec_d, maps=()), maps=("rank",))
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    print(f"derived verify session: mean crps of the speed, forecast {crps_f.tolist()} analysis {crps_a.tolist()}; suggested inflation {infl.tolist()}")
    assert forecast.sums.shape == (B, 1, 8) and forecast.crps.shape == (B, P, 1, C_) and forecast.status.tolist() == [n_mem] * B
    assert torch.equal(forecast.count.cpu(), live.sum((1, 3)).to(F64)) and torch.equal(forecast.hist.sum(2).cpu(), live.sum((1, 3)))
    assert torch.equal((forecast.rank >= 0).cpu(), live) and not bool(torch.isnan(forecast.crps).any()) and float(forecast.mean.min()) >= 0.0
    assert bool((infl >= 1.0).all()) and bool(torch.isfinite(crps_f).all()) and bool(torch.isfinite(crps_a).all())
    assert total.crps is None and total.rank is not None and torch.equal(total.hist, forecast.hist + analysis.hist)
    assert same_bits(dict(s=total.sums), dict(s=forecast.sums + analysis.sums))
    composed = DerivedVerification(dec, P, n_mem, derived, counts=counts, sigma=0.1, fused=False)(y, obs_d, prec_d)
    assert torch.equal(composed.sums[..., 0], forecast.sums[..., 0]) and rel(forecast.crps.cpu(), composed.crps.cpu()) <= 1e-2


def test_crps_and_spread_maps_of_the_speed_on_the_mesh():
    """unpatch_derived puts the crps and spread maps of the speed (physical units already) on the mesh unchanged, on the 3 x 4 partition of
    tests/golden/unpatch_3x4.npz; the derived field comes from MeshUnpatcher.derived_fields; "BPCF" observations give the same scores."""
    from sea_amd.ensemble import DerivedVerification
    from sea_amd.models.encoder_decoder import Decode
    from sea_amd.utils.data_processors import DataPartitioner2D, MeshUnpatcher, MinMaxScaler
    from tests.conftest import load_golden

    gd = load_golden("unpatch_3x4")
    m, n = (int(v) for v in gd["mn"])
    xy = torch.from_numpy(gd["xy"])
    part = DataPartitioner2D(xy[0], xy[1], m=m, n=n, pad_id=-1, pad_field_value=0, device=DEV)
    idx = torch.from_numpy(gd["index_map"])
    P, C = idx.shape
    groups, D, members, B = [[0, 1]], 16, 8, 2
    sc = MinMaxScaler(feature_range=(-1, 1))
    sc.min_val, sc.max_val = torch.tensor(-1.0), torch.tensor(3.0)
    mu = MeshUnpatcher(part, groups, [sc])
    speed = mu.derived_fields([("magnitude", 0, 1, "speed")])
    torch.manual_seed(14)
    n_inp = (C + 3) // 4 * 4
    dec = Decode(groups, n_inp, 40, D).requires_grad_(False).set_compute_dtype("bf16").to(DEV)
    g = torch.Generator().manual_seed(16)
    y = torch.randn(B * members, 1, P * D, generator=g).to(DEV)
    obs = torch.randn(B, P, 2, n_inp, generator=g).to(DEV)
    counts = (idx >= 0).sum(1).tolist()
    s = DerivedVerification(dec, P, members, speed, counts=counts, sigma=0.2, fused=True)(y, obs)
    s2 = DerivedVerification(dec, P, members, speed, counts=counts, sigma=0.2, layout="BPCF", fused=True)(y, obs.permute(0, 1, 3, 2).contiguous())
    assert same_bits({k: getattr(s, k) for k in OUT}, {k: getattr(s2, k) for k in OUT})
    npts = xy.shape[1]
    crps_m, spread_m = mu.unpatch_derived(s.crps[..., :C].contiguous()), mu.unpatch_derived(s.spread[..., :C].contiguous())
    assert crps_m.shape == (B, npts, 1) and crps_m.dtype == torch.float32
    ref = {q: torch.zeros(B, npts, 1) for q in ("crps", "spread")}
    for p in range(P):
        for c_ in range(C):
            if idx[p, c_] >= 0:
                ref["crps"][:, idx[p, c_], 0] = s.crps.cpu()[:, p, 0, c_]
                ref["spread"][:, idx[p, c_], 0] = s.spread.cpu()[:, p, 0, c_]
    assert torch.equal(crps_m.cpu(), ref["crps"]) and torch.equal(spread_m.cpu(), ref["spread"])
    assert float(crps_m.min()) > 0.0 and float(spread_m.min()) > 0.0                      # every mesh point is a live cell of a continuous ensemble


# ------------------------------------------------------------------------------------------------ 10: the default rule
def test_default_rule(monkeypatch):
    """fused=None follows ensemble.DERIVED_VERIFY_FUSED_MIN_ROWS: None — the composed path everywhere (nothing measured); a row count — the fused launches
    in bf16 up to 128 members with both sources in one group from that many decoder rows (B * members * n_patches) on, the composed path below it, in
    fp32, above 128 members and for sources in different groups."""
    from sea_amd import ensemble, ops
    from sea_amd.ensemble import DerivedField, DerivedVerification

    c = case("a")
    P, G, D_, F, C_ = 64, len(c["groups"]), c["D"], sum(len(g) for g in c["groups"]), c["n_inp"]
    dec = decoder("a", "bf16")
    g = torch.Generator().manual_seed(4)
    obs = torch.randn(1, P, F, C_, generator=g).to(DEV)
    speed = [DerivedField("magnitude", 0, 1)]
    calls = []
    native = ops.decode_derived_verify
    monkeypatch.setattr(ops, "decode_derived_verify", lambda *a, **k: (calls.append(1), native(*a, **k))[1])

    def fused_ran(members, derived=speed, d=dec):
        y = torch.randn(members, G, P * D_, generator=g).to(DEV)
        del calls[:]
        s = DerivedVerification(d, P, members, derived, sigma=3.0)(y, obs)
        assert s.status.tolist() == [members] and (ops.last_form()[0] == "decode.derived_verify") is (len(calls) == 1)
        return len(calls) == 1

    shipped = ensemble.DERIVED_VERIFY_FUSED_MIN_ROWS
    if shipped is None:
        assert fused_ran(64) is False and fused_ran(128) is False             # the shipped default: the composed path at every size
    else:
        assert fused_ran(shipped // P) is True
    monkeypatch.setattr(ensemble, "DERIVED_VERIFY_FUSED_MIN_ROWS", 4096)
    assert fused_ran(64) is True and fused_ran(32) is False                  # either side of the row threshold
    monkeypatch.setattr(ensemble, "DERIVED_VERIFY_FUSED_MIN_ROWS", 2048)
    assert fused_ran(32) is True and fused_ran(16) is False
    assert fused_ran(64, derived=[DerivedField("difference", 0, 2)]) is False  # sources in different groups: composed
    assert fused_ran(64, d=decoder("a", "fp32")) is False
    assert DerivedVerification(dec, P, 32, speed, fused=True).fused is True


# ------------------------------------------------------------------------------------------------ 11: refusals
def test_refusals_leave_the_process_usable():
    from sea_amd import ops
    from sea_amd.ensemble import DerivedField, DerivedVerification

    k = derived_case(5, X_COUNTS[0], True, True)
    before = run(k, 5)
    t = k["t"]
    H, W2, bias = t["H"].to(DEV).to(torch.bfloat16), t["W2"].to(DEV).to(torch.bfloat16), t["bias"].to(DEV)
    two = [dict(H=H, W2=W2[:X_CP], bias=bias[:X_CP]), dict(H=H, W2=W2[X_CP:], bias=bias[X_CP:])]       # the same fields, one per group
    with pytest.raises(RuntimeError, match=r"code -3.*different groups"):
        ops.decode_derived_verify(two, derived3(), k["obs"].to(DEV), X_C, X_CP, X_P, 5)
    with pytest.raises(ValueError, match="two different fields"):
        ops.decode_derived_verify(groups_of(t), [DerivedField("energy", 0, 2)], k["obs"][:, :1].contiguous().to(DEV), X_C, X_CP, X_P, 5)
    with pytest.raises(ValueError, match="1 .. 8"):
        ops.decode_derived_verify(groups_of(t), derived3() * 3, k["obs"].to(DEV), X_C, X_CP, X_P, 5)
    with pytest.raises(ValueError, match="accumulate=True"):
        ops.decode_derived_verify(groups_of(t), derived3(), k["obs"].to(DEV), X_C, X_CP, X_P, 5, accumulate=True)
    assert ops.last_form()[0] == "decode.derived_verify"                     # nothing else was launched in between
    # decoder "b" keeps every field in a group of its own: fused=True raises where the launch refuses, fused=False serves
    c = case("b")
    P, G, D_ = c["P"], len(c["groups"]), c["D"]
    F = sum(len(g) for g in c["groups"])
    dec = decoder("b", "bf16")
    y = torch.randn(4, G, P * D_, generator=torch.Generator().manual_seed(8)).to(DEV).to(torch.bfloat16)
    obs = torch.randn(1, P, F, c["n_inp"], generator=torch.Generator().manual_seed(9)).to(DEV)
    d = [DerivedField("magnitude", 0, 1)]
    with pytest.raises(RuntimeError, match="different groups"):
        DerivedVerification(dec, P, 4, d, fused=True)(y, obs)
    s = DerivedVerification(dec, P, 4, d, fused=False)(y, obs)
    assert s.status.tolist() == [4] and s.sums.shape == (1, 1, 8)
    assert same_bits(run(k, 5), before)
