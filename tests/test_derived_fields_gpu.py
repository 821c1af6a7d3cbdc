"""Quantile, exceedance and Brier maps of DERIVED fields on the device: sea_decode_derived_quantiles / sea_decode_derived_brier through
ops.decode_derived_quantiles / ops.decode_derived_brier, Decode.member_derived_quantiles / member_derived_brier and DerivedQuantiles /
DerivedThresholdVerification end to end and on a rollout session.

Reference: `restate_quantiles` / `restate_field_brier` (tests/test_ensemble_quantiles_cpu.py, tests/test_brier_cpu.py) applied to
`_composed_derived`'s float32 values (tests/test_derived_fields_cpu.py ties that function to a plain float32 loop and numpy's root).
  kernel      on EXACT operands (tests/test_field_verify_gpu.exact_case; dyadic coefficients: the affine steps, the squares and their sums are exact in
              float32): quant EQUAL BITS for all three ops — for the magnitude this is the proof that the root is correctly rounded — with the
              restatement's margin asserted; exceed within 1e-6 (tests/test_ensemble_quantiles_gpu.py's bound); every element written.
  decode      random bf16 operands: the member launch run with ONE member per history hands back every member's decoded f32 values; the derived launch
              equals, bit for bit, the restatement on _composed_derived of those values — in every hidden-width form and for every op (random arguments
              of the root included); difference(a, b) with a zero source b equals the member launch's maps of field a.
  Brier       exact operands with ties at the thresholds (energy, difference): hist, hits, counts and status EQUAL, maps and fp64 sums within
              tests/test_brier_gpu.check_exact's bounds; random operands away from the thresholds: m equal, p within 1e-6, at most 2 % of the cells excluded.
  end to end  bf16 fused and composed against the fp64 restatement: fused error <= 1.5 x composed error."""
import functools

import pytest
import torch

from tests.test_brier_cpu import restate_field_brier
from tests.test_brier_gpu import check_exact as check_brier_exact
from tests.test_brier_gpu import R_B, R_C, R_CP, R_F, R_P
from tests.test_brier_gpu import random_case as brier_random_case
from tests.test_decode_loss_cpu import rel
from tests.test_decode_loss_gpu import DEV, case, decoder
from tests.test_ensemble_quantiles_cpu import restate_quantiles
from tests.test_ensemble_quantiles_gpu import dead_rows_nan, masked, members_first, random_case, weights_of
from tests.test_field_enkf_cpu import field_case, field_cases
from tests.test_field_verify_cpu import field_logw
from tests.test_field_verify_gpu import X_B, X_C, X_COUNTS, X_CP, X_F, X_P, X_S, decode_exact, dev, exact_case
from tests.test_verify_cpu import close
from tests.test_verify_gpu import same_bits

pytestmark = pytest.mark.gpu

F64 = torch.float64
MEMBERS = (1, 2, 17, 64, 65, 128)
LEVELS = (0.0, 0.1, 0.5, 0.9, 1.0)
THR = torch.tensor([[1.5, 2.0, 0.25], [0.375, 0.5, -1.0]])                   # [T, n_derived]: magnitude, energy, difference; values the exact case takes
ND = 3


@functools.lru_cache(maxsize=None)
def derived3(sa=0.5, ha=0.25, sb=0.5, hb=0.25):
    from sea_amd.ensemble import DerivedField

    return (DerivedField("magnitude", 0, 1, sa, ha, sb, hb), DerivedField("energy", 0, 1, sa, ha, sb, hb), DerivedField("difference", 1, 0, sa, ha, sb, hb))


def values(Y, n, derived):
    """float64 exact members [B * n, P, F, C] -> _composed_derived's float32 [B, n, P, n_derived, C]: what the launch compares."""
    from sea_amd.ensemble import _composed_derived

    return _composed_derived(members_first(Y, n), derived)


def groups_of(t, H=None):
    return [dict(H=(t["H"] if H is None else H).to(DEV).to(torch.bfloat16), W2=t["W2"].to(DEV).to(torch.bfloat16), bias=t["bias"].to(DEV))]


def run(t, n, derived=None, levels=LEVELS, thr=THR, w=None, H=None, hist=None, out=None, bias=None):
    """ops.decode_derived_quantiles on an exact case (hist: that history alone)."""
    from sea_amd import ops

    derived = derived3() if derived is None else derived
    H = t["H"] if H is None else H
    if hist is not None:
        H = H[hist * n * X_P:(hist + 1) * n * X_P]
        w = None if w is None else w[hist * n:(hist + 1) * n]
    grp = groups_of(t, H)
    if bias is not None:
        grp[0]["bias"] = bias.to(DEV)
    return ops.decode_derived_quantiles(grp, derived, t["C"], t["Cp"], X_P, n, levels=levels, thr=dev(thr), w=dev(w), counts=t["counts"].to(DEV), out=out)


def prefilled(B, width, nd=ND, levels=LEVELS, thr=THR):
    return dict(quant=torch.full((len(levels), B, X_P, nd, width), float("nan"), device=DEV), exceed=torch.full((thr.shape[0], B, X_P, nd, width), float("nan"), device=DEV))


def check_exact(got, t, n, w, counts, C_, tag, H=None, derived=None):
    """quant equal bits, exceed within the bound, pad and invalid columns exactly 0; returns exceed's error / bound."""
    Y = t["Y"] if H is None else decode_exact(H, t["W2"], t["bias"], None, counts, n, C_, t["Cp"])["Y"]
    ref = restate_quantiles(values(Y, n, derived3() if derived is None else derived), None if w is None else w.view(X_B, n), LEVELS, THR)
    assert ref["margin"] > 1e-12, tag + (ref["margin"],)                    # decided: bit equality does not rest on luck
    q, e = got["quant"].cpu(), got["exceed"].cpu()
    assert not bool(torch.isnan(q).any()) and not bool(torch.isnan(e).any()), tag   # every element was written
    assert float(q[..., C_:].abs().max() if q.shape[-1] > C_ else 0.0) == 0.0 and float(e[..., C_:].abs().max() if e.shape[-1] > C_ else 0.0) == 0.0, tag
    want = masked(ref["quant"], counts, C_)
    for i, name in enumerate(("magnitude", "energy", "difference")):
        assert torch.equal(q[:, :, :, i, :C_], want[:, :, :, i]), tag + (name,)
    ok, ratio = close(e[..., :C_], masked(ref["exceed"], counts, C_), 1e-6)
    assert ok, tag + (ratio,)
    return ratio


# ------------------------------------------------------------------------------------------------ 1: the kernel on exact operands
@pytest.mark.parametrize("n", MEMBERS)
def test_kernel_against_fp64_on_exact_operands(n):
    from sea_amd import ops

    worst, cases = 0.0, 0
    for counts in X_COUNTS:
        t = exact_case(n, counts, False, False)
        for w in (None, weights_of(n)):
            H = None if w is None else dead_rows_nan(t["H"], w, n)
            out = prefilled(X_B, X_C + 5)
            got = run(t, n, w=w, H=H, out=out)
            assert ops.last_form()[:2] == ("decode.derived_quantiles", 128) and all(got[k].data_ptr() == out[k].data_ptr() for k in out)
            worst, cases = max(worst, check_exact(got, t, n, w, counts, X_C, (n, counts, w is None), H=H)), cases + 1
    roots = values(exact_case(n, X_COUNTS[0], False, False)["Y"], n, derived3())[:, :, :, 0].unique().numel()
    print(f"derived quantiles N = {n}: quant equal bits for magnitude ({roots} distinct roots), energy, difference; exceed largest error / bound over {cases} cases "
          f"{worst:.3e} (bound 1e-6)")


# ------------------------------------------------------------------------------------------------ 2, 3: the decode's bits, every form
def member_values(r, H=None):
    """Every member's decoded f32 values, from the MEMBER launch run with one member per history: float32 [B, n, P, F, C] on the host."""
    from sea_amd import ops

    grp = [dict(H=(r["H"] if H is None else H).to(DEV).to(torch.bfloat16), W2=r["W2"].to(DEV).to(torch.bfloat16), bias=r["bias"].to(DEV))]
    q = ops.decode_member_quantiles(grp, r["C"], r["Cp"], r["P"], 1, levels=(0.5,))["quant"][0]           # [B n, P, F, C]
    return q.cpu().view(r["B"], r["n"], r["P"], r["F"], r["C"])


@pytest.mark.parametrize("S", [40, 640])
def test_a_zero_source_gives_the_member_launch_bits(S):
    from sea_amd import ops
    from sea_amd.ensemble import DerivedField

    r = dict(random_case(S))
    W2, bias = r["W2"].clone(), r["bias"].clone()
    W2.view(r["F"], r["Cp"], S)[1] = 0.0
    bias.view(r["F"], r["Cp"])[1] = 0.0
    r.update(W2=W2, bias=bias)
    n, B = r["n"], r["B"]
    w = torch.tensor([0.5, 0.2, 0.3, 0.25, 0.0, 0.75])
    levels, thr = (0.0, 0.4, 0.6, 1.0), torch.tensor([[0.0, 0.1]])
    grp = [dict(H=r["H"].to(DEV).to(torch.bfloat16), W2=W2.to(DEV).to(torch.bfloat16), bias=bias.to(DEV))]
    want = ops.decode_member_quantiles(grp, r["C"], r["Cp"], r["P"], n, levels=levels, thr=thr.to(DEV), w=w.to(DEV))
    got = ops.decode_derived_quantiles(grp, [DerivedField("difference", 0, 1)], r["C"], r["Cp"], r["P"], n, levels=levels, thr=thr[:, :1].contiguous().to(DEV), w=w.to(DEV))
    assert torch.equal(got["quant"][:, :, :, 0], want["quant"][:, :, :, 0]) and torch.equal(got["exceed"][:, :, :, 0], want["exceed"][:, :, :, 0]), S


@pytest.mark.parametrize("S", [72, 128, 256, 384, 512, 640])
def test_every_hidden_width_form(S):
    """Each SP the dispatcher instantiates at its widest S (and S = 72, no multiple of 32), random bf16-exact operands, coefficients that are not dyadic:
    the maps equal the restatement on _composed_derived of the member launch's own decoded values, bit for bit."""
    from sea_amd import ops
    from sea_amd.ensemble import _composed_derived

    r = random_case(S)
    n, B = r["n"], r["B"]
    derived = derived3(1.5, -0.25, 0.75, 0.5)
    w = torch.tensor([0.5, 0.2, 0.3, 0.25, 0.0, 0.75])
    levels = (0.0, 0.4, 0.6, 1.0)
    thr = torch.tensor([[0.9, 0.4, 0.3]])
    X = _composed_derived(member_values(r), derived)
    ref = restate_quantiles(X, w.view(B, n), levels, thr)
    assert ref["margin"] > 1e-12
    out = dict(quant=torch.full((4, B, r["P"], ND, r["C"]), float("nan"), device=DEV), exceed=torch.full((1, B, r["P"], ND, r["C"]), float("nan"), device=DEV))
    grp = [dict(H=r["H"].to(DEV).to(torch.bfloat16), W2=r["W2"].to(DEV).to(torch.bfloat16), bias=r["bias"].to(DEV))]
    got = ops.decode_derived_quantiles(grp, derived, r["C"], r["Cp"], r["P"], n, levels=levels, thr=thr.to(DEV), w=w.to(DEV), out=out)
    assert ops.last_form()[:2] == ("decode.derived_quantiles", 128 * ((S + 127) // 128))
    for i, d in enumerate(derived):
        assert torch.equal(got["quant"].cpu()[:, :, :, i], ref["quant"][:, :, :, i]), (S, d.op)
    near = ((X.double() - thr[0].view(1, 1, 1, ND, 1).double()).abs() < 1e-4).any(1)
    ok, ratio = close(got["exceed"].cpu()[0][~near], ref["exceed"][0][~near], 1e-6)
    assert ok, (S, ratio)
    print(f"derived quantiles form S = {S}: quant equal bits against the member launch's values for all three ops; exceed error / bound {ratio:.3e}")


def test_a_field_wider_than_one_chunk_of_tiles():
    """530 columns in 544 are 17 tiles: a workgroup reads out 16, so a derived field has two chunks; counts 513 leave the second chunk ONE valid column."""
    n, C_, Cp = 5, 530, 544
    w = weights_of(n)
    for counts in ((C_, 513), (512, 513)):
        t = exact_case(n, counts, False, False, C_, Cp)
        H = dead_rows_nan(t["H"], w, n)
        got = run(t, n, w=w, H=H, out=prefilled(X_B, C_ + 3))
        ratio = check_exact(got, t, n, w, counts, C_, (counts,), H=H)
        alone = run(t, n, w=w, H=H, hist=1)
        assert torch.equal(alone["quant"][:, 0], got["quant"][:, 1, ..., :C_]) and torch.equal(alone["exceed"][:, 0], got["exceed"][:, 1, ..., :C_])
        print(f"derived quantiles chunks counts {counts}: quant equal bits; exceed error / bound {ratio:.3e}")


@pytest.mark.parametrize("n", [5, 128])
def test_special_calls_and_cells(n):
    t = exact_case(n, X_COUNTS[0], False, False)
    w = weights_of(n)
    want = run(t, n, w=w)
    only_t, only_q = run(t, n, levels=(), w=w), run(t, n, thr=None, w=w)   # a thresholds-only and a levels-only call
    assert only_t["quant"] is None and only_q["exceed"] is None
    assert torch.equal(only_t["exceed"], want["exceed"]) and torch.equal(only_q["quant"], want["quant"])
    valid = (torch.arange(X_C) < t["counts"][:, None]).view(1, X_P, 1, X_C).expand(X_B, X_P, ND, X_C)
    thr = THR.clone()
    thr[1, 0] = float("nan")                                               # a NaN threshold: NaN in that map's live cells of that derived field, and only there
    e = run(t, n, thr=thr, w=w)["exceed"].cpu()
    mark = torch.zeros(2, X_B, X_P, ND, X_C, dtype=torch.bool)
    mark[1, :, :, 0] = valid[:, :, 0]
    assert torch.equal(torch.isnan(e), mark) and torch.equal(e[~mark], want["exceed"].cpu()[~mark])
    w0 = w.clone()
    w0[:n] = 0.0                                                           # history 0 without a live member: zeros
    z = run(t, n, w=w0)
    assert float(z["quant"][:, 0].abs().max()) == 0.0 and float(z["exceed"][:, 0].abs().max()) == 0.0
    assert torch.equal(z["quant"][:, 1], want["quant"][:, 1]) and torch.equal(z["exceed"][:, 1], want["exceed"][:, 1])
    # a source value whose SQUARE overflows (2^100 in field 0, column 3): magnitude and energy are NaN in that column's live cells, the difference is finite
    bias = t["bias"].clone()
    bias.view(X_F, X_CP)[0, 3] = 2.0 ** 100
    got = run(t, n, w=w, bias=bias)
    for k in ("quant", "exceed"):
        nan = torch.isnan(got[k].cpu())
        mark = torch.zeros_like(nan)
        mark[:, :, :, :2, 3] = valid[:, :, :2, 3]
        assert torch.equal(nan, mark), (n, k)
        keep = ~mark
        keep[..., 2, 3] = False                                            # the difference at that column is finite, and another number
        assert torch.equal(got[k].cpu()[keep], want[k].cpu()[keep]), (n, k)
    assert bool(torch.isfinite(got["quant"][..., 2, 3]).all()) and float(got["quant"][:, :, 0, 2, 3].max()) < -2.0 ** 98
    # NaN in a hidden row of a live member: exactly the cells of that (history, patch), in every derived field
    j, p = (1 + 2) % n, 1
    assert float(w[n + j]) > 0
    H = t["H"].clone()
    H[(n + j) * X_P + p] = float("nan")
    got = run(t, n, w=w, H=H)
    for k in ("quant", "exceed"):
        nan = torch.isnan(got[k].cpu())
        mark = torch.zeros_like(nan)
        mark[:, 1, p, :, :int(t["counts"][p])] = True
        assert torch.equal(nan, mark) and torch.equal(got[k].cpu()[~mark], want[k].cpu()[~mark]), (n, k)


# ------------------------------------------------------------------------------------------------ 4: bits
@pytest.mark.parametrize("n", [5, 64, 128])
def test_two_runs_a_history_alone_and_the_company_of_other_derived_fields(n):
    t = exact_case(n, X_COUNTS[0], False, False)
    w = weights_of(n)
    want = run(t, n, w=w)
    again = run(t, n, w=w)
    assert torch.equal(again["quant"], want["quant"]) and torch.equal(again["exceed"], want["exceed"])
    for h in range(X_B):
        alone = run(t, n, w=w, hist=h)
        assert torch.equal(alone["quant"][:, 0], want["quant"][:, h]) and torch.equal(alone["exceed"][:, 0], want["exceed"][:, h]), (n, h)
    for order in ((0,), (2, 1, 0), (1, 1, 2, 0, 0, 1, 2, 0)):               # alone, reversed, and a full table of eight
        d = tuple(derived3()[i] for i in order)
        got = run(t, n, derived=d, thr=THR[:, list(order)].contiguous(), w=w)
        for slot, i in enumerate(order):
            assert torch.equal(got["quant"][:, :, :, slot], want["quant"][:, :, :, i]) and torch.equal(got["exceed"][:, :, :, slot], want["exceed"][:, :, :, i]), (n, order, slot)


# ------------------------------------------------------------------------------------------------ 5: Brier on exact operands, ties at the thresholds
BRIER_D = (1, 2)                                                           # energy and difference: a tie is exact


def brier_case(n, counts, wp, wl):
    """The exact case with its observation and precision brought to the derived fields (energy, difference): dict(t, derived, X [B n, P, 2, C] float32,
    obs [B P, 2, C], prec [B P, 2, C] or None, w [B, P, 2, C] float64, thr [3, 2] taken from the members' and the readings' own values: ties occur)."""
    from sea_amd.ensemble import _composed_derived

    t = exact_case(n, counts, wp, wl)
    derived = tuple(derived3()[i] for i in BRIER_D)
    X = values(t["Y"], n, derived)                                         # [B, n, P, 2, C]
    obs = _composed_derived(t["obs"].view(X_B, X_P, X_F, X_C), derived).view(X_B * X_P, 2, X_C)
    prec = w = None
    on = torch.ones(X_B, X_P, X_F, X_C) if t["prec"] is None else (t["prec"].view(X_B, X_P, X_F, X_C) > 0).float()
    pd = torch.stack([on[:, :, d.a] * on[:, :, d.b] for d in derived], dim=2)
    if t["prec"] is not None:
        prec = pd.view(X_B * X_P, 2, X_C).contiguous()
    w = torch.where((torch.arange(X_C) < torch.tensor(counts)[:, None]).view(1, X_P, 1, X_C), pd.double(), torch.zeros((), dtype=F64))
    o_live = torch.nan_to_num(obs, nan=0.5)
    thr = torch.stack([X[0, 0, 0, :, 0], o_live[0, :, 1], X[1, n - 1, 1, :, 2]]).contiguous()        # [3, 2]
    return dict(t=t, derived=derived, X=X.view(X_B * n, X_P, 2, X_C), obs=obs, prec=prec, w=w, thr=thr)


def run_brier(k, n, out=None, accumulate=False, maps=("prob", "brier"), logw="case"):
    from sea_amd import ops

    t = k["t"]
    logw = t["logw"] if isinstance(logw, str) else logw
    return ops.decode_derived_brier(groups_of(t), k["derived"], k["obs"].to(DEV), X_C, X_CP, X_P, n, k["thr"].to(DEV), prec=dev(k["prec"]), counts=t["counts"].to(DEV),
                                    logw=dev(logw), accumulate=accumulate, maps=maps, out=out)


@pytest.mark.parametrize("n", MEMBERS)
def test_brier_against_fp64_on_exact_operands_with_ties(n):
    from sea_amd import ops

    worst32, worst64, ties = 0.0, 0.0, 0
    for counts in X_COUNTS:
        for wp, wl in ((False, False), (True, True)):
            k = brier_case(n, counts, wp, wl)
            ref = restate_field_brier(k["X"], k["obs"].view(X_B, X_P, 2, X_C), k["w"], k["t"]["logw"], n, k["thr"])
            out = {m: torch.full((3, X_B, X_P, 2, X_C + 3), float("nan"), device=DEV) for m in ("prob", "brier")}
            got = run_brier(k, n, out=out)
            assert ops.last_form()[:2] == ("decode.derived_brier", 128) and all(got[m].data_ptr() == out[m].data_ptr() for m in out)
            assert all(float(got[m][..., X_C:].abs().max()) == 0.0 for m in out)
            a, b = check_brier_exact({m: v[..., :X_C] if m in out else v for m, v in got.items()}, ref, (n, counts, wp, wl))
            worst32, worst64 = max(worst32, a), max(worst64, b)
            tf = k["thr"].view(3, 1, 1, 2, 1)
            live = (k["w"] > 0).unsqueeze(0)
            ties += int(((k["obs"].view(X_B, X_P, 2, X_C).unsqueeze(0) == tf) & live).sum()) + int((k["X"].view(X_B, n, X_P, 2, X_C)[:, 0].unsqueeze(0) == tf).sum())
            if not wp:                                                     # equal weights: the prob map has the bits of the derived quantile launch's exceed map
                e = run(k["t"], n, derived=k["derived"], levels=(), thr=k["thr"])["exceed"]
                assert torch.equal(run_brier(k, n, logw=None)["prob"], e), (n, counts)
                first = run_brier(k, n, maps=())
                assert "prob" not in first
                twice = run_brier(k, n, maps=(), out=dict(sums=first["sums"].clone(), hist=first["hist"].clone(), hits=first["hits"].clone()), accumulate=True)
                assert torch.equal(twice["hist"], 2 * first["hist"]) and torch.equal(twice["hits"], 2 * first["hits"]) and same_bits(dict(s=twice["sums"]), dict(s=2 * first["sums"]))
    assert ties > 0                                                        # x == thr and y == thr occur: strictness is tested
    print(f"derived brier N = {n}: hist, hits, counts, status equal ({ties} ties); largest error / bound: f32 maps {worst32:.3e} (bound 1e-6), fp64 sums {worst64:.3e}")


# ------------------------------------------------------------------------------------------------ 6: random bf16 operands away from the thresholds
R_COEFF = (1.5, -0.25, 0.75, 0.5)
R_THR = torch.tensor([[0.45, 0.15, -1.55], [1.15, 0.65, -0.65], [2.05, 2.05, 0.35]])       # [T, n_derived]: magnitude, energy, difference


def derived64(Y, g, derived):
    """The derived values of fp64 decoded members Y [.., F, C] in fp64, and the band around them: the decode's band g (tests/test_brier_gpu.py: a bound with a
    factor 4 in hand) propagated through the op — first order, and the squares' second-order terms, so it stays a bound — plus the op's own float32
    roundings (each 2^-24 relative of the value it rounds)."""
    eps = 2.0 ** -24
    xs, bands = [], []
    for d in derived:
        ya, yb, ga, gb = Y.select(-2, d.a), Y.select(-2, d.b), g.select(-2, d.a), g.select(-2, d.b)
        a, b = ya * d.scale_a + d.shift_a, yb * d.scale_b + d.shift_b
        da = abs(d.scale_a) * ga + eps * ((ya * d.scale_a).abs() + a.abs())
        db = abs(d.scale_b) * gb + eps * ((yb * d.scale_b).abs() + b.abs())
        if d.op == "difference":
            x = a - b
            dx = da + db + eps * x.abs()
        else:
            q = a * a + b * b
            dq = 2 * a.abs() * da + 2 * b.abs() * db + da * da + db * db + 2 * eps * q
            x, dx = (0.5 * q, 0.5 * dq + eps * 0.5 * q) if d.op == "energy" else (q.sqrt(), dq / (2 * q.sqrt()) + eps * q.sqrt())
        xs.append(x), bands.append(dx)
    return torch.stack(xs, -2), torch.stack(bands, -2)


@pytest.mark.parametrize("n,wl", [(5, False), (17, True), (64, False), (65, True), (128, False)])
def test_random_operands_away_from_the_thresholds(n, wl):
    from sea_amd import ops
    from sea_amd.ensemble import _composed_derived

    k = brier_random_case(n, wl)
    derived = derived3(*R_COEFF)
    derived = (derived[0], derived[1], type(derived[2])("difference", 0, 1, *R_COEFF))
    B, P, C_, T = R_B, R_P, R_C, R_THR.shape[0]
    X, band = derived64(k["Y"], k["g"], derived)                           # [B n, P, 3, C]
    obs = _composed_derived(k["obs"].view(B, P, R_F, C_), derived)         # [B, P, 3, C]
    ref = restate_field_brier(X, obs.double(), torch.ones(B, P, ND, C_, dtype=F64), k["logw"], n, R_THR)
    alive = torch.ones(B, n, dtype=torch.bool) if k["logw"] is None else (k["logw"].view(B, n) != float("-inf"))
    near = ((X.unsqueeze(0) - R_THR.to(F64).view(T, 1, 1, ND, 1)).abs() <= band.unsqueeze(0)).view(T, B, n, P, ND, C_)
    excluded = (near & alive.view(1, B, n, 1, 1, 1)).any(2)                # [T, B, P, 3, C]: from the restatement alone, before the device is touched
    share = float(excluded.double().mean())
    print(f"derived brier random N = {n}: excluded share {share:.4%} (band <= {float(band.max()):.2e})")
    assert share <= 0.02
    grp = [dict(H=k["H"].to(DEV), W2=k["W2"].to(DEV), bias=k["bias"].to(DEV))]
    got = {kk: v.cpu() for kk, v in ops.decode_derived_brier(grp, derived, obs.view(B * P, ND, C_).to(DEV), C_, R_CP, P, n, R_THR.to(DEV), logw=dev(k["logw"])).items()}
    keep = ~excluded
    err = float((got["prob"].to(F64) - ref["prob"])[keep].abs().max())
    assert err <= 1e-6, err
    if not wl:                                                             # equal weights: p = m / L, so m is read from the map
        assert torch.equal((got["prob"].to(F64) * n).round().long()[keep], ref["m"][keep])
    print(f"derived brier random N = {n}: p error {err:.3e} (bound 1e-6) on the kept cells, m equal")


# ------------------------------------------------------------------------------------------------ 7: refusals
def test_refusals_leave_the_process_usable(monkeypatch):
    from sea_amd import ensemble, ops
    from sea_amd.ensemble import DerivedField, DerivedQuantiles

    t = exact_case(5, X_COUNTS[0], False, False)
    before = run(t, 5)
    H, W2, bias = t["H"].to(DEV).to(torch.bfloat16), t["W2"].to(DEV).to(torch.bfloat16), t["bias"].to(DEV)
    two = [dict(H=H, W2=W2[:X_CP], bias=bias[:X_CP]), dict(H=H, W2=W2[X_CP:], bias=bias[X_CP:])]       # the same fields, one per group
    with pytest.raises(RuntimeError, match=r"code -3.*different groups"):
        ops.decode_derived_quantiles(two, derived3(), X_C, X_CP, X_P, 5, levels=(0.5,))
    with pytest.raises(RuntimeError, match=r"code -3.*different groups"):
        ops.decode_derived_brier(two, derived3()[:1], torch.zeros(X_B * X_P, 1, X_C, device=DEV), X_C, X_CP, X_P, 5, torch.zeros(1, 1, device=DEV))
    with pytest.raises(ValueError, match="two different fields"):
        ops.decode_derived_quantiles(groups_of(t), [DerivedField("energy", 0, 2)], X_C, X_CP, X_P, 5, levels=(0.5,))
    with pytest.raises(ValueError, match="1 .. 8"):
        ops.decode_derived_quantiles(groups_of(t), derived3() * 3, X_C, X_CP, X_P, 5, levels=(0.5,))
    assert ops.last_form()[0] == "decode.derived_quantiles"                 # nothing else was launched in between
    # the classes: decoder "b" keeps every field in a group of its own — fused=None composes, fused=True raises; "a" holds 0 and 1 in one group
    monkeypatch.setattr(ensemble, "DERIVED_FUSED_MIN_ROWS", 0)
    g = torch.Generator().manual_seed(8)
    for name, fused in (("b", False), ("a", True)):
        c = case(name)
        P, G, D_ = c["P"], len(c["groups"]), c["D"]
        dec = decoder(name, "bf16")
        y = torch.randn(4, G, P * D_, generator=g).to(DEV).to(torch.bfloat16)
        d = [DerivedField("magnitude", 0, 1)]
        q, e = DerivedQuantiles(dec, P, 4, d, levels=(0.5,))(y)
        assert (ops.last_form()[0] == "decode.derived_quantiles") is fused and e is None and q.shape == (1, 1, P, 1, c["n_inp"])
        if not fused:
            with pytest.raises(RuntimeError, match="different groups"):
                DerivedQuantiles(dec, P, 4, d, levels=(0.5,), fused=True)(y)
        q2, _ = DerivedQuantiles(dec, P, 4, d, levels=(0.5,), fused=False)(y)
        assert rel(q.cpu(), q2.cpu()) <= 1e-2
    after = run(t, 5)
    assert torch.equal(after["quant"], before["quant"]) and torch.equal(after["exceed"], before["exceed"])


# ------------------------------------------------------------------------------------------------ 8: end to end
CASES = [c for c in field_cases() if not c[4]]
BY_SHAPE = {name: [c for c in CASES if c[0] == name] for name in ("a", "c")}
E2E_LEVELS = (0.05, 0.5, 0.95)


@pytest.mark.parametrize("name", ["a", "c"])
def test_derived_quantiles_bf16_against_fp64(name):
    """Decoders "a" (fields [[0, 1], [2]]) and "c" (fields [[0, 1]], hidden 624); "b" keeps every field in its own group and is the composed path's
    (test_refusals_leave_the_process_usable)."""
    from sea_amd.ensemble import DerivedField, DerivedQuantiles, normalised_weights

    derived = (DerivedField("magnitude", 0, 1, *R_COEFF), DerivedField("difference", 1, 0, *R_COEFF))
    P = case(name)["P"]
    worst = 0.0
    for case_ in BY_SHAPE[name]:
        _, members, hist, cnt, wp, local = case_
        k = field_case(*case_)
        logw = torch.randn(hist * members, generator=torch.Generator().manual_seed(66 + members + hist)) if members % 2 else None
        w = None if logw is None else normalised_weights(logw, members).view(hist, members)
        F, C_ = k["obs"].shape[2:]
        X, _ = derived64(k["Y"].view(hist, members, P, F, C_), torch.zeros(hist, members, P, F, C_, dtype=F64), derived)
        ref = restate_quantiles(X, w, E2E_LEVELS, None)["quant"]
        if k["counts"] is not None:
            ref = masked(ref, k["counts"], C_)
        if float(ref.abs().max()) == 0.0:
            continue
        y, lw = k["y"].to(DEV), dev(logw)
        thr = [1.0]
        q, e_map = DerivedQuantiles(decoder(name, "bf16"), P, members, derived, levels=E2E_LEVELS, thresholds=thr, counts=k["counts"], fused=True)(y, lw)
        q_c, e_c_map = DerivedQuantiles(decoder(name, "bf16"), P, members, derived, levels=E2E_LEVELS, thresholds=thr, counts=k["counts"], fused=False)(y, lw)
        assert q.dtype == torch.float32 and q.shape == (3, hist, P, 2, C_) and e_map.shape == (1, hist, P, 2, C_) and q_c.shape == q.shape and e_c_map.shape == e_map.shape
        assert bool((q[1:] >= q[:-1]).all()) and float(e_map.min()) >= 0.0 and float(e_map.max()) <= 1.0 + 1e-6 and float(q[:, :, :, 0].min()) >= 0.0
        e, e_c = rel(q.cpu().double(), ref), rel(q_c.cpu().double(), ref)
        print(f"derived quantiles {name} members {members} x {hist} counts {cnt}: fused {e:.3e} composed {e_c:.3e} ratio {e / e_c:.2f} (bound 1.5)")
        assert e <= 1.5 * e_c, (members, hist, cnt, e, e_c)
        worst = max(worst, e / e_c)
    print(f"derived quantiles shape {name} worst fused / composed error ratio {worst:.2f} (bound 1.5)")


def test_derived_products_on_a_rollout_session_and_on_the_mesh():
    """open_rollout -> fork(n) -> step -> DerivedQuantiles(levels=(0, 0.5, 1)) and DerivedThresholdVerification against a snapshot of the source fields;
    the speed's maps are non-negative and ordered, a forecast verified against one of its own members is never worse than climatology by construction of
    the counts (hist sums to the live cells)."""
    from oracle.recipe import recipe_inputs
    from sea_amd.ensemble import DerivedField, DerivedQuantiles, DerivedThresholdVerification, EnsembleFields
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
    conds = torch.rand(B * n_mem, 1, generator=g).to(DEV)
    counts = [C_, C_ - 1, 1, C_]
    y = open_on(m, x, ib, kk).fork(n_mem).step(conds)
    derived = [DerivedField("magnitude", 0, 1, 2.0, 0.5, 2.0, -0.5, name="speed")]
    q, e = DerivedQuantiles(dec, P, n_mem, derived, levels=(0, 0.5, 1), thresholds=[1.0], counts=counts, fused=True)(y)
    assert q.shape == (3, B, P, 1, C_) and e.shape == (1, B, P, 1, C_) and not bool(torch.isnan(q).any())
    assert bool((q[0] <= q[1]).all()) and bool((q[1] <= q[2]).all()) and float(q.min()) >= 0.0
    mean, _ = EnsembleFields(dec, P, n_mem, counts=counts, fused=True)(y)                  # [B, P, F, C]: a snapshot of the source fields
    ver = DerivedThresholdVerification(dec, P, n_mem, derived, [1.0], counts=counts, fused=True)
    s = ver(y, mean.float().contiguous(), maps=("prob",))
    s_c = DerivedThresholdVerification(dec, P, n_mem, derived, [1.0], counts=counts, fused=False)(y, mean.float().contiguous(), maps=("prob",))
    live = sum(counts)
    assert tuple(s.sums.shape) == (B, 1, 1, 5) and torch.equal(s.hist.sum(-1), torch.full((B, 1, 1), live, device=DEV)) and torch.equal(s.sums[..., 0], s_c.sums[..., 0])
    assert torch.equal(s.prob, e)                                           # equal weights: the Brier launch's prob map has the exceed map's bits
    assert float((s.prob - s_c.prob).abs().max()) <= 1.0 / n_mem + 1e-6      # two bf16 paths: a member next to the threshold may fall on either side
    print(f"derived session: speed envelope width mean {float((q[2] - q[0]).mean()):.3e}; brier fused {float(s.brier.mean()):.4f} composed {float(s_c.brier.mean()):.4f}")


def test_unpatch_derived_round_trips_a_map_with_another_field_count():
    """unpatch_derived puts [T, P, n_derived, C] maps on the mesh unchanged, with n_derived (1 and 3) different from the mesh's 2 fields, on the 3 x 4
    partition of tests/golden/unpatch_3x4.npz; "BPCF" gives the same mesh values."""
    from sea_amd.utils.data_processors import DataPartitioner2D, MeshUnpatcher, MinMaxScaler
    from tests.conftest import load_golden

    gd = load_golden("unpatch_3x4")
    m, n = (int(v) for v in gd["mn"])
    xy = torch.from_numpy(gd["xy"])
    part = DataPartitioner2D(xy[0], xy[1], m=m, n=n, pad_id=-1, pad_field_value=0, device=DEV)
    idx = torch.from_numpy(gd["index_map"])
    P, C = idx.shape
    scalers = []
    for rng_, lo, hi in (((-1, 1), -1.0, 3.0), ((1, -1), 0.5, 2.0)):
        sc = MinMaxScaler(feature_range=rng_)
        sc.min_val, sc.max_val = torch.tensor(lo), torch.tensor(hi)
        scalers.append(sc)
    mu = MeshUnpatcher(part, [[0], [1]], scalers)
    npts = xy.shape[1]
    g = torch.Generator().manual_seed(3)
    for nd in (1, 3):
        v = torch.randn(2, P, nd, C, generator=g)
        got = mu.unpatch_derived(v.to(DEV))
        ref = torch.zeros(2, npts, nd)
        for p in range(P):
            for c_ in range(C):
                if idx[p, c_] >= 0:
                    ref[:, idx[p, c_]] = v[:, p, :, c_]
        assert got.shape == (2, npts, nd) and got.dtype == torch.float32 and torch.equal(got.cpu(), ref), nd   # unchanged: scale 1, shift 0
        assert torch.equal(mu.unpatch_derived(v.permute(0, 1, 3, 2).contiguous().to(DEV), layout="BPCF"), got)
    speed, = mu.derived_fields([("magnitude", 0, 1)])
    assert (speed.scale_a, speed.shift_a) == tuple(float(torch.tensor(c, dtype=torch.float32)) for c in scalers[0].inverse_affine())
