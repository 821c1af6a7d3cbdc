"""What tests/test_bwd_rows_gpu.py rests on, checked without a GPU: its fp64 references equal fp64 autograd of the layer formulas, its emulation restates them with
the roundings off, its LOCAL / EPS constants are not below what it measures, the reference rows of its cases spread by at most 3, and a reference that is wrong
in one row (or in one row of one column) fails the local (per-column) check while passing the global one that tests/test_bwd_ops_gpu.py applies."""
import math

import pytest
import torch

from tests import test_bwd_rows_gpu as R
from tests.test_forced_forms_gpu import BF, rel, rowerr, spread

F32 = torch.float32
SMALL = dict(M=5, d=68)


def close(a, b, tol):
    return float((a - b).norm()) <= tol * max(float(b.norm()), 1.0)


@pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("pattern", list(R.PATTERNS))
def test_norm_reference_equals_autograd(pattern, dtype):
    gelu = R.PATTERNS[pattern][2]
    d = SMALL["d"]
    for g in R.norm_operands(pattern, dtype, SMALL["M"], d, device="cpu"):
        ref = R.norm_bwd_formula(g, gelu, exact_stats=True)
        x = g["x"].double().requires_grad_(True)
        gamma = g["gamma"].double().requires_grad_(True)
        beta = (g["beta"].double() if g["beta"] is not None else torch.zeros(d, dtype=torch.float64)).requires_grad_(True)
        mod = (g["mod"].double() if g["mod"] is not None else torch.zeros(SMALL["M"], 2 * d, dtype=torch.float64)).requires_grad_(True)
        mu = x.mean(-1, keepdim=True)
        xh = (x - mu) / torch.sqrt(((x - mu) ** 2).mean(-1, keepdim=True) + 1e-5)
        y = xh * (gamma + ((1 + mod[:, :d]) if g["mod"] is not None else 0.0)) + (beta + mod[:, d:])
        if gelu:
            y = torch.nn.functional.gelu(y)
        y.backward(g["dy"].double())
        old = g["old"].double() if g["old"] is not None else 0.0
        assert close(ref["dX32"] - old, x.grad, 1e-10)
        assert close(ref["tg"].sum(0), gamma.grad, 1e-10) and close(ref["tb"].sum(0), beta.grad, 1e-10)
        if g["mod"] is not None:
            assert close(ref["dmod"], mod.grad, 1e-10)


@pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])
def test_silu_reference_equals_autograd(dtype):
    su = R.silu_operands(5, (260, 4), dtype, device="cpu")
    for g in su["groups"]:
        tw, tb, _ = R.silu_bwd_formula(su["c"], g)
        w1, b1 = g["w1"].double().requires_grad_(True), g["b1"].double().requires_grad_(True)
        torch.nn.functional.silu(su["c"].double()[:, None] * w1 + b1).backward(g["dH"].double())
        assert close(tw.sum(0), w1.grad, 1e-10) and close(tb.sum(0), b1.grad, 1e-10)


@pytest.mark.parametrize("mode,h,E,dropout", [(0, 8, 260, False), (0, 8, 260, True), (0, 1, 8, True), (0, 64, 8, False), (1, 0, 264, False)])
def test_ib_reference_equals_autograd(mode, h, E, dropout):
    g = R.ib_operands(mode, h, E, 5, 3, device="cpu")
    gen = torch.Generator().manual_seed(5)
    masks = [(torch.rand(5, E, generator=gen) > 0.1).double() * (256.0 / 230.0) for _ in range(3)] if dropout else None
    ref = R.ib_reference(g, masks)
    c = g["c"].double()[:, None]
    if mode == 0:
        ps = {k: g[k].double().requires_grad_(True) for k in ("w1", "b1", "lnw", "lnb", "w2")}
        ps["b2"] = torch.zeros(E, dtype=torch.float64, requires_grad=True)
        hid = torch.nn.functional.gelu(torch.nn.functional.layer_norm(c * ps["w1"] + ps["b1"], (h,), ps["lnw"], ps["lnb"], 1e-5))
        ib = hid @ ps["w2"].t() + ps["b2"]
        names = dict(dw1="w1", db1="b1", dlnw="lnw", dlnb="lnb", dw2="w2", db2="b2")
    else:
        ps = dict(w1=torch.zeros(E, dtype=torch.float64, requires_grad=True), b1=torch.zeros(E, dtype=torch.float64, requires_grad=True))
        ib = c * ps["w1"] + ps["b1"]
        names = dict(dw1="w1", db1="b1")
    sum((x.double() * (m if m is not None else 1.0) * ib).sum() for x, m in zip(g["dX"], masks if masks else [None] * 3)).backward()
    for k, p in names.items():
        s, a, n, extra = ref[k]
        assert close(s, ps[p].grad, 1e-10), k
        assert bool((a >= s.abs() * (1 - 1e-12)).all()) and (extra is None or bool((extra >= 0).all())), k


def _cheap(cases):
    return [c for c in cases if c[3] <= 68]


def test_emulation_restates_the_reference_and_local_is_not_below_the_measurement():
    """measure_local asserts the 1e-12; the worst case of every kind lies at d <= 68 (the comments of LOCAL), so the cheap subset reproduces the constants."""
    worst = R.measure_local(verbose=False, cases=_cheap(R.norm_cases()))
    assert set(worst) == set(R.LOCAL)
    for kind, (v, what) in worst.items():
        assert v > 0, kind
        assert R.LOCAL[kind] / 3 >= v * (1 - 1e-3), (kind, v, what)
        assert R.LOCAL[kind] / 3 <= v * 1.01, (kind, v, what)


def test_emulation_restates_the_reference_at_the_wide_forms():
    cases = [("ln_gelu", BF, 5, 2056, None), ("adaln02", BF, 5, 2052, None), ("final", BF, R.EIGHT["M"], R.EIGHT["d"], R.EIGHT["n"])]
    assert set(cases) <= set(R.norm_cases())
    worst = R.measure_local(verbose=False, cases=cases)
    assert all(worst[k][0] < R.LOCAL[k] / 3 for k in ("dXact", "dXact.gelu", "dmod"))


def test_recorded_approximation_errors():
    ep, ee = R.measure_eps()
    assert ep <= R.EPS_POLY <= 1.01 * ep and ee <= R.EPS_ERF <= 1.01 * ee
    u = torch.linspace(-6, 6, 2001, dtype=torch.float64)
    assert float((R.gelu_grad64(u) - torch.autograd.functional.jvp(torch.nn.functional.gelu, u, torch.ones_like(u))[1]).abs().max()) < 1e-14
    assert float((0.5 * u * (1 + R.erf_as(u)) - torch.nn.functional.gelu(u)).abs().max()) <= 0.5 * 6 * R.EPS_ERF


def test_reference_rows_spread_by_at_most_three():
    for pattern, dtype, M, d, n in R.norm_cases():
        if d > 2056:
            continue
        for g in R.norm_operands(pattern, dtype, M, d, n, device="cpu"):
            ref = R.norm_bwd_formula(g, R.PATTERNS[pattern][2])
            assert spread(ref["dX32"]) <= 3.0 and spread(ref["dmod"]) <= 3.0, (pattern, dtype, M, d)


def test_norm_form_rule():
    """The restated launcher rule at the points the GPU tests name."""
    g1 = [dict(sp=R.PATTERNS["ln_gelu"][4][0])]
    assert R.norm_form(g1, BF, 1, 1, 21, 2048) == ("normbwd.wide8", 256, 21)
    assert R.norm_form(g1, BF, 1, 1, 21, 2052) == ("normbwd.wide4", 512, 21)
    assert R.norm_form(g1, F32, 1, 1, 21, 2048, cap=9, ws_floats=9 * 2 * 2048) == ("normbwd.wide4.ws", 256, 9)
    assert R.norm_form(g1, BF, 1, 1, 37, 516, ws_floats=10 * 2 * 516 - 1) == ("normbwd.wave", 4, 10)
    assert R.norm_form(g1 * 8, BF, 1, 1, 200, 2048)[2] == 128 and R.norm_form(g1 * 8, BF, 1, 1, 200, 16384)[2] == 64


def test_a_reference_wrong_in_one_row_fails_the_local_check_only():
    """One row's c1 shifted (every element of the row off by the same amount): the global rel-L2 of test_bwd_ops_gpu.py passes, the local check does not."""
    # (the fp32 local bound is 4 x the global one: with 21 rows a single row can be off by up to sqrt(21) / 4 = 1.146 x the local bound and pass the global check)
    for dtype, gb, lb, factor in ((BF, R.BF16_GLOBAL, R.LOCAL["dXact"], 1.5), (F32, R.F32_GLOBAL, R.F32_LOCAL, 1.1)):
        g = R.norm_operands("adaln02", dtype, 21, 516, device="cpu")[0]
        ref = R.norm_bwd_formula(g, False)["dX32"]
        out = R.norm_bwd_formula(g, False, BF)["dXact"] if dtype == BF else ref.float().double()   # what a correct kernel stores
        assert rel(out, ref) < gb and rowerr(out, ref) < lb
        wrong = ref.clone()
        wrong[7] += factor * lb * float(ref.norm(dim=1).pow(2).mean().sqrt()) / math.sqrt(516)
        assert rel(out, wrong) < gb, (dtype, rel(out, wrong))
        assert rowerr(out, wrong) > lb, (dtype, rowerr(out, wrong))


def test_a_column_sum_without_one_row_fails_the_per_column_check_only():
    """One row's term left out of one column of dgamma: the global rel-L2 (3e-5) passes where the term is small, the per-column bound does not."""
    M, d = 21, 516
    g = R.norm_operands("adaln02", F32, M, d, device="cpu")[0]
    t = R.norm_bwd_formula(g, False)["tg"]
    old = g["dgamma0"]
    out = old.clone()
    for m in range(M):   # an fp32 sum in row order: what a correct kernel may compute
        out += t[m].float()
    bound = R.colsum_bound(old, t.abs().sum(0), M)
    assert bool(((out.double() - (old.double() + t.sum(0))).abs() <= bound).all())
    target = 1e-3
    idx = int((t.abs() - target).abs().argmin())
    m, c = idx // d, idx % d
    wrong = t.sum(0).clone()
    wrong[c] -= t[m, c]
    assert float(t[m, c].abs()) > 10 * float(bound[c])
    assert rel(out.double() - old.double(), wrong) < 3e-5
    assert not bool(((out.double() - (old.double() + wrong)).abs() <= bound).all())


def _ib_detected(g, masks, g_wrong, masks_wrong):
    """{gradient: fraction of its elements at which the reference of (g_wrong, masks_wrong) lies outside the bound of the right one}."""
    ref, wrong = R.ib_reference(g, masks), R.ib_reference(g_wrong, masks_wrong)
    out = {}
    for k, (s, a, n, extra) in ref.items():
        diff = (s - wrong[k][0]).abs()
        hit = (diff > R.colsum_bound(g["old"][k], a, n, extra))[diff > 1e-12 * a]   # (no difference beyond fp64 rounding: a masked-out element, to which the row gives nothing)
        out[k] = float(hit.double().mean()) if hit.numel() else 0.0
    return out


@pytest.mark.parametrize("F", R.IB_FIELDS)
@pytest.mark.parametrize("h,E", [(h, E) for h, E, _, _ in R.IB_MLP])
def test_an_ib_gradient_without_one_row_or_with_one_row_unmasked_fails_the_per_column_check(h, E, F):
    """At M = 65 (the row count at which a wave walks several rows) a reference that leaves one row out, or takes one row without its dropout mask, lies outside
    the bound of each of the six gradients at nearly every element (the rest: elements to which that row contributes next to nothing).  With one hidden unit
    the LayerNorm output is identically zero: dw1, db1 and dlnw vanish and cannot tell."""
    M = 65
    g = R.ib_operands(0, h, E, M, F, device="cpu")
    gen = torch.Generator().manual_seed(11)
    masks = [(torch.rand(M, E, generator=gen) > 0.1).double() * (256.0 / 230.0) for _ in range(F)]
    live = R.IB_NAMES if h > 1 else ("dlnb", "dw2", "db2")
    for m in (0, 31, 64):
        keep = [i for i in range(M) if i != m]
        cut = dict(g, c=g["c"][keep], dX=[x[keep] for x in g["dX"]])
        for masks_, cut_masks in ((None, None), (masks, [mk[keep] for mk in masks])):
            got = _ib_detected(g, masks_, cut, cut_masks)
            assert all(got[k] >= 0.85 for k in live), (m, masks_ is not None, sorted(got.items()))
        unmasked = [mk.clone() for mk in masks]
        for mk in unmasked:
            mk[m] = 1.0
        got = _ib_detected(g, masks, g, unmasked)
        assert all(got[k] >= 0.7 for k in live), (m, "unmasked", sorted(got.items()))   # (a tenth of one row's elements change: less than a whole row)
