"""The checks of test_fewrow_launches_gpu.py bite, shown on every machine with the CPU emulation of a launch (the fp64 formula, rounded to bf16 where the kernel
rounds) standing in for the kernel's output: the untouched emulation passes every check; ONE element computed without one 8-element piece of a K = 16384
contraction passes the whole-tensor and the per-row bound and fails the element bound; one head row of Q / K / V computed with one 8-column piece of the prologue's
A zeroed fails the per-row bound.  The LOCAL table of the GPU file is re-measured here: measured x 3 must be the table.

A few-row launch has few rows — at head dim 6 Q / K / V are 12 rows of 6 —, so a whole-tensor norm dilutes one wrong row by sqrt(12) at most, and a zeroed piece
of a K = 2048 operand (6 % of the projection) lies above the whole-tensor bound as well (2.3 to 3.1 times it for the piece zeroed here, 1.1 to 4.7 times over every
16th piece of the row): the per-row check is the tighter of the two by 1.3 to 1.7, not the only one that sees it.  Where rows are many — sea_rownorm's 64-column chunks — one wrong 4-column piece does pass the
whole-tensor bound and fail the per-row one; the last test shows that."""
from tests.test_fewrow_launches_gpu import (BF, GLOBAL, LOCAL, a_operand, assert_scaled, bounds, elem_excess, errors, gemm_formula, gemv_plain_groups,
                                            measure_local, qkv_fewrows_case, qkv_fewrows_cases, qkv_formula, rn_formula, rn_group, rounder, skinny_groups,
                                            skinny_long_cases, skinny_short_cases)


def verdicts(kind, out, ref, row=None, f32=False, g32=2e-5):
    """(global, local, element) verdicts of one output, as check() of the GPU file takes them."""
    eg, el = errors(out, ref, row)
    gb, lb = bounds(kind, f32, g32)
    return eg < gb, el < lb, elem_excess(out, ref) <= 1.0


def test_local_table_is_three_times_the_measured_value():
    for kind, (v, what) in measure_local("cpu", verbose=False).items():
        assert f"{v:.3e}" == f"{LOCAL[kind] / 3:.3e}", (kind, v, what, LOCAL[kind] / 3)


def test_gemm_operands_are_scaled_to_an_output_rms_near_one():
    for M in (1, 2, 3, 4):
        for K in (512, 16384):
            assert_scaled(gemv_plain_groups(M, K, "cpu"), (M, K))
    for M, Ks in skinny_short_cases():
        assert_scaled(skinny_groups(M, Ks, device="cpu"), (M, Ks))
    for M, Ks, act in skinny_long_cases():
        if Ks[0] <= 6144:
            assert_scaled(skinny_groups(M, Ks, device="cpu"), (M, Ks))


def test_one_dropped_piece_of_a_long_contraction_fails_the_element_check_alone():
    M, K = 4, 16384
    groups = gemv_plain_groups(M, K, "cpu")
    for g in groups:                                # the untouched emulation passes every check
        ref, emu = gemm_formula(g), gemm_formula(g, BF)
        for k in ref:
            if k == "C32":
                assert verdicts("gemv.C32", emu[k].float(), ref[k], f32=True, g32=3e-5) == (True, True, True), k
            else:
                assert verdicts("gemv." + k, emu[k].to(BF), ref[k]) == (True, True, True), k
    g = groups[2]                                   # N = 50, Cact alone: the plain product
    ref, emu = gemm_formula(g), gemm_formula(g, BF)
    m, n, piece = M - 1, g["N"] - 1, K // 8 - 1     # the last element without the last 8-element piece of its contraction
    part = float(g["A"].double()[m, 8 * piece:] @ g["W"].double()[n, 8 * piece:])
    bad = emu["Cact"].clone()
    bad[m, n] = rounder(BF)(ref["Cact"][m, n] - part)
    assert abs(part) > 0.25 * (8 / K) ** 0.5        # an ordinary piece: its share of an element is ~ sqrt(8 / K) = 2 %
    assert verdicts("gemv.Cact", bad.to(BF), ref["Cact"]) == (True, True, False)
    bad32 = ref["Cact"].clone()                     # the same element of an fp32 output: the element bound is 30 times tighter there
    bad32[m, n] -= part
    assert elem_excess(bad32.float(), ref["Cact"]) > 30


def _hd6_case(pro):
    M, K = 4, 2048
    for H, hd, form, B, T, pos0, p, vout in qkv_fewrows_cases(M, K):
        if hd == 6 and form == "self" and p == pro:
            return qkv_fewrows_case(M, K, H, hd, form, B, T, pos0, p, vout, device="cpu")
    raise AssertionError(pro)


def test_head_dim_6_untouched_passes_and_a_dropped_piece_fails_the_element_check():
    c = _hd6_case(None)
    g = c["groups"][0]
    ref, emu = qkv_formula(g, c), qkv_formula(g, c, BF)
    K = g["K"]
    a = g["A"].double().clone()
    a[-1, K - 8:] = 0                               # the last row without the last 8-element piece of its contraction ...
    bad = qkv_formula(dict(g, A=a), c, BF)
    for k in "QKV":
        assert verdicts("qkv." + k, emu[k].to(BF), ref[k], 6) == (True, True, True), k
        b = emu[k].clone()
        b[-1, -1, -1, -2:] = bad[k][-1, -1, -1, -2:]   # ... in ONE rotary pair of the last head (a pair: the rotation mixes its two columns)
        assert verdicts("qkv." + k, b.to(BF), ref[k], 6)[2] is False, k


def test_head_dim_6_a_zeroed_piece_of_the_prologues_rows_fails_the_local_check():
    c = _hd6_case("adaln")
    g = c["groups"][0]
    ref, emu = qkv_formula(g, c), qkv_formula(g, c, BF)
    a = a_operand(g, rounder(BF)).clone()
    a[-1, g["K"] - 8:] = 0                          # the last 8-column piece of the last normalised row
    bad = qkv_formula(dict(g, pre=None, A=a), c, BF)
    for k in "QKV":
        assert verdicts("qkv." + k, emu[k].to(BF), ref[k], 6)[:2] == (True, True), k
        b = emu[k].clone()
        b[-1, -1, -1] = bad[k][-1, -1, -1]          # ONE head row of 12: (last trajectory, last head, last step)
        g_ok, l_ok, _ = verdicts("qkv." + k, b.to(BF), ref[k], 6)
        eg, el = errors(b, ref[k], 6)
        print(f"{k}: global {eg:.3e} ({eg / GLOBAL['qkv.' + k]:.2f} of its bound)  local {el:.3e} ({el / LOCAL['qkv.' + k]:.2f} of its bound)")
        assert not l_ok, k
        assert el / LOCAL["qkv." + k] > eg / GLOBAL["qkv." + k], k   # the per-row bound is the tighter one


def test_one_wrong_piece_of_a_long_normalised_row_passes_globally_and_fails_locally():
    g = rn_group("mod", 32, 16384, 0, device="cpu")
    ref, emu = rn_formula(g)["Yact"], rn_formula(g, BF)["Yact"]
    assert verdicts("rn.Yact", emu.to(BF), ref, 64)[:2] == (True, True)
    bad = emu.clone()
    bad[31, 16380:] = 0                             # the last 4-column piece of the last row never written
    assert verdicts("rn.Yact", bad.to(BF), ref, 64)[:2] == (True, False)
