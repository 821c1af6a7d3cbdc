"""The three row-walking backward launchers of sea_amd/csrc/bwd.hip — sea_rownorm_bwd, sea_silu_outer_bwd, sea_ib_bwd — per row and per column against fp64, in the
forms training issues and at the edges of their kernels, in the discipline of test_row_launches_gpu.py.

Reference: the fp64 formula of include/sea_hip.h (SeaNormBwdGroup, SeaSiluBwdGroup, SeaIbBwdParams) on the operands as rounded to their storage type, NO intermediate
rounded.  mean / rstd are computed in fp64 from the stored x and handed to the launcher (and to the reference) as fp32: the forward kernel is not called.  Dropout
masks come from sea_dropout_mask.

Row outputs (dX32, dXact, dmod), two checks each, spread(ref) <= 3 asserted:
  global  ||out - ref|| / ||ref|| at the bounds of test_bwd_ops_gpu.py: 3e-5 an fp32 output, 1e-2 a bf16 one.
  local   max over rows ||err_row|| / rms over rows ||ref_row|| (rowerr).  fp32 outputs (nothing is rounded upstream): 4 x 3e-5.  bf16 outputs: LOCAL, 3 x the largest
          rowerr(emulation, reference) over every bf16 case of this file, the emulation being the same fp64 formula with a rounding to bf16 where the kernel rounds (the
          stored output) and, for launches with GELU, the polynomial of gelu_erf_grad_bf16 (sea_common.hpp) restated in torch; with both off it restates the reference
          to 1e-12.  `python tests/test_bwd_rows_gpu.py` measures this on the CPU and prints the worst case per output kind.
  An accumulated dX32 is compared with old + ref formed in fp64.

Column sums (dgamma, dbeta, dw1, db1, the six info-bottleneck gradients), per element c, from NON-ZERO contents `old`:
  |out_c - (old_c + sum_m t_mc)| <= (n + 16) 2^-24 (|old_c| + sum_m |t_mc|) (+ extra),   u = 2^-24
  t_mc the fp64 terms, n their number: an fp32 sum of n + 1 values (the old content is one of them) in any order errs by at most n u times their absolute sum, 16 u
  covers the fp32 arithmetic of a term.  M <= 70 keeps this far below one dropped row (~ 1 / M of the absolute sum).  extra:
    GELU: EPS sum_m |dy_mc| max(1, |xhat_mc|).  The 16 u of a term is a RELATIVE error; GELU' is evaluated with an ABSOLUTE one, which does not vanish with the term
    near GELU' = 0 (at -0.75 and in the negative tail).  bf16 launches: EPS_POLY, the largest error of the restated polynomial against fp64 GELU' on [-6, 6];
    fp32 launches: EPS_AS, the largest error of the restated Abramowitz-Stegun erf plus 8 u for its fp32 evaluation.  Operands run over the whole range.
    (bf16 dgamma reaches 0.97 of its bound at M = 1, where a column is one term whose GELU' argument lies at the polynomial's worst point.  EPS_POLY is a true
    maximum of the restated polynomial, the kernel's fp32 evaluation of it and the order of the atomics move the error by some u of the term, which the
    (n + 16) u part holds: the ratio is a property of the operands, not of the run.)
    SiLU: EPS_SILU sum_m |dHid_mc| (|c_m|), 8 u for the fp32 SiLU' (|SiLU'| <= 1.1), absolute for the same reason (SiLU' = 0 at -1.28); operands over the whole range.
    sea_ib_bwd: a term of the hidden layer's gradients is no single fp32 product but a dot product over the E columns and F fields, a LayerNorm over the h hidden
    units and a GELU by the Abramowitz-Stegun erf; ib_reference() carries their first-order errors through the formula (D... quantities).  The dot product
    takes the probabilistic model of rounding (errors of random sign): (sqrt(E F) + 2) u times the absolute sum, not the worst case E F u, which at E = 1028,
    F = 3 would let a whole row go missing.  db2 / dW2 count a term per (row, field), n = M F.  tests/test_bwd_rows_cpu.py drops a row, and unmasks a row, at
    M = 65 and finds each of the six gradients outside its bound.

Every launch: outputs in NaN frames or guarded buffers, every row-major input the first M rows of a taller tensor whose extra rows are NaN (half of them column
slices of a wider one), ops.last_form() asserted right after the launch with a and b, the frames checked untouched.  Forms are forced through SEA_TUNE (force())."""
import math
import os
import sys

import pytest
import torch

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests.test_forced_forms_gpu import BF, dev, force, frame_untouched, framed, gelu64, rel, rnd, rowerr, spread  # noqa: E402
from tests.test_row_launches_gpu import guard_untouched, guarded, launched, rounder, tall  # noqa: E402

pytestmark = pytest.mark.gpu

NAN = float("nan")
F32 = torch.float32
U = 2.0 ** -24
F32_GLOBAL, F32_LOCAL, BF16_GLOBAL = 3e-5, 4 * 3e-5, 1e-2
# the largest |restated polynomial - fp64 GELU'| on [-6, 6] and the largest error of the restated Abramowitz-Stegun 7.1.26 erf (python tests/test_bwd_rows_gpu.py)
EPS_POLY = 7.320e-05
EPS_ERF = 1.394e-07
EPS_AS = EPS_ERF + 8 * U   # ... and its fp32 evaluation (v_rcp, v_exp)
EPS_SILU = 8 * U            # SiLU' in fp32 (|SiLU'| <= 1.1: the rounded argument, v_exp, the division): an ABSOLUTE error, which the 16 u of a term cannot cover near SiLU' = 0
# 3 x the largest rowerr(emulation, reference) over every bf16 case of the file (python tests/test_bwd_rows_gpu.py, on the CPU); the measured value and its case.
# "@4": the rows of 4 columns, where one rounding is a large part of a row's error (3 to 5 times the value of the wider rows), held to their own bound.
LOCAL = {
    "dXact": 3 * 2.521e-03,   # rownorm_bwd addnorm M=21 d=68 group 0
    "dXact.gelu": 3 * 2.624e-03,   # rownorm_bwd ln_gelu M=37 d=68 group 0
    "dmod": 3 * 2.300e-03,   # rownorm_bwd final M=21 d=68 group 1
    "dXact@4": 3 * 6.790e-03,   # rownorm_bwd adaln02 M=37 d=4 group 1
    "dXact.gelu@4": 3 * 6.152e-03,   # rownorm_bwd ln_gelu M=21 d=4 group 1
    "dmod@4": 3 * 5.216e-03,   # rownorm_bwd adaln02 M=37 d=4 group 0
}


# ------------------------------------------------------------------------------------------------ helpers
def inp(t, strided, extra=4):
    """The first M rows of a tensor `extra` rows taller whose extra rows are NaN; strided: columns [8, 8 + N) of a tensor 24 columns wider that is NaN elsewhere."""
    if t is None:
        return None
    if not strided:
        return tall(t, extra)
    M, N_ = t.shape
    big = torch.full((M + extra, N_ + 24), NAN, device=t.device, dtype=t.dtype)
    big[:M, 8:8 + N_] = t
    return big[:M, 8:8 + N_]


def filled(shape, dtype, value):
    """guarded() with the view set to `value`: (whole, view)."""
    flat, v = guarded(shape, dtype)
    v.copy_(value)
    return flat, v


_SEEN = {}    # row-output kind -> [worst global, worst local, checks, global bound, local bound] of the running test
_SEENC = {}   # column-sum kind -> [worst error / bound, checks]


def check(kind, out, ref, what, f32):
    """Both checks of one row output; f32: an fp32 output (nothing rounded upstream)."""
    assert spread(ref) <= 3.0, (what, kind, spread(ref))
    assert torch.isfinite(out.float()).all(), (what, kind, "not finite")
    eg, el = rel(out, ref), rowerr(out, ref)
    gb, lb = (F32_GLOBAL, F32_LOCAL) if f32 else (BF16_GLOBAL, LOCAL[kind])
    name = kind + (".f32" if f32 else "")
    print(f"{what} {name}: global {eg:.3e} (< {gb:.1e})  local {el:.3e} (< {lb:.3e})")
    w = _SEEN.setdefault(name, [0.0, 0.0, 0, gb, lb])
    w[0], w[1], w[2] = max(w[0], eg), max(w[1], el), w[2] + 1
    assert eg < gb, (what, name, "global", eg, gb)
    assert el < lb, (what, name, "local", el, lb)


def colsum_bound(old, abs_sum, n, extra=None):
    b = (n + 16) * U * (old.double().abs() + abs_sum)
    return b + extra if extra is not None else b


def check_colsum(kind, out, old, ref_sum, abs_sum, n, what, extra=None):
    """A column sum per element: out against old + ref_sum (fp64) at colsum_bound."""
    assert torch.isfinite(out).all(), (what, kind, "not finite")
    err = (out.double() - (old.double() + ref_sum)).abs()
    bound = colsum_bound(old, abs_sum, n, extra)
    ratio = float((err / bound.clamp_min(1e-300)).max())
    print(f"{what} {kind}: largest error / bound {ratio:.3f} (n = {n})")
    w = _SEENC.setdefault(kind, [0.0, 0])
    w[0], w[1] = max(w[0], ratio), w[1] + 1
    assert bool((err <= bound).all()), (what, kind, "element", int((err / bound.clamp_min(1e-300)).argmax()), ratio)


@pytest.fixture(autouse=True)
def _one_line_per_test(request):
    """The line of profiles/bwd_rows_gpu_errors.txt: the largest global and local error of every row-output kind and the largest error / bound of every
    column-sum kind the test checked."""
    _SEEN.clear()
    _SEENC.clear()
    yield
    if _SEEN or _SEENC:
        parts = [f"{k} global {w[0]:.3e} (< {w[3]:.1e}) local {w[1]:.3e} (< {w[4]:.3e}) over {w[2]}" for k, w in sorted(_SEEN.items())]
        parts += [f"{k} error/bound {w[0]:.3f} (< 1) over {w[1]}" for k, w in sorted(_SEENC.items())]
        print("BWD_ROWS " + request.node.name + ": " + "; ".join(parts))


# ------------------------------------------------------------------------------------------------ GELU' and its approximations
_POLY = (-1.903182723e-09, 1.410586208e-07, -4.565313247e-06, 8.634554251e-05, -1.085383119e-03, 9.789848700e-03, -6.636063010e-02, 3.989269733e-01)
_INV_SQRT_2PI = 0.39894228040143267794


def gelu_grad64(u):
    return 0.5 * (1 + torch.erf(u / math.sqrt(2))) + u * _INV_SQRT_2PI * torch.exp(-0.5 * u * u)


def gelu_grad2_64(u):
    """GELU'' = phi(u) (2 - u^2)."""
    return _INV_SQRT_2PI * torch.exp(-0.5 * u * u) * (2 - u * u)


def gelu_grad_poly(u):
    """gelu_erf_grad_bf16 (sea_common.hpp) in fp64: Phi(x) - 1/2 = x P(x^2) with x clamped to [-4, 4], plus x phi(x)."""
    xc = u.clamp(-4.0, 4.0)
    w = xc * xc
    p = torch.full_like(u, float(torch.tensor(_POLY[0], dtype=F32)))
    for c in _POLY[1:]:
        p = p * w + float(torch.tensor(c, dtype=F32))
    return u * _INV_SQRT_2PI * torch.exp(-0.5 * u * u) + (xc * p + 0.5)


def erf_as(x):
    """erf_gauss (sea_common.hpp) in fp64: Abramowitz-Stegun 7.1.26 on z = |x| / sqrt 2."""
    z = x.abs() / math.sqrt(2)
    t = 1.0 / (1.0 + 0.3275911 * z)
    poly = t * (0.254829592 + t * (-0.284496736 + t * (1.421413741 + t * (-1.453152027 + t * 1.061405429))))
    return torch.sign(x) * (1.0 - poly * torch.exp(-0.5 * x * x))


def measure_eps():
    """(EPS_POLY, EPS_ERF) as measured: the restated approximations against fp64 on a dense grid."""
    u = torch.linspace(-6, 6, 1200001, dtype=torch.float64)
    v = torch.linspace(-9, 9, 1800001, dtype=torch.float64)
    return float((gelu_grad_poly(u) - gelu_grad64(u)).abs().max()), float((erf_as(v) - torch.erf(v / math.sqrt(2))).abs().max())


# ------------------------------------------------------------------------------------------------ sea_rownorm_bwd
def _g(mod=0, beta=0, dbeta=None, dx32=None, dxact=None, sums=1, strided=0):
    return dict(mod=mod, beta=beta, dbeta=beta if dbeta is None else dbeta, dx32=dx32, dxact=dxact, sums=sums, strided=strided)


# name: (dy_is_act, x_is_act, gelu, accumulate, the groups of one launch).  dx32: "new" a fresh output, "acc" added to its contents, "inplace" written over dY (both
# the same column slice of one fp32 [M, n d] buffer, as the final norm's dout); dxact: "new", or "inplace" over an act dY (the MLP's LayerNorm + GELU).
PATTERNS = {
    "final": (0, 0, False, False, [_g(mod=1, beta=1, dx32="inplace", dxact="new"), _g(mod=1, beta=1, dx32="inplace", dxact="new", strided=1),
                                   _g(dx32="inplace", dxact="new")]),
    "ln_gelu": (1, 1, True, False, [_g(beta=1, dxact="inplace"), _g(beta=1, dxact="inplace", strided=1), _g(beta=1, dxact="inplace", sums=0)]),
    "adaln02": (1, 0, False, True, [_g(mod=1, beta=1, dx32="acc", dxact="new", strided=1), _g(dx32="acc", dxact="new")]),   # the second: gamma only, dbeta = None
    "addnorm": (1, 0, False, False, [_g(beta=1, dxact="new")]),
    "cross": (0, 0, False, False, [_g(dxact="new", strided=1)]),
    "unused": (0, 1, False, False, [_g(beta=1, dx32="new")]),
}
MS = (1, 4, 5, 21)
PATTERN_D = (68, 516, 2052)                                # every pattern: KMAX 1 and 4 off a chunk edge, and the 4-column wide form
NARROW_D = (4, 68, 256, 260, 512, 516, 1024)               # KMAX = 1 / 2 / 4 and their chunk edges
NARROW_WS_M = 37                                           # the narrow kernel takes ceil(M / 4) workgroups: the two-stage sums need more than 8 of them
WIDE4_D = (1028, 2048, 2052, 4100, 8196, 16384)            # 256 / 512 / 1024 threads, 2 and 4 chunks, the re-reading form above 8192
WIDE4_BF_D = (1028, 2048, 2052)
WIDE8_D = (1032, 2048, 2056, 4104, 8200, 16384)
EIGHT = dict(d=2048, M=5, n=8)
EIGHT_CLAMP_M = 130   # 8 groups at d <= 2048: at most 128 workgroups per group stay resident, so 130 rows reach the clamp


def norm_cases():
    """(pattern, dtype, M, d, n groups or None) of every rownorm launch of this file (forced forms reuse the operands of their shape)."""
    out = []
    for dtype in (F32, BF):
        out += [(p, dtype, M, d, None) for p in PATTERNS for d in PATTERN_D for M in MS]
        out += [(p, dtype, M, d, None) for p in ("adaln02", "ln_gelu") for d in NARROW_D for M in MS + (NARROW_WS_M,)]
        out += [("adaln02", dtype, M, d, None) for d in (WIDE4_D if dtype == F32 else WIDE4_BF_D) for M in MS]
        out += [("final", dtype, M, EIGHT["d"], EIGHT["n"]) for M in (EIGHT["M"], EIGHT_CLAMP_M)]
    out += [("ln_gelu", BF, M, d, None) for d in WIDE8_D for M in MS]
    return list(dict.fromkeys(out))


def norm_operands(pattern, dtype, M, d, n=None, device=None):
    """The groups of one launch, operands in their storage types.  GELU in fp32: gamma ~ 0.3, beta ~ 1 keep GELU's argument in about [-0.3, 2.3] (module docstring)."""
    dy_act, x_act, gelu, acc, specs = PATTERNS[pattern]
    if n is not None:
        specs = [specs[i % len(specs)] for i in range(n)]
    kw = dict(device=device)
    groups = []
    for i, sp in enumerate(specs):
        seed = 50000 + 100000 * list(PATTERNS).index(pattern) + 1000 * i + 7 * d + M
        x = rnd(M, d, seed=seed + 1, **kw)
        if d == 4:   # four samples: every row brought to the same variance, or rstd (and with it the rows of dX) spreads by more than the factor 3 of check()
            x = (x - x.mean(1, keepdim=True)) / x.std(1, keepdim=True)
        x = (x * 1.3 + 0.2).to(dtype if x_act else F32)
        dy = rnd(M, d, seed=seed + 2, **kw).to(dtype if dy_act else F32)
        gamma = 1 + 0.1 * rnd(d, seed=seed + 3, **kw)
        beta = 0.1 * rnd(d, seed=seed + 4, **kw) if sp["beta"] else None
        mod = rnd(M, 2 * d, dtype=dtype, scale=0.3, seed=seed + 5, **kw) if sp["mod"] else None
        xd = x.double()
        mu = xd.mean(1)
        rstd = 1.0 / torch.sqrt(((xd - mu[:, None]) ** 2).mean(1) + 1e-5)
        groups.append(dict(sp=sp, M=M, d=d, x=x, dy=dy, gamma=gamma, beta=beta, mod=mod, mean=mu.float(), rstd=rstd.float(), mean64=mu, rstd64=rstd,
                           old=rnd(M, d, seed=seed + 6, **kw) if acc and sp["dx32"] else None,
                           dgamma0=rnd(d, seed=seed + 7, **kw), dbeta0=rnd(d, seed=seed + 8, **kw)))
    return groups


def norm_bwd_formula(g, gelu, rt=None, poly=False, exact_stats=False):
    """SeaNormBwdGroup in fp64.  rt: the rounding of the stored act outputs (dXact, dmod); poly: GELU' by the bf16 launches' polynomial; exact_stats: the fp64
    mean / rstd instead of the fp32 ones the launcher is given.  tg / tb: the terms of dgamma / dbeta; gw: |dy| max(1, |xhat|), the weight of GELU's error."""
    r = rounder(rt)
    d = g["d"]
    mean, rstd = (g["mean64"], g["rstd64"]) if exact_stats else (g["mean"].double(), g["rstd"].double())
    x, dy = g["x"].double(), g["dy"].double()
    xh = (x - mean[:, None]) * rstd[:, None]
    s = g["gamma"].double() + ((1 + g["mod"].double()[:, :d]) if g["mod"] is not None else 0.0)
    t = (g["beta"].double() if g["beta"] is not None else 0.0) + (g["mod"].double()[:, d:] if g["mod"] is not None else 0.0)
    dv = dy * ((gelu_grad_poly if poly else gelu_grad64)(xh * s + t)) if gelu else dy
    dxh = dv * s
    c1, c2 = dxh.mean(1, keepdim=True), (dxh * xh).mean(1, keepdim=True)
    dx = rstd[:, None] * (dxh - c1 - xh * c2)
    tot = dx + (g["old"].double() if g["old"] is not None else 0.0)
    return dict(dX32=tot, dXact=r(tot), dmod=r(torch.cat([dv * xh, dv], 1)), tg=dv * xh, tb=dv, gw=dy.abs() * xh.abs().clamp_min(1.0))


def norm_form(groups, dtype, dy_act, x_act, M, d, cap=512, wide8_on=True, ws_floats=0):
    """(form, a, b) sea_rownorm_bwd notes: the launcher's rule restated."""
    n = len(groups)
    wide = d > 1024
    nblk = min(M if wide else (M + 3) // 4, cap)
    if wide:
        per_cu = 5 if d <= 2048 else (2 if d <= 4096 else 1)
        fit = (per_cu * 256 // n) // 64 * 64
        if d > 2048 and fit < 64:
            fit = 64
        if fit >= 64 and nblk > fit:
            nblk = fit
    wide8 = (wide and dtype == BF and bool(dy_act) and bool(x_act) and d % 8 == 0 and wide8_on
             and all(not g["sp"]["mod"] and g["sp"]["dx32"] is None for g in groups))
    two = ws_floats >= n * nblk * 2 * d and nblk > 8
    name = ("normbwd.wide8" if wide8 else "normbwd.wide4") if wide else "normbwd.wave"
    a = (256 if d <= 2048 else (512 if d <= 4096 else 1024)) if wide else (1 if d <= 256 else (2 if d <= 512 else 4))
    return name + (".ws" if two else ""), a, nblk


_NORM_REF = {}
_NORM_CASES = None


def _norm_case(pattern, dtype, M, d, n=None):
    """(groups, fp64 references) of one case, computed once per session and left unchanged."""
    global _NORM_CASES
    if _NORM_CASES is None:
        _NORM_CASES = set(norm_cases())
    key = (pattern, dtype, M, d, n)
    assert key in _NORM_CASES, key   # LOCAL is measured over norm_cases(): a launch outside it would be held to a bound that never saw it
    if key not in _NORM_REF:
        groups = norm_operands(pattern, dtype, M, d, n)
        _NORM_REF[key] = (groups, [norm_bwd_formula(g, PATTERNS[pattern][2]) for g in groups])
    return _NORM_REF[key]


def run_norm(monkeypatch, pattern, dtype, M, d, tune="", cap=512, ws_blocks=0, n=None, wide8_on=True, expect=None):
    """One launch of sea_rownorm_bwd and every check of it; returns the form it took."""
    from sea_amd import ops

    dy_act, x_act, gelu, acc, _ = PATTERNS[pattern]
    groups, refs = _norm_case(pattern, dtype, M, d, n)
    ng = len(groups)
    shared = torch.full((M + 4, ng * d + 16), NAN, device=dev(), dtype=F32) if any(g["sp"]["dx32"] == "inplace" for g in groups) else None
    gds, outs = [], []
    for i, g in enumerate(groups):
        sp, o = g["sp"], {}
        gd = dict(X=inp(g["x"], sp["strided"]), gamma=g["gamma"], beta=g["beta"], mod=inp(g["mod"], False), mean=tall(g["mean"], 4), rstd=tall(g["rstd"], 4))
        if sp["dx32"] == "inplace":
            v = shared[:M, 8 + i * d:8 + (i + 1) * d]
            v.copy_(g["dy"])
            gd["dY"] = gd["dX32"] = v
            o["dX32"] = (None, v)
        elif sp["dxact"] == "inplace":
            big = torch.full((M + 4, d + 24), NAN, device=dev(), dtype=g["dy"].dtype)
            v = big[:M, 8:8 + d]
            v.copy_(g["dy"])
            gd["dY"] = gd["dXact"] = v
            o["dXact"] = (big, v)
        else:
            gd["dY"] = inp(g["dy"], sp["strided"])
        if sp["dx32"] in ("new", "acc"):
            o["dX32"] = framed(M, d, F32)
            if g["old"] is not None:
                o["dX32"][1].copy_(g["old"])
            gd["dX32"] = o["dX32"][1]
        if sp["dxact"] == "new":
            o["dXact"] = framed(M, d, dtype)
            gd["dXact"] = o["dXact"][1]
        if sp["mod"]:
            o["dmod"] = framed(M, 2 * d, dtype)
            gd["dmod"] = o["dmod"][1]
        if sp["sums"]:
            o["dgamma"] = filled((d,), F32, g["dgamma0"])
            gd["dgamma"] = o["dgamma"][1]
            if sp["dbeta"]:
                o["dbeta"] = filled((d,), F32, g["dbeta0"])
                gd["dbeta"] = o["dbeta"][1]
        gds.append(gd)
        outs.append(o)
    wsf, ws = guarded((ng * ws_blocks * 2 * d,), F32) if ws_blocks else (None, None)
    force(monkeypatch, tune)
    ops.rownorm_bwd(gds, M, d, dy_act, x_act, gelu, acc, dtype, ws=ws)
    want = norm_form(groups, dtype, dy_act, x_act, M, d, cap=cap, wide8_on=wide8_on, ws_floats=0 if ws is None else ws.numel())
    got = launched(ops, want[0])
    assert got == want, (got, want)
    if expect is not None:
        assert got == expect, (got, expect)
    for i, (g, ref, o) in enumerate(zip(groups, refs, outs)):
        what = f"rownorm_bwd {pattern} {str(dtype)[6:]} M={M} d={d} {tune} {got[0]} group {i}"
        for k, width in (("dX32", d), ("dXact", d), ("dmod", 2 * d)):
            if k not in o:
                continue
            big, v = o[k]
            f32 = v.dtype == F32
            check(k + (".gelu" if gelu and not f32 else "") + ("@4" if d == 4 and not f32 else ""), v, ref[k], what, f32)
            if big is not None:
                assert frame_untouched(big, width) and bool(torch.isnan(big[M:].float()).all()), (what, k, "frame")
        extra = (EPS_POLY if dtype == BF else EPS_AS) * ref["gw"].sum(0) if gelu else None
        for k, t, old in (("dgamma", ref["tg"], g["dgamma0"]), ("dbeta", ref["tb"], g["dbeta0"])):
            if k in o:
                check_colsum("norm." + k, o[k][1], old, t.sum(0), t.abs().sum(0), M, what, extra)
                assert guard_untouched(o[k][0]), (what, k, "guard")
    if shared is not None:
        assert bool(torch.isnan(shared[M:]).all() and torch.isnan(shared[:, :8]).all() and torch.isnan(shared[:, 8 + ng * d:]).all()), (pattern, "shared frame")
    if wsf is not None:
        assert guard_untouched(wsf), (pattern, "workspace guard")
    return got


@pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("pattern", list(PATTERNS))
def test_rownorm_bwd_calling_patterns(monkeypatch, pattern, dtype):
    """Training's calling patterns (operand types, aliased outputs, optional outputs) on the narrow kernel at KMAX 1 and 4 and on the 4-column wide kernel."""
    for d in PATTERN_D:
        for M in MS:
            run_norm(monkeypatch, pattern, dtype, M, d)


@pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("d", NARROW_D)
def test_rownorm_bwd_narrow_widths(monkeypatch, d, dtype):
    """The wave-per-row kernel at KMAX = 1 / 2 / 4 and off its 256-column chunk edges, M around the 4 rows of a workgroup; a wave walking several rows (2 workgroups
    for 21 rows); the two-stage column sums (10 workgroups)."""
    km = 1 if d <= 256 else (2 if d <= 512 else 4)
    for pattern in ("adaln02", "ln_gelu"):
        for M in MS:
            run_norm(monkeypatch, pattern, dtype, M, d, expect=("normbwd.wave", km, (M + 3) // 4))
        run_norm(monkeypatch, pattern, dtype, 21, d, tune="normbwd_blocks=2", cap=2, expect=("normbwd.wave", km, 2))
        run_norm(monkeypatch, pattern, dtype, NARROW_WS_M, d, ws_blocks=10, expect=("normbwd.wave.ws", km, 10))


def _threads(d):
    return 256 if d <= 2048 else (512 if d <= 4096 else 1024)


@pytest.mark.parametrize("dtype,d", [(F32, d) for d in WIDE4_D] + [(BF, d) for d in WIDE4_BF_D], ids=str)
def test_rownorm_bwd_wide_four_columns_with_modulation(monkeypatch, dtype, d):
    """The workgroup-per-row kernel in its 4-column form with mod / dmod, dX32 += and dXact (AdaLN_0 / 2 at the hidden widths): every thread count and chunk count,
    several rows per workgroup with the column sums by atomics (3 workgroups for 21 rows) and through the two-stage workspace (9)."""
    for M in MS:
        run_norm(monkeypatch, "adaln02", dtype, M, d, expect=("normbwd.wide4", _threads(d), M))
    run_norm(monkeypatch, "adaln02", dtype, 21, d, tune="normbwd_blocks=3", cap=3, expect=("normbwd.wide4", _threads(d), 3))
    run_norm(monkeypatch, "adaln02", dtype, 21, d, tune="normbwd_blocks=9", cap=9, ws_blocks=9, expect=("normbwd.wide4.ws", _threads(d), 9))


@pytest.mark.parametrize("d", WIDE8_D)
def test_rownorm_bwd_wide_eight_columns(monkeypatch, d):
    """LayerNorm + GELU in bf16, dXact over dY: the 8-column form at every thread count, one and two chunks; at d = 2048 the 4-column form within the same bounds of
    the same reference."""
    for M in MS:
        run_norm(monkeypatch, "ln_gelu", BF, M, d, expect=("normbwd.wide8", _threads(d), M))
    run_norm(monkeypatch, "ln_gelu", BF, 21, d, tune="normbwd_blocks=3", cap=3, expect=("normbwd.wide8", _threads(d), 3))
    run_norm(monkeypatch, "ln_gelu", BF, 21, d, tune="normbwd_blocks=9", cap=9, ws_blocks=9, expect=("normbwd.wide8.ws", _threads(d), 9))
    if d == 2048:
        for M in MS:
            run_norm(monkeypatch, "ln_gelu", BF, M, d, tune="normbwd_wide8=0", wide8_on=False, expect=("normbwd.wide4", 256, M))
        run_norm(monkeypatch, "ln_gelu", BF, 21, d, tune="normbwd_wide8=0,normbwd_blocks=3", cap=3, wide8_on=False, expect=("normbwd.wide4", 256, 3))


@pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])
def test_rownorm_bwd_eight_groups(monkeypatch, dtype):
    """SEA_MAX_NORM_BWD_GROUPS groups in one wide launch (blockIdx.y up to 7): 5 rows, below the residency clamp of 128 workgroups per group, and 130 rows, which
    reach it (two workgroups of every group walk two rows)."""
    run_norm(monkeypatch, "final", dtype, EIGHT["M"], EIGHT["d"], n=EIGHT["n"], expect=("normbwd.wide4", 256, EIGHT["M"]))
    run_norm(monkeypatch, "final", dtype, EIGHT_CLAMP_M, EIGHT["d"], n=EIGHT["n"], expect=("normbwd.wide4", 256, 128))


# ------------------------------------------------------------------------------------------------ sea_silu_outer_bwd
SILU_K2 = (4, 256, 260, 512, 1024, 1028, 2048)
SILU_MS = (1, 4, 5, 37)
SILU_PAIR = (1028, 260)   # two groups of one launch: the workspace stride is the larger K2, the second group's own width the smaller


def silu_operands(M, K2s, dtype, device=None):
    """c in [0, 1], pre = w1 c + b1 around 0.8 +- 0.5: SiLU' stays away from its zero at -1.28 (module docstring)."""
    kw = dict(device=device)
    seed = 70000 + 13 * M + sum(K2s)
    g = torch.Generator(device="cpu").manual_seed(seed)
    c = (2 * torch.rand(M, generator=g) - 0.5).to(device if device is not None else dev())
    return dict(M=M, c=c, groups=[dict(K2=K2, w1=rnd(K2, seed=seed + 10 * i + 1, **kw), b1=rnd(K2, seed=seed + 10 * i + 2, **kw),
                                       dH=rnd(M, K2, dtype=dtype, seed=seed + 10 * i + 3, **kw), dw10=rnd(K2, seed=seed + 10 * i + 4, **kw),
                                       db10=rnd(K2, seed=seed + 10 * i + 5, **kw)) for i, K2 in enumerate(K2s)])


def silu_bwd_formula(c, g):
    """SeaSiluBwdGroup in fp64: the terms [M, K2] of dw1 and of db1, and |dHid| (the weight of SiLU's absolute error)."""
    cd = c.double()[:, None]
    pre = cd * g["w1"].double() + g["b1"].double()
    sg = torch.sigmoid(pre)
    dpre = g["dH"].double() * sg * (1 + pre * (1 - sg))
    return dpre * cd, dpre, g["dH"].double().abs()


_SILU_REF = {}


def _silu_case(M, K2s, dtype):
    key = (M, K2s, dtype)
    if key not in _SILU_REF:
        su = silu_operands(M, K2s, dtype)
        _SILU_REF[key] = (su, [silu_bwd_formula(su["c"], g) for g in su["groups"]])
    return _SILU_REF[key]


def run_silu(monkeypatch, M, K2s, dtype, tune, ws_floats, expect, strided=False):
    from sea_amd import ops

    su, refs = _silu_case(M, K2s, dtype)
    outs = [(filled((g["K2"],), F32, g["dw10"]), filled((g["K2"],), F32, g["db10"])) for g in su["groups"]]
    gds = [dict(dHid=inp(g["dH"], strided), w1=g["w1"], b1=g["b1"], dw1=o[0][1], db1=o[1][1]) for g, o in zip(su["groups"], outs)]
    wsf, ws = guarded((ws_floats,), F32) if ws_floats else (None, None)
    force(monkeypatch, tune)
    ops.silu_outer_bwd(gds, tall(su["c"], 4), M, dtype, ws=ws)
    got = launched(ops, expect[0])
    assert got == expect, (got, expect)
    ca = su["c"].double().abs()[:, None]
    for i, (g, (tw, tb, ah), o) in enumerate(zip(su["groups"], refs, outs)):
        what = f"silu_outer_bwd {str(dtype)[6:]} M={M} K2={g['K2']} {tune} {got[0]} group {i}"
        check_colsum("silu.dw1", o[0][1], g["dw10"], tw.sum(0), tw.abs().sum(0), M, what, EPS_SILU * (ah * ca).sum(0))
        check_colsum("silu.db1", o[1][1], g["db10"], tb.sum(0), tb.abs().sum(0), M, what, EPS_SILU * ah.sum(0))
        assert guard_untouched(o[0][0]) and guard_untouched(o[1][0]), (what, "guard")
    if wsf is not None:
        assert guard_untouched(wsf), "workspace guard"


def _km(K2):
    return 1 if K2 <= 256 else (2 if K2 <= 512 else (4 if K2 <= 1024 else 8))


@pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("K2", SILU_K2)
def test_silu_outer_bwd_wave_form(monkeypatch, K2, dtype):
    """The wave-per-row kernel at KM = 1 / 2 / 4 / 8 and their chunk edges: without a workspace, with one under silubwd_cols=0 (the two-stage sums at 10 workgroups),
    a wave walking several rows (2 workgroups for 37 rows), dHid contiguous and a column slice."""
    for M in SILU_MS:
        for strided in (False, True):
            run_silu(monkeypatch, M, (K2,), dtype, "", 0, ("silu_bwd.wave", _km(K2), (M + 3) // 4), strided)
    run_silu(monkeypatch, 37, (K2,), dtype, "silubwd_blocks=2", 0, ("silu_bwd.wave", _km(K2), 2), True)
    run_silu(monkeypatch, 37, (K2,), dtype, "silubwd_cols=0", 10 * 2 * K2, ("silu_bwd.wave.ws", _km(K2), 10), True)
    run_silu(monkeypatch, 37, (K2,), dtype, "silubwd_cols=0", 10 * 2 * K2 - 1, ("silu_bwd.wave", _km(K2), 10))   # one float short: atomics


@pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])
def test_silu_outer_bwd_two_widths_in_one_launch(monkeypatch, dtype):
    """Two groups of different K2: the kernel is instantiated for the larger, the workspace slabs are strided by it, each group sums its own width."""
    km = _km(max(SILU_PAIR))
    for M in SILU_MS:
        run_silu(monkeypatch, M, SILU_PAIR, dtype, "", 0, ("silu_bwd.wave", km, (M + 3) // 4), True)
    run_silu(monkeypatch, 37, SILU_PAIR, dtype, "silubwd_cols=0", 2 * 10 * 2 * max(SILU_PAIR), ("silu_bwd.wave.ws", km, 10))
    run_silu(monkeypatch, 37, SILU_PAIR, dtype, "silubwd_cols=0,silubwd_blocks=2", 0, ("silu_bwd.wave", km, 2))


@pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("M", [15, 16, 17])
def test_silu_outer_bwd_column_form_row_splits(monkeypatch, M, dtype):
    """The column-block form around its 16-row trip with a workspace that admits exactly one, then two, row splits."""
    ncb = sum((K2 + 255) // 256 for K2 in SILU_PAIR)
    slab = 2 * 2 * max(SILU_PAIR)
    run_silu(monkeypatch, M, SILU_PAIR, dtype, "", slab, ("silu_bwd.cols", ncb, 1), True)
    run_silu(monkeypatch, M, SILU_PAIR, dtype, "", 2 * slab, ("silu_bwd.cols", ncb, 2 if M > 16 else 1))
    run_silu(monkeypatch, M, SILU_PAIR, dtype, "", slab - 1, ("silu_bwd.wave", _km(max(SILU_PAIR)), (M + 3) // 4))   # less than one split: the wave form


# ------------------------------------------------------------------------------------------------ sea_ib_bwd
IB_MLP = [(8, 8, "ib_bwd.fast", 1), (1, 256, "ib_bwd.fast", 1), (8, 260, "ib_bwd.fast", 4), (8, 1024, "ib_bwd.fast", 4),
          (8, 1028, "ib_bwd.wave", 0), (64, 8, "ib_bwd.wave", 0), (9, 256, "ib_bwd.wave", 0)]   # (h, E, form, a)
IB_LINEAR_E = (8, 264, 2048)
IB_MS = (1, 5, 65)
IB_FIELDS = (1, 3)
IB_DROP = (1234, 5, 26)   # (seed, first stream, thr): field f draws stream 5 + f, about a tenth of the elements dropped
IB_NAMES = ("dw1", "db1", "dlnw", "dlnb", "dw2", "db2")


def ib_operands(mode, h, E, M, F, device=None):
    kw = dict(device=device)
    seed = 90000 + 1000 * mode + 31 * E + 7 * h + 3 * M + F
    g = torch.Generator(device="cpu").manual_seed(seed)
    c = (0.2 + 0.8 * torch.rand(M, generator=g)).to(device if device is not None else dev())
    o = dict(mode=mode, h=h, E=E, M=M, c=c, dX=[rnd(M, E, seed=seed + 20 + f, **kw) for f in range(F)])
    if mode == 0:
        o.update(w1=rnd(h, seed=seed + 1, **kw), b1=0.1 * rnd(h, seed=seed + 2, **kw), lnw=1 + 0.1 * rnd(h, seed=seed + 3, **kw), lnb=0.1 * rnd(h, seed=seed + 4, **kw),
                 w2=0.3 * rnd(E, h, seed=seed + 5, **kw))
        shapes = dict(dw1=(h,), db1=(h,), dlnw=(h,), dlnb=(h,), dw2=(E, h), db2=(E,))
    else:
        shapes = dict(dw1=(E,), db1=(E,))
    o["old"] = {k: rnd(*s, seed=seed + 40 + i, **kw) for i, (k, s) in enumerate(shapes.items())}
    return o


def ib_reference(g, masks=None):
    """SeaIbBwdParams in fp64: {name: (sum of the terms, their absolute sum, number of terms, first-order error of the terms' own fp32 arithmetic)}.
    masks: per field keep * scale as sea_dropout_mask writes it (None: no dropout).  The D... quantities bound, to first order, the error of the fp32 evaluation of
    the quantity they are named after: L u per level of a sum of h values, (E F + 2) u for the dot product over columns and fields, EPS_AS for GELU and GELU'."""
    c = g["c"].double()
    M, F = c.shape[0], len(g["dX"])
    v = [x.double() * (m.double() if m is not None else 1.0) for x, m in zip(g["dX"], masks if masks is not None else [None] * F)]
    dib, adib = sum(v), sum(t.abs() for t in v)   # [M, E]
    ca = c.abs()[:, None]
    if g["mode"] == 1:
        return {"dw1": ((c[:, None] * dib).sum(0), (ca * adib).sum(0), M * F, None), "db1": (dib.sum(0), adib.sum(0), M * F, None)}
    w1, b1, lw, lb, W2 = (g[k].double() for k in ("w1", "b1", "lnw", "lnb", "w2"))
    h, E = w1.numel(), W2.shape[0]
    L = math.log2(h) + 1
    pre = c[:, None] * w1 + b1
    mu = pre.mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((pre - mu) ** 2).mean(1, keepdim=True) + 1e-5)
    xh = (pre - mu) * rstd
    u_ = xh * lw + lb
    hid, gp, gpp = gelu64(u_), gelu_grad64(u_), gelu_grad2_64(u_)
    dhid, adhid = dib @ W2, adib @ W2.abs()
    du = dhid * gp
    dxh = du * lw
    c1, c2 = dxh.mean(1, keepdim=True), (dxh * xh).mean(1, keepdim=True)
    dpre = rstd * (dxh - c1 - xh * c2)
    Dx = U * ((4 + L) * rstd * pre.abs().amax(1, keepdim=True) + (8 + L) * xh.abs())
    if h == 1:   # one hidden unit: pre - mean(pre) is exactly zero in fp32 as in fp64, so xhat carries no error (and rstd = 1e-5^-1/2 would blow the term up)
        Dx = torch.zeros_like(Dx)
    Du = lw.abs() * Dx + 2 * U * ((xh * lw).abs() + lb.abs())
    Dhid = gp.abs() * Du + 0.5 * EPS_AS * u_.abs() + U * hid.abs()   # gelu_erf = x (1 + erf) / 2: the erf's error enters times |x| / 2
    Ddu = gp.abs() * (math.sqrt(E * F) + 2) * U * adhid + dhid.abs() * (gpp.abs() * Du + EPS_AS) + U * du.abs()
    Ddxh = lw.abs() * Ddu + U * dxh.abs()
    Dc1 = Ddxh.mean(1, keepdim=True) + L * U * dxh.abs().mean(1, keepdim=True)
    Dc2 = (Ddxh * xh.abs() + dxh.abs() * Dx).mean(1, keepdim=True) + (L + 2) * U * (dxh * xh).abs().mean(1, keepdim=True)
    Ddpre = rstd * (Ddxh + Dc1 + xh.abs() * Dc2 + c2.abs() * Dx) + (8 + L) * U * rstd * (dxh.abs() + c1.abs() + (xh * c2).abs())
    return {"db2": (dib.sum(0), adib.sum(0), M * F, None),
            "dw2": (dib.t() @ hid, adib.t() @ hid.abs(), M * F, adib.t() @ Dhid),
            "dlnw": ((du * xh).sum(0), (du * xh).abs().sum(0), M, (xh.abs() * Ddu + du.abs() * Dx).sum(0)),
            "dlnb": (du.sum(0), du.abs().sum(0), M, Ddu.sum(0)),
            "dw1": ((dpre * c[:, None]).sum(0), (dpre * c[:, None]).abs().sum(0), M, (ca * Ddpre).sum(0)),
            "db1": (dpre.sum(0), dpre.abs().sum(0), M, Ddpre.sum(0))}


def ib_masks(M, E, F, drop):
    from sea_amd import _native as N

    seed, stream, thr = drop
    masks = []
    for f in range(F):
        mk = torch.empty(M, E, device=dev())
        N.check(N.lib().sea_dropout_mask(mk.data_ptr(), M, E, seed, stream + f, thr, N.stream_ptr()), "sea_dropout_mask")
        masks.append(mk)
    assert all(0 < int((m == 0).sum()) < m.numel() for m in masks) or M * E < 64
    return masks


def run_ib(monkeypatch, mode, h, E, M, F, tune, expect, drop=None, cols_splits=0, strided=False):
    import ctypes

    from sea_amd import _native as N
    from sea_amd import ops

    g = ib_operands(mode, h, E, M, F)
    ref = ib_reference(g, ib_masks(M, E, F, drop) if drop else None)
    outs = {k: filled(tuple(o.shape), F32, o) for k, o in g["old"].items()}
    if strided:   # the fields: column slices of one buffer, as the fused exchange gradient leaves them
        big = torch.full((M + 4, F * E + 16), NAN, device=dev())
        dxs = [big[:M, 8 + f * E:8 + (f + 1) * E] for f in range(F)]
        for d_, x in zip(dxs, g["dX"]):
            d_.copy_(x)
    else:
        dxs = [inp(x, True) for x in g["dX"]]
    layer = {k: g[k] for k in ("w1", "b1", "lnw", "lnb", "w2")} if mode == 0 else {}
    wsf = dh = None
    if cols_splits:
        wsf, ws = guarded((cols_splits * E * (1 + h),), F32)
        dh = torch.zeros(M, 8, device=dev())
        layer.update(ws=ws, dhid=dh)
    P = N.SeaIbBwdParams()
    ops.fill_ib_bwd_params(P, dxs, tall(g["c"], 4), mode=mode, drop=drop, **layer, **{k: o[1] for k, o in outs.items()})
    force(monkeypatch, tune)
    N.check(N.lib().sea_ib_bwd(ctypes.byref(P), N.stream_ptr()), "sea_ib_bwd")
    got = launched(ops, expect[0])
    assert got == expect, (got, expect)
    what = f"ib_bwd mode {mode} h={h} E={E} M={M} F={F} drop={drop is not None} {tune} {got[0]}"
    for k, (flat, v) in outs.items():
        s, a, n, extra = ref[k]
        check_colsum("ib." + ("lin_" if mode == 1 else "") + k, v, g["old"][k], s, a, n, what, extra)
        assert guard_untouched(flat), (what, k, "guard")
    if wsf is not None:
        assert guard_untouched(wsf), (what, "workspace guard")
        assert float(dh.abs().max()) == 0 or E <= 256, (what, "dhid is not left zero")


@pytest.mark.parametrize("h,E,form,a", IB_MLP, ids=str)
def test_ib_bwd_mlp_parameter_gradients(monkeypatch, h, E, form, a):
    """The one-wave-per-row kernels (register forms KE = 1 / 4, the generic one) against fp64: every M and field count, with dropout on the layer's output, a wave
    walking several rows (2 workgroups for 65 rows).  (8, 1028) and (64, 8) are the cases at which the generic kernel's dW2 was wrong by its own size while its
    column loop had a lane-dependent bound: in the last, partial chunk of 256 columns it read hid_k from lanes that were not running.)"""
    for M in IB_MS:
        for F in IB_FIELDS:
            run_ib(monkeypatch, 0, h, E, M, F, "", (form, a, (M + 3) // 4), strided=F == 3)
        run_ib(monkeypatch, 0, h, E, M, 3, "", (form, a, (M + 3) // 4), drop=IB_DROP)
    run_ib(monkeypatch, 0, h, E, 65, 3, "ibbwd_blocks=2", (form, a, 2), drop=IB_DROP)
    run_ib(monkeypatch, 0, h, E, 65, 1, "ibbwd_blocks=2", (form, a, 2))


@pytest.mark.parametrize("E", IB_LINEAR_E)
def test_ib_bwd_linear_parameter_gradients(monkeypatch, E):
    for M in IB_MS:
        for F in IB_FIELDS:
            run_ib(monkeypatch, 1, 0, E, M, F, "", ("ib_bwd.linear", (M + 63) // 64, 0), strided=F == 3)


@pytest.mark.parametrize("drop", [None, IB_DROP], ids=["plain", "dropout"])
def test_ib_bwd_column_block_trio(monkeypatch, drop):
    """ib_bwd_cols / ib_bwd_rows / ib_bwd_finish (two column blocks, five row splits of 13 rows) against fp64, with and without dropout; ibbwd_cols=0 sends the same
    arguments to the register form."""
    run_ib(monkeypatch, 0, 8, 260, 65, 3, "", ("ib_bwd.cols", 2, 5), drop=drop, cols_splits=5)
    run_ib(monkeypatch, 0, 8, 260, 65, 3, "ibbwd_cols=0", ("ib_bwd.fast", 4, 17), drop=drop, cols_splits=5)


# ------------------------------------------------------------------------------------------------ the emulation behind LOCAL, on the CPU
def emulation_cases(device="cpu", cases=None):
    """Yields (what, {kind: (reference, emulation, exact)}) for every bf16 rownorm launch of this file (the only launches with rounded row outputs)."""
    for pattern, dtype, M, d, n in (norm_cases() if cases is None else cases):
        if dtype != BF:
            continue
        gelu = PATTERNS[pattern][2]
        for i, g in enumerate(norm_operands(pattern, dtype, M, d, n, device=device)):
            ref, emu, exact = norm_bwd_formula(g, gelu), norm_bwd_formula(g, gelu, BF, poly=True), norm_bwd_formula(g, gelu, None, poly=False)
            out, at4 = {}, "@4" if d == 4 else ""
            if g["sp"]["dxact"]:
                out[("dXact.gelu" if gelu else "dXact") + at4] = (ref["dXact"], emu["dXact"], exact["dXact"])
            if g["sp"]["mod"]:
                out["dmod" + at4] = (ref["dmod"], emu["dmod"], exact["dmod"])
            yield f"rownorm_bwd {pattern} M={M} d={d} group {i}", out


def measure_local(device="cpu", verbose=True, cases=None):
    """{kind: (largest rowerr(emulation, reference), its case)}; asserts that the emulation without rounding restates the reference to 1e-12."""
    worst = {k: (0.0, "") for k in LOCAL}
    for what, outs in emulation_cases(device, cases):
        line = []
        for kind, (ref, emu, exact) in outs.items():
            assert float((exact - ref).norm()) <= 1e-12 * max(float(ref.norm()), 1.0), (what, kind)
            e = rowerr(emu, ref)
            line.append(f"{kind} local {e:.3e} (global {rel(emu, ref):.3e})")
            if e > worst[kind][0]:
                worst[kind] = (e, what)
        if verbose:
            print(f"{what}: " + "  ".join(line))
    return worst


if __name__ == "__main__":
    for kind, (v, what) in measure_local().items():
        print(f"{kind}: measured {v:.3e} at {what}; LOCAL = 3 * {LOCAL[kind] / 3:.3e}")
    ep, ee = measure_eps()
    print(f"EPS_POLY: measured {ep:.3e}; EPS_POLY = {EPS_POLY:.3e}")
    print(f"EPS_ERF: measured {ee:.3e}; EPS_ERF = {EPS_ERF:.3e}")
