"""The few-row kernels of the shipped-width rollout step — sea_gemm_fewrows / sea_qkv_rope_fewrows (gemv.hip), gemm_skinny / gemm_skinny_long / qkv_skinny behind
sea_gemm_grouped / sea_qkv_rope_grouped (gemm.hip), the one-row attention at head dims 128 / 256 (attention.hip) and sea_rownorm's workgroup-per-row kernel
(rowops.hip) — per row and per element against fp64, in the discipline of test_row_launches_gpu.py.

Reference: the fp64 formula of include/sea_hip.h on the operands as rounded to bf16 / fp32, NO intermediate rounded.  Three checks per output:

  global   ||out - ref|| / ||ref||: 2e-5 an fp32 output with nothing rounded upstream (3e-5 for K > 2048), 4e-3 the bf16 Cact / Z of a plain GEMM, 6e-3 a bf16
           output behind GELU or a norm and Q / K / V, 8e-3 the bf16 attention O, 6e-3 / 1e-5 sea_rownorm in bf16 / fp32.  An fp32 output BEHIND an in-kernel
           rounding (C32 behind a prologue's rounded A) takes the bound of the bf16 output of the same launch.
  local    max over rows ||err_row|| / rms over rows ||ref_row|| (rowerr).  Rows are short: a GEMM output row has at most 50 columns, Q / K / V are a row per head,
           sea_rownorm's outputs 64-column chunks, mean / rstd one row, attention O a row per (trajectory, head).  fp32 outputs with nothing rounded upstream:
           4 x their global bound.  Every other output: LOCAL, 3 x the largest rowerr(emulation, reference) over every case of this file, where the emulation is
           the same fp64 formula with a rounding to bf16 exactly where the kernels round (the normalised A rows of a prologue, behind the GELU of the
           activation-row prologue; the outputs); with the rounding off it restates the reference to 1e-12.  Measured on the CPU by
           `python tests/test_fewrow_launches_gpu.py`.  spread(ref) <= 3 is asserted on every reference.
  element  launches with no in-kernel rounded operand (plain A, no prologue): every fp32 element |out - ref| <= 2e-4 + 1e-4 |ref|, every bf16 element
           |out - ref| <= 2^-8 |ref| + 2e-4 (one bf16 ulp — twice the rounding — plus the fp32 part).  GEMM operands are scaled so that the output rms of a launch,
           pooled over its plain-A groups, lies in [0.5, 3] (asserted): one 8-element piece dropped from a K = 16384 contraction then moves an element by ~2 % of its scale.

Every launch: outputs in NaN frames with a row stride above N, A the first M rows of a taller NaN tensor with lda > K, W the first N rows of a taller NaN tensor,
R and mod strided views, caches pre-filled with NaN (outside [pos0, pos0 + T) still NaN afterwards, inside finite), K / V^T beyond the visible keys NaN,
ops.last_form() asserted right after the launch, and one group of every multi-group launch relaunched alone (same instantiation) bit for bit."""
import os
import sys

import pytest
import torch

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests.test_forced_forms_gpu import BF, attention_ref64, dev, frame_untouched, framed, gelu64, rel, rnd, rope64, rope_table, rowerr, spread  # noqa: E402
from tests.test_row_launches_gpu import guard_untouched, guarded, ln64, modulate, rounder, tall  # noqa: E402

pytestmark = pytest.mark.gpu

NAN = float("nan")
F32 = torch.float32
# 3 x the largest rowerr(emulation, reference) over every case of the file (python tests/test_fewrow_launches_gpu.py, on the CPU); the measured value and its case:
LOCAL = {
    "gemv.Cact": 3 * 2.497e-03,   # gemv plain M=3 K=512 group 0
    "gemv.Z": 3 * 2.335e-03,   # gemv plain M=4 K=512 group 1
    "pre.C32": 3 * 2.119e-03,   # gemv prologue M=3 K=1024 variant adaln group 0
    "pre.Cact": 3 * 2.978e-03,   # gemv prologue M=3 K=1024 variant adaln group 0
    "act.C32": 3 * 1.459e-03,   # gemv activation rows M=1 K=2048 gelu=False group 2
    "act.Cact": 3 * 2.404e-03,   # gemv activation rows M=3 K=4096 gelu=False group 2
    "qkv.Q": 3 * 4.175e-03,   # gemv qkv M=1 K=2048 H=3 hd=6 cross B=1 T=1 pos0=0 pro=ln
    "qkv.K": 3 * 4.040e-03,   # gemv qkv M=4 K=1024 H=3 hd=6 self B=2 T=2 pos0=0 pro=adaln
    "qkv.V": 3 * 5.385e-03,   # gemv qkv M=4 K=512 H=3 hd=6 self B=4 T=1 pos0=0 pro=adaln
    "skinny.Cact": 3 * 3.713e-03,   # skinny M=16 Ks=(384, 512, 1024) group 0
    "skinny.Z": 3 * 3.009e-03,   # skinny M=17 Ks=(512, 512, 512) group 1
    "skinny.Cgelu": 3 * 3.445e-03,   # skinny long M=16 Ks=(6144, 6144, 6144, 2048) act=True group 1
    "sqkv.Q": 3 * 3.104e-03,   # qkv skinny hd=16 B=16 T=1 K=128 pos0=3 cross
    "sqkv.K": 3 * 3.138e-03,   # qkv skinny hd=16 B=2 T=8 K=2048 pos0=0 cross
    "sqkv.V": 3 * 3.896e-03,   # qkv skinny hd=8 B=3 T=5 K=384 pos0=3 cross
    "attn.O": 3 * 2.230e-03,   # attention row hd=256 nk=9 causal problem 1
    "rn.Yact": 3 * 4.039e-03,   # rownorm act_gelu M=32 d=16388 group 0
}
GLOBAL = {"gemv.Cact": 4e-3, "gemv.Z": 4e-3, "pre.C32": 6e-3, "pre.Cact": 6e-3, "act.C32": 6e-3, "act.Cact": 6e-3, "qkv.Q": 6e-3, "qkv.K": 6e-3, "qkv.V": 6e-3,
          "skinny.Cact": 4e-3, "skinny.Z": 4e-3, "skinny.Cgelu": 6e-3, "sqkv.Q": 6e-3, "sqkv.K": 6e-3, "sqkv.V": 6e-3, "attn.O": 8e-3, "rn.Yact": 6e-3}
ELEM_F32 = (2e-4, 1e-4)       # |out - ref| <= 2e-4 + 1e-4 |ref|: what test_fewrows_gpu.py holds C32 to
ELEM_BF16 = (2e-4, 2.0 ** -8)
RMS_RANGE = (0.5, 3.0)


# ------------------------------------------------------------------------------------------------ helpers
def nan_rows(t, extra=4, pad=64):
    """t as the first rows and columns of a NaN tensor `extra` rows taller and `pad` columns wider: a row stride above the row length."""
    big = torch.full((t.shape[0] + extra, t.shape[1] + pad), NAN, device=t.device, dtype=t.dtype)
    big[:t.shape[0], :t.shape[1]] = t
    return big[:t.shape[0], :t.shape[1]]


def strided(t, left=8, right=8):
    """t as columns [left, left + N) of a wider NaN tensor."""
    big = torch.full((t.shape[0], t.shape[1] + left + right), NAN, device=t.device, dtype=t.dtype)
    big[:, left:left + t.shape[1]] = t
    return big[:, left:left + t.shape[1]]


def chunks(t, n=64):
    """[M, d] -> rows of n columns (the last chunk of a row padded with zeros)."""
    M, d = t.shape
    pad = (-d) % n
    if pad:
        t = torch.cat((t.double(), torch.zeros(M, pad, device=t.device, dtype=torch.float64)), dim=1)
    return t.reshape(-1, n)


def elem_excess(out, ref):
    """max over the elements of |out - ref| / (atol + rtol |ref|) at the element bound of out's type: <= 1 passes."""
    atol, rtol = ELEM_F32 if out.dtype == F32 else ELEM_BF16
    return float(((out.double() - ref).abs() / (atol + rtol * ref.abs())).max())


def rms(t):
    return float(t.double().pow(2).mean().sqrt())


_SEEN = {}   # kind -> [worst global, worst local, checks, global bound, local bound, worst element excess] of the running test


def errors(out, ref, row=None):
    """(global, local) error of one output; row: the row length (a row per head; rownorm: 64-column chunks of the rows), None: the output's own rows."""
    if row is None:
        return rel(out, ref), rowerr(out, ref)
    if out.dim() == 2:
        return rel(out, ref), rowerr(chunks(out, row), chunks(ref, row))
    return rel(out, ref), rowerr(out.reshape(-1, row), ref.reshape(-1, row))


def bounds(kind, f32=False, g32=2e-5):
    return (g32, 4 * g32) if f32 else (GLOBAL[kind], LOCAL[kind])


def check(kind, out, ref, what, row=None, f32=False, g32=2e-5, elem=False):
    """The checks of one output.  f32: an fp32 output with nothing rounded upstream (global g32, local 4 g32); elem: the element check."""
    assert torch.isfinite(out.float()).all(), (what, kind, "not finite")
    rr = ref if row is None else (chunks(ref, row) if ref.dim() == 2 else ref.reshape(-1, row))
    assert spread(rr) <= 3.0, (what, kind, "spread", spread(rr))
    eg, el = errors(out, ref, row)
    gb, lb = bounds(kind, f32, g32)
    ee = elem_excess(out, ref) if elem else 0.0
    print(f"{what} {kind}: global {eg:.3e} (< {gb:.1e})  local {el:.3e} (< {lb:.3e})" + (f"  element {ee:.3f} (<= 1)" if elem else ""))
    w = _SEEN.setdefault(kind, [0.0, 0.0, 0, gb, lb, 0.0])
    w[0], w[1], w[2], w[3], w[4], w[5] = max(w[0], eg), max(w[1], el), w[2] + 1, max(w[3], gb), max(w[4], lb), max(w[5], ee)
    assert eg < gb, (what, kind, "global", eg, gb)
    assert el < lb, (what, kind, "local", el, lb)
    assert ee <= 1.0, (what, kind, "element", ee)


@pytest.fixture(autouse=True)
def _one_line_per_test(request):
    """The line of profiles/fewrow_launches_gpu_errors.txt: the largest global, local and element error of every output kind the test checked, beside their bounds."""
    _SEEN.clear()
    yield
    if torch.cuda.is_available():
        try:
            torch.cuda.synchronize()
        except RuntimeError as e:   # a device fault inside the test body: no further test is started on this device
            pytest.exit(f"device error in {request.node.name}: {e}", returncode=3)
    if _SEEN:
        print("FEWROW_LAUNCHES " + request.node.name + ": " + "; ".join(
            f"{k} global {w[0]:.3e} (< {w[3]:.1e}) local {w[1]:.3e} (< {w[4]:.3e})" + (f" element {w[5]:.3f} (<= 1)" if w[5] > 0 else "") + f" over {w[2]}"
            for k, w in sorted(_SEEN.items())))


def launched(ops, form):
    """ops.last_form() right after the launch, before the synchronise; form: the name, or the whole (name, a, b)."""
    got = ops.last_form()
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:   # a device fault: nothing more is started on this device
        pytest.exit(f"device error behind {got}: {e}", returncode=3)
    assert (got[0] == form) if isinstance(form, str) else (got == tuple(form)), (form, got)
    return got


def same(a, b):
    """Bitwise equality of two tensors that may hold NaN frames."""
    return a.shape == b.shape and torch.equal(a.nan_to_num(12345.0), b.nan_to_num(12345.0))


def refused(ops, call, outs):
    """`call` raises before anything is launched: no form is noted, every output is still NaN."""
    before = ops.last_form()
    with pytest.raises((RuntimeError, ValueError)):
        call()
    torch.cuda.synchronize()
    assert ops.last_form() == before
    assert all(bool(torch.isnan(o.float()).all()) for o in outs)


# ------------------------------------------------------------------------------------------------ GEMM groups: sea_gemm_fewrows and the skinny kernels
GEMV_KS = (512, 1024, 2048, 4096, 8192, 16384)
GEMV_MR = {1: 1, 2: 2, 3: 4, 4: 4}
GEMV_NS = (33, 16, 50)   # 4 CW columns per block: a ragged block of one column, exactly one block at CW = 4 (whole blocks at CW = 2 / 1), a ragged block of two
# epilogues: 0 bias x 2 + R -> C32, Cact; 1 act = 1 -> Z, C32; 2 -> Cact; 3 act = 1 -> Z, C32, Cact; 4 bias -> C32, Cact
EPI_OUTS = {0: ("C32", "Cact"), 1: ("Z", "C32"), 2: ("Cact",), 3: ("Z", "C32", "Cact"), 4: ("C32", "Cact")}
PRE_VARIANTS = ("gamma", "ln", "adaln", "adaln_add")


def pre_rows(M, K, variant, seed, device=None):
    """The fp32 rows of a norm prologue and its operands (SeaNormGroup): gamma only / gamma + beta / mod + beta (AdaLN) / AdaLN + addend (+ Xout at the launch)."""
    kw = dict(device=device)
    p = dict(X=nan_rows(rnd(M, K, seed=seed + 1, **kw) * 1.3 + 0.2), gamma=1 + 0.1 * rnd(K, seed=seed + 2, **kw), beta=None, mod=None, addend=None, gelu=False)
    if variant != "gamma":
        p["beta"] = 0.1 * rnd(K, seed=seed + 3, **kw)
    if variant in ("adaln", "adaln_add"):
        p["mod"] = strided(rnd(M, 2 * K, dtype=BF, scale=0.3, seed=seed + 4, **kw))
    if variant == "adaln_add":
        p["addend"] = nan_rows(0.5 * rnd(M, K, seed=seed + 5, **kw), 4, 32)
    return p


def act_rows(M, K, gelu, seed, device=None):
    """Hidden rows in bf16 (ldx = K + 64) with a plain LayerNorm (+ GELU) as the prologue."""
    kw = dict(device=device)
    return dict(X=nan_rows(rnd(M, K, dtype=BF, seed=seed + 1, **kw) * 1.2 + 0.2), gamma=1 + 0.1 * rnd(K, seed=seed + 2, **kw), beta=0.1 * rnd(K, seed=seed + 3, **kw), mod=None,
                addend=None, gelu=gelu)


def gemm_group(M, N_, K, epi, seed, pre=None, device=None):
    """One group: A ~ N(0, 1) (first M rows of a taller NaN tensor, lda = K + 64) or the prologue `pre`, W ~ N(0, 1 / K) (first N rows of a taller NaN tensor),
    bias and R ~ N(0, 1) (R a strided view)."""
    kw = dict(device=device)
    g = dict(M=M, N=N_, K=K, epi=epi, pre=pre, A=(nan_rows(rnd(M, K, dtype=BF, seed=seed + 1, **kw)) if pre is None else None),
             W=tall(rnd(N_, K, dtype=BF, scale=K ** -0.5, seed=seed + 2, **kw), 4), bias=None, R=None, act=int(epi in (1, 3)), bias_scale=1.0)
    if epi in (0, 4):
        g["bias"] = rnd(N_, seed=seed + 3, **kw)
    if epi == 0:
        g.update(bias_scale=2.0, R=strided(rnd(M, N_, seed=seed + 4, **kw)))
    return g


def a_operand(g, r):
    """The A rows of a group in fp64: the operand itself, or the prologue's rows — rounded (r) where the kernel rounds them, behind the GELU."""
    p = g["pre"]
    if p is None:
        return g["A"].double()
    x = p["X"].double() + (p["addend"].double() if p["addend"] is not None else 0.0)
    y = modulate(ln64(x)[0], p["gamma"], p["beta"], p["mod"])
    return r(gelu64(y) if p["gelu"] else y)


def gemm_formula(g, rt=None):
    """{"Z", "C32", "Cact"} of one group.  Rounded where the kernels round: the prologue's A rows; the bf16 outputs."""
    r = rounder(rt)
    v = a_operand(g, r) @ g["W"].double().t()
    if g["bias"] is not None:
        v = v + g["bias_scale"] * g["bias"].double()
    out = {}
    if g["act"]:
        out["Z"] = r(v)
        v = gelu64(v)
    if g["R"] is not None:
        v = v + g["R"].double()
    out["C32"], out["Cact"] = v, r(v)
    return {k: out[k] for k in EPI_OUTS[g["epi"]]}


def gemm_kind(prefix, g, k):
    return prefix + "." + ("Cgelu" if k == "Cact" and g["act"] else k)


def gemm_launch_dict(g):
    """(launch dict, prologue dict or None, {output: (frame, view)}): every output NaN in a frame."""
    o = {k: framed(g["M"], g["N"], F32 if k == "C32" else BF) for k in EPI_OUTS[g["epi"]]}
    d = dict(A=g["A"], W=g["W"], bias=g["bias"], R=g["R"], act=g["act"], bias_scale=g["bias_scale"], **{k: v[1] for k, v in o.items()})
    p = None
    if g["pre"] is not None:
        p = {k: g["pre"][k] for k in ("X", "gamma", "beta", "mod", "addend")}
        if p["addend"] is not None:
            o["Xout"] = framed(g["M"], g["K"], F32)
            p["Xout"] = o["Xout"][1]
    return d, p, o


def gemm_check(prefix, g, o, what):
    """Every output of one group against its reference; plain A: C32 is an fp32 output with nothing rounded upstream, and every element is held."""
    ref = gemm_formula(g)
    plain = g["pre"] is None
    for k, r_ in ref.items():
        if k == "C32" and plain:
            check(prefix + ".C32", o[k][1], r_, what, f32=True, g32=(2e-5 if g["K"] <= 2048 else 3e-5), elem=True)
        else:
            check(gemm_kind(prefix if plain else g["pre_kind"], g, k), o[k][1], r_, what, elem=plain)
        assert frame_untouched(o[k][0], g["N"]), (what, k, "frame")
    if "Xout" in o:
        p = g["pre"]
        assert torch.equal(o["Xout"][1], p["X"] + p["addend"]), (what, "Xout is not X + addend bit for bit")
        assert frame_untouched(o["Xout"][0], g["K"]), (what, "Xout frame")


def launch_rms(groups):
    """The rms of the plain-A outputs of one launch, pooled over its groups (a group of 4 x 1 elements has no rms of its own): the scale the absolute part of the
    element bound is set against."""
    v = torch.cat([gemm_formula(g)["Cact" if "Cact" in EPI_OUTS[g["epi"]] else "C32"].reshape(-1) for g in groups if g["pre"] is None])
    return rms(v)


def assert_scaled(groups, what):
    assert RMS_RANGE[0] <= launch_rms(groups) <= RMS_RANGE[1], (what, "output rms", launch_rms(groups))


def gemv_plain_groups(M, K, device=None):
    """Three groups of N = (33, 16, 50) with M = (M, 1, M) rows: mixed row counts in one launch; epilogues 0, 1, 2."""
    return [gemm_group(m, N_, K, i, 9000 + 1000 * i + 10 * M + K, device=device) for i, (m, N_) in enumerate(zip((M, 1, M), GEMV_NS))]


def gemv_pre_groups(M, K, variant, device=None):
    """A prologue group, a plain-A group of one row (pre[i] = None) and a second prologue group, in one launch."""
    vi = PRE_VARIANTS.index(variant)
    gs = [gemm_group(M, 33, K, 4, 9100 + 7 * vi + 10 * M + K, pre=pre_rows(M, K, variant, 9150 + 7 * vi + 10 * M + K, device), device=device),
          gemm_group(1, 16, K, 4, 9200 + 7 * vi + 10 * M + K, device=device),
          gemm_group(M, 50, K, 0, 9300 + 7 * vi + 10 * M + K, pre=pre_rows(M, K, variant, 9350 + 7 * vi + 10 * M + K, device), device=device)]
    for g in gs:
        g["pre_kind"] = "pre"
    return gs


def gemv_act_groups(M, K, gelu, device=None):
    gs = [gemm_group(M, 33, K, 0, 9400 + gelu + 10 * M + K, pre=act_rows(M, K, gelu, 9450 + gelu + 10 * M + K, device), device=device),
          gemm_group(1, 16, K, 4, 9500 + gelu + 10 * M + K, device=device),
          gemm_group(M, 50, K, 4, 9600 + gelu + 10 * M + K, pre=act_rows(M, K, gelu, 9650 + gelu + 10 * M + K, device), device=device)]
    for g in gs:
        g["pre_kind"] = "act"
    return gs


def _gemv_run(groups, form, what, **kw):
    """One sea_gemm_fewrows launch of `groups`, checked; then its last group alone — same rows, same K: the same instantiation — bit for bit."""
    from sea_amd import ops

    assert_scaled(groups, what)
    built = [gemm_launch_dict(g) for g in groups]
    x_before = [g["pre"]["X"].clone() if g["pre"] is not None else None for g in groups]
    pre = [b[1] for b in built]
    ops.gemm_fewrows([b[0] for b in built], BF, pre=(pre if any(p is not None for p in pre) else None), **kw)
    launched(ops, form)
    for i, (g, (_, _, o)) in enumerate(zip(groups, built)):
        gemm_check("gemv", g, o, f"{what} group {i}")
        if x_before[i] is not None:
            assert torch.equal(g["pre"]["X"], x_before[i]), (what, i, "X changed")
    d, p, o = gemm_launch_dict(groups[-1])
    ops.gemm_fewrows([d], BF, pre=([p] if p is not None else None), **kw)
    launched(ops, form)
    assert all(same(o[k][0], built[-1][2][k][0]) for k in o), (what, "the last group alone differs from the same group inside the launch")


@pytest.mark.parametrize("K", GEMV_KS)
@pytest.mark.parametrize("M", [1, 2, 3, 4])
def test_gemm_fewrows_plain_every_instantiation(M, K):
    _gemv_run(gemv_plain_groups(M, K), ("gemv.gemm", GEMV_MR[M], K // 512), f"gemv plain M={M} K={K}")


@pytest.mark.parametrize("variant", PRE_VARIANTS)
@pytest.mark.parametrize("K", [512, 1024, 2048])
def test_gemm_fewrows_norm_prologue_of_fp32_rows(K, variant):
    for M in (1, 2, 3):
        _gemv_run(gemv_pre_groups(M, K, variant), ("gemv.gemm", GEMV_MR[M], K // 512), f"gemv prologue M={M} K={K} variant {variant}")


@pytest.mark.parametrize("gelu", [False, True])
@pytest.mark.parametrize("K", [512, 2048, 4096, 8192])
def test_gemm_fewrows_layernorm_prologue_of_activation_rows(K, gelu):
    for M in (1, 3):
        _gemv_run(gemv_act_groups(M, K, gelu), ("gemv.gemm", GEMV_MR[M], K // 512), f"gemv activation rows M={M} K={K} gelu={gelu}", pre_x_is_act=True, pre_gelu=gelu)


def test_gemm_fewrows_refusals():
    """Each raises before any launch: the outputs are still NaN and no form is noted."""
    from sea_amd import ops

    def group(M=1, K=512, pre=None, seed=9700):
        g = gemm_group(M, 16, K, 4, seed, pre=pre)
        return gemm_launch_dict(g)

    def run(built, dtype=BF, **kw):
        pre = [b[1] for b in built]
        outs = [v[1] for b in built for v in b[2].values()]
        refused(ops, lambda: ops.gemm_fewrows([b[0] for b in built], dtype, pre=(pre if any(p is not None for p in pre) else None), **kw), outs)

    run([group(K=4096, pre=pre_rows(1, 4096, "ln", 9701))])                                   # an fp32 prologue at K = 4096
    run([group(K=16384, pre=act_rows(1, 16384, False, 9702))], pre_x_is_act=True)             # an activation-row prologue at K = 16384
    b = group(pre=pre_rows(1, 512, "adaln_add", 9703))
    b[1]["Xout"] = b[1]["X"]                                                                  # Xout is X
    x = b[1]["X"].clone()
    run([b])
    assert torch.equal(b[1]["X"], x)
    run([group(pre=pre_rows(1, 512, "ln", 9704))], pre_gelu=True)                             # pre_gelu without pre_x_is_act
    run([group(M=5)])                                                                          # M = 5
    run([group(K=768)])                                                                        # K = 768
    run([group(K=512), group(K=1024, seed=9705)])                                              # groups of different K
    run([group(seed=9710 + i) for i in range(9)])                                              # 9 groups
    run([group()], dtype=F32)                                                                  # the fp32 dtype


# ------------------------------------------------------------------------------------------------ sea_qkv_rope_fewrows / qkv_skinny: q / k / v + rotary embedding + caches
QKV_HEADS = [(2, 128), (1, 256), (3, 6)]   # (3, 6): Ea = 18, N = 54 — a wave's four columns straddle q | k, k | v and head boundaries; the last block is ragged
QKV_FORMS = ("self", "cross", "v")
QKV_PROS = (None, "ln", "adaln")
QKV_POS0 = (0, 5)


def qkv_case(M, K, H, hd, form, B, T, pos0, pro, cap, seed, device=None, vout=False):
    """The groups of one launch — self: [q | k | v] in one group; cross: a q group and a k, v group (col0 = Ea) with another operand; v: col0 = 2 Ea — and the common
    part.  pro: None (plain A), "ln" or "adaln": the norm prologue of every group."""
    kw = dict(device=device)
    Ea = H * hd
    spans = {"self": [(0, 3 * Ea)], "cross": [(0, Ea), (Ea, 2 * Ea)], "v": [(2 * Ea, Ea)]}[form]
    groups = []
    for i, (col0, N_) in enumerate(spans):
        s = seed + 50 * i
        pre = pre_rows(M, K, pro, s + 10, device) if pro is not None else None
        groups.append(dict(M=M, N=N_, K=K, col0=col0, pre=pre, A=(nan_rows(rnd(M, K, dtype=BF, seed=s + 1, **kw)) if pre is None else None),
                           W=tall(rnd(N_, K, dtype=BF, scale=K ** -0.5, seed=s + 2, **kw), 4), bias=rnd(N_, seed=s + 3, **kw)))
    return dict(groups=groups, B=B, T=T, H=H, hd=hd, pos0=pos0, cap=cap, vout=vout, table=rope_table(hd, pos0 + T, device=device if device is not None else dev()))


def qkv_formula(g, c, rt=None):
    """{"Q", "K", "V"} [B, H, T, hd] of the parts a group's columns [col0, col0 + N) cover whole: projection, bias, the rotary pair of the table at pos0 + t on q and
    k, q_scale on q.  Rounded where the kernels round: the prologue's A rows; the outputs."""
    from sea_amd.ops import q_scale

    r = rounder(rt)
    B, T, H, hd = c["B"], c["T"], c["H"], c["hd"]
    Ea = H * hd
    y = a_operand(g, r) @ g["W"].double().t() + g["bias"].double()
    out = {}
    for name, lo in (("Q", 0), ("K", Ea), ("V", 2 * Ea)):
        if g["col0"] <= lo and lo + Ea <= g["col0"] + g["N"]:
            part = y[:, lo - g["col0"]:lo - g["col0"] + Ea].reshape(B, T, H, hd)
            if name != "V":
                part = rope64(part, c["table"], c["pos0"]) * (q_scale(hd) if name == "Q" else 1.0)
            out[name] = r(part).permute(0, 2, 1, 3)
    return out


def qkv_launch_dicts(c):
    """(launch dicts, prologue dicts or None, outputs): Q NaN, the caches NaN, each with NaN guards around it."""
    B, T, H, hd, cap = c["B"], c["T"], c["H"], c["hd"], c["cap"]
    Ea = H * hd
    ds, ps, os_ = [], [], []
    for g in c["groups"]:
        o = {}
        if g["col0"] < Ea:
            o["Q"] = guarded((B, H, T, hd), BF)
        if g["col0"] < 2 * Ea and g["col0"] + g["N"] > Ea:
            o["K"] = guarded((B, H, cap, hd), BF)
        if g["col0"] + g["N"] > 2 * Ea:
            o["Vt"] = guarded((B, H, hd, cap), BF)
            if c["vout"]:
                o["V"] = guarded((B, H, cap, hd), BF)
        ds.append(dict(A=g["A"], W=g["W"], bias=g["bias"], col0=g["col0"], **{k: v[1] for k, v in o.items()}))
        ps.append({k: g["pre"][k] for k in ("X", "gamma", "beta", "mod")} if g["pre"] is not None else None)
        os_.append(o)
    return ds, (ps if any(p is not None for p in ps) else None), os_


def cache_window(kind, cache, ref, pos0, T, hd, what, transposed=False, elem=False):
    """A cache [B, H, cap, hd] (transposed: [B, H, hd, cap]) that was NaN before the launch: positions [pos0, pos0 + T) against ref [B, H, T, hd], a row per head;
    every other position still NaN."""
    c = cache.transpose(2, 3) if transposed else cache
    assert bool(torch.isnan(c[:, :, :pos0].float()).all()) and bool(torch.isnan(c[:, :, pos0 + T:].float()).all()), (what, kind, "outside the window")
    check(kind, c[:, :, pos0:pos0 + T], ref, what, row=hd, elem=elem)


def qkv_check(prefix, c, os_, what):
    for i, (g, o) in enumerate(zip(c["groups"], os_)):
        ref, w, plain = qkv_formula(g, c), f"{what} group {i}", g["pre"] is None
        if "Q" in o:
            check(prefix + ".Q", o["Q"][1], ref["Q"], w, row=c["hd"], elem=plain)
        if "K" in o:
            cache_window(prefix + ".K", o["K"][1], ref["K"], c["pos0"], c["T"], c["hd"], w, elem=plain)
        if "Vt" in o:
            cache_window(prefix + ".V", o["Vt"][1], ref["V"], c["pos0"], c["T"], c["hd"], w, transposed=True, elem=plain)
        if "V" in o:
            cache_window(prefix + ".V", o["V"][1], ref["V"], c["pos0"], c["T"], c["hd"], w, elem=plain)
        assert all(guard_untouched(v[0]) for v in o.values()), (w, "guards")


def qkv_fewrows_cases(M, K):
    """(H, hd, form, B, T, pos0, prologue, Vout) of the launches of one (M, K): every head shape x form x (B, T) x pos0, the prologue rotating through them."""
    n = 0
    for H, hd in QKV_HEADS:
        for form in QKV_FORMS:
            for B, T in [(M, 1)] + ([(2, 2)] if M == 4 else []):
                for pos0 in QKV_POS0:
                    yield H, hd, form, B, T, pos0, QKV_PROS[(n + M + K // 512) % 3], (form == "v" and pos0 == 5)
                    n += 1


def qkv_fewrows_case(M, K, H, hd, form, B, T, pos0, pro, vout, device=None):
    return qkv_case(M, K, H, hd, form, B, T, pos0, pro, pos0 + T + 3, 10000 + 7 * M + K + 13 * hd + 100 * QKV_FORMS.index(form) + 3 * T + pos0, device, vout)


@pytest.mark.parametrize("K", [512, 1024, 2048])
@pytest.mark.parametrize("M", [1, 2, 4])
def test_qkv_rope_fewrows_against_the_formula(M, K):
    from sea_amd import ops

    for H, hd, form, B, T, pos0, pro, vout in qkv_fewrows_cases(M, K):
        c = qkv_fewrows_case(M, K, H, hd, form, B, T, pos0, pro, vout)
        what = f"gemv qkv M={M} K={K} H={H} hd={hd} {form} B={B} T={T} pos0={pos0} pro={pro}"
        ds, ps, os_ = qkv_launch_dicts(c)
        ops.qkv_rope_fewrows(ds, c["table"], H, hd, T, pos0, c["cap"], ops.q_scale(hd), BF, pre=ps)
        launched(ops, ("gemv.qkv", M, K // 512))
        qkv_check("qkv", c, os_, what)
        if len(ds) > 1:   # the k, v group alone
            d1, p1, o1 = qkv_launch_dicts(dict(c, groups=c["groups"][1:]))
            ops.qkv_rope_fewrows(d1, c["table"], H, hd, T, pos0, c["cap"], ops.q_scale(hd), BF, pre=p1)
            launched(ops, ("gemv.qkv", M, K // 512))
            assert all(same(o1[0][k][0], os_[1][k][0]) for k in o1[0]), (what, "the k, v group alone differs")


# ------------------------------------------------------------------------------------------------ gemm_skinny / gemm_skinny_long behind sea_gemm_grouped
SKINNY_KS = (128, 256, 384, 512, 1024, 1920, 2048)   # 1, 2, 3, 4, 8, 15, 16 steps per wave: every arm of the switch and its loop
SKINNY_NS = (4, 16, 44)
SKINNY_LONG_KS = (4096, 6144, 10240, 16384, 32768)   # 2, 3, 5, 8, 16 rounds of the two register sets
SKINNY_EPIS = (0, 3, 2)


def skinny_groups(M, Ks, epis=SKINNY_EPIS, device=None):
    """Groups of N = (4, 16, 44, 16 ...) with the contractions Ks."""
    return [gemm_group(M, (SKINNY_NS + (16,))[i], K, epis[i % len(epis)], 11000 + 1000 * i + 10 * M + K, device=device) for i, K in enumerate(Ks)]


def _skinny_run(groups, forms, what, alone=2):
    from sea_amd import ops

    assert_scaled(groups, what)
    built = [gemm_launch_dict(g) for g in groups]
    ops.gemm_grouped([b[0] for b in built], BF)
    got = ops.last_form()
    launched(ops, got)   # synchronises
    assert got[0] in forms, (what, forms, got)
    for i, (g, (_, _, o)) in enumerate(zip(groups, built)):
        gemm_check("skinny", g, o, f"{what} group {i} -> {got[0]}")
    if alone is not None:
        d, _, o = gemm_launch_dict(groups[alone])
        ops.gemm_grouped([d], BF)
        launched(ops, got[0])
        assert all(same(o[k][0], built[alone][2][k][0]) for k in o), (what, f"group {alone} alone differs from the same group inside the launch")


def skinny_short_cases():
    return [(M, tuple(SKINNY_KS[(j + i) % len(SKINNY_KS)] for i in range(3))) for M in (1, 5, 16) for j in range(len(SKINNY_KS))]


def skinny_long_cases():
    """(M, Ks, act): three groups of one long contraction; at K = 6144 a fourth group of K = 2048, one round."""
    return [(M, (K, K, K) + ((2048,) if K == 6144 else ()), act) for M in (1, 16) for K in SKINNY_LONG_KS for act in (False, True)]


@pytest.mark.parametrize("M", [1, 5, 16])
def test_gemm_skinny_every_step_count(M):
    for m, Ks in skinny_short_cases():
        if m == M:
            _skinny_run(skinny_groups(M, Ks), ("gemm.skinny",), f"skinny M={M} Ks={Ks}")


@pytest.mark.parametrize("K", SKINNY_LONG_KS)
def test_gemm_skinny_long_every_round_count(K):
    for M, Ks, act in skinny_long_cases():
        if Ks[0] == K:
            _skinny_run(skinny_groups(M, Ks, SKINNY_EPIS if act else (0, 4, 2)), ("gemm.skinny_long",), f"skinny long M={M} Ks={Ks} act={act}")


SKINNY_LEFT = [(17, (512, 512, 512)), (16, (2176, 2176, 2176))]


@pytest.mark.parametrize("M,Ks", SKINNY_LEFT)
def test_gemm_grouped_beside_the_skinny_rule_takes_a_tiled_form(M, Ks):
    _skinny_run(skinny_groups(M, Ks), ("gemm.tile64", "gemm.tile128"), f"beside skinny M={M} Ks={Ks}", alone=None)


SQKV_BT = [(1, 1), (3, 5), (16, 1), (2, 8)]
SQKV_KS = (128, 384, 2048)
SQKV_POS0 = (0, 3)
SQKV_H = 2


SQKV_TILE = [(3, 5, 384, 3, "cross", False), (1, 1, 128, 0, "self", True)]   # at head dim 8


def sqkv_cases(hd):
    """(B, T, K, pos0, form, Vout): the forms alternate."""
    if hd == 8:
        yield from SQKV_TILE
        return
    n = 0
    for B, T in SQKV_BT:
        for K in SQKV_KS:
            for pos0 in SQKV_POS0:
                yield B, T, K, pos0, QKV_FORMS[n % 3], n % 4 == 2
                n += 1


def sqkv_case(hd, B, T, K, pos0, form, vout, H=SQKV_H, device=None):
    return qkv_case(B * T, K, H, hd, form, B, T, pos0, None, (pos0 + T) // 8 * 8 + 8, 12000 + 17 * hd + 100 * B + 7 * T + K + pos0, device, vout)


def _sqkv_run(c, form, what):
    from sea_amd import ops

    ds, _, os_ = qkv_launch_dicts(c)
    ops.qkv_rope_grouped(ds, c["table"], c["H"], c["hd"], c["T"], c["pos0"], c["cap"], ops.q_scale(c["hd"]), BF)
    launched(ops, form)
    qkv_check("sqkv", c, os_, what)
    if len(ds) > 1:
        d1, _, o1 = qkv_launch_dicts(dict(c, groups=c["groups"][1:]))
        ops.qkv_rope_grouped(d1, c["table"], c["H"], c["hd"], c["T"], c["pos0"], c["cap"], ops.q_scale(c["hd"]), BF)
        launched(ops, form)
        assert all(same(o1[0][k][0], os_[1][k][0]) for k in o1[0]), (what, "the k, v group alone differs")


@pytest.mark.parametrize("hd", [16, 64, 128])
def test_qkv_skinny_against_the_formula(hd):
    for B, T, K, pos0, form, vout in sqkv_cases(hd):
        _sqkv_run(sqkv_case(hd, B, T, K, pos0, form, vout), "qkv.skinny", f"qkv skinny hd={hd} B={B} T={T} K={K} pos0={pos0} {form}")


def test_qkv_grouped_beside_the_skinny_rule_takes_the_tiled_form():
    """Head dim 8, and a group whose N is no multiple of 16 (q and the first 8 columns of k's head 0, at head dim 16)."""
    from sea_amd import ops

    for B, T, K, pos0, form, vout in sqkv_cases(8):
        _sqkv_run(sqkv_case(8, B, T, K, pos0, form, vout), "qkv.tile", f"qkv tile hd=8 B={B} T={T} K={K} pos0={pos0} {form}")
    B, T, K, pos0, H, hd = 3, 5, 384, 3, 2, 16
    c = sqkv_case(hd, B, T, K, pos0, "cross", False)
    g = c["groups"][1]                         # W of [k | v]: with q's it gives q and k of the full formula
    q = c["groups"][0]
    N_ = H * hd + 8
    W = tall(torch.cat((q["W"], g["W"][:8])), 4)
    bias = torch.cat((q["bias"], g["bias"][:8]))
    Q, Kc = guarded((B, H, T, hd), BF), guarded((B, H, c["cap"], hd), BF)
    ops.qkv_rope_grouped([dict(A=q["A"], W=W, bias=bias, col0=0, Q=Q[1], K=Kc[1])], c["table"], H, hd, T, pos0, c["cap"], ops.q_scale(hd), BF)
    launched(ops, "qkv.tile")
    assert W.shape[0] == N_ and N_ % 16 == 8
    what = "qkv tile N=40"
    check("sqkv.Q", Q[1], qkv_formula(q, c)["Q"], what, row=hd, elem=True)
    kref = qkv_formula(dict(g, A=q["A"]), c)["K"]
    win = Kc[1][:, 0, pos0:pos0 + T, :8]
    check("sqkv.K", win, kref[:, 0, :, :8], what, row=8, elem=True)
    rest = Kc[1].clone()
    rest[:, 0, pos0:pos0 + T, :8] = NAN
    assert bool(torch.isnan(rest.float()).all()) and guard_untouched(Q[0]) and guard_untouched(Kc[0]), what


# ------------------------------------------------------------------------------------------------ the one-row attention at head dims 128 / 256
ATTN_B, ATTN_H = 2, 3
ATTN_KPP = {128: 128, 256: 64}   # keys per pass: 512 threads / (hd / 32 lanes per key)
ATTN_LIMITS = ("causal", "Tk")


def attn_nks(hd):
    """Visible keys: the 8-key vector, the two-keys-per-iteration stride 2 KPP, the switch from the prefetched value rows (<= 512 keys in bf16) to the looped ones."""
    k = ATTN_KPP[hd]
    return sorted({1, 7, 8, 9, k - 1, k, k + 1, 2 * k, 2 * k + 1, 511, 512, 513, 520, 521, 1030})


def attn_problem(dtype, hd, nk, limit, i, device=None):
    """One problem with nk visible keys — limited by the causal rule (q_pos0 + src_len + 1 = nk < Tk) or by Tk (= nk) — every K row / V^T column beyond them NaN;
    O [B, 1, H hd] strided inside a NaN frame (GPU only).  Returns (problem, geometry, fp64 reference, emulation)."""
    Tk = nk + 3 if limit == "causal" else nk
    q_pos0, src_len = (nk - 1, 0) if limit == "causal" else (nk - 1, 4)
    cap = (Tk + 7) // 8 * 8
    seed = 13000 + 1000 * i + hd + 3 * nk
    Q = rnd(ATTN_B, ATTN_H, 1, hd, dtype=dtype, scale=hd ** -0.25, seed=seed, device=device)
    K = rnd(ATTN_B, ATTN_H, cap, hd, dtype=dtype, scale=hd ** -0.25, seed=seed + 1, device=device)
    Vt = rnd(ATTN_B, ATTN_H, hd, cap, dtype=dtype, seed=seed + 2, device=device)
    ref = attention_ref64(Q, K, Vt, q_pos0, src_len, nk)[0]
    emu = attention_ref64(Q, K, Vt, q_pos0, src_len, nk, round_o=(BF if dtype == BF else None))[0]   # fp32 probabilities: O alone is rounded
    K[:, :, nk:] = NAN
    Vt[:, :, :, nk:] = NAN
    return dict(Q=Q, K=K, Vt=Vt), (Tk, cap, q_pos0, src_len), ref, emu


def attn_frame(dtype, hd):
    big = torch.full((ATTN_B, 1, ATTN_H * hd + 24), NAN, device=dev(), dtype=dtype)
    return big, big[:, :, 8:8 + ATTN_H * hd]


@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("hd", [128, 256])
def test_attention_one_row_wide_heads(hd, dtype):
    from sea_amd import ops

    for nk in attn_nks(hd):
        for limit in ATTN_LIMITS:
            built = [attn_problem(dtype, hd, nk, limit, i) for i in range(3)]
            Tk, cap, q_pos0, src_len = built[0][1]
            assert (q_pos0 + src_len + 1 < Tk) == (limit == "causal") and min(q_pos0 + src_len + 1, Tk) == nk
            frames = [attn_frame(dtype, hd) for _ in built]
            ops.attention_fwd([dict(b[0], O=f[1]) for b, f in zip(built, frames)], ATTN_B, ATTN_H, hd, 1, Tk, cap, q_pos0, src_len, dtype)
            launched(ops, ("attn.row", 1, 0))
            for i, (b, (big, O)) in enumerate(zip(built, frames)):
                what = f"attention row hd={hd} nk={nk} {limit} problem {i}"
                check("attn.O", O, b[2], what, row=hd, f32=(dtype == F32))
                assert frame_untouched(big[:, 0], ATTN_H * hd), (what, "frame")
            big1, O1 = attn_frame(dtype, hd)
            ops.attention_fwd([dict(built[1][0], O=O1)], ATTN_B, ATTN_H, hd, 1, Tk, cap, q_pos0, src_len, dtype)
            launched(ops, ("attn.row", 1, 0))
            assert same(big1, frames[1][0]), (hd, nk, limit, "problem 1 alone differs from the same problem inside the launch")


# ------------------------------------------------------------------------------------------------ sea_rownorm, a workgroup per row
RN_DS = (1024, 1028, 4096, 4100, 8192, 16384, 16388, 32768)
RN_MS = (1, 3, 32)
RN_VARIANTS = ("act_gelu", "mod", "add", "f32")   # bf16 rows, LayerNorm + GELU; fp32 rows with mod: Y32, Yact, mean, rstd; ... + addend, Xout (d <= 2048); the fp32 dtype


def rn_km(variant, d):
    return 1 if d <= 4096 else (4 if variant == "act_gelu" and d <= 16384 else 8)


def rn_group(variant, M, d, gi, device=None):
    kw = dict(device=device)
    seed = 14000 + 1000 * gi + 10 * M + d + 100 * RN_VARIANTS.index(variant)
    g = dict(variant=variant, M=M, d=d, gamma=1 + 0.1 * rnd(d, seed=seed + 2, **kw), beta=0.1 * rnd(d, seed=seed + 3, **kw), mod=None, addend=None)
    if variant == "act_gelu":
        g["X"] = nan_rows(rnd(M, d, dtype=BF, seed=seed + 1, **kw) * 1.2 + 0.3)
        return g
    g["X"] = nan_rows(rnd(M, d, seed=seed + 1, **kw) * 1.3 + 0.3)
    g["mod"] = strided(rnd(M, 2 * d, dtype=(F32 if variant == "f32" else BF), scale=0.3, seed=seed + 4, **kw))
    if variant == "add":
        g["addend"] = nan_rows(0.5 * rnd(M, d, seed=seed + 5, **kw), 4, 32)
    return g


def rn_formula(g, rt=None):
    """Rounded where the kernel rounds: the bf16 output alone."""
    r = rounder(rt if g["variant"] != "f32" else None)
    x = g["X"].double() + (g["addend"].double() if g["addend"] is not None else 0.0)
    xh, mean, rstd = ln64(x)
    y = modulate(xh, g["gamma"], g["beta"], g["mod"])
    if g["variant"] == "act_gelu":
        return {"Yact": r(gelu64(y))}
    return {"Y32": y, "Yact": r(y), "mean": mean, "rstd": rstd}


def rn_launch_dict(g):
    M, d, f32 = g["M"], g["d"], g["variant"] == "f32"
    o = dict(Yact=framed(M, d, F32 if f32 else BF))
    if g["variant"] != "act_gelu":
        o.update(Y32=framed(M, d, F32), mean=guarded((M,), F32), rstd=guarded((M,), F32))
    if g["addend"] is not None:
        o["Xout"] = framed(M, d, F32)
    return dict(X=g["X"], gamma=g["gamma"], beta=g["beta"], mod=g["mod"], addend=g["addend"], **{k: v[1] for k, v in o.items()}), o


def rn_check(g, o, what):
    ref = rn_formula(g)
    f32 = g["variant"] == "f32"
    for k, r_ in ref.items():
        if k in ("mean", "rstd"):
            check("rn." + k, o[k][1], r_, what, f32=True, g32=1e-5)
            assert guard_untouched(o[k][0]), (what, k)
            continue
        check("rn." + k + ("(f32)" if f32 and k == "Yact" else ""), o[k][1], r_, what, row=64, f32=(k == "Y32" or f32), g32=1e-5)
        assert frame_untouched(o[k][0], g["d"]), (what, k)
    if "Xout" in o:
        assert torch.equal(o["Xout"][1], g["X"] + g["addend"]) and frame_untouched(o["Xout"][0], g["d"]), (what, "Xout")


def _rn_run(variant, M, d, form):
    from sea_amd import ops

    groups = [rn_group(variant, M, d, gi) for gi in range(2)]
    built = [rn_launch_dict(g) for g in groups]
    args = (M, d, variant == "act_gelu", variant == "act_gelu", 1e-5, F32 if variant == "f32" else BF)
    ops.rownorm([b[0] for b in built], *args)
    got = launched(ops, form)
    for gi, (g, (_, o)) in enumerate(zip(groups, built)):
        rn_check(g, o, f"rownorm {variant} M={M} d={d} group {gi} -> {got}")
    d1, o1 = rn_launch_dict(groups[1])
    ops.rownorm([d1], *args)
    launched(ops, form)
    assert all(same(o1[k][0], built[1][1][k][0]) for k in o1), (variant, M, d, "group 1 alone differs from the same group inside the launch")


def rn_variants(d):
    return [v for v in RN_VARIANTS if v != "add" or d <= 2048]


@pytest.mark.parametrize("d", RN_DS)
def test_rownorm_a_workgroup_per_row(d):
    for variant in rn_variants(d):
        for M in RN_MS:
            _rn_run(variant, M, d, ("rownorm.fewrows", rn_km(variant, d), 0))


RN_33 = [("act_gelu", 4096, "rownorm.ln_rows"), ("act_gelu", 4100, "rownorm.wave"), ("mod", 1024, "rownorm.wave"), ("f32", 8192, "rownorm.wave")]


@pytest.mark.parametrize("variant,d,form", RN_33)
def test_rownorm_of_33_rows_leaves_the_form(variant, d, form):
    _rn_run(variant, 33, d, (form, 0, 0))


# ------------------------------------------------------------------------------------------------ the emulation behind LOCAL, on the CPU
def emulation_cases(device="cpu"):
    """Yields (what, {kind#n: (reference, emulation, exact, row length or None)}) for every bf16-rounded output of every case the tests of this file launch."""
    def gemm(prefix, what, groups):
        for i, g in enumerate(groups):
            ref, emu, exact = gemm_formula(g), gemm_formula(g, BF), gemm_formula(g, None)
            plain = g["pre"] is None
            keys = [k for k in ref if not (k == "C32" and plain)]
            if keys:
                yield f"{what} group {i}", {gemm_kind(prefix if plain else g["pre_kind"], g, k): (ref[k], emu[k], exact[k], None) for k in keys}

    def qkv(prefix, what, c):
        out = {}
        for i, g in enumerate(c["groups"]):
            ref, emu, exact = qkv_formula(g, c), qkv_formula(g, c, BF), qkv_formula(g, c, None)
            out.update({f"{prefix}.{k}#{i}": (ref[k], emu[k], exact[k], c["hd"]) for k in ref})
        yield what, out

    for M in (1, 2, 3, 4):
        for K in GEMV_KS:
            yield from gemm("gemv", f"gemv plain M={M} K={K}", gemv_plain_groups(M, K, device))
    for K in (512, 1024, 2048):
        for variant in PRE_VARIANTS:
            for M in (1, 2, 3):
                yield from gemm("gemv", f"gemv prologue M={M} K={K} variant {variant}", gemv_pre_groups(M, K, variant, device))
    for K in (512, 2048, 4096, 8192):
        for gelu in (False, True):
            for M in (1, 3):
                yield from gemm("gemv", f"gemv activation rows M={M} K={K} gelu={gelu}", gemv_act_groups(M, K, gelu, device))
    for M in (1, 2, 4):
        for K in (512, 1024, 2048):
            for H, hd, form, B, T, pos0, pro, vout in qkv_fewrows_cases(M, K):
                yield from qkv("qkv", f"gemv qkv M={M} K={K} H={H} hd={hd} {form} B={B} T={T} pos0={pos0} pro={pro}", qkv_fewrows_case(M, K, H, hd, form, B, T, pos0, pro, vout, device))
    for M, Ks in skinny_short_cases() + SKINNY_LEFT:
        yield from gemm("skinny", f"skinny M={M} Ks={Ks}", skinny_groups(M, Ks, device=device))
    for M, Ks, act in skinny_long_cases():
        yield from gemm("skinny", f"skinny long M={M} Ks={Ks} act={act}", skinny_groups(M, Ks, SKINNY_EPIS if act else (0, 4, 2), device=device))
    for hd in (16, 64, 128, 8):
        for B, T, K, pos0, form, vout in sqkv_cases(hd):
            yield from qkv("sqkv", f"qkv skinny hd={hd} B={B} T={T} K={K} pos0={pos0} {form}", sqkv_case(hd, B, T, K, pos0, form, vout, device=device))
    for hd in (128, 256):
        for nk in attn_nks(hd):
            for limit in ATTN_LIMITS:
                for i in range(3):
                    _, _, ref, emu = attn_problem(BF, hd, nk, limit, i, device)
                    yield f"attention row hd={hd} nk={nk} {limit} problem {i}", {"attn.O": (ref, emu, ref, hd)}
    for d in RN_DS:
        for variant in rn_variants(d):
            if variant != "f32":
                for M in RN_MS + ((33,) if any((variant, d) == c[:2] for c in RN_33) else ()):
                    for gi in range(2):
                        g = rn_group(variant, M, d, gi, device)
                        ref, emu, exact = rn_formula(g), rn_formula(g, BF), rn_formula(g, None)
                        yield f"rownorm {variant} M={M} d={d} group {gi}", {"rn.Yact": (ref["Yact"], emu["Yact"], exact["Yact"], 64)}


def measure_local(device="cpu", verbose=True):
    """{kind: (largest rowerr(emulation, reference), its case)}; asserts that the emulation without rounding restates the reference to 1e-12."""
    worst = {k: (0.0, "") for k in LOCAL}
    for what, outs in emulation_cases(device):
        line = []
        for key, (ref, emu, exact, row) in outs.items():
            kind = key.split("#")[0]
            assert float((exact - ref).norm()) <= 1e-12 * max(float(ref.norm()), 1.0), (what, key)
            eg, e = errors(emu, ref, row)
            line.append(f"{key} local {e:.3e} (global {eg:.3e})")
            if e > worst[kind][0]:
                worst[kind] = (e, what)
        if verbose:
            print(f"{what}: " + "  ".join(line))
    return worst


if __name__ == "__main__":
    for kind, (v, what) in measure_local().items():
        print(f"{kind}: measured {v:.3e} at {what}; LOCAL = 3 * {LOCAL[kind] / 3:.3e}")
