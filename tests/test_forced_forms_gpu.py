"""Every kernel form a launcher can take, run under the name it is forced by: each case sets SEA_TUNE (where the form is not the launcher's own choice at
the shape), asserts ops.last_form() right after the launch — which kernel really ran — and compares with an fp64 restatement of the operation on the
operands as rounded to the compute dtype.  Two checks per output:

  global  ||out - ref|| / ||ref|| at the tolerances test_ops_gpu.py / test_bwd_ops_gpu.py use for that kind of output;
  local   max over rows ||err_row|| / rms over rows ||ref_row||: one wrong row among thousands moves the global norm by nothing.

Local bounds.  GEMM, GEMM + norm and weight-gradient outputs are rounded to bf16 at most once, 2^-9 relative at most per element, so a bf16 row is off by
at most 2^-9 ||ref_row|| <= 2^-9 * 3 * rms row norm as long as no row is longer than 3 rms row norms — asserted on every reference (`spread`).  fp32
outputs: 4 x the global fp32 tolerance.  A vector output (db, mean, rstd) is one row.  Attention rounds P and O, and the error of P is statistical: its
bf16 bounds are 3 x what a torch restatement that rounds P and O where the kernel does gives for the same metric on these inputs (ATTN_LOCAL; `python
tests/test_forced_forms_gpu.py` prints the measured values on the CPU); fp32 attention rounds nothing: 4 x the global fp32 tolerance.  The attention
backward (dQ, dK, dV rows of one head, against fp64 autograd) follows the same rule: ATTNB_LOCAL from attention_bwd_emulated, which rounds the forward's O,
the P and dS fragments and the three outputs."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]
BF = torch.bfloat16
LOCAL_BF16 = 3 * 2.0 ** -9
LN2 = math.log(2.0)


def dev():
    return torch.device("cuda:0")


def rnd(*shape, dtype=torch.float32, scale=1.0, seed=0, device=None):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(device if device is not None else dev()).to(dtype)


def gelu64(x):
    return 0.5 * x * (1 + torch.erf(x / math.sqrt(2)))


def rows(t):
    return t.double().reshape(1, -1) if t.dim() == 1 else t.double().reshape(-1, t.shape[-1])


def rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def rowerr(a, b):
    a, b = rows(a), rows(b)
    return float((a - b).norm(dim=1).max() / b.norm(dim=1).pow(2).mean().sqrt().clamp_min(1e-30))


def spread(b):
    n = rows(b).norm(dim=1)
    return float(n.max() / n.pow(2).mean().sqrt().clamp_min(1e-30))


def check(out, ref, f32=2e-5, bf16=6e-3, what=""):
    """Both checks of one output against its fp64 reference; the tolerance follows the OUTPUT's type."""
    g, l = (f32, 4 * f32) if out.dtype == torch.float32 else (bf16, LOCAL_BF16)
    assert spread(ref) <= 3.0, (what, spread(ref))
    assert torch.isfinite(out.float()).all(), what
    eg, el = rel(out, ref), rowerr(out, ref)
    print(f"{what}: global {eg:.3e} (< {g:.1e})  local {el:.3e} (< {l:.2e})")
    assert eg < g, (what, "global", eg)
    assert el < l, (what, "local", el)


def force(monkeypatch, tune):
    if tune:
        monkeypatch.setenv("SEA_TUNE", tune)
    else:
        monkeypatch.delenv("SEA_TUNE", raising=False)


def framed(M, N_, dtype, left=8, right=16):
    """(whole, view): an [M, N] view with NaN columns on both sides (row stride N + left + right, 16-byte aligned start)."""
    big = torch.full((M, N_ + left + right), float("nan"), device=dev(), dtype=dtype)
    return big, big[:, left:left + N_]


def frame_untouched(big, N_, left=8):
    return bool(torch.isnan(big[:, :left].float()).all() and torch.isnan(big[:, left + N_:].float()).all())


# ------------------------------------------------------------------------------------------------ sea_gemm_grouped
def _gemm_group(i, M, N_, K, dtype, bias=True, res=False, c32=False, cact=True, act=0, z=False, n_seg=1, bias_scale=1.0, seed=0):
    """One group dict and the fp64 references of its outputs {"Cact", "C32", "Z"}; the act-dtype output sits in a NaN frame, R is a strided view."""
    s = seed + 10 * i
    Aall = rnd(n_seg, M, K, dtype=dtype, seed=s + 1)
    W = rnd(N_, K, dtype=dtype, scale=(K * n_seg) ** -0.5, seed=s + 2)
    d = dict(A=Aall[0], W=W, act=act, n_seg=n_seg, a_seg_stride=M * K, bias_scale=bias_scale)
    v = Aall.double().sum(0) @ W.double().t()
    if bias:
        d["bias"] = rnd(N_, seed=s + 3)
        v = v + bias_scale * d["bias"].double()
    ref = {}
    if act == 1:
        if z:
            d["Z"] = torch.full((M, N_), float("nan"), device=dev(), dtype=dtype)
            ref["Z"] = v
        v = gelu64(v)
    if res:
        Rbig = rnd(M, 3 * N_, seed=s + 4)
        d["R"] = Rbig[:, N_:2 * N_]
        v = v + d["R"].double()
    frame = None
    if cact:
        frame, d["Cact"] = framed(M, N_, dtype)
        ref["Cact"] = v
    if c32:
        d["C32"] = torch.full((M, N_), float("nan"), device=dev())
        ref["C32"] = v
    return d, ref, frame


def _run_gemm(monkeypatch, tune, specs, dtype, form, a=None, seed=0):
    """Build the groups afresh (outputs NaN), launch under `tune`, assert the form, check every output and the frames; returns the outputs."""
    from sea_amd import ops

    built = [_gemm_group(i, dtype=dtype, seed=seed, **sp) for i, sp in enumerate(specs)]
    force(monkeypatch, tune)
    ops.gemm_grouped([b[0] for b in built], dtype)
    got = ops.last_form()
    torch.cuda.synchronize()
    assert got[0] == form if isinstance(form, str) else got[0] in form, (tune, got)
    if a is not None:
        assert got[1] == a, (tune, got)
    outs = []
    for i, ((d, ref, frame), sp) in enumerate(zip(built, specs)):
        for k, r in ref.items():
            check(d[k], r, what=f"{got[0]} [{tune}] group {i} {k}")
        if frame is not None:
            assert frame_untouched(frame, sp["N_"]), (tune, i)
        outs.append({k: d[k].clone() for k in ref})
    return outs, got


G256_SHAPES = [dict(M=300, N_=200, K=64), dict(M=300, N_=264, K=2048), dict(M=2100, N_=256, K=2048), dict(M=300, N_=2048, K=1024)]   # the last: the n_major bit
G256_EPILOGUES = {
    # bf16 output + strided fp32 residual (the staged copy-out that adds the residual, at a column tile narrower than 256 and at a ragged row tile);
    # C32 together with Cact; no residual
    "plain": [dict(res=True), dict(res=True, c32=True), dict(res=True), dict(bias=False)],
    # act = 1: the non-plain kernel, which the 256 tile takes only when forced; the residual then leaves through the general path
    "gelu": [dict(act=1, z=True), dict(act=1, res=True, c32=True), dict(res=True), dict(act=1)],
}


@pytest.mark.parametrize("epi", sorted(G256_EPILOGUES))
def test_gemm256_against_the_tiled_kernels(monkeypatch, epi):
    """gemm256.hip under SEA_TUNE=gemm256=1 (at these row counts and with a GELU it is taken only when forced), then the 64 and the 128 tile on the same
    launch: four groups — a column tile narrower than 256, N not a multiple of 256, a ragged row tile with the staged residual copy-out, the row-tile-
    fastest order —, outputs in NaN frames."""
    specs = [dict(s, **e) for s, e in zip(G256_SHAPES, G256_EPILOGUES[epi])]
    big, _ = _run_gemm(monkeypatch, "gemm256=1", specs, BF, "gemm.256", seed=1000)
    for tile in (64, 128):
        outs, got = _run_gemm(monkeypatch, f"gemm256=0,gemm_tile={tile}", specs, BF, f"gemm.tile{tile}", seed=1000)
        for o256, o in zip(big, outs):
            for k in o:   # both within the tolerance of the same reference
                assert rel(o256[k], o[k]) < 2 * (2e-5 if o[k].dtype == torch.float32 else 6e-3), (tile, k)


@pytest.mark.parametrize("refused", [dict(M=100, N_=64, K=40), dict(M=100, N_=64, K=64, n_seg=2)])
def test_gemm256_refuses_a_launch_it_cannot_run(monkeypatch, refused):
    """One group the 256 tile has no code for (K not a multiple of 64; two segments) beside two it could take: the whole launch stays on a tiled kernel."""
    specs = [dict(G256_SHAPES[0], res=True), dict(G256_SHAPES[1], c32=True), dict(refused, res=True)]
    _run_gemm(monkeypatch, "gemm256=1", specs, BF, ("gemm.tile64", "gemm.tile128"), seed=1100)


@pytest.mark.parametrize("tile", [64, 128])
@pytest.mark.parametrize("dtype", DTYPES)
def test_gemm_tiles_at_ragged_edges(monkeypatch, dtype, tile):
    """The generic square tiles, both sizes forced, with every edge ragged.  Register-staged loop (a K = 40 group keeps the launch off the LDS-DMA ring): bias +
    strided residual into both outputs, GELU with the kept pre-activation on two segments, bias_scale.  LDS-DMA ring (every group's K n_seg >= 1024 in
    whole K-tiles; a = 1, four stages): the same epilogues at (130, 132, 1024) and on two segments of 512."""
    staged = [dict(M=300, N_=200, K=40, res=True, c32=True), dict(M=77, N_=72, K=24, n_seg=2, act=1, z=True, bias_scale=2.0), dict(M=130, N_=132, K=136, bias_scale=3.0, c32=True, cact=False)]
    _, got = _run_gemm(monkeypatch, f"gemm_tile={tile}", staged, dtype, f"gemm.tile{tile}", a=0, seed=1200)
    assert got[2] == 0
    ring = [dict(M=130, N_=132, K=1024, res=True, c32=True), dict(M=70, N_=68, K=512, n_seg=2, bias_scale=2.0, act=1, z=True), dict(M=65, N_=64, K=1024, act=1)]
    _, got = _run_gemm(monkeypatch, f"gemm_tile={tile}", ring, dtype, f"gemm.tile{tile}", a=1, seed=1300)
    assert got[2] == 4


# ------------------------------------------------------------------------------------------------ sea_gemm_rownorm
def _gemm_norm_groups(dtype, M, N_, K, seed):
    """Four groups of one launch: residual + AdaLN modulation, modulation only, gamma only (the kinds of test_gemm_rownorm_matches_gemm_then_rownorm), and the
    exchange tail's group of test_gemm_rownorm_segments_ib_addend (two segments, in-place fp32 residual, pre-addend copy, info-bottleneck addend)."""
    groups, refs = [], []
    for gi in range(4):
        s = seed + 20 * gi
        seg = gi == 3
        n_seg, Kg = (2, K // 2 if K % 16 == 0 else K) if seg else (1, K)
        Aall = rnd(n_seg, M, Kg, dtype=dtype, seed=s + 1)
        W = rnd(N_, Kg, dtype=dtype, scale=0.2, seed=s + 2)
        bias = 0.3 * rnd(N_, seed=s + 3) + 0.5
        mod = rnd(M, 2 * N_, dtype=dtype, scale=0.5, seed=s + 5) if gi != 2 else None
        gamma, beta = 1 + 0.1 * rnd(N_, seed=s + 6), (0.1 * rnd(N_, seed=s + 7) if gi != 2 else None)
        y32big = torch.zeros(M, 3 * N_, device=dev())
        d = dict(A=Aall[0], W=W, bias=bias, mod=mod, gamma=gamma, beta=beta, n_seg=n_seg, a_seg_stride=M * Kg, bias_scale=float(n_seg),
                 Yact=torch.full((M, N_), float("nan"), device=dev(), dtype=dtype), Y32=y32big[:, N_:2 * N_],
                 mean=torch.full((M,), float("nan"), device=dev()), rstd=torch.full((M,), float("nan"), device=dev()))
        pre = Aall.double().sum(0) @ W.double().t() + n_seg * bias.double()
        v = pre
        ref = {}
        if gi == 0:
            d["R"] = rnd(M, N_, seed=s + 4)
            pre = v = pre + d["R"].double()
        if seg:
            h = 8
            x = rnd(M, N_, seed=s + 4)
            pre = pre + x.double()
            ib = dict(c=torch.rand(M, generator=torch.Generator().manual_seed(s + 8)).to(dev()), w1=rnd(h, seed=s + 9), b1=rnd(h, seed=s + 10),
                      lnw=1 + 0.1 * rnd(h, seed=s + 11), lnb=0.1 * rnd(h, seed=s + 12), w2=rnd(N_, h, scale=0.3, seed=s + 13), b2=0.1 * rnd(N_, seed=s + 14), h=h)
            hid = gelu64(torch.nn.functional.layer_norm(ib["c"].double()[:, None] * ib["w1"].double() + ib["b1"].double(), (h,), ib["lnw"].double(), ib["lnb"].double(), 1e-5))
            v = pre + hid @ ib["w2"].double().t() + ib["b2"].double()
            d.update(R=x, C32=x, Cact=torch.full((M, N_), float("nan"), device=dev(), dtype=dtype), ib=ib)
            ref["Cact"] = pre            # written BEFORE the addend
        else:
            d["C32"] = torch.full((M, N_), float("nan"), device=dev())
        ref["C32"] = v
        mu = v.mean(-1, keepdim=True)
        var = ((v - mu) ** 2).mean(-1, keepdim=True)
        xh = (v - mu) / torch.sqrt(var + 1e-5)
        y = xh * (gamma.double() + 1 + mod[:, :N_].double()) + (beta.double() + mod[:, N_:].double()) if mod is not None else xh * gamma.double()
        ref.update(Yact=y, Y32=y, mean=mu[:, 0], rstd=1 / torch.sqrt(var[:, 0] + 1e-5))
        groups.append(d)
        refs.append((ref, y32big))
    return groups, refs


@pytest.mark.parametrize("K", [72, 128, 256, 512])
@pytest.mark.parametrize("N_", [48, 64, 128, 256])
@pytest.mark.parametrize("dtype", DTYPES)
def test_gemm_rownorm_tile_shapes_agree(monkeypatch, dtype, N_, K):
    """The three kernels of sea_gemm_rownorm on the same launches, M in {1, 63, 65, 203}: the 16-row tiles the launcher picks by itself at these lengths —
    with the whole-contraction LDS-DMA burst when every group's contraction is at most four whole K-tiles (bf16: K = 128, 256; fp32: K = 128), the staged
    loop otherwise (K = 72: no whole K-tile; K = 512: too long) — and the 64-row tiles of long launches (cfg3 training), forced.  Every output, mean and
    rstd included, against fp64; then the two tile shapes against each other (both lie within the tolerance of one reference)."""
    from sea_amd import ops

    bk = 64 if dtype == BF else 32
    for M in (1, 63, 65, 203):
        outs = {}
        for tune in (None, "gemm_norm_rows=64"):
            groups, refs = _gemm_norm_groups(dtype, M, N_, K, seed=2000 + M)
            dma = all(g["W"].shape[1] % bk == 0 and g["W"].shape[1] * g["n_seg"] // bk <= 4 for g in groups)
            want = "gemm_norm.rows64" if tune else ("gemm_norm.rows16_dma" if dma else "gemm_norm.rows16")
            force(monkeypatch, tune)
            ops.gemm_rownorm(groups, 1e-5, dtype)
            got = ops.last_form()
            torch.cuda.synchronize()
            assert got[0] == want, (M, tune, got)
            for gi, (d, (ref, y32big)) in enumerate(zip(groups, refs)):
                for k, r in ref.items():
                    norm_out = k in ("Yact", "Y32")
                    check(d[k], r, f32=3e-5 if norm_out else 2e-5, what=f"{got[0]} M={M} group {gi} {k}")
                assert float(y32big[:, :N_].abs().max()) == 0 and float(y32big[:, 2 * N_:].abs().max()) == 0
            outs[want] = [{k: d[k].clone() for k in ref} for d, (ref, _) in zip(groups, refs)]
        (_, small), (_, big) = sorted(outs.items())
        for o16, o64 in zip(small, big):
            for k in o16:
                t = (3e-5 if k in ("Yact", "Y32") else 2e-5) if o16[k].dtype == torch.float32 else 6e-3
                assert rel(o16[k], o64[k]) < 2 * t, (M, k)


# ------------------------------------------------------------------------------------------------ sea_attention_fwd
ATTN_SHAPES = [(257, 257, 0, 0), (330, 330, 0, 3), (5, 300, 295, 0), (257, 257, 0, 264)]   # (Tq, Tk, q_pos0, src_len): two wave groups need Tk >= 256;
ATTN_SHORT = [(200, 200, 0, 3), (200, 200, 0, 200)]   # fewer than 256 keys: one wave group               the last of each: src_len = cap, every key visible
ATTN_ROW = [(1, 300, 299, 0), (1, 257, 100, 3), (1, 200, 199, 0)]      # Tq = 1 without LSE: the one-row kernels (keys limited by the causal rule or by Tk)
ATTN_B, ATTN_H = 1, 3
# Local bounds of the bf16 outputs = 3 x the largest value of the same metric for attention_ref64(round_p, round_o) (P and O rounded to bf16 where the kernel rounds them)
# over every case of this file, measured on the CPU (python tests/test_forced_forms_gpu.py).  Measured: O 1.358e-2 for the tiled kernels (P and O rounded; the
# early queries see few keys, so their rows are several rms row norms long), O 2.957e-3 for the row kernels (fp32 probabilities: O alone), LSE 2.806e-4.  (The shapes with every key visible and
# the three problems of one launch stay below them: at most O 8.236e-3, LSE 2.733e-4.)
ATTN_LOCAL = {"O": 3 * 1.358e-2, "O_row": 3 * 2.957e-3, "LSE": 3 * 2.806e-4}


def attn_inputs(dtype, hd, Tq, Tk, q_pos0, src_len, device=None, seed=0):
    cap = (Tk + 7) // 8 * 8
    Q = rnd(ATTN_B, ATTN_H, Tq, hd, dtype=dtype, scale=hd ** -0.25, seed=seed + 3000 + hd + Tq, device=device)
    K = rnd(ATTN_B, ATTN_H, cap, hd, dtype=dtype, scale=hd ** -0.25, seed=seed + 3001 + hd + Tq, device=device)
    Vt = rnd(ATTN_B, ATTN_H, hd, cap, dtype=dtype, seed=seed + 3002 + hd + Tq, device=device)
    return Q, K, Vt, cap


def attention_ref64(Q, K, Vt, q_pos0, src_len, Tk, round_p=None, round_o=None):
    """fp64 restatement of the kernels' contract (scores in log2 units: P = 2^(S - max), LSE = max + log2 sum P).  round_p / round_o: dtypes P (before the
    row sum, as the bf16 kernels' matrix-core row sum sees it) and O are rounded to — the emulation the local bounds come from."""
    Q, K, V = Q.double(), K[:, :, :Tk].double(), Vt[:, :, :, :Tk].double().transpose(2, 3)
    B, H, Tq, hd = Q.shape
    S = Q @ K.transpose(-1, -2)
    i = torch.arange(Tq, device=Q.device)[:, None] + q_pos0 + src_len
    j = torch.arange(Tk, device=Q.device)[None, :]
    S = S.masked_fill(j > i, float("-inf"))
    mx = S.max(-1, keepdim=True).values
    P = torch.exp2(S - mx)
    if round_p is not None:
        P = P.to(round_p).double()
    l = P.sum(-1, keepdim=True)
    O = (P @ V) / l
    if round_o is not None:
        O = O.to(round_o).double()
    return O.transpose(1, 2).reshape(B, Tq, H * hd), (mx + torch.log2(l))[..., 0]


def attn_rows(O, hd):
    """[B, Tq, H * hd] -> one row per (trajectory, head, query)."""
    return O.reshape(-1, hd)


def _attn_problem(dtype, hd, shape, lse=True, seed=0):
    """One problem dict (padding poisoned, outputs NaN) and the fp64 references of O and LSE."""
    Tq, Tk, q_pos0, src_len = shape
    Q, K, Vt, cap = attn_inputs(dtype, hd, Tq, Tk, q_pos0, src_len, seed=seed)
    Oref, Lref = attention_ref64(Q, K, Vt, q_pos0, src_len, Tk)
    K[:, :, Tk:] = float("nan")        # poison the padding: it must never leak into the result
    Vt[:, :, :, Tk:] = float("nan")
    p = dict(Q=Q, K=K, Vt=Vt, O=torch.full((ATTN_B, Tq, ATTN_H * hd), float("nan"), device=dev(), dtype=dtype))
    if lse:
        p["LSE"] = torch.full((ATTN_B, ATTN_H, Tq), float("nan"), device=dev())
    return p, Oref, Lref, cap


def _attn_check(p, Oref, Lref, dtype, hd, form, what):
    f32 = dtype == torch.float32
    O = p["O"]
    assert torch.isfinite(O.float()).all(), what
    eg, el = rel(O, Oref), rowerr(attn_rows(O, hd), attn_rows(Oref, hd))
    lo = 4 * 2e-5 if f32 else ATTN_LOCAL["O_row" if form == "attn.row" else "O"]
    print(f"{what} O: global {eg:.3e}  local {el:.3e} (< {lo:.2e})")
    assert eg < (2e-5 if f32 else 8e-3), (what, eg)
    assert el < lo, (what, el)
    if "LSE" in p:
        L = p["LSE"]
        assert torch.isfinite(L).all(), what
        eg, el = rel(L, Lref), rowerr(L.reshape(-1, 1), Lref.reshape(-1, 1))
        ll = 4 * 1e-5 if f32 else ATTN_LOCAL["LSE"]
        print(f"{what} LSE: global {eg:.3e}  local {el:.3e} (< {ll:.2e})")
        assert eg < (1e-5 if f32 else 1e-3), (what, eg)
        assert el < ll, (what, el)


def _attn_case(monkeypatch, tune, dtype, hd, shape, form, paired=None, lse=True, n=1):
    """n problems with different tensors in ONE launch under `tune`: the form, then every problem against its reference; returns [(O, LSE)] per problem
    (the pair itself when n = 1)."""
    from sea_amd import ops

    Tq, Tk, q_pos0, src_len = shape
    built = [_attn_problem(dtype, hd, shape, lse, seed=100 * i) for i in range(n)]
    cap = built[0][3]
    force(monkeypatch, tune)
    ops.attention_fwd([b[0] for b in built], ATTN_B, ATTN_H, hd, Tq, Tk, cap, q_pos0, src_len, dtype)
    got = ops.last_form()
    torch.cuda.synchronize()
    assert got[0] == form, (tune, hd, shape, got)
    if paired is not None:
        assert got[1] == paired, (tune, got)
    for i, (p, Oref, Lref, _) in enumerate(built):
        _attn_check(p, Oref, Lref, dtype, hd, form, f"{form} [{tune}] hd={hd} {shape}" + (f" problem {i} of {n}" if n > 1 else ""))
    outs = [(p["O"], p.get("LSE")) for p, _, _, _ in built]
    return outs[0] if n == 1 else outs


@pytest.mark.parametrize("hd", [8, 16, 32])
@pytest.mark.parametrize("dtype", DTYPES)
def test_attention_four_wave_groups(monkeypatch, dtype, hd):
    """Up to 512 workgroups with at least 256 keys at head dims 8 / 16 / 32: the launcher's own choice (nothing to force)."""
    for shape in ATTN_SHAPES:
        _attn_case(monkeypatch, None, dtype, hd, shape, "attn.split4", paired=0)


@pytest.mark.parametrize("hd", [8, 16, 32, 64])
@pytest.mark.parametrize("dtype", DTYPES)
def test_attention_two_wave_groups(monkeypatch, dtype, hd):
    """SPLIT = 2 — what cfg2's self-attention takes (768 workgroups) — on a short launch: forced at head dims 8 / 16 / 32 by switching the four-group form
    off; head dim 64 has no four-group form."""
    for shape in ATTN_SHAPES:
        _attn_case(monkeypatch, "attn_split4=0" if hd < 64 else None, dtype, hd, shape, "attn.split2", paired=0)


@pytest.mark.parametrize("hd", [8, 16, 32, 64])
@pytest.mark.parametrize("dtype", DTYPES)
def test_attention_one_wave_group_and_its_paired_order(monkeypatch, dtype, hd):
    """Fewer than 256 keys: one wave group per query tile.  At head dims 32 / 64 the paired tile order (forced) is bitwise the plain one."""
    for shape in ATTN_SHORT:
        plain = _attn_case(monkeypatch, "attn_paired=0", dtype, hd, shape, "attn.split1", paired=0)
        if hd >= 32:
            pair = _attn_case(monkeypatch, "attn_paired=1", dtype, hd, shape, "attn.split1", paired=1)
            assert torch.equal(plain[0], pair[0]) and torch.equal(plain[1], pair[1])


@pytest.mark.parametrize("tune,hd,form", [(None, 32, "attn.split4"), ("attn_split4=0", 32, "attn.split2"), (None, 128, "attn.split1")])
@pytest.mark.parametrize("dtype", DTYPES)
def test_attention_prefill_of_three_problems_in_one_launch(monkeypatch, dtype, tune, hd, form):
    """Three problems with different tensors (grid.z = 3) at Tq = Tk = 257 in each tiled form (with at least 256 keys one wave group is what a compute
    width above 64 runs): every problem against its own reference, and bitwise what the same problem gives when it is launched alone."""
    shape = (257, 257, 0, 0)
    together = _attn_case(monkeypatch, tune, dtype, hd, shape, form, paired=0, n=3)
    for i, (O, L) in enumerate(together):
        p, _, _, cap = _attn_problem(dtype, hd, shape, seed=100 * i)
        from sea_amd import ops

        ops.attention_fwd([p], ATTN_B, ATTN_H, hd, 257, 257, cap, 0, 0, dtype)
        assert ops.last_form()[0] == form, (i, ops.last_form())
        torch.cuda.synchronize()
        assert torch.equal(O, p["O"]) and torch.equal(L, p["LSE"]), (form, i)


@pytest.mark.parametrize("hd", [8, 16, 32, 64])
@pytest.mark.parametrize("dtype", DTYPES)
def test_attention_row_form(monkeypatch, dtype, hd):
    for shape in ATTN_ROW:
        _attn_case(monkeypatch, None, dtype, hd, shape, "attn.row", lse=False)


# ------------------------------------------------------------------------------------------------ sea_attention_bwd
# (Tq, Tk, q_pos0, src_len) at 64 x 64 tiles and 16-row waves; src_len = CAP: every key visible, with the identity rotary table, as the training engine issues
# its information-bottleneck and spatial-encoder attention
CAP = "cap"
ATTNB_EDGES = [(63, 63, 0, 0), (64, 64, 0, 0), (65, 65, 0, 0), (128, 128, 0, 0), (129, 129, 0, 1)]   # tile and wave edges
ATTNB_SRC = [(80, 80, 0, 16), (130, 130, 0, 15)]                        # src_len one wave high: the unmasked-tile boundaries of both kernels
ATTNB_FULL = [(64, 64, 0, CAP), (70, 70, 0, CAP), (130, 130, 0, CAP)]
# a chunk at the end of a cache; a longer one; key tiles no query sees; queries past the last key; one element
ATTNB_RECT = [(5, 77, 72, 0), (70, 200, 130, 0), (40, 200, 0, 0), (130, 70, 0, 0), (1, 1, 0, 0)]
ATTNB_SHAPES = ATTNB_EDGES + ATTNB_SRC + ATTNB_FULL + ATTNB_RECT           # at head dims 16 and 32
# a fifth entry x puts +c on q0[..., 0] and -c on k0[..., 0] with c^2 q_scale = x: every score lies near -x in log2 units.  At x = 144 the 2^(0 - LSE) of a
# zero-filled tile row past Tk overflows fp32 — what `key < Tk` in the dQ kernel's tile mask is there for (without it inf * 0 makes the tile's dQ rows NaN).
ATTNB_FAR = [(70, 70, 0, CAP, 144.0)]
ATTNB_HD_SHAPES = [(65, 65, 0, 0), (130, 130, 0, CAP), (70, 200, 130, 0)]   # at every other head dim
ATTNB_HDS = [8, 64, 128, 256, 24, 96]                                      # (24 and 96: the masked kernels, compute widths 32 and 96)
ATTNB_MODE_SHAPES = [(65, 65, 0, 0), (129, 129, 0, 1), (130, 130, 0, CAP), (40, 200, 0, 0)]
ATTNB_MODE_BH = [(1, 3), (2, 4)]                                           # B * H = 3: the XCD-local order falls back to the plain one; 8: it is taken
ATTNB_MULTI_SHAPES = [(65, 65, 0, 0), (70, 70, 0, CAP)]                    # hd 16, three and SEA_MAX_ATTN_PROBLEMS (8) problems
ATTNB_DROP = dict(hd=32, shape=(129, 129, 0, CAP), n=2, seed=4242, stream=11, thr=64)
ATTNB_B, ATTNB_H = 1, 3
LOG2E = 1.4426950408889634
# Local bounds of the bf16 gradients = 3 x the largest value of the same metric for attention_bwd_emulated (the fp64 formulas, rounded to bf16 where the kernels
# round: the O the forward stored, the P and dS fragments in front of the second MFMA, the three outputs) over every case of this section, the dropout case
# apart, measured on the CPU (python tests/test_forced_forms_gpu.py).
# Measured: dQ 2.728e-2 (hd 8, (70, 200, 130, 0)), dK 2.474e-2 and dV 2.474e-2 (both hd 16, (40, 200, 0, 0), B * H = 8: four key rows in five are zero, so a
# row is long against the rms row norm); with dropout dQ 9.988e-3, dK 1.090e-2, dV 6.177e-3.
ATTNB_LOCAL = {"dQ": 3 * 2.728e-2, "dK": 3 * 2.474e-2, "dV": 3 * 2.474e-2, "dQ_drop": 3 * 9.988e-3, "dK_drop": 3 * 1.090e-2, "dV_drop": 3 * 6.177e-3}


def attnb_cases():
    """Every (hd, shape, B, H, number of problems) of this section, the dropout case apart: what the tests launch and what ATTNB_LOCAL is measured over."""
    cases = [(hd, sh, ATTNB_B, ATTNB_H, 1) for hd in (16, 32) for sh in ATTNB_SHAPES]
    cases += [(hd, sh, ATTNB_B, ATTNB_H, 1) for hd in ATTNB_HDS for sh in ATTNB_HD_SHAPES]
    cases += [(hd, sh, B, H, 1) for hd in (16, 32) for sh in ATTNB_MODE_SHAPES for B, H in ATTNB_MODE_BH if (B, H) != (ATTNB_B, ATTNB_H)]
    cases += [(16, sh, ATTNB_B, ATTNB_H, n) for sh in ATTNB_MULTI_SHAPES for n in (3, 8)]
    return cases


def rope_table(hd, n, identity=False, device=None):
    if identity:   # cos 1, sin 0
        t = torch.stack((torch.ones(n, hd // 2), torch.zeros(n, hd // 2)), dim=-1)
    else:
        ang = torch.outer(torch.arange(n, dtype=torch.float32), 1.0 / (10000.0 ** (torch.arange(0, hd, 2).float() / hd)))
        t = torch.stack((torch.cos(ang), torch.sin(ang)), dim=-1)
    return t.contiguous().to(device if device is not None else dev())


def rope64(x, table, pos0, inverse=False):
    """x [B, T, H, hd] (fp64) rotated at positions pos0 .. pos0 + T - 1: (e', o') = (e c - o s, e s + o c); inverse: the transposed rotation."""
    T = x.shape[1]
    c, s = table[pos0:pos0 + T, :, 0].double()[None, :, None, :], table[pos0:pos0 + T, :, 1].double()[None, :, None, :]
    if inverse:
        s = -s
    xe, xo = x[..., 0::2], x[..., 1::2]
    return torch.stack((xe * c - xo * s, xe * s + xo * c), dim=-1).flatten(-2)


def drop_mask_host(rows, cols, seed, stream, thr):
    """keep * scale of SeaDropout (include/sea_hip.h) restated on the host, so that the emulation behind the dropout bounds runs without a device; the
    dropout test asserts that sea_dropout_mask gives the same grid."""
    import numpy as np

    M = np.uint64(0xFFFFFFFF)

    def fmix(x):
        x = x ^ (x >> np.uint64(16))
        x = (x * np.uint64(0x85EBCA6B)) & M
        x = x ^ (x >> np.uint64(13))
        x = (x * np.uint64(0xC2B2AE35)) & M
        return x ^ (x >> np.uint64(16))

    row = np.arange(rows, dtype=np.uint64)[:, None]
    col = np.arange(cols, dtype=np.uint64)[None, :]
    base = np.uint64((seed ^ ((stream * 0x9E3779B1) & 0xFFFFFFFF)) & 0xFFFFFFFF)
    x = fmix((base + ((row * np.uint64(0x85EBCA77)) & M)) & M)
    w = fmix(x ^ ((((col >> np.uint64(2)) * np.uint64(0xC2B2AE3D)) + np.uint64(0x27D4EB2F)) & M))
    byte = (w >> (np.uint64(8) * (col & np.uint64(3)))) & np.uint64(0xFF)
    return torch.from_numpy(np.where(byte >= np.uint64(thr), float(np.float32(256.0) / np.float32(256 - thr)), 0.0))   # the kernels' scale is an fp32 quotient


def attnb_inputs(dtype, hd, shape, B, H, prob=0, device=None):
    """The operands of one problem as the QKV epilogue would have written them (rotated, q scaled, rounded to the compute dtype), the fp64 pre-images q0 /
    k0 / v0 [B, T, H, hd] the gradients are taken with respect to, dO, the rotary table and the resolved (cap, src_len)."""
    Tq, Tk, q_pos0, src_len = shape[:4]
    device = device if device is not None else dev()
    cap = (Tk + 15) // 8 * 8                      # at least 8 padding rows
    full = src_len == CAP
    src_len = cap if full else src_len
    seed = 5000 + 1000 * prob + 7 * hd + 13 * Tq + 3 * Tk + 31 * q_pos0 + 101 * B * H
    table = rope_table(hd, max(q_pos0 + Tq, Tk), identity=full, device=device)
    q0, k0, v0 = (rnd(B, T, H, hd, seed=seed + s, device=device).double() for s, T in ((1, Tq), (2, Tk), (3, Tk)))
    scale2 = float(hd) ** -0.5 * LOG2E            # ops.q_scale(hd): the attention kernels score in log2 units
    if len(shape) > 4:                            # (with the identity table: coordinate 0 is not rotated away)
        assert full
        q0[..., 0], k0[..., 0] = (shape[4] / scale2) ** 0.5, -(shape[4] / scale2) ** 0.5
    return dict(q0=q0, k0=k0, v0=v0, table=table, cap=cap, src_len=src_len, scale2=scale2, B=B, H=H, hd=hd, Tq=Tq, Tk=Tk, q_pos0=q_pos0,
                dO=rnd(B, Tq, H * hd, dtype=dtype, seed=seed + 4, device=device),
                Q=(rope64(q0, table, q_pos0) * scale2).permute(0, 2, 1, 3).contiguous().to(dtype),
                K=rope64(k0, table, 0).permute(0, 2, 1, 3).contiguous().to(dtype), V=v0.permute(0, 2, 1, 3).contiguous().to(dtype))


def attnb_visible(inp):
    """[Tq, Tk] bool: query i (at position q_pos0 + i) sees key j iff j <= q_pos0 + i + src_len."""
    i = torch.arange(inp["Tq"], device=inp["Q"].device)[:, None] + inp["q_pos0"] + inp["src_len"]
    return torch.arange(inp["Tk"], device=inp["Q"].device)[None, :] <= i


def attention_bwd_ref64(inp, drop=None):
    """fp64 autograd through rotary -> q_scale -> masked base-2 softmax (-> dropout factors `drop` [B, H, Tq, Tk]) -> P V, evaluated on the operands as
    rounded to the compute dtype (straight-through: the values are the kernel's operands, the gradients flow to q0 / k0 / v0).  Returns the gradients with
    respect to the un-rotated, un-scaled q, k, v ([B, T, H, hd]): what dQ, dK, dV hold."""
    q, k, v = (inp[n].clone().requires_grad_(True) for n in ("q0", "k0", "v0"))
    qr = (rope64(q, inp["table"], inp["q_pos0"]) * inp["scale2"]).permute(0, 2, 1, 3)
    kr, vr = rope64(k, inp["table"], 0).permute(0, 2, 1, 3), v.permute(0, 2, 1, 3)
    qr, kr, vr = (t + (inp[n].double() - t.detach()) for t, n in ((qr, "Q"), (kr, "K"), (vr, "V")))
    S = (qr @ kr.transpose(-1, -2)).masked_fill(~attnb_visible(inp), float("-inf"))
    P = torch.exp2(S - S.max(-1, keepdim=True).values.detach())
    P = P / P.sum(-1, keepdim=True)
    if drop is not None:
        P = P * drop.double()
    O = (P @ vr).transpose(1, 2).reshape(inp["B"], inp["Tq"], -1)
    O.backward(inp["dO"].double())
    return {"dQ": q.grad, "dK": k.grad, "dV": v.grad}


def attention_bwd_emulated(inp, drop=None, rt=BF):
    """The kernels' formulas in fp64 with a rounding to `rt` where the bf16 kernels round: the forward's P (before the row sum) and O, hence delta = sum O dO
    of the ROUNDED O; the P (x dropout factor) and dS fragments in front of the second MFMA (pack_frag); the three outputs.  rt = None rounds nothing and
    restates attention_bwd_ref64 without autograd (checked by this file's __main__)."""
    r = (lambda t: t.to(rt).double()) if rt is not None else (lambda t: t)
    B, H, hd, Tq, Tk = inp["B"], inp["H"], inp["hd"], inp["Tq"], inp["Tk"]
    Q, K, V = inp["Q"].double(), inp["K"].double(), inp["V"].double()
    dO = inp["dO"].double().view(B, Tq, H, hd).permute(0, 2, 1, 3)
    D = drop.double() if drop is not None else 1.0
    S = (Q @ K.transpose(-1, -2)).masked_fill(~attnb_visible(inp), float("-inf"))
    mx = S.max(-1, keepdim=True).values
    Pf = torch.exp2(S - mx)
    l = r(Pf).sum(-1, keepdim=True)                 # the forward's row sum: of the rounded, un-dropped probabilities
    O = r((r(Pf * D) @ V) / l)
    lse = mx + torch.log2(l)
    delta = (O * dO).sum(-1, keepdim=True)
    P = torch.exp2(S - lse)
    dS = P * ((dO @ V.transpose(-1, -2)) * D - delta)
    pf, sf = r(P * D), r(dS)
    dq = rope64((sf @ K).permute(0, 2, 1, 3), inp["table"], inp["q_pos0"], inverse=True) * (inp["scale2"] * LN2)
    dk = rope64((sf.transpose(-1, -2) @ Q).permute(0, 2, 1, 3), inp["table"], 0, inverse=True) * LN2
    dv = (pf.transpose(-1, -2) @ dO).permute(0, 2, 1, 3)
    return {"dQ": r(dq), "dK": r(dk), "dV": r(dv)}


def attnb_drop_factors(inp, prob, seed, stream0, thr):
    """[B, H, Tq, Tk]: the kernels' mask of (problem, b, h) is stream (stream0 + problem) * B * H + b * H + h over the (query, key) grid."""
    B, H = inp["B"], inp["H"]
    return torch.stack([torch.stack([drop_mask_host(inp["Tq"], inp["Tk"], seed, (stream0 + prob) * B * H + b * H + h, thr) for h in range(H)])
                        for b in range(B)]).to(inp["Q"].device)


def _attnb_launch(monkeypatch, tune, dtype, inps, drop=None):
    """One forward (for O and LSE, as in training) and one backward launch of the problems `inps` under `tune`: K / V padding rows [Tk, cap) NaN, O and dO column views of wider NaN-framed buffers (ldo = E + 24, lddo = E + 16), dQ in a NaN frame, dK | dV the halves of one
    [B * Tk, 2 E] buffer, every output NaN before the launch.  Asserts the noted form; returns the problem dicts."""
    import ctypes as C

    from sea_amd import _native as N, ops

    i0 = inps[0]
    B, H, hd, Tq, Tk, cap, q_pos0, src_len = (i0[k] for k in ("B", "H", "hd", "Tq", "Tk", "cap", "q_pos0", "src_len"))
    E, nan = H * hd, float("nan")
    assert abs(ops.q_scale(hd) - i0["scale2"]) < 1e-15
    probs = []
    for inp in inps:
        K, V = (torch.full((B, H, cap, hd), nan, device=dev(), dtype=dtype) for _ in range(2))
        K[:, :, :Tk], V[:, :, :Tk] = inp["K"], inp["V"]
        Obig = torch.full((B, Tq, E + 24), nan, device=dev(), dtype=dtype)
        dObig = torch.full((B, Tq, E + 16), nan, device=dev(), dtype=dtype)
        dObig[:, :, 8:8 + E] = inp["dO"]
        dQbig, dQ = framed(B * Tq, E, dtype)
        dKV = torch.full((B * Tk, 2 * E), nan, device=dev(), dtype=dtype)
        probs.append(dict(Q=inp["Q"], K=K, V=V, Vt=V.transpose(2, 3).contiguous(), O=Obig[:, :, 8:8 + E], dO=dObig[:, :, 8:8 + E], Obig=Obig, dQbig=dQbig,
                          LSE=torch.full((B, H, Tq), nan, device=dev()), delta=torch.full((B, H, Tq), nan, device=dev()), dQ=dQ, dK=dKV[:, :E], dV=dKV[:, E:]))
    force(monkeypatch, tune)
    ops.attention_fwd(probs, B, H, hd, Tq, Tk, cap, q_pos0, src_len, dtype, drop=drop)
    if drop is None:
        ops.attention_bwd(probs, i0["table"], B, H, hd, Tq, Tk, cap, q_pos0, src_len, i0["scale2"], dtype)
    else:
        P = N.SeaAttnBwdParams()
        ops.fill_attn_bwd_params(P, probs, i0["table"], B, H, hd, Tq, Tk, cap, q_pos0, src_len, i0["scale2"], drop)
        N.check(N.lib().sea_attention_bwd(C.byref(P), N.dtype_code(dtype), N.stream_ptr()), "sea_attention_bwd")
    got = ops.last_form()
    torch.cuda.synchronize()
    mode = int(tune.split("=")[1]) if tune else 0      # these launches are far below the 4096 workgroups from which the launcher picks mode 3 itself
    assert got == ("attn_bwd" if hd in (8, 16, 32, 64, 128, 256) else "attn_bwd.masked", mode, mode), (tune, hd, got)
    return probs


def _attnb_check(what, dtype, inp, p, ref, drop=False):
    """Both checks of dQ, dK, dV of one problem, delta, the frames, exact zeros at keys no query sees."""
    B, H, hd, Tq, Tk = inp["B"], inp["H"], inp["hd"], inp["Tq"], inp["Tk"]
    f32 = dtype == torch.float32
    t = 2e-5 if f32 else 2e-2
    floor = 0.1 * float(inp["dO"].double().norm())
    assert frame_untouched(p["dQbig"], H * hd), what
    assert frame_untouched(p["Obig"].view(B * Tq, -1), H * hd), what
    O, dO = p["O"].double(), p["dO"].double()
    assert torch.isfinite(O).all() and torch.isfinite(p["LSE"]).all() and torch.isfinite(p["delta"]).all(), what
    # delta = sum_d O dO of the stored O and dO: hd products (exact in fp32 for bf16 factors, one rounding for fp32 ones) summed in fp32 in some order:
    # at most (hd + 1) 2^-24 sum |O dO| off; asserted at hd 2^-23
    terms = (O * dO).view(B, Tq, H, hd).permute(0, 2, 1, 3)
    ed = (p["delta"].double() - terms.sum(-1)).abs() - hd * 2.0 ** -23 * terms.abs().sum(-1)
    assert float(ed.max()) <= 0, (what, "delta", float(ed.max()))
    first_unseen = inp["q_pos0"] + Tq - 1 + inp["src_len"] + 1     # keys from here on are seen by no query
    for name, T in (("dQ", Tq), ("dK", Tk), ("dV", Tk)):
        out, r = p[name].reshape(B, T, H, hd), ref[name]
        assert torch.isfinite(out.float()).all(), (what, name)
        err, rn = float((out.double() - r).norm()), float(r.norm())
        if rn == 0:    # Tq = Tk = 1: dQ = dK = 0 exactly — the floor of test_bwd_ops_gpu.py
            print(f"{what} {name}: reference 0, error {err:.3e} (<= {t * floor:.2e})")
            assert err <= t * floor, (what, name, err)
            continue
        lo = 4 * t if f32 else ATTNB_LOCAL[name + ("_drop" if drop else "")]
        eg, el = err / rn, rowerr(out.reshape(-1, hd), r.reshape(-1, hd))
        print(f"{what} {name}: global {eg:.3e} (< {t:.1e})  local {el:.3e} (< {lo:.2e})")
        assert eg < t, (what, name, "global", eg)
        assert el < lo, (what, name, "local", el)
        if name != "dQ" and first_unseen < Tk:
            assert bool((out[:, first_unseen:] == 0).all()) and bool((r[:, first_unseen:] == 0).all()), (what, name, "keys no query sees")


_ATTNB_REF = {}


def _attnb_ref(dtype, hd, shape, B, H, prob=0):
    """(inputs, fp64 reference) of one problem, computed once per session and left unchanged."""
    key = (dtype, hd, shape, B, H, prob)
    if key not in _ATTNB_REF:
        inp = attnb_inputs(dtype, hd, shape, B, H, prob)
        _ATTNB_REF[key] = (inp, attention_bwd_ref64(inp))
    return _ATTNB_REF[key]


def _attnb_case(monkeypatch, tune, dtype, hd, shape, B=ATTNB_B, H=ATTNB_H, n=1):
    """n problems in one launch under `tune`, each against its reference; returns [(dQ, dK, dV, delta)] per problem."""
    built = [_attnb_ref(dtype, hd, shape, B, H, i) for i in range(n)]
    probs = _attnb_launch(monkeypatch, tune, dtype, [b[0] for b in built])
    for i, ((inp, ref), p) in enumerate(zip(built, probs)):
        _attnb_check(f"attn_bwd [{tune}] hd={hd} {shape} B*H={B * H}" + (f" problem {i} of {n}" if n > 1 else ""), dtype, inp, p, ref)
    return [(p["dQ"], p["dK"], p["dV"], p["delta"]) for p in probs]


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("hd", [16, 32])
@pytest.mark.parametrize("dtype", DTYPES)
def test_attention_backward_tile_edges_and_geometries(monkeypatch, dtype, hd):
    """The benchmark's head dims at every shape of the section: lengths on and beside the 64-row tile and the 16-row wave edges, src_len one wave high,
    every key visible with the identity rotary table, Tq != Tk with q_pos0 > 0, key tiles no query sees, queries past the last key, one element."""
    for shape in ATTNB_SHAPES:
        _attnb_case(monkeypatch, None, dtype, hd, shape)


@pytest.mark.parametrize("hd", [16, 32])
@pytest.mark.parametrize("dtype", DTYPES)
def test_attention_backward_scores_far_below_zero_stay_finite(monkeypatch, dtype, hd):
    """Every LSE below -128: 2^(0 - LSE) of a zero-filled tile row past Tk overflows before the mask zeroes it, and every output must still be finite.
    (Finiteness only: the common component that pushes the scores down is 5 x as long as the rest of a key and multiplies every rounding of dS into
    dQ, so the section's tolerances, made for well-conditioned operands, do not apply; fp32 measured 6e-5 on dQ.)"""
    inp = attnb_inputs(dtype, hd, ATTNB_FAR[0], ATTNB_B, ATTNB_H)
    p = _attnb_launch(monkeypatch, None, dtype, [inp])[0]
    assert float(p["LSE"].max()) < -128
    for k in ("O", "LSE", "delta", "dQ", "dK", "dV"):
        assert torch.isfinite(p[k].float()).all(), k
    assert frame_untouched(p["dQbig"], ATTNB_H * hd)


@pytest.mark.parametrize("hd", ATTNB_HDS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_attention_backward_head_dims(monkeypatch, dtype, hd):
    """Every other exact head dim and the masked widths 24 and 96 on a length beside a tile edge, on full visibility and on a chunk at the end of a cache."""
    for shape in ATTNB_HD_SHAPES:
        _attnb_case(monkeypatch, None, dtype, hd, shape)


@pytest.mark.parametrize("B,H", ATTNB_MODE_BH)
@pytest.mark.parametrize("hd", [16, 32])
@pytest.mark.parametrize("dtype", DTYPES)
def test_attention_backward_forced_modes(monkeypatch, dtype, hd, B, H):
    """attnb_mode 0 .. 3 (1: XCD-local order, taken at B * H = 8 and falling back at 3; 2: paired tiles — at (40, 200) the paired dK / dV tile sees no query
    and skips its loop): the noted mode bits are the forced ones, every mode meets the reference and is bitwise mode 0 (no atomics)."""
    for shape in ATTNB_MODE_SHAPES:
        plain = _attnb_case(monkeypatch, "attnb_mode=0", dtype, hd, shape, B, H)
        for mode in (1, 2, 3):
            assert _same(plain[0], _attnb_case(monkeypatch, f"attnb_mode={mode}", dtype, hd, shape, B, H)[0]), (mode, shape)


@pytest.mark.parametrize("n", [3, 8])
@pytest.mark.parametrize("dtype", DTYPES)
def test_attention_backward_problems_of_one_launch(monkeypatch, dtype, n):
    """Three and SEA_MAX_ATTN_PROBLEMS problems with different tensors in one launch (grid.z): each against its own reference, and bitwise what the same
    problem gives when it is launched alone."""
    for shape in ATTNB_MULTI_SHAPES:
        together = _attnb_case(monkeypatch, None, dtype, 16, shape, n=n)
        for i, outs in enumerate(together):
            inp, _ = _attnb_ref(dtype, 16, shape, ATTNB_B, ATTNB_H, i)
            alone = _attnb_launch(monkeypatch, None, dtype, [inp])[0]
            assert _same(outs, (alone["dQ"], alone["dK"], alone["dV"], alone["delta"])), (shape, n, i)


@pytest.mark.parametrize("dtype", DTYPES)
def test_attention_backward_with_dropout(monkeypatch, dtype):
    """Dropout of the probabilities (thr = 64, p = 0.25) on two problems with every key visible: the mask is sea_dropout_mask's (equal to its host
    restatement, which the emulated bounds use); global and per-row checks as everywhere."""
    from tests.test_dropout_gpu import mask

    c = ATTNB_DROP
    inps, refs = [], []
    for i in range(c["n"]):
        inp = attnb_inputs(dtype, c["hd"], c["shape"], ATTNB_B, ATTNB_H, i)
        D = attnb_drop_factors(inp, i, c["seed"], c["stream"], c["thr"])
        for h in range(ATTNB_H):   # the same elements kept; the scale to an fp32 ulp (the device's quotient 256 / (256 - thr) need not be correctly rounded)
            m = mask(inp["Tq"], inp["Tk"], c["seed"], (c["stream"] + i) * ATTNB_B * ATTNB_H + h, c["thr"]).double()
            assert torch.equal(m > 0, D[0, h] > 0), (i, h, int(((m > 0) != (D[0, h] > 0)).sum()))
            assert float((m - D[0, h]).abs().max()) <= 2.0 ** -22, (i, h, float((m - D[0, h]).abs().max()))
        inps.append(inp)
        refs.append(attention_bwd_ref64(inp, D))
    probs = _attnb_launch(monkeypatch, None, dtype, inps, drop=(c["seed"], c["stream"], c["thr"]))
    for i, (inp, ref, p) in enumerate(zip(inps, refs, probs)):
        _attnb_check(f"attn_bwd dropout thr={c['thr']} hd={c['hd']} {c['shape']} problem {i}", dtype, inp, p, ref, drop=True)


# ------------------------------------------------------------------------------------------------ sea_wgrad_grouped
def _wgrad_operands(dtype, M, N_, K, seed):
    dY = rnd(M, N_ + 16, dtype=dtype, seed=seed + 1)[:, 8:8 + N_]   # strided
    X = rnd(M, K, dtype=dtype, seed=seed + 2)
    return dY, X, dY.double().t() @ X.double(), dY.double().sum(0)


def _wgrad(monkeypatch, tune, dtype, dY, X, dW, db, overwrite, form, a=None, b=None):
    from sea_amd import ops

    force(monkeypatch, tune)
    ops.wgrad_grouped([dict(dY=dY, X=X, dW=dW, db=db, overwrite=overwrite)], dtype)
    got = ops.last_form()
    torch.cuda.synchronize()
    assert got[0] == form, (tune, got)
    assert a is None or (got[1] == a if isinstance(a, int) else a(got[1])), (tune, got)
    assert b is None or got[2] == b, (tune, got)
    return got


def _check_wgrad(dW, db, ref_w, ref_b, what):
    check(dW, ref_w, what=what + " dW")
    check(db, ref_b, what=what + " db")


@pytest.mark.parametrize("M,N_,K", [(77, 16, 8), (200, 72, 136)])
@pytest.mark.parametrize("dtype", DTYPES)
def test_wgrad_tile64_element_store(monkeypatch, dtype, M, N_, K):
    """One split, every 64-tile partial: overwrite = 1 takes the element store (b = 1); on a zeroed dW it gives what the adding form gives.  db always adds."""
    dY, X, rw, rb = _wgrad_operands(dtype, M, N_, K, seed=4000 + M)
    db0 = rnd(N_, seed=4003)
    outs = []
    for ov in (1, 0):
        dW, db = torch.zeros(N_, K, device=dev()), db0.clone()
        _wgrad(monkeypatch, None, dtype, dY, X, dW, db, ov, "wgrad.tile64", a=1, b=ov)
        _check_wgrad(dW, db, rw, rb + db0.double(), f"wgrad.tile64 overwrite={ov}")
        outs.append(dW)
    assert rel(outs[0], outs[1]) < 2e-5
    # the documented contract: with one split, overwrite = 1 REPLACES what dW held ...
    dW, db = rnd(N_, K, seed=4004), db0.clone()
    _wgrad(monkeypatch, None, dtype, dY, X, dW, db, 1, "wgrad.tile64", a=1, b=1)
    _check_wgrad(dW, db, rw, rb + db0.double(), "wgrad.tile64 overwrite=1 on a pre-filled dW")


@pytest.mark.parametrize("dtype", DTYPES)
def test_wgrad_tile128_staged_store(monkeypatch, dtype):
    """(M 200, N 2048, K 8192): 1024 whole 128-tiles, one split by the launcher's cost rule.  overwrite = 1 leaves through LDS as whole rows (wgrad_stage=1)
    or as dwords (wgrad_stage=0): only the copy-out differs — bitwise equal; both equal the adding form.  A dW view whose row stride is no multiple of 4 floats,
    and one that starts 4 bytes off a 16-byte boundary, cannot take the float4 copy-out: right all the same, and nothing around the view is touched."""
    M, N_, K = 200, 2048, 8192
    dY, X, rw, rb = _wgrad_operands(dtype, M, N_, K, seed=4100)
    db0 = rnd(N_, seed=4103)
    outs = {}
    for tune, ov in (("wgrad_stage=1", 1), ("wgrad_stage=0", 1), (None, 0)):
        dW, db = torch.zeros(N_, K, device=dev()), db0.clone()
        _wgrad(monkeypatch, tune, dtype, dY, X, dW, db, ov, "wgrad.tile128", a=1, b=ov)
        _check_wgrad(dW, db, rw, rb + db0.double(), f"wgrad.tile128 [{tune}] overwrite={ov}")
        outs[(tune, ov)] = dW
    assert torch.equal(outs[("wgrad_stage=1", 1)], outs[("wgrad_stage=0", 1)])
    assert rel(outs[("wgrad_stage=1", 1)], outs[(None, 0)]) < 2e-5
    del outs
    wide = torch.full((N_, K + 3), 7.0, device=dev())                 # lddw = K + 3
    _wgrad(monkeypatch, "wgrad_stage=1", dtype, dY, X, wide[:, :K], db0.clone(), 1, "wgrad.tile128", a=1, b=1)
    check(wide[:, :K], rw, what="wgrad.tile128 lddw % 4 != 0 dW")
    assert bool((wide[:, K:] == 7.0).all())
    flat = torch.full((N_ * K + 8,), 7.0, device=dev())               # the view starts at float 1
    _wgrad(monkeypatch, "wgrad_stage=1", dtype, dY, X, flat[1:1 + N_ * K].view(N_, K), db0.clone(), 1, "wgrad.tile128", a=1, b=1)
    check(flat[1:1 + N_ * K].view(N_, K), rw, what="wgrad.tile128 dW 4 bytes off dW")
    assert float(flat[0]) == 7.0 and bool((flat[1 + N_ * K:] == 7.0).all())


@pytest.mark.parametrize("dtype", DTYPES)
def test_wgrad_overwrite_with_splits_adds(monkeypatch, dtype):
    """(M 2381, N 256, K 256) splits the contraction: several workgroups contribute to an element, so overwrite = 1 must NOT store (b = 0) — the caller has
    zeroed dW — and a pre-filled dW comes back as its content plus the product."""
    M, N_, K = 2381, 256, 256
    dY, X, rw, rb = _wgrad_operands(dtype, M, N_, K, seed=4200)
    db0 = rnd(N_, seed=4203)
    dW, db = torch.zeros(N_, K, device=dev()), db0.clone()
    _wgrad(monkeypatch, None, dtype, dY, X, dW, db, 1, "wgrad.tile64", a=lambda s: s > 1, b=0)
    _check_wgrad(dW, db, rw, rb + db0.double(), "wgrad.tile64 splits overwrite=1")
    dW0 = rnd(N_, K, scale=30.0, seed=4204)
    dW, db = dW0.clone(), db0.clone()
    _wgrad(monkeypatch, None, dtype, dY, X, dW, db, 1, "wgrad.tile64", a=lambda s: s > 1, b=0)
    _check_wgrad(dW, db, rw + dW0.double(), rb + db0.double(), "wgrad.tile64 splits overwrite=1 pre-filled")


@pytest.mark.parametrize("overwrite", [0, 1])
def test_wgrad_tile256(monkeypatch, overwrite):
    """The opt-in 256 x 128 tile (bf16, N a multiple of 256, K of 128); in fp32, or at N = 384, the launcher falls back to a square tile."""
    M, N_, K = 300, 512, 256
    dY, X, rw, rb = _wgrad_operands(BF, M, N_, K, seed=4300)
    db0 = rnd(N_, seed=4303)
    dW, db = torch.zeros(N_, K, device=dev()), db0.clone()
    got = _wgrad(monkeypatch, "wgrad_tile=256", BF, dY, X, dW, db, overwrite, "wgrad.tile256")
    assert got[2] == int(overwrite == 1 and got[1] == 1), got
    _check_wgrad(dW, db, rw, rb + db0.double(), f"wgrad.tile256 overwrite={overwrite}")
    for dtype, n in ((torch.float32, 512), (BF, 384)):
        dY, X, rw, rb = _wgrad_operands(dtype, M, n, K, seed=4310 + n)
        dW, db = torch.zeros(n, K, device=dev()), torch.zeros(n, device=dev())
        _wgrad(monkeypatch, "wgrad_tile=256", dtype, dY, X, dW, db, overwrite, "wgrad.tile64")
        _check_wgrad(dW, db, rw, rb, f"wgrad_tile=256 fallback {dtype} N={n}")


if __name__ == "__main__":   # the emulation behind ATTN_LOCAL, on the CPU
    worst = {"O": 0.0, "O_row": 0.0, "LSE": 0.0}
    cases = [(hd, key, shape, 0) for hd in (8, 16, 32, 64) for key, shapes in (("O", ATTN_SHAPES + ATTN_SHORT), ("O_row", ATTN_ROW)) for shape in shapes]
    cases += [(hd, "O", (257, 257, 0, 0), 100 * i) for hd in (32, 128) for i in range(3)]   # the three problems of one launch
    for hd, key, (Tq, Tk, q_pos0, src_len), seed in cases:
        Q, K, Vt, _ = attn_inputs(BF, hd, Tq, Tk, q_pos0, src_len, device="cpu", seed=seed)
        Oref, Lref = attention_ref64(Q, K, Vt, q_pos0, src_len, Tk)
        Oe, Le = attention_ref64(Q, K, Vt, q_pos0, src_len, Tk, round_p=BF if key == "O" else None, round_o=BF)
        eo, elv = rowerr(attn_rows(Oe, hd), attn_rows(Oref, hd)), rowerr(Le.reshape(-1, 1), Lref.reshape(-1, 1))
        print(f"hd={hd} {(Tq, Tk, q_pos0, src_len)} seed {seed}: O local {eo:.3e}  LSE local {elv:.3e}  (global O {rel(Oe, Oref):.3e}, LSE {rel(Le, Lref):.3e})")
        worst[key] = max(worst[key], eo)
        if key == "O":
            worst["LSE"] = max(worst["LSE"], elv)
    print({k: f"{v:.3e}" for k, v in worst.items()})

    # the emulation behind ATTNB_LOCAL; with no rounding it must restate the autograd reference
    def emulate(what, inp, D, suffix):
        ref, exact, emu = attention_bwd_ref64(inp, D), attention_bwd_emulated(inp, D, rt=None), attention_bwd_emulated(inp, D)
        line = []
        for name in ("dQ", "dK", "dV"):
            assert float((exact[name] - ref[name]).norm()) <= 1e-12 * max(float(ref[name].norm()), 1.0), (what, name)
            if float(ref[name].norm()) == 0:
                line.append(f"{name} reference 0")
                continue
            e = rowerr(emu[name].reshape(-1, inp["hd"]), ref[name].reshape(-1, inp["hd"]))
            line.append(f"{name} local {e:.3e} (global {rel(emu[name], ref[name]):.3e})")
            if e > worstb[name + suffix][0]:
                worstb[name + suffix] = (e, what)
        print(f"{what}: " + "  ".join(line))

    worstb = {k: (0.0, "") for k in ATTNB_LOCAL}
    for hd, shape, B, H, n in attnb_cases():
        for i in range(n):
            emulate(f"attn_bwd hd={hd} {shape} B*H={B * H} problem {i} of {n}", attnb_inputs(BF, hd, shape, B, H, i, device="cpu"), None, "")
    c = ATTNB_DROP
    for i in range(c["n"]):
        inp = attnb_inputs(BF, c["hd"], c["shape"], ATTNB_B, ATTNB_H, i, device="cpu")
        emulate(f"attn_bwd dropout hd={c['hd']} {c['shape']} problem {i}", inp, attnb_drop_factors(inp, i, c["seed"], c["stream"], c["thr"]), "_drop")
    for k, (v, what) in worstb.items():
        print(f"ATTNB_LOCAL[{k!r}]: measured {v:.3e} ({what}); the constant is 3 * {ATTNB_LOCAL[k] / 3:.3e}")
