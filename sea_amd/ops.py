"""Tensor-level wrappers over the C ABI (include/sea_hip.h).

Each ABI struct has ONE filler here (fill_*): it writes the struct's fields from torch tensors (device memory owned by PyTorch)
and plain values, and validates nothing.  The eager wrappers check their operands, call the fillers and launch on the current
stream: they are the un-fused building blocks used by the module mirrors in sea_amd/models/base_blocks.py, by the spatial
autoencoder's training step and by the operator tests.  The plans (sea_amd/engine.py, train_engine.py, kv_engine.py) call the
same fillers once per plan for the whole-model path.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, Optional, Sequence

import torch

from . import _native as N


def _mat(t: torch.Tensor, name: str) -> torch.Tensor:
    N.require_gpu(t, name)
    if t.dim() != 2 or t.stride(1) != 1:
        raise ValueError(f"{name}: need a 2-D tensor with unit inner stride, got shape {tuple(t.shape)} strides {t.stride()}")
    return t


def fill_gemm_group(g: N.SeaGemmGroup, A, W, bias=None, R=None, C32=None, Cact=None, n_seg=1, a_seg_stride=0, act=0,
                    bias_scale=1.0, M=None, N_=None, K=None, Z=None, silu=None, drop=None, ldr=None, ldc32=None) -> None:
    """A: the rows are its last two axes; None with M given (a few-row launch's norm prologue supplies them) or with `silu`.  ldr / ldc32: row strides
    of R / C32 other than their own (a strided view of the caller's tensor)."""
    if silu is not None:   # generated A operand: dict(c f32 [M] — None: patched at bind time, M given —, w1 f32 [K], b1 f32 [K]): A[m, k] = silu(w1[k] c[m] + b1[k])
        c = silu.get("c")
        g.silu_c, g.silu_w1, g.silu_b1 = N.ptr(c), silu["w1"].data_ptr(), silu["b1"].data_ptr()
        A, R, Z, n_seg, a_seg_stride, act = None, None, None, 1, 0, 0
        M = c.numel() if M is None else M
    g.A, g.lda = (A.data_ptr(), A.stride(-2)) if A is not None else (None, 0)
    g.W, g.ldw = W.data_ptr(), W.stride(0)
    g.bias = N.ptr(bias)
    g.R, g.C32, g.Cact = N.ptr(R), N.ptr(C32), N.ptr(Cact)
    g.Z, g.ldz = N.ptr(Z), (Z.stride(0) if Z is not None else 0)
    g.a_seg_stride = a_seg_stride
    g.ldr = (ldr if ldr is not None else R.stride(0)) if R is not None else 0
    g.ldc32 = (ldc32 if ldc32 is not None else C32.stride(0)) if C32 is not None else 0
    g.ldcact = Cact.stride(0) if Cact is not None else 0
    g.M = A.shape[-2] if M is None else M
    g.N = W.shape[0] if N_ is None else N_
    g.K = W.shape[1] if K is None else K
    g.n_seg = n_seg
    g.act = act
    g.bias_scale = bias_scale
    if drop is not None:   # (seed, stream, thr, mode): counter-based dropout of the epilogue (include/sea_hip.h, SeaDropout); a plan's seed is re-keyed every step
        g.drop.seed, g.drop.stream, g.drop.thr, g.drop.mode = drop


def gemm_grouped(groups: Sequence[Dict], dtype: torch.dtype) -> None:
    """groups: dicts with A [M,K] act, W [N,K] act, optional bias f32 [N], R f32 [M,N], C32 f32 [M,N], Cact act [M,N],
    n_seg, a_seg_stride, act (0|1), bias_scale."""
    n = len(groups)
    arr = (N.SeaGemmGroup * n)()
    for i, d in enumerate(groups):
        if d.get("silu") is not None:
            W = _mat(d["W"], "W")
            if W.dtype != dtype:
                raise ValueError(f"gemm group {i}: W dtype {W.dtype} != activation dtype {dtype}")
            fill_gemm_group(arr[i], None, W, d.get("bias"), None, d.get("C32"), d.get("Cact"), bias_scale=d.get("bias_scale", 1.0), silu=d["silu"])
            continue
        A, W = _mat(d["A"], "A"), _mat(d["W"], "W")
        if A.dtype != dtype or W.dtype != dtype:
            raise ValueError(f"gemm group {i}: A/W dtype {A.dtype}/{W.dtype} != activation dtype {dtype}")
        for k in ("bias", "R", "C32"):
            if d.get(k) is not None and d[k].dtype != torch.float32:
                raise ValueError(f"gemm group {i}: {k} must be float32")
        if d.get("Cact") is not None and d["Cact"].dtype != dtype:
            raise ValueError(f"gemm group {i}: Cact dtype mismatch")
        fill_gemm_group(arr[i], A, W, d.get("bias"), d.get("R"), d.get("C32"), d.get("Cact"), d.get("n_seg", 1),
                        d.get("a_seg_stride", 0), d.get("act", 0), d.get("bias_scale", 1.0), K=d.get("K"), Z=d.get("Z"), drop=d.get("drop"))
    N.check(N.lib().sea_gemm_grouped(arr, n, N.dtype_code(dtype), N.stream_ptr()), "sea_gemm_grouped")


def last_form():
    """(form, a, b) of the calling thread's last noted launch — which kernel sea_gemm_grouped / sea_gemm_rownorm / sea_attention_fwd / sea_attention_bwd /
    sea_wgrad_grouped, the row-owning launches (MLP, sea_gemm_adaln, sea_exchange_tail, sea_row_chain, sea_adaln_qkv) and the few-row launches took
    (include/sea_hip.h, sea_last_form): sea_gemm_fewrows ("gemv.gemm", MR, KC), sea_qkv_rope_fewrows ("gemv.qkv", MR, KC), sea_qkv_rope_grouped ("qkv.skinny" /
    "qkv.tile"), sea_rownorm (("rownorm.fewrows", KM, 0) / "rownorm.ln_rows" / "rownorm.wave"), the one-row attention ("attn.row", 1 at head dims >= 64 else 0, 0);
    ("", 0, 0) before any.  For the tests that force a form."""
    a, b = C.c_int(0), C.c_int(0)
    name = N.lib().sea_last_form(C.byref(a), C.byref(b))
    return (name.decode() if name else ""), a.value, b.value


LOG2E = 1.4426950408889634


def q_scale(hd: int) -> float:
    """The factor the QKV epilogue puts on (rotated) q for the attention kernels: hd^-1/2 (reference models/base_blocks.py:191) times log2(e) — the
    attention kernels work in log2 units (P = 2^(S - max): one v_exp_f32 per probability, the subtraction in the MFMA's C operand), see sea_hip.h."""
    return float(hd) ** -0.5 * LOG2E


def fill_qkv_group(g: N.SeaQkvGroup, A, W, bias=None, Q=None, K=None, Vt=None, V=None, col0=0, M=None) -> None:
    """A act [M, K] (None in a few-row launch with a norm prologue: M given), W act [N, K], the attention operands Q / K / Vt / V (sea_hip.h, SeaQkvGroup)."""
    g.A, g.lda = (A.data_ptr(), A.stride(0)) if A is not None else (None, 0)
    g.W, g.ldw, g.bias = W.data_ptr(), W.stride(0), N.ptr(bias)
    g.Qout, g.Kout, g.Vtout, g.Vout = N.ptr(Q), N.ptr(K), N.ptr(Vt), N.ptr(V)
    g.M, g.N, g.K = (A.shape[0] if M is None else M), W.shape[0], W.shape[1]
    g.col0 = col0


def qkv_rope_grouped(groups: Sequence[Dict], rope: torch.Tensor, H: int, hd: int, T: int, pos0: int, cap: int,
                     q_scale: float, dtype: torch.dtype) -> None:
    """groups: dicts with A [M,K], W [N,K], bias f32 [N], col0, Q/K/Vt output tensors (see sea_hip.h)."""
    n = len(groups)
    arr = (N.SeaQkvGroup * n)()
    for i, d in enumerate(groups):
        A, W = _mat(d["A"], "A"), _mat(d["W"], "W")
        if A.dtype != dtype or W.dtype != dtype:
            raise ValueError(f"qkv group {i}: dtype mismatch")
        fill_qkv_group(arr[i], A, W, d.get("bias"), d.get("Q"), d.get("K"), d.get("Vt"), d.get("V"), d.get("col0", 0))
    N.require_gpu(rope, "rope")
    assert rope.dtype == torch.float32 and rope.is_contiguous() and rope.shape[-1] == 2 and rope.shape[-2] == hd // 2
    assert rope.shape[0] >= pos0 + T, "rope table shorter than pos0 + T"
    common = N.SeaQkvCommon(rope.data_ptr(), H, hd, T, pos0, cap, q_scale)
    N.check(N.lib().sea_qkv_rope_grouped(arr, n, C.byref(common), N.dtype_code(dtype), N.stream_ptr()), "sea_qkv_rope_grouped")


def fill_attn_params(P: N.SeaAttnParams, problems: Sequence[Dict], B: int, H: int, hd: int, Tq: int, Tk: int, cap: int, q_pos0: int, src_len: int, ldo: int,
                     drop=None) -> None:
    """problems: dicts with Q, K, Vt, O, optional LSE (see attention_fwd); drop = (seed, first stream, thr): problem i on stream + i."""
    P.n_problems = len(problems)
    for p, d in zip(P.p, problems):
        p.Q, p.K, p.Vt, p.O, p.LSE = d["Q"].data_ptr(), d["K"].data_ptr(), d["Vt"].data_ptr(), d["O"].data_ptr(), N.ptr(d.get("LSE"))
    P.B, P.H, P.hd, P.Tq, P.Tk, P.cap, P.q_pos0, P.src_len, P.ldo = B, H, hd, Tq, Tk, cap, q_pos0, src_len, ldo
    if drop is not None:   # dropout of the attention probabilities
        P.drop.seed, P.drop.stream, P.drop.thr = drop


def attention_fwd(problems: Sequence[Dict], B: int, H: int, hd: int, Tq: int, Tk: int, cap: int, q_pos0: int,
                  src_len: int, dtype: torch.dtype, drop=None) -> None:
    """problems: dicts with Q [B,H,Tq,hd], K [B,H,cap,hd], Vt [B,H,hd,cap], O [B,Tq,H*hd] (row stride = O.stride(1)),
    optional LSE f32 [B,H,Tq]."""
    ldo = None
    for i, d in enumerate(problems):
        for k in ("Q", "K", "Vt", "O"):
            N.require_gpu(d[k], k)
            assert d[k].dtype == dtype, f"attention problem {i}: {k} dtype"
        assert d["Q"].is_contiguous() and d["K"].is_contiguous() and d["Vt"].is_contiguous()
        O = d["O"]
        assert O.dim() == 3 and O.stride(2) == 1 and O.stride(0) == Tq * O.stride(1)
        ldo = O.stride(1) if ldo is None else ldo
        assert O.stride(1) == ldo
    P = N.SeaAttnParams()
    fill_attn_params(P, problems, B, H, hd, Tq, Tk, cap, q_pos0, src_len, ldo, drop)   # drop: (seed, first stream, thr)
    N.check(N.lib().sea_attention_fwd(C.byref(P), N.dtype_code(dtype), N.stream_ptr()), "sea_attention_fwd")


def fill_norm_group(g: N.SeaNormGroup, gd: Dict) -> None:
    """gd: X, optional mod act [M, 2d], gamma f32 [d], optional beta f32 [d], Y32 and/or Yact, optional mean / rstd f32 [M], addend / Xout (include/sea_hip.h, SeaNormGroup)."""
    X = gd["X"]
    g.X, g.ldx = X.data_ptr(), gd.get("ldx", X.stride(0) if X.dim() == 2 else 0)
    mod = gd.get("mod")
    g.mod, g.ldmod = N.ptr(mod), (mod.stride(0) if mod is not None else 0)
    g.gamma, g.beta = gd["gamma"].data_ptr(), N.ptr(gd.get("beta"))
    y32, yact = gd.get("Y32"), gd.get("Yact")
    g.Y32, g.ldy32 = N.ptr(y32), gd.get("ldy32", y32.stride(0) if y32 is not None else 0)
    g.Yact, g.ldyact = N.ptr(yact), (yact.stride(0) if yact is not None else 0)
    g.mean, g.rstd = N.ptr(gd.get("mean")), N.ptr(gd.get("rstd"))
    add, xout = gd.get("addend"), gd.get("Xout")
    g.addend, g.ldadd = N.ptr(add), (add.stride(0) if add is not None else 0)
    g.Xout, g.ldxout = N.ptr(xout), (xout.stride(0) if xout is not None else 0)


def rownorm(groups: Sequence[Dict], M: int, d: int, x_is_act: bool, gelu: bool, eps: float, dtype: torch.dtype) -> None:
    """groups: dicts with X [M,d], optional mod act [M,2d], gamma f32 [d], optional beta f32 [d], Y32 and/or Yact,
    optional mean/rstd f32 [M]."""
    n = len(groups)
    arr = (N.SeaNormGroup * n)()
    for i, gd in enumerate(groups):
        X = _mat(gd["X"], "X")
        assert X.dtype == (dtype if x_is_act else torch.float32)
        fill_norm_group(arr[i], gd)
    N.check(N.lib().sea_rownorm(arr, n, M, d, int(x_is_act), int(gelu), eps, N.dtype_code(dtype), N.stream_ptr()), "sea_rownorm")


def fewrows_supported(dtype: torch.dtype, M: int, Ks: Sequence[int], qkv: bool = False, pre: bool = False) -> bool:
    """Do sea_gemm_fewrows / sea_qkv_rope_fewrows (gemv.hip) cover a launch of these groups?  bf16, M <= 4 rows per group, one K per launch out of N.FEW_K
    (<= 2048 for the q/k/v form and for a norm prologue)."""
    Ks = list(Ks)
    return (dtype == torch.bfloat16 and 1 <= M <= 4 and 1 <= len(Ks) <= N.FEW_MAX_GROUPS and all(k == Ks[0] for k in Ks) and Ks[0] in N.FEW_K
            and (Ks[0] <= 2048 or not (qkv or pre)))


def _norm_array(specs: Optional[Sequence[Optional[Dict]]], n: int):
    if specs is None or all(sp is None for sp in specs):
        return None
    arr = (N.SeaNormGroup * n)()
    for g, sp in zip(arr, specs):
        if sp is not None:
            fill_norm_group(g, sp)
    return arr


def gemm_fewrows(groups: Sequence[Dict], dtype: torch.dtype, pre=None, pre_x_is_act: bool = False, pre_gelu: bool = False, eps: float = 1e-5) -> None:
    """sea_gemm_fewrows: groups as gemm_grouped (A may be None where pre[i] is given); pre: list of rownorm group dicts or None per group (fp32 rows, or —
    pre_x_is_act — rows in the activation dtype with a plain LayerNorm, optionally followed by GELU)."""
    n = len(groups)
    arr = (N.SeaGemmGroup * n)()
    for i, d in enumerate(groups):
        W = _mat(d["W"], "W")
        A = d.get("A")
        fill_gemm_group(arr[i], (_mat(A, "A") if A is not None else None), W, d.get("bias"), d.get("R"), d.get("C32"), d.get("Cact"), act=d.get("act", 0),
                        bias_scale=d.get("bias_scale", 1.0), M=(pre[i]["X"].shape[0] if A is None else None), Z=d.get("Z"))
    N.check(N.lib().sea_gemm_fewrows(arr, _norm_array(pre, n), n, int(pre_x_is_act), int(pre_gelu), eps, N.dtype_code(dtype), N.stream_ptr()), "sea_gemm_fewrows")


def qkv_rope_fewrows(groups: Sequence[Dict], rope: torch.Tensor, H: int, hd: int, T: int, pos0: int, cap: int, q_scale: float, dtype: torch.dtype, pre=None,
                     eps: float = 1e-5) -> None:
    """sea_qkv_rope_fewrows: groups as qkv_rope_grouped (A may be None where pre[i] is given, then 'M' gives the rows)."""
    n = len(groups)
    arr = (N.SeaQkvGroup * n)()
    for i, d in enumerate(groups):
        A = d.get("A")
        fill_qkv_group(arr[i], A, _mat(d["W"], "W"), d.get("bias"), d.get("Q"), d.get("K"), d.get("Vt"), d.get("V"), d.get("col0", 0),
                       M=(None if A is not None else pre[i]["X"].shape[0]))
    common = N.SeaQkvCommon(rope.data_ptr(), H, hd, T, pos0, cap, q_scale)
    N.check(N.lib().sea_qkv_rope_fewrows(arr, _norm_array(pre, n), n, C.byref(common), eps, N.dtype_code(dtype), N.stream_ptr()), "sea_qkv_rope_fewrows")


def fill_gemm_norm_group(g: N.SeaGemmNormGroup, A, W, gamma, bias=None, R=None, C32=None, mod=None, beta=None, Y32=None, Yact=None,
                         mean=None, rstd=None, ldr=None, ldy32=None, n_seg=1, a_seg_stride=0, bias_scale=1.0, Cact=None, ib=None, K=None) -> None:
    """ib: dict(c, w1, b1, lnw, lnb, w2 [N, h], b2, h) — the info-bottleneck addend (sea_hip.h, SeaGemmNormGroup)."""
    g.A, g.W, g.bias, g.R, g.C32 = A.data_ptr(), W.data_ptr(), N.ptr(bias), N.ptr(R), N.ptr(C32)
    g.mod, g.gamma, g.beta = N.ptr(mod), gamma.data_ptr(), N.ptr(beta)
    g.Y32, g.Yact, g.mean, g.rstd = N.ptr(Y32), N.ptr(Yact), N.ptr(mean), N.ptr(rstd)
    g.lda, g.ldw = A.stride(0), W.stride(0)
    g.ldr = (ldr if ldr is not None else R.stride(0)) if R is not None else 0
    g.ldc32 = C32.stride(0) if C32 is not None else 0
    g.ldmod = mod.stride(0) if mod is not None else 0
    g.ldy32 = (ldy32 if ldy32 is not None else Y32.stride(0)) if Y32 is not None else 0
    g.ldyact = Yact.stride(0) if Yact is not None else 0
    g.M, g.N, g.K = A.shape[0], W.shape[0], (W.shape[1] if K is None else K)
    g.n_seg, g.a_seg_stride, g.bias_scale = n_seg, a_seg_stride, bias_scale
    g.Cact, g.ldcact = N.ptr(Cact), (Cact.stride(0) if Cact is not None else 0)
    if ib is not None:
        g.ib_c, g.ib_w1, g.ib_b1, g.ib_lnw, g.ib_lnb = N.ptr(ib.get("c")), ib["w1"].data_ptr(), ib["b1"].data_ptr(), ib["lnw"].data_ptr(), ib["lnb"].data_ptr()
        g.ib_w2, g.ib_b2, g.ib_h = ib["w2"].data_ptr(), ib["b2"].data_ptr(), ib["h"]


def gemm_rownorm(groups: Sequence[Dict], eps: float, dtype: torch.dtype) -> None:
    """Linear + row normalisation in one launch (sea_gemm_rownorm).  groups: dicts with A [M,K] act, W [N,K] act (N <= 256, N % 16 == 0),
    gamma f32 [N], optional bias f32 [N], R f32 [M,N], C32 f32 [M,N] (pre-norm), mod act [M,2N], beta f32 [N], Y32 / Yact, mean / rstd."""
    n = len(groups)
    arr = (N.SeaGemmNormGroup * n)()
    for i, d in enumerate(groups):
        A, W = _mat(d["A"], "A"), _mat(d["W"], "W")
        if A.dtype != dtype or W.dtype != dtype:
            raise ValueError(f"gemm_rownorm group {i}: A/W dtype {A.dtype}/{W.dtype} != activation dtype {dtype}")
        if d.get("Yact") is not None and d["Yact"].dtype != dtype:
            raise ValueError(f"gemm_rownorm group {i}: Yact dtype mismatch")
        if d.get("mod") is not None and d["mod"].dtype != dtype:
            raise ValueError(f"gemm_rownorm group {i}: mod dtype mismatch")
        fill_gemm_norm_group(arr[i], A, W, d["gamma"], d.get("bias"), d.get("R"), d.get("C32"), d.get("mod"), d.get("beta"), d.get("Y32"),
                             d.get("Yact"), d.get("mean"), d.get("rstd"), n_seg=d.get("n_seg", 1), a_seg_stride=d.get("a_seg_stride", 0),
                             bias_scale=d.get("bias_scale", 1.0), Cact=d.get("Cact"), ib=d.get("ib"))
    N.check(N.lib().sea_gemm_rownorm(arr, n, eps, N.dtype_code(dtype), N.stream_ptr()), "sea_gemm_rownorm")


def fill_exchange_tail(P: N.SeaExchangeTail, att: Sequence[torch.Tensor], Wp: Sequence[torch.Tensor], Wup, bup, bias_scale: float, X, Xact=None,
                       down: Optional[Dict] = None) -> None:
    """att: n_seg act [M, D] matrices, Wp: n_seg act [D, D]; Wup act [E, D]; X f32 [M, E] (in place); down: dict(W [D, E], bias, gamma, beta, mod, Yact, Y32)."""
    for s, a in enumerate(att):
        P.att[s] = a.data_ptr()
        P.Wp[s] = Wp[s].data_ptr()
    P.n_seg, P.ldatt, P.ldwp = len(att), att[0].stride(0), Wp[0].stride(0)
    P.Wup, P.ldwup, P.bup, P.bias_scale = Wup.data_ptr(), Wup.stride(0), N.ptr(bup), bias_scale
    P.X, P.ldx = X.data_ptr(), X.stride(0)
    P.Xact, P.ldxact = N.ptr(Xact), (Xact.stride(0) if Xact is not None else 0)
    P.M, P.E, P.D = X.shape[0], Wup.shape[0], Wup.shape[1]
    P.has_down = int(down is not None)
    if down is not None:
        g = P.down
        g.W, g.ldw, g.bias = down["W"].data_ptr(), down["W"].stride(0), N.ptr(down.get("bias"))
        g.gamma, g.beta = down["gamma"].data_ptr(), N.ptr(down.get("beta"))
        mod, y32, yact = down.get("mod"), down.get("Y32"), down.get("Yact")
        g.mod, g.ldmod = N.ptr(mod), (mod.stride(0) if mod is not None else 0)
        g.Y32, g.ldy32 = N.ptr(y32), (y32.stride(0) if y32 is not None else 0)
        g.Yact, g.ldyact = N.ptr(yact), (yact.stride(0) if yact is not None else 0)
        g.mean, g.rstd = N.ptr(down.get("mean")), N.ptr(down.get("rstd"))


def exchange_tail_supported(dtype: torch.dtype, D: int, E: int, n_seg: int) -> bool:
    """Shapes sea_exchange_tail instantiates (include/sea_hip.h)."""
    return dtype == torch.bfloat16 and (D, E) in ((128, 256), (64, 128)) and 1 <= n_seg and n_seg * D <= 256


def exchange_tail(att, Wp, Wup, bup, bias_scale, X, Xact=None, down=None, eps: float = 1e-5, dtype: torch.dtype = torch.bfloat16) -> None:
    """One field's exchange tail in one launch: X += sum_s gelu(att_s Wp_s^T) Wup^T + bias_scale * bup; optionally the down-projection + row norm
    of the updated rows (sea_exchange_tail)."""
    for t in list(att) + list(Wp) + [Wup, X]:
        N.require_gpu(t, "exchange_tail operand")
    P = (N.SeaExchangeTail * 1)()
    fill_exchange_tail(P[0], att, Wp, Wup, bup, bias_scale, X, Xact, down)
    N.check(N.lib().sea_exchange_tail(P, 1, eps, N.dtype_code(dtype), N.stream_ptr()), "sea_exchange_tail")


def exchange_tail_grouped(groups: Sequence[Dict], eps: float = 1e-5, dtype: torch.dtype = torch.bfloat16) -> None:
    """Several problems of one shape in one launch (grid row per group): dicts with the arguments of exchange_tail."""
    P = (N.SeaExchangeTail * len(groups))()
    for p_, d in zip(P, groups):
        fill_exchange_tail(p_, d["att"], d["Wp"], d["Wup"], d.get("bup"), d.get("bias_scale", 1.0), d["X"], d.get("Xact"), d.get("down"))
    N.check(N.lib().sea_exchange_tail(P, len(groups), eps, N.dtype_code(dtype), N.stream_ptr()), "sea_exchange_tail")


def fill_adaln_group(g: N.SeaAdalnGroup, A, W, bias=None, X=None, gamma=None, beta=None, Yact=None, Y32=None, mean=None, rstd=None, ldx=None, ldy32=None) -> None:
    """One group of sea_gemm_adaln: A act [M, K] (silu rows), W act [2d, K] (cond_mlp.2.weight); X f32 [M, d] + gamma (+ beta) -> Yact / Y32 [M, d], or — X None —
    Yact act [M, 2d] receives the modulation itself."""
    g.A, g.lda, g.W, g.ldw, g.bias = A.data_ptr(), A.stride(0), W.data_ptr(), W.stride(0), N.ptr(bias)
    g.X, g.ldx = N.ptr(X), ((ldx if ldx is not None else X.stride(0)) if X is not None else 0)
    g.gamma, g.beta = N.ptr(gamma), N.ptr(beta)
    g.Yact, g.ldyact = N.ptr(Yact), (Yact.stride(0) if Yact is not None else 0)
    g.Y32, g.ldy32 = N.ptr(Y32), ((ldy32 if ldy32 is not None else Y32.stride(0)) if Y32 is not None else 0)
    g.mean, g.rstd = N.ptr(mean), N.ptr(rstd)
    g.M, g.d, g.K = A.shape[0], W.shape[0] // 2, W.shape[1]


def gemm_adaln(groups: Sequence[Dict], eps: float = 1e-5, dtype: torch.dtype = torch.bfloat16) -> None:
    """sea_gemm_adaln: AdaLN as the epilogue of cond_mlp.2's GEMM (dict keys: the arguments of fill_adaln_group)."""
    arr = (N.SeaAdalnGroup * len(groups))()
    for g, d in zip(arr, groups):
        fill_adaln_group(g, **d)
    N.check(N.lib().sea_gemm_adaln(arr, len(groups), eps, N.dtype_code(dtype), N.stream_ptr()), "sea_gemm_adaln")


def adaln_qkv_supported(dtype: torch.dtype, E: int, H: int) -> bool:
    """Shapes sea_adaln_qkv instantiates (include/sea_hip.h): bf16, E = 256, head dim 16 or 32."""
    return dtype == torch.bfloat16 and E == 256 and H > 0 and E % H == 0 and E // H in (16, 32)


def fill_adaln_qkv(g: N.SeaAdalnQkv, X, cond, w1, b1, W2c, b2c, gamma, beta, Wqkv, bqkv, Q, K, Vt, ldx=None, third=None, memo=None) -> None:
    """One group of sea_adaln_qkv: X f32 [M, E] (row stride ldx), cond f32 [M], cond_mlp.0 (w1, b1 f32 [2E]), cond_mlp.2 (W2c act [2E, 2E], b2c), AdaLN_0's gamma / beta,
    [Wq; Wk; Wv] act [3E, E] + bias, the attention operands Q [B,H,T,hd] / K [B,H,cap,hd] / Vt [B,H,hd,cap].  memo: dict(stamps int32 [M, 2] zeroed once, mods act
    [M, 2E], epoch int32 [1], count int32 [2], rows int32 [n_silu + 1, M, 2] zeroed once: the row riders' stamps, group 0 only) — the condition memo, buffers the caller keeps between launches (None: no memo, the pointers stay NULL)."""
    if memo is not None:
        st, tab = memo["stamps"], memo["mods"]
        if st.dtype != torch.int32 or tuple(st.shape) != (X.shape[0], 2) or not st.is_contiguous() or tab.shape[0] != X.shape[0] or tab.shape[1] != W2c.shape[0] or tab.stride(1) != 1:
            raise ValueError(f"adaln_qkv memo: stamps {tuple(st.shape)} {st.dtype} / mods {tuple(tab.shape)} do not fit M = {X.shape[0]}, 2E = {W2c.shape[0]}")
        g.memo_stamps, g.memo_mods, g.ldmemo = st.data_ptr(), tab.data_ptr(), tab.stride(0)
        g.memo_epoch, g.memo_count, g.memo_rows = memo["epoch"].data_ptr(), N.ptr(memo.get("count")), N.ptr(memo.get("rows"))
    g.X, g.ldx, g.cond = X.data_ptr(), (ldx if ldx is not None else X.stride(0)), N.ptr(cond)
    g.w1, g.b1, g.W2c, g.ldw2c, g.b2c = w1.data_ptr(), b1.data_ptr(), W2c.data_ptr(), W2c.stride(0), N.ptr(b2c)
    g.gamma, g.beta, g.Wqkv, g.ldw, g.bqkv = gamma.data_ptr(), N.ptr(beta), Wqkv.data_ptr(), Wqkv.stride(0), N.ptr(bqkv)
    g.Q, g.K, g.Vt = Q.data_ptr(), K.data_ptr(), Vt.data_ptr()
    g.M, g.E = X.shape[0], Wqkv.shape[1]
    if third is not None:   # dict(w1, b1 f32 [N3], W act [N3, N3], bias f32 [N3] or None, out act [M, N3]): the modulation of another AdaLN module of the same rows
        W3, o3 = third["W"], third["out"]
        g.w13, g.b13, g.W3, g.ldw3, g.b3 = third["w1"].data_ptr(), third["b1"].data_ptr(), W3.data_ptr(), W3.stride(0), N.ptr(third.get("bias"))
        g.mod3, g.ldmod3, g.N3 = o3.data_ptr(), o3.stride(0), W3.shape[0]


def adaln_qkv(groups: Sequence[Dict], rope: torch.Tensor, H: int, hd: int, T: int, pos0: int, cap: int, q_scale: float, riders: Sequence[Dict] = (), silu: Sequence[Dict] = (),
              silu_c: Optional[torch.Tensor] = None, eps: float = 1e-5, dtype: torch.dtype = torch.bfloat16, ib: Optional[Dict] = None) -> None:
    """sea_adaln_qkv: the front of a block in one launch (dict keys: the arguments of fill_adaln_qkv); `riders`: plain GEMM groups (A, W, bias, Cact) as sea_gemm_grouped's;
    `silu`: row riders as sea_silu_outer's groups (w1, b1, Hid) evaluated on silu_c; `ib`: the information-bottleneck row rider (the arguments of fill_ib_params: its
    rows xs[0] are stored, evaluated on silu_c too)."""
    arr = (N.SeaAdalnQkv * len(groups))()
    for g, d in zip(arr, groups):
        fill_adaln_qkv(g, **d)
    c = N.SeaQkvCommon()
    c.rope, c.H, c.hd, c.T, c.pos0, c.cap, c.q_scale = rope.data_ptr(), H, hd, T, pos0, cap, q_scale
    rarr = None
    if riders:
        rarr = (N.SeaGemmGroup * len(riders))()
        for g, d in zip(rarr, riders):
            fill_gemm_group(g, **d)
    sarr = None
    if silu:
        sarr = (N.SeaSiluGroup * len(silu))()
        for g, gd in zip(sarr, silu):
            fill_silu_group(g, gd["w1"], gd["b1"], gd["Hid"])
    ibp = None
    if ib is not None:
        ibp = N.SeaIbParams()
        fill_ib_params(ibp, **ib)
    N.check(N.lib().sea_adaln_qkv(arr, len(groups), C.byref(c), rarr, len(riders), sarr, len(silu), (silu_c.data_ptr() if silu_c is not None else None),
                                  (silu_c.numel() if silu_c is not None else 0), (C.byref(ibp) if ibp is not None else None), eps, N.dtype_code(dtype), N.stream_ptr()),
            "sea_adaln_qkv")


def row_chain_supported(dtype: torch.dtype, D: int, E: int, n_seg: int, hd: int) -> bool:
    """Shapes sea_row_chain instantiates (include/sea_hip.h): bf16, (D, E) in {(128, 256), (64, 128)}, n_seg * D <= E, cross head dim 16 or 32."""
    return dtype == torch.bfloat16 and (D, E) in ((128, 256), (64, 128)) and 0 <= n_seg and n_seg * D <= E and hd in (16, 32)


def fill_row_chain(P: N.SeaRowChain, W2, Xin, X, att: Sequence[torch.Tensor] = (), Wp: Sequence[torch.Tensor] = (), a2=None, b2=None, bias_scale: float = 1.0, Xact=None,
                   down: Optional[Dict] = None, proj: Sequence[Dict] = (), ldxin: Optional[int] = None, tile_memo: Optional[Dict] = None) -> None:
    """One group of sea_row_chain.  Form A: a2 act [M, E], W2 act [E, E]; form B: att / Wp lists (n_seg act [M, D] / [D, D]), W2 act [E, D].  Xin f32 [M, E] (row
    stride ldxin when given: the caller's strided tensor), X f32 [M, E]; down: dict(W [D, E], bias, gamma, beta, mod, Yact, Y32); proj: dicts(W [N, D], bias, col0, Q / K / Vt / V).
    tile_memo (group 0 of a launch with riders): dict(stamps int32 [tiles, 128, 2] zeroed once, one set per rider tile; cond f32 [M] or None: patched in later; epoch
    int32 [1]; count int32 [2] or None) — the rider tiles' condition memo, buffers the caller keeps between launches (None: no memo, the pointers stay NULL)."""
    if tile_memo is not None:
        st = tile_memo["stamps"]
        if st.dtype != torch.int32 or st.dim() != 3 or tuple(st.shape[1:]) != (128, 2) or not st.is_contiguous():
            raise ValueError(f"row_chain tile memo: stamps {tuple(st.shape)} {st.dtype}: int32 [tiles, 128, 2], one set per rider tile")
        P.tile_stamps, P.tile_sets = st.data_ptr(), st.shape[0]
        P.tile_cond, P.tile_epoch, P.tile_count = N.ptr(tile_memo.get("cond")), tile_memo["epoch"].data_ptr(), N.ptr(tile_memo.get("count"))
    for s_, a in enumerate(att):
        P.att[s_] = a.data_ptr()
        P.Wp[s_] = Wp[s_].data_ptr()
    P.n_seg = len(att)
    if att:
        P.ldatt, P.ldwp = att[0].stride(0), Wp[0].stride(0)
    if a2 is not None:
        P.a2, P.lda2 = a2.data_ptr(), a2.stride(0)
    P.W2, P.ldw2, P.b2, P.bias_scale = W2.data_ptr(), W2.stride(0), N.ptr(b2), bias_scale
    P.Xin, P.ldxin = Xin.data_ptr(), (ldxin if ldxin is not None else Xin.stride(0))
    P.X, P.ldx = X.data_ptr(), X.stride(0)
    P.Xact, P.ldxact = N.ptr(Xact), (Xact.stride(0) if Xact is not None else 0)
    P.M, P.E = X.shape[0], W2.shape[0]
    P.D = P.E // 2
    P.has_down = int(down is not None)
    if down is not None:
        g = P.down
        g.W, g.ldw, g.bias = down["W"].data_ptr(), down["W"].stride(0), N.ptr(down.get("bias"))
        g.gamma, g.beta = down["gamma"].data_ptr(), N.ptr(down.get("beta"))
        mod, y32, yact = down.get("mod"), down.get("Y32"), down.get("Yact")
        g.mod, g.ldmod = N.ptr(mod), (mod.stride(0) if mod is not None else 0)
        g.Y32, g.ldy32 = N.ptr(y32), (y32.stride(0) if y32 is not None else 0)
        g.Yact, g.ldyact = N.ptr(yact), (yact.stride(0) if yact is not None else 0)
        g.mean, g.rstd = N.ptr(down.get("mean")), N.ptr(down.get("rstd"))
        g.M, g.N, g.K, g.n_seg = P.M, P.D, P.E, 1   # (the launcher sets them again; here for the pointer audit's extents)
    if len(proj) > N.CHAIN_MAX_PROJ:
        raise ValueError(f"row_chain: {len(proj)} projection entries (at most {N.CHAIN_MAX_PROJ})")
    P.n_proj = len(proj)
    for q, d in zip(P.proj, proj):
        W = d["W"]
        q.A, q.lda, q.M = None, 0, P.M
        q.W, q.ldw, q.bias = W.data_ptr(), W.stride(0), N.ptr(d.get("bias"))
        q.N, q.K, q.col0 = W.shape[0], W.shape[1], d.get("col0", 0)
        q.Qout, q.Kout, q.Vtout, q.Vout = N.ptr(d.get("Q")), N.ptr(d.get("K")), N.ptr(d.get("Vt")), N.ptr(d.get("V"))


def row_chain(groups: Sequence[Dict], rope: Optional[torch.Tensor] = None, H: int = 1, hd: int = 4, T: int = 1, pos0: int = 0, cap: int = 0, q_scale_: float = 1.0,
              eps: float = 1e-5, dtype: torch.dtype = torch.bfloat16, riders: Optional[Sequence[Dict]] = None, tile0: Optional[int] = None, n_tiles: Optional[int] = None,
              ib: Optional[Dict] = None) -> None:
    """sea_row_chain: the row-local chain between two attention launches for up to three groups (fields) of one shape (dict keys: the arguments of fill_row_chain).
    With any of riders / tile0 / n_tiles / ib: sea_row_chain_riders — `riders`: plain GEMM groups (the arguments of fill_gemm_group: A, W, bias, Cact) cut into
    128 x 128 tiles numbered group by group, of which this launch runs [tile0, tile0 + n_tiles) (all of them unless given); `ib`: the information-bottleneck
    rows (the arguments of fill_ib_params: xs[0] is stored)."""
    P = (N.SeaRowChain * len(groups))()
    for p_, d in zip(P, groups):
        fill_row_chain(p_, **d)
    common = N.SeaQkvCommon(N.ptr(rope), H, hd, T, pos0, cap, q_scale_) if rope is not None else None
    cref = C.byref(common) if common is not None else None
    if riders is None and tile0 is None and n_tiles is None and ib is None:
        N.check(N.lib().sea_row_chain(P, len(groups), cref, eps, N.dtype_code(dtype), N.stream_ptr()), "sea_row_chain")
        return
    riders = list(riders or ())
    rarr = (N.SeaGemmGroup * len(riders))() if riders else None
    total = 0
    for g, d in zip(rarr or (), riders):
        fill_gemm_group(g, **d)
        total += ((g.M + 127) // 128) * ((g.N + 127) // 128)
    tile0 = 0 if tile0 is None else tile0
    n_tiles = total - tile0 if n_tiles is None else n_tiles
    ibp = None
    if ib is not None:
        ibp = N.SeaIbParams()
        fill_ib_params(ibp, **ib)
    N.check(N.lib().sea_row_chain_riders(P, len(groups), cref, rarr, len(riders), tile0, n_tiles, (C.byref(ibp) if ibp is not None else None), eps, N.dtype_code(dtype),
                                         N.stream_ptr()), "sea_row_chain_riders")


def fill_silu_group(g: N.SeaSiluGroup, w1, b1, Hid) -> None:
    """Hid act [M, K2] = silu(w1[k] c[m] + b1[k]); w1, b1 f32 [K2]."""
    g.w1, g.b1, g.Hid, g.K2, g.ld = w1.data_ptr(), b1.data_ptr(), Hid.data_ptr(), Hid.shape[1], Hid.stride(0)


def silu_outer(groups: Sequence[Dict], c: torch.Tensor, M: int, dtype: torch.dtype) -> None:
    """groups: dicts with w1 f32 [K2], b1 f32 [K2], Hid act [M,K2]."""
    n = len(groups)
    arr = (N.SeaSiluGroup * n)()
    for g, gd in zip(arr, groups):
        fill_silu_group(g, gd["w1"], gd["b1"], _mat(gd["Hid"], "Hid"))
    N.require_gpu(c, "c")
    assert c.dtype == torch.float32 and c.is_contiguous() and c.numel() == M
    N.check(N.lib().sea_silu_outer(arr, n, c.data_ptr(), M, N.dtype_code(dtype), N.stream_ptr()), "sea_silu_outer")


def fill_ib_params(P: N.SeaIbParams, xs: Sequence[torch.Tensor], c, w1, b1=None, lnw=None, lnb=None, w2=None, b2=None, mode: int = 0, M=None, E=None,
                   drop=None) -> None:
    """xs: f32 [M, E] matrices of equal row stride (M, E: their shape unless given); c f32 [M] (None: patched at bind time).  The layer by ib mode
    (models/temporal.py:103-109): 0 the MLP (w1, b1, lnw, lnb f32 [h], w2 f32 [E, h], b2 f32 [E]); 1 nn.Linear(1, E) (w1 = weight [E, 1], b1 = bias);
    2 GaussianFourierProjection (w1 = W [1, E/2]).  drop = (seed, first stream, thr): dropout of the layer's output, field i on stream + i."""
    for i, x in enumerate(xs):
        P.X[i] = x.data_ptr()
    P.n_fields, P.ldx = len(xs), xs[0].stride(0)
    P.mode, P.M, P.E = mode, (xs[0].shape[0] if M is None else M), (xs[0].shape[1] if E is None else E)
    P.c, P.w1, P.b1, P.lnw, P.lnb, P.w2, P.b2 = N.ptr(c), w1.data_ptr(), N.ptr(b1), N.ptr(lnw), N.ptr(lnb), N.ptr(w2), N.ptr(b2)
    P.h = w1.numel() if mode == 0 else 1
    if drop is not None:
        P.drop.seed, P.drop.stream, P.drop.thr = drop


def ib_add(xs: Sequence[torch.Tensor], c: torch.Tensor, w1, b1, lnw, lnb, w2, b2, drop=None) -> None:
    """xs: f32 [M,E] matrices (equal row stride) updated in place: x += W2 gelu(LN(w1 c + b1)) + b2; drop = (seed, first stream, thr): dropout of the MLP output,
    field i on stream + i."""
    M, E = xs[0].shape
    for x in xs:
        _mat(x, "x")
        assert x.dtype == torch.float32 and x.shape == (M, E) and x.stride(0) == xs[0].stride(0)
    for t in (c, w1, b1, lnw, lnb, w2, b2):
        N.require_gpu(t, "ib parameter")
        assert t.dtype == torch.float32 and t.is_contiguous()
    assert c.numel() == M and w2.shape == (E, w1.numel())
    P = N.SeaIbParams()
    fill_ib_params(P, xs, c, w1, b1, lnw, lnb, w2, b2, drop=drop)
    N.check(N.lib().sea_ib_add(C.byref(P), N.stream_ptr()), "sea_ib_add")


def convert(src: torch.Tensor, dst: torch.Tensor) -> None:
    """dst[r, c] = (dst dtype) src[r, c]; src float32, 2-D with unit inner stride."""
    src, dst = _mat(src, "src"), _mat(dst, "dst")
    assert src.dtype == torch.float32 and src.shape == dst.shape
    N.check(N.lib().sea_convert_f32_to_act(src.data_ptr(), src.stride(0), dst.data_ptr(), dst.stride(0), src.shape[0],
                                           src.shape[1], N.dtype_code(dst.dtype), N.stream_ptr()), "sea_convert_f32_to_act")


# ------------------------------------------------------------------------------------------------ backward wrappers
def fill_wgrad_group(g: N.SeaWgradGroup, dY, X, dW, db=None, M=None, overwrite=0) -> None:
    """dW f32 [N, K] (+)= dY^T X over M rows (those of dY unless given); db f32 [N] (+)= the column sums of dY.  overwrite = 1: dW holds zeros (or
    nothing worth keeping) and this group is its only contribution — the kernel may store instead of adding when it does not split the contraction."""
    g.overwrite = int(overwrite)
    g.dY, g.X, g.dW, g.db = dY.data_ptr(), X.data_ptr(), dW.data_ptr(), N.ptr(db)
    g.lddy, g.ldx, g.lddw = dY.stride(0), X.stride(0), dW.stride(0)
    g.M, g.N, g.K = (dY.shape[0] if M is None else M), dW.shape[0], dW.shape[1]


def wgrad_grouped(groups: Sequence[Dict], dtype: torch.dtype) -> None:
    """groups: dicts with dY act [M,N], X act [M,K], dW f32 [N,K] (accumulated), optional db f32 [N] (accumulated), optional overwrite (0 | 1, default 0:
    include/sea_hip.h, SeaWgradGroup)."""
    n = len(groups)
    arr = (N.SeaWgradGroup * n)()
    for g, d in zip(arr, groups):
        dY, X, dW = _mat(d["dY"], "dY"), _mat(d["X"], "X"), _mat(d["dW"], "dW")
        assert dY.dtype == dtype and X.dtype == dtype and dW.dtype == torch.float32
        assert X.shape[0] == dY.shape[0] and dW.shape == (dY.shape[1], X.shape[1])
        fill_wgrad_group(g, dY, X, dW, d.get("db"), overwrite=d.get("overwrite", 0))
    N.check(N.lib().sea_wgrad_grouped(arr, n, N.dtype_code(dtype), N.stream_ptr()), "sea_wgrad_grouped")


def fill_norm_bwd_group(g: N.SeaNormBwdGroup, gd: Dict) -> None:
    """gd: dY, X (row strides lddy / ldx when given: a strided view of the caller's tensor), optional mod / dmod, gamma, optional beta, the forward's
    mean / rstd, dX32 and / or dXact, optional dgamma / dbeta (include/sea_hip.h, SeaNormBwdGroup)."""
    dY, X = gd["dY"], gd["X"]
    g.dY, g.lddy = dY.data_ptr(), gd.get("lddy", dY.stride(0))
    g.X, g.ldx = X.data_ptr(), gd.get("ldx", X.stride(0))
    mod, dmod = gd.get("mod"), gd.get("dmod")
    g.mod, g.ldmod = N.ptr(mod), (mod.stride(0) if mod is not None else 0)
    g.dmod, g.lddmod = N.ptr(dmod), (dmod.stride(0) if dmod is not None else 0)
    g.gamma, g.beta = gd["gamma"].data_ptr(), N.ptr(gd.get("beta"))
    g.mean, g.rstd = gd["mean"].data_ptr(), gd["rstd"].data_ptr()
    dx32, dxa = gd.get("dX32"), gd.get("dXact")
    g.dX32, g.lddx32 = N.ptr(dx32), (dx32.stride(0) if dx32 is not None else 0)
    g.dXact, g.lddxact = N.ptr(dxa), (dxa.stride(0) if dxa is not None else 0)
    g.dgamma, g.dbeta = N.ptr(gd.get("dgamma")), N.ptr(gd.get("dbeta"))


def rownorm_bwd(groups: Sequence[Dict], M: int, d: int, dy_is_act: bool, x_is_act: bool, gelu: bool, accumulate: bool,
                dtype: torch.dtype, ws: Optional[torch.Tensor] = None) -> None:
    n = len(groups)
    arr = (N.SeaNormBwdGroup * n)()
    for g, gd in zip(arr, groups):
        _mat(gd["dY"], "dY")
        _mat(gd["X"], "X")
        fill_norm_bwd_group(g, gd)
    N.check(N.lib().sea_rownorm_bwd(arr, n, M, d, int(dy_is_act), int(x_is_act), int(gelu), int(accumulate), N.dtype_code(dtype),
                                    N.ptr(ws), 0 if ws is None else ws.numel(), N.stream_ptr()), "sea_rownorm_bwd")


def fill_silu_bwd_group(g: N.SeaSiluBwdGroup, dHid, w1, b1, dw1, db1) -> None:
    """dw1 / db1 f32 [K2] (+)= the gradient of silu_outer's w1 / b1 from dHid act [M, K2]."""
    g.dHid, g.w1, g.b1, g.dw1, g.db1 = dHid.data_ptr(), w1.data_ptr(), b1.data_ptr(), dw1.data_ptr(), db1.data_ptr()
    g.K2, g.ld = dHid.shape[1], dHid.stride(0)


def silu_outer_bwd(groups: Sequence[Dict], c: torch.Tensor, M: int, dtype: torch.dtype, ws: Optional[torch.Tensor] = None) -> None:
    n = len(groups)
    arr = (N.SeaSiluBwdGroup * n)()
    for g, gd in zip(arr, groups):
        fill_silu_bwd_group(g, _mat(gd["dHid"], "dHid"), gd["w1"], gd["b1"], gd["dw1"], gd["db1"])
    N.check(N.lib().sea_silu_outer_bwd(arr, n, c.data_ptr(), M, N.dtype_code(dtype), N.ptr(ws), 0 if ws is None else ws.numel(),
                                       N.stream_ptr()), "sea_silu_outer_bwd")


def silu_outer_bwd_dc(groups: Sequence[Dict], c: torch.Tensor, dc: torch.Tensor, M: int, dtype: torch.dtype, ws: Optional[torch.Tensor] = None) -> None:
    """silu_outer_bwd (the same dw1 / db1) that also adds the condition gradient into dc f32 [M] (sea_silu_outer_bwd_dc).  ws: f32 workspace, sized here
    when not given."""
    n = len(groups)
    arr = (N.SeaSiluBwdGroup * n)()
    for g, gd in zip(arr, groups):
        fill_silu_bwd_group(g, _mat(gd["dHid"], "dHid"), gd["w1"], gd["b1"], gd["dw1"], gd["db1"])
    if ws is None:   # the dc partials and the column sums of as many row splits as the column form runs (TrainPlan._silu_bwd sizes it the same way)
        ncb = sum((g.K2 + 255) // 256 for g in arr)
        rs = max(1, min((1024 + ncb - 1) // ncb, (M + 15) // 16))
        ws = torch.empty(ncb * M + n * rs * 2 * max(g.K2 for g in arr), device=c.device, dtype=torch.float32)
    N.check(N.lib().sea_silu_outer_bwd_dc(arr, n, c.data_ptr(), dc.data_ptr(), M, N.dtype_code(dtype), ws.data_ptr(), ws.numel(), N.stream_ptr()),
            "sea_silu_outer_bwd_dc")


def fill_ib_bwd_params(P: N.SeaIbBwdParams, dxs: Sequence[torch.Tensor], c, w1=None, b1=None, lnw=None, lnb=None, w2=None, dw1=None, db1=None, dlnw=None,
                       dlnb=None, dw2=None, db2=None, ws=None, dhid=None, mode: int = 0, M=None, E=None, drop=None) -> None:
    """dxs: f32 [M, E] gradients of the rows fill_ib_params's layer was added to (M, E: their shape unless given); c f32 [M] (None: patched at bind time).
    mode 0 (the MLP): its parameters and their f32 gradients (accumulated); ws / dhid select the column-block form (see ib_bwd); drop as fill_ib_params's.
    mode 1 (nn.Linear(1, E)): dw1 / db1 only."""
    for i, x in enumerate(dxs):
        P.dX[i] = x.data_ptr()
    P.n_fields, P.ldx = len(dxs), dxs[0].stride(0)
    P.mode, P.M, P.E = mode, (dxs[0].shape[0] if M is None else M), (dxs[0].shape[1] if E is None else E)
    P.c, P.w1, P.b1, P.lnw, P.lnb, P.w2 = N.ptr(c), N.ptr(w1), N.ptr(b1), N.ptr(lnw), N.ptr(lnb), N.ptr(w2)
    P.dw1, P.db1, P.dlnw, P.dlnb, P.dw2, P.db2 = N.ptr(dw1), N.ptr(db1), N.ptr(dlnw), N.ptr(dlnb), N.ptr(dw2), N.ptr(db2)
    P.h = w1.numel() if mode == 0 else 0
    if ws is not None and dhid is not None:
        P.ws, P.ws_floats, P.dhid = ws.data_ptr(), ws.numel(), dhid.data_ptr()
    if drop is not None:
        P.drop.seed, P.drop.stream, P.drop.thr = drop


def ib_bwd(dxs: Sequence[torch.Tensor], c, w1, b1, lnw, lnb, w2, dw1, db1, dlnw, dlnb, dw2, db2, ws: Optional[torch.Tensor] = None,
           dhid: Optional[torch.Tensor] = None) -> None:
    """ws (f32, >= E (1 + h) floats per row split) and dhid (f32 [M, 8], zero on entry) select the column-block form (h <= 8)."""
    for x in dxs:
        _mat(x, "dx")
        assert x.dtype == torch.float32 and x.stride(0) == dxs[0].stride(0)
    P = N.SeaIbBwdParams()
    fill_ib_bwd_params(P, dxs, c, w1, b1, lnw, lnb, w2, dw1, db1, dlnw, dlnb, dw2, db2, ws, dhid)
    N.check(N.lib().sea_ib_bwd(C.byref(P), N.stream_ptr()), "sea_ib_bwd")


def ib_bwd_dc(dxs: Sequence[torch.Tensor], c: torch.Tensor, dc: torch.Tensor, mode: int = 0, drop=None, **layer) -> None:
    """dc f32 [M] += the condition gradient of the information-bottleneck layer of `mode` (sea_ib_bwd_dc); `layer`: fill_ib_bwd_params's parameter
    and gradient keywords (with dw1 given, modes 0 / 1 also accumulate the parameter gradients, as ib_bwd)."""
    for x in dxs:
        _mat(x, "dx")
        assert x.dtype == torch.float32 and x.stride(0) == dxs[0].stride(0)
    P = N.SeaIbBwdParams()
    fill_ib_bwd_params(P, dxs, c, mode=mode, drop=drop, **layer)
    N.check(N.lib().sea_ib_bwd_dc(C.byref(P), dc.data_ptr(), N.stream_ptr()), "sea_ib_bwd_dc")


def transpose_weights(src_flat: torch.Tensor, dst_flat: torch.Tensor, desc: torch.Tensor, tile_start: torch.Tensor) -> None:
    """desc int64 [n,4] (src_off, dst_off, rows, cols) and tile_start int32 [n+1] live on the device."""
    n = desc.shape[0]
    total = int(tile_start[-1].item()) if not hasattr(tile_start, "_sea_total") else tile_start._sea_total
    N.check(N.lib().sea_transpose_weights(src_flat.data_ptr(), dst_flat.data_ptr(), N.dtype_code(dst_flat.dtype), desc.data_ptr(),
                                          tile_start.data_ptr(), n, total, N.stream_ptr()), "sea_transpose_weights")


def fill_attn_bwd_params(P: N.SeaAttnBwdParams, problems: Sequence[Dict], rope, B: int, H: int, hd: int, Tq: int, Tk: int, cap: int, q_pos0: int, src_len: int,
                         q_scale: float, drop=None) -> None:
    """problems: dicts as attention_bwd's (the row strides are those of the first problem's O, dO, dQ, dK, dV); drop as fill_attn_params's."""
    P.n_problems = len(problems)
    for q, d in zip(P.p, problems):
        q.Q, q.K, q.V, q.O, q.dO = (d[k].data_ptr() for k in ("Q", "K", "V", "O", "dO"))
        q.LSE, q.delta = d["LSE"].data_ptr(), d["delta"].data_ptr()
        q.dQ, q.dK, q.dV = d["dQ"].data_ptr(), d["dK"].data_ptr(), d["dV"].data_ptr()
    d0 = problems[0]
    P.rope = rope.data_ptr()
    P.B, P.H, P.hd, P.Tq, P.Tk, P.cap, P.q_pos0, P.src_len = B, H, hd, Tq, Tk, cap, q_pos0, src_len
    P.ldo, P.lddo = d0["O"].stride(-2), d0["dO"].stride(-2)
    P.lddq, P.lddk, P.lddv = d0["dQ"].stride(-2), d0["dK"].stride(-2), d0["dV"].stride(-2)
    P.q_scale = q_scale
    if drop is not None:
        P.drop.seed, P.drop.stream, P.drop.thr = drop


def attention_bwd(problems: Sequence[Dict], rope: torch.Tensor, B: int, H: int, hd: int, Tq: int, Tk: int, cap: int, q_pos0: int,
                  src_len: int, q_scale: float, dtype: torch.dtype) -> None:
    """problems: dicts with Q, K, V (row-major), O, dO [B,Tq,H*hd], LSE, delta f32 [B,H,Tq], dQ/dK/dV act [B*T, >= H*hd]."""
    for d in problems:
        for k in ("Q", "K", "V", "O", "dO", "dQ", "dK", "dV"):
            N.require_gpu(d[k], k)
            assert d[k].dtype == dtype, k
    P = N.SeaAttnBwdParams()
    fill_attn_bwd_params(P, problems, rope, B, H, hd, Tq, Tk, cap, q_pos0, src_len, q_scale)
    N.check(N.lib().sea_attention_bwd(C.byref(P), N.dtype_code(dtype), N.stream_ptr()), "sea_attention_bwd")


def unpatchify(fields: torch.Tensor, layout: str, index_map: torch.Tensor, scale: torch.Tensor, shift: torch.Tensor, n_points: int,
               point_slot: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[b, index_map[p, c], f] = fields[b, p, f|c ...] * scale[f] + shift[f] (sea_unpatchify).  `layout` names the order of the last two
    axes of `fields`: "BPFC" (the decoder's output) or "BPCF" (the reference's inverse_scale_and_unpatch argument)."""
    N.require_gpu(fields, "fields")
    assert fields.dtype == torch.float32 and fields.dim() == 4 and layout in ("BPFC", "BPCF")
    assert index_map.dtype == torch.int32 and index_map.is_cuda and index_map.is_contiguous()
    B, P = fields.shape[0], fields.shape[1]
    F, Cc = (fields.shape[2], fields.shape[3]) if layout == "BPFC" else (fields.shape[3], fields.shape[2])
    sb, sp = fields.stride(0), fields.stride(1)
    sf, sc = (fields.stride(2), fields.stride(3)) if layout == "BPFC" else (fields.stride(3), fields.stride(2))
    assert tuple(index_map.shape) == (P, Cc) and scale.numel() == F and shift.numel() == F
    out = torch.empty(B, n_points, F, device=fields.device, dtype=torch.float32)
    if point_slot is not None:
        assert point_slot.dtype == torch.int32 and point_slot.is_cuda and point_slot.numel() == n_points
    N.check(N.lib().sea_unpatchify(fields.data_ptr(), sb, sp, sf, sc, index_map.data_ptr(), N.ptr(point_slot), scale.data_ptr(), shift.data_ptr(),
                                   out.data_ptr(), B, P, F, Cc, n_points, N.stream_ptr()), "sea_unpatchify")
    return out


def patchify(fields: torch.Tensor, index_map: torch.Tensor, scale: torch.Tensor, shift: torch.Tensor, layout: str = "BPFC", c_out: Optional[int] = None,
             pad_value: float = 0.0) -> torch.Tensor:
    """out[b, p, f, c] = fields[b, index_map[p, c], f] * scale[f] + shift[f], pad_value at empty / padded slots (sea_patchify).  fields f32
    [B, n_points, F]; `layout` of the result: "BPFC" (the encoder's input, C padded to c_out) or "BPCF" (the reference's stacked fields)."""
    N.require_gpu(fields, "fields")
    assert fields.dtype == torch.float32 and fields.dim() == 3 and fields.is_contiguous() and layout in ("BPFC", "BPCF")
    assert index_map.dtype == torch.int32 and index_map.is_cuda and index_map.is_contiguous()
    B, n_points, F = fields.shape
    P, C_map = index_map.shape
    C_out = C_map if c_out is None else c_out
    assert C_out >= C_map and scale.numel() == F and shift.numel() == F
    out = torch.empty((B, P, F, C_out) if layout == "BPFC" else (B, P, C_out, F), device=fields.device, dtype=torch.float32)
    sb, sp = out.stride(0), out.stride(1)
    sf, sc = (out.stride(2), out.stride(3)) if layout == "BPFC" else (out.stride(3), out.stride(2))
    N.check(N.lib().sea_patchify(fields.data_ptr(), index_map.data_ptr(), scale.data_ptr(), shift.data_ptr(), out.data_ptr(), sb, sp, sf, sc, B, P, F, C_map, C_out,
                                 n_points, pad_value, N.stream_ptr()), "sea_patchify")
    return out


def fill_splitk_group(g: N.SeaSplitkGroup, P, bias=None, bias_scale=1.0, R=None, C32=None, Cact=None) -> None:
    """P f32 [S, M, N]: the partial products; out = sum_s P[s] + bias * bias_scale + R into C32 and / or Cact."""
    g.P, g.p_stride, g.S, g.M, g.N, g.ldp = P.data_ptr(), P.stride(0), P.shape[0], P.shape[1], P.shape[2], P.stride(1)
    g.bias, g.bias_scale = N.ptr(bias), bias_scale
    g.R, g.ldr = N.ptr(R), (R.stride(0) if R is not None else 0)
    g.C32, g.ldc32 = N.ptr(C32), (C32.stride(0) if C32 is not None else 0)
    g.Cact, g.ldcact = N.ptr(Cact), (Cact.stride(0) if Cact is not None else 0)


def splitk_finish(groups: Sequence[Dict], dtype: torch.dtype) -> None:
    """sea_splitk_finish: out = sum_s P[s] + bias * bias_scale + R; dicts with P f32 [S, M, N], optional bias / bias_scale / R, outputs C32 and / or Cact."""
    arr = (N.SeaSplitkGroup * len(groups))()
    for g, d in zip(arr, groups):
        fill_splitk_group(g, d["P"], d.get("bias"), d.get("bias_scale", 1.0), d.get("R"), d.get("C32"), d.get("Cact"))
    N.check(N.lib().sea_splitk_finish(arr, len(groups), N.dtype_code(dtype), N.stream_ptr()), "sea_splitk_finish")


def mlp_fc1_supported(dtype: torch.dtype, E: int, S: int) -> bool:
    """Shapes sea_mlp_fc1_ln_gelu instantiates (include/sea_hip.h)."""
    return dtype == torch.bfloat16 and (E, S) in ((256, 2048), (128, 1024))


def fill_mlp_group(g: N.SeaMlpGroup, A, W1, b1, lnw, lnb, Hg, norm: Optional[Dict] = None) -> None:
    """norm (optional): dict(X32 f32 [M,E], gamma, beta=None, mod=None, addend=None, Xout=None, eps=1e-5) — the operand rows are normalised inside
    the launch from the fp32 residual stream (A is then None)."""
    g.W1, g.b1, g.lnw, g.lnb, g.Hg = W1.data_ptr(), b1.data_ptr(), lnw.data_ptr(), lnb.data_ptr(), N.ptr(Hg)   # (Hg None: sea_mlp_block)
    g.ldw, g.ldh = W1.stride(0), (Hg.stride(0) if Hg is not None else 0)
    g.E, g.S = W1.shape[1], W1.shape[0]
    if norm is None:
        g.A, g.lda, g.M = A.data_ptr(), A.stride(0), A.shape[0]
        g.X32 = None
        return
    X = norm["X32"]
    g.A, g.lda, g.M = None, 0, X.shape[0]
    g.X32, g.ldx32 = X.data_ptr(), X.stride(0)
    add, xout, mod = norm.get("addend"), norm.get("Xout"), norm.get("mod")
    g.addend, g.ldadd = N.ptr(add), (add.stride(0) if add is not None else 0)
    g.Xout, g.ldxout = N.ptr(xout), (xout.stride(0) if xout is not None else 0)
    g.mod, g.ldmod = N.ptr(mod), (mod.stride(0) if mod is not None else 0)
    g.gamma, g.beta = norm["gamma"].data_ptr(), N.ptr(norm.get("beta"))
    g.norm_eps = norm.get("eps", 1e-5)


def fill_mlp2_group(g: N.SeaMlp2Group, Hg, W2, b2, R, Wproj, bproj, Y32=None, Yact=None, gamma=None, beta=None, mod=None, ldy32=None, M=None) -> None:
    """Hg / R may be None for sea_mlp_block (hidden rows in registers; residual = the norm prologue's x + addend): M is then given."""
    g.Hg, g.W2, g.b2, g.R, g.Wproj, g.bproj = N.ptr(Hg), W2.data_ptr(), b2.data_ptr(), N.ptr(R), Wproj.data_ptr(), bproj.data_ptr()
    g.ldh, g.ldw2, g.ldr, g.ldwp = (Hg.stride(0) if Hg is not None else 0), W2.stride(0), (R.stride(0) if R is not None else 0), Wproj.stride(0)
    g.gamma, g.beta, g.mod, g.ldmod = N.ptr(gamma), N.ptr(beta), N.ptr(mod), (mod.stride(0) if mod is not None else 0)
    g.Y32, g.ldy32 = N.ptr(Y32), (ldy32 if ldy32 is not None else (Y32.stride(0) if Y32 is not None else 0))
    g.Yact, g.ldyact = N.ptr(Yact), (Yact.stride(0) if Yact is not None else 0)
    g.M, g.E, g.S = (Hg.shape[0] if Hg is not None else M), W2.shape[0], W2.shape[1]


def mlp_fc2_proj_norm(groups: Sequence[Dict], eps: float = 1e-5, dtype: torch.dtype = torch.bfloat16) -> None:
    """out = norm(proj(Hg W2^T + b2 + R)) in one launch (sea_mlp_fc2_proj_norm): dicts with Hg [M,S], W2 [E,S], b2, R f32 [M,E], Wproj [E,E], bproj,
    Y32 and / or Yact, optional gamma / beta / mod (no gamma: no norm)."""
    arr = (N.SeaMlp2Group * len(groups))()
    for g, d in zip(arr, groups):
        for k in ("Hg", "W2", "Wproj", "R"):
            _mat(d[k], k)
        fill_mlp2_group(g, d["Hg"], d["W2"], d["b2"], d["R"], d["Wproj"], d["bproj"], d.get("Y32"), d.get("Yact"), d.get("gamma"), d.get("beta"), d.get("mod"),
                        d.get("ldy32"))
    N.check(N.lib().sea_mlp_fc2_proj_norm(arr, len(groups), eps, N.dtype_code(dtype), N.stream_ptr()), "sea_mlp_fc2_proj_norm")


def mlp_block(groups: Sequence[Dict], eps: float = 1e-5, dtype: torch.dtype = torch.bfloat16) -> None:
    """The whole field MLP, proj and the final norm in one launch (sea_mlp_block): dicts with the keys of mlp_fc1_ln_gelu (A or norm, W1, b1, lnw, lnb) and of
    mlp_fc2_proj_norm (W2, b2, R — or None with a norm prologue —, Wproj, bproj, Y32 / Yact, optional gamma / beta / mod); no Hg."""
    a1, a2 = (N.SeaMlpGroup * len(groups))(), (N.SeaMlp2Group * len(groups))()
    for g1, g2, d in zip(a1, a2, groups):
        fill_mlp_group(g1, d.get("A"), d["W1"], d["b1"], d["lnw"], d["lnb"], None, d.get("norm"))
        fill_mlp2_group(g2, None, d["W2"], d["b2"], d.get("R"), d["Wproj"], d["bproj"], d.get("Y32"), d.get("Yact"), d.get("gamma"), d.get("beta"), d.get("mod"), d.get("ldy32"), M=g1.M)
    N.check(N.lib().sea_mlp_block(a1, a2, len(groups), eps, N.dtype_code(dtype), N.stream_ptr()), "sea_mlp_block")


def mlp_fc1_ln_gelu(groups: Sequence[Dict], eps: float = 1e-5, dtype: torch.dtype = torch.bfloat16) -> None:
    """Hg = gelu(LayerNorm(A W1^T + b1) * lnw + lnb) in one launch (sea_mlp_fc1_ln_gelu): dicts with A [M,E], W1 [S,E], b1, lnw, lnb f32 [S], Hg [M,S]."""
    arr = (N.SeaMlpGroup * len(groups))()
    for g, d in zip(arr, groups):
        for k in ("W1", "Hg") + (("A",) if d.get("norm") is None else ()):
            _mat(d[k], k)
        fill_mlp_group(g, d.get("A"), d["W1"], d["b1"], d["lnw"], d["lnb"], d["Hg"], d.get("norm"))
    N.check(N.lib().sea_mlp_fc1_ln_gelu(arr, len(groups), eps, N.dtype_code(dtype), N.stream_ptr()), "sea_mlp_fc1_ln_gelu")


# ------------------------------------------------------------------------------------------------ fused EncoderBlock (encoder_block.hip)
def encoder_block_supported(dtype: torch.dtype, W: int, H: int, P: int) -> bool:
    """The shapes sea_encoder_block_fwd / _bwd instantiate: bf16, W in {32, 64}, H = 8, P <= 128 (S = 4 W by construction)."""
    return dtype == torch.bfloat16 and W in (32, 64) and H == 8 and 1 <= P <= 128


def encoder_block_ws_floats(B: int, P: int, W: int) -> int:
    return int(N.lib().sea_encoder_block_ws_floats(B, P, W))


_ENC_BLOCK_FIELDS = ("Zin", "Zout", "wqkv", "bqkv", "wo", "w1", "b1", "lnw", "lnb", "w2", "b2", "g1", "g2", "dZout", "dZin",
                     "n1", "dqkv", "att", "dz1", "n2", "dh", "hg", "dz2", "u1", "u2", "u3w", "u3b")


def _encoder_block(fn_name: str, t: Dict, B: int, P: int, W: int, H: int, ws: torch.Tensor, eps: float, dtype: torch.dtype) -> None:
    """t: tensors by SeaEncBlock field name (include/sea_hip.h); every given tensor must be contiguous on the GPU."""
    st = N.SeaEncBlock()
    for k in _ENC_BLOCK_FIELDS:
        v = t.get(k)
        if v is not None:
            N.require_gpu(v, k)
            if not v.is_contiguous():
                raise ValueError(f"{fn_name}: {k} must be contiguous")
            setattr(st, k, v.data_ptr())
    N.require_gpu(ws, "ws")
    st.ws, st.ws_floats = ws.data_ptr(), ws.numel()
    st.B, st.P, st.W, st.H, st.eps = B, P, W, H, eps
    from . import ptrcheck

    if ptrcheck.always():
        from types import SimpleNamespace

        ranges = ptrcheck.Ranges()
        for k, v in list(t.items()) + [("ws", ws)]:
            ranges.add_tensor(v, k)
        ptrcheck.check_records([SimpleNamespace(fn=fn_name, args=(), keep=st, name=fn_name)], ranges, 2 if dtype == torch.bfloat16 else 4, fn_name)
    N.check(getattr(N.lib(), fn_name)(C.byref(st), N.dtype_code(dtype), N.stream_ptr()), fn_name)


def encoder_block_fwd(t: Dict, B: int, P: int, W: int, H: int, ws: torch.Tensor, eps: float = 1e-5, dtype: torch.dtype = torch.bfloat16) -> None:
    """Zout = EncoderBlock(Zin), one launch.  t: Zin, Zout and the block's weights (wqkv act [3W, W], bqkv, wo, w1, b1, lnw, lnb, w2, b2, g1, g2)."""
    _encoder_block("sea_encoder_block_fwd", t, B, P, W, H, ws, eps, dtype)


def encoder_block_bwd(t: Dict, B: int, P: int, W: int, H: int, ws: torch.Tensor, eps: float = 1e-5, dtype: torch.dtype = torch.bfloat16) -> None:
    """dZin from dZout (the block's forward recomputed from Zin) plus the wgrad operands n1, dqkv, att, dz1, n2, dh, hg, dz2, u1, u2, u3w, u3b."""
    _encoder_block("sea_encoder_block_bwd", t, B, P, W, H, ws, eps, dtype)


def fill_kv_fill(g: N.SeaKvFill, K, Vt, Kd, Vd, n_pos: int, v_rows: bool) -> None:
    """One entry of sea_kv_cache_fill: K [B, H, cap_src, hd] and Vt [B, H, hd, cap_src] (a full-context plan's buffers) -> Kd [B, H, cap_dst, hd] and
    Vd ([B, H, cap_dst, hd] with v_rows, else [B, H, hd, cap_dst]), positions 0 .. n_pos - 1."""
    B, H, cap_src, hd = K.shape
    g.K, g.Vt, g.Kd, g.Vd = K.data_ptr(), Vt.data_ptr(), Kd.data_ptr(), Vd.data_ptr()
    g.B, g.H, g.hd, g.n_pos, g.cap_src, g.cap_dst, g.v_rows = B, H, hd, n_pos, cap_src, Kd.shape[2], int(bool(v_rows))


def kv_cache_fill(entries: Sequence[Dict], dtype: torch.dtype) -> None:
    """sea_kv_cache_fill over entries dict(K, Vt, Kd, Vd, n_pos, v_rows) (fill_kv_fill's arguments): one launch per N.KV_FILL_MAX entries."""
    for d in entries:
        for name in ("K", "Vt", "Kd", "Vd"):
            t = d[name]
            N.require_gpu(t, name)
            if t.dim() != 4 or not t.is_contiguous() or t.dtype != dtype:
                raise ValueError(f"kv_cache_fill: {name} must be a contiguous 4-D {dtype} tensor, got {tuple(t.shape)} {t.dtype}")
    arr = (N.SeaKvFill * max(len(entries), 1))()
    for g, d in zip(arr, entries):
        fill_kv_fill(g, **d)
    N.check(N.lib().sea_kv_cache_fill(arr, len(entries), N.dtype_code(dtype), N.stream_ptr()), "sea_kv_cache_fill")


def fill_kv_fork(g: N.SeaKvFork, src, dst, n_pos: int, transposed: bool) -> None:
    """One entry of sea_kv_cache_fork: positions 0 .. n_pos - 1 of src ([B_src, H, cap_src, hd], or [B_src, H, hd, cap_src] when `transposed`) into
    dst of the same layout with B_src * n_rep rows: destination row b * n_rep + j receives source row b."""
    Bs, H = src.shape[0], src.shape[1]
    hd, cap_src, cap_dst = (src.shape[2], src.shape[3], dst.shape[3]) if transposed else (src.shape[3], src.shape[2], dst.shape[2])
    if dst.shape[0] % Bs or dst.shape[1] != H or (dst.shape[2] if transposed else dst.shape[3]) != hd:
        raise ValueError(f"kv_cache_fork: dst {tuple(dst.shape)} is not src {tuple(src.shape)} with a multiple of its rows")
    g.src, g.dst = src.data_ptr(), dst.data_ptr()
    g.B_src, g.H, g.hd, g.n_pos, g.cap_src, g.cap_dst, g.n_rep, g.transposed = Bs, H, hd, n_pos, cap_src, cap_dst, dst.shape[0] // Bs, int(bool(transposed))


def kv_cache_fork(entries: Sequence[Dict], dtype: torch.dtype) -> None:
    """sea_kv_cache_fork over entries dict(src, dst, n_pos, transposed) (fill_kv_fork's arguments): one launch per N.KV_FORK_MAX entries."""
    for d in entries:
        for name in ("src", "dst"):
            t = d[name]
            N.require_gpu(t, name)
            if t.dim() != 4 or not t.is_contiguous() or t.dtype != dtype:
                raise ValueError(f"kv_cache_fork: {name} must be a contiguous 4-D {dtype} tensor, got {tuple(t.shape)} {t.dtype}")
    arr = (N.SeaKvFork * max(len(entries), 1))()
    for g, d in zip(arr, entries):
        fill_kv_fork(g, **d)
    N.check(N.lib().sea_kv_cache_fork(arr, len(entries), N.dtype_code(dtype), N.stream_ptr()), "sea_kv_cache_fork")


def fill_kv_gather(g: N.SeaKvGather, src, dst, index, n_pos: int, src_transposed: bool, dst_transposed: bool) -> None:
    """One entry of sea_kv_cache_gather: positions 0 .. n_pos - 1 of row index[j] of src ([B_src, H, cap_src, hd], or [B_src, H, hd, cap_src] when
    `src_transposed`) into row j of dst ([B_dst, H, cap_dst, hd], or [B_dst, H, hd, cap_dst] when `dst_transposed`); index: int32 [B_dst] on the device."""
    Bs, H = src.shape[0], src.shape[1]
    hd, cap_src = (src.shape[2], src.shape[3]) if src_transposed else (src.shape[3], src.shape[2])
    hd_d, cap_dst = (dst.shape[2], dst.shape[3]) if dst_transposed else (dst.shape[3], dst.shape[2])
    if dst.shape[1] != H or hd_d != hd:
        raise ValueError(f"kv_cache_gather: dst {tuple(dst.shape)} (transposed={bool(dst_transposed)}) does not have the heads and head dimension of src "
                         f"{tuple(src.shape)} (transposed={bool(src_transposed)})")
    if index.dim() != 1 or index.dtype != torch.int32 or index.shape[0] != dst.shape[0]:
        raise ValueError(f"kv_cache_gather: index {tuple(index.shape)} {index.dtype} must be int32 [B_dst = {dst.shape[0]}]")
    g.src, g.dst, g.index = src.data_ptr(), dst.data_ptr(), index.data_ptr()
    g.B_src, g.B_dst, g.H, g.hd, g.n_pos, g.cap_src, g.cap_dst = Bs, dst.shape[0], H, hd, n_pos, cap_src, cap_dst
    g.src_transposed, g.dst_transposed = int(bool(src_transposed)), int(bool(dst_transposed))


def check_gather_index(index, B_src: Sequence[int], B_dst: Sequence[int], what: str = "kv_cache_gather") -> list:
    """The index of a gather as a list of ints: a 1-D, non-empty host sequence or CPU integer tensor whose values lie in [0, b) for every b of B_src and
    whose length equals every entry of B_dst.  Raises ValueError; touches no device."""
    if torch.is_tensor(index):
        if index.is_cuda or index.dim() != 1 or index.dtype in (torch.bool,) or index.is_floating_point() or index.is_complex():
            raise ValueError(f"{what}: index must be a 1-D integer tensor on the host, got {tuple(index.shape)} {index.dtype} on {index.device}")
        idx = index.tolist()
    else:
        idx = list(index)
        if any(isinstance(v, bool) or not isinstance(v, int) for v in idx):
            raise ValueError(f"{what}: index must be a 1-D sequence of integers")
    if not idx:
        raise ValueError(f"{what}: index is empty")
    for b in B_src:
        if min(idx) < 0 or max(idx) >= b:
            raise ValueError(f"{what}: index values must lie in [0, B_src = {b}), got {min(idx)} .. {max(idx)}")
    for b in B_dst:
        if b != len(idx):
            raise ValueError(f"{what}: index has {len(idx)} entries for a destination of B_dst = {b} rows")
    return idx


def kv_cache_gather(entries: Sequence[Dict], index, dtype: torch.dtype) -> None:
    """sea_kv_cache_gather over entries dict(src, dst, n_pos, src_transposed, dst_transposed): one launch per N.KV_GATHER_MAX entries.  `index` (a host
    sequence or CPU integer tensor, one value per destination row) is checked against every entry before anything touches the device, then uploaded
    once as the int32 tensor all entries share.  The only way from Python to the entry point."""
    idx = check_gather_index(index, [d["src"].shape[0] for d in entries], [d["dst"].shape[0] for d in entries])
    for d in entries:
        for name in ("src", "dst"):
            t = d[name]
            N.require_gpu(t, name)
            if t.dim() != 4 or not t.is_contiguous() or t.dtype != dtype:
                raise ValueError(f"kv_cache_gather: {name} must be a contiguous 4-D {dtype} tensor, got {tuple(t.shape)} {t.dtype}")
    if not entries:
        raise ValueError("kv_cache_gather: no entries")
    dev_index = torch.tensor(idx, dtype=torch.int32, device=entries[0]["src"].device)
    arr = (N.SeaKvGather * len(entries))()
    for g, d in zip(arr, entries):
        fill_kv_gather(g, index=dev_index, **d)
    N.check(N.lib().sea_kv_cache_gather(arr, len(entries), N.dtype_code(dtype), N.stream_ptr()), "sea_kv_cache_gather")


def fill_decode_mse(groups_arr, P: N.SeaDecodeMse, groups: Sequence[Dict], target, counts, n_patches: int, C_: int, Cp: int, inv_n: float, grad_scale: float,
                    loss, partial) -> None:
    """The argument table of sea_decode_mse.  groups: dicts H act [M, S], W2 act [n_fields * Cp, S], bias f32 [n_fields * Cp], dH act [M, S], optional
    Z act [M, S]; group g's fields follow those of the groups before it in the target.  target: f32 [M, n_fields_total, >= C] with unit inner stride."""
    field0 = 0
    for g, d in zip(groups_arr, groups):
        H, W2, Z = d["H"], d["W2"], d.get("Z")
        g.H, g.W2, g.bias, g.dH, g.Z = H.data_ptr(), W2.data_ptr(), d["bias"].data_ptr(), d["dH"].data_ptr(), N.ptr(Z)
        g.ldh, g.ldw, g.lddh, g.ldz = H.stride(0), W2.stride(0), d["dH"].stride(0), (Z.stride(0) if Z is not None else 0)
        g.n_fields, g.field0 = W2.shape[0] // Cp, field0
        field0 += g.n_fields
    P.target, P.counts, P.loss, P.partial = target.data_ptr(), N.ptr(counts), loss.data_ptr(), partial.data_ptr()
    P.ld_row, P.ld_field = target.stride(0), target.stride(1)
    P.M, P.S, P.C, P.Cp, P.P, P.n_partial_cap = groups[0]["H"].shape[0], groups[0]["H"].shape[1], C_, Cp, n_patches, partial.numel()
    P.inv_n, P.grad_scale = inv_n, grad_scale


def decode_mse(groups: Sequence[Dict], target: torch.Tensor, C_: int, Cp: int, inv_n: float, counts: Optional[torch.Tensor] = None, n_patches: int = 1,
               grad_scale: float = 1.0, dtype: torch.dtype = torch.bfloat16) -> torch.Tensor:
    """sea_decode_mse: loss = inv_n * sum of the squared valid residuals of the decoder's second layer against `target`, and d loss / d H (times GELU'(Z)
    where a group carries Z) written into each group's dH.  groups as fill_decode_mse; target f32 [M, n_fields_total, Cw >= C_] (any row and field
    strides that are multiples of 4, unit inner stride, 16-byte-aligned base); counts: device int32 [n_patches] (row m belongs to patch m % n_patches)
    or None.  Everything is checked on the host before the launch; returns the loss as an f32 tensor of one element."""
    if dtype != torch.bfloat16:
        raise ValueError(f"decode_mse: the fused launch is bf16 only, got {dtype}")
    if not groups or len(groups) > N.DECODE_MSE_MAX_GROUPS:
        raise ValueError(f"decode_mse: {len(groups)} groups; a launch carries 1 .. {N.DECODE_MSE_MAX_GROUPS}")
    if Cp < 32 or Cp % 32 or not 1 <= C_ <= Cp:
        raise ValueError(f"decode_mse: need Cp a multiple of 32 and 1 <= C <= Cp, got C = {C_}, Cp = {Cp}")
    dev = target.device
    M, S = tuple(groups[0]["H"].shape) if groups[0]["H"].dim() == 2 else (0, 0)
    if M < 1 or S < 8 or S % 8 or S > N.DECODE_MSE_MAX_S:
        raise ValueError(f"decode_mse: H must be [M >= 1, S] with S a multiple of 8 up to {N.DECODE_MSE_MAX_S}, got {tuple(groups[0]['H'].shape)}")
    n_fields = 0
    for i, d in enumerate(groups):
        for name in ("H", "W2", "dH", "Z"):
            t = d.get(name)
            if t is None and name == "Z":
                continue
            if t.dim() != 2 or t.stride(1) != 1:
                raise ValueError(f"decode_mse group {i}: {name}: need a 2-D tensor with unit inner stride, got shape {tuple(t.shape)} strides {t.stride()}")
            if t.dtype != dtype or t.device != dev or t.shape[1] != S or (name != "W2" and t.shape[0] != M):
                raise ValueError(f"decode_mse group {i}: {name} must be a {dtype} [{'n_fields * Cp' if name == 'W2' else M}, {S}] tensor on {dev}, got "
                                 f"{tuple(t.shape)} {t.dtype} on {t.device}")
            if t.stride(0) % 8 or t.data_ptr() % 16:
                raise ValueError(f"decode_mse group {i}: {name} needs a row stride that is a multiple of 8 and a 16-byte-aligned base (stride {t.stride(0)})")
        W2, b = d["W2"], d["bias"]
        if W2.shape[0] < Cp or W2.shape[0] % Cp:
            raise ValueError(f"decode_mse group {i}: W2 has {W2.shape[0]} rows, not a multiple of Cp = {Cp}")
        if b.dtype != torch.float32 or b.dim() != 1 or b.shape[0] != W2.shape[0] or not b.is_contiguous() or b.device != dev or b.data_ptr() % 16:
            raise ValueError(f"decode_mse group {i}: bias must be a contiguous, 16-byte-aligned float32 [{W2.shape[0]}] on {dev}, got {tuple(b.shape)} {b.dtype}")
        n_fields += W2.shape[0] // Cp
    if target.dtype != torch.float32 or target.dim() != 3 or target.shape[0] != M or target.shape[1] != n_fields or target.shape[2] < C_:
        raise ValueError(f"decode_mse: target must be float32 [{M}, {n_fields}, >= {C_}], got {tuple(target.shape)} {target.dtype}")
    if target.stride(2) != 1 or target.stride(0) % 4 or target.stride(1) % 4 or target.data_ptr() % 16:
        raise ValueError(f"decode_mse: target needs unit inner stride, row and field strides that are multiples of 4 and a 16-byte-aligned base, got strides "
                         f"{target.stride()} (pad the cell width to a multiple of 4: patchify_and_scale(..., c_out=))")
    if n_patches < 1:
        raise ValueError(f"decode_mse: n_patches = {n_patches} must be positive")
    if counts is not None:
        if counts.dtype != torch.int32 or counts.dim() != 1 or counts.shape[0] != n_patches or not counts.is_contiguous() or counts.device != dev:
            raise ValueError(f"decode_mse: counts must be a contiguous int32 [{n_patches}] on {dev}, got {tuple(counts.shape)} {counts.dtype} on {counts.device}")
        if M % n_patches:
            raise ValueError(f"decode_mse: {M} rows are not a multiple of {n_patches} patches")
    if not inv_n > 0.0:
        raise ValueError(f"decode_mse: inv_n = {inv_n} must be positive")
    N.require_gpu(target, "decode_mse target")   # every operand is on the target's device (checked above)
    n_partial = (M + N.DECODE_MSE_ROWS - 1) // N.DECODE_MSE_ROWS * len(groups)
    loss = torch.empty(1, device=dev, dtype=torch.float32)
    partial = torch.empty(n_partial, device=dev, dtype=torch.float32)
    arr, P = (N.SeaDecodeMseGroup * len(groups))(), N.SeaDecodeMse()
    fill_decode_mse(arr, P, groups, target, counts, n_patches, C_, Cp, float(inv_n), float(grad_scale), loss, partial)
    N.check(N.lib().sea_decode_mse(arr, len(groups), C.byref(P), N.dtype_code(dtype), N.stream_ptr()), "sea_decode_mse")
    return loss


def fill_decode_member_sse(groups_arr, P: N.SeaDecodeMemberSse, groups: Sequence[Dict], target, counts, n_patches: int, members: int, C_: int, Cp: int,
                           sse, work) -> None:
    """The argument table of sea_decode_member_sse.  groups: dicts H act [M, S], W2 act [n_fields * Cp, S], bias f32 [n_fields * Cp] (no dH, no Z); group
    g's fields follow those of the groups before it.  target: f32 [M / members, n_fields_total, >= C] with unit inner stride."""
    field0 = 0
    for g, d in zip(groups_arr, groups):
        H, W2 = d["H"], d["W2"]
        g.H, g.W2, g.bias, g.dH, g.Z = H.data_ptr(), W2.data_ptr(), d["bias"].data_ptr(), None, None
        g.ldh, g.ldw, g.lddh, g.ldz = H.stride(0), W2.stride(0), 0, 0
        g.n_fields, g.field0 = W2.shape[0] // Cp, field0
        field0 += g.n_fields
    P.target, P.counts, P.sse, P.work = target.data_ptr(), N.ptr(counts), sse.data_ptr(), work.data_ptr()
    P.ld_row, P.ld_field, P.work_cap = target.stride(0), target.stride(1), work.numel()
    P.M, P.S, P.C, P.Cp, P.P = groups[0]["H"].shape[0], groups[0]["H"].shape[1], C_, Cp, n_patches
    P.members, P.n_fields_total = members, field0


def decode_member_sse(groups: Sequence[Dict], target: torch.Tensor, C_: int, Cp: int, n_patches: int, members: int = 1, counts: Optional[torch.Tensor] = None,
                      dtype: torch.dtype = torch.bfloat16) -> torch.Tensor:
    """sea_decode_member_sse: the squared error of the decoder's second layer against `target` per member and field, f32 [M / n_patches, n_fields_total].
    groups as fill_decode_member_sse; row m is patch m % n_patches of member m // n_patches, and the `members` consecutive members of one history read
    the same target rows: target f32 [M / members, n_fields_total, Cw >= C_] (row and field strides multiples of 4, unit inner stride, 16-byte-aligned
    base); counts: device int32 [n_patches] or None.  Everything is checked on the host before the launch."""
    if dtype != torch.bfloat16:
        raise ValueError(f"decode_member_sse: the fused launch is bf16 only, got {dtype}")
    if not groups or len(groups) > N.DECODE_MSE_MAX_GROUPS:
        raise ValueError(f"decode_member_sse: {len(groups)} groups; a launch carries 1 .. {N.DECODE_MSE_MAX_GROUPS}")
    if Cp < 32 or Cp % 32 or not 1 <= C_ <= Cp:
        raise ValueError(f"decode_member_sse: need Cp a multiple of 32 and 1 <= C <= Cp, got C = {C_}, Cp = {Cp}")
    dev = target.device
    M, S = tuple(groups[0]["H"].shape) if groups[0]["H"].dim() == 2 else (0, 0)
    if M < 1 or S < 8 or S % 8 or S > N.DECODE_MSE_MAX_S:
        raise ValueError(f"decode_member_sse: H must be [M >= 1, S] with S a multiple of 8 up to {N.DECODE_MSE_MAX_S}, got {tuple(groups[0]['H'].shape)}")
    if n_patches < 1 or members < 1:
        raise ValueError(f"decode_member_sse: n_patches = {n_patches} and members = {members} must be positive")
    if M % (n_patches * members):
        raise ValueError(f"decode_member_sse: {M} rows are not a multiple of n_patches * members = {n_patches} * {members}")
    n_fields = 0
    for i, d in enumerate(groups):
        for name in ("H", "W2"):
            t = d[name]
            if t.dim() != 2 or t.stride(1) != 1:
                raise ValueError(f"decode_member_sse group {i}: {name}: need a 2-D tensor with unit inner stride, got shape {tuple(t.shape)} strides {t.stride()}")
            if t.dtype != dtype or t.device != dev or t.shape[1] != S or (name != "W2" and t.shape[0] != M):
                raise ValueError(f"decode_member_sse group {i}: {name} must be a {dtype} [{'n_fields * Cp' if name == 'W2' else M}, {S}] tensor on {dev}, got "
                                 f"{tuple(t.shape)} {t.dtype} on {t.device}")
            if t.stride(0) % 8 or t.data_ptr() % 16:
                raise ValueError(f"decode_member_sse group {i}: {name} needs a row stride that is a multiple of 8 and a 16-byte-aligned base (stride {t.stride(0)})")
        W2, b = d["W2"], d["bias"]
        if W2.shape[0] < Cp or W2.shape[0] % Cp:
            raise ValueError(f"decode_member_sse group {i}: W2 has {W2.shape[0]} rows, not a multiple of Cp = {Cp}")
        if b.dtype != torch.float32 or b.dim() != 1 or b.shape[0] != W2.shape[0] or not b.is_contiguous() or b.device != dev or b.data_ptr() % 16:
            raise ValueError(f"decode_member_sse group {i}: bias must be a contiguous, 16-byte-aligned float32 [{W2.shape[0]}] on {dev}, got {tuple(b.shape)} {b.dtype}")
        n_fields += W2.shape[0] // Cp
    rows = M // members
    if target.dtype != torch.float32 or target.dim() != 3 or target.shape[0] != rows or target.shape[1] != n_fields or target.shape[2] < C_:
        raise ValueError(f"decode_member_sse: target must be float32 [{rows}, {n_fields}, >= {C_}], got {tuple(target.shape)} {target.dtype}")
    if target.stride(2) != 1 or target.stride(0) % 4 or target.stride(1) % 4 or target.data_ptr() % 16:
        raise ValueError(f"decode_member_sse: target needs unit inner stride, row and field strides that are multiples of 4 and a 16-byte-aligned base, got "
                         f"strides {target.stride()} (pad the cell width to a multiple of 4: patchify_and_scale(..., c_out=))")
    if counts is not None and (counts.dtype != torch.int32 or counts.dim() != 1 or counts.shape[0] != n_patches or not counts.is_contiguous() or counts.device != dev):
        raise ValueError(f"decode_member_sse: counts must be a contiguous int32 [{n_patches}] on {dev}, got {tuple(counts.shape)} {counts.dtype} on {counts.device}")
    N.require_gpu(target, "decode_member_sse target")   # every operand is on the target's device (checked above)
    sse = torch.empty(M // n_patches, n_fields, device=dev, dtype=torch.float32)
    work = torch.empty(M * n_fields, device=dev, dtype=torch.float32)
    arr, P = (N.SeaDecodeMseGroup * len(groups))(), N.SeaDecodeMemberSse()
    fill_decode_member_sse(arr, P, groups, target, counts, n_patches, members, C_, Cp, sse, work)
    N.check(N.lib().sea_decode_member_sse(arr, len(groups), C.byref(P), N.dtype_code(dtype), N.stream_ptr()), "sea_decode_member_sse")
    return sse


def fill_decode_sensor_sse(groups_arr, P: N.SeaDecodeSensorSse, groups: Sequence[Dict], obs, prec, live, wrow, seg, members: int, Cp: int, wsse, pred, work) -> None:
    """The argument table of sea_decode_sensor_sse.  groups: dicts H act [Q * Bm, S] (patch-major: row q * Bm + bm), W2 act [n_fields * Cp, S], bias f32
    [n_fields * Cp] (no dH, no Z).  obs f32 [B, K_pad]; prec None, f32 [K_pad] or [B, K_pad]; live, wrow int32 [K_pad]; seg int32 [n_groups, Q + 1]."""
    field0 = 0
    for g, d in zip(groups_arr, groups):
        H, W2 = d["H"], d["W2"]
        g.H, g.W2, g.bias, g.dH, g.Z = H.data_ptr(), W2.data_ptr(), d["bias"].data_ptr(), None, None
        g.ldh, g.ldw, g.lddh, g.ldz = H.stride(0), W2.stride(0), 0, 0
        g.n_fields, g.field0 = W2.shape[0] // Cp, field0
        field0 += g.n_fields
    P.obs, P.prec, P.live, P.wrow, P.seg = obs.data_ptr(), N.ptr(prec), live.data_ptr(), wrow.data_ptr(), seg.data_ptr()
    P.wsse, P.pred, P.work = wsse.data_ptr(), N.ptr(pred), work.data_ptr()
    P.ld_obs, P.ld_prec, P.work_cap = obs.stride(0), (prec.stride(0) if prec is not None and prec.dim() == 2 else 0), work.numel()
    P.Bm, P.members, P.S, P.Cp, P.Q, P.K_pad = wsse.shape[0], members, groups[0]["H"].shape[1], Cp, seg.shape[1] - 1, live.shape[0]


def decode_sensor_sse(groups: Sequence[Dict], obs: torch.Tensor, live: torch.Tensor, wrow: torch.Tensor, seg: torch.Tensor, Cp: int, members: int = 1,
                      prec: Optional[torch.Tensor] = None, predictions: bool = False, dtype: torch.dtype = torch.bfloat16):
    """sea_decode_sensor_sse: the precision-weighted squared error of every member against sparse observations, f32 [Bm] (and, with predictions=True, the
    decoded values f32 [Bm, K_pad] in sorted, padded order).  groups as fill_decode_sensor_sse; the tables live, wrow int32 [K_pad] and seg int32
    [n_groups, Q + 1] are a SensorSet's (built and range-checked on the host: the kernel trusts their contents); obs f32 [B, K_pad] and prec (None, f32
    [K_pad] or [B, K_pad]) in the same sorted, padded order; Bm = B * members = H rows / Q.  Everything else is checked on the host before the launch."""
    return _sensor_sse_call("decode_sensor_sse", groups, obs, live, wrow, seg, Cp, members, prec, predictions, dtype, None)


def _sensor_sse_call(what: str, groups, obs, live, wrow, seg, Cp: int, members: int, prec, predictions: bool, dtype, _derived):
    """The operand checks and the launch decode_sensor_sse and decode_derived_sensor_sse share, under the caller's name `what`; _derived: None, or the
    pair tables (op, scale, shift) of decode_derived_sensor_sse."""
    if dtype != torch.bfloat16:
        raise ValueError(f"{what}: the fused launch is bf16 only, got {dtype}")
    if not groups or len(groups) > N.DECODE_MSE_MAX_GROUPS:
        raise ValueError(f"{what}: {len(groups)} groups; a launch carries 1 .. {N.DECODE_MSE_MAX_GROUPS}")
    if Cp < 32 or Cp % 32:
        raise ValueError(f"{what}: need Cp a multiple of 32, got Cp = {Cp}")
    dev = obs.device
    if seg.dim() != 2 or seg.shape[0] != len(groups) or seg.shape[1] < 2 or seg.dtype != torch.int32 or not seg.is_contiguous() or seg.device != dev:
        raise ValueError(f"{what}: seg must be a contiguous int32 [{len(groups)}, Q + 1 >= 2] on {dev}, got {tuple(seg.shape)} {seg.dtype} on {seg.device}")
    Q = seg.shape[1] - 1
    if Q > N.SENSOR_MAX_PATCHES:
        raise ValueError(f"{what}: {Q} observed patches; a launch carries 1 .. {N.SENSOR_MAX_PATCHES}")
    for name, t in (("live", live), ("wrow", wrow)):
        if t.dim() != 1 or t.dtype != torch.int32 or not t.is_contiguous() or t.device != dev or t.shape[0] != live.shape[0]:
            raise ValueError(f"{what}: {name} must be a contiguous int32 [K_pad] on {dev}, got {tuple(t.shape)} {t.dtype} on {t.device}")
    K_pad = live.shape[0]
    if K_pad < N.SENSOR_TILE or K_pad % N.SENSOR_TILE:
        raise ValueError(f"{what}: K_pad = {K_pad} must be a positive multiple of {N.SENSOR_TILE}")
    R, S = tuple(groups[0]["H"].shape) if groups[0]["H"].dim() == 2 else (0, 0)
    if R < 1 or R % Q or S < 8 or S % 8 or S > N.DECODE_MSE_MAX_S:
        raise ValueError(f"{what}: H must be [Q * Bm, S] with Q = {Q} and S a multiple of 8 up to {N.DECODE_MSE_MAX_S}, got {tuple(groups[0]['H'].shape)}")
    Bm = R // Q
    if not isinstance(members, int) or members < 1 or Bm % members:
        raise ValueError(f"{what}: members = {members!r} must be a positive integer that divides Bm = {Bm}")
    B = Bm // members
    for i, d in enumerate(groups):
        for name in ("H", "W2"):
            t = d[name]
            if t.dim() != 2 or t.stride(1) != 1:
                raise ValueError(f"{what} group {i}: {name}: need a 2-D tensor with unit inner stride, got shape {tuple(t.shape)} strides {t.stride()}")
            if t.dtype != dtype or t.device != dev or t.shape[1] != S or (name != "W2" and t.shape[0] != R):
                raise ValueError(f"{what} group {i}: {name} must be a {dtype} [{'n_fields * Cp' if name == 'W2' else R}, {S}] tensor on {dev}, got "
                                 f"{tuple(t.shape)} {t.dtype} on {t.device}")
            if t.stride(0) % 8 or t.data_ptr() % 16:
                raise ValueError(f"{what} group {i}: {name} needs a row stride that is a multiple of 8 and a 16-byte-aligned base (stride {t.stride(0)})")
        W2, b = d["W2"], d["bias"]
        if W2.shape[0] < Cp or W2.shape[0] % Cp:
            raise ValueError(f"{what} group {i}: W2 has {W2.shape[0]} rows, not a multiple of Cp = {Cp}")
        if b.dtype != torch.float32 or b.dim() != 1 or b.shape[0] != W2.shape[0] or not b.is_contiguous() or b.device != dev or b.data_ptr() % 16:
            raise ValueError(f"{what} group {i}: bias must be a contiguous, 16-byte-aligned float32 [{W2.shape[0]}] on {dev}, got {tuple(b.shape)} {b.dtype}")
    if obs.dtype != torch.float32 or obs.dim() != 2 or tuple(obs.shape) != (B, K_pad) or obs.stride(1) != 1 or obs.stride(0) % 4 or obs.stride(0) < K_pad \
            or obs.data_ptr() % 16:
        raise ValueError(f"{what}: obs must be a 16-byte-aligned float32 [{B}, {K_pad}] with unit inner stride and a row stride that is a multiple of 4, "
                         f"got {tuple(obs.shape)} {obs.dtype} strides {obs.stride()}")
    if prec is not None:
        if prec.dtype != torch.float32 or prec.device != dev or tuple(prec.shape) not in ((K_pad,), (B, K_pad)) or prec.stride(-1) != 1 or prec.data_ptr() % 16 \
                or (prec.dim() == 2 and (prec.stride(0) % 4 or prec.stride(0) < K_pad)):
            raise ValueError(f"{what}: prec must be None or a 16-byte-aligned float32 [{K_pad}] or [{B}, {K_pad}] on {dev} with unit inner stride, got "
                             f"{tuple(prec.shape)} {prec.dtype} strides {prec.stride()} on {prec.device}")
    if _derived is not None:
        _derived = _check_derived_sensor_tables(what, _derived, K_pad, dev)
    N.require_gpu(obs, f"{what} obs")   # every operand is on the observation's device (checked above)
    wsse = torch.empty(Bm, device=dev, dtype=torch.float32)
    pred = torch.empty(Bm, K_pad, device=dev, dtype=torch.float32) if predictions else None
    work = torch.empty(Q * len(groups) * Bm, device=dev, dtype=torch.float32)
    arr, P = (N.SeaDecodeMseGroup * len(groups))(), N.SeaDecodeSensorSse()
    fill_decode_sensor_sse(arr, P, groups, obs, prec, live, wrow, seg, members, Cp, wsse, pred, work)
    if _derived is not None:
        T = N.SeaDerivedSensorTables()
        fill_derived_sensor_tables(T, *_derived)
        N.check(N.lib().sea_decode_derived_sensor_sse(arr, len(groups), C.byref(P), C.byref(T), N.dtype_code(dtype), N.stream_ptr()), "sea_decode_derived_sensor_sse")
        return (wsse, pred) if predictions else wsse
    N.check(N.lib().sea_decode_sensor_sse(arr, len(groups), C.byref(P), N.dtype_code(dtype), N.stream_ptr()), "sea_decode_sensor_sse")
    return (wsse, pred) if predictions else wsse


def fill_decode_sensor_grad(groups_arr, P: N.SeaDecodeSensorGrad, groups: Sequence[Dict], obs, prec, live, wrow, seg, members: int, Cp: int, wsse, pred, work,
                            grad_scale: float) -> None:
    """The argument table of sea_decode_sensor_grad.  groups: dicts H act [Q * Bm, S] (patch-major: row q * Bm + bm), W2 act [n_fields * Cp, S], bias f32
    [n_fields * Cp], dH act [Q * Bm, S] (output) and Z act [Q * Bm, S] or None (absent).  The rest as fill_decode_sensor_sse."""
    field0 = 0
    for g, d in zip(groups_arr, groups):
        H, W2, dH, Z = d["H"], d["W2"], d["dH"], d.get("Z")
        g.H, g.W2, g.bias, g.dH, g.Z = H.data_ptr(), W2.data_ptr(), d["bias"].data_ptr(), dH.data_ptr(), N.ptr(Z)
        g.ldh, g.ldw, g.lddh, g.ldz = H.stride(0), W2.stride(0), dH.stride(0), (Z.stride(0) if Z is not None else 0)
        g.n_fields, g.field0 = W2.shape[0] // Cp, field0
        field0 += g.n_fields
    P.obs, P.prec, P.live, P.wrow, P.seg = obs.data_ptr(), N.ptr(prec), live.data_ptr(), wrow.data_ptr(), seg.data_ptr()
    P.wsse, P.pred, P.work = wsse.data_ptr(), N.ptr(pred), work.data_ptr()
    P.ld_obs, P.ld_prec, P.work_cap = obs.stride(0), (prec.stride(0) if prec is not None and prec.dim() == 2 else 0), work.numel()
    P.Bm, P.members, P.S, P.Cp, P.Q, P.K_pad = wsse.shape[0], members, groups[0]["H"].shape[1], Cp, seg.shape[1] - 1, live.shape[0]
    P.grad_scale = grad_scale


def decode_sensor_grad(groups: Sequence[Dict], obs: torch.Tensor, live: torch.Tensor, wrow: torch.Tensor, seg: torch.Tensor, Cp: int, members: int = 1,
                       prec: Optional[torch.Tensor] = None, predictions: bool = False, grad_scale: float = 1.0, dtype: torch.dtype = torch.bfloat16):
    """sea_decode_sensor_grad: decode_sensor_sse's score (the same bits) and, in the same launch, its gradient to the hidden rows: every group's dH act
    [Q * Bm, S] is written IN PLACE with 2 grad_scale * (w d rounded to bf16) W2 [* gelu'(Z) where the group carries a Z], zeros at the rows of a
    (group, patch) pair without sensors.  Returns (wsse f32 [Bm], pred f32 [Bm, K_pad] or None).  groups as fill_decode_sensor_grad; the tables and obs /
    prec as decode_sensor_sse.  Everything is checked on the host before the launch."""
    return _sensor_grad_call("decode_sensor_grad", groups, obs, live, wrow, seg, Cp, members, prec, predictions, grad_scale, dtype, None)


def _sensor_grad_call(what: str, groups, obs, live, wrow, seg, Cp: int, members: int, prec, predictions: bool, grad_scale, dtype, _derived):
    """The operand checks and the launch decode_sensor_grad and decode_derived_sensor_grad share, under the caller's name `what`; _derived as in
    _sensor_sse_call."""
    if dtype != torch.bfloat16:
        raise ValueError(f"{what}: the fused launch is bf16 only, got {dtype}")
    if not groups or len(groups) > N.DECODE_MSE_MAX_GROUPS:
        raise ValueError(f"{what}: {len(groups)} groups; a launch carries 1 .. {N.DECODE_MSE_MAX_GROUPS}")
    if Cp < 32 or Cp % 32:
        raise ValueError(f"{what}: need Cp a multiple of 32, got Cp = {Cp}")
    if isinstance(grad_scale, bool) or not isinstance(grad_scale, (int, float)) or not math.isfinite(grad_scale):
        raise ValueError(f"{what}: grad_scale = {grad_scale!r} must be a finite number")
    dev = obs.device
    if seg.dim() != 2 or seg.shape[0] != len(groups) or seg.shape[1] < 2 or seg.dtype != torch.int32 or not seg.is_contiguous() or seg.device != dev:
        raise ValueError(f"{what}: seg must be a contiguous int32 [{len(groups)}, Q + 1 >= 2] on {dev}, got {tuple(seg.shape)} {seg.dtype} on {seg.device}")
    Q = seg.shape[1] - 1
    if Q > N.SENSOR_MAX_PATCHES:
        raise ValueError(f"{what}: {Q} observed patches; a launch carries 1 .. {N.SENSOR_MAX_PATCHES}")
    for name, t in (("live", live), ("wrow", wrow)):
        if t.dim() != 1 or t.dtype != torch.int32 or not t.is_contiguous() or t.device != dev or t.shape[0] != live.shape[0]:
            raise ValueError(f"{what}: {name} must be a contiguous int32 [K_pad] on {dev}, got {tuple(t.shape)} {t.dtype} on {t.device}")
    K_pad = live.shape[0]
    if K_pad < N.SENSOR_TILE or K_pad % N.SENSOR_TILE:
        raise ValueError(f"{what}: K_pad = {K_pad} must be a positive multiple of {N.SENSOR_TILE}")
    R, S = tuple(groups[0]["H"].shape) if groups[0]["H"].dim() == 2 else (0, 0)
    if R < 1 or R % Q or S < 8 or S % 8 or S > N.DECODE_MSE_MAX_S:
        raise ValueError(f"{what}: H must be [Q * Bm, S] with Q = {Q} and S a multiple of 8 up to {N.DECODE_MSE_MAX_S}, got {tuple(groups[0]['H'].shape)}")
    Bm = R // Q
    if not isinstance(members, int) or members < 1 or Bm % members:
        raise ValueError(f"{what}: members = {members!r} must be a positive integer that divides Bm = {Bm}")
    B = Bm // members
    for i, d in enumerate(groups):
        for name in ("H", "W2", "dH", "Z"):
            t = d.get(name)
            if t is None and name == "Z":
                continue
            if t is None or t.dim() != 2 or t.stride(1) != 1:
                raise ValueError(f"{what} group {i}: {name}: need a 2-D tensor with unit inner stride, got "
                                 f"{'None' if t is None else f'shape {tuple(t.shape)} strides {t.stride()}'}")
            if t.dtype != dtype or t.device != dev or t.shape[1] != S or (name != "W2" and t.shape[0] != R):
                raise ValueError(f"{what} group {i}: {name} must be a {dtype} [{'n_fields * Cp' if name == 'W2' else R}, {S}] tensor on {dev}, got "
                                 f"{tuple(t.shape)} {t.dtype} on {t.device}")
            if t.stride(0) % 8 or t.stride(0) < S or t.data_ptr() % 16:
                raise ValueError(f"{what} group {i}: {name} needs a row stride that is a multiple of 8 and covers S = {S}, and a 16-byte-aligned base (stride {t.stride(0)})")
        W2, b = d["W2"], d["bias"]
        if W2.shape[0] < Cp or W2.shape[0] % Cp:
            raise ValueError(f"{what} group {i}: W2 has {W2.shape[0]} rows, not a multiple of Cp = {Cp}")
        if b.dtype != torch.float32 or b.dim() != 1 or b.shape[0] != W2.shape[0] or not b.is_contiguous() or b.device != dev or b.data_ptr() % 16:
            raise ValueError(f"{what} group {i}: bias must be a contiguous, 16-byte-aligned float32 [{W2.shape[0]}] on {dev}, got {tuple(b.shape)} {b.dtype}")
    if obs.dtype != torch.float32 or obs.dim() != 2 or tuple(obs.shape) != (B, K_pad) or obs.stride(1) != 1 or obs.stride(0) % 4 or obs.stride(0) < K_pad \
            or obs.data_ptr() % 16:
        raise ValueError(f"{what}: obs must be a 16-byte-aligned float32 [{B}, {K_pad}] with unit inner stride and a row stride that is a multiple of 4, "
                         f"got {tuple(obs.shape)} {obs.dtype} strides {obs.stride()}")
    if prec is not None:
        if prec.dtype != torch.float32 or prec.device != dev or tuple(prec.shape) not in ((K_pad,), (B, K_pad)) or prec.stride(-1) != 1 or prec.data_ptr() % 16 \
                or (prec.dim() == 2 and (prec.stride(0) % 4 or prec.stride(0) < K_pad)):
            raise ValueError(f"{what}: prec must be None or a 16-byte-aligned float32 [{K_pad}] or [{B}, {K_pad}] on {dev} with unit inner stride, got "
                             f"{tuple(prec.shape)} {prec.dtype} strides {prec.stride()} on {prec.device}")
    if _derived is not None:
        _derived = _check_derived_sensor_tables(what, _derived, K_pad, dev)
    N.require_gpu(obs, f"{what} obs")   # every operand is on the observation's device (checked above)
    wsse = torch.empty(Bm, device=dev, dtype=torch.float32)
    pred = torch.empty(Bm, K_pad, device=dev, dtype=torch.float32) if predictions else None
    work = torch.empty(Q * len(groups) * Bm, device=dev, dtype=torch.float32)
    arr, P = (N.SeaDecodeMseGroup * len(groups))(), N.SeaDecodeSensorGrad()
    fill_decode_sensor_grad(arr, P, groups, obs, prec, live, wrow, seg, members, Cp, wsse, pred, work, float(grad_scale))
    if _derived is not None:
        T = N.SeaDerivedSensorTables()
        fill_derived_sensor_tables(T, *_derived)
        N.check(N.lib().sea_decode_derived_sensor_grad(arr, len(groups), C.byref(P), C.byref(T), N.dtype_code(dtype), N.stream_ptr()), "sea_decode_derived_sensor_grad")
        return wsse, pred
    N.check(N.lib().sea_decode_sensor_grad(arr, len(groups), C.byref(P), N.dtype_code(dtype), N.stream_ptr()), "sea_decode_sensor_grad")
    return wsse, pred


def fill_derived_sensor_tables(T: N.SeaDerivedSensorTables, op, scale, shift) -> None:
    """The pair tables of sea_decode_derived_sensor_sse / _grad: op int32, scale and shift f32, each [K_pad] on the device."""
    T.op, T.scale, T.shift = op.data_ptr(), scale.data_ptr(), shift.data_ptr()


def _check_derived_sensor_tables(what: str, tables, K_pad: int, dev):
    """(op, scale, shift) of a DerivedSensorSet: contiguous, 16-byte-aligned [K_pad] tensors on `dev` (their contents were range-checked by the set)."""
    if not isinstance(tables, (tuple, list)) or len(tables) != 3 or any(not torch.is_tensor(t) for t in tables):
        raise ValueError(f"{what}: the pair tables must be three tensors (op, scale, shift)")
    for name, t, dt in zip(("op", "scale", "shift"), tables, (torch.int32, torch.float32, torch.float32)):
        if t.dim() != 1 or t.shape[0] != K_pad or t.dtype != dt or not t.is_contiguous() or t.device != dev or t.data_ptr() % 16:
            raise ValueError(f"{what}: {name} must be a contiguous, 16-byte-aligned {dt} [{K_pad}] on {dev}, got {tuple(t.shape)} {t.dtype} on {t.device}")
    return tuple(tables)


def decode_derived_sensor_sse(groups: Sequence[Dict], obs: torch.Tensor, live: torch.Tensor, wrow: torch.Tensor, seg: torch.Tensor, op: torch.Tensor,
                              scale: torch.Tensor, shift: torch.Tensor, Cp: int, members: int = 1, prec: Optional[torch.Tensor] = None, predictions: bool = False,
                              dtype: torch.dtype = torch.bfloat16):
    """sea_decode_derived_sensor_sse: decode_sensor_sse for a DerivedSensorSet — a reading is the pair of sorted entries (2 i, 2 i + 1) = (source a, source
    b); op int32, scale, shift f32 [K_pad] are the set's pair tables (op == -1 at entry 2 i: a plain reading).  obs and prec are read at the even
    entries; pred [Bm, K_pad] holds the reading's value at both entries.  Operand checks: those of decode_sensor_sse, plus the three tables."""
    return _sensor_sse_call("decode_derived_sensor_sse", groups, obs, live, wrow, seg, Cp, members, prec, predictions, dtype, (op, scale, shift))


def decode_derived_sensor_grad(groups: Sequence[Dict], obs: torch.Tensor, live: torch.Tensor, wrow: torch.Tensor, seg: torch.Tensor, op: torch.Tensor,
                               scale: torch.Tensor, shift: torch.Tensor, Cp: int, members: int = 1, prec: Optional[torch.Tensor] = None, predictions: bool = False,
                               grad_scale: float = 1.0, dtype: torch.dtype = torch.bfloat16):
    """sea_decode_derived_sensor_grad: decode_derived_sensor_sse's score (the same bits) and the gradient to the hidden rows, every group's dH written in
    place as decode_sensor_grad does.  Returns (wsse, pred or None)."""
    return _sensor_grad_call("decode_derived_sensor_grad", groups, obs, live, wrow, seg, Cp, members, prec, predictions, grad_scale, dtype, (op, scale, shift))



def fill_decode_field_grad(groups_arr, P: N.SeaDecodeFieldGrad, groups: Sequence[Dict], obs, prec, field_prec, counts, n_patches: int, members: int, C_: int, Cp: int,
                           wsse, work, grad_scale: float) -> None:
    """The argument table of sea_decode_field_grad.  groups: dicts H act [M, S], W2 act [n_fields * Cp, S], bias f32 [n_fields * Cp], and either in EVERY
    group or in none dH act [M, S] (output) with an optional Z act [M, S]; group g's fields follow those of the groups before it.  obs: f32
    [M / members, n_fields_total, >= C] with unit inner stride; prec: None or an f32 map with obs's strides."""
    field0 = 0
    for g, d in zip(groups_arr, groups):
        H, W2, dH, Z = d["H"], d["W2"], d.get("dH"), d.get("Z")
        g.H, g.W2, g.bias, g.dH, g.Z = H.data_ptr(), W2.data_ptr(), d["bias"].data_ptr(), N.ptr(dH), N.ptr(Z)
        g.ldh, g.ldw, g.lddh, g.ldz = H.stride(0), W2.stride(0), (dH.stride(0) if dH is not None else 0), (Z.stride(0) if Z is not None else 0)
        g.n_fields, g.field0 = W2.shape[0] // Cp, field0
        field0 += g.n_fields
    P.obs, P.prec, P.field_prec, P.counts, P.wsse, P.work = obs.data_ptr(), N.ptr(prec), N.ptr(field_prec), N.ptr(counts), wsse.data_ptr(), work.data_ptr()
    P.ld_row, P.ld_field, P.work_cap = obs.stride(0), obs.stride(1), work.numel()
    P.M, P.S, P.C, P.Cp, P.P = groups[0]["H"].shape[0], groups[0]["H"].shape[1], C_, Cp, n_patches
    P.members, P.n_fields_total, P.grad_scale = members, field0, grad_scale


def decode_field_grad(groups: Sequence[Dict], obs: torch.Tensor, C_: int, Cp: int, n_patches: int, members: int = 1, prec: Optional[torch.Tensor] = None,
                      field_prec: Optional[torch.Tensor] = None, counts: Optional[torch.Tensor] = None, grad_scale: float = 1.0,
                      work: Optional[torch.Tensor] = None, dtype: torch.dtype = torch.bfloat16) -> torch.Tensor:
    """sea_decode_field_grad: the weighted squared error of the decoder's second layer against a dense observation per member and field, f32
    [M / n_patches, n_fields_total], with the weight w = field_prec * prec applied by selects (a cell without positive weight is neutral whatever obs
    and prec hold there) — and, when the groups carry dH, its gradient to the hidden rows in the same launch: every group's dH act [M, S] is written IN
    PLACE with 2 grad_scale * (w d rounded to bf16) W2 [* gelu'(Z) where the group carries a Z].  Without a dH in any group the launch is score-only and
    returns the same bits; dH in some groups only is refused.  groups as fill_decode_field_grad; rows and obs as decode_member_sse; prec: None or a
    float32 map of obs's shape AND strides; field_prec: None or a contiguous float32 [n_fields_total]; counts: device int32 [n_patches] or None; work:
    None (allocated here) or a contiguous float32 workspace of at least M * n_fields_total elements.  Everything is checked on the host before the launch."""
    what = "decode_field_grad"
    if dtype != torch.bfloat16:
        raise ValueError(f"{what}: the fused launch is bf16 only, got {dtype}")
    if not groups or len(groups) > N.DECODE_MSE_MAX_GROUPS:
        raise ValueError(f"{what}: {len(groups)} groups; a launch carries 1 .. {N.DECODE_MSE_MAX_GROUPS}")
    if Cp < 32 or Cp % 32 or not 1 <= C_ <= Cp:
        raise ValueError(f"{what}: need Cp a multiple of 32 and 1 <= C <= Cp, got C = {C_}, Cp = {Cp}")
    if isinstance(grad_scale, bool) or not isinstance(grad_scale, (int, float)) or not math.isfinite(grad_scale):
        raise ValueError(f"{what}: grad_scale = {grad_scale!r} must be a finite number")
    if not torch.is_tensor(obs):
        raise ValueError(f"{what}: obs must be a tensor, got {type(obs).__name__}")
    dev = obs.device
    H0 = groups[0].get("H")
    M, S = tuple(H0.shape) if torch.is_tensor(H0) and H0.dim() == 2 else (0, 0)
    if M < 1 or S < 8 or S % 8 or S > N.DECODE_MSE_MAX_S:
        raise ValueError(f"{what}: H must be [M >= 1, S] with S a multiple of 8 up to {N.DECODE_MSE_MAX_S}, got {tuple(H0.shape) if torch.is_tensor(H0) else H0!r}")
    if not isinstance(n_patches, int) or not isinstance(members, int) or n_patches < 1 or members < 1:
        raise ValueError(f"{what}: n_patches = {n_patches!r} and members = {members!r} must be positive integers")
    if M % (n_patches * members):
        raise ValueError(f"{what}: {M} rows are not a multiple of n_patches * members = {n_patches} * {members}")
    with_dh = sum(d.get("dH") is not None for d in groups)
    if with_dh not in (0, len(groups)):
        raise ValueError(f"{what}: {with_dh} of the {len(groups)} groups carry a dH: all of them, or none for the score alone")
    n_fields = 0
    for i, d in enumerate(groups):
        for name in ("H", "W2", "dH", "Z"):
            t = d.get(name)
            if t is None and (name == "Z" or (name == "dH" and with_dh == 0)):
                continue
            if name == "Z" and with_dh == 0:
                raise ValueError(f"{what} group {i}: a Z without a dH (the score alone reads no pre-activation)")
            if t is None or t.dim() != 2 or t.stride(1) != 1:
                raise ValueError(f"{what} group {i}: {name}: need a 2-D tensor with unit inner stride, got "
                                 f"{'None' if t is None else f'shape {tuple(t.shape)} strides {t.stride()}'}")
            if t.dtype != dtype or t.device != dev or t.shape[1] != S or (name != "W2" and t.shape[0] != M):
                raise ValueError(f"{what} group {i}: {name} must be a {dtype} [{'n_fields * Cp' if name == 'W2' else M}, {S}] tensor on {dev}, got "
                                 f"{tuple(t.shape)} {t.dtype} on {t.device}")
            if t.stride(0) % 8 or t.stride(0) < S or t.data_ptr() % 16:
                raise ValueError(f"{what} group {i}: {name} needs a row stride that is a multiple of 8 and covers S = {S}, and a 16-byte-aligned base (stride {t.stride(0)})")
        W2, b = d["W2"], d["bias"]
        if W2.shape[0] < Cp or W2.shape[0] % Cp:
            raise ValueError(f"{what} group {i}: W2 has {W2.shape[0]} rows, not a multiple of Cp = {Cp}")
        if b.dtype != torch.float32 or b.dim() != 1 or b.shape[0] != W2.shape[0] or not b.is_contiguous() or b.device != dev or b.data_ptr() % 16:
            raise ValueError(f"{what} group {i}: bias must be a contiguous, 16-byte-aligned float32 [{W2.shape[0]}] on {dev}, got {tuple(b.shape)} {b.dtype}")
        n_fields += W2.shape[0] // Cp
    rows = M // members
    if obs.dtype != torch.float32 or obs.dim() != 3 or obs.shape[0] != rows or obs.shape[1] != n_fields or obs.shape[2] < C_:
        raise ValueError(f"{what}: obs must be float32 [{rows}, {n_fields}, >= {C_}], got {tuple(obs.shape)} {obs.dtype}")
    if obs.stride(2) != 1 or obs.stride(0) % 4 or obs.stride(1) % 4 or obs.stride(0) < 0 or obs.stride(1) < 0 or obs.data_ptr() % 16:
        raise ValueError(f"{what}: obs needs unit inner stride, row and field strides that are multiples of 4 and a 16-byte-aligned base, got strides "
                         f"{obs.stride()} (pad the cell width to a multiple of 4: patchify_and_scale(..., c_out=))")
    if prec is not None:
        if not torch.is_tensor(prec) or prec.dtype != torch.float32 or prec.device != dev or tuple(prec.shape) != tuple(obs.shape):
            raise ValueError(f"{what}: prec must be None or a float32 map of obs's shape {tuple(obs.shape)} on {dev}, got "
                             f"{(tuple(prec.shape), prec.dtype, prec.device) if torch.is_tensor(prec) else type(prec).__name__}")
        if prec.stride() != obs.stride() or prec.data_ptr() % 16:
            raise ValueError(f"{what}: prec needs obs's strides {obs.stride()} and a 16-byte-aligned base, got strides {prec.stride()}")
    if field_prec is not None and (not torch.is_tensor(field_prec) or field_prec.dtype != torch.float32 or tuple(field_prec.shape) != (n_fields,)
                                   or not field_prec.is_contiguous() or field_prec.device != dev):
        raise ValueError(f"{what}: field_prec must be None or a contiguous float32 [{n_fields}] on {dev}")
    if counts is not None and (counts.dtype != torch.int32 or counts.dim() != 1 or counts.shape[0] != n_patches or not counts.is_contiguous() or counts.device != dev):
        raise ValueError(f"{what}: counts must be a contiguous int32 [{n_patches}] on {dev}, got {tuple(counts.shape)} {counts.dtype} on {counts.device}")
    if work is not None and (not torch.is_tensor(work) or work.dtype != torch.float32 or work.device != dev or not work.is_contiguous() or work.numel() < M * n_fields):
        raise ValueError(f"{what}: work must be None or a contiguous float32 workspace of at least M * n_fields_total = {M * n_fields} elements on {dev}, got "
                         f"{(work.numel(), work.dtype, work.device) if torch.is_tensor(work) else type(work).__name__}")
    N.require_gpu(obs, f"{what} obs")   # every operand is on the observation's device (checked above)
    wsse = torch.empty(M // n_patches, n_fields, device=dev, dtype=torch.float32)
    if work is None:
        work = torch.empty(M * n_fields, device=dev, dtype=torch.float32)
    arr, P = (N.SeaDecodeMseGroup * len(groups))(), N.SeaDecodeFieldGrad()
    fill_decode_field_grad(arr, P, groups, obs, prec, field_prec, counts, n_patches, members, C_, Cp, wsse, work, float(grad_scale))
    N.check(N.lib().sea_decode_field_grad(arr, len(groups), C.byref(P), N.dtype_code(dtype), N.stream_ptr()), "sea_decode_field_grad")
    return wsse


def fill_decode_member_moments(groups_arr, P: N.SeaDecodeMemberMoments, groups: Sequence[Dict], weights, var_scale, counts, n_patches: int, members: int, C_: int,
                               Cp: int, mean, var, work) -> None:
    """The argument table of sea_decode_member_moments.  groups: dicts H act [M, S], W2 act [n_fields * Cp, S], bias f32 [n_fields * Cp]; group g's fields
    follow those of the groups before it.  mean, var: f32 [M / members, n_fields_total, ld] contiguous; work: f32 workspace or None."""
    field0 = 0
    for g, d in zip(groups_arr, groups):
        H, W2 = d["H"], d["W2"]
        g.H, g.W2, g.bias, g.dH, g.Z = H.data_ptr(), W2.data_ptr(), d["bias"].data_ptr(), None, None
        g.ldh, g.ldw, g.lddh, g.ldz = H.stride(0), W2.stride(0), 0, 0
        g.n_fields, g.field0 = W2.shape[0] // Cp, field0
        field0 += g.n_fields
    P.w, P.var_scale, P.counts, P.mean, P.var, P.work = N.ptr(weights), N.ptr(var_scale), N.ptr(counts), mean.data_ptr(), var.data_ptr(), N.ptr(work)
    P.work_cap = 0 if work is None else work.numel()
    P.M, P.S, P.C, P.Cp, P.P = groups[0]["H"].shape[0], groups[0]["H"].shape[1], C_, Cp, n_patches
    P.members, P.n_fields_total, P.ld = members, field0, mean.shape[2]


def decode_member_moments(groups: Sequence[Dict], C_: int, Cp: int, n_patches: int, members: int = 1, weights: Optional[torch.Tensor] = None,
                          var_scale: Optional[torch.Tensor] = None, counts: Optional[torch.Tensor] = None, ld: Optional[int] = None,
                          dtype: torch.dtype = torch.bfloat16):
    """sea_decode_member_moments: (mean, var) of the decoder's second layer over the `members` consecutive members of every history, each f32
    [M / members, n_fields_total, ld] (ld: row width of the outputs, default Cp; every element is written, invalid and pad columns as 0).  groups as
    fill_decode_member_moments; row m is patch m % n_patches of member m // n_patches.  weights: f32 [M / n_patches] normalised per history, or None
    (1 / members); var_scale: f32 [M / (n_patches * members)] or None; counts: device int32 [n_patches] or None.  Everything is checked on the host
    before the launch."""
    if dtype != torch.bfloat16:
        raise ValueError(f"decode_member_moments: the fused launch is bf16 only, got {dtype}")
    if not groups or len(groups) > N.DECODE_MSE_MAX_GROUPS:
        raise ValueError(f"decode_member_moments: {len(groups)} groups; a launch carries 1 .. {N.DECODE_MSE_MAX_GROUPS}")
    if Cp < 32 or Cp % 32 or not 1 <= C_ <= Cp:
        raise ValueError(f"decode_member_moments: need Cp a multiple of 32 and 1 <= C <= Cp, got C = {C_}, Cp = {Cp}")
    ld = Cp if ld is None else ld
    if ld < C_ or ld % 4:
        raise ValueError(f"decode_member_moments: ld = {ld} must be a multiple of 4 that covers C = {C_}")
    dev = groups[0]["H"].device
    M, S = tuple(groups[0]["H"].shape) if groups[0]["H"].dim() == 2 else (0, 0)
    if M < 1 or S < 8 or S % 8 or S > N.DECODE_MSE_MAX_S:
        raise ValueError(f"decode_member_moments: H must be [M >= 1, S] with S a multiple of 8 up to {N.DECODE_MSE_MAX_S}, got {tuple(groups[0]['H'].shape)}")
    if n_patches < 1 or members < 1:
        raise ValueError(f"decode_member_moments: n_patches = {n_patches} and members = {members} must be positive")
    if M % (n_patches * members):
        raise ValueError(f"decode_member_moments: {M} rows are not a multiple of n_patches * members = {n_patches} * {members}")
    n_fields = 0
    for i, d in enumerate(groups):
        for name in ("H", "W2"):
            t = d[name]
            if t.dim() != 2 or t.stride(1) != 1:
                raise ValueError(f"decode_member_moments group {i}: {name}: need a 2-D tensor with unit inner stride, got shape {tuple(t.shape)} strides {t.stride()}")
            if t.dtype != dtype or t.device != dev or t.shape[1] != S or (name != "W2" and t.shape[0] != M):
                raise ValueError(f"decode_member_moments group {i}: {name} must be a {dtype} [{'n_fields * Cp' if name == 'W2' else M}, {S}] tensor on {dev}, got "
                                 f"{tuple(t.shape)} {t.dtype} on {t.device}")
            if t.stride(0) % 8 or t.data_ptr() % 16:
                raise ValueError(f"decode_member_moments group {i}: {name} needs a row stride that is a multiple of 8 and a 16-byte-aligned base (stride {t.stride(0)})")
        W2, b = d["W2"], d["bias"]
        if W2.shape[0] < Cp or W2.shape[0] % Cp:
            raise ValueError(f"decode_member_moments group {i}: W2 has {W2.shape[0]} rows, not a multiple of Cp = {Cp}")
        if b.dtype != torch.float32 or b.dim() != 1 or b.shape[0] != W2.shape[0] or not b.is_contiguous() or b.device != dev or b.data_ptr() % 16:
            raise ValueError(f"decode_member_moments group {i}: bias must be a contiguous, 16-byte-aligned float32 [{W2.shape[0]}] on {dev}, got {tuple(b.shape)} {b.dtype}")
        n_fields += W2.shape[0] // Cp
    Bm, B = M // n_patches, M // (n_patches * members)
    for name, t, n in (("weights", weights, Bm), ("var_scale", var_scale, B)):
        if t is not None and (not torch.is_tensor(t) or t.dtype != torch.float32 or t.dim() != 1 or t.shape[0] != n or not t.is_contiguous() or t.device != dev):
            raise ValueError(f"decode_member_moments: {name} must be a contiguous float32 [{n}] tensor on {dev}, got "
                             f"{(tuple(t.shape), t.dtype, str(t.device)) if torch.is_tensor(t) else type(t).__name__}")
    if counts is not None and (counts.dtype != torch.int32 or counts.dim() != 1 or counts.shape[0] != n_patches or not counts.is_contiguous() or counts.device != dev):
        raise ValueError(f"decode_member_moments: counts must be a contiguous int32 [{n_patches}] on {dev}, got {tuple(counts.shape)} {counts.dtype} on {counts.device}")
    N.require_gpu(groups[0]["H"], "decode_member_moments hidden rows")   # every operand is on their device (checked above)
    rows = M // members
    mean = torch.empty(rows, n_fields, ld, device=dev, dtype=torch.float32)
    var = torch.empty(rows, n_fields, ld, device=dev, dtype=torch.float32)
    n_chunks = (members + N.MEMBER_MOMENTS_CHUNK - 1) // N.MEMBER_MOMENTS_CHUNK
    work = torch.empty(n_chunks * (2 * mean.numel() + rows), device=dev, dtype=torch.float32) if n_chunks > 1 else None
    arr, P = (N.SeaDecodeMseGroup * len(groups))(), N.SeaDecodeMemberMoments()
    fill_decode_member_moments(arr, P, groups, weights, var_scale, counts, n_patches, members, C_, Cp, mean, var, work)
    N.check(N.lib().sea_decode_member_moments(arr, len(groups), C.byref(P), N.dtype_code(dtype), N.stream_ptr()), "sea_decode_member_moments")
    return mean, var


def fill_decode_member_gram(groups_arr, P: N.SeaDecodeMemberGram, groups: Sequence[Dict], obs, prec_field, prec, counts, n_patches: int, members: int, C_: int, Cp: int,
                            gram, proj, count) -> None:
    """The argument table of sea_decode_member_gram.  groups as fill_decode_member_moments; obs (and prec, when given) f32 [B * n_patches, n_fields_total,
    >= C] with unit inner stride; prec_field f32 [n_fields_total] or None; gram f64 [B, n_patches, members, members], proj f64 [B, n_patches, members],
    count int32 [B, n_patches], contiguous."""
    field0 = 0
    for g, d in zip(groups_arr, groups):
        H, W2 = d["H"], d["W2"]
        g.H, g.W2, g.bias, g.dH, g.Z = H.data_ptr(), W2.data_ptr(), d["bias"].data_ptr(), None, None
        g.ldh, g.ldw, g.lddh, g.ldz = H.stride(0), W2.stride(0), 0, 0
        g.n_fields, g.field0 = W2.shape[0] // Cp, field0
        field0 += g.n_fields
    P.obs, P.prec_field, P.prec, P.counts = obs.data_ptr(), N.ptr(prec_field), N.ptr(prec), N.ptr(counts)
    P.gram, P.proj, P.count = gram.data_ptr(), proj.data_ptr(), count.data_ptr()
    P.ld_row, P.ld_field = obs.stride(0), obs.stride(1)
    P.ld_prow, P.ld_pfield = (0, 0) if prec is None else (prec.stride(0), prec.stride(1))
    P.M, P.S, P.C, P.Cp, P.P = groups[0]["H"].shape[0], groups[0]["H"].shape[1], C_, Cp, n_patches
    P.members, P.n_fields_total, P.pad_ = members, field0, 0


def decode_member_gram(groups: Sequence[Dict], obs: torch.Tensor, C_: int, Cp: int, n_patches: int, members: int, prec_field: Optional[torch.Tensor] = None,
                       prec: Optional[torch.Tensor] = None, counts: Optional[torch.Tensor] = None, dtype: torch.dtype = torch.bfloat16, out=None):
    """sea_decode_member_gram: per (history, patch) the Gram matrix of the members' weighted decoded anomalies, its product with the innovation and the
    number of live cells (include/sea_hip.h states the formulas): (gram f64 [B, n_patches, members, members], proj f64 [B, n_patches, members], count int32
    [B, n_patches]) on the device; nothing is read back.  groups as fill_decode_member_moments (row m is patch m % n_patches of member m // n_patches);
    obs f32 [B * n_patches, n_fields, >= C] with unit inner stride; prec None or a map of obs's shape; prec_field None or f32 [n_fields]; counts device
    int32 [n_patches] or None; out: (gram, proj, count) tensors to write into (every element is written).  Everything is checked on the host before the
    launch."""
    what = "decode_member_gram"
    if dtype != torch.bfloat16:
        raise ValueError(f"{what}: the fused launch is bf16 only, got {dtype}")
    if not groups or len(groups) > N.DECODE_MSE_MAX_GROUPS:
        raise ValueError(f"{what}: {len(groups)} groups; a launch carries 1 .. {N.DECODE_MSE_MAX_GROUPS}")
    if Cp < 32 or Cp % 32 or not 1 <= C_ <= Cp:
        raise ValueError(f"{what}: need Cp a multiple of 32 and 1 <= C <= Cp, got C = {C_}, Cp = {Cp}")
    dev = groups[0]["H"].device
    M, S = tuple(groups[0]["H"].shape) if groups[0]["H"].dim() == 2 else (0, 0)
    if M < 1 or S < 8 or S % 8 or S > N.DECODE_MSE_MAX_S:
        raise ValueError(f"{what}: H must be [M >= 1, S] with S a multiple of 8 up to {N.DECODE_MSE_MAX_S}, got {tuple(groups[0]['H'].shape)}")
    if not isinstance(members, int) or isinstance(members, bool) or members < 2 or members > N.ENKF_MAX_N:
        raise ValueError(f"{what}: members = {members!r} must be an integer in 2 .. {N.ENKF_MAX_N}")
    if n_patches < 1 or M % (n_patches * members):
        raise ValueError(f"{what}: {M} rows are not a multiple of n_patches * members = {n_patches} * {members}")
    n_fields = 0
    for i, d in enumerate(groups):
        for name in ("H", "W2"):
            t = d[name]
            if t.dim() != 2 or t.stride(1) != 1:
                raise ValueError(f"{what} group {i}: {name}: need a 2-D tensor with unit inner stride, got shape {tuple(t.shape)} strides {t.stride()}")
            if t.dtype != dtype or t.device != dev or t.shape[1] != S or (name != "W2" and t.shape[0] != M):
                raise ValueError(f"{what} group {i}: {name} must be a {dtype} [{'n_fields * Cp' if name == 'W2' else M}, {S}] tensor on {dev}, got "
                                 f"{tuple(t.shape)} {t.dtype} on {t.device}")
            if t.stride(0) % 8 or t.data_ptr() % 16:
                raise ValueError(f"{what} group {i}: {name} needs a row stride that is a multiple of 8 and a 16-byte-aligned base (stride {t.stride(0)})")
        W2, b = d["W2"], d["bias"]
        if W2.shape[0] < Cp or W2.shape[0] % Cp:
            raise ValueError(f"{what} group {i}: W2 has {W2.shape[0]} rows, not a multiple of Cp = {Cp}")
        if b.dtype != torch.float32 or b.dim() != 1 or b.shape[0] != W2.shape[0] or not b.is_contiguous() or b.device != dev or b.data_ptr() % 16:
            raise ValueError(f"{what} group {i}: bias must be a contiguous, 16-byte-aligned float32 [{W2.shape[0]}] on {dev}, got {tuple(b.shape)} {b.dtype}")
        n_fields += W2.shape[0] // Cp
    B = M // (n_patches * members)
    for name, t in (("obs", obs), ("prec", prec)):
        if t is None and name == "prec":
            continue
        if not torch.is_tensor(t) or t.dtype != torch.float32 or t.dim() != 3 or tuple(t.shape[:2]) != (B * n_patches, n_fields) or t.shape[2] < C_ or t.stride(2) != 1 \
                or t.device != dev or t.stride(1) < C_ or (t.shape[0] > 1 and t.stride(0) < 0):
            raise ValueError(f"{what}: {name} must be a float32 [{B * n_patches}, {n_fields}, >= {C_}] tensor with unit inner stride on {dev}, got "
                             f"{(tuple(t.shape), t.dtype, t.stride(), str(t.device)) if torch.is_tensor(t) else type(t).__name__}")
    if prec_field is not None and (not torch.is_tensor(prec_field) or prec_field.dtype != torch.float32 or tuple(prec_field.shape) != (n_fields,)
                                   or not prec_field.is_contiguous() or prec_field.device != dev):
        raise ValueError(f"{what}: prec_field must be None or a contiguous float32 [{n_fields}] tensor on {dev}")
    if counts is not None and (counts.dtype != torch.int32 or counts.dim() != 1 or counts.shape[0] != n_patches or not counts.is_contiguous() or counts.device != dev):
        raise ValueError(f"{what}: counts must be a contiguous int32 [{n_patches}] on {dev}, got {tuple(counts.shape)} {counts.dtype} on {counts.device}")
    if out is not None:
        shapes = ((B, n_patches, members, members), (B, n_patches, members), (B, n_patches))
        if not isinstance(out, (tuple, list)) or len(out) != 3 or any(
                not torch.is_tensor(t) or t.dtype != dt_ or tuple(t.shape) != sh or not t.is_contiguous() or t.device != dev
                for t, sh, dt_ in zip(out, shapes, (torch.float64, torch.float64, torch.int32))):
            raise ValueError(f"{what}: out must be contiguous (float64 {shapes[0]}, float64 {shapes[1]}, int32 {shapes[2]}) tensors on {dev}")
    N.require_gpu(groups[0]["H"], f"{what} hidden rows")   # every operand is on their device (checked above)
    if out is not None:
        gram, proj, count = out
    else:
        gram = torch.empty(B, n_patches, members, members, device=dev, dtype=torch.float64)
        proj = torch.empty(B, n_patches, members, device=dev, dtype=torch.float64)
        count = torch.empty(B, n_patches, device=dev, dtype=torch.int32)
    arr, P = (N.SeaDecodeMseGroup * len(groups))(), N.SeaDecodeMemberGram()
    fill_decode_member_gram(arr, P, groups, obs, prec_field, prec, counts, n_patches, members, C_, Cp, gram, proj, count)
    N.check(N.lib().sea_decode_member_gram(arr, len(groups), C.byref(P), N.dtype_code(dtype), N.stream_ptr()), "sea_decode_member_gram")
    return gram, proj, count


def resample_systematic(logw: torch.Tensor, u: torch.Tensor, members: int, ess_frac: float = -1.0):
    """sea_resample_systematic: logw f32 [G * members] (device, contiguous), u f32 [G] in [0, 1), ess_frac < 0: always resample, else only the histories
    whose effective sample size is below ess_frac * members.  Returns (index int32 [G * members], logw_out f32 [G * members], ess f32 [G], resampled
    int32 [G]) on the device; nothing is read back."""
    n = int(members)
    if n < 1 or n > N.RESAMPLE_MAX_N:
        raise ValueError(f"resample_systematic: members = {members} outside 1 .. {N.RESAMPLE_MAX_N}")
    if logw.dim() != 1 or logw.dtype != torch.float32 or not logw.is_contiguous() or logw.numel() < 1 or logw.numel() % n:
        raise ValueError(f"resample_systematic: logw must be a contiguous float32 [G * {n}] tensor, got {tuple(logw.shape)} {logw.dtype}")
    G = logw.numel() // n
    if u.dim() != 1 or u.dtype != torch.float32 or u.shape[0] != G or not u.is_contiguous() or u.device != logw.device:
        raise ValueError(f"resample_systematic: u must be a contiguous float32 [{G}] tensor on {logw.device}, got {tuple(u.shape)} {u.dtype} on {u.device}")
    ess_frac = float(ess_frac)
    if ess_frac != ess_frac:
        raise ValueError("resample_systematic: ess_frac is NaN")
    N.require_gpu(logw, "resample_systematic log-weights")
    dev = logw.device
    index = torch.empty(G * n, device=dev, dtype=torch.int32)
    logw_out = torch.empty(G * n, device=dev, dtype=torch.float32)
    ess = torch.empty(G, device=dev, dtype=torch.float32)
    resampled = torch.empty(G, device=dev, dtype=torch.int32)
    N.check(N.lib().sea_resample_systematic(logw.data_ptr(), u.data_ptr(), ess_frac, G, n, index.data_ptr(), logw_out.data_ptr(), ess.data_ptr(),
                                            resampled.data_ptr(), N.stream_ptr()), "sea_resample_systematic")
    return index, logw_out, ess, resampled


def fill_enkf_transform(P: N.SeaEnkfTransform, pred, obs, prec, taper, members: int, rho: float, alpha: float, D, status) -> None:
    """The argument table of sea_enkf_transform.  pred f32 [B * members, K], obs f32 [B, K], prec None / f32 [K] / [B, K], taper None / f32 [Ld, K] (unit inner
    strides); D f32 [B, Ld, members, members] and status int32 [B, Ld], contiguous."""
    P.pred, P.obs, P.prec, P.taper, P.D, P.status = pred.data_ptr(), obs.data_ptr(), N.ptr(prec), N.ptr(taper), D.data_ptr(), status.data_ptr()
    P.ld_pred, P.ld_obs = pred.stride(0), obs.stride(0)
    P.ld_prec = 0 if prec is None or prec.dim() == 1 else prec.stride(0)
    P.ld_taper = 0 if taper is None else taper.stride(0)
    P.rho, P.alpha = rho, alpha
    P.B, P.N, P.K, P.Ld = obs.shape[0], members, obs.shape[1], D.shape[1]


def enkf_transform(pred: torch.Tensor, obs: torch.Tensor, members: int, prec: Optional[torch.Tensor] = None, taper: Optional[torch.Tensor] = None,
                   rho: float = 1.0, alpha: float = 0.5, out: Optional[torch.Tensor] = None):
    """sea_enkf_transform: the ensemble-space matrix of the deterministic ensemble Kalman analysis (include/sea_hip.h states the formulas).  pred f32
    [B * members, K] (the predictions of Decode.sensor_sse), obs f32 [B, K], prec None, f32 [K] or [B, K], taper None (one domain) or f32 [Ld, K]; rho >= 1
    the inflation, alpha in [0, 1] the anomaly gain.  Returns (D f32 [B, Ld, members, members], status int32 [B, Ld]: the live sensors of the problem, or
    -1 with D = 0 where a live operand was not finite) on the device; nothing is read back.  out: a D to write into."""
    what = "enkf_transform"
    n = members
    if not isinstance(n, int) or isinstance(n, bool) or n < 2 or n > N.ENKF_MAX_N:
        raise ValueError(f"{what}: members = {members!r} must be an integer in 2 .. {N.ENKF_MAX_N}")
    if not torch.is_tensor(obs) or obs.dim() != 2 or obs.dtype != torch.float32 or obs.shape[0] < 1 or obs.shape[1] < 1 or obs.stride(1) != 1:
        raise ValueError(f"{what}: obs must be a float32 [B, K] tensor with unit inner stride, got {tuple(obs.shape) if torch.is_tensor(obs) else type(obs).__name__}")
    B, K = obs.shape
    dev = obs.device
    if not torch.is_tensor(pred) or pred.dtype != torch.float32 or tuple(pred.shape) != (B * n, K) or pred.stride(1) != 1 or pred.stride(0) < K or pred.device != dev:
        raise ValueError(f"{what}: pred must be a float32 [{B * n}, {K}] tensor with unit inner stride on {dev}, got "
                         f"{(tuple(pred.shape), pred.dtype, str(pred.device)) if torch.is_tensor(pred) else type(pred).__name__}")
    if obs.stride(0) < K and B > 1:
        raise ValueError(f"{what}: obs rows overlap (strides {obs.stride()})")
    if prec is not None and (not torch.is_tensor(prec) or prec.dtype != torch.float32 or tuple(prec.shape) not in ((K,), (B, K)) or prec.stride(-1) != 1
                             or prec.device != dev or (prec.dim() == 2 and B > 1 and prec.stride(0) < K)):
        raise ValueError(f"{what}: prec must be None or a float32 [{K}] or [{B}, {K}] tensor with unit inner stride on {dev}, got "
                         f"{(tuple(prec.shape), prec.dtype, str(prec.device)) if torch.is_tensor(prec) else type(prec).__name__}")
    if prec is not None and prec.dim() == 2 and prec.stride(0) < K:   # one history whose row stride says nothing: the [K] form
        prec = prec[0]
    if taper is not None and (not torch.is_tensor(taper) or taper.dtype != torch.float32 or taper.dim() != 2 or taper.shape[0] < 1 or taper.shape[1] != K
                              or not taper.is_contiguous() or taper.device != dev):
        raise ValueError(f"{what}: taper must be None or a contiguous float32 [Ld, {K}] tensor on {dev}, got "
                         f"{(tuple(taper.shape), taper.dtype, str(taper.device)) if torch.is_tensor(taper) else type(taper).__name__}")
    rho, alpha = float(rho), float(alpha)
    if not (1.0 <= rho < float("inf")) or not (0.0 <= alpha <= 1.0):
        raise ValueError(f"{what}: need a finite inflation rho >= 1 and an anomaly gain alpha in [0, 1], got rho = {rho}, alpha = {alpha}")
    Ld = 1 if taper is None else taper.shape[0]
    if B > 65535:
        raise ValueError(f"{what}: {B} histories; a launch carries up to 65535")
    if out is not None and (not torch.is_tensor(out) or out.dtype != torch.float32 or tuple(out.shape) != (B, Ld, n, n) or not out.is_contiguous() or out.device != dev):
        raise ValueError(f"{what}: out must be a contiguous float32 [{B}, {Ld}, {n}, {n}] tensor on {dev}")
    N.require_gpu(obs, f"{what} obs")   # every operand is on the readings' device (checked above)
    D = torch.empty(B, Ld, n, n, device=dev, dtype=torch.float32) if out is None else out
    status = torch.empty(B, Ld, device=dev, dtype=torch.int32)
    P = N.SeaEnkfTransform()
    fill_enkf_transform(P, pred, obs, prec, taper, n, rho, alpha, D, status)
    P.ld_obs = max(P.ld_obs, K)   # one history: its row stride is never used and may say anything
    N.check(N.lib().sea_enkf_transform(C.byref(P), N.stream_ptr()), "sea_enkf_transform")
    return D, status


def fill_enkf_transform_gram(P: N.SeaEnkfTransformGram, gram, proj, count, taper, rho: float, alpha: float, D, status) -> None:
    """The argument table of sea_enkf_transform_gram.  gram f64 [B, Q, members, members], proj f64 [B, Q, members], count int32 [B, Q], taper None / f32
    [Ld, Q] (unit inner stride); D f32 [B, Ld, members, members] and status int32 [B, Ld], contiguous."""
    P.gram, P.proj, P.count, P.taper, P.D, P.status = gram.data_ptr(), proj.data_ptr(), count.data_ptr(), N.ptr(taper), D.data_ptr(), status.data_ptr()
    P.ld_taper = 0 if taper is None else taper.stride(0)
    P.rho, P.alpha = rho, alpha
    P.B, P.N, P.Q, P.Ld = gram.shape[0], gram.shape[2], gram.shape[1], D.shape[1]


def enkf_transform_gram(gram: torch.Tensor, proj: torch.Tensor, count: torch.Tensor, taper: Optional[torch.Tensor] = None, rho: float = 1.0, alpha: float = 0.5,
                        out: Optional[torch.Tensor] = None):
    """sea_enkf_transform_gram: the ensemble-space matrix of the deterministic ensemble Kalman analysis from Q partial Gram matrices per history
    (decode_member_gram's outputs; include/sea_hip.h states the formulas).  gram f64 [B, Q, n, n], proj f64 [B, Q, n], count int32 [B, Q], contiguous;
    taper None (one domain: every partial with weight 1) or f32 [Ld, Q]; rho >= 1 the inflation, alpha in [0, 1] the anomaly gain.  Returns (D f32 [B, Ld,
    n, n], status int32 [B, Ld]: the live cells of the problem, or -1 with D = 0) on the device; nothing is read back.  out: a D to write into."""
    what = "enkf_transform_gram"
    if not torch.is_tensor(gram) or gram.dim() != 4 or gram.dtype != torch.float64 or not gram.is_contiguous() or gram.shape[2] != gram.shape[3] or gram.shape[0] < 1 \
            or gram.shape[1] < 1:
        raise ValueError(f"{what}: gram must be a contiguous float64 [B, Q, members, members] tensor, got "
                         f"{(tuple(gram.shape), gram.dtype) if torch.is_tensor(gram) else type(gram).__name__}")
    B, Q, n, _ = gram.shape
    dev = gram.device
    if n < 2 or n > N.ENKF_MAX_N:
        raise ValueError(f"{what}: members = {n} outside 2 .. {N.ENKF_MAX_N}")
    if not torch.is_tensor(proj) or proj.dtype != torch.float64 or tuple(proj.shape) != (B, Q, n) or not proj.is_contiguous() or proj.device != dev:
        raise ValueError(f"{what}: proj must be a contiguous float64 [{B}, {Q}, {n}] tensor on {dev}")
    if not torch.is_tensor(count) or count.dtype != torch.int32 or tuple(count.shape) != (B, Q) or not count.is_contiguous() or count.device != dev:
        raise ValueError(f"{what}: count must be a contiguous int32 [{B}, {Q}] tensor on {dev}")
    if taper is not None and (not torch.is_tensor(taper) or taper.dtype != torch.float32 or taper.dim() != 2 or taper.shape[0] < 1 or taper.shape[1] != Q
                              or not taper.is_contiguous() or taper.device != dev):
        raise ValueError(f"{what}: taper must be None or a contiguous float32 [Ld, {Q}] tensor on {dev}, got "
                         f"{(tuple(taper.shape), taper.dtype, str(taper.device)) if torch.is_tensor(taper) else type(taper).__name__}")
    rho, alpha = float(rho), float(alpha)
    if not (1.0 <= rho < float("inf")) or not (0.0 <= alpha <= 1.0):
        raise ValueError(f"{what}: need a finite inflation rho >= 1 and an anomaly gain alpha in [0, 1], got rho = {rho}, alpha = {alpha}")
    Ld = 1 if taper is None else taper.shape[0]
    if B > 65535:
        raise ValueError(f"{what}: {B} histories; a launch carries up to 65535")
    if out is not None and (not torch.is_tensor(out) or out.dtype != torch.float32 or tuple(out.shape) != (B, Ld, n, n) or not out.is_contiguous() or out.device != dev):
        raise ValueError(f"{what}: out must be a contiguous float32 [{B}, {Ld}, {n}, {n}] tensor on {dev}")
    N.require_gpu(gram, f"{what} gram")   # every operand is on its device (checked above)
    D = torch.empty(B, Ld, n, n, device=dev, dtype=torch.float32) if out is None else out
    status = torch.empty(B, Ld, device=dev, dtype=torch.int32)
    P = N.SeaEnkfTransformGram()
    fill_enkf_transform_gram(P, gram, proj, count, taper, rho, alpha, D, status)
    N.check(N.lib().sea_enkf_transform_gram(C.byref(P), N.stream_ptr()), "sea_enkf_transform_gram")
    return D, status


def fill_ensemble_mix(P: N.SeaEnsembleMix, y, D, out, inc, members: int, n_patches: int) -> None:
    """The argument table of sea_ensemble_mix.  y act [Bm, G, n_patches * Dl] contiguous, D f32 [Bm / members, Ld, members, members] contiguous; out (y's
    dtype) and inc (f32) in y's shape, contiguous, either may be None."""
    P.y, P.D, P.out, P.inc = y.data_ptr(), D.data_ptr(), N.ptr(out), N.ptr(inc)
    P.Bm, P.N, P.G, P.P, P.Dl, P.Ld = y.shape[0], members, y.shape[1], n_patches, y.shape[2] // n_patches, D.shape[1]


def ensemble_mix(y: torch.Tensor, D: torch.Tensor, n_patches: int, output: bool = True, increment: bool = False):
    """sea_ensemble_mix: out[b * n + j, g, p, :] = y[...] + sum_i D[b, dom(p), i, j] * y[b * n + i, g, p, :] with n = D.shape[-1] members per history and
    dom(p) = 0 for D [B, 1, n, n], p for D [B, n_patches, n, n].  y [B * n, G, n_patches * Dl] float32 or bfloat16, contiguous.  Returns out (y's dtype;
    a new tensor), the fp32 increment, or (out, increment), as `output` and `increment` ask; nothing is read back."""
    what = "ensemble_mix"
    if not output and not increment:
        raise ValueError(f"{what}: neither the output nor the increment is asked for")
    if not isinstance(n_patches, int) or isinstance(n_patches, bool) or n_patches < 1:
        raise ValueError(f"{what}: n_patches = {n_patches!r} must be a positive integer")
    if not torch.is_tensor(y) or y.dim() != 3 or y.dtype not in (torch.float32, torch.bfloat16) or not y.is_contiguous() or y.shape[0] < 1 or y.shape[1] < 1 \
            or y.shape[2] < 1 or y.shape[2] % n_patches:
        raise ValueError(f"{what}: y must be a contiguous float32 or bfloat16 [B * members, n_groups, {n_patches} * D] tensor, got "
                         f"{(tuple(y.shape), y.dtype) if torch.is_tensor(y) else type(y).__name__}")
    if not torch.is_tensor(D) or D.dim() != 4 or D.dtype != torch.float32 or not D.is_contiguous() or D.shape[2] != D.shape[3] or D.device != y.device:
        raise ValueError(f"{what}: D must be a contiguous float32 [B, Ld, members, members] tensor on {y.device}, got "
                         f"{(tuple(D.shape), D.dtype, str(D.device)) if torch.is_tensor(D) else type(D).__name__}")
    n = D.shape[2]
    if n < 2 or n > N.ENKF_MAX_N:
        raise ValueError(f"{what}: members = {n} outside 2 .. {N.ENKF_MAX_N}")
    if y.shape[0] != D.shape[0] * n:
        raise ValueError(f"{what}: y holds {y.shape[0]} trajectories, D is for {D.shape[0]} histories of {n} members")
    if D.shape[1] not in (1, n_patches):
        raise ValueError(f"{what}: D has {D.shape[1]} domains; need 1 or n_patches = {n_patches}")
    N.require_gpu(y, f"{what} states")
    out = torch.empty_like(y) if output else None
    inc = torch.empty(y.shape, device=y.device, dtype=torch.float32) if increment else None
    P = N.SeaEnsembleMix()
    fill_ensemble_mix(P, y, D, out, inc, n, n_patches)
    N.check(N.lib().sea_ensemble_mix(C.byref(P), N.dtype_code(y.dtype), N.stream_ptr()), "sea_ensemble_mix")
    return (out, inc) if output and increment else (out if output else inc)


VERIFY_OUTPUTS = ("mean", "spread", "crps", "pit", "rank", "sums", "hist", "status")


def fill_ensemble_verify(P: N.SeaEnsembleVerify, pred, obs, prec, logw, members: int, unbiased: bool, accumulate: bool, mean, spread, crps, pit, rank,
                         sums, hist, status, work) -> None:
    """The argument table of sea_ensemble_verify.  pred f32 [B * members, K], obs f32 [B, K], prec None / f32 [K] / [B, K] (unit inner strides), logw None /
    f32 [B * members] contiguous; mean, spread, crps, pit f32 and rank int32 [B, K] contiguous or None; sums f64 [B, 8], hist int64 [B, members + 1],
    status int32 [B] contiguous; work: a uint8 workspace of at least sea_ensemble_verify_ws_bytes(B, members, K) bytes."""
    P.pred, P.obs, P.prec, P.logw = pred.data_ptr(), obs.data_ptr(), N.ptr(prec), N.ptr(logw)
    P.mean, P.spread, P.crps, P.pit, P.rank = N.ptr(mean), N.ptr(spread), N.ptr(crps), N.ptr(pit), N.ptr(rank)
    P.sums, P.hist, P.status, P.work = sums.data_ptr(), hist.data_ptr(), status.data_ptr(), work.data_ptr()
    P.ld_pred, P.ld_obs = pred.stride(0), obs.stride(0)
    P.ld_prec = 0 if prec is None or prec.dim() == 1 else prec.stride(0)
    P.ld_out = obs.shape[1]
    P.work_bytes = work.numel() * work.element_size()
    P.B, P.N, P.K, P.unbiased, P.accumulate, P.pad_ = obs.shape[0], members, obs.shape[1], int(bool(unbiased)), int(bool(accumulate)), 0


def ensemble_verify(pred: torch.Tensor, obs: torch.Tensor, members: int, prec: Optional[torch.Tensor] = None, logw: Optional[torch.Tensor] = None,
                    unbiased: bool = True, accumulate: bool = False, out: Optional[Dict[str, torch.Tensor]] = None) -> Dict[str, torch.Tensor]:
    """sea_ensemble_verify: CRPS, PIT, rank, mean and spread of an ensemble at the sensors, and per history the fp64 sums and the rank histogram
    (include/sea_hip.h states the formulas).  pred f32 [B * members, K] (the predictions of Decode.sensor_sse), obs f32 [B, K], prec None, f32 [K] or
    [B, K] (a host-side one is checked for finite values >= 0; one on the device is not read back), logw None or f32 [B * members] unnormalised
    log-weights.  Returns a dict: mean, spread, crps, pit f32 [B, K], rank int32 [B, K], sums f64 [B, 8], hist int64 [B, members + 1], status int32 [B] —
    on the device; nothing is read back.  out: a dict of tensors to write into, by those names; accumulate=True adds this call's sums and histogram
    onto out["sums"] and out["hist"], which are then required."""
    what = "ensemble_verify"
    n = members
    if not isinstance(n, int) or isinstance(n, bool) or n < 1 or n > N.VERIFY_MAX_N:
        raise ValueError(f"{what}: members = {members!r} must be an integer in 1 .. {N.VERIFY_MAX_N}")
    if not torch.is_tensor(obs) or obs.dim() != 2 or obs.dtype != torch.float32 or obs.shape[0] < 1 or obs.shape[1] < 1 or obs.stride(1) != 1:
        raise ValueError(f"{what}: obs must be a float32 [B, K] tensor with unit inner stride, got {tuple(obs.shape) if torch.is_tensor(obs) else type(obs).__name__}")
    B, K = obs.shape
    dev = obs.device
    if not torch.is_tensor(pred) or pred.dtype != torch.float32 or tuple(pred.shape) != (B * n, K) or pred.stride(1) != 1 or (pred.stride(0) < K and B * n > 1) \
            or pred.device != dev:
        raise ValueError(f"{what}: pred must be a float32 [{B * n}, {K}] tensor with unit inner stride on {dev}, got "
                         f"{(tuple(pred.shape), pred.dtype, str(pred.device)) if torch.is_tensor(pred) else type(pred).__name__}")
    if obs.stride(0) < K and B > 1:
        raise ValueError(f"{what}: obs rows overlap (strides {obs.stride()})")
    if prec is not None and (not torch.is_tensor(prec) or prec.dtype != torch.float32 or tuple(prec.shape) not in ((K,), (B, K)) or prec.stride(-1) != 1
                             or prec.device != dev or (prec.dim() == 2 and B > 1 and prec.stride(0) < K)):
        raise ValueError(f"{what}: prec must be None or a float32 [{K}] or [{B}, {K}] tensor with unit inner stride on {dev}, got "
                         f"{(tuple(prec.shape), prec.dtype, str(prec.device)) if torch.is_tensor(prec) else type(prec).__name__}")
    if prec is not None and prec.device.type == "cpu" and (not bool(torch.isfinite(prec).all()) or not bool((prec >= 0).all())):
        raise ValueError(f"{what}: prec must be finite and >= 0")
    if prec is not None and prec.dim() == 2 and prec.stride(0) < K:   # one history whose row stride says nothing: the [K] form
        prec = prec[0]
    if logw is not None and (not torch.is_tensor(logw) or logw.dtype != torch.float32 or tuple(logw.shape) != (B * n,) or not logw.is_contiguous() or logw.device != dev):
        raise ValueError(f"{what}: logw must be None or a contiguous float32 [{B * n}] tensor on {dev}, got "
                         f"{(tuple(logw.shape), logw.dtype, str(logw.device)) if torch.is_tensor(logw) else type(logw).__name__}")
    if B > 65535:
        raise ValueError(f"{what}: {B} histories; a launch carries up to 65535")
    shapes = {"mean": ((B, K), torch.float32), "spread": ((B, K), torch.float32), "crps": ((B, K), torch.float32), "pit": ((B, K), torch.float32),
              "rank": ((B, K), torch.int32), "sums": ((B, N.VERIFY_SUMS), torch.float64), "hist": ((B, n + 1), torch.int64), "status": ((B,), torch.int32)}
    out = {} if out is None else out
    if not isinstance(out, dict) or any(k not in shapes for k in out):
        raise ValueError(f"{what}: out must be a dict with keys among {VERIFY_OUTPUTS}")
    for k, t in out.items():
        shape, dt = shapes[k]
        if not torch.is_tensor(t) or tuple(t.shape) != shape or t.dtype != dt or not t.is_contiguous() or t.device != dev:
            raise ValueError(f"{what}: out[{k!r}] must be a contiguous {dt} {list(shape)} tensor on {dev}")
    if accumulate and ("sums" not in out or "hist" not in out):
        raise ValueError(f"{what}: accumulate=True adds onto out['sums'] and out['hist']: both are required")
    N.require_gpu(obs, f"{what} obs")   # every operand is on the readings' device (checked above)
    res = {k: out[k] if k in out else torch.empty(shapes[k][0], device=dev, dtype=shapes[k][1]) for k in VERIFY_OUTPUTS}
    work = torch.empty(int(N.lib().sea_ensemble_verify_ws_bytes(B, n, K)), device=dev, dtype=torch.uint8)
    P = N.SeaEnsembleVerify()
    fill_ensemble_verify(P, pred, obs, prec, logw, n, unbiased, accumulate, res["mean"], res["spread"], res["crps"], res["pit"], res["rank"], res["sums"],
                         res["hist"], res["status"], work)
    P.ld_obs, P.ld_pred = max(P.ld_obs, K), max(P.ld_pred, K)   # a single row: its stride is never used and may say anything
    N.check(N.lib().sea_ensemble_verify(C.byref(P), N.stream_ptr()), "sea_ensemble_verify")
    return res


FIELD_VERIFY_MAPS = ("mean", "spread", "crps", "pit", "rank")


def fill_decode_member_verify(groups_arr, P: N.SeaDecodeMemberVerify, groups: Sequence[Dict], obs, prec_field, prec, counts, logw, n_patches: int, members: int,
                              C_: int, Cp: int, unbiased: bool, accumulate: bool, mean, spread, crps, pit, rank, sums, hist, status, work, ld_out: int) -> None:
    """The argument table of sea_decode_member_verify.  groups, obs, prec_field, prec, counts as fill_decode_member_gram; logw None or f32 [B * members]
    contiguous; mean, spread, crps, pit f32 and rank int32 [B, n_patches, n_fields_total, ld_out] contiguous or None; sums f64 [B, n_fields_total, 8], hist
    int64 [B, n_fields_total, members + 1], status int32 [B] contiguous; work: a uint8 workspace of at least sea_decode_member_verify_ws_bytes(...) bytes."""
    field0 = 0
    for g, d in zip(groups_arr, groups):
        H, W2 = d["H"], d["W2"]
        g.H, g.W2, g.bias, g.dH, g.Z = H.data_ptr(), W2.data_ptr(), d["bias"].data_ptr(), None, None
        g.ldh, g.ldw, g.lddh, g.ldz = H.stride(0), W2.stride(0), 0, 0
        g.n_fields, g.field0 = W2.shape[0] // Cp, field0
        field0 += g.n_fields
    P.obs, P.prec_field, P.prec, P.counts, P.logw = obs.data_ptr(), N.ptr(prec_field), N.ptr(prec), N.ptr(counts), N.ptr(logw)
    P.mean, P.spread, P.crps, P.pit, P.rank = N.ptr(mean), N.ptr(spread), N.ptr(crps), N.ptr(pit), N.ptr(rank)
    P.sums, P.hist, P.status, P.work = sums.data_ptr(), hist.data_ptr(), status.data_ptr(), work.data_ptr()
    P.ld_row, P.ld_field = obs.stride(0), obs.stride(1)
    P.ld_prow, P.ld_pfield = (0, 0) if prec is None else (prec.stride(0), prec.stride(1))
    P.ld_out, P.work_bytes = ld_out, work.numel() * work.element_size()
    P.M, P.S, P.C, P.Cp, P.P = groups[0]["H"].shape[0], groups[0]["H"].shape[1], C_, Cp, n_patches
    P.members, P.n_fields_total, P.unbiased, P.accumulate, P.pad_ = members, field0, int(bool(unbiased)), int(bool(accumulate)), 0


def decode_member_verify(groups: Sequence[Dict], obs: torch.Tensor, C_: int, Cp: int, n_patches: int, members: int, prec_field: Optional[torch.Tensor] = None,
                         prec: Optional[torch.Tensor] = None, counts: Optional[torch.Tensor] = None, logw: Optional[torch.Tensor] = None, unbiased: bool = True,
                         accumulate: bool = False, maps: Sequence[str] = FIELD_VERIFY_MAPS, out: Optional[Dict[str, torch.Tensor]] = None,
                         dtype: torch.dtype = torch.bfloat16) -> Dict[str, torch.Tensor]:
    """sea_decode_member_verify: CRPS, PIT, rank, mean and spread of an ensemble at every cell of a dense observation of the decoded fields, and per
    (history, field) the fp64 sums and the rank histogram (include/sea_hip.h states the formulas) — the members' decoded fields are never written.
    groups, obs, prec_field, prec, counts as decode_member_gram; logw None or f32 [B * members] unnormalised log-weights; maps: the per-cell outputs to
    produce, a subset of ("mean", "spread", "crps", "pit", "rank").  Returns a dict: the maps asked for, f32 (rank int32) [B, n_patches, n_fields, C]
    (every element written), sums f64 [B, n_fields, 8], hist int64 [B, n_fields, members + 1], status int32 [B] — on the device; nothing is read back.
    out: a dict of tensors to write into, by those names (a map given there is produced whether `maps` names it or not; its last dimension may be any
    width >= C, the same for all maps); accumulate=True adds this call's sums and histograms onto out["sums"] and out["hist"], which are then required.
    Everything is checked on the host before the launch."""
    what = "decode_member_verify"
    if dtype != torch.bfloat16:
        raise ValueError(f"{what}: the fused launch is bf16 only, got {dtype}")
    if not groups or len(groups) > N.DECODE_MSE_MAX_GROUPS:
        raise ValueError(f"{what}: {len(groups)} groups; a launch carries 1 .. {N.DECODE_MSE_MAX_GROUPS}")
    if Cp < 32 or Cp % 32 or not 1 <= C_ <= Cp:
        raise ValueError(f"{what}: need Cp a multiple of 32 and 1 <= C <= Cp, got C = {C_}, Cp = {Cp}")
    dev = groups[0]["H"].device
    M, S = tuple(groups[0]["H"].shape) if groups[0]["H"].dim() == 2 else (0, 0)
    if M < 1 or S < 8 or S % 8 or S > N.DECODE_MSE_MAX_S:
        raise ValueError(f"{what}: H must be [M >= 1, S] with S a multiple of 8 up to {N.DECODE_MSE_MAX_S}, got {tuple(groups[0]['H'].shape)}")
    n = members
    if not isinstance(n, int) or isinstance(n, bool) or n < 1 or n > N.FIELD_VERIFY_MAX_N:
        raise ValueError(f"{what}: members = {members!r} must be an integer in 1 .. {N.FIELD_VERIFY_MAX_N}")
    if n_patches < 1 or M % (n_patches * n):
        raise ValueError(f"{what}: {M} rows are not a multiple of n_patches * members = {n_patches} * {n}")
    n_fields = 0
    for i, d in enumerate(groups):
        for name in ("H", "W2"):
            t = d[name]
            if t.dim() != 2 or t.stride(1) != 1:
                raise ValueError(f"{what} group {i}: {name}: need a 2-D tensor with unit inner stride, got shape {tuple(t.shape)} strides {t.stride()}")
            if t.dtype != dtype or t.device != dev or t.shape[1] != S or (name != "W2" and t.shape[0] != M):
                raise ValueError(f"{what} group {i}: {name} must be a {dtype} [{'n_fields * Cp' if name == 'W2' else M}, {S}] tensor on {dev}, got "
                                 f"{tuple(t.shape)} {t.dtype} on {t.device}")
            if t.stride(0) % 8 or t.data_ptr() % 16:
                raise ValueError(f"{what} group {i}: {name} needs a row stride that is a multiple of 8 and a 16-byte-aligned base (stride {t.stride(0)})")
        W2, b = d["W2"], d["bias"]
        if W2.shape[0] < Cp or W2.shape[0] % Cp:
            raise ValueError(f"{what} group {i}: W2 has {W2.shape[0]} rows, not a multiple of Cp = {Cp}")
        if b.dtype != torch.float32 or b.dim() != 1 or b.shape[0] != W2.shape[0] or not b.is_contiguous() or b.device != dev or b.data_ptr() % 16:
            raise ValueError(f"{what} group {i}: bias must be a contiguous, 16-byte-aligned float32 [{W2.shape[0]}] on {dev}, got {tuple(b.shape)} {b.dtype}")
        n_fields += W2.shape[0] // Cp
    B = M // (n_patches * n)
    if B > 65535:
        raise ValueError(f"{what}: {B} histories; a launch carries up to 65535")
    for name, t in (("obs", obs), ("prec", prec)):
        if t is None and name == "prec":
            continue
        if not torch.is_tensor(t) or t.dtype != torch.float32 or t.dim() != 3 or tuple(t.shape[:2]) != (B * n_patches, n_fields) or t.shape[2] < C_ or t.stride(2) != 1 \
                or t.device != dev or t.stride(1) < C_ or (t.shape[0] > 1 and t.stride(0) < 0):
            raise ValueError(f"{what}: {name} must be a float32 [{B * n_patches}, {n_fields}, >= {C_}] tensor with unit inner stride on {dev}, got "
                             f"{(tuple(t.shape), t.dtype, t.stride(), str(t.device)) if torch.is_tensor(t) else type(t).__name__}")
    if prec_field is not None and (not torch.is_tensor(prec_field) or prec_field.dtype != torch.float32 or tuple(prec_field.shape) != (n_fields,)
                                   or not prec_field.is_contiguous() or prec_field.device != dev):
        raise ValueError(f"{what}: prec_field must be None or a contiguous float32 [{n_fields}] tensor on {dev}")
    if counts is not None and (not torch.is_tensor(counts) or counts.dtype != torch.int32 or counts.dim() != 1 or counts.shape[0] != n_patches
                               or not counts.is_contiguous() or counts.device != dev):
        raise ValueError(f"{what}: counts must be a contiguous int32 [{n_patches}] on {dev}")
    if logw is not None and (not torch.is_tensor(logw) or logw.dtype != torch.float32 or tuple(logw.shape) != (B * n,) or not logw.is_contiguous() or logw.device != dev):
        raise ValueError(f"{what}: logw must be None or a contiguous float32 [{B * n}] tensor on {dev}, got "
                         f"{(tuple(logw.shape), logw.dtype, str(logw.device)) if torch.is_tensor(logw) else type(logw).__name__}")
    maps = tuple(maps)
    if any(k not in FIELD_VERIFY_MAPS for k in maps) or len(set(maps)) != len(maps):
        raise ValueError(f"{what}: maps must be distinct names among {FIELD_VERIFY_MAPS}, got {maps!r}")
    out = {} if out is None else out
    fixed = {"sums": ((B, n_fields, N.VERIFY_SUMS), torch.float64), "hist": ((B, n_fields, n + 1), torch.int64), "status": ((B,), torch.int32)}
    if not isinstance(out, dict) or any(k not in fixed and k not in FIELD_VERIFY_MAPS for k in out):
        raise ValueError(f"{what}: out must be a dict with keys among {FIELD_VERIFY_MAPS + tuple(fixed)}")
    widths = {t.shape[-1] for k, t in out.items() if k in FIELD_VERIFY_MAPS and torch.is_tensor(t) and t.dim() == 4}
    if len(widths) > 1:
        raise ValueError(f"{what}: the maps in out must share their last dimension, got {sorted(widths)}")
    ld_out = widths.pop() if widths else C_
    for k, t in out.items():
        shape, dt = fixed[k] if k in fixed else ((B, n_patches, n_fields, ld_out), torch.int32 if k == "rank" else torch.float32)
        if not torch.is_tensor(t) or tuple(t.shape) != shape or t.dtype != dt or not t.is_contiguous() or t.device != dev or ld_out < C_:
            raise ValueError(f"{what}: out[{k!r}] must be a contiguous {dt} {list(shape)} tensor on {dev} (maps: last dimension >= {C_})")
    if accumulate and ("sums" not in out or "hist" not in out):
        raise ValueError(f"{what}: accumulate=True adds onto out['sums'] and out['hist']: both are required")
    N.require_gpu(groups[0]["H"], f"{what} hidden rows")   # every operand is on their device (checked above)
    res = {k: out[k] if k in out else torch.empty(fixed[k][0], device=dev, dtype=fixed[k][1]) for k in fixed}
    for k in FIELD_VERIFY_MAPS:
        if k in out:
            res[k] = out[k]
        elif k in maps:
            res[k] = torch.empty(B, n_patches, n_fields, ld_out, device=dev, dtype=torch.int32 if k == "rank" else torch.float32)
    work = torch.empty(int(N.lib().sea_decode_member_verify_ws_bytes(B, n_patches, n_fields, n, Cp)), device=dev, dtype=torch.uint8)
    arr, P = (N.SeaDecodeMseGroup * len(groups))(), N.SeaDecodeMemberVerify()
    fill_decode_member_verify(arr, P, groups, obs, prec_field, prec, counts, logw, n_patches, n, C_, Cp, unbiased, accumulate, res.get("mean"), res.get("spread"),
                              res.get("crps"), res.get("pit"), res.get("rank"), res["sums"], res["hist"], res["status"], work, ld_out)
    N.check(N.lib().sea_decode_member_verify(arr, len(groups), C.byref(P), N.dtype_code(dtype), N.stream_ptr()), "sea_decode_member_verify")
    return res


def fill_decode_member_crps_grad(groups_arr, P: N.SeaDecodeMemberCrpsGrad, groups: Sequence[Dict], obs, prec_field, prec, field_weight, counts, logw, n_patches: int,
                                members: int, C_: int, Cp: int, unbiased: bool, loss, sums, status, work) -> None:
    """The argument table of sea_decode_member_crps_grad.  groups: dicts H act [M, S], W2 act [n_fields * Cp, S], bias f32 [n_fields * Cp], dH act [M, S]
    (output) and an optional Z act [M, S]; obs, prec_field, prec, counts, logw as fill_decode_member_verify; field_weight None or f32 [n_fields_total]
    contiguous; loss f32 [B, n_fields_total], sums f64 [B, n_fields_total, 8], status int32 [B] contiguous; work: a uint8 workspace of at least
    sea_decode_member_crps_grad_ws_bytes(...) bytes."""
    field0 = 0
    for g, d in zip(groups_arr, groups):
        H, W2, dH, Z = d["H"], d["W2"], d["dH"], d.get("Z")
        g.H, g.W2, g.bias, g.dH, g.Z = H.data_ptr(), W2.data_ptr(), d["bias"].data_ptr(), dH.data_ptr(), N.ptr(Z)
        g.ldh, g.ldw, g.lddh, g.ldz = H.stride(0), W2.stride(0), dH.stride(0), (Z.stride(0) if Z is not None else 0)
        g.n_fields, g.field0 = W2.shape[0] // Cp, field0
        field0 += g.n_fields
    P.obs, P.prec_field, P.prec, P.field_weight = obs.data_ptr(), N.ptr(prec_field), N.ptr(prec), N.ptr(field_weight)
    P.counts, P.logw = N.ptr(counts), N.ptr(logw)
    P.loss, P.sums, P.status, P.work = loss.data_ptr(), sums.data_ptr(), status.data_ptr(), work.data_ptr()
    P.ld_row, P.ld_field = obs.stride(0), obs.stride(1)
    P.ld_prow, P.ld_pfield = (0, 0) if prec is None else (prec.stride(0), prec.stride(1))
    P.work_bytes = work.numel() * work.element_size()
    P.M, P.S, P.C, P.Cp, P.P = groups[0]["H"].shape[0], groups[0]["H"].shape[1], C_, Cp, n_patches
    P.members, P.n_fields_total, P.unbiased = members, field0, int(bool(unbiased))


def decode_member_crps_grad_supported(S: int, members: int) -> bool:
    """Whether sea_decode_member_crps_grad carries this hidden width and member count (include/sea_hip.h: above 64 members the fused gradient form
    stops at S = 384; what it refuses takes the composed path)."""
    return 8 <= S <= N.DECODE_MSE_MAX_S and 1 <= members <= N.FIELD_VERIFY_MAX_N and (members <= 64 or S <= N.CRPS_GRAD_W8_MAX_S)


def decode_member_crps_pack_supported(S: int, members: int) -> bool:
    """Whether sea_decode_member_crps_grad_packed carries this hidden width and member count (include/sea_hip.h: 1 .. 32 members at every hidden width
    the unpacked form carries, S up to 640; every instantiation compiles without scratch, so none is refused)."""
    return 8 <= S <= N.DECODE_MSE_MAX_S and S % 8 == 0 and 1 <= members <= N.CRPS_PACK_MAX_N


def decode_member_crps_pack_shape(S: int, members: int):
    """(NP, HG) of the packed form at this shape: NP the member count rounded up to a power of two (at least 2), HG the histories one workgroup
    serves — 64 / NP, except 16 at 1 or 2 members above S = 512 (include/sea_hip.h; DESIGN.md section 7n has the LDS table)."""
    if not decode_member_crps_pack_supported(S, members):
        raise ValueError(f"decode_member_crps_pack_shape: S = {S}, members = {members} is not carried by the packed form")
    NP = 2
    while NP < members:
        NP *= 2
    return NP, (16 if NP == 2 and S > 512 else 64 // NP)


def decode_member_crps_grad(groups: Sequence[Dict], obs: torch.Tensor, C_: int, Cp: int, n_patches: int, members: int, prec: Optional[torch.Tensor] = None,
                            prec_field: Optional[torch.Tensor] = None, field_weight: Optional[torch.Tensor] = None, counts: Optional[torch.Tensor] = None,
                            logw: Optional[torch.Tensor] = None, unbiased: bool = True, dtype: torch.dtype = torch.bfloat16, pack: bool = False):
    """sea_decode_member_crps_grad: the CRPS of an ensemble's decoded fields against a dense observation, summed per (history, field), WITH its gradient
    to the hidden rows (include/sea_hip.h states the formulas) — neither the members' decoded fields nor their gradient are written.  groups: dicts H,
    W2, bias as decode_member_verify, plus dH act [M, S] (written IN PLACE, every element) and an optional Z act [M, S] (gelu' of it is applied); obs,
    prec_field, prec, counts, logw as decode_member_verify; field_weight None or a contiguous f32 [n_fields].  Returns (loss f32 [B, n_fields] =
    field_weight * sums[..., 1], sums f64 [B, n_fields, 8] with decode_member_verify's bits, status int32 [B]) on the device; nothing is read back.
    A shape the fused form does not carry (decode_member_crps_grad_supported) raises RuntimeError from the library's SEA_EUNSUPPORTED.  Everything is
    checked on the host before the launch.  pack=True: sea_decode_member_crps_grad_packed through the same argument table — several histories per
    workgroup for 1 .. 32 members (decode_member_crps_pack_supported), every output with the bits of pack=False; a shape it refuses raises likewise."""
    what = "decode_member_crps_grad"
    if dtype != torch.bfloat16:
        raise ValueError(f"{what}: the fused launch is bf16 only, got {dtype}")
    if not groups or len(groups) > N.DECODE_MSE_MAX_GROUPS:
        raise ValueError(f"{what}: {len(groups)} groups; a launch carries 1 .. {N.DECODE_MSE_MAX_GROUPS}")
    if Cp < 32 or Cp % 32 or not 1 <= C_ <= Cp:
        raise ValueError(f"{what}: need Cp a multiple of 32 and 1 <= C <= Cp, got C = {C_}, Cp = {Cp}")
    H0 = groups[0].get("H")
    if not torch.is_tensor(H0) or H0.dim() != 2:
        raise ValueError(f"{what}: H must be a 2-D tensor, got {tuple(H0.shape) if torch.is_tensor(H0) else type(H0).__name__}")
    dev = H0.device
    M, S = tuple(H0.shape)
    if M < 1 or S < 8 or S % 8 or S > N.DECODE_MSE_MAX_S:
        raise ValueError(f"{what}: H must be [M >= 1, S] with S a multiple of 8 up to {N.DECODE_MSE_MAX_S}, got {tuple(H0.shape)}")
    n = members
    if not isinstance(n, int) or isinstance(n, bool) or n < 1 or n > N.FIELD_VERIFY_MAX_N:
        raise ValueError(f"{what}: members = {members!r} must be an integer in 1 .. {N.FIELD_VERIFY_MAX_N}")
    if not isinstance(n_patches, int) or n_patches < 1 or M % (n_patches * n):
        raise ValueError(f"{what}: {M} rows are not a multiple of n_patches * members = {n_patches} * {n}")
    n_fields = 0
    for i, d in enumerate(groups):
        for name in ("H", "W2", "dH", "Z"):
            t = d.get(name)
            if t is None and name == "Z":
                continue
            if not torch.is_tensor(t) or t.dim() != 2 or t.stride(1) != 1:
                raise ValueError(f"{what} group {i}: {name}: need a 2-D tensor with unit inner stride, got "
                                 f"{f'shape {tuple(t.shape)} strides {t.stride()}' if torch.is_tensor(t) else type(t).__name__}")
            if t.dtype != dtype or t.device != dev or t.shape[1] != S or (name != "W2" and t.shape[0] != M):
                raise ValueError(f"{what} group {i}: {name} must be a {dtype} [{'n_fields * Cp' if name == 'W2' else M}, {S}] tensor on {dev}, got "
                                 f"{tuple(t.shape)} {t.dtype} on {t.device}")
            if t.stride(0) % 8 or t.stride(0) < S or t.data_ptr() % 16:
                raise ValueError(f"{what} group {i}: {name} needs a row stride that is a multiple of 8 and covers S = {S}, and a 16-byte-aligned base (stride {t.stride(0)})")
        W2, b = d["W2"], d["bias"]
        if W2.shape[0] < Cp or W2.shape[0] % Cp:
            raise ValueError(f"{what} group {i}: W2 has {W2.shape[0]} rows, not a multiple of Cp = {Cp}")
        if b.dtype != torch.float32 or b.dim() != 1 or b.shape[0] != W2.shape[0] or not b.is_contiguous() or b.device != dev or b.data_ptr() % 16:
            raise ValueError(f"{what} group {i}: bias must be a contiguous, 16-byte-aligned float32 [{W2.shape[0]}] on {dev}, got {tuple(b.shape)} {b.dtype}")
        n_fields += W2.shape[0] // Cp
    B = M // (n_patches * n)
    if B > 65535:
        raise ValueError(f"{what}: {B} histories; a launch carries up to 65535")
    for name, t in (("obs", obs), ("prec", prec)):
        if t is None and name == "prec":
            continue
        if not torch.is_tensor(t) or t.dtype != torch.float32 or t.dim() != 3 or tuple(t.shape[:2]) != (B * n_patches, n_fields) or t.shape[2] < C_ or t.stride(2) != 1 \
                or t.device != dev or t.stride(1) < C_ or (t.shape[0] > 1 and t.stride(0) < 0):
            raise ValueError(f"{what}: {name} must be a float32 [{B * n_patches}, {n_fields}, >= {C_}] tensor with unit inner stride on {dev}, got "
                             f"{(tuple(t.shape), t.dtype, t.stride(), str(t.device)) if torch.is_tensor(t) else type(t).__name__}")
    for name, t in (("prec_field", prec_field), ("field_weight", field_weight)):
        if t is not None and (not torch.is_tensor(t) or t.dtype != torch.float32 or tuple(t.shape) != (n_fields,) or not t.is_contiguous() or t.device != dev):
            raise ValueError(f"{what}: {name} must be None or a contiguous float32 [{n_fields}] tensor on {dev}")
    if counts is not None and (not torch.is_tensor(counts) or counts.dtype != torch.int32 or counts.dim() != 1 or counts.shape[0] != n_patches
                               or not counts.is_contiguous() or counts.device != dev):
        raise ValueError(f"{what}: counts must be a contiguous int32 [{n_patches}] on {dev}")
    if logw is not None and (not torch.is_tensor(logw) or logw.dtype != torch.float32 or tuple(logw.shape) != (B * n,) or not logw.is_contiguous() or logw.device != dev):
        raise ValueError(f"{what}: logw must be None or a contiguous float32 [{B * n}] tensor on {dev}, got "
                         f"{(tuple(logw.shape), logw.dtype, str(logw.device)) if torch.is_tensor(logw) else type(logw).__name__}")
    N.require_gpu(H0, f"{what} hidden rows")   # every operand is on their device (checked above)
    loss = torch.empty(B, n_fields, device=dev, dtype=torch.float32)
    sums = torch.empty(B, n_fields, N.VERIFY_SUMS, device=dev, dtype=torch.float64)
    status = torch.empty(B, device=dev, dtype=torch.int32)
    need = int(N.lib().sea_decode_member_crps_grad_ws_bytes(B, n_patches, n_fields, n, Cp, S))
    work = torch.empty(max(need, 8), device=dev, dtype=torch.uint8)   # (a refused shape asks for -1: the entry point below says why)
    arr, P = (N.SeaDecodeMseGroup * len(groups))(), N.SeaDecodeMemberCrpsGrad()
    fill_decode_member_crps_grad(arr, P, groups, obs, prec_field, prec, field_weight, counts, logw, n_patches, n, C_, Cp, unbiased, loss, sums, status, work)
    entry = "sea_decode_member_crps_grad_packed" if pack else "sea_decode_member_crps_grad"
    N.check(getattr(N.lib(), entry)(arr, len(groups), C.byref(P), N.dtype_code(dtype), N.stream_ptr()), entry)
    return loss, sums, status


def fill_decode_member_quantiles(groups_arr, P: N.SeaDecodeMemberQuantiles, groups: Sequence[Dict], w, counts, thr, levels: Sequence[float], quant, exceed,
                                 n_patches: int, members: int, C_: int, Cp: int, ld: int, ld_map: int) -> None:
    """The argument table of sea_decode_member_quantiles.  groups as fill_decode_member_verify; w None or f32 [B * members] contiguous; counts None or
    int32 [n_patches]; thr None or f32 [n_thr, n_fields_total] contiguous; levels: the host's floats; quant f32 [n_levels, B, n_patches, n_fields_total,
    ld] and exceed f32 [n_thr, ...] contiguous, or None; ld_map: floats between two maps."""
    field0 = 0
    for g, d in zip(groups_arr, groups):
        H, W2 = d["H"], d["W2"]
        g.H, g.W2, g.bias, g.dH, g.Z = H.data_ptr(), W2.data_ptr(), d["bias"].data_ptr(), None, None
        g.ldh, g.ldw, g.lddh, g.ldz = H.stride(0), W2.stride(0), 0, 0
        g.n_fields, g.field0 = W2.shape[0] // Cp, field0
        field0 += g.n_fields
    P.w, P.counts, P.thr, P.quant, P.exceed = N.ptr(w), N.ptr(counts), N.ptr(thr), N.ptr(quant), N.ptr(exceed)
    for k in range(N.QUANTILE_MAX_LEVELS):
        P.level[k] = float(levels[k]) if k < len(levels) else 0.0
    P.ld, P.ld_map = ld, ld_map
    P.n_levels, P.n_thr = len(levels), 0 if thr is None else thr.shape[0]
    P.M, P.S, P.C, P.Cp, P.P = groups[0]["H"].shape[0], groups[0]["H"].shape[1], C_, Cp, n_patches
    P.members, P.n_fields_total, P.pad_ = members, field0, 0


def decode_member_quantiles(groups: Sequence[Dict], C_: int, Cp: int, n_patches: int, members: int, levels: Sequence[float] = (),
                            thr: Optional[torch.Tensor] = None, w: Optional[torch.Tensor] = None, counts: Optional[torch.Tensor] = None,
                            out: Optional[Dict[str, torch.Tensor]] = None, dtype: torch.dtype = torch.bfloat16) -> Dict[str, Optional[torch.Tensor]]:
    """sea_decode_member_quantiles: weighted quantile maps and exceedance-probability maps of an ensemble's decoded fields in one launch
    (include/sea_hip.h states the definitions) — the members' decoded fields are never written.  groups, counts as decode_member_verify; levels: up to 8
    floats in [0, 1]; thr None or f32 [T <= 8, n_fields] thresholds in the decoder's scaled units; w None (equal weights) or f32 [B * members], normalised
    per history; a member with w <= 0 or NaN is dead.  Returns dict(quant=f32 [Q, B, n_patches, n_fields, C] or None, exceed=f32 [T, ...] or None):
    every element written, nothing read back.  out: a dict with "quant" and / or "exceed" to write into (their last dimension may be any width >= C,
    the same for both).  Everything is checked on the host before the launch."""
    what = "decode_member_quantiles"
    if dtype != torch.bfloat16:
        raise ValueError(f"{what}: the fused launch is bf16 only, got {dtype}")
    if not groups or len(groups) > N.DECODE_MSE_MAX_GROUPS:
        raise ValueError(f"{what}: {len(groups)} groups; a launch carries 1 .. {N.DECODE_MSE_MAX_GROUPS}")
    if Cp < 32 or Cp % 32 or not 1 <= C_ <= Cp:
        raise ValueError(f"{what}: need Cp a multiple of 32 and 1 <= C <= Cp, got C = {C_}, Cp = {Cp}")
    dev = groups[0]["H"].device
    M, S = tuple(groups[0]["H"].shape) if groups[0]["H"].dim() == 2 else (0, 0)
    if groups[0]["H"].dtype != dtype:
        raise ValueError(f"{what}: the fused launch is bf16 only, got hidden rows in {groups[0]['H'].dtype}")
    if M < 1 or S < 8 or S % 8 or S > N.DECODE_MSE_MAX_S:
        raise ValueError(f"{what}: H must be [M >= 1, S] with S a multiple of 8 up to {N.DECODE_MSE_MAX_S}, got {tuple(groups[0]['H'].shape)}")
    n = members
    if not isinstance(n, int) or isinstance(n, bool) or n < 1 or n > N.QUANTILE_MAX_N:
        raise ValueError(f"{what}: members = {members!r} must be an integer in 1 .. {N.QUANTILE_MAX_N}")
    if n_patches < 1 or M % (n_patches * n):
        raise ValueError(f"{what}: {M} rows are not a multiple of n_patches * members = {n_patches} * {n}")
    levels = check_quantile_levels(levels, what)
    n_fields = 0
    for i, d in enumerate(groups):
        for name in ("H", "W2"):
            t = d[name]
            if t.dim() != 2 or t.stride(1) != 1:
                raise ValueError(f"{what} group {i}: {name}: need a 2-D tensor with unit inner stride, got shape {tuple(t.shape)} strides {t.stride()}")
            if t.dtype != dtype or t.device != dev or t.shape[1] != S or (name != "W2" and t.shape[0] != M):
                raise ValueError(f"{what} group {i}: {name} must be a {dtype} [{'n_fields * Cp' if name == 'W2' else M}, {S}] tensor on {dev}, got "
                                 f"{tuple(t.shape)} {t.dtype} on {t.device}")
            if t.stride(0) % 8 or t.data_ptr() % 16:
                raise ValueError(f"{what} group {i}: {name} needs a row stride that is a multiple of 8 and a 16-byte-aligned base (stride {t.stride(0)})")
        W2, b = d["W2"], d["bias"]
        if W2.shape[0] < Cp or W2.shape[0] % Cp:
            raise ValueError(f"{what} group {i}: W2 has {W2.shape[0]} rows, not a multiple of Cp = {Cp}")
        if b.dtype != torch.float32 or b.dim() != 1 or b.shape[0] != W2.shape[0] or not b.is_contiguous() or b.device != dev or b.data_ptr() % 16:
            raise ValueError(f"{what} group {i}: bias must be a contiguous, 16-byte-aligned float32 [{W2.shape[0]}] on {dev}, got {tuple(b.shape)} {b.dtype}")
        n_fields += W2.shape[0] // Cp
    B = M // (n_patches * n)
    if B > 65535:
        raise ValueError(f"{what}: {B} histories; a launch carries up to 65535")
    if thr is not None and (not torch.is_tensor(thr) or thr.dtype != torch.float32 or thr.dim() != 2 or not 1 <= thr.shape[0] <= N.QUANTILE_MAX_LEVELS
                            or thr.shape[1] != n_fields or not thr.is_contiguous() or thr.device != dev):
        raise ValueError(f"{what}: thr must be None or a contiguous float32 [1 .. {N.QUANTILE_MAX_LEVELS}, {n_fields}] tensor on {dev}, got "
                         f"{(tuple(thr.shape), thr.dtype, str(thr.device)) if torch.is_tensor(thr) else type(thr).__name__}")
    if not levels and thr is None:
        raise ValueError(f"{what}: neither levels nor thresholds: there is nothing to compute")
    if w is not None and (not torch.is_tensor(w) or w.dtype != torch.float32 or tuple(w.shape) != (B * n,) or not w.is_contiguous() or w.device != dev):
        raise ValueError(f"{what}: w must be None or a contiguous float32 [{B * n}] tensor on {dev}, got "
                         f"{(tuple(w.shape), w.dtype, str(w.device)) if torch.is_tensor(w) else type(w).__name__}")
    if counts is not None and (not torch.is_tensor(counts) or counts.dtype != torch.int32 or counts.dim() != 1 or counts.shape[0] != n_patches
                               or not counts.is_contiguous() or counts.device != dev):
        raise ValueError(f"{what}: counts must be a contiguous int32 [{n_patches}] on {dev}")
    n_out = {"quant": len(levels), "exceed": 0 if thr is None else thr.shape[0]}
    out = {} if out is None else out
    if not isinstance(out, dict) or any(k not in n_out or n_out[k] == 0 for k in out):
        raise ValueError(f"{what}: out must be a dict with 'quant' (with levels) and / or 'exceed' (with thresholds)")
    widths = {t.shape[-1] for t in out.values() if torch.is_tensor(t) and t.dim() == 5}
    if len(widths) > 1:
        raise ValueError(f"{what}: the maps in out must share their last dimension, got {sorted(widths)}")
    ld = widths.pop() if widths else C_
    for k, t in out.items():
        shape = (n_out[k], B, n_patches, n_fields, ld)
        if not torch.is_tensor(t) or tuple(t.shape) != shape or t.dtype != torch.float32 or not t.is_contiguous() or t.device != dev or ld < C_:
            raise ValueError(f"{what}: out[{k!r}] must be a contiguous float32 {list(shape)} tensor on {dev} (last dimension >= {C_})")
    N.require_gpu(groups[0]["H"], f"{what} hidden rows")   # every operand is on their device (checked above)
    res = {k: (out[k] if k in out else torch.empty(n_out[k], B, n_patches, n_fields, ld, device=dev, dtype=torch.float32)) if n_out[k] else None for k in n_out}
    arr, P = (N.SeaDecodeMseGroup * len(groups))(), N.SeaDecodeMemberQuantiles()
    fill_decode_member_quantiles(arr, P, groups, w, counts, thr, levels, res["quant"], res["exceed"], n_patches, n, C_, Cp, ld, B * n_patches * n_fields * ld)
    N.check(N.lib().sea_decode_member_quantiles(arr, len(groups), C.byref(P), N.dtype_code(dtype), N.stream_ptr()), "sea_decode_member_quantiles")
    return res


def check_quantile_levels(levels, what: str) -> tuple:
    """The levels of a quantile call as a tuple of floats: at most 8, each finite and in [0, 1] — checked on the host, ValueError otherwise."""
    try:
        lv = tuple(float(v) for v in levels)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: levels must be a sequence of numbers in [0, 1], got {levels!r}") from None
    if len(lv) > N.QUANTILE_MAX_LEVELS:
        raise ValueError(f"{what}: {len(lv)} levels; a launch carries up to {N.QUANTILE_MAX_LEVELS}")
    if any(not (0.0 <= v <= 1.0) for v in lv):   # false for NaN
        raise ValueError(f"{what}: every level must be finite and lie in [0, 1], got {lv}")
    return lv


BRIER_MAPS = ("prob", "brier")


def check_brier_thresholds(thr, cols: int, dev, what: str) -> None:
    """thr of a threshold-score call: a contiguous float32 [1 .. 8, cols] tensor on `dev`; one on the host is also checked for finite values (one on the
    device is not read back: the classes check theirs at construction)."""
    if not torch.is_tensor(thr) or thr.dtype != torch.float32 or thr.dim() != 2 or not 1 <= thr.shape[0] <= N.BRIER_MAX_T or thr.shape[1] != cols \
            or not thr.is_contiguous() or thr.device != dev:
        raise ValueError(f"{what}: thr must be a contiguous float32 [1 .. {N.BRIER_MAX_T}, {cols}] tensor on {dev}, got "
                         f"{(tuple(thr.shape), thr.dtype, str(thr.device)) if torch.is_tensor(thr) else type(thr).__name__}")
    if thr.device.type == "cpu" and not bool(torch.isfinite(thr).all()):
        raise ValueError(f"{what}: every threshold must be finite")


def _brier_outputs(what: str, out, maps, accumulate: bool, fixed: Dict, map_shape, width: int, anchor: torch.Tensor):
    """The outputs of a threshold-score call: `out`'s tensors checked against their shapes (a map's last dimension may be any width >= `width`, the same
    for both maps), then — behind the check that `anchor`, the operand every other one was compared with, is on the GPU — the others allocated.
    map_shape(ld) is a map's shape at last dimension ld.  Returns (the dict of outputs, ld)."""
    dev = anchor.device
    maps = tuple(maps)
    if any(k not in BRIER_MAPS for k in maps) or len(set(maps)) != len(maps):
        raise ValueError(f"{what}: maps must be distinct names among {BRIER_MAPS}, got {maps!r}")
    out = {} if out is None else out
    if not isinstance(out, dict) or any(k not in fixed and k not in BRIER_MAPS for k in out):
        raise ValueError(f"{what}: out must be a dict with keys among {BRIER_MAPS + tuple(fixed)}")
    widths = {t.shape[-1] for k, t in out.items() if k in BRIER_MAPS and torch.is_tensor(t) and t.dim() == len(map_shape(width))}
    if len(widths) > 1:
        raise ValueError(f"{what}: the maps in out must share their last dimension, got {sorted(widths)}")
    ld = widths.pop() if widths else width
    for k, t in out.items():
        shape, dt = fixed[k] if k in fixed else (map_shape(ld), torch.float32)
        if not torch.is_tensor(t) or tuple(t.shape) != tuple(shape) or t.dtype != dt or not t.is_contiguous() or t.device != dev or ld < width:
            raise ValueError(f"{what}: out[{k!r}] must be a contiguous {dt} {list(shape)} tensor on {dev} (maps: last dimension >= {width})")
    if accumulate and any(k not in out for k in ("sums", "hist", "hits")):
        raise ValueError(f"{what}: accumulate=True adds onto out['sums'], out['hist'] and out['hits']: all three are required")
    N.require_gpu(anchor, f"{what} operands")   # every operand is on the anchor's device (checked by the caller)
    res = {k: out[k] if k in out else torch.empty(fixed[k][0], device=dev, dtype=fixed[k][1]) for k in fixed}
    for k in BRIER_MAPS:
        if k in out:
            res[k] = out[k]
        elif k in maps:
            res[k] = torch.empty(map_shape(ld), device=dev, dtype=torch.float32)
    return res, ld


def fill_ensemble_brier(P: N.SeaEnsembleBrier, pred, obs, prec, logw, thr, members: int, accumulate: bool, prob, brier, sums, hist, hits, status, work, ld_out: int) -> None:
    """The argument table of sea_ensemble_brier.  pred, obs, prec, logw as fill_ensemble_verify; thr f32 [T, K] contiguous; prob, brier f32 [T, B, ld_out]
    contiguous or None; sums f64 [B, T, 5], hist, hits int64 [B, T, members + 1], status int32 [B] contiguous; work: a uint8 workspace of at least
    sea_ensemble_brier_ws_bytes(B, members, K, T) bytes."""
    P.pred, P.obs, P.prec, P.logw, P.thr = pred.data_ptr(), obs.data_ptr(), N.ptr(prec), N.ptr(logw), thr.data_ptr()
    P.prob, P.brier = N.ptr(prob), N.ptr(brier)
    P.sums, P.hist, P.hits, P.status, P.work = sums.data_ptr(), hist.data_ptr(), hits.data_ptr(), status.data_ptr(), work.data_ptr()
    P.ld_pred, P.ld_obs, P.ld_thr = pred.stride(0), obs.stride(0), thr.stride(0)
    P.ld_prec = 0 if prec is None or prec.dim() == 1 else prec.stride(0)
    P.ld_out, P.ld_map = ld_out, obs.shape[0] * ld_out
    P.work_bytes = work.numel() * work.element_size()
    P.B, P.N, P.K, P.n_thr, P.accumulate, P.pad_ = obs.shape[0], members, obs.shape[1], thr.shape[0], int(bool(accumulate)), 0


def ensemble_brier(pred: torch.Tensor, obs: torch.Tensor, members: int, thr: torch.Tensor, prec: Optional[torch.Tensor] = None,
                   logw: Optional[torch.Tensor] = None, accumulate: bool = False, maps: Sequence[str] = BRIER_MAPS,
                   out: Optional[Dict[str, torch.Tensor]] = None) -> Dict[str, torch.Tensor]:
    """sea_ensemble_brier: the threshold scores of an ensemble at the sensors (include/sea_hip.h states the definitions).  pred, obs, prec, logw as
    ensemble_verify; thr f32 [T <= 8, K], a threshold per sensor.  Returns a dict: the maps asked for — prob, brier f32 [T, B, K] —, sums f64 [B, T, 5],
    hist and hits int64 [B, T, members + 1], status int32 [B]; nothing is read back.  out: a dict of tensors to write into, by those names (a map given
    there is produced whether `maps` names it or not); accumulate=True adds this call's sums, hist and hits onto out's, which are then required."""
    what = "ensemble_brier"
    n = members
    if not isinstance(n, int) or isinstance(n, bool) or n < 1 or n > N.BRIER_MAX_N:
        raise ValueError(f"{what}: members = {members!r} must be an integer in 1 .. {N.BRIER_MAX_N}")
    if not torch.is_tensor(obs) or obs.dim() != 2 or obs.dtype != torch.float32 or obs.shape[0] < 1 or obs.shape[1] < 1 or obs.stride(1) != 1:
        raise ValueError(f"{what}: obs must be a float32 [B, K] tensor with unit inner stride, got {tuple(obs.shape) if torch.is_tensor(obs) else type(obs).__name__}")
    B, K = obs.shape
    dev = obs.device
    if not torch.is_tensor(pred) or pred.dtype != torch.float32 or tuple(pred.shape) != (B * n, K) or pred.stride(1) != 1 or (pred.stride(0) < K and B * n > 1) \
            or pred.device != dev:
        raise ValueError(f"{what}: pred must be a float32 [{B * n}, {K}] tensor with unit inner stride on {dev}, got "
                         f"{(tuple(pred.shape), pred.dtype, str(pred.device)) if torch.is_tensor(pred) else type(pred).__name__}")
    if obs.stride(0) < K and B > 1:
        raise ValueError(f"{what}: obs rows overlap (strides {obs.stride()})")
    check_brier_thresholds(thr, K, dev, what)
    if prec is not None and (not torch.is_tensor(prec) or prec.dtype != torch.float32 or tuple(prec.shape) not in ((K,), (B, K)) or prec.stride(-1) != 1
                             or prec.device != dev or (prec.dim() == 2 and B > 1 and prec.stride(0) < K)):
        raise ValueError(f"{what}: prec must be None or a float32 [{K}] or [{B}, {K}] tensor with unit inner stride on {dev}, got "
                         f"{(tuple(prec.shape), prec.dtype, str(prec.device)) if torch.is_tensor(prec) else type(prec).__name__}")
    if prec is not None and prec.device.type == "cpu" and (not bool(torch.isfinite(prec).all()) or not bool((prec >= 0).all())):
        raise ValueError(f"{what}: prec must be finite and >= 0")
    if prec is not None and prec.dim() == 2 and prec.stride(0) < K:   # one history whose row stride says nothing: the [K] form
        prec = prec[0]
    if logw is not None and (not torch.is_tensor(logw) or logw.dtype != torch.float32 or tuple(logw.shape) != (B * n,) or not logw.is_contiguous() or logw.device != dev):
        raise ValueError(f"{what}: logw must be None or a contiguous float32 [{B * n}] tensor on {dev}, got "
                         f"{(tuple(logw.shape), logw.dtype, str(logw.device)) if torch.is_tensor(logw) else type(logw).__name__}")
    if B > 65535:
        raise ValueError(f"{what}: {B} histories; a launch carries up to 65535")
    T = thr.shape[0]
    fixed = {"sums": ((B, T, N.BRIER_SUMS), torch.float64), "hist": ((B, T, n + 1), torch.int64), "hits": ((B, T, n + 1), torch.int64), "status": ((B,), torch.int32)}
    res, ld = _brier_outputs(what, out, maps, accumulate, fixed, lambda ld: (T, B, ld), K, obs)
    work = torch.empty(int(N.lib().sea_ensemble_brier_ws_bytes(B, n, K, T)), device=dev, dtype=torch.uint8)
    P = N.SeaEnsembleBrier()
    fill_ensemble_brier(P, pred, obs, prec, logw, thr, n, accumulate, res.get("prob"), res.get("brier"), res["sums"], res["hist"], res["hits"], res["status"], work, ld)
    P.ld_obs, P.ld_pred = max(P.ld_obs, K), max(P.ld_pred, K)   # a single row: its stride is never used and may say anything
    N.check(N.lib().sea_ensemble_brier(C.byref(P), N.stream_ptr()), "sea_ensemble_brier")
    return res


def fill_decode_member_brier(groups_arr, P: N.SeaDecodeMemberBrier, groups: Sequence[Dict], obs, prec_field, prec, counts, logw, thr, n_patches: int, members: int,
                             C_: int, Cp: int, accumulate: bool, prob, brier, sums, hist, hits, status, work, ld_out: int) -> None:
    """The argument table of sea_decode_member_brier.  groups, obs, prec_field, prec, counts, logw as fill_decode_member_verify; thr f32 [T, n_fields_total]
    contiguous; prob, brier f32 [T, B, n_patches, n_fields_total, ld_out] contiguous or None; sums f64 [B, n_fields_total, T, 5], hist, hits int64
    [B, n_fields_total, T, members + 1], status int32 [B] contiguous; work: a uint8 workspace of at least sea_decode_member_brier_ws_bytes(...) bytes."""
    field0 = 0
    for g, d in zip(groups_arr, groups):
        H, W2 = d["H"], d["W2"]
        g.H, g.W2, g.bias, g.dH, g.Z = H.data_ptr(), W2.data_ptr(), d["bias"].data_ptr(), None, None
        g.ldh, g.ldw, g.lddh, g.ldz = H.stride(0), W2.stride(0), 0, 0
        g.n_fields, g.field0 = W2.shape[0] // Cp, field0
        field0 += g.n_fields
    P.obs, P.prec_field, P.prec, P.counts, P.logw, P.thr = obs.data_ptr(), N.ptr(prec_field), N.ptr(prec), N.ptr(counts), N.ptr(logw), thr.data_ptr()
    P.prob, P.brier = N.ptr(prob), N.ptr(brier)
    P.sums, P.hist, P.hits, P.status, P.work = sums.data_ptr(), hist.data_ptr(), hits.data_ptr(), status.data_ptr(), work.data_ptr()
    P.ld_row, P.ld_field = obs.stride(0), obs.stride(1)
    P.ld_prow, P.ld_pfield = (0, 0) if prec is None else (prec.stride(0), prec.stride(1))
    P.ld_out, P.ld_map, P.work_bytes = ld_out, obs.shape[0] * field0 * ld_out, work.numel() * work.element_size()
    P.M, P.S, P.C, P.Cp, P.P = groups[0]["H"].shape[0], groups[0]["H"].shape[1], C_, Cp, n_patches
    P.members, P.n_fields_total, P.n_thr, P.accumulate, P.pad_ = members, field0, thr.shape[0], int(bool(accumulate)), 0


def decode_member_brier(groups: Sequence[Dict], obs: torch.Tensor, C_: int, Cp: int, n_patches: int, members: int, thr: torch.Tensor,
                        prec: Optional[torch.Tensor] = None, prec_field: Optional[torch.Tensor] = None, counts: Optional[torch.Tensor] = None,
                        logw: Optional[torch.Tensor] = None, accumulate: bool = False, maps: Sequence[str] = BRIER_MAPS,
                        out: Optional[Dict[str, torch.Tensor]] = None, dtype: torch.dtype = torch.bfloat16) -> Dict[str, torch.Tensor]:
    """sea_decode_member_brier: the threshold scores of an ensemble at every cell of a dense observation of the decoded fields — the Brier sums, the
    histograms of the reliability diagram and the hit counts of the ROC (include/sea_hip.h states the definitions) — the members' decoded fields are
    never written.  groups, obs, prec_field, prec, counts, logw as decode_member_verify; thr f32 [T <= 8, n_fields] in the decoder's scaled units; maps:
    the per-cell outputs to produce, a subset of ("prob", "brier").  Returns a dict: the maps asked for, f32 [T, B, n_patches, n_fields, C] (every
    element written), sums f64 [B, n_fields, T, 5], hist and hits int64 [B, n_fields, T, members + 1], status int32 [B] — on the device; nothing is read
    back.  out: a dict of tensors to write into, by those names (a map given there is produced whether `maps` names it or not; its last dimension may be
    any width >= C, the same for both maps); accumulate=True adds this call's sums, hist and hits onto out's, which are then required.  Everything is
    checked on the host before the launch."""
    what = "decode_member_brier"
    if dtype != torch.bfloat16:
        raise ValueError(f"{what}: the fused launch is bf16 only, got {dtype}")
    if not groups or len(groups) > N.DECODE_MSE_MAX_GROUPS:
        raise ValueError(f"{what}: {len(groups)} groups; a launch carries 1 .. {N.DECODE_MSE_MAX_GROUPS}")
    if Cp < 32 or Cp % 32 or not 1 <= C_ <= Cp:
        raise ValueError(f"{what}: need Cp a multiple of 32 and 1 <= C <= Cp, got C = {C_}, Cp = {Cp}")
    dev = groups[0]["H"].device
    M, S = tuple(groups[0]["H"].shape) if groups[0]["H"].dim() == 2 else (0, 0)
    if M < 1 or S < 8 or S % 8 or S > N.DECODE_MSE_MAX_S:
        raise ValueError(f"{what}: H must be [M >= 1, S] with S a multiple of 8 up to {N.DECODE_MSE_MAX_S}, got {tuple(groups[0]['H'].shape)}")
    n = members
    if not isinstance(n, int) or isinstance(n, bool) or n < 1 or n > N.BRIER_MAX_N:
        raise ValueError(f"{what}: members = {members!r} must be an integer in 1 .. {N.BRIER_MAX_N}")
    if n_patches < 1 or M % (n_patches * n):
        raise ValueError(f"{what}: {M} rows are not a multiple of n_patches * members = {n_patches} * {n}")
    n_fields = 0
    for i, d in enumerate(groups):
        for name in ("H", "W2"):
            t = d[name]
            if t.dim() != 2 or t.stride(1) != 1:
                raise ValueError(f"{what} group {i}: {name}: need a 2-D tensor with unit inner stride, got shape {tuple(t.shape)} strides {t.stride()}")
            if t.dtype != dtype or t.device != dev or t.shape[1] != S or (name != "W2" and t.shape[0] != M):
                raise ValueError(f"{what} group {i}: {name} must be a {dtype} [{'n_fields * Cp' if name == 'W2' else M}, {S}] tensor on {dev}, got "
                                 f"{tuple(t.shape)} {t.dtype} on {t.device}")
            if t.stride(0) % 8 or t.data_ptr() % 16:
                raise ValueError(f"{what} group {i}: {name} needs a row stride that is a multiple of 8 and a 16-byte-aligned base (stride {t.stride(0)})")
        W2, b = d["W2"], d["bias"]
        if W2.shape[0] < Cp or W2.shape[0] % Cp:
            raise ValueError(f"{what} group {i}: W2 has {W2.shape[0]} rows, not a multiple of Cp = {Cp}")
        if b.dtype != torch.float32 or b.dim() != 1 or b.shape[0] != W2.shape[0] or not b.is_contiguous() or b.device != dev or b.data_ptr() % 16:
            raise ValueError(f"{what} group {i}: bias must be a contiguous, 16-byte-aligned float32 [{W2.shape[0]}] on {dev}, got {tuple(b.shape)} {b.dtype}")
        n_fields += W2.shape[0] // Cp
    B = M // (n_patches * n)
    if B > 65535:
        raise ValueError(f"{what}: {B} histories; a launch carries up to 65535")
    for name, t in (("obs", obs), ("prec", prec)):
        if t is None and name == "prec":
            continue
        if not torch.is_tensor(t) or t.dtype != torch.float32 or t.dim() != 3 or tuple(t.shape[:2]) != (B * n_patches, n_fields) or t.shape[2] < C_ or t.stride(2) != 1 \
                or t.device != dev or t.stride(1) < C_ or (t.shape[0] > 1 and t.stride(0) < 0):
            raise ValueError(f"{what}: {name} must be a float32 [{B * n_patches}, {n_fields}, >= {C_}] tensor with unit inner stride on {dev}, got "
                             f"{(tuple(t.shape), t.dtype, t.stride(), str(t.device)) if torch.is_tensor(t) else type(t).__name__}")
    check_brier_thresholds(thr, n_fields, dev, what)
    if prec_field is not None and (not torch.is_tensor(prec_field) or prec_field.dtype != torch.float32 or tuple(prec_field.shape) != (n_fields,)
                                   or not prec_field.is_contiguous() or prec_field.device != dev):
        raise ValueError(f"{what}: prec_field must be None or a contiguous float32 [{n_fields}] tensor on {dev}")
    if counts is not None and (not torch.is_tensor(counts) or counts.dtype != torch.int32 or counts.dim() != 1 or counts.shape[0] != n_patches
                               or not counts.is_contiguous() or counts.device != dev):
        raise ValueError(f"{what}: counts must be a contiguous int32 [{n_patches}] on {dev}")
    if logw is not None and (not torch.is_tensor(logw) or logw.dtype != torch.float32 or tuple(logw.shape) != (B * n,) or not logw.is_contiguous() or logw.device != dev):
        raise ValueError(f"{what}: logw must be None or a contiguous float32 [{B * n}] tensor on {dev}, got "
                         f"{(tuple(logw.shape), logw.dtype, str(logw.device)) if torch.is_tensor(logw) else type(logw).__name__}")
    T = thr.shape[0]
    fixed = {"sums": ((B, n_fields, T, N.BRIER_SUMS), torch.float64), "hist": ((B, n_fields, T, n + 1), torch.int64), "hits": ((B, n_fields, T, n + 1), torch.int64),
             "status": ((B,), torch.int32)}
    res, ld = _brier_outputs(what, out, maps, accumulate, fixed, lambda ld: (T, B, n_patches, n_fields, ld), C_, groups[0]["H"])
    work = torch.empty(int(N.lib().sea_decode_member_brier_ws_bytes(B, n_patches, n_fields, n, Cp, T)), device=dev, dtype=torch.uint8)
    arr, P = (N.SeaDecodeMseGroup * len(groups))(), N.SeaDecodeMemberBrier()
    fill_decode_member_brier(arr, P, groups, obs, prec_field, prec, counts, logw, thr, n_patches, n, C_, Cp, accumulate, res.get("prob"), res.get("brier"), res["sums"],
                             res["hist"], res["hits"], res["status"], work, ld)
    N.check(N.lib().sea_decode_member_brier(arr, len(groups), C.byref(P), N.dtype_code(dtype), N.stream_ptr()), "sea_decode_member_brier")
    return res


# ------------------------------------------------------------------------------------------------ derived fields (|u|, energy, difference)
def fill_derived_table(arr, derived: Sequence) -> None:
    """The derived-field table of sea_decode_derived_quantiles / sea_decode_derived_brier: arr a (SeaDerivedField * len(derived))(); derived: objects with
    op ("magnitude", "energy", "difference", or the ABI's code), a, b, scale_a, shift_a, scale_b, shift_b (sea_amd.ensemble.DerivedField)."""
    for g, d in zip(arr, derived):
        g.op = N.DERIVED_OPS[d.op] if isinstance(d.op, str) else int(d.op)
        g.a, g.b, g.pad_ = int(d.a), int(d.b), 0
        g.scale_a, g.shift_a, g.scale_b, g.shift_b = float(d.scale_a), float(d.shift_a), float(d.scale_b), float(d.shift_b)


def _check_derived_call(what: str, groups: Sequence[Dict], derived: Sequence, C_: int, Cp: int, n_patches: int, members: int, max_n: int, dtype: torch.dtype):
    """The checks decode_derived_quantiles and decode_derived_brier share — decode_member_quantiles' checks of the groups and sizes, and the derived
    table against the source fields.  Returns (device, M, S, n_fields, B)."""
    if dtype != torch.bfloat16:
        raise ValueError(f"{what}: the fused launch is bf16 only, got {dtype}")
    if not groups or len(groups) > N.DECODE_MSE_MAX_GROUPS:
        raise ValueError(f"{what}: {len(groups)} groups; a launch carries 1 .. {N.DECODE_MSE_MAX_GROUPS}")
    if Cp < 32 or Cp % 32 or not 1 <= C_ <= Cp:
        raise ValueError(f"{what}: need Cp a multiple of 32 and 1 <= C <= Cp, got C = {C_}, Cp = {Cp}")
    dev = groups[0]["H"].device
    M, S = tuple(groups[0]["H"].shape) if groups[0]["H"].dim() == 2 else (0, 0)
    if M < 1 or S < 8 or S % 8 or S > N.DECODE_MSE_MAX_S:
        raise ValueError(f"{what}: H must be [M >= 1, S] with S a multiple of 8 up to {N.DECODE_MSE_MAX_S}, got {tuple(groups[0]['H'].shape)}")
    n = members
    if not isinstance(n, int) or isinstance(n, bool) or n < 1 or n > max_n:
        raise ValueError(f"{what}: members = {members!r} must be an integer in 1 .. {max_n}")
    if n_patches < 1 or M % (n_patches * n):
        raise ValueError(f"{what}: {M} rows are not a multiple of n_patches * members = {n_patches} * {n}")
    n_fields = 0
    for i, d in enumerate(groups):
        for name in ("H", "W2"):
            t = d[name]
            if t.dim() != 2 or t.stride(1) != 1:
                raise ValueError(f"{what} group {i}: {name}: need a 2-D tensor with unit inner stride, got shape {tuple(t.shape)} strides {t.stride()}")
            if t.dtype != dtype or t.device != dev or t.shape[1] != S or (name != "W2" and t.shape[0] != M):
                raise ValueError(f"{what} group {i}: {name} must be a {dtype} [{'n_fields * Cp' if name == 'W2' else M}, {S}] tensor on {dev}, got "
                                 f"{tuple(t.shape)} {t.dtype} on {t.device}")
            if t.stride(0) % 8 or t.data_ptr() % 16:
                raise ValueError(f"{what} group {i}: {name} needs a row stride that is a multiple of 8 and a 16-byte-aligned base (stride {t.stride(0)})")
        W2, b = d["W2"], d["bias"]
        if W2.shape[0] < Cp or W2.shape[0] % Cp:
            raise ValueError(f"{what} group {i}: W2 has {W2.shape[0]} rows, not a multiple of Cp = {Cp}")
        if b.dtype != torch.float32 or b.dim() != 1 or b.shape[0] != W2.shape[0] or not b.is_contiguous() or b.device != dev or b.data_ptr() % 16:
            raise ValueError(f"{what} group {i}: bias must be a contiguous, 16-byte-aligned float32 [{W2.shape[0]}] on {dev}, got {tuple(b.shape)} {b.dtype}")
        n_fields += W2.shape[0] // Cp
    B = M // (n_patches * n)
    if B > 65535:
        raise ValueError(f"{what}: {B} histories; a launch carries up to 65535")
    try:
        n_derived = len(derived)
    except TypeError:
        raise ValueError(f"{what}: derived must be a sequence of derived fields, got {type(derived).__name__}") from None
    if not 1 <= n_derived <= N.DERIVED_MAX:
        raise ValueError(f"{what}: {n_derived} derived fields; a launch carries 1 .. {N.DERIVED_MAX}")
    for i, d in enumerate(derived):
        if isinstance(d.op, str) and d.op not in N.DERIVED_OPS:
            raise ValueError(f"{what}: derived field {i}: op {d.op!r} must be one of {tuple(N.DERIVED_OPS)}")
        if not (0 <= d.a < n_fields and 0 <= d.b < n_fields) or d.a == d.b:
            raise ValueError(f"{what}: derived field {i}: sources a = {d.a}, b = {d.b} must be two different fields in 0 .. {n_fields - 1}")
    return dev, M, S, n_fields, B


def decode_derived_quantiles(groups: Sequence[Dict], derived: Sequence, C_: int, Cp: int, n_patches: int, members: int, levels: Sequence[float] = (),
                             thr: Optional[torch.Tensor] = None, w: Optional[torch.Tensor] = None, counts: Optional[torch.Tensor] = None,
                             out: Optional[Dict[str, torch.Tensor]] = None, dtype: torch.dtype = torch.bfloat16) -> Dict[str, Optional[torch.Tensor]]:
    """sea_decode_derived_quantiles: decode_member_quantiles for DERIVED fields — the magnitude, the energy or the difference of two source fields of one
    decoder group, formed per member in registers (include/sea_hip.h states the definitions); neither the decoded components nor the derived field are
    written.  groups, levels, w, counts, out as decode_member_quantiles; derived: 1 .. 8 sea_amd.ensemble.DerivedField; thr None or f32 [T <= 8, n_derived]
    in the derived fields' own units.  Returns dict(quant=f32 [Q, B, n_patches, n_derived, C] or None, exceed=f32 [T, ...] or None).  The launch refuses
    sources in different groups (RuntimeError, code -3): Decode.member_derived_quantiles composes there."""
    what = "decode_derived_quantiles"
    dev, M, S, n_fields, B = _check_derived_call(what, groups, derived, C_, Cp, n_patches, members, N.QUANTILE_MAX_N, dtype)
    n, nd = members, len(derived)
    levels = check_quantile_levels(levels, what)
    if thr is not None and (not torch.is_tensor(thr) or thr.dtype != torch.float32 or thr.dim() != 2 or not 1 <= thr.shape[0] <= N.QUANTILE_MAX_LEVELS
                            or thr.shape[1] != nd or not thr.is_contiguous() or thr.device != dev):
        raise ValueError(f"{what}: thr must be None or a contiguous float32 [1 .. {N.QUANTILE_MAX_LEVELS}, {nd}] tensor on {dev}, got "
                         f"{(tuple(thr.shape), thr.dtype, str(thr.device)) if torch.is_tensor(thr) else type(thr).__name__}")
    if not levels and thr is None:
        raise ValueError(f"{what}: neither levels nor thresholds: there is nothing to compute")
    if w is not None and (not torch.is_tensor(w) or w.dtype != torch.float32 or tuple(w.shape) != (B * n,) or not w.is_contiguous() or w.device != dev):
        raise ValueError(f"{what}: w must be None or a contiguous float32 [{B * n}] tensor on {dev}, got "
                         f"{(tuple(w.shape), w.dtype, str(w.device)) if torch.is_tensor(w) else type(w).__name__}")
    if counts is not None and (not torch.is_tensor(counts) or counts.dtype != torch.int32 or counts.dim() != 1 or counts.shape[0] != n_patches
                               or not counts.is_contiguous() or counts.device != dev):
        raise ValueError(f"{what}: counts must be a contiguous int32 [{n_patches}] on {dev}")
    n_out = {"quant": len(levels), "exceed": 0 if thr is None else thr.shape[0]}
    out = {} if out is None else out
    if not isinstance(out, dict) or any(k not in n_out or n_out[k] == 0 for k in out):
        raise ValueError(f"{what}: out must be a dict with 'quant' (with levels) and / or 'exceed' (with thresholds)")
    widths = {t.shape[-1] for t in out.values() if torch.is_tensor(t) and t.dim() == 5}
    if len(widths) > 1:
        raise ValueError(f"{what}: the maps in out must share their last dimension, got {sorted(widths)}")
    ld = widths.pop() if widths else C_
    for k, t in out.items():
        shape = (n_out[k], B, n_patches, nd, ld)
        if not torch.is_tensor(t) or tuple(t.shape) != shape or t.dtype != torch.float32 or not t.is_contiguous() or t.device != dev or ld < C_:
            raise ValueError(f"{what}: out[{k!r}] must be a contiguous float32 {list(shape)} tensor on {dev} (last dimension >= {C_})")
    N.require_gpu(groups[0]["H"], f"{what} hidden rows")   # every operand is on their device (checked above)
    res = {k: (out[k] if k in out else torch.empty(n_out[k], B, n_patches, nd, ld, device=dev, dtype=torch.float32)) if n_out[k] else None for k in n_out}
    arr, tab, P = (N.SeaDecodeMseGroup * len(groups))(), (N.SeaDerivedField * nd)(), N.SeaDecodeMemberQuantiles()
    fill_decode_member_quantiles(arr, P, groups, w, counts, thr, levels, res["quant"], res["exceed"], n_patches, n, C_, Cp, ld, B * n_patches * nd * ld)
    fill_derived_table(tab, derived)
    N.check(N.lib().sea_decode_derived_quantiles(arr, len(groups), tab, nd, C.byref(P), N.dtype_code(dtype), N.stream_ptr()), "sea_decode_derived_quantiles")
    return res


def decode_derived_brier(groups: Sequence[Dict], derived: Sequence, obs: torch.Tensor, C_: int, Cp: int, n_patches: int, members: int, thr: torch.Tensor,
                         prec: Optional[torch.Tensor] = None, prec_field: Optional[torch.Tensor] = None, counts: Optional[torch.Tensor] = None,
                         logw: Optional[torch.Tensor] = None, accumulate: bool = False, maps: Sequence[str] = BRIER_MAPS,
                         out: Optional[Dict[str, torch.Tensor]] = None, dtype: torch.dtype = torch.bfloat16) -> Dict[str, torch.Tensor]:
    """sea_decode_derived_brier: decode_member_brier for DERIVED fields (include/sea_hip.h states the definitions).  groups, counts, logw, accumulate, maps,
    out as decode_member_brier; derived: 1 .. 8 sea_amd.ensemble.DerivedField; obs and prec f32 [B * n_patches, n_derived, >= C] readings of the derived
    quantities; prec_field f32 [n_derived]; thr f32 [T <= 8, n_derived] in the derived fields' own units.  Returns decode_member_brier's dict with
    n_derived where that has n_fields."""
    what = "decode_derived_brier"
    dev, M, S, n_fields, B = _check_derived_call(what, groups, derived, C_, Cp, n_patches, members, N.BRIER_MAX_N, dtype)
    n, nd = members, len(derived)
    for name, t in (("obs", obs), ("prec", prec)):
        if t is None and name == "prec":
            continue
        if not torch.is_tensor(t) or t.dtype != torch.float32 or t.dim() != 3 or tuple(t.shape[:2]) != (B * n_patches, nd) or t.shape[2] < C_ or t.stride(2) != 1 \
                or t.device != dev or t.stride(1) < C_ or (t.shape[0] > 1 and t.stride(0) < 0):
            raise ValueError(f"{what}: {name} must be a float32 [{B * n_patches}, {nd}, >= {C_}] tensor with unit inner stride on {dev}, got "
                             f"{(tuple(t.shape), t.dtype, t.stride(), str(t.device)) if torch.is_tensor(t) else type(t).__name__}")
    check_brier_thresholds(thr, nd, dev, what)
    if prec_field is not None and (not torch.is_tensor(prec_field) or prec_field.dtype != torch.float32 or tuple(prec_field.shape) != (nd,)
                                   or not prec_field.is_contiguous() or prec_field.device != dev):
        raise ValueError(f"{what}: prec_field must be None or a contiguous float32 [{nd}] tensor on {dev}")
    if counts is not None and (not torch.is_tensor(counts) or counts.dtype != torch.int32 or counts.dim() != 1 or counts.shape[0] != n_patches
                               or not counts.is_contiguous() or counts.device != dev):
        raise ValueError(f"{what}: counts must be a contiguous int32 [{n_patches}] on {dev}")
    if logw is not None and (not torch.is_tensor(logw) or logw.dtype != torch.float32 or tuple(logw.shape) != (B * n,) or not logw.is_contiguous() or logw.device != dev):
        raise ValueError(f"{what}: logw must be None or a contiguous float32 [{B * n}] tensor on {dev}, got "
                         f"{(tuple(logw.shape), logw.dtype, str(logw.device)) if torch.is_tensor(logw) else type(logw).__name__}")
    T = thr.shape[0]
    fixed = {"sums": ((B, nd, T, N.BRIER_SUMS), torch.float64), "hist": ((B, nd, T, n + 1), torch.int64), "hits": ((B, nd, T, n + 1), torch.int64),
             "status": ((B,), torch.int32)}
    res, ld = _brier_outputs(what, out, maps, accumulate, fixed, lambda ld: (T, B, n_patches, nd, ld), C_, groups[0]["H"])
    work = torch.empty(int(N.lib().sea_decode_member_brier_ws_bytes(B, n_patches, nd, n, Cp, T)), device=dev, dtype=torch.uint8)
    arr, tab, P = (N.SeaDecodeMseGroup * len(groups))(), (N.SeaDerivedField * nd)(), N.SeaDecodeMemberBrier()
    fill_decode_member_brier(arr, P, groups, obs, prec_field, prec, counts, logw, thr, n_patches, n, C_, Cp, accumulate, res.get("prob"), res.get("brier"), res["sums"],
                             res["hist"], res["hits"], res["status"], work, ld)
    P.ld_map = obs.shape[0] * nd * ld   # the maps are sized by the derived fields; n_fields_total stays the number of source fields
    fill_derived_table(tab, derived)
    N.check(N.lib().sea_decode_derived_brier(arr, len(groups), tab, nd, C.byref(P), N.dtype_code(dtype), N.stream_ptr()), "sea_decode_derived_brier")
    return res


def decode_derived_verify(groups: Sequence[Dict], derived: Sequence, obs: torch.Tensor, C_: int, Cp: int, n_patches: int, members: int,
                          prec_field: Optional[torch.Tensor] = None, prec: Optional[torch.Tensor] = None, counts: Optional[torch.Tensor] = None,
                          logw: Optional[torch.Tensor] = None, unbiased: bool = True, accumulate: bool = False, maps: Sequence[str] = FIELD_VERIFY_MAPS,
                          out: Optional[Dict[str, torch.Tensor]] = None, dtype: torch.dtype = torch.bfloat16) -> Dict[str, torch.Tensor]:
    """sea_decode_derived_verify: decode_member_verify for DERIVED fields — CRPS, PIT, rank, mean and spread of the members' derived values at every cell,
    and per (history, derived field) the fp64 sums and the rank histogram (include/sea_hip.h states the definitions); neither the decoded components
    nor the derived field are written.  groups, counts, logw, unbiased, accumulate, maps, out as decode_member_verify; derived: 1 .. 8
    sea_amd.ensemble.DerivedField; obs and prec f32 [B * n_patches, n_derived, >= C] readings of the derived quantities, in their own units; prec_field
    f32 [n_derived].  Returns decode_member_verify's dict with n_derived where that has n_fields.  The launch refuses sources in different groups
    (RuntimeError, code -3): Decode.member_derived_verify composes there.  Everything is checked on the host before the launch."""
    what = "decode_derived_verify"
    dev, M, S, n_fields, B = _check_derived_call(what, groups, derived, C_, Cp, n_patches, members, N.FIELD_VERIFY_MAX_N, dtype)
    n, nd = members, len(derived)
    for name, t in (("obs", obs), ("prec", prec)):
        if t is None and name == "prec":
            continue
        if not torch.is_tensor(t) or t.dtype != torch.float32 or t.dim() != 3 or tuple(t.shape[:2]) != (B * n_patches, nd) or t.shape[2] < C_ or t.stride(2) != 1 \
                or t.device != dev or t.stride(1) < C_ or (t.shape[0] > 1 and t.stride(0) < 0):
            raise ValueError(f"{what}: {name} must be a float32 [{B * n_patches}, {nd}, >= {C_}] tensor with unit inner stride on {dev}, got "
                             f"{(tuple(t.shape), t.dtype, t.stride(), str(t.device)) if torch.is_tensor(t) else type(t).__name__}")
    if prec_field is not None and (not torch.is_tensor(prec_field) or prec_field.dtype != torch.float32 or tuple(prec_field.shape) != (nd,)
                                   or not prec_field.is_contiguous() or prec_field.device != dev):
        raise ValueError(f"{what}: prec_field must be None or a contiguous float32 [{nd}] tensor on {dev}")
    if counts is not None and (not torch.is_tensor(counts) or counts.dtype != torch.int32 or counts.dim() != 1 or counts.shape[0] != n_patches
                               or not counts.is_contiguous() or counts.device != dev):
        raise ValueError(f"{what}: counts must be a contiguous int32 [{n_patches}] on {dev}")
    if logw is not None and (not torch.is_tensor(logw) or logw.dtype != torch.float32 or tuple(logw.shape) != (B * n,) or not logw.is_contiguous() or logw.device != dev):
        raise ValueError(f"{what}: logw must be None or a contiguous float32 [{B * n}] tensor on {dev}, got "
                         f"{(tuple(logw.shape), logw.dtype, str(logw.device)) if torch.is_tensor(logw) else type(logw).__name__}")
    maps = tuple(maps)
    if any(k not in FIELD_VERIFY_MAPS for k in maps) or len(set(maps)) != len(maps):
        raise ValueError(f"{what}: maps must be distinct names among {FIELD_VERIFY_MAPS}, got {maps!r}")
    out = {} if out is None else out
    fixed = {"sums": ((B, nd, N.VERIFY_SUMS), torch.float64), "hist": ((B, nd, n + 1), torch.int64), "status": ((B,), torch.int32)}
    if not isinstance(out, dict) or any(k not in fixed and k not in FIELD_VERIFY_MAPS for k in out):
        raise ValueError(f"{what}: out must be a dict with keys among {FIELD_VERIFY_MAPS + tuple(fixed)}")
    widths = {t.shape[-1] for k, t in out.items() if k in FIELD_VERIFY_MAPS and torch.is_tensor(t) and t.dim() == 4}
    if len(widths) > 1:
        raise ValueError(f"{what}: the maps in out must share their last dimension, got {sorted(widths)}")
    ld_out = widths.pop() if widths else C_
    for k, t in out.items():
        shape, dt = fixed[k] if k in fixed else ((B, n_patches, nd, ld_out), torch.int32 if k == "rank" else torch.float32)
        if not torch.is_tensor(t) or tuple(t.shape) != shape or t.dtype != dt or not t.is_contiguous() or t.device != dev or ld_out < C_:
            raise ValueError(f"{what}: out[{k!r}] must be a contiguous {dt} {list(shape)} tensor on {dev} (maps: last dimension >= {C_})")
    if accumulate and ("sums" not in out or "hist" not in out):
        raise ValueError(f"{what}: accumulate=True adds onto out['sums'] and out['hist']: both are required")
    N.require_gpu(groups[0]["H"], f"{what} hidden rows")   # every operand is on their device (checked above)
    res = {k: out[k] if k in out else torch.empty(fixed[k][0], device=dev, dtype=fixed[k][1]) for k in fixed}
    for k in FIELD_VERIFY_MAPS:
        if k in out:
            res[k] = out[k]
        elif k in maps:
            res[k] = torch.empty(B, n_patches, nd, ld_out, device=dev, dtype=torch.int32 if k == "rank" else torch.float32)
    work = torch.empty(int(N.lib().sea_decode_member_verify_ws_bytes(B, n_patches, nd, n, Cp)), device=dev, dtype=torch.uint8)
    arr, tab, P = (N.SeaDecodeMseGroup * len(groups))(), (N.SeaDerivedField * nd)(), N.SeaDecodeMemberVerify()
    fill_decode_member_verify(arr, P, groups, obs, prec_field, prec, counts, logw, n_patches, n, C_, Cp, unbiased, accumulate, res.get("mean"), res.get("spread"),
                              res.get("crps"), res.get("pit"), res.get("rank"), res["sums"], res["hist"], res["status"], work, ld_out)
    fill_derived_table(tab, derived)   # the maps are sized by the derived fields; n_fields_total stays the number of source fields
    N.check(N.lib().sea_decode_derived_verify(arr, len(groups), tab, nd, C.byref(P), N.dtype_code(dtype), N.stream_ptr()), "sea_decode_derived_verify")
    return res
