/*
 * sea_hip.h — C ABI of libsea_hip.so, the MI355X (gfx950) kernels under the SEA temporal-rollout path.
 *
 * The reference (ParsaEsmati/SEA) has no FFI: its boundary is the Python class surface of
 * models/temporal.py + models/base_blocks.py, whose forward()s dispatch eager ATen ops.  Each entry point
 * below replaces the ATen work of the reference lines it cites; sea_amd/ (the host-side mirror of that class
 * surface) binds them with ctypes.  All paths are relative to the reference repository root.
 *
 * Conventions
 *   - plain pointers and sizes only; every pointer is DEVICE memory owned by the caller; the library never
 *     allocates, frees or retains device memory;
 *   - every call is asynchronous on `stream` (a hipStream_t passed as void*), re-entrant, graph-capturable;
 *   - return 0 on success, a negative SEA_E* code on failure (nothing was launched); the message is available
 *     from sea_last_error() (thread-local); the library never throws and never exits;
 *   - `dtype` selects the ACTIVATION/WEIGHT operand type of the matrix contractions: SEA_F32 uses the exact-f32
 *     MFMA (v_mfma_f32_16x16x4_f32), SEA_BF16 the bf16 MFMA (v_mfma_f32_16x16x32_bf16); accumulation, softmax,
 *     normalisation statistics, residual stream and optimizer state are always fp32;
 *   - "act" tensors have element type `dtype`; "f32" tensors are float.
 */
#ifndef SEA_HIP_H
#define SEA_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SEA_ABI_VERSION 8

enum { SEA_F32 = 0, SEA_BF16 = 1 };

enum {
    SEA_OK = 0,
    SEA_EINVAL = -1,   /* bad argument (null, misaligned, unsupported shape) */
    SEA_ELAUNCH = -2,  /* HIP reported a launch error */
    SEA_EUNSUPPORTED = -3
};

int sea_abi_version(void);
const char* sea_last_error(void);
/* The kernel form the calling thread's last noted launch took, for tests: a static string such as "gemm.tile64" ("" before any noted launch) and
 * two small integers whose meaning depends on the launcher (a / b may be NULL).  Noted by sea_gemm_grouped ("gemm.skinny", "gemm.skinny_long",
 * "gemm.ws", "gemm.256", "gemm.tile64", "gemm.tile128"; a = 1 if the LDS-DMA ring is taken, b = its stages), sea_gemm_rownorm ("gemm_norm.rows16",
 * "gemm_norm.rows16_dma", "gemm_norm.rows64"), sea_attention_fwd ("attn.row"; a = 1 for the wide-head kernel of head dims 64 / 128 / 256, 0 below;
 * "attn.split4", "attn.split2", "attn.split1"; a = 1 if paired), the few-row launches sea_gemm_fewrows ("gemv.gemm") and sea_qkv_rope_fewrows ("gemv.qkv";
 * both: a = MR, the rows of the instantiation — 1, 2 or 4 —, b = KC = K / 512), sea_qkv_rope_grouped ("qkv.skinny", "qkv.tile"), sea_rownorm
 * ("rownorm.fewrows"; a = KM, the 4-column pieces per thread: 1, 4 or 8; "rownorm.ln_rows"; "rownorm.wave"),
 * sea_attention_bwd ("attn_bwd" at head dims 8 / 16 / 32 / 64 / 128 / 256, "attn_bwd.masked" at the other widths; a = the mode bits of the dQ kernel,
 * b = those of the dK / dV kernel: 1 XCD-local order, 2 paired tiles) and sea_wgrad_grouped ("wgrad.tile64", "wgrad.tile128", "wgrad.tile256"; a = the
 * largest split count over the groups, b = 1 if any group takes the plain store), and by the row-owning launches: sea_mlp_fc1_ln_gelu / sea_mlp_fc2_proj_norm /
 * sea_mlp_block ("mlp_fc1.rows32", "mlp_fc2.rows32", "mlp_block.rows32"; a = per_xcd of the XCD-local tile order, 0 in the plain order, b = workgroups launched),
 * sea_gemm_adaln ("gemm_adaln.rows64", "gemm_adaln.rows128"; a = tiles), sea_exchange_tail ("xtail.rows16"; a = row tiles per group, b = segments),
 * sea_row_chain / sea_row_chain_riders ("chain.rows16", "chain.rows32"; a = rider tiles run in this launch, b = information-bottleneck workgroups) and
 * sea_adaln_qkv ("adaln_qkv.rows32", "adaln_qkv.rows32_mod3" with the third layer; a = rider tiles, b = row-rider workgroups), and by the row-walking
 * backward launches: sea_rownorm_bwd ("normbwd.wave"; a = KMAX; "normbwd.wide4", "normbwd.wide8"; a = threads per workgroup; b = workgroups per group),
 * sea_silu_outer_bwd ("silu_bwd.wave"; a = KM, b = workgroups per group; "silu_bwd.cols"; a = column blocks, b = row splits) — both with the suffix ".ws" when
 * the column sums go through the two-stage workspace — and sea_ib_bwd ("ib_bwd.fast"; a = 1 or 4; "ib_bwd.wave"; a = 0; b = workgroups; "ib_bwd.cols"; a = column
 * blocks, b = row splits; "ib_bwd.linear"; a = row chunks).  Host only.  (An addition to ABI version 8; no new struct.) */
const char* sea_last_form(int* a, int* b);
/* sizeof of every ABI struct in declaration order (SeaGemmGroup, SeaQkvGroup, SeaQkvCommon, SeaAttnProblem,
 * SeaAttnParams, SeaNormGroup, SeaSiluGroup, SeaIbParams, ..., SeaLaunchRec, SeaGemmNormGroup, SeaExchangeTail, SeaMlpGroup, SeaMlp2Group, SeaKvNorm, SeaKvField, SeaKvPair, SeaKvLayer, SeaKvGlobal, SeaStepPatch, SeaRowChain, SeaAdalnGroup, SeaAdalnQkv, SeaSplitkGroup, SeaEncBlock, SeaKvFill, SeaKvFork last): lets a binding verify its layout.  Host only. */
int sea_struct_sizes(int* out, int cap);
/* Number of compute units / name of device 0's architecture as HIP reports them (diagnostics for bench.py). */
int sea_device_info(int* cu_count, char* arch, int arch_len);

/* ------------------------------------------------------------------------------------------------------------
 * Grouped GEMM with fused epilogue:  for each group g
 *     acc = sum_{s < n_seg} A_s[M,K] . W[N,K]^T                      (W in nn.Linear layout [out, in])
 *     v   = acc + bias_scale * bias                                    (bias may be NULL)
 *     act = 1 (forward GELU):   Z = (act dtype) v if Z != NULL (pre-activation kept for the backward); v = gelu_erf(v)
 *     act = 2 (backward GELU):  v = v * gelu_erf'(Z)                   (Z = the saved pre-activation, required)
 *     v   = v + R                                                      (R fp32 residual, may be NULL; R == C32 accumulates in place)
 *     C32 = v (fp32, may be NULL);  Cact = (act dtype) v (may be NULL)
 * Replaces nn.Linear / `+` / nn.GELU call sites: attention output projection + residual
 * (models/base_blocks.py:201,293; models/temporal.py:136), cross_down / cross_up (+GELU, + sum over j, + residual;
 * models/temporal.py:177-178,185,189-191), MLP Linear layers (models/base_blocks.py:22,25; models/temporal.py:145),
 * proj (models/temporal.py:146), AdaLN cond_mlp.2 (models/base_blocks.py:339,344).
 * n_seg > 1 sums several A operands against the same W (sum_j cross_up(GELU(a_ij)) = cross_up applied to the
 * sum, done inside the MFMA accumulation): segment s is at A + s * a_seg_stride elements.
 * The same entry point runs the data-gradient GEMMs of the backward pass (dX = dY . W with W^T kept as a shadow copy).
 * Requirements: K % 8 == 0; N % 4 == 0; lda, ldw multiples of 8; ldr, ldc32, ldcact, ldz multiples of 4; all pointers
 * 16-byte aligned.
 */
/* Dropout (training only).  thr = round(256 p) in [0, 255], 0 = off.  Element (row, col) of random stream `stream` is KEPT iff
 * byte (col & 3) of the 32-bit word  mix(seed, stream, row, col >> 2)  is >= thr; kept values are scaled by 256 / (256 - thr)
 * (so the effective rate is thr/256 and the expectation is exact).  The same counter-based definition is evaluated by the
 * forward and the backward kernels, so no mask is ever stored.  (The reference draws torch.nn.Dropout masks — models/base_blocks.py:47,
 * 194, 286 — which cannot be reproduced bit for bit; parity is distributional, checked with sea_dropout_mask.) */
typedef struct {
    uint32_t seed;
    uint32_t stream;
    int32_t thr;
    int32_t mode; /* GEMM epilogue: 1 = on (acc + bias) before the residual, 2 = on the act-dtype output only (backward), 3 = on the complete value (acc + bias + R),
                   * both outputs — the position-encoded rows of exchange_mode 'pool' (dropout(x + pe), models/base_blocks.py:370-372) and their gradient */
} SeaDropout;
/* Writes keep * scale (0 or 256/(256-thr)) for a [rows, cols] element grid of one stream: test / debugging aid. */
int sea_dropout_mask(float* out, int64_t rows, int64_t cols, uint32_t seed, uint32_t stream, int32_t thr, void* stream_handle);

#define SEA_MAX_GROUPS 16
typedef struct {
    const void* A;      /* act [M, K], row stride lda */
    const void* W;      /* act [N, K], row stride ldw */
    const float* bias;  /* f32 [N] or NULL */
    const float* R;     /* f32 [M, N] row stride ldr, or NULL */
    float* C32;         /* f32 [M, N] row stride ldc32, or NULL */
    void* Cact;         /* act [M, N] row stride ldcact, or NULL */
    void* Z;            /* act [M, N] row stride ldz: pre-activation out (act = 1, optional) / in (act = 2) */
    int64_t a_seg_stride;
    int32_t lda, ldw, ldr, ldc32, ldcact, ldz;
    int32_t M, N, K, n_seg;
    int32_t act;        /* 0 none, 1 GELU(erf) forward, 2 multiply by GELU'(Z) */
    float bias_scale;
    SeaDropout drop;    /* element grid = (output row, output column) */
    /* generated A operand (all groups of a launch or none): A[m, k] = silu(silu_w1[k] * silu_c[m] + silu_b1[k]) — AdaLN's cond_mlp.0 + SiLU
     * (models/base_blocks.py:337-338, 344) evaluated inside the GEMM of cond_mlp.2; A is ignored, n_seg = 1, act = 0, K <= 1024 */
    const float* silu_c;   /* f32 [M] or NULL */
    const float* silu_w1;  /* f32 [K] */
    const float* silu_b1;  /* f32 [K] */
} SeaGemmGroup;

int sea_gemm_grouped(const SeaGemmGroup* groups, int n_groups, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Q/K/V projection + bias + rotary embedding, written in the layouts the attention kernel consumes.
 * Replaces models/base_blocks.py:179-188 (self) and :271-280 (cross): three nn.Linear, view to heads,
 * apply_rotary_emb (:314-324) on q and k in fp32, transposes.
 * The virtual output row is [q | k | v] (3 * H*hd columns); a group computes columns [col0, col0 + N) of it from
 * its own A and W (self-attention: one group, col0 = 0, N = 3*H*hd, W = [Wq;Wk;Wv]; cross-attention: a q group
 * from x_i with col0 = 0, N = H*hd and a k,v group from x_j with col0 = H*hd, N = 2*H*hd).
 * Row m of A is (trajectory b = m / T, step t = m % T) at absolute position pos0 + t.
 *   Qout  : act [B, H, T,   hd]   (scaled by q_scale after rotation.  The attention kernels below score in LOG2 units: the caller passes
 *                                  q_scale = hd^-1/2 * log2(e) — reference scale models/base_blocks.py:191 times log2 e — so that
 *                                  softmax(q k^T hd^-1/2) = 2^(Q K^T - max) / sum: one v_exp_f32 per probability)
 *   Kout  : act [B, H, cap, hd]   written at row pos0 + t
 *   Vtout : act [B, H, hd, cap]   written at column pos0 + t  (V transposed: keys contiguous)
 *   Vout  : act [B, H, cap, hd]   optional row-major copy of V (training: the attention backward reads it)
 * rope: f32 [>= pos0 + T, hd/2, 2] (cos, sin) — the reference's freqs_cis buffer viewed as real.
 */
typedef struct {
    const void* A;
    const void* W;
    const float* bias; /* f32 [N] */
    void* Qout;
    void* Kout;
    void* Vtout;
    void* Vout;
    int32_t lda, ldw;
    int32_t M, N, K;
    int32_t col0;
} SeaQkvGroup;

typedef struct {
    const float* rope;
    int32_t H, hd, T, pos0, cap;
    float q_scale;
} SeaQkvCommon;

int sea_qkv_rope_grouped(const SeaQkvGroup* groups, int n_groups, const SeaQkvCommon* common, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Causal flash attention forward, several independent problems (fields / field pairs) per launch.
 * Replaces models/base_blocks.py:191-198 and :283-290: (q k^T) * hd^-1/2 (scale already folded into Q),
 * masked_fill(tril(diagonal=src_len) == 0, -inf), softmax, @ v, merge heads — without materialising [T, T].
 * Scores are taken in LOG2 units: P = 2^(Q K^T - rowmax) / rowsum, i.e. Q must carry hd^-1/2 * log2(e) (SeaQkvCommon.q_scale).
 * Query row i (absolute position q_pos0 + i) attends keys j <= q_pos0 + i + src_len, j < Tk.
 * hd: any multiple of 8 in 8..256 (powers of two run kernels of their own width; any other width a kernel of width round_up(hd, 32) that masks
 * the columns past hd); cap % 8 == 0.  Anything else returns -1 ("unsupported head dim").
 *   O   : act [B, Tq, H*hd] row stride ldo
 *   LSE : f32 [B, H, Tq] BASE-2 log-sum-exp of the scores, log2(sum_j 2^(S_ij)) (for the backward pass), may be NULL
 */
#define SEA_MAX_ATTN_PROBLEMS 8
typedef struct {
    const void* Q;
    const void* K;
    const void* Vt;
    void* O;
    float* LSE;
} SeaAttnProblem;

typedef struct {
    SeaAttnProblem p[SEA_MAX_ATTN_PROBLEMS];
    int32_t n_problems;
    int32_t B, H, hd, Tq, Tk, cap, q_pos0, src_len, ldo;
    SeaDropout drop;    /* on the attention probabilities; element grid = (query, key) of stream (drop.stream + problem) * B*H + b*H + h */
} SeaAttnParams;

int sea_attention_fwd(const SeaAttnParams* params, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Row normalisation with optional adaptive modulation and GELU, several groups per launch:
 *     xhat = (x - mean) / sqrt(var_biased + eps)
 *     y    = xhat * (gamma + (mod ? 1 + mod[:, :d] : 0)) + (beta + (mod ? mod[:, d:] : 0));  y = gelu ? gelu_erf(y) : y
 * Replaces AdaLN.forward's normalisation + modulation (models/base_blocks.py:345-350; `mod` is the cond_mlp
 * output), the custom LayerNorm (models/base_blocks.py:87-88: beta NULL, mod NULL) and nn.LayerNorm + nn.GELU inside
 * MLP (models/base_blocks.py:23-24).
 * x is f32 (x_is_act = 0) or act (x_is_act = 1); y is written as f32 (Y32) and/or act (Yact).
 * mean/rstd (f32 [M]) are saved for the backward pass when non-NULL.
 */
typedef struct {
    const void* X;
    const void* mod;    /* act [M, 2d] row stride ldmod, or NULL */
    const float* gamma; /* f32 [d] */
    const float* beta;  /* f32 [d] or NULL */
    float* Y32;
    void* Yact;
    float* mean;
    float* rstd;
    int32_t ldx, ldmod, ldy32, ldyact;
    /* optional addend (x f32, d <= 2048): x' = x + addend is what gets normalised; Xout <- x' when non-NULL (may be X itself) — the
     * info-bottleneck add of models/temporal.py:140-142 folded into the AdaLN_2 pass that follows it */
    const float* addend;  /* f32 [M, d] row stride ldadd, or NULL */
    float* Xout;          /* f32 [M, d] row stride ldxout, or NULL */
    int32_t ldadd, ldxout;
} SeaNormGroup;

int sea_rownorm(const SeaNormGroup* groups, int n_groups, int M, int d, int x_is_act, int gelu, float eps,
                int dtype, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * The Linear layers of a KV-cache rollout STEP (utils/train_utils.py:202-209 with per-layer K/V caches: one row per trajectory and field) at the shipped
 * widths (configs/cylinder_flow.py embed_dim 1024, configs/multiphase_flow.py 2048), where a step's time is its launch count:
 * sea_gemm_grouped / sea_qkv_rope_grouped for M <= 4 rows per group with the row norm in front of the layer folded into the launch.
 *   groups  as sea_gemm_grouped (n_seg = 1, act 0 / 1, no dropout, no generated operand) / sea_qkv_rope_grouped; bf16; every group of a launch has the
 *           same K, one of 512, 1024, 2048 (4096, 8192, 16384 too for sea_gemm_fewrows); n_groups <= 8
 *   pre     NULL, or [n_groups]: pre[g].X != NULL makes the A operand of group g  sea_rownorm(pre[g])  of fp32 rows [M, K] (gamma, beta, mod, addend as
 *           SeaNormGroup; K <= 2048), evaluated by every workgroup for itself — groups[g].A is ignored.  Xout (x + addend, fp32) is written once and must
 *           NOT alias X; Y32 / Yact / mean / rstd must be NULL.  (LayerNorm / AdaLN in front of q/k/v, cross-attention and the MLP: models/temporal.py:126-131,
 *           139-145, 170-186; models/base_blocks.py:345-350.)
 *           sea_gemm_fewrows, pre_x_is_act = 1: pre[g].X are rows in the activation dtype instead and the prologue is sea_rownorm(x_is_act, pre_gelu) with
 *           gamma / beta only — nn.LayerNorm + GELU of the hidden rows in front of MLP.layers.3 (models/base_blocks.py:23-25); K <= 8192.
 * Arithmetic: products of bf16 operands accumulated in fp32 (v_dot2c_f32_bf16), norms in fp32 two-pass form exactly as sea_rownorm. */
int sea_gemm_fewrows(const SeaGemmGroup* groups, const SeaNormGroup* pre, int n_groups, int pre_x_is_act, int pre_gelu, float eps, int dtype, void* stream);
int sea_qkv_rope_fewrows(const SeaQkvGroup* groups, const SeaNormGroup* pre, int n_groups, const SeaQkvCommon* common, float eps, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Linear layer whose output rows are normalised in the same launch (a workgroup tile spans the whole output row, N <= 256):
 *     v    = sum_s A_s[M,K] . W[N,K]^T + bias_scale * bias (+ R)       (as sea_gemm_grouped);  Cact <- (act dtype) v when non-NULL
 *     v    = v + ib(c)  when ib_c != NULL (info-bottleneck addend of sea_ib_add, no dropout);  C32 <- v when non-NULL
 *     y    = LayerNorm_N(v) with gamma / beta / mod exactly as SeaNormGroup (two-pass fp32 statistics, biased variance, eps)
 *     Yact <- (act dtype) y ;  Y32 <- y ;  mean / rstd saved when non-NULL
 * Replaces the pairs cross_down[i] + ln_cross[i] (models/temporal.py:177-181), proj[i] + the model's final per-field norm
 * (models/temporal.py:146, 412-415), and the triple cross_up[i] (+ sum over j, + residual) / _add_info / ln.exp[i][2]
 * (models/temporal.py:178,189-191 / 140-142 / 145) — one launch and one HBM round trip of the [M, N] intermediate less than
 * sea_gemm_grouped followed by sea_rownorm, with identical arithmetic.
 * Requirements: N % 16 == 0, N <= 256; K % 8 == 0; lda, ldw multiples of 8; ldr, ldc32, ldy32, ldyact, ldmod multiples of 4;
 * all pointers 16-byte aligned.
 */
#define SEA_MAX_GEMM_NORM_GROUPS 8
typedef struct {
    const void* A;      /* act [M, K], row stride lda */
    const void* W;      /* act [N, K], row stride ldw */
    const float* bias;  /* f32 [N] or NULL */
    const float* R;     /* f32 [M, N] row stride ldr, or NULL */
    float* C32;         /* f32 [M, N] pre-normalisation output, row stride ldc32, or NULL */
    const void* mod;    /* act [M, 2N] row stride ldmod, or NULL */
    const float* gamma; /* f32 [N] */
    const float* beta;  /* f32 [N] or NULL */
    float* Y32;         /* f32 [M, N] row stride ldy32, or NULL */
    void* Yact;         /* act [M, N] row stride ldyact, or NULL */
    float* mean;        /* f32 [M] or NULL */
    float* rstd;        /* f32 [M] or NULL */
    int32_t lda, ldw, ldr, ldc32, ldmod, ldy32, ldyact;
    int32_t M, N, K;
    /* extensions (all-zero = off, except n_seg >= 1 and bias_scale): */
    int32_t n_seg;          /* sum of n_seg A operands against the same W, segment s at A + s * a_seg_stride (as SeaGemmGroup) */
    int64_t a_seg_stride;
    float bias_scale;
    int32_t ldcact;
    void* Cact;             /* act [M, N]: v BEFORE the info-bottleneck addend (the copy cross_down reads), or NULL */
    const float* ib_c;      /* f32 [M] condition: non-NULL adds ib = W2 . gelu(LN_h(w1 c + b1)) + b2 (SeaIbParams) to v before C32 and the norm */
    const float* ib_w1;
    const float* ib_b1;
    const float* ib_lnw;
    const float* ib_lnb;
    const float* ib_w2;     /* f32 [N, h] */
    const float* ib_b2;     /* f32 [N] */
    int32_t ib_h;           /* 4 or 8 */
    int32_t pad_;
} SeaGemmNormGroup;

int sea_gemm_rownorm(const SeaGemmNormGroup* groups, int n_groups, float eps, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Tail of one field's state-exchange stage in ONE launch (bf16 compute; a workgroup owns 16 rows through all three Linear layers):
 *     g_s   = gelu_erf(att_s[M,D] . Wp_s[D,D]^T)                      s < n_seg      (cross_attn[i][j].projection + GELU, models/temporal.py:183,185)
 *     x     = X + sum_s g_s . Wup[E,D]^T + bias_scale * bup            X updated in place; Xact <- (act dtype) x when non-NULL
 *                                                                      (cross_up[i], the sum over j and the residual, models/temporal.py:185,189-191)
 *     y     = LayerNorm_D(x . Wdown[D,E]^T + bdown) with gamma / beta / mod as SeaNormGroup;  down.Yact / down.Y32 <- y      when has_down
 *                                                                      (cross_down[i] + ln_cross[i] of the UPDATED field: what later fields attend to)
 * The weights of the middle layer go L2 -> LDS in one global_load_lds burst while the first layer runs from registers; the intermediates
 * (g, the new x) never leave the CU.  Replaces three launches (sea_gemm_grouped x 2, sea_gemm_rownorm) on the serial Gauss-Seidel chain.
 * `down`: W, ldw, bias, gamma, beta, mod, ldmod, Yact / Y32 (+ strides), mean, rstd are read; its A, M, N, K and extensions are ignored.
 * Requirements: dtype SEA_BF16; (D, E) in {(128, 256), (64, 128)}; n_seg * D <= 256; all row strides multiples of 8 (act) / 4 (f32);
 * pointers 16-byte aligned.  Returns SEA_EUNSUPPORTED for other shapes / dtypes (callers keep the three-launch form).
 */
#define SEA_XTAIL_MAX_SEG 4
typedef struct {
    const void* att[SEA_XTAIL_MAX_SEG];   /* act [M, D], row stride ldatt */
    const void* Wp[SEA_XTAIL_MAX_SEG];    /* act [D, D], row stride ldwp */
    const void* Wup;                      /* act [E, D], row stride ldwup */
    const float* bup;                     /* f32 [E] or NULL */
    float* X;                             /* f32 [M, E], row stride ldx: residual stream, updated in place */
    void* Xact;                           /* act [M, E], row stride ldxact, or NULL */
    int32_t n_seg, ldatt, ldwp, ldwup, ldx, ldxact;
    int32_t M, D, E, has_down;
    float bias_scale;
    SeaGemmNormGroup down;
} SeaExchangeTail;

/* params: n_groups <= SEA_XTAIL_MAX_GROUPS problems of one shape and mode (e.g. the F fields), one grid row each */
#define SEA_XTAIL_MAX_GROUPS 4
int sea_exchange_tail(const SeaExchangeTail* params, int n_groups, float eps, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * First half of the field MLP in one launch (bf16):  Hg = gelu_erf(LayerNorm_S(A[M,E] . W1[S,E]^T + b1) * lnw + lnb)
 * Replaces models/base_blocks.py:22-24 (Linear(E, S), nn.LayerNorm(S), GELU) = sea_gemm_grouped + sea_rownorm(gelu): a workgroup owns 32 complete
 * rows of the hidden matrix, the pre-activation matrix never reaches HBM.  (E, S) in {(256, 2048), (128, 1024)}; row strides multiples of 8;
 * pointers 16-byte aligned.  Returns SEA_EUNSUPPORTED for other shapes / dtypes (callers keep the two-launch form).
 */
#define SEA_MAX_MLP_GROUPS 8
typedef struct {
    const void* A;      /* act [M, E], row stride lda */
    const void* W1;     /* act [S, E], row stride ldw */
    const float* b1;    /* f32 [S] */
    const float* lnw;   /* f32 [S] */
    const float* lnb;   /* f32 [S] */
    void* Hg;           /* act [M, S], row stride ldh */
    int32_t lda, ldw, ldh;
    int32_t M, E, S;
    /* Optional prologue (X32 != NULL; A is then ignored): the operand rows are produced inside the launch from the fp32 residual stream —
     *     x = X32 (+ addend);  Xout <- x when non-NULL (may be X32);  A row = (x - mean) * rstd * (gamma [+ 1 + mod[0:E]]) + (beta [+ mod[E:2E]])
     * i.e. the info-bottleneck add and AdaLN_2 / LayerNorm in front of the MLP (models/temporal.py:139-145; SeaNormGroup's semantics, two-pass fp32
     * statistics): one launch less on the chain, the normalised rows never reach HBM. */
    const float* X32;    /* f32 [M, E], row stride ldx32 */
    const float* addend; /* f32 [M, E], row stride ldadd, or NULL */
    float* Xout;         /* f32 [M, E], row stride ldxout, or NULL */
    const void* mod;     /* act [M, 2E] (scale | shift), row stride ldmod, or NULL */
    const float* gamma;  /* f32 [E] */
    const float* beta;   /* f32 [E] or NULL */
    int32_t ldx32, ldadd, ldxout, ldmod;
    float norm_eps;
    int32_t pad_;
} SeaMlpGroup;

int sea_mlp_fc1_ln_gelu(const SeaMlpGroup* groups, int n_groups, float eps, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Second half of the field MLP, proj and the final norm in one launch (bf16; a workgroup owns 32 complete rows through both Linear layers):
 *     x3  = Hg[M,S] . W2[E,S]^T + b2 + R            (models/base_blocks.py:25; the residual of models/temporal.py:145)
 *     y   = x3 . Wproj[E,E]^T + bproj               (models/temporal.py:146)
 *     out = norm(y) with gamma / beta / mod as SeaNormGroup when gamma != NULL (the model's final per-field norm, models/temporal.py:412-415), else y
 * Replaces sea_gemm_grouped x 2 + sea_rownorm on the tail of the layer; x3 and y never reach HBM.  Same shapes and requirements as sea_mlp_fc1_ln_gelu.
 */
typedef struct {
    const void* Hg;      /* act [M, S], row stride ldh: the activated hidden rows */
    const void* W2;      /* act [E, S], row stride ldw2 */
    const float* b2;     /* f32 [E] */
    const float* R;      /* f32 [M, E], row stride ldr: the residual stream */
    const void* Wproj;   /* act [E, E], row stride ldwp */
    const float* bproj;  /* f32 [E] */
    const float* gamma;  /* f32 [E] or NULL (no norm) */
    const float* beta;   /* f32 [E] or NULL */
    const void* mod;     /* act [M, 2E] (scale | shift), row stride ldmod, or NULL */
    float* Y32;          /* f32 [M, E], row stride ldy32, or NULL */
    void* Yact;          /* act [M, E], row stride ldyact, or NULL */
    int32_t ldh, ldw2, ldr, ldwp, ldmod, ldy32, ldyact;
    int32_t M, E, S;
} SeaMlp2Group;

int sea_mlp_fc2_proj_norm(const SeaMlp2Group* groups, int n_groups, float eps, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * The whole field MLP, proj and the final norm in ONE launch (bf16): sea_mlp_fc1_ln_gelu(g1[i]) followed by sea_mlp_fc2_proj_norm(g2[i]) for every group i,
 * with the activated hidden rows kept in the owning workgroup's registers (models/base_blocks.py:22-25, models/temporal.py:139-146, 412-415): g1[i].Hg and
 * g2[i].Hg are ignored (may be NULL), g1[i].Xout must be NULL, and g2[i].R may be NULL when g1[i] carries the norm prologue — the residual is then
 * X32 (+ addend), formed by the same fp32 add as the prologue's.  g2[i].Y32 / Yact may alias g1[i].X32 (a workgroup writes its rows after its last read of
 * them).  Same shapes and requirements as the two entry points; g1[i].M == g2[i].M.  Returns SEA_EUNSUPPORTED for other shapes / dtypes.
 */
int sea_mlp_block(const SeaMlpGroup* g1, const SeaMlp2Group* g2, int n_groups, float eps, int dtype, void* stream);


/* ------------------------------------------------------------------------------------------------------------
 * Hidden layer of the AdaLN condition MLP for a scalar condition: Hid[m, k] = silu(w1[k] * c[m] + b1[k]).
 * Replaces cond_mlp.0 (Linear(1, 2d)) + nn.SiLU (models/base_blocks.py:337-338, 344); cond_mlp.2 is a
 * sea_gemm_grouped group.  c: f32 [M]; w1, b1: f32 [K2]; Hid: act [M, K2] row stride ld.
 */
typedef struct {
    const float* w1;
    const float* b1;
    void* Hid;
    int32_t K2, ld;
} SeaSiluGroup;

int sea_silu_outer(const SeaSiluGroup* groups, int n_groups, const float* c, int M, int dtype, void* stream);
/* The same launch with up to SEA_MAX_SILU_IB extra row passes that EVALUATE the information-bottleneck MLP of a block (SeaIbParams below;
 * both depend on the condition only): ibs[k].X[0][m, :] = W2 . gelu(LN_h(w1 c[m] + b1)) + b2 is STORED (f32 [M, E], row stride ldx;
 * n_fields, c and drop of ibs[k] are ignored).  A later sea_rownorm adds it through SeaNormGroup.addend: no launch of its own for the add. */
#define SEA_MAX_SILU_IB 4
struct SeaIbParams_;
int sea_silu_outer_ib(const SeaSiluGroup* groups, int n_groups, const float* c, int M, int dtype, const struct SeaIbParams_* ibs, int n_ib, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Information-bottleneck add: ib = W2 . gelu(LN_h(w1 * c + b1)) + b2, then X_f += ib for every field f.
 * Replaces BaseBlockTemporal._add_info with ib_scale_mode='mlp', ib_addition_mode='add'
 * (models/temporal.py:111-116,140-142) = MLP(1 -> h -> E) of models/base_blocks.py:22-26 with h = scale_ratio.
 * X: n_fields f32 [M, E] matrices (row stride ldx); all parameters f32; h <= 64.
 */
typedef struct SeaIbParams_ {
    float* X[8];
    int32_t n_fields, ldx;
    const float* c;   /* [M] */
    const float* w1;  /* [h] (Linear(1,h).weight) */
    const float* b1;  /* [h] */
    const float* lnw; /* [h] */
    const float* lnb; /* [h] */
    const float* w2;  /* [E, h] */
    const float* b2;  /* [E] */
    int32_t M, E, h;
    SeaDropout drop;  /* on the MLP output, an independent stream (drop.stream + field) per field; element grid = (row, column) */
    int32_t mode;     /* which ib layer (models/temporal.py:103-109): 0 = 'mlp' (the fields above); 1 = 'linear': ib = w1[E] * c + b1[E] (nn.Linear(1, E));
                       * 2 = 'fourier': ib = [sin(2 pi c W), cos(2 pi c W)] with w1 = W[E/2] (GaussianFourierProjection, models/base_blocks.py:143-151).
                       * Modes 1 and 2 read only c, w1 (and b1), ignore h / lnw / lnb / w2 / b2 and take no dropout. */
    int32_t pad_;
} SeaIbParams;

int sea_ib_add(const SeaIbParams* params, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Strided 2-D conversions between fp32 and the activation dtype (weights shadow copy, model input split).
 * dst[r, c] = (dst type) src[r, c] for r < rows, c < cols (cols % 4 == 0).
 */
int sea_convert_f32_to_act(const float* src, int64_t lds, void* dst, int64_t ldd, int64_t rows, int64_t cols, int dtype,
                           void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Mean-squared-error loss and its gradient in one pass: loss[0] = mean((out - tgt)^2),
 * dout = 2 * grad_scale / n * (out - tgt) (dout may be NULL for evaluation).  Replaces nn.MSELoss forward + backward
 * (train/train_temporal.py:221,256-257).  `partial` is an f32 workspace of n_partial_cap >= 1 elements (<= 1024 used); the
 * reduction order is fixed, so the loss is bitwise reproducible.  Any n >= 1; pointers 4-byte aligned (16-byte-aligned ones take the
 * float4 path, with the n % 4 tail handled apart).
 */
int sea_mse_fwd_bwd(const float* out, const float* tgt, float* dout, float* loss, float* partial, int n_partial_cap,
                    int64_t n, float grad_scale, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * relativeMSE (utils/train_utils.py:112-116) over the last dimension:
 * y[row] = sum_d (pred - truth)^2 / (sum_d truth^2 + 1e-8), rows = product of the leading dimensions, any d >= 1; pointers 4-byte
 * aligned (d % 4 == 0 with 16-byte-aligned pointers takes the 16-byte-load path).
 */
int sea_relative_mse(const float* pred, const float* truth, float* y, int64_t rows, int d, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * One AdamW step over a flat fp32 parameter buffer (torch.optim.AdamW as configured by initialize_optimizer,
 * utils/train_utils.py:33-34: decoupled weight decay, bias-corrected moments; `step` counts from 1):
 *     g' = grad_scale * g;  p -= (lr*wd) p;  m = b1 m + (1-b1) g';  v = b2 v + (1-b2) g'^2;
 *     p -= lr/(1-b1^step) * m / (sqrt(v)/sqrt(1-b2^step) + eps)
 * and, in the same pass, the refreshed shadow of the parameters in shadow_dtype (SEA_BF16: rounded to nearest even; SEA_F32: a copy;
 * shadow may be NULL).
 * grad_scale = 1/world_size folds the data-parallel mean into the step.  n % 4 == 0.
 */
int sea_adamw_flat(float* p, const float* g, float* m, float* v, void* shadow, int shadow_dtype, int64_t n, float lr, float beta1,
                   float beta2, float eps, float weight_decay, int step, float grad_scale, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Gradient clipping by global norm and skipping of non-finite steps, decided on the device: what
 * torch.nn.utils.clip_grad_norm_ + a host-side isfinite() test do with hundreds of ATen launches and a sync, as two
 * short launches in front of the AdamW launch and no sync.  The two entry points are a PAIR: one sea_grad_norm_ctl per
 * sea_adamw_flat_ctl, on the same stream, over the same g, n and grad_scale (the first counts the step the second applies).
 *
 * The step control block `ctl`: eight 32-bit words of device memory, 16-byte aligned, owned by the caller, zeroed (or
 * word SEA_CTL_STEP set to the steps already taken) before the first call and carried from step to step:
 */
enum {
    SEA_CTL_GRAD_NORM = 0,     /* f32  2-norm of grad_scale * g, the mean gradient AdamW consumes */
    SEA_CTL_CLIP = 1,          /* f32  factor applied on top of grad_scale (0 on a skipped step) */
    SEA_CTL_INV_BC1 = 2,       /* f32  1 / (1 - beta1^step) */
    SEA_CTL_INV_SQRT_BC2 = 3,  /* f32  1 / sqrt(1 - beta2^step) */
    SEA_CTL_APPLIED = 4,       /* i32  1: this step updates the parameters; 0: it is skipped */
    SEA_CTL_STEP = 5,          /* i32  number of applied steps, this one included when applied */
    SEA_CTL_SKIPPED = 6,       /* i32  running count of skipped steps */
    SEA_CTL_CLIPPED = 7,       /* i32  running count of applied steps with clip < 1 */
    SEA_CTL_WORDS = 8
};

/* total = sum g^2, every square and sum in fp64 (elements of 1e25 or 1e-30 neither overflow nor vanish, and the total is
 * non-finite exactly when an element is), in a fixed order: partial[b] per workgroup (at most min(1024, n_partial_cap) of
 * them), then one workgroup whose first thread, in fp64, writes the control block:
 *     norm = |grad_scale| sqrt(total);  grad_norm = (float)norm;  finite = isfinite(grad_norm)
 *     !finite && skip_nonfinite:  applied = 0, clip = 0, skipped += 1; step and the two bias corrections keep their values
 *     otherwise:  applied = 1, step += 1, inv_bc1 / inv_sqrt_bc2 from the new step,
 *                 clip = (max_norm > 0 && finite) ? min(1, max_norm / (norm + 1e-6)) : 1   (clip_grad_norm_'s formula),
 *                 clipped += 1 when the stored fp32 clip < 1
 * so with skip_nonfinite = 0 a non-finite norm is applied with clip = 1, as sea_adamw_flat would.  max_norm <= 0: no clipping
 * (NaN is refused).  n % 4 == 0, n >= 4; g and ctl 16-byte aligned, partial 8-byte aligned; 0 <= beta < 1.
 * g is read only; nothing but partial[0 .. min(workgroups, n_partial_cap)) and the eight control words is written. */
int sea_grad_norm_ctl(const float* g, int64_t n, float grad_scale, float max_norm, int skip_nonfinite, float beta1, float beta2,
                      double* partial, int n_partial_cap, int32_t* ctl, void* stream);

/* sea_adamw_flat with g' = (grad_scale * clip) * g and the bias corrections read from the control block instead of computed
 * from a host-side step number.  ctl[SEA_CTL_APPLIED] == 0: every workgroup returns before its first load; p, m, v and the
 * shadow stay bitwise what they were.  g is not scaled in place: after the step it still holds the unclipped gradients.
 * Constraints of sea_adamw_flat, and ctl 16-byte aligned. */
int sea_adamw_flat_ctl(float* p, const float* g, float* m, float* v, void* shadow, int shadow_dtype, int64_t n, float lr, float beta1,
                       float beta2, float eps, float weight_decay, float grad_scale, const int32_t* ctl, void* stream);

/* ============================================================================================================
 * Backward pass.  The reference gets it from autograd (loss.backward(), train/train_temporal.py:257); here every
 * operator has a hand-written backward.  Data gradients of the Linear layers reuse sea_gemm_grouped with the W^T shadow
 * (sea_transpose_weights); parameter gradients are ACCUMULATED (fp32 atomics) into buffers the caller zeroes each step.
 * ============================================================================================================ */

/* Weight gradient of y = x W^T + b for several layers per launch: dW[N,K] += dY[M,N]^T . X[M,K]; db[N] += sum_m dY[m,:]
 * (db may be NULL).  The contraction over M is split across workgroups (unless M is short).  N % 8 == 0, K % 8 == 0.  At most 32 groups per call (weight gradients
 * have no consumers inside the backward: a caller may collect the small ones of a layer and run them as one call). */
typedef struct {
    const void* dY; /* act [M, N] row stride lddy */
    const void* X;  /* act [M, K] row stride ldx */
    float* dW;      /* f32 [N, K] row stride lddw, accumulated */
    float* db;      /* f32 [N] accumulated, or NULL */
    int32_t lddy, ldx, lddw;
    int32_t M, N, K;
    int32_t overwrite;   /* non-zero: dW holds zeros and this launch is its only contribution in the step — the kernel may STORE instead of adding
                          * (taken when the contraction is not split across workgroups; db is always accumulated) */
    int32_t pad_;
} SeaWgradGroup;
int sea_wgrad_grouped(const SeaWgradGroup* groups, int n_groups, int dtype, void* stream);

/* Activation-dtype TRANSPOSED shadow of weight matrices: for each descriptor {src_off, dst_off, rows, cols} (int64 x 4, in
 * elements, DEVICE memory) dst[dst_off + c*rows + r] = src[src_off + r*cols + c].  tile_start (int32 [n_desc+1], DEVICE) is the
 * prefix sum of ceil(rows/32)*ceil(cols/32). */
int sea_transpose_weights(const float* src, void* dst, int dst_dtype, const int64_t* desc, const int32_t* tile_start, int n_desc,
                          int total_tiles, void* stream);

/* Backward of sea_rownorm.  Given dY, the forward input X, the saved mean/rstd and the modulation:
 *   dX   = rstd * (dxhat - mean_d(dxhat) - xhat * mean_d(dxhat * xhat)),  dxhat = dY' * (gamma (+ 1 + mod_w)),
 *          dY' = dY * gelu'(y_pre) when gelu (beta is needed only then); written to dX32 (added to it when accumulate) and/or dXact;
 *   dmod = [dY' * xhat | dY'] (act, optional);  dgamma += sum_m dY' * xhat;  dbeta += sum_m dY' (dbeta may be NULL). */
typedef struct {
    const void* dY;     /* f32 or act [M, d] */
    const void* X;      /* f32 or act [M, d] */
    const void* mod;    /* act [M, 2d] or NULL */
    const float* gamma; /* [d] */
    const float* beta;  /* [d] or NULL */
    const float* mean;  /* [M] */
    const float* rstd;  /* [M] */
    float* dX32;
    void* dXact;
    void* dmod;
    float* dgamma;
    float* dbeta;
    int32_t lddy, ldx, ldmod, lddx32, lddxact, lddmod;
} SeaNormBwdGroup;
/* ws (optional, f32, >= n_groups * min(ceil(M/4), 512) * 2 * d floats): when given, the column sums are written as per-workgroup
 * partials and reduced by a second small launch instead of hundreds of workgroups atomically adding to the same addresses. */
int sea_rownorm_bwd(const SeaNormBwdGroup* groups, int n_groups, int M, int d, int dy_is_act, int x_is_act, int gelu,
                    int accumulate, int dtype, float* ws, int64_t ws_floats, void* stream);

/* Backward of sea_attention_fwd + the rotary embedding of sea_qkv_rope_grouped (flash-style: P is recomputed from Q, K and the
 * forward's LSE).  For each problem, from dO (gradient of the attention output, [B, Tq, H*hd] row stride lddo):
 * hd: the forward's set, any multiple of 8 in 8..256.
 *   dQ [B*Tq, H*hd] (row stride lddq), dK, dV [B*Tk, H*hd] (lddk, lddv) = gradients with respect to the OUTPUTS of the q / k / v
 *   Linear layers (RoPE and the q scale are undone in the epilogue), i.e. the dY operands of sea_wgrad_grouped / the dgrad GEMM.
 * V is the row-major copy written by sea_qkv_rope_grouped (Vout); delta (f32 [B, H, Tq]) is workspace.  Deterministic.
 * Q, LSE and q_scale are the forward's: Q in log2 units (q_scale = hd^-1/2 * log2 e is the factor sea_qkv_rope_grouped put on q), LSE base 2; the
 * kernels carry the ln 2 of d(2^s)/ds themselves. */
typedef struct {
    const void* Q;   /* act [B, H, Tq, hd]  (rotated, scaled) */
    const void* K;   /* act [B, H, cap, hd] (rotated) */
    const void* V;   /* act [B, H, cap, hd] */
    const void* O;   /* act [B, Tq, H*hd] row stride ldo */
    const void* dO;  /* act [B, Tq, H*hd] row stride lddo */
    const float* LSE;
    float* delta;
    void* dQ;
    void* dK;
    void* dV;
} SeaAttnBwdProblem;

typedef struct {
    SeaAttnBwdProblem p[SEA_MAX_ATTN_PROBLEMS];
    const float* rope; /* f32 [>= max(q_pos0 + Tq, Tk), hd/2, 2] */
    int32_t n_problems;
    int32_t B, H, hd, Tq, Tk, cap, q_pos0, src_len;
    int32_t ldo, lddo, lddq, lddk, lddv;
    float q_scale;
    SeaDropout drop;   /* must equal the forward's */
} SeaAttnBwdParams;
int sea_attention_bwd(const SeaAttnBwdParams* params, int dtype, void* stream);

/* Backward of sea_silu_outer: dpre = dHid * silu'(w1 c + b1); dw1[k] += sum_m dpre * c[m]; db1[k] += sum_m dpre. */
typedef struct {
    const void* dHid; /* act [M, K2] row stride ld */
    const float* w1;
    const float* b1;
    float* dw1;
    float* db1;
    int32_t K2, ld;
} SeaSiluBwdGroup;
int sea_silu_outer_bwd(const SeaSiluBwdGroup* groups, int n_groups, const float* c, int M, int dtype, float* ws, int64_t ws_floats,
                       void* stream);  /* ws: as for sea_rownorm_bwd, >= n_groups * min(ceil(M/4), 256) * 2 * max K2 floats */

/* Parameter gradients of the information-bottleneck MLP (sea_ib_add) from dib = sum_f dX_f; dX itself passes through. */
typedef struct {
    const float* dX[8];
    int32_t n_fields, ldx;
    const float* c;
    const float* w1;
    const float* b1;
    const float* lnw;
    const float* lnb;
    const float* w2;
    float* dw1;
    float* db1;
    float* dlnw;
    float* dlnb;
    float* dw2;
    float* db2;
    int32_t M, E, h;
    SeaDropout drop;
    int32_t mode;   /* 0: the MLP form above; 1: ib = nn.Linear(1, E) (ib_scale_mode 'linear', models/temporal.py:106-107): dw1 [E] += sum_m c[m] sum_f dX_f[m, :],
                     * db1 [E] += sum_m sum_f dX_f[m, :]; the other pointers are ignored */
    int32_t pad_;
    /* workspaces of the column-block form (mode 0, h <= 8; both optional — without them the one-wave-per-row kernel runs):
     *   ws   f32 [>= rs * E * (1 + h)]   per-row-split partial sums of db2 | dW2, rs = ws_floats / (E * (1 + h)) row splits at most
     *   dhid f32 [M, 8]                   d(loss)/d(hidden) per row; must be ZERO on entry when E > 256 (column blocks add into it) and is left zero */
    float* ws;
    int64_t ws_floats;
    float* dhid;
} SeaIbBwdParams;
int sea_ib_bwd(const SeaIbBwdParams* params, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Condition gradients (the gradient of the loss with respect to the per-row condition c [M], fp32).  Both ADD into dc; neither uses a float atomic
 * on dc: per-workgroup partials and a fixed-order finish (AdaLN), one wave per row with a fixed-order wave sum (information bottleneck), so dc is
 * bitwise repeatable whenever its operands are.  (Of the operands a training plan passes in, dhid of sea_ib_bwd's column-block form is accumulated
 * atomically when E > 256 — it feeds the PARAMETER gradients only; sea_ib_bwd_dc recomputes d hidden itself.)
 *
 * sea_silu_outer_bwd_dc: sea_silu_outer_bwd (the same dw1 / db1) plus dc[m] += sum_groups sum_j dpre[m, j] w1[j], from the same single read of dHid.
 *   ws: >= sea_silu_outer_bwd_dc_ws_floats(groups, n_groups, M) floats = ncb * M (dc partials, ncb = sum_groups ceil(K2 / 256)) + n_groups * 2 * max K2
 *   (column-sum partials of one row split; more row splits run when more is given).  Limits as sea_silu_outer_bwd: K2 <= 2048, SEA_MAX_SILU_BWD_GROUPS.
 * sea_ib_bwd_dc: dc[m] += d(loss)/d(c[m]) through the layer of params->mode, from dib = sum_f dX_f (mode 0: with the forward's dropout masks):
 *   mode 0 'mlp' (h <= 64): back through W2, GELU and LN_h, dc += sum_k dpre[m, k] w1[k];  mode 1 'linear': dc += sum_e w1[e] dib[m, e];
 *   mode 2 'fourier': dc += 2 pi sum_e W[e] (cos theta_e dib[m, e] - sin theta_e dib[m, E/2 + e]), theta_e = 2 pi c W[e] in fp32 as the forward forms it.
 *   With params->dw1 set (modes 0 / 1) the same call first produces the parameter gradients exactly as sea_ib_bwd does (mode 2 has none: dw1 must be NULL).
 * Bad sizes or pointers return -1 before anything is launched. */
int64_t sea_silu_outer_bwd_dc_ws_floats(const SeaSiluBwdGroup* groups, int n_groups, int M);
int sea_silu_outer_bwd_dc(const SeaSiluBwdGroup* groups, int n_groups, const float* c, float* dc, int M, int dtype, float* ws, int64_t ws_floats,
                          void* stream);
int sea_ib_bwd_dc(const SeaIbBwdParams* params, float* dc, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * AdaLN whose modulation never reaches memory (bf16 compute): the normalisation is the epilogue of cond_mlp.2's GEMM.
 *     [w | b] = A[M, K] . W[2d, K]^T + bias            A = silu(cond_mlp.0(c)) rows (sea_silu_outer), W = cond_mlp.2.weight (scale rows 0..d-1, shift rows d..2d-1)
 *     y       = xhat * (gamma + 1 + w) + (beta + b),   xhat = (X - mean) / sqrt(var_biased + eps) over the d columns of a row of X
 * (models/base_blocks.py:337-350: AdaLN.forward) — instead of storing [w | b] as an [M, 2 d] matrix that a row-norm launch reads back.  A group WITHOUT X is
 * the plain GEMM: Yact [M, 2 d] receives [w | b] (modulations whose normalisation is another launch's epilogue: ln_cross); one launch carries both kinds.
 * mean / rstd (f32 [M]) are saved when non-NULL.  Requirements: dtype SEA_BF16; 16 <= d <= 1024, d % 8 == 0; K % 8 == 0; strides multiples of 8 (act) /
 * 4 (f32); pointers 16-byte aligned.  Returns SEA_EUNSUPPORTED for fp32.
 */
#define SEA_MAX_ADALN_GROUPS 16
typedef struct {
    const void* A;        /* act [M, K], row stride lda */
    const void* W;        /* act [2d, K], row stride ldw */
    const float* bias;    /* f32 [2d] or NULL */
    const float* X;       /* f32 [M, d], row stride ldx: the rows to normalise; NULL = plain group */
    const float* gamma;   /* f32 [d] */
    const float* beta;    /* f32 [d] or NULL */
    void* Yact;           /* act [M, d] (normalising group) or act [M, 2d] (plain group), row stride ldyact */
    float* Y32;           /* f32 [M, d], row stride ldy32, or NULL */
    float* mean;          /* f32 [M] or NULL */
    float* rstd;          /* f32 [M] or NULL */
    int32_t lda, ldw, ldx, ldyact, ldy32;
    int32_t M, d, K;
} SeaAdalnGroup;
int sea_gemm_adaln(const SeaAdalnGroup* groups, int n_groups, float eps, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Split-K finish: out = sum_s P[s] + bias * bias_scale + R, as fp32 (C32) and / or in the activation dtype (Cact) — the pass behind a sea_gemm_grouped
 * launch whose groups are K-slices of ONE Linear layer writing fp32 partial matrices (a few row tiles against a contraction of 16384: the MLP of
 * configs/multiphase_flow.py:112-141 at M = B T = 796).  The partial sums are added in split order.  N % 4 == 0; strides multiples of 4.
 */
typedef struct {
    const float* P;      /* f32 [S][M, N]: the partial matrices, p_stride elements apart, row stride ldp */
    const float* bias;   /* f32 [N] or NULL */
    const float* R;      /* f32 [M, N] row stride ldr, or NULL */
    float* C32;          /* f32 [M, N] row stride ldc32, or NULL */
    void* Cact;          /* act [M, N] row stride ldcact, or NULL */
    int64_t p_stride;
    int32_t S, M, N, ldp, ldr, ldc32, ldcact;
    float bias_scale;
} SeaSplitkGroup;
int sea_splitk_finish(const SeaSplitkGroup* groups, int n_groups, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * The front of a block in one launch (bf16, E = 256): the AdaLN condition MLP of AdaLN_0 with its hidden rows generated in place, AdaLN_0, and the
 * self-attention's q / k / v projections with the rotary epilogue —
 *     h = silu(w1 * cond[m] + b1)  [2E];   [w | b] = h . W2c^T + b2c;   y = xhat(X) * (gamma + 1 + w) + (beta + b)              (models/base_blocks.py:337-350)
 *     [q | k | v] = y . Wqkv^T + bqkv -> rotary embedding on q / k, q scale, Q [B,H,T,hd] / K [B,H,cap,hd] / Vt [B,H,hd,cap] as sea_qkv_rope_grouped (col0 = 0, N = 3E)
 * — a workgroup owns 32 rows from the caller's rows to the attention operands: replaces sea_silu_outer + sea_gemm_adaln + sea_qkv_rope_grouped for these modules
 * (no hidden matrix, no modulation matrix, no normalised rows in memory).  `riders`: plain bf16 groups (A, W, bias, Cact only; whole 64-wide K-tiles) of later
 * launches, run as 128 x 128 tiles by extra workgroups (sea_row_chain_riders' contract).  M = B * T rows per group; head dim 16 or 32, H * hd = E; cap % 8 == 0.
 * Returns SEA_EUNSUPPORTED for other shapes / dtypes.
 */
#define SEA_MAX_AQKV_GROUPS 4
typedef struct {
    const float* X;      /* f32 [M, E], row stride ldx */
    const float* cond;   /* f32 [M]: the condition scalar of a row */
    const float* w1;     /* f32 [2E]: cond_mlp.0.weight */
    const float* b1;     /* f32 [2E]: cond_mlp.0.bias */
    const void* W2c;     /* act [2E, 2E], row stride ldw2c: cond_mlp.2.weight (rows 0..E-1 scale, E..2E-1 shift) */
    const float* b2c;    /* f32 [2E] or NULL */
    const float* gamma;  /* f32 [E] */
    const float* beta;   /* f32 [E] or NULL */
    const void* Wqkv;    /* act [3E, E], row stride ldw: [Wq; Wk; Wv] */
    const float* bqkv;   /* f32 [3E] or NULL */
    void* Q;             /* act [B, H, T, hd] */
    void* K;             /* act [B, H, cap, hd], rows pos0 + t */
    void* Vt;            /* act [B, H, hd, cap], columns pos0 + t */
    int32_t ldx, ldw2c, ldw, M, E, N3;
    /* optional third layer (W3 != NULL; N3 = 256): mod3 = silu(w13 * cond[m] + b13) . W3^T + b3 — the modulation of another AdaLN module of the same rows
     * (ln_cross of the field, 2 D = 256 columns), stored for a later launch */
    const float* w13;    /* f32 [N3] */
    const float* b13;    /* f32 [N3] */
    const void* W3;      /* act [N3, N3], row stride ldw3 */
    const float* b3;     /* f32 [N3] or NULL */
    void* mod3;          /* act [M, N3], row stride ldmod3 */
    int32_t ldw3, ldmod3;
    /* optional condition memo (memo_stamps != NULL; NULL: none, every launch computes everything).  The modulation rows of a row are functions of cond[m] and the
     * weights alone.  A workgroup (32 rows) whose rows all carry the stamp {bits of cond[m], *memo_epoch} skips cond_mlp.2 of AdaLN_0 and the third layer: it reads
     * its AdaLN_0 modulation rows from memo_mods, and mod3 is left as it is.  Any other workgroup computes as without a memo, stores its modulation rows to
     * memo_mods and, at its end, writes its stamps.  The caller keeps stamps (zeroed once), memo_mods and mod3 between launches and changes *memo_epoch (never
     * to 0) whenever a weight of these modules changes.  memo_count: hits / misses are counted per workgroup where SEA_TUNE=memo_count=1. */
    uint32_t* memo_stamps;        /* u32 [M][2] */
    void* memo_mods;              /* act [M, 2E], row stride ldmemo: [scale | shift] of AdaLN_0 */
    const uint32_t* memo_epoch;   /* u32 [1], device memory */
    int32_t* memo_count;          /* i32 [2] (hits, misses) or NULL */
    uint32_t* memo_rows;          /* u32 [n_silu + 1][silu_M][2] or NULL, read from group 0 only: the stamps of the launch's ROW RIDERS, one set per silu group and
                                   * one (the last) for the information-bottleneck rows.  A row-rider workgroup (64 rows) whose rows all match exits: its hidden /
                                   * information-bottleneck rows of an earlier launch are still in the caller's buffers.  Any other computes and stamps its rows. */
    int32_t ldmemo, pad_;
} SeaAdalnQkv;
/* silu / silu_c / silu_M, ib (both optional): row riders — hidden rows silu(w1 * silu_c[m] + b1) of up to 8 other modules (sea_silu_outer's groups) and the
 * information-bottleneck rows (sea_silu_outer_ib's SeaIbParams), evaluated by extra workgroups for launches further down the step. */
int sea_adaln_qkv(const SeaAdalnQkv* groups, int n_groups, const SeaQkvCommon* common, const SeaGemmGroup* riders, int n_riders, const SeaSiluGroup* silu, int n_silu,
                  const float* silu_c, int silu_M, const SeaIbParams* ib, float eps, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * A ROW-LOCAL CHAIN of the state-exchange block in one launch (bf16 compute; a workgroup owns 16 or 32 rows from an attention launch's output to the
 * next attention launch's operands; sea_amd/csrc/chain.hip).  Per group (field), in order:
 *   form A (n_seg = 0):   x = Xin + a2[M,E] . W2[E,E]^T (+ b2)                          self-attention out-projection + residual
 *                                                                                       (models/base_blocks.py:201, models/temporal.py:136)
 *   form B (n_seg >= 1):  g = sum_s gelu_erf(att_s[M,D] . Wp_s[D,D]^T);  x = Xin + g . W2[E,D]^T + bias_scale * b2
 *                                                                                       (cross_attn[i][j].projection + GELU, cross_up[i] of the sum, the residual:
 *                                                                                       models/temporal.py:183-191 — exactly sea_exchange_tail's first two layers)
 *   X <- x (f32; Xin and X may be the same rows, or Xin the caller's strided [B,T,F,E] tensor);  Xact <- (act) x when non-NULL
 *   has_down:             y = LayerNorm_D(x . Wd[D,E]^T + bd) with gamma / beta / mod as SeaNormGroup -> down.Yact / down.Y32 when non-NULL
 *                                                                                       (cross_down[i] + ln_cross[i], models/temporal.py:177-181)
 *   n_proj entries:       columns [col0, col0 + N) of the virtual [q | k | v] row of  y . W[N,D]^T + bias, rotary embedding on q / k, q scale, written in the
 *                         attention layouts exactly as sea_qkv_rope_grouped (proj[e].A / lda / M are ignored; K = D; an entry is a q projection — N = D, col0 = 0 — or
 *                         a k | v projection — N = 2 D, col0 = D):
 *                         every q of the field and the k / v of the pairs that read this field's rows at this point of the Gauss-Seidel sweep
 *                         (models/base_blocks.py:271-280; models/temporal.py:187-192)
 * `down` is read as in SeaExchangeTail.  Requirements: dtype SEA_BF16; (D, E) in {(128, 256), (64, 128)}; n_seg * D <= E; H * hd == D for the projections;
 * sum of the projections' N <= 1024; head dim 16 or 32 (16 for launches of more than 256 16-row tiles), col0 a multiple of 16; strides multiples of 8 (act) / 4 (f32); pointers
 * 16-byte aligned.  Returns SEA_EUNSUPPORTED for other shapes / dtypes (callers keep the separate launches).
 */
#define SEA_CHAIN_MAX_PROJ 6
#define SEA_CHAIN_MAX_GROUPS 3
typedef struct {
    const void* att[SEA_XTAIL_MAX_SEG];   /* act [M, D], row stride ldatt (form B) */
    const void* Wp[SEA_XTAIL_MAX_SEG];    /* act [D, D], row stride ldwp */
    const void* a2;                       /* act [M, E], row stride lda2 (form A) */
    const void* W2;                       /* act [E, K2], row stride ldw2; K2 = D (form B) or E (form A) */
    const float* b2;                      /* f32 [E] or NULL */
    const float* Xin;                     /* f32 [M, E], row stride ldxin: the residual rows */
    float* X;                             /* f32 [M, E], row stride ldx: the updated rows (may alias Xin) */
    void* Xact;                           /* act [M, E], row stride ldxact, or NULL */
    int32_t n_seg, ldatt, ldwp, lda2, ldw2, ldxin, ldx, ldxact;
    int32_t M, D, E, has_down, n_proj;
    float bias_scale;
    SeaGemmNormGroup down;
    SeaQkvGroup proj[SEA_CHAIN_MAX_PROJ];
    /* optional condition memo of the launch's RIDER TILES (sea_row_chain_riders; read from group 0 only; tile_stamps NULL: none, every tile computes).  A rider tile's
     * 128 x 128 outputs are functions of tile_cond[m] of its rows, the weights and hidden rows that are themselves functions of both.  Tile t (numbered as the riders'
     * tiles are, over ALL the rider groups) owns the stamp set tile_stamps[t]: a tile whose live rows all carry the stamp {bits of tile_cond[m], *tile_epoch} exits and
     * touches nothing else; any other computes as without a memo and then stores its stamps.  The caller keeps the stamps (zeroed once), the riders' outputs AND their
     * A operands between launches, and changes *tile_epoch (never to 0) whenever a weight of these modules changes.  tile_count: hits / misses, one count per tile,
     * where SEA_TUNE=memo_count=1. */
    uint32_t* tile_stamps;        /* u32 [tile_sets][128][2] */
    const float* tile_cond;       /* f32 [riders' M] */
    const uint32_t* tile_epoch;   /* u32 [1], device memory */
    int32_t* tile_count;          /* i32 [2] (hits, misses) or NULL */
    int32_t tile_sets, pad_;      /* stamp sets behind tile_stamps: at least the riders' tile count */
} SeaRowChain;

/* params: n_groups <= SEA_CHAIN_MAX_GROUPS problems of one (D, E) (e.g. the F fields), one grid row each; common: rotary table, heads, positions of the projections
 * (may be NULL when no group has projections) */
int sea_row_chain(const SeaRowChain* params, int n_groups, const SeaQkvCommon* common, float eps, int dtype, void* stream);
/* The same launch carrying RIDERS: work of later launches that depends on nothing this one computes, run by extra workgroups on the CUs the chain leaves idle
 * (at one trajectory a chain launch is 127-192 workgroups on 256 CUs):
 *   riders   n_riders <= 8 plain groups as sea_gemm_grouped takes them (A, W, bias, Cact; bf16, K a multiple of 64: AdaLN's cond_mlp.2 of the modules the field
 *            MLP and the final norm read, models/base_blocks.py:339,344), cut into 128 x 128 tiles numbered group by group; THIS launch runs tiles
 *            [tile0, tile0 + n_tiles) — the caller spreads a GEMM over several chain launches;
 *   ib       NULL, or the information-bottleneck MLP whose rows ib->X[0][m, :] are STORED as sea_silu_outer_ib stores them (models/temporal.py:111-116).
 * Results are complete when the launch is; nothing in the same launch may read them.  params[0].tile_stamps != NULL: the rider tiles' condition memo (SeaRowChain:
 * the pointers travel in group 0, so sea_run_list's SEA_OP_CHAIN entry and a captured graph carry them as they carry every other field). */
struct SeaIbParams_;
int sea_row_chain_riders(const SeaRowChain* params, int n_groups, const SeaQkvCommon* common, const SeaGemmGroup* riders, int n_riders, int tile0, int n_tiles,
                         const struct SeaIbParams_* ib, float eps, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Launch list: a whole plan (every launch of TemporalModel.forward, models/temporal.py:405-416, in order) replayed by ONE call, so the host
 * side of a replay is a C loop over prepared argument structs instead of one interpreter round trip per launch (KV-cache rollout steps
 * and plain, un-captured forwards are host-bound otherwise).  `op` selects the entry point, the other fields are its arguments:
 *     SEA_OP_GEMM   p0 = SeaGemmGroup[n]                          SEA_OP_QKV    p0 = SeaQkvGroup[n], p1 = SeaQkvCommon
 *     SEA_OP_ATTN   p0 = SeaAttnParams                            SEA_OP_NORM   p0 = SeaNormGroup[n], i0 = M, i1 = d, i2 = x_is_act, i3 = gelu, f0 = eps
 *     SEA_OP_SILU   p0 = SeaSiluGroup[n], p1 = c, i0 = M, l0 = (intptr) SeaIbParams[l1] or 0, l1 = n_ib      SEA_OP_IB     p0 = SeaIbParams
 *     SEA_OP_CONVERT p0 = src, p1 = dst, l0 = lds, l1 = ldd, l2 = rows, l3 = cols
 *     SEA_OP_GEMM_NORM p0 = SeaGemmNormGroup[n], f0 = eps          SEA_OP_XTAIL  p0 = SeaExchangeTail[n], f0 = eps
 *     SEA_OP_MLP1   p0 = SeaMlpGroup[n], f0 = eps
 *     SEA_OP_MLP2   p0 = SeaMlp2Group[n], f0 = eps
 *     SEA_OP_GEMM_FEW p0 = SeaGemmGroup[n], p1 = pre or NULL, i0 = pre_x_is_act, i1 = pre_gelu, f0 = eps
 *     SEA_OP_QKV_FEW  p0 = SeaQkvGroup[n], p1 = SeaQkvCommon, l0 = (intptr) pre or 0, f0 = eps
 *     SEA_OP_ADALN    p0 = SeaAdalnGroup[n], f0 = eps
 *     SEA_OP_MLPB     p0 = SeaMlpGroup[n], p1 = SeaMlp2Group[n], f0 = eps
 *     SEA_OP_SPLITK   p0 = SeaSplitkGroup[n]
 *     SEA_OP_AQKV     p0 = SeaAdalnQkv[n], p1 = SeaQkvCommon, l0 = (intptr) SeaGemmGroup[i0] riders or 0, l1 = (intptr) SeaSiluGroup[i1] or 0, l2 = (intptr) silu_c, i2 = silu_M,
 *                     l3 = (intptr) SeaIbParams or 0, f0 = eps
 *     SEA_OP_CHAIN    p0 = SeaRowChain[n], p1 = SeaQkvCommon or NULL, f0 = eps; riders (sea_row_chain_riders): l0 = (intptr) SeaGemmGroup[i0] or 0, i1 = tile0, i2 = n_tiles,
 *                     l1 = (intptr) SeaIbParams or 0
 * Returns 0, or the failing entry's error code with sea_last_error() set (entries before it have been launched).
 */
enum { SEA_OP_GEMM = 1, SEA_OP_QKV = 2, SEA_OP_ATTN = 3, SEA_OP_NORM = 4, SEA_OP_SILU = 5, SEA_OP_IB = 6, SEA_OP_CONVERT = 8, SEA_OP_GEMM_NORM = 9, SEA_OP_XTAIL = 10, SEA_OP_MLP1 = 11, SEA_OP_MLP2 = 13, SEA_OP_GEMM_FEW = 14, SEA_OP_QKV_FEW = 15, SEA_OP_CHAIN = 16, SEA_OP_ADALN = 17, SEA_OP_MLPB = 18, SEA_OP_AQKV = 19, SEA_OP_SPLITK = 20 };   /* 7 and 12 were round-1 entry points (sea_rowchain, sea_cond_mlp), removed in ABI v2 */
typedef struct {
    int32_t op, n, dtype, i0, i1, i2, i3;
    float f0;
    const void* p0;
    const void* p1;
    int64_t l0, l1, l2, l3;
} SeaLaunchRec;
int sea_run_list(const SeaLaunchRec* recs, int n_recs, void* stream);

/* The same list replayed for n_steps consecutive steps of a KV-cache rollout (the loop of utils/train_utils.py:202-209) without returning to the caller's
 * language between steps: before step s (s = step0 .. step0 + n_steps - 1) every patch writes  base + s * stride  into the HOST argument struct it points
 * into — the position of a SeaQkvCommon / SeaAttnParams (kind 0: int32), the row pointers of the step's input / condition / output (kind 1: 64-bit) —, then
 * the list is launched (kernel arguments are copied at launch, so the structs may change under launches still in flight). */
typedef struct {
    void* addr;          /* host address of the field (inside a struct a SeaLaunchRec points to, or inside a SeaLaunchRec of `recs`) */
    int32_t kind;        /* 0: int32 field, 1: 64-bit field (a device pointer) */
    int32_t pad_;
    int64_t base, stride;
} SeaStepPatch;
int sea_run_list_steps(const SeaLaunchRec* recs, int n_recs, const SeaStepPatch* patches, int n_patches, int step0, int n_steps, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Un-patchify + inverse MinMax scaling of decoded fields: the scatter of DataPartitioner2D.inverse_partition
 * (utils/data_processors.py:93-111) fused with MinMaxScaler.inverse_transform (:258-273) and with the [B,P,F,C] -> [B,P,C,F]
 * permute of the evaluation loop (utils/train_utils.py:223-226):
 *     out[b, index_map[p, c], f] = in[b, p, f, c] * scale[f] + shift[f]        for index_map[p, c] >= 0 (pad_id = -1 skipped)
 * `in` is addressed with element strides (sb, sp, sf, sc) so that both the decoder's [B,P,F,C] output and the reference's
 * [T,P,C,F] argument layout are read in place; out f32 [B, n_points, F] contiguous; index_map int32 [P, C]; scale, shift f32 [F].
 * Every mesh point belongs to exactly one (p, c), so the scatter needs no atomics and writes every output element once.
 * `point_slot` (optional, int32 [n_points], point_slot[index_map[p, c]] = p * C + c) selects the GATHER form: one thread per output
 * point, fully coalesced writes, reads served from L2 (one snapshot's decoded cells are ~1 MB) — 3x faster on a 30000-point mesh.
 */
int sea_unpatchify(const float* in, int64_t sb, int64_t sp, int64_t sf, int64_t sc, const int32_t* index_map, const int32_t* point_slot,
                   const float* scale, const float* shift, float* out, int B, int P, int F, int C, int n_points, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Patchify + MinMax scaling of mesh fields (forward direction): MeshProcessor._scale_fields
 * (utils/data_processors.py:528-536: MinMaxScaler.transform per field group, :241-247) followed by DataPartitioner2D.create_partitions /
 * pad_partitions (:60-92) and the stack / permute the encoder's input needs (:519-525):
 *     out[b, p, f, c] = in[b, index_map[p, c], f] * scale[f] + shift[f]     for c < C_map and index_map[p, c] >= 0
 *                     = pad_value                                           otherwise (empty slots; the row padding C_map .. C_out - 1)
 * `in` f32 [B, n_points, F] contiguous; index_map int32 [P, C_map] (pad_id = -1); `out` is addressed with element strides (sb, sp, sf, sc), so
 * both the encoder's [B, P, F, C_out] layout and the reference's [T, P, C, F] are written in place.  The pad value is NOT scaled (the reference
 * scales first and pads with pad_field_value afterwards).
 */
int sea_patchify(const float* in, const int32_t* index_map, const float* scale, const float* shift, float* out, int64_t sb, int64_t sp, int64_t sf,
                 int64_t sc, int B, int P, int F, int C_map, int C_out, int n_points, float pad_value, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Exact KV-cache rollout, the whole step loop in one call (utils/train_utils.py:202-209 around models/temporal.py:120-200, 398-417; one row per
 * call instead of the growing prefix).  Step k (position pos0 + k) reads traj[pos0 + k] ([B, F, E] f32), appends this position's keys / values to the
 * caches, attends over positions <= pos0 + k and writes traj[pos0 + k + 1].  Seven launches per layer and step (sea_amd/csrc/kvstep.hip): every
 * Linear is a GEMV of fp32 activation vectors against act-dtype weights; the q/k/v projections of a head ride in its attention workgroup; the
 * Gauss-Seidel tails of all fields are one launch whose workgroups hand the updated field over through tagged 8-byte granules.
 * Supported: exchange_mode 'sea' (exchange = 1, F >= 2) or 'simple' (exchange = 0), LN_type adaln / ln, any info-bottleneck mode (the caller
 * evaluates the term for all steps), src_len = 0, E <= 512, head dims 8 / 16 / 32 / 64, widths whose 16-byte chunk count is a power of two <= 64
 * or 128 / 256 / 512.
 * What depends on the condition only is evaluated by the CALLER for all steps before the call: SeaKvNorm.mod = act [n_rows, 2 d] (row k * B + b of step k:
 * AdaLN's cond_mlp output, models/base_blocks.py:337-344; NULL for LN_type 'ln'), SeaKvLayer.ib = f32 [n_rows, E] (the info-bottleneck term,
 * models/temporal.py:103-114; NULL for ib_addition_mode 'none').
 * Caches are act [B, H, cap, hd] for keys AND values (row-major values: an append is one row).  Workspaces are f32, sized in elements:
 * att_e, xr, xq, x3, xl[0], xl[1]: B F E; hbuf: B F S; nd_old: B F D; oc, qc: F (F-1) B D; ml: F (F-1) B H 2; handoff: B F D 8-byte words, zeroed once
 * by the caller; err: one int32, zeroed by the caller — non-zero after the call's work has completed means a hand-off wait gave up (results invalid).
 * tag0: the caller's running launch counter (each (step, layer) consumes one value; values must not repeat while `handoff` lives; 0 is never used).
 */
#define SEA_KV_MAX_FIELDS 4
typedef struct {
    const float* gamma;   /* f32 [d] */
    const float* beta;    /* f32 [d] or NULL */
    const void* mod;      /* act [n_rows, ldmod] (scale | shift) or NULL */
    int32_t ldmod, pad_;
} SeaKvNorm;
typedef struct {
    SeaKvNorm ln0, ln_cross, ln2;                  /* ln.exp.i.0, ln_cross.i, ln.exp.i.2 */
    const void* Wqkv; const float* bqkv;           /* act [3E, E] (q | k | v), f32 [3E] */
    const void* Wo;                                /* act [E, E], no bias */
    const void* Wdown; const float* bdown;         /* act [D, E] */
    const void* Wup; const float* bup;             /* act [E, D] */
    const void* W1; const float* b1;               /* act [S, E] */
    const float* lnw; const float* lnb;            /* f32 [S]: nn.LayerNorm(S) */
    const void* W2; const float* b2;               /* act [E, S] */
    const void* Wproj; const float* bproj;         /* act [E, E] */
    void* Ks; void* Vs;                            /* act [B, H, cap, E / H] */
} SeaKvField;
typedef struct {
    const void* Wq; const float* bq;               /* act [D, D] */
    const void* Wkv; const float* bkv;             /* act [2D, D] (k | v) */
    const void* Wp;                                /* act [D, D], no bias */
    void* Kc; void* Vc;                            /* act [B, H, cap, D / H] */
} SeaKvPair;
typedef struct {
    SeaKvField f[SEA_KV_MAX_FIELDS];
    SeaKvPair p[SEA_KV_MAX_FIELDS][SEA_KV_MAX_FIELDS];   /* p[i][j]: field i attends to field j (j != i) */
    const float* ib;
} SeaKvLayer;
typedef struct {
    int32_t F, E, D, S, H, B, L, cap, exchange, ib_after_cross;
    SeaKvNorm final_ln[SEA_KV_MAX_FIELDS];
    const float* rope_self;    /* f32 [max_len, E / H / 2, 2] (cos, sin) */
    const float* rope_cross;   /* f32 [max_len, D / H / 2, 2] */
    float* traj;               /* f32 [n_positions + 1, B, F, E] */
    float* xl[2];
    float* att_e; float* xr; float* xq; float* x3; float* hbuf; float* nd_old; float* oc; float* qc; float* ml;
    unsigned long long* handoff;
    int32_t* err;
    int64_t handoff_words;     /* size of `handoff` in 8-byte words: >= B F D; with >= sea_kv_arena_words() words, B = 1 and L = 1 the whole rollout runs as ONE
                                * persistent launch (every workgroup keeps the weights of its role in registers across steps) */
} SeaKvGlobal;

int sea_kv_rollout(const SeaKvGlobal* G, const SeaKvLayer* layers, int pos0, int n_steps, uint32_t tag0, int dtype, void* stream);
/* Words of `handoff` the persistent form of sea_kv_rollout needs for these sizes (host only). */
int64_t sea_kv_arena_words(const SeaKvGlobal* G);

/* ------------------------------------------------------------------------------------------------------------
 * KV-cache prefill from a multi-step context (the reference rolls out from a known prefix by recomputing the full forward over it every step,
 * utils/train_utils.py:202-209): the full-context forward over the k context rows leaves every attention module's keys K [B, H, cap_src, hd] and
 * values V^T [B, H, hd, cap_src] for positions 0 .. k-1 in its own buffers; ONE launch moves them into the decode caches, so that the exact KV
 * decode continues from position k.  Per table entry, positions 0 .. n_pos-1 of every (b, h):
 *   K -> Kd [B, H, cap_dst, hd];
 *   Vt -> Vd, either as [B, H, cap_dst, hd] rows (v_rows = 1: sea_kv_rollout's caches, transposed through LDS tiles) or as [B, H, hd, cap_dst]
 *   (v_rows = 0: the generic step plan's caches, only the capacity stride changes).
 * Positions >= n_pos of a destination are never touched.  Requirements: hd a multiple of 8 in [8, 256]; 1 <= n_pos <= cap_src, cap_dst; cap_src and
 * cap_dst multiples of 8; every pointer 16-byte aligned.  One launch per SEA_KV_FILL_MAX entries (the table travels in the kernel arguments).
 */
#define SEA_KV_FILL_MAX 32
typedef struct {
    const void* K;     /* act [B, H, cap_src, hd] */
    const void* Vt;    /* act [B, H, hd, cap_src] */
    void* Kd;          /* act [B, H, cap_dst, hd] */
    void* Vd;          /* act [B, H, cap_dst, hd] (v_rows = 1) or [B, H, hd, cap_dst] (v_rows = 0) */
    int32_t B, H, hd, n_pos, cap_src, cap_dst, v_rows, pad_;
} SeaKvFill;
int sea_kv_cache_fill(const SeaKvFill* entries, int n, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * KV-cache fork: a rollout session that branches into n_rep what-if continuations per trajectory copies the cache positions it has filled so far
 * into the caches of a session of B_src * n_rep trajectories instead of prefilling the repeated history again.  Per table entry, ONE cache tensor:
 * positions 0 .. n_pos-1 of every head of source row b go to destination rows b * n_rep + j, j = 0 .. n_rep-1 (row b * n_rep + j is branch j of b).
 * Source and destination have the same layout:
 *   transposed = 0: [B, H, cap, hd] rows (every key cache, the value rows of sea_kv_rollout): n_pos * hd contiguous elements per (b, h);
 *   transposed = 1: [B, H, hd, cap] (V^T of the generic step plan): hd runs of n_pos elements per (b, h), the last 16-byte chunk of a run may be partial.
 * Every 16-byte line of the source is read once and written n_rep times; the copy is exact (raw bits).  Positions >= n_pos of the destination are
 * never touched.  Requirements: B_src, H, n_rep >= 1 (n_rep = 1: a plain copy); hd a multiple of 8 in [8, 256]; 1 <= n_pos <= cap_src, cap_dst; cap_src
 * and cap_dst multiples of 8, independent of each other; both pointers 16-byte aligned; source and destination do not overlap.  One launch per
 * SEA_KV_FORK_MAX entries (the table travels in the kernel arguments).  Returns -1, with the entry named in sea_last_error(), otherwise.
 */
#define SEA_KV_FORK_MAX 32
typedef struct {
    const void* src;   /* act [B_src, H, cap_src, hd] (transposed = 0) or [B_src, H, hd, cap_src] (transposed = 1) */
    void* dst;         /* act [B_src * n_rep, H, cap_dst, hd] or [B_src * n_rep, H, hd, cap_dst] */
    int32_t B_src, H, hd, n_pos, cap_src, cap_dst, n_rep, transposed;
} SeaKvFork;
int sea_kv_cache_fork(const SeaKvFork* entries, int n, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * KV-cache gather: the other direction of the fork.  A rollout session that keeps, drops, repeats or reorders trajectories (ensemble resampling,
 * beam / MPC pruning) copies the cache positions it has filled so far into the caches of a session of B_dst trajectories instead of prefilling the
 * selected histories again.  Per table entry, ONE cache tensor: positions 0 .. n_pos-1 of every head of source row index[j] go to destination row j,
 * j = 0 .. B_dst-1; a source row may appear several times or not at all.  Source and destination state their layouts separately:
 *   0: [B, H, cap, hd] rows (every key cache, the value rows of sea_kv_rollout);  1: [B, H, hd, cap] (V^T of the generic step plan).
 * Equal layouts are copied in 16-byte chunks as sea_kv_cache_fork does (the partial last chunk of a V^T run element by element); rows -> V^T and
 * V^T -> rows go through an LDS tile of 64 positions x 64 value columns, 16 bytes per lane on both global sides.  The copy is exact (raw bits);
 * positions >= n_pos of the destination are never touched.  The kernel reads `index` itself and skips a destination row whose index lies outside
 * [0, B_src): a guard against reading outside the source, not an interface — callers validate the index.
 * Requirements: B_src, B_dst, H >= 1; hd a multiple of 8 in [8, 256]; 1 <= n_pos <= cap_src, cap_dst; cap_src and cap_dst multiples of 8, independent
 * of each other; the layout flags 0 or 1; all three pointers non-NULL, src and dst 16-byte aligned; source and destination do not overlap.  One launch
 * per SEA_KV_GATHER_MAX entries (the table travels in the kernel arguments).  Returns -1, with the entry named in sea_last_error(), otherwise.
 * (An addition to ABI version 8.  sea_struct_sizes() keeps its 33 entries, SeaKvFork last: sizeof(SeaKvGather) is 64.)
 */
#define SEA_KV_GATHER_MAX 32
typedef struct {
    const void* src;        /* act [B_src, H, cap_src, hd] (src_transposed = 0) or [B_src, H, hd, cap_src] (1) */
    void* dst;              /* act [B_dst, H, cap_dst, hd] (dst_transposed = 0) or [B_dst, H, hd, cap_dst] (1) */
    const int32_t* index;   /* device, B_dst entries, each in [0, B_src) */
    int32_t B_src, B_dst, H, hd, n_pos, cap_src, cap_dst, src_transposed, dst_transposed, pad_;
} SeaKvGather;
int sea_kv_cache_gather(const SeaKvGather* entries, int n, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Field-space loss of the spatial decoder: the mean-squared error of the DECODED fields against patch targets and its gradient with respect to the
 * decoder's hidden rows, in one launch for all field groups (plus a one-block finish).  Replaces, for a loss taken on decoded fields
 * (F.mse_loss(Decode(z), target) over models/encoder_decoder.py:126-146), the second decoder Linear (sea_gemm_grouped into an [M, n_fields * Cp] fp32
 * output), sea_mse_fwd_bwd over that output and the data-gradient GEMM back to the hidden rows — without the output or the residual ever existing
 * in memory.  Per group, rows m = 0 .. M-1:
 *     Y[m, j, c] = sum_s H[m, s] W2[j Cp + c, s] + bias[j Cp + c]        j < n_fields, c < C        (fp32 accumulation)
 *     D[m, j, c] = valid(m, c) ? Y[m, j, c] - target[m, field0 + j, c] : 0
 *     loss       = inv_n * sum over groups, m, j, c of D^2
 *     dH[m, s]   = 2 grad_scale inv_n * sum_{j, c} D[m, j, c] W2[j Cp + c, s]   [* gelu_erf'(Z[m, s]) when Z != NULL]     (written in the act dtype)
 * H: the hidden rows GELU(z W1^T) and W2: the padded second-layer shadow copy, as Decode.forward prepares them; field j of a group sits at rows
 * [j Cp, j Cp + C) of W2, the pad rows are zero.  Z: the saved pre-activation of the first layer (sea_gemm_grouped act = 1 with Z kept): with it dH is
 * the gradient of the PRE-activation, ready for the data-gradient GEMM against W1.  target element (m, f, c) is at target + m ld_row + f ld_field + c
 * (what sea_patchify writes in layout "BPFC"); f = field0 + j counts over all groups in the decoder's output order; only c < C is ever read.
 * valid(m, c) = c < C when counts == NULL, else c < counts[m % P] (device int32 [P], values in [0, C]: a cell's mesh points are a prefix of its
 * row; the kernel clamps a value outside [0, C] — a guard, not an interface).  Invalid slots and the pad columns contribute neither loss nor
 * gradient, whatever the target holds there (NaN included).  inv_n is the caller's 1 / (number of valid elements).
 * The residual is rounded to the act dtype once between the two products; the loss is summed from the fp32 residual through `partial` (f32,
 * n_partial_cap >= ceil(M / 64) * n_groups) in a fixed order and dH has one writer per element: two runs give the same bits.
 * Requirements: dtype SEA_BF16 (SEA_F32 returns SEA_EUNSUPPORTED: the fp32 decoder composes the launches above); M >= 1; S a multiple of 8, at most
 * 640 (above: SEA_EUNSUPPORTED); any S in that range — the contraction is padded by masking in the kernel, the shadow copies stay [.., S]; Cp a
 * multiple of 32, 1 <= C <= Cp; P >= 1 and M % P == 0 when counts is given; ld_row, ld_field multiples of 4, target 16-byte aligned; per group all
 * pointers but Z non-NULL and 16-byte aligned, ldh, ldw multiples of 8, every row stride >= S; 1 <= n_groups <= SEA_DECODE_MSE_MAX_GROUPS.
 * Returns -1, with the entry point and the offending group named in sea_last_error(), otherwise; nothing touches a device before the checks pass.
 * (An addition to ABI version 8.  sea_struct_sizes() keeps its 33 entries: sizeof(SeaDecodeMseGroup) is 64, sizeof(SeaDecodeMse) 80.)
 */
#define SEA_DECODE_MSE_MAX_GROUPS 16
typedef struct {
    const void* H;       /* act [M, S], row stride ldh */
    const void* W2;      /* act [n_fields * Cp, S], row stride ldw */
    const float* bias;   /* f32 [n_fields * Cp] */
    void* dH;            /* act [M, S], row stride lddh (output) */
    const void* Z;       /* act [M, S], row stride ldz, or NULL */
    int32_t ldh, ldw, lddh, ldz;
    int32_t n_fields;    /* fields of this group */
    int32_t field0;      /* index of the group's first field in the target */
} SeaDecodeMseGroup;
typedef struct {
    const float* target;
    const int32_t* counts;   /* device int32 [P] or NULL */
    float* loss;             /* f32 [1] (output) */
    float* partial;          /* f32 [n_partial_cap] workspace */
    int64_t ld_row, ld_field;
    int32_t M, S, C, Cp, P, n_partial_cap;
    float inv_n, grad_scale;
} SeaDecodeMse;
int sea_decode_mse(const SeaDecodeMseGroup* groups, int n_groups, const SeaDecodeMse* p, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Ensemble weighting: the squared error of the DECODED fields of every ensemble member against an observation, per member and per field, in one
 * launch for all field groups (plus a short finish launch) — the likelihood term of a particle filter over rollout sessions (RolloutSession.fork /
 * resample).  Replaces the second decoder Linear into an [M, n_fields * Cp] fp32 output and the reductions over it; neither the decoded fields nor
 * the residual ever exist in memory.  It takes the SeaDecodeMseGroup operands H, W2, bias, ldh, ldw, n_fields, field0 as sea_decode_mse does (dH, Z,
 * lddh, ldz are not read and may be NULL / 0).  Row m belongs to member m / P and patch m % P; the `members` consecutive members of one history share
 * one observation, so the target row of m is trow(m) = ((m / P) / members) * P + m % P:
 *     Y[m, j, c]               = sum_s H[m, s] W2[j Cp + c, s] + bias[j Cp + c]        j < n_fields, c < C        (fp32 accumulation)
 *     sse[m / P, field0 + j]  += valid(m, c) ? (Y[m, j, c] - target[trow(m), field0 + j, c])^2 : 0
 * target element (r, f, c) is at target + r ld_row + f ld_field + c; only c < C is ever read.  valid(m, c) = c < C when counts == NULL, else
 * c < counts[m % P] (device int32 [P]; a value outside [0, C] is clamped — a guard, not an interface).  An invalid slot is neutral whatever the target
 * holds there, NaN included.  The residual stays in fp32 (no second product consumes it).  sse: f32 [M / P, n_fields_total], every element written
 * (not accumulated into): the groups' field ranges [field0, field0 + n_fields) must cover 0 .. n_fields_total-1 exactly once.
 * work: f32 workspace of work_cap >= M * n_fields_total floats, private to the call: the main kernel writes the per-row, per-field sums there (the four
 * lanes that hold a row's columns folded first), the finish launch sums the P rows of each member.  No atomics; every element has one writer and a
 * fixed summation order: two runs give the same bits, and the result does not depend on `members` beyond the target row it selects.
 * Requirements: those of sea_decode_mse — dtype SEA_BF16 (SEA_F32 returns SEA_EUNSUPPORTED); M >= 1; S a multiple of 8, at most 640 (above:
 * SEA_EUNSUPPORTED), padded by masking; Cp a multiple of 32, 1 <= C <= Cp; ld_row, ld_field multiples of 4, target 16-byte aligned; per group H, W2,
 * bias non-NULL and 16-byte aligned, ldh, ldw multiples of 8 and >= S; 1 <= n_groups <= SEA_DECODE_MSE_MAX_GROUPS — and P >= 1, members >= 1,
 * M % (P * members) == 0, work_cap >= M * n_fields_total.
 * Returns -1, with the entry point and the offending group named in sea_last_error(), otherwise; nothing touches a device before the checks pass.
 * (An addition to ABI version 8.  sea_struct_sizes() keeps its 33 entries, SeaKvFork last: sizeof(SeaDecodeMemberSse) is 88.)
 */
typedef struct {
    const float* target;     /* f32, rows of the observation: [M / (P * members) * P, n_fields_total, >= C] through ld_row, ld_field */
    const int32_t* counts;   /* device int32 [P] or NULL */
    float* sse;              /* f32 [M / P, n_fields_total] (output) */
    float* work;             /* f32 [work_cap] workspace */
    int64_t ld_row, ld_field, work_cap;
    int32_t M, S, C, Cp, P, members, n_fields_total, pad_;
} SeaDecodeMemberSse;
int sea_decode_member_sse(const SeaDecodeMseGroup* groups, int n_groups, const SeaDecodeMemberSse* p, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * The forecast of an ensemble: the weighted mean and the weighted, centred variance of the DECODED fields over the members of every history, in one
 * launch for all field groups (plus a short finish launch above 128 members).  The decoded member fields never exist in memory.  Operands H, W2,
 * bias, ldh, ldw, n_fields, field0 of SeaDecodeMseGroup as in sea_decode_member_sse (dH, Z, lddh, ldz are not read); there is no target.  Row
 * m = (b * members + j) * P + patch of H is member j of history b (the order of RolloutSession.fork); B = M / (P * members) histories.
 *     y_j[b, patch, f, c]    = sum_s H[m, s] W2[(f - field0) Cp + c, s] + bias[(f - field0) Cp + c]           (fp32 accumulation; never stored)
 *     mean[b, patch, f, c]   = sum_j w_j y_j / sum_j w_j                                                      over the LIVE members j
 *     var[b, patch, f, c]    = var_scale[b] * sum_j w_j (y_j - mean)^2
 * w: f32 [B * members], the weight of member j of history b at b * members + j, normalised per history by the caller (sum 1: the mean is then
 * sum_j w_j y_j); NULL: 1 / members each.  A member with w <= 0 or NaN is DEAD: it is passed over by a select, not multiplied by 0 — its hidden row is
 * not read, and NaN or Inf in it reaches no output.  A history without a live member gets mean = var = 0.  var_scale: f32 [B] or NULL (1) — the caller's
 * correction factor, e.g. 1 / (1 - sum_j w_j^2) for the unbiased estimator.  counts: device int32 [P] or NULL; valid(patch, c) = c < counts[patch]
 * (clamped to [0, C]; NULL: c < C).  mean, var: f32 [B * P, n_fields_total, ld], element (bp, f, c) at (bp * n_fields_total + f) * ld + c; EVERY element
 * is written: invalid columns and the columns [C, ld) are exactly 0 in both, so a freshly allocated output holds nothing uninitialised.  Only the
 * ceil(counts[patch] / 32) column tiles of a field that hold valid columns are computed.
 * Numerics: every partial result is a triple (W, mean, M2) with M2 taken about the partial's own mean — a lane's four members about their mean, then
 * Chan's pairwise update  M2 = M2_a + M2_b + W_a W_b / (W_a + W_b) (m_a - m_b)^2  over lane groups, the 8 waves of a workgroup (16 members each) and the
 * 128-member chunks, in a fixed order.  Nothing is formed as E[y^2] - E[y]^2.  A history whose weight sits on one member returns that member's decoded
 * row bit for bit and var == 0 exactly.  No atomics, one writer per output element: two runs give the same bits, and a history's result does not
 * depend on the other histories of the call.
 * work: f32 workspace, private to the call, read only when members > 128: work_cap >= ceil(members / 128) * (2 * B * P * n_fields_total * ld + B * P)
 * floats (a partial mean and M2 per chunk and output element, a weight per chunk and output row); may be NULL up to 128 members.
 * Requirements: dtype SEA_BF16 (SEA_F32 returns SEA_EUNSUPPORTED); M >= 1; S a multiple of 8, at most 640 (above: SEA_EUNSUPPORTED), padded by
 * masking; Cp a multiple of 32, 1 <= C <= Cp; P >= 1, members >= 1, M % (P * members) == 0; ld >= C, ld % 4 == 0; mean, var 16-byte aligned; w,
 * var_scale, counts, work 4-byte aligned; per group H, W2, bias non-NULL and 16-byte aligned, ldh, ldw multiples of 8 and >= S; the groups' field
 * ranges cover 0 .. n_fields_total-1 exactly once; 1 <= n_groups <= SEA_DECODE_MSE_MAX_GROUPS.
 * Returns -1, with the entry point and the offending group named in sea_last_error(), otherwise; nothing touches a device before the checks pass.
 * (An addition to ABI version 8.  sea_struct_sizes() keeps its 33 entries, SeaKvFork last: sizeof(SeaDecodeMemberMoments) is 88.)
 */
typedef struct {
    const float* w;           /* f32 [B * members] normalised weights, or NULL (1 / members) */
    const float* var_scale;   /* f32 [B], or NULL (1) */
    const int32_t* counts;    /* device int32 [P] or NULL */
    float* mean;              /* f32 [B * P, n_fields_total, ld] (output) */
    float* var;               /* f32 [B * P, n_fields_total, ld] (output) */
    float* work;              /* f32 [work_cap] workspace (members > 128), or NULL */
    int64_t work_cap;
    int32_t M, S, C, Cp, P, members, n_fields_total, ld;
} SeaDecodeMemberMoments;
int sea_decode_member_moments(const SeaDecodeMseGroup* groups, int n_groups, const SeaDecodeMemberMoments* p, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * The ensemble Kalman analysis from a DENSE observation of the decoded fields, part 1: per (history, patch) the N x N Gram matrix of the members'
 * weighted decoded anomalies and its product with the innovation, in one launch for all field groups (looped inside the workgroup in ascending
 * order).  Neither the members' decoded fields nor an [B N, K] prediction matrix ever exist in memory.  Operands H, W2, bias, ldh, ldw, n_fields,
 * field0 of SeaDecodeMseGroup exactly as in sea_decode_member_moments; row m = (b * members + j) * P + p of H is member j of history b;
 * B = M / (P * members); N = members.  Per history b and patch p:
 *     y_j[f, c]     = sum_s H[m, s] W2[(f - field0) Cp + c, s] + bias[(f - field0) Cp + c]                   (fp32 accumulation; never stored)
 *     w[f, c]       = valid(p, c) ? (pf[f] > 0 ? pf[f] : 0) * (prec != NULL ? (prec[b, p, f, c] > 0 ? prec[b, p, f, c] : 0) : 1) : 0
 *                     selects: a NaN counts as 0; pf = prec_field (NULL: 1); valid(p, c) = c < counts[p] (clamped to [0, C]; NULL: c < C)
 *     ybar[f, c]    = (1 / N) sum_j y_j[f, c]           a_j = y_j - ybar                                     (centred form, fixed member order, fp32)
 *     gram[b,p,i,j] = sum_{w > 0} w a_i a_j                                                                  f64 [B, P, N, N], written in full, exactly symmetric
 *     proj[b,p,j]   = sum_{w > 0} w a_j (obs[b, p, f, c] - ybar[f, c])                                       f64 [B, P, N]
 *     count[b,p]    = #{(f, c): w > 0}, or -1 when obs or a member's value at such a cell, or a stored sum, is not finite       int32 [B, P]
 * obs element (b P + p, f, c) is at obs + (b P + p) ld_row + f ld_field + c (the layout of SeaDecodeMemberSse.target); prec, when given, has the same
 * layout through ld_prow, ld_pfield.  A cell without weight — an invalid slot, a pad column, prec or pf not positive — is neutral by a select whatever
 * obs and prec hold there, NaN and Inf included; obs is not even read there.  Member rows beyond N inside a 16-row block contribute nothing.
 * Numerics: the mean and the anomalies in fp32; sqrt(w) is put on both factors, so that a product commutes; products are summed in fp32 only inside one
 * 32-column tile (the f32-input MFMA: an ordered fmaf chain); everything across tiles, fields and groups is added in fp64 in ascending (group, field,
 * tile) order; proj is summed in fp64 per lane (16 column classes per member) and the classes are folded in ascending order.  Only the
 * ceil(counts[p] / 32) tiles of a field that hold valid columns are walked; a patch without a valid column gets zeros and count 0.
 * One workgroup per (history, patch), no atomics, one writer per element: two runs give the same bits, and a history's outputs do not depend on the
 * other histories of the call.
 * Requirements: dtype SEA_BF16 (SEA_F32: SEA_EUNSUPPORTED); M >= 1; S a multiple of 8, at most 640 (above: SEA_EUNSUPPORTED), padded by masking; Cp a
 * multiple of 32, 1 <= C <= Cp; P >= 1; members >= 2 (above 128: SEA_EUNSUPPORTED); M % (P * members) == 0; ld_field, ld_pfield >= C; obs, prec,
 * prec_field, counts, count 4-byte, gram and proj 8-byte aligned; per group H, W2, bias non-NULL and 16-byte aligned, ldh, ldw multiples of 8 and
 * >= S; the groups' field ranges cover 0 .. n_fields_total-1 exactly once; 1 <= n_groups <= SEA_DECODE_MSE_MAX_GROUPS.
 * Returns -1, with the entry point and the offending group named in sea_last_error(), otherwise; nothing touches a device before the checks pass.
 * Notes the form "decode.member_gram" (a = the padded hidden width, b = the dynamic LDS bytes).
 * (An addition to ABI version 8.  sea_struct_sizes() keeps its 33 entries, SeaKvFork last: sizeof(SeaDecodeMemberGram) is 120.)
 */
typedef struct {
    const float* obs;          /* f32, rows of the observation: [B * P, n_fields_total, >= C] through ld_row, ld_field */
    const float* prec_field;   /* f32 [n_fields_total], or NULL (1) */
    const float* prec;         /* f32 map in obs's layout through ld_prow, ld_pfield, or NULL (1) */
    const int32_t* counts;     /* device int32 [P] or NULL */
    double* gram;              /* f64 [B, P, members, members] (output) */
    double* proj;              /* f64 [B, P, members] (output) */
    int32_t* count;            /* int32 [B, P] (output) */
    int64_t ld_row, ld_field, ld_prow, ld_pfield;
    int32_t M, S, C, Cp, P, members, n_fields_total, pad_;
} SeaDecodeMemberGram;       /* 120 bytes */
int sea_decode_member_gram(const SeaDecodeMseGroup* groups, int n_groups, const SeaDecodeMemberGram* p, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Ensemble weighting against SPARSE observations: K sensors, each reading one decoded field at one cell of one patch, shared by all histories of the
 * call; the precision-weighted squared error of every member in one launch for all field groups (plus a short finish launch).  The host sorts the
 * sensors by (group, patch, given order), pads every (group, observed patch) segment to a multiple of 32 entries and hands over the tables
 * (sea_amd/ensemble.py, SensorSet); K_pad is the length of the sorted, padded list and Q the number of observed patches (the sorted union over all
 * groups).  Operands H, W2, bias, ldh, ldw, n_fields of SeaDecodeMseGroup (dH, Z, lddh, ldz, field0 are not read).  H holds the hidden rows of the
 * OBSERVED patches only, patch-major: row q * Bm + bm is member bm at observed patch q, [Q * Bm, S].  For sorted position k of group g in patch q
 * (seg[g * (Q + 1) + q] <= k < seg[g * (Q + 1) + q + 1]), member bm of history b = bm / members:
 *     y[bm, k]   = sum_s H_g[q * Bm + bm, s] W2_g[wrow[k], s] + bias_g[wrow[k]]                       (fp32 accumulation)
 *     w          = live[k] != 0 and prec[b * ld_prec + k] > 0 ? prec[b * ld_prec + k] : 0              (prec == NULL: 1)
 *     d          = w > 0 ? y[bm, k] - obs[b * ld_obs + k] : 0          (a select: without weight a sensor is neutral whatever obs holds, NaN and Inf included)
 *     wsse[bm]   = sum_k (w d) d                                        (fp32)
 *     pred[bm * K_pad + k] = y[bm, k]                                   (when pred != NULL; pad positions are written too — W2 row wrow[k] = 0, a defined value)
 * obs, prec: f32 in sorted, padded order, one row per history (ld_prec == 0: one precision row for all histories); live: int32 [K_pad], 0 at the pad
 * entries; wrow: int32 [K_pad], the W2 row (field - first field of the group) * Cp + cell of every entry — the PADDED column index — and 0 at the
 * pad entries; seg: int32 [n_groups, Q + 1], every row ascending in steps that are multiples of 32 (an empty step: the group has no sensor in that
 * patch).  The kernel TRUSTS wrow (0 <= wrow < n_fields * Cp of its group) and seg (0 <= seg <= K_pad): they are device data the entry point cannot
 * read; the caller range-checks them on the host before the upload.  work: f32 workspace of work_cap >= Q * n_groups * Bm floats, private to the
 * call: one partial per (patch, group, member), every one written (zeros for an empty segment), summed per member by the finish launch in ascending
 * order.  No atomics, one writer per element: two runs give the same bits, and a member's score does not depend on `members`, on the number of
 * histories or on the row tile the member falls into.
 * Requirements: dtype SEA_BF16 (SEA_F32 returns SEA_EUNSUPPORTED); Bm >= 1, members >= 1, Bm % members == 0; S a multiple of 8, at most 640
 * (above: SEA_EUNSUPPORTED), padded by masking; Cp a multiple of 32; K_pad a multiple of 32, >= 32; 1 <= Q <= 65535; ld_obs >= K_pad, a multiple of
 * 4; ld_prec 0 or as ld_obs; obs, prec (nullable), pred (nullable) 16-byte aligned, live, wrow, seg, wsse, work non-NULL and 4-byte aligned; per
 * group H, W2, bias non-NULL and 16-byte aligned, ldh, ldw multiples of 8 and >= S; 1 <= n_groups <= SEA_DECODE_MSE_MAX_GROUPS.
 * Returns -1, with the entry point named in sea_last_error(), otherwise; nothing touches a device before the checks pass.
 * One kernel form ("sensor_sse.rows64" in sea_last_form): 64 members per workgroup.
 * (An addition to ABI version 8.  sea_struct_sizes() keeps its 33 entries, SeaKvFork last: sizeof(SeaDecodeSensorSse) is 112.)
 */
typedef struct {
    const float* obs;        /* f32 [Bm / members, K_pad] through ld_obs, sorted and padded */
    const float* prec;       /* f32 [K_pad] (ld_prec 0) or [Bm / members, K_pad] through ld_prec, or NULL (1) */
    const int32_t* live;     /* int32 [K_pad]: 1 a sensor, 0 a pad entry */
    const int32_t* wrow;     /* int32 [K_pad]: row of the group's W2 */
    const int32_t* seg;      /* int32 [n_groups, Q + 1] */
    float* wsse;             /* f32 [Bm] (output) */
    float* pred;             /* f32 [Bm, K_pad] (output) or NULL */
    float* work;             /* f32 [work_cap] workspace */
    int64_t ld_obs, ld_prec, work_cap;
    int32_t Bm, members, S, Cp, Q, K_pad;
} SeaDecodeSensorSse;
int sea_decode_sensor_sse(const SeaDecodeMseGroup* groups, int n_groups, const SeaDecodeSensorSse* p, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * The sparse-sensor score WITH its gradient to the hidden rows of the observed patches, in one launch for all field groups (plus the finish launch of
 * sea_decode_sensor_sse): what nudging, 3D-Var corrections, gradient moves of resampled duplicates and sensor terms of a training loss need.  It
 * replaces Decode.forward under autograd, a gather of K values and the backward of an [M, n_fields * Cp] output gradient that is zero outside K
 * columns of the observed patches (reference models/encoder_decoder.py: the decoder MLP's second Linear and its backward, run over all P patches).
 * Tables, obs, prec, live, wrow, seg, wsse, pred, work and the SeaDecodeMseGroup operands H, W2, bias, ldh, ldw, n_fields are those of
 * sea_decode_sensor_sse; dH and lddh are OUTPUT; Z and ldz are nullable and read.  H, Z and dH are [Q * Bm, S], patch-major: row q * Bm + bm.  For sorted
 * position k of group g in observed patch q, member bm of history b = bm / members:
 *     y[bm, k]   = sum_s H_g[q * Bm + bm, s] W2_g[wrow[k], s] + bias_g[wrow[k]]                       (fp32 accumulation, as sea_decode_sensor_sse)
 *     w          = live[k] != 0 and prec[b * ld_prec + k] > 0 ? prec[b * ld_prec + k] : 0              (prec == NULL: 1)
 *     d          = w > 0 ? y[bm, k] - obs[b * ld_obs + k] : 0          (a select: NaN / Inf in obs is neutral without weight)
 *     wsse[bm]   = sum_k (w d) d                                        (fp32; the same order as sea_decode_sensor_sse)
 *     pred[bm * K_pad + k] = y[bm, k]                                   (when pred != NULL)
 *     r          = act(w d)                                             (rounded ONCE between the two products, as sea_decode_mse rounds its residual)
 *     dH_g[q * Bm + bm, s] = 2 grad_scale * sum_{k in segment (g, q), ascending} r[bm, k] W2_g[wrow[k], s]     [* gelu_erf'(Z_g[q * Bm + bm, s]) when Z != NULL]
 * dH is written in the act dtype; EVERY element of rows [0, Q * Bm) by columns [0, S) is written, the rows of an empty (group, patch) segment as exact
 * zeros.  One writer per dH element, no atomics, the tiles of a segment accumulated in ascending order: two runs give the same bits, and a member's dH
 * rows and score do not depend on `members`, on the number of histories or on the row tile the member falls into.  wsse and pred equal what
 * sea_decode_sensor_sse writes for the same operands bit for bit (the same accumulator layout, per-lane order, butterfly and finish launch).
 * The kernel TRUSTS wrow and seg exactly as sea_decode_sensor_sse does: the caller range-checks them on the host before the upload (SensorSet).
 * Requirements: those of sea_decode_sensor_sse — and per group dH non-NULL and 16-byte aligned, lddh a multiple of 8 and >= S; Z NULL, or 16-byte
 * aligned with ldz a multiple of 8 and >= S; grad_scale finite.  SEA_F32 returns SEA_EUNSUPPORTED; so does S > 640.
 * Returns -1, with the entry point and the offending group named in sea_last_error(), otherwise; nothing touches a device before the checks pass.
 * One kernel form ("sensor_grad.rows64" in sea_last_form): 64 members per workgroup, 4 waves of 16 members, SP / 8 fragment registers and SP / 4 fp32
 * dH accumulators per lane (sea_amd/csrc/decode_loss.hip).
 * (An addition to ABI version 8.  sea_struct_sizes() keeps its 33 entries, SeaKvFork last: sizeof(SeaDecodeSensorGrad) is 120.)
 */
typedef struct {
    const float* obs;        /* as SeaDecodeSensorSse */
    const float* prec;
    const int32_t* live;
    const int32_t* wrow;
    const int32_t* seg;
    float* wsse;             /* f32 [Bm] (output) */
    float* pred;             /* f32 [Bm, K_pad] (output) or NULL */
    float* work;             /* f32 [work_cap] workspace, >= Q * n_groups * Bm */
    int64_t ld_obs, ld_prec, work_cap;
    int32_t Bm, members, S, Cp, Q, K_pad;
    float grad_scale;        /* dH = 2 grad_scale * (...) */
    int32_t pad_;
} SeaDecodeSensorGrad;
int sea_decode_sensor_grad(const SeaDecodeMseGroup* groups, int n_groups, const SeaDecodeSensorGrad* p, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * The DENSE-snapshot score with a per-cell precision map and per-field precisions, per member and field, WITH its gradient to the hidden rows, in one
 * launch for all field groups (plus the finish launch of sea_decode_member_sse): what a particle filter's weights, nudging of members and the pull of
 * a single trajectory towards a GAPPY snapshot need (a PIV frame with masked regions, a field known on some cells only).  It replaces Decode.forward
 * under autograd, the weighted reductions over its [M, n_fields * Cp] output and the backward through an output gradient of that size; neither the
 * decoded fields nor the residual ever exist in memory.  Group operands H, W2, bias, ldh, ldw, n_fields, field0 as in sea_decode_mse; dH and lddh are
 * OUTPUT; Z and ldz are nullable and read, as in sea_decode_mse.  Rows as in sea_decode_member_sse: row m belongs to member m / P and patch m % P, and
 * the `members` consecutive members of one history share one observation: trow(m) = ((m / P) / members) * P + m % P.  Per group, j < n_fields, c < C,
 * f = field0 + j:
 *     Y[m, j, c]      = sum_s H[m, s] W2[j Cp + c, s] + bias[j Cp + c]                                      (fp32 accumulation)
 *     pw              = prec == NULL ? 1 : prec[trow(m), f, c];      fw = field_prec == NULL ? 1 : field_prec[f]
 *     w               = valid(m, c) && pw > 0 && fw > 0 ? fw * pw : 0                   (selects: NaN, a negative value, Inf * 0 give 0)
 *     d               = w > 0 ? Y[m, j, c] - obs[trow(m), f, c] : 0                     (a select: NaN / Inf in obs is neutral without weight)
 *     wsse[m / P, f]  = sum over the member's P rows and c of (w d) d                   (f32 [M / P, n_fields_total], every element written)
 *     r               = act(w d)                                                       (rounded ONCE between the two products, as sea_decode_mse rounds its residual)
 *     dH[m, s]        = 2 grad_scale * sum_{j, c} r[m, j, c] W2[j Cp + c, s]   [* gelu_erf'(Z[m, s]) when Z != NULL]          (written in the act dtype)
 * valid(m, c) and the clamping of counts are exactly those of sea_decode_mse (c < C when counts == NULL, else c < counts[m % P], clamped to [0, C]).
 * obs element (r, f, c) is at obs + r ld_row + f ld_field + c; prec, when given, is an f32 map with the SAME strides; only c < C is ever read of
 * either.  field_prec: device f32 [n_fields_total] or NULL.  A row without a weighted cell gets dH = 0 exactly.
 * dH is all-or-nothing: with dH == NULL in EVERY group the launch is score-only (the second product is compiled out; Z, lddh, ldz are not read) and
 * wsse has the bits of the gradient launch; NULL in some groups but not all is refused.
 * work: f32 workspace of work_cap >= M * n_fields_total floats, private to the call: the main kernel writes the per-row, per-field sums there when the
 * tile walk crosses a field boundary (the four lanes that hold a row's columns folded first, as sea_decode_member_sse does), the finish launch adds
 * the P rows of a member.  One writer per dH and wsse element, no atomics: two runs give the same bits, and a member's dH rows and wsse row do not
 * depend on `members`, on the number of histories or on the 64-row tile the member falls into.
 * Requirements: dtype SEA_BF16 (SEA_F32 returns SEA_EUNSUPPORTED); M >= 1; S a multiple of 8, at most 640 (above: SEA_EUNSUPPORTED), padded by
 * masking; Cp a multiple of 32, 1 <= C <= Cp; P >= 1, members >= 1, M % (P * members) == 0; ld_row, ld_field multiples of 4; obs, prec 16-byte,
 * field_prec, counts, wsse, work 4-byte aligned; per group H, W2, bias non-NULL and 16-byte aligned, ldh, ldw multiples of 8 and >= S; with dH: dH
 * (and Z, when given) 16-byte aligned, lddh even and >= S, ldz >= S; the groups' field ranges cover 0 .. n_fields_total-1 exactly once;
 * grad_scale finite; 1 <= n_groups <= SEA_DECODE_MSE_MAX_GROUPS.
 * Returns -1, with the entry point and the offending group named in sea_last_error(), otherwise; nothing touches a device before the checks pass.
 * One kernel form ("field_grad.rows64" in sea_last_form; a = 1 with the gradient, 0 score-only): 64 rows per workgroup, 4 waves of 16 rows, SP / 8
 * fragment registers and, with the gradient, SP / 4 fp32 dH accumulators per lane; every SP in {128, 256, 384, 512, 640} compiles without scratch
 * (DESIGN.md section 7m has the register table), so S up to 640 is served as by sea_decode_mse.
 * (An addition to ABI version 8.  sea_struct_sizes() keeps its 33 entries, SeaKvFork last: sizeof(SeaDecodeFieldGrad) is 104.)
 */
typedef struct {
    const float* obs;          /* f32, rows of the observation: [M / (P * members) * P, n_fields_total, >= C] through ld_row, ld_field */
    const float* prec;         /* f32 map with obs's strides, or NULL (1) */
    const float* field_prec;   /* f32 [n_fields_total], or NULL (1) */
    const int32_t* counts;     /* device int32 [P] or NULL */
    float* wsse;               /* f32 [M / P, n_fields_total] (output) */
    float* work;               /* f32 [work_cap] workspace, >= M * n_fields_total */
    int64_t ld_row, ld_field, work_cap;
    int32_t M, S, C, Cp, P, members, n_fields_total;
    float grad_scale;          /* dH = 2 grad_scale * (...) */
} SeaDecodeFieldGrad;        /* 104 bytes */
int sea_decode_field_grad(const SeaDecodeMseGroup* groups, int n_groups, const SeaDecodeFieldGrad* p, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Systematic resampling of an ensemble, gated by the effective sample size, in one launch: log-weights in, the int32 device index that
 * sea_kv_cache_gather (RolloutSession.resample / select) takes out.  G histories with n members each, one workgroup per history, all sums in fp64.
 * Per history g (member j is element g n + j):
 *     a member is DEAD when its log-weight is NaN, +inf or -inf: its weight is 0 and it is never selected;
 *     mx = max over the live members;  w_j = exp(logw_j - mx);  W = sum_j w_j;  c_i = sum_{k <= i} w_k;  ess = W^2 / sum_j w_j^2
 *     no live member:                       index = identity (g n + j), logw_out = 0, ess = 0, resampled = -1
 *     ess_frac < 0 or ess < ess_frac * n:   index[g n + j] = g n + min{ i : c_i > (j + u_g) / n * W } (clamped to the last live member),
 *                                           logw_out = 0, resampled = 1
 *     otherwise:                            index = identity, logw_out_j = logw_j - mx - log W (dead members: -inf), resampled = 0
 * Indices never leave their history; within one they are non-decreasing and member i appears floor(n p_i) or ceil(n p_i) times (p_i = w_i / W).
 * logw f32 [G n]; u f32 [G], offsets in [0, 1); index int32 [G n]; logw_out f32 [G n]; ess f32 [G]; resampled int32 [G] — all on the device, all
 * non-NULL.  The cumulative sum has a fixed order (fp64, in LDS): two runs give the same bits.  The decision is taken on the device: nothing is read
 * back.  Requirements: G >= 1; 1 <= n <= 4096 (above: SEA_EUNSUPPORTED); G n < 2^31; ess_frac not NaN.  Returns -1 with the entry point named in
 * sea_last_error() otherwise, before any device is touched.  (An addition to ABI version 8; no new struct.)
 */
int sea_resample_systematic(const float* logw, const float* u, float ess_frac, int G, int n, int32_t* index, float* logw_out, float* ess, int32_t* resampled,
                            void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Ensemble Kalman analysis from sensor readings, in ensemble space, in two launches (the deterministic EnKF of Sakov & Oke 2008; no random numbers).
 * B histories with N members each (member j of history b is row b N + j), K sensors, Ld analysis domains.  sea_enkf_transform turns the members'
 * predictions into one [N, N] matrix D per (history, domain); sea_ensemble_mix applies it to the latent states.  Per history b and domain d:
 *     w_k    = (prec_k > 0 ? prec_k : 0) * (taper[d, k] > 0 ? taper[d, k] : 0)     selects: a reading without weight is neutral whatever obs holds
 *                                                                                  there, NaN and Inf included (prec NULL: 1; taper NULL: 1, Ld = 1)
 *     ybar_k = mean_j pred[j, k]
 *     S[j,k] = rho (pred[j, k] - ybar_k) sqrt(w_k / (N - 1))                       0 where w_k = 0, by a select
 *     dl_k   = sqrt(w_k) (obs_k - ybar_k)                                          0 where w_k = 0, by a select
 *     C = S S^T [N, N],  v = S dl [N],  W = (I + C)^-1                             fp64 throughout; I + C is SPD with eigenvalues >= 1: Cholesky
 *                                                                                  without pivoting, then the inverse in LAPACK's potrf, trtri, lauum order
 *     G = (W v) 1^T / sqrt(N - 1) - alpha (I - W)
 *     D = (rho - 1) Pi + rho Pi G,  Pi = I - 1 1^T / N                             Pi G: G with every column's mean over i removed
 * and the analysed state of member j is y[j] + sum_i D[i, j] y[i] per latent element: its member mean is xbar + K (obs - H xbar) and its anomalies
 * are A - alpha K H A, K the ensemble Kalman gain of the rho-inflated forecast.  Without a live reading and with rho = 1, D is exactly 0.
 * D f32 [B, Ld, N, N] and status int32 [B, Ld] are written in full: status = the number of live sensors (w_k > 0), or -1 when a live operand is not
 * finite or a pivot is not a positive finite number — D is then all zeros for that problem (no update).  One workgroup per (domain, history), every
 * sum in a fixed order given by (N, K) alone: two runs give the same bits, and a problem's bits do not depend on the other problems of the launch.
 * Requirements: pred, obs, D, status non-NULL, 4-byte aligned; B in 1 .. 65535; N >= 2 (above 128: SEA_EUNSUPPORTED); K >= 1; Ld >= 1, Ld = 1 without
 * a taper; ld_pred, ld_obs, ld_taper >= K; ld_prec = 0 (one row [K] for all histories) or >= K; rho finite and >= 1; alpha in [0, 1].  Returns -1 with
 * the entry point named in sea_last_error() otherwise, before any device is touched.  Notes the form "enkf.transform" (a = the register block edge
 * 1, 2, 4 or 8; b = the dynamic LDS bytes).  (An addition to ABI version 8; the struct is not in sea_struct_sizes().)
 */
typedef struct {
    const float* pred;       /* f32 [B N, ld_pred]: pred[b N + j, k], the decoded value of member j at sensor k (Decode.sensor_sse's predictions) */
    const float* obs;        /* f32 [B, ld_obs] */
    const float* prec;       /* NULL (1), f32 [K] (ld_prec = 0) or f32 [B, ld_prec] */
    const float* taper;      /* NULL (1; Ld = 1) or f32 [Ld, ld_taper] */
    float* D;                /* f32 [B, Ld, N, N] */
    int32_t* status;         /* int32 [B, Ld] */
    int64_t ld_pred, ld_obs, ld_prec, ld_taper;
    double rho, alpha;
    int32_t B, N, K, Ld;
} SeaEnkfTransform;          /* 112 bytes */
int sea_enkf_transform(const SeaEnkfTransform* p, void* stream);

/* The second form of the transform: the same analysis from Q partial Gram matrices per history — sea_decode_member_gram's gram, proj and count with
 * Q = P, one partial per patch — and an optional f32 taper [Ld, ld_taper] over the partials (NULL: all ones, Ld = 1).  Per (history b, domain d), with
 * t_q = taper[d, q] > 0 ? taper[d, q] : 0:
 *     C = rho^2 / (N - 1) sum_q t_q gram[b, q]        v = rho / sqrt(N - 1) sum_q t_q proj[b, q]          q ascending, fp64
 *     status = sum_{t_q > 0} count[b, q], or -1 if a contributing count is -1 or C, v or a pivot is not finite (then D = 0 for that problem alone)
 * A partial with t_q = 0 or count 0 is passed over by the whole workgroup.  From I + C on, the analysis is sea_enkf_transform's, by the same code:
 * potrf -> trtri -> lauum in one LDS image, then G and D; D f32 [B, Ld, N, N] and status int32 [B, Ld] are written in full.  By construction D equals
 * sea_enkf_transform's D for "every valid cell is a sensor with precision w and taper T[d, patch(k)]".  Without a live cell and with rho = 1, D is
 * exactly 0.  One workgroup per (domain, history); two runs give the same bits, and a problem's bits do not depend on the other problems.
 * Requirements: gram, proj (8-byte aligned), count, D, status non-NULL; B in 1 .. 65535; N >= 2 (above 128: SEA_EUNSUPPORTED); Q >= 1; Ld >= 1, Ld = 1
 * without a taper; ld_taper >= Q; rho finite and >= 1; alpha in [0, 1].  Returns -1 with the entry point named in sea_last_error() otherwise, before any
 * device is touched.  Notes the form "enkf.transform_gram" (a = the register block edge, b = the dynamic LDS bytes).  (An addition to ABI version 8; the
 * struct is not in sea_struct_sizes().)
 */
typedef struct {
    const double* gram;      /* f64 [B, Q, N, N] */
    const double* proj;      /* f64 [B, Q, N] */
    const int32_t* count;    /* int32 [B, Q] */
    const float* taper;      /* NULL (1; Ld = 1) or f32 [Ld, ld_taper] */
    float* D;                /* f32 [B, Ld, N, N] */
    int32_t* status;         /* int32 [B, Ld] */
    int64_t ld_taper;
    double rho, alpha;
    int32_t B, N, Q, Ld;
} SeaEnkfTransformGram;      /* 88 bytes */
int sea_enkf_transform_gram(const SeaEnkfTransformGram* p, void* stream);

/* out[b N + j, g, p, :] = y[b N + j, g, p, :] + sum_i D[b, dom(p), i, j] y[b N + i, g, p, :], dom(p) = 0 when Ld = 1 and p when Ld = P.
 * y act [Bm, G, P Dl] (contiguous; what RolloutSession.step returns), D f32 [Bm / N, Ld, N, N]; the sum is accumulated in fp32 over i in ascending
 * order, one writer per element.  inc (f32, same shape, may be NULL) receives the sum alone; out (act, may be NULL) receives y + inc rounded to the
 * act dtype — exactly that: with D = 0, out has the bits of y.  At least one of out and inc is required; out must not overlap y.  Requirements:
 * N >= 2 (above 128: SEA_EUNSUPPORTED), Bm a multiple of N with at most 65535 histories, G, P, Dl >= 1, Ld 1 or P.  Returns -1 with the entry point
 * named in sea_last_error() otherwise, before any device is touched.  Notes the form "enkf.mix_bf16" / "enkf.mix_f32" (a = 1 with P domains).
 * (An addition to ABI version 8; the struct is not in sea_struct_sizes().)
 */
typedef struct {
    const void* y;
    const float* D;
    void* out;
    float* inc;
    int32_t Bm, N, G, P, Dl, Ld;
} SeaEnsembleMix;            /* 56 bytes */
int sea_ensemble_mix(const SeaEnsembleMix* p, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Verification of an ensemble against sensor readings, in two launches: CRPS, rank, PIT, mean and spread per (history, sensor), and per history
 * the fp64 sums and the rank histogram that calibration is read from.  B histories with N members each (member j of history b is row b N + j), K
 * sensors; pred, obs and prec as for sea_enkf_transform (the same selects).  Per history b, in fp64:
 *     logw NULL: lw_j = 0.  A member with lw_j = -inf is DEAD: weight 0, not counted in ranks; every other member is live (L of them).
 *     mx = max_j lw_j;  e_j = exp(lw_j - mx) (dead: 0);  W = sum_j e_j;  w_j = e_j / W;  q = sum_j w_j^2          (sums over j ascending)
 *     c = unbiased ? 1 - q : 1                        (N / (N - 1) scaling for equal weights; c <= 0 — one member carries all weight — is handled by selects)
 *     status[b] = L, or -1 when a lw_j is NaN or +inf or none is finite: all per-sensor floats of the history are then 0, its ranks -1, and it adds
 *     nothing to sums and hist.
 * Per sensor k of history b, with y = obs[b, k], x_j = pred[b N + j, k] over the live members, p = prec[b, k] (NULL: 1):
 *     DEAD reading (not p > 0):  mean = spread = crps = pit = 0, rank = -1, whatever obs and pred hold there (NaN, Inf, 3e38 included)
 *     BAD sensor (live, and y, p or a live member's x_j is not finite): the four floats are NaN, rank = -2; counted in sums[6], left out of every other sum
 *     mean   = sum_j w_j x_j
 *     spread = c > 0 ? sqrt(sum_j w_j (x_j - mean)^2 / c) : 0
 *     crps   = sum_j w_j |x_j - y| - (c > 0 ? (1 / (2 c)) sum_i sum_j w_i w_j |x_i - x_j| : 0)                (unbiased: the fair CRPS)
 *              the double sum is evaluated as 2 sum_i w_i (x_i - y) (2 Wb_i + w_i - 1), Wb_i = sum_j w_j [(x_j, j) < (x_i, i)] accumulated over j
 *              ascending: the weight below member i under the total order (value, member index) — no sort, ties and zero weights included
 *     pit    = sum_j w_j [x_j < y] + 0.5 sum_j w_j [x_j == y]
 *     rank   = the number of live members with x_j < y                                                        (int32, 0 .. L)
 * Per history, over its live, good sensors in ascending k, from the fp64 per-sensor values before they are rounded to fp32:
 *     sums[b, 0..7] = count, sum crps, sum (y - mean)^2, sum spread^2, sum (y - mean)^2 / (spread^2 + 1 / p), sum (mean - y), count of bad sensors,
 *                     sum 1 / p                        (f64)
 *     hist[b, r]    = the number of those sensors with rank r, r = 0 .. N                                      (int64 [B, N + 1])
 * accumulate = 1 adds a call's sums and hist into the existing ones (one writer per element); 0 overwrites them.  status is always overwritten.
 * mean, spread, crps, pit f32 [B, ld_out] and rank int32 [B, ld_out] may each be NULL; every element [b, k < K] of the others is written.
 * Launch 1: a workgroup per (tile of 16 sensors, history): the tile's predictions are staged in LDS as [sensor][member], a wave takes a sensor at a
 * time with a member (two above 64 members) per lane, the lane sums are reduced by a fixed butterfly, thread k writes sensor k, and the tile's fp64
 * partial sums (sensors ascending) and its partial histogram go to `work`.  Launch 2: a workgroup per history adds the tiles in ascending order.
 * No atomics to global memory: two runs give the same bits; a history's outputs are those of a launch holding it alone; a sensor's own outputs do
 * not depend on K, on its place in a tile or on the other sensors.
 * Requirements: pred, obs, sums, hist, status, work non-NULL; f32 / int32 buffers 4-byte, sums, hist and work 8-byte aligned; B in 1 .. 65535;
 * N >= 1 (above 128: SEA_EUNSUPPORTED); K >= 1; ld_pred, ld_obs, ld_out >= K; ld_prec = 0 (one row [K] for all histories) or >= K; unbiased and
 * accumulate 0 or 1; work_bytes >= sea_ensemble_verify_ws_bytes(B, N, K) (the workspace is private to the call until it has run).  Returns -1 with
 * the entry point named in sea_last_error() otherwise, before any device is touched.  Notes the form "verify" (a = members per lane, 1 or 2; b =
 * the dynamic LDS bytes).  (An addition to ABI version 8; the struct is not in sea_struct_sizes().)
 */
typedef struct {
    const float* pred;       /* f32 [B N, ld_pred] */
    const float* obs;        /* f32 [B, ld_obs] */
    const float* prec;       /* NULL (1), f32 [K] (ld_prec = 0) or f32 [B, ld_prec] */
    const float* logw;       /* NULL (equal weights) or f32 [B N], unnormalised */
    float* mean;             /* f32 [B, ld_out] or NULL */
    float* spread;
    float* crps;
    float* pit;
    int32_t* rank;           /* int32 [B, ld_out] or NULL */
    double* sums;            /* f64 [B, 8] */
    int64_t* hist;           /* int64 [B, N + 1] */
    int32_t* status;         /* int32 [B] */
    void* work;              /* work_bytes bytes */
    int64_t ld_pred, ld_obs, ld_prec, ld_out, work_bytes;
    int32_t B, N, K, unbiased, accumulate, pad_;
} SeaEnsembleVerify;         /* 168 bytes */
int64_t sea_ensemble_verify_ws_bytes(int B, int N, int K);   /* -1 for sizes the entry point refuses */
int sea_ensemble_verify(const SeaEnsembleVerify* p, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Verification of an ensemble against a DENSE observation of the decoded fields, in two launches: sea_ensemble_verify's scores with every cell of
 * the mesh a reading, without the members' decoded fields or a prediction matrix ever existing in memory.  Operands H, W2, bias, ldh, ldw,
 * n_fields, field0 of SeaDecodeMseGroup, and obs, prec_field, prec, counts with their strides, exactly as in sea_decode_member_gram; row
 * m = (b * members + j) * P + p of H is member j of history b; B = M / (P * members); N = members; F = n_fields_total.  Per history b and patch p:
 *     y_j[f, c] = sum_s H[m, s] W2[(f - field0) Cp + c, s] + bias[(f - field0) Cp + c]                       (fp32 accumulation; never stored)
 *     w[f, c]   = valid(p, c) ? (pf[f] > 0 ? pf[f] : 0) * (prec != NULL ? (prec[b, p, f, c] > 0 ? prec[b, p, f, c] : 0) : 1) : 0    (an fp32 product)
 *                 selects: a NaN counts as 0; pf = prec_field (NULL: 1); valid(p, c) = c < counts[p] (clamped to [0, C]; NULL: c < C)
 * The history's weights, status[b] and c come from logw and unbiased as in sea_ensemble_verify.  A cell with w > 0 is a live reading with
 * x_j = y_j[f, c] (compared as the f32 values they are), y = obs[b, p, f, c] and precision w; mean, spread, crps, pit and rank are
 * sea_ensemble_verify's, evaluated by the same device code in fp64.  A cell without weight is DEAD: the four floats 0, rank -1, and obs is not read
 * there.  A live cell whose y, w or a live member's value is not finite is BAD: the four floats NaN, rank -2.  A history whose log-weights are
 * invalid (status -1) has all its maps 0, its ranks -1, and adds nothing to sums and hist.
 *     mean, spread, crps, pit f32 and rank int32 [B, P, F, ld_out]: each may be NULL; EVERY element of the others is written, the columns from C
 *                             (and from counts[p]) up to ld_out as dead cells
 *     sums[b, f, 0..7]        sea_ensemble_verify's eight sums over the live, good cells of field f of history b, patches ascending, columns
 *                             ascending inside a patch, from the fp64 per-cell values before any rounding (entry 3 adds spread^2)          (f64 [B, F, 8])
 *     hist[b, f, r]           the number of those cells with rank r, r = 0 .. N                                                            (int64 [B, F, N + 1])
 *     status[b]               the number of live members, or -1                                                                            (int32 [B])
 * accumulate = 1 adds a call's sums and hist onto the existing ones; 0 overwrites them.  status is always overwritten.
 * Launch 1: a workgroup of 8 waves per (history, patch, field, chunk of 512 columns) decodes 32 columns of its field at a time as
 * sea_decode_member_gram does, stages the values in LDS as [column][member], a wave scores a column at a time with a member (two above 64) per lane,
 * thread k stores column k, and the workgroup's partial sums (columns ascending) and partial histogram (integer LDS adds) go to `work`.  Launch 2: a
 * workgroup per history adds the partials in ascending (patch, chunk) order.  No floating-point atomics: two runs give the same bits; a history's outputs are those of a call holding it alone; a
 * cell's own outputs do not depend on the other cells of its patch.
 * Requirements: dtype SEA_BF16 (SEA_F32: SEA_EUNSUPPORTED); M >= 1; S a multiple of 8, at most 640 (above: SEA_EUNSUPPORTED), padded by masking; Cp a
 * multiple of 32, 1 <= C <= Cp; P >= 1; members >= 1 (above 128: SEA_EUNSUPPORTED); M % (P * members) == 0; at most 65535 histories and fields; ld_field,
 * ld_pfield >= C, and ld_out >= C when a map is given; f32 and int32 buffers 4-byte, sums, hist and work 8-byte aligned; unbiased and accumulate 0 or
 * 1; work_bytes >= sea_decode_member_verify_ws_bytes(B, P, F, members, Cp); per group H, W2, bias non-NULL and 16-byte aligned, ldh, ldw multiples of 8
 * and >= S; the groups' field ranges cover 0 .. F-1 exactly once; 1 <= n_groups <= SEA_DECODE_MSE_MAX_GROUPS.  Returns -1, with the entry point and
 * the offending group named in sea_last_error(), otherwise; nothing touches a device before the checks pass.
 * Notes the form "decode.member_verify" (a = the padded hidden width, b = the dynamic LDS bytes).
 * (An addition to ABI version 8.  The struct is not in sea_struct_sizes(): sizeof(SeaDecodeMemberVerify) is 200.)
 */
typedef struct {
    const float* obs;          /* f32, rows of the observation: [B * P, F, >= C] through ld_row, ld_field */
    const float* prec_field;   /* f32 [F], or NULL (1) */
    const float* prec;         /* f32 map in obs's layout through ld_prow, ld_pfield, or NULL (1) */
    const int32_t* counts;     /* device int32 [P] or NULL */
    const float* logw;         /* NULL (equal weights) or f32 [B N], unnormalised */
    float* mean;               /* f32 [B, P, F, ld_out] or NULL */
    float* spread;
    float* crps;
    float* pit;
    int32_t* rank;             /* int32 [B, P, F, ld_out] or NULL */
    double* sums;              /* f64 [B, F, 8] */
    int64_t* hist;             /* int64 [B, F, N + 1] */
    int32_t* status;           /* int32 [B] */
    void* work;                /* work_bytes bytes */
    int64_t ld_row, ld_field, ld_prow, ld_pfield, ld_out, work_bytes;
    int32_t M, S, C, Cp, P, members, n_fields_total, unbiased, accumulate, pad_;
} SeaDecodeMemberVerify;     /* 200 bytes */
int64_t sea_decode_member_verify_ws_bytes(int B, int P, int n_fields_total, int members, int Cp);   /* -1 for sizes the entry point refuses */
int sea_decode_member_verify(const SeaDecodeMseGroup* groups, int n_groups, const SeaDecodeMemberVerify* p, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * The CRPS of the decoded fields as a LOSS: per (history, field) the sum of the cells' CRPS, WITH its gradient to the hidden rows, in two launches,
 * without the members' decoded fields or their gradient ever existing in memory.  Operands, rows, groups, counts, prec_field, prec, logw, unbiased,
 * the decode, the cells' weights, the history's weights w_m, status[b] and c exactly as in sea_decode_member_verify; the groups also carry dH (the
 * output, act [M, >= S] through lddh) and optionally Z (the pre-activation, through ldz).  For one live, good cell with member values x_m (the f32
 * decoded values), reading y, q = sum_m w_m^2, c = unbiased ? 1 - q : 1 and below_m the weight of the members below m under the order (value, member
 * index):
 *     crps  = sum_m w_m |x_m - y|  -  (1 / c) sum_m w_m (x_m - y) (2 below_m + w_m - 1)                  (sea_ensemble_verify's, the same device code)
 *     G[m]  = d crps / d x_m = w_m (sign(x_m - y) - (2 below_m + w_m - 1) / c)       sign(0) = 0;  c <= 0: the second term is 0      (fp64)
 * away from ties the derivative, at ties the subgradient that the order selects.  G = 0 exactly, by selects (whatever obs holds, NaN included),
 * for a dead member (logw = -inf), a dead cell (no weight), a bad cell (a non-finite live member value, reading or weight: counted in sums[.., 6])
 * and a history that is not scored (status -1).  With fw = field_weight (NULL: 1; a value that is not positive counts as 0):
 *     sums[b, f, 0..7]   sea_decode_member_verify's eight fp64 sums, with that launch's BITS for the same operands                  (f64 [B, F, 8])
 *     loss[b, f]         float(fw[f] * sums[b, f, 1])                                                                                (f32 [B, F])
 *     dH[m, s]           sum over the fields j of the group and their cells c of (g0 + g1) * W2[j Cp + c, s]  [* gelu_erf'(Z[m, s])]  with
 *                        g = float(fw[f] G[m, j, c]) (formed in fp64), g0 = bf16(g) — g rounded to bf16 ONCE, the A operand of the second product as
 *                        sea_decode_mse rounds its residual — and g1 = bf16(g - g0), what that rounding left, as a second A operand against the same
 *                        W2 tile (g1 = 0 wherever g is a bf16 value: the result is then the one-term product's, bit for bit; elsewhere the operand
 *                        carries 16 bits, so that a row with ONE live cell is not 2^-8 off); fp32 accumulation, the g0 product first; rounded once
 *                        to the act dtype.  Every element of dH [M, S] is written.
 *     status[b]          the number of live members, or -1                                                                           (int32 [B])
 * Launch 1 has sea_decode_member_verify's grid — a workgroup per (history, patch, field, chunk of 512 columns) — and its walk; the scoring lanes
 * place G in LDS as two [member][32 columns] bf16 fragments (g0, g1) and the wave that decoded members 16 w .. 16 w + 15 multiplies it against the same LDS
 * image of the W2 tile into its [16, S] fp32 slice of dH, which goes to the workgroup's private partial in `work`.  Launch 2 adds a row's partials
 * in ascending (field, chunk) order and the sums in ascending (patch, chunk) order.  No floating-point atomics, one writer per element: two runs
 * give the same bits, and a history's outputs are those of a call holding it alone.
 * Requirements: those of sea_decode_member_verify (without maps, hist and accumulate), and per group dH non-NULL, dH and Z 16-byte aligned, lddh and
 * ldz >= S; loss and field_weight 4-byte aligned; work_bytes >= sea_decode_member_crps_grad_ws_bytes(B, P, F, members, Cp, S), which is
 * B P F ceil(Cp / 512) (64 + 4 members S) bytes.  members above 64 at S above 384 returns SEA_EUNSUPPORTED with a message (the dH slice and the
 * two-member fp64 walk do not fit the register file without scratch), as do SEA_F32, S above 640 and members above 128.  Returns -1, with the entry
 * point and the offending group named in sea_last_error(), for anything else; nothing touches a device before the checks pass.
 * Notes the form "decode.member_crps_grad.w8" (8 waves; members above 64, or S up to 384) or "decode.member_crps_grad.w4" (4 waves: members up to
 * 64 at S above 384) with a = the padded hidden width, b = the dynamic LDS bytes.
 * (An addition to ABI version 8.  The struct is not in sea_struct_sizes(): sizeof(SeaDecodeMemberCrpsGrad) is 152.)
 */
typedef struct {
    const float* obs;          /* f32, rows of the observation: [B * P, F, >= C] through ld_row, ld_field */
    const float* prec_field;   /* f32 [F], or NULL (1) */
    const float* prec;         /* f32 map in obs's layout through ld_prow, ld_pfield, or NULL (1) */
    const float* field_weight; /* f32 [F], or NULL (1) */
    const int32_t* counts;     /* device int32 [P] or NULL */
    const float* logw;         /* NULL (equal weights) or f32 [B N], unnormalised */
    float* loss;               /* f32 [B, F] */
    double* sums;              /* f64 [B, F, 8] */
    int32_t* status;           /* int32 [B] */
    void* work;                /* work_bytes bytes */
    int64_t ld_row, ld_field, ld_prow, ld_pfield, work_bytes;
    int32_t M, S, C, Cp, P, members, n_fields_total, unbiased;
} SeaDecodeMemberCrpsGrad;   /* 152 bytes */
int64_t sea_decode_member_crps_grad_ws_bytes(int B, int P, int n_fields_total, int members, int Cp, int S);   /* -1 for sizes the entry point refuses */
int sea_decode_member_crps_grad(const SeaDecodeMseGroup* groups, int n_groups, const SeaDecodeMemberCrpsGrad* p, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * sea_decode_member_crps_grad for SMALL ensembles: the same operands, the same struct, the same workspace (sea_decode_member_crps_grad_ws_bytes) and
 * the same outputs — loss, sums, status and every dH have the BITS of sea_decode_member_crps_grad on the same operands — with several histories per
 * workgroup in launch 1.  For 1 .. 32 members, with NP the member count rounded up to a power of two (at least 2): a workgroup serves (a group of HG
 * histories, patch, field, chunk of 512 columns), HG = 64 / NP (16 at NP = 2 above S = 512, where the staging of 32 histories does not fit the LDS
 * beside the 640-wide W2 tile images); slot g NP + i of 64 is member i of the group's history g.  Waves 0 - 3 decode 16 slots each; a wave scores a
 * column of all the group's histories at once (segments of NP lanes: the walk over the lane's own segment, the butterflies stopped at the segment, the
 * reading, its precision, c and the good / bad test per segment) and the second MFMA product runs over the slot rows.  A history that is not scored,
 * and a history index beyond B in the last group, are dead segments by selects.  The unpacked form spends a workgroup — the W2 tile loads, the
 * barriers, 32 wave-passes per tile — on 4 real rows of a 16-row MFMA tile and 4 of 64 scoring lanes at 4 members; this form amortises them over HG
 * histories.  Launch 2 is sea_decode_member_crps_grad's.  Why the bits agree: an MFMA row does not depend on the other rows of its tile; the
 * unpacked butterfly's stages beyond NP add exact +0.0 terms; every per-history chain (weights, q, the column sums) is the same chain.
 * Requirements and messages: those of sea_decode_member_crps_grad, under this entry point's name.  SEA_EUNSUPPORTED with a message for members above 32,
 * SEA_F32 and S above 640; every (S, NP) below that is shipped (none needs scratch).
 * Notes the form "decode.member_crps_grad.pk<NP>" (pk2, pk4, pk8, pk16, pk32: HG = 64 / NP; "pk2h16": NP = 2 with HG = 16) with a = the padded hidden
 * width, b = the dynamic LDS bytes.  8 waves up to S = 384, 4 waves above (the dH slice needs the register file).
 * (An addition to ABI version 8.)
 */
int sea_decode_member_crps_grad_packed(const SeaDecodeMseGroup* groups, int n_groups, const SeaDecodeMemberCrpsGrad* p, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * The forecast products of an ensemble beyond mean and variance: weighted QUANTILE maps (median, a 5 % / 95 % band, the envelope) and EXCEEDANCE
 * probability maps of the decoded fields, in ONE launch, without the members' decoded fields ever existing in memory.  Operands H, W2, bias, ldh, ldw,
 * n_fields, field0 of SeaDecodeMseGroup and the row order exactly as in sea_decode_member_verify: row m = (b * members + j) * P + p of H is member j of
 * history b; B = M / (P * members); F = n_fields_total.
 *     y_j[b, p, f, c] = sum_s H[m, s] W2[(f - field0) Cp + c, s] + bias[(f - field0) Cp + c]        (fp32 accumulation from bf16 MFMAs; never stored;
 *                       compared as the f32 values they are; the decode is sea_decode_member_verify's code: a cell has the bits of the cell it scores)
 * w: f32 [B * members], normalised per history by the caller, as in sea_decode_member_moments; NULL: equal weights (1 each — the definitions below only
 * see ratios of weights).  A member with w <= 0 or NaN is DEAD: it is passed over by selects, and NaN or Inf in its hidden row reaches nothing.
 *     W       = sum of w_j over the live members, in fp64, one chain over j ascending
 *     below_i = sum of w_j over the live j with (y_j, j) < (y_i, i)     for a live member i; fp64, accumulated over j ascending (the walk of
 *               sea_ensemble_verify's CRPS); cum_i = below_i + w_i
 * Weighted quantile at a level tau in [0, 1], the inverted weighted empirical distribution function:
 *     q_tau = min { y_i : i live, cum_i >= tau * W }      both sides fp64, tau * W ONE fp64 product of the f32 level
 *     and the largest live value when no live member qualifies (by rounding, at tau = 1).  tau = 0 gives the smallest live value.  q_tau is the decoded
 *     value of one member bit for bit (an f32 min / max over lanes: the result does not depend on the order); the maps are non-decreasing in tau; with
 *     equal weights this is numpy.quantile(..., method="inverted_cdf").
 * Exceedance probability of a threshold thr[t, f] (f32 [n_thr, F], per field, in the decoder's scaled units):
 *     e_t = (sum of w_i over the live i with y_i > thr[t, f]) / W      strict >; fp64 through a fixed xor butterfly over the lanes; stored as f32
 * Cells: a column at or beyond counts[p] (clamped to [0, C]; NULL: C) up to ld is dead: 0 in every map — EVERY element of quant and exceed is written.
 * A live cell where a live member's value is not finite gives NaN in all its maps and in no other cell.  A history without a live member gives 0
 * everywhere.  A threshold that is NaN gives NaN in that map's live cells.
 *     quant  f32 [n_levels, B * P, F, ld]: level k's map starts at quant + k * ld_map, element (bp, f, c) at (bp * F + f) * ld + c
 *     exceed f32 [n_thr, B * P, F, ld]:    threshold t's map starts at exceed + t * ld_map
 * One launch: a workgroup of 8 waves per (history, patch, field, chunk of 512 columns) — sea_decode_member_verify's grid and walk — decodes 32 columns
 * at a time, stages the values in LDS as [column][member]; a wave reads out a column at a time with a member (two above 64) per lane; thread k stores
 * column k of every map.  The O(N^2) walk for below_i runs only when n_levels > 0 (a branch uniform over the launch).  Nothing is reduced across
 * workgroups and there are no atomics: two runs give the same bits, a history's outputs are those of a call holding it alone, and a cell's outputs
 * depend on its own column only.
 * Requirements: dtype SEA_BF16 (SEA_F32: SEA_EUNSUPPORTED); M >= 1; S a multiple of 8, at most 640 (above: SEA_EUNSUPPORTED), padded by masking; Cp a
 * multiple of 32, 1 <= C <= Cp; P >= 1; members >= 1 (above 128: SEA_EUNSUPPORTED); M % (P * members) == 0; at most 65535 histories and fields;
 * 0 <= n_levels, n_thr <= SEA_QUANTILE_MAX_LEVELS, not both 0; every level finite and in [0, 1]; quant non-NULL when n_levels > 0, thr and exceed
 * non-NULL when n_thr > 0; ld >= C, ld_map >= B * P * F * ld; all f32 and int32 buffers 4-byte aligned; per group H, W2, bias non-NULL and 16-byte
 * aligned, ldh, ldw multiples of 8 and >= S; the groups' field ranges cover 0 .. F-1 exactly once; 1 <= n_groups <= SEA_DECODE_MSE_MAX_GROUPS.
 * Returns -1, with the entry point and the offending group named in sea_last_error(), otherwise; nothing touches a device before the checks pass.
 * Notes the form "decode.member_quantiles" (a = the padded hidden width, b = the dynamic LDS bytes).
 * (An addition to ABI version 8.  The struct is not in sea_struct_sizes(): sizeof(SeaDecodeMemberQuantiles) is 128.)
 */
#define SEA_QUANTILE_MAX_LEVELS 8
typedef struct {
    const float* w;            /* f32 [B * members], or NULL (equal weights) */
    const int32_t* counts;     /* device int32 [P] or NULL */
    const float* thr;          /* f32 [n_thr, F], or NULL when n_thr == 0 */
    float* quant;              /* f32 [n_levels, B * P, F, ld] through ld_map, or NULL when n_levels == 0 */
    float* exceed;             /* f32 [n_thr, B * P, F, ld] through ld_map, or NULL when n_thr == 0 */
    float level[SEA_QUANTILE_MAX_LEVELS];   /* the first n_levels are read */
    int64_t ld, ld_map;        /* floats between two rows of a map, and between two maps */
    int32_t n_levels, n_thr, M, S, C, Cp, P, members, n_fields_total, pad_;
} SeaDecodeMemberQuantiles;  /* 128 bytes */
int sea_decode_member_quantiles(const SeaDecodeMseGroup* groups, int n_groups, const SeaDecodeMemberQuantiles* p, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Verification of EXCEEDANCE forecasts ("the probability that the field is above thr here"): the Brier score, the counts its reliability / resolution /
 * uncertainty decomposition and the reliability diagram are read from, and the hit counts of the ROC curve — for a dense snapshot of the decoded
 * fields (sea_decode_member_brier, two launches, the members' decoded fields never written) and for predictions at sensors that already exist
 * (sea_ensemble_brier, two launches).  Both run the same device code per reading (sea_amd/csrc/brier_score.hpp).
 * Members and weights: per history b, from logw exactly as in sea_ensemble_verify, in fp64: lw_j = 0 when logw is NULL; a member with lw_j = -inf is
 * DEAD; mx = max_j lw_j; e_j = exp(lw_j - mx) (dead: 0); W = sum_j e_j over j ascending; status[b] = L (the live members), or -1 when a lw_j is NaN or
 * +inf or none is finite: the history's maps are then 0 and it adds nothing to sums, hist and hits.
 * Readings: a reading is LIVE, DEAD or BAD exactly as in sea_decode_member_verify (a cell: the weight w[f, c] of that entry point from counts,
 * prec_field and prec, the same selects, a NaN counts as 0) and sea_ensemble_verify (a sensor: p = prec[b, k], NULL: 1; dead when not p > 0).  A live
 * reading whose y, weight or a live member's value is not finite is BAD.  The precision only decides live or dead: no score is weighted by it.  obs is
 * not read at a dead reading.
 * Per live, good reading with members' values x_j (f32, compared as the f32 they are), reading y, and threshold thr (thr[t, f] per field for the
 * dense form, thr[t, k] per sensor for the sensor form; f32; 1 <= n_thr <= 8):
 *     m = #{ live j : x_j > thr }                                     strict; an integer in 0 .. L
 *     p = (sum of e_j over the live j with x_j > thr) / W             fp64: summed first — through the fixed xor butterfly over the lanes that
 *                                                                     sea_decode_member_quantiles uses for its exceedance maps — then divided once.
 *                                                                     With equal weights p = m / L exactly, and the f32 prob map has the bits of that
 *                                                                     launch's exceed map.
 *     o = [ y > thr ]                                                 strict
 *     A NaN threshold makes every comparison false (p = 0, m = 0, o = 0); the Python layer refuses thresholds that are not finite.
 * Per (history, field, threshold) — per (history, threshold) for the sensor form — over the live, good readings in the order
 * sea_decode_member_verify / sea_ensemble_verify add their sums (patches ascending, columns ascending inside a patch; sensors ascending), from the
 * fp64 values before any rounding:
 *     sums[.., t, 0..4] = count, sum (p - o)^2, sum p, sum o, count of BAD readings                                  (f64 [B, F, T, 5] / [B, T, 5])
 *     hist[.., t, m]    = the number of live, good readings with m exceeding members, m = 0 .. N                     (int64 [B, F, T, N + 1] / [B, T, N + 1])
 *     hits[.., t, m]    = the number of those readings with o = 1                                                    (int64, hist's shape)
 * accumulate = 1 adds a call's sums, hist and hits onto the existing ones; 0 overwrites them.  status is always overwritten.
 * Optional per-reading maps, each may be NULL; threshold t's map starts at t * ld_map:
 *     prob  f32 [T, B, P, F, ld_out] (sensor form: [T, B, ld_out])   (float) p
 *     brier f32, the same shape                                      (float) (p - o)^2
 * EVERY element of a given map is written: a dead reading, the columns from C (and from counts[p]) up to ld_out and a history with status -1 give 0, a
 * BAD reading NaN (the sensor form writes [b, k < K]).
 * No floating-point atomics; the histograms are counted with integer adds in LDS.  Two runs give the same bits; a history's outputs are those of a call
 * holding it alone; a reading's own outputs do not depend on the other readings.
 *
 * sea_decode_member_brier: operands H, W2, bias, ldh, ldw, n_fields, field0 of SeaDecodeMseGroup and obs, prec_field, prec, counts with their strides
 * exactly as in sea_decode_member_verify; the row order and the decode are sea_decode_member_quantiles' (the same device functions: a cell has that
 * launch's bits).  Launch 1: that launch's grid in its thresholds-only form — a workgroup of 8 waves per (history, patch, field, chunk of 512 columns),
 * 32 columns decoded at a time and staged in LDS as [column][member], a wave per column at a time with a member (two above 64) per lane — plus
 * sea_decode_member_verify's reads of obs, prec_field, prec and counts; thread (k, t) finishes threshold t of column k; the workgroup's fp64 partial sums
 * (columns ascending) and its integer histograms, sized by the call's n_thr and members, go to `work`.  Launch 2: a workgroup per (history, field,
 * threshold) adds its partials in ascending (patch, chunk) order.
 * Requirements: as sea_decode_member_verify (dtype SEA_BF16, SEA_F32: SEA_EUNSUPPORTED; S a multiple of 8, above 640: SEA_EUNSUPPORTED; members above
 * 128: SEA_EUNSUPPORTED; ...; at most 8191 fields: fields x thresholds is a grid dimension), and 1 <= n_thr <= 8, thr non-NULL, hits non-NULL and 8-byte aligned, ld_out >= C and ld_map >= B * P * F * ld_out when
 * a map is given, work_bytes >= sea_decode_member_brier_ws_bytes(B, P, F, members, Cp, n_thr).  Returns -1 with the entry point named in
 * sea_last_error() otherwise, before any device is touched.  Notes the form "decode.member_brier" (a = the padded hidden width, b = the dynamic LDS
 * bytes).
 * sea_ensemble_brier: pred, obs, prec and logw exactly as in sea_ensemble_verify; thr f32 [n_thr, ld_thr], a threshold per sensor.  Launch 1: a
 * workgroup per (tile of 16 sensors, history), the tile's predictions staged as [sensor][member]; launch 2: a workgroup per (history, threshold) adds the tiles in
 * ascending order.  Requirements as sea_ensemble_verify, and 1 <= n_thr <= 8, ld_thr >= K, ld_map >= B * ld_out when a map is given, work_bytes >=
 * sea_ensemble_brier_ws_bytes(B, N, K, n_thr).  Notes the form "brier" (a = members per lane, 1 or 2; b = the dynamic LDS bytes).
 * (Additions to ABI version 8.  The structs are not in sea_struct_sizes(): sizeof(SeaDecodeMemberBrier) is 200, sizeof(SeaEnsembleBrier) 176.)
 */
#define SEA_BRIER_SUMS 5
typedef struct {
    const float* obs;          /* f32, rows of the observation: [B * P, F, >= C] through ld_row, ld_field */
    const float* prec_field;   /* f32 [F], or NULL (1) */
    const float* prec;         /* f32 map in obs's layout through ld_prow, ld_pfield, or NULL (1) */
    const int32_t* counts;     /* device int32 [P] or NULL */
    const float* logw;         /* NULL (equal weights) or f32 [B N], unnormalised */
    const float* thr;          /* f32 [n_thr, F] */
    float* prob;               /* f32 [n_thr, B, P, F, ld_out] through ld_map, or NULL */
    float* brier;
    double* sums;              /* f64 [B, F, n_thr, 5] */
    int64_t* hist;             /* int64 [B, F, n_thr, N + 1] */
    int64_t* hits;             /* int64 [B, F, n_thr, N + 1] */
    int32_t* status;           /* int32 [B] */
    void* work;                /* work_bytes bytes */
    int64_t ld_row, ld_field, ld_prow, ld_pfield, ld_out, ld_map, work_bytes;
    int32_t M, S, C, Cp, P, members, n_fields_total, n_thr, accumulate, pad_;
} SeaDecodeMemberBrier;      /* 200 bytes */
int64_t sea_decode_member_brier_ws_bytes(int B, int P, int n_fields_total, int members, int Cp, int n_thr);   /* -1 for sizes the entry point refuses */
int sea_decode_member_brier(const SeaDecodeMseGroup* groups, int n_groups, const SeaDecodeMemberBrier* p, int dtype, void* stream);

typedef struct {
    const float* pred;       /* f32 [B N, ld_pred] */
    const float* obs;        /* f32 [B, ld_obs] */
    const float* prec;       /* NULL (1), f32 [K] (ld_prec = 0) or f32 [B, ld_prec] */
    const float* logw;       /* NULL (equal weights) or f32 [B N], unnormalised */
    const float* thr;        /* f32 [n_thr, ld_thr] */
    float* prob;             /* f32 [n_thr, B, ld_out] through ld_map, or NULL */
    float* brier;
    double* sums;            /* f64 [B, n_thr, 5] */
    int64_t* hist;           /* int64 [B, n_thr, N + 1] */
    int64_t* hits;           /* int64 [B, n_thr, N + 1] */
    int32_t* status;         /* int32 [B] */
    void* work;              /* work_bytes bytes */
    int64_t ld_pred, ld_obs, ld_prec, ld_thr, ld_out, ld_map, work_bytes;
    int32_t B, N, K, n_thr, accumulate, pad_;
} SeaEnsembleBrier;          /* 176 bytes */
int64_t sea_ensemble_brier_ws_bytes(int B, int N, int K, int n_thr);   /* -1 for sizes the entry point refuses */
int sea_ensemble_brier(const SeaEnsembleBrier* p, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Quantile, exceedance and Brier maps of DERIVED fields — the speed |u| = sqrt(u^2 + v^2), a kinetic energy, a difference of two fields — of an
 * ensemble, without the members' decoded components or the derived field ever existing in memory.  A quantile of |u| is not a function of the
 * quantiles of u and v: the derived value has to be formed per member, before the read-out.  A derived field d is (op, a, b, scale_a, shift_a,
 * scale_b, shift_b): a != b are SOURCE fields that lie in the same SeaDecodeMseGroup (they share the hidden row and land in the same lane and register
 * of the same accumulator layout); y_a, y_b are the decoded f32 values of member j at one cell, exactly as sea_decode_member_quantiles decodes them
 * (the same sums in the same order).  All arithmetic is f32, every operation rounded ONCE — no fused multiply-add, no reassociation:
 *     a' = y_a * scale_a + shift_a          b' = y_b * scale_b + shift_b          (one multiply, one add each)
 *     SEA_DERIVED_MAGNITUDE   x = sqrt(a' * a' + b' * b')       two products, one add, one CORRECTLY ROUNDED f32 root (the hardware root, one
 *                                                                Newton step, and a choice among the result and its two neighbours by the
 *                                                                sign of two fma residuals; arguments below 2^-96 are scaled by 2^32)
 *     SEA_DERIVED_ENERGY      x = 0.5f * (a' * a' + b' * b')
 *     SEA_DERIVED_DIFFERENCE  x = a' - b'
 * scale and shift carry the mesh's inverse scaling: x is in PHYSICAL units (a magnitude of min-max-scaled components means nothing).  f32 denormals
 * are flushed to zero, as everywhere in this library.
 * From x_j on everything is sea_decode_member_quantiles and sea_decode_member_brier with "field" read as "derived field" — the same device code
 * behind the value image: weights and dead members; below_i, the weighted quantile and the strict exceedance; m, p, o, sums, hist, hits, status; live,
 * dead and bad cells; counts.  A cell where a live member's x is not finite (NaN or Inf in a source, overflow of a square) is NaN (quantiles) or BAD
 * (Brier), as a non-finite decoded value is there.  thr is f32 [n_thr, n_derived], in the derived field's own units.
 * p->n_fields_total stays the number of SOURCE fields (the groups cover them exactly once); every map, thr, obs, prec, prec_field, sums, hist, hits and
 * the workspace have n_derived where the member entry points have F: quant f32 [n_levels, B * P, n_derived, ld], ld_map >= B * P * n_derived * ld;
 * obs [B * P, n_derived, >= C]; sums f64 [B, n_derived, n_thr, 5]; work_bytes >= sea_decode_member_brier_ws_bytes(B, P, n_derived, members, Cp, n_thr).
 * Launches: the member launches' grids with n_derived for F.  Per tile of 32 columns the W2 tiles of source a and of source b go through the SAME two
 * LDS images (the stream a_0, b_0, a_1, b_1, ...; hidden rows loaded once); a wave decodes a's tile into 8 registers, b's tile on top, applies the op per
 * element and stores x to the value image.  sea_decode_derived_brier is followed by sea_decode_member_brier's finish launch.  No workspace (quantiles),
 * no floating-point atomics: two runs give the same bits, a history's outputs are those of a call holding it alone, and a derived field's outputs do not
 * depend on the other derived fields of the call.
 * Returns -1, with the entry point and the offending derived field named in sea_last_error(), before any device is touched, for: n_derived outside
 * 1 .. SEA_DERIVED_MAX; an unknown op; a or b outside 0 .. n_fields_total-1; a == b; a coefficient that is not finite; and everything
 * sea_decode_member_quantiles / sea_decode_member_brier refuse.  Returns SEA_EUNSUPPORTED (callers compose the decode and torch ops) for sources in
 * different groups, SEA_F32, S above 640 and more than 128 members.  Notes the forms "decode.derived_quantiles" and "decode.derived_brier" (a = the
 * padded hidden width, b = the dynamic LDS bytes).
 * (Additions to ABI version 8.  The struct is not in sea_struct_sizes(): sizeof(SeaDerivedField) is 32.)
 */
#define SEA_DERIVED_MAX 8
#define SEA_DERIVED_MAGNITUDE 0
#define SEA_DERIVED_ENERGY 1
#define SEA_DERIVED_DIFFERENCE 2
typedef struct {
    int32_t op, a, b, pad_;
    float scale_a, shift_a, scale_b, shift_b;
} SeaDerivedField;           /* 32 bytes */
int sea_decode_derived_quantiles(const SeaDecodeMseGroup* groups, int n_groups, const SeaDerivedField* derived, int n_derived,
                                 const SeaDecodeMemberQuantiles* p, int dtype, void* stream);
int sea_decode_derived_brier(const SeaDecodeMseGroup* groups, int n_groups, const SeaDerivedField* derived, int n_derived,
                             const SeaDecodeMemberBrier* p, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * sea_decode_derived_verify: sea_decode_member_verify for DERIVED fields — is the ensemble of the speed calibrated, is its spread the size of its
 * error, what is its CRPS, is its rank histogram flat.  None of this follows from the scores of u and v: the derived value x_j of member j at a cell is
 * formed first, exactly as sea_decode_derived_quantiles forms it (the definitions above: the same decode, the same single-rounded f32 arithmetic, the
 * correctly rounded root), and from x_j on everything is sea_decode_member_verify with "field" read as "derived field" — the same device code behind
 * the value image: the history's weights w_m, c and status; mean, spread, CRPS, PIT and rank per cell; the eight fp64 sums and the rank histogram per
 * (history, derived field).  A derived cell scored from the same f32 values has the bits of a cell of sea_decode_member_verify and of a sensor of
 * sea_ensemble_verify.
 * p->n_fields_total stays the number of SOURCE fields (the groups cover them exactly once); every other quantity that has F in
 * sea_decode_member_verify has n_derived here: obs and prec [B * P, n_derived, >= C] — READINGS OF THE DERIVED QUANTITY, in its own units, and their
 * precisions — prec_field [n_derived]; mean, spread, crps, pit f32 and rank int32 [B * P, n_derived, ld_out]; sums f64 [B, n_derived, 8]; hist int64
 * [B, n_derived, members + 1]; work_bytes >= sea_decode_member_verify_ws_bytes(B, P, n_derived, members, Cp).
 * Cells: LIVE, DEAD and BAD exactly as in sea_decode_member_verify (the weight w[d, c] from counts, prec_field[d] and prec by selects; obs is never
 * read at a dead cell).  A live cell where a live member's x is not finite (NaN or Inf in a source, overflow of a square) is BAD: its floats are NaN,
 * its rank -2, sums[.., 6] counts it and nothing else is added.  accumulate, unbiased, logw, dead members and status are as in
 * sea_decode_member_verify (status[b] = -1 for invalid log-weights or no live member: maps 0 / -1, nothing added).
 * Launches: two.  Launch 1 has sea_decode_member_verify's grid with n_derived for F — a workgroup of 8 waves per (history, patch, derived field, chunk
 * of 512 columns) — and per tile of 32 columns the two-source decode of the derived launches above (the W2 tiles of source a and of source b through
 * the SAME two LDS images, the stream a_0, b_0, a_1, b_1, ...; hidden rows loaded once; a's tile into 8 registers, b's on top, the op per element, x
 * to the value image), then sea_decode_member_verify's scoring, finish and sums; launch 2 is that entry point's finish launch.  No floating-point
 * atomics: two runs give the same bits, a history's outputs are those of a call holding it alone, and a derived field's outputs do not depend on the
 * other derived fields of the call.
 * Returns -1, with the entry point and the offending derived field named in sea_last_error(), before any device is touched, for everything
 * sea_decode_derived_brier refuses of the derived table and everything sea_decode_member_verify refuses.  Returns SEA_EUNSUPPORTED (callers compose
 * the decode and torch ops) for sources in different groups, SEA_F32, S above 640 and more than 128 members.  Notes the form "decode.derived_verify"
 * (a = the padded hidden width, b = the dynamic LDS bytes).
 * (Addition to ABI version 8; SeaDecodeMemberVerify and SeaDerivedField are reused unchanged.)
 */
int sea_decode_derived_verify(const SeaDecodeMseGroup* groups, int n_groups, const SeaDerivedField* derived, int n_derived,
                              const SeaDecodeMemberVerify* p, int dtype, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Sparse sensors that read a DERIVED quantity: sea_decode_sensor_sse and sea_decode_sensor_grad for instruments that give a speed (hot-wire, Pitot
 * tube, cup anemometer), an energy / dynamic pressure or a difference of two values (a differential tap) at a point — mixed freely with plain
 * sensors.  SeaDecodeSensorSse, SeaDecodeSensorGrad and the SeaDecodeMseGroup operands are reused unchanged; one table struct is added.
 * Layout.  A READING occupies two adjacent entries of the sorted, padded list: entry 2 i gathers the W2 row of source a (wrow[2 i]), entry 2 i + 1
 * the W2 row of source b (wrow[2 i + 1]) — same group, same observed patch, same cell.  A (group, patch) segment is padded to a multiple of 32
 * entries as before: 16 readings per tile.  With y[bm, k] EXACTLY sea_decode_sensor_sse's (the same accumulators, the same bits), ya = y[bm, 2 i],
 * yb = y[bm, 2 i + 1]:
 *     op[2 i] == -1 (plain)   x = ya                       (wrow[2 i + 1] is 0 and yb is not used)
 *     otherwise               a' = ya * scale[2 i] + shift[2 i],  b' = yb * scale[2 i + 1] + shift[2 i + 1],  x = SEA_DERIVED_* of (a', b') as defined
 *                             above for sea_decode_derived_quantiles: the same device function, every operation rounded once, the rounded root
 *     w          = live[2 i] != 0 and prec[b * ld_prec + 2 i] > 0 ? prec[b * ld_prec + 2 i] : 0       (prec == NULL: 1)
 *     d          = w > 0 ? x - obs[b * ld_obs + 2 i] : 0                 (a select; obs in the units of x)
 *     wsse[bm]   = sum over pairs of (w d) d    (fp32; the lane's pairs per tile ascending, tiles ascending, the butterfly and finish launch of
 *                                                sea_decode_sensor_sse)
 *     pred[bm * K_pad + 2 i] = pred[bm * K_pad + 2 i + 1] = x            (when pred != NULL)
 * live, obs and prec at the odd entries and op at the odd entries are not read.  sea_decode_derived_sensor_grad forms, in fp32 from the same a', b', x,
 *     ga = dx / dya:  plain 1 | difference scale_a | energy a' scale_a | magnitude x > 0 ? a' scale_a / x : 0     (a select: exactly 0 at x == 0)
 *     gb = dx / dyb:  plain 0 | difference -scale_b | energy b' scale_b | magnitude x > 0 ? b' scale_b / x : 0
 *     (ga, gb are NOT single-rounded like x: the magnitude quotient is a' scale_a * rcp(x) with the hardware's approximate reciprocal v_rcp_f32, about
 *      1 ulp of f32 — far below the rounding of r to the act dtype that follows)
 *     r[2 i] = act(w d ga),  r[2 i + 1] = act(w d gb)                    (each rounded to the act dtype ONCE)
 * and then runs sea_decode_sensor_grad's second product unchanged: dH = 2 grad_scale * sum_k r[bm, k] W2[wrow[k]] [* gelu_erf'(Z)]; every element of
 * dH is written, rows of empty segments are exact zeros, and wsse and pred have the bits of sea_decode_derived_sensor_sse.
 * Tables: op int32, scale f32, shift f32, each [K_pad] on the device, non-NULL and 16-byte aligned (a lane reads them by 16-byte loads, as obs and
 * prec).  The kernels TRUST op (-1 or a SEA_DERIVED_* code at even entries), wrow and seg: the caller range-checks them on the host before the
 * upload (sea_amd/ensemble.py, DerivedSensorSet).  No atomics, one writer per element: two runs give the same bits, and a member's outputs do not
 * depend on `members`, on the number of histories or on its row tile.
 * Everything sea_decode_sensor_sse / sea_decode_sensor_grad refuse is refused here, before any device is touched, with the entry point named in
 * sea_last_error(); so is a NULL or misaligned table pointer.  SEA_F32 and S > 640 return SEA_EUNSUPPORTED.  Forms noted:
 * "derived_sensor_sse.rows64", "derived_sensor_grad.rows64".
 * (Additions to ABI version 8.  The struct is not in sea_struct_sizes(): sizeof(SeaDerivedSensorTables) is 24.)
 */
typedef struct {
    const int32_t* op;       /* int32 [K_pad]: -1 plain, or SEA_DERIVED_* at entry 2 i */
    const float* scale;      /* f32 [K_pad]: scale_a at 2 i, scale_b at 2 i + 1 */
    const float* shift;      /* f32 [K_pad]: shift_a at 2 i, shift_b at 2 i + 1 */
} SeaDerivedSensorTables;    /* 24 bytes */
int sea_decode_derived_sensor_sse(const SeaDecodeMseGroup* groups, int n_groups, const SeaDecodeSensorSse* p, const SeaDerivedSensorTables* tables, int dtype,
                                  void* stream);
int sea_decode_derived_sensor_grad(const SeaDecodeMseGroup* groups, int n_groups, const SeaDecodeSensorGrad* p, const SeaDerivedSensorTables* tables, int dtype,
                                   void* stream);

/* Tuning aid: register a device buffer of n_steps * 64 8-byte words that the persistent form fills with 100 MHz clock stamps of its hand-offs
 * (tools/kv_persist_timeline.py); NULL switches it off. */
void sea_kv_debug_stamps(unsigned long long* buf);

/* ------------------------------------------------------------------------------------------------------------
 * Self-test of the MFMA fragment maps this library relies on (16x16x32 bf16 and 16x16x4 f32, A/B/C lane maps):
 * multiplies exact small-integer matrices on the device and checks every element on the host.  Synchronous.
 * Returns 0 when both maps are as documented in cdna_hip_programming.md §3.
 */
int sea_selftest_mfma(void);


/* ------------------------------------------------------------------------------------------------------------
 * One EncoderBlock of the spatial encoder (reference models/base_blocks.py:123-139: x += MHA(LN(x)); x += MLP_x4(LN(x)), weight-only
 * LayerNorms, un-masked attention without rotary embedding, projection without bias, MLP = Linear, LayerNorm + GELU, Linear), fused per snapshot:
 * one workgroup owns the P rows of one snapshot and runs every phase of the block; rows m = snapshot * P + patch.
 *
 * sea_encoder_block_fwd: Zout = block(Zin).  ONE launch per block.
 * sea_encoder_block_bwd: from dZout, recomputes the block's forward from Zin and writes dZin (f32) plus the activation-dtype operands of ONE
 *   sea_wgrad_grouped launch that yields every parameter gradient of the block (Linear: dY | X pairs; LayerNorm weights / bias: the column sums of
 *   u1, u2, u3w, u3b, i.e. the db of a wgrad group).  The backward of a block is therefore two launches.
 * Supported: dtype SEA_BF16, W in {32, 64}, H = 8 (head dim W / 8), S = 4 W, 1 <= P <= 128 — anything else returns SEA_EUNSUPPORTED (-3)
 * and the caller composes the block from the other entry points.  Weights are act [out, in] (nn.Linear layout); wqkv = [q; k; v] rows, bqkv f32 [3W].
 * ws: f32 workspace of >= sea_encoder_block_ws_floats(B, P, W) floats, private to the call.
 */
typedef struct {
    const float* Zin;   /* f32 [M, W] block input */
    float* Zout;        /* f32 [M, W] block output (forward) */
    const void* wqkv;   /* act [3W, W] */
    const float* bqkv;  /* f32 [3W] */
    const void* wo;     /* act [W, W] */
    const void* w1;     /* act [S, W] */
    const float* b1;    /* f32 [S] */
    const float* lnw;   /* f32 [S] */
    const float* lnb;   /* f32 [S] */
    const void* w2;     /* act [W, S] */
    const float* b2;    /* f32 [W] */
    const float* g1;    /* f32 [W] ln_exp1_1.weight */
    const float* g2;    /* f32 [W] ln_exp1_2.weight */
    const float* dZout; /* f32 [M, W] (backward) */
    float* dZin;        /* f32 [M, W] (backward; may not alias dZout) */
    /* backward outputs, act, contiguous rows: the wgrad operands */
    void* n1;    /* [M, W]  LN1 output: X of q / k / v */
    void* dqkv;  /* [M, 3W] dY of q | k | v */
    void* att;   /* [M, W]  attention output: X of the projection */
    void* dz1;   /* [M, W]  dY of the projection */
    void* n2;    /* [M, W]  X of fc1 */
    void* dh;    /* [M, S]  dY of fc1 */
    void* hg;    /* [M, S]  X of fc2 */
    void* dz2;   /* [M, W]  dY of fc2 */
    void* u1;    /* [M, W]  column sums = d ln_exp1_1.weight */
    void* u2;    /* [M, W]  column sums = d ln_exp1_2.weight */
    void* u3w;   /* [M, S]  column sums = d mlp LayerNorm weight */
    void* u3b;   /* [M, S]  column sums = d mlp LayerNorm bias */
    float* ws;
    int64_t ws_floats;
    int32_t B, P, W, H;
    float eps;
    int32_t pad_;
} SeaEncBlock;
int64_t sea_encoder_block_ws_floats(int B, int P, int W);
int sea_encoder_block_fwd(const SeaEncBlock* params, int dtype, void* stream);
int sea_encoder_block_bwd(const SeaEncBlock* params, int dtype, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SEA_HIP_H */
