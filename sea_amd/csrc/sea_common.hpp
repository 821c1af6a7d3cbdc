// Shared device helpers for libsea_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdarg.h>
#include <string.h>
#include <math.h>
#include <type_traits>

#include "../../include/sea_hip.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));

// ------------------------------------------------------------------------------------------------ errors
void sea_set_error(const char* fmt, ...);
// Tuning aid `key` of the SEA_TUNE environment variable ("key=value,key=value"), or dflt: every native switch goes through this one variable (core.hip)
int sea_tune(const char* key, int dflt);
// The kernel form a launcher took, for tests (sea_last_form): `literal` must be a string literal — only the pointer and the two ints are kept (core.hip)
void sea_note_form(const char* literal, int a, int b);
int sea_cu_count();   // CUs of the current device (core.hip)
#define SEA_REQUIRE(cond, ...)            \
    do {                                  \
        if (!(cond)) {                    \
            sea_set_error(__VA_ARGS__);   \
            return SEA_EINVAL;            \
        }                                 \
    } while (0)
#define SEA_CHECK_LAUNCH(name)                                                     \
    do {                                                                           \
        hipError_t e_ = hipGetLastError();                                         \
        if (e_ != hipSuccess) {                                                    \
            sea_set_error("%s: launch failed: %s", name, hipGetErrorString(e_));   \
            return SEA_ELAUNCH;                                                    \
        }                                                                          \
    } while (0)

static inline bool sea_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
static inline bool sea_aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }

// ------------------------------------------------------------------------------------------------ dtype traits
// One "fragment" is 16 bytes per lane along the contraction dimension: 8 bf16 or 4 f32.
// mma16(a, b, acc) contracts CK = 4 * EPC elements (the 4 lane groups g = lane >> 4 each hold EPC of them):
//   bf16: one v_mfma_f32_16x16x32_bf16 (lane holds k = 8g + j);
//   f32 : four v_mfma_f32_16x16x4_f32, the j-th taking element j of every lane (k = 4g + j).
// Operand maps (cdna_hip_programming.md §3): A[row = lane & 15][k], B[k][col = lane & 15],
// C/D: col = lane & 15, row = 4 * (lane >> 4) + reg.
template <typename T>
struct ActTraits;
template <>
struct ActTraits<float> {
    static constexpr int EPC = 4;  // elements per 16-byte chunk
    static constexpr int CK = 16;  // contraction elements per mma16
};
template <>
struct ActTraits<__bf16> {
    static constexpr int EPC = 8;
    static constexpr int CK = 32;
};

template <typename T>
__device__ __forceinline__ void mma16(const uint4& a, const uint4& b, f32x4& acc);

template <>
__device__ __forceinline__ void mma16<__bf16>(const uint4& a, const uint4& b, f32x4& acc) {
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), acc, 0, 0, 0);
}
template <>
__device__ __forceinline__ void mma16<float>(const uint4& a, const uint4& b, f32x4& acc) {
    const f32x4 fa = __builtin_bit_cast(f32x4, a);
    const f32x4 fb = __builtin_bit_cast(f32x4, b);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[0], fb[0], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[1], fb[1], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[2], fb[2], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[3], fb[3], acc, 0, 0, 0);
}

__device__ __forceinline__ float to_f32(float v) { return v; }
__device__ __forceinline__ float to_f32(__bf16 v) { return (float)v; }
template <typename T>
__device__ __forceinline__ T from_f32(float v);
template <>
__device__ __forceinline__ float from_f32<float>(float v) { return v; }
template <>
__device__ __forceinline__ __bf16 from_f32<__bf16>(float v) { return (__bf16)v; }

// erf(x / sqrt 2) and exp(-x^2 / 2) together, from ONE v_exp and one v_rcp: Abramowitz & Stegun 7.1.26
// (erf z = 1 - (a1 t + ... + a5 t^5) e^{-z^2}, t = 1/(1 + p z), |error| <= 1.5e-7 absolute — below fp32 rounding of 1 + erf).
// The exponential of the formula, e^{-z^2} with z = x / sqrt 2, is the Gaussian factor GELU' needs anyway.  ocml's erff costs
// ~4x the instructions; the LayerNorm+GELU passes over [M, 8E] are VALU-bound on it.
__device__ __forceinline__ void erf_gauss(float x, float& erf_v, float& gauss) {
    const float z = fabsf(x) * 0.70710678118654752440f;
    const float t = __builtin_amdgcn_rcpf(fmaf(0.3275911f, z, 1.0f));
    gauss = __expf(-0.5f * x * x);
    const float poly = t * (0.254829592f + t * (-0.284496736f + t * (1.421413741f + t * (-1.453152027f + t * 1.061405429f))));
    erf_v = copysignf(1.0f - poly * gauss, x);
}
__device__ __forceinline__ float gelu_erf(float x) {
    float e, g;
    erf_gauss(x, e, g);
    return 0.5f * x * (1.0f + e);
}
// d/dx gelu_erf(x) = Phi(x) + x phi(x)
__device__ __forceinline__ float gelu_erf_grad(float x) {
    float e, g;
    erf_gauss(x, e, g);
    return 0.5f * (1.0f + e) + x * 0.39894228040143267794f * g;
}
// GELU for results that are rounded to bf16 at once: x Phi(x) with Phi(x) - 1/2 = x P(x^2) on |x| <= 4 (degree-7 polynomial in x^2, Chebyshev fit of
// erf(x / sqrt 2) / (2 x)), the argument clamped to [-4, 4] (1 - Phi(4) = 3e-5).  |error| <= 1.8e-4 for |x| <= 4 and <= 7e-5 |x| beyond — below the bf16
// rounding of the result (2^-9 relative) over the range LayerNorm outputs live in — for 11 plain fp32 instructions and no v_exp / v_rcp (quarter rate),
// against ~22 + 2 transcendental for the A&S form above.  The fp32 path (parity bar 1e-4) never uses it.
__device__ __forceinline__ float gelu_erf_bf16(float x) {
    const float xc = __builtin_amdgcn_fmed3f(x, -4.0f, 4.0f);
    const float u = xc * xc;
    float p = -1.903182723e-09f;
    p = fmaf(p, u, 1.410586208e-07f);
    p = fmaf(p, u, -4.565313247e-06f);
    p = fmaf(p, u, 8.634554251e-05f);
    p = fmaf(p, u, -1.085383119e-03f);
    p = fmaf(p, u, 9.789848700e-03f);
    p = fmaf(p, u, -6.636063010e-02f);
    p = fmaf(p, u, 3.989269733e-01f);
    return x * fmaf(xc, p, 0.5f);
}
template <typename T>
__device__ __forceinline__ float gelu_for(float x) {   // the GELU whose result is stored as T
    if constexpr (sizeof(T) == 2) return gelu_erf_bf16(x);
    else return gelu_erf(x);
}
// d/dx gelu for gradients that are rounded to bf16 at once: Phi from the same polynomial, the Gaussian factor from one v_exp (the LayerNorm + GELU
// backward over [M, 8E] is VALU-bound on this function: ~14 instructions against ~26)
__device__ __forceinline__ float gelu_erf_grad_bf16(float x) {
    const float xc = __builtin_amdgcn_fmed3f(x, -4.0f, 4.0f);
    const float u = xc * xc;
    float p = -1.903182723e-09f;
    p = fmaf(p, u, 1.410586208e-07f);
    p = fmaf(p, u, -4.565313247e-06f);
    p = fmaf(p, u, 8.634554251e-05f);
    p = fmaf(p, u, -1.085383119e-03f);
    p = fmaf(p, u, 9.789848700e-03f);
    p = fmaf(p, u, -6.636063010e-02f);
    p = fmaf(p, u, 3.989269733e-01f);
    const float gauss = __builtin_amdgcn_exp2f(-0.72134752044448170368f * x * x);   // e^{-x^2 / 2}
    return fmaf(x * 0.39894228040143267794f, gauss, fmaf(xc, p, 0.5f));
}
template <typename T>
__device__ __forceinline__ float gelu_grad_for(float x) {   // GELU' for a gradient stored as T
    if constexpr (sizeof(T) == 2) return gelu_erf_grad_bf16(x);
    else return gelu_erf_grad(x);
}
__device__ __forceinline__ float silu_f(float x) { return x / (1.0f + __expf(-x)); }

// ------------------------------------------------------------------------------------------------ scalar-lane fp32 arithmetic
// gfx950 erratum (tools/isa_variants.py, tools/pk_opsel_bench.hip): a packed fp32 instruction (v_pk_fma_f32 / v_pk_mul_f32 /
// v_pk_add_f32) whose LOW result half selects the HIGH dword of its src1 pair (op_sel:[x,1,..]) returns a wrong low result in lanes 48-63
// whenever another wave of the CU issues MFMAs at the same time.  hipcc's SLP vectoriser builds exactly that form out of scalar code with a
// lane swap: the RoPE rotation (x_e c - x_o s, x_e s + x_o c), sums of squares, horizontal adds.  The build checks every device listing for
// it (sea_amd/build.py: lint_isa); code that trips the check is written with these helpers, which the vectoriser cannot pack.
__device__ __forceinline__ float fma1(float a, float b, float c) {
    float r;
    asm("v_fma_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}
__device__ __forceinline__ float mul1(float a, float b) {
    float r;
    asm("v_mul_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ float add1(float a, float b) {
    float r;
    asm("v_add_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
// (xe + i xo)(c + i s) in fp32: the interleaved-pair rotation of apply_rotary_emb (reference models/base_blocks.py:313-324)
__device__ __forceinline__ void rope_pair(float xe, float xo, float c, float s, float& oe, float& oo) {
    oe = fma1(xe, c, -mul1(xo, s));
    oo = fma1(xe, s, mul1(xo, c));
}
// its inverse (rotation by -angle): the backward of the rotation
__device__ __forceinline__ void unrope_pair(float& e, float& o, float c, float s) {
    const float ne = fma1(e, c, mul1(o, s));
    const float no = fma1(o, c, -mul1(e, s));
    e = ne;
    o = no;
}

// ------------------------------------------------------------------------------------------------ counter-based dropout
__device__ __forceinline__ uint32_t fmix32(uint32_t x) {
    x ^= x >> 16; x *= 0x85ebca6bu; x ^= x >> 13; x *= 0xc2b2ae35u; x ^= x >> 16;
    return x;
}
// 4 random bytes for elements (row, 4*cb .. 4*cb+3) of a stream (include/sea_hip.h, SeaDropout)
__device__ __forceinline__ uint32_t drop_word(uint32_t seed, uint32_t stream, uint32_t row, uint32_t cb) {
    uint32_t x = fmix32((seed ^ (stream * 0x9E3779B1u)) + row * 0x85EBCA77u);
    return fmix32(x ^ (cb * 0xC2B2AE3Du + 0x27D4EB2Fu));
}
__device__ __forceinline__ float drop_scale(int thr) { return 256.0f / (float)(256 - thr); }
// keep-and-scale factor of element j (0..3) of a word
__device__ __forceinline__ float drop_factor(uint32_t word, int j, int thr, float scale) {
    return (int)((word >> (8 * j)) & 0xffu) >= thr ? scale : 0.f;
}

// Attention grids are (tile, batch*head, problem).  Workgroups are dealt to the CUs round-robin in linear block order; with the
// tile index fastest, CU c receives blocks c, c + 256, ... which all have the SAME tile index (256 % 32 == 0), i.e. the same causal
// workload: the CUs holding the last query tiles would work 32x longer than those holding the first.  Re-decode the linear id
// with (batch*head, problem) fastest: tiles go out heaviest-first across the whole chip and every CU gets a mix of weights.
// Rounds of 256 workgroups (one per CU) alternate direction — a CU that received the heaviest tile of one round receives the lightest of
// the next — so the per-CU sums stay close (3 resident workgroups per CU at cfg2: max/mean load 1.29 -> 1.07).
// (Round 3, measured and not kept: an order that lets each XCD walk its (trajectory, head) pairs one after the other — all tiles of a pair before the next, so that
// the pair's K / V rows stay in that XCD's L2 instead of 8 pairs' 6 MB evicting each other; PMC at cfg3 shows 626 MB fetched by the self-attention forward for
// 100 MB of operands — was SLOWER everywhere: cfg3 train 3.644 -> 3.795 ms, B = 8 forward 1.087 -> 1.131, cfg2 forward 0.2259 -> 0.2473.  The launches are
// bound by the balance of causal work across CUs, not by those re-reads.)
__device__ __forceinline__ void decode_attn_block(int& tile, int& bh, int& z) {
    int L = blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z);
    const int nbz = gridDim.y * gridDim.z;
    {
        const int total = gridDim.x * nbz, round = L >> 8;
        if ((round & 1) && total >= 512) {  // measured: with fewer than two full rounds the plain order is faster (384 workgroups: 10.1 vs 11.5 us)
            const int left = total - (round << 8);
            const int in_round = left < 256 ? left : 256;
            L = (round << 8) + in_round - 1 - (L & 255);
        }
    }
    tile = L / nbz;
    const int inner = L - tile * nbz;
    z = inner / gridDim.y;
    bh = inner - z * gridDim.y;
}

// max over the 4 lane groups {l, l^16, l^32, l^48} without touching the LDS crossbar: gfx950's half / row swaps
// (v_permlane32_swap exchanges the upper half of vdst with the lower half of src, v_permlane16_swap the odd 16-lane rows of
// vdst with the even rows of src; with vdst = src = x the two results hold both partners of every lane).
// (max1: one v_max_f32 — fmaxf on values the compiler cannot see through, such as the swap results, is preceded by a canonicalising v_max x, x each)
__device__ __forceinline__ float max1(float a, float b) {
    float r;
    asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ float group_max4(float x) {
    const unsigned u = __float_as_uint(x);
    const auto a = __builtin_amdgcn_permlane32_swap(u, u, false, false);
    x = max1(__uint_as_float(a[0]), __uint_as_float(a[1]));
    const unsigned v = __float_as_uint(x);
    const auto b = __builtin_amdgcn_permlane16_swap(v, v, false, false);
    return max1(__uint_as_float(b[0]), __uint_as_float(b[1]));
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// Value of lane (lane ^ X) without the LDS crossbar (a ds_bpermute costs a trip through the LDS pipeline; a chain of six of them is most of what a few-row launch
// does after its last load): half / row swaps for 32 / 16 (with vdst = src the two results of a swap hold the lower-half and the upper-half — the even-row and the
// odd-row — value of every lane: the partner's is the one this lane does not own), DPP row rotations for 8 / 4 (row_ror:n gives lane i the value of lane
// (i - n) mod 16), quad permutations for 2 / 1.
template <int CTRL>
__device__ __forceinline__ float dpp_mov(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, true));
}
template <int X>
__device__ __forceinline__ float lane_xor(float v, int lane) {
    static_assert(X == 32 || X == 16 || X == 8 || X == 4 || X == 2 || X == 1, "lane_xor distance");
    if constexpr (X == 32) {
        const unsigned u = __float_as_uint(v);
        const auto r = __builtin_amdgcn_permlane32_swap(u, u, false, false);
        return __uint_as_float((lane & 32) ? r[0] : r[1]);
    } else if constexpr (X == 16) {
        const unsigned u = __float_as_uint(v);
        const auto r = __builtin_amdgcn_permlane16_swap(u, u, false, false);
        return __uint_as_float((lane & 16) ? r[0] : r[1]);
    } else if constexpr (X == 8) {
        return dpp_mov<0x128>(v);                       // row_ror:8
    } else if constexpr (X == 4) {
        const float dn = dpp_mov<0x124>(v), up = dpp_mov<0x12C>(v);   // row_ror:4: from lane i - 4; row_ror:12: from lane i + 4 (mod 16)
        return (lane & 4) ? dn : up;
    } else if constexpr (X == 2) {
        return dpp_mov<0x4E>(v);                        // quad_perm:[2,3,0,1]
    } else {
        return dpp_mov<0xB1>(v);                        // quad_perm:[1,0,3,2]
    }
}
// all 64 lanes' maximum in every lane
__device__ __forceinline__ float wave_max_xor(float v, int lane) {
    v = fmaxf(v, lane_xor<1>(v, lane));
    v = fmaxf(v, lane_xor<2>(v, lane));
    v = fmaxf(v, lane_xor<4>(v, lane));
    v = fmaxf(v, lane_xor<8>(v, lane));
    v = fmaxf(v, lane_xor<16>(v, lane));
    v = fmaxf(v, lane_xor<32>(v, lane));
    return v;
}
// all 64 lanes' sum in every lane
__device__ __forceinline__ float wave_sum_xor(float v, int lane) {
    v += lane_xor<1>(v, lane);
    v += lane_xor<2>(v, lane);
    v += lane_xor<4>(v, lane);
    v += lane_xor<8>(v, lane);
    v += lane_xor<16>(v, lane);
    v += lane_xor<32>(v, lane);
    return v;
}

// Sum over the 64 lanes of each of NV values (NV a power of two <= 64), total number (lane / (64 / NV)) left in lane `lane`: NV - 1 + (6 - log2 NV) exchanges
// instead of 6 NV for NV separate butterflies, and the result spread over the lanes (one epilogue element per lane).
// step with exchange distance X: the lanes whose bit X is set keep the upper half of the values and hand over the lower half (every stage in registers of
// its own: the in-place form is compiled into a dynamically indexed scratch array)
template <int N, int X>
__device__ __forceinline__ float lane_scatter_step(const float (&v)[N], int lane) {
    if constexpr (X == 0) {
        return v[0];
    } else if constexpr (N > 1) {
        const bool up = (lane & X) != 0;
        float nv[N / 2];
#pragma unroll
        for (int i = 0; i < N / 2; ++i) {
            const float lo = v[i], hi = v[i + N / 2];
            const float send = up ? lo : hi;
            const float keep = up ? hi : lo;
            nv[i] = keep + lane_xor<X>(send, lane);
        }
        return lane_scatter_step<N / 2, X / 2>(nv, lane);
    } else {
        const float nv[1] = {v[0] + lane_xor<X>(v[0], lane)};
        return lane_scatter_step<1, X / 2>(nv, lane);
    }
}
template <int NV>
__device__ __forceinline__ float lane_scatter_sum(const float (&v)[NV], int lane) {
    return lane_scatter_step<NV, 32>(v, lane);
}

// Pack 4 fp32 values into 4 consecutive act elements and store them (8 B for bf16, 16 B for f32).
__device__ __forceinline__ void store4(float* dst, float a, float b, float c, float d) {
    *reinterpret_cast<float4*>(dst) = make_float4(a, b, c, d);
}
__device__ __forceinline__ void store4(__bf16* dst, float a, float b, float c, float d) {
    bf16x4 v = {(__bf16)a, (__bf16)b, (__bf16)c, (__bf16)d};
    *reinterpret_cast<bf16x4*>(dst) = v;
}
__device__ __forceinline__ void load4(const float* src, float (&o)[4]) {
    float4 v = *reinterpret_cast<const float4*>(src);
    o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w;
}
__device__ __forceinline__ void load4(const __bf16* src, float (&o)[4]) {
    bf16x4 v = *reinterpret_cast<const bf16x4*>(src);
    o[0] = (float)v[0]; o[1] = (float)v[1]; o[2] = (float)v[2]; o[3] = (float)v[3];
}

// 8 consecutive elements (16 bytes of bf16: one full-width access per lane; 2 x 16 bytes of f32)
__device__ __forceinline__ void load8(const __bf16* src, float (&o)[8]) {
    const bf16x8 v = *reinterpret_cast<const bf16x8*>(src);
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = (float)v[e];
}
__device__ __forceinline__ void load8(const float* src, float (&o)[8]) {
    const float4 a = *reinterpret_cast<const float4*>(src), b = *reinterpret_cast<const float4*>(src + 4);
    o[0] = a.x; o[1] = a.y; o[2] = a.z; o[3] = a.w; o[4] = b.x; o[5] = b.y; o[6] = b.z; o[7] = b.w;
}
__device__ __forceinline__ void store8(__bf16* dst, const float (&v)[8]) {
    bf16x8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = (__bf16)v[e];
    *reinterpret_cast<bf16x8*>(dst) = o;
}

// Workgroups are dealt round-robin over the 8 XCDs (blocks b and b + 8 share an L2).  Kernels that number their tiles so that consecutive
// tiles re-read the same operand panel give each XCD a CONTIGUOUS range of tile numbers, so that those re-reads hit its own L2 instead of
// crossing the fabric once per XCD (bijective form of the T1 remap, cdna_hip_programming.md; only placement, never correctness).
__device__ __forceinline__ int xcd_remap(int bid, int nwg) {
    const int q = nwg >> 3, r = nwg & 7, xcd = bid & 7, idx = bid >> 3;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
}
