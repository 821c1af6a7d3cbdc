// Loss, metric and optimizer kernels of the SEA temporal train step (gfx950): sea_mse_fwd_bwd, sea_relative_mse,
// sea_adamw_flat, and the clipped / skippable pair sea_grad_norm_ctl + sea_adamw_flat_ctl.  All HBM-bandwidth-bound streaming passes:
// 16-byte accesses, grid-stride, fp32 arithmetic (the gradient norm accumulates in fp64).
#include "sea_common.hpp"

__device__ __forceinline__ float block_sum_256(float v, float* red) {
    v = wave_sum(v);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) red[wave] = v;
    __syncthreads();
    const float total = red[0] + red[1] + red[2] + red[3];
    __syncthreads();
    return total;
}

// ---------------------------------------------------------------------------------------------- MSE
// pass 1: partial[b] = sum over the block's elements of (out - tgt)^2 ; dout = (out - tgt) * gscale2 (gscale2 = 2*scale/n).
// VEC: 16-byte-aligned pointers, float4 body over the first 4*(n/4) elements, then the n % 4 tail on threads 0..2 of block 0.
// !VEC (a pointer that is only 4-byte aligned): one element per thread and step.  Either way each thread's terms are summed in a fixed order.
template <bool VEC>
__global__ __launch_bounds__(256) void mse_partial_kernel(const float* __restrict__ out, const float* __restrict__ tgt, float* __restrict__ dout,
                                                          float* __restrict__ partial, int64_t n, float gscale2) {
    __shared__ float red[4];
    float acc = 0.f;
    const int64_t first = (int64_t)blockIdx.x * 256 + threadIdx.x, stride = (int64_t)gridDim.x * 256;
    if (VEC) {
        const int64_t n4 = n >> 2;
        for (int64_t i = first; i < n4; i += stride) {
            const float4 a = reinterpret_cast<const float4*>(out)[i];
            const float4 b = reinterpret_cast<const float4*>(tgt)[i];
            const float4 d = make_float4(a.x - b.x, a.y - b.y, a.z - b.z, a.w - b.w);
            acc += (d.x * d.x + d.y * d.y) + (d.z * d.z + d.w * d.w);
            if (dout != nullptr) reinterpret_cast<float4*>(dout)[i] = make_float4(d.x * gscale2, d.y * gscale2, d.z * gscale2, d.w * gscale2);
        }
        const int64_t t = 4 * n4 + first;
        if (t < n) {
            const float d = out[t] - tgt[t];
            acc = fma1(d, d, acc);
            if (dout != nullptr) dout[t] = d * gscale2;
        }
    } else {
        for (int64_t i = first; i < n; i += stride) {
            const float d = out[i] - tgt[i];
            acc = fma1(d, d, acc);
            if (dout != nullptr) dout[i] = d * gscale2;
        }
    }
    const float total = block_sum_256(acc, red);
    if (threadIdx.x == 0) partial[blockIdx.x] = total;
}

// pass 2 (one block): loss = sum(partial) / n, summed in a fixed order (deterministic)
__global__ __launch_bounds__(256) void mse_final_kernel(const float* __restrict__ partial, int n_partial, float* __restrict__ loss, float inv_n) {
    __shared__ float red[4];
    float acc = 0.f;
    for (int i = threadIdx.x; i < n_partial; i += 256) acc += partial[i];
    const float total = block_sum_256(acc, red);
    if (threadIdx.x == 0) loss[0] = total * inv_n;
}

extern "C" int sea_mse_fwd_bwd(const float* out, const float* tgt, float* dout, float* loss, float* partial, int n_partial_cap,
                               int64_t n, float grad_scale, void* stream) {
    SEA_REQUIRE(out && tgt && loss && partial, "sea_mse_fwd_bwd: null pointer");
    SEA_REQUIRE(n >= 1, "sea_mse_fwd_bwd: n=%lld must be positive", (long long)n);
    SEA_REQUIRE(sea_aligned4(out) && sea_aligned4(tgt) && sea_aligned4(dout), "sea_mse_fwd_bwd: pointers must be 4-byte aligned");
    SEA_REQUIRE(n_partial_cap >= 1, "sea_mse_fwd_bwd: partial workspace too small");
    const bool vec = sea_aligned16(out) && sea_aligned16(tgt) && sea_aligned16(dout);
    const int64_t items = vec ? (n + 3) / 4 : n;   // VEC: a thread's first item also covers one tail element
    int64_t blocks = (items + 255) / 256;
    if (blocks > 1024) blocks = 1024;
    if (blocks > n_partial_cap) blocks = n_partial_cap;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const float gscale2 = 2.0f * grad_scale / (float)n;
    if (vec) mse_partial_kernel<true><<<dim3((unsigned)blocks), dim3(256), 0, s>>>(out, tgt, dout, partial, n, gscale2);
    else mse_partial_kernel<false><<<dim3((unsigned)blocks), dim3(256), 0, s>>>(out, tgt, dout, partial, n, gscale2);
    mse_final_kernel<<<dim3(1), dim3(256), 0, s>>>(partial, (int)blocks, loss, 1.0f / (float)n);
    SEA_CHECK_LAUNCH("sea_mse_fwd_bwd");
    return SEA_OK;
}

// ---------------------------------------------------------------------------------------------- relative MSE
// one wave per row of the last dimension: y[row] = sum (p - t)^2 / (sum t^2 + 1e-8).
// VEC: d % 4 == 0 and 16-byte-aligned pointers (so every row is): 16-byte loads.  !VEC: any d, 4-byte loads.
template <bool VEC>
__global__ __launch_bounds__(256) void relative_mse_kernel(const float* __restrict__ p, const float* __restrict__ t, float* __restrict__ y,
                                                           int64_t rows, int d) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float* pr = p + row * d;
    const float* tr = t + row * d;
    float num4[4] = {0.f, 0.f, 0.f, 0.f}, den4[4] = {0.f, 0.f, 0.f, 0.f};   // scalar-lane FMAs: see sea_common.hpp (packed horizontal adds trip the build's ISA check)
    if (VEC) {
        for (int i = lane * 4; i < d; i += 256) {
            float a[4], b[4];
            load4(pr + i, a);
            load4(tr + i, b);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float df = a[e] - b[e];
                num4[e] = fma1(df, df, num4[e]);
                den4[e] = fma1(b[e], b[e], den4[e]);
            }
        }
    } else {
        for (int i = lane; i < d; i += 64) {
            const float a = pr[i], b = tr[i], df = a - b;
            num4[0] = fma1(df, df, num4[0]);
            den4[0] = fma1(b, b, den4[0]);
        }
    }
    const float num = wave_sum(add1(add1(num4[0], num4[1]), add1(num4[2], num4[3])));
    const float den = wave_sum(add1(add1(den4[0], den4[1]), add1(den4[2], den4[3])));
    if (lane == 0) y[row] = num / (den + 1e-8f);
}

extern "C" int sea_relative_mse(const float* pred, const float* truth, float* y, int64_t rows, int d, void* stream) {
    SEA_REQUIRE(pred && truth && y && rows >= 1 && d >= 1, "sea_relative_mse: bad arguments rows=%lld d=%d", (long long)rows, d);
    SEA_REQUIRE(sea_aligned4(pred) && sea_aligned4(truth) && sea_aligned4(y), "sea_relative_mse: pointers must be 4-byte aligned");
    SEA_REQUIRE((rows + 3) / 4 <= 0x7fffffffLL, "sea_relative_mse: too many rows");
    const dim3 grid((unsigned)((rows + 3) / 4));
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (d % 4 == 0 && sea_aligned16(pred) && sea_aligned16(truth)) relative_mse_kernel<true><<<grid, dim3(256), 0, s>>>(pred, truth, y, rows, d);
    else relative_mse_kernel<false><<<grid, dim3(256), 0, s>>>(pred, truth, y, rows, d);
    SEA_CHECK_LAUNCH("sea_relative_mse");
    return SEA_OK;
}

// ---------------------------------------------------------------------------------------------- AdamW over the flat buffer
template <typename T>
__global__ __launch_bounds__(256) void adamw_flat_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                         float* __restrict__ v, T* __restrict__ shadow, int64_t n4, float lr, float beta1,
                                                         float beta2, float eps, float lr_wd, float inv_bc1, float inv_sqrt_bc2,
                                                         float grad_scale) {
    // scalar-lane helpers pin the evaluation order: -ffast-math would otherwise rewrite b m + (1-b) g as g + b (m - g), whose cancellation
    // costs log2(1 / (1 - b)) bits (10 for b2 = 0.999)
    const float omb1 = 1.0f - beta1, omb2 = 1.0f - beta2, step_size = lr * inv_bc1;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        float pp[4], gg[4], mm[4], vv[4];
        load4(p + 4 * i, pp);
        load4(g + 4 * i, gg);
        load4(m + 4 * i, mm);
        load4(v + 4 * i, vv);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float gr = mul1(gg[e], grad_scale);
            if (lr_wd != 0.f) pp[e] = fma1(-lr_wd, pp[e], pp[e]);   // decoupled weight decay p *= 1 - lr*wd, as p - (lr*wd) p: 1 - lr*wd rounded to fp32 would lose its low bits
            mm[e] = fma1(beta1, mm[e], mul1(omb1, gr));
            vv[e] = fma1(beta2, vv[e], mul1(mul1(omb2, gr), gr));
            // plain C from here: the wait states a v_sqrt / v_rcp result needs before a VALU reads it are inserted for compiled code only,
            // not for an asm helper reading it
            const float denom = sqrtf(vv[e]) * inv_sqrt_bc2 + eps;
            pp[e] -= step_size * (mm[e] / denom);
        }
        store4(p + 4 * i, pp[0], pp[1], pp[2], pp[3]);
        store4(m + 4 * i, mm[0], mm[1], mm[2], mm[3]);
        store4(v + 4 * i, vv[0], vv[1], vv[2], vv[3]);
        if (shadow != nullptr) store4(shadow + 4 * i, pp[0], pp[1], pp[2], pp[3]);
    }
}

extern "C" int sea_adamw_flat(float* p, const float* g, float* m, float* v, void* shadow, int shadow_dtype, int64_t n, float lr, float beta1,
                              float beta2, float eps, float weight_decay, int step, float grad_scale, void* stream) {
    SEA_REQUIRE(p && g && m && v, "sea_adamw_flat: null pointer");
    SEA_REQUIRE(n >= 4 && n % 4 == 0 && step >= 1, "sea_adamw_flat: n=%lld must be a positive multiple of 4, step >= 1", (long long)n);
    SEA_REQUIRE(sea_aligned16(p) && sea_aligned16(g) && sea_aligned16(m) && sea_aligned16(v) && sea_aligned16(shadow), "sea_adamw_flat: pointers must be 16-byte aligned");
    SEA_REQUIRE(!shadow || shadow_dtype == SEA_BF16 || shadow_dtype == SEA_F32, "sea_adamw_flat: bad shadow dtype");
    const double bc1 = 1.0 - pow((double)beta1, step), bc2 = 1.0 - pow((double)beta2, step);
    const int64_t n4 = n / 4;
    int64_t blocks = (n4 + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const float lr_wd = (float)((double)lr * (double)weight_decay);
    if (shadow != nullptr && shadow_dtype == SEA_BF16)
        adamw_flat_kernel<__bf16><<<dim3((unsigned)blocks), dim3(256), 0, s>>>(p, g, m, v, static_cast<__bf16*>(shadow), n4, lr, beta1, beta2, eps, lr_wd,
                                                                              (float)(1.0 / bc1), (float)(1.0 / sqrt(bc2)), grad_scale);
    else
        adamw_flat_kernel<float><<<dim3((unsigned)blocks), dim3(256), 0, s>>>(p, g, m, v, static_cast<float*>(shadow), n4, lr, beta1, beta2, eps, lr_wd,
                                                                             (float)(1.0 / bc1), (float)(1.0 / sqrt(bc2)), grad_scale);
    SEA_CHECK_LAUNCH("sea_adamw_flat");
    return SEA_OK;
}

// ---------------------------------------------------------------------------------------------- gradient norm -> step control block
__device__ __forceinline__ double block_sum_256_f64(double v, double* red) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) red[wave] = v;
    __syncthreads();
    const double total = (red[0] + red[1]) + (red[2] + red[3]);
    __syncthreads();
    return total;
}

// pass 1: partial[b] = sum over the block's elements of g^2, every square and every sum in fp64: no fp32 square overflows (|g| = 1e25) or vanishes
// (|g| = 1e-30), and the total is non-finite exactly when an element is.  One accumulator per float4 component (four independent FMA chains);
// four 16-byte loads in flight per thread while a full round of the grid remains.  The order of a thread's terms is fixed.
__global__ __launch_bounds__(256) void grad_norm_partial_kernel(const float* __restrict__ g, int64_t n4, double* __restrict__ partial) {
    __shared__ double red[4];
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    const float4* g4 = reinterpret_cast<const float4*>(g);
    const int64_t stride = (int64_t)gridDim.x * 256;
    int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    for (; i + 3 * stride < n4; i += 4 * stride) {
        const float4 a = g4[i], b = g4[i + stride], c = g4[i + 2 * stride], d = g4[i + 3 * stride];
        const float x[16] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x, c.y, c.z, c.w, d.x, d.y, d.z, d.w};
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[e & 3] = fma((double)x[e], (double)x[e], acc[e & 3]);
    }
    for (; i < n4; i += stride) {
        const float4 a = g4[i];
        const float x[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] = fma((double)x[e], (double)x[e], acc[e]);
    }
    const double total = block_sum_256_f64((acc[0] + acc[1]) + (acc[2] + acc[3]), red);
    if (threadIdx.x == 0) partial[blockIdx.x] = total;
}

__device__ __forceinline__ double powi_f64(double b, int e) {   // b^e, e >= 1, by squaring: a few fp64 ulps, no libm call on the device
    double r = 1.0;
    for (; e > 0; e >>= 1, b *= b)
        if (e & 1) r *= b;
    return r;
}

// pass 2 (one block): the partials summed in a fixed order, then ONE thread decides the step and writes the control block (include/sea_hip.h)
__global__ __launch_bounds__(256) void grad_norm_final_kernel(const double* __restrict__ partial, int n_partial, float grad_scale, float max_norm,
                                                              int skip_nonfinite, float beta1, float beta2, int32_t* __restrict__ ctl) {
    __shared__ double red[4];
    double acc = 0.0;
    for (int i = threadIdx.x; i < n_partial; i += 256) acc += partial[i];
    const double total = block_sum_256_f64(acc, red);
    if (threadIdx.x != 0) return;
    const double norm = fabs((double)grad_scale) * sqrt(total);
    const float norm32 = (float)norm;
    const bool finite = (__float_as_uint(norm32) & 0x7f800000u) != 0x7f800000u;   // the exponent field itself: no floating-point compare to reason about
    ctl[SEA_CTL_GRAD_NORM] = __float_as_int(norm32);
    if (!finite && skip_nonfinite) {   // the step is dropped: step and the bias corrections keep the last applied step's values
        ctl[SEA_CTL_CLIP] = __float_as_int(0.f);
        ctl[SEA_CTL_APPLIED] = 0;
        ctl[SEA_CTL_SKIPPED] += 1;
        return;
    }
    const int step = ctl[SEA_CTL_STEP] + 1;
    const double bc1 = 1.0 - powi_f64((double)beta1, step), bc2 = 1.0 - powi_f64((double)beta2, step);
    double clip = 1.0;
    if (max_norm > 0.f && finite) clip = fmin(1.0, (double)max_norm / (norm + 1e-6));   // torch.nn.utils.clip_grad_norm_
    const float clip32 = (float)clip;
    ctl[SEA_CTL_CLIP] = __float_as_int(clip32);
    ctl[SEA_CTL_INV_BC1] = __float_as_int((float)(1.0 / bc1));
    ctl[SEA_CTL_INV_SQRT_BC2] = __float_as_int((float)(1.0 / sqrt(bc2)));
    ctl[SEA_CTL_APPLIED] = 1;
    ctl[SEA_CTL_STEP] = step;
    if (clip32 < 1.f) ctl[SEA_CTL_CLIPPED] += 1;
}

extern "C" int sea_grad_norm_ctl(const float* g, int64_t n, float grad_scale, float max_norm, int skip_nonfinite, float beta1, float beta2,
                                 double* partial, int n_partial_cap, int32_t* ctl, void* stream) {
    SEA_REQUIRE(g && partial && ctl, "sea_grad_norm_ctl: null pointer");
    SEA_REQUIRE(n >= 4 && n % 4 == 0, "sea_grad_norm_ctl: n=%lld must be a positive multiple of 4", (long long)n);
    SEA_REQUIRE(sea_aligned16(g) && sea_aligned16(ctl) && (reinterpret_cast<uintptr_t>(partial) & 7u) == 0,
                "sea_grad_norm_ctl: g and ctl must be 16-byte aligned, partial 8-byte aligned");
    SEA_REQUIRE(n_partial_cap >= 1, "sea_grad_norm_ctl: partial workspace too small");
    SEA_REQUIRE(beta1 >= 0.f && beta1 < 1.f && beta2 >= 0.f && beta2 < 1.f, "sea_grad_norm_ctl: betas (%g, %g) must lie in [0, 1)", (double)beta1, (double)beta2);
    SEA_REQUIRE(max_norm == max_norm, "sea_grad_norm_ctl: max_norm is NaN (<= 0 means no clipping)");
    const int64_t n4 = n / 4;
    int64_t blocks = (n4 + 255) / 256;
    if (blocks > 1024) blocks = 1024;
    if (blocks > n_partial_cap) blocks = n_partial_cap;
    hipStream_t s = static_cast<hipStream_t>(stream);
    grad_norm_partial_kernel<<<dim3((unsigned)blocks), dim3(256), 0, s>>>(g, n4, partial);
    grad_norm_final_kernel<<<dim3(1), dim3(256), 0, s>>>(partial, (int)blocks, grad_scale, max_norm, skip_nonfinite, beta1, beta2, ctl);
    SEA_CHECK_LAUNCH("sea_grad_norm_ctl");
    return SEA_OK;
}

// ---------------------------------------------------------------------------------------------- AdamW steered by the control block
// adamw_flat_kernel with grad_scale * clip, the two bias corrections and the applied flag read from the control block sea_grad_norm_ctl wrote on the
// same stream (wave-uniform loads).  A copy, not a shared body: the launch of sea_adamw_flat stays the code it was.  A skipped step returns before
// any load or store of p, m, v or the shadow.
template <typename T>
__global__ __launch_bounds__(256) void adamw_flat_ctl_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                             float* __restrict__ v, T* __restrict__ shadow, int64_t n4, float lr, float beta1,
                                                             float beta2, float eps, float lr_wd, float grad_scale, const int32_t* __restrict__ ctl) {
    if (ctl[SEA_CTL_APPLIED] == 0) return;
    const float inv_bc1 = __int_as_float(ctl[SEA_CTL_INV_BC1]), inv_sqrt_bc2 = __int_as_float(ctl[SEA_CTL_INV_SQRT_BC2]);
    const float gscale = mul1(grad_scale, __int_as_float(ctl[SEA_CTL_CLIP]));
    // scalar-lane helpers pin the evaluation order, as in adamw_flat_kernel (b m + (1-b) g must not become g + b (m - g))
    const float omb1 = 1.0f - beta1, omb2 = 1.0f - beta2, step_size = lr * inv_bc1;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        float pp[4], gg[4], mm[4], vv[4];
        load4(p + 4 * i, pp);
        load4(g + 4 * i, gg);
        load4(m + 4 * i, mm);
        load4(v + 4 * i, vv);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float gr = mul1(gg[e], gscale);
            if (lr_wd != 0.f) pp[e] = fma1(-lr_wd, pp[e], pp[e]);   // p - (lr*wd) p, as in adamw_flat_kernel
            mm[e] = fma1(beta1, mm[e], mul1(omb1, gr));
            vv[e] = fma1(beta2, vv[e], mul1(mul1(omb2, gr), gr));
            // plain C from here (adamw_flat_kernel: the wait states after v_sqrt / v_rcp are inserted for compiled code only)
            const float denom = sqrtf(vv[e]) * inv_sqrt_bc2 + eps;
            pp[e] -= step_size * (mm[e] / denom);
        }
        store4(p + 4 * i, pp[0], pp[1], pp[2], pp[3]);
        store4(m + 4 * i, mm[0], mm[1], mm[2], mm[3]);
        store4(v + 4 * i, vv[0], vv[1], vv[2], vv[3]);
        if (shadow != nullptr) store4(shadow + 4 * i, pp[0], pp[1], pp[2], pp[3]);
    }
}

extern "C" int sea_adamw_flat_ctl(float* p, const float* g, float* m, float* v, void* shadow, int shadow_dtype, int64_t n, float lr, float beta1,
                                  float beta2, float eps, float weight_decay, float grad_scale, const int32_t* ctl, void* stream) {
    SEA_REQUIRE(p && g && m && v && ctl, "sea_adamw_flat_ctl: null pointer");
    SEA_REQUIRE(n >= 4 && n % 4 == 0, "sea_adamw_flat_ctl: n=%lld must be a positive multiple of 4", (long long)n);
    SEA_REQUIRE(sea_aligned16(p) && sea_aligned16(g) && sea_aligned16(m) && sea_aligned16(v) && sea_aligned16(shadow) && sea_aligned16(ctl),
                "sea_adamw_flat_ctl: pointers must be 16-byte aligned");
    SEA_REQUIRE(!shadow || shadow_dtype == SEA_BF16 || shadow_dtype == SEA_F32, "sea_adamw_flat_ctl: bad shadow dtype");
    const int64_t n4 = n / 4;
    int64_t blocks = (n4 + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const float lr_wd = (float)((double)lr * (double)weight_decay);
    if (shadow != nullptr && shadow_dtype == SEA_BF16)
        adamw_flat_ctl_kernel<__bf16><<<dim3((unsigned)blocks), dim3(256), 0, s>>>(p, g, m, v, static_cast<__bf16*>(shadow), n4, lr, beta1, beta2, eps,
                                                                                  lr_wd, grad_scale, ctl);
    else
        adamw_flat_ctl_kernel<float><<<dim3((unsigned)blocks), dim3(256), 0, s>>>(p, g, m, v, static_cast<float*>(shadow), n4, lr, beta1, beta2, eps,
                                                                                 lr_wd, grad_scale, ctl);
    SEA_CHECK_LAUNCH("sea_adamw_flat_ctl");
    return SEA_OK;
}
