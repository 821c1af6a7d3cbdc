// Ensemble resampling on the device (gfx950): sea_resample_systematic.  Log-weights of G histories with n members each become the int32 index that
// sea_kv_cache_gather (RolloutSession.resample / select) takes — normalisation, cumulative sum, effective sample size, the decision whether to resample
// at all and the n searches in ONE launch, one workgroup per history, everything in fp64:
//   1  every thread owns a run of ceil(n / 256) consecutive members: it finds the maximum of the live ones (finite log-weight), the workgroup reduces it
//      (a maximum does not depend on the order) together with the index of the last live member;
//   2  w = exp(logw - mx) (0 for a dead member) goes to LDS; the thread sums its run and the squares in index order; a Hillis-Steele scan over the 256
//      run sums (8 steps, two LDS images) gives each run its offset, and the run is rewritten in place as the inclusive cumulative sum c.  The order of
//      every addition is fixed by n alone: two runs give the same bits;
//   3  ess = W^2 / sum w^2 decides, uniformly for the workgroup; member j then either searches c for the first entry above (j + u) / n * W (binary
//      search in LDS; c is non-decreasing and the first entry above a threshold belongs to a member of positive weight) or keeps its own index and
//      gets its normalised log-weight.
// What bounds it: nothing but latency — 32 kB of LDS, a few barriers and 12 dependent LDS reads per member; the launch itself is most of the time.
#include "sea_common.hpp"

#include <math.h>

constexpr int RS_THREADS = 256;
constexpr int RS_MAX_N = 4096;

__device__ __forceinline__ bool rs_live(float v) { return !(isnan(v) || isinf(v)); }

__global__ __launch_bounds__(RS_THREADS) void resample_systematic_kernel(const float* __restrict__ logw, const float* __restrict__ u, float ess_frac, int n,
                                                                          int32_t* __restrict__ index, float* __restrict__ logw_out, float* __restrict__ ess_out,
                                                                          int32_t* __restrict__ resampled) {
    __shared__ double c[RS_MAX_N];
    __shared__ double scan_w[2][RS_THREADS];
    __shared__ double scan_q[2][RS_THREADS];
    __shared__ float red_mx[RS_THREADS / 64];
    __shared__ int red_last[RS_THREADS / 64];

    const int g = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* lw = logw + (int64_t)g * n;
    const int per = (n + RS_THREADS - 1) / RS_THREADS;
    const int j0 = tid * per < n ? tid * per : n, j1 = j0 + per < n ? j0 + per : n;

    // 1: maximum over the live members, index of the last live one (-1: none)
    float mx = -INFINITY;
    int last = -1;
    for (int j = j0; j < j1; ++j) {
        const float v = lw[j];
        if (rs_live(v)) {
            mx = fmaxf(mx, v);
            last = j;
        }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        mx = fmaxf(mx, __shfl_xor(mx, o));
        const int other = __shfl_xor(last, o);
        last = other > last ? other : last;
    }
    if (lane == 0) {
        red_mx[wave] = mx;
        red_last[wave] = last;
    }
    __syncthreads();
    mx = fmaxf(fmaxf(red_mx[0], red_mx[1]), fmaxf(red_mx[2], red_mx[3]));
    last = max(max(red_last[0], red_last[1]), max(red_last[2], red_last[3]));

    int32_t* idx = index + (int64_t)g * n;
    float* lo = logw_out + (int64_t)g * n;
    if (last < 0) {   // no live member (uniform): identity, zero log-weights
        for (int j = tid; j < n; j += RS_THREADS) {
            idx[j] = g * n + j;
            lo[j] = 0.f;
        }
        if (tid == 0) {
            ess_out[g] = 0.f;
            resampled[g] = -1;
        }
        return;
    }

    // 2: weights, run sums in index order, scan of the run sums
    const double dmx = (double)mx;
    double sw = 0.0, sq = 0.0;
    for (int j = j0; j < j1; ++j) {
        const float v = lw[j];
        const double w = rs_live(v) ? exp((double)v - dmx) : 0.0;
        c[j] = w;
        sw += w;
        sq += w * w;
    }
    scan_w[0][tid] = sw;
    scan_q[0][tid] = sq;
    __syncthreads();
    int cur = 0;
#pragma unroll
    for (int o = 1; o < RS_THREADS; o <<= 1) {
        double a = scan_w[cur][tid], b = scan_q[cur][tid];
        if (tid >= o) {
            a += scan_w[cur][tid - o];
            b += scan_q[cur][tid - o];
        }
        scan_w[cur ^ 1][tid] = a;
        scan_q[cur ^ 1][tid] = b;
        cur ^= 1;
        __syncthreads();
    }
    double run = tid > 0 ? scan_w[cur][tid - 1] : 0.0;   // exclusive offset of this thread's run
    for (int j = j0; j < j1; ++j) {
        run += c[j];
        c[j] = run;
    }
    __syncthreads();
    const double W = c[n - 1], Q = scan_q[cur][RS_THREADS - 1];
    const double ess = W * W / Q;
    const bool doit = ess_frac < 0.f || ess < (double)ess_frac * (double)n;

    // 3
    if (doit) {
        const double ug = (double)u[g];
        for (int j = tid; j < n; j += RS_THREADS) {
            const double thr = ((double)j + ug) / (double)n * W;
            int lo_i = 0, hi_i = n;   // first i in [0, n) with c[i] > thr, n when there is none
            while (lo_i < hi_i) {
                const int mid = (lo_i + hi_i) >> 1;
                if (c[mid] > thr) hi_i = mid;
                else lo_i = mid + 1;
            }
            idx[j] = g * n + (lo_i < last ? lo_i : last);
            lo[j] = 0.f;
        }
    } else {
        const double shift = dmx + log(W);
        for (int j = tid; j < n; j += RS_THREADS) {
            const float v = lw[j];
            idx[j] = g * n + j;
            lo[j] = rs_live(v) ? (float)((double)v - shift) : -INFINITY;
        }
    }
    if (tid == 0) {
        ess_out[g] = (float)ess;
        resampled[g] = doit ? 1 : 0;
    }
}

extern "C" int sea_resample_systematic(const float* logw, const float* u, float ess_frac, int G, int n, int32_t* index, float* logw_out, float* ess, int32_t* resampled,
                                       void* stream) {
    SEA_REQUIRE(logw != nullptr && u != nullptr && index != nullptr && logw_out != nullptr && ess != nullptr && resampled != nullptr,
                "sea_resample_systematic: null pointer (logw, u, index, logw_out, ess and resampled are all required)");
    SEA_REQUIRE(G >= 1, "sea_resample_systematic: G=%d must be positive", G);
    SEA_REQUIRE(n >= 1, "sea_resample_systematic: n=%d must be positive", n);
    SEA_REQUIRE(!(ess_frac != ess_frac), "sea_resample_systematic: ess_frac is NaN");
    SEA_REQUIRE(sea_aligned4(logw) && sea_aligned4(u) && sea_aligned4(index) && sea_aligned4(logw_out) && sea_aligned4(ess) && sea_aligned4(resampled),
                "sea_resample_systematic: misaligned pointer");
    if (n > RS_MAX_N) {
        sea_set_error("sea_resample_systematic: unsupported: n=%d members per history above %d", n, RS_MAX_N);
        return SEA_EUNSUPPORTED;
    }
    SEA_REQUIRE((int64_t)G * n <= 0x7fffffffLL, "sea_resample_systematic: G * n = %lld does not fit an int32 index", (long long)G * n);
    resample_systematic_kernel<<<dim3((unsigned)G), dim3(RS_THREADS), 0, static_cast<hipStream_t>(stream)>>>(logw, u, ess_frac, n, index, logw_out, ess, resampled);
    SEA_CHECK_LAUNCH("sea_resample_systematic");
    return SEA_OK;
}
