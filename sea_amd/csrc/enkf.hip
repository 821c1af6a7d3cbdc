// Ensemble Kalman analysis in ensemble space (gfx950): sea_enkf_transform, sea_enkf_transform_gram and sea_ensemble_mix.  The deterministic EnKF of Sakov & Oke (2008): from the
// members' predictions at K sensors, the readings and their precisions, one [N, N] matrix D per (history, analysis domain) such that the analysed
// state of member j is y[j] + sum_i D[i, j] y[i] (include/sea_hip.h states the formulas).  Two launches, both without atomics, spin-waits or any
// exchange between workgroups; every loop bound is a kernel argument.
//
// sea_enkf_transform: one workgroup of 256 threads per (domain, history); the whole problem lives in it, in fp64.
//   1  C = S S^T and v = S delta over the sensors: the threads form a 16 x 16 grid, thread (ti, tj) owns the R x R register block of C at rows
//      ti + 16 r, columns tj + 16 c (R = 1, 2, 4, 8 for N <= 16, 32, 64, 128) and the R entries of v at its rows.  The sensors come through LDS in chunks of
//      256 / R: the raw predictions [sensor][member], then thread k of the chunk sums its sensor's column in member order (the mean), forms the
//      weight, the scale and the innovation, and the chunk is rewritten in place as S.  A chunk without a live sensor is passed over by the whole
//      workgroup (adding its zeros would change no bit).  Every sum runs over the sensors in ascending order: the bits depend on (N, K) alone.
//   2  the chunk region is overlaid by ONE [N][N | 1] image of I + C (132 kB at N = 128; an odd row stride keeps column walks off one bank), and
//      LAPACK's potrf -> trtri -> lauum order runs in place in it: a right-looking Cholesky (column scale, then the rank-1 update of the trailing
//      triangle over the thread grid), the inverse of the triangular factor by elementary column eliminations (row scale, rank-1 update of the
//      rectangle below-left, column finish), and W = X^T X accumulated in the same register blocks as C and written back over X.
//   3  u = W v / sqrt(N - 1), the column means of G, and D in fp32.
//   A live operand that is not finite, or a pivot that is not a positive finite number, gives status -1 and D = 0 (no update); every such exit is
//   taken by the whole workgroup at once, between barriers.
// What bounds it: at few sensors the 5 barriers per elimination step (latency); at thousands of sensors the fp64 FMAs of step 1 (N^2 K).
//
// sea_enkf_transform_gram: the second form of the transform.  Step 1 is a weighted sum of Q partial Gram matrices per history (sea_decode_member_gram's
// outputs, decode_loss.hip) in the same thread grid and register blocks; steps 2 and 3 are the device function ek_analyse, which both kernels call.
//
// sea_ensemble_mix: one workgroup per (patch, history).  The N member rows of the patch come through LDS in chunks of 64 columns of the flattened
// (group, latent) range as fp32; wave w produces members w, w + 4, ...: fp32 FMAs over i in ascending order with D[i, j] uniform over the wave
// (read from an LDS copy of the problem's D up to 64 members, from global memory above).
#include "sea_common.hpp"

#include <math.h>

constexpr int EK_THREADS = 256;
constexpr int EK_MAX_N = 128;
constexpr int EK_MIX_COLS = 64;
constexpr int EK_MIX_STAGE_N = 64;

template <int R>
constexpr int ek_lds_bytes() {   // the larger of the sensor chunk [256 / R][16 R + 1] and the largest image [N][N | 1] of the form (N <= 16 R)
    constexpr int stage = (256 / R) * (16 * R + 1), image = 16 * R * (16 * R + 1);
    return 8 * (stage > image ? stage : image);
}

// Steps 2 and 3 of the analysis, shared by both forms of the transform: from a thread grid's register blocks of C (acc) and v (vac) to D and status.
// Called by the whole workgroup; ek_lds is free to be overlaid after the barrier at the top.
template <int R>
__device__ __forceinline__ void ek_analyse(double (&acc)[R][R], double (&vac)[R], int bad, const int nlive, double* ek_lds, double* v_s, double* u_s, double* cm_s,
                                           const int N, const double rho, const double alpha, const double inv_n, const double inv_sqrt_nm1, float* Dout,
                                           int32_t* status) {
#pragma clang fp reassociate(off)
    const int tid = threadIdx.x, tj = tid & 15, ti = tid >> 4;
    __syncthreads();   // the last chunk has been consumed: the image may overlay it

    // 2: the image of I + C, v
    const int LD = N | 1;
    double* M = ek_lds;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int i = ti + 16 * r;
#pragma unroll
        for (int c = 0; c < R; ++c) {
            const int j = tj + 16 * c;
            if (i < N && j < N) M[i * LD + j] = acc[r][c] + (i == j ? 1.0 : 0.0);
        }
        if (tj == 0 && i < N) v_s[i] = vac[r];
    }
    __syncthreads();
    if (tid < N && !isfinite(v_s[tid])) bad = 1;
    bad = __syncthreads_or(bad);

    if (!bad) {   // uniform
        // potrf (lower): L L^T = I + C
        for (int k = 0; k < N; ++k) {
            const double piv = M[k * LD + k];                       // the same LDS word for every thread: the exit is uniform
            if (!(piv > 0.0 && isfinite(piv))) {
                bad = 1;
                break;
            }
            const double dk = sqrt(piv), ik = 1.0 / dk;
            for (int i = k + 1 + tid; i < N; i += EK_THREADS) M[i * LD + k] *= ik;
            __syncthreads();
            if (tid == 0) M[k * LD + k] = dk;
            for (int i = k + 1 + ti; i < N; i += 16) {
                const double lik = M[i * LD + k];
                for (int j = k + 1 + tj; j <= i; j += 16) M[i * LD + j] -= lik * M[j * LD + k];
            }
            __syncthreads();
        }
    }
    if (bad) {    // uniform: no update for this problem
        for (int e = tid; e < N * N; e += EK_THREADS) Dout[e] = 0.f;
        if (tid == 0) *status = -1;
        return;
    }

    // trtri (lower, in place): X = L^-1 as the product of the inverses of L's elementary column matrices, first column first
    for (int k = 0; k < N; ++k) {
        const double dk = 1.0 / M[k * LD + k];
        for (int j = tid; j < k; j += EK_THREADS) M[k * LD + j] *= dk;
        __syncthreads();
        for (int i = k + 1 + ti; i < N; i += 16) {
            const double lik = M[i * LD + k];
            for (int j = tj; j < k; j += 16) M[i * LD + j] -= lik * M[k * LD + j];
        }
        __syncthreads();
        for (int i = k + 1 + tid; i < N; i += EK_THREADS) M[i * LD + k] *= -dk;
        if (tid == 0) M[k * LD + k] = dk;
        __syncthreads();
    }

    // lauum: W = X^T X, W[i][j] = sum_{l >= max(i, j)} X[l][i] X[l][j], in the register blocks, then over X
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int c = 0; c < R; ++c) acc[r][c] = 0.0;
    for (int l = ti > tj ? ti : tj; l < N; ++l) {
        const double* row = M + l * LD;
        double a[R], bb[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            a[r] = ti + 16 * r <= l ? row[ti + 16 * r] : 0.0;
            bb[r] = tj + 16 * r <= l ? row[tj + 16 * r] : 0.0;
        }
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
            for (int c = 0; c < R; ++c) acc[r][c] = fma(a[r], bb[c], acc[r][c]);
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int i = ti + 16 * r;
#pragma unroll
        for (int c = 0; c < R; ++c) {
            const int j = tj + 16 * c;
            if (i < N && j < N) M[i * LD + j] = acc[r][c];
        }
    }
    __syncthreads();

    // 3: u = W v / sqrt(N - 1); G = u 1^T - alpha (I - W); D = (rho - 1) Pi + rho (G - its column means)
    if (tid < N) {
        double s = 0.0;
        for (int j = 0; j < N; ++j) s = fma(M[tid * LD + j], v_s[j], s);
        u_s[tid] = s * inv_sqrt_nm1;
    }
    __syncthreads();
    if (tid < N) {
        double s = 0.0;
        for (int i = 0; i < N; ++i) s += u_s[i] - alpha * ((i == tid ? 1.0 : 0.0) - M[i * LD + tid]);
        cm_s[tid] = s * inv_n;
    }
    __syncthreads();
    for (int e = tid; e < N * N; e += EK_THREADS) {
        const int i = e / N, j = e - i * N;
        const double eye = i == j ? 1.0 : 0.0;
        const double g = u_s[i] - alpha * (eye - M[i * LD + j]);
        Dout[e] = (float)((rho - 1.0) * (eye - inv_n) + rho * (g - cm_s[j]));
    }
    if (tid == 0) *status = nlive;
}

template <int R>
__global__ __launch_bounds__(EK_THREADS) void enkf_transform_kernel(const SeaEnkfTransform p, const double inv_n, const double inv_nm1, const double inv_sqrt_nm1) {
#pragma clang fp reassociate(off)
    constexpr int NS = 16 * R, KC = 256 / R, SLD = NS + 1;
    extern __shared__ __attribute__((aligned(16))) double ek_lds[];   // the sensor chunk [KC][SLD], later the image [N][LD]
    __shared__ double ybar_s[KC], scl_s[KC], dlt_s[KC];
    __shared__ double v_s[EK_MAX_N], u_s[EK_MAX_N], cm_s[EK_MAX_N];

    const int tid = threadIdx.x, tj = tid & 15, ti = tid >> 4;
    const int d = blockIdx.x, b = blockIdx.y;
    const int N = p.N, K = p.K;
    const float* pred = p.pred + (int64_t)b * N * p.ld_pred;
    const float* obs = p.obs + (int64_t)b * p.ld_obs;
    const float* prec = p.prec != nullptr ? p.prec + (int64_t)b * p.ld_prec : nullptr;
    const float* tap = p.taper != nullptr ? p.taper + (int64_t)d * p.ld_taper : nullptr;
    float* Dout = p.D + ((int64_t)b * p.Ld + d) * N * N;
    int32_t* status = p.status + (int64_t)b * p.Ld + d;
    const double rho = p.rho, alpha = p.alpha;

    // 1: C and v over the sensors
    double acc[R][R], vac[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        vac[r] = 0.0;
#pragma unroll
        for (int c = 0; c < R; ++c) acc[r][c] = 0.0;
    }
    int nlive = 0, bad = 0;
    double* st = ek_lds;
    for (int k0 = 0; k0 < K; k0 += KC) {
        const int kcn = K - k0 < KC ? K - k0 : KC;
        double w = 0.0;
        if (tid < kcn) {
            const float pv = prec != nullptr ? prec[k0 + tid] : 1.f;
            const float tv = tap != nullptr ? tap[k0 + tid] : 1.f;
            w = (pv > 0.f ? (double)pv : 0.0) * (tv > 0.f ? (double)tv : 0.0);
        }
        const bool live = w > 0.0;
        const int cnt = __syncthreads_count(live);   // also: the chunk before this one has been consumed
        if (cnt == 0) continue;                      // uniform: no live sensor in the chunk
        nlive += cnt;
        for (int e = tid; e < N * KC; e += EK_THREADS) {
            const int j = e / KC, kc = e % KC;
            if (kc < kcn) st[kc * SLD + j] = (double)pred[(int64_t)j * p.ld_pred + k0 + kc];
        }
        __syncthreads();
        if (tid < kcn) {
            double s = 0.0;
            for (int j = 0; j < N; ++j) s += st[tid * SLD + j];
            const double yb = s * inv_n;
            const double sc = live ? rho * sqrt(w * inv_nm1) : 0.0;
            const double dl = live ? sqrt(w) * ((double)obs[k0 + tid] - yb) : 0.0;
            if (live && !(isfinite(sc) && isfinite(dl))) bad = 1;
            ybar_s[tid] = yb;
            scl_s[tid] = sc;
            dlt_s[tid] = dl;
        }
        __syncthreads();
        for (int e = tid; e < N * KC; e += EK_THREADS) {
            const int j = e / KC, kc = e % KC;
            if (kc < kcn) {
                const double sc = scl_s[kc];
                const double s = sc > 0.0 ? (st[kc * SLD + j] - ybar_s[kc]) * sc : 0.0;
                if (!isfinite(s)) bad = 1;
                st[kc * SLD + j] = s;
            }
        }
        __syncthreads();
        for (int kc = 0; kc < kcn; ++kc) {
            const double* row = st + kc * SLD;
            const double dl = dlt_s[kc];
            double a[R], bb[R];
#pragma unroll
            for (int r = 0; r < R; ++r) {
                a[r] = row[ti + 16 * r];
                bb[r] = row[tj + 16 * r];
            }
#pragma unroll
            for (int r = 0; r < R; ++r) {
                vac[r] = fma(a[r], dl, vac[r]);
#pragma unroll
                for (int c = 0; c < R; ++c) acc[r][c] = fma(a[r], bb[c], acc[r][c]);
            }
        }
    }
    ek_analyse<R>(acc, vac, bad, nlive, ek_lds, v_s, u_s, cm_s, N, rho, alpha, inv_n, inv_sqrt_nm1, Dout, status);
}

template <int R>
static void enkf_transform_launch(const SeaEnkfTransform& p, hipStream_t s) {
    constexpr int lds = ek_lds_bytes<R>();
    static bool set_on[64] = {false};   // per device: R = 8 needs 132 kB, above the 64 kB a kernel gets without the attribute
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = -1;
    if (dev < 0 || !set_on[dev]) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(enkf_transform_kernel<R>), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
        if (dev >= 0) set_on[dev] = true;
    }
    const double n = (double)p.N;
    enkf_transform_kernel<R><<<dim3((unsigned)p.Ld, (unsigned)p.B), dim3(EK_THREADS), lds, s>>>(p, 1.0 / n, 1.0 / (n - 1.0), 1.0 / sqrt(n - 1.0));
    sea_note_form("enkf.transform", R, lds);
}

extern "C" int sea_enkf_transform(const SeaEnkfTransform* pp, void* stream) {
    SEA_REQUIRE(pp != nullptr, "sea_enkf_transform: null argument table");
    const SeaEnkfTransform& p = *pp;
    SEA_REQUIRE(p.pred != nullptr && p.obs != nullptr && p.D != nullptr && p.status != nullptr,
                "sea_enkf_transform: null pointer (pred, obs, D and status are required; prec and taper may be NULL)");
    SEA_REQUIRE(sea_aligned4(p.pred) && sea_aligned4(p.obs) && sea_aligned4(p.prec) && sea_aligned4(p.taper) && sea_aligned4(p.D) && sea_aligned4(p.status),
                "sea_enkf_transform: misaligned pointer");
    SEA_REQUIRE(p.B >= 1 && p.B <= 65535, "sea_enkf_transform: B=%d histories outside 1 .. 65535", p.B);
    SEA_REQUIRE(p.N >= 2, "sea_enkf_transform: N=%d: an analysis needs at least 2 members", p.N);
    SEA_REQUIRE(p.K >= 1, "sea_enkf_transform: K=%d must be positive", p.K);
    SEA_REQUIRE(p.Ld >= 1, "sea_enkf_transform: Ld=%d must be positive", p.Ld);
    SEA_REQUIRE(p.taper != nullptr || p.Ld == 1, "sea_enkf_transform: Ld=%d domains need a taper", p.Ld);
    SEA_REQUIRE(p.ld_pred >= p.K && p.ld_obs >= p.K, "sea_enkf_transform: ld_pred=%lld and ld_obs=%lld must cover K=%d", (long long)p.ld_pred, (long long)p.ld_obs, p.K);
    SEA_REQUIRE(p.prec == nullptr || p.ld_prec == 0 || p.ld_prec >= p.K, "sea_enkf_transform: ld_prec=%lld must be 0 (one row for all histories) or cover K=%d",
                (long long)p.ld_prec, p.K);
    SEA_REQUIRE(p.taper == nullptr || p.ld_taper >= p.K, "sea_enkf_transform: ld_taper=%lld must cover K=%d", (long long)p.ld_taper, p.K);
    SEA_REQUIRE(p.rho >= 1.0 && p.rho < INFINITY, "sea_enkf_transform: inflation rho=%g must be finite and >= 1", p.rho);
    SEA_REQUIRE(p.alpha >= 0.0 && p.alpha <= 1.0, "sea_enkf_transform: anomaly gain alpha=%g outside [0, 1]", p.alpha);
    if (p.N > EK_MAX_N) {
        sea_set_error("sea_enkf_transform: unsupported: N=%d members above %d", p.N, EK_MAX_N);
        return SEA_EUNSUPPORTED;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (p.N <= 16) enkf_transform_launch<1>(p, s);
    else if (p.N <= 32) enkf_transform_launch<2>(p, s);
    else if (p.N <= 64) enkf_transform_launch<4>(p, s);
    else enkf_transform_launch<8>(p, s);
    SEA_CHECK_LAUNCH("sea_enkf_transform");
    return SEA_OK;
}

// ------------------------------------------------------------------------------------------------------------------------------------------------
// sea_enkf_transform_gram: the same analysis from Q partial Gram matrices per history (sea_decode_member_gram's outputs, one per patch) instead of the
// sensors' predictions.  Step 1 becomes a weighted sum of the partials in ascending q, in the same thread grid and register blocks:
//     C = rho^2 / (N - 1) sum_q t_q gram[b, q],   v = rho / sqrt(N - 1) sum_q t_q proj[b, q],   t_q = taper[d, q] > 0 ? taper[d, q] : 0  (NULL: 1)
// A partial with t_q = 0 or count 0 is passed over by the whole workgroup (every thread reads the same two words); a contributing count of -1, or
// a sum that is not finite, takes the no-update exit of ek_analyse.  Steps 2 and 3 are ek_analyse, the code of the sensor form.
template <int R>
__global__ __launch_bounds__(EK_THREADS) void enkf_transform_gram_kernel(const SeaEnkfTransformGram p, const double inv_n, const double c_scale, const double v_scale,
                                                                         const double inv_sqrt_nm1) {
#pragma clang fp reassociate(off)
    extern __shared__ __attribute__((aligned(16))) double ek_lds[];   // the image [N][N | 1]
    __shared__ double v_s[EK_MAX_N], u_s[EK_MAX_N], cm_s[EK_MAX_N];
    const int tid = threadIdx.x, tj = tid & 15, ti = tid >> 4;
    const int d = blockIdx.x, b = blockIdx.y;
    const int N = p.N, Q = p.Q;
    const float* tap = p.taper != nullptr ? p.taper + (int64_t)d * p.ld_taper : nullptr;
    float* Dout = p.D + ((int64_t)b * p.Ld + d) * N * N;
    int32_t* status = p.status + (int64_t)b * p.Ld + d;

    double acc[R][R], vac[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        vac[r] = 0.0;
#pragma unroll
        for (int c = 0; c < R; ++c) acc[r][c] = 0.0;
    }
    int nlive = 0, bad = 0;
    for (int q = 0; q < Q; ++q) {
        const float tv = tap != nullptr ? tap[q] : 1.f;
        const int cnt = p.count[(int64_t)b * Q + q];
        if (!(tv > 0.f) || cnt == 0) continue;   // uniform: the same words for every thread
        if (cnt < 0) {
            bad = 1;
            continue;
        }
        nlive += cnt;
        const double t = (double)tv;
        const double* g = p.gram + ((int64_t)b * Q + q) * N * N;
        const double* pr = p.proj + ((int64_t)b * Q + q) * N;
        // rows and columns at or beyond N are clamped to N - 1: their register blocks repeat real entries and are never stored
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int i = ti + 16 * r < N ? ti + 16 * r : N - 1;
            vac[r] = fma(t, pr[i], vac[r]);
#pragma unroll
            for (int c = 0; c < R; ++c) {
                const int j = tj + 16 * c < N ? tj + 16 * c : N - 1;
                acc[r][c] = fma(t, g[i * N + j], acc[r][c]);
            }
        }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
        vac[r] *= v_scale;
        if (!isfinite(vac[r])) bad = 1;
#pragma unroll
        for (int c = 0; c < R; ++c) {
            acc[r][c] *= c_scale;
            if (!isfinite(acc[r][c])) bad = 1;
        }
    }
    ek_analyse<R>(acc, vac, bad, nlive, ek_lds, v_s, u_s, cm_s, N, p.rho, p.alpha, inv_n, inv_sqrt_nm1, Dout, status);
}

template <int R>
static void enkf_transform_gram_launch(const SeaEnkfTransformGram& p, hipStream_t s) {
    constexpr int lds = 8 * 16 * R * (16 * R + 1);
    static bool set_on[64] = {false};   // per device: R = 8 needs 132 kB, above the 64 kB a kernel gets without the attribute
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = -1;
    if (dev < 0 || !set_on[dev]) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(enkf_transform_gram_kernel<R>), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
        if (dev >= 0) set_on[dev] = true;
    }
    const double n = (double)p.N;
    enkf_transform_gram_kernel<R><<<dim3((unsigned)p.Ld, (unsigned)p.B), dim3(EK_THREADS), lds, s>>>(p, 1.0 / n, p.rho * p.rho / (n - 1.0), p.rho / sqrt(n - 1.0),
                                                                                                   1.0 / sqrt(n - 1.0));
    sea_note_form("enkf.transform_gram", R, lds);
}

extern "C" int sea_enkf_transform_gram(const SeaEnkfTransformGram* pp, void* stream) {
    SEA_REQUIRE(pp != nullptr, "sea_enkf_transform_gram: null argument table");
    const SeaEnkfTransformGram& p = *pp;
    SEA_REQUIRE(p.gram != nullptr && p.proj != nullptr && p.count != nullptr && p.D != nullptr && p.status != nullptr,
                "sea_enkf_transform_gram: null pointer (gram, proj, count, D and status are required; taper may be NULL)");
    SEA_REQUIRE((reinterpret_cast<uintptr_t>(p.gram) & 7u) == 0 && (reinterpret_cast<uintptr_t>(p.proj) & 7u) == 0 && sea_aligned4(p.count) && sea_aligned4(p.taper) &&
                    sea_aligned4(p.D) && sea_aligned4(p.status),
                "sea_enkf_transform_gram: misaligned pointer");
    SEA_REQUIRE(p.B >= 1 && p.B <= 65535, "sea_enkf_transform_gram: B=%d histories outside 1 .. 65535", p.B);
    SEA_REQUIRE(p.N >= 2, "sea_enkf_transform_gram: N=%d: an analysis needs at least 2 members", p.N);
    SEA_REQUIRE(p.Q >= 1, "sea_enkf_transform_gram: Q=%d partials must be positive", p.Q);
    SEA_REQUIRE(p.Ld >= 1, "sea_enkf_transform_gram: Ld=%d must be positive", p.Ld);
    SEA_REQUIRE(p.taper != nullptr || p.Ld == 1, "sea_enkf_transform_gram: Ld=%d domains need a taper", p.Ld);
    SEA_REQUIRE(p.taper == nullptr || p.ld_taper >= p.Q, "sea_enkf_transform_gram: ld_taper=%lld must cover Q=%d", (long long)p.ld_taper, p.Q);
    SEA_REQUIRE(p.rho >= 1.0 && p.rho < INFINITY, "sea_enkf_transform_gram: inflation rho=%g must be finite and >= 1", p.rho);
    SEA_REQUIRE(p.alpha >= 0.0 && p.alpha <= 1.0, "sea_enkf_transform_gram: anomaly gain alpha=%g outside [0, 1]", p.alpha);
    if (p.N > EK_MAX_N) {
        sea_set_error("sea_enkf_transform_gram: unsupported: N=%d members above %d", p.N, EK_MAX_N);
        return SEA_EUNSUPPORTED;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (p.N <= 16) enkf_transform_gram_launch<1>(p, s);
    else if (p.N <= 32) enkf_transform_gram_launch<2>(p, s);
    else if (p.N <= 64) enkf_transform_gram_launch<4>(p, s);
    else enkf_transform_gram_launch<8>(p, s);
    SEA_CHECK_LAUNCH("sea_enkf_transform_gram");
    return SEA_OK;
}

// ------------------------------------------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(EK_THREADS) void ensemble_mix_kernel(const SeaEnsembleMix p) {
#pragma clang fp reassociate(off)
    __shared__ float ysh[EK_MAX_N * EK_MIX_COLS];
    __shared__ float dsh[EK_MIX_STAGE_N * EK_MIX_STAGE_N];   // the problem's D up to 64 members: its reads then leave the chain of global loads
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int pch = blockIdx.x, b = blockIdx.y;
    const int N = p.N, G = p.G, Dl = p.Dl;
    const int64_t E = (int64_t)p.P * Dl;                 // a group's row of a member
    const int ncol = G * Dl;                             // the patch's columns over all groups
    const float* Dm = p.D + ((int64_t)b * p.Ld + (p.Ld == 1 ? 0 : pch)) * N * N;
    const T* y = static_cast<const T*>(p.y);
    T* out = static_cast<T*>(p.out);
    const bool staged = N <= EK_MIX_STAGE_N;   // uniform
    if (staged)
        for (int e = tid; e < N * N; e += EK_THREADS) dsh[e] = Dm[e];   // visible after the first barrier below
    for (int c0 = 0; c0 < ncol; c0 += EK_MIX_COLS) {
        const int c = c0 + lane;
        const bool on = c < ncol;
        const int g = on ? c / Dl : 0, e = on ? c - g * Dl : 0;
        const int64_t off = (int64_t)g * E + (int64_t)pch * Dl + e;
        for (int i = wave; i < N; i += 4) ysh[i * EK_MIX_COLS + lane] = on ? to_f32(y[((int64_t)b * N + i) * G * E + off]) : 0.f;
        __syncthreads();
        for (int j = wave; j < N; j += 4) {
            float acc = 0.f;
            if (staged)
                for (int i = 0; i < N; ++i) acc = __builtin_fmaf(dsh[i * N + j], ysh[i * EK_MIX_COLS + lane], acc);
            else
                for (int i = 0; i < N; ++i) acc = __builtin_fmaf(Dm[(int64_t)i * N + j], ysh[i * EK_MIX_COLS + lane], acc);
            if (on) {
                const int64_t idx = ((int64_t)b * N + j) * G * E + off;
                if (p.inc != nullptr) p.inc[idx] = acc;
                if (out != nullptr) out[idx] = from_f32<T>(ysh[j * EK_MIX_COLS + lane] + acc);
            }
        }
        __syncthreads();
    }
}

extern "C" int sea_ensemble_mix(const SeaEnsembleMix* pp, int dtype, void* stream) {
    SEA_REQUIRE(pp != nullptr, "sea_ensemble_mix: null argument table");
    const SeaEnsembleMix& p = *pp;
    SEA_REQUIRE(dtype == SEA_F32 || dtype == SEA_BF16, "sea_ensemble_mix: dtype=%d is neither SEA_F32 nor SEA_BF16", dtype);
    SEA_REQUIRE(p.y != nullptr && p.D != nullptr, "sea_ensemble_mix: null pointer (y and D are required)");
    SEA_REQUIRE(p.out != nullptr || p.inc != nullptr, "sea_ensemble_mix: neither out nor inc is given");
    const int esz = dtype == SEA_BF16 ? 2 : 4;
    SEA_REQUIRE((reinterpret_cast<uintptr_t>(p.y) & (esz - 1)) == 0 && (reinterpret_cast<uintptr_t>(p.out) & (esz - 1)) == 0 && sea_aligned4(p.D) && sea_aligned4(p.inc),
                "sea_ensemble_mix: misaligned pointer");
    SEA_REQUIRE(p.N >= 2, "sea_ensemble_mix: N=%d: an ensemble needs at least 2 members", p.N);
    SEA_REQUIRE(p.Bm >= p.N && p.Bm % p.N == 0, "sea_ensemble_mix: Bm=%d must be a positive multiple of N=%d", p.Bm, p.N);
    SEA_REQUIRE(p.G >= 1 && p.P >= 1 && p.Dl >= 1, "sea_ensemble_mix: G=%d, P=%d and Dl=%d must be positive", p.G, p.P, p.Dl);
    SEA_REQUIRE(p.Ld == 1 || p.Ld == p.P, "sea_ensemble_mix: Ld=%d must be 1 or P=%d", p.Ld, p.P);
    SEA_REQUIRE(p.Bm / p.N <= 65535, "sea_ensemble_mix: %d histories; a launch carries up to 65535", p.Bm / p.N);
    SEA_REQUIRE((int64_t)p.G * p.Dl <= 0x7fffffffLL, "sea_ensemble_mix: G * Dl = %lld does not fit an int", (long long)p.G * p.Dl);
    if (p.out != nullptr) {   // out must not overlap y: a member's row is read after other members' rows have been written
        const uintptr_t bytes = (uintptr_t)p.Bm * p.G * p.P * p.Dl * esz, a = reinterpret_cast<uintptr_t>(p.y), o = reinterpret_cast<uintptr_t>(p.out);
        SEA_REQUIRE(o + bytes <= a || a + bytes <= o, "sea_ensemble_mix: out aliases y");
    }
    if (p.N > EK_MAX_N) {
        sea_set_error("sea_ensemble_mix: unsupported: N=%d members above %d", p.N, EK_MAX_N);
        return SEA_EUNSUPPORTED;
    }
    const dim3 grid((unsigned)p.P, (unsigned)(p.Bm / p.N));
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (dtype == SEA_BF16) ensemble_mix_kernel<__bf16><<<grid, dim3(EK_THREADS), 0, s>>>(p);
    else ensemble_mix_kernel<float><<<grid, dim3(EK_THREADS), 0, s>>>(p);
    sea_note_form(dtype == SEA_BF16 ? "enkf.mix_bf16" : "enkf.mix_f32", p.Ld == 1 ? 0 : 1, 0);
    SEA_CHECK_LAUNCH("sea_ensemble_mix");
    return SEA_OK;
}
