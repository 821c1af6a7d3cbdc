// Verification of an ensemble against sensor readings (gfx950): sea_ensemble_verify.  From the members' predictions at K sensors, the readings, their
// precisions and the members' log-weights: CRPS, PIT, rank, mean and spread per (history, sensor), and per history the fp64 sums and the rank
// histogram (include/sea_hip.h states the formulas).  Two launches, both without atomics to global memory, spin-waits or any exchange between
// workgroups; every loop bound is a kernel argument; every early exit is taken by the whole workgroup between barriers.
//
// verify_kernel<V>: one workgroup of 256 threads per (tile of 16 sensors, history); V = 1 up to 64 members, 2 above.
//   1  the history's weights, in fp64: the log-weights go to LDS, every thread walks them in ascending order (broadcast reads) for the maximum, the
//      sum of the exponentials and q = sum w^2 — the same bits in every thread and in every tile of the history.
//   2  the tile's N x 16 block of pred is read along each member row (64-byte segments) and staged as [sensor][member | 1] fp32 (an odd row stride: the
//      transposing stores and the per-sensor reads both stay off one bank).
//   3  wave w takes sensors w, w + 4, ...: lane l holds member l (and l + 64), walks j = 0 .. N - 1 with broadcast LDS reads and accumulates the
//      weight below its own member under the total order (value, member index); that gives the pair sum of the CRPS without a sort.  The lane
//      terms are reduced by a fixed xor butterfly (the mean first: the spread is centred on it).  A dead reading is passed over by its wave.
//   4  thread k of the tile finishes sensor k (the selects on c, the fp32 stores) and files its terms; threads 0 .. 7 add the tile's terms in
//      ascending sensor order; the partial histogram is counted in LDS with integer adds (order-independent).  Both go to the workspace.
// verify_finish_kernel: one workgroup per history adds the tiles' partials in ascending tile order into sums and hist (or onto them: accumulate);
// the partial sums come through LDS 256 tiles at a time, so that their loads are in flight together and only the additions are serial.
// What bounds it: per sensor a wave pays N broadcast reads, compares and fp64 adds per lane and two rounds of butterflies; a workgroup therefore
// holds only 16 sensors, four per wave, and a few hundred sensors already spread over the chip; below that the two launches' latency.
#include "verify_score.hpp"   // the per-reading arithmetic, shared with decode_member_verify_kernel (decode_loss.hip)
#include "brier_score.hpp"    // the per-reading threshold scores, shared with decode_member_brier_kernel (decode_loss.hip)

constexpr int VF_THREADS = 256;
constexpr int VF_TILE = 16;    // sensors per workgroup: four per wave
constexpr int VF_FIN_TILES = 256;   // tiles whose partial sums the finish kernel holds in LDS at a time

static inline int64_t vf_tile_words(int N) { return VF_SUMS + (N + 2) / 2; }   // 8-byte words per (history, tile): 8 sums, then N + 1 int32 bins

template <int V>
__global__ __launch_bounds__(VF_THREADS) void verify_kernel(const SeaEnsembleVerify p, const int tiles, const int words) {
#pragma clang fp reassociate(off)
    extern __shared__ __attribute__((aligned(16))) float vf_stage[];   // [VF_TILE][N | 1]
    __shared__ double lw_s[VF_MAX_N], w_s[VF_MAX_N];
    __shared__ int live_s[VF_MAX_N];
    __shared__ double r_mean[VF_TILE], r_var[VF_TILE], r_abs[VF_TILE], r_pair[VF_TILE], r_pit[VF_TILE];
    __shared__ int r_rank[VF_TILE], r_state[VF_TILE];                  // state: 0 live and good, 1 dead, 2 bad
    __shared__ double term_s[VF_SUMS][VF_TILE];
    __shared__ int hist_s[VF_MAX_N + 1];
    __shared__ float y_s[VF_TILE], pv_s[VF_TILE];                      // the tile's readings and precisions: no global load inside the sensor loop

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tile = blockIdx.x, b = blockIdx.y;
    const int N = p.N, K = p.K, SLD = N | 1;
    const int k0 = tile * VF_TILE;
    const int kcn = K - k0 < VF_TILE ? K - k0 : VF_TILE;
    const float* pred = p.pred + (int64_t)b * N * p.ld_pred;
    const float* obs = p.obs + (int64_t)b * p.ld_obs;
    const float* prec = p.prec != nullptr ? p.prec + (int64_t)b * p.ld_prec : nullptr;
    const int64_t orow = (int64_t)b * p.ld_out;
    double* wsum = reinterpret_cast<double*>(p.work) + ((int64_t)b * tiles + tile) * words;
    int32_t* whist = reinterpret_cast<int32_t*>(wsum + VF_SUMS);

    // 1: the weights of the history
    int invalid = 0, alive = 0;
    if (tid < N) {
        const float lw = p.logw != nullptr ? p.logw[(int64_t)b * N + tid] : 0.f;
        invalid = (lw != lw || lw == INFINITY) ? 1 : 0;
        alive = (!invalid && lw != -INFINITY) ? 1 : 0;
        lw_s[tid] = (double)lw;
        live_s[tid] = alive;
    }
    for (int r = tid; r <= N; r += VF_THREADS) hist_s[r] = 0;
    const int n_live = __syncthreads_count(alive);
    invalid = __syncthreads_or(invalid);
    if (invalid || n_live == 0) {   // uniform: the history is not scored
        if (tid < kcn) {
            if (p.mean != nullptr) p.mean[orow + k0 + tid] = 0.f;
            if (p.spread != nullptr) p.spread[orow + k0 + tid] = 0.f;
            if (p.crps != nullptr) p.crps[orow + k0 + tid] = 0.f;
            if (p.pit != nullptr) p.pit[orow + k0 + tid] = 0.f;
            if (p.rank != nullptr) p.rank[orow + k0 + tid] = -1;
        }
        if (tid < VF_SUMS) wsum[tid] = 0.0;
        for (int r = tid; r <= N; r += VF_THREADS) whist[r] = 0;
        if (tile == 0 && tid == 0) p.status[b] = -1;
        return;
    }
    double mx = -INFINITY;
    for (int j = 0; j < N; ++j) mx = lw_s[j] > mx ? lw_s[j] : mx;
    if (tid < N) w_s[tid] = alive ? exp(lw_s[tid] - mx) : 0.0;
    __syncthreads();
    double W = 0.0;
    for (int j = 0; j < N; ++j) W += w_s[j];
    const double my_w = tid < N ? w_s[tid] / W : 0.0;
    __syncthreads();   // every thread has read the exponentials
    if (tid < N) w_s[tid] = my_w;

    // 2: the tile's predictions, [sensor][member]
    for (int e = tid; e < N * VF_TILE; e += VF_THREADS) {
        const int j = e / VF_TILE, kc = e % VF_TILE;
        if (kc < kcn) vf_stage[kc * SLD + j] = pred[(int64_t)j * p.ld_pred + k0 + kc];
    }
    if (tid < kcn) {
        y_s[tid] = obs[k0 + tid];
        pv_s[tid] = prec != nullptr ? prec[k0 + tid] : 1.f;
    }
    __syncthreads();
    double q = 0.0;
    for (int j = 0; j < N; ++j) q = fma(w_s[j], w_s[j], q);
    const double c = p.unbiased ? 1.0 - q : 1.0;

    // 3: a sensor per wave at a time
    for (int kc = wave; kc < kcn; kc += 4) {
        const float pv = pv_s[kc];
        if (!(pv > 0.f)) {   // the same word in every lane: the wave passes a dead reading over, whatever obs and pred hold there
            if (lane == 0) r_state[kc] = 1;
            continue;
        }
        const VfReading r = vf_score_wave<V>(vf_stage + kc * SLD, w_s, live_s, N, lane, y_s[kc], pv);
        if (lane == 0) {
            r_mean[kc] = r.mean;
            r_var[kc] = r.var;
            r_abs[kc] = r.ab;
            r_pair[kc] = r.pair;
            r_pit[kc] = r.pit;
            r_rank[kc] = r.rank;
            r_state[kc] = r.state;
        }
    }
    __syncthreads();

    // 4: thread k finishes sensor k
    if (tid < VF_TILE) {
        double t[VF_SUMS];
#pragma unroll
        for (int i = 0; i < VF_SUMS; ++i) t[i] = 0.0;
        if (tid < kcn) {
            VfReading r;
            r.mean = r_mean[tid];
            r.var = r_var[tid];
            r.ab = r_abs[tid];
            r.pair = r_pair[tid];
            r.pit = r_pit[tid];
            r.rank = r_rank[tid];
            r.state = r_state[tid];
            const VfOut o = vf_finish_reading(r, y_s[tid], pv_s[tid], c, t);
            if (r.state == 0) atomicAdd(&hist_s[o.rank], 1);   // LDS, integers: the order does not matter; 0 <= rank <= N
            if (p.mean != nullptr) p.mean[orow + k0 + tid] = o.mean;
            if (p.spread != nullptr) p.spread[orow + k0 + tid] = o.spread;
            if (p.crps != nullptr) p.crps[orow + k0 + tid] = o.crps;
            if (p.pit != nullptr) p.pit[orow + k0 + tid] = o.pit;
            if (p.rank != nullptr) p.rank[orow + k0 + tid] = o.rank;
        }
#pragma unroll
        for (int i = 0; i < VF_SUMS; ++i) term_s[i][tid] = t[i];
    }
    __syncthreads();
    if (tid < VF_SUMS) {
        double s = 0.0;
        for (int k = 0; k < kcn; ++k) s += term_s[tid][k];
        wsum[tid] = s;
    }
    for (int r = tid; r <= N; r += VF_THREADS) whist[r] = hist_s[r];
    if (tile == 0 && tid == 0) p.status[b] = n_live;
}

__global__ __launch_bounds__(VF_THREADS) void verify_finish_kernel(const SeaEnsembleVerify p, const int tiles, const int words) {
#pragma clang fp reassociate(off)
    __shared__ double part[VF_FIN_TILES][VF_SUMS];   // a chunk of the tiles' partial sums: read together, then added in ascending tile order
    const int tid = threadIdx.x, b = blockIdx.x, N = p.N;
    const double* base = reinterpret_cast<const double*>(p.work) + (int64_t)b * tiles * words;
    double acc = 0.0;
    for (int t0 = 0; t0 < tiles; t0 += VF_FIN_TILES) {
        const int n = tiles - t0 < VF_FIN_TILES ? tiles - t0 : VF_FIN_TILES;
        for (int e = tid; e < n * VF_SUMS; e += VF_THREADS) part[e / VF_SUMS][e % VF_SUMS] = base[(int64_t)(t0 + e / VF_SUMS) * words + e % VF_SUMS];
        __syncthreads();
        if (tid < VF_SUMS)
            for (int t = 0; t < n; ++t) acc += part[t][tid];
        __syncthreads();   // the chunk has been consumed
    }
    if (tid < VF_SUMS) {
        double* dst = p.sums + (int64_t)b * VF_SUMS + tid;
        *dst = p.accumulate ? *dst + acc : acc;
    }
    for (int r = tid; r <= N; r += VF_THREADS) {
        int64_t s = 0;
#pragma unroll 8
        for (int t = 0; t < tiles; ++t) s += reinterpret_cast<const int32_t*>(base + (int64_t)t * words + VF_SUMS)[r];   // integers: any order
        int64_t* dst = p.hist + (int64_t)b * (N + 1) + r;
        *dst = p.accumulate ? *dst + s : s;
    }
}

static inline bool vf_aligned8(const void* q) { return (reinterpret_cast<uintptr_t>(q) & 7u) == 0; }

extern "C" int64_t sea_ensemble_verify_ws_bytes(int B, int N, int K) {
    if (B < 1 || B > 65535 || N < 1 || N > VF_MAX_N || K < 1) return -1;
    const int64_t tiles = ((int64_t)K + VF_TILE - 1) / VF_TILE;
    return (int64_t)B * tiles * vf_tile_words(N) * 8;
}

template <int V>
static void verify_launch(const SeaEnsembleVerify& p, int tiles, hipStream_t s) {
    const int lds = VF_TILE * (p.N | 1) * (int)sizeof(float);
    verify_kernel<V><<<dim3((unsigned)tiles, (unsigned)p.B), dim3(VF_THREADS), lds, s>>>(p, tiles, (int)vf_tile_words(p.N));
    sea_note_form("verify", V, lds);
}

extern "C" int sea_ensemble_verify(const SeaEnsembleVerify* pp, void* stream) {
    SEA_REQUIRE(pp != nullptr, "sea_ensemble_verify: null argument table");
    const SeaEnsembleVerify& p = *pp;
    SEA_REQUIRE(p.pred != nullptr && p.obs != nullptr && p.sums != nullptr && p.hist != nullptr && p.status != nullptr && p.work != nullptr,
                "sea_ensemble_verify: null pointer (pred, obs, sums, hist, status and work are required; prec, logw and the per-sensor outputs may be NULL)");
    SEA_REQUIRE(sea_aligned4(p.pred) && sea_aligned4(p.obs) && sea_aligned4(p.prec) && sea_aligned4(p.logw) && sea_aligned4(p.mean) && sea_aligned4(p.spread) &&
                    sea_aligned4(p.crps) && sea_aligned4(p.pit) && sea_aligned4(p.rank) && sea_aligned4(p.status) && vf_aligned8(p.sums) && vf_aligned8(p.hist) &&
                    vf_aligned8(p.work),
                "sea_ensemble_verify: misaligned pointer (f32 and int32 buffers need 4 bytes; sums, hist and work 8)");
    SEA_REQUIRE(p.B >= 1 && p.B <= 65535, "sea_ensemble_verify: B=%d histories outside 1 .. 65535", p.B);
    SEA_REQUIRE(p.N >= 1, "sea_ensemble_verify: N=%d must be positive", p.N);
    SEA_REQUIRE(p.K >= 1, "sea_ensemble_verify: K=%d must be positive", p.K);
    SEA_REQUIRE(p.ld_pred >= p.K && p.ld_obs >= p.K, "sea_ensemble_verify: ld_pred=%lld and ld_obs=%lld must cover K=%d", (long long)p.ld_pred, (long long)p.ld_obs, p.K);
    SEA_REQUIRE(p.prec == nullptr || p.ld_prec == 0 || p.ld_prec >= p.K, "sea_ensemble_verify: ld_prec=%lld must be 0 (one row for all histories) or cover K=%d",
                (long long)p.ld_prec, p.K);
    SEA_REQUIRE((p.mean == nullptr && p.spread == nullptr && p.crps == nullptr && p.pit == nullptr && p.rank == nullptr) || p.ld_out >= p.K,
                "sea_ensemble_verify: ld_out=%lld must cover K=%d", (long long)p.ld_out, p.K);
    SEA_REQUIRE((p.unbiased == 0 || p.unbiased == 1) && (p.accumulate == 0 || p.accumulate == 1), "sea_ensemble_verify: unbiased=%d and accumulate=%d must be 0 or 1",
                p.unbiased, p.accumulate);
    if (p.N > VF_MAX_N) {
        sea_set_error("sea_ensemble_verify: unsupported: N=%d members above %d", p.N, VF_MAX_N);
        return SEA_EUNSUPPORTED;
    }
    const int64_t need = sea_ensemble_verify_ws_bytes(p.B, p.N, p.K);
    SEA_REQUIRE(p.work_bytes >= need, "sea_ensemble_verify: work_bytes=%lld below the %lld that sea_ensemble_verify_ws_bytes(B=%d, N=%d, K=%d) asks for",
                (long long)p.work_bytes, (long long)need, p.B, p.N, p.K);
    const int tiles = (int)(((int64_t)p.K + VF_TILE - 1) / VF_TILE);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (p.N <= 64) verify_launch<1>(p, tiles, s);
    else verify_launch<2>(p, tiles, s);
    verify_finish_kernel<<<dim3((unsigned)p.B), dim3(VF_THREADS), 0, s>>>(p, tiles, (int)vf_tile_words(p.N));
    SEA_CHECK_LAUNCH("sea_ensemble_verify");
    return SEA_OK;
}

// ------------------------------------------------------------------------------------------------------------------------------------------------
// sea_ensemble_brier: the threshold scores of an ensemble at sensors — Brier sums, the histograms of the reliability diagram and the hit counts of the ROC
// (include/sea_hip.h states the definitions) — from predictions that already exist.  verify_kernel's grid and staging; the reading is scored by the device
// functions decode_member_brier_kernel runs per cell (brier_score.hpp).
// brier_kernel<V>: one workgroup of 256 threads per (tile of 16 sensors, history).
//   1  the history's weights (bs_history_weights); 2  the tile's N x 16 block of pred staged as [sensor][member | 1], the readings, precisions and the
//   sensors' thresholds; 3  wave w scores sensors w, w + 4, ... (bs_column_wave); 4  thread (k, t), k + 16 t, finishes threshold t of sensor k — the maps, the
//   terms, the LDS histograms; thread (t, i) adds the tile's terms in ascending sensor order.  brier_finish_kernel: a workgroup per (history, threshold) adds the tiles in ascending order.
template <int V>
__global__ __launch_bounds__(VF_THREADS) void brier_kernel(const SeaEnsembleBrier p, const int tiles, const int words) {
#pragma clang fp reassociate(off)
    extern __shared__ __attribute__((aligned(16))) float vf_stage[];   // [VF_TILE][N | 1]
    __shared__ double lw_s[VF_MAX_N], w_s[VF_MAX_N];
    __shared__ int live_s[VF_MAX_N];
    __shared__ BsCell cell_s[VF_TILE];
    __shared__ double term_s[BS_MAX_T * BS_SUMS][VF_TILE];
    __shared__ int hist_s[2 * BS_MAX_T * (VF_MAX_N + 1)];   // [hist | hits][t][m] at the call's T and N
    __shared__ float y_s[VF_TILE], pv_s[VF_TILE], thr_s[VF_TILE][BS_MAX_T];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tile = blockIdx.x, b = blockIdx.y;
    const int N = p.N, K = p.K, T = p.n_thr, SLD = N | 1, nb = T * (N + 1);
    const int k0 = tile * VF_TILE;
    const int kcn = K - k0 < VF_TILE ? K - k0 : VF_TILE;
    const float* pred = p.pred + (int64_t)b * N * p.ld_pred;
    const float* obs = p.obs + (int64_t)b * p.ld_obs;
    const float* prec = p.prec != nullptr ? p.prec + (int64_t)b * p.ld_prec : nullptr;
    const int64_t orow = (int64_t)b * p.ld_out;
    double* wsum = reinterpret_cast<double*>(p.work) + ((int64_t)b * tiles + tile) * words;
    int32_t* whist = reinterpret_cast<int32_t*>(wsum + T * BS_SUMS);

    for (int r = tid; r < 2 * nb; r += VF_THREADS) hist_s[r] = 0;
    double W;
    const int n_live = bs_history_weights(p.logw, b, N, tid, lw_s, w_s, live_s, W);
    if (tile == 0 && tid == 0) p.status[b] = n_live;
    if (n_live < 0) {   // uniform: the history is not scored
        if (tid < kcn)
            for (int t = 0; t < T; ++t) {
                if (p.prob != nullptr) p.prob[t * p.ld_map + orow + k0 + tid] = 0.f;
                if (p.brier != nullptr) p.brier[t * p.ld_map + orow + k0 + tid] = 0.f;
            }
        for (int e = tid; e < words; e += VF_THREADS) wsum[e] = 0.0;   // the sums, and the int32 bins: all bits zero
        return;
    }

    // 2: the tile's predictions, [sensor][member]
    for (int e = tid; e < N * VF_TILE; e += VF_THREADS) {
        const int j = e / VF_TILE, kc = e % VF_TILE;
        if (kc < kcn) vf_stage[kc * SLD + j] = pred[(int64_t)j * p.ld_pred + k0 + kc];
    }
    if (tid < kcn) {
        y_s[tid] = obs[k0 + tid];
        pv_s[tid] = prec != nullptr ? prec[k0 + tid] : 1.f;
    }
    if (tid < VF_TILE * T) {
        const int kc = tid & (VF_TILE - 1), t = tid / VF_TILE;
        if (kc < kcn) thr_s[kc][t] = p.thr[(int64_t)t * p.ld_thr + k0 + kc];
    }
    __syncthreads();

    // 3: a sensor per wave at a time
    for (int kc = wave; kc < kcn; kc += 4) {
        const float pv = pv_s[kc];
        if (!(pv > 0.f)) {   // the same word in every lane: the wave passes a dead reading over, whatever obs and pred hold there
            if (lane == 0) cell_s[kc].state = 1;
            continue;
        }
        bs_column_wave<V>(vf_stage + kc * SLD, w_s, live_s, N, lane, W, y_s[kc], pv, thr_s[kc], T, &cell_s[kc]);
    }
    __syncthreads();

    // 4: thread (k, q) finishes threshold q of sensor k
    if (tid < VF_TILE * T) {
        const int k = tid & (VF_TILE - 1), q = tid / VF_TILE;
        double tm[BS_SUMS];
#pragma unroll
        for (int i = 0; i < BS_SUMS; ++i) tm[i] = 0.0;
        if (k < kcn) {
            const BsOut o = bs_finish_cell(cell_s[k], q, y_s[k], thr_s[k][q], tm);
            if (o.m >= 0) {   // LDS, integers: the order does not matter; 0 <= m <= N
                atomicAdd(&hist_s[q * (N + 1) + o.m], 1);
                if (o.o) atomicAdd(&hist_s[nb + q * (N + 1) + o.m], 1);
            }
            const int64_t at = q * p.ld_map + orow + k0 + k;
            if (p.prob != nullptr) p.prob[at] = o.prob;
            if (p.brier != nullptr) p.brier[at] = o.brier;
        }
#pragma unroll
        for (int i = 0; i < BS_SUMS; ++i) term_s[q * BS_SUMS + i][k] = tm[i];
    }
    __syncthreads();
    if (tid < T * BS_SUMS) {
        double s = 0.0;
        for (int k = 0; k < kcn; ++k) s += term_s[tid][k];
        wsum[tid] = s;
    }
    for (int r = tid; r < 2 * nb; r += VF_THREADS) whist[r] = hist_s[r];
}

__global__ __launch_bounds__(VF_THREADS) void brier_finish_kernel(const SeaEnsembleBrier p, const int tiles, const int words) {
    const int b = blockIdx.x, t = blockIdx.y, N = p.N, T = p.n_thr;   // a workgroup per (history, threshold)
    const double* part = reinterpret_cast<const double*>(p.work) + (int64_t)b * tiles * words;
    const int64_t o = (int64_t)b * T + t;
    bs_finish_threshold(part, tiles, words, T, N, t, p.sums + o * BS_SUMS, p.hist + o * (N + 1), p.hits + o * (N + 1), p.accumulate, threadIdx.x, VF_THREADS);
}

extern "C" int64_t sea_ensemble_brier_ws_bytes(int B, int N, int K, int n_thr) {
    if (B < 1 || B > 65535 || N < 1 || N > VF_MAX_N || K < 1 || n_thr < 1 || n_thr > BS_MAX_T) return -1;
    const int64_t tiles = ((int64_t)K + VF_TILE - 1) / VF_TILE;
    return (int64_t)B * tiles * bs_words(n_thr, N) * 8;
}

template <int V>
static void brier_launch(const SeaEnsembleBrier& p, int tiles, hipStream_t s) {
    const int lds = VF_TILE * (p.N | 1) * (int)sizeof(float);
    brier_kernel<V><<<dim3((unsigned)tiles, (unsigned)p.B), dim3(VF_THREADS), lds, s>>>(p, tiles, (int)bs_words(p.n_thr, p.N));
    sea_note_form("brier", V, lds);
}

extern "C" int sea_ensemble_brier(const SeaEnsembleBrier* pp, void* stream) {
    SEA_REQUIRE(pp != nullptr, "sea_ensemble_brier: null argument table");
    const SeaEnsembleBrier& p = *pp;
    SEA_REQUIRE(p.pred != nullptr && p.obs != nullptr && p.thr != nullptr && p.sums != nullptr && p.hist != nullptr && p.hits != nullptr && p.status != nullptr &&
                    p.work != nullptr,
                "sea_ensemble_brier: null pointer (pred, obs, thr, sums, hist, hits, status and work are required; prec, logw and the maps may be NULL)");
    SEA_REQUIRE(sea_aligned4(p.pred) && sea_aligned4(p.obs) && sea_aligned4(p.prec) && sea_aligned4(p.logw) && sea_aligned4(p.thr) && sea_aligned4(p.prob) &&
                    sea_aligned4(p.brier) && sea_aligned4(p.status) && vf_aligned8(p.sums) && vf_aligned8(p.hist) && vf_aligned8(p.hits) && vf_aligned8(p.work),
                "sea_ensemble_brier: misaligned pointer (f32 and int32 buffers need 4 bytes; sums, hist, hits and work 8)");
    SEA_REQUIRE(p.B >= 1 && p.B <= 65535, "sea_ensemble_brier: B=%d histories outside 1 .. 65535", p.B);
    SEA_REQUIRE(p.N >= 1, "sea_ensemble_brier: N=%d must be positive", p.N);
    SEA_REQUIRE(p.K >= 1, "sea_ensemble_brier: K=%d must be positive", p.K);
    SEA_REQUIRE(p.n_thr >= 1 && p.n_thr <= BS_MAX_T, "sea_ensemble_brier: n_thr=%d outside 1 .. %d", p.n_thr, BS_MAX_T);
    SEA_REQUIRE(p.ld_pred >= p.K && p.ld_obs >= p.K && p.ld_thr >= p.K, "sea_ensemble_brier: ld_pred=%lld, ld_obs=%lld and ld_thr=%lld must cover K=%d",
                (long long)p.ld_pred, (long long)p.ld_obs, (long long)p.ld_thr, p.K);
    SEA_REQUIRE(p.prec == nullptr || p.ld_prec == 0 || p.ld_prec >= p.K, "sea_ensemble_brier: ld_prec=%lld must be 0 (one row for all histories) or cover K=%d",
                (long long)p.ld_prec, p.K);
    SEA_REQUIRE((p.prob == nullptr && p.brier == nullptr) || (p.ld_out >= p.K && p.ld_map >= (int64_t)p.B * p.ld_out),
                "sea_ensemble_brier: ld_out=%lld must cover K=%d, and ld_map=%lld a whole map", (long long)p.ld_out, p.K, (long long)p.ld_map);
    SEA_REQUIRE(p.accumulate == 0 || p.accumulate == 1, "sea_ensemble_brier: accumulate=%d must be 0 or 1", p.accumulate);
    if (p.N > VF_MAX_N) {
        sea_set_error("sea_ensemble_brier: unsupported: N=%d members above %d", p.N, VF_MAX_N);
        return SEA_EUNSUPPORTED;
    }
    const int64_t need = sea_ensemble_brier_ws_bytes(p.B, p.N, p.K, p.n_thr);
    SEA_REQUIRE(p.work_bytes >= need, "sea_ensemble_brier: work_bytes=%lld below the %lld that sea_ensemble_brier_ws_bytes(B=%d, N=%d, K=%d, n_thr=%d) asks for",
                (long long)p.work_bytes, (long long)need, p.B, p.N, p.K, p.n_thr);
    const int tiles = (int)(((int64_t)p.K + VF_TILE - 1) / VF_TILE);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (p.N <= 64) brier_launch<1>(p, tiles, s);
    else brier_launch<2>(p, tiles, s);
    brier_finish_kernel<<<dim3((unsigned)p.B, (unsigned)p.n_thr), dim3(VF_THREADS), 0, s>>>(p, tiles, (int)bs_words(p.n_thr, p.N));
    SEA_CHECK_LAUNCH("sea_ensemble_brier");
    return SEA_OK;
}
