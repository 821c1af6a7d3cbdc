// Threshold scores of an ensemble at one reading: the device code shared by decode_member_brier_kernel (decode_loss.hip: a reading is a cell of a dense
// snapshot) and brier_kernel (verify.hip: a reading is a sensor).  include/sea_hip.h (sea_decode_member_brier, sea_ensemble_brier) states the definitions.
//   bs_history_weights  the history's members from its log-weights, sea_ensemble_verify's step 1 without the normalisation: e_j = exp(lw_j - mx), W = sum e_j
//   bs_column_wave<V>   one wave scores one reading: lane l holds member l (and l + 64 at V = 2) through qs_load_column; per threshold the weight above it
//                       (qs_exceed_sum: the butterfly of qs_column_wave's exceedance, so p = e / W has that launch's bits) and the number of live members
//                       above it (two ballots)
//   bs_finish_cell      one thread finishes one (reading, threshold): o, (p - o)^2, the two f32 map values and the five terms of the sums
//   bs_finish_threshold one workgroup adds the partial sums of one (history, field, threshold) in ascending order of its parts, and its integer histograms
// Workspace of a part (a workgroup of launch 1): T * 5 fp64 sums [t][i], then 2 * T * (N + 1) int32 bins [hist | hits][t][m].
#pragma once
#include "quantile_select.hpp"

constexpr int BS_MAX_T = SEA_QUANTILE_MAX_LEVELS;   // thresholds per call
constexpr int BS_SUMS = SEA_BRIER_SUMS;             // count, sum (p - o)^2, sum p, sum o, count of bad readings

static inline int64_t bs_words(int T, int N) { return (int64_t)T * BS_SUMS + ((int64_t)2 * T * (N + 1) + 1) / 2; }   // 8-byte words per part

struct BsCell {   // what a wave leaves per reading; state: 0 live and good, 1 dead, 2 bad
    double p[BS_MAX_T];
    int m[BS_MAX_T];
    int state, pad_;
};

// Every thread of the workgroup calls this (two barriers inside); tid < N needs a workgroup of at least N threads.  Returns the number of live members, or
// -1 for a history that is not scored (a log-weight NaN or +inf, or no live member); then w_s and W are not set.  w_s[j] = e_j (0 for a dead member).
__device__ __forceinline__ int bs_history_weights(const float* logw, const int64_t b, const int N, const int tid, double* lw_s, double* w_s, int* live_s, double& W) {
#pragma clang fp reassociate(off)
    int invalid = 0, alive = 0;
    if (tid < N) {
        const float lw = logw != nullptr ? logw[b * N + tid] : 0.f;
        invalid = (lw != lw || lw == INFINITY) ? 1 : 0;
        alive = (!invalid && lw != -INFINITY) ? 1 : 0;
        lw_s[tid] = (double)lw;
        live_s[tid] = alive;
    }
    const int n_live = __syncthreads_count(alive);
    invalid = __syncthreads_or(invalid);
    W = 0.0;
    if (invalid || n_live == 0) return -1;   // uniform over the workgroup
    double mx = -INFINITY;
    for (int j = 0; j < N; ++j) mx = lw_s[j] > mx ? lw_s[j] : mx;
    if (tid < N) w_s[tid] = alive ? exp(lw_s[tid] - mx) : 0.0;
    __syncthreads();
    for (int j = 0; j < N; ++j) W += w_s[j];   // one chain, j ascending: the same bits in every thread
    return n_live;
}

// row: the reading's member values [N] in LDS; w_s, live_s, W: bs_history_weights'; yf, pv: the reading and its precision (pv > 0: the caller passes a dead
// reading over); thr: the reading's nt thresholds.  Lane 0 files the result.
template <int V>
__device__ __forceinline__ void bs_column_wave(const float* row, const double* w_s, const int* live_s, const int N, const int lane, const double W, const float yf,
                                               const float pv, const float* thr, const int nt, BsCell* out) {
#pragma clang fp reassociate(off)
    float x[V];
    double w[V];
    bool lv[V];
    const int bad = qs_load_column<V>(row, w_s, live_s, N, lane, x, w, lv) | (isfinite(yf) ? 0 : 1) | (isfinite(pv) ? 0 : 1);
    for (int t = 0; t < nt; ++t) {
        const float th = thr[t];
        const double e = qs_exceed_sum<V>(x, w, lv, th);
        int m = 0;
#pragma unroll
        for (int v = 0; v < V; ++v) m += __popcll(__ballot(lv[v] && x[v] > th));
        if (lane == 0) {
            out->p[t] = e / W;
            out->m[t] = m;
        }
    }
    if (lane == 0) out->state = bad ? 2 : 0;
}

struct BsOut {
    float prob, brier;
    int m, o;   // m = -1: the reading is in no bin
};

__device__ __forceinline__ BsOut bs_finish_cell(const BsCell& c, const int t, const float yf, const float th, double (&tm)[BS_SUMS]) {
#pragma clang fp reassociate(off)
    BsOut r;
    r.prob = r.brier = 0.f;
    r.m = -1;
    r.o = 0;
#pragma unroll
    for (int i = 0; i < BS_SUMS; ++i) tm[i] = 0.0;
    if (c.state == 2) {
        r.prob = r.brier = NAN;
        tm[4] = 1.0;
    } else if (c.state == 0) {
        const double p = c.p[t];
        r.o = yf > th ? 1 : 0;
        const double d = p - (double)r.o;
        const double sq = d * d;
        r.m = c.m[t];
        r.prob = (float)p;
        r.brier = (float)sq;
        tm[0] = 1.0;
        tm[1] = sq;
        tm[2] = p;
        tm[3] = (double)r.o;
    }
    return r;
}

// One workgroup finishes one (history, field, threshold t).  part: the words of the field in the history's first part; stride: 8-byte words between two
// parts; sums [5], hist and hits [N + 1]: the outputs of this (history, field, threshold).  The fp64 sums are added in ascending order of the parts.
__device__ __forceinline__ void bs_finish_threshold(const double* part, const int n_parts, const int64_t stride, const int T, const int N, const int t, double* sums,
                                                    int64_t* hist, int64_t* hits, const int accumulate, const int tid, const int nthreads) {
#pragma clang fp reassociate(off)
    const int ns = T * BS_SUMS, nb = T * (N + 1);
    for (int e = tid; e < BS_SUMS + 2 * (N + 1); e += nthreads) {
        if (e < BS_SUMS) {
            double acc = 0.0;
#pragma unroll 8
            for (int pt = 0; pt < n_parts; ++pt) acc += part[(int64_t)pt * stride + t * BS_SUMS + e];   // parts ascending
            sums[e] = accumulate ? sums[e] + acc : acc;
        } else {
            const int r = e - BS_SUMS, which = r / (N + 1), m = r - which * (N + 1);   // which: 0 hist, 1 hits
            const int idx = which * nb + t * (N + 1) + m;
            int64_t s = 0;
#pragma unroll 8
            for (int pt = 0; pt < n_parts; ++pt) s += reinterpret_cast<const int32_t*>(part + (int64_t)pt * stride + ns)[idx];   // integers: any order
            int64_t* dst = which ? hits + m : hist + m;
            *dst = accumulate ? *dst + s : s;
        }
    }
}
