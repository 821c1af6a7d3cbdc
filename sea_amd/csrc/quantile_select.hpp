// The per-column read-outs of decode_member_quantiles_kernel (decode_loss.hip): weighted quantiles and exceedance probabilities of an ensemble's decoded
// values at one cell.  include/sea_hip.h (sea_decode_member_quantiles) states the definitions.  verify_score.hpp is left as it is: the walk below RESTATES
// the walk of vf_score_wave (the same loop, the same order test, the same fp64 adds in j ascending order), and the sums go through vf_wave_sum.
//   qs_column_wave<V>  one wave reads out one column: lane l holds member l (and l + 64 at V = 2).  With levels, every lane walks j = 0 .. N - 1 with
//                      broadcast LDS reads and accumulates the weight below its own member under the total order (value, member index); per level a
//                      select and an f32 wave-min (the wave-max of the live members where no member qualifies).  Per threshold one fp64 butterfly.
//                      Without levels the walk is not run: `n_levels > 0` is a branch that is uniform over the launch, not a template parameter.
// An f32 min or max over lanes returns one of its operands whatever the order, so a quantile is the decoded value of one member bit for bit.
#pragma once
#include "verify_score.hpp"

constexpr int QS_MAX_OUT = 2 * SEA_QUANTILE_MAX_LEVELS;   // results per column: up to 8 levels and up to 8 thresholds

__device__ __forceinline__ float qs_wave_min(float v) {
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) v = fminf(v, __shfl_xor(v, m, 64));
    return v;
}

__device__ __forceinline__ float qs_wave_max(float v) {
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) v = fmaxf(v, __shfl_xor(v, m, 64));
    return v;
}

// A lane's members of one column: values, weights (0 for a dead member) and live flags; returns (in every lane) whether a live member's value is not
// finite.  Shared with bs_column_wave (brier_score.hpp).
template <int V>
__device__ __forceinline__ int qs_load_column(const float* row, const double* w_s, const int* live_s, const int N, const int lane, float (&x)[V], double (&w)[V],
                                              bool (&lv)[V]) {
    int bad = 0;
#pragma unroll
    for (int v = 0; v < V; ++v) {
        const int i = lane + 64 * v;
        const bool in = i < N;
        x[v] = in ? row[i] : 0.f;
        w[v] = in ? w_s[i] : 0.0;
        lv[v] = in && live_s[i] != 0;
        bad |= (lv[v] && !isfinite(x[v])) ? 1 : 0;
    }
    return __any(bad);
}

// The weight of the live members above a threshold (strict, f32 compares), in fp64 through the fixed xor butterfly: the same bits in every lane.
template <int V>
__device__ __forceinline__ double qs_exceed_sum(const float (&x)[V], const double (&w)[V], const bool (&lv)[V], const float th) {
#pragma clang fp reassociate(off)
    double e = 0.0;
#pragma unroll
    for (int v = 0; v < V; ++v) e += (lv[v] && x[v] > th) ? w[v] : 0.0;
    return vf_wave_sum(e);
}

// row: the column's member values [N] in LDS; w_s, live_s: the history's weights (0 for a dead member) and live flags [N] in LDS; W: the sum of the
// live weights (> 0: the caller passes a history without a live member over); level: the launch's levels; thr_s: the field's thresholds in LDS.
// Lane 0 files n_levels quantiles, then n_thr probabilities, in res.  A dead member's weight is 0: its value, NaN included, reaches nothing.
template <int V>
__device__ __forceinline__ void qs_column_wave(const float* row, const double* w_s, const int* live_s, const int N, const int lane, const double W, const float* level,
                                               const int n_levels, const float* thr_s, const int n_thr, float* res) {
#pragma clang fp reassociate(off)
    float x[V];
    double w[V], below[V];
    bool lv[V];
#pragma unroll
    for (int v = 0; v < V; ++v) below[v] = 0.0;
    const int bad = qs_load_column<V>(row, w_s, live_s, N, lane, x, w, lv);   // a live member's value is not finite: NaN in every map of this cell
    if (n_levels > 0) {
        // the walk of vf_score_wave, j ascending; eight members' reads are issued together, the order test has no short-circuit
        int j = 0;
        for (; j + VF_WALK <= N; j += VF_WALK) {
            float xj[VF_WALK];
            double wj[VF_WALK];
#pragma unroll
            for (int u = 0; u < VF_WALK; ++u) {
                xj[u] = row[j + u];
                wj[u] = w_s[j + u];
            }
#pragma unroll
            for (int u = 0; u < VF_WALK; ++u)
#pragma unroll
                for (int v = 0; v < V; ++v) {
                    const bool lower = (xj[u] < x[v]) | ((xj[u] == x[v]) & (j + u < lane + 64 * v));
                    below[v] += lower ? wj[u] : 0.0;
                }
        }
        for (; j < N; ++j) {
            const float xj = row[j];
            const double wj = w_s[j];
#pragma unroll
            for (int v = 0; v < V; ++v) {
                const bool lower = (xj < x[v]) | ((xj == x[v]) & (j < lane + 64 * v));
                below[v] += lower ? wj : 0.0;
            }
        }
        float hi = -INFINITY;
#pragma unroll
        for (int v = 0; v < V; ++v) hi = lv[v] ? fmaxf(hi, x[v]) : hi;
        hi = qs_wave_max(hi);   // the largest live value: the answer where rounding leaves no member with cum >= tau W
        for (int k = 0; k < n_levels; ++k) {
            const double tw = (double)level[k] * W;
            float lo = INFINITY;
#pragma unroll
            for (int v = 0; v < V; ++v) lo = (lv[v] && below[v] + w[v] >= tw) ? fminf(lo, x[v]) : lo;
            lo = qs_wave_min(lo);
            const float q = lo == INFINITY ? hi : lo;   // the live values of a good cell are finite: INFINITY says that no member qualified
            if (lane == 0) res[k] = bad ? NAN : q;
        }
    }
    for (int t = 0; t < n_thr; ++t) {
        const float th = thr_s[t];
        const double e = qs_exceed_sum<V>(x, w, lv, th);
        if (lane == 0) res[n_levels + t] = (bad || th != th) ? NAN : (float)(e / W);
    }
}
