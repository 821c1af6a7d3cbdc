// The per-reading arithmetic of ensemble verification, shared by verify_kernel (verify.hip: a reading is a sensor) and decode_member_verify_kernel
// (decode_loss.hip: a reading is a cell of the decoded field).  Both call the SAME two device functions, so a cell scored from the same member values,
// reading, precision and weights has the same bits as a sensor.  include/sea_hip.h (sea_ensemble_verify) states the formulas.
//   vf_score_wave<V>  one wave scores one reading: lane l holds member l (and l + 64 at V = 2), walks j = 0 .. N - 1 with broadcast LDS reads and
//                     accumulates the weight below its own member under the total order (value, member index); the lane terms are reduced by a fixed
//                     xor butterfly (the mean first: the spread is centred on it).  Every lane returns the same sums.
//   vf_score_wave_ex  vf_score_wave's copy that hands back the lane's value, weight, weight below and live flag; vf_crps_grad: the CRPS derivative from them.
//   vf_score_seg_ex   vf_score_wave_ex for a wave that holds 64 / NP histories of up to NP <= 32 members each (segments of NP lanes): the same bits.
//   vf_finish_reading one thread finishes one reading: the selects on c, the fp32 roundings, the eight terms of the per-history sums.
#pragma once
#include "sea_common.hpp"

#include <math.h>

constexpr int VF_MAX_N = 128;
constexpr int VF_SUMS = 8;
constexpr int VF_WALK = 8;   // members whose LDS reads are issued together in the walk

__device__ __forceinline__ double vf_wave_sum(double v) {
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) v += __shfl_xor(v, m, 64);
    return v;
}

struct VfReading {   // what a wave leaves per reading; state: 0 live and good, 1 dead, 2 bad
    double mean, var, ab, pair, pit;
    int rank, state;
};

// row: the reading's member values [N] in LDS; w_s, live_s: the history's normalised weights and live flags [N] in LDS; yf, pv: the reading and its
// precision (pv > 0: the caller passes dead readings over).  A dead member's weight is 0: its value, NaN included, reaches nothing.
template <int V>
__device__ __forceinline__ VfReading vf_score_wave(const float* row, const double* w_s, const int* live_s, const int N, const int lane, const float yf, const float pv) {
#pragma clang fp reassociate(off)
    const double y = (double)yf;
    float x[V];
    double w[V], below[V];
    bool lv[V];
#pragma unroll
    for (int v = 0; v < V; ++v) {
        const int i = lane + 64 * v;
        const bool in = i < N;
        x[v] = in ? row[i] : 0.f;
        w[v] = in ? w_s[i] : 0.0;
        lv[v] = in && live_s[i] != 0;
        below[v] = 0.0;
    }
    // the walk, j ascending; eight members' reads are issued together, and the order test is written without short-circuits: no branch in the chain
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
    double m = 0.0;
    int bad = (isfinite(yf) && isfinite(pv)) ? 0 : 1, rk = 0;
#pragma unroll
    for (int v = 0; v < V; ++v) {
        m += lv[v] ? w[v] * (double)x[v] : 0.0;
        bad |= (lv[v] && !isfinite(x[v])) ? 1 : 0;
        rk += (lv[v] && x[v] < yf) ? 1 : 0;
    }
    const double mean = vf_wave_sum(m);
    double var = 0.0, ab = 0.0, pr = 0.0, pt = 0.0;
#pragma unroll
    for (int v = 0; v < V; ++v) {
        const double xd = (double)x[v], d = xd - y, dm = xd - mean;
        var += lv[v] ? w[v] * dm * dm : 0.0;
        ab += lv[v] ? w[v] * fabs(d) : 0.0;
        pr += lv[v] ? w[v] * d * (2.0 * below[v] + w[v] - 1.0) : 0.0;
        pt += lv[v] ? w[v] * (x[v] < yf ? 1.0 : (x[v] == yf ? 0.5 : 0.0)) : 0.0;
    }
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {   // six butterflies, stage by stage: their exchanges are in flight together; each sum has vf_wave_sum's order
        const double o_var = __shfl_xor(var, m, 64), o_ab = __shfl_xor(ab, m, 64), o_pr = __shfl_xor(pr, m, 64), o_pt = __shfl_xor(pt, m, 64);
        const int o_rk = __shfl_xor(rk, m, 64), o_bad = __shfl_xor(bad, m, 64);
        var += o_var;
        ab += o_ab;
        pr += o_pr;
        pt += o_pt;
        rk += o_rk;
        bad += o_bad;
    }
    VfReading r;
    r.mean = mean;
    r.var = var;
    r.ab = ab;
    r.pair = pr;
    r.pit = pt;
    r.rank = rk;
    r.state = bad ? 2 : 0;
    return r;
}

// vf_score_wave's sibling for the gradient launch (sea_decode_member_crps_grad): the SAME statements in the same order, and it also hands back what the
// lane holds of its own members — the value x, the weight w, the weight below and the live flag (a member at or beyond N: 0, 0, 0, false).  It is a
// copy and not a wrapper so that vf_score_wave's callers keep their code, instruction for instruction.
template <int V>
__device__ __forceinline__ VfReading vf_score_wave_ex(const float* row, const double* w_s, const int* live_s, const int N, const int lane, const float yf, const float pv,
                                                      float (&x)[V], double (&w)[V], double (&below)[V], bool (&lv)[V]) {
#pragma clang fp reassociate(off)
    const double y = (double)yf;
#pragma unroll
    for (int v = 0; v < V; ++v) {
        const int i = lane + 64 * v;
        const bool in = i < N;
        x[v] = in ? row[i] : 0.f;
        w[v] = in ? w_s[i] : 0.0;
        lv[v] = in && live_s[i] != 0;
        below[v] = 0.0;
    }
    // the walk, j ascending; eight members' reads are issued together, and the order test is written without short-circuits: no branch in the chain
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
    double m = 0.0;
    int bad = (isfinite(yf) && isfinite(pv)) ? 0 : 1, rk = 0;
#pragma unroll
    for (int v = 0; v < V; ++v) {
        m += lv[v] ? w[v] * (double)x[v] : 0.0;
        bad |= (lv[v] && !isfinite(x[v])) ? 1 : 0;
        rk += (lv[v] && x[v] < yf) ? 1 : 0;
    }
    const double mean = vf_wave_sum(m);
    double var = 0.0, ab = 0.0, pr = 0.0, pt = 0.0;
#pragma unroll
    for (int v = 0; v < V; ++v) {
        const double xd = (double)x[v], d = xd - y, dm = xd - mean;
        var += lv[v] ? w[v] * dm * dm : 0.0;
        ab += lv[v] ? w[v] * fabs(d) : 0.0;
        pr += lv[v] ? w[v] * d * (2.0 * below[v] + w[v] - 1.0) : 0.0;
        pt += lv[v] ? w[v] * (x[v] < yf ? 1.0 : (x[v] == yf ? 0.5 : 0.0)) : 0.0;
    }
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {   // six butterflies, stage by stage: their exchanges are in flight together; each sum has vf_wave_sum's order
        const double o_var = __shfl_xor(var, m, 64), o_ab = __shfl_xor(ab, m, 64), o_pr = __shfl_xor(pr, m, 64), o_pt = __shfl_xor(pt, m, 64);
        const int o_rk = __shfl_xor(rk, m, 64), o_bad = __shfl_xor(bad, m, 64);
        var += o_var;
        ab += o_ab;
        pr += o_pr;
        pt += o_pt;
        rk += o_rk;
        bad += o_bad;
    }
    VfReading r;
    r.mean = mean;
    r.var = var;
    r.ab = ab;
    r.pair = pr;
    r.pit = pt;
    r.rank = rk;
    r.state = bad ? 2 : 0;
    return r;
}

// vf_score_wave_ex<1>'s sibling for the packed gradient launch (sea_decode_member_crps_grad_packed): the SAME statements in the same order, for a wave
// that holds 64 / NP histories' readings of one cell.  NP (2, 4, 8, 16 or 32) is the member count N rounded up to a power of two, at least 2; lane l is
// member i = l & (NP - 1) of segment g = l / NP and takes its value, weight and live flag from row[g NP + i], w_s[g NP + i], live_s[g NP + i] (0, 0,
// false for i >= N and for a segment that is off: seg_on false).  The walk runs over j = 0 .. N - 1 of the lane's OWN segment, ascending, with the same
// order test; yf and pv are the segment's reading and precision (each history has its own observation and precision map: they differ between lanes of
// different segments), and so is the good/bad test.  The butterflies are the same xor butterfly stopped at the stages m < NP: a segment is an aligned
// block of NP lanes, so those stages never leave it, and every lane of a segment returns that segment's sums.
// Why the bits are vf_score_wave_ex<1>'s at the same N: there the butterfly runs m = 1, 2, 4, .., 32 ascending and every lane >= N contributes +0.0 —
// each lane term is accumulated from +0.0 and so is never -0.0 — so the stages m >= NP add exact zeros (x + (+0.0) = x for every x that is not -0.0,
// and +0.0 + +0.0 = +0.0), and the stages m < NP pair the lanes 0 .. NP - 1 exactly as they pair the lanes g NP .. g NP + NP - 1 here.  The integer sums
// (rank, bad) are exact in any order.  A caller passes a segment whose cell is dead over by selects on what is returned (state 1): nothing branches here.
template <int NP>
__device__ __forceinline__ VfReading vf_score_seg_ex(const float* row, const double* w_s, const int* live_s, const int N, const int lane, const bool seg_on, const float yf,
                                                     const float pv, float& x, double& w, double& below, bool& lv) {
#pragma clang fp reassociate(off)
    static_assert(NP == 2 || NP == 4 || NP == 8 || NP == 16 || NP == 32, "a segment is a power of two of lanes, 2 .. 32");
    const double y = (double)yf;
    const int i = lane & (NP - 1), base = lane - i;
    {
        const bool in = seg_on && i < N;
        x = in ? row[base + i] : 0.f;
        w = in ? w_s[base + i] : 0.0;
        lv = in && live_s[base + i] != 0;
        below = 0.0;
    }
    // the walk, j ascending; eight members' reads are issued together, and the order test is written without short-circuits: no branch in the chain
    int j = 0;
    for (; j + VF_WALK <= N; j += VF_WALK) {
        float xj[VF_WALK];
        double wj[VF_WALK];
#pragma unroll
        for (int u = 0; u < VF_WALK; ++u) {
            xj[u] = row[base + j + u];
            wj[u] = w_s[base + j + u];
        }
#pragma unroll
        for (int u = 0; u < VF_WALK; ++u) {
            const bool lower = (xj[u] < x) | ((xj[u] == x) & (j + u < i));
            below += lower ? wj[u] : 0.0;
        }
    }
    for (; j < N; ++j) {
        const float xj = row[base + j];
        const double wj = w_s[base + j];
        const bool lower = (xj < x) | ((xj == x) & (j < i));
        below += lower ? wj : 0.0;
    }
    double m = 0.0;
    int bad = (isfinite(yf) && isfinite(pv)) ? 0 : 1, rk = 0;
    {
        m += lv ? w * (double)x : 0.0;
        bad |= (lv && !isfinite(x)) ? 1 : 0;
        rk += (lv && x < yf) ? 1 : 0;
    }
    double mean = m;
#pragma unroll
    for (int s = 1; s < NP; s <<= 1) mean += __shfl_xor(mean, s, 64);   // vf_wave_sum, stopped at the segment
    double var = 0.0, ab = 0.0, pr = 0.0, pt = 0.0;
    {
        const double xd = (double)x, d = xd - y, dm = xd - mean;
        var += lv ? w * dm * dm : 0.0;
        ab += lv ? w * fabs(d) : 0.0;
        pr += lv ? w * d * (2.0 * below + w - 1.0) : 0.0;
        pt += lv ? w * (x < yf ? 1.0 : (x == yf ? 0.5 : 0.0)) : 0.0;
    }
#pragma unroll
    for (int s = 1; s < NP; s <<= 1) {   // the six butterflies, stage by stage, stopped at the segment
        const double o_var = __shfl_xor(var, s, 64), o_ab = __shfl_xor(ab, s, 64), o_pr = __shfl_xor(pr, s, 64), o_pt = __shfl_xor(pt, s, 64);
        const int o_rk = __shfl_xor(rk, s, 64), o_bad = __shfl_xor(bad, s, 64);
        var += o_var;
        ab += o_ab;
        pr += o_pr;
        pt += o_pt;
        rk += o_rk;
        bad += o_bad;
    }
    VfReading r;
    r.mean = mean;
    r.var = var;
    r.ab = ab;
    r.pair = pr;
    r.pit = pt;
    r.rank = rk;
    r.state = bad ? 2 : 0;
    return r;
}

// The derivative of a reading's CRPS with respect to the lane's member (include/sea_hip.h, sea_decode_member_crps_grad):
//     G = w (sign(x - y) - (2 below + w - 1) / c),   sign(0) = 0;  c <= 0: the second term is 0, as in vf_finish_reading;  a dead member: 0
// in fp64.  At ties it is the subgradient that the walk's order (value, member index) selects.
__device__ __forceinline__ double vf_crps_grad(const float x, const double w, const double below, const bool lv, const float yf, const double c) {
#pragma clang fp reassociate(off)
    const double sg = x > yf ? 1.0 : (x < yf ? -1.0 : 0.0);
    const double pr = c > 0.0 ? (2.0 * below + w - 1.0) / c : 0.0;
    return lv ? w * (sg - pr) : 0.0;
}

struct VfOut {
    float mean, spread, crps, pit;
    int rank;
};

// t: the reading's eight terms of the per-history sums (all 0 for a dead reading).  c = unbiased ? 1 - q : 1.
__device__ __forceinline__ VfOut vf_finish_reading(const VfReading& r, const float yf, const float pv, const double c, double (&t)[VF_SUMS]) {
#pragma clang fp reassociate(off)
    VfOut o;
    o.mean = o.spread = o.crps = o.pit = 0.f;
    o.rank = -1;
#pragma unroll
    for (int i = 0; i < VF_SUMS; ++i) t[i] = 0.0;
    if (r.state == 2) {
        o.mean = o.spread = o.crps = o.pit = NAN;
        o.rank = -2;
        t[6] = 1.0;
    } else if (r.state == 0) {
        const double y = (double)yf;
        const double rvar = 1.0 / (double)pv;
        const double mean = r.mean;
        const double sp2 = c > 0.0 ? r.var / c : 0.0;
        const double crps = r.ab - (c > 0.0 ? r.pair / c : 0.0);
        const double err = y - mean;
        o.mean = (float)mean;
        o.spread = (float)sqrt(sp2);
        o.crps = (float)crps;
        o.pit = (float)r.pit;
        o.rank = r.rank;
        t[0] = 1.0;
        t[1] = crps;
        t[2] = err * err;
        t[3] = sp2;
        t[4] = err * err / (sp2 + rvar);
        t[5] = mean - y;
        t[7] = rvar;
    }
    return o;
}
