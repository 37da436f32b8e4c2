// select_math.hpp -- the selection arithmetic, ONE definition of each piece: the reference-arithmetic ("exact") score of a
// hypothesis, the softMax / entropy statistics and draw's argmax.  Every route of the selection (k_select_rescore, k_spec_join,
// k_rescore, k_stats_*, the selection folded into the refinement team, refine_pick_winner, spec_pick_fast) calls these, so "every
// route returns the serial route's bits" holds by construction.  What touches no thread index is ESAC_HD: the CPU suite runs it
// (tests/native/host_math_probe.cpp).
#pragma once
#include "device_common.hpp"
#include "pose_math.hpp"

namespace esac {

// ---------------------------------------------------------------- the exact score (esac_util.h:235-260)
// One cell's term: reprojection error, clamped at maxReproj, through the soft inlier function.
// STRICT (ESAC_FLAG_STRICT_REFERENCE): std::min's own argument order, std::min(l, maxReproj) = (maxReproj < l) ? maxReproj : l --
// a NaN error (non-finite scene coordinate) stays NaN and with it the hypothesis' score, as in the reference (oracle: repro_errs).
// Otherwise `l < maxReproj ? l : maxReproj` (esac_util.h:358 for every finite l): such a cell is an outlier at maxReproj.
template <bool STRICT>
ESAC_HD double exact_cell_term(const double (&R)[9], const double (&t)[3], const Cam& cam, float X, float Y, float Z, float px, float py,
                               float max_reproj, float tau, float beta) {
    float err = project_exact_err(R, t, cam, X, Y, Z, px, py);
    if (STRICT) err = max_reproj < err ? max_reproj : err;
    else        err = err < max_reproj ? err : max_reproj;
    return soft_inlier_exact(err, tau, beta);
}
// the sum of a hypothesis' terms -> its score: float / int / int, then double *= float (esac_util.h:256)
ESAC_HD double exact_score_scaled(double sum, float alpha, int W, int H) {
    const float scale = alpha / W / H;
    sum *= scale;
    return sum;
}
// Sum of the terms of cells [c0, c1) of hypothesis h over a workgroup of B threads, in every thread (thread t takes cells c0 + t,
// c0 + t + B, ...; block_sum's fixed order).  R = rodrigues_vec2mat(rvec) as the sampler stored it (the reference re-expands
// rvec, esac_util.h:302).  s_part: >= B / 64 doubles, s_tot: >= 1.  Contains workgroup barriers.
template <int B, bool STRICT>
__device__ __forceinline__ double block_exact_score(const KArgs& a, int h, const Cam& cam, int P, int c0, int c1, double* s_part, double* s_tot) {
    const float* __restrict__ mx = a.sc + (size_t)expert_of(a, h) * 3 * P;
    const double* hp = a.hyps + (size_t)h * 6;
    const double t[3] = {hp[3], hp[4], hp[5]};
    double R[9];
#pragma unroll
    for (int k = 0; k < 9; k++) R[k] = a.hyps_R[(size_t)h * 9 + k];
    double acc[1] = {0};
    for (int i = c0 + threadIdx.x; i < c1; i += B) {
        const int row = i / a.W, col = i - row * a.W;
        acc[0] += exact_cell_term<STRICT>(R, t, cam, mx[i], mx[P + i], mx[2 * P + i], cell_px(a, col), cell_py(a, row), a.max_reproj, a.tau, a.beta);
    }
    block_sum<1, B>(acc, s_part, s_tot);
    return acc[0];
}
// what the selection leaves of hypothesis h: its score (workspace and, if asked for, the caller's vector) and whether it is exact
__device__ __forceinline__ void store_score(const KArgs& a, int h, double value, int exact) {
    a.scores[h] = value;
    if (a.scores_user) a.scores_user[user_slot(a, h)] = value;
    a.exact_flag[h] = exact;
}

// ---------------------------------------------------------------- softMax / entropy statistics (esac_util.h:461-497)
// S = sum exp(s - m), T = sum exp(s - m) (s - m) over the scores s, m their maximum
ESAC_HD void softmax_add(double& S, double& T, double s, double m) {
    const double d = s - m;
    const double ex = exp(d);
    S += ex;
    T += ex * d;
}
// entropy = -sum p log2 p,  p = exp(d) / S  ->  log2(S) - T / (S ln 2)
ESAC_HD double entropy_bits(double S, double T) { return log2(S) - T / (S * 0.6931471805599453); }
// NaN-ignoring maximum over a workgroup of B threads, in every thread.  s_max: B / 64 values.  Contains a workgroup barrier.
__device__ __forceinline__ float max_ignoring_nan(float x, float y) { return fmaxf(x, y); }
__device__ __forceinline__ double max_ignoring_nan(double x, double y) { return fmax(x, y); }
template <int B, typename T>
__device__ __forceinline__ T block_max(T m, T* s_max) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = max_ignoring_nan(m, __shfl_xor(m, o));
    if ((threadIdx.x & 63) == 0) s_max[threadIdx.x >> 6] = m;
    __syncthreads();
    m = s_max[0];
#pragma unroll
    for (int k = 1; k < B / 64; k++) m = max_ignoring_nan(m, s_max[k]);
    return m;
}
__device__ __forceinline__ void write_stats(const KArgs& a, int n_contenders, double m, double S, double entropy) {
    a.n_contenders[0] = n_contenders;
    a.stats[0] = m;        // max
    a.stats[1] = S;        // sum exp(s - max)
    a.stats[2] = entropy;
}

// ---------------------------------------------------------------- draw(probs, training=false) (esac_util.h:512-529)
// argmax of the scores (softmax is monotone), first GLOBAL index on ties; a NaN never wins (both comparisons are false for it).
// The incumbent starts as (-inf, BEST_NONE, BEST_NONE): "none".
constexpr int BEST_NONE = 0x7fffffff;
template <typename T>
ESAC_HD void best_take(T& bs, int& bi, int& bg, T os, int oi, int og) {
    if (os > bs || (os == bs && og < bg)) {
        bs = os;
        bi = oi;
        bg = og;
    }
}
// every thread's candidate in, the workgroup's best in every thread out.  T: double, or float where the scores are fp32 (widening
// is exact and keeps the order: the shared array is the double one either way).  s_best / s_besti / s_bestg: B / 64 entries;
// PRE_BARRIER: they may still be read when this is called.  Contains a workgroup barrier.
template <int B, bool PRE_BARRIER, typename T>
__device__ __forceinline__ void block_best(T& bs, int& bi, int& bg, double* s_best, int* s_besti, int* s_bestg) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const T os = __shfl_xor(bs, o);
        const int oi = __shfl_xor(bi, o);
        const int og = __shfl_xor(bg, o);
        best_take(bs, bi, bg, os, oi, og);
    }
    if (PRE_BARRIER) __syncthreads();
    if ((threadIdx.x & 63) == 0) {
        s_best[threadIdx.x >> 6] = (double)bs;
        s_besti[threadIdx.x >> 6] = bi;
        s_bestg[threadIdx.x >> 6] = bg;
    }
    __syncthreads();
    bs = (T)s_best[0];
    bi = s_besti[0];
    bg = s_bestg[0];
#pragma unroll
    for (int w = 1; w < B / 64; w++) best_take(bs, bi, bg, (T)s_best[w], s_besti[w], s_bestg[w]);
}

}  // namespace esac
