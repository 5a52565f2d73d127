// vcm_robust.h -- the firefly-robust image estimate: median of means over M buckets of iterations, the trim adapted by the
// Gini coefficient of the bucket means (Jung et al. 2015; Buisine et al. 2021, "G-MoN"), host+device: the kernels of
// vcm_robust.hip and the host emulation of the tests (tests/host_emul_robust) run THESE functions, so that a host build and
// a device build give the same bits.  Arithmetic: + - * / only, comparisons, compiled with -ffp-contract=off like the rest
// of vcm_core.h.
//
// The framebuffer is a running SUM S_k over iterations, and the iterations are independent samples x_k = S_k - S_{k-1} of
// the image (vcm_variance.h).  Beside it a tracked context keeps M + 2 float4 images,
//   prev       { S_{k-1}.rgb, 0 }   the sum as the last update saw it (its own, not the variance tracker's)
//   B_0..B_M-1 { sum.rgb, 0 }       M planes [M][n]: iteration k (from 1) adds x_k to plane (k - 1) mod M
//   out        { rgb, 1 }           the resolved estimate
// (M + 2) x 16 bytes per pixel.  One update reads the sum (12 B) and reads and writes prev and ONE plane (4 x 16 B): 76
// bytes per pixel.  After k >= M iterations bucket j holds n_j = ceil((k - j) / M) of them, and a pixel resolves as
//   m_j = B_j / n_j,  y_j = luminance(m_j)                         buckets with a non-finite key are dropped, M' stay
//   r_j = #{ kept i : y_i < y_j, or y_i == y_j and i < j }        the rank: M^2 comparisons, no data moves
//   G   = clamp(sum_j (2 (r_j + 1) - M' - 1) y_j / (M' sum_j y_j), 0, 1),  0 where sum_j y_j <= 0 (or G is NaN)
//   t   = min((M' - 1) / 2, floor(G M' / 2))                       buckets trimmed from each end of the ranking
//   out = sum_{t <= r_j < M' - t} B_j / sum n_j                    whole RGB triples, weighted by their counts
// so that equal bucket means (G = 0) give the plain mean, sum of all buckets over k, and one bucket that carries everything
// (G -> 1) gives the median bucket.  M' == 0 passes prev / k through.  All sums run in bucket-index order.
#ifndef SMALLVCM_AMD_VCM_ROBUST_H
#define SMALLVCM_AMD_VCM_ROBUST_H

#include "vcm_core.h"
#include "vcm_variance.h"

namespace vcm {

#define VCM_ROBUST_MIN_BUCKETS 3
#define VCM_ROBUST_MAX_BUCKETS 15
/* VCM_ROBUST_DEFAULT_BUCKETS (include/smallvcm_amd.h): the sweep of tests/robust_tune.py (DESIGN.md "Robust estimate") */

inline bool robust_buckets_ok(int M) { return M >= VCM_ROBUST_MIN_BUCKETS && M <= VCM_ROBUST_MAX_BUCKETS && (M & 1) == 1; }

/* the plane iteration k (from 1) adds to */
inline int robust_bucket_of(int k, int M) { return (k - 1) % M; }

/* the iterations plane j holds after k: ceil((k - j) / M), 0 while k <= j */
VCM_HD int robust_bucket_count(int k, int j, int M) { return (k - j + M - 1) / M; }

/* ---------------- accumulation ---------------- */
/* iteration k of one pixel: s = S_k; `bucket` is the pixel of plane (k - 1) mod M */
VCM_HD void robust_update_pixel(float sr, float sg, float sb, F4 &prev, F4 &bucket)
{
    bucket = mk4(bucket.x + (sr - prev.x), bucket.y + (sg - prev.y), bucket.z + (sb - prev.z), 0.f);
    prev = mk4(sr, sg, sb, 0.f);
}

/* ---------------- the resolve ---------------- */
/* what the rule decided for a pixel, beside the colour */
struct RobustInfo {
    float gini;
    int trim, kept;   /* t; M' */
};

/* One pixel after k >= M iterations: the rule of the header.  bucket(j) gives the pixel of plane j (called once for
 * every j, in order), prevSum() the pixel of prev (called only where M' == 0).  M is a template argument so that every loop
 * unrolls and B, y, keep and the ranks are registers: no array below is indexed by a run-time value. */
template <int M, class Bucket, class Prev>
VCM_HD F4 robust_resolve_pixel(int k, Bucket &&bucket, Prev &&prevSum, RobustInfo &info)
{
    F4 B[M];
    float y[M];
    bool keep[M];
    int cnt[M];
    int mp = 0;
#pragma unroll
    for (int j = 0; j < M; j++) {
        B[j] = bucket(j);
        cnt[j] = robust_bucket_count(k, j, M);
        const float nf = (float)cnt[j];
        y[j] = luminance(mk3(B[j].x / nf, B[j].y / nf, B[j].z / nf));
        keep[j] = var_finite(y[j]);
        mp += keep[j] ? 1 : 0;
    }
    info.kept = mp;
    info.gini = 0.f;
    info.trim = 0;
    if (mp == 0) {
        const F4 s = prevSum();
        const float kf = (float)k;
        return mk4(s.x / kf, s.y / kf, s.z / kf, 1.f);
    }
    int rank[M];
    float num = 0.f, den = 0.f;
#pragma unroll
    for (int j = 0; j < M; j++) {
        int r = 0;
#pragma unroll
        for (int i = 0; i < M; i++) {
            if (i == j) continue;
            const bool before = (i < j) ? (y[i] <= y[j]) : (y[i] < y[j]);
            r += (keep[i] && before) ? 1 : 0;
        }
        rank[j] = r;
        const float coef = (float)(2 * (r + 1) - mp - 1);
        num = num + (keep[j] ? coef * y[j] : 0.f);   /* selects: a dropped bucket adds 0, which changes no sum */
        den = den + (keep[j] ? y[j] : 0.f);
    }
    const float mpf = (float)mp;
    float g = (den > 0.f) ? num / (mpf * den) : 0.f;
    g = (g > 0.f) ? g : 0.f;     /* a NaN (inf / inf of overflowed sums) compares false: 0 */
    g = (g < 1.f) ? g : 1.f;
    const int half = (mp - 1) / 2, want = (int)((g * mpf) * 0.5f);
    const int t = want < half ? want : half;
    info.gini = g;
    info.trim = t;
    float r_ = 0.f, g_ = 0.f, b_ = 0.f;
    int n = 0;
#pragma unroll
    for (int j = 0; j < M; j++) {
        const bool in = keep[j] && rank[j] >= t && rank[j] < mp - t;
        r_ = r_ + (in ? B[j].x : 0.f);
        g_ = g_ + (in ? B[j].y : 0.f);
        b_ = b_ + (in ? B[j].z : 0.f);
        n += in ? cnt[j] : 0;
    }
    const float nf = (float)n;
    return mk4(r_ / nf, g_ / nf, b_ / nf, 1.f);
}

/* ---------------- the statistics ---------------- */
/* The reduction IS that of vcm_variance.h -- its grid (var_grid_blocks), its VarAcc, its tree (var_tree_step) and its second
 * level (var_lane_sum_partials) -- with the members read as
 *   sum = sum of G over pixels (binary64),  max = the largest G,  above = pixels with t > 0,  nonFinite = pixels with M' < M */
VCM_HD void robust_acc_pixel(VarAcc &a, const RobustInfo &info, int M)
{
    a.sum = a.sum + (double)info.gini;
    a.max = (info.gini > a.max) ? info.gini : a.max;
    a.above = a.above + (info.trim > 0 ? 1 : 0);
    a.nonFinite = a.nonFinite + (info.kept < M ? 1 : 0);
}

/* what lane `lane` of workgroup `block` sums, in index order: the pixels g, g + G, g + 2 G, ... (var_lane_sum's order);
   bucket(p, j) and prevSum(p) load pixel p */
template <int M, class Bucket, class Prev>
VCM_HD VarAcc robust_lane_sum(long long n, int blocks, int block, int lane, int k, Bucket &&bucket, Prev &&prevSum)
{
    VarAcc a = var_acc_zero();
    const long long G = (long long)blocks * VCM_VAR_BLOCK;
    for (long long p = (long long)block * VCM_VAR_BLOCK + lane; p < n; p += G) {
        RobustInfo info;
        (void)robust_resolve_pixel<M>(k, [&](int j) { return bucket(p, j); }, [&]() { return prevSum(p); }, info);
        robust_acc_pixel(a, info, M);
    }
    return a;
}

/* the image's VarAcc as the caller's record (include/smallvcm_amd.h) */
inline void robust_finish_stats(const VarAcc &a, int k, int M, long long n, vcm_robust_stats *out)
{
    out->iterations = k;
    out->buckets = M;
    out->pixels = n;
    out->trimmed = a.above;
    out->nonFinite = a.nonFinite;
    out->meanGini = n > 0 ? a.sum / (double)n : 0.0;
    out->maxGini = n > 0 ? (double)a.max : 0.0;
}

/* CALL(M) with the run-time M as a constant: one instantiation per odd M, 3 .. 15 (robust_buckets_ok) */
#define VCM_ROBUST_DISPATCH(M, CALL) \
    switch (M) { \
    case 3: CALL(3); break; case 5: CALL(5); break; case 7: CALL(7); break; case 9: CALL(9); break; \
    case 11: CALL(11); break; case 13: CALL(13); break; case 15: CALL(15); break; \
    }

/* ---------------- launches (vcm_robust.hip; the C-ABI of vcm_api.hip calls them) ---------------- */
#if defined(__HIPCC__)
/* iteration k's update of the n-pixel images prev and buckets ([M][n]) from the sum image sum3 (3 floats per pixel) */
hipError_t robust_launch_update(long long n, const float *sum3, int k, int M, F4 *prev, F4 *buckets, hipStream_t stream);
/* out = the estimate after k >= M iterations */
hipError_t robust_launch_resolve(long long n, const F4 *prev, const F4 *buckets, int k, int M, F4 *out, hipStream_t stream);
/* *result (device) = the reduced VarAcc of the image; partials: maxBlocks VarAcc of device scratch */
hipError_t robust_launch_stats(long long n, const F4 *prev, const F4 *buckets, int k, int M, int maxBlocks, VarAcc *partials,
                               VarAcc *result, hipStream_t stream);
#endif

} // namespace vcm
#endif
