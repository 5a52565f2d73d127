// vcm_variance.h -- the per-pixel variance of the running mean and the noise statistic reduced from it, host+device: the
// kernels of vcm_variance.hip and the host emulation of the tests (tests/host_emul_variance) run THESE functions, so that
// a host build and a device build give the same bits.  Arithmetic: + - * / only (sqrt is not needed), comparisons,
// compiled with -ffp-contract=off like the rest of vcm_core.h.
//
// The framebuffer is a running SUM S_k over iterations, and the iterations are independent samples x_k = S_k - S_{k-1} of
// the image.  Beside it a tracked context keeps two float4 images,
//   prev  { S_{k-1}.rgb, 0 }       the sum as the last update saw it
//   mom   { M2_r, M2_g, M2_b, 0 }  Welford's sum of squared deviations of the x_i from their mean
// 2 x 16 = 32 bytes per pixel, 134 MB at 2048^2, from vcm_track_variance(ctx, 1) to vcm_destroy.  One update reads the sum
// (12 B) and reads and writes both images (4 x 16 B): 76 bytes per pixel.  The variance of the MEAN S_k / k is
//   V_c = M2_c / (k (k - 1)),  k >= 2
// and the noise statistic is the reduction of  noise = V / (mean^2 + 0.01)  over pixels and channels: the expectation of
// the relative squared error (img - ref)^2 / (ref^2 + 0.01) the project measures against converged references.
#ifndef SMALLVCM_AMD_VCM_VARIANCE_H
#define SMALLVCM_AMD_VCM_VARIANCE_H

#include "../../include/smallvcm_amd.h"
#include "vcm_math.h"

namespace vcm {

#define VCM_VAR_BLOCK 256            /* lanes of a workgroup of both kernels */
#define VCM_VAR_DEFAULT_MAX_BLOCKS 2048   /* the grid's cap: 8 workgroups per CU of an MI355X; beyond it lanes stride */

VCM_HD bool var_finite(float x) { return (f2u(x) & 0x7f800000u) != 0x7f800000u; }

/* the grid of both kernels for n pixels: a function of n and the cap alone (never of the device), so that the order of
   the additions below is fixed */
inline int var_grid_blocks(long long n, int maxBlocks)
{
    long long b = (n + VCM_VAR_BLOCK - 1) / VCM_VAR_BLOCK;
    if (b > maxBlocks) b = maxBlocks;
    return b < 1 ? 1 : (int)b;
}

/* ---------------- accumulation ---------------- */
/* One channel of iteration k (1-based): s = S_k, prev = S_{k-1}, m2 the moment so far.  Welford's update
 *   M2 += (x - mean_{k-1}) (x - mean_k),  x = S_k - S_{k-1},  mean_j = S_j / j
 * -- not a sum of squares: a converged pixel's relative variance lies far below what Q - k mean^2 keeps in fp32.  k == 1
 * gives 0.  A non-finite x makes m2 non-finite from k == 2 on (inf - inf and NaN - anything are NaN). */
VCM_HD float var_update_channel(float s, float prev, float m2, int k, float km1, float kf)
{
    if (k <= 1) return 0.f;
    const float x = s - prev;
    return m2 + (x - prev / km1) * (x - s / kf);
}

VCM_HD void var_update_pixel(float sr, float sg, float sb, int k, float km1, float kf, F4 &prev, F4 &mom)
{
    mom = mk4(var_update_channel(sr, prev.x, mom.x, k, km1, kf), var_update_channel(sg, prev.y, mom.y, k, km1, kf),
              var_update_channel(sb, prev.z, mom.z, k, km1, kf), 0.f);
    prev = mk4(sr, sg, sb, 0.f);
}

/* variance of the mean of one channel; kk = (float)(k (k - 1)) */
VCM_HD float var_of_mean(float m2, float kk) { return m2 / kk; }

/* ---------------- the noise statistic ---------------- */
/* what a lane, a wave, a workgroup and the whole image carry: binary64 sum, fp32 maximum, two counts */
struct VarAcc {
    double sum;
    float max;
    int pad;
    long long above, nonFinite;
};

VCM_HD VarAcc var_acc_zero()
{
    VarAcc a;
    a.sum = 0.0; a.max = u2f(0xff800000u) /* -inf */; a.pad = 0; a.above = 0; a.nonFinite = 0;
    return a;
}

/* one element: noise = V / (mean^2 + 0.01); a non-finite one is counted and left out of sum, max and above */
VCM_HD void var_acc_element(VarAcc &a, float s, float m2, float kf, float kk, float threshold)
{
    const float mean = s / kf;
    const float noise = var_of_mean(m2, kk) / (mean * mean + 0.01f);
    const bool fin = var_finite(noise);   /* selects, not branches: the members stay in registers (adding 0.0 changes no sum) */
    a.nonFinite = a.nonFinite + (fin ? 0 : 1);
    a.sum = a.sum + (fin ? (double)noise : 0.0);
    a.max = (fin && noise > a.max) ? noise : a.max;
    a.above = a.above + ((fin && noise > threshold) ? 1 : 0);
}

VCM_HD void var_acc_pixel(VarAcc &a, F4 prev, F4 mom, float kf, float kk, float threshold)
{
    var_acc_element(a, prev.x, mom.x, kf, kk, threshold);
    var_acc_element(a, prev.y, mom.y, kf, kk, threshold);
    var_acc_element(a, prev.z, mom.z, kf, kk, threshold);
}

/* a += b: the one combination of the tree */
VCM_HD void var_acc_combine(VarAcc &a, const VarAcc &b)
{
    a.sum = a.sum + b.sum;
    if (b.max > a.max) a.max = b.max;
    a.above = a.above + b.above;
    a.nonFinite = a.nonFinite + b.nonFinite;
}

/* THE TREE over the VCM_VAR_BLOCK slots v[] of a workgroup, written once: step s of VCM_VAR_TREE_STEPS, lane `lane`.
 *   steps 0 .. 5   inside every wave of 64: slot += slot + 32, 16, 8, 4, 2, 1
 *   steps 6, 7     across the waves: slots 0 and 128 take 64 and 192, then slot 0 takes 128
 * The device runs a step on all lanes and a barrier, the emulation a step over all lanes in a loop: a step reads only slots
 * no lane of that step writes, so both orders give the same additions.  The result is v[0]. */
#define VCM_VAR_TREE_STEPS 8
VCM_HD void var_tree_step(VarAcc *v, int step, int lane)
{
    if (step < 6) {
        const int off = 32 >> step;
        if ((lane & 63) < off) var_acc_combine(v[lane], v[lane + off]);
    } else {
        const int off = 64 << (step - 6);
        if (lane % (2 * off) == 0) var_acc_combine(v[lane], v[lane + off]);
    }
}

/* what lane `lane` of workgroup `block` sums, in index order: the pixels g, g + G, g + 2 G, ... (g its global index, G
   the lanes of the grid), three channels each */
template <class Load>
VCM_HD VarAcc var_lane_sum(long long n, int blocks, int block, int lane, float kf, float kk, float threshold, Load &&load)
{
    VarAcc a = var_acc_zero();
    const long long G = (long long)blocks * VCM_VAR_BLOCK;
    for (long long p = (long long)block * VCM_VAR_BLOCK + lane; p < n; p += G) {
        F4 prev, mom;
        load(p, prev, mom);
        var_acc_pixel(a, prev, mom, kf, kk, threshold);
    }
    return a;
}

/* the second level: lane `lane` of ONE workgroup sums the workgroups' partials lane, lane + 256, ... in index order */
VCM_HD VarAcc var_lane_sum_partials(const VarAcc *partials, int blocks, int lane)
{
    VarAcc a = var_acc_zero();
    for (int b = lane; b < blocks; b += VCM_VAR_BLOCK) var_acc_combine(a, partials[b]);
    return a;
}

/* the image's VarAcc as the caller's record (include/smallvcm_amd.h) */
inline void var_finish_stats(const VarAcc &a, int k, long long n, vcm_noise_stats *out)
{
    out->iterations = k;
    out->elements = 3 * n;
    out->above = a.above;
    out->nonFinite = a.nonFinite;
    const long long counted = 3 * n - a.nonFinite;
    out->mean = counted > 0 ? a.sum / (double)counted : 0.0;
    out->max = counted > 0 ? (double)a.max : 0.0;
}

/* ---------------- launches (vcm_variance.hip; the C-ABI of vcm_api.hip calls them) ---------------- */
#if defined(__HIPCC__)
/* the tree over the LDS slots of a workgroup (vcm_robust.hip reduces with it too); v[0] holds the result for lane 0
   afterwards */
__device__ inline void var_block_tree(VarAcc *v, int lane)
{
    __syncthreads();
    for (int s = 0; s < VCM_VAR_TREE_STEPS; s++) {
        var_tree_step(v, s, lane);
        __syncthreads();
    }
}
/* the cap of the grid of the kernels (vcm_debug_variance_max_blocks) */
int var_max_blocks();
void var_set_max_blocks(int blocks);
/* iteration k's update of the n-pixel images prev, mom from the sum image sum3 (3 floats per pixel) */
hipError_t var_launch_update(long long n, const float *sum3, int k, F4 *prev, F4 *mom, hipStream_t stream);
/* *result (device) = the reduced VarAcc of the image; partials: maxBlocks VarAcc of device scratch */
hipError_t var_launch_stats(long long n, const F4 *prev, const F4 *mom, int k, float threshold, int maxBlocks, VarAcc *partials,
                            VarAcc *result, hipStream_t stream);
/* out[3 p + c] = V_c of pixel p */
hipError_t var_launch_read(long long n, const F4 *mom, int k, float *out3, hipStream_t stream);
#endif

} // namespace vcm
#endif
