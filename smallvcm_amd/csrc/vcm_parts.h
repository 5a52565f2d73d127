// vcm_parts.h -- the technique breakdown: which part of the VertexCM estimator carries a pixel, host+device: the kernels of
// vcm_parts.hip and the host emulation of the tests (tests/host_emul_parts) run THESE functions, so that a host build and
// a device build give the same bits.  Compiled with -ffp-contract=off like the rest of vcm_core.h.
//
// Wavefront mode keeps every addend of every camera path apart until k_resolve adds them up (replay_path_color): the
// direct-illumination term, the vertex connections and the merge term of every camera vertex, and the emission term of
// the path's last segment; the light-tracing splats are added per pixel in vertex order by k_splat_apply /
// k_splat_apply_long.  A tracked context keeps, beside the framebuffer, VCM_PART_COUNT planes of 3 floats per pixel with
// the framebuffer's layout and meaning (running sums over iterations): 5 x 12 = 60 bytes per pixel, 252 MB at 2048^2, from
// vcm_track_parts(ctx, 1) to vcm_destroy.  The first vcm_part_device adds one float4 image (16 bytes per pixel).
//
// THE ORDER (part of the contract: the tests compare bits).  For pixel q and each of the four camera planes the plane's
// value is loaded once and the addends are added one at a time to that running value, with no per-path partial sum:
//   1. source paths ascending over { q - resX - 1, q - resX, q - 1, q }, those whose camOut.w == q, as k_resolve selects them;
//   2. within a path, vertices by ascending set bit L of camMask[lp];
//   3. within a vertex, the vertex connections k ascending.
// EMISSION takes camOut[lp].xyz once per source path.  LIGHT_TRACE is what k_splat_apply / k_splat_apply_long do to the
// framebuffer, with the plane in the framebuffer's place: the pixel's splats in increasing vertex index.
#ifndef SMALLVCM_AMD_VCM_PARTS_H
#define SMALLVCM_AMD_VCM_PARTS_H

#include "../../include/smallvcm_amd.h"
#include "vcm_core.h"

namespace vcm {

#define VCM_PARTS_BLOCK 256                /* lanes of a workgroup of every kernel here */
#define VCM_PARTS_DEFAULT_MAX_BLOCKS 2048  /* the grids' cap: 8 workgroups per CU of an MI355X; beyond it lanes stride */
#define VCM_PARTS_CAMERA 4                 /* the planes k_resolve_parts fills: EMISSION, DIRECT, CONNECT, MERGE */

VCM_HD bool parts_finite(float x) { return (f2u(x) & 0x7f800000u) != 0x7f800000u; }

/* the grid of the statistic and of the reads for n pixels: a function of n and the cap alone (never of the device), so
   that the order of the additions below is fixed */
inline int parts_grid_blocks(long long n, int maxBlocks)
{
    long long b = (n + VCM_PARTS_BLOCK - 1) / VCM_PARTS_BLOCK;
    if (b > maxBlocks) b = maxBlocks;
    return b < 1 ? 1 : (int)b;
}

/* ---------------- the split of one camera path ---------------- */
/* replay_path_color with the addends kept apart: pure latency like it, so per vertex the three slot-indexed loads go out
   together and the VC addends in batches of 4 */
VCM_HD void parts_replay_path(const IterParams &P, const VertexStore &vs, int lp, uint32_t mask, V3 emission,
                              V3 &em, V3 &di, V3 &vc, V3 &mg)
{
    while (mask) {
        const int L = __builtin_ctz(mask);
        mask &= mask - 1u;
        const size_t ps = path_slot(P, (uint32_t)L, (uint32_t)lp);
        const I4 m = vs.meta[ps];
        const F4 d = vs.diOut[ps];
        const F4 g = P.useVM ? vs.mergeOut[ps] : mk4(0.f, 0.f, 0.f, 0.f);
        if (m.x >= 0) di = di + mk3(d.x, d.y, d.z);
        for (int k0 = 0; k0 < m.z; k0 += 4) {
            F4 t[4];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
            for (int u = 0; u < 4; u++) t[u] = (k0 + u < m.z) ? vs.vcOut[m.y + k0 + u] : mk4(0.f, 0.f, 0.f, 0.f);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
            for (int u = 0; u < 4; u++) if (k0 + u < m.z) vc = vc + mk3(t[u].x, t[u].y, t[u].z);
        }
        if (P.useVM) mg = mg + mk3(g.x, g.y, g.z);
    }
    em = em + emission;
}

/* pixel q of the four camera planes (parts + i * planeStride, 3 floats per pixel) */
VCM_HD void parts_resolve_pixel(const IterParams &P, const F4 *camOut, const uint32_t *camMask, const VertexStore &vs, int q,
                                float *parts, size_t planeStride)
{
    const int src[4] = { q - P.resX - 1, q - P.resX, q - 1, q };
    float *p0 = parts + (size_t)q * 3, *p1 = p0 + planeStride, *p2 = p1 + planeStride, *p3 = p2 + planeStride;
    V3 em = mk3(p0[0], p0[1], p0[2]), di = mk3(p1[0], p1[1], p1[2]), vc = mk3(p2[0], p2[1], p2[2]), mg = mk3(p3[0], p3[1], p3[2]);
    bool touched = false;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int i = 0; i < 4; i++) {
        const int lp = src[i] - P.p0;
        if (lp < 0 || lp >= P.nLocal) continue;
        const F4 c = camOut[lp];
        if ((int)f2u(c.w) != q) continue;
        parts_replay_path(P, vs, lp, camMask[lp], mk3(c.x, c.y, c.z), em, di, vc, mg);
        touched = true;
    }
    if (!touched) return;
    p0[0] = em.x; p0[1] = em.y; p0[2] = em.z;
    p1[0] = di.x; p1[1] = di.y; p1[2] = di.z;
    p2[0] = vc.x; p2[1] = vc.y; p2[2] = vc.z;
    p3[0] = mg.x; p3[1] = mg.y; p3[2] = mg.z;
}

/* ---------------- the statistic ---------------- */
/* what a lane, a wave, a workgroup and the whole image carry: the luminance sums of the planes in binary64 and the count
   of pixels left out */
struct PartsAcc {
    double lum[VCM_PART_COUNT];
    long long nonFinite;
};

VCM_HD PartsAcc parts_acc_zero()
{
    PartsAcc a;
    for (int i = 0; i < VCM_PART_COUNT; i++) a.lum[i] = 0.0;
    a.nonFinite = 0;
    return a;
}

/* one pixel: a non-finite value in ANY plane leaves the pixel out of every sum (selects, not branches) */
VCM_HD void parts_acc_pixel(PartsAcc &a, const float *parts, size_t planeStride, long long p)
{
    double y[VCM_PART_COUNT];
    bool fin = true;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int i = 0; i < VCM_PART_COUNT; i++) {
        const float *v = parts + (size_t)i * planeStride + (size_t)p * 3;
        const float r = v[0], g = v[1], b = v[2];
        fin = fin && parts_finite(r) && parts_finite(g) && parts_finite(b);
        y[i] = 0.212671 * (double)r + 0.715160 * (double)g + 0.072169 * (double)b;
    }
    a.nonFinite = a.nonFinite + (fin ? 0 : 1);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int i = 0; i < VCM_PART_COUNT; i++) a.lum[i] = a.lum[i] + (fin ? y[i] : 0.0);
}

/* a += b: the one combination of the tree */
VCM_HD void parts_acc_combine(PartsAcc &a, const PartsAcc &b)
{
    for (int i = 0; i < VCM_PART_COUNT; i++) a.lum[i] = a.lum[i] + b.lum[i];
    a.nonFinite = a.nonFinite + b.nonFinite;
}

/* THE TREE over the VCM_PARTS_BLOCK slots v[] of a workgroup (the shape of var_tree_step, vcm_variance.h):
 *   steps 0 .. 5   inside every wave of 64: slot += slot + 32, 16, 8, 4, 2, 1
 *   steps 6, 7     across the waves: slots 0 and 128 take 64 and 192, then slot 0 takes 128
 * The device runs a step on all lanes and a barrier, the emulation a step over all lanes in a loop: a step reads only slots
 * no lane of that step writes, so both orders give the same additions.  The result is v[0]. */
#define VCM_PARTS_TREE_STEPS 8
VCM_HD void parts_tree_step(PartsAcc *v, int step, int lane)
{
    if (step < 6) {
        const int off = 32 >> step;
        if ((lane & 63) < off) parts_acc_combine(v[lane], v[lane + off]);
    } else {
        const int off = 64 << (step - 6);
        if (lane % (2 * off) == 0) parts_acc_combine(v[lane], v[lane + off]);
    }
}

/* what lane `lane` of workgroup `block` sums, in index order: the pixels g, g + G, g + 2 G, ... (g its global index, G
   the lanes of the grid) */
VCM_HD PartsAcc parts_lane_sum(long long n, int blocks, int block, int lane, const float *parts, size_t planeStride)
{
    PartsAcc a = parts_acc_zero();
    const long long G = (long long)blocks * VCM_PARTS_BLOCK;
    for (long long p = (long long)block * VCM_PARTS_BLOCK + lane; p < n; p += G) parts_acc_pixel(a, parts, planeStride, p);
    return a;
}

/* the second level: lane `lane` of ONE workgroup sums the workgroups' partials lane, lane + 256, ... in index order */
VCM_HD PartsAcc parts_lane_sum_partials(const PartsAcc *partials, int blocks, int lane)
{
    PartsAcc a = parts_acc_zero();
    for (int b = lane; b < blocks; b += VCM_PARTS_BLOCK) parts_acc_combine(a, partials[b]);
    return a;
}

/* the image's PartsAcc as the caller's record (include/smallvcm_amd.h) */
inline void parts_finish_stats(const PartsAcc &a, int k, long long n, vcm_parts_stats *out)
{
    out->iterations = k;
    out->pixels = n;
    out->nonFinite = a.nonFinite;
    for (int i = 0; i < VCM_PART_COUNT; i++) out->luminance[i] = a.lum[i] / (double)k;
}

/* ---------------- launches (vcm_parts.hip; the C-ABI of vcm_api.hip calls them) ---------------- */
#if defined(__HIPCC__)
/* the cap of the grids (vcm_debug_parts_max_blocks) */
int parts_max_blocks();
void parts_set_max_blocks(int blocks);
/* the four camera planes of one iteration, behind its k_resolve; `blocks`: k_resolve's grid, capped by parts_max_blocks */
hipError_t parts_launch_resolve(const IterParams &P, const F4 *camOut, const uint32_t *camMask, const VertexStore &vs, float *parts,
                                size_t planeStride, int blocks, hipStream_t stream);
/* *result (device) = the reduced PartsAcc of the planes; partials: maxBlocks PartsAcc of device scratch */
hipError_t parts_launch_stats(long long n, const float *parts, size_t planeStride, int maxBlocks, PartsAcc *partials, PartsAcc *result,
                              hipStream_t stream);
/* out3[3 p + c] = plane[3 p + c] * scale;  out4[p] = { plane rgb * scale, 1 } */
hipError_t parts_launch_read3(long long n, const float *plane, float scale, float *out3, hipStream_t stream);
hipError_t parts_launch_read4(long long n, const float *plane, float scale, F4 *out4, hipStream_t stream);
#endif

} // namespace vcm
#endif
