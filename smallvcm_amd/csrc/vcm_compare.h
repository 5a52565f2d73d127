// vcm_compare.h -- the comparison of an image with a reference image, host+device: what one pixel and one window compute
// and the order in which lanes are combined.  The kernels of vcm_compare.hip and the host emulation of the tests
// (tests/host_emul_compare) run THESE functions, so that a host build and a device build give the same bits.  Arithmetic:
// + - * / and comparisons only, compiled with -ffp-contract=off like vcm_denoise.h.
//
// img = source * scale and ref are linear RGB images of 3 or 4 floats per pixel; d_c = img_c - ref_c in binary32.
//   a pixel with a non-finite channel in either image is counted in nonFinite and left out of every sum, of the maximum
//   and of every window that holds it (vcm_get_noise_stats treats its elements the same way)
//   se   d^2                             mse    = its mean over the counted pixels' channels
//   rel  d^2 / (ref^2 + relEpsilon)      relMse = its mean: rel_mse() of the tests
//   ae   |d|                             mae    = its mean
//   maxAbs = the largest |d|, maxPixel the pixel that holds it (the lowest index on ties)
//   above  = the pixels whose largest rel exceeds `threshold`
// The three sums are binary64 sums of binary32 terms.
//
// SSIM (Wang, Bovik, Sheikh, Simoncelli 2004) on the luminance Y = 0.212671 r + 0.715160 g + 0.072169 b of both images,
// clamped to [0, peak] and divided by peak: x of img, y of ref.  The window is the 11 x 11 Gaussian of sigma 1.5, separable:
// cmp_window_weights() is its one-dimensional table.  The five moments E[x], E[y], E[xx], E[yy], E[xy] of a window are
// summed in binary32, along the rows first (cmp_hpass), then along the columns (cmp_vpass), the taps in index order.  Only
// the windows that lie wholly inside the image exist: (W - 10) x (H - 10) of them, none in an image narrower or lower than
// 11 pixels.  A non-finite pixel enters as x = y = NaN, so that exactly the windows that hold one have a NaN mean: they are
// left out.
#ifndef SMALLVCM_AMD_VCM_COMPARE_H
#define SMALLVCM_AMD_VCM_COMPARE_H

#include "../../include/smallvcm_amd.h"
#include "vcm_math.h"

namespace vcm {

#define VCM_CMP_BLOCK 256                 /* lanes of a workgroup of every kernel */
#define VCM_CMP_DEFAULT_MAX_BLOCKS 2048   /* the pixel kernel's grid cap: 8 workgroups per CU of an MI355X; beyond it lanes stride */
#define VCM_CMP_RADIUS 5
#define VCM_CMP_TAPS (2 * VCM_CMP_RADIUS + 1)
#define VCM_CMP_TILE_X 32                 /* the windows of a workgroup of the SSIM kernel: 32 x 8 */
#define VCM_CMP_TILE_Y 8
#define VCM_CMP_MAX_TILES_Y 65535         /* the y dimension of a grid: with ssim on, a frame of at most 524290 rows */

VCM_HD bool cmp_finite(float x) { return (f2u(x) & 0x7f800000u) != 0x7f800000u; }
VCM_HD bool cmp_finite3(V3 c) { return cmp_finite(c.x) && cmp_finite(c.y) && cmp_finite(c.z); }

/* ---------------- parameters ---------------- */
inline void cmp_defaults(vcm_compare_params *p)
{
    p->relEpsilon = 0.01f; p->peak = 1.f; p->threshold = u2f(0x7f800000u) /* +Inf: counts none */; p->ssim = 1; p->writeMap = 0;
}

inline const char *cmp_check_params(const vcm_compare_params *p)
{
    if (!p) return "params is NULL";
    if (!cmp_finite(p->relEpsilon) || !(p->relEpsilon > 0.f)) return "relEpsilon must be positive and finite";
    if (!cmp_finite(p->peak) || !(p->peak > 0.f)) return "peak must be positive and finite";
    if (!(p->threshold == p->threshold) || p->threshold == u2f(0xff800000u)) return "threshold must be finite or +Inf";
    if (p->ssim != 0 && p->ssim != 1) return "ssim must be 0 or 1";
    if (p->writeMap != 0 && p->writeMap != 1) return "writeMap must be 0 or 1";
    return NULL;
}

/* The 11 weights exp(-(k - 5)^2 / (2 * 1.5^2)) / their sum: divided in binary64 and rounded to binary32 once.  Written
   down as the binary32 numbers themselves, so that the table does not depend on a host's exp(); tests/test_compare.py
   derives it again. */
struct CmpWin { float w[VCM_CMP_TAPS]; };
inline CmpWin cmp_window_weights()
{
    const CmpWin t = { { 0x1.0d956cp-10f, 0x1.f1fe02p-8f, 0x1.26eb18p-5f, 0x1.bff0fep-4f, 0x1.b43c4p-3f, 0x1.10656p-2f,
                         0x1.b43c4p-3f, 0x1.bff0fep-4f, 0x1.26eb18p-5f, 0x1.f1fe02p-8f, 0x1.0d956cp-10f } };
    return t;
}

/* the grid of the pixel kernel for n pixels: a function of n and the cap alone (never of the device), so that the order
   of the additions below is fixed */
inline int cmp_grid_blocks(long long n, int maxBlocks)
{
    long long b = (n + VCM_CMP_BLOCK - 1) / VCM_CMP_BLOCK;
    if (b > maxBlocks) b = maxBlocks;
    return b < 1 ? 1 : (int)b;
}
/* the grid of the SSIM kernel: the tiles of 32 x 8 windows that cover the (W - 10) x (H - 10) windows; 0 x 0 without one */
inline int cmp_tiles_x(int W) { return W < VCM_CMP_TAPS ? 0 : (W - 2 * VCM_CMP_RADIUS + VCM_CMP_TILE_X - 1) / VCM_CMP_TILE_X; }
inline int cmp_tiles_y(int H) { return H < VCM_CMP_TAPS ? 0 : (H - 2 * VCM_CMP_RADIUS + VCM_CMP_TILE_Y - 1) / VCM_CMP_TILE_Y; }
inline long long cmp_tiles(int W, int H) { return (W < VCM_CMP_TAPS || H < VCM_CMP_TAPS) ? 0 : (long long)cmp_tiles_x(W) * cmp_tiles_y(H); }

/* what the SSIM kernel's grid cannot cover: refused by name where ssim is on */
inline const char *cmp_check_size(int H, const vcm_compare_params *p)
{
    if (p->ssim && cmp_tiles_y(H) > VCM_CMP_MAX_TILES_Y) return "the frame has more than 524290 rows: too tall for the SSIM kernel's grid, compare it with ssim 0";
    return NULL;
}

/* ---------------- the pixel ---------------- */
/* what a lane, a workgroup and the whole image carry of the pixel metrics */
struct CmpAcc {
    double se, rel, ae;
    float maxAbs;
    int pad;
    long long maxPixel, nonFinite, above;
};
/* ... and of the windows */
struct SsimAcc {
    double sum;
    long long windows;
};
/* what the last kernel leaves for the host */
struct CmpResult {
    CmpAcc pix;
    SsimAcc win;
};

#define VCM_CMP_NO_PIXEL 0x7fffffffffffffffll

VCM_HD CmpAcc cmp_acc_zero()
{
    CmpAcc a;
    a.se = 0.0; a.rel = 0.0; a.ae = 0.0; a.maxAbs = u2f(0xff800000u) /* -inf */; a.pad = 0;
    a.maxPixel = VCM_CMP_NO_PIXEL; a.nonFinite = 0; a.above = 0;
    return a;
}
VCM_HD SsimAcc cmp_ssim_zero() { SsimAcc a; a.sum = 0.0; a.windows = 0; return a; }

VCM_HD float cmp_abs(float d) { return d < 0.f ? 0.f - d : d; }
VCM_HD float cmp_max3(float a, float b, float c) { const float m = b > a ? b : a; return c > m ? c : m; }

/* pixel p of an image of `channels` (3 or 4) floats per pixel */
VCM_HD V3 cmp_load(const float *src, int channels, long long p)
{
    const float *c = src + (size_t)p * (size_t)channels;
    return mk3(c[0], c[1], c[2]);
}
VCM_HD V3 cmp_scaled(V3 c, float scale) { return mk3(c.x * scale, c.y * scale, c.z * scale); }

/* One pixel: img (scaled already) against ref.  Returns the map's entry { rel r, g, b; 0 }; a non-finite pixel gives
   { 0, 0, 0, 0 } and counts in nonFinite alone.  Selects, not branches, on the accumulators: adding 0.0 changes no sum. */
VCM_HD F4 cmp_pixel(CmpAcc &a, V3 img, V3 ref, long long p, float relEps, float threshold)
{
    const bool fin = cmp_finite3(img) && cmp_finite3(ref);
    const float dx = img.x - ref.x, dy = img.y - ref.y, dz = img.z - ref.z;
    const float sx = dx * dx, sy = dy * dy, sz = dz * dz;
    const float rx = sx / (ref.x * ref.x + relEps), ry = sy / (ref.y * ref.y + relEps), rz = sz / (ref.z * ref.z + relEps);
    const float ax = cmp_abs(dx), ay = cmp_abs(dy), az = cmp_abs(dz);
    const float amax = cmp_max3(ax, ay, az), rmax = cmp_max3(rx, ry, rz);
    a.nonFinite = a.nonFinite + (fin ? 0 : 1);
    a.se = ((a.se + (fin ? (double)sx : 0.0)) + (fin ? (double)sy : 0.0)) + (fin ? (double)sz : 0.0);
    a.rel = ((a.rel + (fin ? (double)rx : 0.0)) + (fin ? (double)ry : 0.0)) + (fin ? (double)rz : 0.0);
    a.ae = ((a.ae + (fin ? (double)ax : 0.0)) + (fin ? (double)ay : 0.0)) + (fin ? (double)az : 0.0);
    const bool larger = fin && amax > a.maxAbs;   /* a lane meets its pixels in index order: the first of equals stays */
    a.maxPixel = larger ? p : a.maxPixel;
    a.maxAbs = larger ? amax : a.maxAbs;
    a.above = a.above + ((fin && rmax > threshold) ? 1 : 0);
    return fin ? mk4(rx, ry, rz, 0.f) : mk4(0.f, 0.f, 0.f, 0.f);
}

/* a += b: the one combination of the tree.  Of two equal maxima the lower pixel index wins, whatever the order. */
VCM_HD void cmp_acc_combine(CmpAcc &a, const CmpAcc &b)
{
    a.se = a.se + b.se;
    a.rel = a.rel + b.rel;
    a.ae = a.ae + b.ae;
    const bool take = b.maxAbs > a.maxAbs || (b.maxAbs == a.maxAbs && b.maxPixel < a.maxPixel);
    a.maxPixel = take ? b.maxPixel : a.maxPixel;
    a.maxAbs = take ? b.maxAbs : a.maxAbs;
    a.nonFinite = a.nonFinite + b.nonFinite;
    a.above = a.above + b.above;
}
VCM_HD void cmp_ssim_combine(SsimAcc &a, const SsimAcc &b) { a.sum = a.sum + b.sum; a.windows = a.windows + b.windows; }

/* THE TREE over the VCM_CMP_BLOCK slots v[] of a workgroup: step s of VCM_CMP_TREE_STEPS, lane `lane` (the tree of
 * vcm_variance.h, stated again for this unit's accumulators).
 *   steps 0 .. 5   inside every wave of 64: slot += slot + 32, 16, 8, 4, 2, 1
 *   steps 6, 7     across the waves: slots 0 and 128 take 64 and 192, then slot 0 takes 128
 * The device runs a step on all lanes and a barrier, the emulation a step over all lanes in a loop: a step reads only slots
 * no lane of that step writes, so both orders give the same additions.  The result is v[0]. */
#define VCM_CMP_TREE_STEPS 8
VCM_HD bool cmp_tree_pair(int step, int lane, int &other)
{
    if (step < 6) {
        const int off = 32 >> step;
        other = lane + off;
        return (lane & 63) < off;
    }
    const int off = 64 << (step - 6);
    other = lane + off;
    return lane % (2 * off) == 0;
}
VCM_HD void cmp_tree_step(CmpAcc *v, int step, int lane) { int o; if (cmp_tree_pair(step, lane, o)) cmp_acc_combine(v[lane], v[o]); }
VCM_HD void cmp_tree_step(SsimAcc *v, int step, int lane) { int o; if (cmp_tree_pair(step, lane, o)) cmp_ssim_combine(v[lane], v[o]); }

/* what lane `lane` of workgroup `block` of the pixel kernel sums, in index order: the pixels g, g + G, g + 2 G, ... (g its
   global index, G the lanes of the grid); pixel(p, acc) runs cmp_pixel on pixel p */
template <class Pixel>
VCM_HD CmpAcc cmp_lane_sum(long long n, int blocks, int block, int lane, Pixel &&pixel)
{
    CmpAcc a = cmp_acc_zero();
    const long long G = (long long)blocks * VCM_CMP_BLOCK;
    for (long long p = (long long)block * VCM_CMP_BLOCK + lane; p < n; p += G) pixel(p, a);
    return a;
}

/* the second level: lane `lane` of ONE workgroup sums the workgroups' partials lane, lane + 256, ... in index order */
VCM_HD CmpAcc cmp_lane_sum_partials(const CmpAcc *partials, long long count, int lane)
{
    CmpAcc a = cmp_acc_zero();
    for (long long b = lane; b < count; b += VCM_CMP_BLOCK) cmp_acc_combine(a, partials[b]);
    return a;
}
VCM_HD SsimAcc cmp_lane_sum_partials(const SsimAcc *partials, long long count, int lane)
{
    SsimAcc a = cmp_ssim_zero();
    for (long long b = lane; b < count; b += VCM_CMP_BLOCK) cmp_ssim_combine(a, partials[b]);
    return a;
}

/* ---------------- the window ---------------- */
struct CmpXY { float x, y; };
struct CmpMom { float mx, my, xx, yy, xy; };

VCM_HD float cmp_luminance(V3 c) { return (0.212671f * c.x + 0.715160f * c.y) + 0.072169f * c.z; }
VCM_HD float cmp_clamp(float v, float peak) { return v > 0.f ? (v < peak ? v : peak) : 0.f; }

/* what a pixel enters the windows as; img scaled already */
VCM_HD CmpXY cmp_window_input(V3 img, V3 ref, float peak)
{
    CmpXY r;
    if (!(cmp_finite3(img) && cmp_finite3(ref))) { r.x = u2f(0x7fc00000u); r.y = u2f(0x7fc00000u); return r; }
    r.x = cmp_clamp(cmp_luminance(img), peak) / peak;
    r.y = cmp_clamp(cmp_luminance(ref), peak) / peak;
    return r;
}
/* ... and a place outside the image (only windows that do not exist reach it) */
VCM_HD CmpXY cmp_window_outside() { CmpXY r; r.x = u2f(0x7fc00000u); r.y = u2f(0x7fc00000u); return r; }

/* the rows' pass: load(k) gives the pixel k - 5 columns from the centre, k = 0 .. 10 */
template <class Load>
VCM_HD CmpMom cmp_hpass(const CmpWin &win, Load &&load)
{
    CmpMom m;
    {
        const CmpXY v = load(0);
        const float wx = win.w[0] * v.x, wy = win.w[0] * v.y;
        m.mx = wx; m.my = wy; m.xx = wx * v.x; m.yy = wy * v.y; m.xy = wx * v.y;
    }
#pragma unroll
    for (int k = 1; k < VCM_CMP_TAPS; k++) {
        const CmpXY v = load(k);
        const float wx = win.w[k] * v.x, wy = win.w[k] * v.y;
        m.mx = m.mx + wx; m.my = m.my + wy; m.xx = m.xx + wx * v.x; m.yy = m.yy + wy * v.y; m.xy = m.xy + wx * v.y;
    }
    return m;
}

/* the columns' pass: load(k) gives the rows' moments k - 5 rows from the centre */
template <class Load>
VCM_HD CmpMom cmp_vpass(const CmpWin &win, Load &&load)
{
    CmpMom m;
    {
        const CmpMom v = load(0);
        m.mx = win.w[0] * v.mx; m.my = win.w[0] * v.my; m.xx = win.w[0] * v.xx; m.yy = win.w[0] * v.yy; m.xy = win.w[0] * v.xy;
    }
#pragma unroll
    for (int k = 1; k < VCM_CMP_TAPS; k++) {
        const CmpMom v = load(k);
        m.mx = m.mx + win.w[k] * v.mx; m.my = m.my + win.w[k] * v.my; m.xx = m.xx + win.w[k] * v.xx;
        m.yy = m.yy + win.w[k] * v.yy; m.xy = m.xy + win.w[k] * v.xy;
    }
    return m;
}

/* a window counts where no pixel of it is non-finite: x and y lie in [0, 1] otherwise, and so does their mean */
VCM_HD bool cmp_window_counts(const CmpMom &m) { return cmp_finite(m.mx); }

/* SSIM of a window's moments, C1 = 0.01^2, C2 = 0.03^2.  With x == y, bit for bit: mx == my and xx == yy == xy, so that
 * mx * my == mx * mx == my * my and the three (co)variances are one number; 2 a is written a + a, and numerator and
 * denominator are then the same two sums and the same product: the quotient is exactly 1.  The denominator is positive:
 * mx^2 + my^2 + C1 >= C1, and the variances, a few ulp of 1 below zero at worst, leave C2 = 9e-4 standing. */
VCM_HD float cmp_ssim(const CmpMom &m)
{
    const float C1 = 0.0001f, C2 = 0.0009f;
    const float mxy = m.mx * m.my, mxx = m.mx * m.mx, myy = m.my * m.my;
    const float sxy = m.xy - mxy, sxx = m.xx - mxx, syy = m.yy - myy;
    return (((mxy + mxy) + C1) * ((sxy + sxy) + C2)) / (((mxx + myy) + C1) * ((sxx + syy) + C2));
}

/* ---------------- the result ---------------- */
/* the image's accumulators as the caller's record (include/smallvcm_amd.h); psnr in binary64 on the host.  Without a
   counted pixel the means are NaN (0 / 0) and maxPixel is -1; without a window ssim is NaN. */
inline void cmp_finish_stats(const CmpResult &r, int iterations, long long n, float peak, vcm_compare_stats *out)
{
    const double nan = (double)u2f(0x7fc00000u), inf = (double)u2f(0x7f800000u);
    const long long counted = n - r.pix.nonFinite;
    out->iterations = iterations;
    out->pixels = n;
    out->nonFinite = r.pix.nonFinite;
    out->above = r.pix.above;
    out->ssimWindows = r.win.windows;
    out->maxPixel = counted > 0 ? r.pix.maxPixel : -1;
    out->mse = counted > 0 ? r.pix.se / (3.0 * (double)counted) : nan;
    out->relMse = counted > 0 ? r.pix.rel / (3.0 * (double)counted) : nan;
    out->mae = counted > 0 ? r.pix.ae / (3.0 * (double)counted) : nan;
    out->maxAbs = counted > 0 ? (double)r.pix.maxAbs : 0.0;
    out->psnr = counted > 0 ? (out->mse > 0.0 ? 10.0 * log10(((double)peak * (double)peak) / out->mse) : (out->mse == 0.0 ? inf : nan)) : nan;
    out->ssim = r.win.windows > 0 ? r.win.sum / (double)r.win.windows : nan;
}

/* ---------------- launches (vcm_compare.hip; the C-ABI of vcm_api.hip calls them) ---------------- */
/* accumulators of device scratch a comparison of a W x H image needs at most: the pixel kernel's partials, the SSIM
   kernel's, the result; in bytes, each part 16-byte aligned */
inline size_t cmp_scratch_bytes(int W, int H, int maxBlocks)
{
    return (size_t)maxBlocks * sizeof(CmpAcc) + (size_t)cmp_tiles(W, H) * sizeof(SsimAcc) + sizeof(CmpResult);
}

#if defined(__HIPCC__)
/* the cap of the pixel kernel's grid (vcm_debug_compare_max_blocks) */
int cmp_max_blocks();
void cmp_set_max_blocks(int blocks);
/* The comparison of img * scale with ref, both W x H pixels of 3 or 4 floats, on `stream`: the pixel kernel, the SSIM kernel
   with p.ssim, the kernel that combines their partials.  scratch: cmp_scratch_bytes(W, H, maxBlocks) bytes, 16-byte aligned;
   the CmpResult lies at its end (cmp_result_of).  map: W * H float4 { rel r, g, b; the SSIM of the pixel's window or 0 }, or
   NULL. */
hipError_t cmp_launch(int W, int H, const float *img, int imgChannels, float scale, const float *ref, int refChannels,
                      const vcm_compare_params &p, int maxBlocks, F4 *map, char *scratch, hipStream_t stream);
inline CmpResult *cmp_result_of(char *scratch, int W, int H, int maxBlocks)
{
    return (CmpResult *)(scratch + cmp_scratch_bytes(W, H, maxBlocks) - sizeof(CmpResult));
}
#endif

} // namespace vcm
#endif
