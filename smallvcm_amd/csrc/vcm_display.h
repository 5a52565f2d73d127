// vcm_display.h -- the display transform, host+device: what turns a linear HDR image into something a screen can show.
// The kernels of vcm_display.hip and the host emulation of the tests (tests/host_emul_display) run THESE functions, so that
// a host build and a device build give the same bits.  Arithmetic: + - * /, comparisons, integer operations on the bit
// pattern, float <-> int conversions, and dm_powf (detmath.h) for the transfer curve; compiled with -ffp-contract=off.
//
// The pipeline on the linear pixel c * scale, in this order:
//   1 exposure   E = (c * scale) * m, m = (float)exp2(autoEV + exposureEV); autoEV from a log-luminance histogram
//   2 bloom      (1 - s) E + s B, B an energy-preserving pyramid blur of E (below, "bloom")
//   3 tone curve CLAMP | REINHARD | ACES | HABLE on the sanitised pixel, then clamped to [0, 1]
//   4 transfer   GAMMA (dm_powf(c, 1 / gamma), as k_encode_image) | SRGB
//   5 bytes      truncation (the reference's), or stochastic rounding by an integer hash (vcm_read_display_image only)
// Steps 1-4 give the float4 image { rgb in [0, 1], 1 }.
//
// Auto-exposure reads 264 64-bit counters (2112 bytes) back and synchronises the stream once: the exposure is a host
// number (binary64, disp_auto_exposure below) that the later kernels take as an argument.  A frame's display transform
// is not the inner loop of anything, and a device-side log2/exp2 would have to be a second implementation of that function.
#ifndef SMALLVCM_AMD_VCM_DISPLAY_H
#define SMALLVCM_AMD_VCM_DISPLAY_H

#include "../../include/smallvcm_amd.h"
#include "vcm_math.h"
#include "detmath.h"

namespace vcm {

#define VCM_DISP_BLOCK 256                 /* lanes of a workgroup of every kernel */
#define VCM_DISP_DEFAULT_MAX_BLOCKS 2048   /* the grid's cap: 8 workgroups per CU of an MI355X; beyond it lanes stride */
#define VCM_DISP_BINS 256
/* the counters: bins 0 .. 255, then */
#define VCM_DISP_ZERO 256          /* Y <= 0 */
#define VCM_DISP_NONFINITE 257     /* Y NaN or +-Inf */
#define VCM_DISP_CLAMPED_LOW 258   /* Y < 2^-20: counted in bin 0 too */
#define VCM_DISP_CLAMPED_HIGH 259  /* Y >= 2^12: counted in bin 255 too */
#define VCM_DISP_CLIPPED 260       /* channels that reached 1.0 after the curve */
#define VCM_DISP_COUNTERS 264      /* rounded up: 2112 bytes */
#define VCM_DISP_MAX_LEVELS 8
#define VCM_DISP_MAX_LINEAR 1099511627776.f   /* 2^40: what +Inf enters a curve as (its square is finite in fp32) */

VCM_HD bool disp_finite(float x) { return (f2u(x) & 0x7f800000u) != 0x7f800000u; }
VCM_HD float disp_clamp01(float x) { return x > 0.f ? (x < 1.f ? x : 1.f) : 0.f; }   /* NaN -> 0 */

/* ---------------- parameters ---------------- */
inline const char *disp_check_params(const vcm_display_params *p)
{
    if (!p) return "params is NULL";
    if (p->curve < VCM_CURVE_CLAMP || p->curve > VCM_CURVE_HABLE) return "unknown curve";
    if (!disp_finite(p->whitePoint) || !(p->whitePoint > 0.f)) return "whitePoint must be positive and finite";
    if (!disp_finite(p->exposureEV) || p->exposureEV < -32.f || p->exposureEV > 32.f) return "exposureEV must lie in [-32, 32]";
    if (p->autoExposure != 0 && p->autoExposure != 1) return "autoExposure must be 0 or 1";
    if (!disp_finite(p->key) || !(p->key > 0.f)) return "key must be positive and finite";
    if (!(p->lowPercentile >= 0.f) || !(p->highPercentile <= 1.f) || !(p->lowPercentile < p->highPercentile))
        return "percentiles must satisfy 0 <= lowPercentile < highPercentile <= 1";
    if (!(p->minEV >= -32.f) || !(p->maxEV <= 32.f) || !(p->minEV <= p->maxEV)) return "minEV, maxEV must satisfy -32 <= minEV <= maxEV <= 32";
    if (p->transfer != VCM_TRANSFER_GAMMA && p->transfer != VCM_TRANSFER_SRGB) return "unknown transfer";
    if (!disp_finite(p->gamma) || !(p->gamma > 0.f)) return "gamma must be positive and finite";
    if (!(p->bloomStrength >= 0.f) || !(p->bloomStrength <= 1.f)) return "bloomStrength must lie in [0, 1]";
    if (p->bloomLevels < 1 || p->bloomLevels > VCM_DISP_MAX_LEVELS) return "bloomLevels must lie in 1 .. 8";
    if (p->dither != 0 && p->dither != 1) return "dither must be 0 or 1";
    return NULL;
}

inline void disp_defaults(vcm_display_params *p)
{
    p->curve = VCM_CURVE_CLAMP; p->whitePoint = 4.f; p->exposureEV = 0.f;
    p->autoExposure = 0; p->key = 0.18f; p->lowPercentile = 0.10f; p->highPercentile = 0.95f; p->minEV = -16.f; p->maxEV = 16.f;
    p->transfer = VCM_TRANSFER_GAMMA; p->gamma = 2.2f;
    p->bloomStrength = 0.f; p->bloomLevels = 5;
    p->dither = 0; p->ditherSeed = 0u;
}

/* the grid for n pixels: a function of n and the cap alone */
inline int disp_grid_blocks(long long n, int maxBlocks)
{
    long long b = (n + VCM_DISP_BLOCK - 1) / VCM_DISP_BLOCK;
    if (b > maxBlocks) b = maxBlocks;
    return b < 1 ? 1 : (int)b;
}

/* ---------------- the pixel ---------------- */
/* pixel p of an image of `channels` (3 or 4) floats per pixel, times scale */
VCM_HD V3 disp_load(const float *src, int channels, long long p, float scale)
{
    const float *c = src + (size_t)p * (size_t)channels;
    return mk3(c[0] * scale, c[1] * scale, c[2] * scale);
}

VCM_HD float disp_luminance(V3 c) { return (0.2126f * c.x + 0.7152f * c.y) + 0.0722f * c.z; }

VCM_HD bool disp_finite3(V3 c) { return disp_finite(c.x) && disp_finite(c.y) && disp_finite(c.z); }

/* ---------------- the histogram ---------------- */
/* The counter a luminance goes to (a bin, VCM_DISP_ZERO or VCM_DISP_NONFINITE), and in `second` VCM_DISP_CLAMPED_LOW / _HIGH
 * or -1.  The bin is read from the bit pattern alone: exponent and the top three mantissa bits, eight bins per octave from
 * 2^-20 (bin 0) to 2^12 (the upper edge of bin 255); bin b = 8 o + m covers 2^(o - 20) [1 + m / 8, 1 + (m + 1) / 8). */
VCM_HD int disp_counter(float Y, int &second)
{
    second = -1;
    if (!disp_finite(Y)) return VCM_DISP_NONFINITE;
    if (!(Y > 0.f)) return VCM_DISP_ZERO;
    const int raw = (int)(f2u(Y) >> 20) - ((127 - 20) << 3);
    if (raw < 0) { second = VCM_DISP_CLAMPED_LOW; return 0; }
    if (raw > VCM_DISP_BINS - 1) { second = VCM_DISP_CLAMPED_HIGH; return VCM_DISP_BINS - 1; }
    return raw;
}

/* The exposure from the counters, in binary64, on the host: the library and the emulation both call it.
 *   N = sum of the bins, lo = lowPercentile N, hi = highPercentile N; bin b occupies the ranks [C_b, C_b + h_b) and weighs
 *   max(0, min(C_b + h_b, hi) - max(C_b, lo)); log2 Lavg = the weighted mean of the bins' log2 centres (the mean of the
 *   log2 of a bin's two edges); autoEV = clamp(log2(key / Lavg), minEV, maxEV), 0 with no weight.
 * Fills every member of *out but `clipped`; the multiplier is the fp32 number the kernels apply. */
inline void disp_auto_exposure(const unsigned long long *counters, const vcm_display_params &p, vcm_display_stats *out)
{
    double N = 0.0;
    for (int b = 0; b < VCM_DISP_BINS; b++) N += (double)counters[b];
    const double lo = (double)p.lowPercentile * N, hi = (double)p.highPercentile * N;
    double C = 0.0, wsum = 0.0, lsum = 0.0;
    for (int b = 0; b < VCM_DISP_BINS; b++) {
        const double h = (double)counters[b];
        const double top = (C + h < hi) ? C + h : hi, bot = (C > lo) ? C : lo;
        const double w = top > bot ? top - bot : 0.0;
        if (w > 0.0) {
            const double o = (double)((b >> 3) - 20), m = (double)(b & 7);
            const double centre = o + 0.5 * (log2(1.0 + m / 8.0) + log2(1.0 + (m + 1.0) / 8.0));
            wsum += w; lsum += w * centre;
        }
        C += h;
    }
    double ev = 0.0, logAvg = 0.0;
    if (wsum > 0.0) {
        logAvg = lsum / wsum;
        ev = log2((double)p.key) - logAvg;
        if (ev < (double)p.minEV) ev = (double)p.minEV;
        if (ev > (double)p.maxEV) ev = (double)p.maxEV;
    }
    if (!p.autoExposure) { ev = 0.0; }
    out->autoEV = ev;
    out->logAvgLuminance = logAvg;
    out->multiplier = (double)(float)exp2(ev + (double)p.exposureEV);
    out->counted = N < 9.0e18 ? (long long)N : (long long)9.0e18;   /* (an image's counters stay below 2^39) */
    out->zero = (long long)counters[VCM_DISP_ZERO];
    out->nonFinite = (long long)counters[VCM_DISP_NONFINITE];
    out->clampedLow = (long long)counters[VCM_DISP_CLAMPED_LOW];
    out->clampedHigh = (long long)counters[VCM_DISP_CLAMPED_HIGH];
    out->clipped = 0;
}

/* ---------------- bloom ----------------
 * Level 0 is the exposed image E (a pixel with a non-finite channel enters as 0).  Level l has
 * w_l = max(1, (w_{l-1} + 1) / 2) columns, and rows likewise.
 *   D_l  the mean of the 2 x 2 block of G_{l-1} (G_0 = E), coordinates clamped to the edge
 *   G_l  D_l blurred by the separable binomial [1 4 6 4 1] / 16, rows first, then columns, clamp-to-edge
 *   U_L = G_L, U_l = G_l + up(U_{l+1}); B = up(U_1) / L
 *   up   x 2 bilinear, source coordinate (x + 0.5) / 2 - 0.5: weights 0.75 / 0.25, indices clamped
 * and the result is (1 - s) E + s B; a pixel of E with a non-finite channel stays what it was.  Every weight is
 * non-negative and every stage's weights sum to one: a constant image stays constant, and away from the border the sum
 * of the image is kept. */
VCM_HD int disp_level_dim(int w) { const int h = (w + 1) / 2; return h < 1 ? 1 : h; }
VCM_HD int disp_clampi(int i, int n) { return i < 0 ? 0 : (i > n - 1 ? n - 1 : i); }

VCM_HD F4 disp_add4(F4 a, F4 b) { return mk4(a.x + b.x, a.y + b.y, a.z + b.z, 0.f); }
VCM_HD F4 disp_mul4(F4 a, float s) { return mk4(a.x * s, a.y * s, a.z * s, 0.f); }

/* E of a pixel as the bloom sees it */
VCM_HD F4 disp_bloom_input(V3 c, float mult)
{
    const V3 e = mk3(c.x * mult, c.y * mult, c.z * mult);
    if (!disp_finite3(e)) return mk4(0.f, 0.f, 0.f, 0.f);
    return mk4(e.x, e.y, e.z, 0.f);
}

/* D_l(x, y): load(xs, ys) gives level l - 1 (ws x hs) */
template <class Load>
VCM_HD F4 disp_down(int x, int y, int ws, int hs, Load &&load)
{
    const int x0 = disp_clampi(2 * x, ws), x1 = disp_clampi(2 * x + 1, ws), y0 = disp_clampi(2 * y, hs), y1 = disp_clampi(2 * y + 1, hs);
    return disp_mul4(disp_add4(disp_add4(load(x0, y0), load(x1, y0)), disp_add4(load(x0, y1), load(x1, y1))), 0.25f);
}

/* one axis of the blur: the five taps at i - 2 .. i + 2 (clamped to 0 .. n - 1), load(j) gives tap j */
template <class Load>
VCM_HD F4 disp_blur5(int i, int n, Load &&load)
{
    const F4 a = load(disp_clampi(i - 2, n)), b = load(disp_clampi(i - 1, n)), c = load(i), d = load(disp_clampi(i + 1, n)), e = load(disp_clampi(i + 2, n));
    const F4 outer = disp_add4(a, e), inner = disp_mul4(disp_add4(b, d), 4.f), mid = disp_mul4(c, 6.f);
    return disp_mul4(disp_add4(disp_add4(outer, inner), mid), 0.0625f);
}

/* up(S)(x, y): S has ws x hs pixels, load(xs, ys) gives it */
template <class Load>
VCM_HD F4 disp_up(int x, int y, int ws, int hs, Load &&load)
{
    /* even x: x / 2 - 1 weighs 0.25 and x / 2 weighs 0.75; odd x: (x - 1) / 2 weighs 0.75 and (x + 1) / 2 weighs 0.25 */
    const int xa = (x >> 1) - 1 + (x & 1), ya = (y >> 1) - 1 + (y & 1);
    const float wxa = (x & 1) ? 0.75f : 0.25f, wya = (y & 1) ? 0.75f : 0.25f;
    const int x0 = disp_clampi(xa, ws), x1 = disp_clampi(xa + 1, ws), y0 = disp_clampi(ya, hs), y1 = disp_clampi(ya + 1, hs);
    const F4 r0 = disp_add4(disp_mul4(load(x0, y0), wxa), disp_mul4(load(x1, y0), 1.f - wxa));
    const F4 r1 = disp_add4(disp_mul4(load(x0, y1), wxa), disp_mul4(load(x1, y1), 1.f - wxa));
    return disp_add4(disp_mul4(r0, wya), disp_mul4(r1, 1.f - wya));
}

/* (1 - s) E + s B of one pixel; up1 = up(U_1) at the pixel, invLevels = 1 / L */
VCM_HD V3 disp_bloom_combine(V3 c, float mult, F4 up1, float invLevels, float s)
{
    const V3 e = mk3(c.x * mult, c.y * mult, c.z * mult);
    if (!disp_finite3(e)) return e;
    const float t = 1.f - s;
    return mk3(t * e.x + s * (up1.x * invLevels), t * e.y + s * (up1.y * invLevels), t * e.z + s * (up1.z * invLevels));
}

/* ---------------- tone curves ---------------- */
/* what a curve takes: NaN and negative numbers as 0, +Inf as 2^40 */
VCM_HD float disp_sanitise(float c) { return c > 0.f ? (c < VCM_DISP_MAX_LINEAR ? c : VCM_DISP_MAX_LINEAR) : 0.f; }

VCM_HD float disp_aces(float x) { return (x * (2.51f * x + 0.03f)) / (x * (2.43f * x + 0.59f) + 0.14f); }

/* Hable's filmic curve.  The constant E / F is written (D E) / (D F), the quotient of the very products the fraction
   beside it holds at x = 0, so that h(0) is 0 in fp32 and not an ulp of 1/15 */
VCM_HD float disp_hable_h(float x)
{
    const float A = 0.15f, B = 0.5f, C = 0.1f, D = 0.2f, E = 0.02f, F = 0.3f;
    return (x * (A * x + C * B) + D * E) / (x * (A * x + B) + D * F) - (D * E) / (D * F);
}
VCM_HD float disp_hable(float x) { return disp_hable_h(2.f * x) / disp_hable_h(11.2f); }

/* step 3: the curve on a linear pixel, clamped to [0, 1]; `clipped` counts the channels that reached 1 */
VCM_HD V3 disp_curve(V3 lin, int curve, float whitePoint, int &clipped)
{
    V3 c = mk3(disp_sanitise(lin.x), disp_sanitise(lin.y), disp_sanitise(lin.z));
    if (curve == VCM_CURVE_REINHARD) {
        const float L = disp_luminance(c);
        if (L > 0.f) {
            const float Ld = (L * (1.f + L / (whitePoint * whitePoint))) / (1.f + L);
            const float s = Ld / L;
            c = mk3(c.x * s, c.y * s, c.z * s);
        } else c = mk3(0.f, 0.f, 0.f);
    } else if (curve == VCM_CURVE_ACES) {
        c = mk3(disp_aces(c.x), disp_aces(c.y), disp_aces(c.z));
    } else if (curve == VCM_CURVE_HABLE) {
        c = mk3(disp_hable(c.x), disp_hable(c.y), disp_hable(c.z));
    }
    clipped = (c.x >= 1.f ? 1 : 0) + (c.y >= 1.f ? 1 : 0) + (c.z >= 1.f ? 1 : 0);
    return mk3(disp_clamp01(c.x), disp_clamp01(c.y), disp_clamp01(c.z));
}

/* ---------------- transfer curves ---------------- */
/* step 4 on a channel in [0, 1]; invGamma = 1.f / gamma */
VCM_HD float disp_transfer(float c, int transfer, float invGamma)
{
    if (transfer == VCM_TRANSFER_SRGB) return c <= 0.0031308f ? 12.92f * c : 1.055f * dm_powf(c, 1.f / 2.4f) - 0.055f;
    return dm_powf(c, invGamma);
}

/* steps 3 and 4 */
VCM_HD F4 disp_finish(V3 lin, int curve, float whitePoint, int transfer, float invGamma, int &clipped)
{
    const V3 c = disp_curve(lin, curve, whitePoint, clipped);
    return mk4(disp_transfer(c.x, transfer, invGamma), disp_transfer(c.y, transfer, invGamma), disp_transfer(c.z, transfer, invGamma), 1.f);
}

/* ---------------- bytes ---------------- */
/* d in [0, 1) of (pixel index, channel, seed): the key (3 p + channel) ^ (seed * 0x9e3779b9) through the 32-bit integer
   finaliser x ^= x >> 16, x *= 0x7feb352d, x ^= x >> 15, x *= 0x846ca68b, x ^= x >> 16; the top 24 bits / 2^24 */
VCM_HD float disp_dither(long long p, int channel, unsigned seed)
{
    uint32_t x = (uint32_t)((unsigned long long)p * 3ull + (unsigned long long)channel) ^ (seed * 0x9e3779b9u);
    x ^= (uint32_t)((unsigned long long)p >> 30);   /* images beyond 2^30 pixels: the index's high bits */
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    return (float)(x >> 8) * (1.f / 16777216.f);
}

/* step 5: v in [0, 1] (anything else is clamped; NaN gives 0) */
VCM_HD unsigned char disp_byte(float v, int dither, long long p, int channel, unsigned seed)
{
    float t = v * 255.f;
    if (dither) t = t + disp_dither(p, channel, seed);   /* floor(v 255 + d): unbiased stochastic rounding */
    t = t > 0.f ? (t < 255.f ? t : 255.f) : 0.f;
    return (unsigned char)(int)t;   /* t >= 0: the conversion truncates = floor */
}

/* the bytes of pixel (x, y) (top-down) and where they go */
VCM_HD void disp_encode_pixel(F4 v, int x, int y, int resX, int resY, int format, int dither, unsigned seed, unsigned char *out)
{
    const long long p = (long long)y * resX + x;
    const unsigned char r = disp_byte(v.x, dither, p, 0, seed), g = disp_byte(v.y, dither, p, 1, seed), b = disp_byte(v.z, dither, p, 2, seed);
    if (format == VCM_IMAGE_BGR8) {   /* bottom-up, B G R: vcm_read_image's layout */
        unsigned char *o = out + ((size_t)(resY - 1 - y) * resX + x) * 3;
        o[0] = b; o[1] = g; o[2] = r;
    } else {                          /* VCM_IMAGE_RGBA8: top-down */
        unsigned char *o = out + (size_t)p * 4;
        o[0] = r; o[1] = g; o[2] = b; o[3] = 255;
    }
}

/* ---------------- launches (vcm_display.hip; the C-ABI of vcm_api.hip calls them) ---------------- */
/* floats of bloom scratch for a width x height image and `levels` levels: the G chain and two level-1 images (D, T) */
inline size_t disp_bloom_scratch_f4(int width, int height, int levels)
{
    size_t total = 0;
    int w = width, h = height;
    for (int l = 1; l <= levels; l++) { w = disp_level_dim(w); h = disp_level_dim(h); total += (size_t)w * h; }
    return total + 2 * (size_t)disp_level_dim(width) * disp_level_dim(height);
}

#if defined(__HIPCC__)
int disp_max_blocks();
void disp_set_max_blocks(int blocks);
/* counters (VCM_DISP_COUNTERS words, zeroed by the caller) += the histogram of the n pixels of src * scale */
hipError_t disp_launch_histogram(long long n, const float *src, int channels, float scale, unsigned long long *counters, hipStream_t stream);
/* out = steps 1-4 of src * scale with the multiplier mult; counters[VCM_DISP_CLIPPED] += the clipped channels; scratch:
   disp_bloom_scratch_f4() float4 when p.bloomStrength > 0, else unused */
hipError_t disp_launch_transform(int width, int height, const float *src, int channels, float scale, float mult, const vcm_display_params &p,
                                 F4 *scratch, F4 *out, unsigned long long *counters, hipStream_t stream);
/* bytes of the float4 image (VCM_IMAGE_BGR8 / VCM_IMAGE_RGBA8) */
hipError_t disp_launch_encode(int width, int height, const F4 *img, int format, int dither, unsigned seed, unsigned char *out, hipStream_t stream);
#endif

} // namespace vcm
#endif
