// vcm_denoise.h -- first-hit feature buffers and the edge-avoiding a-trous filter (Dammertz et al. 2010), host+device:
// the kernels of vcm_denoise.hip and the host emulation of the tests (tests/host_emul_denoise) run THESE functions, so
// that a host build and a device build give the same bits.  Arithmetic: + - * /, comparisons and detmath.h's dm_powf,
// compiled with -ffp-contract=off like the rest of vcm_core.h.
//
//   guide   float4 { isect.normal.xyz, distance along the ray }   (0, 0, 0, 0) on a miss: no hit has distance 0
//   albedo  float4 { clamp(diffuse + phong + mirror, 0, 1), 1 }   (1, 1, 1) for glass, emitters and misses; a 0 becomes 1
#ifndef SMALLVCM_AMD_VCM_DENOISE_H
#define SMALLVCM_AMD_VCM_DENOISE_H

#include "vcm_core.h"
#include "scene_kind.h"

namespace vcm {

#define VCM_DN_MAX_PASSES 12
/* vcm_denoise_defaults: the set with the lowest mean relative MSE of the sweep in DESIGN.md "Denoising" */
#define VCM_DN_DEFAULT_SIGMA_COLOR 16.0f
#define VCM_DN_DEFAULT_SIGMA_NORMAL 32.0f
#define VCM_DN_DEFAULT_SIGMA_DEPTH 0.05f

/* ---------------- features ---------------- */
VCM_HD float dn_albedo_component(float a)
{
    a = smin(smax(a, 0.f), 1.f);
    return (a == 0.f) ? 1.f : a;   /* demodulation never divides by 0 */
}

/* One ray through the CENTRE of pixel `pixel` from the pinhole (a thin lens is ignored: guides stay sharp), the scene
 * kind's own closest-hit routine.  A fisheye or panorama context sends the ray through its projection instead. */
template <class SC>
VCM_HD void feature_pixel(const SC &sc, int resX, int pixel, F4 &guide, F4 &albedo)
{
    const vcm_camera &cam = sc.camera;
    const float sx = float(pixel % resX) + 0.5f, sy = float(pixel / resX) + 0.5f;
    Ray ray;
    const V3 worldRaster = transform_point(cam.rasterToWorld, mk3(sx, sy, 0.f));   /* camera.hxx:108-117 */
    ray.org = ld3(cam.position);
    ray.dir = normalize(worldRaster - ray.org);
    ray.tmin = 0;
    Isect isect; isect.dist = 1e36f; isect.matID = 0; isect.lightID = -1; isect.normal = sp3(0.f); isect.prim = -1;
    guide = mk4(0.f, 0.f, 0.f, 0.f);
    albedo = mk4(1.f, 1.f, 1.f, 1.f);
    if (VCM_PROJ_ON(SC, sc)) {   /* a fisheye or a panorama (the WithLens forms): the guides line up with the image; a pixel
                                   centre outside the fisheye's circle reads as a miss */
        float cameraPdfW;
        if (!proj_raster_to_dir(sc, sx, sy, ray.dir, cameraPdfW)) return;
    }
    if (!scene_intersect(sc, ray, isect)) return;
    guide = mk4(isect.normal.x, isect.normal.y, isect.normal.z, isect.dist);
    if (isect.lightID >= 0) return;   /* an emitter */
    const vcm_material m = scene_material(sc, isect.matID);
    if (m.ior > 0.f) return;          /* refracts: what is seen lies behind it */
    V3 a = ld3(m.diffuse) + ld3(m.phong) + ld3(m.mirror);
    if (VCM_GGX_ON(SC, sc)) a = a + ld3(scene_material_ext(sc, isect.matID).ggx);   /* the lobe's F0 */
    albedo = mk4(dn_albedo_component(a.x), dn_albedo_component(a.y), dn_albedo_component(a.z), 1.f);
}

/* ---------------- the filter ---------------- */
VCM_HD bool dn_finite(float x) { return (f2u(x) & 0x7f800000u) != 0x7f800000u; }
VCM_HD bool dn_finite3(F4 c) { return dn_finite(c.x) && dn_finite(c.y) && dn_finite(c.z); }

/* what one pass needs; dn_pass() derives it from the caller's parameters on the host (the same code in the library
   and in the emulation) */
struct DnPass {
    int resX, resY, step;
    float invSigmaColorSqr;   /* 1 / (sigmaColor 2^-pass)^2: sigmaColor halves after every pass */
    float sigmaNormal, sigmaDepth;
    int remodulate;           /* the last pass of a demodulated run multiplies the albedo back */
};

/* NULL, or why the parameters are refused */
inline const char *dn_check_params(const vcm_denoise_params *p)
{
    if (!p) return "params is NULL";
    if (p->passes < 0 || p->passes > VCM_DN_MAX_PASSES) return "passes must be in [0, 12]";
    const float s[3] = { p->sigmaColor, p->sigmaNormal, p->sigmaDepth };
    for (int k = 0; k < 3; k++)
        if (!dn_finite(s[k]) || !(s[k] > 0.f)) return "sigmaColor, sigmaNormal and sigmaDepth must be finite and positive";
    return NULL;
}
inline DnPass dn_pass(const vcm_denoise_params &p, int resX, int resY, int pass)
{
    DnPass P;
    P.resX = resX; P.resY = resY; P.step = 1 << pass;
    float sc = p.sigmaColor;
    for (int i = 0; i < pass; i++) sc = sc * 0.5f;
    P.invSigmaColorSqr = 1.f / (sc * sc);
    P.sigmaNormal = p.sigmaNormal; P.sigmaDepth = p.sigmaDepth;
    P.remodulate = (p.demodulate && pass == p.passes - 1) ? 1 : 0;
    return P;
}

/* the B3-spline weights 1/16, 1/4, 3/8, 1/4, 1/16 */
VCM_HD float dn_b3(int i) { return (i == 2) ? 0.375f : ((i == 1 || i == 3) ? 0.25f : 0.0625f); }

/* colour * scale, divided by the albedo where the run demodulates: what the first pass reads */
VCM_HD F4 dn_prepare(float r, float g, float b, float scale, F4 albedo, int demodulate)
{
    r = r * scale; g = g * scale; b = b * scale;
    if (demodulate) { r = r / albedo.x; g = g / albedo.y; b = b / albedo.z; }
    return mk4(r, g, b, 1.f);
}

struct DnAcc { float r, g, b, w; };

/* One tap q seen from the centre p.  weight = h w_n w_z w_c with
 *   w_n = max(0, n_p . n_q)^sigmaNormal                       (dm_powf: the binary exponentiation for an integer sigma)
 *   w_z = f((|z_p - z_q| / (sigmaDepth max(z_p, z_q)))^2)
 *   w_c = f(|c_p - c_q|^2 / sigmaColor_pass^2)                f(x) = 1 / (1 + x / 4)^4, the rational stand-in of exp(-x)
 * A miss matches only misses (and then on colour alone), a non-finite tap or weight counts 0.  The sum runs over the
 * DIFFERENCES c_q - c_p: a tap of the centre's colour adds an exact 0, so a constant region stays what it is, bit for
 * bit, and an edge whose weights are 0 stays two constants. */
VCM_HD void dn_tap(DnAcc &a, const DnPass &P, F4 cp, F4 gp, F4 cq, F4 gq, float h)
{
    if (!dn_finite3(cq)) return;
    const bool missP = gp.w == 0.f, missQ = gq.w == 0.f;
    if (missP != missQ) return;
    float w = h, az = 1.f;
    if (!missP) {
        const float d = dot(mk3(gp.x, gp.y, gp.z), mk3(gq.x, gq.y, gq.z));
        if (!(d > 0.f)) return;
        w = w * dm_powf(d, P.sigmaNormal);
        const float t = fabsf(gp.w - gq.w) / (P.sigmaDepth * smax(gp.w, gq.w));
        az = 1.f + 0.25f * (t * t);
    }
    const float dr = cq.x - cp.x, dg = cq.y - cp.y, db = cq.z - cp.z;
    const float dist2 = (dr * dr + dg * dg) + db * db;
    const float ac = 1.f + 0.25f * (dist2 * P.invSigmaColorSqr);
    const float t1 = ac * az, t2 = t1 * t1, t4 = t2 * t2;
    w = w / t4;
    if (!(w > 0.f) || !dn_finite(w)) return;
    a.r = a.r + w * dr; a.g = a.g + w * dg; a.b = a.b + w * db; a.w = a.w + w;
}

/* the filtered pixel (x, y): load(xq, yq, cq, gq) fetches a tap's colour and guide, rows first, columns inside */
template <class Load>
VCM_HD F4 dn_filter_pixel(const DnPass &P, int x, int y, F4 albedoP, Load &&load)
{
    F4 cp, gp;
    load(x, y, cp, gp);
    if (!dn_finite3(cp)) return mk4(cp.x, cp.y, cp.z, 1.f);   /* a non-finite centre passes through */
    DnAcc a; a.r = a.g = a.b = a.w = 0.f;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int j = 0; j < 5; j++) {
        const int yq = y + (j - 2) * P.step;
        if (yq < 0 || yq >= P.resY) continue;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (int i = 0; i < 5; i++) {
            const int xq = x + (i - 2) * P.step;
            if (xq < 0 || xq >= P.resX) continue;
            F4 cq, gq;
            load(xq, yq, cq, gq);
            dn_tap(a, P, cp, gp, cq, gq, dn_b3(j) * dn_b3(i));
        }
    }
    F4 o = mk4(cp.x, cp.y, cp.z, 1.f);
    if (a.w > 0.f) { o.x = cp.x + a.r / a.w; o.y = cp.y + a.g / a.w; o.z = cp.z + a.b / a.w; }
    if (P.remodulate) { o.x = o.x * albedoP.x; o.y = o.y * albedoP.y; o.z = o.z * albedoP.z; }
    return o;
}

/* ---------------- the variance-guided filter (vcm_denoise2) ----------------
 * The colour image's .w, which dn_prepare sets to 1 and no tap of the filter above reads, carries the total variance of
 * the colour the passes see: a tap stays one 16-byte colour load and one guide load.  The colour stop of a tap becomes
 *   x_c = |c_p - c_q|^2 / (sigmaVariance^2 v~_p + eps)
 * with v~_p the 3 x 3 Gaussian (1/4, 1/8, 1/16) of .w around the centre at unit spacing in every pass (taps outside the
 * image skipped, the rest renormalised); sigmaColor and its halving per pass play no part.  eps = 1e-10 is the square of
 * 1e-5, about the rounding error of a colour near 1: a region without variance then treats any visible difference as an
 * edge (x_c > 1e10 d^2, weight 0) while equal colours still divide 0 by eps and not by 0 -- every tap adds an exact 0 and
 * the region comes back bit for bit.  The variance travels with the colour:
 *   .w_out = sum w_q^2 .w_q / (sum w_q)^2   over the taps that counted, the centre included
 * (the variance of the weighted mean of independent taps).  A non-finite v~_p falls back to the fixed stop of the pass for
 * that pixel; a tap whose .w is not finite counts like a non-finite colour. */
#define VCM_DN_VAR_EPS 1e-10f
/* vcm_denoise_defaults2: DESIGN.md "Variance", the sweep of tests/variance_tune.py */
#define VCM_DN_DEFAULT_SIGMA_VARIANCE 4.0f
#define VCM_DN_DEFAULT_VARIANCE_GUIDED 1

struct DnPass2 {
    DnPass p;
    float sigmaVarSqr;   /* sigmaVariance^2 */
};

inline vcm_denoise_params dn_base_params(const vcm_denoise_params2 &q)
{
    vcm_denoise_params p;
    p.passes = q.passes; p.sigmaColor = q.sigmaColor; p.sigmaNormal = q.sigmaNormal; p.sigmaDepth = q.sigmaDepth; p.demodulate = q.demodulate;
    return p;
}
inline const char *dn_check_params2(const vcm_denoise_params2 *q)
{
    if (!q) return "params is NULL";
    const vcm_denoise_params p = dn_base_params(*q);
    if (const char *why = dn_check_params(&p)) return why;
    if (q->varianceGuided != 0 && q->varianceGuided != 1) return "varianceGuided must be 0 or 1";
    if (!dn_finite(q->sigmaVariance) || !(q->sigmaVariance > 0.f)) return "sigmaVariance must be finite and positive";
    return NULL;
}
inline DnPass2 dn_pass2(const vcm_denoise_params2 &q, int resX, int resY, int pass)
{
    DnPass2 P;
    P.p = dn_pass(dn_base_params(q), resX, resY, pass);
    P.sigmaVarSqr = q.sigmaVariance * q.sigmaVariance;
    return P;
}

/* dn_prepare, and .w = sum_c M2_c varFactor (/ albedo_c^2 where the run demodulates): the total variance of that colour */
VCM_HD F4 dn_prepare2(float r, float g, float b, float scale, F4 albedo, int demodulate, F4 mom, float varFactor)
{
    F4 o = dn_prepare(r, g, b, scale, albedo, demodulate);
    float vr = mom.x * varFactor, vg = mom.y * varFactor, vb = mom.z * varFactor;
    if (demodulate) { vr = vr / (albedo.x * albedo.x); vg = vg / (albedo.y * albedo.y); vb = vb / (albedo.z * albedo.z); }
    o.w = (vr + vg) + vb;
    return o;
}

VCM_HD float dn_gauss3(int i) { return (i == 1) ? 0.5f : 0.25f; }   /* products: 1/4, 1/8, 1/16 */

/* v~_p: load(xq, yq, cq, gq) as in dn_filter_pixel */
template <class Load>
VCM_HD float dn_center_variance(const DnPass &P, int x, int y, Load &&load)
{
    float s = 0.f, n = 0.f;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int j = 0; j < 3; j++) {
        const int yq = y + j - 1;
        if (yq < 0 || yq >= P.resY) continue;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (int i = 0; i < 3; i++) {
            const int xq = x + i - 1;
            if (xq < 0 || xq >= P.resX) continue;
            F4 cq, gq;
            load(xq, yq, cq, gq);
            const float g = dn_gauss3(j) * dn_gauss3(i);
            s = s + g * cq.w;
            n = n + g;
        }
    }
    return s / n;
}

struct DnAcc2 { float r, g, b, w, v; };

/* dn_tap with the colour stop 1 / invStop given by the caller, and the tap's variance accumulated */
VCM_HD void dn_tap2(DnAcc2 &a, const DnPass &P, float invStop, F4 cp, F4 gp, F4 cq, F4 gq, float h)
{
    if (!dn_finite3(cq) || !dn_finite(cq.w)) return;
    const bool missP = gp.w == 0.f, missQ = gq.w == 0.f;
    if (missP != missQ) return;
    float w = h, az = 1.f;
    if (!missP) {
        const float d = dot(mk3(gp.x, gp.y, gp.z), mk3(gq.x, gq.y, gq.z));
        if (!(d > 0.f)) return;
        w = w * dm_powf(d, P.sigmaNormal);
        const float t = fabsf(gp.w - gq.w) / (P.sigmaDepth * smax(gp.w, gq.w));
        az = 1.f + 0.25f * (t * t);
    }
    const float dr = cq.x - cp.x, dg = cq.y - cp.y, db = cq.z - cp.z;
    const float dist2 = (dr * dr + dg * dg) + db * db;
    const float ac = 1.f + 0.25f * (dist2 * invStop);
    const float t1 = ac * az, t2 = t1 * t1, t4 = t2 * t2;
    w = w / t4;
    if (!(w > 0.f) || !dn_finite(w)) return;
    a.r = a.r + w * dr; a.g = a.g + w * dg; a.b = a.b + w * db; a.w = a.w + w;
    a.v = a.v + (w * w) * cq.w;
}

/* the guided pixel (x, y): colour in .xyz, its propagated variance in .w */
template <class Load>
VCM_HD F4 dn_filter_pixel2(const DnPass2 &P2, int x, int y, F4 albedoP, Load &&load)
{
    const DnPass &P = P2.p;
    F4 cp, gp;
    load(x, y, cp, gp);
    if (!dn_finite3(cp)) return cp;   /* a non-finite centre passes through, its variance with it */
    float invStop = P.invSigmaColorSqr;
    const float vt = dn_center_variance(P, x, y, load);
    if (dn_finite(vt)) invStop = 1.f / (P2.sigmaVarSqr * smax(vt, 0.f) + VCM_DN_VAR_EPS);
    DnAcc2 a; a.r = a.g = a.b = a.w = a.v = 0.f;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int j = 0; j < 5; j++) {
        const int yq = y + (j - 2) * P.step;
        if (yq < 0 || yq >= P.resY) continue;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (int i = 0; i < 5; i++) {
            const int xq = x + (i - 2) * P.step;
            if (xq < 0 || xq >= P.resX) continue;
            F4 cq, gq;
            load(xq, yq, cq, gq);
            dn_tap2(a, P, invStop, cp, gp, cq, gq, dn_b3(j) * dn_b3(i));
        }
    }
    F4 o = cp;
    if (a.w > 0.f) { o.x = cp.x + a.r / a.w; o.y = cp.y + a.g / a.w; o.z = cp.z + a.b / a.w; o.w = a.v / (a.w * a.w); }
    if (P.remodulate) { o.x = o.x * albedoP.x; o.y = o.y * albedoP.y; o.z = o.z * albedoP.z; }
    return o;
}

/* ---------------- launches (vcm_denoise.hip; the C-ABI of vcm_api.hip calls them) ---------------- */
#if defined(__HIPCC__)
/* guide / albedo of the pixels [p0, p0 + nLocal), by the k_features of the context's kind (proj: its WithLens form) */
hipError_t dn_launch_features(const DScene *dScene, SceneKind kind, bool ggx, bool proj, int resX, int p0, int nLocal, F4 *guide, F4 *albedo,
                              hipStream_t stream);
/* out = the filtered colour.  fb3 != NULL: the colour is a W*H*3 float image times `scale`, else the float4 image
   `color`.  tmpA, tmpB: two W*H float4 images of scratch (unused when passes == 0).  Parameters already checked. */
/* dst[p * nComp + k] = component comp0 + k of src[p] */
hipError_t dn_launch_unpack(int n, const F4 *src, int comp0, int nComp, float *dst, hipStream_t stream);
hipError_t dn_launch_denoise(int resX, int resY, const F4 *color, const float *fb3, float scale, const F4 *albedo,
                             const F4 *guide, F4 *out, F4 *tmpA, F4 *tmpB, const vcm_denoise_params &p, hipStream_t stream);
/* the same with vcm_denoise_params2: varianceGuided == 0 IS dn_launch_denoise; else mom = the moments image and the
   variance of a colour channel is M2 * varFactor.  tmpA, tmpB as above. */
hipError_t dn_launch_denoise2(int resX, int resY, const F4 *color, const float *fb3, float scale, const F4 *albedo,
                              const F4 *guide, const F4 *mom, float varFactor, F4 *out, F4 *tmpA, F4 *tmpB,
                              const vcm_denoise_params2 &p, hipStream_t stream);
#endif

} // namespace vcm
#endif
