// scene_host.h -- host side of the scene: copies a C-ABI scene description (vcm_scene_desc: the reference's built-in
// boxes, fixed capacities; vcm_scene_desc2: any counts) into owned arrays and builds what the intersection code walks:
//   * <= VCM_MAX_PRIMS primitives: GeometryList order, consecutive triangles packed in pairs (vcm_core.h TriPair) --
//     the brute-force loop of Scene::Intersect (scene.hxx:53-70), which is what the reference does for every scene;
//   * more (or SMALLVCM_AMD_FORCE_BVH=1): a binary BVH over the primitives' boxes, SAH-binned over the three axes, at most 2 primitives per
//     leaf, nodes in depth-first order with escape indices (stackless traversal, vcm_core.h bvh_intersect).  The
//     reference has no acceleration structure (README:208-209); results are the same because the traversal only decides
//     WHICH primitives are tested, never how (vcm_core.h explains the tie rule).
// Host only (std::vector); vcm_api.hip uploads the arrays and hands the kernels a DScene of device pointers,
// tests/host_emul walks the same structure on the CPU.
#ifndef SMALLVCM_AMD_SCENE_HOST_H
#define SMALLVCM_AMD_SCENE_HOST_H

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <queue>
#include <string>
#include <utility>
#include <vector>

#include "vcm_core.h"

namespace vcm {

struct SceneHost {
    std::vector<vcm_prim> prims;
    std::vector<vcm_material> materials;
    std::vector<int> mat2light;
    std::vector<vcm_light> lights;
    int backgroundLight;
    float sceneCenter[3], sceneRadius, invSceneRadiusSqr;
    vcm_camera camera;
    std::vector<PrimOp> ops;
    std::vector<TriPair> pairs;
    std::vector<FastPair> fastPairs;      /* the filter's view of the list (vcm_core.h): triangles two by two, */
    std::vector<FastSphere> fastSpheres;  /* and the spheres */
    std::vector<FastRect> fastRects;      /* the same pairs as axis-aligned rectangles, grouped by normal axis -- if ALL of them are */
    int nFastRects[3]; float fastGmax;
    float fastRw2, fastCenter[3], fastRadius;
    std::vector<BvhNode> nodes;
    std::vector<BvhWide> wide;            /* one per inner node: both children's boxes (the ordered traversals, vcm_core.h) */
    std::vector<int> leafPrims;
    std::vector<LeafPrim> leafData;       /* the leaves' primitives in leaf order (what the traversals read) */
    /* the environment map (scene_host_set_envmap; envW == 0: none) and its sampling tables, DScene::envW ... */
    int envW = 0, envH = 0, envGuideW = 0, envGuideH = 0;
    std::vector<F4> envTexels;
    std::vector<float> envMarg, envCond;
    std::vector<int> envMargGuide, envCondGuide;
    /* the thin lens (scene_host_set_lens; lensRadius == 0: the pinhole), DScene::lensRadius ... */
    float lensRadius = 0.f, lensFocus = 1.f, lensRight[3] = { 0.f, 0.f, 0.f }, lensUp[3] = { 0.f, 0.f, 0.f };
    /* the pixel filter (scene_host_set_filter; filterKind BOX: the reference's), DScene::filterKind ... */
    int filterKind = VCM_FILTER_BOX;
    float filterRadius = 0.f;
    /* the sampler (scene_host_set_sampler; PHILOX: the default), DScene::samplerKind */
    int sampler = VCM_SAMPLER_PHILOX;
    /* the GGX lobes (scene_host_set_material_ext): one entry per material when some material has a lobe, else empty,
       DScene::ggxOn */
    std::vector<vcm_material_ext> materialExt;
    /* the camera's projection (scene_host_set_projection; projKind PERSPECTIVE: the reference's pinhole), DScene::projKind ... */
    int projKind = VCM_PROJ_PERSPECTIVE;
    float projFovDegrees = 0.f, projK = 0.f, projThetaMax = 0.f;
    float projF[3] = { 0.f, 0.f, 0.f }, projEx[3] = { 0.f, 0.f, 0.f }, projEy[3] = { 0.f, 0.f, 0.f };
    /* how lights are chosen (scene_host_set_pick; pickMode UNIFORM: no tables), DScene::pickMode ...; pickWeights are
       the weights before the mix and pickQuanta the m_i of pmf[i] = m_i 2^-23 (for reports and tests) */
    int pickMode = VCM_LIGHT_PICK_UNIFORM, pickGuide = 0;
    std::vector<float> pickPmf, pickCdf;
    std::vector<int> pickGuideTable;
    std::vector<double> pickWeights;
    std::vector<int> pickQuanta;

    /* the view the device functions take, filled IN PLACE: the arrays are addressed relative to the DScene object
       itself (vcm_core.h), so `d` must stay where it is while it is in use (host emulation) */
    void view(DScene &d) const
    {
        fill_scalars(d);
        const char *base = reinterpret_cast<const char *>(&d);
        d.offPrims = (const char *)prims.data() - base; d.offMaterials = (const char *)materials.data() - base;
        d.offMat2light = (const char *)mat2light.data() - base; d.offLights = (const char *)lights.data() - base;
        d.offOps = (const char *)ops.data() - base; d.offPairs = (const char *)pairs.data() - base;
        d.offNodes = (const char *)nodes.data() - base; d.offLeafPrims = (const char *)leafPrims.data() - base;
        d.offFastPairs = (const char *)fastPairs.data() - base; d.offFastSpheres = (const char *)fastSpheres.data() - base;
        d.offWide = (const char *)wide.data() - base; d.offLeafData = (const char *)leafData.data() - base;
        d.offFastRects = (const char *)fastRects.data() - base;
        d.offEnvTexels = (const char *)envTexels.data() - base; d.offEnvMarg = (const char *)envMarg.data() - base;
        d.offEnvCond = (const char *)envCond.data() - base; d.offEnvMargGuide = (const char *)envMargGuide.data() - base;
        d.offEnvCondGuide = (const char *)envCondGuide.data() - base;
        d.offPickPmf = (const char *)pickPmf.data() - base; d.offPickCdf = (const char *)pickCdf.data() - base;
        d.offPickGuide = (const char *)pickGuideTable.data() - base;
        d.offMaterialExt = (const char *)materialExt.data() - base;
    }
    void fill_scalars(DScene &d) const
    {
        d.nPrims = (int)prims.size(); d.nMaterials = (int)materials.size(); d.nLights = (int)lights.size();
        d.backgroundLight = backgroundLight;
        for (int k = 0; k < 3; k++) d.sceneCenter[k] = sceneCenter[k];
        d.sceneRadius = sceneRadius; d.invSceneRadiusSqr = invSceneRadiusSqr;
        d.camera = camera;
        d.nOps = (int)ops.size(); d.nNodes = (int)nodes.size();
        d.fastRw2 = fastRw2; d.fastRadius = fastRadius;
        d.nFastPairs = (int)fastPairs.size(); d.nFastSpheres = (int)fastSpheres.size();
        d.fastOnePlane = 1;
        for (const FastPair &f : fastPairs) if (!(f.flags & 4)) d.fastOnePlane = 0;
        { const char *e = getenv("SMALLVCM_AMD_NO_ONEPLANE"); if (e && e[0] == '1') d.fastOnePlane = 0; }   /* measurement switch */
        for (int k = 0; k < 3; k++) d.fastCenter[k] = fastCenter[k];
        for (int k = 0; k < 3; k++) d.nFastRects[k] = nFastRects[k];
        d.fastGmax = fastGmax;
        d.envW = envW; d.envH = envH; d.envGuideW = envGuideW; d.envGuideH = envGuideH;
        d.lensRadius = lensRadius; d.lensFocus = lensFocus;
        for (int k = 0; k < 3; k++) { d.lensRight[k] = lensRight[k]; d.lensUp[k] = lensUp[k]; }
        d.pickMode = pickMode; d.pickGuide = pickGuide;
        d.filterKind = filterKind; d.filterRadius = filterRadius;
        d.samplerKind = sampler;
        d.ggxOn = materialExt.empty() ? 0 : 1; d.offMaterialExt = 0;
        d.projKind = projKind; d.projK = projK; d.projThetaMax = projThetaMax;
        for (int k = 0; k < 3; k++) { d.projF[k] = projF[k]; d.projEx[k] = projEx[k]; d.projEy[k] = projEy[k]; }
        { const char *e = getenv("SMALLVCM_AMD_NO_RECTS"); if (e && e[0] == '1') d.nFastRects[0] = d.nFastRects[1] = d.nFastRects[2] = 0; }   /* measurement switch */
    }
};

/* does the scene hold a light of the types only the WithLights kernels know (vcm_core.h)? */
inline bool scene_host_has_new_lights(const SceneHost &s)
{
    for (const vcm_light &l : s.lights) if (l.type == VCM_LIGHT_SPOT || l.type == VCM_LIGHT_SPHERE) return true;
    return false;
}

inline void scene_host_lights_need_table(SceneHost &s);   /* below, with the light-pick tables */

/* spot and sphere lights (include/smallvcm_amd.h has the fields); every other type value stays unchecked, as it was */
inline bool scene_host_check_lights(const SceneHost &s, std::string &err)
{
    for (size_t i = 0; i < s.lights.size(); i++) {
        const vcm_light &l = s.lights[i];
        if (l.type != VCM_LIGHT_SPOT && l.type != VCM_LIGHT_SPHERE) continue;
        const bool spot = l.type == VCM_LIGHT_SPOT;
        if ((int)i == s.backgroundLight) { err = spot ? "a spot light cannot be the backgroundLight" : "a sphere light cannot be the backgroundLight"; return false; }
        for (int k = 0; k < 3; k++)
            if (!std::isfinite(l.p0[k]) || !std::isfinite(l.intensity[k])) {
                err = spot ? "spot light: position and intensity must be finite" : "sphere light: centre and intensity must be finite"; return false;
            }
        if (spot) {
            for (int k = 0; k < 3; k++)
                if (!std::isfinite(l.frameX[k]) || !std::isfinite(l.frameY[k]) || !std::isfinite(l.frameZ[k]) || !std::isfinite(l.e1[k])) {
                    err = "spot light: direction and angles must be finite"; return false;
                }
            const float cosOuter = l.e1[0], cosInner = l.e1[1];
            if (!(cosOuter >= -1.f) || !(cosOuter < 1.f)) { err = "spot light: the outer half-angle must be > 0 and <= 180 degrees"; return false; }
            if (!(cosInner >= cosOuter) || !(cosInner <= 1.f)) { err = "spot light: the inner half-angle must be >= 0 and <= the outer one"; return false; }
            if (l.e1[2] < 0.f) { err = "spot light: the falloff scale e1[2] must be >= 0"; return false; }
            if (!std::isfinite(l.scale) || !(l.scale > 0.f)) { err = "spot light: the cone pdf must be finite and > 0"; return false; }
        } else {
            const float r = l.e1[0];
            if (!std::isfinite(r) || !(r > 0.f)) { err = "sphere light: radius must be finite and > 0"; return false; }
            if (!std::isfinite(l.invArea) || !(l.invArea > 0.f)) { err = "sphere light: invArea must be finite and > 0"; return false; }
            int owner = -1, count = 0;
            for (size_t p = 0; p < s.prims.size(); p++)
                if (s.mat2light[(size_t)s.prims[p].matID] == (int)i) { owner = (int)p; count++; }
            if (count != 1) { err = "sphere light: exactly one primitive must carry a material mapped to it"; return false; }
            const vcm_prim &pr = s.prims[(size_t)owner];
            if (pr.type != VCM_PRIM_SPHERE || pr.p0[0] != l.p0[0] || pr.p0[1] != l.p0[1] || pr.p0[2] != l.p0[2] || pr.p1[0] != r) {
                err = "sphere light: its primitive must be a VCM_PRIM_SPHERE of the same centre and radius"; return false;
            }
        }
    }
    return true;
}

inline bool scene_host_check(const SceneHost &s, std::string &err)
{
    if (s.lights.empty()) { err = "scene has no light"; return false; }
    if (s.materials.empty()) { err = "scene has no material"; return false; }
    if (s.materials.size() >= (1u << 24)) { err = "more than 2^24 materials"; return false; }
    for (const vcm_prim &p : s.prims)
        if (p.matID < 0 || p.matID >= (int)s.materials.size()) { err = "primitive with a material index out of range"; return false; }
    for (int l : s.mat2light)
        if (l >= (int)s.lights.size()) { err = "mat2light entry out of range"; return false; }
    if (s.backgroundLight >= (int)s.lights.size()) { err = "backgroundLight out of range"; return false; }
    return scene_host_check_lights(s, err);
}

/* an env-map light comes with its image (scene_host_set_envmap): vcm_scene_desc / vcm_scene_desc2 cannot carry one */
inline bool scene_host_no_envmap(const SceneHost &s, std::string &err)
{
    for (const vcm_light &l : s.lights)
        if (l.type == VCM_LIGHT_ENVMAP) { err = "an env-map light needs its image: vcm_scene_desc3 / vcm_create3"; return false; }
    return true;
}

inline bool scene_host_from_desc(const vcm_scene_desc &sc, SceneHost &s, std::string &err)
{
    if (sc.nPrims < 0 || sc.nPrims > VCM_MAX_PRIMS || sc.nMaterials < 0 || sc.nMaterials > VCM_MAX_MATERIALS || sc.nLights < 1 ||
        sc.nLights > VCM_MAX_LIGHTS) { err = "scene exceeds the fixed capacities of vcm_scene_desc (use vcm_scene_desc2)"; return false; }
    s.prims.assign(sc.prims, sc.prims + sc.nPrims);
    s.materials.assign(sc.materials, sc.materials + sc.nMaterials);
    s.mat2light.assign(sc.mat2light, sc.mat2light + sc.nMaterials);
    s.lights.assign(sc.lights, sc.lights + sc.nLights);
    s.backgroundLight = sc.backgroundLight;
    for (int k = 0; k < 3; k++) s.sceneCenter[k] = sc.sceneCenter[k];
    s.sceneRadius = sc.sceneRadius; s.invSceneRadiusSqr = sc.invSceneRadiusSqr;
    s.camera = sc.camera;
    if (!(scene_host_check(s, err) && scene_host_no_envmap(s, err))) return false;
    scene_host_lights_need_table(s);
    return true;
}

inline bool scene_host_copy_desc2(const vcm_scene_desc2 &sc, SceneHost &s, std::string &err)
{
    if (sc.nPrims < 0 || sc.nMaterials < 1 || sc.nLights < 1 || (sc.nPrims > 0 && !sc.prims) || !sc.materials || !sc.mat2light || !sc.lights) {
        err = "vcm_scene_desc2: bad counts or NULL arrays"; return false;
    }
    s.prims.assign(sc.prims, sc.prims + sc.nPrims);
    s.materials.assign(sc.materials, sc.materials + sc.nMaterials);
    s.mat2light.assign(sc.mat2light, sc.mat2light + sc.nMaterials);
    s.lights.assign(sc.lights, sc.lights + sc.nLights);
    s.backgroundLight = sc.backgroundLight;
    for (int k = 0; k < 3; k++) s.sceneCenter[k] = sc.sceneCenter[k];
    s.sceneRadius = sc.sceneRadius; s.invSceneRadiusSqr = sc.invSceneRadiusSqr;
    s.camera = sc.camera;
    return scene_host_check(s, err);
}
inline bool scene_host_from_desc2(const vcm_scene_desc2 &sc, SceneHost &s, std::string &err)
{
    if (!(scene_host_copy_desc2(sc, s, err) && scene_host_no_envmap(s, err))) return false;
    scene_host_lights_need_table(s);
    return true;
}

/* ---- the environment map's tables (vcm_core.h env_search / env_sample_dir / env_eval) ----
 * In binary64, stored as binary32: texel = {rgb * scale, pdf_uv / (2 pi^2)} with pdf_uv = W H x the probability the two
 * float CDFs actually give the texel (so the pdf is that of the sampler, not of the weights before rounding); CDFs start
 * at 0 and end at exactly 1; a row of zero weight gets a uniform conditional CDF (it is never drawn).  The guide of a
 * CDF of n entries has G + 1 entries, G = the power of two >= n: guide[k] = the largest r < n with cdf[r] <= k / G. */
inline int scene_host_env_guide_size(int n) { int g = 1; while (g < n) g <<= 1; return g; }
inline void scene_host_env_guide(const float *cdf, int n, int G, int *guide)
{
    int r = 0;
    for (int k = 0; k < G; k++) {
        const float x = (float)k / (float)G;
        while (r + 1 < n && cdf[r + 1] <= x) r++;
        guide[k] = r;
    }
    guide[G] = n - 1;
}
inline bool scene_host_set_envmap(SceneHost &s, const vcm_envmap *m, std::string &err)
{
    int envLight = -1, nBackground = 0;
    for (size_t i = 0; i < s.lights.size(); i++) {
        if (s.lights[i].type == VCM_LIGHT_ENVMAP) { if (envLight >= 0) { err = "more than one env-map light"; return false; } envLight = (int)i; }
        if (s.lights[i].type == VCM_LIGHT_ENVMAP || s.lights[i].type == VCM_LIGHT_BACKGROUND) nBackground++;
    }
    if (!m && envLight < 0) return true;   /* a version-3 description without a map: the version-2 scene */
    if (!m) { err = "an env-map light without a map (vcm_scene_desc3::envmap is NULL)"; return false; }
    if (envLight < 0) { err = "a map without an env-map light (vcm_make_envmap_light)"; return false; }
    if (envLight != s.backgroundLight) { err = "the env-map light must be the scene's backgroundLight"; return false; }
    if (nBackground > 1) { err = "a scene has at most one background or env-map light"; return false; }
    const int W = m->width, H = m->height;
    if (W < 1 || W > 8192 || H < 1 || H > 4096) { err = "env map size outside 1..8192 x 1..4096"; return false; }
    if (!m->rgb) { err = "env map without texels"; return false; }
    const float scale = s.lights[envLight].scale;
    if (!std::isfinite(scale) || !(scale > 0.f)) { err = "env-map light scale must be finite and > 0"; return false; }
    const size_t n = (size_t)W * H;
    std::vector<double> rowSum((size_t)H, 0.0), w(n);
    double total = 0.0;
    for (int i = 0; i < H; i++) {
        const double st = std::sin(3.14159265358979323846 * (i + 0.5) / H);
        for (int j = 0; j < W; j++) {
            const float *t = m->rgb + ((size_t)i * W + j) * 3;
            for (int c = 0; c < 3; c++)
                if (!std::isfinite(t[c]) || t[c] < 0.f) { err = "env map texel not finite or negative"; return false; }
            const double lum = 0.212671 * t[0] + 0.715160 * t[1] + 0.072169 * t[2];   /* Luminance, utils.hxx:36-41 */
            w[(size_t)i * W + j] = lum * st;
            rowSum[(size_t)i] += lum * st;
        }
        total += rowSum[(size_t)i];
    }
    if (!(total > 0.0) || !std::isfinite(total)) { err = "env map has zero total luminance"; return false; }
    s.envW = W; s.envH = H;
    s.envMarg.assign((size_t)H + 1, 0.f);
    s.envCond.assign((size_t)H * (W + 1), 0.f);
    double acc = 0.0;
    for (int i = 0; i < H; i++) {
        acc += rowSum[(size_t)i];
        s.envMarg[(size_t)i + 1] = i + 1 == H ? 1.f : (float)(acc / total);
        float *cond = &s.envCond[(size_t)i * (W + 1)];
        double a = 0.0;
        for (int j = 0; j < W; j++) {
            a += w[(size_t)i * W + j];
            cond[j + 1] = j + 1 == W ? 1.f : (rowSum[(size_t)i] > 0.0 ? (float)(a / rowSum[(size_t)i]) : (float)((double)(j + 1) / W));
        }
    }
    s.envTexels.resize(n);
    const double norm = (double)W * H / (2.0 * 3.14159265358979323846 * 3.14159265358979323846);
    for (int i = 0; i < H; i++) {
        const double pr = (double)s.envMarg[(size_t)i + 1] - s.envMarg[(size_t)i];
        const float *cond = &s.envCond[(size_t)i * (W + 1)];
        for (int j = 0; j < W; j++) {
            const float *t = m->rgb + ((size_t)i * W + j) * 3;
            const double p = pr * ((double)cond[j + 1] - cond[j]);
            s.envTexels[(size_t)i * W + j] = mk4(t[0] * scale, t[1] * scale, t[2] * scale, (float)(p * norm));
        }
    }
    s.envGuideH = scene_host_env_guide_size(H);
    s.envGuideW = scene_host_env_guide_size(W);
    s.envMargGuide.resize((size_t)s.envGuideH + 1);
    scene_host_env_guide(s.envMarg.data(), H, s.envGuideH, s.envMargGuide.data());
    s.envCondGuide.resize((size_t)H * (s.envGuideW + 1));
    for (int i = 0; i < H; i++)
        scene_host_env_guide(&s.envCond[(size_t)i * (W + 1)], W, s.envGuideW, &s.envCondGuide[(size_t)i * (s.envGuideW + 1)]);
    return true;
}

inline bool scene_host_from_desc3(const vcm_scene_desc3 &sc, SceneHost &s, std::string &err)
{
    if (!(scene_host_copy_desc2(sc.base, s, err) && scene_host_set_envmap(s, sc.envmap, err))) return false;
    scene_host_lights_need_table(s);
    return true;
}

/* ---- the thin lens (vcm_core.h lens_point / lens_ray / lens_project) ----
 * The disc's basis, in binary64 from the camera as stored: right = the world direction of raster +x (the difference of
 * rasterToWorld at raster (1, 0) and (0, 0)) made orthogonal to forward, up = forward x right. */
inline bool scene_host_set_lens(SceneHost &s, const vcm_thin_lens *lens, std::string &err)
{
    s.lensRadius = 0.f; s.lensFocus = 1.f;
    if (!lens) return true;
    const float R = lens->apertureRadius, F = lens->focusDistance;
    if (!std::isfinite(R) || R < 0.f) { err = "thin lens: apertureRadius must be finite and >= 0"; return false; }
    if (!std::isfinite(F) || !(F > 0.f)) { err = "thin lens: focusDistance must be finite and > 0"; return false; }
    if (R == 0.f) return true;   /* the pinhole */
    const float *m = s.camera.rasterToWorld;
    double a[3], b[3], f[3], r[3], u[3];
    for (int k = 0; k < 3; k++) {   /* transform_point at (0, 0, 0) and (1, 0, 0) */
        a[k] = (double)m[12 + k] / (double)m[15];
        b[k] = ((double)m[12 + k] + m[k]) / ((double)m[15] + m[3]);
        f[k] = s.camera.forward[k];
    }
    const double fl = std::sqrt(f[0] * f[0] + f[1] * f[1] + f[2] * f[2]);
    if (!(fl > 0.0) || !std::isfinite(fl)) { err = "thin lens: the camera has no forward direction"; return false; }
    for (int k = 0; k < 3; k++) { f[k] /= fl; r[k] = b[k] - a[k]; }
    const double rf = r[0] * f[0] + r[1] * f[1] + r[2] * f[2];
    for (int k = 0; k < 3; k++) r[k] -= rf * f[k];
    const double rl = std::sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
    if (!(rl > 0.0) || !std::isfinite(rl)) { err = "thin lens: the camera's raster axes are degenerate"; return false; }
    for (int k = 0; k < 3; k++) r[k] /= rl;
    u[0] = f[1] * r[2] - f[2] * r[1]; u[1] = f[2] * r[0] - f[0] * r[2]; u[2] = f[0] * r[1] - f[1] * r[0];
    s.lensRadius = R; s.lensFocus = F;
    for (int k = 0; k < 3; k++) { s.lensRight[k] = (float)r[k]; s.lensUp[k] = (float)u[k]; }
    return true;
}

inline bool scene_host_from_desc4(const vcm_scene_desc4 &sc, SceneHost &s, std::string &err)
{
    return scene_host_from_desc3(sc.base, s, err) && scene_host_set_lens(s, sc.lens, err);
}

/* ---- light selection (vcm_core.h pick_light / light_pick_prob) ----
 * POWER's weight of a light: the flux its Emit estimator integrates to, in binary64 (include/smallvcm_amd.h
 * vcm_light_pick has the table).  The environment map's is pi R^2 x the sum over the texels of lum(texel scale) x the
 * texel's solid angle (2 pi / W) (cos theta_top - cos theta_bottom); a constant map gives the background's value. */
inline double scene_host_light_power(const SceneHost &s, int i)
{
    const double PI = 3.14159265358979323846;
    const vcm_light &l = s.lights[(size_t)i];
    const double lum = 0.212671 * l.intensity[0] + 0.715160 * l.intensity[1] + 0.072169 * l.intensity[2];   /* utils.hxx:36-41 */
    const double R = s.sceneRadius;
    double w = 0.0;
    switch (l.type) {
    case VCM_LIGHT_AREA: w = l.invArea > 0.f ? PI * lum / (double)l.invArea : 0.0; break;
    case VCM_LIGHT_POINT: w = 4.0 * PI * lum; break;
    case VCM_LIGHT_SPOT: w = 2.0 * PI * lum * ((1.0 - (double)l.e1[1]) + ((double)l.e1[1] - (double)l.e1[0]) / 2.0); break;
    case VCM_LIGHT_SPHERE: w = l.invArea > 0.f ? PI * lum / (double)l.invArea : 0.0; break;
    case VCM_LIGHT_DIRECTIONAL: w = PI * R * R * lum; break;
    case VCM_LIGHT_BACKGROUND: w = 4.0 * PI * PI * R * R * lum * (double)l.scale; break;
    case VCM_LIGHT_ENVMAP: {
        double sum = 0.0;
        for (int r = 0; r < s.envH; r++) {
            const double omega = (2.0 * PI / s.envW) * (std::cos(PI * r / s.envH) - std::cos(PI * (r + 1) / s.envH));
            double row = 0.0;
            for (int c = 0; c < s.envW; c++) {
                const F4 &t = s.envTexels[(size_t)r * s.envW + c];   /* rgb * scale */
                row += 0.212671 * t.x + 0.715160 * t.y + 0.072169 * t.z;
            }
            sum += row * omega;
        }
        w = PI * R * R * sum;
    } break;
    default: break;
    }
    return (w > 0.0 && std::isfinite(w)) ? w : 0.0;
}

/* Largest-remainder apportionment of 2^23 quanta to the weights (>= 0, not all zero, at most 2^23 of them non-zero):
 * m_i = floor(w_i / sum w x 2^23), the quanta left over go to the largest remainders (ties: the lower index); then every
 * light of non-zero weight that got none takes one from the light that holds the most at that moment. */
inline void scene_host_apportion(const std::vector<double> &w, std::vector<int> &m)
{
    const long long Q = 1ll << 23;
    const size_t n = w.size();
    double total = 0.0;
    for (double x : w) total += x;
    m.assign(n, 0);
    std::vector<std::pair<double, size_t>> frac;
    long long used = 0;
    for (size_t i = 0; i < n; i++) {
        if (!(w[i] > 0.0)) continue;
        const double q = w[i] / total * (double)Q;
        long long f = (long long)std::floor(q);
        f = f > Q ? Q : f;
        m[i] = (int)f; used += f;
        frac.push_back(std::make_pair(q - (double)f, i));
    }
    std::stable_sort(frac.begin(), frac.end(), [](const std::pair<double, size_t> &a, const std::pair<double, size_t> &b) { return a.first > b.first; });
    for (size_t k = 0; used < Q; k = (k + 1) % frac.size()) { m[frac[k].second]++; used++; }
    std::priority_queue<std::pair<int, long long>> big;   /* (quanta, -index): the most quanta, then the lower index */
    long long need = 0;
    for (size_t i = 0; i < n; i++) {
        if (m[i] >= 2) big.push(std::make_pair(m[i], -(long long)i));
        if (w[i] > 0.0 && m[i] == 0) need++;
    }
    need += used - Q;   /* (rounding may have handed out a quantum too many: taken back the same way) */
    for (size_t i = 0; i < n; i++) if (w[i] > 0.0 && m[i] == 0) m[i] = 1;
    for (; need > 0; need--) {
        std::pair<int, long long> t = big.top(); big.pop();
        m[(size_t)-t.second]--; t.first--;
        if (t.first >= 2) big.push(t);
    }
}

/* the tables of the probabilities `mixed` (>= 0, sum 1) */
inline void scene_host_pick_tables(SceneHost &s, const std::vector<double> &mixed, int mode)
{
    const size_t n = s.lights.size();
    scene_host_apportion(mixed, s.pickQuanta);
    s.pickPmf.resize(n); s.pickCdf.resize(n + 1);
    long long acc = 0;
    s.pickCdf[0] = 0.f;
    for (size_t i = 0; i < n; i++) {   /* whole multiples of 2^-23 up to 1: exact in binary32 */
        s.pickPmf[i] = (float)s.pickQuanta[i] * 1.1920928955078125e-07f;
        acc += s.pickQuanta[i];
        s.pickCdf[i + 1] = (float)acc * 1.1920928955078125e-07f;
    }
    s.pickGuide = scene_host_env_guide_size((int)n);
    s.pickGuideTable.resize((size_t)s.pickGuide + 1);
    scene_host_env_guide(s.pickCdf.data(), (int)n, s.pickGuide, s.pickGuideTable.data());
    s.pickMode = mode;
}

/* A scene with a spot or a sphere light always has a table: the branches of those lights exist only in the kernels that
   wrap the table kinds (vcm_core.h WithLights).  Where the caller asked for the uniform choice the table says so: CUSTOM
   with one weight for every light, i.e. 2^23 / n quanta each, the remainder to the lowest indices. */
inline void scene_host_lights_need_table(SceneHost &s)
{
    if (s.pickMode != VCM_LIGHT_PICK_UNIFORM || !scene_host_has_new_lights(s)) return;
    const size_t n = s.lights.size();
    s.pickWeights.assign(n, 1.0);
    scene_host_pick_tables(s, std::vector<double>(n, 1.0 / (double)n), VCM_LIGHT_PICK_CUSTOM);
}

/* the tables the caller asked for (NULL or UNIFORM: none) */
inline bool scene_host_pick_as_asked(SceneHost &s, const vcm_light_pick *pick, std::string &err)
{
    s.pickMode = VCM_LIGHT_PICK_UNIFORM; s.pickGuide = 0;
    s.pickPmf.clear(); s.pickCdf.clear(); s.pickGuideTable.clear(); s.pickWeights.clear(); s.pickQuanta.clear();
    if (!pick) return true;
    if (pick->mode != VCM_LIGHT_PICK_UNIFORM && pick->mode != VCM_LIGHT_PICK_POWER && pick->mode != VCM_LIGHT_PICK_CUSTOM) {
        err = "light pick: mode must be VCM_LIGHT_PICK_UNIFORM, _POWER or _CUSTOM"; return false;
    }
    const float a = pick->uniformMix;
    if (!std::isfinite(a) || a < 0.f || a > 1.f) { err = "light pick: uniformMix must be finite and in [0, 1]"; return false; }
    if (pick->mode == VCM_LIGHT_PICK_UNIFORM) return true;
    const size_t n = s.lights.size();
    std::vector<double> w(n);
    for (size_t i = 0; i < n; i++) w[i] = scene_host_light_power(s, (int)i);
    if (pick->mode == VCM_LIGHT_PICK_CUSTOM) {
        if (!pick->weights) { err = "light pick: CUSTOM needs weights"; return false; }
        for (size_t i = 0; i < n; i++) {
            const float x = pick->weights[i];
            if (!std::isfinite(x) || x < 0.f) { err = "light pick: weights must be finite and >= 0"; return false; }
            if (x == 0.f && w[i] > 0.0) { err = "light pick: a zero weight on a light that is not black (light tracing would lose it)"; return false; }
            w[i] = x;
        }
    }
    double total = 0.0;
    size_t nz = 0;
    for (double x : w) { total += x; if (x > 0.0) nz++; }
    if (nz == 0 || !(total > 0.0) || !std::isfinite(total)) { err = "light pick: all weights are zero"; return false; }
    if (nz > ((size_t)1 << 23)) { err = "light pick: more than 2^23 lights with non-zero weight"; return false; }
    s.pickWeights = w;
    std::vector<double> mixed(n, 0.0);
    for (size_t i = 0; i < n; i++) if (w[i] > 0.0) mixed[i] = (1.0 - (double)a) * w[i] / total + (double)a / (double)nz;
    scene_host_pick_tables(s, mixed, pick->mode);
    return true;
}
inline bool scene_host_set_pick(SceneHost &s, const vcm_light_pick *pick, std::string &err)
{
    if (!scene_host_pick_as_asked(s, pick, err)) return false;
    scene_host_lights_need_table(s);
    return true;
}

inline bool scene_host_from_desc5(const vcm_scene_desc5 &sc, SceneHost &s, std::string &err)
{
    return scene_host_from_desc4(sc.base, s, err) && scene_host_set_pick(s, sc.pick, err);
}

/* ---- the pixel filter (vcm_core.h filter_offset) ---- */
inline bool scene_host_set_filter(SceneHost &s, const vcm_pixel_filter *filter, std::string &err)
{
    s.filterKind = VCM_FILTER_BOX; s.filterRadius = 0.f;
    if (!filter || filter->kind == VCM_FILTER_BOX) return true;
    if (filter->kind != VCM_FILTER_TENT && filter->kind != VCM_FILTER_BSPLINE) { err = "pixel filter: unknown kind"; return false; }
    const float r = filter->radius;
    if (!std::isfinite(r) || !(r > 0.f) || r > 16.f) { err = "pixel filter: radius must be finite, > 0 and <= 16 pixels"; return false; }
    s.filterKind = filter->kind; s.filterRadius = r;
    return true;
}

inline bool scene_host_from_desc6(const vcm_scene_desc6 &sc, SceneHost &s, std::string &err)
{
    return scene_host_from_desc5(sc.base, s, err) && scene_host_set_filter(s, sc.filter, err);
}

/* ---- the sampler (sobol.h) ---- */
inline bool scene_host_set_sampler(SceneHost &s, const vcm_sampler *sampler, std::string &err)
{
    s.sampler = VCM_SAMPLER_PHILOX;
    if (!sampler || sampler->kind == VCM_SAMPLER_PHILOX) return true;
    if (sampler->kind != VCM_SAMPLER_SOBOL) { err = "sampler: unknown kind"; return false; }
    s.sampler = VCM_SAMPLER_SOBOL;
    return true;
}

inline bool scene_host_from_desc7(const vcm_scene_desc7 &sc, SceneHost &s, std::string &err)
{
    return scene_host_from_desc6(sc.base, s, err) && scene_host_set_sampler(s, sc.sampler, err);
}

/* ---- the GGX lobes (vcm_core.h bsdf_eval_ggx) ---- */
inline bool scene_host_set_material_ext(SceneHost &s, const vcm_material_ext *ext, std::string &err)
{
    s.materialExt.clear();
    if (!ext) return true;
    bool any = false;
    for (size_t m = 0; m < s.materials.size(); m++) {
        const vcm_material_ext &x = ext[m];
        const std::string who = "materialExt[" + std::to_string(m) + "]: ";
        if (!std::isfinite(x.ggx[0]) || !std::isfinite(x.ggx[1]) || !std::isfinite(x.ggx[2]) || !std::isfinite(x.alpha)) { err = who + "a field is not finite"; return false; }
        for (int k = 0; k < 3; k++)
            if (x.ggx[k] < 0.f || x.ggx[k] > 1.f) { err = who + "ggx (F0) must lie in [0, 1]"; return false; }
        if (x.ggx[0] == 0.f && x.ggx[1] == 0.f && x.ggx[2] == 0.f) continue;
        if (x.alpha < 0.01f || x.alpha > 1.f) { err = who + "alpha must lie in [0.01, 1]"; return false; }
        if (s.mat2light[m] >= 0) { err = who + "a material that is a light cannot have a GGX lobe"; return false; }
        any = true;
    }
    if (any) s.materialExt.assign(ext, ext + s.materials.size());   /* else: the version-7 scene */
    return true;
}

inline bool scene_host_from_desc8(const vcm_scene_desc8 &sc, SceneHost &s, std::string &err)
{
    return scene_host_from_desc7(sc.base, s, err) && scene_host_set_material_ext(s, sc.materialExt, err);
}

/* ---- the camera's projection (vcm_core.h proj_raster_to_dir / proj_dir_to_raster) ----
 * The camera frame in binary64 from the camera as stored: f = forward, ex = the world direction of raster +x (the
 * difference of rasterToWorld at raster (1, 0) and (0, 0)) made orthogonal to f -- what lensRight is --, ey = +-(f x ex),
 * the sign that points along raster +y (rasterToWorld at (0, 1) minus at (0, 0)).  The fisheye's k = W / fov[rad] pixels
 * per radian and theta_max = fov / 2.  A thin lens is refused with either angular projection: its focus plane has no
 * meaning there. */
inline bool scene_host_set_projection(SceneHost &s, const vcm_camera_model *model, std::string &err)
{
    s.projKind = VCM_PROJ_PERSPECTIVE; s.projFovDegrees = 0.f; s.projK = 0.f; s.projThetaMax = 0.f;
    if (!model || model->kind == VCM_PROJ_PERSPECTIVE) return true;
    if (model->kind != VCM_PROJ_FISHEYE && model->kind != VCM_PROJ_PANORAMA) { err = "camera model: unknown projection kind"; return false; }
    const double PI = 3.14159265358979323846;
    const float fov = model->fovDegrees;
    if (model->kind == VCM_PROJ_FISHEYE && (!std::isfinite(fov) || !(fov > 0.f) || !(fov < 360.f))) {
        err = "camera model: a fisheye's fovDegrees must be finite and in (0, 360)"; return false;
    }
    if (s.lensRadius > 0.f) { err = "camera model: a thin lens combines with the perspective projection only"; return false; }
    const float *m = s.camera.rasterToWorld;
    double o[3], f[3], x[3], y[3], u[3];
    for (int k = 0; k < 3; k++) {   /* transform_point at (0, 0, 0), (1, 0, 0) and (0, 1, 0) */
        o[k] = (double)m[12 + k] / (double)m[15];
        x[k] = ((double)m[12 + k] + m[k]) / ((double)m[15] + m[3]) - o[k];
        y[k] = ((double)m[12 + k] + m[4 + k]) / ((double)m[15] + m[7]) - o[k];
        f[k] = s.camera.forward[k];
    }
    const double fl = std::sqrt(f[0] * f[0] + f[1] * f[1] + f[2] * f[2]);
    if (!(fl > 0.0) || !std::isfinite(fl)) { err = "camera model: the camera has no forward direction"; return false; }
    for (int k = 0; k < 3; k++) f[k] /= fl;
    const double xf = x[0] * f[0] + x[1] * f[1] + x[2] * f[2];
    for (int k = 0; k < 3; k++) x[k] -= xf * f[k];
    const double xl = std::sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2]);
    if (!(xl > 0.0) || !std::isfinite(xl)) { err = "camera model: the camera's raster axes are degenerate"; return false; }
    for (int k = 0; k < 3; k++) x[k] /= xl;
    u[0] = f[1] * x[2] - f[2] * x[1]; u[1] = f[2] * x[0] - f[0] * x[2]; u[2] = f[0] * x[1] - f[1] * x[0];
    const double uy = u[0] * y[0] + u[1] * y[1] + u[2] * y[2];
    if (!std::isfinite(uy) || uy == 0.0) { err = "camera model: the camera's raster axes are degenerate"; return false; }
    const double sign = uy < 0.0 ? -1.0 : 1.0;
    for (int k = 0; k < 3; k++) { s.projF[k] = (float)f[k]; s.projEx[k] = (float)x[k]; s.projEy[k] = (float)(sign * u[k]); }
    s.projKind = model->kind;
    if (model->kind == VCM_PROJ_FISHEYE) {
        const double rad = (double)fov * PI / 180.0;
        s.projFovDegrees = fov;
        s.projK = (float)((double)s.camera.resolution[0] / rad);
        s.projThetaMax = (float)(0.5 * rad);
    }
    return true;
}

inline bool scene_host_from_desc9(const vcm_scene_desc9 &sc, SceneHost &s, std::string &err)
{
    return scene_host_from_desc8(sc.base, s, err) && scene_host_set_projection(s, sc.model, err);
}

/* ---- brute-force list: consecutive triangles in pairs, fields interleaved (vcm_core.h TriPair) ---- */
inline void scene_host_build_pairs(SceneHost &s)
{
    s.ops.clear(); s.pairs.clear();
    const int n = (int)s.prims.size();
    for (int i = 0; i < n; ) {
        PrimOp op;
        if (s.prims[i].type != VCM_PRIM_TRIANGLE) { op.kind = 1; op.index = i; s.ops.push_back(op); i++; continue; }
        op.kind = 0; op.index = (int)s.pairs.size();
        s.ops.push_back(op);
        TriPair tp;
        std::memset(&tp, 0, sizeof(tp));
        const bool two = (i + 1 < n) && s.prims[i + 1].type == VCM_PRIM_TRIANGLE;
        for (int h = 0; h < 2; h++) {
            const vcm_prim &t = s.prims[(h == 1 && two) ? i + 1 : i];
            tp.p0x[h] = t.p0[0]; tp.p0y[h] = t.p0[1]; tp.p0z[h] = t.p0[2];
            tp.p1x[h] = t.p1[0]; tp.p1y[h] = t.p1[1]; tp.p1z[h] = t.p1[2];
            tp.p2x[h] = t.p2[0]; tp.p2y[h] = t.p2[1]; tp.p2z[h] = t.p2[2];
            tp.nx[h] = t.n[0]; tp.ny[h] = t.n[1]; tp.nz[h] = t.n[2];
            tp.matID[h] = t.matID;
            tp.prim[h] = (h == 1 && two) ? i + 1 : i;
        }
        tp.valid1 = two ? 1 : 0;
        s.pairs.push_back(tp);
        i += two ? 2 : 1;
    }
}

/* ---- the pairs as axis-aligned rectangles (vcm_core.h FastRect), if EVERY pair is one: the reference's own boxes ---- */
inline bool scene_host_rect_triangle(const vcm_prim &t, int k, const float *(&diag)[2], float c[2], float g[2])
{   /* the reference's edge functions (geometry.hxx:133-139): V(c, b), V(b, a), V(a, c); one must be the diagonal, one
       run along u = k+1 (constant v), one along v = k+2 (constant u) */
    const int u = (k + 1) % 3, v = (k + 2) % 3;
    const float *e[3][2] = { { t.p2, t.p1 }, { t.p1, t.p0 }, { t.p0, t.p2 } };
    bool haveU = false, haveV = false, haveD = false;
    for (int i = 0; i < 3; i++) {
        const float *P = e[i][0], *Q = e[i][1];
        const bool sameU = P[u] == Q[u], sameV = P[v] == Q[v];
        if (sameV && !sameU) { if (haveU) return false; haveU = true; c[0] = P[v]; g[0] = (float)((double)P[u] - (double)Q[u]); }        /* along u: V = d_k (P_u - Q_u)(c - X_v) */
        else if (sameU && !sameV) { if (haveV) return false; haveV = true; c[1] = P[u]; g[1] = (float)((double)Q[v] - (double)P[v]); }   /* along v: V = d_k (Q_v - P_v)(c - X_u) */
        else if (!sameU && !sameV) { if (haveD) return false; haveD = true; diag[0] = P; diag[1] = Q; }
        else return false;   /* a degenerate edge */
    }
    return haveU && haveV && haveD;
}
inline void scene_host_build_rects(SceneHost &s)
{
    s.fastRects.clear();
    s.nFastRects[0] = s.nFastRects[1] = s.nFastRects[2] = 0; s.fastGmax = 0.f;
    std::vector<FastRect> byAxis[3];
    for (const FastPair &f : s.fastPairs) {
        if ((f.flags & 7) != 7) return;   /* two triangles, shared diagonal, one plane */
        const vcm_prim &t = s.prims[(size_t)f.prim[0]], &w = s.prims[(size_t)f.prim[1]];
        int k = -1;
        for (int a = 0; a < 3; a++) if (std::fabs(t.n[a]) == 1.f && t.n[(a + 1) % 3] == 0.f && t.n[(a + 2) % 3] == 0.f) k = a;
        if (k < 0) return;
        const float *vs[6] = { t.p0, t.p1, t.p2, w.p0, w.p1, w.p2 };
        for (int i = 1; i < 6; i++) if (vs[i][k] != vs[0][k]) return;
        if (w.n[k] != t.n[k]) return;
        FastRect r;
        std::memset(&r, 0, sizeof(r));
        const float *da[2], *db[2];
        if (!scene_host_rect_triangle(t, k, da, r.c, r.g) || !scene_host_rect_triangle(w, k, db, r.c + 2, r.g + 2)) return;
        /* B's diagonal must be A's, reversed: then B's third edge function is exactly minus A's */
        bool rev = true;
        for (int a = 0; a < 3; a++) rev = rev && da[0][a] == db[1][a] && da[1][a] == db[0][a];
        if (!rev) return;
        {   /* V(P, Q) = Dot(dir, P x Q) + Dot(o x dir, Q - P), binary64, rounded once (as scene_host_build_fast) */
            const double p[3] = { da[0][0], da[0][1], da[0][2] }, q[3] = { da[1][0], da[1][1], da[1][2] };
            r.NEd[0] = (float)(p[1] * q[2] - p[2] * q[1]); r.NEd[1] = (float)(p[2] * q[0] - p[0] * q[2]); r.NEd[2] = (float)(p[0] * q[1] - p[1] * q[0]);
            for (int a = 0; a < 3; a++) r.NEd[3 + a] = (float)(q[a] - p[a]);
        }
        r.pk = t.p0[k]; r.nk = t.n[k];
        r.prim[0] = f.prim[0]; r.prim[1] = f.prim[1];
        for (int a = 0; a < 4; a++) s.fastGmax = std::max(s.fastGmax, std::fabs(r.g[a]) * 1.000001f);
        byAxis[k].push_back(r);
    }
    if (s.fastPairs.empty()) return;
    for (int k = 0; k < 3; k++) { s.nFastRects[k] = (int)byAxis[k].size(); s.fastRects.insert(s.fastRects.end(), byAxis[k].begin(), byAxis[k].end()); }
}

/* ---- the filter's view of the list (vcm_core.h "certified filters"): planes and Pluecker edge data, computed in
 *      binary64 and rounded once; the two triangles of a quad share their diagonal, which the second one reuses ---- */
inline void scene_host_build_fast(SceneHost &s)
{
    const int n = (int)s.prims.size();
    s.fastPairs.clear(); s.fastSpheres.clear();
    double lo[3] = { 1e300, 1e300, 1e300 }, hi[3] = { -1e300, -1e300, -1e300 }, rw2 = 0.0;
    auto edge = [](const float *P, const float *Q, float *NE) {   /* V(P, Q) = Dot(dir, P x Q) + Dot(o x dir, Q - P) */
        const double p[3] = { P[0], P[1], P[2] }, q[3] = { Q[0], Q[1], Q[2] };
        NE[0] = (float)(p[1] * q[2] - p[2] * q[1]); NE[1] = (float)(p[2] * q[0] - p[0] * q[2]); NE[2] = (float)(p[0] * q[1] - p[1] * q[0]);
        for (int k = 0; k < 3; k++) NE[3 + k] = (float)(q[k] - p[k]);
    };
    auto same = [](const float *a, const float *b) { return a[0] == b[0] && a[1] == b[1] && a[2] == b[2]; };
    for (int i = 0; i < n; ) {
        const vcm_prim &t = s.prims[i];
        if (t.type != VCM_PRIM_TRIANGLE) {
            FastSphere f;
            std::memset(&f, 0, sizeof(f));
            for (int k = 0; k < 3; k++) f.c[k] = t.p0[k];
            f.radius = t.p1[0]; f.prim = i;
            s.fastSpheres.push_back(f);
            i++;
            continue;
        }
        const bool two = (i + 1 < n) && s.prims[i + 1].type == VCM_PRIM_TRIANGLE;
        const vcm_prim &u = s.prims[two ? i + 1 : i];
        FastPair f;
        std::memset(&f, 0, sizeof(f));
        for (int k = 0; k < 3; k++) { f.p0[0][k] = t.p0[k]; f.n[0][k] = t.n[k]; f.p0[1][k] = u.p0[k]; f.n[1][k] = u.n[k]; }
        f.prim[0] = i; f.prim[1] = two ? i + 1 : i;
        f.flags = two ? 1 : 0;
        /* the reference's three edge functions (geometry.hxx:133-139): v0 = V(c, b), v1 = V(b, a), v2 = V(a, c);
           the sign test is symmetric in them, so each triangle may list them in any order */
        const float *te[3][2] = { { t.p2, t.p1 }, { t.p1, t.p0 }, { t.p0, t.p2 } };
        const float *ue[3][2] = { { u.p2, u.p1 }, { u.p1, u.p0 }, { u.p0, u.p2 } };
        int ta = 2, ub = 2;
        bool shared = false;
        if (two)
            for (int a = 0; a < 3 && !shared; a++)
                for (int b = 0; b < 3 && !shared; b++)
                    if (same(te[a][0], ue[b][1]) && same(te[a][1], ue[b][0])) { ta = a; ub = b; shared = true; }
        const int to[3] = { (ta + 1) % 3, (ta + 2) % 3, ta }, uo[3] = { (ub + 1) % 3, (ub + 2) % 3, ub };
        for (int k = 0; k < 3; k++) edge(te[to[k]][0], te[to[k]][1], f.NE[k]);
        edge(ue[uo[0]][0], ue[uo[0]][1], f.NE[3]);
        edge(ue[uo[1]][0], ue[uo[1]][1], f.NE[4]);
        edge(ue[uo[2]][0], ue[uo[2]][1], f.NE[5]);
        if (shared) f.flags |= 2;
        if (two) {   /* one plane part for both? (FastPair::flags bit 2) */
            bool same = true;
            for (int k = 0; k < 3; k++) same = same && (t.n[k] == u.n[k]) && (t.n[k] == 0.f || t.p0[k] == u.p0[k]);
            if (same) f.flags |= 4;
        }
        s.fastPairs.push_back(f);
        for (int w = 0; w < (two ? 2 : 1); w++) {
            const vcm_prim &q = s.prims[i + w];
            const float *vs[3] = { q.p0, q.p1, q.p2 };
            for (int v = 0; v < 3; v++) {
                double l2 = 0.0;
                for (int k = 0; k < 3; k++) { lo[k] = std::min(lo[k], (double)vs[v][k]); hi[k] = std::max(hi[k], (double)vs[v][k]); l2 += (double)vs[v][k] * vs[v][k]; }
                rw2 = std::max(rw2, l2);
            }
        }
        i += two ? 2 : 1;
    }
    double c[3] = { 0, 0, 0 }, r2 = 0.0;
    if (lo[0] <= hi[0]) for (int k = 0; k < 3; k++) c[k] = 0.5 * (lo[k] + hi[k]);
    for (int i = 0; i < n; i++) {
        const vcm_prim &t = s.prims[i];
        if (t.type != VCM_PRIM_TRIANGLE) continue;
        const float *vs[3] = { t.p0, t.p1, t.p2 };
        for (int v = 0; v < 3; v++) {
            double d2 = 0.0;
            for (int k = 0; k < 3; k++) d2 += (vs[v][k] - c[k]) * (vs[v][k] - c[k]);
            r2 = std::max(r2, d2);
        }
    }
    scene_host_build_rects(s);
    /* rounded up: they enter error BOUNDS */
    s.fastRw2 = (float)(rw2 * 1.0001) + 1e-30f;
    s.fastRadius = (float)(std::sqrt(r2) * 1.0001) + 1e-30f;
    for (int k = 0; k < 3; k++) s.fastCenter[k] = (float)c[k];
}

/* ---- BVH ---- */
/* primitives per leaf.  A wave pays for its slowest lane in both halves of the traversal, and with up to four primitives per
   leaf the leaf half was the longer one: replayed as waves of 64 rays over the mesh scene (profiles/tools/bvh_sim.py) a
   closest-hit ray costs 9.0 inner steps + 2.7 triangle tests with two, 7.4 + 7.2 with four -- a fifth fewer
   wave-instructions at the same lane utilisation.  (The descriptor holds up to 15: coincident centroids stay together.) */
#ifndef VCM_BVH_LEAF_MAX
#define VCM_BVH_LEAF_MAX 2
#endif
struct BvhBuildPrim { float lo[3], hi[3], c[3]; int index; };

inline void bvh_prim_box(const vcm_prim &p, float lo[3], float hi[3])
{
    if (p.type == VCM_PRIM_TRIANGLE) {
        for (int k = 0; k < 3; k++) {
            lo[k] = std::min(p.p0[k], std::min(p.p1[k], p.p2[k]));
            hi[k] = std::max(p.p0[k], std::max(p.p1[k], p.p2[k]));
        }
    } else {   /* sphere: p0 = centre, p1[0] = radius */
        for (int k = 0; k < 3; k++) { lo[k] = p.p0[k] - p.p1[0]; hi[k] = p.p0[k] + p.p1[0]; }
    }
}

inline int bvh_build_node(SceneHost &s, std::vector<BvhBuildPrim> &bp, int first, int count, float pad)
{
    const int me = (int)s.nodes.size();
    s.nodes.push_back(BvhNode());
    float lo[3] = { 1e36f, 1e36f, 1e36f }, hi[3] = { -1e36f, -1e36f, -1e36f }, clo[3] = { 1e36f, 1e36f, 1e36f }, chi[3] = { -1e36f, -1e36f, -1e36f };
    for (int i = first; i < first + count; i++)
        for (int k = 0; k < 3; k++) {
            lo[k] = std::min(lo[k], bp[i].lo[k]); hi[k] = std::max(hi[k], bp[i].hi[k]);
            clo[k] = std::min(clo[k], bp[i].c[k]); chi[k] = std::max(chi[k], bp[i].c[k]);
        }
    /* grown: the traversal's slab test and the primitives' own hit computations round (relative 1e-6); a box that is
       larger by 1e-4 of the scene can only add visits */
    for (int k = 0; k < 3; k++) { s.nodes[me].bmin[k] = lo[k] - pad; s.nodes[me].bmax[k] = hi[k] + pad; }
    int axis = 0;
    for (int k = 1; k < 3; k++) if (chi[k] - clo[k] > chi[axis] - clo[axis]) axis = k;
    const bool flat = !(chi[axis] - clo[axis] > 0.f);
    if (count <= VCM_BVH_LEAF_MAX || (flat && count <= 15)) {
        s.nodes[me].leaf = ((int)s.leafPrims.size() << 4) | count;
        for (int i = first; i < first + count; i++) s.leafPrims.push_back(bp[i].index);
        s.nodes[me].escape = (int)s.nodes.size();
        return me;
    }
    /* binned surface-area heuristic over all three axes (16 bins each; the axis of the largest centroid extent alone --
       rounds 2-3 -- left the room's large wall triangles in the floor mesh's subtrees); median split as the fallback */
    int mid = first + count / 2;
    if (!flat) {
        const int B = 16;
        auto area = [](const float *l, const float *h) { const float x = h[0] - l[0], y = h[1] - l[1], z = h[2] - l[2]; return x * y + y * z + z * x; };
        float best = 1e36f; int bestSplit = -1, bestAxis = axis;
        for (int ax = 0; ax < 3; ax++) {
            if (!(chi[ax] - clo[ax] > 0.f)) continue;
            float blo[B][3], bhi[B][3]; int bn[B];
            for (int b = 0; b < B; b++) { bn[b] = 0; for (int k = 0; k < 3; k++) { blo[b][k] = 1e36f; bhi[b][k] = -1e36f; } }
            const float scale = (float)B / (chi[ax] - clo[ax]);
            for (int i = first; i < first + count; i++) {
                int b = (int)((bp[i].c[ax] - clo[ax]) * scale); b = b < 0 ? 0 : (b >= B ? B - 1 : b);
                bn[b]++;
                for (int k = 0; k < 3; k++) { blo[b][k] = std::min(blo[b][k], bp[i].lo[k]); bhi[b][k] = std::max(bhi[b][k], bp[i].hi[k]); }
            }
            for (int sp = 1; sp < B; sp++) {
                float l0[3] = { 1e36f, 1e36f, 1e36f }, h0[3] = { -1e36f, -1e36f, -1e36f }, l1[3] = { 1e36f, 1e36f, 1e36f }, h1[3] = { -1e36f, -1e36f, -1e36f };
                int n0 = 0, n1 = 0;
                for (int b = 0; b < B; b++) {
                    if (!bn[b]) continue;
                    float *l = b < sp ? l0 : l1, *h = b < sp ? h0 : h1;
                    (b < sp ? n0 : n1) += bn[b];
                    for (int k = 0; k < 3; k++) { l[k] = std::min(l[k], blo[b][k]); h[k] = std::max(h[k], bhi[b][k]); }
                }
                if (!n0 || !n1) continue;
                const float cost = area(l0, h0) * n0 + area(l1, h1) * n1;
                if (cost < best) { best = cost; bestSplit = sp; bestAxis = ax; }
            }
        }
        if (bestSplit > 0) {
            axis = bestAxis;
            const float scale = (float)B / (chi[axis] - clo[axis]);
            auto bin_of = [&](const BvhBuildPrim &p) { int b = (int)((p.c[axis] - clo[axis]) * scale); return b < 0 ? 0 : (b >= B ? B - 1 : b); };
            auto it = std::stable_partition(bp.begin() + first, bp.begin() + first + count, [&](const BvhBuildPrim &p) { return bin_of(p) < bestSplit; });
            mid = (int)(it - bp.begin());
        }
    }
    if (mid <= first || mid >= first + count) {   /* degenerate: all centroids in one bin */
        std::stable_sort(bp.begin() + first, bp.begin() + first + count, [&](const BvhBuildPrim &a, const BvhBuildPrim &b) { return a.c[axis] < b.c[axis]; });
        mid = first + count / 2;
    }
    s.nodes[me].leaf = -1;
    bvh_build_node(s, bp, first, mid - first, pad);
    bvh_build_node(s, bp, mid, first + count - mid, pad);
    s.nodes[me].escape = (int)s.nodes.size();
    return me;
}

inline void scene_host_build_bvh(SceneHost &s)
{
    s.nodes.clear(); s.leafPrims.clear();
    const int n = (int)s.prims.size();
    if (n == 0) return;
    std::vector<BvhBuildPrim> bp((size_t)n);
    float lo[3] = { 1e36f, 1e36f, 1e36f }, hi[3] = { -1e36f, -1e36f, -1e36f };
    for (int i = 0; i < n; i++) {
        bvh_prim_box(s.prims[i], bp[i].lo, bp[i].hi);
        bp[i].index = i;
        for (int k = 0; k < 3; k++) {
            bp[i].c[k] = 0.5f * (bp[i].lo[k] + bp[i].hi[k]);
            lo[k] = std::min(lo[k], bp[i].lo[k]); hi[k] = std::max(hi[k], bp[i].hi[k]);
        }
    }
    float extent = 0.f;
    for (int k = 0; k < 3; k++) extent = std::max(extent, std::max(hi[k] - lo[k], std::max(std::fabs(lo[k]), std::fabs(hi[k]))));
    const float pad = 1e-4f * extent + 1e-30f;
    s.nodes.reserve((size_t)n);
    bvh_build_node(s, bp, 0, n, pad);
    /* the wide view: inner nodes numbered in depth-first order, each holding the boxes of its two children -- the left
       child is the next node in memory, the right one the left's escape */
    s.wide.clear();
    for (size_t i = 0; i < s.nodes.size(); i++) if (s.nodes[i].leaf < 0) { s.nodes[i].leaf = -1 - (int)s.wide.size(); s.wide.push_back(BvhWide()); }
    for (size_t i = 0; i < s.nodes.size(); i++) {
        if (s.nodes[i].leaf >= 0) continue;
        BvhWide &w = s.wide[(size_t)(-1 - s.nodes[i].leaf)];
        const int l = (int)i + 1, r = s.nodes[(size_t)l].escape;
        const BvhNode &nl = s.nodes[(size_t)l], &nr = s.nodes[(size_t)r];
        for (int k = 0; k < 3; k++) { w.lmin[k] = nl.bmin[k]; w.lmax[k] = nl.bmax[k]; w.rmin[k] = nr.bmin[k]; w.rmax[k] = nr.bmax[k]; }
        w.lnode = l; w.lref = nl.leaf; w.rnode = r; w.rref = nr.leaf;
    }
    s.leafData.resize(s.leafPrims.size());
    for (size_t i = 0; i < s.leafPrims.size(); i++) { s.leafData[i].prim = s.prims[(size_t)s.leafPrims[i]]; s.leafData[i].index = s.leafPrims[i]; s.leafData[i].pad = 0; }
}

/* what the intersection code walks: the packed list for the reference's own scenes, the BVH beyond */
inline void scene_host_build_accel(SceneHost &s, bool forceBvh)
{
    s.ops.clear(); s.pairs.clear(); s.nodes.clear(); s.wide.clear(); s.leafPrims.clear(); s.leafData.clear(); s.fastPairs.clear(); s.fastSpheres.clear(); s.fastRects.clear();
    s.nFastRects[0] = s.nFastRects[1] = s.nFastRects[2] = 0; s.fastGmax = 0.f;
    s.fastRw2 = s.fastRadius = 0.f; s.fastCenter[0] = s.fastCenter[1] = s.fastCenter[2] = 0.f;
    if ((int)s.prims.size() > VCM_MAX_PRIMS || (forceBvh && !s.prims.empty())) scene_host_build_bvh(s);
    else { scene_host_build_pairs(s); scene_host_build_fast(s); }
}
inline bool scene_host_force_bvh()
{
    const char *e = getenv("SMALLVCM_AMD_FORCE_BVH");
    return e && e[0] == '1';
}

} // namespace vcm
#endif
