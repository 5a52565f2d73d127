// TEST INFRASTRUCTURE.  The host emulation of tests/host_emul/emul.cpp for scenes with GGX lobes: a version-8 scene
// description (vcm_scene_desc8) for the emulated renderer and the known-answer records, the scene host's verdict on a
// description and the ext table as it stores it, for tests/test_ggx.py and tests/test_gpu_ggx.py.  Never built into
// libsmallvcm_amd.so.
#include "../host_emul/emul.cpp"
#include "../../smallvcm_amd/csrc/vcm_denoise.h"

namespace {
std::string g_ggxErr;
}

extern "C" {

const char *emul_ggx_error() { return g_ggxErr.c_str(); }

void *emul_create8(const vcm_scene_desc8 *scene, int algorithm, float radiusFactor, float radiusAlpha, int seed,
                   int rank, int world)
{
    Emul *e = new Emul();
    if (!scene_host_from_desc8(*scene, e->host, g_ggxErr)) { delete e; return NULL; }
    return emul_finish_create(e, algorithm, radiusFactor, radiusAlpha, seed, rank, world);
}
void *emul_create7(const vcm_scene_desc7 *scene, int algorithm, float radiusFactor, float radiusAlpha, int seed,
                   int rank, int world)
{
    Emul *e = new Emul();
    if (!scene_host_from_desc7(*scene, e->host, g_ggxErr)) { delete e; return NULL; }
    return emul_finish_create(e, algorithm, radiusFactor, radiusAlpha, seed, rank, world);
}

/* 0, or -1 when the description is rejected */
int emul_kat8(const vcm_scene_desc8 *scene, int op, int n, const float *in, float *out)
{
    SceneHost h;
    if (!scene_host_from_desc8(*scene, h, g_ggxErr)) return -1;
    scene_host_build_accel(h, scene_host_force_bvh());
    DScene view;
    h.view(view);
    with_scene(view, [&](const auto &sc) {
        for (int i = 0; i < n; i++) kat_eval(sc, op, in + (size_t)i * VCM_KAT_FLOATS, out + (size_t)i * VCM_KAT_FLOATS);
    });
    return 0;
}

/* guide (normal.xyz | depth) and albedo (rgb | 1) of every pixel, 4 floats each, as the feature kernel computes them;
   -1 when the description is rejected */
int emul_features8(const vcm_scene_desc8 *scene, float *guide, float *albedo)
{
    SceneHost h;
    if (!scene_host_from_desc8(*scene, h, g_ggxErr)) return -1;
    scene_host_build_accel(h, scene_host_force_bvh());
    DScene view;
    h.view(view);
    const int resX = (int)h.camera.resolution[0], N = resX * (int)h.camera.resolution[1];
    with_scene(view, [&](const auto &sc) {
        for (int p = 0; p < N; p++) feature_pixel(sc, resX, p, ((F4 *)guide)[p], ((F4 *)albedo)[p]);
    });
    return 0;
}

/* what every create path does with a description: 0 = accepted, -1 = refused (emul_ggx_error has the text).  On success
   *nExt = the entries of the stored table (0: the version-7 scene, else nMaterials) and ext receives them (4 floats each). */
int emul_ggx_check(const vcm_scene_desc8 *scene, int *nExt, float *ext)
{
    SceneHost h;
    if (!scene_host_from_desc8(*scene, h, g_ggxErr)) return -1;
    *nExt = (int)h.materialExt.size();
    for (size_t m = 0; m < h.materialExt.size(); m++) {
        for (int k = 0; k < 3; k++) ext[4 * m + k] = h.materialExt[m].ggx[k];
        ext[4 * m + 3] = h.materialExt[m].alpha;
    }
    return 0;
}

} // extern "C"
