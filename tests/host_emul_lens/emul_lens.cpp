// TEST INFRASTRUCTURE.  The host emulation of tests/host_emul/emul.cpp with the thin-lens entry points: a version-4
// scene description (vcm_scene_desc4) for the emulated renderer and the known-answer records (VCM_KAT_LENS among
// them), for tests/test_thin_lens.py and tests/test_gpu_thin_lens.py.  Never built into libsmallvcm_amd.so.
#include "../host_emul/emul.cpp"

namespace {
std::string g_lensErr;
}

extern "C" {

const char *emul_lens_error() { return g_lensErr.c_str(); }

void *emul_create4(const vcm_scene_desc4 *scene, int algorithm, float radiusFactor, float radiusAlpha, int seed,
                   int rank, int world)
{
    Emul *e = new Emul();
    if (!scene_host_from_desc4(*scene, e->host, g_lensErr)) { delete e; return NULL; }
    return emul_finish_create(e, algorithm, radiusFactor, radiusAlpha, seed, rank, world);
}

/* 0, or -1 when the description is rejected */
int emul_kat4(const vcm_scene_desc4 *scene, int op, int n, const float *in, float *out)
{
    SceneHost h;
    if (!scene_host_from_desc4(*scene, h, g_lensErr)) return -1;
    scene_host_build_accel(h, scene_host_force_bvh());
    DScene view;
    h.view(view);
    with_scene(view, [&](const auto &sc) {
        for (int i = 0; i < n; i++) kat_eval(sc, op, in + (size_t)i * VCM_KAT_FLOATS, out + (size_t)i * VCM_KAT_FLOATS);
    });
    return 0;
}

/* the lens as the scene host stores it: radius, focus, right[3], up[3] (8 floats) */
int emul_lens_params(const vcm_scene_desc4 *scene, float *out8)
{
    SceneHost h;
    if (!scene_host_from_desc4(*scene, h, g_lensErr)) return -1;
    out8[0] = h.lensRadius; out8[1] = h.lensFocus;
    for (int k = 0; k < 3; k++) { out8[2 + k] = h.lensRight[k]; out8[5 + k] = h.lensUp[k]; }
    return 0;
}

} // extern "C"
