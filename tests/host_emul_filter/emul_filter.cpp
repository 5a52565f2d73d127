// TEST INFRASTRUCTURE.  The host emulation of tests/host_emul/emul.cpp with the pixel-filter entry points: a version-6
// scene description (vcm_scene_desc6) for the emulated renderer and the known-answer records (VCM_KAT_FILTER among
// them), for tests/test_pixel_filter.py and tests/test_gpu_pixel_filter.py.  Never built into libsmallvcm_amd.so.
#include "../host_emul/emul.cpp"

namespace {
std::string g_filterErr;
}

extern "C" {

const char *emul_filter_error() { return g_filterErr.c_str(); }

void *emul_create6(const vcm_scene_desc6 *scene, int algorithm, float radiusFactor, float radiusAlpha, int seed,
                   int rank, int world)
{
    Emul *e = new Emul();
    if (!scene_host_from_desc6(*scene, e->host, g_filterErr)) { delete e; return NULL; }
    return emul_finish_create(e, algorithm, radiusFactor, radiusAlpha, seed, rank, world);
}

/* 0, or -1 when the description is rejected */
int emul_kat6(const vcm_scene_desc6 *scene, int op, int n, const float *in, float *out)
{
    SceneHost h;
    if (!scene_host_from_desc6(*scene, h, g_filterErr)) return -1;
    scene_host_build_accel(h, scene_host_force_bvh());
    DScene view;
    h.view(view);
    with_scene(view, [&](const auto &sc) {
        for (int i = 0; i < n; i++) kat_eval(sc, op, in + (size_t)i * VCM_KAT_FLOATS, out + (size_t)i * VCM_KAT_FLOATS);
    });
    return 0;
}

/* the filter as the scene host stores it: kind and radius */
int emul_filter_params(const vcm_scene_desc6 *scene, int *kind, float *radius)
{
    SceneHost h;
    if (!scene_host_from_desc6(*scene, h, g_filterErr)) return -1;
    *kind = h.filterKind; *radius = h.filterRadius;
    return 0;
}

} // extern "C"
