// TEST INFRASTRUCTURE.  The host emulation of tests/host_emul/emul.cpp with the light-selection entry points: a
// version-5 scene description (vcm_scene_desc5) for the emulated renderer and the known-answer records
// (VCM_KAT_LIGHT_PICK among them), and the tables as the scene host builds them, for tests/test_light_pick.py and
// tests/test_gpu_light_pick.py.  Never built into libsmallvcm_amd.so.
#include "../host_emul/emul.cpp"

namespace {
std::string g_pickErr;
}

extern "C" {

const char *emul_pick_error() { return g_pickErr.c_str(); }

void *emul_create5(const vcm_scene_desc5 *scene, int algorithm, float radiusFactor, float radiusAlpha, int seed,
                   int rank, int world)
{
    Emul *e = new Emul();
    if (!scene_host_from_desc5(*scene, e->host, g_pickErr)) { delete e; return NULL; }
    return emul_finish_create(e, algorithm, radiusFactor, radiusAlpha, seed, rank, world);
}

/* 0, or -1 when the description is rejected */
int emul_kat5(const vcm_scene_desc5 *scene, int op, int n, const float *in, float *out)
{
    SceneHost h;
    if (!scene_host_from_desc5(*scene, h, g_pickErr)) return -1;
    scene_host_build_accel(h, scene_host_force_bvh());
    DScene view;
    h.view(view);
    with_scene(view, [&](const auto &sc) {
        for (int i = 0; i < n; i++) kat_eval(sc, op, in + (size_t)i * VCM_KAT_FLOATS, out + (size_t)i * VCM_KAT_FLOATS);
    });
    return 0;
}

/* the tables as the scene host stores them: mode, the weights before the mix (nLights doubles), the quanta m_i
   (nLights ints), pmf (nLights floats), cdf (nLights + 1 floats); -1 when the description is rejected.  A UNIFORM
   scene has no tables: mode 0 and nothing written. */
int emul_pick_tables(const vcm_scene_desc5 *scene, int *mode, double *weights, int *quanta, float *pmf, float *cdf)
{
    SceneHost h;
    if (!scene_host_from_desc5(*scene, h, g_pickErr)) return -1;
    *mode = h.pickMode;
    if (h.pickMode == VCM_LIGHT_PICK_UNIFORM) return 0;
    const size_t n = h.lights.size();
    for (size_t i = 0; i < n; i++) { weights[i] = h.pickWeights[i]; quanta[i] = h.pickQuanta[i]; pmf[i] = h.pickPmf[i]; }
    for (size_t i = 0; i <= n; i++) cdf[i] = h.pickCdf[i];
    return 0;
}

/* how many of the generator's 2^23 floats (2j + 1) 2^-24, j in [j0, j1), pick each light: counts[nLights] += ... */
int emul_pick_count(const vcm_scene_desc5 *scene, unsigned j0, unsigned j1, long long *counts)
{
    SceneHost h;
    if (!scene_host_from_desc5(*scene, h, g_pickErr)) return -1;
    DScene view;
    h.view(view);
    for (unsigned j = j0; j < j1; j++) {
        float pmf = 0.f;
        const float r = (float)(2u * j + 1u) * 5.9604644775390625e-08f;
        counts[pick_light(view, r, pmf)]++;
    }
    return 0;
}

} // extern "C"
