// TEST INFRASTRUCTURE.  The host emulation of tests/host_emul/emul.cpp for scenes with spot and sphere lights: a
// version-6 scene description (vcm_scene_desc6) for the emulated renderer and the known-answer records
// (VCM_KAT_LIGHT_RADIANCE_AT among them), the scene host's verdict on a description, and its POWER weights, for
// tests/test_lights.py and tests/test_gpu_lights.py.  Never built into libsmallvcm_amd.so.
#include "../host_emul/emul.cpp"

namespace {
std::string g_lightsErr;
}

extern "C" {

const char *emul_lights_error() { return g_lightsErr.c_str(); }

void *emul_lights_create(const vcm_scene_desc6 *scene, int algorithm, float radiusFactor, float radiusAlpha, int seed,
                         int rank, int world)
{
    Emul *e = new Emul();
    if (!scene_host_from_desc6(*scene, e->host, g_lightsErr)) { delete e; return NULL; }
    return emul_finish_create(e, algorithm, radiusFactor, radiusAlpha, seed, rank, world);
}

/* 0, or -1 when the description is rejected */
int emul_lights_kat(const vcm_scene_desc6 *scene, int op, int n, const float *in, float *out)
{
    SceneHost h;
    if (!scene_host_from_desc6(*scene, h, g_lightsErr)) return -1;
    scene_host_build_accel(h, scene_host_force_bvh());
    DScene view;
    h.view(view);
    with_scene(view, [&](const auto &sc) {
        for (int i = 0; i < n; i++) kat_eval(sc, op, in + (size_t)i * VCM_KAT_FLOATS, out + (size_t)i * VCM_KAT_FLOATS);
    });
    return 0;
}

/* what every create path does with a description: 0 = accepted, -1 = refused (emul_lights_error has the text).  On
   success info = { the scene holds a spot or sphere light, pickMode as stored, nLights } and, where there is a table,
   pmf[nLights]; power[nLights] = scene_host_light_power of every light. */
int emul_lights_check(const vcm_scene_desc6 *scene, int *info, float *pmf, double *power)
{
    SceneHost h;
    if (!scene_host_from_desc6(*scene, h, g_lightsErr)) return -1;
    info[0] = scene_host_has_new_lights(h) ? 1 : 0;
    info[1] = h.pickMode;
    info[2] = (int)h.lights.size();
    for (size_t i = 0; i < h.lights.size(); i++) {
        if (h.pickMode != VCM_LIGHT_PICK_UNIFORM) pmf[i] = h.pickPmf[i];
        power[i] = scene_host_light_power(h, (int)i);
    }
    return 0;
}

/* the version-1 path (vcm_scene_desc: fixed capacities): 0 = accepted, -1 = refused */
int emul_lights_check1(const vcm_scene_desc *scene, int *info)
{
    SceneHost h;
    if (!scene_host_from_desc(*scene, h, g_lightsErr)) return -1;
    info[0] = scene_host_has_new_lights(h) ? 1 : 0;
    info[1] = h.pickMode;
    info[2] = (int)h.lights.size();
    return 0;
}

} // extern "C"
