// TEST INFRASTRUCTURE.  The host emulation of tests/host_emul/emul.cpp with the sampler entry points: a version-7 scene
// description (vcm_scene_desc7) for the emulated renderer, the known-answer records (VCM_KAT_SAMPLER among them) and a
// log of where the draw groups of the paths start, for tests/test_sampler.py and tests/test_gpu_sampler.py.  Never built
// into libsmallvcm_amd.so.
#include <stdint.h>
#include <vector>
static std::vector<uint32_t> g_samplerTrace;   /* (group, kind, k0) per draw group, in the order the emulation runs them */
static bool g_samplerTraceOn = false;
#define VCM_SAMPLER_TRACE(group, kind, k0) \
    do { if (g_samplerTraceOn) { g_samplerTrace.push_back((uint32_t)(group)); g_samplerTrace.push_back((uint32_t)(kind)); g_samplerTrace.push_back((uint32_t)(k0)); } } while (0)
#include "../host_emul/emul.cpp"

namespace {
std::string g_samplerErr;
}

extern "C" {

const char *emul_sampler_error() { return g_samplerErr.c_str(); }

void *emul_create7(const vcm_scene_desc7 *scene, int algorithm, float radiusFactor, float radiusAlpha, int seed,
                   int rank, int world)
{
    Emul *e = new Emul();
    if (!scene_host_from_desc7(*scene, e->host, g_samplerErr)) { delete e; return NULL; }
    return emul_finish_create(e, algorithm, radiusFactor, radiusAlpha, seed, rank, world);
}
void *emul_create6(const vcm_scene_desc6 *scene, int algorithm, float radiusFactor, float radiusAlpha, int seed,
                   int rank, int world)
{
    Emul *e = new Emul();
    if (!scene_host_from_desc6(*scene, e->host, g_samplerErr)) { delete e; return NULL; }
    return emul_finish_create(e, algorithm, radiusFactor, radiusAlpha, seed, rank, world);
}

/* 0, or -1 when the description is rejected */
int emul_kat7(const vcm_scene_desc7 *scene, int op, int n, const float *in, float *out)
{
    SceneHost h;
    if (!scene_host_from_desc7(*scene, h, g_samplerErr)) return -1;
    if (op == VCM_KAT_SAMPLER) {
        for (int i = 0; i < n; i++) kat_sampler(in + (size_t)i * VCM_KAT_FLOATS, out + (size_t)i * VCM_KAT_FLOATS);
        return 0;
    }
    scene_host_build_accel(h, scene_host_force_bvh());
    DScene view;
    h.view(view);
    with_scene(view, [&](const auto &sc) {
        for (int i = 0; i < n; i++) kat_eval(sc, op, in + (size_t)i * VCM_KAT_FLOATS, out + (size_t)i * VCM_KAT_FLOATS);
    });
    return 0;
}

/* the sampler as the scene host stores it */
int emul_sampler_params(const vcm_scene_desc7 *scene, int *kind)
{
    SceneHost h;
    if (!scene_host_from_desc7(*scene, h, g_samplerErr)) return -1;
    *kind = h.sampler;
    return 0;
}

/* the three scramble seeds of pair j of a stream (sobol.h), for the tests of the streams */
void emul_sampler_seeds(uint32_t seed, uint32_t path, uint32_t kind, uint32_t j, uint32_t *out3)
{
    uint32_t s3;
    philox4x32_10(path, kind, j, 1u, seed, 0u, out3[0], out3[1], out3[2], s3);
}

/* the log of draw-group starts: on / off (clears), size in triples, copy */
void emul_sampler_trace(int on) { g_samplerTraceOn = on != 0; g_samplerTrace.clear(); }
long long emul_sampler_trace_size() { return (long long)(g_samplerTrace.size() / 3); }
void emul_sampler_trace_get(uint32_t *out) { memcpy(out, g_samplerTrace.data(), g_samplerTrace.size() * 4); }

} // extern "C"
