// TEST INFRASTRUCTURE.  The host emulation of tests/host_emul/emul.cpp with the environment-map entry points: a
// version-3 scene description (vcm_scene_desc3) for the emulated renderer and the known-answer records, plus the
// env map's own functions (detmath.h dm_atan2f / dm_acosf, vcm_core.h env_eval / env_sample_dir, scene_host.h's
// tables) for tests/test_envmap.py.  Never built into libsmallvcm_amd.so.
#include "../host_emul/emul.cpp"

namespace {
/* a scene host + its view, built from a version-3 description (NULL on a rejected description, reason in g_envErr) */
struct EnvScene { SceneHost host; DScene sc; };
std::string g_envErr;
EnvScene *env_scene(const vcm_scene_desc3 *d)
{
    EnvScene *e = new EnvScene();
    if (!scene_host_from_desc3(*d, e->host, g_envErr)) { delete e; return NULL; }
    scene_host_build_accel(e->host, scene_host_force_bvh());
    e->host.view(e->sc);
    return e;
}
}

extern "C" {

const char *emul_envmap_error() { return g_envErr.c_str(); }

void *emul_create3(const vcm_scene_desc3 *scene, int algorithm, float radiusFactor, float radiusAlpha, int seed,
                   int rank, int world)
{
    Emul *e = new Emul();
    if (!scene_host_from_desc3(*scene, e->host, g_envErr)) { delete e; return NULL; }
    return emul_finish_create(e, algorithm, radiusFactor, radiusAlpha, seed, rank, world);
}

/* 0, or -1 when the description is rejected */
int emul_kat3(const vcm_scene_desc3 *scene, int op, int n, const float *in, float *out)
{
    EnvScene *e = env_scene(scene);
    if (!e) return -1;
    with_scene(e->sc, [&](const auto &sc) {
        for (int i = 0; i < n; i++) kat_eval(sc, op, in + (size_t)i * VCM_KAT_FLOATS, out + (size_t)i * VCM_KAT_FLOATS);
    });
    delete e;
    return 0;
}

/* the tables: texels W*H*4, marginal H+1, conditional H*(W+1); sizes in dims[0..3] = W, H, guide W, guide H */
int emul_env_tables(const vcm_scene_desc3 *scene, int *dims, float *texels, float *marg, float *cond)
{
    EnvScene *e = env_scene(scene);
    if (!e) return -1;
    const SceneHost &h = e->host;
    dims[0] = h.envW; dims[1] = h.envH; dims[2] = h.envGuideW; dims[3] = h.envGuideH;
    if (texels) memcpy(texels, h.envTexels.data(), h.envTexels.size() * sizeof(F4));
    if (marg) memcpy(marg, h.envMarg.data(), h.envMarg.size() * sizeof(float));
    if (cond) memcpy(cond, h.envCond.data(), h.envCond.size() * sizeof(float));
    delete e;
    return 0;
}

/* per direction: the texel index (row * W + col) env_eval reads and the pdf it returns */
int emul_env_lookup(const vcm_scene_desc3 *scene, int n, const float *dirs, int *texel, float *pdf)
{
    EnvScene *e = env_scene(scene);
    if (!e) return -1;
    for (int i = 0; i < n; i++) {
        float rho;
        texel[i] = env_texel_index(e->sc, ld3(dirs + 3 * i), rho);
        (void)env_eval(e->sc, ld3(dirs + 3 * i), pdf[i]);
    }
    delete e;
    return 0;
}

/* the direction of (u, v) as the sampler computes it (v * pi, u * 2 pi through dm_sincosf) */
void emul_env_uv_dir(int n, const float *uv, float *dirs)
{
    for (int i = 0; i < n; i++) {
        float st, ct, sp, cp;
        dm_sincosf(uv[2 * i + 1] * 3.14159265f, st, ct);
        dm_sincosf(uv[2 * i] * 6.28318531f, sp, cp);
        dirs[3 * i] = st * cp; dirs[3 * i + 1] = st * sp; dirs[3 * i + 2] = ct;
    }
}

void emul_atan2f_n(int n, const float *y, const float *x, float *out) { for (int i = 0; i < n; i++) out[i] = dm_atan2f(y[i], x[i]); }
void emul_acosf_n(int n, const float *z, float *out) { for (int i = 0; i < n; i++) out[i] = dm_acosf(z[i]); }

} // extern "C"
