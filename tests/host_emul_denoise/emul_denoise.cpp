// TEST INFRASTRUCTURE.  The host emulation of tests/host_emul_pick/emul_pick.cpp with the feature buffers and the
// a-trous filter of smallvcm_amd/csrc/vcm_denoise.h: the functions the kernels of vcm_denoise.hip run, compiled for the
// host and driven serially in the order the library launches them, for tests/test_denoise.py and
// tests/test_gpu_denoise.py.  Never built into libsmallvcm_amd.so.
#include "../host_emul_pick/emul_pick.cpp"
#include "../../smallvcm_amd/csrc/vcm_denoise.h"

extern "C" {

/* guide (normal.xyz | depth) and albedo (rgb | 1) of the pixels of shard rank / world, 4 floats per pixel of the WHOLE
   frame (pixels of other shards stay 0); -1 when the description is rejected */
int emul_features5(const vcm_scene_desc5 *scene, int rank, int world, float *guide, float *albedo)
{
    SceneHost h;
    if (!scene_host_from_desc5(*scene, h, g_pickErr)) return -1;
    scene_host_build_accel(h, scene_host_force_bvh());
    DScene view;
    h.view(view);
    const int resX = (int)h.camera.resolution[0], N = resX * (int)h.camera.resolution[1];
    const int p0 = (int)((long long)N * rank / world), p1 = (int)((long long)N * (rank + 1) / world);
    memset(guide, 0, (size_t)N * 16); memset(albedo, 0, (size_t)N * 16);
    with_scene(view, [&](const auto &sc) {
        for (int p = p0; p < p1; p++) feature_pixel(sc, resX, p, ((F4 *)guide)[p], ((F4 *)albedo)[p]);
    });
    return 0;
}

/* the library's dn_launch_denoise, serially: out = the filtered image (4 floats per pixel).  fb3 != NULL: the colour is
   the W*H*3 image fb3 times scale, else the float4 image color.  -1 (and emul_pick_error) for refused parameters. */
int emul_denoise(int W, int H, const float *color, const float *fb3, float scale, const float *albedo, const float *guide,
                 float *out, const vcm_denoise_params *p)
{
    if (const char *why = dn_check_params(p)) { g_pickErr = why; return -1; }
    const size_t n = (size_t)W * H;
    const F4 *al = (const F4 *)albedo, *gd = (const F4 *)guide;
    std::vector<F4> a(n), b(n);
    auto prepare = [&](int demodulate, F4 *dst) {
        for (size_t q = 0; q < n; q++) {
            const float r = fb3 ? fb3[q * 3] : color[q * 4], g = fb3 ? fb3[q * 3 + 1] : color[q * 4 + 1], bl = fb3 ? fb3[q * 3 + 2] : color[q * 4 + 2];
            dst[q] = dn_prepare(r, g, bl, scale, demodulate ? al[q] : mk4(1.f, 1.f, 1.f, 1.f), demodulate);
        }
    };
    if (p->passes == 0) {
        if (!fb3) memcpy(out, color, n * 16); else prepare(0, (F4 *)out);
        return 0;
    }
    const F4 *src = (const F4 *)color;
    if (fb3 || p->demodulate) { prepare(p->demodulate ? 1 : 0, a.data()); src = a.data(); }
    for (int i = 0; i < p->passes; i++) {
        const DnPass P = dn_pass(*p, W, H, i);
        F4 *dst = (i == p->passes - 1) ? (F4 *)out : (src == a.data() ? b.data() : a.data());
        for (int y = 0; y < H; y++)
            for (int x = 0; x < W; x++)
                dst[(size_t)y * W + x] = dn_filter_pixel(P, x, y, al[(size_t)y * W + x], [&](int xq, int yq, F4 &cq, F4 &gq) {
                    cq = src[(size_t)yq * W + xq]; gq = gd[(size_t)yq * W + xq];
                });
        src = dst;
    }
    return 0;
}

} // extern "C"
