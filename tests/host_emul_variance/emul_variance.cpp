// TEST INFRASTRUCTURE.  The host emulation of tests/host_emul_denoise/emul_denoise.cpp with the per-pixel variance and the
// noise statistic of smallvcm_amd/csrc/vcm_variance.h: the functions the kernels of vcm_variance.hip run, compiled for the
// host and driven serially -- the lanes of the grid in a loop, the combination tree step by step -- for
// tests/test_variance.py and tests/test_gpu_variance.py.  Never built into libsmallvcm_amd.so.
#include "../host_emul_denoise/emul_denoise.cpp"
#include "../../smallvcm_amd/csrc/vcm_variance.h"

static void emul_block_tree(VarAcc *v)
{
    for (int s = 0; s < VCM_VAR_TREE_STEPS; s++)
        for (int lane = 0; lane < VCM_VAR_BLOCK; lane++) var_tree_step(v, s, lane);
}

extern "C" {

/* k_var_update: iteration k (from 1) of the n-pixel float4 images prev, mom from the running sum sum3 */
void emul_var_update(long long n, const float *sum3, int k, float *prev, float *mom)
{
    const float km1 = (float)(k - 1), kf = (float)k;
    for (long long p = 0; p < n; p++)
        var_update_pixel(sum3[p * 3], sum3[p * 3 + 1], sum3[p * 3 + 2], k, km1, kf, ((F4 *)prev)[p], ((F4 *)mom)[p]);
}

/* k_var_read: out3 = V of every pixel and channel */
void emul_var_read(long long n, const float *mom, int k, float *out3)
{
    const float kk = (float)((double)k * (double)(k - 1));
    for (long long p = 0; p < n; p++) {
        const F4 m = ((const F4 *)mom)[p];
        out3[p * 3] = var_of_mean(m.x, kk); out3[p * 3 + 1] = var_of_mean(m.y, kk); out3[p * 3 + 2] = var_of_mean(m.z, kk);
    }
}

/* k_var_stats + k_var_stats2 with the grid var_grid_blocks(n, maxBlocks); -1 for k < 2 */
int emul_var_stats(long long n, const float *prev, const float *mom, int k, float threshold, int maxBlocks, vcm_noise_stats *out)
{
    if (k < 2) { g_pickErr = "the variance needs at least two iterations"; return -1; }
    const int blocks = var_grid_blocks(n, maxBlocks);
    const float kf = (float)k, kk = (float)((double)k * (double)(k - 1));
    std::vector<VarAcc> partials((size_t)blocks), v(VCM_VAR_BLOCK);
    for (int b = 0; b < blocks; b++) {
        for (int lane = 0; lane < VCM_VAR_BLOCK; lane++)
            v[(size_t)lane] = var_lane_sum(n, blocks, b, lane, kf, kk, threshold, [&](long long p, F4 &pv, F4 &m) {
                pv = ((const F4 *)prev)[p]; m = ((const F4 *)mom)[p];
            });
        emul_block_tree(v.data());
        partials[(size_t)b] = v[0];
    }
    for (int lane = 0; lane < VCM_VAR_BLOCK; lane++) v[(size_t)lane] = var_lane_sum_partials(partials.data(), blocks, lane);
    emul_block_tree(v.data());
    var_finish_stats(v[0], k, n, out);
    return 0;
}

/* the library's dn_launch_denoise2, serially (see emul_denoise): mom = the moments image, the variance of a colour channel is
   M2 * varFactor.  -1 (and emul_pick_error) for refused parameters. */
int emul_denoise2(int W, int H, const float *color, const float *fb3, float scale, const float *albedo, const float *guide,
                  const float *mom, float varFactor, float *out, const vcm_denoise_params2 *p)
{
    if (const char *why = dn_check_params2(p)) { g_pickErr = why; return -1; }
    if (!p->varianceGuided || p->passes == 0) {
        const vcm_denoise_params base = dn_base_params(*p);
        return emul_denoise(W, H, color, fb3, scale, albedo, guide, out, &base);
    }
    const size_t n = (size_t)W * H;
    const F4 *al = (const F4 *)albedo, *gd = (const F4 *)guide, *mo = (const F4 *)mom;
    std::vector<F4> a(n), b(n);
    for (size_t q = 0; q < n; q++) {
        const float r = fb3 ? fb3[q * 3] : color[q * 4], g = fb3 ? fb3[q * 3 + 1] : color[q * 4 + 1], bl = fb3 ? fb3[q * 3 + 2] : color[q * 4 + 2];
        a[q] = dn_prepare2(r, g, bl, scale, p->demodulate ? al[q] : mk4(1.f, 1.f, 1.f, 1.f), p->demodulate ? 1 : 0, mo[q], varFactor);
    }
    const F4 *src = a.data();
    for (int i = 0; i < p->passes; i++) {
        const DnPass2 P = dn_pass2(*p, W, H, i);
        F4 *dst = (i == p->passes - 1) ? (F4 *)out : (src == a.data() ? b.data() : a.data());
        for (int y = 0; y < H; y++)
            for (int x = 0; x < W; x++)
                dst[(size_t)y * W + x] = dn_filter_pixel2(P, x, y, al[(size_t)y * W + x], [&](int xq, int yq, F4 &cq, F4 &gq) {
                    cq = src[(size_t)yq * W + xq]; gq = gd[(size_t)yq * W + xq];
                });
        src = dst;
    }
    return 0;
}

} // extern "C"
