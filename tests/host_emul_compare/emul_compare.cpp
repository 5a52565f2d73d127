// TEST INFRASTRUCTURE.  The host emulation of the comparison with a reference image: the functions of
// smallvcm_amd/csrc/vcm_compare.h that the kernels of vcm_compare.hip run, compiled for the host and driven serially -- the
// lanes of a workgroup, the workgroups of a grid and the steps of the tree in loops, in the library's order -- for
// tests/test_compare.py and tests/test_gpu_compare.py.  Never built into libsmallvcm_amd.so.
#include <math.h>
#include <string.h>
#include <string>
#include <vector>
#include "../../smallvcm_amd/csrc/vcm_compare.h"

using namespace vcm;

static thread_local std::string g_err;
static int refuse(const char *why) { g_err = why; return -1; }

template <class Acc>
static void block_tree(Acc *v)
{
    for (int s = 0; s < VCM_CMP_TREE_STEPS; s++)
        for (int lane = 0; lane < VCM_CMP_BLOCK; lane++) cmp_tree_step(v, s, lane);
}

/* k_cmp_pixels: one CmpAcc per workgroup */
static void pixels(long long n, const float *img, int imgCh, float scale, const float *ref, int refCh, const vcm_compare_params &p, int blocks,
                   F4 *map, std::vector<CmpAcc> &partials)
{
    partials.resize((size_t)blocks);
    std::vector<CmpAcc> v(VCM_CMP_BLOCK);
    for (int b = 0; b < blocks; b++) {
        for (int lane = 0; lane < VCM_CMP_BLOCK; lane++)
            v[lane] = cmp_lane_sum(n, blocks, b, lane, [&](long long q, CmpAcc &a) {
                const F4 m = cmp_pixel(a, cmp_scaled(cmp_load(img, imgCh, q), scale), cmp_load(ref, refCh, q), q, p.relEpsilon, p.threshold);
                if (map) map[q] = m;
            });
        block_tree(v.data());
        partials[(size_t)b] = v[0];
    }
}

/* k_cmp_ssim: one SsimAcc per tile of 32 x 8 windows.  What a workgroup stages in LDS is here two images: the luminance
   pairs, and the rows' moments of the columns that are a window's centre. */
static void windows(int W, int H, const float *img, int imgCh, float scale, const float *ref, int refCh, const vcm_compare_params &p, F4 *map,
                    std::vector<SsimAcc> &partials)
{
    const CmpWin win = cmp_window_weights();
    const int R = VCM_CMP_RADIUS, tilesX = cmp_tiles_x(W), tilesY = cmp_tiles_y(H);
    std::vector<CmpXY> xy((size_t)W * H);
    for (long long q = 0; q < (long long)W * H; q++)
        xy[(size_t)q] = cmp_window_input(cmp_scaled(cmp_load(img, imgCh, q), scale), cmp_load(ref, refCh, q), p.peak);
    const int nc = W - 2 * R;   /* centres along a row */
    std::vector<CmpMom> rows((size_t)nc * H);
    for (int y = 0; y < H; y++)
        for (int c = 0; c < nc; c++) rows[(size_t)y * nc + c] = cmp_hpass(win, [&](int k) { return xy[(size_t)y * W + c + k]; });
    partials.resize((size_t)tilesX * tilesY);
    std::vector<SsimAcc> v(VCM_CMP_BLOCK);
    for (int by = 0; by < tilesY; by++)
        for (int bx = 0; bx < tilesX; bx++) {
            for (int lane = 0; lane < VCM_CMP_BLOCK; lane++) {
                const int cx = bx * VCM_CMP_TILE_X + R + lane % VCM_CMP_TILE_X, cy = by * VCM_CMP_TILE_Y + R + lane / VCM_CMP_TILE_X;
                SsimAcc a = cmp_ssim_zero();
                if (cx < W - R && cy < H - R) {
                    const CmpMom m = cmp_vpass(win, [&](int k) { return rows[(size_t)(cy - R + k) * nc + (cx - R)]; });
                    if (cmp_window_counts(m)) {
                        const float s = cmp_ssim(m);
                        a.sum = (double)s; a.windows = 1;
                        if (map) map[(size_t)cy * W + cx].w = s;
                    }
                }
                v[lane] = a;
            }
            block_tree(v.data());
            partials[(size_t)by * tilesX + bx] = v[0];
        }
}

/* k_cmp_finish */
static CmpResult finish(const std::vector<CmpAcc> &pix, const std::vector<SsimAcc> &win)
{
    std::vector<CmpAcc> v(VCM_CMP_BLOCK);
    std::vector<SsimAcc> u(VCM_CMP_BLOCK);
    for (int lane = 0; lane < VCM_CMP_BLOCK; lane++) {
        v[lane] = cmp_lane_sum_partials(pix.data(), (long long)pix.size(), lane);
        u[lane] = cmp_lane_sum_partials(win.data(), (long long)win.size(), lane);
    }
    block_tree(v.data());
    block_tree(u.data());
    CmpResult r;
    r.pix = v[0]; r.win = u[0];
    return r;
}

extern "C" {

const char *emul_compare_error() { return g_err.c_str(); }

void emul_compare_defaults(vcm_compare_params *out) { cmp_defaults(out); }

void emul_compare_weights(float *out11) { const CmpWin w = cmp_window_weights(); memcpy(out11, w.w, sizeof(w.w)); }

/* what vcm_compare and vcm_compare_buffers refuse of their numbers */
int emul_compare_check(float scale, const vcm_compare_params *p)
{
    if (const char *why = cmp_check_params(p)) return refuse(why);
    if (!cmp_finite(scale)) return refuse("scale is not finite");
    return 0;
}

/* what they refuse of a frame's height */
int emul_compare_check_size(int H, const vcm_compare_params *p)
{
    if (const char *why = cmp_check_size(H, p)) return refuse(why);
    return 0;
}

/* what vcm_set_reference refuses of its texels */
int emul_compare_reference_check(long long n, const float *rgb)
{
    if (!rgb) return refuse("NULL argument");
    for (long long i = 0; i < n; i++)
        if (!cmp_finite3(ld3(rgb + i * 3))) return refuse("the reference holds a non-finite texel");
    return 0;
}

/* vcm_compare_buffers with the pixel kernel's grid capped at maxBlocks (0: the default); map: W * H float4 or NULL; -1 (and
   emul_compare_error) where the library refuses */
int emul_compare(int W, int H, const float *img, int imgCh, float scale, const float *ref, int refCh, const vcm_compare_params *p, int maxBlocks,
                 float *map, vcm_compare_stats *out)
{
    if (!img || !ref || !p || !out) return refuse("NULL argument");
    if (W <= 0 || H <= 0 || (long long)W * H > 0x7fffffffll) return refuse("bad size");
    if ((imgCh != 3 && imgCh != 4) || (refCh != 3 && refCh != 4)) return refuse("channels must be 3 or 4");
    if (emul_compare_check(scale, p)) return -1;
    if (const char *why = cmp_check_size(H, p)) return refuse(why);
    if (p->writeMap && !map) return refuse("writeMap without mapOutDev");
    if (map && (map == img || map == ref)) return refuse("mapOutDev is one of the inputs");
    F4 *m = p->writeMap ? (F4 *)map : NULL;
    const long long n = (long long)W * H;
    std::vector<CmpAcc> pix;
    std::vector<SsimAcc> win;
    pixels(n, img, imgCh, scale, ref, refCh, *p, cmp_grid_blocks(n, maxBlocks > 0 ? maxBlocks : VCM_CMP_DEFAULT_MAX_BLOCKS), m, pix);
    if (p->ssim && cmp_tiles(W, H) > 0) windows(W, H, img, imgCh, scale, ref, refCh, *p, m, win);
    cmp_finish_stats(finish(pix, win), 0, n, p->peak, out);
    return 0;
}

} // extern "C"
