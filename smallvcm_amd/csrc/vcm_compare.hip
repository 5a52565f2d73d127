// vcm_compare.hip -- the kernels of the comparison with a reference image (vcm_compare.h holds what a pixel and a window
// compute and the order in which lanes are combined).  A translation unit of its own: no kernel of the other translation
// units is recompiled differently because these exist.
//
//   k_cmp_pixels   a pure stream: 12 or 16 B of the image and 12 or 16 B of the reference read per pixel (both
//                  kinds end as one 12-byte load per pixel, global_load_dwordx3: .w is never used, and a 3-float image's
//                  64 x 12 B per wave are one contiguous 768-byte run), 16 B written with a map.  Every lane sums its pixels in index order in binary64,
//                  the workgroup combines its 256 lanes through LDS by cmp_tree_step, one CmpAcc per workgroup goes to
//                  `partials`.
//   k_cmp_ssim     a workgroup of 256 lanes owns a tile of 32 x 8 windows.  It stages the (x, y) luminance pairs of the
//                  tile and its halo of 5 pixels, 42 x 18 x 8 B = 6048 B, in LDS; the rows' pass writes the five moments
//                  of 18 rows x 32 columns, 5 x 2304 B = 11520 B; the columns' pass and the ratio run from there.  A wave
//                  is two rows of 32 lanes: in the rows' pass its lanes read consecutive 8-byte slots (5 ds_read2_b64 + 1 ds_read_b64
//                  per output), in the columns' pass 64 consecutive 4-byte slots of one moment -- no bank is asked twice.
//                  The kernel's ds_read_b128 are the reduction tree's 16-byte SsimAcc slots.  One SsimAcc per workgroup.
//   k_cmp_finish   ONE workgroup: lane l sums the partials l, l + 256, ... of both kernels and the same tree gives the
//                  image's CmpResult.
// No floating-point atomics anywhere: the grids are functions of the image's size (and the cap) alone, and the same grid
// gives the same bits on every run.
#include <hip/hip_runtime.h>
#include <atomic>
#include "vcm_compare.h"

using namespace vcm;

#define VCM_CMP_LDS_X (VCM_CMP_TILE_X + 2 * VCM_CMP_RADIUS)   /* 42 */
#define VCM_CMP_LDS_Y (VCM_CMP_TILE_Y + 2 * VCM_CMP_RADIUS)   /* 18 */

/* pixel p of an image of kChannels floats per pixel: one 16-byte load, or three 4-byte loads */
template <int kChannels>
static __device__ inline V3 cmp_load_dev(const float *__restrict__ src, long long p)
{
    if constexpr (kChannels == 4) {
        const F4 v = ((const F4 *)src)[p];
        return mk3(v.x, v.y, v.z);
    } else {
        return mk3(src[(size_t)p * 3], src[(size_t)p * 3 + 1], src[(size_t)p * 3 + 2]);
    }
}

template <class Acc>
static __device__ inline void cmp_block_tree(Acc *v, int lane)
{
    __syncthreads();
    for (int s = 0; s < VCM_CMP_TREE_STEPS; s++) {
        cmp_tree_step(v, s, lane);
        __syncthreads();
    }
}

template <int kImg, int kRef>
__global__ void __launch_bounds__(VCM_CMP_BLOCK)
k_cmp_pixels(long long n, const float *__restrict__ img, float scale, const float *__restrict__ ref, float relEps, float threshold,
             F4 *__restrict__ map, CmpAcc *__restrict__ partials)
{
    __shared__ CmpAcc v[VCM_CMP_BLOCK];
    const int lane = (int)threadIdx.x;
    v[lane] = cmp_lane_sum(n, (int)gridDim.x, (int)blockIdx.x, lane, [&](long long p, CmpAcc &a) {
        const F4 m = cmp_pixel(a, cmp_scaled(cmp_load_dev<kImg>(img, p), scale), cmp_load_dev<kRef>(ref, p), p, relEps, threshold);
        if (map) map[p] = m;
    });
    cmp_block_tree(v, lane);
    if (lane == 0) partials[blockIdx.x] = v[0];
}

template <int kImg, int kRef>
__global__ void __launch_bounds__(VCM_CMP_BLOCK)
k_cmp_ssim(int W, int H, const float *__restrict__ img, float scale, const float *__restrict__ ref, float peak, CmpWin win,
           F4 *__restrict__ map, SsimAcc *__restrict__ partials)
{
    __shared__ CmpXY sXY[VCM_CMP_LDS_X * VCM_CMP_LDS_Y];
    __shared__ float sM[5][VCM_CMP_LDS_Y * VCM_CMP_TILE_X];
    __shared__ SsimAcc v[VCM_CMP_BLOCK];
    const int lane = (int)threadIdx.x;
    /* the staged pixels start at the tile's first window centre - 5: (32 bx, 8 by) */
    const int gx0 = (int)blockIdx.x * VCM_CMP_TILE_X, gy0 = (int)blockIdx.y * VCM_CMP_TILE_Y;
    for (int i = lane; i < VCM_CMP_LDS_X * VCM_CMP_LDS_Y; i += VCM_CMP_BLOCK) {
        const int lx = i % VCM_CMP_LDS_X, ly = i / VCM_CMP_LDS_X;
        const int gx = gx0 + lx, gy = gy0 + ly;
        CmpXY xy = cmp_window_outside();
        if (gx < W && gy < H) {
            const long long q = (long long)gy * W + gx;
            xy = cmp_window_input(cmp_scaled(cmp_load_dev<kImg>(img, q), scale), cmp_load_dev<kRef>(ref, q), peak);
        }
        sXY[i] = xy;
    }
    __syncthreads();
    for (int i = lane; i < VCM_CMP_LDS_Y * VCM_CMP_TILE_X; i += VCM_CMP_BLOCK) {
        const int col = i % VCM_CMP_TILE_X, row = i / VCM_CMP_TILE_X;
        const CmpXY *r = sXY + row * VCM_CMP_LDS_X + col;
        const CmpMom m = cmp_hpass(win, [&](int k) { return r[k]; });
        sM[0][i] = m.mx; sM[1][i] = m.my; sM[2][i] = m.xx; sM[3][i] = m.yy; sM[4][i] = m.xy;
    }
    __syncthreads();
    const int tx = lane % VCM_CMP_TILE_X, ty = lane / VCM_CMP_TILE_X;
    const CmpMom m = cmp_vpass(win, [&](int k) {
        const int s = (ty + k) * VCM_CMP_TILE_X + tx;
        CmpMom r;
        r.mx = sM[0][s]; r.my = sM[1][s]; r.xx = sM[2][s]; r.yy = sM[3][s]; r.xy = sM[4][s];
        return r;
    });
    const int cx = gx0 + VCM_CMP_RADIUS + tx, cy = gy0 + VCM_CMP_RADIUS + ty;
    const bool counts = cx < W - VCM_CMP_RADIUS && cy < H - VCM_CMP_RADIUS && cmp_window_counts(m);
    const float s = cmp_ssim(m);
    SsimAcc a;
    a.sum = counts ? (double)s : 0.0;
    a.windows = counts ? 1 : 0;
    if (counts && map) map[(size_t)cy * W + cx].w = s;
    v[lane] = a;
    cmp_block_tree(v, lane);
    if (lane == 0) partials[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = v[0];
}

__global__ void __launch_bounds__(VCM_CMP_BLOCK)
k_cmp_finish(const CmpAcc *__restrict__ pix, int nPix, const SsimAcc *__restrict__ win, long long nWin, CmpResult *__restrict__ result)
{
    __shared__ CmpAcc v[VCM_CMP_BLOCK];
    __shared__ SsimAcc u[VCM_CMP_BLOCK];
    const int lane = (int)threadIdx.x;
    v[lane] = cmp_lane_sum_partials(pix, (long long)nPix, lane);
    u[lane] = cmp_lane_sum_partials(win, nWin, lane);
    cmp_block_tree(v, lane);
    cmp_block_tree(u, lane);
    if (lane == 0) { result->pix = v[0]; result->win = u[0]; }
}

namespace vcm {

static std::atomic<int> g_cmpMaxBlocks(VCM_CMP_DEFAULT_MAX_BLOCKS);
int cmp_max_blocks() { return g_cmpMaxBlocks.load(); }
void cmp_set_max_blocks(int blocks) { g_cmpMaxBlocks.store(blocks > 0 ? blocks : VCM_CMP_DEFAULT_MAX_BLOCKS); }

/* the two kernels of a comparison; the first launch that fails ends it (what comes after would read partials never written) */
template <int kImg, int kRef>
static hipError_t cmp_launch_kernels(int W, int H, const float *img, float scale, const float *ref, const vcm_compare_params &p, int blocks,
                                     F4 *map, CmpAcc *pix, SsimAcc *win, hipStream_t stream)
{
    const long long n = (long long)W * H;
    hipLaunchKernelGGL((k_cmp_pixels<kImg, kRef>), dim3(blocks), dim3(VCM_CMP_BLOCK), 0, stream, n, img, scale, ref, p.relEpsilon, p.threshold, map, pix);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess || !p.ssim || cmp_tiles(W, H) == 0) return e;
    hipLaunchKernelGGL((k_cmp_ssim<kImg, kRef>), dim3((unsigned)cmp_tiles_x(W), (unsigned)cmp_tiles_y(H)), dim3(VCM_CMP_BLOCK), 0, stream, W, H, img,
                       scale, ref, p.peak, cmp_window_weights(), map, win);
    return hipGetLastError();
}

hipError_t cmp_launch(int W, int H, const float *img, int imgChannels, float scale, const float *ref, int refChannels,
                      const vcm_compare_params &p, int maxBlocks, F4 *map, char *scratch, hipStream_t stream)
{
    const int blocks = cmp_grid_blocks((long long)W * H, maxBlocks);
    CmpAcc *pix = (CmpAcc *)scratch;
    SsimAcc *win = (SsimAcc *)(scratch + (size_t)maxBlocks * sizeof(CmpAcc));
    F4 *m = p.writeMap ? map : NULL;
    if (p.ssim && cmp_tiles_y(H) > VCM_CMP_MAX_TILES_Y) return hipErrorInvalidConfiguration;   /* (the C-ABI refuses it by name first) */
    hipError_t e;
    if (imgChannels == 4 && refChannels == 4) e = cmp_launch_kernels<4, 4>(W, H, img, scale, ref, p, blocks, m, pix, win, stream);
    else if (imgChannels == 4) e = cmp_launch_kernels<4, 3>(W, H, img, scale, ref, p, blocks, m, pix, win, stream);
    else if (refChannels == 4) e = cmp_launch_kernels<3, 4>(W, H, img, scale, ref, p, blocks, m, pix, win, stream);
    else e = cmp_launch_kernels<3, 3>(W, H, img, scale, ref, p, blocks, m, pix, win, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_cmp_finish, dim3(1), dim3(VCM_CMP_BLOCK), 0, stream, (const CmpAcc *)pix, blocks, (const SsimAcc *)win,
                       p.ssim ? cmp_tiles(W, H) : 0ll, cmp_result_of(scratch, W, H, maxBlocks));
    return hipGetLastError();
}

} // namespace vcm
