// vcm_display.hip -- the kernels of the display transform (vcm_display.h holds what a lane computes).  A translation unit
// of its own: no kernel of the other translation units is recompiled differently because these exist.
//
//   k_disp_histogram  every wave counts into an LDS sub-histogram of its own (4 x 260 32-bit counters); a wave whose 64
//                     lanes all go to one counter -- a constant image, a flat sky -- adds once, by one lane, instead of
//                     serialising 64 LDS atomics on one address.  A workgroup adds its non-zero counters to the 64-bit
//                     global ones when it is done: integer additions, the same counts in any order.
//   k_disp_finish     a pure stream: 12 or 16 B read, 16 B written per pixel; curve and transfer in registers
//   bloom             per level three small kernels (2 x 2 mean, row blur, column blur), then the up-and-add chain; the
//                     last upsample is fused into k_disp_finish_bloom, so that E is never written.  The levels together hold a
//                     third of the image's pixels: the two full-resolution passes (k_disp_down0 reads the source,
//                     k_disp_finish_bloom reads it again and writes the result) carry the traffic, which is why the 5 x 5
//                     blur is two plain passes over L2-resident levels and not an LDS tile.
#include <hip/hip_runtime.h>
#include <atomic>
#include "vcm_display.h"

using namespace vcm;

#define VCM_DISP_WAVES (VCM_DISP_BLOCK / 64)
#define VCM_DISP_LDS_COUNTERS (VCM_DISP_CLAMPED_HIGH + 1)   /* 260: the bins and the four counters beside them */

/* one counter of a wave's sub-histogram += the lanes of the wave that name it */
static __device__ inline void disp_count(unsigned *h, int slot, bool active)
{
    const unsigned long long act = __ballot(active);
    if (act == 0ull) return;
    const int first = __ffsll((long long)act) - 1;
    const int s0 = __shfl(slot, first);
    const unsigned long long same = __ballot(active && slot == s0);
    if (same == act) {   /* all of them agree: one addition by one lane */
        if ((int)(threadIdx.x & 63) == first) atomicAdd(&h[s0], (unsigned)__popcll(act));
    } else if (active) atomicAdd(&h[slot], 1u);
}

__global__ void __launch_bounds__(VCM_DISP_BLOCK)
k_disp_histogram(long long n, const float *__restrict__ src, int channels, float scale, unsigned long long *__restrict__ counters)
{
    __shared__ unsigned h[VCM_DISP_WAVES][VCM_DISP_LDS_COUNTERS];
    for (int i = (int)threadIdx.x; i < VCM_DISP_WAVES * VCM_DISP_LDS_COUNTERS; i += VCM_DISP_BLOCK) (&h[0][0])[i] = 0u;
    __syncthreads();
    unsigned *mine = h[threadIdx.x >> 6];
    const long long G = (long long)gridDim.x * VCM_DISP_BLOCK;
    /* every lane of a wave takes every turn of the loop (the ballots want whole waves); a lane past the end counts nothing.
       A lane's 32-bit counters cannot wrap: an image has fewer than 2^31 pixels */
    for (long long base = (long long)blockIdx.x * VCM_DISP_BLOCK; base < n; base += G) {
        const long long p = base + threadIdx.x;
        const bool in = p < n;
        int second = -1, slot = 0;
        if (in) slot = disp_counter(disp_luminance(disp_load(src, channels, p, scale)), second);
        disp_count(mine, slot, in);
        disp_count(mine, second, in && second >= 0);
    }
    __syncthreads();
    for (int i = (int)threadIdx.x; i < VCM_DISP_LDS_COUNTERS; i += VCM_DISP_BLOCK) {
        unsigned long long s = 0ull;
        for (int w = 0; w < VCM_DISP_WAVES; w++) s += (unsigned long long)h[w][i];
        if (s) atomicAdd(&counters[i], s);
    }
}

/* the clipped channels of a workgroup's lanes -> one 64-bit atomic addition per workgroup */
static __device__ inline void disp_add_clipped(unsigned clipped, unsigned long long *counters)
{
    __shared__ unsigned sClipped;
    if (threadIdx.x == 0) sClipped = 0u;
    __syncthreads();
    for (int off = 32; off > 0; off >>= 1) clipped += __shfl_down(clipped, off);
    if ((threadIdx.x & 63) == 0 && clipped) atomicAdd(&sClipped, clipped);
    __syncthreads();
    if (threadIdx.x == 0 && sClipped) atomicAdd(&counters[VCM_DISP_CLIPPED], (unsigned long long)sClipped);
}

struct DispFinish { int curve, transfer; float whitePoint, invGamma; };

/* steps 1, 3, 4 without bloom */
__global__ void __launch_bounds__(VCM_DISP_BLOCK)
k_disp_finish(long long n, const float *__restrict__ src, int channels, float scale, float mult, DispFinish f, F4 *__restrict__ out,
              unsigned long long *__restrict__ counters)
{
    unsigned clipped = 0u;
    const long long G = (long long)gridDim.x * VCM_DISP_BLOCK;
    for (long long p = (long long)blockIdx.x * VCM_DISP_BLOCK + threadIdx.x; p < n; p += G) {
        const V3 c = disp_load(src, channels, p, scale);
        int cl;
        out[p] = disp_finish(mk3(c.x * mult, c.y * mult, c.z * mult), f.curve, f.whitePoint, f.transfer, f.invGamma, cl);
        clipped += (unsigned)cl;
    }
    disp_add_clipped(clipped, counters);
}

/* D_1 from the source image: level 0 is E, never stored */
__global__ void __launch_bounds__(VCM_DISP_BLOCK)
k_disp_down0(int ws, int hs, const float *__restrict__ src, int channels, float scale, float mult, int wd, int hd, F4 *__restrict__ dst)
{
    const long long n = (long long)wd * hd, G = (long long)gridDim.x * VCM_DISP_BLOCK;
    for (long long q = (long long)blockIdx.x * VCM_DISP_BLOCK + threadIdx.x; q < n; q += G) {
        const int x = (int)(q % wd), y = (int)(q / wd);
        dst[q] = disp_down(x, y, ws, hs, [&](int xs, int ys) { return disp_bloom_input(disp_load(src, channels, (long long)ys * ws + xs, scale), mult); });
    }
}

/* D_l from G_{l-1}, l >= 2 */
__global__ void __launch_bounds__(VCM_DISP_BLOCK)
k_disp_down(int ws, int hs, const F4 *__restrict__ srcL, int wd, int hd, F4 *__restrict__ dst)
{
    const long long n = (long long)wd * hd, G = (long long)gridDim.x * VCM_DISP_BLOCK;
    for (long long q = (long long)blockIdx.x * VCM_DISP_BLOCK + threadIdx.x; q < n; q += G) {
        const int x = (int)(q % wd), y = (int)(q / wd);
        dst[q] = disp_down(x, y, ws, hs, [&](int xs, int ys) { return srcL[(size_t)ys * ws + xs]; });
    }
}

/* one axis of the binomial blur: kRows ? along a row : along a column */
template <bool kRows>
__global__ void __launch_bounds__(VCM_DISP_BLOCK)
k_disp_blur(int w, int h, const F4 *__restrict__ srcL, F4 *__restrict__ dst)
{
    const long long n = (long long)w * h, G = (long long)gridDim.x * VCM_DISP_BLOCK;
    for (long long q = (long long)blockIdx.x * VCM_DISP_BLOCK + threadIdx.x; q < n; q += G) {
        const int x = (int)(q % w), y = (int)(q / w);
        if constexpr (kRows) dst[q] = disp_blur5(x, w, [&](int j) { return srcL[(size_t)y * w + j]; });
        else dst[q] = disp_blur5(y, h, [&](int j) { return srcL[(size_t)j * w + x]; });
    }
}

/* U_l = G_l + up(U_{l+1}), in place in G_l */
__global__ void __launch_bounds__(VCM_DISP_BLOCK)
k_disp_up_add(int w, int h, F4 *__restrict__ g, int ws, int hs, const F4 *__restrict__ upper)
{
    const long long n = (long long)w * h, G = (long long)gridDim.x * VCM_DISP_BLOCK;
    for (long long q = (long long)blockIdx.x * VCM_DISP_BLOCK + threadIdx.x; q < n; q += G) {
        const int x = (int)(q % w), y = (int)(q / w);
        g[q] = disp_add4(g[q], disp_up(x, y, ws, hs, [&](int xs, int ys) { return upper[(size_t)ys * ws + xs]; }));
    }
}

/* steps 1-4 with bloom: (1 - s) E + s up(U_1) / L, curve, transfer */
__global__ void __launch_bounds__(VCM_DISP_BLOCK)
k_disp_finish_bloom(int w, int h, const float *__restrict__ src, int channels, float scale, float mult, DispFinish f, int w1, int h1,
                    const F4 *__restrict__ u1, float invLevels, float strength, F4 *__restrict__ out, unsigned long long *__restrict__ counters)
{
    unsigned clipped = 0u;
    const long long n = (long long)w * h, G = (long long)gridDim.x * VCM_DISP_BLOCK;
    for (long long p = (long long)blockIdx.x * VCM_DISP_BLOCK + threadIdx.x; p < n; p += G) {
        const int x = (int)(p % w), y = (int)(p / w);
        const F4 up1 = disp_up(x, y, w1, h1, [&](int xs, int ys) { return u1[(size_t)ys * w1 + xs]; });
        int cl;
        out[p] = disp_finish(disp_bloom_combine(disp_load(src, channels, p, scale), mult, up1, invLevels, strength), f.curve, f.whitePoint,
                             f.transfer, f.invGamma, cl);
        clipped += (unsigned)cl;
    }
    disp_add_clipped(clipped, counters);
}

__global__ void __launch_bounds__(VCM_DISP_BLOCK)
k_disp_encode(int resX, int resY, const F4 *__restrict__ img, int format, int dither, unsigned seed, unsigned char *__restrict__ out)
{
    const long long n = (long long)resX * resY, G = (long long)gridDim.x * VCM_DISP_BLOCK;
    for (long long p = (long long)blockIdx.x * VCM_DISP_BLOCK + threadIdx.x; p < n; p += G)
        disp_encode_pixel(img[p], (int)(p % resX), (int)(p / resX), resX, resY, format, dither, seed, out);
}

namespace vcm {

static std::atomic<int> g_dispMaxBlocks(VCM_DISP_DEFAULT_MAX_BLOCKS);
int disp_max_blocks() { return g_dispMaxBlocks.load(); }
void disp_set_max_blocks(int blocks) { g_dispMaxBlocks.store(blocks > 0 ? blocks : VCM_DISP_DEFAULT_MAX_BLOCKS); }

hipError_t disp_launch_histogram(long long n, const float *src, int channels, float scale, unsigned long long *counters, hipStream_t stream)
{
    const int blocks = disp_grid_blocks(n, disp_max_blocks());
    hipLaunchKernelGGL(k_disp_histogram, dim3(blocks), dim3(VCM_DISP_BLOCK), 0, stream, n, src, channels, scale, counters);
    return hipGetLastError();
}

hipError_t disp_launch_transform(int width, int height, const float *src, int channels, float scale, float mult, const vcm_display_params &p,
                                 F4 *scratch, F4 *out, unsigned long long *counters, hipStream_t stream)
{
    const long long n = (long long)width * height;
    const DispFinish f = { p.curve, p.transfer, p.whitePoint, 1.f / p.gamma };
    const dim3 block(VCM_DISP_BLOCK);
    if (!(p.bloomStrength > 0.f)) {
        hipLaunchKernelGGL(k_disp_finish, dim3(disp_grid_blocks(n, VCM_DISP_DEFAULT_MAX_BLOCKS)), block, 0, stream, n, src, channels, scale, mult, f, out, counters);
        return hipGetLastError();
    }
    const int L = p.bloomLevels;
    int w[VCM_DISP_MAX_LEVELS + 1], h[VCM_DISP_MAX_LEVELS + 1];
    F4 *g[VCM_DISP_MAX_LEVELS + 1];
    w[0] = width; h[0] = height; g[0] = NULL;
    F4 *next = scratch;
    for (int l = 1; l <= L; l++) { w[l] = disp_level_dim(w[l - 1]); h[l] = disp_level_dim(h[l - 1]); g[l] = next; next += (size_t)w[l] * h[l]; }
    F4 *d = next, *t = next + (size_t)w[1] * h[1];
    for (int l = 1; l <= L; l++) {
        const dim3 grid(disp_grid_blocks((long long)w[l] * h[l], VCM_DISP_DEFAULT_MAX_BLOCKS));
        if (l == 1) hipLaunchKernelGGL(k_disp_down0, grid, block, 0, stream, w[0], h[0], src, channels, scale, mult, w[1], h[1], d);
        else hipLaunchKernelGGL(k_disp_down, grid, block, 0, stream, w[l - 1], h[l - 1], (const F4 *)g[l - 1], w[l], h[l], d);
        hipLaunchKernelGGL(k_disp_blur<true>, grid, block, 0, stream, w[l], h[l], (const F4 *)d, t);
        hipLaunchKernelGGL(k_disp_blur<false>, grid, block, 0, stream, w[l], h[l], (const F4 *)t, g[l]);
    }
    for (int l = L - 1; l >= 1; l--)
        hipLaunchKernelGGL(k_disp_up_add, dim3(disp_grid_blocks((long long)w[l] * h[l], VCM_DISP_DEFAULT_MAX_BLOCKS)), block, 0, stream, w[l], h[l], g[l],
                           w[l + 1], h[l + 1], (const F4 *)g[l + 1]);
    hipLaunchKernelGGL(k_disp_finish_bloom, dim3(disp_grid_blocks(n, VCM_DISP_DEFAULT_MAX_BLOCKS)), block, 0, stream, width, height, src, channels, scale, mult,
                       f, w[1], h[1], (const F4 *)g[1], 1.f / (float)L, p.bloomStrength, out, counters);
    return hipGetLastError();
}

hipError_t disp_launch_encode(int width, int height, const F4 *img, int format, int dither, unsigned seed, unsigned char *out, hipStream_t stream)
{
    const long long n = (long long)width * height;
    hipLaunchKernelGGL(k_disp_encode, dim3(disp_grid_blocks(n, VCM_DISP_DEFAULT_MAX_BLOCKS)), dim3(VCM_DISP_BLOCK), 0, stream, width, height, img, format, dither,
                       seed, out);
    return hipGetLastError();
}

} // namespace vcm
