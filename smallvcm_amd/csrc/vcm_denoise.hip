// vcm_denoise.hip -- the kernels of the feature buffers and of the a-trous filter (vcm_denoise.h holds what a lane
// computes).  A translation unit of its own: no kernel of vcm_api.hip is recompiled differently because these exist.
//
// Shape of the filter kernel.  A workgroup of 256 lanes owns a tile of 32 x 8 pixels: a wave is two rows of 32 pixels,
// every tap of a wave two coalesced 512-byte row segments of 16-byte loads.
//   step 1, 2   the tile and its halo of 2 * step pixels (at most 40 x 16) of BOTH images are staged in LDS once
//               (2 x 10 KB) and the 25 taps are ds_read_b128 of consecutive 16-byte slots: reuse through LDS.
//   step >= 4   a lane's taps are far apart, neighbouring lanes' taps stay contiguous: the taps are global 16-byte loads
//               and the reuse (25 reads of every pixel by 25 different workgroups) is left to L2.
#include <hip/hip_runtime.h>
#include "vcm_denoise.h"

using namespace vcm;

#define VCM_DN_TILE_X 32
#define VCM_DN_TILE_Y 8
#define VCM_DN_MAX_HALO 4
#define VCM_DN_LDS_X (VCM_DN_TILE_X + 2 * VCM_DN_MAX_HALO)
#define VCM_DN_LDS_Y (VCM_DN_TILE_Y + 2 * VCM_DN_MAX_HALO)

template <class SC>
__global__ void __launch_bounds__(256)
k_features(const DScene *__restrict__ scp, int resX, int p0, int nLocal, F4 *__restrict__ guide, F4 *__restrict__ albedo)
{
    const SC &sc = *static_cast<const SC *>(scp);
    stage_scene_tables(sc);   /* before any thread leaves: it holds a barrier */
    for (int lp = blockIdx.x * blockDim.x + threadIdx.x; lp < nLocal; lp += gridDim.x * blockDim.x) {
        F4 g, a;
        feature_pixel(sc, resX, p0 + lp, g, a);
        guide[p0 + lp] = g;
        albedo[p0 + lp] = a;
    }
}

/* colour (three floats per pixel, or a float4 image) * scale, demodulated: the first pass's input */
__global__ void __launch_bounds__(256)
k_dn_prepare(int n, const F4 *__restrict__ color, const float *__restrict__ fb3, float scale, const F4 *__restrict__ albedo,
             int demodulate, F4 *__restrict__ out)
{
    for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < n; p += gridDim.x * blockDim.x) {
        float r, g, b;
        if (fb3) { r = fb3[(size_t)p * 3]; g = fb3[(size_t)p * 3 + 1]; b = fb3[(size_t)p * 3 + 2]; }
        else { const F4 c = color[p]; r = c.x; g = c.y; b = c.z; }
        F4 a = mk4(1.f, 1.f, 1.f, 1.f);
        if (demodulate) a = albedo[p];
        out[p] = dn_prepare(r, g, b, scale, a, demodulate);
    }
}

/* nComp components of a float4 image, from comp0 on, as a dense float image (read-back) */
__global__ void __launch_bounds__(256)
k_dn_unpack(int n, const F4 *__restrict__ src, int comp0, int nComp, float *__restrict__ dst)
{
    for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < n; p += gridDim.x * blockDim.x) {
        const F4 v = src[p];
        const float c[4] = { v.x, v.y, v.z, v.w };
        for (int k = 0; k < nComp; k++) dst[(size_t)p * nComp + k] = (comp0 + k == 0) ? c[0] : (comp0 + k == 1) ? c[1] : (comp0 + k == 2) ? c[2] : c[3];
    }
}

template <bool kLds>
__global__ void __launch_bounds__(256)
k_atrous(DnPass P, const F4 *__restrict__ color, const F4 *__restrict__ guide, const F4 *__restrict__ albedo, F4 *__restrict__ out)
{
    const int tx = (int)threadIdx.x % VCM_DN_TILE_X, ty = (int)threadIdx.x / VCM_DN_TILE_X;
    const int x0 = (int)blockIdx.x * VCM_DN_TILE_X, y0 = (int)blockIdx.y * VCM_DN_TILE_Y;
    const int x = x0 + tx, y = y0 + ty;
    const bool inside = x < P.resX && y < P.resY;
    if constexpr (kLds) {
        __shared__ F4 sC[VCM_DN_LDS_X * VCM_DN_LDS_Y], sG[VCM_DN_LDS_X * VCM_DN_LDS_Y];
        const int halo = 2 * P.step;   /* <= VCM_DN_MAX_HALO: the launch picks this kernel for steps 1 and 2 only */
        const int w = VCM_DN_TILE_X + 2 * halo, h = VCM_DN_TILE_Y + 2 * halo;
        for (int i = (int)threadIdx.x; i < w * h; i += 256) {
            const int lx = i % w, ly = i / w;
            const int gx = x0 - halo + lx, gy = y0 - halo + ly;
            if (gx >= 0 && gx < P.resX && gy >= 0 && gy < P.resY) {   /* what lies outside is never read: dn_filter_pixel skips it */
                const size_t q = (size_t)gy * P.resX + gx;
                sC[ly * VCM_DN_LDS_X + lx] = color[q];
                sG[ly * VCM_DN_LDS_X + lx] = guide[q];
            }
        }
        __syncthreads();
        if (!inside) return;
        F4 a = mk4(1.f, 1.f, 1.f, 1.f);
        if (P.remodulate) a = albedo[(size_t)y * P.resX + x];
        out[(size_t)y * P.resX + x] = dn_filter_pixel(P, x, y, a, [&](int xq, int yq, F4 &cq, F4 &gq) {
            const int s = (yq - y0 + halo) * VCM_DN_LDS_X + (xq - x0 + halo);
            cq = sC[s]; gq = sG[s];
        });
    } else {
        if (!inside) return;
        F4 a = mk4(1.f, 1.f, 1.f, 1.f);
        if (P.remodulate) a = albedo[(size_t)y * P.resX + x];
        out[(size_t)y * P.resX + x] = dn_filter_pixel(P, x, y, a, [&](int xq, int yq, F4 &cq, F4 &gq) {
            const size_t q = (size_t)yq * P.resX + xq;
            cq = color[q]; gq = guide[q];
        });
    }
}

/* colour and its variance (dn_prepare2): the first guided pass's input */
__global__ void __launch_bounds__(256)
k_dn_prepare_var(int n, const F4 *__restrict__ color, const float *__restrict__ fb3, float scale, const F4 *__restrict__ albedo,
                 int demodulate, const F4 *__restrict__ mom, float varFactor, F4 *__restrict__ out)
{
    for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < n; p += gridDim.x * blockDim.x) {
        float r, g, b;
        if (fb3) { r = fb3[(size_t)p * 3]; g = fb3[(size_t)p * 3 + 1]; b = fb3[(size_t)p * 3 + 2]; }
        else { const F4 c = color[p]; r = c.x; g = c.y; b = c.z; }
        F4 a = mk4(1.f, 1.f, 1.f, 1.f);
        if (demodulate) a = albedo[p];
        out[p] = dn_prepare2(r, g, b, scale, a, demodulate, mom[p], varFactor);
    }
}

/* k_atrous with the variance-guided colour stop (dn_filter_pixel2): a sibling, so that k_atrous itself compiles as before.
   steps 1, 2: the 3 x 3 of the centre's variance lies inside the staged tile (halo >= 2); steps >= 4: nine more global loads */
template <bool kLds>
__global__ void __launch_bounds__(256)
k_atrous_var(DnPass2 P2, const F4 *__restrict__ color, const F4 *__restrict__ guide, const F4 *__restrict__ albedo, F4 *__restrict__ out)
{
    const DnPass &P = P2.p;
    const int tx = (int)threadIdx.x % VCM_DN_TILE_X, ty = (int)threadIdx.x / VCM_DN_TILE_X;
    const int x0 = (int)blockIdx.x * VCM_DN_TILE_X, y0 = (int)blockIdx.y * VCM_DN_TILE_Y;
    const int x = x0 + tx, y = y0 + ty;
    const bool inside = x < P.resX && y < P.resY;
    if constexpr (kLds) {
        __shared__ F4 sC[VCM_DN_LDS_X * VCM_DN_LDS_Y], sG[VCM_DN_LDS_X * VCM_DN_LDS_Y];
        const int halo = 2 * P.step;   /* 2 or 4: the launch picks this kernel for steps 1 and 2 only */
        const int w = VCM_DN_TILE_X + 2 * halo, h = VCM_DN_TILE_Y + 2 * halo;
        for (int i = (int)threadIdx.x; i < w * h; i += 256) {
            const int lx = i % w, ly = i / w;
            const int gx = x0 - halo + lx, gy = y0 - halo + ly;
            if (gx >= 0 && gx < P.resX && gy >= 0 && gy < P.resY) {
                const size_t q = (size_t)gy * P.resX + gx;
                sC[ly * VCM_DN_LDS_X + lx] = color[q];
                sG[ly * VCM_DN_LDS_X + lx] = guide[q];
            }
        }
        __syncthreads();
        if (!inside) return;
        F4 a = mk4(1.f, 1.f, 1.f, 1.f);
        if (P.remodulate) a = albedo[(size_t)y * P.resX + x];
        out[(size_t)y * P.resX + x] = dn_filter_pixel2(P2, x, y, a, [&](int xq, int yq, F4 &cq, F4 &gq) {
            const int s = (yq - y0 + halo) * VCM_DN_LDS_X + (xq - x0 + halo);
            cq = sC[s]; gq = sG[s];
        });
    } else {
        if (!inside) return;
        F4 a = mk4(1.f, 1.f, 1.f, 1.f);
        if (P.remodulate) a = albedo[(size_t)y * P.resX + x];
        out[(size_t)y * P.resX + x] = dn_filter_pixel2(P2, x, y, a, [&](int xq, int yq, F4 &cq, F4 &gq) {
            const size_t q = (size_t)yq * P.resX + xq;
            cq = color[q]; gq = guide[q];
        });
    }
}

namespace vcm {

hipError_t dn_launch_features(const DScene *dScene, SceneKind kind, bool ggx, bool proj, int resX, int p0, int nLocal, F4 *guide, F4 *albedo,
                              hipStream_t stream)
{
    int blocks = (nLocal + 255) / 256;
    blocks = blocks < 1 ? 1 : (blocks > 4096 ? 4096 : blocks);
    if (proj) {   /* a fisheye or a panorama: the WithLens forms, WithLens<S> and WithGgx<WithLens<S>>, which hold the projection */
        with_scene_kind<kWrapLens | kWrapGgx>(kind, SceneWrappers{ true, false, false, false, ggx }, [&](auto tag) {
            using S = typename decltype(tag)::type;
            hipLaunchKernelGGL((k_features<S>), dim3(blocks), dim3(256), 0, stream, dScene, resX, p0, nLocal, guide, albedo);
        });
        return hipGetLastError();
    }
    with_scene_kind<kWrapGgx>(kind, SceneWrappers{ false, false, false, false, ggx }, [&](auto tag) {   /* one more form per kind: WithGgx<S> */
        using S = typename decltype(tag)::type;
        hipLaunchKernelGGL((k_features<S>), dim3(blocks), dim3(256), 0, stream, dScene, resX, p0, nLocal, guide, albedo);
    });
    return hipGetLastError();
}

hipError_t dn_launch_unpack(int n, const F4 *src, int comp0, int nComp, float *dst, hipStream_t stream)
{
    int blocks = (n + 255) / 256;
    blocks = blocks > 2048 ? 2048 : blocks;
    hipLaunchKernelGGL(k_dn_unpack, dim3(blocks), dim3(256), 0, stream, n, src, comp0, nComp, dst);
    return hipGetLastError();
}

hipError_t dn_launch_denoise(int resX, int resY, const F4 *color, const float *fb3, float scale, const F4 *albedo,
                             const F4 *guide, F4 *out, F4 *tmpA, F4 *tmpB, const vcm_denoise_params &p, hipStream_t stream)
{
    const long long n = (long long)resX * resY;
    int blocks = (int)((n + 255) / 256);
    blocks = blocks > 2048 ? 2048 : blocks;
    if (p.passes == 0) {   /* the input itself (no demodulation: it would not give the same bits back) */
        if (!fb3) return hipMemcpyAsync(out, color, (size_t)n * sizeof(F4), hipMemcpyDeviceToDevice, stream);
        hipLaunchKernelGGL(k_dn_prepare, dim3(blocks), dim3(256), 0, stream, (int)n, color, fb3, scale, albedo, 0, out);
        return hipGetLastError();
    }
    const F4 *src = color;
    if (fb3 || p.demodulate) {
        hipLaunchKernelGGL(k_dn_prepare, dim3(blocks), dim3(256), 0, stream, (int)n, color, fb3, scale, albedo, p.demodulate ? 1 : 0, tmpA);
        src = tmpA;
    }
    const dim3 grid((unsigned)((resX + VCM_DN_TILE_X - 1) / VCM_DN_TILE_X), (unsigned)((resY + VCM_DN_TILE_Y - 1) / VCM_DN_TILE_Y));
    for (int i = 0; i < p.passes; i++) {
        const DnPass P = dn_pass(p, resX, resY, i);
        F4 *dst = (i == p.passes - 1) ? out : (src == tmpA ? tmpB : tmpA);
        if (2 * P.step <= VCM_DN_MAX_HALO) hipLaunchKernelGGL(k_atrous<true>, grid, dim3(256), 0, stream, P, src, guide, albedo, dst);
        else hipLaunchKernelGGL(k_atrous<false>, grid, dim3(256), 0, stream, P, src, guide, albedo, dst);
        src = dst;
    }
    return hipGetLastError();
}

hipError_t dn_launch_denoise2(int resX, int resY, const F4 *color, const float *fb3, float scale, const F4 *albedo,
                              const F4 *guide, const F4 *mom, float varFactor, F4 *out, F4 *tmpA, F4 *tmpB,
                              const vcm_denoise_params2 &p, hipStream_t stream)
{
    if (!p.varianceGuided || p.passes == 0)   /* the fixed stop, bit for bit; no pass: the input itself */
        return dn_launch_denoise(resX, resY, color, fb3, scale, albedo, guide, out, tmpA, tmpB, dn_base_params(p), stream);
    const long long n = (long long)resX * resY;
    int blocks = (int)((n + 255) / 256);
    blocks = blocks > 2048 ? 2048 : blocks;
    hipLaunchKernelGGL(k_dn_prepare_var, dim3(blocks), dim3(256), 0, stream, (int)n, color, fb3, scale, albedo, p.demodulate ? 1 : 0, mom, varFactor, tmpA);
    const F4 *src = tmpA;
    const dim3 grid((unsigned)((resX + VCM_DN_TILE_X - 1) / VCM_DN_TILE_X), (unsigned)((resY + VCM_DN_TILE_Y - 1) / VCM_DN_TILE_Y));
    for (int i = 0; i < p.passes; i++) {
        const DnPass2 P = dn_pass2(p, resX, resY, i);
        F4 *dst = (i == p.passes - 1) ? out : (src == tmpA ? tmpB : tmpA);
        if (2 * P.p.step <= VCM_DN_MAX_HALO) hipLaunchKernelGGL(k_atrous_var<true>, grid, dim3(256), 0, stream, P, src, guide, albedo, dst);
        else hipLaunchKernelGGL(k_atrous_var<false>, grid, dim3(256), 0, stream, P, src, guide, albedo, dst);
        src = dst;
    }
    return hipGetLastError();
}

} // namespace vcm
