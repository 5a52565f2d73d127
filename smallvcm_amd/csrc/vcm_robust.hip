// vcm_robust.hip -- the kernels of the firefly-robust estimate (vcm_robust.h holds what a lane computes, vcm_variance.h
// the order in which lanes are combined).  A translation unit of its own: no kernel of vcm_api.hip, vcm_denoise.hip or
// vcm_variance.hip is recompiled differently because these exist.
//
//   k_robust_update      a pure stream, 76 B per pixel: three 4-byte loads of the sum image (a wave's 64 x 12 B are one
//                        contiguous 768-byte run), one 16-byte load and one 16-byte store for each of prev and the ONE
//                        bucket plane the iteration adds to
//   k_robust_resolve<M>  M coalesced 16-byte loads (one per plane) and one 16-byte store per pixel; the ranking is M^2
//                        unrolled comparisons on registers: no LDS, no scratch.  prev is read only by a pixel whose
//                        every bucket is non-finite
//   k_robust_stats<M>    every lane resolves its pixels in index order and sums what the rule decided in binary64, the
//                        workgroup combines its 256 lanes through LDS by var_tree_step, one VarAcc per workgroup
//   k_robust_stats2      ONE workgroup: lane l sums the partials l, l + 256, ... and the same tree gives the image's VarAcc
// No floating-point atomics anywhere: the same grid (var_grid_blocks) gives the same bits on every run.
#include <hip/hip_runtime.h>
#include "vcm_robust.h"

using namespace vcm;

__global__ void __launch_bounds__(VCM_VAR_BLOCK)
k_robust_update(long long n, const float *__restrict__ sum3, F4 *__restrict__ prev, F4 *__restrict__ bucket)
{
    const long long G = (long long)gridDim.x * VCM_VAR_BLOCK;
    for (long long p = (long long)blockIdx.x * VCM_VAR_BLOCK + threadIdx.x; p < n; p += G) {
        const float sr = sum3[(size_t)p * 3], sg = sum3[(size_t)p * 3 + 1], sb = sum3[(size_t)p * 3 + 2];
        F4 pv = prev[p], b = bucket[p];
        robust_update_pixel(sr, sg, sb, pv, b);
        prev[p] = pv;
        bucket[p] = b;
    }
}

template <int M>
__global__ void __launch_bounds__(VCM_VAR_BLOCK)
k_robust_resolve(long long n, const F4 *__restrict__ prev, const F4 *__restrict__ buckets, int k, F4 *__restrict__ out)
{
    const long long G = (long long)gridDim.x * VCM_VAR_BLOCK;
    for (long long p = (long long)blockIdx.x * VCM_VAR_BLOCK + threadIdx.x; p < n; p += G) {
        RobustInfo info;
        out[p] = robust_resolve_pixel<M>(k, [&](int j) { return buckets[(size_t)j * (size_t)n + (size_t)p]; },
                                         [&]() { return prev[p]; }, info);
    }
}

template <int M>
__global__ void __launch_bounds__(VCM_VAR_BLOCK)
k_robust_stats(long long n, const F4 *__restrict__ prev, const F4 *__restrict__ buckets, int k, VarAcc *__restrict__ partials)
{
    __shared__ VarAcc v[VCM_VAR_BLOCK];
    const int lane = (int)threadIdx.x;
    v[lane] = robust_lane_sum<M>(n, (int)gridDim.x, (int)blockIdx.x, lane, k,
                                 [&](long long p, int j) { return buckets[(size_t)j * (size_t)n + (size_t)p]; },
                                 [&](long long p) { return prev[p]; });
    var_block_tree(v, lane);
    if (lane == 0) partials[blockIdx.x] = v[0];
}

__global__ void __launch_bounds__(VCM_VAR_BLOCK)
k_robust_stats2(const VarAcc *__restrict__ partials, int blocks, VarAcc *__restrict__ result)
{
    __shared__ VarAcc v[VCM_VAR_BLOCK];
    const int lane = (int)threadIdx.x;
    v[lane] = var_lane_sum_partials(partials, blocks, lane);
    var_block_tree(v, lane);
    if (lane == 0) *result = v[0];
}

namespace vcm {

hipError_t robust_launch_update(long long n, const float *sum3, int k, int M, F4 *prev, F4 *buckets, hipStream_t stream)
{
    const int blocks = var_grid_blocks(n, var_max_blocks());
    hipLaunchKernelGGL(k_robust_update, dim3(blocks), dim3(VCM_VAR_BLOCK), 0, stream, n, sum3, prev,
                       buckets + (size_t)robust_bucket_of(k, M) * (size_t)n);
    return hipGetLastError();
}

hipError_t robust_launch_resolve(long long n, const F4 *prev, const F4 *buckets, int k, int M, F4 *out, hipStream_t stream)
{
    const int blocks = var_grid_blocks(n, var_max_blocks());
#define VCM_ROBUST_RESOLVE(m) hipLaunchKernelGGL(k_robust_resolve<m>, dim3(blocks), dim3(VCM_VAR_BLOCK), 0, stream, n, prev, buckets, k, out)
    VCM_ROBUST_DISPATCH(M, VCM_ROBUST_RESOLVE)
#undef VCM_ROBUST_RESOLVE
    return hipGetLastError();
}

hipError_t robust_launch_stats(long long n, const F4 *prev, const F4 *buckets, int k, int M, int maxBlocks, VarAcc *partials,
                               VarAcc *result, hipStream_t stream)
{
    const int blocks = var_grid_blocks(n, maxBlocks);
#define VCM_ROBUST_STATS(m) hipLaunchKernelGGL(k_robust_stats<m>, dim3(blocks), dim3(VCM_VAR_BLOCK), 0, stream, n, prev, buckets, k, partials)
    VCM_ROBUST_DISPATCH(M, VCM_ROBUST_STATS)
#undef VCM_ROBUST_STATS
    hipLaunchKernelGGL(k_robust_stats2, dim3(1), dim3(VCM_VAR_BLOCK), 0, stream, (const VarAcc *)partials, blocks, result);
    return hipGetLastError();
}

} // namespace vcm
