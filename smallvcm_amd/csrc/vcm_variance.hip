// vcm_variance.hip -- the kernels of the per-pixel variance and of the noise statistic (vcm_variance.h holds what a lane
// computes and the order in which lanes are combined).  A translation unit of its own: no kernel of vcm_api.hip or
// vcm_denoise.hip is recompiled differently because these exist.
//
//   k_var_update    a pure stream, 76 B per pixel: three 4-byte loads of the sum image (a wave's 64 x 12 B are one
//                   contiguous 768-byte run), one 16-byte load and one 16-byte store for each of prev and mom
//   k_var_stats     every lane sums its pixels in index order in binary64, the workgroup combines its 256 lanes through
//                   LDS by var_tree_step, one VarAcc per workgroup goes to `partials`
//   k_var_stats2    ONE workgroup: lane l sums the partials l, l + 256, ... and the same tree gives the image's VarAcc
// No floating-point atomics anywhere: the same grid (var_grid_blocks) gives the same bits on every run.
#include <hip/hip_runtime.h>
#include <atomic>
#include "vcm_variance.h"

using namespace vcm;

__global__ void __launch_bounds__(VCM_VAR_BLOCK)
k_var_update(long long n, const float *__restrict__ sum3, int k, float km1, float kf, F4 *__restrict__ prev, F4 *__restrict__ mom)
{
    const long long G = (long long)gridDim.x * VCM_VAR_BLOCK;
    for (long long p = (long long)blockIdx.x * VCM_VAR_BLOCK + threadIdx.x; p < n; p += G) {
        const float sr = sum3[(size_t)p * 3], sg = sum3[(size_t)p * 3 + 1], sb = sum3[(size_t)p * 3 + 2];
        F4 pv = prev[p], m = mom[p];
        var_update_pixel(sr, sg, sb, k, km1, kf, pv, m);
        prev[p] = pv;
        mom[p] = m;
    }
}

__global__ void __launch_bounds__(VCM_VAR_BLOCK)
k_var_stats(long long n, const F4 *__restrict__ prev, const F4 *__restrict__ mom, float kf, float kk, float threshold,
            VarAcc *__restrict__ partials)
{
    __shared__ VarAcc v[VCM_VAR_BLOCK];
    const int lane = (int)threadIdx.x;
    v[lane] = var_lane_sum(n, (int)gridDim.x, (int)blockIdx.x, lane, kf, kk, threshold,
                           [&](long long p, F4 &pv, F4 &m) { pv = prev[p]; m = mom[p]; });
    var_block_tree(v, lane);
    if (lane == 0) partials[blockIdx.x] = v[0];
}

__global__ void __launch_bounds__(VCM_VAR_BLOCK)
k_var_stats2(const VarAcc *__restrict__ partials, int blocks, VarAcc *__restrict__ result)
{
    __shared__ VarAcc v[VCM_VAR_BLOCK];
    const int lane = (int)threadIdx.x;
    v[lane] = var_lane_sum_partials(partials, blocks, lane);
    var_block_tree(v, lane);
    if (lane == 0) *result = v[0];
}

__global__ void __launch_bounds__(VCM_VAR_BLOCK)
k_var_read(long long n, const F4 *__restrict__ mom, float kk, float *__restrict__ out3)
{
    const long long G = (long long)gridDim.x * VCM_VAR_BLOCK;
    for (long long p = (long long)blockIdx.x * VCM_VAR_BLOCK + threadIdx.x; p < n; p += G) {
        const F4 m = mom[p];
        out3[(size_t)p * 3] = var_of_mean(m.x, kk);
        out3[(size_t)p * 3 + 1] = var_of_mean(m.y, kk);
        out3[(size_t)p * 3 + 2] = var_of_mean(m.z, kk);
    }
}

namespace vcm {

static std::atomic<int> g_varMaxBlocks(VCM_VAR_DEFAULT_MAX_BLOCKS);
int var_max_blocks() { return g_varMaxBlocks.load(); }
void var_set_max_blocks(int blocks) { g_varMaxBlocks.store(blocks > 0 ? blocks : VCM_VAR_DEFAULT_MAX_BLOCKS); }

hipError_t var_launch_update(long long n, const float *sum3, int k, F4 *prev, F4 *mom, hipStream_t stream)
{
    const int blocks = var_grid_blocks(n, var_max_blocks());
    hipLaunchKernelGGL(k_var_update, dim3(blocks), dim3(VCM_VAR_BLOCK), 0, stream, n, sum3, k, (float)(k - 1), (float)k, prev, mom);
    return hipGetLastError();
}

hipError_t var_launch_stats(long long n, const F4 *prev, const F4 *mom, int k, float threshold, int maxBlocks, VarAcc *partials,
                            VarAcc *result, hipStream_t stream)
{
    const int blocks = var_grid_blocks(n, maxBlocks);
    const float kf = (float)k, kk = (float)((double)k * (double)(k - 1));
    hipLaunchKernelGGL(k_var_stats, dim3(blocks), dim3(VCM_VAR_BLOCK), 0, stream, n, prev, mom, kf, kk, threshold, partials);
    hipLaunchKernelGGL(k_var_stats2, dim3(1), dim3(VCM_VAR_BLOCK), 0, stream, (const VarAcc *)partials, blocks, result);
    return hipGetLastError();
}

hipError_t var_launch_read(long long n, const F4 *mom, int k, float *out3, hipStream_t stream)
{
    const int blocks = var_grid_blocks(n, var_max_blocks());
    hipLaunchKernelGGL(k_var_read, dim3(blocks), dim3(VCM_VAR_BLOCK), 0, stream, n, mom, (float)((double)k * (double)(k - 1)), out3);
    return hipGetLastError();
}

} // namespace vcm
