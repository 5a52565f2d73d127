// vcm_parts.hip -- the kernels of the technique breakdown (vcm_parts.h holds what a lane computes and the order in which
// lanes are combined).  A translation unit of its own: no kernel of vcm_api.hip is recompiled differently because these
// exist, and a context that does not track launches none of them.
//
//   k_resolve_parts  one lane per pixel, behind the iteration's k_resolve: the addends k_resolve has just summed, read
//                    again from the camera-vertex store and added to four planes instead of one colour, 4 x 3
//                    accumulators in registers.  Latency-bound like k_resolve (per vertex the meta / diOut / mergeOut
//                    loads go out together, the vcOut loads in batches of 4); no atomics; a wave's 64 x 12 B of a plane
//                    are one contiguous 768-byte run; the grid is k_resolve's.
//   k_parts_stats    every lane sums the luminances of its pixels in index order in binary64, the workgroup combines its
//                    256 lanes through LDS by parts_tree_step, one PartsAcc per workgroup goes to `partials`
//   k_parts_stats2   ONE workgroup: lane l sums the partials l, l + 256, ... and the same tree gives the image's PartsAcc
//   k_part_read3/4   plane * scale as 3 floats or as { rgb, 1 } per pixel
// The LIGHT_TRACE plane needs no kernel of its own: a tracked context launches k_splat_apply / k_splat_apply_long a second
// time over the iteration's splat lists with the plane in the framebuffer's place (vcm_api.hip flush_light_splats).
// No floating-point atomics anywhere: the same grid (parts_grid_blocks) gives the same bits on every run.
#include <hip/hip_runtime.h>
#include <atomic>
#undef VCM_REGION_CLOCK   /* (a measurement build's clock table belongs to vcm_api.hip) */
#include "vcm_parts.h"

using namespace vcm;

__global__ void __launch_bounds__(VCM_PARTS_BLOCK)
k_resolve_parts(IterParams P, const F4 *__restrict__ camOut, const uint32_t *__restrict__ camMask, VertexStore vs, float *parts,
                size_t planeStride)
{
    const int lastQ = min(P.N, P.p0 + P.nLocal + P.resX + 1);
    for (int q = P.p0 + blockIdx.x * blockDim.x + threadIdx.x; q < lastQ; q += gridDim.x * blockDim.x)
        parts_resolve_pixel(P, camOut, camMask, vs, q, parts, planeStride);
}

/* the tree over the LDS slots of a workgroup; v[0] holds the result for lane 0 afterwards */
__device__ inline void parts_block_tree(PartsAcc *v, int lane)
{
    __syncthreads();
    for (int s = 0; s < VCM_PARTS_TREE_STEPS; s++) {
        parts_tree_step(v, s, lane);
        __syncthreads();
    }
}

__global__ void __launch_bounds__(VCM_PARTS_BLOCK)
k_parts_stats(long long n, const float *__restrict__ parts, size_t planeStride, PartsAcc *__restrict__ partials)
{
    __shared__ PartsAcc v[VCM_PARTS_BLOCK];
    const int lane = (int)threadIdx.x;
    v[lane] = parts_lane_sum(n, (int)gridDim.x, (int)blockIdx.x, lane, parts, planeStride);
    parts_block_tree(v, lane);
    if (lane == 0) partials[blockIdx.x] = v[0];
}

__global__ void __launch_bounds__(VCM_PARTS_BLOCK)
k_parts_stats2(const PartsAcc *__restrict__ partials, int blocks, PartsAcc *__restrict__ result)
{
    __shared__ PartsAcc v[VCM_PARTS_BLOCK];
    const int lane = (int)threadIdx.x;
    v[lane] = parts_lane_sum_partials(partials, blocks, lane);
    parts_block_tree(v, lane);
    if (lane == 0) *result = v[0];
}

__global__ void __launch_bounds__(VCM_PARTS_BLOCK)
k_part_read3(long long n3, const float *__restrict__ plane, float scale, float *__restrict__ out3)
{
    const long long G = (long long)gridDim.x * VCM_PARTS_BLOCK;
    for (long long i = (long long)blockIdx.x * VCM_PARTS_BLOCK + threadIdx.x; i < n3; i += G) out3[i] = plane[i] * scale;
}

__global__ void __launch_bounds__(VCM_PARTS_BLOCK)
k_part_read4(long long n, const float *__restrict__ plane, float scale, F4 *__restrict__ out4)
{
    const long long G = (long long)gridDim.x * VCM_PARTS_BLOCK;
    for (long long p = (long long)blockIdx.x * VCM_PARTS_BLOCK + threadIdx.x; p < n; p += G)
        out4[p] = mk4(plane[(size_t)p * 3] * scale, plane[(size_t)p * 3 + 1] * scale, plane[(size_t)p * 3 + 2] * scale, 1.f);
}

namespace vcm {

static std::atomic<int> g_partsMaxBlocks(VCM_PARTS_DEFAULT_MAX_BLOCKS);
int parts_max_blocks() { return g_partsMaxBlocks.load(); }
void parts_set_max_blocks(int blocks) { g_partsMaxBlocks.store(blocks > 0 ? blocks : VCM_PARTS_DEFAULT_MAX_BLOCKS); }

hipError_t parts_launch_resolve(const IterParams &P, const F4 *camOut, const uint32_t *camMask, const VertexStore &vs, float *parts,
                                size_t planeStride, int blocks, hipStream_t stream)
{
    const int cap = parts_max_blocks();
    if (blocks > cap) blocks = cap;
    hipLaunchKernelGGL(k_resolve_parts, dim3(blocks < 1 ? 1 : blocks), dim3(VCM_PARTS_BLOCK), 0, stream, P, camOut, camMask, vs, parts,
                       planeStride);
    return hipGetLastError();
}

hipError_t parts_launch_stats(long long n, const float *parts, size_t planeStride, int maxBlocks, PartsAcc *partials, PartsAcc *result,
                              hipStream_t stream)
{
    const int blocks = parts_grid_blocks(n, maxBlocks);
    hipLaunchKernelGGL(k_parts_stats, dim3(blocks), dim3(VCM_PARTS_BLOCK), 0, stream, n, parts, planeStride, partials);
    hipLaunchKernelGGL(k_parts_stats2, dim3(1), dim3(VCM_PARTS_BLOCK), 0, stream, (const PartsAcc *)partials, blocks, result);
    return hipGetLastError();
}

hipError_t parts_launch_read3(long long n, const float *plane, float scale, float *out3, hipStream_t stream)
{
    const int blocks = parts_grid_blocks(n * 3, parts_max_blocks());
    hipLaunchKernelGGL(k_part_read3, dim3(blocks), dim3(VCM_PARTS_BLOCK), 0, stream, n * 3, plane, scale, out3);
    return hipGetLastError();
}

hipError_t parts_launch_read4(long long n, const float *plane, float scale, F4 *out4, hipStream_t stream)
{
    const int blocks = parts_grid_blocks(n, parts_max_blocks());
    hipLaunchKernelGGL(k_part_read4, dim3(blocks), dim3(VCM_PARTS_BLOCK), 0, stream, n, plane, scale, out4);
    return hipGetLastError();
}

} // namespace vcm
