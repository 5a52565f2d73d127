// TEST INFRASTRUCTURE.  The host emulation of tests/host_emul_variance/emul_variance.cpp with the firefly-robust estimate of
// smallvcm_amd/csrc/vcm_robust.h: the functions the kernels of vcm_robust.hip run, compiled for the host and driven
// serially -- the lanes of the grid in a loop, the combination tree step by step -- for tests/test_robust.py and
// tests/test_gpu_robust.py.  Never built into libsmallvcm_amd.so.
#include "../host_emul_variance/emul_variance.cpp"
#include "../../smallvcm_amd/csrc/vcm_robust.h"

static const char *robust_refusal(int k, int M, bool resolving)
{
    if (!robust_buckets_ok(M)) return "buckets must be odd, 3 .. 15";
    if (k < 1) return "k counts the iterations from 1";
    if (resolving && k < M) return "the robust estimate needs at least as many iterations as buckets";
    return NULL;
}

template <int M>
static void resolve_all(long long n, const F4 *prev, const F4 *buckets, int k, F4 *out, float *gini, int *trim, int *kept)
{
    for (long long p = 0; p < n; p++) {
        RobustInfo info;
        out[p] = robust_resolve_pixel<M>(k, [&](int j) { return buckets[(size_t)j * (size_t)n + (size_t)p]; }, [&]() { return prev[p]; }, info);
        if (gini) gini[p] = info.gini;
        if (trim) trim[p] = info.trim;
        if (kept) kept[p] = info.kept;
    }
}

template <int M>
static VarAcc stats_all(long long n, const F4 *prev, const F4 *buckets, int k, int blocks)
{
    std::vector<VarAcc> partials((size_t)blocks), v(VCM_VAR_BLOCK);
    for (int b = 0; b < blocks; b++) {
        for (int lane = 0; lane < VCM_VAR_BLOCK; lane++)
            v[(size_t)lane] = robust_lane_sum<M>(n, blocks, b, lane, k, [&](long long p, int j) { return buckets[(size_t)j * (size_t)n + (size_t)p]; },
                                                 [&](long long p) { return prev[p]; });
        emul_block_tree(v.data());
        partials[(size_t)b] = v[0];
    }
    for (int lane = 0; lane < VCM_VAR_BLOCK; lane++) v[(size_t)lane] = var_lane_sum_partials(partials.data(), blocks, lane);
    emul_block_tree(v.data());
    return v[0];
}

extern "C" {

/* k_robust_update: iteration k (from 1) of the n-pixel float4 images prev, buckets [M][n] from the running sum sum3 */
int emul_robust_update(long long n, const float *sum3, int k, int M, float *prev, float *buckets)
{
    if (const char *why = robust_refusal(k, M, false)) { g_pickErr = why; return -1; }
    F4 *plane = (F4 *)buckets + (size_t)robust_bucket_of(k, M) * (size_t)n;
    for (long long p = 0; p < n; p++) robust_update_pixel(sum3[p * 3], sum3[p * 3 + 1], sum3[p * 3 + 2], ((F4 *)prev)[p], plane[p]);
    return 0;
}

/* k_robust_resolve<M>: out = n float4; gini, trim, kept (each n, or NULL) take what the rule decided per pixel */
int emul_robust_resolve(long long n, const float *prev, const float *buckets, int k, int M, float *out, float *gini, int *trim, int *kept)
{
    if (const char *why = robust_refusal(k, M, true)) { g_pickErr = why; return -1; }
    if ((const void *)out == (const void *)prev || (out + n * 4 > buckets && out < buckets + (size_t)M * n * 4)) { g_pickErr = "outDev is one of the inputs"; return -1; }
#define RESOLVE(m) resolve_all<m>(n, (const F4 *)prev, (const F4 *)buckets, k, (F4 *)out, gini, trim, kept)
    VCM_ROBUST_DISPATCH(M, RESOLVE)
#undef RESOLVE
    return 0;
}

/* k_robust_stats<M> + k_robust_stats2 with the grid var_grid_blocks(n, maxBlocks) */
int emul_robust_stats(long long n, const float *prev, const float *buckets, int k, int M, int maxBlocks, vcm_robust_stats *out)
{
    if (const char *why = robust_refusal(k, M, true)) { g_pickErr = why; return -1; }
    const int blocks = var_grid_blocks(n, maxBlocks);
    VarAcc a = var_acc_zero();
#define STATS(m) a = stats_all<m>(n, (const F4 *)prev, (const F4 *)buckets, k, blocks)
    VCM_ROBUST_DISPATCH(M, STATS)
#undef STATS
    robust_finish_stats(a, k, M, n, out);
    return 0;
}

int emul_robust_bucket_count(int k, int j, int M) { return robust_bucket_count(k, j, M); }

} // extern "C"
