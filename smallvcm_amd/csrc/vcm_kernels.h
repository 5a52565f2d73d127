// vcm_kernels.h -- HIP kernels of one VCM iteration on gfx950 (MI355X).
//
//   K1  k_light_trace     light sub-paths: trace, scattering, vertex store (80-byte slot records)
//   K1b scan + k_compact_records   mPathEnds; dense vertex -> slot list (+ the 52-byte merge records
//                         when they have to travel: sharded renderer, debug read-out)
//   K1c k_connect_camera  every stored vertex to the camera: BSDF, MIS, one shadow ray -> (rgb, pixel)
//   K1d pixel histogram / scan / k_splat_scatter / k_splat_apply
//                         the light splats added per pixel in the reference's order
//   K2  k_cell_keys / 3 x (k_radix_hist, scan, k_radix_scatter) / k_cell_starts / k_cell_rank_gather
//                         hash-grid build with vertices SORTED BY CELL (a stable radix sort; the reference's
//                         counting sort -- k_cell_count / scan / k_cell_scatter -- behind SMALLVCM_AMD_GRID_SORT=count)
//   K3  k_camera_trace    camera sub-paths: trace, emission, scattering; appends a
//                         record per non-delta vertex + its DI / VC tasks
//   K3b k_connect_di      direct illumination tasks (dense, one lane each)
//   K3c k_connect_vc      vertex connection tasks (dense, one lane each)
//   K4a k_query_count/scatter  counting sort of the camera vertices by the cell they lie in
//   K4  k_merge_pairs / k_merge_walk   range-merge: one lane per camera vertex scans, the accepted pairs evaluated 64 at a time
//   K5  k_resolve         replays every path's additions in the reference's order,
//                         Framebuffer::AddColor
//   PathTracer / EyeLight: k_path_trace, k_eye_light (+ K5)
//
// Execution model: one lane per sub-path.  K1/K3 are persistent: each wave
// owns a contiguous chunk of path indices and REFILLS lanes whose path ended
// with the next unstarted index, found with a wave ballot + prefix popcount
// (no atomics, no LDS) -- paths are independent because every path has its
// own counter-based random stream (philox.h).  The scene (<= 32 primitives)
// is read with wave-uniform indices, i.e. through scalar loads.
#ifndef SMALLVCM_AMD_VCM_KERNELS_H
#define SMALLVCM_AMD_VCM_KERNELS_H

#include <hip/hip_runtime.h>
#include "vcm_core.h"

namespace vcm {

enum { STAT_LIGHT_RAYS = 0, STAT_CAMERA_RAYS, STAT_SHADOW_RAYS, STAT_MERGE_QUERIES, STAT_MERGE_CANDIDATES,
       STAT_MERGE_ACCEPTED, STAT_CONNECTIONS, STAT_LIGHT_SPLATS, STAT_STORED, STAT_COUNT };

#define VCM_TRACE_BLOCK 256
#define VCM_WAVE 64

/* Phase stamps without launches of their own: a kernel that starts a phase gets the stamp slots that are pending
 * on its stream and writes the device's wall clock into them at entry (one lane).  Replaces a one-lane stamp kernel
 * plus a HIP event per mark, 13 per iteration: 1 % of an iteration at 2048^2, 6 % at 512^2. */
struct StampArgs { unsigned long long *p[4]; };
__device__ __forceinline__ void stamp_entry(const StampArgs &s)
{
    if (blockIdx.x == 0 && threadIdx.x == 0 && s.p[0]) {
        const unsigned long long t = wall_clock64();
#pragma unroll
        for (int k = 0; k < 4; k++) if (s.p[k]) *s.p[k] = t;
    }
}

__device__ __forceinline__ unsigned lane_id() { return __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)); }

__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ __forceinline__ void flush_stats(const LaneStats &ls, unsigned long long *g)
{
    const uint32_t v[STAT_COUNT] = { ls.lightRays, ls.cameraRays, ls.shadowRays, ls.mergeQueries, ls.mergeCandidates,
                                     ls.mergeAccepted, ls.connections, ls.lightSplats, ls.stored };
    /* per-lane counters are 32 bit; a lane sees < 2^32 events per launch, the
       wave sum is widened before it leaves the wave */
#pragma unroll
    for (int i = 0; i < STAT_COUNT; i++) {
        unsigned long long lo = wave_sum_u32(v[i] & 0xffffu);
        unsigned long long hi = wave_sum_u32(v[i] >> 16);
        const unsigned long long s = lo + (hi << 16);
        if (lane_id() == 0 && s) atomicAdd(&g[i], s);
    }
}

__device__ __forceinline__ uint32_t float_order_key(float f)
{   /* order-preserving float -> uint */
    const uint32_t u = f2u(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float float_from_order_key(uint32_t k)
{
    return u2f((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

/* Path indices for the persistent waves of K1 / K3.  A wave takes CHUNKS of `chunk` consecutive indices from a global
 * counter (one atomic per chunk, lane 0) and hands them to its dead lanes with ballot + prefix popcount; when the
 * chunk cannot serve every dead lane the rest comes out of the next one in the same step.  The first version gave
 * every wave ONE fixed range: the waves of K3 that start late -- the grid build on the side stream holds part of the
 * chip when K3 is launched -- then finish late by the whole length of their range: K3 took 2.35 ms next to the build
 * against 1.71 ms alone (profiles/archive/r03d_ab_summary.txt).  Which wave traces which path does not matter: every path has
 * its own random stream and its own slots in the stores. */
struct WaveWork { int next, end, dynBase; bool exhausted; };
/* the FIRST chunk of every wave is fixed (chunk number = wave number): 4096 waves asking one counter word at the same
   moment wait ~50 us for it (it sustains ~88 returning atomics per microsecond), which a 512^2 frame -- one chunk per
   wave, 0.2 ms per kernel -- cannot afford; the counter deals out the chunks after those */
__device__ __forceinline__ void wave_work_init(WaveWork &w, int chunk, int total)
{
    const int wave = (int)((blockIdx.x * blockDim.x + threadIdx.x) / VCM_WAVE), nWaves = (int)(gridDim.x * blockDim.x / VCM_WAVE);
    w.next = min(total, wave * chunk); w.end = min(total, w.next + chunk);
    w.dynBase = nWaves * chunk;
    w.exhausted = w.dynBase >= total;
}
/* returns the path index for this lane (dead lanes only; -1: none left for it in this step) */
__device__ __forceinline__ int wave_work_take(WaveWork &w, int *counter, int chunk, int total, unsigned long long need, unsigned lane)
{
    const int want = __popcll(need);                                   /* wave-uniform */
    const int rank = __popcll(need & ((1ull << lane) - 1ull));
    const int rem = max(w.end - w.next, 0);
    int idx = (rank < rem) ? w.next + rank : -1;
    if (want > rem && !w.exhausted) {                                  /* wave-uniform branch */
        int base = 0;
        /* (one counter per XCD was measured too: the XCDs then finish at different times, K3 2.07 instead of 1.98 ms) */
        if (lane == 0) base = atomicAdd(counter, chunk);
        base = w.dynBase + __builtin_amdgcn_readfirstlane(base);
        if (base >= total) w.exhausted = true;
        const int nend = min(total, base + chunk);
        if (rank >= rem) { const int i2 = base + (rank - rem); idx = (i2 < nend) ? i2 : -1; }
        w.next = base + (want - rem); w.end = nend;
    } else w.next += want;
    return idx;
}

/* ---------------- K1: light sub-paths (vertexcm.hxx:321-396) ------------ */
#if defined(VCM_K1_WAVES)
#define VCM_K1_ATTR __attribute__((amdgpu_waves_per_eu(VCM_K1_WAVES, VCM_K1_WAVES)))
#else
#define VCM_K1_ATTR
#endif
template <int MODE, class SC>
__global__ void __launch_bounds__(VCM_TRACE_BLOCK) VCM_K1_ATTR
k_light_trace(const DScene *__restrict__ scp, IterParams P, LightStore store, float *fb,
              unsigned char *rngCount, unsigned long long *gstats, int chunk, StampArgs st, int *work, GridHeader *hdr)
{
    stamp_entry(st);
    const SC &sc = *static_cast<const SC *>(scp);
    stage_scene_tables(sc);
    stage_pick_tables(sc);
    const unsigned lane = lane_id();
    WaveWork ww; wave_work_init(ww, chunk, P.nLocal);
    LaneStats ls; lane_stats_zero(ls);
    LaneBox box; lane_box_init(box);
    LightPath path;
    bool alive = false;
    RC_DECL;
    for (;;) {
        /* refill dead lanes: ballot + prefix popcount over the wave */
        const unsigned long long need = __builtin_amdgcn_ballot_w64(!alive);
        if (need) {
            const int idx = wave_work_take(ww, work, chunk, P.nLocal, need, lane);
            if (!alive && idx >= 0) { light_path_begin(sc, P, path, idx); alive = true; }
        }
        RC_MARK(19);
        if (!wave_any(alive)) { if (ww.exhausted) break; else continue; }
        if (alive) {
            alive = light_path_step<MODE>(sc, P, path, store, fb, ls, box);
            RC_RESET;
            if (!alive) {
                store.count[path.lp] = (unsigned char)path.nStored;   /* mPathEnds :395 */
                store.lenMask[path.lp] = path.lenMask;
                rngCount[path.lp] = (unsigned char)path.rng.k;
            }
        }
        RC_MARK(21);
    }
    {   /* the box of the vertices this block stored -> the grid header, both ends as order keys under atomicMax (the
           minimum inverted): the words start at zero, which the iteration's zeroing kernel provides */
        uint32_t key[6];
#pragma unroll
        for (int c = 0; c < 3; c++) { key[c] = ~float_order_key(box.mn[c]); key[3 + c] = float_order_key(box.mx[c]); }
        __shared__ uint32_t sbox[VCM_TRACE_BLOCK / VCM_WAVE][6];
#pragma unroll
        for (int c = 0; c < 6; c++) {
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) key[c] = max(key[c], (uint32_t)__shfl_xor((int)key[c], o, 64));
            if (lane == 0) sbox[threadIdx.x / VCM_WAVE][c] = key[c];
        }
        __syncthreads();
        if (threadIdx.x < 6) {
            uint32_t v = sbox[0][threadIdx.x];
            for (int w = 1; w < VCM_TRACE_BLOCK / VCM_WAVE; w++) v = max(v, sbox[w][threadIdx.x]);
            if (threadIdx.x < 3) atomicMax(&hdr->bboxMinU[threadIdx.x], v); else atomicMax(&hdr->bboxMaxU[threadIdx.x - 3], v);
        }
    }
    flush_stats(ls, gstats);
}

/* ---------------- K3: camera sub-paths (vertexcm.hxx:415-545) ----------- */
/* MODE 1 (default, "wavefront"): trace + scatter only; DI / VC / merge become
 *        records and tasks for K3b / K3c / K4, k_resolve replays the additions;
 * MODE 0 ("strict"): everything inside the path. */
#if defined(VCM_K3_WAVES)   /* experiment: cap K3's registers for more waves per SIMD (spills go to scratch) */
#define VCM_K3_ATTR __attribute__((amdgpu_waves_per_eu(VCM_K3_WAVES, VCM_K3_WAVES)))
#else   /* (amdgpu_waves_per_eu(4) here would hold the wavefront instantiations, which sit at 126-129 registers, to four
           waves per SIMD -- and the strict ones, which share the template, to 128 registers with spills: not set; the
           SceneQuads instantiation, the fallback for quads that are not axis-aligned rectangles, is the one at 129) */
#define VCM_K3_ATTR
#endif
template <int MODE, class SC>
__global__ void __launch_bounds__(VCM_TRACE_BLOCK) VCM_K3_ATTR
k_camera_trace(const DScene *__restrict__ scp, IterParams P, LightStore store, GridStore grid, VertexStore vs,
               F4 *camOut, uint32_t *camMask, unsigned char *rngCount, unsigned long long *gstats, int chunk, StampArgs st)
{
    stamp_entry(st);
    const SC &sc = *static_cast<const SC *>(scp);
    stage_scene_tables(sc);
    stage_pick_tables(sc);
    const unsigned lane = lane_id();
    WaveWork ww; wave_work_init(ww, chunk, P.nLocal);
    int *work = vs.count + 8;   /* the chunk counter of this launch (zeroed with the queue counts) */
    LaneStats ls; lane_stats_zero(ls);
    __shared__ uint32_t accQ[MODE == 1 ? 1 : (VCM_MERGE_Q + 1) * VCM_TRACE_BLOCK];   /* [entry][thread]: conflict-free */
    MergeScratch ms; ms.q = accQ + (MODE == 1 ? 0 : threadIdx.x); ms.stride = VCM_TRACE_BLOCK; ms.cap = VCM_MERGE_Q;
    __shared__ int wqState[(VCM_TRACE_BLOCK / VCM_WAVE) * 6];   /* per wave: 3 queues x {next, left} */
    int *myState = wqState + (threadIdx.x / VCM_WAVE) * 6;
    if (lane < 6) myState[lane] = 0;
    CameraWaveQueues wqs;
    wqs.v.p = (WaveQueueWords)myState; wqs.di.p = (WaveQueueWords)(myState + 2); wqs.vc.p = (WaveQueueWords)(myState + 4);
    wqs.pendingVertex = -1; wqs.pendingArrival = 0;
    QueryKey qk = { 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 1u, 1u, 0, 0, 0 };
    if (MODE == 1 && vs.sortKey && P.useVM) qk = query_key_load(P, vs.sortHdr);
    CameraPath path;
    bool alive = false;
    RC_DECL;
    for (;;) {
        const unsigned long long need = __builtin_amdgcn_ballot_w64(!alive);
        if (need) {
            const int idx = wave_work_take(ww, work, chunk, P.nLocal, need, lane);
            if (!alive && idx >= 0) { camera_path_begin(sc, P, path, idx, MODE == 1 ? store.lenMask : (const uint32_t *)0); alive = true; }
        }
        RC_MARK(20);
        if (!wave_any(alive)) { if (ww.exhausted) break; else continue; }
        if (alive) {
            alive = camera_path_step<MODE>(sc, P, path, store, grid, ls, ms, vs, wqs, qk);
            RC_RESET;
            if (!alive) {
                const int target = camera_path_target(P, path);
                camOut[path.lp] = mk4(path.color.x, path.color.y, path.color.z, u2f((uint32_t)target));
                if (MODE == 1) camMask[path.lp] = path.queryMask;
                rngCount[path.lp] = (unsigned char)path.rng.k;
            }
        }
        RC_MARK(22);
    }
    if (MODE == 1 && wqs.pendingVertex >= 0) vs.sortArrival[wqs.pendingVertex] = wqs.pendingArrival;   /* the last append's place (vcm_core.h) */
    if (MODE == 1) {   /* mark the unused tails of this wave's last blocks as holes */
        const int vb = wq_load(wqs.v.p), vl = wq_load(wqs.v.p + 1), db = wq_load(wqs.di.p), dl = wq_load(wqs.di.p + 1), cb = wq_load(wqs.vc.p), cl = wq_load(wqs.vc.p + 1);
        for (int i = (int)lane; i < vl; i += VCM_WAVE) {
            vq(vs, 0, vb + i) = mk4(0.f, 0.f, 0.f, u2f(0xffffffffu));
            if (vs.sortKey) vs.sortKey[vb + i] = -1;
        }
        for (int i = (int)lane; i < dl; i += VCM_WAVE) vs.diTask[db + i] = -1;
        for (int i = (int)lane; i < cl; i += VCM_WAVE) vs.vcTask[2 * (cb + i)] = -1;
    }
    flush_stats(ls, gstats);
}

/* ---------------- PathTracer / EyeLight (pathtracer.hxx:45-215, eyelight.hxx:46-77) ---------------- */
/* Same shape as K3: persistent waves, one lane per pixel, dead lanes refilled by ballot + prefix popcount.
 * The colour of a path goes to camOut with the pixel of its jittered sample; k_resolve adds it in path order. */
template <class SC>
__global__ void __launch_bounds__(VCM_TRACE_BLOCK)
k_path_trace(const DScene *__restrict__ scp, IterParams P, F4 *camOut, unsigned char *rngCount,
             unsigned long long *gstats, int chunk, StampArgs st, int *work)
{
    stamp_entry(st);
    const SC &sc = *static_cast<const SC *>(scp);
    stage_scene_tables(sc);
    stage_pick_tables(sc);
    const unsigned lane = lane_id();
    WaveWork ww; wave_work_init(ww, chunk, P.nLocal);
    LaneStats ls; lane_stats_zero(ls);
    PtPath path;
    bool alive = false;
    for (;;) {
        const unsigned long long need = __builtin_amdgcn_ballot_w64(!alive);
        if (need) {
            const int idx = wave_work_take(ww, work, chunk, P.nLocal, need, lane);
            if (!alive && idx >= 0) { pt_path_begin(sc, P, path, idx); alive = true; }
        }
        if (!wave_any(alive)) { if (ww.exhausted) break; else continue; }
        if (alive) {
            alive = pt_path_step(sc, P, path, ls);
            if (!alive) {
                camOut[path.lp] = mk4(path.color.x, path.color.y, path.color.z, u2f((uint32_t)raster_target(P, path.sx, path.sy)));
                rngCount[path.lp] = (unsigned char)path.rng.k;
            }
        }
    }
    flush_stats(ls, gstats);
}

template <class SC>
__global__ void __launch_bounds__(256)
k_eye_light(const DScene *__restrict__ scp, IterParams P, F4 *camOut, unsigned char *rngCount,
            unsigned long long *gstats, StampArgs st)
{
    stamp_entry(st);
    const SC &sc = *static_cast<const SC *>(scp);
    stage_scene_tables(sc);
    LaneStats ls; lane_stats_zero(ls);
    for (int lp = blockIdx.x * blockDim.x + threadIdx.x; lp < P.nLocal; lp += gridDim.x * blockDim.x) {
        V3 color = sp3(0.f);
        float sx, sy;
        uint32_t drawn;
        const bool hit = eyelight_path(sc, P, lp, color, sx, sy, drawn, ls);
        camOut[lp] = mk4(color.x, color.y, color.z, u2f((uint32_t)(hit ? raster_target(P, sx, sy) : -1)));
        rngCount[lp] = (unsigned char)drawn;
    }
    flush_stats(ls, gstats);
}

/* ---------------- K3b / K3c: dense connection tasks ----------------------- */
/* One lane per task; every lane of a wave runs the same code path (a BSDF
 * evaluation or two and ONE shadow ray), which is what the fused path could
 * not offer: there the connection loop ran at the trip count of the busiest
 * lane and at 23 % lane utilisation (profiles/archive/r01b_pmc_*). */
#define VCM_TASK_BLOCK 256
/* (Round 4 dealt the tasks of K3b / K3c out by (cell of the ray's origin, cell of its end point) for scenes behind a BVH --
 * a counting sort with chunk histograms in LDS.  The host replay had promised half the wave-instructions per ray
 * (profiles/archive/r06m1_bvh_sim.txt) and the kernels delivered: K3b 850 -> 360 us, K3c 1040 -> 700 us on the mesh scene.  The two
 * sorts cost what they saved -- 452 against 455 Mpaths/s, the same on meshes of 80 000 and 320 000 triangles -- because
 * everything behind K3 is throughput-bound there and K4 is the longest of it: profiles/archive/r06ts_tasksort_m1.txt.  Commit ce1ce6b
 * has the code.) */
#if defined(VCM_TASK_WAVES)   /* experiment: cap the registers of K3b / K3c for more waves per SIMD */
#define VCM_TASK_ATTR __attribute__((amdgpu_waves_per_eu(VCM_TASK_WAVES, VCM_TASK_WAVES)))
#else
#define VCM_TASK_ATTR
#endif
template <class SC>
__global__ void __launch_bounds__(VCM_TASK_BLOCK) VCM_TASK_ATTR
k_connect_di(const DScene *__restrict__ scp, IterParams P, VertexStore vs, unsigned long long *gstats,
             const int *__restrict__ bucketStart, int *sortedVertex, StampArgs st)
{
    stamp_entry(st);
    const SC &sc = *static_cast<const SC *>(scp);
    stage_scene_tables(sc);
    stage_pick_tables(sc);
    const int n = vs.count[1];
    LaneStats ls; lane_stats_zero(ls);
    for (int t = blockIdx.x * VCM_TASK_BLOCK + threadIdx.x; t < n; t += gridDim.x * VCM_TASK_BLOCK) {
        const int vi = vs.diTask[t];
        if (vi < 0) continue;   /* hole */
        size_t ps;
        const V3 v = eval_di_task(sc, P, vs, vi, ls, ps);
        vs.diOut[ps] = mk4(v.x, v.y, v.z, 0.f);
        if (sortedVertex) {   /* K4a's scatter pass, here: this kernel visits every camera vertex once */
            const int k = vs.sortKey[vi];
            if (k >= 0) sortedVertex[bucketStart[k] + vs.sortArrival[vi]] = vi;
        }
    }
    flush_stats(ls, gstats);
}

template <class SC>
__global__ void __launch_bounds__(VCM_TASK_BLOCK) VCM_TASK_ATTR
k_connect_vc(const DScene *__restrict__ scp, IterParams P, VertexStore vs, LightStore store,
             unsigned long long *gstats)
{
    const SC &sc = *static_cast<const SC *>(scp);
    stage_scene_tables(sc);
    const int n = vs.count[2];
    LaneStats ls; lane_stats_zero(ls);
    for (int t = blockIdx.x * VCM_TASK_BLOCK + threadIdx.x; t < n; t += gridDim.x * VCM_TASK_BLOCK) {
        const VcTaskPair pr = reinterpret_cast<const VcTaskPair *>(vs.vcTask)[t];
        const int vi = pr.vertex;
        if (vi < 0) continue;   /* hole */
        const V3 v = eval_vc_task(sc, P, vs, store, vi, pr.j, ls);
        vs.vcOut[t] = mk4(v.x, v.y, v.z, 0.f);
    }
    flush_stats(ls, gstats);
}

/* ---------------- K4a: sort the camera vertices by base cell -------------- */
/* Counting sort (indices only) of the vertex records on the Morton code of the
 * cell that contains the query point (hashgrid.hxx:124-131).  Same cell =>
 * same key, so the lanes of a wave walk the same cell lists (broadcast loads,
 * equal trip counts); neighbouring keys are neighbouring cells of a row, so consecutive
 * waves share most of their 8-cell neighbourhoods and find them in L2 -- with
 * the hash bucket as key (first version) consecutive waves were spatially
 * unrelated and K4 re-fetched ~10x the photon data from HBM.  The order inside
 * a key is arbitrary (atomics) and does not matter: every vertex has its own
 * output slot. */

/* holes and out-of-bbox vertices are not sorted at all (key -1): they would all
 * land in one bucket, i.e. on one atomic word */
__global__ void __launch_bounds__(256) k_query_count(IterParams P, VertexStore vs, const GridHeader *__restrict__ hdr, int *key, int *arrival,
                              int *bucketCount, StampArgs st)
{
    stamp_entry(st);
    const int nQ = vs.count[0];
    for (int q = blockIdx.x * blockDim.x + threadIdx.x; q < nQ; q += gridDim.x * blockDim.x) {
        const F4 r0 = vq(vs, 0, q);
        int k = -1;
        if (f2u(r0.w) != 0xffffffffu) {
            k = query_sort_key(P, hdr, mk3(r0.x, r0.y, r0.z));
            if (k < 0)   /* empty query: contrib = 0 */
                vs.mergeOut[merge_out_slot(P, f2u(vq(vs, 1, q).w) & 0xffu, f2u(r0.w), q)] = mk4(0.f, 0.f, 0.f, 0.f);
        }
        key[q] = k;
        /* the value the atomic returns is the vertex's place in its bucket: the scatter needs no second atomic */
        if (k >= 0) arrival[q] = atomicAdd(&bucketCount[k], 1);
    }
}

__global__ void __launch_bounds__(256) k_query_scatter(VertexStore vs, const int *__restrict__ key, const int *__restrict__ arrival,
                                const int *__restrict__ bucketStart, int *sortedVertex)
{
    const int nQ = vs.count[0];
    for (int q = blockIdx.x * blockDim.x + threadIdx.x; q < nQ; q += gridDim.x * blockDim.x) {
        const int k = key[q];
        if (k >= 0) sortedVertex[bucketStart[k] + arrival[q]] = q;
    }
}

/* ---------------- K4: range-merge of the camera vertices ------------------ */
/* HashGrid::Process + RangeQuery::Process (hashgrid.hxx:110-169,
 * vertexcm.hxx:130-169).  One lane per camera vertex (merge_query): a wave
 * keeps 64 dependent-load chains in flight, and because the vertices arrive
 * sorted by base-cell bucket (K4a) its lanes read the same cell lists --
 * broadcast loads, equal trip counts.  The per-query sum is in the reference's
 * order (:157-168).
 * (A wave-per-query mapping was measured too: 17 ms vs 6 ms for this one at
 * 2048^2 -- one query per wave exposes its 4 dependent memory round trips.) */
#ifndef VCM_MERGE_BLOCK
#define VCM_MERGE_BLOCK 256
#endif
/* (k_merge_lane, the lockstep kernel of round 1 -- merge_query of vcm_core.h as a task kernel, 3.93 ms at 2048^2 -- was retired in
   round 6; merge_query itself stays: the fused in-path variant k_camera_trace<0> and the host emulation run it) */

/* ---------------- K4 (walk): every lane walks ITS candidate runs without waiting for the others ---------------- */
/* merge_query (k_merge_lane) visits the 8 cells in lockstep: in step j every lane scans its j-th cell and the wave
 * iterates until the LONGEST of the 64 runs is done -- measured 40 % of the candidate slots of a step hold a candidate
 * (48.6 M ds_write per launch = 12.1 M wave steps x 256 slots for 1.25 G candidates, profiles/archive/r01u_pmc_sq.json), and
 * both halves of the scan, the per-lane loads (TA-bound) and the distance arithmetic, pay for the empty ones.
 * Here a lane first writes the (at most 8) NON-EMPTY runs of its query to LDS -- all 8 hashes and 16 range words in
 * flight together -- and then walks them back to back: when its run ends it takes its next one in the same step,
 * whatever the other lanes are doing.  The wave iterates until the lane with the most candidates IN TOTAL is done,
 * and the lanes of a wave are neighbours in space with similar totals.  The order in which a lane meets its
 * candidates -- cells in the reference's order (hashgrid.hxx:142-155), vertices in index order inside a cell -- is
 * unchanged, so the per-query sum is the same bits. */
#if defined(VCM_K4_WAVES)
#define VCM_K4_ATTR __attribute__((amdgpu_waves_per_eu(VCM_K4_WAVES, VCM_K4_WAVES)))
#else
#define VCM_K4_ATTR
#endif
#ifndef VCM_WALK_Q
#define VCM_WALK_Q 20   /* accepted-index queue per lane: 21 rows + 8 run rows of 8 bytes = 37 KB per block, four blocks per CU
                           (12 / 16 / 20 entries: 3.51 / 3.40 / 3.35 ms, profiles/archive/r03a_ab_summary.txt) */
#endif
#if defined(__HIP_DEVICE_COMPILE__)
struct alignas(8) WalkRun { int lo, hi; };
/* first half of a query: hashgrid.hxx:116-155 -- bbox test, the 8 cells toward the nearer faces, and the NON-EMPTY ones'
   ranges written to the lane's column of `runs`; returns their number, `total` = the query's candidates */
__device__ __forceinline__ int merge_walk_runs(const IterParams &P, const GridStore &g, V3 queryPos, WalkRun *runs /* [k * stride + thread] */,
                                               int stride, int &total)
{
    int n = 0;
    total = 0;
    const V3 bmin = ld3(g.hdr->bboxMin), bmax = ld3(g.hdr->bboxMax);
    const V3 distMin = queryPos - bmin, distMax = bmax - queryPos;
    const bool inside = !(distMin.x < 0.f || distMax.x < 0.f || distMin.y < 0.f || distMax.y < 0.f ||
                          distMin.z < 0.f || distMax.z < 0.f);
    const V3 cellPt = P.invCellSize * distMin;
    const V3 coordF = mk3(floorf(cellPt.x), floorf(cellPt.y), floorf(cellPt.z));
    const int px = int(coordF.x), py = int(coordF.y), pz = int(coordF.z);
    const V3 fractCoord = cellPt - coordF;
    const int pxo = px + (fractCoord.x < 0.5f ? -1 : +1);
    const int pyo = py + (fractCoord.y < 0.5f ? -1 : +1);
    const int pzo = pz + (fractCoord.z < 0.5f ? -1 : +1);
    /* (Round 3 tried to leave out the edge / corner probes that cannot hold a photon within the radius -- 21 % of the
       edge probes, 48 % of the corner probes for evenly spread queries, decided from the query's position in its
       cell with a 1 % margin and only when no other probe shares the bucket: bit-exact, 14 % fewer candidates, and
       2 % SLOWER, profiles/archive/r05b_ab_summary.txt: the wave walks until the lane with the MOST candidates is done,
       and that is a lane near a cell corner, which skips nothing.) */
    int lo[8], hi[8];
#pragma unroll
    for (int j = 0; j < 8; j++) {
        lo[j] = 0; hi[j] = 0;
        if (inside) {
            const int cell = grid_cell_hash((j & 4) ? pxo : px, (j & 2) ? pyo : py, (j & 1) ? pzo : pz, P.nCells);
            lo[j] = g.cellStart[cell];
            hi[j] = g.cellStart[cell + 1];
        }
    }
#pragma unroll
    for (int j = 0; j < 8; j++) {
        total += hi[j] - lo[j];   /* one distance test per entry (:162-165) */
        if (hi[j] > lo[j]) { WalkRun r; r.lo = lo[j]; r.hi = hi[j]; runs[n * stride] = r; n++; }
    }
    return n;
}

/* second half: walk the n runs of column `runs`, queue the accepted photons, drain (RangeQuery::Process) */
template <bool IP, class S>
__device__ __forceinline__ V3 merge_query_walk(const S &sc, const IterParams &P, const GridStore &g, const Bsdf &cameraBsdf,
                                               const SubPathState &st, V3 queryPos, LaneStats &ls, const MergeScratch &ms,
                                               const WalkRun *runs /* [k * stride] */, int stride, int n)
{
    typedef float f4u __attribute__((ext_vector_type(4), aligned(4)));
    V3 contrib = sp3(0.f);
    RC_DECL;
    MergeEval ev;
    merge_eval_setup(ev, sc, P, cameraBsdf, st, false);
    RC_MARK(14);
    const f2 qx = f2_sp(queryPos.x), qy = f2_sp(queryPos.y), qz = f2_sp(queryPos.z);
    int qn = 0, k = 0;
    WalkRun cur, nxt;
    cur.lo = 0; cur.hi = 0; nxt = cur;
    if (n > 0) cur = runs[0];
    if (n > 1) nxt = runs[stride];
    f4u X = *(const f4u *)(g.gx + cur.lo), Y = *(const f4u *)(g.gy + cur.lo), Z = *(const f4u *)(g.gz + cur.lo);
    while (wave_any(cur.lo < cur.hi)) {
        const int stepEnd = cur.lo + VCM_MERGE_UNROLL;
        const bool last = stepEnd >= cur.hi;            /* this step finishes the lane's run (or the lane has none left) */
        const int aNext = last ? nxt.lo : stepEnd;      /* software-pipelined: the candidates of the NEXT step */
        const f4u Xn = *(const f4u *)(g.gx + aNext), Yn = *(const f4u *)(g.gy + aNext), Zn = *(const f4u *)(g.gz + aNext);
        float distSqr[VCM_MERGE_UNROLL];
        {   /* LenSqr(query - position), hashgrid.hxx:162, math.hxx:107: two candidates per packed operation */
            const f2 dxa = qx - X.xy, dya = qy - Y.xy, dza = qz - Z.xy;
            const f2 dxb = qx - X.zw, dyb = qy - Y.zw, dzb = qz - Z.zw;
            const f2 da = dxa * dxa + dya * dya + dza * dza;
            const f2 db = dxb * dxb + dyb * dyb + dzb * dzb;
            distSqr[0] = da.x; distSqr[1] = da.y; distSqr[2] = db.x; distSqr[3] = db.y;
        }
        X = Xn; Y = Yn; Z = Zn;
#pragma unroll
        for (int u = 0; u < VCM_MERGE_UNROLL; u++) {
            const int idx = cur.lo + u;
            const bool acc = (idx < cur.hi) & (distSqr[u] <= P.radiusSqr);   /* :165 */
            ms.q[qn * ms.stride] = (uint32_t)idx;
            qn += acc ? 1 : 0;
        }
        if (last) {   /* on to this lane's next run; the one after it comes out of LDS while this one is scanned */
            cur = nxt;
            k++;
            nxt.lo = 0; nxt.hi = 0;
            if (k + 1 < n) nxt = runs[(k + 1) * stride];
        } else cur.lo = stepEnd;
        /* (draining only when K lanes are full was measured in round 3, K = 4 .. 24: no gain, profiles/archive/r05zz_k4full_*.txt) */
        if (wave_any(qn > ms.cap - VCM_MERGE_UNROLL)) {
            ls.mergeAccepted += (uint32_t)qn;
            RC_MARK(15);
            merge_drain<IP, S::kGgx>(P, g, ev, ms, qn, contrib);
            RC_MARK(16);
            qn = 0;
        }
    }
    ls.mergeAccepted += (uint32_t)qn;
    RC_MARK(15);
    merge_drain<IP, S::kGgx>(P, g, ev, ms, qn, contrib);
    RC_MARK(16);
    return contrib;
}
#endif

/* The batches (256 consecutive queries of the cell-sorted order) reach the workgroups in chunks of `chunk` batches dealt round-robin to
 * the XCDs (workgroup i runs on XCD i mod 8, and each XCD has its own L2: a region's photons are fetched into ONE L2 and reused by the
 * neighbouring queries, while dense regions, which span many chunks, are still spread over all XCDs).  (One contiguous eighth of the
 * sorted queries per XCD drawn from eight counters with stealing -- SMALLVCM_AMD_MERGE_DEAL=slab, rounds 3-5 -- moved 19 % less HBM
 * traffic and was 1.5 % faster on the Cornell scenes and 40 % slower on a mesh with a caustic: retired in round 6,
 * profiles/archive/r05e_ab_summary.txt, r05f_ab_summary.txt.) */
/* (the body of k_merge_walk: S = DScene, or WithGgx<DScene> for a scene with GGX lobes) */
template <bool IP, class S>
__device__ __forceinline__ void merge_walk_body(const DScene *__restrict__ scp, const IterParams &P, const GridStore &g, const VertexStore &vs,
                                                const int *__restrict__ sortedVertex, const int *__restrict__ nSorted, unsigned long long *gstats, int chunk)
{
#if defined(__HIP_DEVICE_COMPILE__)
    const S &sc = *static_cast<const S *>(scp);
    const int nQ = *nSorted;
    __shared__ uint32_t accQ[(VCM_WALK_Q + 1) * VCM_MERGE_BLOCK];
    __shared__ WalkRun runs[8 * VCM_MERGE_BLOCK];
    MergeScratch ms; ms.q = accQ + threadIdx.x; ms.stride = VCM_MERGE_BLOCK; ms.cap = VCM_WALK_Q;
    LaneStats ls; lane_stats_zero(ls);
    const int nBatches = (nQ + VCM_MERGE_BLOCK - 1) / VCM_MERGE_BLOCK;
    const int xcd = blockIdx.x & 7, wgOfXcd = blockIdx.x >> 3, wgPerXcd = gridDim.x >> 3;
    for (int t = wgOfXcd;; t += wgPerXcd) {
        const int b = ((t / chunk) * 8 + xcd) * chunk + (t % chunk);
        if ((t / chunk) * 8 * chunk >= nBatches) break;
        if (b >= nBatches) continue;
        const int q = b * VCM_MERGE_BLOCK + (int)threadIdx.x;
        if (q < nQ) {   /* the runs of a lane are private to it: no barrier */
            const int vi = sortedVertex[q];
            const F4 a = vq(vs, 0, vi), bq = vq(vs, 1, vi), c = vq(vs, 2, vi), d = vq(vs, 3, vi);
            const size_t ps = merge_out_slot(P, f2u(bq.w) & 0xffu, f2u(a.w), vi);
            Bsdf bsdf;
            bsdf_restore(bsdf, mk3(bq.x, bq.y, bq.z), mk3(c.x, c.y, c.z), f2u(bq.w) >> 8, sc, false);
            SubPathState sps;
            sps.pathLength = f2u(bq.w) & 0xffu; sps.dVCM = c.w; sps.dVM = d.w;
            int total;
            const int n = merge_walk_runs(P, g, mk3(a.x, a.y, a.z), runs + threadIdx.x, VCM_MERGE_BLOCK, total);
            ls.mergeCandidates += (uint32_t)total;
            const V3 contrib = merge_query_walk<IP>(sc, P, g, bsdf, sps, mk3(a.x, a.y, a.z), ls, ms, runs + threadIdx.x, VCM_MERGE_BLOCK, n);
            const V3 v = mk3(d.x, d.y, d.z) * P.vmNormalization * contrib;
            vs.mergeOut[ps] = mk4(v.x, v.y, v.z, 0.f);
        }
    }
    flush_stats(ls, gstats);
#endif
}
/* GGX: K4 of a scene with GGX lobes (vcm_core.h WithGgx): MergeEval carries the lobe's per-query part */
template <bool IP, bool GGX>
__global__ void __launch_bounds__(VCM_MERGE_BLOCK) VCM_K4_ATTR
k_merge_walk(const DScene *__restrict__ scp, IterParams P, GridStore g, VertexStore vs,
             const int *__restrict__ sortedVertex, const int *__restrict__ nSorted, unsigned long long *gstats, int chunk, StampArgs st)
{
    stamp_entry(st);
    merge_walk_body<IP, std::conditional_t<GGX, WithGgx<DScene>, DScene>>(scp, P, g, vs, sortedVertex, nSorted, gstats, chunk);
}

#if defined(VCM_K4_TIMES)
__device__ unsigned long long g_k4Times[2 * 32768];
#endif
#if defined(VCM_K4_REGIONS)   /* measurement variant: where the residence time of k_merge_pairs' waves goes (profiles/tools/k4_regions.py).
   The clock is the wave's, kept in registers (the kernel's LDS is spent); a mark charges the cycles since the previous one to its region and
   leaves its own cost out; s_memtime also waits for the wave's outstanding LDS operations, which the region before the mark is charged. */
__device__ unsigned long long g_k4Regions[16];
struct K4Regions { unsigned long long t, c[8]; };
#define K4R_PARAM , K4Regions &k4r
#define K4R_ARG , k4r
#define K4R(id) { const unsigned long long n_ = clock64(); k4r.c[id] += n_ - k4r.t; k4r.t = clock64(); }
#else
#define K4R_PARAM
#define K4R_ARG
#define K4R(id)
#endif
#if defined(VCM_K4_STEPS)   /* measurement variant: the scan steps every query needs, in the order K4 takes them (profiles/tools/k4_lanes.py) */
__device__ unsigned short g_k4Steps[1 << 24];
#endif
/* ---------------- K4 (pairs): the scan per lane, RangeQuery::Process per PAIR ---------------- */
/* Round 6 (profiles/r13a_pmc_mem.json): k_merge_walk is bound by the texture path -- TD busy 97 % of the kernel's cycles, TA
 * 83 %, 46 % of the cycles moving data at the full 64 bytes per clock, the rest stalled behind L1 misses -- and that path is
 * charged per LANE of a load whether or not the lane's data is wanted: the drain of k_merge_walk evaluates the queued photons
 * of a wave's 64 queries in lockstep, the wave drains when ONE lane's queue is full, and on average 38 % of the lanes then
 * hold an entry -- 2.6 gathers of 40 bytes x 64 lanes (and 2.6 evaluations of ~75 instructions) per useful one.
 * Here the accepted (query lane, photon) PAIRS of a wave go to ONE ring in LDS (ballot + prefix popcount, in the order the
 * lanes meet them) and are evaluated 64 at a time by whichever lane gets them: every gather and every evaluation is a
 * wanted one.  What a pair's lane needs of ITS query -- the frame, mLocalDirFix, the component probabilities, the MIS terms:
 * 20 words -- the query's lane wrote to an LDS row when the batch started (the 12 words a diffuse surface needs first, the 8
 * only a Phong lobe reads behind them); the material constants come from a table staged at kernel start.
 * ORDER, and why the sum is still the reference's (vertexcm.hxx:168): a query's pairs enter the ring in the order its lane
 * walks its candidates (cells in the reference's order, hashgrid.hxx:142-155, vertices in index order) and leave it first
 * in, first out.  Every entry carries how many pairs ITS query had pushed before it (`seq`, counted by the query's lane); in a batch
 * of 64 the pairs of a query have consecutive counts, so `occ` = seq - the smallest of them = how many pairs of its query precede the
 * entry in its batch; the terms are added to the queries' accumulators in rounds -- round r: the lanes whose entry
 * has occ = r, which are pairs of DIFFERENT queries, each a plain read-add-write on its query's three words.  (ds_add_f32
 * would do the same in one instruction -- the LDS serialises it by lane -- at 195 cycles per wave-instruction against 4-5 for
 * a read or a write: profiles/r13d_lds_bench.txt; the first version of this kernel spent its time there.)
 * The gathers of a batch are issued when it is full and its evaluation waits until the NEXT batch is full (or the scan has
 * ended): the scan steps in between hide their latency. */
#define VCM_PAIR_RING 128          /* entries per wave: 63 pending + the 64 one candidate column can add */
#define VCM_PAIR_MATERIALS 32      /* material rows in LDS; a scene with more keeps k_merge_walk (vcm_api.hip) */
#define VCM_PAIR_ROW 5             /* 16-byte words of a query's row */
#if defined(__HIP_DEVICE_COMPILE__)
typedef float vcm_f4 __attribute__((ext_vector_type(4)));
struct alignas(8) PairEntry { uint32_t idx, meta; };   /* photon | query lane (bits 0-5), seq (bits 6-31): how many pairs its query had before it */
typedef uint32_t __attribute__((may_alias)) vcm_u32_alias;
struct PairLds {
    int runLo[8 * VCM_MERGE_BLOCK];
    unsigned short runLen[8 * VCM_MERGE_BLOCK];   /* saturates at 65535: the lane then re-reads the cell's end (merge_pairs_run_end) */
    vcm_f4 row[VCM_MERGE_BLOCK * VCM_PAIR_ROW];   /* {mZ | ldf.z}, {diffProb, phongProb, contProb, code}, {camTerm, camdVM, revPdfDiffuse, seqMin}; Phong only: {mX | ldf.x}, {mY | ldf.y} */
    float acc[3 * VCM_MERGE_BLOCK];
    PairEntry ring[(VCM_MERGE_BLOCK / 64) * VCM_PAIR_RING];
    vcm_f4 mat[VCM_PAIR_MATERIALS * 2];           /* {diffuse / pi, phongExp}, {rho, -} */
};
static_assert(sizeof(PairLds) <= 40960, "four workgroups per CU");
struct PairBatch { uint32_t meta; MergePhoton ph; bool valid; };

/* the end of probe j's cell, for a run whose 16-bit length saturated (a cell with 65535 photons or more: a caustic, a point
   light next to a wall).  Cold: recomputes the probe's cell from the query position exactly as merge_pairs_runs did. */
__device__ __noinline__ int merge_pairs_run_end(const IterParams &P, const GridStore &g, V3 queryPos, int probe)
{
    const V3 bmin = ld3(g.hdr->bboxMin);
    const V3 cellPt = P.invCellSize * (queryPos - bmin);
    const V3 coordF = mk3(floorf(cellPt.x), floorf(cellPt.y), floorf(cellPt.z));
    const int px = int(coordF.x), py = int(coordF.y), pz = int(coordF.z);
    const V3 fractCoord = cellPt - coordF;
    const int pxo = px + (fractCoord.x < 0.5f ? -1 : +1);
    const int pyo = py + (fractCoord.y < 0.5f ? -1 : +1);
    const int pzo = pz + (fractCoord.z < 0.5f ? -1 : +1);
    const int cell = grid_cell_hash((probe & 4) ? pxo : px, (probe & 2) ? pyo : py, (probe & 1) ? pzo : pz, P.nCells);
    return g.cellStart[cell + 1];
}

/* hashgrid.hxx:116-155 as in merge_walk_runs, the runs as {lo, 16-bit length}; `probes` = which of the 8 probes they are */
__device__ __forceinline__ int merge_pairs_runs(const IterParams &P, const GridStore &g, V3 queryPos, PairLds &L, int tid, int &total, uint32_t &probes)
{
    int n = 0;
    total = 0; probes = 0u;
    const V3 bmin = ld3(g.hdr->bboxMin), bmax = ld3(g.hdr->bboxMax);
    const V3 distMin = queryPos - bmin, distMax = bmax - queryPos;
    const bool inside = !(distMin.x < 0.f || distMax.x < 0.f || distMin.y < 0.f || distMax.y < 0.f ||
                          distMin.z < 0.f || distMax.z < 0.f);
    const V3 cellPt = P.invCellSize * distMin;
    const V3 coordF = mk3(floorf(cellPt.x), floorf(cellPt.y), floorf(cellPt.z));
    const int px = int(coordF.x), py = int(coordF.y), pz = int(coordF.z);
    const V3 fractCoord = cellPt - coordF;
    const int pxo = px + (fractCoord.x < 0.5f ? -1 : +1);
    const int pyo = py + (fractCoord.y < 0.5f ? -1 : +1);
    const int pzo = pz + (fractCoord.z < 0.5f ? -1 : +1);
    int lo[8], hi[8];
#pragma unroll
    for (int j = 0; j < 8; j++) {
        lo[j] = 0; hi[j] = 0;
        if (inside) {
            const int cell = grid_cell_hash((j & 4) ? pxo : px, (j & 2) ? pyo : py, (j & 1) ? pzo : pz, P.nCells);
            lo[j] = g.cellStart[cell];
            hi[j] = g.cellStart[cell + 1];
        }
    }
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const int len = hi[j] - lo[j];
        total += len;   /* one distance test per entry (:162-165) */
        if (len > 0) {
            L.runLo[n * VCM_MERGE_BLOCK + tid] = lo[j];
            L.runLen[n * VCM_MERGE_BLOCK + tid] = (unsigned short)(len < 65535 ? len : 65535);
            probes |= (uint32_t)j << (3 * n);
            n++;
        }
    }
    return n;
}
/* where a step of a lane's walk stands: candidates [lo, min((lo & ~3) + 4, hi)) of its run k -- the rest of lo's block of four
   (GridStore::gb) -- (lo = hi = 0: the lane is done) */
struct PairPos { int lo, hi, k; bool sat; };
__device__ __forceinline__ PairPos merge_pairs_run_pos(const PairLds &L, int tid, int k, int n)
{
    PairPos r; r.lo = 0; r.hi = 0; r.k = k; r.sat = false;
    if (k < n) {
        const int len = L.runLen[k * VCM_MERGE_BLOCK + tid];
        r.lo = L.runLo[k * VCM_MERGE_BLOCK + tid];
        r.hi = r.lo + len;
        r.sat = len == 65535;
    }
    return r;
}
__device__ __forceinline__ PairPos merge_pairs_first(const PairLds &L, int tid, int n) { return merge_pairs_run_pos(L, tid, 0, n); }
/* the step after p: the next four candidates of its run, or the first of the lane's next run */
__device__ __forceinline__ PairPos merge_pairs_next(const IterParams &P, const GridStore &g, const PairLds &L, int tid, int n, V3 queryPos,
                                                     uint32_t probes, PairPos p)
{
    if ((p.lo & ~3) + VCM_MERGE_UNROLL < p.hi) { p.lo = (p.lo & ~3) + VCM_MERGE_UNROLL; return p; }   /* the steps after a run's first are aligned blocks */
    if (p.sat) {   /* cold: 65535 candidates of this cell done, it has more (hi is where the next piece starts) */
        const int end = merge_pairs_run_end(P, g, queryPos, (int)((probes >> (3 * p.k)) & 7u));
        const int rest = end - p.hi;
        if (rest > 0) { p.lo = p.hi; p.hi = p.lo + (rest < 65535 ? rest : 65535); p.sat = rest >= 65535; return p; }
    }
    return merge_pairs_run_pos(L, tid, p.lo < p.hi ? p.k + 1 : p.k, n);
}

/* a batch leaves the ring: its (at most 64) entries, the gathers of their photons */
__device__ __forceinline__ void merge_pairs_issue(const GridStore &g, const PairEntry *ring, int lane, int &head, int &cnt, PairBatch &b K4R_PARAM)
{
    const int n = cnt < 64 ? cnt : 64;
    b.valid = lane < n;
    __builtin_amdgcn_wave_barrier();   /* the entries are other lanes' stores: LDS operations of a wave complete in order */
    const PairEntry e = ring[(head + lane) & (VCM_PAIR_RING - 1)];
    b.meta = e.meta;
    /* lanes without an entry read photon 0 (always allocated); the value is not used */
    const uint32_t idx = b.valid ? e.idx : 0u;
    const F2 t = g.g3[idx];
    b.ph.lenBits = t.y;
    b.ph.b = g.g1[idx];
    b.ph.c = g.g2[idx];
    b.ph.dVM = t.x;
    head = (head + n) & (VCM_PAIR_RING - 1);
    cnt -= n;
    K4R(3)
}
/* RangeQuery::Process (vertexcm.hxx:130-169) for the pair of every lane: merge_eval_setup + merge_eval_photon (vcm_core.h)
   statement by statement, the query's side out of its LDS row; then the terms to the accumulators, round by round */
/* GGX (k_merge_pairs<IP, true>, a scene with GGX lobes): the query's row holds mGgxProb where the other form keeps the reverse
   pdf of the diffuse lobe (recomputed here from diffProb and ldf.z: the same two operations on the same values), rows 3 and
   4 are written for a lobe as for Phong, and F0 and alpha come from `ext`, the scene's table in global memory (the LDS
   of this kernel is full: four workgroups per CU); then bsdf_eval_ggx's operations through ggx_eval_core.  ext is not
   looked at in the other form. */
template <bool IP, bool GGX>
__device__ __forceinline__ void merge_pairs_eval(const IterParams &P, PairLds &L, int waveBase, const PairBatch &b, const vcm_material_ext *ext K4R_PARAM)
{
    V3 term = sp3(0.f);
    const int ql = waveBase + (int)(b.meta & 63u);
    /* how many pairs of ITS query precede the entry in this batch: a query's pairs in a batch have consecutive `seq` (they enter the
       ring in its lane's order and a batch is a contiguous piece of the ring), so seq minus the smallest of them -- one ds_min_u32
       per batch on the free word of the query's row (15 cycles per wave-instruction against ds_add_f32's 195: r13d_lds_bench.txt) */
    const uint32_t seq = b.meta >> 6;
    vcm_u32_alias *seqMin = (vcm_u32_alias *)(L.row + ql * VCM_PAIR_ROW + 2) + 3;
    if (b.valid) __hip_atomic_fetch_min(seqMin, seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    __builtin_amdgcn_wave_barrier();
    const uint32_t occ = b.valid ? seq - *seqMin : 0u;
    __builtin_amdgcn_wave_barrier();
    if (b.valid) *seqMin = 0xffffffffu;   /* (in order behind the reads: LDS operations of a wave complete in order) */
    if (b.valid) {
        const vcm_f4 *row = L.row + ql * VCM_PAIR_ROW;
        const vcm_f4 h0 = row[0], h1 = row[1], h2 = row[2];
        const float codeBits = h1.w;   /* (by value: __builtin_bit_cast of the vector ELEMENT h1.w read element 0, ROCm 7.2) */
        const uint32_t code = f2u(codeBits);
        const vcm_f4 m0 = L.mat[(code >> 8) * 2];
        const V3 lightDirection = mk3(b.ph.b.x, b.ph.b.y, b.ph.b.z);
        const float ldfz = h0.w, diffProb = h1.x, phongProb = h1.y;
        const uint32_t lvLen = f2u(b.ph.lenBits), pathLength = code & 0xffu;
        const float genz = dot(lightDirection, mk3(h0.x, h0.y, h0.z));                        /* bsdf.hxx:140 (ToLocal's z) */
        const bool valid = !((lvLen + pathLength > P.maxLen) || (lvLen + pathLength < P.minLen))   /* :133-135 */
                           && !(genz * ldfz < 0.f);                                          /* bsdf.hxx:142 */
        const bool ok = !(ldfz < VCM_EPS_COSINE) && !(genz < VCM_EPS_COSINE);                /* :402, :423 */
        const bool dOn = valid && ok && (diffProb != 0.f);
        float dirPdf = dOn ? diffProb * smax(0.f, genz * VCM_INV_PI_F) : 0.f;
        float revPdf = dOn ? (GGX ? diffProb * smax(0.f, ldfz * VCM_INV_PI_F) : h2.z) : 0.f;
        V3 result = sp3(0.f) + (dOn ? mk3(m0.x, m0.y, m0.z) : sp3(0.f));
        V3 ph = sp3(0.f);
        if (valid && ok && (phongProb != 0.f)) {   /* EvaluatePhong: the other two axes of the frame, mLocalDirFix.xy, rho */
            const vcm_f4 c0 = row[3], c1 = row[4];
            const vcm_f4 m1 = L.mat[(code >> 8) * 2 + 1];
            const V3 gen = mk3(dot(lightDirection, mk3(c0.x, c0.y, c0.z)), dot(lightDirection, mk3(c1.x, c1.y, c1.z)), genz);
            const float dot_R_Wi = dot(reflect_local(mk3(c0.w, c1.w, ldfz)), gen);
            if (!(dot_R_Wi <= VCM_EPS_PHONG)) {
                const float pw = dm_powf_wave(dot_R_Wi, m0.w, false, IP);
                const float pdfW = phongProb * ((m0.w + 1.f) * pw * (VCM_INV_PI_F * 0.5f));
                dirPdf += pdfW;
                revPdf += pdfW;
                ph = mk3(m1.x, m1.y, m1.z) * pw;
            }
        }
        result = result + ph;
        if constexpr (GGX) {
            const float ggxProb = h2.z;
            if (valid && ok && (ggxProb != 0.f)) {   /* bsdf_eval_ggx */
                const vcm_f4 c0 = row[3], c1 = row[4];
                const V3 gen = mk3(dot(lightDirection, mk3(c0.x, c0.y, c0.z)), dot(lightDirection, mk3(c1.x, c1.y, c1.z)), genz);
                const V3 ldf = mk3(c0.w, c1.w, ldfz);
                const vcm_material_ext x = ext[code >> 8];
                const float a2 = x.alpha * x.alpha;
                result = result + ggx_eval_core(ldf, gen, ld3(x.ggx), a2, ggx_lambda(ldf, a2), ggxProb, &dirPdf, &revPdf);
            }
        }
        if (valid && !iszero(result)) {                                                     /* :145-146 */
            dirPdf *= h1.z;                                                                 /* :148 */
            revPdf *= b.ph.b.w;                                                             /* :153 */
            const float wLight = b.ph.c.w * P.misVcWeightFactor + b.ph.dVM * mis(dirPdf);   /* :156-157 */
            const float wCamera = h2.x + h2.y * mis(revPdf);                                /* :160-161 */
            const float misWeight = P.ppm ? 1.f : 1.f / (wLight + 1.f + wCamera);           /* :164-166 */
            term = term + misWeight * result * mk3(b.ph.c.x, b.ph.c.y, b.ph.c.z);           /* :168: 0 + x is x */
        }
    }
    K4R(4)
    /* contrib += term, a query's terms in the order of its pairs: round r = the entries with r pairs of their query before them */
    const bool live = b.valid && (term.x != 0.f || term.y != 0.f || term.z != 0.f);
    for (uint32_t r = 0;; r++) {
        if (live && occ == r) {
            const float ax = L.acc[ql], ay = L.acc[VCM_MERGE_BLOCK + ql], az = L.acc[2 * VCM_MERGE_BLOCK + ql];
            L.acc[ql] = ax + term.x; L.acc[VCM_MERGE_BLOCK + ql] = ay + term.y; L.acc[2 * VCM_MERGE_BLOCK + ql] = az + term.z;
        }
        __builtin_amdgcn_wave_barrier();
        if (!wave_any(live && occ > r)) break;
    }
    K4R(5)
}
/* the four candidates of a step: the accepted ones to the ring.  Four ballots and their counts first; if the ring takes all of
   them -- 63 pending + 64 is the most it holds; the usual step accepts ~30 -- the four candidate COLUMNS (candidate u of all 64
   lanes) go in one after the other without a test in between: a lane's place = the entries before its column + the accepting
   lanes below it.  Then the batches that are full leave.  Nothing in the push depends on where a batch ends (the entries carry a
   running count per query, merge_pairs_eval makes it relative): round 6's first version kept a per-batch count, tested for a full
   batch after every column in a real loop and patched the entries behind the cut -- 36 instructions per column against 15.
   A step that accepts more than the ring has room for (a caustic) goes column by column. */
#define VCM_PAIR_COLUMN(u, mu, au, before)                                                                              \
    {                                                                                                                   \
        const int pos = (int)__builtin_amdgcn_mbcnt_hi((uint32_t)((mu) >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)(mu), (uint32_t)(before))); \
        if (au) { PairEntry e; e.idx = (uint32_t)(blk + (u)); e.meta = metaCur; ring[pos & (VCM_PAIR_RING - 1)] = e; metaCur += 64u; } \
    }
template <bool IP, bool GGX>
__device__ __forceinline__ void merge_pairs_push(const IterParams &P, const GridStore &g, PairLds &L, PairEntry *ring, int lane, int waveBase,
                                                 int lo, int hi, float d0, float d1, float d2, float d3,
                                                 int &head, int &cnt, uint32_t &metaCur, bool &inflight, PairBatch &pb, uint32_t &waveAccepted,
                                                 const vcm_material_ext *ext K4R_PARAM)
{
    const int blk = lo & ~3;   /* the step's block of four; its candidates are those of [lo, hi) */
    const uint32_t first = (uint32_t)(lo & 3), len = (uint32_t)(hi - lo);
    const bool v0 = (0u - first) < len, v1 = (1u - first) < len, v2 = (2u - first) < len, v3 = (3u - first) < len;
    const bool c0 = d0 <= P.radiusSqr, c1 = d1 <= P.radiusSqr, c2 = d2 <= P.radiusSqr, c3 = d3 <= P.radiusSqr;   /* :165 */
    const unsigned long long m0 = __builtin_amdgcn_ballot_w64(v0) & __builtin_amdgcn_ballot_w64(c0),
                             m1 = __builtin_amdgcn_ballot_w64(v1) & __builtin_amdgcn_ballot_w64(c1),
                             m2 = __builtin_amdgcn_ballot_w64(v2) & __builtin_amdgcn_ballot_w64(c2),
                             m3 = __builtin_amdgcn_ballot_w64(v3) & __builtin_amdgcn_ballot_w64(c3);
    const int t0 = __popcll(m0), t1 = __popcll(m1), t2 = __popcll(m2), t3 = __popcll(m3);
    const int T = t0 + t1 + t2 + t3;
    waveAccepted += (uint32_t)T;
    int u = 0;
    do {
        if (u == 0 && cnt + T <= VCM_PAIR_RING) {
            const int at = head + cnt;
            VCM_PAIR_COLUMN(0, m0, v0 & c0, at)
            VCM_PAIR_COLUMN(1, m1, v1 & c1, at + t0)
            VCM_PAIR_COLUMN(2, m2, v2 & c2, at + t0 + t1)
            VCM_PAIR_COLUMN(3, m3, v3 & c3, at + t0 + t1 + t2)
            cnt += T;
            u = 4;
        } else {   /* cold */
            const unsigned long long m = u == 0 ? m0 : u == 1 ? m1 : u == 2 ? m2 : m3;
            const bool a = ((m >> lane) & 1ull) != 0ull;
            VCM_PAIR_COLUMN(u, m, a, head + cnt)
            cnt += __popcll(m);
            u++;
        }
        K4R(2)
        while (cnt >= 64) {   /* a batch is full: it leaves, the one in flight is evaluated */
            if (inflight) merge_pairs_eval<IP, GGX>(P, L, waveBase, pb, ext K4R_ARG);
            merge_pairs_issue(g, ring, lane, head, cnt, pb K4R_ARG);
            inflight = true;
        }
    } while (u < 4);
}
#undef VCM_PAIR_COLUMN
#endif

/* GGX: K4 of a scene with GGX lobes, over WithGgx<DScene>: mGgxProb in the query's row, rows 3 and 4 for a lobe as for Phong,
   and the lobe evaluated by merge_pairs_eval<IP, true> (its comment has the layout).  The text stands in the kernel itself,
   not in a body function that the forms call: so every form's code is what its own text gave (DESIGN.md "Microfacet materials", Kinds). */
template <bool IP, bool GGX>
__global__ void __launch_bounds__(VCM_MERGE_BLOCK) VCM_K4_ATTR
k_merge_pairs(const DScene *__restrict__ scp, IterParams P, GridStore g, VertexStore vs,
              const int *__restrict__ sortedVertex, const int *__restrict__ nSorted, unsigned long long *gstats, int chunk, StampArgs st)
{
    stamp_entry(st);
#if defined(__HIP_DEVICE_COMPILE__)
#if defined(VCM_K4_TIMES)   /* measurement variant: when every workgroup of the launch started and ended (profiles/tools/k4_tail.py) */
    if (threadIdx.x == 0 && blockIdx.x < 32768) g_k4Times[2 * blockIdx.x] = wall_clock64();
#endif
    using S = std::conditional_t<GGX, WithGgx<DScene>, DScene>;
    const S &sc = *static_cast<const S *>(scp);
    const vcm_material_ext *ext = 0;
    if constexpr (GGX) ext = sc.materialExt();
    const int nQ = *nSorted;
    __shared__ __attribute__((aligned(16))) PairLds L;
    const int tid = (int)threadIdx.x, lane = tid & 63, waveBase = tid & ~63;
    PairEntry *ring = L.ring + (tid >> 6) * VCM_PAIR_RING;
    for (int m = tid; m < sc.nMaterials && m < VCM_PAIR_MATERIALS; m += VCM_MERGE_BLOCK) {
        const vcm_material mm = scene_material(sc, m, false);
        const V3 dv = ld3(mm.diffuse) * VCM_INV_PI_F;                                    /* bsdf.hxx:411 */
        const V3 rho = ld3(mm.phong) * (mm.phongExp + 2.f) * 0.5f * VCM_INV_PI_F;       /* :442-443 */
        vcm_f4 a, b;
        a.x = dv.x; a.y = dv.y; a.z = dv.z; a.w = mm.phongExp;
        b.x = rho.x; b.y = rho.y; b.z = rho.z; b.w = 0.f;
        L.mat[m * 2] = a; L.mat[m * 2 + 1] = b;
    }
    __syncthreads();   /* the only barrier: from here on a wave touches its own quarter of the LDS */
    LaneStats ls; lane_stats_zero(ls);
    uint32_t waveAccepted = 0;   /* wave-uniform */
#if defined(VCM_K4_REGIONS)
    K4Regions k4r;
    for (int i = 0; i < 8; i++) k4r.c[i] = 0ull;
    k4r.t = clock64();
#endif
    const int nBatches = (nQ + VCM_MERGE_BLOCK - 1) / VCM_MERGE_BLOCK;
    const int xcd = blockIdx.x & 7, wgOfXcd = blockIdx.x >> 3, wgPerXcd = gridDim.x >> 3;
    for (int t = wgOfXcd;; t += wgPerXcd) {   /* k_merge_walk's static dealing: chunks of batches round-robin over the XCDs */
        const int bt = ((t / chunk) * 8 + xcd) * chunk + (t % chunk);
        if ((t / chunk) * 8 * chunk >= nBatches) break;
        if (bt >= nBatches) continue;
        const int q = bt * VCM_MERGE_BLOCK + tid;
        V3 qp = sp3(0.f), thr = sp3(0.f);
        size_t ps = 0;
        int n = 0;
        uint32_t probes = 0u;
        if (q < nQ) {
            const int vi = sortedVertex[q];
            const F4 a = vq(vs, 0, vi), bq = vq(vs, 1, vi), c = vq(vs, 2, vi), d = vq(vs, 3, vi);
            ps = merge_out_slot(P, f2u(bq.w) & 0xffu, f2u(a.w), vi);
            Bsdf bsdf;
            bsdf_restore(bsdf, mk3(bq.x, bq.y, bq.z), mk3(c.x, c.y, c.z), f2u(bq.w) >> 8, sc, false);
            vcm_f4 r;
            vcm_f4 *row = L.row + tid * VCM_PAIR_ROW;
            r.x = bsdf.frame.mZ.x; r.y = bsdf.frame.mZ.y; r.z = bsdf.frame.mZ.z; r.w = bsdf.localDirFix.z; row[0] = r;
            r.x = bsdf.diffProb; r.y = bsdf.phongProb; r.z = bsdf.contProb; r.w = bq.w; row[1] = r;   /* bq.w: pathLength | matID << 8 */
            r.x = c.w * P.misVcWeightFactor;                                              /* vertexcm.hxx:160 */
            r.y = d.w;
            r.z = GGX ? bsdf.ggxProb   /* (merge_pairs_eval<IP, true> recomputes bsdf.hxx:408) */
                      : bsdf.diffProb * smax(0.f, bsdf.localDirFix.z * VCM_INV_PI_F);     /* bsdf.hxx:408 */
            r.w = u2f(0xffffffffu); row[2] = r;   /* seqMin (merge_pairs_eval) */
            if (bsdf.phongProb != 0.f || (GGX && bsdf.ggxProb != 0.f)) {
                r.x = bsdf.frame.mX.x; r.y = bsdf.frame.mX.y; r.z = bsdf.frame.mX.z; r.w = bsdf.localDirFix.x; row[3] = r;
                r.x = bsdf.frame.mY.x; r.y = bsdf.frame.mY.y; r.z = bsdf.frame.mY.z; r.w = bsdf.localDirFix.y; row[4] = r;
            }
            qp = mk3(a.x, a.y, a.z); thr = mk3(d.x, d.y, d.z);
            int total;
            n = merge_pairs_runs(P, g, qp, L, tid, total, probes);
            ls.mergeCandidates += (uint32_t)total;
#if defined(VCM_K4_STEPS)
            if (q < (1 << 24)) {
                int steps = 0;
                for (int k = 0; k < n; k++) steps += ((L.runLo[k * VCM_MERGE_BLOCK + tid] & 3) + (int)L.runLen[k * VCM_MERGE_BLOCK + tid] + 3) >> 2;
                g_k4Steps[q] = (unsigned short)(steps < 65535 ? steps : 65535);
            }
#endif
        }
        L.acc[tid] = 0.f; L.acc[VCM_MERGE_BLOCK + tid] = 0.f; L.acc[2 * VCM_MERGE_BLOCK + tid] = 0.f;
        /* ---- scan (merge_query_walk's) with the accepted pairs to the wave's ring.  The candidates of a step are loaded TWO
           steps ahead (k_merge_walk: one): the kernel waits for memory, not for issue slots -- three workgroups per CU instead
           of four cost it 16 % (profiles/r13i) -- and the two register sets that hold a step's candidates serve: a set is
           free the moment its distances are formed, and takes the candidates of the step after next. */
        const f2 qx = f2_sp(qp.x), qy = f2_sp(qp.y), qz = f2_sp(qp.z);
        int head = 0, cnt = 0;
        uint32_t metaCur = (uint32_t)lane;   /* the next entry's meta: lane | the pairs this lane has pushed << 6 */
        bool inflight = false;
        PairBatch pb;
        pb.valid = false; pb.meta = 0u;
        PairPos it0 = merge_pairs_first(L, tid, n), it1 = merge_pairs_next(P, g, L, tid, n, qp, probes, it0), it2 = merge_pairs_next(P, g, L, tid, n, qp, probes, it1);
#define VCM_PAIR_LOAD(SX, SY, SZ, at) { const vcm_f4 *blk = (const vcm_f4 *)(g.gb + (size_t)((at) >> 2) * 12u); SX = blk[0]; SY = blk[1]; SZ = blk[2]; }
        vcm_f4 AX, AY, AZ, BX, BY, BZ;
        VCM_PAIR_LOAD(AX, AY, AZ, it0.lo)
        VCM_PAIR_LOAD(BX, BY, BZ, it1.lo)
        K4R(0)
#define VCM_PAIR_AHEAD it2
#define VCM_PAIR_SHIFT it0 = it1; it1 = it2; it2 = merge_pairs_next(P, g, L, tid, n, qp, probes, it2);
#if defined(VCM_K4_REGIONS)   /* (the distances must exist before the mark: they wait for the step's loads) */
#define K4R_DIST(a, b, c, d) { asm volatile("" :: "v"(a), "v"(b), "v"(c), "v"(d)); K4R(1) }
#else
#define K4R_DIST(a, b, c, d)
#endif
#define VCM_PAIR_STEP(SX, SY, SZ)                                                                                              \
        {                                                                                                                      \
            float d0, d1, d2, d3;                                                                                              \
            {   /* LenSqr(query - position), hashgrid.hxx:162, math.hxx:107: two candidates per packed operation */          \
                const f2 dxa = qx - SX.xy, dya = qy - SY.xy, dza = qz - SZ.xy;                                                 \
                const f2 dxb = qx - SX.zw, dyb = qy - SY.zw, dzb = qz - SZ.zw;                                                 \
                const f2 da = dxa * dxa + dya * dya + dza * dza;                                                               \
                const f2 db = dxb * dxb + dyb * dyb + dzb * dzb;                                                               \
                d0 = da.x; d1 = da.y; d2 = db.x; d3 = db.y;                                                                    \
            }                                                                                                                  \
            VCM_PAIR_LOAD(SX, SY, SZ, VCM_PAIR_AHEAD.lo)                                                                       \
            K4R_DIST(d0, d1, d2, d3)                                                                                           \
            merge_pairs_push<IP, GGX>(P, g, L, ring, lane, waveBase, it0.lo, it0.hi, d0, d1, d2, d3, head, cnt, metaCur, inflight, pb, waveAccepted, ext K4R_ARG); \
            VCM_PAIR_SHIFT                                                                                                     \
            K4R(6)                                                                                                             \
        }
        for (;;) {
            if (!wave_any(it0.lo < it0.hi)) break;
            VCM_PAIR_STEP(AX, AY, AZ)
            if (!wave_any(it0.lo < it0.hi)) break;
            VCM_PAIR_STEP(BX, BY, BZ)
        }
#undef VCM_PAIR_STEP
#undef VCM_PAIR_LOAD
#undef VCM_PAIR_AHEAD
#undef VCM_PAIR_SHIFT
        if (inflight) merge_pairs_eval<IP, GGX>(P, L, waveBase, pb, ext K4R_ARG);
        while (cnt > 0) {
            merge_pairs_issue(g, ring, lane, head, cnt, pb K4R_ARG);
            merge_pairs_eval<IP, GGX>(P, L, waveBase, pb, ext K4R_ARG);
        }
        if (q < nQ) {
            const V3 contrib = mk3(L.acc[tid], L.acc[VCM_MERGE_BLOCK + tid], L.acc[2 * VCM_MERGE_BLOCK + tid]);
            const V3 v = thr * P.vmNormalization * contrib;
            vs.mergeOut[ps] = mk4(v.x, v.y, v.z, 0.f);
        }
        K4R(7)
    }
#if defined(VCM_K4_REGIONS)
    if (lane == 0) for (int i = 0; i < 8; i++) atomicAdd(&g_k4Regions[i], k4r.c[i]);
#endif
    if (lane == 0) ls.mergeAccepted = waveAccepted;
    flush_stats(ls, gstats);
#if defined(VCM_K4_TIMES)
    __syncthreads();
    if (threadIdx.x == 0 && blockIdx.x < 32768) g_k4Times[2 * blockIdx.x + 1] = wall_clock64();
#endif
#endif
}

/* (k_merge_staged -- a workgroup of 512 staging the cell lists of its queries through LDS behind an open-addressed table, 27 % less
   HBM traffic than the lockstep kernel and slower than it: 4.2 ms, barriers and a lockstep scan -- was retired in round 6 with the
   kernel it was measured against; the record is HISTORY.md and profiles/archive/r02c_ab_summary.txt.) */

/* ---------------- the merge sharded by SPACE (round 6 prototype) ---------------- */
/* Ranks own slabs of UN-hashed cell coordinates along one axis: slab s = cells [X[s], X[s+1]) (X[0] = -inf, X[S] = +inf).  A query in slab
 * s probes its base cell and one neighbour per axis (hashgrid.hxx:124-155), so the slab's owner needs the photons of cells
 * [X[s] - 1, X[s+1]]: a light vertex goes to every slab whose range, widened by one cell on both sides, holds its cell -- one, two,
 * rarely three owners.  Both partitions below are STABLE (element order inside a destination = index order): the receiver's grid build
 * then reproduces HashGrid::Build's in-cell order (hashgrid.hxx:83-88) on the photons it was given. */
#define VCM_SPACE_MAX_SLABS 64
struct SpaceSlabs { int S, axis; int X[VCM_SPACE_MAX_SLABS + 1]; };
__device__ __forceinline__ int space_cell(const IterParams &P, const GridHeader *hdr, int axis, float coord)
{   /* HashGrid::GetCellIndex's floor (:189-193) for one axis */
    return int(floorf(P.invCellSize * (coord - hdr->bboxMin[axis])));
}
/* histogram of the local light vertices' coordinate along `axis` in 256 bins over [lo, lo + 256 / invBin) (the split points of the slabs
   come out of the sum over the ranks) */
__global__ void __launch_bounds__(256) k_space_hist(const float *__restrict__ records, const int *__restrict__ nPtr, int axis, float lo, float invBin, int *hist)
{
    __shared__ int sH[256];
    sH[threadIdx.x] = 0;
    __syncthreads();
    const int n = *nPtr;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        int b = int((records[(size_t)i * VCM_MERGE_RECORD_FLOATS + axis] - lo) * invBin);
        b = b < 0 ? 0 : (b > 255 ? 255 : b);
        atomicAdd(&sH[b], 1);
    }
    __syncthreads();
    if (sH[threadIdx.x]) atomicAdd(&hist[threadIdx.x], sH[threadIdx.x]);
}
/* KIND 0: light records (13 floats; halo: up to three destinations).  KIND 1: camera vertices = queries (the 4 x 16-byte record of
   VertexStore::q; ONE destination, the slab of the base cell; holes and vertices outside the photon box have none: their merge term is 0
   and K3 has written it). */
template <int KIND>
__device__ __forceinline__ void space_dest_range(const IterParams &P, const GridHeader *hdr, const SpaceSlabs &sl, const float *rec, int &d0, int &d1)
{
    d0 = 0; d1 = -1;
    if (KIND == 1) {
        const uint32_t tag = f2u(rec[3]);
        if (tag == 0xffffffffu) return;   /* hole */
        const V3 p = mk3(rec[0], rec[1], rec[2]);
        const V3 dmin = p - ld3(hdr->bboxMin), dmax = ld3(hdr->bboxMax) - p;   /* hashgrid.hxx:116-122 */
        if (dmin.x < 0.f || dmax.x < 0.f || dmin.y < 0.f || dmax.y < 0.f || dmin.z < 0.f || dmax.z < 0.f) return;
    }
    const int c = space_cell(P, hdr, sl.axis, rec[sl.axis]);
    const int lo = KIND == 0 ? c - 1 : c, hi = KIND == 0 ? c + 1 : c;   /* slab s takes cells [X[s] - 1, X[s+1]] of photons, [X[s], X[s+1]) of queries */
    int a = 0;
    while (a + 1 < sl.S && sl.X[a + 1] <= lo) a++;   /* first slab whose end is beyond lo */
    int b = a;
    while (b + 1 < sl.S && sl.X[b + 1] <= hi) b++;
    d0 = a; d1 = b;
}
__device__ __forceinline__ int space_chunk(int n, int V) { return (((n + V - 1) / V) + 255) & ~255; }
template <int KIND>
__global__ void __launch_bounds__(256) k_space_count(IterParams P, const GridHeader *__restrict__ hdr, SpaceSlabs sl, const float *__restrict__ recs,
                                                     const int *__restrict__ nPtr, int *matrix /* [dest * V + workgroup] */, int *totals /* [dest] */)
{
    __shared__ int sC[VCM_SPACE_MAX_SLABS];
    const int tid = (int)threadIdx.x, V = (int)gridDim.x, n = *nPtr;
    const int W = KIND == 0 ? VCM_MERGE_RECORD_FLOATS : 16;
    if (tid < VCM_SPACE_MAX_SLABS) sC[tid] = 0;
    __syncthreads();
    const int chunk = space_chunk(n, V);
    const long long lo64 = (long long)blockIdx.x * chunk;
    const int lo = lo64 < n ? (int)lo64 : n, hi = (n - lo < chunk) ? n : lo + chunk;
    for (int i = lo + tid; i < hi; i += 256) {
        int d0, d1;
        space_dest_range<KIND>(P, hdr, sl, recs + (size_t)i * W, d0, d1);
        for (int d = d0; d <= d1; d++) atomicAdd(&sC[d], 1);
    }
    __syncthreads();
    if (tid < sl.S) { matrix[tid * V + (int)blockIdx.x] = sC[tid]; if (sC[tid]) atomicAdd(&totals[tid], sC[tid]); }
}
/* scattered[dest * V + workgroup] = the exclusive scan of `matrix` taken as ONE array (dest-major): where this workgroup's first element
   of `dest` goes = that value - the scan's value at [dest * V] (the start of the destination's row) */
template <int KIND>
__global__ void __launch_bounds__(256) k_space_scatter(IterParams P, const GridHeader *__restrict__ hdr, SpaceSlabs sl, const float *__restrict__ recs,
                                                       const int *__restrict__ nPtr, const int *__restrict__ scanned, float *out, long long strideElems,
                                                       int *whereDest /* KIND 1: per source element its destination (-1: none) */, int *wherePos)
{
    __shared__ int sBase[VCM_SPACE_MAX_SLABS];   /* next position of this workgroup in every destination */
    __shared__ int sWave[4];
    const int tid = (int)threadIdx.x, lane = tid & 63, w = tid >> 6, V = (int)gridDim.x, n = *nPtr;
    const int W = KIND == 0 ? VCM_MERGE_RECORD_FLOATS : 16;
    if (tid < sl.S) sBase[tid] = scanned[tid * V + (int)blockIdx.x] - scanned[tid * V];
    __syncthreads();
    const int chunk = space_chunk(n, V);
    const long long lo64 = (long long)blockIdx.x * chunk;
    const int lo = lo64 < n ? (int)lo64 : n, hi = (n - lo < chunk) ? n : lo + chunk;
    for (int t0 = lo; t0 < hi; t0 += 256) {   /* tiles in index order, waves in index order inside a tile: stable */
        const int i = t0 + tid;
        int d0 = 0, d1 = -1;
        if (i < hi) space_dest_range<KIND>(P, hdr, sl, recs + (size_t)i * W, d0, d1);
        if (KIND == 1 && i < hi) { whereDest[i] = d1 >= d0 ? d0 : -1; }
        for (int d = 0; d < sl.S; d++) {   /* wave-uniform loop; most destinations take nothing from a tile */
            const bool mine = d >= d0 && d <= d1;
            const unsigned long long m = __builtin_amdgcn_ballot_w64(mine);
            if (lane == 0) sWave[w] = (int)__popcll(m);
            __syncthreads();
            const int tileTotal = sWave[0] + sWave[1] + sWave[2] + sWave[3];
            if (tileTotal) {   /* workgroup-uniform */
                int before = 0;
                for (int x = 0; x < w; x++) before += sWave[x];
                if (mine) {
                    const int pos = sBase[d] + before + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
                    float *o = out + ((size_t)d * (size_t)strideElems + (size_t)pos) * W;
                    const float *r = recs + (size_t)i * W;
                    if (KIND == 1) { const F4 *r4 = (const F4 *)r; F4 *o4 = (F4 *)o; o4[0] = r4[0]; o4[1] = r4[1]; o4[2] = r4[2]; o4[3] = r4[3]; wherePos[i] = pos; }
                    else { for (int k = 0; k < VCM_MERGE_RECORD_FLOATS; k++) o[k] = r[k]; }
                }
            }
            __syncthreads();
            if (tid == 0 && tileTotal) sBase[d] += tileTotal;
            __syncthreads();
        }
    }
}
__global__ void k_set_int(int *p, int v) { p[0] = v; }
/* the merge terms of this rank's queries, evaluated by the slabs' owners, back into mergeOut (what K4 would have written) */
__global__ void __launch_bounds__(256) k_space_results(IterParams P, VertexStore vs, const int *__restrict__ whereDest, const int *__restrict__ wherePos,
                                                       const F4 *__restrict__ results, long long strideElems)
{
    const int n = vs.count[0];
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const int d = whereDest[i];
        if (d < 0) continue;
        const F4 a = vq(vs, 0, i), b = vq(vs, 1, i);
        vs.mergeOut[path_slot(P, f2u(b.w) & 0xffu, f2u(a.w))] = results[(size_t)d * (size_t)strideElems + (size_t)wherePos[i]];
    }
}

/* ---------------- K5: Framebuffer::AddColor of camera colours ----------- */
/* vertexcm.hxx:544 adds colour p to the pixel of its jittered sample, in path
 * order.  Pixel q can receive from paths q-resX-1, q-resX, q-1, q (ascending
 * = the reference's order); light splats of the iteration are already in.
 * Wavefront mode: a path's colour is rebuilt by replay_path_color. */
__global__ void __launch_bounds__(256) k_resolve(IterParams P, const F4 *__restrict__ camOut, const uint32_t *__restrict__ camMask,
                          VertexStore vs, float *fb, StampArgs st)
{
    stamp_entry(st);
    const int lastQ = min(P.N, P.p0 + P.nLocal + P.resX + 1);
    for (int q = P.p0 + blockIdx.x * blockDim.x + threadIdx.x; q < lastQ; q += gridDim.x * blockDim.x) {
        const int src[4] = { q - P.resX - 1, q - P.resX, q - 1, q };
        float r = fb[(size_t)q * 3 + 0], g = fb[(size_t)q * 3 + 1], b = fb[(size_t)q * 3 + 2];
        bool touched = false;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int lp = src[i] - P.p0;
            if (lp < 0 || lp >= P.nLocal) continue;
            const F4 c = camOut[lp];
            if ((int)f2u(c.w) != q) continue;
            V3 col = mk3(c.x, c.y, c.z);
            if (P.wavefront) col = replay_path_color(P, vs, lp, camMask[lp], col);
            r = r + col.x; g = g + col.y; b = b + col.z;
            touched = true;
        }
        if (touched) { fb[(size_t)q * 3 + 0] = r; fb[(size_t)q * 3 + 1] = g; fb[(size_t)q * 3 + 2] = b; }
    }
}

/* ---------------- exclusive scan (ints), 2 launches ---------------------- */
/* A tile = 2048 consecutive items, one workgroup each.  (1) k_scan_tile_sums: the sum of every tile.  (2) k_scan_apply:
 * a workgroup adds up the sums of ALL tiles before its own -- its 256 threads take them in strides, at most 8192 tile
 * sums = 32 KB out of L2 -- and scans its tile from there.  No workgroup waits for another: the first version put a
 * single 256-thread block between the two (40 us per scan at 512^2, four scans per iteration: 0.31 of 1.54 ms,
 * profiles/archive/r02n_trace512_summary.txt), and a single-pass scan with decoupled look-back (one launch; tried in round 3)
 * is bound by the latency of its look-back chain on this chip -- 64 tiles per ~4 us step: 1.2 ms for the 16.8 M-entry
 * bucket table of a 2048^2 frame against 70 us here (profiles/archive/r05b_ab_summary.txt).  Wave scans are shuffles
 * (6 steps), the four wave totals cross LDS once. */
#define VCM_SCAN_BLOCK 256
#define VCM_SCAN_ITEMS 8
#define VCM_SCAN_TILE (VCM_SCAN_BLOCK * VCM_SCAN_ITEMS)

/* sum over the block (every thread gets it); one barrier pair */
__device__ __forceinline__ int block_sum(int v)
{
    __shared__ int sW[VCM_SCAN_BLOCK / VCM_WAVE];
    v = (int)wave_sum_u32((uint32_t)v);
    __syncthreads();   /* the previous use of sW is over */
    if ((threadIdx.x & (VCM_WAVE - 1)) == 0) sW[threadIdx.x / VCM_WAVE] = v;
    __syncthreads();
    int t = 0;
#pragma unroll
    for (int w = 0; w < VCM_SCAN_BLOCK / VCM_WAVE; w++) t += sW[w];
    return t;
}

template <typename T>
__global__ void __launch_bounds__(VCM_SCAN_BLOCK) k_scan_tile_sums(const T *__restrict__ in, int n, int *tileSums, StampArgs st)
{
    stamp_entry(st);
    const int base = blockIdx.x * VCM_SCAN_TILE + threadIdx.x * VCM_SCAN_ITEMS;
    int sum = 0;
#pragma unroll
    for (int i = 0; i < VCM_SCAN_ITEMS; i++) if (base + i < n) sum += (int)in[base + i];
    const int total = block_sum(sum);
    if (threadIdx.x == 0) tileSums[blockIdx.x] = total;
}

template <typename T>
__global__ void __launch_bounds__(VCM_SCAN_BLOCK)
k_scan_apply(const T *__restrict__ in, int n, const int *__restrict__ tileSums, int *out, int *totalOut, int writeTotalAtN)
{
#if defined(__HIP_DEVICE_COMPILE__)
    const int tid = (int)threadIdx.x, lane = tid & (VCM_WAVE - 1), wave = tid / VCM_WAVE;
    const int base = blockIdx.x * VCM_SCAN_TILE + tid * VCM_SCAN_ITEMS;
    int v[VCM_SCAN_ITEMS];
    int sum = 0;
#pragma unroll
    for (int i = 0; i < VCM_SCAN_ITEMS; i++) { v[i] = (base + i < n) ? (int)in[base + i] : 0; sum += v[i]; }
    /* everything before this tile */
    int before = 0;
    for (int t = tid; t < (int)blockIdx.x; t += VCM_SCAN_BLOCK) before += tileSums[t];
    const int tileOffset = block_sum(before);
    /* inclusive scan of the thread sums inside the wave, then the four wave totals through LDS */
    int incl = sum;
#pragma unroll
    for (int o = 1; o < VCM_WAVE; o <<= 1) { const int t = __shfl_up(incl, o, VCM_WAVE); if (lane >= o) incl += t; }
    __shared__ int sWave[VCM_SCAN_BLOCK / VCM_WAVE];
    if (lane == VCM_WAVE - 1) sWave[wave] = incl;
    __syncthreads();
    int waveOffset = 0;
#pragma unroll
    for (int w = 0; w < VCM_SCAN_BLOCK / VCM_WAVE; w++) if (w < wave) waveOffset += sWave[w];
    int run = tileOffset + waveOffset + (incl - sum);
#pragma unroll
    for (int i = 0; i < VCM_SCAN_ITEMS; i++) {
        if (base + i < n) out[base + i] = run;
        run += v[i];
    }
    /* the thread that holds item n-1 knows the total */
    if (n > 0 && base <= n - 1 && n - 1 < base + VCM_SCAN_ITEMS) {
        if (writeTotalAtN) out[n] = run;
        if (totalOut) *totalOut = run;
    }
#endif
}

/* ---------------- K1b: compaction into merge records --------------------- */
/* Record = the 13 floats of LightVertex that RangeQuery::Process reads
 * (vertexcm.hxx:130-169): pos, WorldDirFix, throughput, dVCM, dVM,
 * ContinuationProb, pathLength.  Record order = the reference's
 * mLightVertices order (path-major, then bounce). */
/* the box K1 left in the header's key words (minimum as ~key), or the plain keys of k_bbox -> floats (hashgrid.hxx:47-61) */
__device__ __forceinline__ void bbox_finalize_component(GridHeader *hdr, int c, int nRecords, int minInverted)
{
    if (nRecords > 0) {
        hdr->bboxMin[c] = float_from_order_key(minInverted ? ~hdr->bboxMinU[c] : hdr->bboxMinU[c]);
        hdr->bboxMax[c] = float_from_order_key(hdr->bboxMaxU[c]);
    } else {   /* :47-48 initial values */
        hdr->bboxMin[c] = 1e36f;
        hdr->bboxMax[c] = -1e36f;
    }
}
/* hdr != NULL (single rank): the first block also publishes the vertex counts (what k_set_counts does) and, with
   finalizeBox, turns the box K1 accumulated into floats -- two one-lane launches less per iteration */
/* S = DScene, or WithGgx<DScene> for a scene with GGX lobes: the continuation probability of a stored vertex depends on the
   lobe.  (As in k_merge_pairs the text stands in the kernel, not in an inlined body: there the workgroup's size is loaded by
   the longer sequence for partial workgroups, which cost each of these kernels a VGPR -- DESIGN.md "Microfacet materials", Kinds.) */
template <class S>
__global__ void __launch_bounds__(256) k_compact_records(const DScene *__restrict__ scp, IterParams P, LightStore store, const int *__restrict__ pathStart,
                                  float *records, int *slotOfVertex, int writeRecords, GridHeader *hdr, const int *localTotal, int finalizeBox)
{
    if (hdr && blockIdx.x == 0 && threadIdx.x < 3) {
        const int n = *localTotal;
        if (threadIdx.x == 0) { hdr->nLocalRecords = n; hdr->nRecords = n; }
        if (finalizeBox) bbox_finalize_component(hdr, (int)threadIdx.x, n, 1);
    }
    /* one lane per light path: slot reads are coalesced across the wave for every j (slot-major store) */
    for (int lp = blockIdx.x * blockDim.x + threadIdx.x; lp < P.nLocal; lp += gridDim.x * blockDim.x) {
        const int n = (int)store.count[lp];
        const int base = pathStart[lp];
        for (int j = 0; j < n; j++) {
            const size_t slot = (size_t)j * (size_t)P.nLocal + (size_t)lp;
            const int vtx = base + j;
            slotOfVertex[vtx] = (int)slot;   /* dense vertex list for k_connect_camera */
            if (!writeRecords) continue;
            const F4 a = lv(store, slot, 0), b = lv(store, slot, 1), d = lv(store, slot, 3);
            const F4 e = light_vertex_wdir_contprob(*static_cast<const S *>(scp), a, lv(store, slot, 2), d, false);
            float *r = records + (size_t)vtx * VCM_MERGE_RECORD_FLOATS;
            r[0] = a.x; r[1] = a.y; r[2] = a.z;
            r[3] = e.x; r[4] = e.y; r[5] = e.z;
            r[6] = b.x; r[7] = b.y; r[8] = b.z;
            r[9] = b.w; r[10] = d.w; r[11] = e.w;
            r[12] = u2f(f2u(a.w) & 0xffu);
        }
    }
}

/* ---------------- K1c: connect every stored light vertex to the camera ---- */
/* vertexcm.hxx:380-384 / :862-933, one lane per stored vertex (dense list, which
 * is the reference's vertex order): BSDF evaluation, MIS weight, one shadow
 * ray.  The splat is NOT added here: Framebuffer::AddColor (:931) runs in
 * vertex order in the reference, and fp32 addition does not commute with
 * rounding, so the splats are written out and K1d adds them per pixel in that
 * order -- bit-identical to the serial loop and reproducible from run to run
 * (fp32 atomics gave an RMSE of 5e-9 and a different image every run). */
template <class SC>
__global__ void __launch_bounds__(256)
k_connect_camera(const DScene *__restrict__ scp, IterParams P, LightStore store,
                 const int *__restrict__ slotOfVertex, const int *__restrict__ nVertices, float *fb, F4 *splat,
                 int *pixCount, int *arrival, unsigned long long *gstats)
{
    const SC &sc = *static_cast<const SC *>(scp);
    stage_scene_tables(sc);
    const int n = *nVertices;
    LaneStats ls; lane_stats_zero(ls);
    /* the place of a splat in its pixel's list comes back from a returning atomic: it is stored one task later, so
       that the wave does not wait for the round trip at the end of every task */
    int pendI = -1, pendArrival = 0;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        F4 sp;
        connect_stored_vertex_to_camera(sc, P, store, (size_t)slotOfVertex[i], fb, ls, &sp);
        if (pendI >= 0) arrival[pendI] = pendArrival;
        pendI = -1;
        splat[i] = sp;
        if (f2u(sp.w) != 0xffffffffu) { pendI = i; pendArrival = atomicAdd(&pixCount[f2u(sp.w)], 1); }
    }
    if (pendI >= 0) arrival[pendI] = pendArrival;
    flush_stats(ls, gstats);
}

/* ---------------- K1d: ordered application of the light splats ------------ */
/* the scatter moves the splat VALUE (rgb | vertex index) into its pixel's segment, so that k_splat_apply reads
 * one contiguous run per pixel instead of gathering 16 bytes per splat from all over the vertex-ordered array */
__global__ void __launch_bounds__(256) k_splat_scatter(const F4 *__restrict__ splat, const int *__restrict__ nVertices,
                                const int *__restrict__ pixStart, const int *__restrict__ arrival, F4 *list, int *longCount)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) *longCount = 0;   /* k_splat_apply's queue of long lists (the word is dead by now) */
    const int n = *nVertices;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const F4 s = splat[i];
        const uint32_t pix = f2u(s.w);
        if (pix != 0xffffffffu) list[pixStart[pix] + arrival[i]] = mk4(s.x, s.y, s.z, u2f((uint32_t)i));
    }
}

/* one lane per pixel: its splats in increasing vertex index.  A pixel holds 1.7 splats on average and the
 * kernel is pure latency (the busiest of a wave's 64 pixels has ~7): up to VCM_SPLAT_REG entries are loaded
 * ONCE, all loads in flight together, and ordered in registers by rank (number of smaller indices); up to
 * VCM_SPLAT_LONG the lane selects the next index k times; longer lists -- the pixels a caustic lands on: a thousand
 * and more splats -- go to k_splat_apply_long, one WAVE per pixel (sending every list above 8 there cost 0.7 ms at
 * 2048^2, r02y: a wave per pixel and a fence per pixel for lists of a dozen).
 * (They used to take a per-lane selection loop here, quadratic in the list length on ONE lane: 5.2 of the 11.5 ms of an
 * iteration of the 10 380-triangle room, profiles/archive/r02w.) */
#define VCM_SPLAT_REG 8
#define VCM_SPLAT_LONG 48   /* up to here a lane orders its list by selection (k^2 / 2 loads that hit the cache) */
__global__ void __launch_bounds__(256) k_splat_apply(int N, const int *__restrict__ pixStart, const F4 *__restrict__ list, float *fb,
                              int *longPix, int *longCount, int longThreshold /* VCM_SPLAT_LONG; tests lower it */)
{
    for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < N; p += gridDim.x * blockDim.x) {
        const int lo = pixStart[p], hi = pixStart[p + 1];
        const int k = hi - lo;
        if (k == 0) continue;
        if (k > longThreshold) { longPix[atomicAdd(longCount, 1)] = p; continue; }
        float r = fb[(size_t)p * 3 + 0], g = fb[(size_t)p * 3 + 1], b = fb[(size_t)p * 3 + 2];
        if (k > VCM_SPLAT_REG) {   /* selection: the next larger vertex index, k times */
            int last = -1;
            for (int t = lo; t < hi; t++) {
                int best = 0x7fffffff, at = lo;
                for (int q = lo; q < hi; q++) {
                    const int v = (int)f2u(list[q].w);
                    if (v > last && v < best) { best = v; at = q; }
                }
                const F4 s = list[at];
                r = r + s.x; g = g + s.y; b = b + s.z;
                last = best;
            }
            fb[(size_t)p * 3 + 0] = r; fb[(size_t)p * 3 + 1] = g; fb[(size_t)p * 3 + 2] = b;
            continue;
        }
        F4 e[VCM_SPLAT_REG];
#pragma unroll
        for (int j = 0; j < VCM_SPLAT_REG; j++) e[j] = (j < k) ? list[lo + j] : mk4(0.f, 0.f, 0.f, u2f(0x7fffffffu));
        int rank[VCM_SPLAT_REG];
#pragma unroll
        for (int j = 0; j < VCM_SPLAT_REG; j++) {
            int c = 0;
#pragma unroll
            for (int m = 0; m < VCM_SPLAT_REG; m++) c += ((int)f2u(e[m].w) < (int)f2u(e[j].w)) ? 1 : 0;
            rank[j] = c;   /* indices are distinct, padding sorts last */
        }
#pragma unroll
        for (int t = 0; t < VCM_SPLAT_REG; t++) {
            if (t < k) {
                float sx = 0.f, sy = 0.f, sz = 0.f;
#pragma unroll
                for (int j = 0; j < VCM_SPLAT_REG; j++) {
                    const bool me = rank[j] == t;
                    sx = me ? e[j].x : sx; sy = me ? e[j].y : sy; sz = me ? e[j].z : sz;
                }
                r = r + sx; g = g + sy; b = b + sz;   /* framebuffer.hxx:56 */
            }
        }
        fb[(size_t)p * 3 + 0] = r; fb[(size_t)p * 3 + 1] = g; fb[(size_t)p * 3 + 2] = b;
    }
}

/* One wave per pixel with a long list: (1) every entry's rank = the number of entries of the list with a smaller
 * vertex index -- lane l ranks entries l, l + 64, ... against the list, read 64 keys at a time and passed round with
 * v_readlane, k^2 / 64 comparisons per lane instead of k^2 on one lane; (2) the entry goes to its place in `sorted`
 * (the vertex-ordered splat array, dead since the scatter); (3) the sum in that order -- Framebuffer::AddColor in
 * the order of the serial light loop (vertexcm.hxx:931) -- 64 entries per load, added one after the other. */
__global__ void __launch_bounds__(256) k_splat_apply_long(const int *__restrict__ pixStart, const F4 *__restrict__ list, F4 *sorted,
                                                        float *fb, const int *__restrict__ longPix, const int *__restrict__ longCount)
{
#if defined(__HIP_DEVICE_COMPILE__)
    const int nLong = *longCount;
    const int lane = (int)lane_id();
    const int wave = (int)((blockIdx.x * blockDim.x + threadIdx.x) / VCM_WAVE), nWaves = (int)(gridDim.x * blockDim.x / VCM_WAVE);
    for (int w = wave; w < nLong; w += nWaves) {
        const int p = longPix[w];
        const int lo = pixStart[p], k = pixStart[p + 1] - lo;
        for (int jb = 0; jb < k; jb += VCM_WAVE) {
            const int j = jb + lane;
            F4 ej = mk4(0.f, 0.f, 0.f, 0.f);
            if (j < k) ej = list[lo + j];
            const int vj = (j < k) ? (int)f2u(ej.w) : 0x7fffffff;
            int rank = 0;
            for (int mb = 0; mb < k; mb += VCM_WAVE) {
                const int m = mb + lane;
                const int vm = (m < k) ? (int)f2u(list[lo + m].w) : 0x7fffffff;   /* padding is smaller than nothing */
#pragma unroll
                for (int t = 0; t < VCM_WAVE; t++) rank += (__builtin_amdgcn_readlane(vm, t) < vj) ? 1 : 0;
            }
            if (j < k) sorted[lo + rank] = ej;
        }
        __threadfence();   /* the wave reads back what its lanes wrote */
        float r = fb[(size_t)p * 3 + 0], g = fb[(size_t)p * 3 + 1], b = fb[(size_t)p * 3 + 2];
        for (int cb = 0; cb < k; cb += VCM_WAVE) {
            F4 e = mk4(0.f, 0.f, 0.f, 0.f);
            if (cb + lane < k) {   /* after the fence: not from a stale L1 line */
                typedef float vf4 __attribute__((ext_vector_type(4)));
                const vf4 v = __builtin_nontemporal_load((const vf4 *)&sorted[lo + cb + lane]);
                e = mk4(v.x, v.y, v.z, v.w);
            }
            const int cnt = min(VCM_WAVE, k - cb);
            for (int t = 0; t < cnt; t++) {   /* framebuffer.hxx:56, in vertex order; every lane keeps the same sum */
                r = r + __shfl(e.x, t, VCM_WAVE); g = g + __shfl(e.y, t, VCM_WAVE); b = b + __shfl(e.z, t, VCM_WAVE);
            }
        }
        if (lane == 0) { fb[(size_t)p * 3 + 0] = r; fb[(size_t)p * 3 + 1] = g; fb[(size_t)p * 3 + 2] = b; }
    }
#endif
}

__global__ void k_set_counts(GridHeader *hdr, const int *localTotal, int useLocalAsGlobal, int globalTotal, StampArgs st)
{
    stamp_entry(st);
    hdr->nLocalRecords = *localTotal;
    hdr->nRecords = useLocalAsGlobal ? *localTotal : globalTotal;
}

/* ---------------- K2: hash-grid build (hashgrid.hxx:41-107) ------------- */

/* Where the grid build reads the light vertices from: the contiguous 13-float merge records (a sharded
 * renderer: the all-gathered array) or, for a single-rank renderer, the slot-major store of K1 itself through
 * the dense vertex -> slot table -- the records are then never materialised (0.6 ms at 2048^2). */
struct VertexSource {
    const float *records;      /* NULL: read the store */
    LightStore store;
    const int *slotOfVertex;
};
__device__ __forceinline__ V3 source_position(const VertexSource &src, int i)
{
    if (src.records) { const float *r = src.records + (size_t)i * VCM_MERGE_RECORD_FLOATS; return mk3(r[0], r[1], r[2]); }
    const F4 a = lv(src.store, src.slotOfVertex[i], 0);
    return mk3(a.x, a.y, a.z);
}

__global__ void k_grid_init(GridHeader *hdr, StampArgs st)
{
    stamp_entry(st);
    if (threadIdx.x < 3) { hdr->bboxMinU[threadIdx.x] = 0xffffffffu; hdr->bboxMaxU[threadIdx.x] = 0u; }
}

__global__ void __launch_bounds__(256) k_bbox(VertexSource src, GridHeader *hdr)
{   /* :50-61.  min/max are exact and order-free; one atomic set per BLOCK (wave shuffle, then LDS):
       per-wave atomics on six hot words cost 0.5 ms at 8192 waves */
    const int n = hdr->nRecords;
    uint32_t mn[3] = { 0xffffffffu, 0xffffffffu, 0xffffffffu }, mx[3] = { 0u, 0u, 0u };
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const V3 pos = source_position(src, i);
        const float r[3] = { pos.x, pos.y, pos.z };
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const uint32_t k = float_order_key(r[c]);
            mn[c] = min(mn[c], k);
            mx[c] = max(mx[c], k);
        }
    }
    __shared__ uint32_t smn[4][3], smx[4][3];
    const int w = threadIdx.x / VCM_WAVE;
#pragma unroll
    for (int c = 0; c < 3; c++) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            mn[c] = min(mn[c], (uint32_t)__shfl_xor((int)mn[c], o, 64));
            mx[c] = max(mx[c], (uint32_t)__shfl_xor((int)mx[c], o, 64));
        }
        if (lane_id() == 0) { smn[w][c] = mn[c]; smx[w][c] = mx[c]; }
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        const int c = threadIdx.x;
        const uint32_t a = min(min(smn[0][c], smn[1][c]), min(smn[2][c], smn[3][c]));
        const uint32_t b = max(max(smx[0][c], smx[1][c]), max(smx[2][c], smx[3][c]));
        atomicMin(&hdr->bboxMinU[c], a);
        atomicMax(&hdr->bboxMaxU[c], b);
    }
}

__global__ void k_bbox_finalize(GridHeader *hdr, int minInverted /* the words K1 left: minimum as ~key */)
{
    if (threadIdx.x < 3) bbox_finalize_component(hdr, (int)threadIdx.x, hdr->nRecords, minInverted);
}

__global__ void __launch_bounds__(256) k_cell_count(IterParams P, VertexSource src, const GridHeader *__restrict__ hdr,
                             int *cellId, int *arrival, int *cellCount, StampArgs st)
{
    stamp_entry(st);   /* :67-71 */
    const int n = hdr->nRecords;
    const V3 bmin = ld3(hdr->bboxMin);
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const int cell = grid_cell_of_point(source_position(src, i), bmin, P.invCellSize, P.nCells);
        cellId[i] = cell;
        arrival[i] = atomicAdd(&cellCount[cell], 1);
    }
}

/* list entry of a cell: everything k_cell_rank_gather needs about the vertex, in one 16-byte element -- one random
 * write here instead of three dependent random 4-byte reads (cell id, slot, then the data) per vertex there */
__global__ void __launch_bounds__(256) k_cell_scatter(const GridHeader *__restrict__ hdr, const int *__restrict__ cellId,
                               const int *__restrict__ arrival, const int *__restrict__ cellStart,
                               const int *__restrict__ slotOfVertex /* NULL: records */, I4 *unsorted)
{   /* :83-88, but in arbitrary order inside a cell; k_cell_rank_gather restores the order */
    const int n = hdr->nRecords;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const int cell = cellId[i];
        I4 e; e.x = i; e.y = slotOfVertex ? slotOfVertex[i] : i; e.z = cell; e.w = 0;
        unsorted[cellStart[cell] + arrival[i]] = e;
    }
}

/* ---- K2 as a radix sort (round 5) ----
 * HashGrid::Build is a stable counting sort of the vertices by cell (hashgrid.hxx:67-88).  The kernels above do it the way the
 * reference does -- one counter per cell -- which on this chip means one device-scope atomic per vertex on a 16.8 MB table (a
 * fabric transaction each), the table's zeroing and 4.2 M-entry scan, a random 16-byte write per vertex and a ranking pass that
 * re-reads every cell: 4.65 GB and 1.23 ms for 0.64 GB of design bytes (VERDICT r4 "weak" 4; this build: 3.8 GB, 0.93 ms, of
 * which the two reads of the 64-byte store records are 2.7 GB).  The same order comes out of a stable LSD
 * radix sort of (cell, vertex) over the cell id's bits, 8 at a time, starting from the vertices in index order:
 *   k_cell_keys      key[v] = cell, pay[v] = {v, slot} (+ the first digit's histogram)
 *   per 8-bit digit  k_radix_hist (workgroup b counts the digits of ITS contiguous chunk -> hist[digit][b]), the scan of that
 *                    matrix, k_radix_scatter (the chunk again: stable rank of every entry among its digit inside the chunk --
 *                    wave by wave with ballots, no atomics --, entries staged by digit in LDS, written out in runs)
 *   k_cell_starts    cellStart from the sorted keys (a vertex whose key differs from its predecessor's starts every cell in between)
 * and k_cell_rank_gather / k_cell_rank_pack read the sorted {v, slot} list: their position IS the destination. */
struct alignas(8) I2 { int x, y; };
#define VCM_RSORT_TILE 2048   /* entries staged per round of a workgroup: 30 KB of LDS, five workgroups per CU */
__device__ __forceinline__ int radix_chunk(int n, int V) { return (((n + V - 1) / V) + 255) & ~255; }

/* workgroup b: the keys of ITS chunk of the vertices (the chunks of the sort's first pass) and, while they are at hand, the
   histogram of their first digit */
__global__ void __launch_bounds__(256) k_cell_keys(IterParams P, VertexSource src, const GridHeader *__restrict__ hdr, uint32_t *key, I2 *pay,
                                                    int *hist /* [digit * V + workgroup], digit = key & 255 */, StampArgs st)
{
    stamp_entry(st);   /* :67-71, without the count */
    __shared__ int sH[256];
    const int tid = (int)threadIdx.x, n = hdr->nRecords, V = (int)gridDim.x;
    const int chunk = radix_chunk(n, V);
    const long long lo64 = (long long)blockIdx.x * chunk;
    const int lo = lo64 < n ? (int)lo64 : n, hi = (n - lo < chunk) ? n : lo + chunk;
    const V3 bmin = ld3(hdr->bboxMin);
    sH[tid] = 0;
    __syncthreads();
    for (int i = lo + tid; i < hi; i += 256) {
        /* (vertex order is path-major and most paths store one vertex: neighbouring lanes read neighbouring slots) */
        const int slot = src.records ? i : src.slotOfVertex[i];
        V3 pos;
        if (src.records) { const float *r = src.records + (size_t)i * VCM_MERGE_RECORD_FLOATS; pos = mk3(r[0], r[1], r[2]); }
        else { const F4 a = lv(src.store, (size_t)slot, 0); pos = mk3(a.x, a.y, a.z); }
        const uint32_t cell = (uint32_t)grid_cell_of_point(pos, bmin, P.invCellSize, P.nCells);
        key[i] = cell;
        I2 e; e.x = i; e.y = slot;
        pay[i] = e;
        atomicAdd(&sH[cell & 255u], 1);
    }
    __syncthreads();
    hist[tid * V + (int)blockIdx.x] = sH[tid];
}

__global__ void __launch_bounds__(256) k_radix_hist(const uint32_t *__restrict__ key, const GridHeader *__restrict__ hdr, int shift, int *hist /* [digit * V + workgroup] */)
{
    __shared__ int sH[256];
    const int tid = (int)threadIdx.x, n = hdr->nRecords, V = (int)gridDim.x;
    const int chunk = radix_chunk(n, V);
    const long long lo64 = (long long)blockIdx.x * chunk;
    const int lo = lo64 < n ? (int)lo64 : n, hi = (n - lo < chunk) ? n : lo + chunk;
    sH[tid] = 0;
    __syncthreads();
    for (int i = lo + tid; i < hi; i += 256) atomicAdd(&sH[(key[i] >> shift) & 255u], 1);
    __syncthreads();
    hist[tid * V + (int)blockIdx.x] = sH[tid];
}

__global__ void __launch_bounds__(256) k_radix_scatter(const uint32_t *__restrict__ keyIn, const I2 *__restrict__ payIn, uint32_t *keyOut, I2 *payOut,
                                                        const GridHeader *__restrict__ hdr, int shift, const int *__restrict__ histScanned)
{
#if defined(__HIP_DEVICE_COMPILE__)
    __shared__ uint32_t sKey[VCM_RSORT_TILE];
    __shared__ I2 sPay[VCM_RSORT_TILE];
    __shared__ int sRun[4][256];     /* per wave and digit: entries so far; after the rounds: where the wave's entries of the digit start in the tile */
    __shared__ int sBinStart[256];   /* where the digit starts in the staged tile */
    __shared__ int sGlobal[256];     /* where this workgroup's next entry of the digit goes in the output */
    __shared__ int sWaveTotal[4];
    const int tid = (int)threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int n = hdr->nRecords, V = (int)gridDim.x;
    const int chunk = radix_chunk(n, V);
    const long long lo64 = (long long)blockIdx.x * chunk;
    const int lo = lo64 < n ? (int)lo64 : n, hi = (n - lo < chunk) ? n : lo + chunk;
    sGlobal[tid] = histScanned[tid * V + (int)blockIdx.x];
    static_assert(VCM_WAVE == 64, "the ballots and `below` are 64-bit lane masks");
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int t0 = lo; t0 < hi; t0 += VCM_RSORT_TILE) {
        const int m = (hi - t0 < VCM_RSORT_TILE) ? hi - t0 : VCM_RSORT_TILE;
        const int q = ((m + 255) >> 8) << 6;   /* entries per wave: contiguous quarters, so wave order = index order */
        sRun[0][tid] = 0; sRun[1][tid] = 0; sRun[2][tid] = 0; sRun[3][tid] = 0;
        __syncthreads();   /* (also: the previous tile's output loop has left sKey / sPay / sBinStart) */
        const int wlo = t0 + w * q, whi = (t0 + m < wlo + q) ? t0 + m : wlo + q;
        uint32_t k[VCM_RSORT_TILE / 256]; I2 p[VCM_RSORT_TILE / 256]; int r[VCM_RSORT_TILE / 256];
        uint32_t validBits = 0;
#pragma unroll
        for (int round = 0; round < VCM_RSORT_TILE / 256; round++) {
            k[round] = 0; p[round].x = 0; p[round].y = 0; r[round] = 0;
            if (round * 64 < q) {   /* wave-uniform */
                const int idx = wlo + round * 64 + lane;
                const bool valid = idx < whi;
                if (valid) { k[round] = keyIn[idx]; p[round] = payIn[idx]; }
                const uint32_t d = (k[round] >> shift) & 255u;
                unsigned long long peers = __ballot(valid);
#pragma unroll
                for (int b = 0; b < 8; b++) {
                    const bool bit = (d >> b) & 1u;
                    const unsigned long long bal = __ballot(bit);
                    peers &= bit ? bal : ~bal;
                }
                const int before = __popcll(peers & below);
                const int run = sRun[w][d];
                r[round] = run + before;
                if (valid && before == 0) sRun[w][d] = run + __popcll(peers);   /* the first lane of the group */
                __builtin_amdgcn_wave_barrier();   /* the next round's loads of sRun[w][*] stay behind this store */
                validBits |= valid ? (1u << round) : 0u;
            }
        }
        __syncthreads();
        {   /* thread = digit: its entries per wave -> its start in the tile (exclusive scan over the 256 digits) */
            const int c0 = sRun[0][tid], c1 = sRun[1][tid], c2 = sRun[2][tid], c3 = sRun[3][tid];
            const int total = c0 + c1 + c2 + c3;
            int incl = total;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_up(incl, o, 64); if (lane >= o) incl += t; }
            if (lane == 63) sWaveTotal[w] = incl;
            __syncthreads();
            int start = incl - total;
#pragma unroll
            for (int x = 0; x < 4; x++) if (x < w) start += sWaveTotal[x];
            sBinStart[tid] = start;
            sRun[0][tid] = start; sRun[1][tid] = start + c0; sRun[2][tid] = start + c0 + c1; sRun[3][tid] = start + c0 + c1 + c2;
            __syncthreads();
            /* stage by digit */
#pragma unroll
            for (int round = 0; round < VCM_RSORT_TILE / 256; round++) {
                if (validBits & (1u << round)) {
                    const uint32_t d = (k[round] >> shift) & 255u;
                    const int pos = sRun[w][d] + r[round];
                    sKey[pos] = k[round];
                    sPay[pos] = p[round];
                }
            }
            __syncthreads();
            for (int j = tid; j < m; j += 256) {
                const uint32_t kk = sKey[j];
                const uint32_t d = (kk >> shift) & 255u;
                const int dst = sGlobal[d] + (j - sBinStart[d]);
                keyOut[dst] = kk;
                payOut[dst] = sPay[j];
            }
            __syncthreads();
            sGlobal[tid] += total;
        }
    }
#endif
}

/* cellStart (hashgrid.hxx:75-81: the exclusive scan of the cell counts) from the sorted keys: cellStart[c] = the first position
   whose key is >= c; position n stands for "key = nCells".  Gaps are ~18 cells on average (most hash cells are empty);
   long ones are filled by the whole wave. */
__global__ void __launch_bounds__(256) k_cell_starts(const uint32_t *__restrict__ key, const GridHeader *__restrict__ hdr, int nCells, int *cellStart)
{
#if defined(__HIP_DEVICE_COMPILE__)
    const int n = hdr->nRecords;
    const int lane = (int)threadIdx.x & 63;
    const int stride = (int)(gridDim.x * blockDim.x);
    for (int base = (int)(blockIdx.x * blockDim.x) + ((int)threadIdx.x & ~63); base <= n; base += stride) {   /* wave-uniform */
        const int pos = base + lane;
        int c0 = 0, len = 0;
        if (pos <= n) {
            const int prev = pos > 0 ? (int)key[pos - 1] : -1;
            const int cur = pos < n ? (int)key[pos] : nCells;
            c0 = prev + 1; len = cur - prev;   /* cells c0 .. cur */
        }
        const int head = len < 8 ? len : 8;
        for (int c = 0; c < head; c++) cellStart[c0 + c] = pos;
        unsigned long long longOnes = __ballot(len > 8);
        while (longOnes) {
            const int l = __ffsll((long long)longOnes) - 1;
            longOnes &= longOnes - 1ull;
            const int s = __shfl(c0 + 8, l, 64), e = __shfl(c0 + len, l, 64), v = __shfl(pos, l, 64);
            for (int c = s + lane; c < e; c += 64) cellStart[c] = v;
        }
    }
#endif
}

/* The reference's counting sort is stable: inside a cell, vertices keep their
 * index order (:83-88), and the merge sums contributions in that order
 * (:157-167).  Rank of vertex i inside its cell = number of vertices of the
 * cell with a smaller index; the vertex data is then written to its final
 * position, so the query reads contiguous, cell-sorted memory and needs no
 * mIndices indirection. */
/* the entry at `pos` of the list ({vertex, slot, ...}) and, in dst, its place in the cell-sorted order */
__device__ __forceinline__ I4 cell_rank_entry(const int *__restrict__ cellStart, const I4 *__restrict__ unsorted, const I2 *__restrict__ sorted, int pos, int &dst)
{
    I4 me;
    dst = pos;
    if (sorted) {   /* the radix sort's list: {vertex, slot} in the grid's final order -- position = destination */
        const I2 e = sorted[pos];
        me.x = e.x; me.y = e.y; me.z = 0; me.w = 0;
    } else {
        me = unsorted[pos];
        const int cell = me.z;
        const int lo = cellStart[cell], hi = cellStart[cell + 1];
        int rank = 0;
        for (int q = lo; q < hi; q++) rank += (unsorted[q].x < me.x) ? 1 : 0;
        dst = lo + rank;
    }
    return me;
}
/* (S, and why the text is the kernel's own: k_compact_records) */
template <class S>
__global__ void __launch_bounds__(256) k_cell_rank_gather(const DScene *__restrict__ scp, const GridHeader *__restrict__ hdr, VertexSource src,
                                   const int *__restrict__ cellStart, const I4 *__restrict__ unsorted, const I2 *__restrict__ sorted,
                                   float *gx, float *gy, float *gz, float *gb, F4 *g1, F4 *g2, F2 *g3, int *sortedIndex)
{
    const int n = hdr->nRecords;
    for (int pos = blockIdx.x * blockDim.x + threadIdx.x; pos < n; pos += gridDim.x * blockDim.x) {
        int dst;
        const I4 me = cell_rank_entry(cellStart, unsorted, sorted, pos, dst);
        const int i = me.x;
        F2 t;
        if (src.records) {
            const float *r = src.records + (size_t)i * VCM_MERGE_RECORD_FLOATS;
            gx[dst] = r[0]; gy[dst] = r[1]; gz[dst] = r[2];
            gb[grid_blocked_index(dst, 0)] = r[0]; gb[grid_blocked_index(dst, 1)] = r[1]; gb[grid_blocked_index(dst, 2)] = r[2];
            g1[dst] = mk4(r[3], r[4], r[5], r[11]);
            g2[dst] = mk4(r[6], r[7], r[8], r[9]);
            t.x = r[10]; t.y = r[12];
        } else {   /* the same 13 values k_compact_records would have written */
            const size_t slot = (size_t)me.y;
            const F4 a = lv(src.store, slot, 0), b = lv(src.store, slot, 1), d = lv(src.store, slot, 3);
            const F4 e = light_vertex_wdir_contprob(*static_cast<const S *>(scp), a, lv(src.store, slot, 2), d, false);   /* (one 64-byte record: one line) */
            gx[dst] = a.x; gy[dst] = a.y; gz[dst] = a.z;
            gb[grid_blocked_index(dst, 0)] = a.x; gb[grid_blocked_index(dst, 1)] = a.y; gb[grid_blocked_index(dst, 2)] = a.z;
            g1[dst] = e;
            g2[dst] = b;
            t.x = d.w; t.y = u2f(f2u(a.w) & 0xffu);
        }
        g3[dst] = t;
        if (sortedIndex) sortedIndex[dst] = i;
    }
}


/* ---------------- K2 of a SHARDED renderer: sort locally, exchange, merge by cell block (round 5) ---------------- */
/* North_star's decomposition all-gathers every rank's light vertices before the grid build.  Rounds 2-4 then ran the WHOLE
 * build -- cell count with 8.9 M scattered atomics, scan, scatter, in-cell ranking -- on EVERY rank over ALL vertices: ~3 ms
 * of serialised kernels at 2048^2 that do not shrink with the number of GPUs (the builder's own estimate: 3.3 x at 8 GPUs).
 * The reference's order makes a cheaper protocol exact: path-index blocks are contiguous per rank, so a cell's vertices in
 * HashGrid::Build's stable order (by vertex index, hashgrid.hxx:83-88) are rank 0's in local order, then rank 1's, ...
 *   sender:    counting sort of its OWN vertices by cell (the kernels above, 1 / S of the work) -> its records in cell
 *              order + localStart[b * K] for every block b of K cells (k_cell_rank_pack);
 *   exchange:  ONE all-gather of those slabs (52 B per vertex + 4 B per K cells: no histograms travel);
 *   receiver:  k_grid_merge_blocks -- one workgroup per block of K cells streams the S segments that fall into its cells
 *              (contiguous in every rank's slab), counts (cell, rank) runs in LDS, scans them cell-major / rank-minor and
 *              writes the block's contiguous piece of the final cell-sorted arrays and of cellStart.  No global scan
 *              (cellStart[c] = sum over ranks of localStart_r[c]), no atomics on global memory, no gathers.
 * A record's 13th word carries the path length (8 bits) and the vertex's index in its rank's reference order (24 bits):
 * the parity read-out wants sortedIndex (grid position -> vertex index); a shard of 2^24 vertices or more keeps the
 * unsorted exchange (vcm_sort_light_records refuses). */
#define VCM_SORTED_WORDS 13
#define VCM_SORTED_MAX_SHARDS 64   /* SortedSlabs::rankBase, k_grid_merge_blocks' sSeg; more shards: the unsorted exchange */
#define VCM_SORTED_MAX_TABLE 4096   /* K * S entries per LDS table */
inline __host__ __device__ int sorted_block_cells(int S)
{   /* K: the largest power of two <= 4096 / S, within [16, 1024] */
    const int k = VCM_SORTED_MAX_TABLE / (S > 0 ? S : 1);
    int p = 16;
    while (p * 2 <= k && p < 1024) p *= 2;
    return p;
}

/* k_cell_rank_gather for the exchange: the vertex's 13 words go to its place in the cell-sorted SLAB (array of records),
 * and the table of block starts behind it */
template <class S>
__global__ void __launch_bounds__(256) k_cell_rank_pack(const DScene *__restrict__ scp, const GridHeader *__restrict__ hdr, VertexSource src,
                                 const int *__restrict__ cellStart, const I4 *__restrict__ unsorted, const I2 *__restrict__ sorted,
                                 uint32_t *slab, int *blockStart, int nCells, int K, int nBlocks)
{
    const int n = hdr->nRecords;
    for (int b = blockIdx.x * blockDim.x + threadIdx.x; b <= nBlocks; b += gridDim.x * blockDim.x) {
        const long long c = (long long)b * K;
        blockStart[b] = cellStart[c < nCells ? (int)c : nCells];
    }
    for (int pos = blockIdx.x * blockDim.x + threadIdx.x; pos < n; pos += gridDim.x * blockDim.x) {
        int dst;
        const I4 me = cell_rank_entry(cellStart, unsorted, sorted, pos, dst);
        const int i = me.x;
        uint32_t *r = slab + (size_t)dst * VCM_SORTED_WORDS;
        float w[13];
        if (src.records) {
            const float *q = src.records + (size_t)i * VCM_MERGE_RECORD_FLOATS;
#pragma unroll
            for (int k = 0; k < 13; k++) w[k] = q[k];
        } else {
            const size_t slot = (size_t)me.y;
            const F4 a = lv(src.store, slot, 0), b = lv(src.store, slot, 1), d = lv(src.store, slot, 3);
            const F4 e = light_vertex_wdir_contprob(*static_cast<const S *>(scp), a, lv(src.store, slot, 2), d, false);
            w[0] = a.x; w[1] = a.y; w[2] = a.z; w[3] = e.x; w[4] = e.y; w[5] = e.z; w[6] = b.x; w[7] = b.y; w[8] = b.z;
            w[9] = b.w; w[10] = d.w; w[11] = e.w; w[12] = u2f(f2u(a.w) & 0xffu);
        }
#pragma unroll
        for (int k = 0; k < 12; k++) r[k] = f2u(w[k]);
        r[12] = (f2u(w[12]) & 0xffu) | ((uint32_t)i << 8);
    }
}

struct SortedSlabs {
    const uint32_t *base;        /* S slabs of slabWords words: [stride records of 13 words][nBlocks + 1 block starts] */
    long long slabWords, strideRecords;
    int S, K, nBlocks;
    int rankBase[VCM_SORTED_MAX_SHARDS + 1];            /* vertices of the ranks before r (r = 0 .. S): global index of rank r's first vertex */
};

__global__ void __launch_bounds__(256) k_grid_merge_blocks(IterParams P, const GridHeader *__restrict__ hdr, SortedSlabs in,
                                    int *cellStart, float *gx, float *gy, float *gz, float *gb, F4 *g1, F4 *g2, F2 *g3, int *sortedIndex, StampArgs st)
{
#if defined(__HIP_DEVICE_COMPILE__)
    stamp_entry(st);
    __shared__ int sCnt[VCM_SORTED_MAX_TABLE];     /* [cell][rank]: run length, then (scanned in place) the run's offset in the block's output */
    __shared__ int sFirst[VCM_SORTED_MAX_TABLE];   /* [cell][rank]: slab index of the run's first record */
    __shared__ int sSeg[2 * VCM_SORTED_MAX_SHARDS + 2];               /* per rank: segment start, end; [128] = output start of the block, [129] = records */
    __shared__ int sPart[256];
    const int tid = (int)threadIdx.x, S = in.S, K = in.K;
    const V3 bmin = ld3(hdr->bboxMin);
    for (int b = (int)blockIdx.x; b < in.nBlocks; b += (int)gridDim.x) {
        const int c0 = b * K, c1 = min(P.nCells, c0 + K), nc = c1 - c0, T = nc * S;
        __syncthreads();   /* the previous block's tables are no longer read */
        if (tid < S) {
            const int *bs = (const int *)(in.base + (size_t)tid * (size_t)in.slabWords + (size_t)in.strideRecords * VCM_SORTED_WORDS);
            sSeg[2 * tid] = bs[b]; sSeg[2 * tid + 1] = bs[b + 1];
        }
        for (int i = tid; i < T; i += 256) { sCnt[i] = 0; sFirst[i] = 0x7fffffff; }
        __syncthreads();
        if (tid == 0) { int g = 0, m = 0; for (int r = 0; r < S; r++) { g += sSeg[2 * r]; m += sSeg[2 * r + 1] - sSeg[2 * r]; } sSeg[128] = g; sSeg[129] = m; }
        /* pass 1: run lengths and run heads */
        for (int r = 0; r < S; r++) {
            const uint32_t *slab = in.base + (size_t)r * (size_t)in.slabWords;
            const int s = sSeg[2 * r], e = sSeg[2 * r + 1];
            for (int i = s + tid; i < e; i += 256) {
                const uint32_t *q = slab + (size_t)i * VCM_SORTED_WORDS;
                const int cell = grid_cell_of_point(mk3(u2f(q[0]), u2f(q[1]), u2f(q[2])), bmin, P.invCellSize, P.nCells);
                const int k = (cell - c0) * S + r;   /* the sender sorted with the same function: c0 <= cell < c1 */
                atomicAdd(&sCnt[k], 1);
                atomicMin(&sFirst[k], i);
            }
        }
        __syncthreads();
        /* exclusive scan of the T run lengths in (cell, rank) order, in place: <= 16 consecutive entries per thread */
        const int per = (T + 255) / 256, lo = tid * per, hi = min(T, lo + per);
        int sum = 0;
        for (int i = lo; i < hi; i++) sum += sCnt[i];
        sPart[tid] = sum;
        __syncthreads();
        if (tid < 64) {   /* 256 partial sums: four per lane of the first wave, one wave scan */
            const int a0 = sPart[4 * tid], a1 = sPart[4 * tid + 1], a2 = sPart[4 * tid + 2], a3 = sPart[4 * tid + 3];
            const int mine = a0 + a1 + a2 + a3;
            int incl = mine;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_up(incl, o, 64); if (tid >= o) incl += t; }
            const int ex = incl - mine;
            sPart[4 * tid] = ex; sPart[4 * tid + 1] = ex + a0; sPart[4 * tid + 2] = ex + a0 + a1; sPart[4 * tid + 3] = ex + a0 + a1 + a2;
        }
        __syncthreads();
        {
            int run = sPart[tid];
            for (int i = lo; i < hi; i++) { const int c = sCnt[i]; sCnt[i] = run; run += c; }
        }
        __syncthreads();
        const int g0 = sSeg[128];
        /* the cells' starts: the offset of rank 0's run (hashgrid.hxx:75-81: the exclusive prefix over cells) */
        for (int c = tid; c < nc; c += 256) cellStart[c0 + c] = g0 + sCnt[c * S];
        if (c1 == P.nCells && tid == 0) cellStart[P.nCells] = g0 + sSeg[129];
        /* pass 2: every record to its place */
        for (int r = 0; r < S; r++) {
            const uint32_t *slab = in.base + (size_t)r * (size_t)in.slabWords;
            const int s = sSeg[2 * r], e = sSeg[2 * r + 1];
            for (int i = s + tid; i < e; i += 256) {
                const uint32_t *q = slab + (size_t)i * VCM_SORTED_WORDS;
                uint32_t w[13];
#pragma unroll
                for (int k = 0; k < 13; k++) w[k] = q[k];
                const int cell = grid_cell_of_point(mk3(u2f(w[0]), u2f(w[1]), u2f(w[2])), bmin, P.invCellSize, P.nCells);
                const int k = (cell - c0) * S + r;
                const int dst = g0 + sCnt[k] + (i - sFirst[k]);
                gx[dst] = u2f(w[0]); gy[dst] = u2f(w[1]); gz[dst] = u2f(w[2]);
                gb[grid_blocked_index(dst, 0)] = u2f(w[0]); gb[grid_blocked_index(dst, 1)] = u2f(w[1]); gb[grid_blocked_index(dst, 2)] = u2f(w[2]);
                g1[dst] = mk4(u2f(w[3]), u2f(w[4]), u2f(w[5]), u2f(w[11]));
                g2[dst] = mk4(u2f(w[6]), u2f(w[7]), u2f(w[8]), u2f(w[9]));
                F2 t; t.x = u2f(w[10]); t.y = u2f(w[12] & 0xffu);
                g3[dst] = t;
                if (sortedIndex) sortedIndex[dst] = in.rankBase[r] + (int)(w[12] >> 8);
            }
        }
    }
#endif
}

} // namespace vcm
#endif
