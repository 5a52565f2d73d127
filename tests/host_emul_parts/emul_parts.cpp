// TEST INFRASTRUCTURE.  A serial host build of the WAVEFRONT functions of smallvcm_amd/csrc/vcm_core.h and of the split of
// smallvcm_amd/csrc/vcm_parts.h: what a context with vcm_track_parts on computes, kernel by kernel, on one host thread --
//   K1   light_path_step<1>            the light vertices go to the store, nothing is splatted
//   K1c  connect_stored_vertex_to_camera, the splat list in vertex order; K1d adds it per pixel in that order
//   K2   the hash grid (as tests/host_emul builds it)
//   K3   camera_path_step<1> into a host VertexStore: records, DI and VC tasks
//   K3b / K3c / K4  eval_di_task, eval_vc_task, eval_merge_task over the task lists
//   K5   replay_path_color for the framebuffer, parts_resolve_pixel for the planes
// and the statistic of vcm_get_parts_stats on the kernels' grid.  tests/host_emul runs the same device functions in strict
// order; tests/test_parts.py ties the two framebuffers together bit for bit.  This is not a fallback: it is never built
// into libsmallvcm_amd.so and nothing in the package loads it.  The scene is built by scene_host.h, which reads
// SMALLVCM_AMD_NO_ONEPLANE and SMALLVCM_AMD_FORCE_BVH as tests/host_emul does (SMALLVCM_AMD_GENERAL_POW changes no bit).
#include <vector>
#include <string>
#include <algorithm>
#include <string.h>
#include "../../smallvcm_amd/csrc/vcm_parts.h"
#include "../../smallvcm_amd/csrc/scene_host.h"

using namespace vcm;

/* the ray-casting functions are instantiated per kind of scene: pick like the product's launches do */
template <class F> static void with_scene(const DScene &sc, F &&f)
{
    if (sc.nNodes > 0) f(static_cast<const SceneBvh &>(sc));
    else if (sc.fastOnePlane && sc.nFastRects[0] + sc.nFastRects[1] + sc.nFastRects[2] > 0) f(static_cast<const SceneRects &>(sc));
    else if (sc.fastOnePlane) f(static_cast<const SceneQuads &>(sc));
    else f(static_cast<const SceneList &>(sc));
}

struct PartsEmul {
    SceneHost host;
    DScene sc;   /* offsets from THIS object into `host` (a PartsEmul never moves) */
    bool useVM, useVC, lightTraceOnly, ppm;
    float baseRadius, radiusAlpha;
    int seed, iterations;
    int resX, resY, N;
    std::vector<float> fb, parts;   /* N x 3; VCM_PART_COUNT planes of N x 3 */
    long long lastSplats, lastMaxPerPixel, maxSplats;   /* of the last iteration: splats, the longest list; the most splats of any iteration */
    LaneStats ls;
};

extern "C" {

void *emul_parts_create(const vcm_scene_desc *scene, int algorithm, float radiusFactor, float radiusAlpha, int seed)
{
    if (algorithm < VCM_ALGO_LIGHT_TRACE || algorithm > VCM_ALGO_VCM) return NULL;   /* the VertexCM algorithms */
    PartsEmul *e = new PartsEmul();
    std::string err;
    if (!scene_host_from_desc(*scene, e->host, err)) { delete e; return NULL; }
    scene_host_build_accel(e->host, scene_host_force_bvh());
    e->host.view(e->sc);
    e->useVM = e->useVC = e->lightTraceOnly = e->ppm = false;
    switch (algorithm) {
    case VCM_ALGO_LIGHT_TRACE: e->lightTraceOnly = true; break;
    case VCM_ALGO_PPM: e->ppm = true; e->useVM = true; break;
    case VCM_ALGO_BPM: e->useVM = true; break;
    case VCM_ALGO_BPT: e->useVC = true; break;
    default: e->useVC = true; e->useVM = true; break;
    }
    if (e->ppm) {
        for (size_t i = 0; i < e->host.materials.size(); i++) {
            const vcm_material &m = e->host.materials[i];
            if (((vmax3(ld3(m.diffuse)) > 0) || (vmax3(ld3(m.phong)) > 0)) && ((vmax3(ld3(m.mirror)) > 0) || (m.ior > 0))) {
                e->ppm = false; break;
            }
        }
    }
    e->baseRadius = radiusFactor * e->host.sceneRadius;
    e->radiusAlpha = radiusAlpha;
    e->seed = seed; e->iterations = 0;
    e->resX = (int)e->host.camera.resolution[0]; e->resY = (int)e->host.camera.resolution[1];
    e->N = e->resX * e->resY;
    e->fb.assign((size_t)e->N * 3, 0.f);
    e->parts.assign((size_t)VCM_PART_COUNT * e->N * 3, 0.f);
    e->lastSplats = e->lastMaxPerPixel = e->maxSplats = 0;
    return e;
}
void emul_parts_destroy(void *h) { delete (PartsEmul *)h; }

int emul_parts_run_iteration(void *h, int iteration, unsigned minLen, unsigned maxLen)
{
    PartsEmul &e = *(PartsEmul *)h;
    if (maxLen > 31) return -1;   /* the iteration would not be wavefront */
    const int N = e.N, nLocal = N;
    IterParams P;
    memset(&P, 0, sizeof(P));
    const int S = (maxLen >= 2) ? (int)maxLen - 1 : 1;
    const int L = (maxLen >= 1) ? (int)maxLen : 1;
    P.seed = (uint32_t)e.seed; P.localIter = (uint32_t)e.iterations;
    P.minLen = minLen; P.maxLen = maxLen;
    P.resX = e.resX; P.resY = e.resY; P.N = N; P.p0 = 0; P.nLocal = nLocal; P.S = S;
    P.useVM = e.useVM; P.useVC = e.useVC; P.lightTraceOnly = e.lightTraceOnly; P.ppm = e.ppm;
    P.lightSubPathCount = float(e.resX * e.resY);
    float radius = e.baseRadius;
    radius /= dm_powf(float(iteration + 1), 0.5f * (1 - e.radiusAlpha));
    radius = smax(radius, 1e-7f);
    const float radiusSqr = sqr(radius);
    P.radius = radius; P.radiusSqr = radiusSqr;
    P.vmNormalization = 1.f / (radiusSqr * VCM_PI_F * P.lightSubPathCount);
    const float etaVCM = (VCM_PI_F * radiusSqr) * P.lightSubPathCount;
    P.misVmWeightFactor = e.useVM ? mis(etaVCM) : 0.f;
    P.misVcWeightFactor = e.useVC ? mis(1.f / etaVCM) : 0.f;
    P.cellSize = radius * 2.f;
    P.invCellSize = 1.f / P.cellSize;
    P.nCells = N;
    P.wavefront = e.lightTraceOnly ? 0 : 1;
    P.renderer = 0; P.iteration = iteration;
    P.qblockVertex = P.qblockDI = 256; P.qblockVC = 512; P.nBuckets = 1 << 18;   /* (the host allocator is a counter, and there is no query sort) */
    lane_stats_zero(e.ls);

    /* K1: the light paths, wavefront mode */
    const size_t slots = (size_t)S * nLocal;
    std::vector<F4> v0(slots * VCM_LV_FIELDS, mk4(0, 0, 0, 0));
    std::vector<unsigned char> count((size_t)nLocal, 0);
    std::vector<uint32_t> lenMask((size_t)nLocal, 0u);
    LightStore store; store.v = v0.data(); store.count = count.data(); store.lenMask = lenMask.data();
    for (int lp = 0; lp < nLocal; lp++) {
        LightPath path;
        light_path_begin(e.sc, P, path, lp);
        LaneBox box; lane_box_init(box);
        with_scene(e.sc, [&](const auto &sc) { while (light_path_step<1>(sc, P, path, store, (float *)0, e.ls, box)) {} });
        count[lp] = (unsigned char)path.nStored;
        lenMask[lp] = path.lenMask;
    }
    /* K1c / K1d: the splats in the reference's vertex order (path ascending, vertex ascending), added as they come: per pixel
       that is increasing vertex index, to the framebuffer and to the LIGHT_TRACE plane alike */
    e.lastSplats = 0; e.lastMaxPerPixel = 0;
    if (e.useVC || e.lightTraceOnly) {
        std::vector<int> perPixel((size_t)N, 0);
        float *plane = e.parts.data() + (size_t)VCM_PART_LIGHT_TRACE * N * 3;
        for (int lp = 0; lp < nLocal; lp++)
            for (int j = 0; j < count[lp]; j++) {
                F4 sp;
                with_scene(e.sc, [&](const auto &sc) { connect_stored_vertex_to_camera(sc, P, store, (size_t)j * nLocal + lp, (float *)0, e.ls, &sp); });
                const uint32_t pix = f2u(sp.w);
                if (pix == 0xffffffffu) continue;
                float *px = &e.fb[(size_t)pix * 3], *pp = plane + (size_t)pix * 3;
                px[0] = px[0] + sp.x; px[1] = px[1] + sp.y; px[2] = px[2] + sp.z;
                pp[0] = pp[0] + sp.x; pp[1] = pp[1] + sp.y; pp[2] = pp[2] + sp.z;
                e.lastSplats++;
                perPixel[pix]++;
            }
        for (int p = 0; p < N; p++) e.lastMaxPerPixel = std::max(e.lastMaxPerPixel, (long long)perPixel[p]);
    }
    e.maxSplats = std::max(e.maxSplats, e.lastSplats);
    if (e.lightTraceOnly) { e.iterations++; return 0; }

    /* K1b / K2: records in reference order, stable counting sort by cell (tests/host_emul/emul.cpp) */
    std::vector<float> records;
    for (int lp = 0; lp < nLocal; lp++)
        for (int j = 0; j < count[lp]; j++) {
            const size_t slot = (size_t)j * nLocal + lp;
            const F4 a = lv(store, slot, 0), b = lv(store, slot, 1), d = lv(store, slot, 3);
            const F4 w = light_vertex_wdir_contprob(e.sc, a, lv(store, slot, 2), d, false);
            const float r[13] = { a.x, a.y, a.z, w.x, w.y, w.z, b.x, b.y, b.z, b.w, d.w, w.w, u2f(f2u(a.w) & 0xffu) };
            records.insert(records.end(), r, r + 13);
        }
    const int n = (int)(records.size() / 13);
    GridHeader hdr;
    memset(&hdr, 0, sizeof(hdr));
    hdr.nRecords = n;
    for (int c = 0; c < 3; c++) { hdr.bboxMin[c] = 1e36f; hdr.bboxMax[c] = -1e36f; }
    std::vector<int> cellStart((size_t)P.nCells + 1, 0);
    std::vector<float> gx((size_t)n + VCM_MERGE_UNROLL, 0.f), gy = gx, gz = gx;
    std::vector<F4> g1((size_t)n + 1, mk4(0, 0, 0, 0)), g2 = g1;
    F2 z2; z2.x = z2.y = 0.f;
    std::vector<F2> g3((size_t)n + 1, z2);
    if (e.useVM) {
        for (int i = 0; i < n; i++)
            for (int c = 0; c < 3; c++) {
                hdr.bboxMax[c] = smax(hdr.bboxMax[c], records[(size_t)i * 13 + c]);
                hdr.bboxMin[c] = smin(hdr.bboxMin[c], records[(size_t)i * 13 + c]);
            }
        std::vector<int> cell((size_t)n);
        for (int i = 0; i < n; i++) {
            const float *r = &records[(size_t)i * 13];
            cell[i] = grid_cell_of_point(mk3(r[0], r[1], r[2]), ld3(hdr.bboxMin), P.invCellSize, P.nCells);
            cellStart[cell[i] + 1]++;
        }
        for (int c = 0; c < P.nCells; c++) cellStart[c + 1] += cellStart[c];
        std::vector<int> fill(cellStart.begin(), cellStart.end() - 1);
        for (int i = 0; i < n; i++) {
            const float *r = &records[(size_t)i * 13];
            const int dst = fill[cell[i]]++;
            gx[dst] = r[0]; gy[dst] = r[1]; gz[dst] = r[2];
            g1[dst] = mk4(r[3], r[4], r[5], r[11]);
            g2[dst] = mk4(r[6], r[7], r[8], r[9]);
            g3[dst].x = r[10]; g3[dst].y = r[12];
        }
    }
    GridStore grid;
    memset(&grid, 0, sizeof(grid));
    grid.cellStart = cellStart.data(); grid.gx = gx.data(); grid.gy = gy.data(); grid.gz = gz.data(); grid.g1 = g1.data();
    grid.g2 = g2.data(); grid.g3 = g3.data(); grid.hdr = &hdr;

    /* K3: the camera paths append records and tasks to a host VertexStore */
    const size_t pathSlots = (size_t)L * nLocal, maxVertices = pathSlots + 1, maxVc = pathSlots * (size_t)S + 1;
    std::vector<F4> q(maxVertices * 4, mk4(0, 0, 0, 0)), q4(maxVertices, mk4(0, 0, 0, 0));
    std::vector<F4> diOut(pathSlots, mk4(0, 0, 0, 0)), mergeOut(pathSlots, mk4(0, 0, 0, 0)), vcOut(maxVc, mk4(0, 0, 0, 0));
    I4 noMeta; noMeta.x = -1; noMeta.y = 0; noMeta.z = 0; noMeta.w = 0;
    std::vector<I4> meta(pathSlots, noMeta);
    std::vector<int> diTask(maxVertices, -1), vcTask(maxVc * 2, -1);
    int counts[32];
    memset(counts, 0, sizeof(counts));
    VertexStore vs;
    memset(&vs, 0, sizeof(vs));
    vs.q = q.data(); vs.q4 = q4.data(); vs.qcap = maxVertices; vs.meta = meta.data(); vs.count = counts;
    vs.diTask = diTask.data(); vs.vcTask = vcTask.data(); vs.diOut = diOut.data(); vs.vcOut = vcOut.data(); vs.mergeOut = mergeOut.data();
    std::vector<F4> camOut((size_t)nLocal, mk4(0, 0, 0, 0));
    std::vector<uint32_t> camMask((size_t)nLocal, 0u);
    for (int lp = 0; lp < nLocal; lp++) {
        CameraPath path;
        uint32_t mq[VCM_MERGE_Q + 1];
        MergeScratch ms; ms.q = mq; ms.stride = 1; ms.cap = VCM_MERGE_Q;
        camera_path_begin(e.sc, P, path, lp, lenMask.data());
        int wqState[6] = { 0, 0, 0, 0, 0, 0 };
        CameraWaveQueues wqs; wqs.v.p = wqState; wqs.di.p = wqState + 2; wqs.vc.p = wqState + 4; wqs.pendingVertex = -1; wqs.pendingArrival = 0;
        QueryKey qk = { 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 1u, 1u, 0, 0, 0 };
        with_scene(e.sc, [&](const auto &sc) { while (camera_path_step<1>(sc, P, path, store, grid, e.ls, ms, vs, wqs, qk)) {} });
        camOut[lp] = mk4(path.color.x, path.color.y, path.color.z, u2f((uint32_t)camera_path_target(P, path)));
        camMask[lp] = path.queryMask;
    }
    if ((size_t)counts[0] > maxVertices || (size_t)counts[1] > maxVertices || (size_t)counts[2] > maxVc) return -2;
    /* K3b, K3c, K4: the deferred terms of every camera vertex */
    with_scene(e.sc, [&](const auto &sc) {
        using SC = typename std::decay<decltype(sc)>::type;
        for (int t = 0; t < counts[1]; t++) {
            size_t ps;
            const V3 v = eval_di_task(sc, P, vs, diTask[t], e.ls, ps);
            diOut[ps] = mk4(v.x, v.y, v.z, 0.f);
        }
        for (int t = 0; t < counts[2]; t++) {
            const V3 v = eval_vc_task(sc, P, vs, store, vcTask[2 * t], vcTask[2 * t + 1], e.ls);
            vcOut[t] = mk4(v.x, v.y, v.z, 0.f);
        }
        if (e.useVM)
            for (int vi = 0; vi < counts[0]; vi++) {
                uint32_t mq[VCM_MERGE_Q + 1];
                MergeScratch ms; ms.q = mq; ms.stride = 1; ms.cap = VCM_MERGE_Q;
                size_t ps;
                const V3 v = eval_merge_task<SC::kIntPhong>(sc, P, vs, grid, vi, e.ls, ms, ps);
                mergeOut[ps] = mk4(v.x, v.y, v.z, 0.f);
            }
    });
    /* K5: the framebuffer in path order (per pixel: ascending source path), then the planes pixel by pixel */
    for (int lp = 0; lp < nLocal; lp++) {
        const int t = (int)f2u(camOut[lp].w);
        if (t < 0) continue;
        const V3 col = replay_path_color(P, vs, lp, camMask[lp], mk3(camOut[lp].x, camOut[lp].y, camOut[lp].z));
        float *px = &e.fb[(size_t)t * 3];
        px[0] = px[0] + col.x; px[1] = px[1] + col.y; px[2] = px[2] + col.z;
    }
    for (int p = 0; p < N; p++) parts_resolve_pixel(P, camOut.data(), camMask.data(), vs, p, e.parts.data(), (size_t)N * 3);
    e.iterations++;
    return 0;
}

void emul_parts_get_framebuffer(void *h, float *out) { PartsEmul &e = *(PartsEmul *)h; memcpy(out, e.fb.data(), e.fb.size() * 4); }
/* all VCM_PART_COUNT planes, [part][pixel][3] */
void emul_parts_get_planes(void *h, float *out) { PartsEmul &e = *(PartsEmul *)h; memcpy(out, e.parts.data(), e.parts.size() * 4); }
/* out3: splats of the last iteration, its longest per-pixel list, the most splats of any iteration so far */
void emul_parts_get_splat_info(void *h, long long *out3)
{
    PartsEmul &e = *(PartsEmul *)h;
    out3[0] = e.lastSplats; out3[1] = e.lastMaxPerPixel; out3[2] = e.maxSplats;
}
/* vcm_get_parts_stats on the kernels' grid: k_parts_stats's lanes and tree, then k_parts_stats2's */
int emul_parts_stats(void *h, int maxBlocks, vcm_parts_stats *out)
{
    PartsEmul &e = *(PartsEmul *)h;
    if (e.iterations < 1) return -1;
    const int blocks = parts_grid_blocks(e.N, maxBlocks > 0 ? maxBlocks : VCM_PARTS_DEFAULT_MAX_BLOCKS);
    std::vector<PartsAcc> partials((size_t)blocks), v(VCM_PARTS_BLOCK);
    for (int b = 0; b < blocks; b++) {
        for (int lane = 0; lane < VCM_PARTS_BLOCK; lane++) v[lane] = parts_lane_sum(e.N, blocks, b, lane, e.parts.data(), (size_t)e.N * 3);
        for (int s = 0; s < VCM_PARTS_TREE_STEPS; s++)
            for (int lane = 0; lane < VCM_PARTS_BLOCK; lane++) parts_tree_step(v.data(), s, lane);
        partials[b] = v[0];
    }
    for (int lane = 0; lane < VCM_PARTS_BLOCK; lane++) v[lane] = parts_lane_sum_partials(partials.data(), blocks, lane);
    for (int s = 0; s < VCM_PARTS_TREE_STEPS; s++)
        for (int lane = 0; lane < VCM_PARTS_BLOCK; lane++) parts_tree_step(v.data(), s, lane);
    parts_finish_stats(v[0], e.iterations, e.N, out);
    return 0;
}

} // extern "C"
