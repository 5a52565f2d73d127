// TEST INFRASTRUCTURE.  A re-walk of the BVH the scene host builds (scene_host.h), in the order of vcm_core.h's
// bvh_intersect / bvh_occluded but with a stack that cannot fill up: per ray, the largest number of subtrees that were
// pending at once.  A ray whose count exceeds VCM_BVH_STACK is one for which the product's traversal sets `overflow`
// and finishes with the threaded walk -- tests/test_capacity_edges.py asserts that the deep scene has such rays before
// the GPU tests rely on it.  The answers of the walk are returned too (same layout as VCM_KAT_INTERSECT /
// VCM_KAT_OCCLUDED), so that the test can hold this walk against the product's own.
#include <string>
#include <vector>
#include <string.h>
#include "../../smallvcm_amd/csrc/vcm_core.h"
#include "../../smallvcm_amd/csrc/scene_host.h"
#include "../../include/smallvcm_amd_debug.h"

using namespace vcm;

static int walk_intersect(const DScene &sc, const Ray &ray, Isect &res, bool &hit)
{
    const V3 invDir = mk3(1.f / ray.dir.x, 1.f / ray.dir.y, 1.f / ray.dir.z);
    const Isect start = res;
    bool any = false, ambiguous = false, bestIsSphere = false;
    std::vector<int> stack;
    size_t most = 0;
    int ref = VCM_BVH_NONE;
    auto pop = [&]() {
        ref = VCM_BVH_NONE;
        while (ref == VCM_BVH_NONE && !stack.empty()) {
            const BvhNode nd = sc.nodes()[stack.back()];
            stack.pop_back();
            float t;
            if (bvh_box_near(nd, ray.org, invDir, res.dist, t)) ref = nd.leaf;
        }
    };
    if (sc.nNodes > 0) {
        const BvhNode root = sc.nodes()[0];
        float t;
        if (bvh_box_near(root, ray.org, invDir, res.dist, t)) ref = root.leaf;
    }
    for (;;) {
        while (ref < 0) {
            const BvhWide w = sc.wide()[-1 - ref];
            float tl, tr;
            const bool hl = bvh_box_near6(w.lmin, w.lmax, ray.org, invDir, res.dist, tl);
            const bool hr = bvh_box_near6(w.rmin, w.rmax, ray.org, invDir, res.dist, tr);
            if (hl && hr) {
                const bool leftFirst = tl <= tr;
                stack.push_back(leftFirst ? w.rnode : w.lnode);
                most = std::max(most, stack.size());
                ref = leftFirst ? w.lref : w.rref;
            } else if (hl) ref = w.lref;
            else if (hr) ref = w.rref;
            else pop();
        }
        if (ref == VCM_BVH_NONE) break;
        bvh_leaf(sc, ref, ray, res, any, ambiguous, bestIsSphere);
        pop();
        if (ref == VCM_BVH_NONE) break;
    }
    if (ambiguous) { res = start; hit = list_intersect(sc, ray, res); return (int)most; }
    if (any) res.lightID = sc.mat2light()[res.matID];
    hit = any;
    return (int)most;
}

static int walk_occluded(const DScene &sc, const Ray &ray, float tmaxp, bool &occluded)
{
    const V3 invDir = mk3(1.f / ray.dir.x, 1.f / ray.dir.y, 1.f / ray.dir.z);
    std::vector<int> stack;
    size_t most = 0;
    int ref = VCM_BVH_NONE;
    occluded = false;
    if (sc.nNodes > 0) {
        const BvhNode root = sc.nodes()[0];
        if (bvh_box_hit(root, ray.org, invDir, tmaxp)) ref = root.leaf;
    }
    for (;;) {
        while (ref < 0) {
            const BvhWide w = sc.wide()[-1 - ref];
            float tl, tr;
            const bool hl = bvh_box_near6(w.lmin, w.lmax, ray.org, invDir, tmaxp, tl);
            const bool hr = bvh_box_near6(w.rmin, w.rmax, ray.org, invDir, tmaxp, tr);
            if (hl && hr) {
                const bool leftFirst = tl <= tr;
                stack.push_back(leftFirst ? w.rref : w.lref);
                most = std::max(most, stack.size());
                ref = leftFirst ? w.lref : w.rref;
            } else if (hl) ref = w.lref;
            else if (hr) ref = w.rref;
            else if (!stack.empty()) { ref = stack.back(); stack.pop_back(); }
            else ref = VCM_BVH_NONE;
        }
        if (ref == VCM_BVH_NONE) break;
        if (bvh_leaf_occluded(sc, ref, ray, tmaxp)) { occluded = true; break; }
        if (!stack.empty()) { ref = stack.back(); stack.pop_back(); }
        else break;
    }
    return (int)most;
}

extern "C" {

/* op VCM_KAT_INTERSECT / VCM_KAT_OCCLUDED over n records of VCM_KAT_FLOATS floats: pending[i] = the most subtrees pending
   at once for ray i, out = the walk's answers; info = { nodes, depth of the tree, VCM_BVH_STACK }.  -1: no BVH */
int bvh_pending(const vcm_scene_desc2 *scene, int op, int n, const float *in, int *pending, float *out, int *info)
{
    SceneHost h;
    std::string err;
    if (!scene_host_from_desc2(*scene, h, err)) return -2;
    scene_host_build_accel(h, scene_host_force_bvh());
    if (h.nodes.empty()) return -1;
    DScene sc;
    h.view(sc);
    int depth = 0;
    {   /* nodes are in depth-first order: a node's subtree ends at its escape index */
        std::vector<int> ends;
        for (int i = 0; i < (int)h.nodes.size(); i++) {
            while (!ends.empty() && ends.back() <= i) ends.pop_back();
            ends.push_back(h.nodes[(size_t)i].escape);
            depth = std::max(depth, (int)ends.size());
        }
    }
    info[0] = (int)h.nodes.size(); info[1] = depth; info[2] = VCM_BVH_STACK;
    for (int i = 0; i < n; i++) {
        const float *r = in + (size_t)i * VCM_KAT_FLOATS;
        float *o = out + (size_t)i * VCM_KAT_FLOATS;
        memset(o, 0, VCM_KAT_FLOATS * sizeof(float));
        if (op == VCM_KAT_INTERSECT) {
            Ray ray; ray.org = ld3(r); ray.dir = ld3(r + 3); ray.tmin = r[6];
            Isect is; is.dist = 1e36f; is.matID = 0; is.lightID = -1; is.normal = sp3(0.f);
            bool hit;
            pending[i] = walk_intersect(sc, ray, is, hit);
            if (hit) { o[0] = 1.f; o[1] = is.dist; o[2] = (float)is.matID; o[3] = (float)is.lightID; o[4] = is.normal.x; o[5] = is.normal.y; o[6] = is.normal.z; }
        } else {   /* scene_occluded's ray */
            const V3 dir = ld3(r + 3);
            Ray ray; ray.org = ld3(r) + dir * VCM_EPS_RAY; ray.dir = dir; ray.tmin = 0;
            bool occ;
            pending[i] = walk_occluded(sc, ray, r[6] - 2 * VCM_EPS_RAY, occ);
            o[0] = occ ? 1.f : 0.f;
        }
    }
    return 0;
}

} // extern "C"
