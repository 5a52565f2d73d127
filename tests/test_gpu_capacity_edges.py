"""The scene tables' capacity branches ON THE DEVICE (vcm_core.h stage_scene_tables / scene_material / scene_prim /
scene_mat2light / scene_light / stage_pick_tables / pick_light / light_pick_prob, vcm_api.hip's fall-back from
k_merge_pairs to k_merge_walk, the traversal stack of bvh_intersect / bvh_occluded): every count at its room, one below
and one above.  These are `#if defined(__HIP_DEVICE_COMPILE__)` branches and launch-time choices, so the host emulation
never takes them; the checker is the oracle (a list walk without LDS or BVH; tests/test_capacity_edges.py holds it
against the unmodified reference), and the host emulation for what the reference cannot express (light selection).
Framebuffer bits, both random-number tapes and the nine workload counters; which path a context took is asserted
through vcm_debug_context_info, not inferred."""
import ctypes as C

import numpy as np
import pytest

import capacity_lib as cl
import oracle_lib
import pick_lib as pl
from mesh_scenes import deep_bvh_scene
from oracle_lib import Oracle
from smallvcm_amd._abi import SceneDesc2
from smallvcm_amd.renderer import HipBackend, VertexCM

pytestmark = pytest.mark.gpu
_fp = C.POINTER(C.c_float)
LDS_MATERIALS = PAIR_MATERIALS = LDS_PRIMS = 32
LDS_LIGHTS, LDS_PICK = 4, 256


def _device_equals_oracle(sc, algo, merge_kernel=None, nit=2, expect=None):
    """-> vcm_debug_context_info after the last iteration"""
    o = Oracle(sc, algo, threads=cl.THREADS)
    r = VertexCM(sc, algo, 0.003, 0.75, 1234)
    r.mMinPathLength, r.mMaxPathLength = 0, 10
    if merge_kernel is not None:
        assert r.backend.L.vcm_set_merge_kernel(r.backend.ctx, merge_kernel) == 0
    total = dict.fromkeys(cl.COUNTERS, 0)
    for it in range(nit):
        o.run_iteration(it, 0, 10)
        r.RunIteration(it)
        lc, cc = r.backend.rng_counts()
        olc, occ = o.counts()
        assert np.array_equal(lc, olc), ("light tape", it)
        assert np.array_equal(cc, occ), ("camera tape", it)
        so, sg = o.stats(), r.stats()
        for k in cl.COUNTERS:
            assert so[k] == sg[k], (it, k, so[k], sg[k])
            total[k] += so[k]
    info = cl.context_info(r.backend)
    fb, want = r.framebuffer_sum(), o.framebuffer()
    r.close()
    cl.check_checker(want, total, algo)
    assert np.array_equal(fb.view(np.uint32), want.view(np.uint32)), float(np.abs(fb - want).max())
    for k, v in (expect or {}).items():
        assert info[k] == v, (k, info)
    return info


def _device_equals_emulation(d, algo, strict, seed=77, nit=2):
    emu = pl.Emul5(d, algo, seed=seed)
    r = VertexCM(d, algo, 0.003, 0.75, seed, strict_order=strict)
    r.mMinPathLength, r.mMaxPathLength = 0, 10
    total = dict.fromkeys(cl.COUNTERS, 0)
    for it in range(nit):
        emu.run_iteration(it, 0, 10)
        r.RunIteration(it)
        lc, cc = r.backend.rng_counts()
        elc, ecc = emu.counts()
        assert np.array_equal(lc, elc), ("light tape", it)
        assert np.array_equal(cc, ecc), ("camera tape", it)
        se, sg = emu.stats(), r.stats()
        for k in cl.COUNTERS:
            assert se[k] == sg[k], (it, k, se[k], sg[k])
            total[k] += se[k]
    info = cl.context_info(r.backend)
    gpu, host = r.framebuffer_sum(), emu.framebuffer()
    r.close()
    cl.check_checker(host, total, algo)
    if strict and algo in cl.SPLATTING:   # strict mode splats with fp32 atomics: their order is not defined
        assert np.all(np.abs(gpu - host) <= 2e-5 * np.abs(host) + 2e-7), float(np.abs(gpu - host).max())
    else:
        assert np.array_equal(gpu.view(np.uint32), host.view(np.uint32))
    return info


# ---- 1. materials: VCM_LDS_MATERIALS and VCM_PAIR_MATERIALS ----
@pytest.mark.parametrize("n_mat,n_prims,kind,algo", cl.MATERIAL_CASES)
def test_material_table_at_its_room_and_beyond(n_mat, n_prims, kind, algo):
    """31, 32: the LDS copy (exactly full at 32) and k_merge_pairs; 33, 64: materials and mat2light from global memory
    and the automatic fall-back to k_merge_walk -- as a list and behind a BVH, integer and fractional exponents"""
    sc = cl.material_scene(n_mat, n_prims, kind)
    merged = algo in cl.MERGING
    want = cl.MERGE_PAIRS if n_mat <= PAIR_MATERIALS else cl.MERGE_WALK
    _device_equals_oracle(sc, algo, expect={"nMaterials": n_mat, "nPrims": n_prims, "nLights": 2, "nodes": int(n_prims > LDS_PRIMS),
                                            "intPhong": int(kind == "int"), "envMap": 0, "lens": 0, "pick": 0,
                                            "mergeKernel": want if merged else 0})


@pytest.mark.parametrize("algo", cl.WALK_ALGOS)
@pytest.mark.parametrize("kind", ["int", "frac"])
@pytest.mark.parametrize("n_mat", [32, 33])
def test_material_table_with_the_walk_kernel_chosen(n_mat, kind, algo):
    """k_merge_walk by vcm_set_merge_kernel: scene_material(..., lds = false) at the room's edge and beyond"""
    _device_equals_oracle(cl.material_scene(n_mat, 30, kind), algo, merge_kernel=cl.MERGE_WALK,
                          expect={"nMaterials": n_mat, "mergeKernel": cl.MERGE_WALK})


# ---- 2. primitives: VCM_LDS_PRIMS, the list / BVH switch ----
@pytest.mark.parametrize("n_prims,force_bvh,algo", cl.PRIM_CASES)
def test_primitive_table_at_its_room_and_beyond(monkeypatch, n_prims, force_bvh, algo):
    if force_bvh:
        monkeypatch.setenv("SMALLVCM_AMD_FORCE_BVH", "1")   # read when the scene is built
    bvh = force_bvh or n_prims > LDS_PRIMS
    _device_equals_oracle(cl.prim_scene(n_prims), algo, expect={"nPrims": n_prims, "nodes": int(bvh), "rects": 0, "nMaterials": 12})


# ---- 3. lights: VCM_LDS_LIGHTS ----
@pytest.mark.parametrize("algo", range(7))
@pytest.mark.parametrize("n", cl.LIGHT_COUNTS)
def test_light_table_at_its_room_and_beyond_uniform_pick(n, algo):
    """area lights, hit by camera paths through mat2light (the last material names the last light: asserted on the oracle's
    frames of path length 1 with every other light dark)"""
    assert cl.last_light_pixels("light", n) >= cl.MIN_LAST_LIGHT_PIXELS
    _device_equals_oracle(cl.light_scene(n), algo, expect={"nLights": n, "pick": 0, "nodes": 0})


@pytest.mark.parametrize("algo", range(7))
@pytest.mark.parametrize("mode", ["power", "custom"])
@pytest.mark.parametrize("n", cl.LIGHT_COUNTS)
def test_light_table_at_its_room_and_beyond_with_a_pick_table(n, mode, algo):
    """the same counts and the same frame with POWER and CUSTOM selection, all seven algorithms"""
    assert cl.last_light_pixels("light", n) >= cl.MIN_LAST_LIGHT_PIXELS
    m, mix, w = cl.small_light_settings(n)[mode]
    info = _device_equals_emulation(pl.with_pick(cl.light_scene(n), m, mix, w), algo, False)
    assert info["nLights"] == n and info["pick"] == 1


# ---- 4. the pick table: VCM_LDS_PICK ----
@pytest.mark.parametrize("strict", [False, True])
@pytest.mark.parametrize("algo", [cl.VCM, cl.BPT, cl.PATH_TRACE])
@pytest.mark.parametrize("mode", ["power", "custom"])
@pytest.mark.parametrize("n", cl.PICK_COUNTS)
def test_pick_table_at_its_room_and_beyond(n, mode, algo, strict):
    """255, 256: cdf (n + 1 entries) and pmf in LDS, exactly full at 256; 257: the guided search in global memory.  Camera
    rays of THIS frame hit the last light (asserted on the oracle's frame of path length 1 with every other light dark), so
    mat2light -> light n - 1 -> light_pick_prob runs in the render"""
    assert cl.last_light_pixels("pick", n) >= cl.MIN_LAST_LIGHT_PIXELS
    m, mix, w = cl.pick_settings(n)[mode]
    info = _device_equals_emulation(pl.with_pick(cl.pick_scene(n), m, mix, w), algo, strict)
    assert info["nLights"] == n and info["pick"] == 1 and info["nMaterials"] == 64


@pytest.mark.parametrize("mode", ["power", "custom"])
@pytest.mark.parametrize("n", cl.PICK_COUNTS)
def test_device_pick_at_every_interval_boundary(n, mode):
    """VCM_KAT_LIGHT_PICK at the first and the last float of every light's interval, the generator's extremes (the float
    just below 1 must give the last live light) and random floats"""
    m, mix, w = cl.pick_settings(n)[mode]
    d = pl.with_pick(cl.pick_scene(n), m, mix, w)
    rng = np.random.default_rng(n)
    _, _, quanta, pmf, cdf = pl.tables(d)
    live = np.nonzero(quanta > 0)[0]
    assert live[-1] == n - 1, "the last light must be live"
    first = (cdf[live].astype(np.float64) + 2.0 ** -24).astype(np.float32)
    last = (cdf[live + 1].astype(np.float64) - 2.0 ** -24).astype(np.float32)
    assert last[-1] == np.float32(1.0 - 2.0 ** -24)
    j = rng.integers(0, pl.Q, 20000)
    rnd = ((2 * j + 1) * 2.0 ** -24).astype(np.float32)
    r = np.concatenate([first, last, np.float32([2.0 ** -24, 1.0 - 2.0 ** -24]), rnd])
    light = np.concatenate([live, live, [live[0], n - 1], rng.integers(0, n, len(rnd))])
    inp = pl.pick_records(r, light)
    b = HipBackend(d, 4, 0.003, 0.75, 1234)
    b.L.vcm_debug_kat.argtypes = [C.c_void_p, C.c_int, C.c_int, _fp, _fp]
    dev = np.zeros_like(inp)
    assert b.L.vcm_debug_kat(b.ctx, pl.OP_LIGHT_PICK, len(inp), inp.ctypes.data_as(_fp), dev.ctypes.data_as(_fp)) == 0, \
        b.L.vcm_last_error()
    info = cl.context_info(b)
    b.close()
    assert info["nLights"] == n and info["pick"] == 1
    k = len(live)
    assert np.array_equal(dev[:k, 0], live.astype(np.float32)) and np.array_equal(dev[k:2 * k, 0], live.astype(np.float32))
    assert np.array_equal(dev[:k, 1], pmf[live]) and np.array_equal(dev[:2 * k + 2, 2], pmf[light[:2 * k + 2]])
    assert (dev[2 * k, 0], dev[2 * k + 1, 0]) == (live[0], n - 1)
    host = pl.kat5(d, pl.OP_LIGHT_PICK, inp)
    assert np.array_equal(dev.view(np.uint32), host.view(np.uint32))


# ---- 5. the traversal stack: VCM_BVH_STACK ----
@pytest.mark.parametrize("op", [0, 1])
def test_deep_bvh_traversal_on_the_device(op):
    """rays of which thousands hold more than 32 subtrees pending (counted here, on these very rays, by the unbounded
    re-walk; tests/test_capacity_edges.py asserts the same without a GPU): the `overflow` branch and the threaded re-walk,
    against the reference's list walk (the host build where oracle/_ref is not there), bit for bit"""
    sc = deep_bvh_scene(96, 96)
    rays = cl.deep_kat_rays(sc)
    if op == 1:
        rays[:, 6] = 6.0
    pend, _, tree = cl.bvh_pending(sc, op, rays)
    assert tree["stack"] == 32 and np.count_nonzero(pend > tree["stack"]) >= 1000
    b = HipBackend(sc, 4, 0.003, 0.75, 1234)
    b.L.vcm_debug_kat.argtypes = [C.c_void_p, C.c_int, C.c_int, _fp, _fp]
    dev = np.zeros_like(rays)
    assert b.L.vcm_debug_kat(b.ctx, op, len(rays), rays.ctypes.data_as(_fp), dev.ctypes.data_as(_fp)) == 0, b.L.vcm_last_error()
    info = cl.context_info(b)
    b.close()
    assert info["nodes"] == 1 and info["nPrims"] == sc.nPrims
    want = np.zeros_like(rays)
    if oracle_lib.have_ref():
        R = oracle_lib.ref_tape()
        R.ref_kat2.argtypes = [C.POINTER(SceneDesc2), C.c_int, C.c_int, _fp, _fp]
        assert R.ref_kat2(C.byref(sc), op, len(rays), rays.ctypes.data_as(_fp), want.ctypes.data_as(_fp)) == 0
    else:
        from emul_lib import emul
        E = emul()
        E.emul_kat2.argtypes = [C.POINTER(SceneDesc2), C.c_int, C.c_int, _fp, _fp]
        E.emul_kat2(C.byref(sc), op, len(rays), rays.ctypes.data_as(_fp), want.ctypes.data_as(_fp))
    assert 0 < np.count_nonzero(want[:, 0]) < len(rays)
    bad = np.nonzero((want.view(np.uint32) != dev.view(np.uint32)).any(axis=1))[0]
    assert len(bad) == 0, "%d of %d rays differ, first %s" % (len(bad), len(rays), bad[:5])


@pytest.mark.parametrize("algo", [cl.VCM, cl.PATH_TRACE])
def test_deep_bvh_render_equals_the_oracle(algo):
    _device_equals_oracle(deep_bvh_scene(96, 96), algo, expect={"nodes": 1, "intPhong": 1})
