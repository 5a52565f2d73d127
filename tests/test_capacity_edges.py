"""The checkers of tests/test_gpu_capacity_edges.py and tests/test_gpu_widened_at_size.py, checked without a GPU: on every
capacity_scene case the oracle (a list walk: no LDS, no BVH) equals the product's device functions compiled for the host
(and the unmodified reference where oracle/_ref is built); the scenes have the table sizes, the used rows and the
visible last light the device tests rely on; the deep scene really overflows the traversal stack; and the host
emulation the at-size tests compare with is itself exercised on each of their scenes."""
import ctypes as C

import numpy as np
import pytest

import capacity_lib as cl
import oracle_lib
import pick_lib as pl
from emul_lib import Emul, emul
from mesh_scenes import capacity_scene, deep_bvh_scene
from oracle_lib import Oracle
from smallvcm_amd._abi import SceneDesc2

needs_ref = pytest.mark.skipif(not oracle_lib.have_ref(), reason="oracle/_ref not built")
_fp = C.POINTER(C.c_float)
THREADS = cl.THREADS


def _oracle_equals_emulation(sc, algo, nit=2, with_ref=True):
    o, e = Oracle(sc, algo, threads=THREADS), Emul(sc, algo)
    lcs, ccs = [], []
    for it in range(nit):
        o.run_iteration(it, 0, 10)
        e.run_iteration(it, 0, 10)
        a, b = o.counts()
        lcs.append(a)
        ccs.append(b)
        for x, y in zip((a, b), e.counts()):
            assert np.array_equal(x, y), it
        so, se = o.stats(), e.stats()
        for k in cl.COUNTERS:
            assert so[k] == se[k], (it, k, so[k], se[k])
    fb = o.framebuffer()
    cl.check_checker(fb, o.stats(), algo)
    assert np.array_equal(fb.view(np.uint32), e.framebuffer().view(np.uint32))
    if with_ref and oracle_lib.have_ref():
        assert oracle_lib.ref_check_scene2(sc) == 0
        ref, consumed, bad = oracle_lib.ref_run_tape2(sc, algo, np.concatenate(lcs), np.concatenate(ccs), n_iter=nit)
        assert bad == 0
        assert np.array_equal(ref.view(np.uint32), fb.view(np.uint32))


def _used_rows(sc):
    return sorted({sc.prims[i].matID for i in range(sc.nPrims)})


# ---- the scenes are what the device tests need them to be ----
@pytest.mark.parametrize("n_mat,n_prims,n_area,n_point", [(31, 30, 2, 0), (32, 60, 2, 0), (33, 30, 2, 0), (64, 30, 2, 0), (12, 31, 2, 0),
                                                          (12, 33, 2, 0), (12, 24, 5, 0), (64, 74, 60, 196), (5, 14, 0, 1)])
def test_capacity_scene_has_the_three_counts_and_uses_the_first_and_the_last_row(n_mat, n_prims, n_area, n_point):
    sc = capacity_scene(n_mat, n_prims, n_area, "frac", 16, 16, n_point_lights=n_point)
    assert (sc.nMaterials, sc.nPrims, sc.nLights) == (n_mat, n_prims, n_area + n_point)
    used = _used_rows(sc)
    assert used[0] == 0 and used[-1] == n_mat - 1
    if n_mat > n_prims:
        assert len(used) < n_mat            # unused rows: they count towards nMaterials all the same
    m2l = [sc.mat2light[i] for i in range(n_mat)]
    if n_area:
        assert m2l[-1] == sc.nLights - 1 and sorted(x for x in m2l if x >= 0) == list(range(n_point, sc.nLights))
    frac = [sc.materials[i].phongExp for i in range(n_mat) if any(sc.materials[i].phong) and sc.materials[i].phongExp != int(sc.materials[i].phongExp)]
    assert frac
    ints = capacity_scene(n_mat, n_prims, n_area, "int", 16, 16, n_point_lights=n_point)
    assert all(ints.materials[i].phongExp == int(ints.materials[i].phongExp) and 1 <= ints.materials[i].phongExp <= 65536 for i in range(n_mat))
    if oracle_lib.have_ref():
        assert oracle_lib.ref_check_scene2(sc) == 0


@pytest.mark.parametrize("n", cl.LIGHT_COUNTS)
def test_camera_paths_hit_the_last_area_light(n):
    """frames of path length 1 with every other light dark, the scene and the size the device tests render: camera rays
    hit the light the last material names"""
    assert cl.last_light_pixels("light", n) >= cl.MIN_LAST_LIGHT_PIXELS
    assert cl.camera_hits_light(lambda only_light: cl.light_scene(n, only_light=only_light), n - 1, algo=cl.VCM) > 0


@pytest.mark.parametrize("n", cl.PICK_COUNTS)
def test_camera_paths_hit_the_last_light_of_the_pick_scenes(n):
    """pick_scene(n) exactly as tests/test_gpu_capacity_edges.py renders it"""
    assert cl.last_light_pixels("pick", n) >= cl.MIN_LAST_LIGHT_PIXELS


# ---- oracle = host emulation (= reference) on every capacity case ----
@pytest.mark.parametrize("n_mat,n_prims,kind,algo", cl.MATERIAL_CASES)
def test_material_cases_oracle_equals_the_device_functions(n_mat, n_prims, kind, algo):
    _oracle_equals_emulation(cl.material_scene(n_mat, n_prims, kind, 48), algo)


@pytest.mark.parametrize("n_prims,force_bvh,algo", cl.PRIM_CASES)
def test_primitive_cases_oracle_equals_the_device_functions(monkeypatch, n_prims, force_bvh, algo):
    if force_bvh:
        monkeypatch.setenv("SMALLVCM_AMD_FORCE_BVH", "1")
    _oracle_equals_emulation(cl.prim_scene(n_prims, 48), algo)


@pytest.mark.parametrize("algo", range(7))
@pytest.mark.parametrize("n", cl.LIGHT_COUNTS)
def test_light_cases_oracle_equals_the_device_functions(n, algo):
    _oracle_equals_emulation(cl.light_scene(n, 48), algo)


@pytest.mark.parametrize("n", cl.LIGHT_COUNTS)
@pytest.mark.parametrize("mode", ["power", "custom"])
def test_light_cases_with_a_pick_table_exercise_the_emulation(n, mode):
    m, mix, w = cl.small_light_settings(n)[mode]
    d = pl.with_pick(cl.light_scene(n, 48), m, mix, w)
    for algo in range(7):
        e = pl.Emul5(d, algo, seed=77)
        e.run_iteration(0, 0, 10)
        cl.check_checker(e.framebuffer(), e.stats(), algo)


@pytest.mark.parametrize("n", cl.PICK_COUNTS)
@pytest.mark.parametrize("mode", ["power", "custom"])
def test_pick_table_cases_exercise_the_emulation_and_every_live_light(n, mode):
    m, mix, w = cl.pick_settings(n)[mode]
    d = pl.with_pick(cl.pick_scene(n), m, mix, w)
    _, _, quanta, pmf, cdf = pl.tables(d)
    assert len(pmf) == n and len(cdf) == n + 1 and cdf[-1] == 1.0 and quanta[-1] > 0
    if mode == "custom":
        live = w[quanta > 0]
        assert live.max() / w.min() > 1e8          # nine decades asked for, the table keeps what 2^-23 can hold
    for algo in (cl.VCM, cl.BPT, cl.PATH_TRACE):
        e = pl.Emul5(d, algo, seed=77)
        e.run_iteration(0, 0, 10)
        cl.check_checker(e.framebuffer(), e.stats(), algo)


# ---- the deep BVH ----
def _emul_kat2(sc, op, rays):
    E = emul()
    E.emul_kat2.argtypes = [C.POINTER(SceneDesc2), C.c_int, C.c_int, _fp, _fp]
    out = np.zeros_like(rays)
    E.emul_kat2(C.byref(sc), op, len(rays), rays.ctypes.data_as(_fp), out.ctypes.data_as(_fp))
    return out


@pytest.mark.parametrize("op", [0, 1])
def test_the_deep_scene_overflows_the_traversal_stack(op):
    """PRECONDITION of the device tests: a re-walk of the node arrays with an unbounded stack (tests/host_emul_bvh) counts
    more than VCM_BVH_STACK pending subtrees for at least 1 000 of the KAT rays and for camera rays of the render; and
    the product's traversal on the host -- 32 levels, then the threaded walk -- returns what the unbounded walk returns"""
    sc = deep_bvh_scene(96, 96)
    rays = cl.deep_kat_rays(sc)
    if op == 1:
        rays[:, 6] = 6.0
    pend, walk, info = cl.bvh_pending(sc, op, rays)
    assert info["stack"] == 32 and info["depth"] > 34, info
    assert np.count_nonzero(pend > info["stack"]) >= 1000, (int(pend.max()), int(np.count_nonzero(pend > 32)))
    mine = _emul_kat2(sc, op, rays)
    assert np.array_equal(mine.view(np.uint32), walk.view(np.uint32))
    assert 0 < np.count_nonzero(mine[:, 0]) and (op == 0 or np.count_nonzero(mine[:, 0]) < len(rays))
    n_cam = sc.camera.resolution[0] * sc.camera.resolution[1]     # the render's primary rays close the set
    assert np.count_nonzero(pend[-int(n_cam):] > info["stack"]) > 0, int(pend[-int(n_cam):].max())


@needs_ref
@pytest.mark.parametrize("op", [0, 1])
def test_the_deep_traversal_on_the_host_equals_the_reference_walk(op):
    sc = deep_bvh_scene(96, 96)
    rays = cl.deep_kat_rays(sc)
    if op == 1:
        rays[:, 6] = 6.0
    R = oracle_lib.ref_tape()
    R.ref_kat2.argtypes = [C.POINTER(SceneDesc2), C.c_int, C.c_int, _fp, _fp]
    want = np.zeros_like(rays)
    assert R.ref_kat2(C.byref(sc), op, len(rays), rays.ctypes.data_as(_fp), want.ctypes.data_as(_fp)) == 0
    assert np.array_equal(want.view(np.uint32), _emul_kat2(sc, op, rays).view(np.uint32))


@pytest.mark.parametrize("algo", [cl.VCM, cl.PATH_TRACE])
def test_the_deep_scene_oracle_equals_the_device_functions(algo):
    _oracle_equals_emulation(deep_bvh_scene(48, 48), algo)


# ---- B: the emulation is exercised on every scene of the at-size tests ----
@pytest.mark.parametrize("kind", cl.KINDS)
def test_the_emulation_is_exercised_on_the_widened_scenes(monkeypatch, kind):
    """at 64 x 40 (the device tests assert the same on the emulation's numbers at their own sizes): every algorithm of
    every kind merges, connects and splats where it should; and the features are on"""
    for k, v in cl.KIND_ENV.get(kind, {}).items():
        monkeypatch.setenv(k, v)
    d = cl.widened_scene(kind, (64, 40))
    assert pl.n_lights(d) > 4 and d.pick and d.base.lens
    assert bool(d.base.base.envmap) == bool(cl.KIND_FLAGS[kind][4])
    for algo in range(7):
        e = pl.Emul5(d, algo, seed=77)
        e.run_iteration(0, 0, 10)
        cl.check_checker(e.framebuffer(), e.stats(), algo)


@pytest.mark.parametrize("kind,features", cl.FEATURES_ALONE)
def test_the_emulation_is_exercised_with_each_feature_alone(kind, features):
    d = cl.widened_scene(kind, (64, 40), **features)
    assert (bool(d.base.base.envmap), bool(d.base.lens), bool(d.pick)) == (features["env"], features["lens"], features["pick"])
    e = pl.Emul5(d, cl.VCM, seed=77)
    e.run_iteration(0, 0, 10)
    cl.check_checker(e.framebuffer(), e.stats(), cl.VCM)
