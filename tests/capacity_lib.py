"""Shared by the capacity-edge and at-size tests (test infrastructure): the case tables, the checkers' preconditions,
the binding of vcm_debug_context_info and of tests/host_emul_bvh/libbvh_depth.so."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

import envmap_lib as el
import lens_lib as ll
import pick_lib as pl
from mesh_scenes import bumpy_room, capacity_scene, tilted_room
from smallvcm_amd._abi import SceneDesc2, SceneDesc3

HERE = os.path.dirname(os.path.abspath(__file__))
COUNTERS = ("lightVertices", "lightRays", "cameraRays", "shadowRays", "mergeQueries", "mergeCandidates", "mergeAccepted",
            "connections", "lightSplats")
LIGHT_TRACE, PPM, BPM, BPT, VCM, PATH_TRACE, EYE_LIGHT = range(7)    # include/smallvcm_amd.h vcm_algorithm
MERGING, CONNECTING, SPLATTING = (PPM, BPM, VCM), (BPT, VCM), (LIGHT_TRACE, BPT, VCM)
MERGE_WALK, MERGE_PAIRS = 2, 3                                       # VCM_MERGE_WALK / VCM_MERGE_PAIRS
INFO_KEYS = ("rects", "quads", "nodes", "intPhong", "envMap", "lens", "pick", "nMaterials", "nPrims", "nLights", "mergeKernel")
_fp = C.POINTER(C.c_float)
THREADS = min(16, os.cpu_count() or 1)   # the checkers' thread pool: never sized by a whole shared machine


def context_info(backend):
    """vcm_debug_context_info of a HipBackend as a dict (include/smallvcm_amd_debug.h)"""
    out = (C.c_int * len(INFO_KEYS))()
    backend.L.vcm_debug_context_info.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
    assert backend.L.vcm_debug_context_info(backend.ctx, out) == 0, backend.L.vcm_last_error()
    return dict(zip(INFO_KEYS, list(out)))


def check_checker(fb, stats, algo):
    """the checker itself was exercised: asserted on ITS numbers, never the device's"""
    assert np.isfinite(fb).all() and np.count_nonzero(fb) > 0
    if algo in MERGING:
        assert stats["mergeAccepted"] > 0, stats
    if algo in CONNECTING:
        assert stats["connections"] > 0, stats
    if algo in SPLATTING:
        assert stats["lightSplats"] > 0, stats


# ---- A: the scene tables' capacities -------------------------------------------------------------------------------
RES_A = 96
MATERIAL_CASES = [(m, p, k, a) for m in (31, 32, 33, 64) for p in (30, 60) for k in ("int", "frac") for a in (VCM, BPM, BPT, PATH_TRACE)]
PRIM_CASES = [(p, f, a) for p in (31, 32, 33) for f in (False, True) for a in (VCM, PATH_TRACE)]
LIGHT_COUNTS = (3, 4, 5, 8)
PICK_COUNTS = (255, 256, 257)


def material_scene(n_mat, n_prims, kind, res=RES_A):
    return capacity_scene(n_mat, n_prims, 2, kind, res, res, seed=n_mat)


def prim_scene(n_prims, res=RES_A):
    return capacity_scene(12, n_prims, 2, "int", res, res, seed=n_prims)


def light_scene(n_lights, res=RES_A, only_light=None):
    return capacity_scene(12, 24, n_lights, "int", res, res, seed=n_lights, only_light=only_light)


def pick_scene(n_lights, res=RES_A, only_light=None):
    """point and area lights mixed, the area lights last (so the last light can be hit)"""
    n_area = 60
    return capacity_scene(64, 10 + n_area + 4, n_area, "int", res, res, n_point_lights=n_lights - n_area, seed=n_lights,
                          only_light=only_light)


def pick_settings(n_lights):
    """POWER with a uniform share, and CUSTOM with weights spanning nine decades (the last light's among the largest)"""
    rng = np.random.default_rng(n_lights)
    w = (10.0 ** rng.uniform(0, 9, n_lights)).astype(np.float32)
    w[-1] = np.float32(3e8)
    return {"power": (pl.POWER, 0.1, None), "custom": (pl.CUSTOM, 0.0, w)}


def small_light_settings(n_lights):
    return {"power": (pl.POWER, 0.2, None), "custom": (pl.CUSTOM, 0.0, np.float32([1.0, 5.0, 0.5, 2.0, 8.0, 0.25, 3.0, 1.5][:n_lights]))}


WALK_ALGOS = (PPM, BPM, VCM)   # every algorithm that launches a merge kernel


def camera_hits_light(scene_fn, light, algo=PATH_TRACE):
    """paths of length 1 (camera -> emitter) over the scene in which only `light` emits: what the oracle's frame holds
    is the radiance of camera rays that HIT that light -> the number of such pixels"""
    from oracle_lib import Oracle
    o = Oracle(scene_fn(only_light=light), algo, threads=THREADS)
    o.run_iteration(0, 0, 1)
    return int(np.count_nonzero(o.framebuffer().sum(axis=2)))


MIN_LAST_LIGHT_PIXELS = 8   # "camera paths hit the last light" means more than a pixel or two


@functools.lru_cache(maxsize=None)
def last_light_pixels(which, n):
    """pixels of the frame the DEVICE tests render -- light_scene(n) / pick_scene(n) at their default size -- whose camera
    ray hits the last light, on the oracle; depends on the scene alone, so once per n"""
    fn = {"light": light_scene, "pick": pick_scene}[which]
    return camera_hits_light(lambda only_light: fn(n, only_light=only_light), n - 1)


def deep_kat_rays(scene):
    """THE ray set of the deep-BVH known-answer tests, on the CPU (where it is shown to overflow the stack) and on the
    device alike: 50 000 seeded rays and the render's primary rays"""
    from mesh_scenes import deep_bvh_rays
    return np.ascontiguousarray(np.concatenate([deep_bvh_rays(50000, seed=2), camera_rays(scene)]))


# ---- the deep BVH ---------------------------------------------------------------------------------------------------
_B = None


def bvh_depth_lib():
    global _B
    if _B is None:
        d = os.path.join(HERE, "host_emul_bvh")
        subprocess.run(["make", "-C", d], check=True, stdout=subprocess.DEVNULL)
        B = C.CDLL(os.path.join(d, "libbvh_depth.so"))
        B.bvh_pending.argtypes = [C.POINTER(SceneDesc2), C.c_int, C.c_int, _fp, C.POINTER(C.c_int), _fp, C.POINTER(C.c_int)]
        _B = B
    return _B


def bvh_pending(scene, op, rays):
    """-> (most subtrees pending per ray, the re-walk's answers, {nodes, depth, stack})"""
    rays = np.ascontiguousarray(rays, np.float32)
    pend = np.zeros(len(rays), np.int32)
    out = np.zeros_like(rays)
    info = (C.c_int * 3)()
    rc = bvh_depth_lib().bvh_pending(C.byref(scene), op, len(rays), rays.ctypes.data_as(_fp), pend.ctypes.data_as(C.POINTER(C.c_int)),
                                     out.ctypes.data_as(_fp), info)
    assert rc == 0, rc
    return pend, out, dict(zip(("nodes", "depth", "stack"), list(info)))


def camera_rays(scene):
    """the primary ray of every pixel centre as VCM_KAT_INTERSECT records (VCM_KAT_CAMERA gives the direction)"""
    from emul_lib import emul
    E = emul()
    E.emul_kat2.argtypes = [C.POINTER(SceneDesc2), C.c_int, C.c_int, _fp, _fp]
    rx, ry = int(scene.camera.resolution[0]), int(scene.camera.resolution[1])
    inp = np.zeros((rx * ry, 16), np.float32)
    xs, ys = np.meshgrid(np.arange(rx) + 0.5, np.arange(ry) + 0.5)
    inp[:, 0], inp[:, 1] = xs.ravel(), ys.ravel()
    out = np.zeros_like(inp)
    E.emul_kat2(C.byref(scene), 7, len(inp), inp.ctypes.data_as(_fp), out.ctypes.data_as(_fp))
    rays = np.zeros_like(inp)
    rays[:, 0:3] = np.float32(list(scene.camera.position))
    rays[:, 3:6] = out[:, 0:3]
    return rays


# ---- B: the widened kernels at size ---------------------------------------------------------------------------------
SHAPES = ((161, 97), (256, 256), (3, 2200))
KINDS = ("rects", "quads", "list", "bvh", "bvhG", "listE", "bvhE")
KIND_FLAGS = {   # what vcm_debug_context_info must report: (rects, quads, nodes, intPhong, envMap)
    "rects": (1, 0, 0, 1, 1), "quads": (0, 1, 0, 1, 0), "list": (0, 0, 0, 1, 0), "bvh": (0, 0, 1, 1, 0),
    "bvhG": (0, 0, 1, 0, 0), "listE": (0, 0, 0, 0, 1), "bvhE": (0, 0, 1, 0, 1)}
KIND_ENV = {"quads": {"SMALLVCM_AMD_NO_RECTS": "1"}}   # scene 3's box without its rectangles: the SceneQuads kernels
EXTRA_LIGHTS = [((0.3, 0.2, 0.5), (1.0, 0.8, 0.6)), ((-0.4, 0.1, 0.2), (0.1, 0.2, 0.3)), ((0.5, -0.6, -0.4), (0.02, 0.03, 0.02)),
                ((-0.7, -0.5, 0.7), (3.0, 2.5, 2.0)), ((0.1, 0.6, -0.8), (0.3, 0.1, 0.4))]


def _sky():
    return el.sky(50, 23, sun=(0.55, 0.2), sun_size=2, sun_value=(30.0, 27.0, 22.0))   # not a power of two


def _as3(d):
    if isinstance(d, SceneDesc3):
        return d
    assert isinstance(d, SceneDesc2)
    d3 = SceneDesc3()
    d3.base = d
    d3._keep = (getattr(d, "_keep", None), d)
    return d3


def widened_scene(kind, shape, env=True, lens=True, pick=True):
    """the scene of one kind with the features its kernels can carry (an environment map only exists for the E kinds and
    the rectangles), at one frame shape; lens / pick / env False: that feature left out"""
    rx, ry = shape
    has_env = KIND_FLAGS[kind][4] and env
    if kind == "rects":
        d3 = el.builtin_with_envmap(_sky(), scale=1.3, resx=rx, resy=ry) if has_env else ll.builtin3(resx=rx, resy=ry)
    elif kind == "quads":
        d3 = ll.builtin3(resx=rx, resy=ry)
    elif kind == "list":
        d3 = _as3(tilted_room(rx, ry))
    elif kind == "bvh":
        d3 = _as3(bumpy_room(grid=21, resx=rx, resy=ry))
    elif kind == "bvhG":
        d3 = _as3(bumpy_room(grid=21, resx=rx, resy=ry, exponent=37.5))
    elif kind == "listE":
        assert has_env
        d3 = el.builtin_with_envmap(_sky(), scale=1.3, resx=rx, resy=ry)
        glossy = [i for i in range(d3.base.nMaterials) if any(d3.base.materials[i].phong)]
        assert glossy
        d3.base.materials[glossy[0]].phongExp = 3.25
    elif kind == "bvhE":
        assert has_env
        d3 = bumpy_room(grid=21, resx=rx, resy=ry, exponent=37.5, envmap=(_sky(), 1.3))
        assert isinstance(d3, SceneDesc3)
    else:
        raise ValueError(kind)
    if pick:
        d3 = pl.add_point_lights(d3, EXTRA_LIGHTS)
        assert pl.n_lights(d3) > 4
    d4 = ll.with_lens(d3, 0.06, 4.0) if lens else ll.with_lens(d3, None, None)
    return pl.with_pick(d4, pl.POWER, 0.2) if pick else pl.with_pick(d4, None)


def widened_cases():
    """(kind, shape, algorithm, strict): VCM, BPT and the path tracer for every kind x shape; the other four algorithms
    and one strict-order VCM once per kind at 161 x 97"""
    cases = [(k, s, a, False) for k in KINDS for s in SHAPES for a in (VCM, BPT, PATH_TRACE)]
    cases += [(k, SHAPES[0], a, False) for k in KINDS for a in (LIGHT_TRACE, PPM, BPM, EYE_LIGHT)]
    cases += [(k, SHAPES[0], VCM, True) for k in KINDS]
    return cases


FEATURES_ALONE = [("rects", dict(env=True, lens=False, pick=False)), ("rects", dict(env=False, lens=True, pick=False)),
                  ("rects", dict(env=False, lens=False, pick=True)), ("bvhE", dict(env=True, lens=False, pick=False)),
                  ("bvhG", dict(env=False, lens=True, pick=False)), ("list", dict(env=False, lens=False, pick=True))]
