"""Environment-map scenes for the tests (test infrastructure): procedural skies, the built-in scene 3 with its
BackgroundLight replaced by a map, and the ctypes binding of tests/host_emul_envmap/libemul_envmap.so."""
import ctypes as C
import os
import subprocess

import numpy as np

from smallvcm_amd._abi import SCENE_CONFIGS, Light, Material, Prim, SceneDesc2, SceneDesc3, EnvMap
from smallvcm_amd.renderer import cornell_scene, load_library

HERE = os.path.dirname(os.path.abspath(__file__))
EMUL_DIR = os.path.join(HERE, "host_emul_envmap")
_fp, _ip = C.POINTER(C.c_float), C.POINTER(C.c_int)
_E = None


def sky(W, H, sun=(0.3, 0.2), sun_size=2, sun_value=(60.0, 55.0, 45.0), black_below=0.875):
    """a gradient sky (bright at the horizon, blue at the zenith), a `sun_size`^2 block of bright texels whose corner sits
    at (u, v) = sun, and black texels below v = black_below (the ground: rows of zero weight)"""
    v = (np.arange(H, dtype=np.float64) + 0.5) / H
    u = (np.arange(W, dtype=np.float64) + 0.5) / W
    base = np.stack([0.25 + 0.6 * v, 0.45 + 0.4 * v, 0.9 + 0.05 * v], axis=1)
    img = np.repeat(base[:, None, :], W, axis=1) * (1.0 + 0.1 * np.cos(2 * np.pi * u))[None, :, None]
    img[v >= black_below] = 0.0
    r0, c0 = int(sun[1] * H), int(sun[0] * W)
    img[r0:r0 + sun_size, c0:c0 + sun_size] = sun_value
    return np.ascontiguousarray(img, dtype=np.float32)


def builtin_with_envmap(img, scale=1.0, resx=24, resy=24, mask=SCENE_CONFIGS[3]):
    """a built-in box with a BackgroundLight (default: scene 3; `mask` = Scene::BoxMask bits) as a SceneDesc3 whose
    background light is the map"""
    L = load_library(require_gpu=False)
    L.vcm_make_envmap_light.argtypes = [C.c_float, C.POINTER(Light)]
    L.vcm_make_envmap_light.restype = None
    d1 = cornell_scene(mask, resx, resy, is_mask=True)
    assert d1.backgroundLight >= 0
    prims = (Prim * d1.nPrims)(*d1.prims[:d1.nPrims])
    mats = (Material * d1.nMaterials)(*d1.materials[:d1.nMaterials])
    m2l = (C.c_int * d1.nMaterials)(*d1.mat2light[:d1.nMaterials])
    lights = (Light * d1.nLights)(*d1.lights[:d1.nLights])
    L.vcm_make_envmap_light(float(scale), C.byref(lights[d1.backgroundLight]))
    b = SceneDesc2()
    b.nPrims, b.prims = d1.nPrims, C.cast(prims, C.POINTER(Prim))
    b.nMaterials, b.materials, b.mat2light = d1.nMaterials, C.cast(mats, C.POINTER(Material)), C.cast(m2l, C.POINTER(C.c_int))
    b.nLights, b.lights = d1.nLights, C.cast(lights, C.POINTER(Light))
    b.backgroundLight = d1.backgroundLight
    b.sceneCenter[:] = d1.sceneCenter[:]
    b.sceneRadius, b.invSceneRadiusSqr = d1.sceneRadius, d1.invSceneRadiusSqr
    b.camera = d1.camera
    img = np.ascontiguousarray(img, dtype=np.float32)
    m = EnvMap()
    m.height, m.width = img.shape[0], img.shape[1]
    m.rgb = img.ctypes.data_as(_fp)
    d = SceneDesc3()
    d.base = b
    d.envmap = C.pointer(m)
    d._keep = (prims, mats, m2l, lights, img, m)
    return d


def emul_envmap():
    """build (make: a no-op when up to date) and load the env-map host emulation"""
    global _E
    if _E is None:
        subprocess.run(["make", "-C", EMUL_DIR], check=True, stdout=subprocess.DEVNULL)
        E = C.CDLL(os.path.join(EMUL_DIR, "libemul_envmap.so"))
        P3 = C.POINTER(SceneDesc3)
        E.emul_create3.restype = C.c_void_p
        E.emul_create3.argtypes = [P3, C.c_int, C.c_float, C.c_float, C.c_int, C.c_int, C.c_int]
        E.emul_destroy.argtypes = [C.c_void_p]
        E.emul_run_iteration.argtypes = [C.c_void_p, C.c_int, C.c_uint, C.c_uint]
        E.emul_get_framebuffer.argtypes = [C.c_void_p, _fp]
        E.emul_get_counts.argtypes = [C.c_void_p, C.POINTER(C.c_ubyte), C.POINTER(C.c_ubyte)]
        E.emul_get_stats.argtypes = [C.c_void_p, C.POINTER(C.c_longlong)]
        E.emul_kat3.argtypes = [P3, C.c_int, C.c_int, _fp, _fp]
        E.emul_env_tables.argtypes = [P3, _ip, _fp, _fp, _fp]
        E.emul_env_lookup.argtypes = [P3, C.c_int, _fp, _ip, _fp]
        E.emul_env_uv_dir.argtypes = [C.c_int, _fp, _fp]
        E.emul_env_uv_dir.restype = None
        E.emul_atan2f_n.argtypes = [C.c_int, _fp, _fp, _fp]
        E.emul_atan2f_n.restype = None
        E.emul_acosf_n.argtypes = [C.c_int, _fp, _fp]
        E.emul_acosf_n.restype = None
        E.emul_envmap_error.restype = C.c_char_p
        _E = E
    return _E


class Emul3:
    """one emulated renderer over a SceneDesc3 (rank / world: a shard of it)"""

    def __init__(self, scene, algo, seed=1234, rank=0, world=1, radius_factor=0.003, radius_alpha=0.75):
        self.E = emul_envmap()
        self.scene = scene
        self.h = self.E.emul_create3(C.byref(scene), algo, radius_factor, radius_alpha, seed, rank, world)
        assert self.h, self.E.emul_envmap_error().decode()
        self.resx, self.resy = int(scene.camera.resolution[0]), int(scene.camera.resolution[1])
        self.N = self.resx * self.resy
        self.rank, self.world = rank, world

    def __del__(self):
        if getattr(self, "h", None):
            self.E.emul_destroy(self.h)
            self.h = None

    def run_iteration(self, it, min_len=0, max_len=10):
        self.E.emul_run_iteration(self.h, it, min_len, max_len)

    def framebuffer(self):
        out = np.zeros((self.resy, self.resx, 3), np.float32)
        self.E.emul_get_framebuffer(self.h, out.ctypes.data_as(_fp))
        return out

    def counts(self):
        n = self.N * (self.rank + 1) // self.world - self.N * self.rank // self.world
        a, b = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
        self.E.emul_get_counts(self.h, a.ctypes.data_as(C.POINTER(C.c_ubyte)), b.ctypes.data_as(C.POINTER(C.c_ubyte)))
        return a, b

    def stats(self):
        st = (C.c_longlong * 9)()
        self.E.emul_get_stats(self.h, st)
        keys = ("lightRays", "cameraRays", "shadowRays", "mergeQueries", "mergeCandidates", "mergeAccepted",
                "connections", "lightSplats", "lightVertices")
        return dict(zip(keys, list(st)))


def kat3(scene, op, inp):
    out = np.zeros_like(inp)
    assert emul_envmap().emul_kat3(C.byref(scene), op, len(inp), inp.ctypes.data_as(_fp), out.ctypes.data_as(_fp)) == 0
    return out


def tables(scene):
    E = emul_envmap()
    dims = (C.c_int * 4)()
    assert E.emul_env_tables(C.byref(scene), dims, None, None, None) == 0, E.emul_envmap_error().decode()
    W, H = dims[0], dims[1]
    tex = np.zeros((H, W, 4), np.float32)
    marg = np.zeros(H + 1, np.float32)
    cond = np.zeros((H, W + 1), np.float32)
    assert E.emul_env_tables(C.byref(scene), dims, tex.ctypes.data_as(_fp), marg.ctypes.data_as(_fp), cond.ctypes.data_as(_fp)) == 0
    return tex, marg, cond


def lookup(scene, dirs):
    dirs = np.ascontiguousarray(dirs, np.float32)
    idx = np.zeros(len(dirs), np.int32)
    pdf = np.zeros(len(dirs), np.float32)
    assert emul_envmap().emul_env_lookup(C.byref(scene), len(dirs), dirs.ctypes.data_as(_fp), idx.ctypes.data_as(_ip),
                                         pdf.ctypes.data_as(_fp)) == 0
    return idx, pdf


def uv_dirs(uv):
    uv = np.ascontiguousarray(uv, np.float32)
    out = np.zeros((len(uv), 3), np.float32)
    emul_envmap().emul_env_uv_dir(len(uv), uv.ctypes.data_as(_fp), out.ctypes.data_as(_fp))
    return out
