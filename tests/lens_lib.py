"""Thin-lens scenes for the tests (test infrastructure): the built-in boxes as version-4 descriptions, and the ctypes
binding of tests/host_emul_lens/libemul_lens.so."""
import ctypes as C
import os
import subprocess

import numpy as np

from smallvcm_amd._abi import SCENE_CONFIGS, Light, Material, Prim, SceneDesc2, SceneDesc3, SceneDesc4, ThinLens
from smallvcm_amd.renderer import cornell_scene

HERE = os.path.dirname(os.path.abspath(__file__))
EMUL_DIR = os.path.join(HERE, "host_emul_lens")
OP_LENS = 8   # VCM_KAT_LENS
KAT = 16
_fp = C.POINTER(C.c_float)
_E = None


def with_lens(d3, aperture, focus):
    """a SceneDesc3 seen through a thin lens (aperture None: lens = NULL)"""
    d = SceneDesc4()
    d.base = d3
    keep = [getattr(d3, "_keep", None), d3]
    if aperture is not None:
        lens = ThinLens(float(aperture), float(focus))
        d.lens = C.pointer(lens)
        keep.append(lens)
    d._keep = tuple(keep)
    return d


def builtin3(mask=SCENE_CONFIGS[3], resx=24, resy=24):
    """a built-in box (Scene::BoxMask bits; default: scene 3) as a SceneDesc3 without an env map"""
    d1 = cornell_scene(mask, resx, resy, is_mask=True)
    prims = (Prim * d1.nPrims)(*d1.prims[:d1.nPrims])
    mats = (Material * d1.nMaterials)(*d1.materials[:d1.nMaterials])
    m2l = (C.c_int * d1.nMaterials)(*d1.mat2light[:d1.nMaterials])
    lights = (Light * d1.nLights)(*d1.lights[:d1.nLights])
    b = SceneDesc2()
    b.nPrims, b.prims = d1.nPrims, C.cast(prims, C.POINTER(Prim))
    b.nMaterials, b.materials, b.mat2light = d1.nMaterials, C.cast(mats, C.POINTER(Material)), C.cast(m2l, C.POINTER(C.c_int))
    b.nLights, b.lights = d1.nLights, C.cast(lights, C.POINTER(Light))
    b.backgroundLight = d1.backgroundLight
    b.sceneCenter[:] = d1.sceneCenter[:]
    b.sceneRadius, b.invSceneRadiusSqr = d1.sceneRadius, d1.invSceneRadiusSqr
    b.camera = d1.camera
    d = SceneDesc3()
    d.base = b
    d._keep = (prims, mats, m2l, lights)
    return d


def builtin_lens(aperture, focus, mask=SCENE_CONFIGS[3], resx=24, resy=24):
    return with_lens(builtin3(mask, resx, resy), aperture, focus)


def emul_lens():
    """build (make: a no-op when up to date) and load the thin-lens host emulation"""
    global _E
    if _E is None:
        subprocess.run(["make", "-C", EMUL_DIR], check=True, stdout=subprocess.DEVNULL)
        E = C.CDLL(os.path.join(EMUL_DIR, "libemul_lens.so"))
        P4 = C.POINTER(SceneDesc4)
        E.emul_create4.restype = C.c_void_p
        E.emul_create4.argtypes = [P4, C.c_int, C.c_float, C.c_float, C.c_int, C.c_int, C.c_int]
        E.emul_destroy.argtypes = [C.c_void_p]
        E.emul_run_iteration.argtypes = [C.c_void_p, C.c_int, C.c_uint, C.c_uint]
        E.emul_get_framebuffer.argtypes = [C.c_void_p, _fp]
        E.emul_get_counts.argtypes = [C.c_void_p, C.POINTER(C.c_ubyte), C.POINTER(C.c_ubyte)]
        E.emul_get_stats.argtypes = [C.c_void_p, C.POINTER(C.c_longlong)]
        E.emul_kat4.argtypes = [P4, C.c_int, C.c_int, _fp, _fp]
        E.emul_lens_params.argtypes = [P4, _fp]
        E.emul_lens_error.restype = C.c_char_p
        _E = E
    return _E


class Emul4:
    """one emulated renderer over a SceneDesc4 (rank / world: a shard of it)"""

    def __init__(self, scene, algo, seed=1234, rank=0, world=1, radius_factor=0.003, radius_alpha=0.75):
        self.E = emul_lens()
        self.scene = scene
        self.h = self.E.emul_create4(C.byref(scene), algo, radius_factor, radius_alpha, seed, rank, world)
        assert self.h, self.E.emul_lens_error().decode()
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


def kat4(scene, op, inp):
    inp = np.ascontiguousarray(inp, np.float32)
    out = np.zeros_like(inp)
    E = emul_lens()
    assert E.emul_kat4(C.byref(scene), op, len(inp), inp.ctypes.data_as(_fp), out.ctypes.data_as(_fp)) == 0, \
        E.emul_lens_error().decode()
    return out


def lens_params(scene):
    """(radius, focus, right[3], up[3]) as the scene host stores them"""
    out = np.zeros(8, np.float32)
    E = emul_lens()
    assert E.emul_lens_params(C.byref(scene), out.ctypes.data_as(_fp)) == 0, E.emul_lens_error().decode()
    return float(out[0]), float(out[1]), out[2:5].copy(), out[5:8].copy()


def lens_records(raster, lens_uv, world):
    """VCM_KAT_LENS input records: raster x, y; lens sample u1, u2; world point"""
    n = len(raster)
    inp = np.zeros((n, KAT), np.float32)
    inp[:, 0:2] = raster
    inp[:, 2:4] = lens_uv
    inp[:, 4:7] = world
    return inp
