"""Feature buffers and denoiser for the tests (test infrastructure): the ctypes binding of
tests/host_emul_denoise/libemul_denoise.so, built on demand, and helpers to make guide images and renders."""
import ctypes as C
import os
import subprocess

import numpy as np

import pick_lib as pl
from smallvcm_amd._abi import DenoiseParams, SceneDesc5

HERE = os.path.dirname(os.path.abspath(__file__))
EMUL_DIR = os.path.join(HERE, "host_emul_denoise")
_fp = C.POINTER(C.c_float)
_E = None


def emul_denoise():
    """build (make: a no-op when up to date) and load the denoiser host emulation"""
    global _E
    if _E is None:
        subprocess.run(["make", "-C", EMUL_DIR], check=True, stdout=subprocess.DEVNULL)
        E = C.CDLL(os.path.join(EMUL_DIR, "libemul_denoise.so"))
        P5 = C.POINTER(SceneDesc5)
        E.emul_create5.restype = C.c_void_p
        E.emul_create5.argtypes = [P5, C.c_int, C.c_float, C.c_float, C.c_int, C.c_int, C.c_int]
        E.emul_destroy.argtypes = [C.c_void_p]
        E.emul_run_iteration.argtypes = [C.c_void_p, C.c_int, C.c_uint, C.c_uint]
        E.emul_get_framebuffer.argtypes = [C.c_void_p, _fp]
        E.emul_features5.argtypes = [P5, C.c_int, C.c_int, _fp, _fp]
        E.emul_denoise.argtypes = [C.c_int, C.c_int, _fp, _fp, C.c_float, _fp, _fp, _fp, C.POINTER(DenoiseParams)]
        E.emul_pick_error.restype = C.c_char_p
        _E = E
    return _E


def desc5(d):
    """any scene description as a SceneDesc5 (no lens, no light table added)"""
    return d if isinstance(d, SceneDesc5) else pl.with_pick(d, None)


def box(scene_id, resx, resy):
    """built-in box `scene_id` (config.hxx:146-151) as a SceneDesc5"""
    import lens_lib as ll
    from smallvcm_amd._abi import SCENE_CONFIGS
    return desc5(ll.builtin3(SCENE_CONFIGS[scene_id], resx, resy))


def defaults():
    from smallvcm_amd.renderer import load_library
    L = load_library(require_gpu=False)
    L.vcm_denoise_defaults.argtypes = [C.POINTER(DenoiseParams)]
    L.vcm_denoise_defaults.restype = None
    p = DenoiseParams()
    L.vcm_denoise_defaults(C.byref(p))
    return p


def params(**kw):
    """the defaults with some members replaced (passes, sigmaColor, sigmaNormal, sigmaDepth, demodulate)"""
    p = defaults()
    for k, v in kw.items():
        assert hasattr(p, k), k
        setattr(p, k, v)
    return p


def features(scene, rank=0, world=1):
    """-> (guide [H, W, 4] = normal.xyz | depth, albedo [H, W, 4] = rgb | 1) of the host emulation"""
    d = desc5(scene)
    W, H = int(d.camera.resolution[0]), int(d.camera.resolution[1])
    g, a = np.zeros((H, W, 4), np.float32), np.zeros((H, W, 4), np.float32)
    E = emul_denoise()
    assert E.emul_features5(C.byref(d), rank, world, g.ctypes.data_as(_fp), a.ctypes.data_as(_fp)) == 0, E.emul_pick_error().decode()
    return g, a


def denoise(color, albedo, guide, p, scale=1.0, check=True):
    """the emulated filter: color [H, W, 4] (a float4 image) or [H, W, 3] (a framebuffer, multiplied by scale first)
    -> [H, W, 4]; check=False: returns None where the parameters are refused"""
    color = np.ascontiguousarray(color, np.float32)
    albedo, guide = np.ascontiguousarray(albedo, np.float32), np.ascontiguousarray(guide, np.float32)
    H, W = color.shape[:2]
    assert albedo.shape == (H, W, 4) and guide.shape == (H, W, 4)
    out = np.zeros((H, W, 4), np.float32)
    E = emul_denoise()
    c4 = color.ctypes.data_as(_fp) if color.shape[2] == 4 else None
    c3 = color.ctypes.data_as(_fp) if color.shape[2] == 3 else None
    rc = E.emul_denoise(W, H, c4, c3, scale, albedo.ctypes.data_as(_fp), guide.ctypes.data_as(_fp), out.ctypes.data_as(_fp), C.byref(p))
    if rc != 0:
        assert not check, E.emul_pick_error().decode()
        return None
    return out


def flat_guides(H, W, normal=(0.0, 0.0, 1.0), depth=1.0):
    """one surface everywhere: guide and a white albedo"""
    g = np.zeros((H, W, 4), np.float32)
    g[..., :3] = normal
    g[..., 3] = depth
    return g, np.ones((H, W, 4), np.float32)


def as4(rgb):
    out = np.ones(rgb.shape[:2] + (4,), np.float32)
    out[..., :3] = rgb
    return out


class Emul:
    """one emulated renderer over any scene description"""

    def __init__(self, scene, algo, seed=1234):
        self.E = emul_denoise()
        self.scene = desc5(scene)
        self.h = self.E.emul_create5(C.byref(self.scene), algo, 0.003, 0.75, seed, 0, 1)
        assert self.h, self.E.emul_pick_error().decode()
        self.resx, self.resy = int(self.scene.camera.resolution[0]), int(self.scene.camera.resolution[1])
        self.iterations = 0

    def __del__(self):
        if getattr(self, "h", None):
            self.E.emul_destroy(self.h)
            self.h = None

    def run(self, n, max_len=10):
        for _ in range(n):
            self.E.emul_run_iteration(self.h, self.iterations, 0, max_len)
            self.iterations += 1
        return self

    def framebuffer(self):
        out = np.zeros((self.resy, self.resx, 3), np.float32)
        self.E.emul_get_framebuffer(self.h, out.ctypes.data_as(_fp))
        return out

    def mean(self):
        return self.framebuffer() * np.float32(1.0 / self.iterations)


def rel_mse(img, ref):
    """mean over pixels and channels of (img - ref)^2 / (ref^2 + 0.01)"""
    img, ref = np.asarray(img, np.float64)[..., :3], np.asarray(ref, np.float64)[..., :3]
    return float(np.mean((img - ref) ** 2 / (ref ** 2 + 1e-2)))
