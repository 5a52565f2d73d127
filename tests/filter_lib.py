"""Pixel-filter scenes for the tests (test infrastructure): any description as a version-6 one, the ctypes binding of
tests/host_emul_filter/libemul_filter.so, and the effective filter h = box * g by quadrature."""
import ctypes as C
import os
import subprocess

import numpy as np

import lens_lib as ll
import pick_lib as pl
from smallvcm_amd._abi import FILTER_BOX, FILTER_BSPLINE, FILTER_TENT, PixelFilter, SceneDesc5, SceneDesc6

HERE = os.path.dirname(os.path.abspath(__file__))
EMUL_DIR = os.path.join(HERE, "host_emul_filter")
OP_FILTER = 10   # VCM_KAT_FILTER
KAT = 16
BOX, TENT, BSPLINE = FILTER_BOX, FILTER_TENT, FILTER_BSPLINE
_fp = C.POINTER(C.c_float)
_E = None


def as_desc5(d):
    """any description up to version 5 as a SceneDesc5 (no lens, no light selection added)"""
    return d if isinstance(d, SceneDesc5) else pl.with_pick(d, None)


def with_filter(d, kind, radius=0.0):
    """a description seen with a pixel filter (kind None: filter = NULL)"""
    d5 = as_desc5(d)
    d6 = SceneDesc6()
    d6.base = d5
    keep = [getattr(d5, "_keep", None), d5]
    if kind is not None:
        f = PixelFilter(int(kind), float(radius))
        d6.filter = C.pointer(f)
        keep.append(f)
    d6._keep = tuple(keep)
    return d6


def builtin_filter(kind, radius=0.0, mask=ll.SCENE_CONFIGS[3], resx=24, resy=24):
    return with_filter(ll.builtin3(mask, resx, resy), kind, radius)


def emul_filter():
    """build (make: a no-op when up to date) and load the pixel-filter host emulation"""
    global _E
    if _E is None:
        subprocess.run(["make", "-C", EMUL_DIR], check=True, stdout=subprocess.DEVNULL)
        E = C.CDLL(os.path.join(EMUL_DIR, "libemul_filter.so"))
        P6 = C.POINTER(SceneDesc6)
        E.emul_create6.restype = C.c_void_p
        E.emul_create6.argtypes = [P6, C.c_int, C.c_float, C.c_float, C.c_int, C.c_int, C.c_int]
        E.emul_destroy.argtypes = [C.c_void_p]
        E.emul_run_iteration.argtypes = [C.c_void_p, C.c_int, C.c_uint, C.c_uint]
        E.emul_get_framebuffer.argtypes = [C.c_void_p, _fp]
        E.emul_get_counts.argtypes = [C.c_void_p, C.POINTER(C.c_ubyte), C.POINTER(C.c_ubyte)]
        E.emul_get_stats.argtypes = [C.c_void_p, C.POINTER(C.c_longlong)]
        E.emul_kat6.argtypes = [P6, C.c_int, C.c_int, _fp, _fp]
        E.emul_filter_params.argtypes = [P6, C.POINTER(C.c_int), _fp]
        E.emul_filter_error.restype = C.c_char_p
        _E = E
    return _E


class Emul6(ll.Emul4):
    """one emulated renderer over a SceneDesc6, or over an older description without a filter (rank / world: a shard of it)"""

    def __init__(self, scene, algo, seed=1234, rank=0, world=1, radius_factor=0.003, radius_alpha=0.75):
        self.E = emul_filter()
        scene = scene if isinstance(scene, SceneDesc6) else with_filter(scene, None)
        self.scene = scene
        self.h = self.E.emul_create6(C.byref(scene), algo, radius_factor, radius_alpha, seed, rank, world)
        assert self.h, self.E.emul_filter_error().decode()
        self.resx, self.resy = int(scene.camera.resolution[0]), int(scene.camera.resolution[1])
        self.N = self.resx * self.resy
        self.rank, self.world = rank, world


def render(scene, algo, iters=2, seed=1234, **kw):
    """-> (framebuffer, stats, (light counts, camera counts)) of `iters` emulated iterations"""
    e = Emul6(scene, algo, seed=seed, **kw)
    for it in range(iters):
        e.run_iteration(it)
    return e.framebuffer(), e.stats(), e.counts()


def kat6(scene, op, inp):
    inp = np.ascontiguousarray(inp, np.float32)
    out = np.zeros_like(inp)
    E = emul_filter()
    assert E.emul_kat6(C.byref(scene), op, len(inp), inp.ctypes.data_as(_fp), out.ctypes.data_as(_fp)) == 0, \
        E.emul_filter_error().decode()
    return out


def filter_params(scene):
    """(kind, radius) as the scene host stores them"""
    k, r = C.c_int(-1), C.c_float(-1.0)
    E = emul_filter()
    assert E.emul_filter_params(C.byref(scene), C.byref(k), C.byref(r)) == 0, E.emul_filter_error().decode()
    return k.value, r.value


def filter_records(raster, u):
    """VCM_KAT_FILTER input records: raster x, y, then the 8 floats of a filter draw"""
    n = len(u)
    inp = np.zeros((n, KAT), np.float32)
    inp[:, 0:2] = raster
    inp[:, 2:10] = u
    return inp


def uniforms(rng, n):
    """n x 8 floats of the generator's form (2j + 1) 2^-24, j < 2^23: in (0, 1), as the device draws them"""
    j = rng.integers(0, 1 << 23, size=(n, 8), dtype=np.int64)
    return ((2 * j + 1).astype(np.float64) * 2.0 ** -24).astype(np.float32)


def g_cdf(kind, radius, t):
    """the distribution function of one axis of the offset density g at t (float64, analytic)"""
    x = np.clip(np.asarray(t, np.float64) / radius, -1.0, 1.0)
    if kind == TENT:       # u1 - u2: the triangle on (-1, 1)
        return np.where(x < 0, 0.5 * (1 + x) ** 2, 1 - 0.5 * (1 - x) ** 2)
    assert kind == BSPLINE   # (u1 + u2 + u3 + u4 - 2) / 2: Irwin-Hall of order 4, s = 2 x + 2 in (0, 4)
    s = 2 * x + 2
    k = np.arange(5)[:, None]
    binom = np.array([1, 4, 6, 4, 1], np.float64)[:, None]
    terms = (-1.0) ** k * binom * np.clip(s[None, ...].reshape(1, -1) - k, 0, None) ** 4
    return (terms.sum(axis=0) / 24.0).reshape(np.shape(s))


def pixel_prob_1d(kind, radius, x, pixels):
    """the probability that x + o, o ~ g, falls into pixel q = [q, q + 1) for every q in `pixels`: h(c_q - x)"""
    q = np.asarray(pixels, np.float64)
    return g_cdf(kind, radius, q + 1 - x) - g_cdf(kind, radius, q - x)


def h_1d(kind, radius, d):
    """the effective filter h = box * g at distance d from the pixel centre, in closed form"""
    return g_cdf(kind, radius, d + 0.5) - g_cdf(kind, radius, d - 0.5)
