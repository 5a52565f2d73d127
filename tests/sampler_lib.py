"""The sampler for the tests (test infrastructure): any description as a version-7 one, the ctypes binding of
tests/host_emul_sampler/libemul_sampler.so, a numpy restatement of the Owen-scrambled Sobol sampler written from its
definition (DESIGN.md "Sampler": not from csrc/sobol.h), the known-answer records and the net check."""
import ctypes as C
import os
import subprocess

import numpy as np

import filter_lib as fl
import lens_lib as ll
from smallvcm_amd._abi import SAMPLER_PHILOX, SAMPLER_SOBOL, SceneDesc6, SceneDesc7, with_sampler

HERE = os.path.dirname(os.path.abspath(__file__))
EMUL_DIR = os.path.join(HERE, "host_emul_sampler")
OP_SAMPLER = 12   # VCM_KAT_SAMPLER
KAT = 16
PHILOX, SOBOL = SAMPLER_PHILOX, SAMPLER_SOBOL
GROUP_LIGHT, GROUP_DI, GROUP_SCATTER = 0, 1, 2   # VCM_SAMPLER_TRACE's groups
_fp = C.POINTER(C.c_float)
_up = C.POINTER(C.c_uint32)
_E = None
M32 = np.uint64(0xffffffff)


def as_desc6(d):
    return d if isinstance(d, SceneDesc6) else fl.with_filter(d, None)


def with_kind(d, kind):
    """a description seen with a sampler (kind None: sampler = NULL)"""
    return with_sampler(d.base if isinstance(d, SceneDesc7) else as_desc6(d), kind)


def builtin_sampler(kind, mask=ll.SCENE_CONFIGS[3], resx=24, resy=24):
    return with_kind(ll.builtin3(mask, resx, resy), kind)


def emul_sampler():
    """build (make: a no-op when up to date) and load the sampler host emulation"""
    global _E
    if _E is None:
        subprocess.run(["make", "-C", EMUL_DIR], check=True, stdout=subprocess.DEVNULL)
        E = C.CDLL(os.path.join(EMUL_DIR, "libemul_sampler.so"))
        P7, P6 = C.POINTER(SceneDesc7), C.POINTER(SceneDesc6)
        for name, P in (("emul_create7", P7), ("emul_create6", P6)):
            getattr(E, name).restype = C.c_void_p
            getattr(E, name).argtypes = [P, C.c_int, C.c_float, C.c_float, C.c_int, C.c_int, C.c_int]
        E.emul_destroy.argtypes = [C.c_void_p]
        E.emul_run_iteration.argtypes = [C.c_void_p, C.c_int, C.c_uint, C.c_uint]
        E.emul_get_framebuffer.argtypes = [C.c_void_p, _fp]
        E.emul_get_counts.argtypes = [C.c_void_p, C.POINTER(C.c_ubyte), C.POINTER(C.c_ubyte)]
        E.emul_get_stats.argtypes = [C.c_void_p, C.POINTER(C.c_longlong)]
        E.emul_kat7.argtypes = [P7, C.c_int, C.c_int, _fp, _fp]
        E.emul_sampler_params.argtypes = [P7, C.POINTER(C.c_int)]
        E.emul_sampler_error.restype = C.c_char_p
        E.emul_sampler_seeds.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, _up]
        E.emul_sampler_trace.argtypes = [C.c_int]
        E.emul_sampler_trace_size.restype = C.c_longlong
        E.emul_sampler_trace_get.argtypes = [_up]
        _E = E
    return _E


class Emul7(ll.Emul4):
    """one emulated renderer over a SceneDesc7 (or, version6=True, over its SceneDesc6 through emul_create6)"""

    def __init__(self, scene, algo, seed=1234, rank=0, world=1, radius_factor=0.003, radius_alpha=0.75, version6=False):
        self.E = emul_sampler()
        self.scene = scene
        create = self.E.emul_create6 if version6 else self.E.emul_create7
        assert isinstance(scene, SceneDesc6 if version6 else SceneDesc7)
        self.h = create(C.byref(scene), algo, radius_factor, radius_alpha, seed, rank, world)
        assert self.h, self.E.emul_sampler_error().decode()
        self.resx, self.resy = int(scene.camera.resolution[0]), int(scene.camera.resolution[1])
        self.N = self.resx * self.resy
        self.rank, self.world = rank, world


def kat7(scene, op, inp):
    inp = np.ascontiguousarray(inp, np.float32)
    out = np.zeros_like(inp)
    E = emul_sampler()
    assert E.emul_kat7(C.byref(scene), op, len(inp), inp.ctypes.data_as(_fp), out.ctypes.data_as(_fp)) == 0, \
        E.emul_sampler_error().decode()
    return out


def sampler_params(scene):
    k = C.c_int(-1)
    E = emul_sampler()
    assert E.emul_sampler_params(C.byref(scene), C.byref(k)) == 0, E.emul_sampler_error().decode()
    return k.value


def trace(run):
    """the (group, kind, k0) triples of the draw groups the emulation starts while run() runs"""
    E = emul_sampler()
    E.emul_sampler_trace(1)
    try:
        run()
        n = E.emul_sampler_trace_size()
        out = np.zeros((n, 3), np.uint32)
        if n:
            E.emul_sampler_trace_get(out.ctypes.data_as(_up))
    finally:
        E.emul_sampler_trace(0)
    return out


# ---- the known-answer records ----
def sampler_records(seed, i, path, kind, k):
    """VCM_KAT_SAMPLER input records: the five integers as bit patterns in floats 0..4"""
    cols = [np.asarray(c, np.uint32) for c in (seed, i, path, kind, k)]
    inp = np.zeros((len(cols[0]), KAT), np.uint32)
    for c, v in enumerate(cols):
        inp[:, c] = v
    return inp.view(np.float32)


def random_records(n=50000, seed=5):
    """n random records: i and seed over all 32 bits (the largest ones among them), k <= 127, all six kinds"""
    rng = np.random.default_rng(seed)
    u32 = lambda: rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)   # noqa: E731
    s, i, p = u32(), u32(), rng.integers(0, 1 << 22, n).astype(np.uint32)
    i[:4] = [0, 1, 0xffffffff, 0x80000000]
    s[:2] = [0xffffffff, 0]
    kind = rng.integers(0, 6, n).astype(np.uint32)
    k = rng.integers(0, 128, n).astype(np.uint32)
    k[:2] = [127, 0]
    return s, i, p, kind, k


# ---- the numpy restatement (uint64 arithmetic, masked to 32 bits) ----
def _u(x):
    return np.asarray(x, np.uint64) & M32


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    c0, c1, c2, c3, k0, k1 = (_u(np.broadcast_arrays(c0, c1, c2, c3, k0, k1)[t]).copy() for t in range(6))
    A, B = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
    for _ in range(10):
        p0, p1 = A * c0, B * c2
        n0 = (p1 >> np.uint64(32)) ^ c1 ^ k0
        n2 = (p0 >> np.uint64(32)) ^ c3 ^ k1
        c0, c1, c2, c3 = n0, p1 & M32, n2, p0 & M32
        k0 = (k0 + np.uint64(0x9E3779B9)) & M32
        k1 = (k1 + np.uint64(0xBB67AE85)) & M32
    return c0, c1, c2, c3


def brev(x):
    x = _u(x)
    r = np.zeros_like(x)
    for b in range(32):
        r |= ((x >> np.uint64(b)) & np.uint64(1)) << np.uint64(31 - b)
    return r


def lk(x, s):
    x = (_u(x) + _u(s)) & M32
    for m in (0x6c50b47c, 0xb82f1e52, 0xc7afe638, 0x8d22f6e6):
        x ^= (x * np.uint64(m)) & M32
    return x


def t_map(x):
    x = _u(x).copy()
    for sh, m in ((1, 0x55555555), (2, 0x33333333), (4, 0x0f0f0f0f), (8, 0x00ff00ff), (16, 0x0000ffff)):
        x ^= (x >> np.uint64(sh)) & np.uint64(m)
    return x


def scramble_seeds(seed, path, kind, j):
    s0, s1, s2, _ = philox4x32_10(path, kind, j, 1, seed, 0)
    return s0, s1, s2


def sobol_words(seed, i, path, kind, k):
    """the 32-bit word of float k of stream (seed, path, kind) at sample index i"""
    k = _u(k)
    s0, s1, s2 = scramble_seeds(seed, path, kind, k >> np.uint64(1))
    ip = brev(lk(brev(i), s0))
    w0 = brev(lk(ip, s1))
    w1 = brev(lk(t_map(ip), s2))
    return np.where((k & np.uint64(1)) == 1, w1, w0).astype(np.uint32)


def word_to_float(w):
    w = np.asarray(w, np.uint32)
    return ((((w >> 9).astype(np.uint64) << np.uint64(1)) | np.uint64(1)).astype(np.float64) * 2.0 ** -24).astype(np.float32)


# ---- the net property ----
def is_net(w0, w1, m):
    """do the 2^m points (w0, w1) (32-bit words; the 23 bits the floats keep are checked) put exactly one point into every
    elementary interval 2^-a x 2^-b, a + b = m?"""
    x, y = (np.asarray(w0, np.uint32) >> 9).astype(np.int64), (np.asarray(w1, np.uint32) >> 9).astype(np.int64)
    assert len(x) == 1 << m
    for a in range(m + 1):
        b = m - a
        cell = ((x >> (23 - a)) << b) | (y >> (23 - b)) if a and b else (x >> (23 - a)) if a else (y >> (23 - b)) if b else x * 0
        if len(np.unique(cell)) != 1 << m:
            return False
    return True


def float_bits23(f):
    """the 23 bits a generated float keeps: f = (2 q + 1) 2^-24 -> q, as a word with q in its top 23 bits"""
    q = ((np.asarray(f, np.float64) * 2.0 ** 24 - 1) / 2).astype(np.int64)
    return (q << 9).astype(np.uint32)
