"""The firefly-robust estimate for the tests (test infrastructure): the ctypes binding of
tests/host_emul_robust/libemul_robust.so, built on demand, an emulated renderer with robust (and variance) tracking, and a
float64 numpy restatement of the rule of vcm_robust.h."""
import ctypes as C
import os
import subprocess

import numpy as np

import variance_lib as vl
from smallvcm_amd._abi import ROBUST_DEFAULT_BUCKETS, RobustStats

HERE = os.path.dirname(os.path.abspath(__file__))
EMUL_DIR = os.path.join(HERE, "host_emul_robust")
DEFAULT_MAX_BLOCKS = vl.DEFAULT_MAX_BLOCKS   # the robust kernels run on the variance kernels' grid
DEFAULT_BUCKETS = ROBUST_DEFAULT_BUCKETS
ODD = (3, 5, 7, 9, 11, 13, 15)
LUMA = (0.212671, 0.715160, 0.072169)
_fp = C.POINTER(C.c_float)
_ip = C.POINTER(C.c_int)
_E = None


def emul_robust():
    """build (make: a no-op when up to date) and load the robust host emulation"""
    global _E
    if _E is None:
        subprocess.run(["make", "-C", EMUL_DIR], check=True, stdout=subprocess.DEVNULL)
        E = C.CDLL(os.path.join(EMUL_DIR, "libemul_robust.so"))
        E.emul_robust_update.argtypes = [C.c_longlong, _fp, C.c_int, C.c_int, _fp, _fp]
        E.emul_robust_resolve.argtypes = [C.c_longlong, _fp, _fp, C.c_int, C.c_int, _fp, _fp, _ip, _ip]
        E.emul_robust_stats.argtypes = [C.c_longlong, _fp, _fp, C.c_int, C.c_int, C.c_int, C.POINTER(RobustStats)]
        E.emul_robust_bucket_count.argtypes = [C.c_int, C.c_int, C.c_int]
        E.emul_pick_error.restype = C.c_char_p
        _E = E
    return _E


def new_images(n, M):
    """(prev [n, 4], buckets [M, n, 4]), zeroed"""
    return np.zeros((n, 4), np.float32), np.zeros((M, n, 4), np.float32)


def bucket_counts(k, M):
    """n_j = ceil((k - j) / M), j = 0 .. M - 1: the iterations bucket j holds after k"""
    return np.array([max(0, -((j - k) // M)) for j in range(M)])


def update(sum3, k, prev, buckets, check=True):
    """iteration k's (1, 2, ...) update of prev ([n, 4]) and buckets ([M, n, 4]) from the running sum sum3 ([..., 3]), in
    place; check=False: False where it is refused"""
    sum3 = np.ascontiguousarray(sum3, np.float32)
    M, n = buckets.shape[:2]
    assert sum3.size == 3 * n and prev.shape == (n, 4) and buckets.shape == (M, n, 4) and prev.dtype == buckets.dtype == np.float32
    E = emul_robust()
    rc = E.emul_robust_update(n, sum3.ctypes.data_as(_fp), k, M, prev.ctypes.data_as(_fp), buckets.ctypes.data_as(_fp))
    assert rc == 0 or not check, E.emul_pick_error().decode()
    return rc == 0


def resolve(prev, buckets, k, info=False, check=True, out=None):
    """the emulated k_robust_resolve: [n, 4] = {rgb, 1}; info=True: (out, gini [n], trim [n], kept [n]); check=False: None
    where it is refused"""
    M, n = buckets.shape[:2]
    out = np.zeros((n, 4), np.float32) if out is None else out
    gini, trim, kept = np.zeros(n, np.float32), np.zeros(n, np.int32), np.zeros(n, np.int32)
    E = emul_robust()
    rc = E.emul_robust_resolve(n, prev.ctypes.data_as(_fp), buckets.ctypes.data_as(_fp), k, M, out.ctypes.data_as(_fp),
                               gini.ctypes.data_as(_fp), trim.ctypes.data_as(_ip), kept.ctypes.data_as(_ip))
    if rc != 0:
        assert not check, E.emul_pick_error().decode()
        return None
    return (out, gini, trim, kept) if info else out


def stats(prev, buckets, k, max_blocks=DEFAULT_MAX_BLOCKS, check=True):
    """the emulated vcm_get_robust_stats as a dict; check=False: None where it is refused"""
    M, n = buckets.shape[:2]
    st = RobustStats()
    E = emul_robust()
    rc = E.emul_robust_stats(n, prev.ctypes.data_as(_fp), buckets.ctypes.data_as(_fp), k, M, max_blocks, C.byref(st))
    if rc != 0:
        assert not check, E.emul_pick_error().decode()
        return None
    return st.asdict()


def feed(frames, M):
    """frames [K, n, 3] -> (sums [K, n, 3] as the fp32 framebuffer accumulates them, prev, buckets after the K updates)"""
    frames = np.asarray(frames, np.float32)
    prev, buckets = new_images(frames.shape[1], M)
    s = np.zeros(frames.shape[1:], np.float32)
    sums = []
    for k in range(frames.shape[0]):
        s = s + frames[k]
        sums.append(s.copy())
        update(s, k + 1, prev, buckets)
    return np.stack(sums), prev, buckets


def buckets64(sums, M):
    """float64 restatement of the accumulation: the running sums [K, n, 3] taken as exact -> [M, n, 3], bucket j the sum of
    the frames j, j + M, ... (0-based)"""
    s = np.asarray(sums, np.float64)
    x = np.diff(np.concatenate([np.zeros_like(s[:1]), s]), axis=0)
    return np.stack([x[j::M].sum(axis=0) if j < x.shape[0] else np.zeros_like(x[0]) for j in range(M)])


def resolve64(prev, buckets, k, trim=None):
    """float64 numpy restatement of the rule over the fp32 images taken as exact -> (rgb [n, 3], G [n], t [n], M' [n], edge
    [n]: G M' / 2 lies within 1e-5 of an integer, where a last-bit difference of G may move floor()).
    trim: None = the rule; "never" = t 0 everywhere (the mean of all finite buckets); "median" = t (M' - 1) / 2 everywhere."""
    M, n = buckets.shape[:2]
    B = buckets[..., :3].astype(np.float64)
    cnt = bucket_counts(k, M).astype(np.float64)
    with np.errstate(all="ignore"):
        m = B / cnt[:, None, None]
        y = m @ np.array(LUMA)                                       # [M, n]
        keep = np.isfinite(y) & (np.abs(y) <= np.finfo(np.float32).max)   # the fp32 key overflows where this one exceeds fp32
    mp = keep.sum(axis=0)
    idx = np.arange(M)
    yk = np.where(keep, y, 0.0)
    before = (yk[:, None, :] < yk[None, :, :]) | ((yk[:, None, :] == yk[None, :, :]) & (idx[:, None, None] < idx[None, :, None]))
    rank = (before & keep[:, None, :]).sum(axis=0)                   # [j, n]: kept i that come before j
    with np.errstate(all="ignore"):
        den = yk.sum(axis=0)
        num = (np.where(keep, (2 * (rank + 1) - mp - 1), 0) * yk).sum(axis=0)
        G = np.where(den > 0, num / (mp * den), 0.0)
    G = np.clip(np.nan_to_num(G, nan=0.0), 0.0, 1.0)
    half = np.maximum(mp - 1, 0) // 2
    x = G * mp / 2
    t = np.minimum(half, np.floor(x).astype(np.int64))
    edge = (np.abs(x - np.round(x)) < 1e-5) & (np.round(x) <= half) & (np.round(x) >= 1)
    if trim == "never":
        t = np.zeros_like(half)
    elif trim == "median":
        t = half
    inside = keep & (rank >= t) & (rank < mp - t)
    with np.errstate(all="ignore"):
        rgb = np.where(inside[..., None], B, 0.0).sum(axis=0) / np.where(inside, cnt[:, None], 0.0).sum(axis=0)[:, None]
        rgb = np.where((mp == 0)[:, None], prev[:, :3].astype(np.float64) / k, rgb)
    return rgb, G, np.where(mp == 0, 0, t), mp, edge


def stats64(prev, buckets, k):
    """float64 numpy restatement of the statistics over what the fp32 rule decided per pixel (the emulation's own gini, trim
    and kept: the reduction is what is restated)"""
    M, n = buckets.shape[:2]
    _, gini, trim, kept = resolve(prev, buckets, k, info=True)
    g = gini.astype(np.float64)
    return {"iterations": k, "buckets": M, "pixels": n, "trimmed": int((trim > 0).sum()), "nonFinite": int((kept < M).sum()),
            "meanGini": float(g.mean()), "maxGini": float(g.max())}


class RobustEmul(vl.TrackedEmul):
    """vl.TrackedEmul -- an emulated renderer with variance tracking, driven by render_until -- that also does what a
    context with vcm_track_robust(M) does, iteration by iteration; buckets=0: robust tracking off"""

    def __init__(self, scene, algo, seed=1234, max_len=10, max_blocks=DEFAULT_MAX_BLOCKS, buckets=DEFAULT_BUCKETS):
        super().__init__(scene, algo, seed, max_len, max_blocks)
        self.M = buckets
        if buckets:
            self.rprev, self.buckets = new_images(self.emul.resx * self.emul.resy, buckets)

    def RunIteration(self, it):
        super().RunIteration(it)
        if self.M:
            update(self.emul.framebuffer(), self.mIterations, self.rprev, self.buckets)

    def robust4(self):
        return resolve(self.rprev, self.buckets, self.mIterations)

    def robust(self):
        return self.robust4()[:, :3].reshape(self.emul.resy, self.emul.resx, 3)

    def robust_stats(self, check=True):
        return stats(self.rprev, self.buckets, self.mIterations, self.max_blocks, check)
