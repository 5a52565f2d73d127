"""Per-pixel variance and the noise statistic for the tests (test infrastructure): the ctypes binding of
tests/host_emul_variance/libemul_variance.so, built on demand, a tracked emulated renderer, and float64 numpy
restatements of what vcm_variance.h computes."""
import ctypes as C
import os
import subprocess

import numpy as np

import denoise_lib as dl
from smallvcm_amd._abi import DenoiseParams2, NoiseStats

HERE = os.path.dirname(os.path.abspath(__file__))
EMUL_DIR = os.path.join(HERE, "host_emul_variance")
DEFAULT_MAX_BLOCKS = 2048   # VCM_VAR_DEFAULT_MAX_BLOCKS
BLOCK = 256                 # VCM_VAR_BLOCK
_fp = C.POINTER(C.c_float)
_E = None


def emul_variance():
    """build (make: a no-op when up to date) and load the variance host emulation"""
    global _E
    if _E is None:
        subprocess.run(["make", "-C", EMUL_DIR], check=True, stdout=subprocess.DEVNULL)
        E = C.CDLL(os.path.join(EMUL_DIR, "libemul_variance.so"))
        E.emul_var_update.argtypes = [C.c_longlong, _fp, C.c_int, _fp, _fp]
        E.emul_var_update.restype = None
        E.emul_var_read.argtypes = [C.c_longlong, _fp, C.c_int, _fp]
        E.emul_var_read.restype = None
        E.emul_var_stats.argtypes = [C.c_longlong, _fp, _fp, C.c_int, C.c_float, C.c_int, C.POINTER(NoiseStats)]
        E.emul_denoise2.argtypes = [C.c_int, C.c_int, _fp, _fp, C.c_float, _fp, _fp, _fp, C.c_float, _fp, C.POINTER(DenoiseParams2)]
        E.emul_pick_error.restype = C.c_char_p
        _E = E
    return _E


def new_images(n):
    """(prev, mom): two zeroed float4 images of n pixels"""
    return np.zeros((n, 4), np.float32), np.zeros((n, 4), np.float32)


def update(sum3, k, prev, mom):
    """iteration k's (1, 2, ...) update of prev, mom ([n, 4]) from the running sum sum3 ([..., 3]), in place"""
    sum3 = np.ascontiguousarray(sum3, np.float32)
    n = prev.shape[0]
    assert sum3.size == 3 * n and prev.shape == mom.shape == (n, 4) and prev.dtype == mom.dtype == np.float32
    emul_variance().emul_var_update(n, sum3.ctypes.data_as(_fp), k, prev.ctypes.data_as(_fp), mom.ctypes.data_as(_fp))


def variance(mom, k):
    """V = M2 / (k (k - 1)) of every pixel and channel, [n, 3]"""
    out = np.zeros((mom.shape[0], 3), np.float32)
    emul_variance().emul_var_read(mom.shape[0], mom.ctypes.data_as(_fp), k, out.ctypes.data_as(_fp))
    return out


def stats(prev, mom, k, threshold=np.inf, max_blocks=DEFAULT_MAX_BLOCKS, check=True):
    """the emulated vcm_get_noise_stats as a dict; check=False: None where it is refused"""
    st = NoiseStats()
    E = emul_variance()
    rc = E.emul_var_stats(prev.shape[0], prev.ctypes.data_as(_fp), mom.ctypes.data_as(_fp), k, threshold, max_blocks, C.byref(st))
    if rc != 0:
        assert not check, E.emul_pick_error().decode()
        return None
    return st.asdict()


def feed(frames):
    """frames [K, n, 3] -> (sums [K, n, 3] as the fp32 framebuffer accumulates them, prev, mom after the K updates)"""
    frames = np.asarray(frames, np.float32)
    prev, mom = new_images(frames.shape[1])
    s = np.zeros(frames.shape[1:], np.float32)
    sums = []
    for k in range(frames.shape[0]):
        s = s + frames[k]
        sums.append(s.copy())
        update(s, k + 1, prev, mom)
    return np.stack(sums), prev, mom


def welford64(sums):
    """float64 restatement: the running sums [K, n, 3] taken as exact -> M2 [n, 3] of the K samples S_k - S_{k-1}"""
    s = np.asarray(sums, np.float64)
    x = np.diff(np.concatenate([np.zeros_like(s[:1]), s]), axis=0)
    return ((x - x.mean(axis=0)) ** 2).sum(axis=0)


def stats64(prev, mom, k, threshold=np.inf):
    """float64 numpy restatement of the statistic over the fp32 per-element noise the kernel forms"""
    k32, kk32 = np.float32(k), np.float32(float(k) * float(k - 1))
    with np.errstate(all="ignore"):
        mean = prev[:, :3] / k32
        noise = (mom[:, :3] / kk32) / (mean * mean + np.float32(0.01))
    assert noise.dtype == np.float32
    fin = np.isfinite(noise)
    good = noise[fin].astype(np.float64)
    return {"iterations": k, "elements": noise.size, "above": int((good > threshold).sum()), "nonFinite": int((~fin).sum()),
            "mean": float(good.mean()) if good.size else 0.0, "max": float(good.max()) if good.size else 0.0}


def params2(**kw):
    """vcm_denoise_defaults2 with some members replaced"""
    from smallvcm_amd.renderer import denoise_params2
    return denoise_params2(**kw)


def denoise2(color, albedo, guide, mom, var_factor, p, scale=1.0, check=True):
    """the emulated guided filter: color [H, W, 4] or a framebuffer [H, W, 3] (times scale), mom [H * W, 4] or [H, W, 4];
    the variance of a colour channel is M2 * var_factor -> [H, W, 4] (rgb | propagated variance)"""
    color = np.ascontiguousarray(color, np.float32)
    albedo, guide, mom = (np.ascontiguousarray(x, np.float32) for x in (albedo, guide, mom))
    H, W = color.shape[:2]
    assert albedo.shape == (H, W, 4) and guide.shape == (H, W, 4) and mom.size == H * W * 4
    out = np.zeros((H, W, 4), np.float32)
    E = emul_variance()
    c4 = color.ctypes.data_as(_fp) if color.shape[2] == 4 else None
    c3 = color.ctypes.data_as(_fp) if color.shape[2] == 3 else None
    rc = E.emul_denoise2(W, H, c4, c3, scale, albedo.ctypes.data_as(_fp), guide.ctypes.data_as(_fp), mom.ctypes.data_as(_fp),
                         var_factor, out.ctypes.data_as(_fp), C.byref(p))
    if rc != 0:
        assert not check, E.emul_pick_error().decode()
        return None
    return out


def var_factor_context(scale, k):
    """what vcm_denoise2 multiplies M2 by: the colour is S * scale"""
    kf = np.float32(k)
    return float((np.float32(scale) * np.float32(scale)) * (kf / (kf - np.float32(1.0))))


def var_factor_mean(k):
    """what vcm_denoise_buffers2 multiplies M2 by: the colour is the mean"""
    return float(np.float32(1.0) / np.float32(float(k) * float(k - 1)))


class TrackedEmul:
    """an emulated renderer with variance tracking: what a tracked context does, iteration by iteration.  It has the
    interface smallvcm_amd.renderer.render_until() drives (RunIteration, mIterations, backend.noise_stats)."""

    def __init__(self, scene, algo, seed=1234, max_len=10, max_blocks=DEFAULT_MAX_BLOCKS):
        self.emul = dl.Emul(scene, algo, seed)
        self.prev, self.mom = new_images(self.emul.resx * self.emul.resy)
        self.max_len, self.max_blocks = max_len, max_blocks
        self.mIterations = 0
        self.backend = self

    def RunIteration(self, it):
        assert it == self.mIterations
        self.emul.run(1, self.max_len)
        self.mIterations += 1
        update(self.emul.framebuffer(), self.mIterations, self.prev, self.mom)

    def run(self, n):
        for _ in range(n):
            self.RunIteration(self.mIterations)
        return self

    def framebuffer(self):
        return self.emul.framebuffer()

    def noise_stats(self, threshold=np.inf, check=True):
        return stats(self.prev, self.mom, self.mIterations, threshold, self.max_blocks, check)

    def variance(self):
        return variance(self.mom, self.mIterations).reshape(self.emul.resy, self.emul.resx, 3)
