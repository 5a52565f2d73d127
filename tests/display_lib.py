"""The display transform for the tests (test infrastructure): the ctypes binding of
tests/host_emul_display/libemul_display.so, built on demand, and float64 numpy restatements written from the definitions
(include/smallvcm_amd.h "the display transform"), not from smallvcm_amd/csrc/vcm_display.h."""
import ctypes as C
import os
import subprocess

import numpy as np

from smallvcm_amd._abi import CURVES, DisplayParams, DisplayStats, IMAGE_BGR8, IMAGE_RGBA8, IMAGE_RGBE, TRANSFERS  # noqa: F401

HERE = os.path.dirname(os.path.abspath(__file__))
EMUL_DIR = os.path.join(HERE, "host_emul_display")
BINS = 256
COUNTERS = 264      # VCM_DISP_COUNTERS
ZERO, NONFINITE, CLAMPED_LOW, CLAMPED_HIGH, CLIPPED = 256, 257, 258, 259, 260
BLOCK = 256         # VCM_DISP_BLOCK
WIDEST_BIN = float(np.log2(9.0 / 8.0))   # octaves: the first of an octave's eight bins
_fp = C.POINTER(C.c_float)
_up = C.POINTER(C.c_ulonglong)
_E = None


def emul():
    """build (make: a no-op when up to date) and load the display host emulation"""
    global _E
    if _E is None:
        subprocess.run(["make", "-C", EMUL_DIR], check=True, stdout=subprocess.DEVNULL)
        E = C.CDLL(os.path.join(EMUL_DIR, "libemul_display.so"))
        E.emul_display_error.restype = C.c_char_p
        E.emul_display_defaults.argtypes = [C.POINTER(DisplayParams)]
        E.emul_display_defaults.restype = None
        E.emul_display_check.argtypes = [C.POINTER(DisplayParams)]
        E.emul_display_histogram.argtypes = [C.c_longlong, _fp, C.c_int, C.c_float, _up]
        E.emul_display_histogram.restype = None
        E.emul_display_exposure.argtypes = [_up, C.POINTER(DisplayParams), C.POINTER(DisplayStats)]
        E.emul_display_exposure.restype = None
        E.emul_display.argtypes = [C.c_int, C.c_int, _fp, C.c_int, C.c_float, C.POINTER(DisplayParams), _fp, C.POINTER(DisplayStats), _up]
        E.emul_display_bloom.argtypes = [C.c_int, C.c_int, _fp, C.c_int, C.c_float, C.c_float, C.c_int, _fp]
        E.emul_display_curve.argtypes = [C.c_longlong, _fp, C.c_int, C.c_float, C.c_int, C.c_float, C.c_int, _fp]
        E.emul_display_curve.restype = None
        E.emul_display_transfer.argtypes = [C.c_longlong, _fp, C.c_int, C.c_float, _fp]
        E.emul_display_transfer.restype = None
        E.emul_display_encode.argtypes = [C.c_int, C.c_int, _fp, C.c_int, C.c_int, C.c_uint, C.POINTER(C.c_ubyte)]
        _E = E
    return _E


def params(**kw):
    """the emulation's defaults (vcm_display_defaults) with some members replaced; needs no library of the product"""
    p = DisplayParams()
    emul().emul_display_defaults(C.byref(p))
    for k, v in kw.items():
        assert k in [n for n, _ in DisplayParams._fields_], k
        if k == "curve" and isinstance(v, str):
            v = CURVES[v]
        if k == "transfer" and isinstance(v, str):
            v = TRANSFERS[v]
        setattr(p, k, v)
    return p


def check(p):
    """None where the parameters pass, else the refusal's text"""
    E = emul()
    return None if E.emul_display_check(C.byref(p)) == 0 else E.emul_display_error().decode()


def histogram(img, scale=1.0):
    """the 264 counters of img ([..., 3] or [..., 4]) * scale"""
    img = np.ascontiguousarray(img, np.float32)
    out = np.zeros(COUNTERS, np.uint64)
    emul().emul_display_histogram(img.size // img.shape[-1], img.ctypes.data_as(_fp), img.shape[-1], scale, out.ctypes.data_as(_up))
    return out


def exposure(counters, p):
    """disp_auto_exposure on the counters -> the stats dict (clipped 0)"""
    counters = np.ascontiguousarray(counters, np.uint64)
    assert counters.size == COUNTERS
    st = DisplayStats()
    emul().emul_display_exposure(counters.ctypes.data_as(_up), C.byref(p), C.byref(st))
    return st.asdict()


def display(img, p, scale=1.0, check=True):
    """the emulated vcm_display_buffers: img [H, W, 3 | 4] -> (out [H, W, 4], stats dict, bins [256]); check=False: None
    where it is refused"""
    img = np.ascontiguousarray(img, np.float32)
    H, W, ch = img.shape
    out = np.zeros((H, W, 4), np.float32)
    st = DisplayStats()
    bins = np.zeros(BINS, np.uint64)
    E = emul()
    rc = E.emul_display(W, H, img.ctypes.data_as(_fp), ch, scale, C.byref(p), out.ctypes.data_as(_fp), C.byref(st), bins.ctypes.data_as(_up))
    if rc != 0:
        assert not check, E.emul_display_error().decode()
        return None
    return out, st.asdict(), bins


def bloom(img, strength, levels, mult=1.0):
    """steps 1 and 2 alone: img [H, W, 3 | 4] -> the linear image [H, W, 3] the curve would take"""
    img = np.ascontiguousarray(img, np.float32)
    H, W, ch = img.shape
    out = np.zeros((H, W, 3), np.float32)
    E = emul()
    rc = E.emul_display_bloom(W, H, img.ctypes.data_as(_fp), ch, mult, strength, levels, out.ctypes.data_as(_fp))
    assert rc == 0, E.emul_display_error().decode()
    return out


def curve(lin, curve_id, white_point=4.0, transfer=None, gamma=2.2):
    """step 3 (and step 4 with `transfer`) of linear pixels [..., 3] -> the same shape, fp32"""
    lin = np.ascontiguousarray(lin, np.float32)
    out = np.zeros_like(lin)
    c = CURVES[curve_id] if isinstance(curve_id, str) else curve_id
    t = 0 if transfer is None else (TRANSFERS[transfer] if isinstance(transfer, str) else transfer)
    emul().emul_display_curve(lin.size // 3, lin.ctypes.data_as(_fp), c, white_point, t, gamma, 0 if transfer is None else 1, out.ctypes.data_as(_fp))
    return out


def transfer(c, which, gamma=2.2):
    """step 4 of channels in [0, 1]"""
    c = np.ascontiguousarray(c, np.float32)
    out = np.zeros_like(c)
    emul().emul_display_transfer(c.size, c.ctypes.data_as(_fp), TRANSFERS[which] if isinstance(which, str) else which, gamma, out.ctypes.data_as(_fp))
    return out


def encode(img4, fmt, dither=0, seed=0, check=True):
    """the emulated vcm_read_display_image of a display image [H, W, 4] -> bytes [H, W, 3 | 4]"""
    img4 = np.ascontiguousarray(img4, np.float32)
    H, W, _ = img4.shape
    out = np.zeros((H, W, 3 if fmt == IMAGE_BGR8 else 4), np.uint8)
    E = emul()
    rc = E.emul_display_encode(W, H, img4.ctypes.data_as(_fp), fmt, dither, seed, out.ctypes.data_as(C.POINTER(C.c_ubyte)))
    if rc != 0:
        assert not check, E.emul_display_error().decode()
        return None
    return out


# ---------------- restatements ----------------
def luminance32(img):
    """Y = 0.2126 r + 0.7152 g + 0.0722 b in fp32, in that order"""
    img = np.asarray(img, np.float32)
    with np.errstate(all="ignore"):
        return (np.float32(0.2126) * img[..., 0] + np.float32(0.7152) * img[..., 1]) + np.float32(0.0722) * img[..., 2]


def histogram_bits(Y):
    """the counters from the bit pattern of the fp32 luminances Y, by numpy: {bins, zero, nonFinite, clampedLow, clampedHigh}"""
    Y = np.asarray(Y, np.float32).ravel()
    fin = np.isfinite(Y)
    pos = fin & (Y > 0)
    raw = (Y[pos].view(np.uint32) >> np.uint32(20)).astype(np.int64) - ((127 - 20) << 3)
    bins = np.bincount(np.clip(raw, 0, BINS - 1), minlength=BINS).astype(np.uint64)
    return {"bins": bins, "zero": int((fin & ~pos).sum()), "nonFinite": int((~fin).sum()),
            "clampedLow": int((raw < 0).sum()), "clampedHigh": int((raw > BINS - 1).sum())}


def auto_ev64(Y, key=0.18, low=0.10, high=0.95, min_ev=-16.0, max_ev=16.0):
    """float64 restatement of the exposure rule WITHOUT bins: the positive finite luminances' log2, sorted; the pixel of rank
    i occupies [i, i + 1) and weighs its overlap with [low N, high N); autoEV = clamp(log2 key - weighted mean)"""
    Y = np.asarray(Y, np.float64).ravel()
    Y = Y[np.isfinite(Y) & (Y > 0)]
    if Y.size == 0:
        return 0.0
    lg = np.sort(np.log2(Y))
    N = float(Y.size)
    i = np.arange(Y.size, dtype=np.float64)
    w = np.maximum(0.0, np.minimum(i + 1.0, high * N) - np.maximum(i, low * N))
    if w.sum() <= 0:
        return 0.0
    return float(np.clip(np.log2(key) - (w * lg).sum() / w.sum(), min_ev, max_ev))


def curve64(x, which, white_point=4.0):
    """float64 formulas of the four curves on grey pixels x (r = g = b = x, so the luminance is x), clamped to [0, 1]"""
    x = np.asarray(x, np.float64)
    if which == "clamp":
        y = x
    elif which == "reinhard":
        with np.errstate(all="ignore"):
            y = np.where(x > 0, x * (1.0 + x / white_point ** 2) / (1.0 + x), 0.0)
    elif which == "aces":
        y = x * (2.51 * x + 0.03) / (x * (2.43 * x + 0.59) + 0.14)
    else:
        A, B, Cc, D, E, F = 0.15, 0.5, 0.1, 0.2, 0.02, 0.3

        def h(v):
            return (v * (A * v + Cc * B) + D * E) / (v * (A * v + B) + D * F) - E / F
        y = h(2.0 * x) / h(11.2)
    return np.clip(y, 0.0, 1.0)


def srgb64(c):
    c = np.asarray(c, np.float64)
    return np.where(c <= 0.0031308, 12.92 * c, 1.055 * np.power(np.maximum(c, 0.0), 1.0 / 2.4) - 0.055)


def _clamped(a, idx, axis):
    return np.take(a, np.clip(idx, 0, a.shape[axis] - 1), axis=axis)


def _down64(a):
    H, W = a.shape[:2]
    h, w = max(1, (H + 1) // 2), max(1, (W + 1) // 2)
    ys, xs = 2 * np.arange(h), 2 * np.arange(w)
    r0, r1 = _clamped(a, ys, 0), _clamped(a, ys + 1, 0)
    return 0.25 * (_clamped(r0, xs, 1) + _clamped(r0, xs + 1, 1) + _clamped(r1, xs, 1) + _clamped(r1, xs + 1, 1))


def _blur64(a):
    k = np.array([1.0, 4.0, 6.0, 4.0, 1.0]) / 16.0
    for axis in (1, 0):
        i = np.arange(a.shape[axis])
        a = sum(k[j] * _clamped(a, i + j - 2, axis) for j in range(5))
    return a


def _up64(a, H, W):
    def axis_up(b, n, axis):
        s = (np.arange(n) + 0.5) / 2.0 - 0.5
        i0 = np.floor(s).astype(np.int64)
        f = s - i0
        shape = [1, 1, 1]
        shape[axis] = n
        f = f.reshape(shape)
        return (1.0 - f) * _clamped(b, i0, axis) + f * _clamped(b, i0 + 1, axis)
    return axis_up(axis_up(a, W, 1), H, 0)


def bloom64(img, strength, levels):
    """float64 restatement of step 2 on the exposed image E [H, W, 3]: level l = the 2 x 2 mean of level l - 1 blurred by the
    binomial (level 0 = E with non-finite pixels as 0), U_L = G_L, U_l = G_l + up(U_{l+1}), B = up(U_1) / L, and
    (1 - s) E + s B; a pixel with a non-finite channel stays what it was"""
    E = np.asarray(img, np.float64)[..., :3]
    if not strength > 0:
        return E.copy()
    bad = ~np.isfinite(E).all(axis=2)
    g = [np.where(bad[..., None], 0.0, E)]
    for _ in range(levels):
        g.append(_blur64(_down64(g[-1])))
    u = g[levels]
    for l in range(levels - 1, 0, -1):
        u = g[l] + _up64(u, g[l].shape[0], g[l].shape[1])
    B = _up64(u, E.shape[0], E.shape[1]) / levels
    with np.errstate(all="ignore"):
        out = (1.0 - strength) * E + strength * B
    out[bad] = E[bad]
    return out
