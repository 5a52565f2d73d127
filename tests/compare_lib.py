"""The comparison with a reference image for the tests (test infrastructure): the ctypes binding of
tests/host_emul_compare/libemul_compare.so, built on demand, and a float64 numpy restatement written from the definitions
(include/smallvcm_amd.h "image comparison"), not from smallvcm_amd/csrc/vcm_compare.h."""
import ctypes as C
import os
import subprocess

import numpy as np

from smallvcm_amd._abi import CompareParams, CompareStats

HERE = os.path.dirname(os.path.abspath(__file__))
EMUL_DIR = os.path.join(HERE, "host_emul_compare")
BLOCK = 256          # VCM_CMP_BLOCK
RADIUS, TAPS = 5, 11
U = 2.0 ** -24       # the unit roundoff of binary32
_fp = C.POINTER(C.c_float)
_E = None


def emul():
    """build (make: a no-op when up to date) and load the compare host emulation"""
    global _E
    if _E is None:
        subprocess.run(["make", "-C", EMUL_DIR], check=True, stdout=subprocess.DEVNULL)
        E = C.CDLL(os.path.join(EMUL_DIR, "libemul_compare.so"))
        E.emul_compare_error.restype = C.c_char_p
        E.emul_compare_defaults.argtypes = [C.POINTER(CompareParams)]
        E.emul_compare_defaults.restype = None
        E.emul_compare_weights.argtypes = [_fp]
        E.emul_compare_weights.restype = None
        E.emul_compare_check.argtypes = [C.c_float, C.POINTER(CompareParams)]
        E.emul_compare_check_size.argtypes = [C.c_int, C.POINTER(CompareParams)]
        E.emul_compare_reference_check.argtypes = [C.c_longlong, _fp]
        E.emul_compare.argtypes = [C.c_int, C.c_int, _fp, C.c_int, C.c_float, _fp, C.c_int, C.POINTER(CompareParams), C.c_int, _fp,
                                   C.POINTER(CompareStats)]
        _E = E
    return _E


def params(**kw):
    """the emulation's defaults (vcm_compare_defaults) with some members replaced; needs no library of the product"""
    p = CompareParams()
    emul().emul_compare_defaults(C.byref(p))
    for k, v in kw.items():
        assert k in [n for n, _ in CompareParams._fields_], k
        setattr(p, k, v)
    return p


def check(p, scale=1.0):
    """None where scale and parameters pass, else the refusal's text"""
    E = emul()
    return None if E.emul_compare_check(scale, C.byref(p)) == 0 else E.emul_compare_error().decode()


def check_size(H, p):
    """None where a frame of H rows passes, else the refusal's text"""
    E = emul()
    return None if E.emul_compare_check_size(H, C.byref(p)) == 0 else E.emul_compare_error().decode()


def reference_check(rgb):
    """None where vcm_set_reference would take the image, else the refusal's text"""
    rgb = np.ascontiguousarray(rgb, np.float32)
    E = emul()
    return None if E.emul_compare_reference_check(rgb.size // 3, rgb.ctypes.data_as(_fp)) == 0 else E.emul_compare_error().decode()


def weights():
    """the library's table of the 11 one-dimensional window weights, binary32"""
    w = np.zeros(TAPS, np.float32)
    emul().emul_compare_weights(w.ctypes.data_as(_fp))
    return w


def compare(img, ref, scale=1.0, max_blocks=0, check=True, **kw):
    """the emulated vcm_compare_buffers: img, ref [H, W, 3 | 4] -> (stats dict, map [H, W, 4] or None); max_blocks caps the
    pixel kernel's grid (0: the default); check=False: None where it is refused"""
    img, ref = np.ascontiguousarray(img, np.float32), np.ascontiguousarray(ref, np.float32)
    H, W, ch = img.shape
    assert ref.shape[:2] == (H, W)
    p = params(**kw)
    out = np.zeros((H, W, 4), np.float32) if p.writeMap else None
    st = CompareStats()
    E = emul()
    rc = E.emul_compare(W, H, img.ctypes.data_as(_fp), ch, scale, ref.ctypes.data_as(_fp), ref.shape[2], C.byref(p), max_blocks,
                        out.ctypes.data_as(_fp) if out is not None else None, C.byref(st))
    if rc != 0:
        assert not check, E.emul_compare_error().decode()
        return None
    return st.asdict(), out


def same_stats(a, b):
    """every field of two stats dicts, bit for bit (NaN equals NaN)"""
    return a.keys() == b.keys() and all(np.float64(a[k]).tobytes() == np.float64(b[k]).tobytes() if isinstance(a[k], float) else a[k] == b[k] for k in a)


def sample_images(W, H, channels=3, seed=0, bad=True):
    """a smooth reference with highlights above 1 and a noisy copy of it, [H, W, channels] binary32; with `bad` and room for
    them a NaN in the image and an Inf in the reference at two different pixels"""
    rng = np.random.default_rng(1000 * W + H + seed)
    y, x = np.mgrid[0:H, 0:W]
    base = 0.45 + 0.4 * np.sin(0.37 * x + 0.11 * y)[..., None] * np.array([1.0, 0.8, 0.6]) + 0.25 * np.cos(0.23 * y)[..., None]
    ref = np.ones((H, W, channels), np.float32)
    ref[..., :3] = np.abs(base) * np.exp2(rng.uniform(-0.3, 0.5, (H, W, 1)))
    img = ref.copy()
    img[..., :3] = ref[..., :3] * rng.gamma(8.0, 1.0 / 8.0, (H, W, 3))
    if bad and W * H >= 6:
        img.reshape(-1, channels)[(W * H) // 3, 1] = np.nan
        ref.reshape(-1, channels)[(2 * W * H) // 3, 0] = np.inf
    return img.astype(np.float32), ref.astype(np.float32)


# ---------------- the restatement ----------------
def weights64():
    """exp(-(k - 5)^2 / (2 * 1.5^2)) over its sum, in binary64"""
    g = np.exp(-((np.arange(TAPS) - RADIUS) ** 2) / (2.0 * 1.5 * 1.5))
    return g / g.sum()


def _valid_conv(a, w, axis):
    n = a.shape[axis] - TAPS + 1
    return sum(w[k] * np.take(a, np.arange(k, k + n), axis=axis) for k in range(TAPS))


def restate(img, ref, scale=1.0, relEpsilon=0.01, peak=1.0, threshold=np.inf, ssim=1):
    """float64 restatement: (stats dict, map [H, W, 4] float64).  img * scale is the binary32 product (that is the image the
    definitions speak of); everything after it binary64.  The SSIM moments are separable 'valid' convolutions with the
    library's binary32 weight table."""
    img = (np.asarray(img, np.float32)[..., :3] * np.float32(scale)).astype(np.float64)
    ref = np.asarray(ref, np.float32)[..., :3].astype(np.float64)
    H, W, _ = img.shape
    fin = np.isfinite(img).all(axis=2) & np.isfinite(ref).all(axis=2)
    n = int(fin.sum())
    with np.errstate(all="ignore"):
        d = np.where(fin[..., None], img - ref, 0.0)
        rel = np.where(fin[..., None], d * d / (ref * ref + relEpsilon), 0.0)
    nan = float("nan")
    st = {"iterations": 0, "pixels": W * H, "nonFinite": W * H - n, "above": int((rel.max(axis=2) > threshold).sum())}
    absmax = np.where(fin, np.abs(d).max(axis=2), -1.0)
    st["maxPixel"] = int(np.argmax(absmax)) if n else -1        # argmax: the first of equals
    st["maxAbs"] = float(absmax.max()) if n else 0.0
    st["mse"] = float((d * d).sum() / (3 * n)) if n else nan
    st["relMse"] = float(rel.sum() / (3 * n)) if n else nan
    st["mae"] = float(np.abs(d).sum() / (3 * n)) if n else nan
    with np.errstate(all="ignore"):
        st["psnr"] = (float(10.0 * np.log10(peak * peak / st["mse"])) if st["mse"] > 0 else float("inf")) if n else nan
    out = np.zeros((H, W, 4))
    out[..., :3] = rel
    st["ssimWindows"], st["ssim"] = 0, nan
    if ssim and W >= TAPS and H >= TAPS:
        lum = np.array([0.212671, 0.715160, 0.072169])
        with np.errstate(all="ignore"):
            x = np.where(fin, np.clip(np.where(fin[..., None], img, 0.0) @ lum, 0.0, peak) / peak, np.nan)
            y = np.where(fin, np.clip(np.where(fin[..., None], ref, 0.0) @ lum, 0.0, peak) / peak, np.nan)
            w = weights().astype(np.float64)
            mom = [_valid_conv(_valid_conv(a, w, 1), w, 0) for a in (x, y, x * x, y * y, x * y)]
            mx, my, xx, yy, xy = mom
            C1, C2 = 0.01 ** 2, 0.03 ** 2
            s = ((2 * mx * my + C1) * (2 * (xy - mx * my) + C2)) / ((mx * mx + my * my + C1) * ((xx - mx * mx) + (yy - my * my) + C2))
        ok = np.isfinite(mx)
        st["ssimWindows"] = int(ok.sum())
        if ok.any():
            st["ssim"] = float(s[ok].mean())
        out[RADIUS:H - RADIUS, RADIUS:W - RADIUS, 3] = np.where(ok, s, 0.0)
    return st, out
