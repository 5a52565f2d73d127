"""The display transform on the CPU: the functions of smallvcm_amd/csrc/vcm_display.h compiled for the host
(tests/host_emul_display) against float64 numpy restatements written from the definitions, the invariants of the bloom and
of the dither, and the library's argument checks.  tests/test_gpu_display.py holds the GPU to these bits."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import display_lib as dsp
from smallvcm_amd._abi import DisplayParams, DisplayStats
from smallvcm_amd.renderer import display_params, load_library

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HALF_BIN = dsp.WIDEST_BIN / 2.0   # 0.085 EV: a pixel's log2 luminance is at most this far from its bin's centre
CURVE_NAMES = ["clamp", "reinhard", "aces", "hable"]


def grey(x):
    x = np.asarray(x, np.float32)
    return np.stack([x, x, x], axis=-1)


# ---------------- the histogram ----------------
def histogram_inputs():
    rng = np.random.default_rng(11)
    n = 5000
    Y = np.exp2(rng.uniform(-18.0, 10.0, n)).astype(np.float32)
    img = grey(Y) * rng.uniform(0.5, 1.5, (n, 3)).astype(np.float32)
    img[10:14] = 0.0                       # zeros
    img[20:23] = -1.5                      # negatives: counted as zero
    img[30, 1] = np.nan
    img[31, 0] = np.inf
    img[40:45] = np.float32(2.0 ** -23)    # below 2^-20: bin 0 and clampedLow
    img[45] = np.float32(1e-41)            # a subnormal
    img[50:57] = np.float32(2.0 ** 13)     # above 2^12: bin 255 and clampedHigh
    img[57] = np.float32(4096.0)           # 2^12 itself is the first luminance past the last bin (weights sum to 1 +- 1 ulp)
    return img


def test_the_emulated_histogram_equals_the_bit_pattern_histogram():
    img = histogram_inputs()
    got = dsp.histogram(img)
    want = dsp.histogram_bits(dsp.luminance32(img))
    assert np.array_equal(got[:dsp.BINS], want["bins"])
    assert int(got[dsp.ZERO]) == want["zero"] == 7
    assert int(got[dsp.NONFINITE]) == want["nonFinite"] == 2
    assert int(got[dsp.CLAMPED_LOW]) == want["clampedLow"] == 6
    assert int(got[dsp.CLAMPED_HIGH]) == want["clampedHigh"] >= 7
    assert int(got[:dsp.BINS].sum()) + 9 == img.shape[0]
    assert (got[1:dsp.BINS - 1] > 0).sum() > 200   # the random part spreads over 28 octaves of bins
    # eight bins per octave: the luminances 2^o (1 + m / 8) open the bins 8 (o + 20) + m
    edges = np.array([2.0 ** o * (1.0 + m / 8.0) for o in (-20, -3, 0, 11) for m in range(8)], np.float32)
    h = dsp.histogram(grey(edges) * np.float32(1.0))
    Yb = dsp.luminance32(grey(edges))
    assert np.array_equal(h[:dsp.BINS], dsp.histogram_bits(Yb)["bins"])
    # scale enters before the luminance
    assert np.array_equal(dsp.histogram(img, 0.25)[:dsp.BINS], dsp.histogram_bits(dsp.luminance32(img * np.float32(0.25)))["bins"])


# ---------------- auto-exposure against float64 ----------------
def exposure_image(kind):
    rng = np.random.default_rng(5)
    n = 64 * 48
    if kind == "constant":
        return np.full((n, 3), 0.37, np.float32)
    if kind == "loguniform":
        return (grey(np.exp2(rng.uniform(-18.0, 10.0, n))) * rng.uniform(0.8, 1.2, (n, 3))).astype(np.float32)
    img = grey(0.05 * np.exp2(rng.normal(0.0, 0.5, n))).astype(np.float32)   # a dim room ...
    lamp = rng.choice(n, n * 4 // 100, replace=False)
    img[lamp] = grey(50.0 * np.exp2(rng.normal(0.0, 0.2, lamp.size))).astype(np.float32)   # ... and a lamp on 4 % of it
    return img


def emulated_ev(img, **kw):
    p = dsp.params(autoExposure=1, **kw)
    st = dsp.exposure(dsp.histogram(img), p)
    return st, p


@pytest.mark.parametrize("kind", ["constant", "loguniform", "bimodal"])
def test_auto_ev_agrees_with_the_float64_rank_rule(kind):
    """the bins' centres stand for the pixels' own log2 luminance: at most half the widest bin off per pixel, so at most
    that for the weighted mean (the weights are the same rank overlaps), plus 1e-4 for the fp32 luminance"""
    img = exposure_image(kind)
    Y64 = img.astype(np.float64) @ np.array([0.2126, 0.7152, 0.0722])
    st, p = emulated_ev(img)
    want = dsp.auto_ev64(Y64, p.key, p.lowPercentile, p.highPercentile, p.minEV, p.maxEV)
    print(kind, "autoEV", st["autoEV"], "float64", want)
    assert abs(st["autoEV"] - want) <= HALF_BIN + 1e-4
    assert st["counted"] == img.shape[0] and st["zero"] == st["nonFinite"] == 0
    assert st["multiplier"] == float(np.float32(np.exp2(st["autoEV"])))
    assert abs(st["logAvgLuminance"] - (np.log2(p.key) - st["autoEV"])) < 1e-12
    if kind == "bimodal":   # without the trim the lamp pulls the exposure down by more than the bins can blur
        full, pf = emulated_ev(img, lowPercentile=0.0, highPercentile=1.0)
        want_full = dsp.auto_ev64(Y64, pf.key, 0.0, 1.0, pf.minEV, pf.maxEV)
        assert abs(full["autoEV"] - want_full) <= HALF_BIN + 1e-4
        assert st["autoEV"] - full["autoEV"] > HALF_BIN and want - want_full > HALF_BIN


def test_auto_ev_edge_cases():
    p = dsp.params(autoExposure=1)
    empty = dsp.exposure(np.zeros(dsp.COUNTERS, np.uint64), p)
    assert empty["autoEV"] == 0.0 and empty["multiplier"] == 1.0 and empty["counted"] == 0
    dark = np.full((100, 3), 1e-9, np.float32)
    st, _ = emulated_ev(dark, maxEV=3.0, exposureEV=1.0)
    assert st["autoEV"] == 3.0 and st["multiplier"] == 16.0 and st["clampedLow"] == 100   # clamped to maxEV, then + exposureEV
    st, _ = emulated_ev(np.full((100, 3), 1e6, np.float32), minEV=-2.0)
    assert st["autoEV"] == -2.0 and st["clampedHigh"] == 100
    off = dsp.exposure(dsp.histogram(dark), dsp.params(exposureEV=-1.0))   # autoExposure off: the manual stops alone
    assert off["autoEV"] == 0.0 and off["multiplier"] == 0.5


# ---------------- the curves ----------------
X = np.concatenate([[0.0], np.exp2(np.linspace(-12.0, 12.0, 4096))]).astype(np.float32)


@pytest.mark.parametrize("name", CURVE_NAMES)
def test_curve_properties_and_float64_formula(name):
    y = dsp.curve(grey(X), name, 4.0)
    assert y.dtype == np.float32 and np.array_equal(y[:, 0], y[:, 1]) and np.array_equal(y[:, 0], y[:, 2])
    y = y[:, 0]
    assert y[0] == 0.0
    assert (np.diff(y) >= 0).all()
    assert y.min() >= 0.0 and y.max() <= 1.0 and y.max() == 1.0
    want = dsp.curve64(X.astype(np.float64), name, 4.0)
    err = np.abs(y.astype(np.float64) - want)
    print(name, "max relative error", (err / np.maximum(want, 1e-300)).max(), "max absolute", err.max())
    assert (err <= 1e-5 * want + (1e-6 if name == "hable" else 0.0)).all()


def test_reinhard_reaches_one_at_the_white_point():
    for W in (1.0, 4.0, 7.5):
        y = dsp.curve(grey(np.array([W], np.float32)), "reinhard", W)
        assert abs(float(y[0, 0]) - 1.0) <= 1e-6
        below = dsp.curve(grey(np.array([0.9 * W], np.float32)), "reinhard", W)
        assert below[0, 0] < 1.0


def test_curves_take_bad_pixels_as_the_old_encoding_does():
    """NaN and negative channels give 0, +Inf gives 1, under every curve"""
    bad = np.array([[np.nan, -1.0, np.inf]], np.float32)
    assert np.array_equal(dsp.curve(bad, "clamp"), np.array([[0.0, 0.0, 1.0]], np.float32))
    for name in CURVE_NAMES:
        y = dsp.curve(grey(np.array([np.nan, -3.0, np.inf], np.float32)), name)
        assert np.array_equal(y[:, 0], np.array([0.0, 0.0, 1.0], np.float32)), name


def test_transfer_curves():
    c = np.linspace(0.0, 1.0, 2001).astype(np.float32)
    s = dsp.transfer(c, "srgb")
    assert np.abs(s.astype(np.float64) - dsp.srgb64(c.astype(np.float64))).max() <= 1e-6
    assert s[0] == 0.0 and abs(float(s[-1]) - 1.0) <= 1e-6 and (np.diff(s) >= 0).all()
    knee = np.float32(0.0031308)
    pair = dsp.transfer(np.array([knee, np.nextafter(knee, np.float32(1.0))], np.float32), "srgb")
    assert abs(float(pair[1]) - float(pair[0])) <= 1e-6          # the two branches meet
    assert abs(float(pair[0]) - 12.92 * 0.0031308) <= 1e-7
    g = dsp.transfer(c, "gamma", 2.2)
    assert np.abs(g.astype(np.float64) - c.astype(np.float64) ** (1.0 / 2.2)).max() <= 1e-6
    # the curve then the transfer = the whole of steps 3 and 4
    lin = grey(X)
    both = dsp.curve(lin, "aces", 4.0, "srgb")
    assert np.array_equal(both, dsp.transfer(dsp.curve(lin, "aces", 4.0), "srgb"))


# ---------------- bloom ----------------
SIZES = [(1, 1), (2, 1), (3, 2), (5, 7), (20, 14), (67, 45)]   # W x H


def levels_to_one(W, H):
    n = 0
    while W > 1 or H > 1:
        W, H, n = max(1, (W + 1) // 2), max(1, (H + 1) // 2), n + 1
    return max(1, n)


@pytest.mark.parametrize("size", SIZES)
def test_bloom_matches_the_float64_restatement(size):
    """all weights are non-negative and an output sums fewer than a hundred terms per stage: 1e-5 relative"""
    W, H = size
    rng = np.random.default_rng(W * 100 + H)
    img = (rng.gamma(2.0, 0.5, (H, W, 3)) * np.exp2(rng.uniform(-4.0, 6.0, (H, W, 1)))).astype(np.float32)
    for levels in sorted({1, 3, levels_to_one(W, H)}):
        for s in (0.35, 1.0):
            got = dsp.bloom(img, s, levels)
            want = dsp.bloom64(img, s, levels)
            assert want.min() > 0
            assert np.allclose(got, want, rtol=1e-5, atol=0.0), (size, levels, s, np.abs(got / want - 1).max())
    assert np.array_equal(dsp.bloom(img, 0.0, 3), img)   # strength 0: the exposed image itself
    assert np.array_equal(dsp.bloom(img, 0.0, 3, mult=2.0), img * np.float32(2.0))
    assert np.allclose(dsp.bloom(img[..., [0, 1, 2, 2]], 0.5, 2), dsp.bloom(img, 0.5, 2), rtol=0, atol=0)   # four floats per pixel


def test_bloom_keeps_a_constant_image_constant():
    for (W, H) in SIZES:
        img = np.full((H, W, 3), 3.7, np.float32)
        for levels in (1, 3, levels_to_one(W, H)):
            out = dsp.bloom(img, 0.8, levels)
            assert np.abs(out / np.float32(3.7) - 1.0).max() <= 1e-6, (W, H, levels)


def test_bloom_keeps_the_sum_of_an_impulse_away_from_the_border():
    """64 x 56, two levels, the impulse at (32, 28): on the emulation its footprint spans -15 .. +18 pixels on either axis
    (with three levels -39 .. +38, which wants an image the test need not pay for), so the outer ring of 8 pixels stays
    exactly zero, no clamped coordinate sees it, and the sum is kept"""
    W, H, levels = 64, 56, 2
    img = np.zeros((H, W, 3), np.float32)
    img[28, 32] = (900.0, 500.0, 100.0)
    out = dsp.bloom(img, 1.0, levels)
    ring = out.copy()
    ring[8:-8, 8:-8] = 0.0
    assert ring.max() == 0.0 and ring.min() == 0.0
    ys, xs = np.nonzero(out[..., 0])
    assert (ys.min(), ys.max(), xs.min(), xs.max()) == (28 - 15, 28 + 18, 32 - 15, 32 + 18) and out.min() >= 0.0
    assert np.abs(out.astype(np.float64).sum(axis=(0, 1)) / np.array([900.0, 500.0, 100.0]) - 1.0).max() <= 1e-5
    mixed = dsp.bloom(img, 0.25, levels)   # (1 - s) E + s B keeps it as well
    assert np.abs(mixed.astype(np.float64).sum(axis=(0, 1)) / np.array([900.0, 500.0, 100.0]) - 1.0).max() <= 1e-5
    assert mixed[28, 32, 0] > 0.75 * 900.0


def test_a_nan_pixel_passes_through_the_bloom_and_spoils_no_other():
    rng = np.random.default_rng(3)
    img = rng.uniform(0.1, 2.0, (14, 20, 3)).astype(np.float32)
    img[5, 7, 1] = np.nan
    img[9, 2, 0] = np.inf
    for levels in (1, 3, 5):
        out = dsp.bloom(img, 0.6, levels)
        bad = np.zeros((14, 20), bool)
        bad[5, 7] = bad[9, 2] = True
        assert np.isfinite(out[~bad]).all()
        assert out[5, 7].tobytes() == img[5, 7].tobytes() and out[9, 2].tobytes() == img[9, 2].tobytes()
        assert np.allclose(out[~bad], dsp.bloom64(img, 0.6, levels)[~bad], rtol=1e-5, atol=0.0)
    shown, st, _ = dsp.display(img, dsp.params(bloomStrength=0.6, bloomLevels=3, curve="aces"))
    assert np.isfinite(shown).all() and shown[5, 7, 1] == 0.0 and shown[9, 2, 0] == 1.0 and (shown[..., 3] == 1.0).all()


# ---------------- bytes ----------------
def test_without_dither_the_bytes_are_the_reference_truncation():
    rng = np.random.default_rng(9)
    v = rng.uniform(0.0, 1.0, (9, 13, 4)).astype(np.float32)
    v[0, 0, :3] = (0.0, 1.0, 0.5)
    want = np.minimum(255.0, np.maximum(0.0, v[..., :3] * np.float32(255.0))).astype(np.uint8)   # (unsigned char)min(255, max(0, v * 255))
    bgr = dsp.encode(v, dsp.IMAGE_BGR8)
    assert np.array_equal(bgr, want[::-1, :, ::-1])      # bottom-up, B G R
    rgba = dsp.encode(v, dsp.IMAGE_RGBA8)
    assert np.array_equal(rgba[..., :3], want) and (rgba[..., 3] == 255).all()
    assert dsp.encode(v, dsp.IMAGE_RGBE, check=False) is None and "RGBE" in dsp.emul().emul_display_error().decode()
    assert dsp.encode(v, 7, check=False) is None


DITHER_SEED = 1   # seeds 0 .. 7 were tried on the emulation: every one keeps all three channels inside the bound below


def test_dither_is_unbiased_stateless_stochastic_rounding():
    """a constant 100.3 / 255 on 64 x 64: a channel's 4096 bytes are 100 or 101 and their mean is within 0.05 = 7 sigma
    (sigma = sqrt(0.3 * 0.7 / 4096)) of 100.3"""
    v = np.zeros((64, 64, 4), np.float32)
    v[..., :3] = np.float32(100.3 / 255.0)
    plain = dsp.encode(v, dsp.IMAGE_RGBA8)
    assert (plain[..., :3] == 100).all()
    a = dsp.encode(v, dsp.IMAGE_RGBA8, 1, DITHER_SEED)
    assert set(np.unique(a[..., :3])) == {100, 101}
    for ch in range(3):
        mean = a[..., ch].astype(np.float64).mean()
        print("channel", ch, "mean byte", mean)
        assert abs(mean - 100.3) <= 0.05
    assert np.array_equal(a, dsp.encode(v, dsp.IMAGE_RGBA8, 1, DITHER_SEED))     # no state
    assert not np.array_equal(a, dsp.encode(v, dsp.IMAGE_RGBA8, 1, DITHER_SEED + 1))
    assert not np.array_equal(a[..., 0], a[..., 1])                                # the channels draw apart
    b = dsp.encode(v, dsp.IMAGE_BGR8, 1, DITHER_SEED)
    assert np.array_equal(b, a[::-1, :, 2::-1])                                     # one draw per (pixel, channel), whatever the layout
    ends = np.zeros((1, 2, 4), np.float32)
    ends[0, 1, :3] = 1.0
    e = dsp.encode(ends, dsp.IMAGE_RGBA8, 1, DITHER_SEED)
    assert (e[0, 0, :3] == 0).all() and (e[0, 1, :3] == 255).all()                  # 0 stays 0, 1 stays 255


# ---------------- the defaults and the refusals ----------------
def test_defaults_and_the_ctypes_mirror():
    src = open(os.path.join(ROOT, "include", "smallvcm_amd.h")).read()
    for name, mirror in (("vcm_display_params", DisplayParams), ("vcm_display_stats", DisplayStats)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), src, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        fields = [f.strip() for decl in body.split(";") for f in re.sub(r"^\s*(unsigned int|long long|int|float|double)\s", "", decl.strip()).split(",") if f.strip()]
        assert fields == [n for n, _ in mirror._fields_], name
    assert C.sizeof(DisplayParams) == 60 and C.sizeof(DisplayStats) == 72
    p = display_params()                   # the library's defaults: today's look
    q = dsp.params()
    assert bytes(p) == bytes(q)
    assert (p.curve, p.transfer, p.autoExposure, p.dither) == (0, 0, 0, 0) and p.gamma == np.float32(2.2)
    assert p.exposureEV == 0.0 and p.bloomStrength == 0.0 and 1 <= p.bloomLevels <= 8
    assert p.key == np.float32(0.18) and p.lowPercentile == np.float32(0.10) and p.highPercentile == np.float32(0.95)
    assert display_params(curve="aces", transfer="srgb").curve == 2
    with pytest.raises(TypeError):
        display_params(nonsense=1)


BAD = [dict(curve=-1), dict(curve=4), dict(whitePoint=0.0), dict(whitePoint=-1.0), dict(whitePoint=np.inf), dict(whitePoint=np.nan),
       dict(exposureEV=np.nan), dict(exposureEV=np.inf), dict(exposureEV=33.0), dict(exposureEV=-33.0),
       dict(autoExposure=2), dict(autoExposure=-1), dict(key=0.0), dict(key=-0.18), dict(key=np.nan), dict(key=np.inf),
       dict(lowPercentile=-0.1), dict(highPercentile=1.1), dict(lowPercentile=0.6, highPercentile=0.5), dict(lowPercentile=0.5, highPercentile=0.5),
       dict(lowPercentile=np.nan), dict(highPercentile=np.nan),
       dict(minEV=2.0, maxEV=1.0), dict(minEV=-40.0), dict(maxEV=40.0), dict(minEV=np.nan), dict(maxEV=np.nan), dict(minEV=-np.inf), dict(maxEV=np.inf),
       dict(transfer=-1), dict(transfer=2), dict(gamma=0.0), dict(gamma=-2.2), dict(gamma=np.nan), dict(gamma=np.inf),
       dict(bloomStrength=-0.1), dict(bloomStrength=1.1), dict(bloomStrength=np.nan), dict(bloomLevels=0), dict(bloomLevels=9),
       dict(dither=2), dict(dither=-1)]
GOOD = [dict(), dict(curve=3, transfer=1, autoExposure=1, dither=1, ditherSeed=0xffffffff), dict(lowPercentile=0.0, highPercentile=1.0),
        dict(minEV=-32.0, maxEV=32.0), dict(minEV=1.0, maxEV=1.0), dict(bloomStrength=1.0, bloomLevels=8), dict(bloomStrength=0.0, bloomLevels=1),
        dict(exposureEV=-32.0), dict(whitePoint=1e-3)]


def buffers_rc(p, color=0x10000, out=0x20000, channels=3, scale=1.0, size=(4, 4)):
    """vcm_display_buffers with pointers it must not touch: the refusals come before anything looks for a device"""
    L = load_library(require_gpu=False)
    rc = L.vcm_display_buffers(0, size[0], size[1], color, channels, scale, C.byref(p) if p is not None else None, out, None, None)
    return rc, (L.vcm_last_error() or b"").decode()


def test_every_parameter_range_is_refused_by_the_emulation_and_by_the_library():
    img = np.ones((4, 4, 3), np.float32)
    for kw in BAD:
        p = dsp.params(**kw)
        why = dsp.check(p)
        assert why, kw
        assert dsp.display(img, p, check=False) is None, kw
        rc, err = buffers_rc(p)
        assert rc == -1 and err == "vcm_display_buffers: " + why, (kw, err)
    for kw in GOOD:
        assert dsp.check(dsp.params(**kw)) is None, kw
        assert dsp.display(img, dsp.params(**kw)) is not None


def test_the_buffers_call_refuses_bad_images():
    p = dsp.params()
    for kw, word in ((dict(channels=2), "channels"), (dict(channels=5), "channels"), (dict(channels=1), "channels"), (dict(out=0x10000), "input"),
                     (dict(color=0), "NULL"), (dict(out=0), "NULL"), (dict(size=(0, 4)), "size"), (dict(size=(4, -1)), "size"),
                     (dict(size=(65536, 65536)), "size"), (dict(out=0x20004), "aligned"), (dict(color=0x10002), "aligned"),
                     (dict(scale=float("nan")), "scale"), (dict(scale=float("inf")), "scale")):
        rc, err = buffers_rc(p, **kw)
        assert rc == -1 and word in err, (kw, err)
    rc, err = buffers_rc(None)
    assert rc == -1 and "params" in err
    img = np.ones((4, 4, 3), np.float32)
    E = dsp.emul()
    fp = C.POINTER(C.c_float)
    for ch in (1, 2, 5):
        assert E.emul_display(4, 4, img.ctypes.data_as(fp), ch, 1.0, C.byref(p), np.zeros((4, 4, 4), np.float32).ctypes.data_as(fp), None, None) == -1
    four = np.ones((4, 4, 4), np.float32)
    assert E.emul_display(4, 4, four.ctypes.data_as(fp), 4, 1.0, C.byref(p), four.ctypes.data_as(fp), None, None) == -1   # outDev == colorDev


def test_the_context_calls_refuse_null_and_the_debug_entry_points_are_debug_only():
    L = load_library(require_gpu=False)
    p = dsp.params()
    st = DisplayStats()
    assert L.vcm_display(None, 0, 1.0, C.byref(p)) == -1
    assert L.vcm_display_device(None, None) == -1 and L.vcm_read_display(None, None) == -1
    assert L.vcm_read_display_image(None, 0, None) == -1 and L.vcm_get_display_stats(None, C.byref(st)) == -1
    hdr = open(os.path.join(ROOT, "include", "smallvcm_amd.h")).read()
    dbg = open(os.path.join(ROOT, "include", "smallvcm_amd_debug.h")).read()
    for n in ("vcm_debug_display_max_blocks", "vcm_debug_read_display_histogram"):
        assert n in dbg and n not in hdr
    L.vcm_debug_display_max_blocks(2)
    L.vcm_debug_display_max_blocks(0)
    assert L.vcm_debug_read_display_histogram(None) == -1


# ---------------- host sanitizers ----------------
def test_the_flag_parsing_the_bmp_writer_and_the_exposure_run_clean_under_the_host_sanitizers(tmp_path):
    """tests/host_emul_display/sanitize_display: vcm_render's display flags, the BMP file and the host functions of
    vcm_display.h in a stand-alone program built with -fsanitize=address,undefined (CPU only)"""
    import subprocess
    subprocess.run(["make", "-C", dsp.EMUL_DIR, "sanitize_display"], check=True, stdout=subprocess.DEVNULL)
    r = subprocess.run([os.path.join(dsp.EMUL_DIR, "sanitize_display"), str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.stdout[-300:], r.stderr[-1500:])
    assert not list(tmp_path.iterdir())   # it removes the file it wrote
