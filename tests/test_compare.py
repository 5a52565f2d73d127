"""The comparison with a reference image on the CPU: the host emulation of smallvcm_amd/csrc/vcm_compare.h
(tests/host_emul_compare: the library's pixel and window functions, run serially with the library's reduction tree) against
known answers and against a float64 numpy restatement (compare_lib.restate), the defaults, and every refusal -- through the
emulation and through the library's own host checks, which come before anything looks for a device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import compare_lib as cl
import denoise_lib as dl
from smallvcm_amd._abi import CompareParams, CompareStats
from smallvcm_amd.renderer import compare_params, load_library

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = cl.U
# Bounds of the pixel sums against the float64 restatement, from the roundings of a term (u = 2^-24 each, relative), every
# term being >= 0 so that the bound of a term is the bound of the sum; the binary64 additions add n * 2^-53, below 1e-9 u.
#   d^2:   d rounded once (the inputs are binary32 numbers, their difference is rounded once), squared: 2 u, the product
#          rounded: 3 u
#   rel:   the 3 u of d^2, ref * ref rounded, + epsilon rounded, the quotient rounded: 6 u; the binary32 epsilon is
#          0.01 (1 - 2.2e-8), within 0.4 u of the restatement's 0.01: 7 u
#   |d|:   1 u
MSE_BOUND, REL_BOUND, MAE_BOUND = 3 * U + 1e-12, 7 * U + 1e-12, 1 * U + 1e-12
# The SSIM map of the emulation against the float64 restatement: the binary32 cancellation in E[xx] - mu^2 against binary64.
# MEASURED on the inputs of this file (the seven synthetic shapes with and without planted non-finite pixels, and the
# 64 x 64 golden pair): the largest absolute difference is 1.16e-5 (67 x 45); the 64 x 64 pair gives 9.3e-6, 12 x 11 1.5e-6,
# 11 x 11 9.7e-8.  The tests assert four times the largest.
SSIM_MAP_MEASURED = 1.16e-5
SSIM_MAP_BOUND = 4 * SSIM_MAP_MEASURED
SHAPES = [(1, 1), (3, 2), (10, 64), (11, 11), (12, 11), (33, 9), (67, 45)]
WINDOWS = {(1, 1): 0, (3, 2): 0, (10, 64): 0, (11, 11): 1, (12, 11): 2, (33, 9): 0, (67, 45): 57 * 35}


def golden_pair():
    """64 x 64, scene 3 under path tracing: 16384 iterations of the sampler's reference against 1000 of the denoiser's"""
    ref = np.load(os.path.join(ROOT, "tests", "golden", "denoise_ref_s3_pt_64_1000.npy"))
    img = np.load(os.path.join(ROOT, "tests", "golden", "sampler_ref_s3_pt_64_16384.npy"))
    assert ref.shape == img.shape == (64, 64, 3)
    return img, ref


def close(a, b, rel):
    return (np.isnan(a) and np.isnan(b)) or a == b or abs(a - b) <= rel * abs(b)


def against_restatement(img, ref, **kw):
    st, m = cl.compare(img, ref, writeMap=1, **kw)
    rs, rm = cl.restate(img, ref, **{k: v for k, v in kw.items() if k != "max_blocks"})
    print("shape %s: ssim map |diff| max %.3e; mse %.3f u relMse %.3f u mae %.3f u" % (
        img.shape, np.abs(m[..., 3] - rm[..., 3]).max(), *[(st[k] / rs[k] - 1) / U if rs[k] else 0.0 for k in ("mse", "relMse", "mae")]))
    for k in ("pixels", "nonFinite", "above", "ssimWindows", "maxPixel"):
        assert st[k] == rs[k], (k, st[k], rs[k])
    assert close(st["mse"], rs["mse"], MSE_BOUND) and close(st["relMse"], rs["relMse"], REL_BOUND) and close(st["mae"], rs["mae"], MAE_BOUND), (st, rs)
    assert close(st["maxAbs"], rs["maxAbs"], U)
    assert close(st["psnr"], rs["psnr"], 0.0) or abs(st["psnr"] - rs["psnr"]) <= 10.0 / np.log(10.0) * 2 * MSE_BOUND
    assert np.abs(m[..., :3] - rm[..., :3]).max() <= REL_BOUND * max(1e-30, rm[..., :3].max())
    assert np.abs(m[..., 3] - rm[..., 3]).max() <= SSIM_MAP_BOUND
    assert close(st["ssim"], rs["ssim"], 0.0) or abs(st["ssim"] - rs["ssim"]) <= SSIM_MAP_BOUND
    return st, m


# ---------------- the defaults and the refusals ----------------
def test_defaults_the_ctypes_mirror_and_the_weight_table():
    src = open(os.path.join(ROOT, "include", "smallvcm_amd.h")).read()
    for name, mirror in (("vcm_compare_params", CompareParams), ("vcm_compare_stats", CompareStats)):
        body = re.search(r"typedef struct %s\s*\{(.*?)\} %s;" % (name, name), src, re.S).group(1)
        fields = [f.strip() for decl in body.split(";") for f in re.sub(r"^\s*(long long|int|float|double)\s", "", decl.strip()).split(",") if f.strip()]
        assert fields == [n for n, _ in mirror._fields_], name
    assert C.sizeof(CompareParams) == 20 and C.sizeof(CompareStats) == 96
    p, q = compare_params(), cl.params()
    assert bytes(p) == bytes(q)
    assert p.relEpsilon == np.float32(0.01) and p.peak == 1.0 and p.threshold == np.inf and p.ssim == 1 and p.writeMap == 0
    with pytest.raises(TypeError):
        compare_params(nonsense=1)
    # the table: normalised in binary64, rounded once
    assert cl.weights().tobytes() == cl.weights64().astype(np.float32).tobytes()
    assert abs(float(cl.weights().astype(np.float64).sum()) - 1.0) < 11 * U


BAD = [dict(relEpsilon=0.0), dict(relEpsilon=-0.01), dict(relEpsilon=np.nan), dict(relEpsilon=np.inf), dict(peak=0.0), dict(peak=-1.0),
       dict(peak=np.nan), dict(peak=np.inf), dict(threshold=np.nan), dict(threshold=-np.inf), dict(ssim=2), dict(ssim=-1),
       dict(writeMap=2), dict(writeMap=-1)]
GOOD = [dict(), dict(threshold=np.inf), dict(threshold=0.0), dict(threshold=-1.0), dict(relEpsilon=1e-6, peak=16.0), dict(ssim=0)]


def buffers_rc(p, img=0x10000, ref=0x20000, channels=(3, 3), scale=1.0, size=(4, 4), map_out=None, stats=True):
    """vcm_compare_buffers with pointers it must not touch: the refusals come before anything looks for a device"""
    L = load_library(require_gpu=False)
    st = CompareStats()
    rc = L.vcm_compare_buffers(0, size[0], size[1], img, channels[0], scale, ref, channels[1], C.byref(p) if p is not None else None, map_out,
                               C.byref(st) if stats else None, None)
    return rc, (L.vcm_last_error() or b"").decode()


def test_every_parameter_range_is_refused_by_the_emulation_and_by_the_library():
    img = np.ones((4, 4, 3), np.float32)
    for kw in BAD:
        p = cl.params(**kw)
        why = cl.check(p)
        assert why, kw
        assert cl.compare(img, img, check=False, **kw) is None, kw
        rc, err = buffers_rc(p)
        assert rc == -1 and err == "vcm_compare_buffers: " + why, (kw, err)
    for scale in (np.nan, np.inf, -np.inf):
        assert "scale" in cl.check(cl.params(), scale)
        rc, err = buffers_rc(cl.params(), scale=scale)
        assert rc == -1 and "scale" in err
    for kw in GOOD:
        assert cl.check(cl.params(**kw)) is None, kw
        assert cl.compare(img, img, **kw) is not None


def test_the_buffers_call_refuses_bad_images_and_the_context_calls_null():
    p = cl.params()
    for kw, word in ((dict(channels=(2, 3)), "channels"), (dict(channels=(3, 5)), "channels"), (dict(img=0), "NULL"), (dict(ref=0), "NULL"),
                     (dict(stats=False), "NULL"), (dict(size=(0, 4)), "size"), (dict(size=(4, -1)), "size"), (dict(size=(65536, 65536)), "size"),
                     (dict(img=0x10002), "aligned"), (dict(img=0x10004, channels=(4, 3)), "aligned"), (dict(ref=0x20008, channels=(3, 4)), "aligned"),
                     (dict(map_out=0x30004), "aligned")):
        rc, err = buffers_rc(p, **kw)
        assert rc == -1 and word in err, (kw, err)
    rc, err = buffers_rc(None)
    assert rc == -1 and "NULL" in err
    # a frame whose SSIM tiles exceed a grid's y dimension: refused by name with ssim on, taken with ssim off
    rc, err = buffers_rc(p, size=(11, 524291))
    assert rc == -1 and "524290 rows" in err and "524290 rows" in cl.check_size(524291, p)
    assert cl.check_size(524290, p) is None and cl.check_size(524291, cl.params(ssim=0)) is None
    pm = cl.params(writeMap=1)
    assert "writeMap without mapOutDev" in buffers_rc(pm)[1]
    assert "one of the inputs" in buffers_rc(pm, map_out=0x10000)[1] and "one of the inputs" in buffers_rc(pm, map_out=0x20000, channels=(3, 4))[1]
    E, fp = cl.emul(), C.POINTER(C.c_float)
    one, st = np.ones((4, 4, 4), np.float32), CompareStats()
    ptr = one.ctypes.data_as(fp)
    assert E.emul_compare(4, 4, ptr, 2, 1.0, ptr, 3, C.byref(p), 0, None, C.byref(st)) == -1 and b"channels" in E.emul_compare_error()
    assert E.emul_compare(4, 4, ptr, 4, 1.0, ptr, 4, C.byref(pm), 0, None, C.byref(st)) == -1 and b"writeMap" in E.emul_compare_error()
    assert E.emul_compare(4, 4, ptr, 4, 1.0, ptr, 4, C.byref(pm), 0, ptr, C.byref(st)) == -1 and b"inputs" in E.emul_compare_error()
    assert E.emul_compare(4, 4, None, 4, 1.0, ptr, 4, C.byref(p), 0, None, C.byref(st)) == -1 and E.emul_compare(0, 4, ptr, 4, 1.0, ptr, 4, C.byref(p), 0, None, C.byref(st)) == -1
    # a reference handed to vcm_set_reference must be finite
    ref = np.ones((3, 2, 3), np.float32)
    assert cl.reference_check(ref) is None
    for bad in (np.nan, np.inf, -np.inf):
        ref[1, 1, 2] = bad
        assert "non-finite" in cl.reference_check(ref)
    L = load_library(require_gpu=False)
    assert L.vcm_set_reference(None, ptr) == -1 and L.vcm_set_reference_device(None, None) == -1
    assert L.vcm_compare(None, 0, 1.0, C.byref(p), C.byref(st)) == -1 and b"NULL" in L.vcm_last_error()
    assert L.vcm_compare_map_device(None, None) == -1 and L.vcm_read_compare_map(None, ptr) == -1
    L.vcm_compare_defaults(None)
    hdr = open(os.path.join(ROOT, "include", "smallvcm_amd.h")).read()
    dbg = open(os.path.join(ROOT, "include", "smallvcm_amd_debug.h")).read()
    assert "vcm_debug_compare_max_blocks" in dbg and "vcm_debug_compare_max_blocks" not in hdr


# ---------------- known answers ----------------
def test_identical_images_give_zero_error_infinite_psnr_and_ssim_exactly_one():
    for W, H in SHAPES + [(64, 64)]:
        ref = golden_pair()[1] if (W, H) == (64, 64) else cl.sample_images(W, H, bad=False)[1]
        st, m = cl.compare(ref, ref, writeMap=1)
        assert st["mse"] == 0.0 and st["relMse"] == 0.0 and st["mae"] == 0.0 and st["maxAbs"] == 0.0 and st["psnr"] == np.inf
        assert st["maxPixel"] == 0 and st["above"] == 0 and st["nonFinite"] == 0 and st["pixels"] == W * H
        want = WINDOWS.get((W, H), 54 * 54)
        assert st["ssimWindows"] == want
        if want:
            assert st["ssim"] == 1.0 and (m[5:H - 5, 5:W - 5, 3] == 1.0).all()      # every window exactly 1
        else:
            assert np.isnan(st["ssim"])
        assert (m[..., :3] == 0).all()


def test_a_constant_offset_gives_its_square_and_its_magnitude():
    """ref + d: every |img - ref| is d within the rounding of the sum ref + d, half an ulp of the larger operand's binade:
    |ref + d| < 4 here, so |err| <= 2^-23 (ulp(x) = 2^-22 for 2 <= x < 4) per pixel; mae is within that of |d| and mse within
    2 |d| 2^-23 + 2^-46 of d^2, plus the 3 u of MSE_BOUND for squaring in binary32"""
    ref = cl.sample_images(67, 45, bad=False)[1]
    assert np.abs(ref).max() < 3.0
    for d in (0.25, -0.5, 0.1, -1e-3):
        img = (ref + np.float32(d)).astype(np.float32)
        st, _ = cl.compare(img, ref)
        e = 2.0 ** -23
        assert abs(st["mae"] - abs(d)) <= e + abs(d) * MAE_BOUND, (d, st)
        assert abs(st["mse"] - d * d) <= (2 * abs(d) * e + e * e) + d * d * MSE_BOUND, (d, st)
        assert abs(st["maxAbs"] - abs(d)) <= e
        assert abs(st["psnr"] - 10 * np.log10(1.0 / (d * d))) < 1e-3


def test_planted_outliers_are_found_and_equal_ones_resolve_to_the_lower_index():
    _, ref = cl.sample_images(67, 45, bad=False)
    img = ref.copy()
    img[30, 41, 1] += np.float32(8.0)
    for cap in (0, 2):           # one lane per pixel; a grid of two workgroups whose lanes stride
        st, m = cl.compare(img, ref, writeMap=1, threshold=1.0, max_blocks=cap)
        assert st["maxPixel"] == 30 * 67 + 41 and st["maxAbs"] == 8.0 and st["above"] == 1
        assert m[30, 41, 1] > 1.0 and np.count_nonzero(m[..., :3]) == 1
    # two equal outliers (exact differences: powers of two added to zeros), in pixels of different lanes, waves and workgroups
    ref0 = np.zeros_like(ref)
    for a, b in (((40, 3), (2, 60)), ((2, 60), (2, 61)), ((44, 66), (0, 0)), ((10, 10), (10, 9))):
        img = ref0.copy()
        img[a[0], a[1], 0] = 4.0
        img[b[0], b[1], 2] = -4.0
        for cap in (0, 2, 3):
            st, _ = cl.compare(img, ref0, threshold=0.5, max_blocks=cap)
            assert st["maxPixel"] == min(a[0] * 67 + a[1], b[0] * 67 + b[1]) and st["maxAbs"] == 4.0 and st["above"] == 2, (a, b, cap, st)


@pytest.mark.parametrize("where", ["img", "ref"])
def test_non_finite_pixels_are_counted_and_leave_every_other_figure_alone(where):
    """one NaN and one Inf pixel: nonFinite is exact, the sums equal those of the image without those pixels (their error
    made zero in a copy: an added zero changes no sum), and SSIM skips exactly the windows that hold them"""
    W, H = 67, 45
    img, ref = cl.sample_images(W, H, bad=False)
    clean, _ = cl.compare(img, ref, threshold=0.05, writeMap=1)
    pa, pb = (20, 30), (30, 50)      # pixels at least 10 from every border and more than 10 apart: 121 windows each
    bi, br = img.copy(), ref.copy()
    (bi if where == "img" else br)[pa[0], pa[1], 1] = np.nan
    (bi if where == "img" else br)[pb[0], pb[1], 2] = -np.inf
    st, m = cl.compare(bi, br, threshold=0.05, writeMap=1)
    assert st["nonFinite"] == 2 and st["pixels"] == W * H
    assert st["ssimWindows"] == clean["ssimWindows"] - 2 * 121
    zi = img.copy()
    zi[pa], zi[pb] = ref[pa], ref[pb]           # no error there
    z, zm = cl.compare(zi, ref, threshold=0.05, writeMap=1)
    n = W * H
    for k in ("mse", "relMse", "mae"):
        assert st[k] * (n - 2) == pytest.approx(z[k] * n, rel=1e-15), k   # the same sums over two pixels fewer
    assert st["maxAbs"] == z["maxAbs"] and st["maxPixel"] == z["maxPixel"] and st["above"] == z["above"]
    assert st["ssimWindows"] == z["ssimWindows"] - 2 * 121
    skipped = np.zeros((H, W), bool)
    for y, x in (pa, pb):
        skipped[y - 5:y + 6, x - 5:x + 6] = True
    assert (m[skipped, 3] == 0).all() and (m[pa] == 0).all() and (m[pb] == 0).all()
    inner = np.zeros((H, W), bool)
    inner[5:H - 5, 5:W - 5] = True
    keep = inner & ~skipped
    far = np.ones((H, W), bool)                 # windows that hold neither pixel nor the two made equal: untouched, bit for bit
    for y, x in (pa, pb):
        far[max(0, y - 5):y + 6, max(0, x - 5):x + 6] = False
    assert (m[keep & far, 3] == zm[keep & far, 3]).all() and (m[keep, 3] != 0).all()


# ---------------- the shapes against the float64 restatement ----------------
@pytest.mark.parametrize("shape", SHAPES)
def test_shapes_against_the_float64_restatement(shape):
    W, H = shape
    for bad in (False, True):
        for channels in (3, 4):
            img, ref = cl.sample_images(W, H, channels, bad=bad)
            st, _ = against_restatement(img, ref, threshold=0.05)
            if not bad:
                assert st["ssimWindows"] == WINDOWS[shape]
            assert np.isnan(st["ssim"]) == (st["ssimWindows"] == 0)
    img, ref = cl.sample_images(W, H, bad=True)
    against_restatement(img, ref, scale=0.75, relEpsilon=1e-3, peak=2.0, threshold=0.2, max_blocks=2)
    st, m = cl.compare(img, ref, ssim=0, writeMap=1)
    assert st["ssimWindows"] == 0 and np.isnan(st["ssim"]) and (m[..., 3] == 0).all()


def test_the_golden_pair_and_rel_mse_of_the_tests():
    img, ref = golden_pair()
    st, _ = against_restatement(img, ref)
    rs, _ = cl.restate(img, ref)
    want = dl.rel_mse(img, ref)
    # The 1e-12 line checks the YARDSTICK, not the code under test: the float64 restatement is rel_mse() of the tests.  The code
    # under test, the library's arithmetic in binary32 terms, is held to rel_mse() by the line after it, within the 7 u that
    # the roundings of one term allow (REL_BOUND above); binary32 terms cannot meet 1e-12.
    assert abs(rs["relMse"] - want) <= 1e-12 * want
    assert abs(st["relMse"] - want) <= REL_BOUND * want
    assert st["ssimWindows"] == 54 * 54 and 0.9 < st["ssim"] < 1.0 and 40.0 < st["psnr"] < 50.0


# ---------------- repeatability ----------------
def test_two_runs_give_the_same_bits():
    img, ref = cl.sample_images(67, 45)
    a, am = cl.compare(img, ref, writeMap=1, threshold=0.05)
    b, bm = cl.compare(img.copy(), ref.copy(), writeMap=1, threshold=0.05)
    assert cl.same_stats(a, b) and am.tobytes() == bm.tobytes()
    c, _ = cl.compare(img, ref, threshold=0.05, max_blocks=2)     # another grid is another tree: the counts and the maximum stay
    for k in ("pixels", "nonFinite", "above", "ssimWindows", "maxPixel", "maxAbs", "ssim"):
        assert a[k] == c[k]


# ---------------- host sanitizers ----------------
def test_the_emulation_runs_clean_under_the_host_sanitizers():
    """tests/host_emul_compare/sanitize_compare: every function of vcm_compare.h over the shapes at which the indexing
    changes, in a stand-alone program built with -fsanitize=address,undefined (CPU only)"""
    subprocess.run(["make", "-C", cl.EMUL_DIR, "sanitize_compare"], check=True, stdout=subprocess.DEVNULL)
    r = subprocess.run([os.path.join(cl.EMUL_DIR, "sanitize_compare")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.stdout[-300:], r.stderr[-1500:])
