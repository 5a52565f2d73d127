"""The comparison with a reference image on the GPU: the kernels of smallvcm_amd/csrc/vcm_compare.hip against the host
emulation of the same functions (tests/host_emul_compare), bit for bit -- every field of the statistics and the map -- the
context calls on renders, their refusals, the Python wrappers and vcm_render's flags."""
import ctypes as C
import csv
import json
import os
import subprocess

import numpy as np
import pytest

import compare_lib as cl
import denoise_lib as dl
from smallvcm_amd._abi import ALGO_VCM, CompareStats
from smallvcm_amd.renderer import HipBackend, VertexCM, compare_params, compare_tensors, load_library

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VCM_RENDER = os.path.join(ROOT, "smallvcm_amd", "host", "vcm_render")
# W x H: fewer pixels than a wave; exactly one window; no window and a row that straddles the tile edge of the pixel kernel;
# a partial tile on both axes of the SSIM kernel (57 x 35 windows: 2 x 5 tiles); several workgroups per row and 16 x 63 tiles
SHAPES = [(3, 2), (11, 11), (33, 9), (67, 45), (512, 512)]


def backend(scene, algo=ALGO_VCM, seed=1234, **kw):
    return HipBackend(dl.desc5(scene), algo, 0.003, 0.75, seed, **kw)


def same_bits(a, b):
    return np.ascontiguousarray(a, np.float32).tobytes() == np.ascontiguousarray(b, np.float32).tobytes()


@pytest.fixture
def small_grid():
    """the pixel kernel's grid capped at 2 workgroups, so that a few hundred pixels reach the grid-stride path and the
    second level sums more than one partial per lane"""
    L = load_library()
    L.vcm_debug_compare_max_blocks(2)
    yield 2
    L.vcm_debug_compare_max_blocks(0)


def check_buffers(img, ref, cap=0, **kw):
    """vcm_compare_buffers on (img, ref) through compare_tensors = the emulation: every field, and the map"""
    import torch
    want, wmap = cl.compare(img, ref, max_blocks=cap, **kw)
    timg, tref = torch.from_numpy(img).cuda(), torch.from_numpy(ref).cuda()
    if kw.get("writeMap"):
        tmap = torch.full((img.shape[0], img.shape[1], 4), 7.0, dtype=torch.float32, device="cuda")
        got = compare_tensors(timg, tref, map_out=tmap, **{k: v for k, v in kw.items() if k != "writeMap"})
        assert same_bits(tmap.cpu().numpy(), wmap), (img.shape, kw, np.abs(tmap.cpu().numpy() - wmap).max())
    else:
        got = compare_tensors(timg, tref, **kw)
    assert cl.same_stats(got, want), (img.shape, ref.shape, kw, got, want)
    return got


# ---------------- vcm_compare_buffers = the emulation, bit for bit ----------------
@pytest.mark.parametrize("shape", SHAPES)
def test_buffers_equal_the_emulation(shape):
    W, H = shape
    seen = 0
    for ic in (3, 4):
        for rc in (3, 4):
            img, _ = cl.sample_images(W, H, ic)
            _, ref = cl.sample_images(W, H, rc)
            for ssim in (1, 0):
                for write_map in (1, 0):
                    st = check_buffers(img, ref, ssim=ssim, writeMap=write_map, threshold=0.05)
                    seen += st["nonFinite"]
                    assert st["pixels"] == W * H and (st["ssimWindows"] > 0) == (ssim == 1 and W >= 11 and H >= 11 and (W, H) != (11, 11))
    assert seen == (32 if W * H >= 6 else 0)           # the planted NaN and Inf, in every one of the sixteen calls
    img, ref = cl.sample_images(W, H, 3)
    check_buffers(img, ref, scale=0.75, relEpsilon=1e-3, peak=2.0, threshold=0.2, writeMap=1)


@pytest.mark.parametrize("shape", [(33, 9), (67, 45)])
def test_buffers_equal_the_emulation_on_a_grid_that_strides(shape, small_grid):
    W, H = shape
    for ic, rc in ((3, 4), (4, 3)):
        img, _ = cl.sample_images(W, H, ic)
        _, ref = cl.sample_images(W, H, rc)
        check_buffers(img, ref, cap=small_grid, writeMap=1, threshold=0.05)


def test_identical_images_and_repeatability():
    import torch
    img, ref = cl.sample_images(67, 45, 4, bad=False)
    st = check_buffers(ref, ref, writeMap=1)
    assert st["mse"] == 0.0 and st["psnr"] == np.inf and st["ssim"] == 1.0 and st["ssimWindows"] == 57 * 35
    timg, tref = torch.from_numpy(img).cuda(), torch.from_numpy(ref).cuda()
    m1, m2 = torch.zeros((45, 67, 4), device="cuda"), torch.zeros((45, 67, 4), device="cuda")
    a, b = compare_tensors(timg, tref, map_out=m1, threshold=0.05), compare_tensors(timg, tref, map_out=m2, threshold=0.05)
    assert cl.same_stats(a, b) and same_bits(m1.cpu().numpy(), m2.cpu().numpy())
    with pytest.raises(RuntimeError, match="peak"):
        compare_tensors(timg, tref, peak=0.0)
    with pytest.raises(ValueError):
        compare_tensors(timg[..., :2].contiguous(), tref)


# ---------------- a context ----------------
def ctx_stats(want, iterations):
    return dict(want, iterations=iterations)


def test_a_context_equals_the_buffers_call_and_the_emulation_and_leaves_the_framebuffer_alone():
    import torch
    W, H, its = 20, 14, 2
    sc = dl.box(1, W, H)
    mean = dl.Emul(sc, ALGO_VCM).run(its).mean()        # the emulation's own 2-iteration image
    b = backend(sc)
    try:
        for it in range(its):
            b.run_iteration(it, 0, 10)
        fb = b.framebuffer_sum()
        for ref in (mean, np.roll(mean, 1, axis=1)):
            b.set_reference(ref)
            for kw in (dict(), dict(writeMap=1, threshold=0.05), dict(ssim=0)):
                want, wmap = cl.compare(fb, dl.as4(ref), scale=1.0 / its, **kw)      # the context keeps its reference as float4
                got = b.compare(**kw)
                assert cl.same_stats(got, ctx_stats(want, its)), (kw, got, want)
                tens = compare_tensors(torch.from_numpy(fb).cuda(), torch.from_numpy(ref).cuda(), scale=1.0 / its,
                                       **{k: v for k, v in kw.items() if k != "writeMap"})
                assert cl.same_stats(tens, want), (kw, tens, want)
                if kw.get("writeMap"):
                    assert same_bits(b.compare_map(), wmap)
            assert same_bits(b.framebuffer_sum(), fb)                                 # the call leaves the framebuffer alone
        assert got["ssimWindows"] == 0 and got["pixels"] == W * H
        if same_bits(fb * np.float32(1.0 / its), mean):                               # the default mode is bit-exact
            b.set_reference(mean)
            assert b.compare()["mse"] == 0.0
        # the other sources: refused before the calls that make them, then the emulation fed the same image
        L, p, st = b.L, compare_params(), CompareStats()
        assert L.vcm_compare(b.ctx, 1, 1.0, C.byref(p), C.byref(st)) == -1 and b"vcm_denoise has not run" in L.vcm_last_error()
        assert L.vcm_compare(b.ctx, 2, 1.0, C.byref(p), C.byref(st)) == -1 and b"vcm_track_robust is off" in L.vcm_last_error()
        clean = b.denoise(1.0 / its)
        want, _ = cl.compare(dl.as4(clean), dl.as4(mean))
        assert cl.same_stats(b.compare("denoised"), ctx_stats(want, its))
        # the context's own image as the reference: the denoiser without a pass gives framebuffer * scale as a float4 image
        b.denoise(1.0 / its, passes=0)
        pv = C.c_void_p()
        assert L.vcm_denoised_device(b.ctx, C.byref(pv)) == 0
        b.set_reference_device(pv.value)
        for source in ("framebuffer", "denoised"):
            st0 = b.compare(source)
            assert st0["mse"] == 0.0 and st0["psnr"] == np.inf and st0["maxAbs"] == 0.0 and st0["nonFinite"] == 0
        b.set_reference(None)
        assert L.vcm_compare(b.ctx, 0, 1.0, C.byref(p), C.byref(st)) == -1 and b"no reference" in L.vcm_last_error()
    finally:
        b.close()


def test_the_robust_source_and_a_larger_frame():
    W, H, its = 67, 45, 4
    sc = dl.box(3, W, H)
    b = backend(sc)
    try:
        b.track_robust(3)
        for it in range(its):
            b.run_iteration(it, 0, 10)
        fb = b.framebuffer_sum()
        ref = fb * np.float32(1.0 / its)
        ref[10, 20] += np.float32(0.5)
        b.set_reference(ref)
        rob = b.robust()
        want, wmap = cl.compare(dl.as4(rob), dl.as4(ref), writeMap=1, threshold=0.05)
        assert cl.same_stats(b.compare("robust", writeMap=1, threshold=0.05), ctx_stats(want, its)) and same_bits(b.compare_map(), wmap)
        got = b.compare(threshold=1.0)
        assert got["maxPixel"] == 10 * W + 20 and got["maxAbs"] == pytest.approx(0.5, abs=1e-6) and got["ssimWindows"] == 57 * 35 and got["ssim"] < 1.0
        assert same_bits(b.framebuffer_sum(), fb)
    finally:
        b.close()


def test_refusals_of_the_context_calls():
    sc = dl.box(1, 20, 14)
    b = backend(sc)
    try:
        L, p, st, pv = b.L, compare_params(), CompareStats(), C.c_void_p()
        fp = C.POINTER(C.c_float)
        ref = np.full((14, 20, 3), 0.5, np.float32)
        b.run_iteration(0, 0, 10)
        assert L.vcm_compare(b.ctx, 0, 1.0, C.byref(p), C.byref(st)) == -1 and b"no reference" in L.vcm_last_error()
        bad = ref.copy()
        bad[3, 4, 1] = np.nan
        assert L.vcm_set_reference(b.ctx, bad.ctypes.data_as(fp)) == -1 and b"non-finite" in L.vcm_last_error()
        assert L.vcm_compare(b.ctx, 0, 1.0, C.byref(p), C.byref(st)) == -1            # a refused reference leaves none behind
        b.set_reference(ref)
        assert L.vcm_compare(b.ctx, 3, 1.0, C.byref(p), C.byref(st)) == -1 and b"unknown source" in L.vcm_last_error()
        assert L.vcm_compare(b.ctx, 0, float("inf"), C.byref(p), C.byref(st)) == -1 and b"scale" in L.vcm_last_error()
        assert L.vcm_compare(b.ctx, 0, 1.0, None, C.byref(st)) == -1 and L.vcm_compare(b.ctx, 0, 1.0, C.byref(p), None) == -1
        with pytest.raises(RuntimeError, match="relEpsilon"):
            b.compare(relEpsilon=0.0)
        assert L.vcm_compare_map_device(b.ctx, C.byref(pv)) == -1 and b"writeMap" in L.vcm_last_error()
        assert L.vcm_read_compare_map(b.ctx, np.zeros((14, 20, 4), np.float32).ctypes.data_as(fp)) == -1
        assert b.compare()["pixels"] == 280
        assert L.vcm_compare_map_device(b.ctx, C.byref(pv)) == -1                      # a compare without a map makes none
        b.compare(writeMap=1)
        assert b.compare_map_device() and b.compare_map().shape == (14, 20, 4)
        with pytest.raises(ValueError):
            b.set_reference(np.zeros((14, 21, 3), np.float32))
    finally:
        b.close()
    s = backend(sc, rank=1, world=2)
    try:
        for rc in (s.L.vcm_compare(s.ctx, 0, 1.0, C.byref(p), C.byref(st)), s.L.vcm_set_reference(s.ctx, ref.ctypes.data_as(fp)),
                   s.L.vcm_set_reference_device(s.ctx, None), s.L.vcm_read_compare_map(s.ctx, ref.ctypes.data_as(fp))):
            assert rc == -1 and b"reduce the frame and call vcm_compare_buffers" in s.L.vcm_last_error()
    finally:
        s.close()


def test_render_to_error_stops_at_the_first_look_at_or_below_the_target():
    sc = dl.box(1, 20, 14)
    mean = dl.Emul(sc, ALGO_VCM).run(2).mean()
    v = VertexCM(sc, VertexCM.kVcm, 0.003, 0.75, 1234)
    try:
        v.mMaxPathLength = 10
        looks = v.render_to_error(mean, 1e9, check_every=2, max_iterations=8)         # a loose target: the first look meets it
        assert len(looks) == 1 and v.mIterations == 2 and looks[0]["iterations"] == 2 and looks[0]["relMse"] <= 1e9
        looks = v.render_to_error(mean, 0.0, check_every=3, max_iterations=5)         # never met (other iterations): 3 and 5
        assert [k["iterations"] for k in looks] == [3, 5] and v.mIterations == 5 and looks[-1]["relMse"] > 0.0
    finally:
        v.close()


# ---------------- vcm_render ----------------
def test_vcm_render_compares_with_a_reference_file(tmp_path):
    W, H, its, seed = 31, 23, 3, 5
    base = [VCM_RENDER, "-s", "1", "-a", "vcm", "--res", str(W), str(H), "--seed", str(seed)]
    a, b2, log, emap = str(tmp_path / "a.pfm"), str(tmp_path / "b.pfm"), str(tmp_path / "c.csv"), str(tmp_path / "e.pfm")
    r = subprocess.run(base + ["-i", str(its), "-o", a], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "compare after" not in r.stdout, r.stderr[-500:]
    # the same seed and iteration count against its own file: every iteration checked, the last one is the file itself
    r = subprocess.run(base + ["-i", str(its), "-o", b2, "--reference", a, "--compare-every", "1", "--compare-log", log, "--error-map", emap],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-500:]
    assert open(a, "rb").read() == open(b2, "rb").read()                       # it writes what it wrote
    rows = list(csv.reader(open(log)))
    assert rows[0] == ["iteration", "relMSE", "MSE", "PSNR", "SSIM", "maxAbs", "nonFinite"] and [int(x[0]) for x in rows[1:]] == [1, 2, 3]
    assert float(rows[-1][2]) == 0.0 and float(rows[-1][1]) == 0.0 and rows[-1][3] == "inf" and float(rows[-1][4]) == 1.0 and rows[-1][6] == "0"
    assert float(rows[1][2]) > 0.0 and r.stdout.count("compare after") == 3
    raw = open(emap, "rb").read()
    assert raw.startswith(b"PF\n31 23\n-1\n") and not np.frombuffer(raw[len(b"PF\n31 23\n-1\n"):], np.float32).any()
    # the first row is what the library's own comparison of one iteration gives
    ref = np.frombuffer(open(a, "rb").read()[len(b"PF\n31 23\n-1\n"):], np.float32).reshape(H, W, 3)
    v = backend(dl.box(1, W, H), seed=seed)
    try:
        v.run_iteration(0, 0, 10)
        v.set_reference(ref)
        st = v.compare()
        assert float(rows[1][1]) == st["relMse"] and float(rows[1][2]) == st["mse"] and float(rows[1][4]) == st["ssim"]
    finally:
        v.close()
    # a loose target stops at the first check; --json carries the last check
    r = subprocess.run(base + ["--reference", a, "--error-target", "1e9", "--compare-every", "2", "--max-iterations", "9", "--compare-log", log, "--json"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-500:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["iterations"] == 2 and out["compare"]["iterations"] == 2 and out["compare"]["pixels"] == W * H and len(list(csv.reader(open(log)))) == 2
    # a target never met runs to --max-iterations, checked every 4 iterations and after the last
    r = subprocess.run(base + ["--reference", a, "--error-target", "0", "--max-iterations", "5", "--compare-log", log], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and [int(x[0]) for x in list(csv.reader(open(log)))[1:]] == [4, 5] and "5 iteration(s) used" in r.stdout
    # with --noise-target the run stops by the noise statistic and the error is looked at on the way and where it stops: a
    # target never met runs the three iterations of the file once each, so that the last look is the file itself
    r = subprocess.run(base + ["--reference", a, "--noise-target", "0", "--check-every", "2", "--max-iterations", str(its), "--compare-log", log, "--json"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-500:]
    out, rows = json.loads(r.stdout.strip().splitlines()[-1]), list(csv.reader(open(log)))
    assert [int(x[0]) for x in rows[1:]] == [2, 3] and float(rows[-1][2]) == 0.0 and float(rows[1][2]) > 0.0
    assert out["iterations"] == its and out["compare"]["iterations"] == its and out["compare"]["mse"] == 0.0
    # a loose noise target stops at the first look (two iterations): the error is that of the two-iteration image
    r = subprocess.run(base + ["--reference", a, "--noise-target", "1e9", "--check-every", "2", "--max-iterations", "9", "--compare-every", "5", "--json"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-500:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    v = backend(dl.box(1, W, H), seed=seed)
    try:
        v.run_iteration(0, 0, 10)
        v.run_iteration(1, 0, 10)
        v.set_reference(ref)
        st = v.compare()
        assert out["iterations"] == 2 and out["compare"]["iterations"] == 2 and out["compare"]["relMse"] == st["relMse"] and out["compare"]["mse"] == st["mse"]
    finally:
        v.close()
    # the refusals: another resolution, flags without --reference, several renderers, a robust estimate that cannot be resolved
    r = subprocess.run(base + ["-a", "pt", "--reference", a, "--robust", "3", "-i", "2"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and "at least 3 iterations" in r.stderr
    r = subprocess.run(base + ["--reference", a, "--error-target", "1", "--noise-target", "1"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and "do not combine" in r.stderr
    r = subprocess.run([VCM_RENDER, "-s", "1", "--res", "30", "23", "--reference", a], capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and "31 x 23" in r.stderr
    r = subprocess.run(base + ["--compare-every", "2"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and "--reference" in r.stderr
    r = subprocess.run(base + ["--reference", a, "--renderers", "2"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and "one renderer" in r.stderr
    r = subprocess.run(base + ["--reference", str(tmp_path / "missing.pfm")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and "--reference" in r.stderr


def test_vcm_render_compares_the_image_it_writes(tmp_path):
    W, H, its = 20, 14, 4
    base = [VCM_RENDER, "-s", "1", "-a", "pt", "--res", str(W), str(H), "--seed", "9", "-i", str(its), "--json"]
    for flags in (["--denoise"], ["--robust", "3"]):
        a = str(tmp_path / ("a%d.pfm" % len(flags)))
        assert subprocess.run(base + flags + ["-o", a], capture_output=True, text=True, timeout=300).returncode == 0
        r = subprocess.run(base + flags + ["--reference", a], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-500:]
        cmp_ = json.loads(r.stdout.strip().splitlines()[-1])["compare"]
        assert cmp_["mse"] == 0.0 and cmp_["psnr"] is None and cmp_["iterations"] == its, (flags, cmp_)
