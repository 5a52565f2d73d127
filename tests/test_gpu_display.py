"""The display transform on the GPU: the kernels of smallvcm_amd/csrc/vcm_display.hip against the host emulation of the
same functions (tests/host_emul_display), bit for bit -- the float4 image, the histogram, the statistics, the bytes --
the default parameters against the encoding they replace, the refusals of the context calls, vcm_render's flags and the
Python wrappers."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import denoise_lib as dl
import display_lib as dsp
from smallvcm_amd._abi import ALGO_PATH_TRACE, ALGO_VCM, DisplayStats
from smallvcm_amd.renderer import HipBackend, VertexCM, display_params, display_tensors, load_library

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VCM_RENDER = os.path.join(ROOT, "smallvcm_amd", "host", "vcm_render")
CAP = 2   # workgroups of the histogram's small grid: CAP * 256 lanes
# W x H.  One row of 1, 255, 256, 257, CAP * 256 + 3 pixels: one lane; a partial wave; one workgroup; two; a lane owns two
# pixels (the grid-stride path).  Then images whose levels have odd sizes, one column, one row.
SHAPES = [(1, 1), (255, 1), (256, 1), (257, 1), (CAP * 256 + 3, 1), (3, 2), (5, 7), (67, 45), (257, 3)]
RICH = dict(curve="aces", transfer="srgb", autoExposure=1, bloomStrength=0.3, bloomLevels=3, dither=1, ditherSeed=7, exposureEV=0.5)


def backend(scene, algo=ALGO_VCM, seed=1234, **kw):
    return HipBackend(dl.desc5(scene), algo, 0.003, 0.75, seed, **kw)


def same_bits(a, b):
    return np.ascontiguousarray(a, np.float32).tobytes() == np.ascontiguousarray(b, np.float32).tobytes()


def levels_to_one(W, H):
    n = 0
    while W > 1 or H > 1:
        W, H, n = max(1, (W + 1) // 2), max(1, (H + 1) // 2), n + 1
    return min(8, max(1, n))


def hdr_image(W, H, channels, seed=0):
    """a random HDR image over fourteen octaves with a NaN, an Inf, zeros and a negative pixel planted (where it has room)"""
    rng = np.random.default_rng(seed + 1000 * W + H)
    img = (rng.gamma(2.0, 0.5, (H, W, channels)) * np.exp2(rng.uniform(-8.0, 6.0, (H, W, 1)))).astype(np.float32)
    flat = img.reshape(-1, channels)
    if flat.shape[0] >= 6:
        flat[1, 1] = np.nan
        flat[2, 0] = np.inf
        flat[3] = 0.0
        flat[4, :3] = -0.25
        flat[5, :3] = 2.0 ** -24
    return img


def gpu_histogram():
    L = load_library()
    bins = np.zeros(dsp.BINS, np.uint64)
    assert L.vcm_debug_read_display_histogram(bins.ctypes.data_as(C.POINTER(C.c_ulonglong))) == 0, L.vcm_last_error()
    return bins


def check_buffers(img, **kw):
    """vcm_display_buffers on img (through display_tensors) = the emulation: image, statistics, histogram"""
    import torch
    p = dsp.params(**kw)
    want, st, bins = dsp.display(img, p)
    out, got = display_tensors(torch.from_numpy(img).cuda(), **kw)
    out = out.cpu().numpy()
    assert same_bits(out, want), (img.shape, kw, np.abs(out - want).max())
    assert got == st, (img.shape, kw, got, st)
    if p.autoExposure:
        assert np.array_equal(gpu_histogram(), bins), (img.shape, kw)
    return out, got


@pytest.fixture
def small_grid():
    """the histogram kernel's grid capped at CAP workgroups, so that a few hundred pixels reach the grid-stride path"""
    L = load_library()
    L.vcm_debug_display_max_blocks(CAP)
    yield CAP
    L.vcm_debug_display_max_blocks(0)


# ---------------- vcm_display_buffers = the emulation, bit for bit ----------------
@pytest.mark.parametrize("shape", SHAPES)
def test_buffers_equal_the_emulation(shape, small_grid):
    """both channel strides x the four curves x both transfers x bloom off, at one level and down to 1 x 1 (at most 8
    levels), auto-exposure on, NaN / Inf / zeros planted"""
    W, H = shape
    clipped = 0
    for channels in (3, 4):
        img = hdr_image(W, H, channels)
        for curve in ("clamp", "reinhard", "aces", "hable"):
            for transfer in ("gamma", "srgb"):
                for strength, levels in ((0.0, 5), (0.4, 1), (1.0, levels_to_one(W, H))):
                    _, st = check_buffers(img, curve=curve, transfer=transfer, autoExposure=1, bloomStrength=strength, bloomLevels=levels,
                                          whitePoint=2.5, exposureEV=1.0)
                    clipped += st["clipped"]
                    assert st["counted"] + st["zero"] + st["nonFinite"] == W * H
    if W * H >= 6:
        assert st["nonFinite"] == 2 and st["zero"] == 2 and st["clampedLow"] == 1 and clipped > 0


@pytest.mark.parametrize("shape", [(256, 1), (CAP * 256 + 3, 1), (67, 45)])
def test_a_constant_image_sends_every_lane_to_one_bin(shape, small_grid):
    W, H = shape
    img = np.full((H, W, 3), 0.37, np.float32)
    out, st = check_buffers(img, autoExposure=1, curve="reinhard", bloomStrength=0.5, bloomLevels=2)
    bins = gpu_histogram()
    assert bins.max() == W * H and (bins > 0).sum() == 1 and st["counted"] == W * H
    assert np.unique(out.reshape(-1, 4), axis=0).shape[0] == 1                      # the bloom keeps it constant
    img[0, W // 2] = 3.0                                                            # one lane of one wave differs
    check_buffers(img, autoExposure=1)
    assert sorted(gpu_histogram()[gpu_histogram() > 0].tolist()) == [1, W * H - 1]


def test_buffers_without_auto_exposure_and_with_scale():
    import torch
    img = hdr_image(67, 45, 3, seed=5)
    _, st = check_buffers(img, curve="hable", exposureEV=-2.0)
    assert st["autoEV"] == 0.0 and st["multiplier"] == 0.25 and st["counted"] == 0 and st["clipped"] >= 0
    p = dsp.params(autoExposure=1, curve="aces")
    want, wst, _ = dsp.display(img, p, scale=0.125)
    out, got = display_tensors(torch.from_numpy(img).cuda(), scale=0.125, autoExposure=1, curve="aces")
    assert same_bits(out.cpu().numpy(), want) and got == wst
    # a caller's out tensor, and twice the same bits
    mine = torch.empty((45, 67, 4), dtype=torch.float32, device="cuda")
    back, _ = display_tensors(torch.from_numpy(img).cuda(), out=mine, scale=0.125, autoExposure=1, curve="aces")
    assert back is mine and same_bits(mine.cpu().numpy(), want)
    with pytest.raises(RuntimeError, match="bloomLevels"):
        display_tensors(torch.from_numpy(img).cuda(), bloomLevels=9)
    with pytest.raises(ValueError):
        display_tensors(torch.from_numpy(img[..., :2].copy()).cuda())


# ---------------- a context = the emulation fed the same image ----------------
@pytest.mark.parametrize("algo", [ALGO_PATH_TRACE, ALGO_VCM])
@pytest.mark.parametrize("res", [(20, 14), (67, 45)])
@pytest.mark.parametrize("scene", [1, 3])
def test_a_context_equals_the_emulation_fed_its_images(scene, res, algo):
    sc = dl.box(scene, *res)
    b, plain = backend(sc, algo), backend(sc, algo)
    try:
        b.track_robust(3)
        for it in range(5):
            b.run_iteration(it, 0, 10)
            plain.run_iteration(it, 0, 10)
            if it == 2:
                b.display(**RICH)        # between iterations: it must not disturb the next
        fb = b.framebuffer_sum()
        sources = {"framebuffer": (fb, 1.0 / 5), "denoised": (b.denoise(1.0 / 5), 1.0), "robust": (b.robust(), 1.0)}
        for source, (img, scale) in sources.items():
            for kw in (RICH, dict(curve="reinhard", autoExposure=1), dict()):
                p = dsp.params(**kw)
                want, st, bins = dsp.display(img, p, scale=scale)
                got = b.display(source, **kw)
                assert same_bits(got, want[..., :3]), (source, kw)
                assert b.display_stats() == st, (source, kw)
                if p.autoExposure:
                    assert np.array_equal(gpu_histogram(), bins)
                    assert st["counted"] > 0
                for fmt in (dsp.IMAGE_BGR8, dsp.IMAGE_RGBA8):
                    assert np.array_equal(b.read_display_image(fmt), dsp.encode(want, fmt, p.dither, p.ditherSeed)), (source, kw, fmt)
        assert same_bits(b.framebuffer_sum(), fb) and same_bits(fb, plain.framebuffer_sum())   # the display does not disturb rendering
    finally:
        b.close()
        plain.close()


# ---------------- the default is the old path ----------------
def test_default_parameters_give_the_bytes_of_vcm_read_image():
    sc = dl.box(1, 67, 45)
    b = backend(sc)
    try:
        for it in range(3):
            b.run_iteration(it, 0, 10)
        for scale in (1.0 / 3, 16.0):    # the image, and one where much of it clips
            old = b.read_image(0, scale, 2.2)
            b.display("framebuffer", scale)
            assert np.array_equal(b.read_display_image(dsp.IMAGE_BGR8), old)
            assert b.display_stats()["clipped"] == int((old == 255).sum())
        assert (old == 255).mean() > 0.05
        clean = b.denoise(1.0 / 3)
        old = b.read_denoised_image(0, 2.2)
        b.display("denoised")
        assert np.array_equal(b.read_display_image(dsp.IMAGE_BGR8), old)
        assert b.display("denoised", gamma=1.7).shape == clean.shape
        assert np.array_equal(b.read_display_image(dsp.IMAGE_BGR8), b.read_denoised_image(0, 1.7))
    finally:
        b.close()


def read_bmp(path, W, H):
    raw = open(path, "rb").read()
    assert raw[:2] == b"BM" and len(raw) == 54 + W * H * 3
    return raw, np.frombuffer(raw[54:], np.uint8).reshape(H, W, 3)


def test_vcm_render_without_the_flags_writes_what_it_wrote_and_with_them_the_display(tmp_path):
    W, H, its, seed = 31, 23, 2, 5
    base = [VCM_RENDER, "-s", "1", "-a", "vcm", "-i", str(its), "--res", str(W), str(H), "--seed", str(seed)]
    a, c, d = str(tmp_path / "a.bmp"), str(tmp_path / "c.bmp"), str(tmp_path / "d.bmp")
    r = subprocess.run(base + ["-o", a, "--json"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-500:]
    assert "display" not in json.loads(r.stdout.strip().splitlines()[-1])
    v = VertexCM(dl.box(1, W, H), VertexCM.kVcm, 0.003, 0.75, seed)
    try:
        v.mMaxPathLength = 10
        for it in range(its):
            v.RunIteration(it)
        raw_a, px_a = read_bmp(a, W, H)
        assert np.array_equal(px_a, v.backend.read_image(0, 1.0 / its, 2.2))          # the old path, through vcm_read_image
        # a flag that changes nothing (the default curve) goes through the display transform: the same file, byte for byte
        r = subprocess.run(base + ["-o", c, "--tonemap", "clamp", "--json"], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-500:]
        assert open(c, "rb").read() == raw_a
        assert json.loads(r.stdout.strip().splitlines()[-1])["display"]["multiplier"] == 1.0
        flags = ["--tonemap", "aces", "--exposure", "0.5", "--auto-exposure", "0.25", "--bloom", "0.3", "3", "--srgb", "--dither"]
        r = subprocess.run(base + ["-o", d, "--json"] + flags, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-500:]
        shown = v.GetDisplay(curve="aces", exposureEV=0.5, autoExposure=1, key=0.25, bloomStrength=0.3, bloomLevels=3, transfer="srgb", dither=1)
        assert shown.shape == (H, W, 3) and shown.min() >= 0.0 and shown.max() <= 1.0
        assert json.loads(r.stdout.strip().splitlines()[-1])["display"] == v.backend.display_stats()
        assert np.array_equal(read_bmp(d, W, H)[1], v.backend.read_display_image(dsp.IMAGE_BGR8))
        assert not np.array_equal(read_bmp(d, W, H)[1], px_a)
    finally:
        v.close()
    # .pfm stays linear whatever the flags; the statistics are still reported
    e, f = str(tmp_path / "e.pfm"), str(tmp_path / "f.pfm")
    assert subprocess.run(base + ["-o", e], capture_output=True, text=True, timeout=300).returncode == 0
    r = subprocess.run(base + ["-o", f] + flags, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "display transform: exposure x" in r.stdout, (r.stdout, r.stderr[-500:])
    assert open(e, "rb").read() == open(f, "rb").read()
    r = subprocess.run(base + ["--renderers", "2", "--srgb"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and "one renderer" in r.stderr
    r = subprocess.run(base + ["--tonemap", "filmic"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and "--tonemap" in r.stderr


def test_vcm_render_displays_the_denoised_and_the_robust_image(tmp_path):
    W, H = 20, 14
    base = [VCM_RENDER, "-s", "1", "-a", "pt", "--res", str(W), str(H), "--seed", "9", "--tonemap", "hable", "--auto-exposure", "--json"]
    b = backend(dl.box(1, W, H), ALGO_PATH_TRACE, 9)
    try:
        b.track_robust(3)
        for it in range(4):
            b.run_iteration(it, 0, 10)
        out = str(tmp_path / "r.bmp")
        r = subprocess.run(base + ["-i", "4", "--robust", "3", "-o", out], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-500:]
        b.display("robust", curve="hable", autoExposure=1)
        assert np.array_equal(read_bmp(out, W, H)[1], b.read_display_image(dsp.IMAGE_BGR8))
        assert json.loads(r.stdout.strip().splitlines()[-1])["display"] == b.display_stats()
        out = str(tmp_path / "n.bmp")
        r = subprocess.run(base + ["-i", "4", "--denoise", "-o", out], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-500:]
        b.denoise(1.0 / 4)
        b.display("denoised", curve="hable", autoExposure=1)
        assert np.array_equal(read_bmp(out, W, H)[1], b.read_display_image(dsp.IMAGE_BGR8))
        assert json.loads(r.stdout.strip().splitlines()[-1])["display"] == b.display_stats()
        b.display("framebuffer", curve="hable", autoExposure=1)
        assert np.array_equal(read_bmp(str(tmp_path / "n.noisy.bmp"), W, H)[1], b.read_display_image(dsp.IMAGE_BGR8))
    finally:
        b.close()


# ---------------- the layouts, repeatability, the wrappers, the refusals ----------------
def test_layouts_repeatability_and_the_device_image():
    import torch
    b = backend(dl.box(3, 67, 45))
    try:
        for it in range(2):
            b.run_iteration(it, 0, 10)
        shown = b.display(**RICH)
        bgr, rgba = b.read_display_image(dsp.IMAGE_BGR8), b.read_display_image(dsp.IMAGE_RGBA8)
        assert np.array_equal(rgba[..., :3], bgr[::-1, :, ::-1]) and (rgba[..., 3] == 255).all()
        assert shown.min() >= 0.0 and shown.max() <= 1.0 and shown.std() > 0.01
        st = b.display_stats()
        again = b.display(**RICH)
        assert same_bits(shown, again) and b.display_stats() == st
        assert np.array_equal(b.read_display_image(dsp.IMAGE_BGR8), bgr) and np.array_equal(b.read_display_image(dsp.IMAGE_RGBA8), rgba)
        plain = b.display(**dict(RICH, dither=0))
        assert same_bits(plain, shown)                                        # the dither touches the bytes alone
        trunc = b.read_display_image(dsp.IMAGE_RGBA8)
        diff = rgba[..., :3].astype(np.int32) - trunc[..., :3].astype(np.int32)
        assert diff.min() == 0 and diff.max() == 1 and 0.2 < diff.mean() < 0.8   # floor(x + d) is x's floor or one more
        # the device image: W * H float4 {rgb, 1}, what display_tensors would have made of the mean
        b.synchronize()
        ptr = b.display_device()

        class DevImage:
            __cuda_array_interface__ = {"shape": (45, 67, 4), "typestr": "<f4", "data": (ptr, False), "version": 2}

        dev = torch.as_tensor(DevImage(), device="cuda").cpu().numpy()
        assert same_bits(dev[..., :3], plain) and (dev[..., 3] == 1.0).all()
        mean = torch.from_numpy(b.framebuffer_sum() * np.float32(0.5)).cuda()
        out, st2 = display_tensors(mean, **dict(RICH, dither=0))
        assert st2["counted"] == st["counted"] and out.shape == (45, 67, 4)
        # auto-exposure brings the mean log luminance of the trimmed pixels to the key
        st = b.display_stats()
        assert abs(st["autoEV"] + st["logAvgLuminance"] - np.log2(float(np.float32(0.18)))) < 1e-9 or st["autoEV"] in (-16.0, 16.0)   # the key is fp32
    finally:
        b.close()


def test_refusals_of_the_context_calls():
    sc = dl.box(1, 20, 14)
    b = backend(sc)
    try:
        L = b.L
        p, st, pv = display_params(), DisplayStats(), C.c_void_p()
        px = np.zeros((14, 20, 4), np.uint8)
        ub = px.ctypes.data_as(C.POINTER(C.c_ubyte))
        b.run_iteration(0, 0, 10)
        assert L.vcm_read_display_image(b.ctx, 0, ub) == -1 and b"vcm_display has not run" in L.vcm_last_error()
        assert L.vcm_get_display_stats(b.ctx, C.byref(st)) == -1 and L.vcm_display_device(b.ctx, C.byref(pv)) == -1
        assert L.vcm_display(b.ctx, 1, 1.0, C.byref(p)) == -1 and b"vcm_denoise has not run" in L.vcm_last_error()
        assert L.vcm_display(b.ctx, 2, 1.0, C.byref(p)) == -1 and b"vcm_track_robust is off" in L.vcm_last_error()
        assert L.vcm_display(b.ctx, 3, 1.0, C.byref(p)) == -1 and b"unknown source" in L.vcm_last_error()
        assert L.vcm_display(b.ctx, -1, 1.0, C.byref(p)) == -1
        assert L.vcm_display(b.ctx, 0, float("nan"), C.byref(p)) == -1 and b"scale" in L.vcm_last_error()
        assert L.vcm_display(b.ctx, 0, 1.0, None) == -1
        with pytest.raises(RuntimeError, match="gamma"):
            b.display(gamma=0.0)
        assert L.vcm_read_display_image(b.ctx, 0, ub) == -1          # a refused vcm_display leaves nothing behind
        b.display()
        assert L.vcm_read_display_image(b.ctx, 1, ub) == -1 and b"RGBE" in L.vcm_last_error()
        assert L.vcm_read_display_image(b.ctx, 3, ub) == -1 and b"unknown format" in L.vcm_last_error()
        assert L.vcm_read_display_image(b.ctx, 2, ub) == 0 and (px[..., 3] == 255).all()
        assert L.vcm_read_image(b.ctx, 2, 1.0, 2.2, ub) == -1       # RGBA8 belongs to the display transform alone
    finally:
        b.close()
    s = backend(sc, rank=1, world=2)
    try:
        assert s.L.vcm_display(s.ctx, 0, 1.0, C.byref(p)) == -1 and b"sharded" in s.L.vcm_last_error()
        assert s.L.vcm_read_display(s.ctx, np.zeros(20 * 14 * 3, np.float32).ctypes.data_as(C.POINTER(C.c_float))) == -1
        assert b"sharded" in s.L.vcm_last_error()
    finally:
        s.close()
