"""Feature buffers and denoiser on the GPU: the kernels of smallvcm_amd/csrc/vcm_denoise.hip against the host emulation
of the same functions (tests/host_emul_denoise), bit for bit, and the equivalences between the entry points."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import denoise_lib as dl
import envmap_lib as el
import pick_lib as pl
from smallvcm_amd._abi import ALGO_PATH_TRACE, ALGO_VCM
from smallvcm_amd.renderer import HipBackend, VertexCM, denoise_params, denoise_tensors

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VCM_RENDER = os.path.join(ROOT, "smallvcm_amd", "host", "vcm_render")


def gpu_features(b):
    g = np.zeros((b.resy, b.resx, 4), np.float32)
    g[..., :3] = b.feature("normal")
    g[..., 3] = b.feature("depth")
    a = np.ones((b.resy, b.resx, 4), np.float32)
    a[..., :3] = b.feature("albedo")
    return g, a


def backend(scene, algo=ALGO_VCM, seed=1234, **kw):
    return HipBackend(dl.desc5(scene), algo, 0.003, 0.75, seed, **kw)


def same_bits(a, b):
    return np.ascontiguousarray(a, np.float32).tobytes() == np.ascontiguousarray(b, np.float32).tobytes()


# ---------------- GPU = host emulation, bit for bit ----------------
@pytest.mark.parametrize("kind", ["rects", "list", "bvh", "rects_envmap", "bvh_envmap", "mesh"])
def test_features_equal_the_emulation(kind, monkeypatch):
    if kind in ("list",):
        monkeypatch.setenv("SMALLVCM_AMD_NO_ONEPLANE", "1")   # read when the scene is built, on both sides
        monkeypatch.setenv("SMALLVCM_AMD_GENERAL_POW", "1")
    if kind in ("bvh", "bvh_envmap"):
        monkeypatch.setenv("SMALLVCM_AMD_FORCE_BVH", "1")
    if kind == "mesh":
        sc = pl.lamp_room(resx=31, resy=23)
    elif kind.endswith("envmap"):
        sc = el.builtin_with_envmap(el.sky(32, 16), resx=31, resy=23)
    else:
        sc = dl.box(1, 31, 23)
    b = backend(sc)
    try:
        g, a = gpu_features(b)
    finally:
        b.close()
    eg, ea = dl.features(sc)
    assert (eg[..., 3] > 0).any()
    assert same_bits(g, eg)
    assert same_bits(a[..., :3], ea[..., :3])


@pytest.mark.parametrize("algo", [ALGO_PATH_TRACE, ALGO_VCM])
@pytest.mark.parametrize("res", [(20, 14), (67, 45)])
def test_denoised_render_equals_the_emulation(algo, res):
    sc = dl.box(1, *res)
    b = backend(sc, algo)
    try:
        for it in range(2):
            b.run_iteration(it, 0, 10)
        fb = b.framebuffer_sum()
        out = b.denoise(0.5)
        g, a = gpu_features(b)
        raw = b.denoise(0.5, demodulate=0, passes=3)
    finally:
        b.close()
    assert np.isfinite(out).all() and out.max() > 0
    assert same_bits(out, dl.denoise(fb, a, g, dl.defaults(), scale=0.5)[..., :3])
    assert same_bits(raw, dl.denoise(fb, a, g, dl.params(demodulate=0, passes=3), scale=0.5)[..., :3])


def synthetic(H, W, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    g = np.zeros((H, W, 4), np.float32)
    n = np.stack([np.sin(xx / 37.0), np.cos(yy / 23.0), np.ones_like(xx, float)], -1)
    n[(xx // 64 + yy // 96) % 2 == 1] *= (-1.0, 1.0, 0.2)
    g[..., :3] = n / np.linalg.norm(n, axis=-1, keepdims=True)
    g[..., 3] = 2.0 + np.sin(xx / 50.0) + (yy // 128) * 0.7
    g[(xx - 300) ** 2 + (yy - 200) ** 2 < 60 ** 2] = 0.0   # a hole: misses
    a = np.ones((H, W, 4), np.float32)
    a[..., :3] = rng.uniform(0.1, 1.0, (H, W, 3))
    c = np.ones((H, W, 4), np.float32)
    c[..., :3] = (0.5 + 0.5 * np.sin(xx / 91.0 + yy / 57.0))[..., None] * a[..., :3] * rng.gamma(2.0, 0.5, (H, W, 3))
    c[100, 100, 0] = np.inf
    c[400, 17, 2] = np.nan
    return c, a, g


@pytest.mark.parametrize("demodulate", [0, 1])
def test_denoise_buffers_equals_the_emulation_on_512x512(demodulate):
    import torch
    c, a, g = synthetic(512, 512, 3)
    tc, ta, tg = (torch.from_numpy(x).cuda() for x in (c, a, g))
    for passes in range(1, 7):
        out = denoise_tensors(tc, ta, tg, passes=passes, demodulate=demodulate).cpu().numpy()
        ref = dl.denoise(c, a, g, dl.params(passes=passes, demodulate=demodulate))
        fin = np.isfinite(ref)
        assert np.array_equal(np.isnan(out), np.isnan(ref)) and not fin.all() and fin.mean() > 0.99
        assert np.array_equal(out.view(np.uint32)[fin], ref.view(np.uint32)[fin]), passes
        assert np.array_equal(out[~fin & ~np.isnan(ref)], ref[~fin & ~np.isnan(ref)])
    assert same_bits(denoise_tensors(tc, ta, tg, passes=0).cpu().numpy(), c)


# ---------------- equivalences ----------------
def test_context_buffers_and_tensor_paths_agree_and_the_framebuffer_is_untouched():
    import torch
    sc = dl.box(3, 67, 45)
    b = backend(sc)
    try:
        b.run_iteration(0, 0, 10)
        before = b.framebuffer_sum()
        out = b.denoise(1.0)
        assert same_bits(b.framebuffer_sum(), before)   # denoising does not disturb accumulation
        g, a = gpu_features(b)
        # vcm_denoise_buffers on the context's own feature images and the exported frame
        pa, pg = b.features_device()
        color = torch.from_numpy(dl.as4(before)).cuda()
        res = torch.empty_like(color)
        p = denoise_params()
        assert b.L.vcm_denoise_buffers(0, 67, 45, color.data_ptr(), pa, pg, res.data_ptr(), C.byref(p), torch.cuda.current_stream().cuda_stream) == 0
        assert same_bits(res.cpu().numpy()[..., :3], out)
        # the torch-tensor path over copies of everything
        t = denoise_tensors(color, torch.from_numpy(a).cuda(), torch.from_numpy(g).cuda())
        assert same_bits(t.cpu().numpy()[..., :3], out)
        # the 8-bit encodings of the denoised image = the host encoding of vcm_read_denoised
        bgr = b.read_denoised_image(0)
        L = b.L
        L.vcm_host_powf.restype = C.c_float
        want = np.zeros_like(bgr)
        for y in range(45):
            for x in range(67):
                px = out[45 - y - 1, x]
                want[y, x] = [min(255.0, max(0.0, float(np.float32(L.vcm_host_powf(float(px[2 - k]), np.float32(1.0) / np.float32(2.2))) * np.float32(255.0)))) for k in range(3)]
        assert np.array_equal(bgr, want)
        rgbe = b.read_denoised_image(1)
        top = out.max(axis=2)
        lit = top >= 1e-32
        assert lit.mean() > 0.9 and (rgbe[~lit] == 0).all()
        m, e = np.frexp(top[lit].astype(np.float64))
        v = (m * 256.0 / top[lit]).astype(np.float32)
        assert np.array_equal(rgbe[lit][:, 3], (e + 128).astype(np.uint8))
        assert np.array_equal(rgbe[lit][:, :3], (out[lit] * v[:, None]).astype(np.uint8))
    finally:
        b.close()


def test_iterate_denoise_iterate_denoise_equals_a_fresh_context():
    sc = dl.box(0, 40, 30)
    a = VertexCM(dl.desc5(sc), VertexCM.kVcm, 0.003, 0.75, 77)
    b = VertexCM(dl.desc5(sc), VertexCM.kVcm, 0.003, 0.75, 77)
    a.mMaxPathLength = b.mMaxPathLength = 10
    try:
        a.RunIteration(0)
        first = a.GetDenoised()
        a.RunIteration(1)
        second = a.GetDenoised()
        b.RunIteration(0)
        b.RunIteration(1)
        fresh = b.GetDenoised()
        assert same_bits(a.framebuffer_sum(), b.framebuffer_sum())
        assert same_bits(second, fresh) and not same_bits(first, second)
    finally:
        a.close()
        b.close()


def read_pfm(path):
    with open(path, "rb") as f:
        kind = f.readline().strip()
        w, h = (int(x) for x in f.readline().split())
        assert float(f.readline()) == -1.0
        return np.frombuffer(f.read(), np.float32).reshape(h, w, 3 if kind == b"PF" else 1)


def test_vcm_render_denoise_and_features_out_write_the_python_paths_images(tmp_path):
    out = str(tmp_path / "img.pfm")
    r = subprocess.run([VCM_RENDER, "-s", "1", "-a", "vcm", "-i", "2", "--res", "67", "45", "--seed", "5", "-o", out, "--denoise", "4",
                        "--denoise-sigma", "8,16,0.1", "--features-out", str(tmp_path / "feat")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-500:]
    v = VertexCM(dl.box(1, 67, 45), VertexCM.kVcm, 0.003, 0.75, 5)
    v.mMaxPathLength = 10
    try:
        v.RunIteration(0)
        v.RunIteration(1)
        assert same_bits(read_pfm(str(tmp_path / "img.noisy.pfm")), v.GetFramebuffer())
        assert same_bits(read_pfm(out), v.GetDenoised(passes=4, sigmaColor=8.0, sigmaNormal=16.0, sigmaDepth=0.1))
        for name in ("albedo", "normal", "depth"):
            assert same_bits(read_pfm(str(tmp_path / ("feat.%s.pfm" % name))).squeeze(), v.backend.feature(name))
    finally:
        v.close()
    r = subprocess.run([VCM_RENDER, "-s", "1", "-i", "1", "--res", "16", "16", "--renderers", "2", "--denoise"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 2 and "one renderer" in r.stderr


# ---------------- refusal ----------------
def test_a_sharded_context_is_refused_with_a_message_but_renders_its_features():
    sc = dl.box(1, 24, 18)
    b = backend(sc, rank=1, world=2)
    try:
        p = denoise_params()
        pv = C.c_void_p()
        buf = np.zeros((18, 24, 3), np.float32)
        img = np.zeros((18, 24, 4), np.uint8)
        for rc in (b.L.vcm_denoise(b.ctx, 1.0, C.byref(p)), b.L.vcm_read_denoised(b.ctx, buf.ctypes.data_as(C.POINTER(C.c_float))),
                   b.L.vcm_denoised_device(b.ctx, C.byref(pv)), b.L.vcm_read_denoised_image(b.ctx, 0, 2.2, img.ctypes.data_as(C.POINTER(C.c_ubyte)))):
            assert rc == -1
            assert b"sharded" in b.L.vcm_last_error()
        g, a = gpu_features(b)
        eg, ea = dl.features(sc, rank=1, world=2)
        assert same_bits(g, eg)
        assert (g.reshape(-1, 4)[:b.first] == 0).all() and (g.reshape(-1, 4)[b.first:, 3] > 0).any()
    finally:
        b.close()


def test_unknown_feature_format_and_order_are_refused():
    b = backend(dl.box(1, 16, 16))
    try:
        buf = np.zeros((16, 16, 3), np.float32)
        img = np.zeros((16, 16, 4), np.uint8)
        fp, up = buf.ctypes.data_as(C.POINTER(C.c_float)), img.ctypes.data_as(C.POINTER(C.c_ubyte))
        assert b.L.vcm_read_feature(b.ctx, 3, fp) == -1 and b"unknown feature" in b.L.vcm_last_error()
        assert b.L.vcm_read_denoised(b.ctx, fp) == -1 and b"has not run" in b.L.vcm_last_error()
        p = denoise_params(passes=13)
        assert b.L.vcm_denoise(b.ctx, 1.0, C.byref(p)) == -1 and b"passes" in b.L.vcm_last_error()
        p = denoise_params()
        assert b.L.vcm_denoise(b.ctx, 1.0, C.byref(p)) == 0   # needs no iteration: a black frame
        assert b.L.vcm_read_denoised_image(b.ctx, 7, 2.2, up) == -1 and b"unknown format" in b.L.vcm_last_error()
        assert b.L.vcm_read_denoised(b.ctx, fp) == 0 and (buf == 0).all()
    finally:
        b.close()
