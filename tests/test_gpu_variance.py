"""Per-pixel variance, the noise statistic and render-to-target on the GPU: the kernels of
smallvcm_amd/csrc/vcm_variance.hip against the host emulation of the same functions (tests/host_emul_variance), bit for
bit, the refusals of the context calls, and the equivalences between the entry points."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import denoise_lib as dl
import variance_lib as vl
from smallvcm_amd._abi import ALGO_PATH_TRACE, ALGO_VCM, NoiseStats
from smallvcm_amd.renderer import HipBackend, VertexCM, load_library, noise_stats_tensors, variance_update_tensors

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VCM_RENDER = os.path.join(ROOT, "smallvcm_amd", "host", "vcm_render")
_fp = C.POINTER(C.c_float)
CAP = 2                                        # workgroups of the small grid: CAP * 256 lanes
COUNTS = [1, 255, 256, 257, CAP * 256 + 3]     # one lane; a partial wave; one workgroup; two; a lane owns two pixels


def backend(scene, algo=ALGO_VCM, seed=1234, **kw):
    return HipBackend(dl.desc5(scene), algo, 0.003, 0.75, seed, **kw)


def same_bits(a, b):
    return np.ascontiguousarray(a, np.float32).tobytes() == np.ascontiguousarray(b, np.float32).tobytes()


def images(b):
    """(prev, mom) of a tracked context, [N, 4] each"""
    prev, mom = vl.new_images(b.N)
    b.L.vcm_debug_read_variance_images.argtypes = [C.c_void_p, _fp, _fp]
    assert b.L.vcm_debug_read_variance_images(b.ctx, prev.ctypes.data_as(_fp), mom.ctypes.data_as(_fp)) == 0, b.L.vcm_last_error()
    return prev, mom


@pytest.fixture
def small_grid():
    """the kernels' grid capped at CAP workgroups, so that a few hundred pixels reach the grid-stride path"""
    L = load_library()
    L.vcm_debug_variance_max_blocks(CAP)
    yield CAP
    L.vcm_debug_variance_max_blocks(0)


# ---------------- a tracked context = the emulation, bit for bit ----------------
@pytest.mark.parametrize("algo", [ALGO_PATH_TRACE, ALGO_VCM])
@pytest.mark.parametrize("kind", ["rects", "list", "bvh"])
@pytest.mark.parametrize("res", [(20, 14), (67, 45)])
def test_tracked_moments_equal_the_emulation(algo, kind, res, monkeypatch):
    if kind == "list":
        monkeypatch.setenv("SMALLVCM_AMD_NO_ONEPLANE", "1")   # read when the scene is built, on both sides
        monkeypatch.setenv("SMALLVCM_AMD_GENERAL_POW", "1")
    if kind == "bvh":
        monkeypatch.setenv("SMALLVCM_AMD_FORCE_BVH", "1")
    sc = dl.box(1, *res)
    e = vl.TrackedEmul(sc, algo)
    b, plain = backend(sc, algo), backend(sc, algo)
    try:
        b.track_variance()
        for it in range(5):
            b.run_iteration(it, 0, 10)
            plain.run_iteration(it, 0, 10)
            e.run(1)
            if it + 1 in (1, 2, 5):
                prev, mom = images(b)
                assert same_bits(prev, e.prev) and same_bits(mom, e.mom), it + 1
                fb = b.framebuffer_sum()
                assert same_bits(fb, plain.framebuffer_sum())    # the hook does not disturb rendering
                assert same_bits(fb.reshape(-1, 3), prev[:, :3])
        assert mom[:, :3].max() > 0
        assert same_bits(b.variance(), e.variance())
        st = b.noise_stats(0.01)
        assert st == e.noise_stats(0.01) and st["iterations"] == 5 and 0 < st["above"] < st["elements"]
    finally:
        b.close()
        plain.close()


# ---------------- the buffers calls on synthetic inputs ----------------
def synthetic_frames(n, K=5, seed=0):
    rng = np.random.default_rng(seed + n)
    f = (rng.gamma(2.0, 0.5, (K, n, 3)) * rng.uniform(0.0, 2.0, (1, n, 3))).astype(np.float32)
    if n > 200:
        f[K - 2, 100, 1] = np.nan
        f[K - 1, 7, 0] = np.inf
    return f


@pytest.mark.parametrize("n", COUNTS)
def test_update_and_stats_buffers_equal_the_emulation(n, small_grid):
    import torch
    frames = synthetic_frames(n)
    sums, eprev, emom = vl.feed(frames)
    prev, mom = torch.zeros(n, 4, device="cuda"), torch.zeros(n, 4, device="cuda")
    for k in range(1, frames.shape[0] + 1):
        variance_update_tensors(torch.from_numpy(sums[k - 1]).cuda(), k, prev, mom)
    gp, gm = prev.cpu().numpy(), mom.cpu().numpy()
    assert same_bits(gp, eprev) and same_bits(gm, emom)
    assert np.isnan(gm).sum() == (2 if n > 200 else 0)
    thr = 0.05
    st = noise_stats_tensors(prev, mom, frames.shape[0], thr)
    ref = vl.stats(eprev, emom, frames.shape[0], thr, max_blocks=small_grid)
    assert st == ref and np.float64(st["mean"]).tobytes() == np.float64(ref["mean"]).tobytes()
    assert st["nonFinite"] == (2 if n > 200 else 0) and st["elements"] == 3 * n
    assert st == noise_stats_tensors(prev, mom, frames.shape[0], thr)     # the same bits on every run
    s64 = vl.stats64(eprev, emom, frames.shape[0], np.float32(thr))
    assert (st["above"], st["max"]) == (s64["above"], s64["max"]) and abs(st["mean"] - s64["mean"]) <= 1e-13 * s64["mean"]


def test_the_default_grid_equals_the_emulation_on_a_larger_image():
    """67 x 45 under the default cap: 12 workgroups, the last one partial, the second level with 12 of 256 lanes busy"""
    import torch
    n = 67 * 45
    frames = synthetic_frames(n, K=3)
    sums, eprev, emom = vl.feed(frames)
    prev, mom = torch.zeros(45, 67, 4, device="cuda"), torch.zeros(45, 67, 4, device="cuda")
    for k in range(1, 4):
        variance_update_tensors(torch.from_numpy(sums[k - 1].reshape(45, 67, 3)).cuda(), k, prev, mom)
    assert same_bits(mom.cpu().numpy(), emom)
    assert noise_stats_tensors(prev, mom, 3, 0.1) == vl.stats(eprev, emom, 3, 0.1)


def test_context_buffers_and_tensors_agree():
    """vcm_track_variance is vcm_variance_update_buffers on the context's images: the frames of a context fed through
    the tensor call give the context's moments, and its moments image through the buffers statistic gives its statistic"""
    import torch
    sc = dl.box(3, 31, 23)
    b = backend(sc, ALGO_PATH_TRACE)
    try:
        b.track_variance()
        prev, mom = torch.zeros(b.N, 4, device="cuda"), torch.zeros(b.N, 4, device="cuda")
        for it in range(3):
            b.run_iteration(it, 0, 10)
            variance_update_tensors(torch.from_numpy(b.framebuffer_sum()).cuda(), it + 1, prev, mom)
        cprev, cmom = images(b)
        assert same_bits(prev.cpu().numpy(), cprev) and same_bits(mom.cpu().numpy(), cmom)
        st = NoiseStats()
        assert b.L.vcm_noise_stats_buffers(0, b.N, prev.data_ptr(), b.variance_device(), 3, 0.02, C.byref(st),
                                           torch.cuda.current_stream().cuda_stream) == 0, b.L.vcm_last_error()
        assert st.asdict() == b.noise_stats(0.02)
    finally:
        b.close()


# ---------------- refusals and edges ----------------
def test_refusals_of_a_context():
    sc = dl.box(1, 24, 18)
    b = backend(sc, ALGO_PATH_TRACE)
    try:
        L = b.L
        out = np.zeros((18, 24, 3), np.float32)
        st = NoiseStats()
        # off: the readers say so
        assert L.vcm_read_variance(b.ctx, out.ctypes.data_as(_fp)) == -1 and b"off" in L.vcm_last_error()
        assert L.vcm_get_noise_stats(b.ctx, 0.0, C.byref(st)) == -1 and b"off" in L.vcm_last_error()
        b.run_iteration(0, 0, 10)
        # after an iteration
        assert L.vcm_track_variance(b.ctx, 1) == -1 and b"holds iterations" in L.vcm_last_error()
        # ... but right after a clear
        b.clear_framebuffer()
        b.track_variance()
        eprev, emom = vl.new_images(b.N)
        b.run_iteration(1, 0, 10)
        vl.update(b.framebuffer_sum(), 1, eprev, emom)
        # k < 2
        assert L.vcm_read_variance(b.ctx, out.ctypes.data_as(_fp)) == -1 and b"two iterations" in L.vcm_last_error()
        assert L.vcm_get_noise_stats(b.ctx, 0.0, C.byref(st)) == -1 and b"two iterations" in L.vcm_last_error()
        b.run_iteration(2, 0, 10)
        vl.update(b.framebuffer_sum(), 2, eprev, emom)
        prev, mom = images(b)
        assert same_bits(prev, eprev) and same_bits(mom, emom) and mom.any()   # the count started over with the clear
        assert b.noise_stats() == vl.stats(eprev, emom, 2)
        # a clear resets the images and the count
        b.clear_framebuffer()
        prev, mom = images(b)
        assert not prev.any() and not mom.any()
        assert L.vcm_get_noise_stats(b.ctx, 0.0, C.byref(st)) == -1 and b"two iterations" in L.vcm_last_error()
    finally:
        b.close()


def test_a_sharded_context_is_refused_in_the_words_of_the_denoiser():
    sc = dl.box(1, 24, 18)
    b = backend(sc, rank=1, world=3)
    try:
        L = b.L
        pv, st = C.c_void_p(), NoiseStats()
        buf = np.zeros((18, 24, 3), np.float32)
        for rc in (L.vcm_track_variance(b.ctx, 1), L.vcm_variance_device(b.ctx, C.byref(pv)),
                   L.vcm_read_variance(b.ctx, buf.ctypes.data_as(_fp)), L.vcm_get_noise_stats(b.ctx, 0.0, C.byref(st))):
            assert rc == -1
            assert b"sharded context: its framebuffer is a shard of the image" in L.vcm_last_error()
    finally:
        b.close()


def test_stats_between_iterations_change_nothing():
    """iterate -> stats -> iterate -> stats = a fresh context that only iterates"""
    sc = dl.box(1, 31, 23)
    a, b = backend(sc), backend(sc)
    try:
        a.track_variance()
        b.track_variance()
        seen = []
        for it in range(4):
            a.run_iteration(it, 0, 10)
            b.run_iteration(it, 0, 10)
            if it >= 1:
                seen.append(a.noise_stats(0.01))   # a looks after every iteration, b only at the end
        pa, ma = images(a)
        pb, mb = images(b)
        assert same_bits(pa, pb) and same_bits(ma, mb)
        assert seen[-1] == b.noise_stats(0.01) and [s["iterations"] for s in seen] == [2, 3, 4]
        assert same_bits(a.framebuffer_sum(), b.framebuffer_sum())
    finally:
        a.close()
        b.close()


# ---------------- render to a target ----------------
def test_vcm_render_noise_target_equals_render_until(tmp_path):
    res, check = (40, 30), 3
    sc = dl.box(1, *res)
    probe = VertexCM(dl.desc5(sc), ALGO_PATH_TRACE, 0.003, 0.75, 1234)
    probe.mMaxPathLength = 10
    looks = probe.render_until(0.0, check_every=check, max_iterations=9)
    assert [h["iterations"] for h in looks] == [3, 6, 9] and looks[0]["mean"] > looks[1]["mean"]
    target = float(np.float32(0.5 * (looks[0]["mean"] + looks[1]["mean"])))   # between the first look and the second
    probe.close()
    r = VertexCM(dl.desc5(sc), ALGO_PATH_TRACE, 0.003, 0.75, 1234)
    r.mMaxPathLength = 10
    hist = r.render_until(target, check_every=check, max_iterations=50)
    frame = r.GetFramebuffer()
    r.close()
    assert r.mIterations == 6 and [h["iterations"] for h in hist] == [3, 6] and hist[0]["mean"] > target
    out = str(tmp_path / "o.pfm")
    p = subprocess.run([VCM_RENDER, "-s", "1", "-a", "pt", "--res", str(res[0]), str(res[1]), "--noise-target", repr(float(target)),
                        "--check-every", str(check), "--max-iterations", "50", "-o", out], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-400:]
    assert "6 iteration(s) used" in p.stdout and p.stdout.count("noise after") == 2, p.stdout
    with open(out, "rb") as f:
        assert f.readline() == b"PF\n" and f.readline() == b"%d %d\n" % res and f.readline() == b"-1\n"
        img = np.frombuffer(f.read(), np.float32).reshape(res[1], res[0], 3)
    assert same_bits(img, frame)


# ---------------- the variance-guided filter ----------------
def gpu_features(b):
    g = np.zeros((b.resy, b.resx, 4), np.float32)
    g[..., :3] = b.feature("normal")
    g[..., 3] = b.feature("depth")
    a = np.ones((b.resy, b.resx, 4), np.float32)
    a[..., :3] = b.feature("albedo")
    return g, a


@pytest.mark.parametrize("algo", [ALGO_PATH_TRACE, ALGO_VCM])
@pytest.mark.parametrize("res", [(20, 14), (67, 45)])
def test_guided_denoise_of_a_render_equals_the_emulation(algo, res):
    sc = dl.box(1, *res)
    b = backend(sc, algo)
    try:
        b.track_variance()
        for it in range(4):
            b.run_iteration(it, 0, 10)
        fb = b.framebuffer_sum()
        _, mom = images(b)
        out = b.denoise2(0.25, varianceGuided=1)
        raw = b.denoise2(0.25, varianceGuided=1, demodulate=0, passes=3, sigmaVariance=2.0)
        plain2, plain = b.denoise2(0.25, varianceGuided=0), b.denoise(0.25)          # varianceGuided = 0 is vcm_denoise
        g, a = gpu_features(b)
        assert same_bits(b.framebuffer_sum(), fb)
    finally:
        b.close()
    f = vl.var_factor_context(0.25, 4)
    assert np.isfinite(out).all() and out.max() > 0
    assert same_bits(out, vl.denoise2(fb, a, g, mom, f, vl.params2(varianceGuided=1), scale=0.25)[..., :3])
    assert same_bits(raw, vl.denoise2(fb, a, g, mom, f, vl.params2(varianceGuided=1, demodulate=0, passes=3, sigmaVariance=2.0), scale=0.25)[..., :3])
    assert same_bits(plain2, plain) and not same_bits(plain, out)


def synthetic_guided(H, W, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    g = np.zeros((H, W, 4), np.float32)
    n = np.stack([np.sin(xx / 17.0), np.cos(yy / 13.0), np.ones_like(xx, float)], -1)
    n[(xx // 40 + yy // 30) % 2 == 1] *= (-1.0, 1.0, 0.2)
    g[..., :3] = n / np.linalg.norm(n, axis=-1, keepdims=True)
    g[..., 3] = 2.0 + np.sin(xx / 25.0) + (yy // 40) * 0.7
    g[(xx - 90) ** 2 + (yy - 40) ** 2 < 15 ** 2] = 0.0   # a hole: misses
    a = np.ones((H, W, 4), np.float32)
    a[..., :3] = rng.uniform(0.1, 1.0, (H, W, 3))
    sig = 0.02 + 0.3 * rng.uniform(size=(H, W, 1)) ** 3
    c = np.ones((H, W, 4), np.float32)
    c[..., :3] = (0.5 + 0.5 * np.sin(xx / 31.0 + yy / 19.0))[..., None] * a[..., :3] * (1.0 + sig * rng.normal(size=(H, W, 3)))
    mom = np.zeros((H, W, 4), np.float32)
    mom[..., :3] = (sig * c[..., :3]) ** 2 * 12.0     # k = 4: V = M2 / 12
    c[30, 100, 0] = np.inf
    c[60, 17, 2] = np.nan
    mom[5, 5, 1] = np.nan
    mom[50, 70, 0] = np.inf
    return c, a, g, mom


@pytest.mark.parametrize("demodulate", [0, 1])
def test_denoise_buffers2_equals_the_emulation_on_128x72(demodulate):
    """passes 1 .. 6: the LDS kernel (steps 1, 2) and the global-tap kernel (steps 4 .. 32), a frame no multiple of the
    32 x 8 tile, non-finite colours and variances planted"""
    import torch
    from smallvcm_amd.renderer import denoise_tensors, denoise_tensors2
    c, a, g, mom = synthetic_guided(72, 128, 3)
    tc, ta, tg, tm = (torch.from_numpy(x).cuda() for x in (c, a, g, mom))
    for passes in range(1, 7):
        out = denoise_tensors2(tc, ta, tg, tm, 4, passes=passes, demodulate=demodulate, varianceGuided=1).cpu().numpy()
        ref = vl.denoise2(c, a, g, mom, vl.var_factor_mean(4), vl.params2(passes=passes, demodulate=demodulate, varianceGuided=1))
        fin = np.isfinite(ref)
        assert np.array_equal(np.isfinite(out), fin) and np.array_equal(np.isnan(out), np.isnan(ref)) and not fin.all() and fin.mean() > 0.99
        assert np.array_equal(out.view(np.uint32)[fin], ref.view(np.uint32)[fin]), passes
    off = denoise_tensors2(tc, ta, tg, tm, 4, passes=4, demodulate=demodulate, varianceGuided=0).cpu().numpy()
    old = denoise_tensors(tc, ta, tg, passes=4, demodulate=demodulate).cpu().numpy()
    assert off.tobytes() == old.tobytes()


def test_guided_denoise_wants_tracking_and_two_iterations():
    sc = dl.box(1, 24, 18)
    b = backend(sc, ALGO_PATH_TRACE)
    try:
        p = vl.params2()       # guided by default
        assert p.varianceGuided == 1
        b.run_iteration(0, 0, 10)
        assert b.L.vcm_denoise2(b.ctx, 1.0, C.byref(p)) == -1 and b"off" in b.L.vcm_last_error()
        b.clear_framebuffer()
        b.track_variance()
        b.run_iteration(1, 0, 10)
        assert b.L.vcm_denoise2(b.ctx, 1.0, C.byref(p)) == -1 and b"two iterations" in b.L.vcm_last_error()
        assert np.isfinite(b.denoise2(1.0, varianceGuided=0)).all()      # unguided: no variance needed
        b.run_iteration(2, 0, 10)
        assert np.isfinite(b.denoise2(0.5, varianceGuided=1)).all()
    finally:
        b.close()
    s = backend(sc, rank=1, world=3)
    try:
        assert s.L.vcm_denoise2(s.ctx, 1.0, C.byref(p)) == -1 and b"sharded" in s.L.vcm_last_error()
    finally:
        s.close()
