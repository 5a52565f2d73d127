"""The firefly-robust estimate on the GPU: the kernels of smallvcm_amd/csrc/vcm_robust.hip against the host emulation of
the same functions (tests/host_emul_robust), bit for bit, the refusals of the context calls, and the equivalences between
the entry points."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import denoise_lib as dl
import robust_lib as rl
import variance_lib as vl
from smallvcm_amd._abi import ALGO_PATH_TRACE, ALGO_VCM, ROBUST_DEFAULT_BUCKETS, RobustStats
from smallvcm_amd.renderer import (HipBackend, VertexCM, load_library, robust_resolve_tensors, robust_stats_tensors,
                                   robust_update_tensors)

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


def images(b, M):
    """(prev [N, 4], buckets [M, N, 4]) of a context that tracks M buckets"""
    prev, buckets = rl.new_images(b.N, M)
    b.L.vcm_debug_read_robust_images.argtypes = [C.c_void_p, _fp, _fp]
    assert b.L.vcm_debug_read_robust_images(b.ctx, prev.ctypes.data_as(_fp), buckets.ctypes.data_as(_fp)) == 0, b.L.vcm_last_error()
    return prev, buckets


def variance_images(b):
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
BUCKETS = (3, 5, 15)


@pytest.mark.parametrize("algo", [ALGO_PATH_TRACE, ALGO_VCM])
@pytest.mark.parametrize("kind", ["rects", "list", "bvh"])
@pytest.mark.parametrize("res", [(20, 14), (67, 45)])
def test_tracked_buckets_and_the_estimate_equal_the_emulation(algo, kind, res, monkeypatch):
    """one emulated render of 2 x 15 + 3 iterations bucketed for M = 3, 5 and 15 at once, against three contexts (the one
    with 15 buckets tracks the variance too) and an untracked one: prev, every plane and the resolved image after
    k = M, M + 1 and 2 M + 3"""
    if kind == "list":
        monkeypatch.setenv("SMALLVCM_AMD_NO_ONEPLANE", "1")   # read when the scene is built, on both sides
        monkeypatch.setenv("SMALLVCM_AMD_GENERAL_POW", "1")
    if kind == "bvh":
        monkeypatch.setenv("SMALLVCM_AMD_FORCE_BVH", "1")
    sc = dl.box(1, *res)
    e = vl.TrackedEmul(sc, algo)
    emul = {M: rl.new_images(e.emul.resx * e.emul.resy, M) for M in BUCKETS}
    ctx = {M: backend(sc, algo) for M in BUCKETS}
    plain = backend(sc, algo)
    try:
        for M in BUCKETS:
            ctx[M].track_robust(M)
        ctx[15].track_variance()
        checked = 0
        for k in range(1, 2 * 15 + 4):
            e.run(1)
            plain.run_iteration(k - 1, 0, 10)
            for M in BUCKETS:
                if k > 2 * M + 3:
                    continue
                rl.update(e.framebuffer(), k, *emul[M])
                ctx[M].run_iteration(k - 1, 0, 10)
                if k not in (M, M + 1, 2 * M + 3):
                    continue
                prev, buckets = images(ctx[M], M)
                assert same_bits(prev, emul[M][0]) and same_bits(buckets, emul[M][1]), (M, k)
                want = rl.resolve(*emul[M], k)
                assert same_bits(ctx[M].robust(), want[:, :3]), (M, k)
                assert ctx[M].robust_stats() == rl.stats(*emul[M], k), (M, k)
                checked += 1
                if k == 2 * M + 3:
                    assert same_bits(ctx[M].framebuffer_sum(), plain.framebuffer_sum())   # the hook does not disturb rendering
                    assert same_bits(prev[:, :3], plain.framebuffer_sum().reshape(-1, 3))
        assert checked == 9 and buckets[..., :3].max() > 0
        vprev, vmom = variance_images(ctx[15])                     # both trackers on: the variance is what it was
        assert same_bits(vprev, e.prev) and same_bits(vmom, e.mom)
        assert ctx[15].noise_stats(0.01) == e.noise_stats(0.01)
    finally:
        for b in list(ctx.values()) + [plain]:
            b.close()


# ---------------- the buffers calls on synthetic inputs ----------------
def synthetic_frames(n, K, seed=0):
    rng = np.random.default_rng(seed + n)
    f = (rng.gamma(0.7, 1.0, (K, n, 3)) * rng.uniform(0.1, 2.0, (1, n, 3))).astype(np.float32)
    f[rng.integers(0, K, 1 + n // 8), rng.integers(0, n, 1 + n // 8)] *= 300.0        # fireflies: the trim has work to do
    if n > 200:
        f[K - 2, 100, 1] = np.nan       # through the running sum: this bucket and the next of the pixel are dropped
        f[K - 1, 7, 0] = np.inf
    return f


def plant(buckets):
    """non-finite values written into the planes themselves, [M, n, 4]: ONE bucket of pixel 50, every bucket of pixel 60"""
    if buckets.shape[1] > 200:
        buckets[1, 50, 0] = float("inf")
        buckets[2, 50, 2] = float("nan")
        buckets[:, 60, 1] = float("inf")


@pytest.mark.parametrize("M", rl.ODD)
@pytest.mark.parametrize("n", COUNTS)
def test_update_resolve_and_stats_buffers_equal_the_emulation(n, M, small_grid):
    import torch
    K = M + 2
    frames = synthetic_frames(n, K)
    sums, eprev, ebuckets = rl.feed(frames, M)
    prev, buckets = torch.zeros(n, 4, device="cuda"), torch.zeros(M, n, 4, device="cuda")
    for k in range(1, K + 1):
        robust_update_tensors(torch.from_numpy(sums[k - 1]).cuda(), k, prev, buckets)
    assert same_bits(prev.cpu().numpy(), eprev) and same_bits(buckets.cpu().numpy(), ebuckets)
    plant(ebuckets)
    plant(buckets)
    out = robust_resolve_tensors(prev, buckets, K).cpu().numpy()
    ref, gini, trim, kept = rl.resolve(eprev, ebuckets, K, info=True)
    assert same_bits(out, ref) and (out[:, 3] == 1).all()
    if n > 200:
        assert kept[50] == M - 2 and kept[60] == 0 and kept[100] < M and kept[7] < M
        assert np.isfinite(out[[50, 60]]).all() and same_bits(out[60, :3], eprev[60, :3] / np.float32(K))
    st = robust_stats_tensors(prev, buckets, K)
    want = rl.stats(eprev, ebuckets, K, max_blocks=small_grid)
    assert st == want and np.float64(st["meanGini"]).tobytes() == np.float64(want["meanGini"]).tobytes()
    assert st == robust_stats_tensors(prev, buckets, K)                   # the same bits on every run
    assert st["nonFinite"] == (4 if n > 200 else 0) and st["pixels"] == n and st["buckets"] == M and st["iterations"] == K
    s64 = rl.stats64(eprev, ebuckets, K)
    assert (st["trimmed"], st["maxGini"]) == (s64["trimmed"], s64["maxGini"]) and abs(st["meanGini"] - s64["meanGini"]) <= 1e-13 * s64["meanGini"]
    assert M == 3 or n < 200 or st["trimmed"] > 0


@pytest.mark.parametrize("M", [5, ROBUST_DEFAULT_BUCKETS, 15])
def test_the_default_grid_equals_the_emulation_on_128x72(M):
    """36 workgroups, one lane per pixel, the second level with 36 of 256 lanes busy; k no multiple of M"""
    import torch
    n, K = 128 * 72, 2 * M + 3
    frames = synthetic_frames(n, K, seed=1)
    sums, eprev, ebuckets = rl.feed(frames, M)
    prev, buckets = torch.zeros(72, 128, 4, device="cuda"), torch.zeros(M, 72, 128, 4, device="cuda")
    for k in range(1, K + 1):
        robust_update_tensors(torch.from_numpy(sums[k - 1].reshape(72, 128, 3)).cuda(), k, prev, buckets)
    assert same_bits(buckets.cpu().numpy(), ebuckets)
    plant(ebuckets)
    plant(buckets.view(M, n, 4))
    out = torch.full((72, 128, 4), -1.0, device="cuda")
    assert robust_resolve_tensors(prev, buckets, K, out=out) is out
    assert same_bits(out.cpu().numpy(), rl.resolve(eprev, ebuckets, K))
    assert robust_stats_tensors(prev, buckets, K) == rl.stats(eprev, ebuckets, K)


def test_context_buffers_and_tensors_agree_on_a_side_stream():
    """vcm_track_robust is vcm_robust_update_buffers on the context's images: the frames of a context fed through the
    tensor calls on a non-default torch stream give the context's planes, estimate and statistics"""
    import torch
    sc = dl.box(3, 31, 23)
    M = 5
    b = backend(sc, ALGO_PATH_TRACE)
    side = torch.cuda.Stream()
    try:
        b.track_robust(M)
        with torch.cuda.stream(side):
            prev, buckets = torch.zeros(b.N, 4, device="cuda"), torch.zeros(M, b.N, 4, device="cuda")
            for it in range(M + 2):
                b.run_iteration(it, 0, 10)
                robust_update_tensors(torch.from_numpy(b.framebuffer_sum()).cuda(), it + 1, prev, buckets)
            out = robust_resolve_tensors(prev, buckets, M + 2)
            st = robust_stats_tensors(prev, buckets, M + 2)
            side.synchronize()
        cprev, cbuckets = images(b, M)
        assert same_bits(prev.cpu().numpy(), cprev) and same_bits(buckets.cpu().numpy(), cbuckets)
        assert same_bits(out.cpu().numpy()[:, :3], b.robust().reshape(-1, 3)) and st == b.robust_stats()
        # the buffers calls themselves, on the context's own planes
        dev = C.c_void_p()
        assert b.L.vcm_robust_device(b.ctx, C.byref(dev)) == 0
        b.synchronize()
        rs = RobustStats()
        assert b.L.vcm_robust_stats_buffers(0, b.N, prev.data_ptr(), buckets.data_ptr(), M + 2, M, C.byref(rs), None) == 0, b.L.vcm_last_error()
        assert rs.asdict() == st
    finally:
        b.close()


# ---------------- refusals and state ----------------
def test_refusals_of_a_context():
    sc = dl.box(1, 24, 18)
    b = backend(sc, ALGO_PATH_TRACE)
    try:
        L = b.L
        out = np.zeros((18, 24, 3), np.float32)
        st, dev = RobustStats(), C.c_void_p()
        # off: the readers say so
        for rc in (L.vcm_robust_resolve(b.ctx), L.vcm_read_robust(b.ctx, out.ctypes.data_as(_fp)), L.vcm_robust_device(b.ctx, C.byref(dev)),
                   L.vcm_get_robust_stats(b.ctx, C.byref(st))):
            assert rc == -1 and b"vcm_track_robust is off" in L.vcm_last_error()
        # bad bucket counts
        for M in (1, 2, 4, 16, 17, -1):
            assert L.vcm_track_robust(b.ctx, M) == -1 and b"odd, 3 .. 15" in L.vcm_last_error()
        b.run_iteration(0, 0, 10)
        # after an iteration
        assert L.vcm_track_robust(b.ctx, 3) == -1 and b"holds iterations" in L.vcm_last_error()
        assert L.vcm_track_robust(b.ctx, 0) == 0          # switching off is always allowed
        # ... but right after a clear
        b.clear_framebuffer()
        b.track_robust(3)
        eprev, ebuckets = rl.new_images(b.N, 3)
        for k in (1, 2):
            b.run_iteration(k, 0, 10)
            rl.update(b.framebuffer_sum(), k, eprev, ebuckets)
            # k < M
            for rc in (L.vcm_robust_resolve(b.ctx), L.vcm_read_robust(b.ctx, out.ctypes.data_as(_fp)), L.vcm_robust_device(b.ctx, C.byref(dev)),
                       L.vcm_get_robust_stats(b.ctx, C.byref(st))):
                assert rc == -1 and b"as many iterations as buckets" in L.vcm_last_error()
        b.run_iteration(3, 0, 10)
        rl.update(b.framebuffer_sum(), 3, eprev, ebuckets)
        prev, buckets = images(b, 3)
        assert same_bits(prev, eprev) and same_bits(buckets, ebuckets) and buckets.any()   # the count started over with the clear
        assert same_bits(b.robust().reshape(-1, 3), rl.resolve(eprev, ebuckets, 3)[:, :3])
        # a clear resets the images and the count
        b.clear_framebuffer()
        prev, buckets = images(b, 3)
        assert not prev.any() and not buckets.any()
        assert L.vcm_get_robust_stats(b.ctx, C.byref(st)) == -1 and b"as many iterations as buckets" in L.vcm_last_error()
        # another M after the clear: the planes are allocated anew and start at zero
        b.track_robust(5)
        prev, buckets = images(b, 5)
        assert buckets.shape[0] == 5 and not buckets.any()
    finally:
        b.close()


def test_a_sharded_context_is_refused_in_the_words_of_the_denoiser():
    sc = dl.box(1, 24, 18)
    b = backend(sc, rank=1, world=3)
    try:
        L = b.L
        pv, st = C.c_void_p(), RobustStats()
        buf = np.zeros((18, 24, 3), np.float32)
        for rc in (L.vcm_track_robust(b.ctx, 5), L.vcm_robust_resolve(b.ctx), L.vcm_robust_device(b.ctx, C.byref(pv)),
                   L.vcm_read_robust(b.ctx, buf.ctypes.data_as(_fp)), L.vcm_get_robust_stats(b.ctx, C.byref(st))):
            assert rc == -1
            assert b"sharded context: its framebuffer is a shard of the image" in L.vcm_last_error()
    finally:
        b.close()


def test_resolving_between_iterations_changes_nothing():
    """iterate -> resolve -> iterate -> resolve = a fresh context that only iterates"""
    sc = dl.box(1, 31, 23)
    a, b = backend(sc), backend(sc)
    try:
        a.track_robust(3)
        b.track_robust(3)
        seen = []
        for it in range(6):
            a.run_iteration(it, 0, 10)
            b.run_iteration(it, 0, 10)
            if it >= 2:
                seen.append((a.robust(), a.robust_stats()))   # a looks after every iteration, b only at the end
        pa, ba = images(a, 3)
        pb, bb = images(b, 3)
        assert same_bits(pa, pb) and same_bits(ba, bb)
        assert same_bits(seen[-1][0], b.robust()) and seen[-1][1] == b.robust_stats()
        assert [s[1]["iterations"] for s in seen] == [3, 4, 5, 6] and not same_bits(seen[0][0], seen[-1][0])
        assert same_bits(a.framebuffer_sum(), b.framebuffer_sum())
    finally:
        a.close()
        b.close()


# ---------------- hosts ----------------
def test_vcm_render_robust_equals_the_python_path(tmp_path):
    res, its = (40, 30), 9
    r = VertexCM(dl.desc5(dl.box(1, *res)), ALGO_PATH_TRACE, 0.003, 0.75, 1234)
    r.mMaxPathLength = 10
    r.backend.track_robust()              # the default M
    for it in range(its):
        r.RunIteration(it)
    frame, st, mean = r.GetRobust(), r.backend.robust_stats(), r.GetFramebuffer()
    r.close()
    assert st["buckets"] == ROBUST_DEFAULT_BUCKETS and st["iterations"] == its and not same_bits(frame, mean)
    out = str(tmp_path / "o.pfm")
    p = subprocess.run([VCM_RENDER, "-s", "1", "-a", "pt", "--res", str(res[0]), str(res[1]), "-i", str(its), "--robust", "-o", out, "--json"],
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-400:]
    assert json.loads(p.stdout.strip().splitlines()[-1])["robust"] == st
    with open(out, "rb") as f:
        assert f.readline() == b"PF\n" and f.readline() == b"%d %d\n" % res and f.readline() == b"-1\n"
        img = np.frombuffer(f.read(), np.float32).reshape(res[1], res[0], 3)
    assert same_bits(img, frame)
    # an explicit M, in words
    p = subprocess.run([VCM_RENDER, "-s", "1", "-a", "pt", "--res", "20", "14", "-i", "4", "--robust", "3"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "robust estimate after 4 iteration(s) in 3 buckets" in p.stdout, (p.stdout, p.stderr[-400:])


def test_vcm_render_refuses_robust_with_denoise_and_bad_bucket_counts():
    p = subprocess.run([VCM_RENDER, "-s", "1", "-a", "pt", "--res", "20", "14", "-i", "9", "--robust", "--denoise"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 2 and "--robust and --denoise do not combine" in p.stderr
    p = subprocess.run([VCM_RENDER, "-s", "1", "-a", "pt", "--res", "20", "14", "-i", "9", "--robust", "4"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 2 and "odd number of buckets" in p.stderr


# ---------------- the estimate as the denoiser's colour input ----------------
def test_the_resolved_image_feeds_vcm_denoise_buffers():
    import torch
    from smallvcm_amd.renderer import denoise_params
    sc = dl.box(1, 67, 45)
    M = 5
    b = backend(sc, ALGO_PATH_TRACE)
    try:
        b.track_robust(M)
        for it in range(M + 1):
            b.run_iteration(it, 0, 10)
        prev, buckets = images(b, M)
        color, albedo, guide = C.c_void_p(), C.c_void_p(), C.c_void_p()
        assert b.L.vcm_robust_device(b.ctx, C.byref(color)) == 0, b.L.vcm_last_error()
        assert b.L.vcm_features_device(b.ctx, C.byref(albedo), C.byref(guide)) == 0, b.L.vcm_last_error()
        b.synchronize()                  # the three images are written on the context's stream, the filter runs on torch's
        out = torch.zeros(45, 67, 4, device="cuda")
        p = denoise_params()
        assert b.L.vcm_denoise_buffers(0, 67, 45, color, albedo, guide, out.data_ptr(), C.byref(p),
                                       torch.cuda.current_stream().cuda_stream) == 0, b.L.vcm_last_error()
        got = out.cpu().numpy()
    finally:
        b.close()
    resolved = rl.resolve(prev, buckets, M + 1).reshape(45, 67, 4)
    assert (resolved[..., 3] == 1).all()                                  # the .w = 1 contract of a colour image
    g, a = dl.features(sc)
    assert same_bits(got, dl.denoise(resolved, a, g, dl.defaults()))
    assert not same_bits(got[..., :3], resolved[..., :3])
