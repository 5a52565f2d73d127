"""Per-pixel variance of the running mean, the noise statistic and render-to-target on the CPU: the functions of
smallvcm_amd/csrc/vcm_variance.h compiled for the host (tests/host_emul_variance) against float64 numpy restatements, and
the library's argument checks.  tests/test_gpu_variance.py holds the GPU to these bits."""
import ctypes as C
import os

import numpy as np
import pytest

import denoise_lib as dl
import variance_lib as vl
from smallvcm_amd._abi import ALGO_PATH_TRACE, ALGO_VCM, NoiseStats
from smallvcm_amd.renderer import load_library, render_until

HERE = os.path.dirname(os.path.abspath(__file__))
K = 64


# ---------------- accumulation against float64 ----------------
def sequences(kind, n=128):
    """K frames of n pixels: every pixel has mean 1 and its own sigma from 3e-3 to 1 (relative variance of the mean after
    64 iterations from 1.4e-7 to 1.6e-2: both sides of the 1e-6 the check starts at)"""
    rng = np.random.default_rng(7)
    if kind == "constant":
        return np.full((K, n, 3), 0.75, np.float32)   # k * 0.75 is exact in fp32 for every k <= 64
    sig = np.logspace(np.log10(3e-3), 0.0, n)[None, :, None]
    f = 1.0 + sig * rng.normal(size=(K, n, 3))
    if kind == "outlier":
        f[20, n // 2, 1] = 1e4
    return f.astype(np.float32)


@pytest.mark.parametrize("kind", ["constant", "gaussian", "outlier"])
def test_the_update_matches_float64_for_every_iteration_count(kind):
    """V of the emulation against the float64 restatement (the fp32 running sums taken as exact) after k = 2 .. 64
    updates: relative 1e-4 wherever the true relative variance of the mean is at least 1e-6"""
    frames = sequences(kind)
    prev, mom = vl.new_images(frames.shape[1])
    s = np.zeros(frames.shape[1:], np.float32)
    sums, checked = [], 0
    for k in range(1, K + 1):
        s = s + frames[k - 1]
        sums.append(s.copy())
        vl.update(s, k, prev, mom)
        assert np.array_equal(prev[:, :3], s) and not prev[:, 3].any() and not mom[:, 3].any()
        if k == 1:
            assert not mom.any()
            continue
        if kind == "constant":
            assert not mom.any(), k   # M2 = 0 exactly
            continue
        ref = vl.welford64(np.stack(sums)) / (k * (k - 1))
        rel = ref / (s.astype(np.float64) / k) ** 2
        mask = rel >= 1e-6
        V = vl.variance(mom, k).astype(np.float64)
        err = np.abs(V - ref)[mask] / ref[mask]
        assert err.max() <= 1e-4, (k, err.max())
        checked += int(mask.sum())
    if kind != "constant":
        assert checked > 0.5 * (K - 1) * frames[0].size
        assert (rel < 1e-6).any() and rel.max() > 1e-3   # the sequence reaches below the checked range and far above it


def test_a_nan_stays_in_its_pixel_and_is_counted():
    frames = sequences("gaussian", 67 * 5)[:8].copy()
    clean = vl.feed(frames)
    frames[3, 100, 2] = np.nan
    frames[5, 200, 0] = np.inf
    _, prev, mom = vl.feed(frames)
    bad = np.zeros(mom.shape, bool)
    bad[100, 2] = bad[200, 0] = True
    assert np.isnan(mom[bad]).all() and np.isfinite(mom[~bad]).all()
    assert np.array_equal(mom[~bad], clean[2][~bad])
    st, ref = vl.stats(prev, mom, 8, 0.001), vl.stats(clean[1], clean[2], 8, 0.001)
    assert st["nonFinite"] == 2 and ref["nonFinite"] == 0 and st["elements"] == ref["elements"] == 3 * 67 * 5
    assert np.isfinite(st["mean"]) and np.isfinite(st["max"])
    s64 = vl.stats64(prev, mom, 8, np.float32(0.001))
    assert (st["above"], st["max"]) == (s64["above"], s64["max"]) and abs(st["mean"] - s64["mean"]) <= 1e-13 * s64["mean"]


# ---------------- refusals ----------------
def test_fewer_than_two_iterations_are_refused_by_the_emulation():
    _, prev, mom = vl.feed(sequences("gaussian", 16)[:1])
    assert vl.stats(prev, mom, 1, check=False) is None
    assert vl.stats(prev, mom, 0, check=False) is None


def test_null_arguments_and_bad_sizes_are_refused_by_the_library():
    L = load_library(require_gpu=False)
    st = NoiseStats()
    one = C.c_void_p(16)   # never dereferenced: the checks come first
    assert L.vcm_track_variance(None, 1) == -1 and b"vcm_track_variance" in L.vcm_last_error()
    assert L.vcm_read_variance(None, None) == -1
    assert L.vcm_variance_device(None, None) == -1
    assert L.vcm_get_noise_stats(None, 0.0, C.byref(st)) == -1
    assert L.vcm_variance_update_buffers(0, 4, None, 1, one, one, None) == -1 and b"NULL" in L.vcm_last_error()
    assert L.vcm_variance_update_buffers(0, 4, one, 0, one, C.c_void_p(32), None) == -1 and b"from 1" in L.vcm_last_error()
    assert L.vcm_variance_update_buffers(0, 4, one, 1, one, one, None) == -1 and b"differ" in L.vcm_last_error()
    assert L.vcm_variance_update_buffers(0, 0, C.c_void_p(48), 1, one, C.c_void_p(32), None) == -1 and b"bad size" in L.vcm_last_error()
    assert L.vcm_noise_stats_buffers(0, 4, one, C.c_void_p(32), 1, 0.0, C.byref(st), None) == -1 and b"two iterations" in L.vcm_last_error()
    assert L.vcm_noise_stats_buffers(0, 4, one, C.c_void_p(32), 2, 0.0, None, None) == -1


# ---------------- the statistic ----------------
@pytest.mark.parametrize("shape", [(1, 1), (3, 2), (67, 45)])
def test_stats_match_numpy_and_repeat_bit_for_bit(shape):
    n = shape[0] * shape[1]
    rng = np.random.default_rng(n)
    frames = (rng.gamma(2.0, 0.5, (6, n, 3)) * rng.uniform(0.0, 2.0, (1, n, 3))).astype(np.float32)
    _, prev, mom = vl.feed(frames)
    ref = vl.stats64(prev, mom, 6)
    thr = np.float32(ref["mean"])   # about half of the elements lie above it
    ref = vl.stats64(prev, mom, 6, thr)
    for cap in (vl.DEFAULT_MAX_BLOCKS, 3, 1):   # one lane per pixel; the grid-stride path and partial second level
        a, b = vl.stats(prev, mom, 6, thr, cap), vl.stats(prev, mom, 6, thr, cap)
        assert a == b and np.float64(a["mean"]).tobytes() == np.float64(b["mean"]).tobytes()
        assert a["iterations"] == 6 and a["elements"] == 3 * n and a["nonFinite"] == 0
        assert a["above"] == ref["above"] and a["max"] == ref["max"]
        assert abs(a["mean"] - ref["mean"]) <= 1e-13 * ref["mean"]   # binary64 sums of <= 9045 terms in two orders
    assert n == 1 or 0 < ref["above"] < 3 * n


def test_the_statistic_is_v_over_mean_squared_plus_a_hundredth():
    """one pixel, by hand: samples 1, 3 -> mean 2, M2 = 2, V = 1, noise = 1 / 4.01"""
    _, prev, mom = vl.feed(np.array([[[1.0, 1.0, 1.0]], [[3.0, 1.0, 0.0]]], np.float32))
    assert mom[0].tolist() == [2.0, 0.0, 0.5, 0.0] and prev[0].tolist() == [4.0, 2.0, 1.0, 0.0]
    assert vl.variance(mom, 2)[0].tolist() == [1.0, 0.0, 0.25]
    st = vl.stats(prev, mom, 2, 0.5)
    assert st["max"] == float(np.float32(0.25) / (np.float32(0.25) + np.float32(0.01)))
    assert st["above"] == 1 and abs(st["mean"] - (1 / 4.01 + 0.0 + 0.25 / 0.26) / 3) < 1e-7


# ---------------- the statistic predicts the error ----------------
# stats.mean over the measured (img - ref)^2 / (ref^2 + 0.01) against the 1000-iteration goldens, 64 x 64, 16 iterations,
# seeds 11 .. 88: the eight ratios per case as MEASURED on the emulation (DESIGN.md "Variance").  Asserted: every ratio in
# [min / 1.5, max * 1.5] of its case.  The variant that forgets the division by k reports 16 times as much; the test
# shows that this lies outside the interval.  Scene 1 under path tracing is NOT evidence of prediction: its ratios say the
# statistic is thirty times too small there (fireflies; DESIGN.md "Variance" has the reason).  Its interval is a pin of
# that known behaviour which still tells V from k V; a remedy (a statistic normalised by a filtered mean) will have to
# move it.
SEEDS = (11, 22, 33, 44, 55, 66, 77, 88)
PREDICTS = [(1, "pt", ALGO_PATH_TRACE, 0.029, 0.043), (3, "pt", ALGO_PATH_TRACE, 0.899, 0.961), (3, "vcm", ALGO_VCM, 0.931, 0.987)]


@pytest.mark.parametrize("scene_id,name,algo,lo,hi", PREDICTS)
def test_the_statistic_predicts_the_measured_error(scene_id, name, algo, lo, hi):
    ref = np.load(os.path.join(HERE, "golden", "denoise_ref_s%d_%s_64_1000.npy" % (scene_id, name)))
    sc = dl.box(scene_id, 64, 64)
    assert hi * 1.5 < 16 * lo / 1.5   # the interval tells the two apart at all
    for seed in SEEDS:
        r = vl.TrackedEmul(sc, algo, seed).run(16)
        st = r.noise_stats()
        err = dl.rel_mse(r.emul.mean(), ref)
        ratio = st["mean"] / err
        print("scene %d %s seed %d: stats.mean %.5f, measured error %.5f, ratio %.3f" % (scene_id, name, seed, st["mean"], err, ratio))
        assert lo / 1.5 <= ratio <= hi * 1.5
        assert not lo / 1.5 <= 16 * ratio <= hi * 1.5   # V = M2 / (k - 1): the variance of a sample, not of the mean


# ---------------- render to a target ----------------
def test_render_until_stops_at_the_first_check_at_or_below_the_target():
    sc = dl.box(1, 20, 14)
    probe = vl.TrackedEmul(sc, ALGO_PATH_TRACE).run(12)
    means = {}
    full = vl.TrackedEmul(sc, ALGO_PATH_TRACE)
    for k in range(1, 13):
        full.run(1)
        if k >= 2:
            means[k] = full.noise_stats()["mean"]
    assert means[12] == probe.noise_stats()["mean"] and means[12] < means[4]   # the noise falls
    target = means[8]                                # reached at the second look of check_every = 4
    assert means[4] > target
    r = vl.TrackedEmul(sc, ALGO_PATH_TRACE)
    hist = render_until(r, target, check_every=4, max_iterations=100)
    assert r.mIterations == 8 and [h["iterations"] for h in hist] == [4, 8]
    assert [h["mean"] for h in hist] == [means[4], means[8]]
    assert hist[-1]["above"] == vl.stats64(r.prev, r.mom, 8, np.float32(target))["above"]


def test_render_until_never_exceeds_the_maximum_and_a_zero_target_runs_to_it():
    sc = dl.box(1, 20, 14)
    r = vl.TrackedEmul(sc, ALGO_PATH_TRACE)
    hist = render_until(r, 0.0, check_every=3, max_iterations=7)
    assert r.mIterations == 7 and [h["iterations"] for h in hist] == [3, 6, 7]
    r = vl.TrackedEmul(sc, ALGO_PATH_TRACE)
    hist = render_until(r, 1e9, check_every=1, max_iterations=7)   # never looked at before the second iteration
    assert r.mIterations == 2 and [h["iterations"] for h in hist] == [2]
    with pytest.raises(ValueError):
        render_until(r, 0.1, check_every=0)


# ---------------- the variance-guided filter ----------------
RNG = np.random.default_rng(11)
SIGMA2_B3 = (2 * 0.0625 ** 2 + 2 * 0.25 ** 2 + 0.375 ** 2) ** 2   # sum h^2 / (sum h)^2 of the 5 x 5 B3 kernel (sum h = 1)


def mom_of(total_per_channel, shape, k=2):
    """a moments image whose every channel has variance of the mean `total_per_channel` after k iterations"""
    m = np.zeros(shape[:2] + (4,), np.float32)
    m[..., :3] = np.float32(total_per_channel) / np.float32(vl.var_factor_mean(k))
    return m


def guided(color, a, g, mom, k=2, **kw):
    return vl.denoise2(color, a, g, mom, vl.var_factor_mean(k), vl.params2(varianceGuided=1, **kw))


def soft_guides(H, W, rng):
    """one gently curved surface: every tap keeps a positive weight"""
    g = np.zeros((H, W, 4), np.float32)
    n = np.concatenate([0.1 * rng.normal(size=(H, W, 2)), np.ones((H, W, 1))], axis=2)
    g[..., :3] = n / np.linalg.norm(n, axis=2, keepdims=True)
    g[..., 3] = rng.uniform(1.0, 1.05, (H, W))
    a = np.ones((H, W, 4), np.float32)
    a[..., :3] = rng.uniform(0.2, 1.0, (H, W, 3))
    return g, a


def test_unguided_params2_equal_emul_denoise_bit_for_bit():
    g, a = soft_guides(23, 31, RNG)
    c = dl.as4(RNG.gamma(2.0, 0.5, (23, 31, 3)).astype(np.float32))
    mom = mom_of(0.01, c.shape)
    for passes, dem in ((0, 1), (1, 0), (3, 1), (5, 1)):
        ref = dl.denoise(c, a, g, dl.params(passes=passes, demodulate=dem))
        out = vl.denoise2(c, a, g, mom, 0.5, vl.params2(passes=passes, demodulate=dem, varianceGuided=0, sigmaVariance=3.0))
        assert out.tobytes() == ref.tobytes()
    fb = c[..., :3].copy()
    assert vl.denoise2(fb, a, g, mom, 0.5, vl.params2(varianceGuided=0), scale=0.25).tobytes() == dl.denoise(fb, a, g, dl.defaults(), scale=0.25).tobytes()


def test_defaults2_are_the_defaults_with_the_tuned_guidance():
    p, q = dl.defaults(), vl.params2()
    assert (q.passes, q.sigmaColor, q.sigmaNormal, q.sigmaDepth, q.demodulate) == (p.passes, p.sigmaColor, p.sigmaNormal, p.sigmaDepth, p.demodulate)
    assert q.varianceGuided == 1 and q.sigmaVariance == 4.0   # DESIGN.md "Variance": the sweep of tests/variance_tune.py


def test_guided_refusals():
    from smallvcm_amd._abi import DenoiseParams2
    L = load_library(require_gpu=False)
    L.vcm_denoise_buffers2.argtypes = [C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 4 + [C.c_int, C.c_void_p, C.POINTER(DenoiseParams2), C.c_void_p]
    one, two, three, four, five = (C.c_void_p(16 * i) for i in range(1, 6))
    p = vl.params2(varianceGuided=1)
    assert L.vcm_denoise_buffers2(0, 4, 4, one, two, three, four, 1, five, C.byref(p), None) == -1 and b"two iterations" in L.vcm_last_error()
    assert L.vcm_denoise_buffers2(0, 4, 4, one, two, three, None, 2, five, C.byref(p), None) == -1 and b"NULL" in L.vcm_last_error()
    assert L.vcm_denoise_buffers2(0, 4, 4, one, two, three, four, 2, four, C.byref(p), None) == -1 and b"one of the inputs" in L.vcm_last_error()
    assert L.vcm_denoise2(None, 1.0, C.byref(p)) == -1
    g, a = dl.flat_guides(4, 4)
    for bad in (dict(sigmaVariance=0.0), dict(sigmaVariance=float("nan")), dict(varianceGuided=2), dict(passes=13)):
        q = vl.params2(**bad)
        assert L.vcm_denoise_buffers2(0, 4, 4, one, two, three, four, 2, five, C.byref(q), None) == -1
        assert vl.denoise2(np.ones((4, 4, 4), np.float32), a, g, np.zeros((4, 4, 4), np.float32), 0.5, q, check=False) is None


@pytest.mark.parametrize("value", [0.0, 0.3, 7.0])
def test_a_constant_image_without_variance_returns_bit_for_bit(value):
    g, a = soft_guides(17, 29, RNG)
    c = np.full((17, 29, 4), value, np.float32)
    out = guided(c, a, g, np.zeros((17, 29, 4), np.float32), demodulate=0)
    assert out[..., :3].tobytes() == c[..., :3].tobytes() and not out[..., 3].any()


def half_planes(lo, hi, sigma, H=48, W=64, seed=3):
    rng = np.random.default_rng(seed)
    c = np.ones((H, W, 4), np.float32)
    c[:, :W // 2, :3] = lo
    c[:, W // 2:, :3] = hi
    c[..., :3] += (sigma * rng.normal(size=(H, W, 3))).astype(np.float32)
    g, a = dl.flat_guides(H, W)
    return c, a, g, mom_of(sigma ** 2, c.shape)


def test_a_step_above_the_noise_stays_a_step_and_the_fixed_stop_blurs_it():
    """means 1 | 2 with noise 0.05 on one flat surface: the guides see no edge, only the colour stop can keep it"""
    sigma = 0.05
    c, a, g, mom = half_planes(1.0, 2.0, sigma)
    W = c.shape[1]
    out = guided(c, a, g, mom, demodulate=0)[..., :3].astype(np.float64)
    fixed = dl.denoise(c, a, g, dl.params(demodulate=0))[..., :3].astype(np.float64)   # sigmaColor = the tuned 16
    leak = max(abs(out[:, W // 2 - 1].mean() - 1.0), abs(out[:, W // 2].mean() - 2.0))
    leak_fixed = max(abs(fixed[:, W // 2 - 1].mean() - 1.0), abs(fixed[:, W // 2].mean() - 2.0))
    print("leak across the edge: guided %.4f, fixed stop %.4f (noise %.2f)" % (leak, leak_fixed, sigma))
    assert leak < sigma                       # below the noise
    assert leak_fixed > 4 * sigma             # the fixed stop at 16 sees a difference of 1 as nothing
    assert out[:, :W // 2 - 2].std() < sigma / 2 and out[:, W // 2 + 2:].std() < sigma / 2   # and the sides are smoothed


def test_noise_on_equal_means_is_smoothed():
    sigma = 0.5
    c, a, g, mom = half_planes(1.0, 1.0, sigma)
    out = guided(c, a, g, mom, demodulate=0)[..., :3].astype(np.float64)
    print("std in %.3f -> out %.3f" % (c[..., :3].std(), out.std()))
    assert out.std() < sigma / 4 and abs(out.mean() - c[..., :3].mean()) < 0.02


def test_one_pass_propagates_the_variance_of_a_b3_mean():
    """White noise of per-channel variance s^2 on a flat surface, one pass with a colour stop so wide that every weight is
    h (sigmaVariance 1000: x_c <= 25 s^2 6 / (1e6 3 s^2) = 5e-5, weights within 5e-5 of h): .w goes from 3 s^2 to
    3 s^2 sum h^2 / (sum h)^2 in the interior, to a relative 2e-4 (four weights' worth).  The image's own variance must
    agree within sampling error: N interior values per channel, neighbours correlated over about 1 / sum h^2 = 13.4 pixels,
    so N_eff = 3 N sum h^2 and the relative standard error of a variance estimate is sqrt(2 / N_eff); asserted at four of
    them."""
    s, H, W = 0.2, 96, 128
    c, a, g, mom = half_planes(1.0, 1.0, s, H, W, seed=5)
    out = guided(c, a, g, mom, passes=1, demodulate=0, sigmaVariance=1000.0)
    inner = out[2:-2, 2:-2]
    want = 3 * s * s * SIGMA2_B3
    assert np.abs(inner[..., 3] / want - 1).max() < 2e-4
    n_eff = 3 * inner[..., 0].size * SIGMA2_B3
    se = (2.0 / n_eff) ** 0.5
    measured = 3 * inner[..., :3].astype(np.float64).var()
    print("propagated %.6f, closed form %.6f, measured %.6f (relative s.e. %.3f)" % (inner[..., 3].mean(), want, measured, se))
    assert abs(measured / want - 1) < 4 * se


def guided64(c, a, g, mom, var_factor, p):
    """float64 numpy restatement of the guided filter (demodulation included)"""
    H, W = c.shape[:2]
    c, a, g = c.astype(np.float64), a.astype(np.float64), g.astype(np.float64)
    b3 = [0.0625, 0.25, 0.375, 0.25, 0.0625]
    g3 = [0.25, 0.5, 0.25]
    img = np.zeros((H, W, 4))
    al = a[..., :3] if p.demodulate else np.ones((H, W, 3))
    img[..., :3] = c[..., :3] / al
    img[..., 3] = (mom[..., :3].reshape(H, W, 3).astype(np.float64) * np.float64(np.float32(var_factor)) / al ** 2).sum(axis=2)
    for i in range(p.passes):
        step, out = 1 << i, img.copy()
        for y in range(H):
            for x in range(W):
                sv = sn = 0.0
                for j in range(3):
                    for k in range(3):
                        yq, xq = y + j - 1, x + k - 1
                        if 0 <= yq < H and 0 <= xq < W:
                            sv += g3[j] * g3[k] * img[yq, xq, 3]
                            sn += g3[j] * g3[k]
                inv = 1.0 / (p.sigmaVariance ** 2 * max(sv / sn, 0.0) + 1e-10)
                acc, aw, av = np.zeros(3), 0.0, 0.0
                for j in range(5):
                    for k in range(5):
                        yq, xq = y + (j - 2) * step, x + (k - 2) * step
                        if not (0 <= yq < H and 0 <= xq < W):
                            continue
                        d = float(g[y, x, :3] @ g[yq, xq, :3])
                        if d <= 0:
                            continue
                        t = abs(g[y, x, 3] - g[yq, xq, 3]) / (p.sigmaDepth * max(g[y, x, 3], g[yq, xq, 3]))
                        diff = img[yq, xq, :3] - img[y, x, :3]
                        w = b3[j] * b3[k] * d ** p.sigmaNormal / ((1 + 0.25 * (diff @ diff) * inv) * (1 + 0.25 * t * t)) ** 4
                        acc, aw, av = acc + w * diff, aw + w, av + w * w * img[yq, xq, 3]
                out[y, x, :3] = img[y, x, :3] + acc / aw
                out[y, x, 3] = av / aw ** 2
        img = out
    if p.demodulate and p.passes > 0:
        img[..., :3] *= a[..., :3]
    return img


@pytest.mark.parametrize("shape,passes", [((2, 3), 1), ((2, 3), 3), ((5, 7), 4), ((9, 6), 2)])
def test_small_odd_and_overstepped_frames_against_numpy(shape, passes):
    H, W = shape
    rng = np.random.default_rng(H * 100 + W + passes)
    g, a = soft_guides(H, W, rng)
    c = dl.as4(rng.uniform(0.2, 1.5, (H, W, 3)).astype(np.float32))
    mom = np.zeros((H, W, 4), np.float32)
    mom[..., :3] = rng.uniform(0.001, 0.05, (H, W, 3))
    p = vl.params2(varianceGuided=1, passes=passes, sigmaVariance=2.0)
    out = vl.denoise2(c, a, g, mom, vl.var_factor_mean(3), p)
    ref = guided64(c, a, g, mom, vl.var_factor_mean(3), p)
    assert np.abs(out[..., :3] - ref[..., :3]).max() < 2e-5 * np.abs(ref[..., :3]).max()
    assert np.abs(out[..., 3] / ref[..., 3] - 1).max() < 1e-4


def test_a_non_finite_variance_falls_back_and_spreads_nowhere():
    """the pixel and its eight neighbours (whose 3 x 3 holds it) filter with the fixed stop, no tap takes the value, and
    what lies beyond the two passes' reach (2 + 4 taps, + 1 for the 3 x 3) is the clean run, bit for bit"""
    c, a, g, mom = half_planes(1.0, 1.0, 0.1, 24, 32)
    clean = guided(c, a, g, mom, passes=2, demodulate=0)
    mom[10, 10, 1] = np.nan
    out = guided(c, a, g, mom, passes=2, demodulate=0)
    assert np.isfinite(out).all()
    far = np.ones((24, 32), bool)
    far[10 - 7:10 + 8, 10 - 7:10 + 8] = False
    assert out[far].tobytes() == clean[far].tobytes() and out[~far].tobytes() != clean[~far].tobytes()


# ---------------- guidance helps ----------------
# relMSE(vcm_denoise_defaults: the parent's filter) / relMSE(vcm_denoise_defaults2: guided, sigmaVariance 4) against the
# 1000-iteration goldens, 64 x 64, 4 iterations, means over seeds 11 .. 44.  MEASURED on the emulation (DESIGN.md
# "Variance"): all three exceed 1; asserted: the geometric mean of 1 and the measured ratio.
GUIDANCE_HELPS = [(1, "pt", ALGO_PATH_TRACE, 1.835), (3, "pt", ALGO_PATH_TRACE, 1.979), (3, "vcm", ALGO_VCM, 2.075)]


@pytest.mark.parametrize("scene_id,name,algo,measured", GUIDANCE_HELPS)
def test_the_guided_defaults_beat_the_fixed_stop(scene_id, name, algo, measured):
    ref = np.load(os.path.join(HERE, "golden", "denoise_ref_s%d_%s_64_1000.npy" % (scene_id, name)))
    sc = dl.box(scene_id, 64, 64)
    g, a = dl.features(sc)
    fixed, guided_mse = [], []
    for seed in (11, 22, 33, 44):
        r = vl.TrackedEmul(sc, algo, seed).run(4)
        fb = r.framebuffer()
        fixed.append(dl.rel_mse(dl.denoise(fb, a, g, dl.defaults(), scale=0.25), ref))
        guided_mse.append(dl.rel_mse(vl.denoise2(fb, a, g, r.mom, vl.var_factor_context(0.25, 4), vl.params2(), scale=0.25), ref))
    ratio = float(np.mean(fixed) / np.mean(guided_mse))
    print("scene %d %s: relMSE fixed / guided = %.3f (recorded %.3f, bound %.3f)" % (scene_id, name, ratio, measured, measured ** 0.5))
    assert measured > 1 and ratio >= measured ** 0.5
