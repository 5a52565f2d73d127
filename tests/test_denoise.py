"""Feature buffers and the edge-avoiding denoiser on the CPU: the functions of smallvcm_amd/csrc/vcm_denoise.h compiled
for the host (tests/host_emul_denoise), and the library's argument checks.  tests/test_gpu_denoise.py holds the GPU to
these bits."""
import ctypes as C
import os

import numpy as np
import pytest

import denoise_lib as dl
from smallvcm_amd._abi import ALGO_PATH_TRACE, ALGO_VCM
from smallvcm_amd.renderer import load_library

HERE = os.path.dirname(os.path.abspath(__file__))
RNG = np.random.default_rng(5)


def ulp_diff(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    return int(np.abs(ia - ib).max())


def random_guides(H, W, rng, misses=True):
    g = np.zeros((H, W, 4), np.float32)
    n = rng.normal(size=(H, W, 3))
    g[..., :3] = n / np.linalg.norm(n, axis=2, keepdims=True)
    g[..., 3] = rng.uniform(0.5, 5.0, (H, W))
    if misses:
        g[rng.uniform(size=(H, W)) < 0.2] = 0.0
    a = np.ones((H, W, 4), np.float32)
    a[..., :3] = rng.uniform(0.05, 1.0, (H, W, 3))
    return g, a


# ---------------- input checks ----------------
def test_defaults_are_the_tuned_set():
    p = dl.defaults()
    assert (p.passes, p.demodulate) == (5, 1)
    assert (p.sigmaColor, p.sigmaNormal, p.sigmaDepth) == (16.0, 32.0, np.float32(0.05))   # DESIGN.md "Denoising": the sweep's winner


@pytest.mark.parametrize("bad", [dict(passes=-1), dict(passes=13), dict(sigmaColor=0.0), dict(sigmaColor=-1.0),
                                 dict(sigmaNormal=float("nan")), dict(sigmaDepth=float("inf")), dict(sigmaDepth=0.0)])
def test_bad_parameters_are_refused_by_library_and_emulation(bad):
    L = load_library(require_gpu=False)
    L.vcm_denoise_buffers.restype = C.c_int
    p = dl.params(**bad)
    one = C.c_void_p(16), C.c_void_p(32), C.c_void_p(48), C.c_void_p(64)   # never dereferenced: the checks come first
    assert L.vcm_denoise_buffers(0, 4, 4, one[0], one[1], one[2], one[3], C.byref(p), None) == -1
    assert b"vcm_denoise_buffers" in L.vcm_last_error()
    g, a = dl.flat_guides(4, 4)
    assert dl.denoise(np.ones((4, 4, 4), np.float32), a, g, p, check=False) is None


def test_null_aliased_and_empty_buffers_are_refused():
    L = load_library(require_gpu=False)
    p = dl.defaults()
    a, b, c, d = C.c_void_p(16), C.c_void_p(32), C.c_void_p(48), C.c_void_p(64)
    for args in [(None, b, c, d), (a, None, c, d), (a, b, None, d), (a, b, c, None),      # NULL images
                 (a, b, c, a), (a, b, c, b), (a, b, c, c)]:                               # outDev is an input
        assert L.vcm_denoise_buffers(0, 4, 4, args[0], args[1], args[2], args[3], C.byref(p), None) == -1
        assert L.vcm_last_error()
    assert L.vcm_denoise_buffers(0, 0, 4, a, b, c, d, C.byref(p), None) == -1
    assert L.vcm_denoise_buffers(0, 4, -1, a, b, c, d, C.byref(p), None) == -1
    assert L.vcm_denoise_buffers(0, 4, 4, a, b, c, d, None, None) == -1
    # a NULL context: every context call (tests/test_abi.py walks the header for the same)
    pv = C.c_void_p()
    assert L.vcm_render_features(None) == -1 and L.vcm_read_feature(None, 0, None) == -1
    assert L.vcm_denoise(None, 1.0, C.byref(p)) == -1 and L.vcm_read_denoised(None, None) == -1
    assert L.vcm_denoised_device(None, C.byref(pv)) == -1 and L.vcm_read_denoised_image(None, 0, 2.2, None) == -1


# ---------------- identity and exactness ----------------
def test_zero_passes_return_the_input_bit_for_bit():
    g, a = random_guides(9, 13, RNG)
    c = RNG.uniform(0, 3, (9, 13, 4)).astype(np.float32)
    for demod in (0, 1):
        out = dl.denoise(c, a, g, dl.params(passes=0, demodulate=demod))
        assert out.tobytes() == c.tobytes()


@pytest.mark.parametrize("value", [0.0, 1.0, 0.3137, 1234.5])
def test_a_constant_image_returns_itself_whatever_the_guides(value):
    g, a = random_guides(37, 29, RNG)
    c = np.full((37, 29, 4), value, np.float32)
    c[..., 3] = 1.0
    out = dl.denoise(c, a, g, dl.params(demodulate=0))
    assert ulp_diff(out[..., :3], c[..., :3]) <= 4
    flat = np.ones_like(a) * np.float32(0.37)
    flat[..., 3] = 1.0
    out = dl.denoise(c, flat, g, dl.params(demodulate=1))   # a uniform albedo divided out and multiplied back
    assert ulp_diff(out[..., :3], c[..., :3]) <= 4


def test_albedo_times_constant_survives_with_demodulation_and_blurs_without():
    H, W = 32, 32
    g, _ = dl.flat_guides(H, W)
    a = np.ones((H, W, 4), np.float32)
    yy, xx = np.mgrid[0:H, 0:W]
    a[..., :3] = np.where(((xx // 2 + yy // 2) % 2 == 0)[..., None], 0.9, 0.2)   # a checkerboard texture
    c = a.copy()
    c[..., :3] *= np.float32(0.7)
    out = dl.denoise(c, a, g, dl.params(demodulate=1))
    assert np.max(np.abs(out[..., :3] - c[..., :3]) / c[..., :3]) <= 1e-6
    blurred = dl.denoise(c, a, g, dl.params(demodulate=0))
    contrast_in = c[..., 0].max() - c[..., 0].min()
    contrast_out = blurred[8:24, 8:24, 0].max() - blurred[8:24, 8:24, 0].min()
    print("texture contrast %.4f -> %.4f without demodulation" % (contrast_in, contrast_out))
    assert contrast_out < 0.5 * contrast_in   # the texture visibly blurs


# ---------------- edges ----------------
def two_halves(H, W, lo=0.25, hi=2.0):
    c = np.ones((H, W, 4), np.float32)
    c[:, :W // 2, :3] = lo
    c[:, W // 2:, :3] = hi
    return c


def test_perpendicular_normals_keep_two_constants_exactly():
    H, W = 24, 40
    g, a = dl.flat_guides(H, W)
    g[:, W // 2:, :3] = (1.0, 0.0, 0.0)
    c = two_halves(H, W)
    for sc in (16.0, 1e6):   # also where the colour weight stops nothing
        out = dl.denoise(c, a, g, dl.params(sigmaColor=sc, demodulate=0))
        assert out[..., :3].tobytes() == c[..., :3].tobytes()


def test_a_hit_miss_boundary_keeps_two_constants_exactly():
    H, W = 24, 40
    g, a = dl.flat_guides(H, W)
    g[:, W // 2:] = 0.0   # a miss: normal 0, depth 0
    c = two_halves(H, W)
    out = dl.denoise(c, a, g, dl.params(sigmaColor=1e6, demodulate=0))
    assert out[..., :3].tobytes() == c[..., :3].tobytes()


def test_a_depth_step_of_two_leaks_less_than_a_thousandth_of_the_contrast():
    H, W = 48, 64
    g, a = dl.flat_guides(H, W, depth=1.0)
    g[:, W // 2:, 3] = 2.0
    c = two_halves(H, W, 0.0, 1.0)
    out = dl.denoise(c, a, g, dl.defaults())
    leak = float(np.abs(out[..., :3] - c[..., :3]).max())   # contrast 1
    print("leak across a 2x depth step at default sigmas: %.3e of the contrast" % leak)
    assert leak < 1e-3


# ---------------- robustness and geometry ----------------
@pytest.mark.parametrize("bad", [float("nan"), float("inf"), -float("inf")])
def test_a_non_finite_pixel_spreads_to_no_neighbour(bad):
    H, W = 20, 21
    g, a = dl.flat_guides(H, W)
    c = RNG.uniform(0.2, 1.0, (H, W, 4)).astype(np.float32)
    c[7, 9, 1] = bad
    for demod in (0, 1):
        out = dl.denoise(c, a, g, dl.params(demodulate=demod))
        mask = np.ones((H, W), bool)
        mask[7, 9] = False
        assert np.isfinite(out[mask]).all()
        assert not np.isfinite(out[7, 9, 1])   # the centre passes through
        clean = c.copy()
        clean[7, 9, :3] = 0.5
        assert np.abs(out[mask] - dl.denoise(clean, a, g, dl.params(demodulate=demod))[mask]).max() < 0.5   # and pulls nothing along


@pytest.mark.parametrize("shape,passes", [((2, 3), 5), ((45, 67), 5), ((5, 7), 12), ((45, 67), 8)])
def test_small_odd_and_overstepped_frames(shape, passes):
    """smaller than a tile, not a multiple of the tile, passes whose step exceeds the frame: against a plain numpy
    restatement of the filter (float64, the same weights)"""
    H, W = shape
    rng = np.random.default_rng(H * 100 + W)
    g, a = random_guides(H, W, rng)
    c = rng.uniform(0, 2, (H, W, 4)).astype(np.float32)
    p = dl.params(passes=passes, demodulate=1, sigmaNormal=4.0)
    out = dl.denoise(c, a, g, p)
    ref = numpy_atrous(c, a, g, p)
    assert np.isfinite(out).all()
    assert np.abs(out[..., :3] - ref).max() <= 2e-4 * max(1.0, float(np.abs(ref).max()))


def numpy_atrous(c, a, g, p):
    """the issue's filter in float64, pixel by pixel (slow; small frames only)"""
    H, W = c.shape[:2]
    k = np.array([1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16])
    cur = c[..., :3].astype(np.float64)
    if p.demodulate:
        cur = cur / a[..., :3]
    n, z = g[..., :3].astype(np.float64), g[..., 3].astype(np.float64)
    f = lambda x: 1.0 / (1.0 + x / 4.0) ** 4
    for i in range(p.passes):
        step, sc = 1 << i, p.sigmaColor / (1 << i)
        nxt = cur.copy()
        for y in range(H):
            for x in range(W):
                ws, acc = 0.0, np.zeros(3)
                for j in range(5):
                    yq = y + (j - 2) * step
                    if not 0 <= yq < H:
                        continue
                    for ii in range(5):
                        xq = x + (ii - 2) * step
                        if not 0 <= xq < W:
                            continue
                        w = k[j] * k[ii]
                        if (z[y, x] == 0) != (z[yq, xq] == 0):
                            continue
                        if z[y, x] != 0:
                            d = float(n[y, x] @ n[yq, xq])
                            if d <= 0:
                                continue
                            w *= d ** p.sigmaNormal * f((abs(z[y, x] - z[yq, xq]) / (p.sigmaDepth * max(z[y, x], z[yq, xq]))) ** 2)
                        w *= f(float(((cur[yq, xq] - cur[y, x]) ** 2).sum()) / sc ** 2)
                        ws += w
                        acc += w * cur[yq, xq]
                nxt[y, x] = acc / ws
        cur = nxt
    return cur * a[..., :3] if p.demodulate else cur


# ---------------- features of the built-in boxes against geometry worked out here ----------------
BOX = dict(x0=-1.27029, x1=1.28975, y0=-1.25549, y1=1.30455, z0=-1.28002, z1=1.28002)   # scene.hxx:213-222
BIG_SPHERE = ((0.5 * (BOX["x0"] + BOX["x1"]), 0.5 * (BOX["y0"] + BOX["y1"]), BOX["z0"] + 0.8), 0.8)   # scene.hxx:292-301


def pixel_rays(scene):
    """origin and float64 directions through the pixel centres (camera.hxx:108-117)"""
    cam = scene.camera
    W, H = int(cam.resolution[0]), int(cam.resolution[1])
    m = np.array(list(cam.rasterToWorld), np.float64).reshape(4, 4).T   # column-major storage
    yy, xx = np.mgrid[0:H, 0:W]
    v = np.stack([xx + 0.5, yy + 0.5, np.zeros_like(xx, float), np.ones_like(xx, float)], axis=-1) @ m.T
    world = v[..., :3] / v[..., 3:]
    org = np.array(list(cam.position), np.float64)
    d = world - org
    return org, d / np.linalg.norm(d, axis=-1, keepdims=True)


def plane_hits(org, d, spheres=()):
    """per pixel: (name of the nearest of the box's five walls and the spheres, its distance, the margin to the second)"""
    H, W = d.shape[:2]
    ts = {}
    walls = {"back": (1, BOX["y1"]), "floor": (2, BOX["z0"]), "ceiling": (2, BOX["z1"]), "left": (0, BOX["x0"]), "right": (0, BOX["x1"])}
    lo = np.array([BOX["x0"], BOX["y0"], BOX["z0"]]); hi = np.array([BOX["x1"], BOX["y1"], BOX["z1"]])
    for name, (axis, val) in walls.items():
        with np.errstate(divide="ignore", invalid="ignore"):
            t = (val - org[axis]) / d[..., axis]
        p = org + t[..., None] * d
        ok = (t > 0)
        for k in range(3):
            if k != axis:
                ok &= (p[..., k] > lo[k] + 0.02) & (p[..., k] < hi[k] - 0.02)
                near_edge = (np.abs(p[..., k] - lo[k]) <= 0.02) | (np.abs(p[..., k] - hi[k]) <= 0.02)
                t = np.where(near_edge & (t > 0), -1.0, t)   # too close to an edge to call: poisons the pixel below
        ts[name] = np.where(ok, t, np.where(t == -1.0, -1.0, np.inf))
    for k, (cen, rad) in enumerate(spheres):
        oc = org - np.array(cen)
        b = d @ oc
        disc = b * b - (oc @ oc - rad * rad)
        t = np.where(disc > 1e-3, -b - np.sqrt(np.maximum(disc, 0)), np.where(disc > -1e-3, -1.0, np.inf))
        ts["sphere%d" % k] = t
    names = list(ts)
    stack = np.stack([ts[n] for n in names])
    poisoned = (stack == -1.0).any(axis=0)
    stack = np.where(stack == -1.0, np.inf, stack)
    order = np.argsort(stack, axis=0)
    best = np.take_along_axis(stack, order[:1], 0)[0]
    second = np.take_along_axis(stack, order[1:2], 0)[0]
    which = np.array(names)[order[0]]
    with np.errstate(invalid="ignore"):
        close = second - best < 0.02
    which = np.where(poisoned | ~np.isfinite(best) | close, "unsure", which)
    return which, best


def test_walls_of_scene_0_have_their_normals_and_analytic_depths():
    sc = dl.box(0, 48, 40)
    g, a = dl.features(sc)
    org, d = pixel_rays(sc)
    which, t = plane_hits(org, d, spheres=())   # the small spheres are not modelled: only pixels whose depth agrees are walls
    for name, normal in (("back", (0.0, -1.0, 0.0)), ("floor", (0.0, 0.0, 1.0))):
        m = (which == name) & (np.abs(g[..., 3] - t) <= 1e-5 * t)
        assert m.sum() > 40, (name, int(m.sum()))
        assert (g[m][:, :3] == np.array(normal, np.float32)).all()
    # every pixel the analytic box calls a wall either has that wall's depth or is covered by one of the small spheres
    walls = which != "unsure"
    agree = np.abs(g[..., 3] - t) <= 1e-5 * np.where(walls, t, 1.0)
    assert (agree | (g[..., 3] < t))[walls].all()
    assert agree[walls].mean() > 0.6


def test_sphere_pixels_of_scene_1_have_unit_normals_through_the_hit_point():
    sc = dl.box(1, 96, 80)
    g, a = dl.features(sc)
    org, d = pixel_rays(sc)
    which, t = plane_hits(org, d, spheres=(BIG_SPHERE,))
    m = which == "sphere0"
    assert m.sum() > 100
    n = g[m][:, :3].astype(np.float64)
    assert np.abs(np.linalg.norm(n, axis=1) - 1.0).max() <= 1e-6
    hit = org + g[m][:, 3:4].astype(np.float64) * d[m]
    assert np.abs(n - (hit - np.array(BIG_SPHERE[0])) / BIG_SPHERE[1]).max() <= 1e-5
    assert (a[m][:, :3] == 1.0).all()   # the mirror's albedo (1, 1, 1)
    # the lamp of scene 1: the underside of the small box under the ceiling (scene.hxx:303-315) is the emitter
    with np.errstate(divide="ignore", invalid="ignore"):
        tl = (1.26002 - org[2]) / d[..., 2]
    pl_ = org + tl[..., None] * d
    lamp = (tl > 0) & (np.abs(pl_[..., 0]) < 0.23) & (np.abs(pl_[..., 1]) < 0.23) & (np.abs(g[..., 3] - tl) <= 1e-5 * np.abs(tl))
    assert lamp.sum() >= 3, int(lamp.sum())
    assert (a[lamp][:, :3] == 1.0).all() and (g[lamp][:, :3] == np.array([0, 0, -1], np.float32)).all()
    ceil = (which == "ceiling") & (np.abs(g[..., 3] - t) <= 1e-5 * t)   # (the lamp's box covers some of it)
    assert ceil.sum() > 20 and (a[ceil][:, :3] == np.float32(0.803922)).all()   # a plain diffuse wall beside it
    assert (a[..., 3] == 1.0).all()


def quad_under_sky(resx=20, resy=16):
    from smallvcm_amd.scene2 import SceneBuilder
    b = SceneBuilder()
    grey = b.material(diffuse=(0.6, 0.0, 1.5))   # a 0 component and one above 1
    b.triangle((-0.5, 0, -0.5), (0.5, 0, -0.5), (0.5, 0, 0.5), grey)
    b.triangle((0.5, 0, 0.5), (-0.5, 0, 0.5), (-0.5, 0, -0.5), grey)
    b.background_light(1.0)
    return b.build((0, -3, 0), (0, 1, 0), (0, 0, 1), 40.0, resx, resy)


def test_misses_are_flagged_and_the_albedo_is_clamped_and_never_zero():
    sc = quad_under_sky()
    g, a = dl.features(sc)
    hit = g[..., 3] > 0
    assert 20 < hit.sum() < hit.size - 20
    assert hit[8, 10] and not hit[0, 0] and not hit[8, 0]      # the quad in the middle, nothing beside it
    assert (g[~hit] == 0.0).all() and (a[~hit] == 1.0).all()
    assert np.abs(g[hit][:, 3] - 3.0 / pixel_rays(dl.desc5(sc))[1][hit][:, 1]).max() <= 3e-5
    assert (a[hit] == np.array([0.6, 1.0, 1.0, 1.0], np.float32)).all()   # 0 -> 1, 1.5 -> 1


@pytest.mark.parametrize("scene_id", [0, 1, 3])
def test_list_and_bvh_builds_give_the_bits_of_the_rectangle_kind(scene_id, monkeypatch):
    sc = dl.box(scene_id, 33, 27)
    g0, a0 = dl.features(sc)
    monkeypatch.setenv("SMALLVCM_AMD_NO_ONEPLANE", "1")   # read when the scene is built: the plain list walk
    g1, a1 = dl.features(sc)
    monkeypatch.delenv("SMALLVCM_AMD_NO_ONEPLANE")
    monkeypatch.setenv("SMALLVCM_AMD_FORCE_BVH", "1")
    g2, a2 = dl.features(sc)
    assert g0.tobytes() == g1.tobytes() == g2.tobytes()
    assert a0.tobytes() == a1.tobytes() == a2.tobytes()


def test_a_shard_renders_its_own_pixel_range():
    sc = dl.box(3, 21, 17)
    g, a = dl.features(sc)
    parts = [dl.features(sc, rank=r, world=3) for r in range(3)]
    n = 21 * 17
    for r, (pg, pa) in enumerate(parts):   # its own range as the whole frame has it, zeros elsewhere
        lo, hi = n * r // 3, n * (r + 1) // 3
        own = np.zeros(n, bool)
        own[lo:hi] = True
        assert pg.reshape(n, 4)[own].tobytes() == g.reshape(n, 4)[own].tobytes() and pa.reshape(n, 4)[own].tobytes() == a.reshape(n, 4)[own].tobytes()
        assert (pg.reshape(n, 4)[~own] == 0).all() and (pa.reshape(n, 4)[~own] == 0).all()


# ---------------- it helps ----------------
# MSE(noisy) / MSE(denoised) against the 1000-iteration render of the same emulation (tests/golden/denoise_ref_*.npy,
# written by tests/denoise_tune.py), 64 x 64, 4 iterations, means over 4 seeds, default parameters.  MEASURED on the
# emulation (DESIGN.md "Denoising"); asserted: the square roots, as tests/test_light_pick.py does, which leaves room for
# seeds and still fails a filter that ignores the guides (a plain B3 blur measures 0.94 / 0.84 / 0.66 on these cases).
# Cases not taken, with their figures: scene 1 under VCM measures 1.5 (VCM renders the mirror sphere's reflection
# cleanly and the filter smooths it): its root would be a bound below 1.5.  Scene 0 measures 6.2 (PT) and 3.7 (VCM), but
# there the plain blur measures 3.4 as well -- the sun's noise at 4 iterations is so strong that any smoothing helps --
# so a root bound could not tell the two filters apart.
HELPS = [(1, "pt", ALGO_PATH_TRACE, 27.9), (3, "pt", ALGO_PATH_TRACE, 7.47), (3, "vcm", ALGO_VCM, 5.90)]


def helps_case(scene_id, name, algo, blur=False):
    ref = np.load(os.path.join(HERE, "golden", "denoise_ref_s%d_%s_64_1000.npy" % (scene_id, name)))
    sc = dl.box(scene_id, 64, 64)
    g, a = dl.features(sc)
    p = dl.defaults()
    if blur:   # the deliberately wrong variant: one flat surface everywhere, no colour stop, no demodulation
        g, a = dl.flat_guides(64, 64)
        p = dl.params(sigmaColor=1e9, demodulate=0)
    noisy_mse, clean_mse = [], []
    for seed in (11, 22, 33, 44):
        img = dl.Emul(sc, algo, seed).run(4).mean()
        noisy_mse.append(dl.rel_mse(img, ref))
        clean_mse.append(dl.rel_mse(dl.denoise(img, a, g, p), ref))
    return float(np.mean(noisy_mse) / np.mean(clean_mse))


@pytest.mark.parametrize("scene_id,name,algo,measured", HELPS)
def test_denoising_helps(scene_id, name, algo, measured):
    ratio = helps_case(scene_id, name, algo)
    print("scene %d %s: MSE(noisy) / MSE(denoised) = %.2f (recorded %.2f, bound %.2f)" % (scene_id, name, ratio, measured, measured ** 0.5))
    assert measured ** 0.5 >= 1.5
    assert ratio >= measured ** 0.5


@pytest.mark.parametrize("scene_id,name,algo,measured", HELPS)
def test_a_plain_blur_misses_the_bound(scene_id, name, algo, measured):
    """the bound is one a filter that ignores the guides does not reach"""
    ratio = helps_case(scene_id, name, algo, blur=True)
    print("scene %d %s: plain B3 blur ratio %.2f (bound %.2f)" % (scene_id, name, ratio, measured ** 0.5))
    assert ratio < measured ** 0.5
