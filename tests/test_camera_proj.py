"""Fisheye and panoramic camera projections (vcm_scene_desc9) on the CPU: both maps against an independent binary64
restatement, the round trip, the normalisation of cameraPdfW, a constant sky, the panorama of an environment map
against that map, the estimators against the path tracer on the host emulation (tests/host_emul_proj), the unchanged
perspective default, and the interface: refusals, the scene-file directive, SceneBuilder, the host sanitizers."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import proj_lib as pl
from smallvcm_amd._abi import CameraModel, SceneDesc8, SceneDesc9, with_projection
from smallvcm_amd.renderer import load_library

ALGOS = {"lt": 0, "ppm": 1, "bpm": 2, "bpt": 3, "vcm": 4, "pt": 5, "eye": 6}
# (name, projection, W, H): a square and a non-square image for the fisheyes (90, 180 and 300 degrees), 2:1 and an odd
# size for the panorama
MAPPING_CASES = [("fisheye180", ("fisheye", 180.0), 48, 48), ("fisheye90", ("fisheye", 90.0), 40, 60), ("fisheye300", ("fisheye", 300.0), 36, 24),
                 ("panorama", ("panorama",), 64, 32), ("panorama_odd", ("panorama",), 37, 23)]


@pytest.fixture(scope="module")
def E():
    return pl.emul_proj()   # builds tests/host_emul_proj


def _kind(proj):
    return pl.FISHEYE if proj[0] == "fisheye" else pl.PANORAMA


def _scene(proj, W, H, **kw):
    return pl.box(W, H, proj=proj, **kw)


@pytest.fixture(scope="module")
def mapping():
    """per case: the scene, the reference, the 50 000 records and what the emulation answers -- computed once"""
    out = {}
    for name, proj, W, H in MAPPING_CASES:
        d = _scene(proj, W, H)
        inp = pl.records(d)
        out[name] = (d, pl.Reference(d, _kind(proj), proj[1] if len(proj) > 1 else 0.0), inp, pl.kat9(d, inp))
    return out


# ---------------------------------------------------------------- the maps

def test_the_frame_is_the_cameras(E):
    d = _scene(("fisheye", 200.0), 30, 20)
    err, p = pl.params(d)
    assert err is None and p["kind"] == pl.FISHEYE and p["fov"] == 200.0
    c, f, ex, ey, W, H = pl.camera_frame(d.camera)
    for got, want in ((p["f"], f), (p["ex"], ex), (p["ey"], ey)):
        assert np.abs(got - want).max() < 1e-6
    assert ey[2] < 0   # an upright camera: raster +y points down
    assert abs(p["k"] - 30 / np.deg2rad(200.0)) < 1e-5 and abs(p["theta_max"] - np.deg2rad(100.0)) < 1e-6


@pytest.mark.parametrize("name", [c[0] for c in MAPPING_CASES])
def test_both_maps_against_the_binary64_restatement(mapping, name):
    """direction, cameraPdfW and the inverse raster of 50 000 records: 1e-4 relative, 1e-3 px.  Left out, by rules on
    the inputs alone (the reference's angles): theta within 1e-4 of theta_max, |sin theta| < 0.05 where the azimuth is
    ill-conditioned, and for the inside-the-image flag a reference raster within 2e-3 px of the image's border; at
    most 5 % in all, which the reference alone is held to."""
    d, ref, inp, out = mapping[name]
    n = len(inp)
    # forward
    rdir, rpdf, rvalid, rtheta = ref.forward(inp[:, 0:2])
    skip = ref.left_out(rtheta) & rvalid   # (of the records that would be compared)
    edge = np.abs(rtheta - ref.theta_max) < 1e-4 if ref.kind == pl.FISHEYE else np.zeros(n, bool)
    assert (skip | edge).mean() <= 0.05
    assert rvalid.mean() > 0.3 and (ref.kind == pl.PANORAMA or (~rvalid).mean() > 0.02)
    valid = out[:, 4] == 1.0
    assert np.array_equal(valid[~edge], rvalid[~edge])
    ok = valid & rvalid
    assert np.abs(out[ok, 0:3] - rdir[ok]).max() < 1e-4
    assert np.abs(np.linalg.norm(out[ok, 0:3].astype(np.float64), axis=1) - 1).max() < 1e-6
    ok &= ~skip
    assert np.abs(out[ok, 3] / rpdf[ok] - 1).max() < 1e-4
    assert np.all(out[~valid, 0:4] == 0)
    # inverse
    rras, rpdf, rfov, rtheta = ref.inverse(inp[:, 2:5])
    skip = ref.left_out(rtheta)
    edge = np.abs(rtheta - ref.theta_max) < 1e-4 if ref.kind == pl.FISHEYE else np.zeros(n, bool)
    border = np.minimum(np.minimum(np.abs(rras[:, 0]), np.abs(rras[:, 0] - ref.W)), np.minimum(np.abs(rras[:, 1]), np.abs(rras[:, 1] - ref.H))) < 2e-3
    assert (skip | border | edge).mean() <= 0.05
    rin = rfov & (rras[:, 0] >= 0) & (rras[:, 1] >= 0) & (rras[:, 0] < ref.W) & (rras[:, 1] < ref.H)
    use = ~(edge | border)
    assert np.array_equal((out[:, 7] == 1.0)[use], rin[use])
    assert (out[:, 7] == 1.0).mean() > 0.1   # (a 90 degree fisheye sees 15 % of the sphere)
    ok = rfov & ~edge & ~skip
    assert ok.mean() > 0.1
    assert ref.raster_error(out[ok, 5:7], rras[ok]).max() < 1e-3
    assert np.abs(out[ok, 8] / rpdf[ok] - 1).max() < 1e-4


@pytest.mark.parametrize("name", [c[0] for c in MAPPING_CASES])
def test_points_on_a_ray_project_back_to_its_sample(mapping, name):
    d, ref, inp, out = mapping[name]
    valid = out[:, 4] == 1.0
    _, _, _, theta = ref.forward(inp[:, 0:2])
    inside = valid & ~ref.left_out(theta) & (inp[:, 0] >= 0) & (inp[:, 1] >= 0) & (inp[:, 0] < ref.W) & (inp[:, 1] < ref.H)
    assert inside.sum() > 10000
    for t in (0.07, 0.9, 3.0, 40.0):
        rec = inp[inside].copy()
        rec[:, 2:5] = ref.c + t * out[inside, 0:3].astype(np.float64)
        back = pl.kat9(d, rec)
        err = ref.raster_error(back[:, 5:7], rec[:, 0:2].astype(np.float64))
        assert err.max() < 1e-3, (t, float(err.max()))
        # the density is the same number on both sides of the camera vertex
        assert np.abs(back[:, 8] / out[inside, 3] - 1).max() < 1e-4
        near = np.minimum(np.minimum(rec[:, 0], ref.W - rec[:, 0]), np.minimum(rec[:, 1], ref.H - rec[:, 1])) > 2e-3
        assert np.all(back[near, 7] == 1.0)


@pytest.mark.parametrize("proj,W,H,want", [
    (("panorama",), 64, 32, 4 * np.pi), (("panorama",), 37, 23, 4 * np.pi),
    (("fisheye", 90.0), 48, 48, 2 * np.pi * (1 - np.cos(np.pi / 4))), (("fisheye", 90.0), 32, 50, 2 * np.pi * (1 - np.cos(np.pi / 4))),
    (("fisheye", 180.0), 48, 48, 2 * np.pi), (("fisheye", 180.0), 32, 50, 2 * np.pi),
    (("fisheye", 300.0), 48, 48, 2 * np.pi * (1 - np.cos(np.deg2rad(150.0)))), (("fisheye", 300.0), 32, 50, 2 * np.pi * (1 - np.cos(np.deg2rad(150.0))))])
def test_camera_pdf_integrates_to_the_solid_angle(E, proj, W, H, want):
    """the mean of 1 / cameraPdfW over uniform raster samples (0 where the sample is not valid) times the raster area:
    4 pi for the panorama, 2 pi (1 - cos theta_max) for a fisheye whose circle lies inside the image (W <= H)"""
    d = _scene(proj, W, H)
    rng = np.random.default_rng(11)
    n = 200000
    inp = np.zeros((n, pl.KAT), np.float32)
    inp[:, 0], inp[:, 1] = rng.uniform(0, W, n), rng.uniform(0, H, n)
    inp[:, 0:2] = np.minimum(inp[:, 0:2], np.nextafter(np.float32([W, H]), np.float32(0)))
    out = pl.kat9(d, inp)
    v = np.where(out[:, 4] == 1.0, 1.0 / np.maximum(out[:, 3].astype(np.float64), 1e-30), 0.0) * (W * H)
    mean, se = v.mean(), v.std(ddof=1) / np.sqrt(n)
    print(proj, W, H, "integral %.5f want %.5f se %.5f z %.2f" % (mean, want, se, (mean - want) / se))
    assert abs(mean - want) < 5 * se
    assert se < 0.02 * want


# ---------------------------------------------------------------- images on the emulation

SKY_RADIANCE = np.array([135 / 255.0, 206 / 255.0, 250 / 255.0], np.float32)   # the reference's BackgroundLight, scale 1


SPHERE_CENTRE, SPHERE_RADIUS = (0.0, -1.0, 0.0), 0.05


def _sky_only(proj, W, H, sky=None):
    """nothing but a background (constant, or the map `sky`) around a camera at the origin, and one small sphere on the
    horizon: the scene loader and the scene's bounding sphere want a primitive"""
    from smallvcm_amd.scene2 import SceneBuilder
    b = SceneBuilder()
    b.sphere(SPHERE_CENTRE, SPHERE_RADIUS, b.material(diffuse=(0.5, 0.5, 0.5)))
    if sky is None:
        b.background_light(1.0)
    else:
        b.envmap_light(sky, 1.0)
    b.projection(*proj)
    return b


def _sphere_mask(ref, W, H, grow=2.0):
    """pixels within `grow` px of the disc the sphere of _sky_only covers, seen from the origin, by its projection"""
    ang = np.arcsin(SPHERE_RADIUS / 1.0)
    t = np.linspace(0, 2 * np.pi, 721)
    axis = np.array(SPHERE_CENTRE)
    u, v = np.array([1.0, 0.0, 0.0]), np.array([0.0, 0.0, 1.0])
    mask = np.zeros((H, W), bool)
    yy, xx = np.mgrid[0:H, 0:W]
    for a in np.linspace(0, ang, 12):
        ring = np.cos(a) * axis + np.sin(a) * (np.cos(t)[:, None] * u + np.sin(t)[:, None] * v)
        r, _, fov, _ = ref.inverse(ref.c + ring)
        for x, y in r[fov]:
            dx = np.abs(xx + 0.5 - x)
            if ref.kind == pl.PANORAMA:
                dx = np.minimum(dx, W - dx)
            mask |= (dx <= grow + 0.5) & (np.abs(yy + 0.5 - y) <= grow + 0.5)
    return mask


@pytest.mark.parametrize("proj,W,H", [(("panorama",), 32, 16), (("fisheye", 180.0), 24, 24), (("fisheye", 240.0), 30, 20), (("fisheye", 120.0), 20, 30)])
def test_constant_sky(E, proj, W, H):
    """path tracing, path length 1, under the reference's constant background: every panorama pixel and every fisheye
    pixel wholly inside the circle is the radiance, every pixel wholly outside is exactly 0"""
    d = _sky_only(proj, W, H).build((0, 0, 0), (0, 1, 0), (0, 0, 1), 45.0, W, H)
    ref = pl.Reference(d, _kind(proj), proj[1] if len(proj) > 1 else 0.0)
    iters = 3
    r = pl.Emul9(d, ALGOS["pt"], seed=4)
    for it in range(iters):
        r.run_iteration(it, 0, 1)
    img = r.framebuffer() / iters
    sphere = _sphere_mask(ref, W, H)
    assert sphere.mean() < 0.15
    yy, xx = np.mgrid[0:H, 0:W]
    if ref.kind == pl.PANORAMA:
        inside, outside = np.ones((H, W), bool), np.zeros((H, W), bool)
    else:
        R = ref.k * ref.theta_max
        cx, cy = np.abs(xx + 0.5 - W / 2), np.abs(yy + 0.5 - H / 2)
        far = np.hypot(cx + 0.5, cy + 0.5)
        near = np.hypot(np.maximum(cx - 0.5, 0), np.maximum(cy - 0.5, 0))
        inside, outside = far < R - 1e-3, near > R + 1e-3
        assert outside.sum() > 0 or W <= H
    assert (inside & ~sphere).sum() > 0.3 * W * H
    assert np.allclose(img[inside & ~sphere], SKY_RADIANCE, rtol=1e-6, atol=0)
    assert np.all(img[outside] == 0)
    st = r.stats()
    if ref.kind == pl.FISHEYE and outside.sum() > 0:
        assert st["cameraRays"] < iters * W * H   # a sample outside the circle casts and counts no ray


def test_panorama_of_an_environment_map_is_that_map(E):
    """the closed loop: an 8 x 4-texel sky seen through a 256 x 128 panorama whose axes are the map's (forward -x, up +z).
    Each pixel is the texel the map's convention (u = atan2(y, x) / 2 pi, v = acos(z) / pi, row 0 up) gives for the pixel's
    direction, and the image mirrored left-right is the map enlarged: the recipe of DESIGN.md.  Left out: pixels whose
    footprint grown by 0.01 px touches a texel edge, and the small sphere's silhouette grown by 2 px; 15 % at most."""
    W, H, TW, TH = 256, 128, 8, 4
    rng = np.random.default_rng(5)
    sky = rng.uniform(0.2, 3.0, (TH, TW, 3)).astype(np.float32)
    d = _sky_only(("panorama",), W, H, sky=sky).build((0, 0, 0), (-1, 0, 0), (0, 0, 1), 45.0, W, H)
    ref = pl.Reference(d, pl.PANORAMA)
    r = pl.Emul9(d, ALGOS["pt"], seed=2)
    r.run_iteration(0, 0, 1)
    img = r.framebuffer()
    yy, xx = np.mgrid[0:H, 0:W]
    dirs, _, _, _ = ref.forward(np.stack([xx.ravel() + 0.5, yy.ravel() + 0.5], axis=1))
    phi = np.mod(np.arctan2(dirs[:, 1], dirs[:, 0]), 2 * np.pi)
    col = np.minimum((phi / (2 * np.pi) * TW).astype(int), TW - 1).reshape(H, W)
    row = np.minimum((np.arccos(np.clip(dirs[:, 2], -1, 1)) / np.pi * TH).astype(int), TH - 1).reshape(H, W)
    px, py = W // TW, H // TH
    edge_x = ((xx % px) == 0) | ((xx % px) == px - 1)       # [x - 0.01, x + 1.01] holds a multiple of 32 (0 and W wrap)
    edge_y = ((yy % py) == 0) | ((yy % py) == py - 1)
    skip = edge_x | edge_y | _sphere_mask(ref, W, H)
    print("left out: %.3f" % skip.mean())
    assert skip.mean() <= 0.15
    # a path's colour goes to the pixel that holds its jittered sample, and float(x) + jitter may round up to x + 1 (the
    # reference's Framebuffer::AddColor; about one sample in 3e5 at this size): count the samples per pixel from the
    # tape's first two floats.  Away from the texel edges the neighbour's sample reads the same texel.
    E.emul_path_float.argtypes = [C.c_uint32] * 5
    E.emul_path_float.restype = C.c_float
    count = np.zeros((H, W), np.int64)
    for p in range(W * H):
        sx = np.float32(p % W) + np.float32(E.emul_path_float(2, 0, p, 1, 0))
        sy = np.float32(p // W) + np.float32(E.emul_path_float(2, 0, p, 1, 1))
        if sx < W and sy < H:
            count[int(sy), int(sx)] += 1
    assert (count != 1).sum() <= 4
    want = sky[row, col] * count[:, :, None].astype(np.float32)
    assert np.array_equal(img[~skip], want[~skip])
    # the recipe: mirrored left-right, the panorama is the map itself
    enlarged = np.repeat(np.repeat(sky, py, axis=0), px, axis=1) * count[:, ::-1, None].astype(np.float32)
    assert np.array_equal(img[:, ::-1][~skip[:, ::-1]], enlarged[~skip[:, ::-1]])


# ---------------------------------------------------------------- estimators

def _blocks(img, b):
    H, W = img.shape[:2]
    return img[: H // b * b, : W // b * b].reshape(H // b, b, W // b, b, 3).mean(axis=(1, 3))


def _estimate(d, algo, iters, seed, rf=0.003, b=4):
    """mean and standard error per b x b block over the iterations of one render (they are independent draws)"""
    r = pl.Emul9(d, algo, seed=seed, radius_factor=rf)
    prev = np.zeros((r.resy, r.resx, 3), np.float64)
    per = []
    for it in range(iters):
        r.run_iteration(it)
        fb = r.framebuffer().astype(np.float64)
        per.append(_blocks(fb - prev, b))
        prev = fb
    per = np.array(per)
    return per.mean(axis=0), per.std(axis=0, ddof=1) / np.sqrt(iters)


def _agree(a, b, what, bias=0.0):
    """per block within 5 combined standard errors (test_thin_lens._agree); bias: the merging estimators' 2 % radius term"""
    (m, s), (rm, rs) = a, b
    z = np.abs(m - rm) / np.sqrt(s ** 2 + rs ** 2 + (bias * rm) ** 2 + 1e-8)
    print("%s: max z %.2f, mean ratio %.4f" % (what, float(z.max()), m.mean() / rm.mean()))
    assert z.max() < 5.0, (what, float(z.max()))
    assert abs(m.mean() / rm.mean() - 1) < 0.05, (what, m.mean(), rm.mean())


ESTIMATOR_CASES = [("panorama", ("panorama",), 32, 16, {}), ("fisheye_square", ("fisheye", 200.0), 24, 24, {}),
                   ("fisheye_3_2", ("fisheye", 160.0), 30, 20, {}),
                   ("panorama_tent", ("panorama",), 32, 16, {"flt": ("tent", 1.5)}), ("fisheye_tent", ("fisheye", 200.0), 24, 24, {"flt": ("tent", 1.5)}),
                   ("panorama_sobol", ("panorama",), 32, 16, {"sampler": "sobol"}), ("fisheye_sobol", ("fisheye", 160.0), 30, 20, {"sampler": "sobol"})]


@pytest.mark.parametrize("name,proj,W,H,kw", ESTIMATOR_CASES, ids=[c[0] for c in ESTIMATOR_CASES])
def test_estimators_agree_with_the_path_tracer(E, name, proj, W, H, kw):
    """LT and BPM against PT in the box without spheres (a point light: nothing emissive in view), BPT and VCM against PT
    in the room (an area light, a mirror sphere), the camera inside so that every direction sees geometry.  A mirrored
    inverse map or a cameraPdfW without its Jacobian fails this (DESIGN.md has the z-scores of both planted errors)."""
    box = pl.box(W, H, proj=proj, **kw)
    pt = _estimate(box, ALGOS["pt"], 256, 510)
    assert pt[0].mean() > 0.01
    _agree(_estimate(box, ALGOS["lt"], 256, 10), pt, name + " lt")
    _agree(_estimate(box, ALGOS["bpm"], 128, 210, rf=0.02), pt, name + " bpm", bias=0.02)
    room = pl.box(W, H, proj=proj, room=True, **kw)
    pt = _estimate(room, ALGOS["pt"], 256, 520)
    _agree(_estimate(room, ALGOS["bpt"], 128, 310), pt, name + " bpt")
    _agree(_estimate(room, ALGOS["vcm"], 128, 410), pt, name + " vcm", bias=0.02)


# ---------------------------------------------------------------- the default

@pytest.mark.parametrize("algo", range(7))
def test_perspective_through_create9_equals_create8(E, algo):
    """model = NULL and kind PERSPECTIVE render exactly what the version-8 description renders: framebuffer, both tapes,
    nine counters"""
    d8 = pl.as_desc8(pl.box(20, 14, room=True))
    ref = pl.Emul9(d8, algo, seed=5, version8=True)
    emus = [pl.Emul9(with_projection(d8, None), algo, seed=5), pl.Emul9(with_projection(d8, "perspective", 123.0), algo, seed=5)]
    for it in range(2):
        ref.run_iteration(it)
        for e in emus:
            e.run_iteration(it)
    want = ref.framebuffer()
    assert np.count_nonzero(want) > 0
    for e in emus:
        assert np.array_equal(e.framebuffer().view(np.uint32), want.view(np.uint32))
        for k in range(2):
            assert np.array_equal(e.counts()[k], ref.counts()[k])
        assert e.stats() == ref.stats()
    err, p = pl.params(emus[1].scene)
    assert err is None and p["kind"] == pl.PERSPECTIVE


@pytest.mark.parametrize("algo", [0, 3, 5, 6])
@pytest.mark.parametrize("proj", [("fisheye", 220.0), ("panorama",)], ids=["fisheye", "panorama"])
def test_sharded_emulation_equals_unsharded(E, algo, proj):
    """world 2 of the emulation (no exchange of light vertices: the algorithms without merging): every pixel's camera
    path and every light path on one rank, with the filter offsets of the global path"""
    d = pl.box(20, 14, proj=proj, room=True, flt=("tent", 1.5))
    full = pl.Emul9(d, algo, seed=3)
    shards = [pl.Emul9(d, algo, seed=3, rank=r, world=2) for r in range(2)]
    for it in range(2):
        full.run_iteration(it)
        for s in shards:
            s.run_iteration(it)
    fb = shards[0].framebuffer() + shards[1].framebuffer()
    assert np.count_nonzero(fb) > 0
    if algo in (5, 6):
        assert np.array_equal(fb, full.framebuffer())
    else:
        assert np.allclose(fb, full.framebuffer(), rtol=2e-6, atol=1e-7)
    for k in range(2):
        assert np.array_equal(np.concatenate([s.counts()[k] for s in shards]), full.counts()[k])


# ---------------------------------------------------------------- the interface

def _create9(L):
    L.vcm_create9.restype = C.c_void_p
    L.vcm_create9.argtypes = [C.POINTER(SceneDesc9), C.c_int, C.c_float, C.c_float, C.c_int]
    L.vcm_last_error.restype = C.c_char_p
    return L.vcm_create9


def test_create9_refusals(E):
    """the library's checks run before it looks for a device; the emulation shares them (scene_host.h)"""
    L = load_library(require_gpu=False)
    create9 = _create9(L)
    plain = pl.as_desc8(pl.box(12, 8))
    cases = [((3, 90.0), "unknown projection"), ((-1, 90.0), "unknown projection"), ((pl.FISHEYE, 0.0), "fovDegrees"),
             ((pl.FISHEYE, 360.0), "fovDegrees"), ((pl.FISHEYE, -5.0), "fovDegrees"), ((pl.FISHEYE, float("nan")), "fovDegrees"),
             ((pl.FISHEYE, float("inf")), "fovDegrees")]
    for (kind, fov), text in cases:
        d = with_projection(plain, kind, fov)
        assert not create9(C.byref(d), 4, 0.003, 0.75, 1), (kind, fov)
        assert text in L.vcm_last_error().decode() and "vcm_create9" in L.vcm_last_error().decode(), (kind, fov)
        err, _ = pl.params(d)
        assert err is not None and text in err
    # a thin lens with either projection; a closed lens is the pinhole
    from smallvcm_amd.scene2 import SceneBuilder

    def lensed(radius):
        b = SceneBuilder()
        b.triangle((-1, -1, 0), (1, -1, 0), (1, 1, 0), b.material(diffuse=(0.7, 0.7, 0.7)))
        b.background_light(1.0)
        b.thin_lens(radius, 3.0)
        return b.build((0, -4, 2), (0, 1, -0.4), (0, 0, 1), 50, 12, 8)
    for kind, fov in ((pl.FISHEYE, 180.0), (pl.PANORAMA, 0.0)):
        d = with_projection(lensed(0.1), kind, fov)
        assert not create9(C.byref(d), 5, 0.003, 0.75, 1)
        assert "thin lens" in L.vcm_last_error().decode()
        assert "thin lens" in pl.params(d)[0]
        assert pl.params(with_projection(lensed(0.0), kind, fov))[0] is None
    assert pl.params(with_projection(lensed(0.1), pl.PERSPECTIVE))[0] is None
    # a bad version-8 part is still refused
    from smallvcm_amd._abi import with_material_ext
    bad = with_projection(with_material_ext(pl.box(12, 8), [(2.0, 0.5, 0.5, 0.3)] * 5), "panorama")
    assert pl.params(bad)[0] is not None
    # the known-answer op answers nothing in a perspective scene
    d = with_projection(plain, None)
    assert np.all(pl.kat9(d, pl.records(d, n=16)) == 0)


def _quad(tmp_path):
    (tmp_path / "quad.obj").write_text("mtllib quad.mtl\nv -1 -1 0\nv 1 -1 0\nv 1 1 0\nv -1 1 0\nusemtl white\nf 1 2 3 4\n")
    (tmp_path / "quad.mtl").write_text("newmtl white\nKd 0.8 0.8 0.8\n")


def test_scene_file_projection_directive(tmp_path):
    from smallvcm_amd.scene2 import SceneBuilder
    from smallvcm_amd.scene_file import load_scene
    _quad(tmp_path)
    head = "obj quad.obj\ncamera 0 -4 2  0 1 -0.4  0 0 1  50\nlight background 1\n"
    for line, args in (("projection fisheye 187.5   # wide\n", ("fisheye", 187.5)), ("projection panorama\n", ("panorama",))):
        (tmp_path / "s.vcmscene").write_text(head + line)
        d = load_scene(tmp_path / "s.vcmscene", 16, 12)
        assert isinstance(d, SceneDesc9) and d.model
        b = SceneBuilder()
        b.triangle((-1, -1, 0), (1, -1, 0), (1, 1, 0), b.material(diffuse=(0.8, 0.8, 0.8)))
        b.background_light(1.0)
        b.projection(*args)
        want = b.build((0, -4, 2), (0, 1, -0.4), (0, 0, 1), 50, 16, 12)
        assert isinstance(want, SceneDesc9)
        assert bytes(d.model.contents) == bytes(want.model.contents)   # field for field
        assert bytes(d.camera) == bytes(want.camera)
        assert not d.base.materialExt and not d.base.base.sampler
        e1, p1 = pl.params(d)
        e2, p2 = pl.params(want)
        assert e1 is None and e2 is None
        for k in p1:
            assert np.array_equal(p1[k], p2[k])
    (tmp_path / "plain.vcmscene").write_text(head)
    assert not isinstance(load_scene(tmp_path / "plain.vcmscene", 8, 8), SceneDesc9)
    for bad in ("projection", "projection fisheye", "projection fisheye x", "projection fisheye 0", "projection fisheye 360",
                "projection fisheye -3", "projection fisheye nan", "projection fisheye inf", "projection fisheye 90 1",
                "projection panorama 90", "projection ortho", "projection perspective", "projection panorama\nprojection panorama"):
        (tmp_path / "bad.vcmscene").write_text(head + bad + "\n")
        with pytest.raises(ValueError, match=r"line [45]: .*projection"):
            load_scene(tmp_path / "bad.vcmscene", 8, 8)


def test_scene_builder_projection():
    from smallvcm_amd.scene2 import SceneBuilder

    def builder():
        b = SceneBuilder()
        b.triangle((-1, -1, 0), (1, -1, 0), (1, 1, 0), b.material(diffuse=(0.7, 0.7, 0.7)))
        b.background_light(1.0)
        return b
    cam = ((0, -4, 2), (0, 1, -0.4), (0, 0, 1), 50, 16, 12)
    plain = builder().build(*cam)
    assert not isinstance(plain, SceneDesc9)
    b = builder()
    b.projection("fisheye", 180.0)
    d = b.build(*cam)
    assert isinstance(d, SceneDesc9) and isinstance(d.base, SceneDesc8)
    assert (d.model.contents.kind, d.model.contents.fovDegrees) == (pl.FISHEYE, 180.0)
    assert bytes(d.camera) == bytes(plain.camera)
    b = builder()
    b.projection("panorama")
    d = b.build(*cam)
    assert (d.model.contents.kind, d.model.contents.fovDegrees) == (pl.PANORAMA, 0.0)
    e = pl.Emul9(d, ALGOS["pt"], seed=1)   # the description is complete
    e.run_iteration(0)
    assert np.count_nonzero(e.framebuffer()) > 0
    for kind, fov in (("ortho", 0), ("fisheye", 0), ("fisheye", 360), ("fisheye", float("nan")), ("fisheye", -1)):
        with pytest.raises(ValueError):
            builder().projection(kind, fov)
    assert C.sizeof(CameraModel) == 8


def test_the_model_checks_and_the_directive_run_clean_under_the_host_sanitizers(tmp_path):
    """tests/host_emul_proj/sanitize_proj: scene_host_set_projection on ordinary and hostile camera models and the
    loader's `projection` directive on good and malformed files, in a stand-alone program built with
    -fsanitize=address,undefined (CPU only)"""
    subprocess.run(["make", "-C", pl.EMUL_DIR, "sanitize_proj"], check=True, stdout=subprocess.DEVNULL)
    r = subprocess.run([os.path.join(pl.EMUL_DIR, "sanitize_proj"), str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
