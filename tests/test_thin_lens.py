"""The thin-lens camera (vcm_scene_desc4) on the CPU: input checks, the pinhole equivalence of a missing or closed lens,
the lens geometry through the known-answer records of the host emulation (tests/host_emul_lens), unbiasedness of the
emulated renderer across algorithms, the random-number streams, sharding, and the scene-file / SceneBuilder surface."""
import ctypes as C

import numpy as np
import pytest

import envmap_lib as el
import lens_lib as ll
from smallvcm_amd._abi import SceneDesc3, SceneDesc4
from smallvcm_amd.renderer import load_library

# a strong defocus of scene 3 at 24 x 24: the back wall (about 5.4 from the camera) blurs over ~3 pixels
R_STRONG, F_STRONG = 0.8, 3.0


@pytest.fixture(scope="module")
def E():
    return ll.emul_lens()   # builds tests/host_emul_lens


# ---------------------------------------------------------------- C-ABI

def test_create4_rejects_bad_lenses(E):
    """the library's checks run before it looks for a device; the emulation shares them (scene_host.h)"""
    L = load_library(require_gpu=False)
    L.vcm_create4.restype = C.c_void_p
    L.vcm_create4.argtypes = [C.POINTER(SceneDesc4), C.c_int, C.c_float, C.c_float, C.c_int]
    L.vcm_last_error.restype = C.c_char_p
    for r, f in [(-0.1, 3.0), (float("nan"), 3.0), (float("inf"), 3.0), (0.1, 0.0), (0.1, -2.0), (0.1, float("nan")),
                 (0.1, float("inf"))]:
        d = ll.builtin_lens(r, f)
        assert not L.vcm_create4(C.byref(d), 4, 0.003, 0.75, 1), (r, f)
        assert "thin lens" in L.vcm_last_error().decode(), (r, f)
        assert not E.emul_create4(C.byref(d), 4, 0.003, 0.75, 1, 0, 1), (r, f)
        assert "thin lens" in E.emul_lens_error().decode()
    # a bad version-3 part is still refused
    d = ll.with_lens(el.builtin_with_envmap(np.zeros((4, 8, 3), np.float32)), 0.1, 3.0)
    assert not E.emul_create4(C.byref(d), 4, 0.003, 0.75, 1, 0, 1)
    assert ll.lens_params(ll.builtin_lens(0.0, 2.0))[0] == 0.0   # a closed lens is the pinhole
    assert ll.lens_params(ll.builtin_lens(None, None))[0] == 0.0


@pytest.mark.parametrize("algo", range(7))
def test_no_lens_and_closed_lens_equal_create3(algo):
    """lens = NULL and apertureRadius = 0 render exactly what the version-3 description renders"""
    d3 = ll.builtin3(resx=20, resy=14)
    ref = el.Emul3(d3, algo, seed=5)
    emus = [ll.Emul4(ll.with_lens(d3, None, None), algo, seed=5), ll.Emul4(ll.with_lens(d3, 0.0, 2.5), algo, seed=5)]
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


# ---------------------------------------------------------------- geometry (VCM_KAT_LENS)

def test_lens_basis_is_orthonormal():
    d = ll.builtin_lens(0.3, 3.0)
    r, f, right, up = ll.lens_params(d)
    fwd = np.array(d.camera.forward[:], np.float64)
    assert (r, f) == (np.float32(0.3), 3.0)
    for a, b in ((right, up), (right, fwd), (up, fwd)):
        assert abs(float(np.dot(a, b))) < 1e-6
    assert abs(np.linalg.norm(right) - 1) < 1e-6 and abs(np.linalg.norm(up) - 1) < 1e-6


def _ray(d, raster, uv):
    out = ll.kat4(d, ll.OP_LENS, ll.lens_records(raster, uv, np.zeros((len(raster), 3))))
    return out[:, 0:3].astype(np.float64), out[:, 3:6].astype(np.float64), out


def test_points_on_a_ray_project_back_to_its_sample():
    d = ll.builtin_lens(0.5, 3.0, resx=64, resy=48)
    rng = np.random.default_rng(1)
    n = 4000
    raster = rng.random((n, 2)) * [64, 48]
    uv = rng.random((n, 2))
    org, dirs, out = _ray(d, raster, uv)
    assert np.allclose(np.linalg.norm(dirs, axis=1), 1, atol=1e-6)
    # cameraPdfW = (imagePlaneDist / cos)^2 / cos with cos = forward . dir
    cos = dirs @ np.array(d.camera.forward[:], np.float64)
    ipd = d.camera.imagePlaneDist
    assert np.allclose(out[:, 6], (ipd / cos) ** 2 / cos, rtol=1e-5)
    # lens points lie on the disc of radius R around the camera, in the plane perpendicular to forward
    rel = org - np.array(d.camera.position[:], np.float64)
    assert np.all(np.linalg.norm(rel, axis=1) <= 0.5 * (1 + 1e-6))
    assert np.abs(rel @ np.array(d.camera.forward[:], np.float64)).max() < 1e-6
    for t in (0.7, 2.0, 3.0, 5.5, 12.0):
        q = org + t * dirs
        back = ll.kat4(d, ll.OP_LENS, ll.lens_records(raster, uv, q))
        assert np.all(back[:, 9] == 1.0)
        err = np.abs(back[:, 7:9] - raster).max()
        assert err < 1e-3, (t, err)


def test_focus_plane_is_sharp():
    d = ll.builtin_lens(0.5, 3.0, resx=64, resy=48)
    rng = np.random.default_rng(2)
    n = 500
    raster = rng.random((n, 2)) * [64, 48]
    org, dirs, _ = _ray(d, raster, np.full((n, 2), 0.5))   # (0.5, 0.5) is the lens centre: the pinhole ray
    assert np.allclose(org, np.array(d.camera.position[:], np.float64), atol=1e-7)
    fwd = np.array(d.camera.forward[:], np.float64)
    p = org + dirs * (3.0 / (dirs @ fwd))[:, None]   # on the focus plane
    for k in range(8):
        uv = rng.random((n, 2))
        back = ll.kat4(d, ll.OP_LENS, ll.lens_records(raster, uv, p))
        assert np.abs(back[:, 7:9] - raster).max() < 1e-3, k


@pytest.mark.parametrize("z", [1.5, 2.5, 6.0, 20.0])
def test_circle_of_confusion(z):
    """a point on the axis at depth z spreads over a disc of radius R * imagePlaneDist * |1/F - 1/z| pixels, uniformly"""
    R, F = 0.4, 3.0
    d = ll.builtin_lens(R, F, resx=64, resy=64)
    c = np.array(d.camera.position[:], np.float64)
    f = np.array(d.camera.forward[:], np.float64)
    n = 20000
    uv = np.random.default_rng(3).random((n, 2))
    centre = ll.kat4(d, ll.OP_LENS, ll.lens_records(np.zeros((1, 2)), np.full((1, 2), 0.5), [c + z * f]))[0, 7:9]
    out = ll.kat4(d, ll.OP_LENS, ll.lens_records(np.zeros((n, 2)), uv, np.tile(c + z * f, (n, 1))))
    assert np.all(out[:, 9] == 1.0)
    rad = np.linalg.norm(out[:, 7:9].astype(np.float64) - centre, axis=1)
    want = R * d.camera.imagePlaneDist * abs(1 / F - 1 / z)
    assert rad.max() <= want * (1 + 1e-3) + 1e-3
    assert rad.max() >= want * 0.99
    assert abs(rad.mean() / want - 2 / 3) < 0.01   # uniform over the disc


def test_points_behind_the_lens_do_not_project():
    d = ll.builtin_lens(0.4, 3.0)
    c = np.array(d.camera.position[:], np.float64)
    f = np.array(d.camera.forward[:], np.float64)
    out = ll.kat4(d, ll.OP_LENS, ll.lens_records(np.zeros((2, 2)), np.full((2, 2), 0.3), [c - f, c]))
    assert np.all(out[:, 9] == 0.0)


# ---------------------------------------------------------------- renders on the emulation

def _blocks(img, b=6):
    H, W = img.shape[:2]
    return img[: H // b * b, : W // b * b].reshape(H // b, b, W // b, b, 3).mean(axis=(1, 3))


def _estimate(d, algo, iters, seed0, rf=0.003, b=6):
    """mean and standard error per b x b block over 4 independent renders"""
    reps = []
    for k in range(4):
        r = ll.Emul4(d, algo, seed=seed0 + k, radius_factor=rf)
        for it in range(iters):
            r.run_iteration(it)
        reps.append(_blocks(r.framebuffer() / iters, b))
    reps = np.array(reps)
    return reps.mean(axis=0), reps.std(axis=0, ddof=1) / 2.0


def _agree(a, b, what):   # the bounds of test_envmap.py
    (m, s), (rm, rs) = a, b
    z = np.abs(m - rm) / np.sqrt(s ** 2 + rs ** 2 + (0.02 * rm) ** 2 + 1e-8)
    assert z.max() < 5.0, (what, float(z.max()))
    assert abs(m.mean() / rm.mean() - 1) < 0.05, (what, m.mean(), rm.mean())


def test_algorithms_agree_through_a_lens():
    """PT, BPT and VCM estimate the same defocused image of scene 3.  LT cannot render what is seen through the specular
    spheres or the background itself, and BPM's merges only converge as the radius shrinks, so these two are compared
    on a box without spheres lit by a point light (no light in view): LT per block against PT -- the check of the
    projection and the importance of the lens -- and BPM (a wider radius) per block."""
    d = ll.builtin_lens(R_STRONG, F_STRONG)
    pt = _estimate(d, 5, 24, 500)
    assert pt[0].mean() > 0.05
    _agree(_estimate(d, 3, 12, 300), pt, "bpt")
    _agree(_estimate(d, 4, 10, 400), pt, "vcm")
    box = ll.builtin_lens(R_STRONG, F_STRONG, mask=256 | 4)   # kGlossyFloor | kLightPoint
    # 3x3 blocks: at 6x6 a pinhole projection in the connection (no blur in LT) still passes; here it gives z ~ 20
    pt = _estimate(box, 5, 200, 510, b=3)
    _agree(_estimate(box, 0, 200, 10, b=3), pt, "lt")
    _agree(_estimate(box, 2, 48, 210, rf=0.02, b=3), pt, "bpm")


@pytest.mark.parametrize("algo", [0, 3, 4])
def test_lens_leaves_the_light_tape_alone(algo):
    """the lens draws from streams of its own: the light sub-paths draw exactly what they draw through the pinhole"""
    a = ll.Emul4(ll.builtin_lens(R_STRONG, F_STRONG, resx=20, resy=14), algo, seed=9)
    b = ll.Emul4(ll.builtin_lens(None, None, resx=20, resy=14), algo, seed=9)
    for it in range(2):
        a.run_iteration(it)
        b.run_iteration(it)
        assert np.array_equal(a.counts()[0], b.counts()[0])
    assert not np.array_equal(a.framebuffer(), b.framebuffer())


@pytest.mark.parametrize("algo", range(7))
def test_sharded_emulation_equals_unsharded(algo):
    """world 2: every pixel's camera path and every light path on one rank, with the lens points of the global path.
    Pixel-local renderers (PT, EyeLight) and PPM / BPM (no splats) are bit for bit; the splats of LT / BPT / VCM are
    summed in another order (rounding)"""
    d = ll.builtin_lens(R_STRONG, F_STRONG, resx=20, resy=14)
    full = ll.Emul4(d, algo, seed=3)
    shards = [ll.Emul4(d, algo, seed=3, rank=r, world=2) for r in range(2)]
    for it in range(2):
        full.run_iteration(it)
        for s in shards:
            s.run_iteration(it)
    fb = shards[0].framebuffer() + shards[1].framebuffer()
    assert np.count_nonzero(fb) > 0
    if algo in (1, 2, 5, 6):
        assert np.array_equal(fb, full.framebuffer())
    else:
        assert np.allclose(fb, full.framebuffer(), rtol=2e-6, atol=1e-7)
    for k in range(2):
        assert np.array_equal(np.concatenate([s.counts()[k] for s in shards]), full.counts()[k])


# ---------------------------------------------------------------- scene files and SceneBuilder

def _quad(tmp_path):
    (tmp_path / "quad.obj").write_text("mtllib quad.mtl\nv -1 -1 0\nv 1 -1 0\nv 1 1 0\nv -1 1 0\nusemtl white\nf 1 2 3 4\n")
    (tmp_path / "quad.mtl").write_text("newmtl white\nKd 0.8 0.8 0.8\n")


def test_scene_file_lens_directive(tmp_path):
    from smallvcm_amd.scene_file import load_scene
    _quad(tmp_path)
    (tmp_path / "s.vcmscene").write_text("obj quad.obj\ncamera 0 -4 2  0 1 -0.4  0 0 1  50\nlight background 1\n"
                                         "lens 0.125 4.5   # aperture, focus\n")
    d = load_scene(tmp_path / "s.vcmscene", 16, 12)
    assert isinstance(d, SceneDesc4) and d.lens
    assert (d.lens.contents.apertureRadius, d.lens.contents.focusDistance) == (0.125, 4.5)
    assert not d.base.envmap
    assert d.camera.resolution[0] == 16
    (tmp_path / "plain.vcmscene").write_text("obj quad.obj\nlight background 1\n")
    assert not isinstance(load_scene(tmp_path / "plain.vcmscene", 8, 8), SceneDesc4)
    # with an env map: the version-3 part carries the map
    img = el.sky(16, 8)
    (tmp_path / "sky.pfm").write_bytes(b"PF\n16 8\n-1\n" + img[::-1].astype("<f4").tobytes())
    (tmp_path / "e.vcmscene").write_text("obj quad.obj\nlight envmap sky.pfm 2.0\nlens 0.2 3\n")
    d = load_scene(tmp_path / "e.vcmscene", 8, 8)
    assert isinstance(d, SceneDesc4) and d.base.envmap and d.lens.contents.focusDistance == 3.0
    for bad in ("lens 0.1", "lens", "lens a 3", "lens 0.1 3 7", "lens -0.1 3", "lens 0.1 0", "lens 0.1 -1",
                "lens nan 3", "lens 0.1 inf", "lens 0.1 3\nlens 0.2 3"):
        (tmp_path / "bad.vcmscene").write_text("obj quad.obj\nlight background 1\n" + bad + "\n")
        with pytest.raises(ValueError, match="lens"):
            load_scene(tmp_path / "bad.vcmscene", 8, 8)


def test_scene_builder_thin_lens():
    from smallvcm_amd.scene2 import SceneBuilder
    L = load_library(require_gpu=False)

    def builder():
        b = SceneBuilder()
        m = b.material(diffuse=(0.7, 0.7, 0.7))
        b.triangle((-1, -1, 0), (1, -1, 0), (1, 1, 0), m)
        b.background_light(1.0)
        return b

    cam = ((0, -4, 2), (0, 1, -0.4), (0, 0, 1), 50, 16, 12)
    b = builder()
    b.thin_lens(0.25, 4.0)
    d = b.build(*cam)
    assert isinstance(d, SceneDesc4) and not d.base.envmap
    assert (d.lens.contents.apertureRadius, d.lens.contents.focusDistance) == (0.25, 4.0)
    plain = builder().build(*cam)
    assert not isinstance(plain, (SceneDesc3, SceneDesc4))
    assert bytes(d.camera) == bytes(plain.camera)
    e = ll.Emul4(d, 5, seed=1)   # the description is complete
    e.run_iteration(0)
    assert np.count_nonzero(e.framebuffer()) > 0
    b = builder()
    b.envmap_light(el.sky(8, 4))
    b.thin_lens(0.1, 2.0)
    d = b.build(*cam)
    assert isinstance(d, SceneDesc4) and d.base.envmap
    for r, f in ((-1, 2), (float("nan"), 2), (0.1, 0), (0.1, float("inf"))):
        with pytest.raises(ValueError):
            builder().thin_lens(r, f)
