"""The environment-map light (VCM_LIGHT_ENVMAP) on the CPU: the map loaders, dm_atan2f / dm_acosf, the light functions
through known-answer records of the host emulation (tests/host_emul_envmap), unbiasedness of the emulated renderer,
and a sharded emulation.  Maps are procedural (envmap_lib.sky)."""
import ctypes as C
import struct

import numpy as np
import pytest
from scipy.stats import chi2

import envmap_lib as el
from smallvcm_amd._abi import SceneDesc3
from smallvcm_amd.renderer import cornell_scene, load_library

OP_EMIT, OP_ILLUMINATE, OP_RADIANCE = 4, 5, 6
KAT = 16
INV_PI_F = np.float32(1.0) / np.float32(3.14159265358979)


@pytest.fixture(scope="module")
def E():
    return el.emul_envmap()   # builds tests/host_emul_envmap


def _lib():
    L = load_library(require_gpu=False)
    L.vcm_envmap_load.restype = C.c_void_p
    L.vcm_envmap_load.argtypes = [C.c_char_p]
    L.vcm_envmap_free.argtypes = [C.c_void_p]
    L.vcm_envmap_free.restype = None
    L.vcm_scene_load_error.restype = C.c_char_p
    return L


def _load(path):
    L = _lib()
    h = L.vcm_envmap_load(str(path).encode())
    if not h:
        return None, L.vcm_scene_load_error().decode()
    m = C.cast(h, C.POINTER(el.EnvMap)).contents
    img = np.ctypeslib.as_array(m.rgb, shape=(m.height, m.width, 3)).copy()
    L.vcm_envmap_free(h)
    return img, None


# ---------------------------------------------------------------- loaders

def _rgbe_bytes(rng, W, H):
    b = rng.integers(0, 256, size=(H, W, 4)).astype(np.uint8)
    b[..., 3] = rng.integers(120, 140, size=(H, W))
    b[:, :3, :] = b[:, 3:4, :]     # runs for the encoder
    b[0, 0, 3] = 0                 # E = 0: black
    return b


def _decode_rgbe(b):
    f = np.where(b[..., 3:4] > 0, np.ldexp(1.0, b[..., 3:4].astype(np.int32) - 136), 0.0)
    return (b[..., :3].astype(np.float64) * f).astype(np.float32)


def _rle_channel(v):
    out, i, n = bytearray(), 0, len(v)
    while i < n:
        j = i
        while j < n and j - i < 127 and v[j] == v[i]:
            j += 1
        if j - i >= 3:
            out += bytes([128 + j - i, v[i]])
            i = j
        else:
            j = i
            while j < n and j - i < 128 and not (j + 2 < n and v[j] == v[j + 1] == v[j + 2]):
                j += 1
            out += bytes([j - i]) + bytes(v[i:j])
            i = j
    return bytes(out)


def _write_hdr(path, b, rle, header="#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n", res=None):
    H, W = b.shape[:2]
    data = bytearray((header + (res or "-Y %d +X %d\n" % (H, W))).encode())
    for y in range(H):
        if rle:
            data += bytes([2, 2, W >> 8, W & 255])
            for c in range(4):
                data += _rle_channel(b[y, :, c].tobytes())
        else:
            data += b[y].tobytes()
    path.write_bytes(bytes(data))
    return bytes(data)


@pytest.mark.parametrize("rle", [False, True])
def test_hdr_loader_round_trip(tmp_path, rle):
    b = _rgbe_bytes(np.random.default_rng(1), 37, 11)
    _write_hdr(tmp_path / "m.hdr", b, rle)
    img, err = _load(tmp_path / "m.hdr")
    assert err is None, err
    assert img.shape == (11, 37, 3)
    assert np.array_equal(img, _decode_rgbe(b))   # row 0 of the file = row 0 of the map (the top)


@pytest.mark.parametrize("little", [True, False])
def test_pfm_loader_round_trip_and_flip(tmp_path, little):
    rng = np.random.default_rng(2)
    img = (rng.random((9, 13, 3)) * 5).astype(np.float32)
    rows = img[::-1]   # PFM rows run bottom-up
    data = rows.astype("<f4" if little else ">f4").tobytes()
    (tmp_path / "m.pfm").write_bytes(b"PF\n13 9\n%s\n" % (b"-1.0" if little else b"1.0") + data)
    got, err = _load(tmp_path / "m.pfm")
    assert err is None, err
    assert np.array_equal(got, img)


def test_loaders_reject_bad_files(tmp_path):
    b = _rgbe_bytes(np.random.default_rng(3), 16, 4)
    full = _write_hdr(tmp_path / "ok.hdr", b, True)
    cases = {
        "trunc.hdr": full[: len(full) - 7],
        "trunc_hdr_header.hdr": b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n",
        "badmagic.hdr": b"#?NOTRADIANCE\n\n-Y 1 +X 1\n\x00\x00\x00\x00",
        "format.hdr": b"#?RADIANCE\nFORMAT=32-bit_rle_xyze\n\n-Y 1 +X 1\n\x00\x00\x00\x00",
        "orient.hdr": b"#?RADIANCE\n\n+Y 1 +X 1\n\x00\x00\x00\x00",
        "huge.hdr": b"#?RADIANCE\n\n-Y 5000 +X 9000\n",
        "trunc.pfm": b"PF\n4 4\n-1\n" + b"\x00" * 100,
        "badhdr.pfm": b"PF\nfour 4\n-1\n" + b"\x00" * 192,
        "gray.pfm": b"Pf\n4 4\n-1\n" + b"\x00" * 64,
        "nan.pfm": b"PF\n1 1\n-1\n" + struct.pack("<3f", 1.0, float("nan"), 1.0),
        "neg.pfm": b"PF\n1 1\n-1\n" + struct.pack("<3f", 1.0, -0.5, 1.0),
        "inf.pfm": b"PF\n1 1\n-1\n" + struct.pack("<3f", float("inf"), 0.5, 1.0),
    }
    for name, data in cases.items():
        (tmp_path / name).write_bytes(data)
        img, err = _load(tmp_path / name)
        assert img is None and err, name
    assert _load(tmp_path / "missing.hdr")[1].startswith("cannot open")


def test_scene_file_envmap_directive(tmp_path):
    from smallvcm_amd.scene_file import load_scene
    img = el.sky(16, 8)
    (tmp_path / "sky.pfm").write_bytes(b"PF\n16 8\n-1\n" + img[::-1].astype("<f4").tobytes())
    (tmp_path / "quad.obj").write_text("mtllib quad.mtl\nv -1 -1 0\nv 1 -1 0\nv 1 1 0\nv -1 1 0\nusemtl white\nf 1 2 3 4\n")
    (tmp_path / "quad.mtl").write_text("newmtl white\nKd 0.8 0.8 0.8\n")
    (tmp_path / "s.vcmscene").write_text("obj quad.obj\ncamera 0 -4 2  0 1 -0.4  0 0 1  50\nlight envmap sky.pfm 2.0\n")
    d = load_scene(tmp_path / "s.vcmscene", 16, 12)
    assert isinstance(d, SceneDesc3) and d.envmap
    m = d.envmap.contents
    assert (m.width, m.height) == (16, 8)
    assert np.array_equal(np.ctypeslib.as_array(m.rgb, shape=(8, 16, 3)), img)
    assert d.base.lights[d.base.backgroundLight].type == 4 and d.base.lights[d.base.backgroundLight].scale == 2.0
    (tmp_path / "plain.vcmscene").write_text("obj quad.obj\nlight background 1\n")
    assert not isinstance(load_scene(tmp_path / "plain.vcmscene", 8, 8), SceneDesc3)
    (tmp_path / "bad.vcmscene").write_text("obj quad.obj\nlight envmap missing.hdr 1\n")
    with pytest.raises(ValueError, match="missing.hdr"):
        load_scene(tmp_path / "bad.vcmscene", 8, 8)


def test_create3_rejects_bad_descriptions(E):
    """the library's checks run before it looks for a device; the emulation shares them (scene_host.h)"""
    L = _lib()
    L.vcm_create3.restype = C.c_void_p
    L.vcm_create3.argtypes = [C.POINTER(SceneDesc3), C.c_int, C.c_float, C.c_float, C.c_int]
    L.vcm_last_error.restype = C.c_char_p

    def rejected(d, what):
        assert not L.vcm_create3(C.byref(d), 4, 0.003, 0.75, 1), what
        assert L.vcm_last_error().decode(), what
        assert not E.emul_create3(C.byref(d), 4, 0.003, 0.75, 1, 0, 1), what
        return E.emul_envmap_error().decode()

    good = el.sky(8, 4)
    for img, what in [(np.where(np.arange(8 * 4 * 3).reshape(4, 8, 3) == 5, np.nan, good), "nan"),
                      (np.where(np.arange(8 * 4 * 3).reshape(4, 8, 3) == 7, -1.0, good), "negative"),
                      (np.zeros((4, 8, 3)), "black"), (np.ones((4097, 1, 3)), "too tall")]:
        rejected(el.builtin_with_envmap(img.astype(np.float32)), what)
    d = el.builtin_with_envmap(good)
    d.base.lights[d.base.backgroundLight].type = 3     # a map without an env light
    assert "without an env-map light" in rejected(d, "no light")
    d = el.builtin_with_envmap(good)
    d.envmap = None                                   # an env light without a map
    assert "without a map" in rejected(d, "no map")
    d = el.builtin_with_envmap(good)
    d.base.backgroundLight = -1                       # an env light that is not the background
    assert "backgroundLight" in rejected(d, "not background")
    # the version-2 entry points refuse an env light outright
    L.vcm_create2.restype = C.c_void_p
    L.vcm_create2.argtypes = [C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_int]
    assert not L.vcm_create2(C.byref(el.builtin_with_envmap(good).base), 4, 0.003, 0.75, 1)


# ---------------------------------------------------------------- detmath

def test_atan2_acos_error_bounds(E):
    fp = C.POINTER(C.c_float)
    n = 1 << 22
    a = np.linspace(-np.pi, np.pi, n)
    out = np.zeros(n, np.float32)
    for r in (1e-30, 1e-3, 1.0, 1e3, 1e30):
        y, x = (np.sin(a) * r).astype(np.float32), (np.cos(a) * r).astype(np.float32)
        E.emul_atan2f_n(n, y.ctypes.data_as(fp), x.ctypes.data_as(fp), out.ctypes.data_as(fp))
        d = np.abs(out - np.arctan2(y.astype(np.float64), x.astype(np.float64)))
        assert np.minimum(d, 2 * np.pi - d).max() <= 2.8e-7, r
    z = np.linspace(-1, 1, n).astype(np.float32)
    E.emul_acosf_n(n, z.ctypes.data_as(fp), out.ctypes.data_as(fp))
    assert np.abs(out - np.arccos(z.astype(np.float64))).max() <= 2.9e-7
    E.emul_atan2f_n(1, np.zeros(1, np.float32).ctypes.data_as(fp), np.zeros(1, np.float32).ctypes.data_as(fp), out.ctypes.data_as(fp))
    assert out[0] == 0.0


@pytest.mark.parametrize("W,H", [(7, 3), (64, 32), (2048, 1024)])
def test_texel_centre_round_trip(E, W, H):
    d = el.builtin_with_envmap(np.ones((H, W, 3), np.float32))
    jj, ii = np.meshgrid(np.arange(W), np.arange(H))
    uv = np.stack([(jj.ravel() + 0.5) / W, (ii.ravel() + 0.5) / H], axis=1)
    idx, pdf = el.lookup(d, el.uv_dirs(uv))
    assert np.array_equal(idx, np.arange(W * H))
    assert np.all(pdf > 0)


# ---------------------------------------------------------------- the light functions

@pytest.fixture(scope="module")
def sun_scene():
    return el.builtin_with_envmap(el.sky(32, 16, sun=(0.3, 0.25), sun_size=2), scale=1.5)


def _records(op, rx, ry, light, extra=None):
    inp = np.zeros((len(rx), KAT), np.float32)
    inp[:, 0] = light
    if op == OP_EMIT:
        inp[:, 1], inp[:, 2] = rx, ry
        inp[:, 3], inp[:, 4] = extra
    elif op == OP_ILLUMINATE:
        inp[:, 1:4] = (0.1, -0.2, 0.3)
        inp[:, 4], inp[:, 5] = rx, ry
    return inp


def _rnd(n, seed):
    rng = np.random.default_rng(seed)
    return rng.random(n, dtype=np.float32), rng.random(n, dtype=np.float32)


def test_illuminate_and_emit_agree_with_get_radiance(sun_scene):
    d, n = sun_scene, 100000
    bg = d.base.backgroundLight
    rx, ry = _rnd(n, 5)
    il = el.kat3(d, OP_ILLUMINATE, _records(OP_ILLUMINATE, rx, ry, bg))
    dirs = il[:, 3:6]
    rad_in = np.zeros((n, KAT), np.float32)
    rad_in[:, 0] = bg
    rad_in[:, 1:4] = dirs
    gr = el.kat3(d, OP_RADIANCE, rad_in)
    assert np.array_equal(il[:, 0:3].view(np.uint32), gr[:, 0:3].view(np.uint32))      # radiance
    assert np.array_equal(il[:, 7:9].view(np.uint32), gr[:, 3:5].view(np.uint32))      # directPdfW, emissionPdfW
    assert np.all(il[:, 6] == np.float32(1e36)) and np.all(il[:, 9] == 1.0)
    assert np.count_nonzero(il[:, 0]) > 0.99 * n
    px, py = _rnd(n, 6)
    em = el.kat3(d, OP_EMIT, _records(OP_EMIT, rx, ry, bg, (px, py)))
    assert np.array_equal(em[:, 6:9], -dirs)                                            # the photon travels along -d
    assert np.array_equal(em[:, 0:3], il[:, 0:3])                                        # radiance texel(d)
    assert np.array_equal(em[:, 10], il[:, 7])                                           # directPdfA = pdf(d)
    want = (em[:, 10] * INV_PI_F) * np.float32(d.base.invSceneRadiusSqr)
    assert np.array_equal(em[:, 9].view(np.uint32), want.view(np.uint32))               # emissionPdfW
    # the photon starts on the disc at distance R on the side it comes FROM
    off = em[:, 3:6].astype(np.float64) - np.array(d.base.sceneCenter[:])
    assert np.allclose(np.einsum("ij,ij->i", off, dirs.astype(np.float64)), d.base.sceneRadius, rtol=1e-4)
    assert np.all(em[:, 12] == 0) and np.all(em[:, 13] == 0)                            # infinite, not delta


def test_sampled_texels_follow_the_table(sun_scene):
    d, n = sun_scene, 200000
    tex, marg, cond = el.tables(d)
    H, W = tex.shape[:2]
    assert marg[0] == 0 and marg[-1] == 1 and np.all(cond[:, 0] == 0) and np.all(cond[:, -1] == 1)
    p = np.diff(marg.astype(np.float64))[:, None] * np.diff(cond.astype(np.float64), axis=1)
    rx, ry = _rnd(n, 7)
    il = el.kat3(d, OP_ILLUMINATE, _records(OP_ILLUMINATE, rx, ry, d.base.backgroundLight))
    idx, _ = el.lookup(d, il[:, 3:6])
    counts = np.bincount(idx, minlength=W * H).astype(np.float64)
    exp = p.ravel() * n
    assert counts[exp == 0].sum() <= 1e-4 * n     # texel-edge rounding may land on a black neighbour, rarely
    big, small = exp >= 5, (exp > 0) & (exp < 5)
    obs, ex = counts[big], exp[big]
    if small.any():
        obs, ex = np.append(obs, counts[small].sum()), np.append(ex, exp[small].sum())
    stat = ((obs - ex) ** 2 / ex).sum()
    assert chi2.sf(stat, len(ex) - 1) > 1e-3, stat


def test_pdf_integrates_to_one(sun_scene):
    d, M = sun_scene, 1024
    rng = np.random.default_rng(8)
    jj, ii = np.meshgrid(np.arange(2 * M), np.arange(M))
    uv = np.stack([(jj.ravel() + rng.random(jj.size)) / (2 * M), (ii.ravel() + rng.random(ii.size)) / M], axis=1)
    _, pdf = el.lookup(d, el.uv_dirs(uv))
    integral = (pdf.astype(np.float64) * np.sin(np.pi * uv[:, 1])).sum() * (2 * np.pi * np.pi) / uv.shape[0]
    assert abs(integral - 1.0) < 1e-3, integral


# ---------------------------------------------------------------- renders on the emulation

def _mean_image(scene, algo, iters, seed):
    r = el.Emul3(scene, algo, seed=seed)
    for it in range(iters):
        r.run_iteration(it)
    return r.framebuffer() / iters


def _blocks(img, b=6):
    H, W = img.shape[:2]
    return img[: H // b * b, : W // b * b].reshape(H // b, b, W // b, b, 3).mean(axis=(1, 3))


def _estimate(d, algo, iters, seed0, rf=0.003):
    """mean and standard error per 6x6 block over 4 independent renders"""
    reps = []
    for k in range(4):
        r = el.Emul3(d, algo, seed=seed0 + k, radius_factor=rf)
        for it in range(iters):
            r.run_iteration(it)
        reps.append(_blocks(r.framebuffer() / iters))
    reps = np.array(reps)
    return reps.mean(axis=0), reps.std(axis=0, ddof=1) / 2.0


def _agree(a, b, what):
    (m, s), (rm, rs) = a, b
    z = np.abs(m - rm) / np.sqrt(s ** 2 + rs ** 2 + (0.02 * rm) ** 2 + 1e-8)
    assert z.max() < 5.0, (what, float(z.max()))
    assert abs(m.mean() / rm.mean() - 1) < 0.05, (what, m.mean(), rm.mean())


def test_algorithms_agree_on_an_envmap_scene():
    """PT, BPT and VCM estimate the same image of scene 3 with a sky + sun map: per 6x6 block and channel within
    5 sigma (sigma from 4 independent renders each, plus 2 % for the heavy-tailed sun paths).  LT cannot render what
    is seen through the specular spheres or the sky itself (nothing connects them to the pinhole), and BPM's merges
    only converge as the radius shrinks, so these two are compared on the box without spheres: LT per block against PT,
    BPM (a wider radius) by its mean."""
    sun = dict(sun=(0.55, 0.2), sun_size=3, sun_value=(20.0, 18.0, 15.0))
    d = el.builtin_with_envmap(el.sky(64, 32, **sun), resx=24, resy=24)
    pt = _estimate(d, 5, 24, 500)
    assert pt[0].mean() > 0.05
    _agree(_estimate(d, 3, 12, 300), pt, "bpt")
    _agree(_estimate(d, 4, 10, 400), pt, "vcm")
    box = el.builtin_with_envmap(el.sky(64, 32, **sun), resx=24, resy=24, mask=256 | 8)   # kGlossyFloor | kLightBackground
    pt = _estimate(box, 5, 24, 510)
    _agree(_estimate(box, 0, 24, 10), pt, "lt")
    bpm = _estimate(box, 2, 48, 210, rf=0.02)
    assert abs(bpm[0].mean() / pt[0].mean() - 1) < 0.08, (bpm[0].mean(), pt[0].mean())


def test_constant_map_equals_the_background_light():
    """a map of the BackgroundLight's colour renders what the BackgroundLight renders (different sampling, same
    integral): the mean images agree within their noise"""
    from emul_lib import Emul
    col = np.array([135, 206, 250], np.float32) / np.float32(255)
    d = el.builtin_with_envmap(np.tile(col, (16, 32, 1)), resx=24, resy=24)
    bg = cornell_scene(3, 24, 24)
    for algo, iters in ((5, 40), (4, 16)):
        a = _blocks(_mean_image(d, algo, iters, seed=11))
        r = Emul(bg, algo, seed=12)
        for it in range(iters):
            r.run_iteration(it, 0, 10)
        b = _blocks(r.framebuffer() / iters)
        assert abs(a.mean() / b.mean() - 1) < 0.03, (algo, a.mean(), b.mean())
        assert np.abs(a - b).max() < 0.25 * b.max(), algo


@pytest.mark.parametrize("algo", [5, 6, 3])
def test_sharded_emulation_equals_unsharded(algo):
    """world 2: every pixel's camera path and every light path on one rank; the ranks' framebuffers summed.  Pixel-local
    renderers (PT, EyeLight) are bit for bit; BPT's light splats are summed in another order (rounding)"""
    d = el.builtin_with_envmap(el.sky(32, 16), resx=20, resy=14)
    full = el.Emul3(d, algo, seed=3)
    shards = [el.Emul3(d, algo, seed=3, rank=r, world=2) for r in range(2)]
    for it in range(2):
        full.run_iteration(it)
        for s in shards:
            s.run_iteration(it)
    fb = shards[0].framebuffer() + shards[1].framebuffer()
    if algo in (5, 6):
        assert np.array_equal(fb, full.framebuffer())
    else:
        assert np.allclose(fb, full.framebuffer(), rtol=2e-6, atol=1e-7)
    for k in range(2):
        assert np.array_equal(np.concatenate([s.counts()[k] for s in shards]), full.counts()[k])
