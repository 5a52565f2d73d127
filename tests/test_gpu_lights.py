"""Spot and sphere lights on the GPU: the WithLights kernels against the host emulation of the same device functions
(tests/host_emul_lights), bit for bit -- framebuffer, random-number tapes and workload counters -- for every algorithm,
scene kind and execution order, with the table of the uniform choice and with POWER, under a thin lens plus an
environment map, under a tent filter, and with more lights than the pick table's LDS room; the known-answer ops one
call at a time; two shards against one context; vcm_render's scene-file path against the Python one; the feature
kernel and the technique planes on a frame that sees the bulb; and that a scene without the two types launches what it
launched."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import denoise_lib as dl
import envmap_lib as el
import lights_lib as L
import pick_lib as pl
from smallvcm_amd._abi import PART_COUNT, PART_EMISSION
from smallvcm_amd.renderer import HipBackend, VertexCM

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPLAT_ALGOS = (0, 3, 4)
STAT_KEYS = ("lightVertices", "lightRays", "cameraRays", "shadowRays", "mergeQueries", "mergeCandidates",
             "mergeAccepted", "connections", "lightSplats")
INFO_NODES, INFO_INT_PHONG, INFO_PICK = 2, 3, 6   # VCM_INFO_*
_fp = C.POINTER(C.c_float)


def _lights_kind(b):
    b.L.vcm_debug_lights_kind.argtypes = [C.c_void_p]
    info = (C.c_int * 11)()
    b.L.vcm_debug_context_info.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
    assert b.L.vcm_debug_context_info(b.ctx, info) == 0
    _lights_kind.last = info
    return b.L.vcm_debug_lights_kind(b.ctx), info[INFO_PICK]


def _compare(d, algo, strict, seed=77, iters=2, kind=None):
    """test_gpu_thin_lens.py::_compare over the lights emulation; 20 x 14 x 2 iterations = 280 paths per iteration:
    four full waves and a partial one"""
    emu = L.EmulL(d, algo, seed=seed)
    r = VertexCM(d, algo, 0.003, 0.75, seed, strict_order=strict)
    assert _lights_kind(r.backend) == (1, 1)
    if kind is not None:   # the switch took: a BVH / a list with the general pow / neither
        assert _lights_kind.last[INFO_NODES] == (1 if kind == "bvh" else 0)
        assert kind == "bvh" or _lights_kind.last[INFO_INT_PHONG] == (0 if kind == "list" else 1)
    r.mMinPathLength, r.mMaxPathLength = 0, 10
    for it in range(iters):
        emu.run_iteration(it, 0, 10)
        r.RunIteration(it)
        lc, cc = r.backend.rng_counts()
        elc, ecc = emu.counts()
        assert np.array_equal(lc, elc), "light tape"
        assert np.array_equal(cc, ecc), "camera tape"
        se, sg = emu.stats(), r.stats()
        for k in STAT_KEYS:
            assert se[k] == sg[k], (k, se[k], sg[k])
    gpu, host = r.framebuffer_sum(), emu.framebuffer()
    r.close()
    assert np.count_nonzero(host) > 0
    if strict and algo in SPLAT_ALGOS:   # strict mode splats with fp32 atomics: their order is not defined
        assert np.all(np.abs(gpu - host) <= 2e-5 * np.abs(host) + 2e-7), float(np.abs(gpu - host).max())
    else:
        assert np.array_equal(gpu.view(np.uint32), host.view(np.uint32))


def _set_kind(kind, monkeypatch):
    if kind == "bvh":
        monkeypatch.setenv("SMALLVCM_AMD_FORCE_BVH", "1")   # read when the scene is built: both sides
    if kind == "list":
        monkeypatch.setenv("SMALLVCM_AMD_GENERAL_POW", "1")


@pytest.mark.parametrize("strict", [False, True])
@pytest.mark.parametrize("kind", ["asbuilt", "list", "bvh"])
@pytest.mark.parametrize("algo", range(7))
def test_gpu_equals_host_emulation(monkeypatch, algo, kind, strict):
    """the room (a sphere light, a spot, an emissive triangle, a glass and a mirror sphere) as the kind its geometry
    takes, with general pow forced and behind a BVH: the uniform choice through the table, POWER, a thin lens plus an
    environment map (WithLights over WithPick over WithLens over an E kind) and a tent filter"""
    _set_kind(kind, monkeypatch)
    _compare(L.room(), algo, strict, kind=kind)
    _compare(L.room(pick="power", mix=0.1), algo, strict, kind=kind)
    _compare(L.room(pick="power", lens=(0.05, 3.5), sky=el.sky(32, 16, sun=(0.55, 0.2), sun_size=2, sun_value=(30.0, 27.0, 22.0))), algo, strict)
    _compare(L.room(flt=("tent", 1.5)), algo, strict)


@pytest.mark.parametrize("strict", [False, True])
@pytest.mark.parametrize("algo", [5, 3, 4])
def test_gpu_pick_table_beyond_lds(algo, strict):
    """262 lights with a bulb and a spot among them: the table the new kinds ride on in global memory (VCM_LDS_PICK = 256)"""
    d = L.many_lights_room()
    assert pl.n_lights(d) == 262
    _compare(d, algo, strict)


def _kat(b, op, inp):
    b.L.vcm_debug_kat.argtypes = [C.c_void_p, C.c_int, C.c_int, _fp, _fp]
    dev = np.zeros_like(inp)
    rc = b.L.vcm_debug_kat(b.ctx, op, len(inp), inp.ctypes.data_as(_fp), dev.ctypes.data_as(_fp))
    return rc, dev


@pytest.mark.parametrize("kind", ["asbuilt", "bvh"])
def test_device_known_answers_equal_the_host(kind, monkeypatch):
    """Emit, Illuminate, the emitter hit with and without the normal: 50 000 records over the room's three lights"""
    _set_kind(kind, monkeypatch)
    d = L.room(pick="power")
    rng = np.random.default_rng(8)
    n = 50000
    light = rng.integers(0, 3, n)
    u = L.uniforms(rng, (n, 4))
    v = rng.standard_normal((n, 6))
    unit = (v[:, 0:3] / np.linalg.norm(v[:, 0:3], axis=1, keepdims=True)).astype(np.float32)
    unit2 = (v[:, 3:6] / np.linalg.norm(v[:, 3:6], axis=1, keepdims=True)).astype(np.float32)
    recv = rng.uniform(-1.2, 1.2, (n, 3)).astype(np.float32)
    b = HipBackend(d, 4, 0.003, 0.75, 1234)
    try:
        for op, inp in ((L.OP_LIGHT_EMIT, L.emit_records(light, u)),
                        (L.OP_LIGHT_ILLUMINATE, L.illuminate_records(light, recv, u[:, 0:2])),
                        (L.OP_LIGHT_RADIANCE, L.radiance_at_records(light, unit, unit2)),
                        (L.OP_LIGHT_RADIANCE_AT, L.radiance_at_records(light, unit, unit2))):
            rc, dev = _kat(b, op, inp)
            assert rc == 0, b.L.vcm_last_error()
            host = L.kat(d, op, inp)
            assert np.count_nonzero(host) > 0
            assert np.array_equal(dev.view(np.uint32), host.view(np.uint32)), op
    finally:
        b.close()


def test_the_normal_op_needs_a_context_with_such_a_light():
    """a context whose scene has neither type launches no kernel that knows them: its op is refused, not answered wrongly"""
    d = pl.with_pick(pl.lamp_room(8, 8, n_dim=3), pl.POWER)
    b = HipBackend(d, 4, 0.003, 0.75, 1234)
    try:
        assert _lights_kind(b) == (0, 1)
        rc, _ = _kat(b, L.OP_LIGHT_RADIANCE_AT, L.radiance_at_records(np.zeros(4), np.ones((4, 3), np.float32), np.ones((4, 3), np.float32)))
        assert rc == -1 and b"needs a context with a spot or a sphere light" in b.L.vcm_last_error()
    finally:
        b.close()


@pytest.mark.parametrize("algo", range(7))
def test_a_scene_without_the_new_types_launches_what_it_launched(algo):
    """no table unless asked for, no WithLights kind ever; with either type: both, whatever the caller asked for"""
    for d, want in ((pl.lamp_room(8, 8, n_dim=3), (0, 0)), (pl.with_pick(pl.lamp_room(8, 8, n_dim=3), pl.POWER), (0, 1)),
                    (pl.with_pick(pl.lamp_room(8, 8, n_dim=3), pl.UNIFORM), (0, 0)), (L.room(8, 8), (1, 1)),
                    (L.room(8, 8, pick="uniform"), (1, 1)), (L.floor_scene("spot", 8), (1, 1))):
        b = HipBackend(d, algo, 0.003, 0.75, 1234)
        try:
            assert _lights_kind(b) == want
        finally:
            b.close()


@pytest.mark.parametrize("algo", [5, 0, 3, 4])
def test_two_thread_rank_shards_equal_one_context(algo):
    """vcm_create_sharded6, world 2: two rank threads on one device exchanging light records against one context -- the
    path tracer bit for bit, the splatting algorithms within rounding of the summation order"""
    import threading
    from smallvcm_amd.renderer import ShardedVertexCM
    from test_gpu_dropin_sharded import _ThreadCollectives
    d = L.room(pick="power", mix=0.1)
    world, iters = 2, 2
    coll = _ThreadCollectives(world)
    results, errors = [None] * world, []

    def run(rank):
        try:
            coll.bind(rank)
            b = HipBackend(d, algo, 0.003, 0.75, 3, device=0, rank=rank, world=world)
            r = ShardedVertexCM(b, rank, world)
            r.dist = coll
            r.mMaxPathLength, r.mMinPathLength = 10, 0
            for it in range(iters):
                r.RunIteration(it)
            results[rank] = r.framebuffer_sum()
            b.close()
        except Exception as e:   # noqa: BLE001
            errors.append(repr(e))
            try:
                coll.bar.abort()
            except Exception:
                pass

    ts = [threading.Thread(target=run, args=(k,)) for k in range(world)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(timeout=300)
    assert not errors, errors
    one = VertexCM(d, algo, 0.003, 0.75, 3)
    one.mMaxPathLength, one.mMinPathLength = 10, 0
    for it in range(iters):
        one.RunIteration(it)
    want = one.framebuffer_sum()
    one.close()
    assert np.count_nonzero(want) > 0
    for fb in results:
        if algo == 5:
            assert np.array_equal(fb, want)
        else:
            assert np.allclose(fb, want, rtol=2e-6, atol=2e-7)


def test_vcm_render_scene_file_equals_python(tmp_path):
    from smallvcm_amd.scene_file import load_scene
    (tmp_path / "room.obj").write_text(
        "mtllib room.mtl\nv -2 -2 0\nv 2 -2 0\nv 2 2 0\nv -2 2 0\nv -2 2 3\nv 2 2 3\nv -0.3 -0.3 0\nv 0.3 -0.3 0\nv 0 0.2 0.6\n"
        "usemtl white\nf 1 2 3 4\nf 4 3 6 5\nusemtl red\nf 7 8 9\n")
    (tmp_path / "room.mtl").write_text("newmtl white\nKd 0.8 0.8 0.8\nnewmtl red\nKd 0.7 0.2 0.2\nKs 0.2 0.2 0.2\nNs 40\n")
    (tmp_path / "s.vcmscene").write_text("obj room.obj\ncamera 0 -4 2  0 1 -0.45  0 0 1  50\n"
                                         "light spot -1 -1 2.5  1 1 -2  3 3 4  35 20\n"
                                         "light sphere 0.6 0.4 1.2 0.25  9 8 6\nlightpick power 0.1\n")
    res, iters, seed = (24, 18), 2, 4321
    exe = os.path.join(ROOT, "smallvcm_amd", "host", "vcm_render")
    out = tmp_path / "out.pfm"
    p = subprocess.run([exe, "--scene-file", str(tmp_path / "s.vcmscene"), "-a", "vcm", "-i", str(iters), "--res",
                        str(res[0]), str(res[1]), "--seed", str(seed), "-o", str(out), "--light-pick-report"],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    data = out.read_bytes()
    img = np.frombuffer(data[len(b"PF\n%d %d\n-1\n" % res):], np.float32).reshape(res[1], res[0], 3)
    d = load_scene(tmp_path / "s.vcmscene", *res)
    assert pl.n_lights(d) == 2
    r = VertexCM(d, 4, 0.003, 0.75, seed)
    r.mMaxPathLength = 10
    for it in range(iters):
        r.RunIteration(it)
    want = r.GetFramebuffer()
    r.close()
    assert np.count_nonzero(want) > 0
    assert np.array_equal(img.view(np.uint32), want.view(np.uint32))
    assert "(spot): pmf" in p.stdout and "(sphere): pmf" in p.stdout, p.stdout


def _same_bits(a, b):
    return np.ascontiguousarray(a, np.float32).tobytes() == np.ascontiguousarray(b, np.float32).tobytes()


@pytest.mark.parametrize("kind", ["asbuilt", "bvh"])
def test_features_of_a_frame_that_sees_the_bulb_equal_the_emulation(kind, monkeypatch):
    """a hit on the sphere light is an emitter hit: the sphere's normal and depth, albedo 1, as for an emissive triangle"""
    _set_kind(kind, monkeypatch)
    d = L.floor_scene("sphere", 31)
    _, inside = L.bulb_pixel_masks(d, 31, 1)
    assert inside.sum() >= 8
    b = HipBackend(d, 4, 0.003, 0.75, 1234)
    try:
        g = np.zeros((31, 31, 4), np.float32)
        g[..., :3], g[..., 3] = b.feature("normal"), b.feature("depth")
        a = b.feature("albedo")
    finally:
        b.close()
    eg, ea = dl.features(d.base)
    assert _same_bits(g, eg) and _same_bits(a, ea[..., :3])
    assert np.all(a[inside] == 1.0) and np.all(g[inside][:, 3] > 0)
    org = np.array(L.FLOOR_CAMERA[0])
    hit = org + g[inside][:, 3:4].astype(np.float64) * L.camera_rays(d, np.argwhere(inside)[:, ::-1] + 0.5)[1]
    assert np.all(np.abs((hit - np.array(L.BULB_CENTRE)) / L.BULB_RADIUS - g[inside][:, :3]) <= 1e-4)   # the outward normal


@pytest.mark.parametrize("algo", [3, 4])
def test_parts_with_a_visible_bulb(algo):
    """tracking does not disturb the framebuffer (bit for bit), the five planes add up to it (test_parts.py's bound for two
    orders of the same addends), and the pixels that see only the bulb hold its radiance in the emission plane alone"""
    d = L.floor_scene("sphere")
    _, inside = L.bulb_pixel_masks(d)
    K = 3
    b, plain = HipBackend(d, algo, 0.003, 0.75, 1234), HipBackend(d, algo, 0.003, 0.75, 1234)
    try:
        b.track_parts()
        for it in range(K):
            b.run_iteration(it, 0, 10)
            plain.run_iteration(it, 0, 10)
        fb, ref = b.framebuffer_sum(), plain.framebuffer_sum()
        planes = np.stack([b.part(i, 1.0) for i in range(PART_COUNT)])
        splats = b.stats()["lightSplats"]
    finally:
        b.close()
        plain.close()
    assert _same_bits(fb, ref)
    m = K * (splats + 4 * (1 + 10 * 12))
    S = planes.astype(np.float64).sum(axis=0)
    assert (planes >= 0).all() and (np.abs(S - fb) <= 2.0 * m * 2.0 ** -24 * fb).all()
    want = K * np.array(L.BULB_L)
    assert np.all(np.abs(planes[PART_EMISSION][inside] - want) <= 1e-6 * want)
    others = [i for i in range(PART_COUNT) if i != PART_EMISSION]
    assert not np.any(planes[others][:, inside])
    assert _same_bits(planes[PART_EMISSION][inside], fb[inside])
