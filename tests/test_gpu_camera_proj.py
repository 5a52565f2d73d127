"""The fisheye and the panorama on the GPU: the WithLens kernels, which a context with either projection launches,
against the host emulation of the same device functions (tests/host_emul_proj), bit for bit -- framebuffer,
random-number tapes and workload counters -- for every algorithm, scene kind, execution order and both projections; beside
an env map and a B-spline filter, spot and sphere lights with a POWER table, the Sobol sampler, a GGX material, and all of
them at once; the known-answer op; the default unchanged; two shards against one context; the feature kernel; the tracked
parts; vcm_render on a scene file with a `projection` line."""
import ctypes as C
import os
import subprocess
import threading

import numpy as np
import pytest

import envmap_lib as el
import proj_lib as pl
from smallvcm_amd._abi import SceneDesc9, with_projection
from smallvcm_amd.renderer import HipBackend, VertexCM

pytestmark = pytest.mark.gpu

SPLAT_ALGOS = (0, 3, 4)
STAT_KEYS = ("lightVertices", "lightRays", "cameraRays", "shadowRays", "mergeQueries", "mergeCandidates",
             "mergeAccepted", "connections", "lightSplats")
PROJECTIONS = {"fisheye": ("fisheye", 220.0), "panorama": ("panorama",)}
_fp = C.POINTER(C.c_float)


def _set_kind(kind, monkeypatch):
    if kind == "bvh":
        monkeypatch.setenv("SMALLVCM_AMD_FORCE_BVH", "1")   # read when the scene is built: both sides
    if kind == "list":
        monkeypatch.setenv("SMALLVCM_AMD_GENERAL_POW", "1")


def _debug_projection(backend):
    kind, fov = C.c_int(-1), C.c_float(-1.0)
    backend.L.vcm_debug_projection.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_float)]
    return backend.L.vcm_debug_projection(backend.ctx, C.byref(kind), C.byref(fov)), kind.value, fov.value


def _compare(d, algo, strict, seed=77, iters=2, rf=0.003):
    emu = pl.Emul9(d, algo, seed=seed, radius_factor=rf)
    r = VertexCM(d, algo, rf, 0.75, seed, strict_order=strict)
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
    model = d.model.contents
    assert _debug_projection(r.backend) == (1, model.kind, model.fovDegrees)
    r.close()
    assert np.count_nonzero(host) > 0
    if strict and algo in SPLAT_ALGOS:   # strict mode splats with fp32 atomics: their order is not defined (as test_gpu_pixel_filter.py)
        assert np.all(np.abs(gpu - host) <= 2e-5 * np.abs(host) + 2e-7), float(np.abs(gpu - host).max())
    else:
        assert np.array_equal(gpu.view(np.uint32), host.view(np.uint32))


@pytest.mark.parametrize("proj", sorted(PROJECTIONS))
@pytest.mark.parametrize("strict", [False, True])
@pytest.mark.parametrize("kind", ["rects", "list", "bvh"])
@pytest.mark.parametrize("algo", range(7))
def test_gpu_equals_host_emulation(monkeypatch, algo, kind, strict, proj):
    """The room is a list of axis-aligned rectangles and a sphere: WithLens over SceneRects; with general pow forced, over
    SceneList; with a BVH forced, over SceneBvh.  20 x 14: a partial workgroup"""
    _set_kind(kind, monkeypatch)
    _compare(pl.box(20, 14, proj=PROJECTIONS[proj], room=True), algo, strict)


@pytest.mark.parametrize("proj", sorted(PROJECTIONS))
@pytest.mark.parametrize("strict", [False, True])
@pytest.mark.parametrize("algo", SPLAT_ALGOS)
def test_gpu_equals_host_emulation_at_67_by_45(algo, strict, proj):
    """the three algorithms that connect to the camera, at a size that is no multiple of the wave or the workgroup"""
    _compare(pl.box(67, 45, proj=PROJECTIONS[proj], room=True), algo, strict)


@pytest.mark.parametrize("proj", sorted(PROJECTIONS))
@pytest.mark.parametrize("strict", [False, True])
@pytest.mark.parametrize("algo", [5, 0, 3, 4, 2])
def test_gpu_projection_beside_every_other_widening(algo, strict, proj):
    p = PROJECTIONS[proj]
    sky = el.sky(48, 24, sun=(0.55, 0.2), sun_size=2, sun_value=(30.0, 27.0, 22.0))
    _compare(pl.box(20, 14, proj=p, room=True, sky=sky, flt=("bspline", 2.0)), algo, strict)
    _compare(pl.box(20, 14, proj=p, room=True, lights=True, pick=("power", 0.25)), algo, strict)
    _compare(pl.box(20, 14, proj=p, room=True, sampler="sobol"), algo, strict)
    _compare(pl.box(20, 14, proj=p, room=True, ggx=True), algo, strict)
    _compare(pl.box(20, 14, proj=p, room=True, sky=sky, flt=("bspline", 2.0), lights=True, pick=("power", 0.25), sampler="sobol", ggx=True),
             algo, strict)


def _device_kat(backend, op, inp):
    backend.L.vcm_debug_kat.argtypes = [C.c_void_p, C.c_int, C.c_int, _fp, _fp]
    inp = np.ascontiguousarray(inp, np.float32)
    dev = np.zeros_like(inp)
    rc = backend.L.vcm_debug_kat(backend.ctx, op, len(inp), inp.ctypes.data_as(_fp), dev.ctypes.data_as(_fp))
    return rc, dev


@pytest.mark.parametrize("proj,W,H", [(("fisheye", 180.0), 48, 48), (("fisheye", 300.0), 36, 24), (("panorama",), 64, 32), (("panorama",), 37, 23)])
def test_device_op_equals_the_host(proj, W, H):
    """VCM_KAT_PROJECTION on the 50 000 records of test_camera_proj.py, bit for bit"""
    d = pl.box(W, H, proj=proj)
    rec = pl.records(d)
    b = HipBackend(d, 4, 0.003, 0.75, 1234)
    host = pl.kat9(d, rec)
    rc, dev = _device_kat(b, pl.OP_PROJECTION, rec)
    b.close()
    assert rc == 0
    assert np.count_nonzero(host[:, 4]) > 0.3 * len(host) and np.count_nonzero(host[:, 7]) > 0.1 * len(host)
    assert np.array_equal(dev.view(np.uint32), host.view(np.uint32))


@pytest.mark.parametrize("algo", range(7))
def test_default_is_unchanged(algo):
    """vcm_create9 with model NULL and with kind PERSPECTIVE = vcm_create8, bit for bit, on the kernels of version 8
    (vcm_debug_projection, VCM_INFO_LENS); the op is refused there; a projection changes the image"""
    import capacity_lib as cl
    d8 = pl.as_desc8(pl.box(20, 14, room=True))
    out = []
    for d, want in ((d8, (0, 0, 0.0)), (with_projection(d8, None), (0, 0, 0.0)), (with_projection(d8, "perspective", 90.0), (0, 0, 0.0)),
                    (with_projection(d8, "fisheye", 200.0), (1, 1, 200.0))):
        r = VertexCM(d, algo, 0.003, 0.75, 31)
        r.mMaxPathLength = 10
        for it in range(2):
            r.RunIteration(it)
        assert _debug_projection(r.backend) == want
        assert cl.context_info(r.backend)["lens"] == 0
        rc, _ = _device_kat(r.backend, pl.OP_PROJECTION, np.zeros((4, pl.KAT), np.float32))
        assert (rc == 0) == (want[0] == 1)
        if rc != 0:
            assert b"VCM_KAT_PROJECTION" in r.backend.L.vcm_last_error()
        out.append((r.framebuffer_sum(), r.backend.rng_counts(), r.stats()))
        r.close()
    assert np.count_nonzero(out[0][0]) > 0
    for fb, (lc, cc), st in out[1:3]:
        assert np.array_equal(fb.view(np.uint32), out[0][0].view(np.uint32))
        assert np.array_equal(lc, out[0][1][0]) and np.array_equal(cc, out[0][1][1])
        for k in STAT_KEYS:
            assert st[k] == out[0][2][k]
    assert not np.array_equal(out[3][0], out[0][0])


@pytest.mark.parametrize("proj", sorted(PROJECTIONS))
@pytest.mark.parametrize("algo", [5, 0, 4, 2])
def test_two_thread_rank_shards_equal_one_context(algo, proj):
    """vcm_create_sharded9, world 2: two rank threads on one device exchanging light records against one context -- the
    path tracer bit for bit, the others within rounding of the summation order"""
    from smallvcm_amd.renderer import ShardedVertexCM
    from test_gpu_dropin_sharded import _ThreadCollectives
    d = pl.box(20, 14, proj=PROJECTIONS[proj], room=True, flt=("tent", 1.5))
    world, iters = 2, 3
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


@pytest.mark.parametrize("ggx", [False, True])
@pytest.mark.parametrize("proj", sorted(PROJECTIONS))
def test_features_equal_the_emulation(proj, ggx):
    """vcm_render_features through the projection (the WithLens forms of the feature kernel), bit for bit; fisheye pixels
    outside the circle read as a miss"""
    p = ("fisheye", 150.0) if proj == "fisheye" else PROJECTIONS[proj]
    d = pl.box(67, 45, proj=p, room=True, ggx=ggx)
    guide, albedo = pl.features(d)
    b = HipBackend(d, 4, 0.003, 0.75, 1234)
    b.render_features()
    got_a, got_n, got_z = b.feature("albedo"), b.feature("normal"), b.feature("depth")
    b.close()
    assert np.array_equal(got_a.view(np.uint32), albedo[:, :, :3].view(np.uint32))
    assert np.array_equal(got_n.view(np.uint32), guide[:, :, :3].view(np.uint32))
    assert np.array_equal(got_z.view(np.uint32), guide[:, :, 3].view(np.uint32))
    miss = guide[:, :, 3] == 0
    if proj == "fisheye":   # the circle of radius 67 / 2 around (33.5, 22.5): the corners lie outside, the rest sees the box
        yy, xx = np.mgrid[0:45, 0:67]
        outside = np.hypot(xx + 0.5 - 33.5, yy + 0.5 - 22.5) > 33.5
        assert outside.sum() > 20 and np.array_equal(miss, outside)
        assert np.all(got_a[outside] == 1.0)
    else:
        assert not miss.any()   # the camera is inside a closed box


@pytest.mark.parametrize("proj", sorted(PROJECTIONS))
@pytest.mark.parametrize("algo", [4, 3])
def test_track_parts_still_sums_to_the_framebuffer(algo, proj):
    """a projection context with the technique breakdown on: the framebuffer is an untracked twin's bit for bit, and the
    planes add up to it within the documented bound (DESIGN.md "Technique breakdown": 2 m 2^-24 of the sum for m addends)"""
    from smallvcm_amd._abi import PART_COUNT
    d = pl.box(20, 14, proj=PROJECTIONS[proj], room=True)
    K = 3
    plain = HipBackend(d, algo, 0.05, 0.75, 1234)
    b = HipBackend(d, algo, 0.05, 0.75, 1234)
    try:
        b.track_parts()
        splats = 0
        for it in range(K):
            b.run_iteration(it, 0, 10)
            plain.run_iteration(it, 0, 10)
            splats += b.stats()["lightSplats"]
        fb = b.framebuffer_sum()
        assert np.array_equal(fb.view(np.uint32), plain.framebuffer_sum().view(np.uint32)) and fb.any()
        planes = np.stack([b.part(i, 1.0) for i in range(PART_COUNT)])
        m = splats + K * 4 * (1 + 10 * 12)
        S = planes.astype(np.float64).sum(axis=0)
        assert (np.abs(S - fb) <= 2.0 * m * 2.0 ** -24 * fb).all()
    finally:
        b.close()
        plain.close()


@pytest.mark.parametrize("line,flag", [("projection fisheye 200\n", []), ("projection panorama\n", []), ("", ["--projection", "panorama"]),
                                       ("projection panorama\n", ["--projection", "fisheye", "200"])])
def test_vcm_render_scene_file_with_projection_equals_python(tmp_path, line, flag):
    """the `projection` line of a scene file, and --projection overriding it, against the Python path"""
    from smallvcm_amd.scene_file import load_scene
    (tmp_path / "room.obj").write_text(
        "mtllib room.mtl\nv -1 -1 0\nv 1 -1 0\nv 1 1 0\nv -1 1 0\nv -0.3 -0.3 0\nv 0.3 -0.3 0\nv 0 0.2 0.6\n"
        "usemtl glossy\nf 1 2 3 4\nusemtl red\nf 5 6 7\n")
    (tmp_path / "room.mtl").write_text("newmtl glossy\nKd 0.3 0.3 0.3\nKs 0.6 0.5 0.4\nNs 30\nnewmtl red\nKd 0.7 0.2 0.2\nKs 0.2 0.2 0.2\nNs 40\n")
    head = "obj room.obj\ncamera 0 -1.5 1  0 1 -0.45  0 0 1  50\nlight background 1.5\nlight point 0 0 2  3 3 3\nfilter tent 1.5\n"
    (tmp_path / "s.vcmscene").write_text(head + line)
    res, iters, seed = (24, 18), 3, 4321
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "smallvcm_amd", "host", "vcm_render")
    out = tmp_path / "out.pfm"
    p = subprocess.run([exe, "-a", "vcm", "-i", str(iters), "--res", str(res[0]), str(res[1]), "--seed", str(seed),
                        "-o", str(out), "--scene-file", str(tmp_path / "s.vcmscene")] + flag, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    data = out.read_bytes()
    cli = np.frombuffer(data[len(b"PF\n%d %d\n-1\n" % res):], np.float32).reshape(res[1], res[0], 3)
    if flag:   # what the flag asks for, as a directive
        (tmp_path / "s.vcmscene").write_text(head + "projection " + " ".join(flag[1:]) + "\n")
    d = load_scene(tmp_path / "s.vcmscene", *res)
    assert isinstance(d, SceneDesc9)
    r = VertexCM(d, 4, 0.003, 0.75, seed)
    r.mMaxPathLength = 10
    for it in range(iters):
        r.RunIteration(it)
    want = r.GetFramebuffer()
    assert _debug_projection(r.backend)[0] == 1
    r.close()
    assert np.count_nonzero(want) > 0
    assert np.array_equal(cli.view(np.uint32), want.view(np.uint32))
    if not line and flag:   # with --gpus the projection is refused, like the other scene extensions
        q = subprocess.run([exe, "-a", "vcm", "-i", "1", "--res", "8", "8", "--gpus", "1"] + flag, capture_output=True, text=True, timeout=300)
        assert q.returncode != 0 and "--gpus" in q.stderr
