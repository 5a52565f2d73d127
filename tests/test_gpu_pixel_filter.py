"""The pixel filter on the GPU: the WithLens kernels, which a filtered scene launches, against the host emulation of the
same device functions (tests/host_emul_filter), bit for bit -- framebuffer, random-number tapes and workload counters --
for every algorithm, scene kind, execution order and two image sizes; filter plus lens and filter plus env map; the filter
one call at a time (VCM_KAT_FILTER); a box filter against vcm_create5; two shards against one context; the tracked
images of a filtered context; the farm; and vcm_render's flag and scene-file path against the Python one."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import envmap_lib as el
import filter_lib as fl
import lens_lib as ll
import pick_lib as pl
from smallvcm_amd._abi import PART_COUNT
from smallvcm_amd.renderer import HipBackend, VertexCM

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPLAT_ALGOS = (0, 3, 4)
STAT_KEYS = ("lightVertices", "lightRays", "cameraRays", "shadowRays", "mergeQueries", "mergeCandidates",
             "mergeAccepted", "connections", "lightSplats")
_fp = C.POINTER(C.c_float)


def _set_kind(kind, monkeypatch):
    if kind == "bvh":
        monkeypatch.setenv("SMALLVCM_AMD_FORCE_BVH", "1")   # read when the scene is built: both sides
    if kind == "list":
        monkeypatch.setenv("SMALLVCM_AMD_GENERAL_POW", "1")


def _compare(d, algo, strict, seed=77, iters=2):
    emu = fl.Emul6(d, algo, seed=seed)
    r = VertexCM(d, algo, 0.003, 0.75, seed, strict_order=strict)
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
    kind, radius = C.c_int(-1), C.c_float(-1)
    r.backend.L.vcm_debug_pixel_filter.argtypes = [C.c_void_p, C.POINTER(C.c_int), _fp]
    assert r.backend.L.vcm_debug_pixel_filter(r.backend.ctx, C.byref(kind), C.byref(radius)) == 0
    r.close()
    assert (kind.value, radius.value) == fl.filter_params(d)
    assert np.count_nonzero(host) > 0
    if strict and algo in SPLAT_ALGOS:   # strict mode splats with fp32 atomics: their order is not defined (as test_gpu_thin_lens.py)
        assert np.all(np.abs(gpu - host) <= 2e-5 * np.abs(host) + 2e-7), float(np.abs(gpu - host).max())
    else:
        assert np.array_equal(gpu.view(np.uint32), host.view(np.uint32))
    return se


@pytest.mark.parametrize("res", [(20, 14), (67, 45)])
@pytest.mark.parametrize("strict", [False, True])
@pytest.mark.parametrize("kind", ["rects", "list", "bvh"])
@pytest.mark.parametrize("algo", range(7))
def test_gpu_equals_host_emulation(monkeypatch, algo, kind, strict, res):
    """tent r = 1.5.  Scene 3's box takes WithLens<SceneRects>; with general pow forced, WithLens<SceneList>; with a BVH
    forced, WithLens<SceneBvh>.  20 x 14: a partial workgroup; 67 x 45: no multiple of the wave or the workgroup"""
    _set_kind(kind, monkeypatch)
    _compare(fl.builtin_filter(fl.TENT, 1.5, resx=res[0], resy=res[1]), algo, strict)


@pytest.mark.parametrize("strict", [False, True])
@pytest.mark.parametrize("algo,kind", [(0, "rects"), (3, "bvh"), (4, "rects"), (4, "list"), (5, "rects"), (6, "bvh"), (2, "rects")])
def test_gpu_widest_bspline(monkeypatch, algo, kind, strict):
    """B-spline r = 16, the largest support, wider than the 14 rows of the image: camera rays leave the image rectangle
    and most splats near the border are rejected, fewer than without a filter but not none"""
    _set_kind(kind, monkeypatch)
    st = _compare(fl.builtin_filter(fl.BSPLINE, 16.0, resx=20, resy=14), algo, strict)
    if algo in SPLAT_ALGOS:
        _, ref, _ = fl.render(fl.builtin_filter(None, resx=20, resy=14), algo, 2, seed=77)
        assert 0 < st["lightSplats"] < ref["lightSplats"]


@pytest.mark.parametrize("strict", [False, True])
@pytest.mark.parametrize("algo", [5, 3, 4])
def test_gpu_filter_with_lens_and_with_envmap(algo, strict):
    _compare(fl.with_filter(ll.builtin_lens(0.6, 3.2, resx=20, resy=14), fl.TENT, 1.5), algo, strict)
    sky = el.sky(48, 24, sun=(0.55, 0.2), sun_size=2, sun_value=(30.0, 27.0, 22.0))
    _compare(fl.with_filter(el.builtin_with_envmap(sky, scale=1.3, resx=20, resy=14), fl.BSPLINE, 2.0), algo, strict)


def test_device_filter_equals_the_host():
    n = 50000
    rng = np.random.default_rng(8)
    raster = rng.random((n, 2)) * [70, 54] - 3.0   # some projections outside the 64 x 48 image
    inp = fl.filter_records(raster, fl.uniforms(rng, n))
    for kind, radius in ((fl.TENT, 1.5), (fl.BSPLINE, 2.0), (fl.BSPLINE, 16.0)):
        d = fl.builtin_filter(kind, radius, resx=64, resy=48)
        b = HipBackend(d, 4, 0.003, 0.75, 1234)
        b.L.vcm_debug_kat.argtypes = [C.c_void_p, C.c_int, C.c_int, _fp, _fp]
        dev = np.zeros_like(inp)
        assert b.L.vcm_debug_kat(b.ctx, fl.OP_FILTER, n, inp.ctypes.data_as(_fp), dev.ctypes.data_as(_fp)) == 0, \
            b.L.vcm_last_error()
        b.close()
        host = fl.kat6(d, fl.OP_FILTER, inp)
        assert np.count_nonzero(host[:, 2] >= 0) > 0.05 * n and np.count_nonzero(host[:, 2] < 0) > 0
        assert np.array_equal(dev.view(np.uint32), host.view(np.uint32))
    # a context without a filter refuses the op
    b = HipBackend(fl.builtin_filter(None, resx=8, resy=8), 4, 0.003, 0.75, 1)
    assert b.L.vcm_debug_kat(b.ctx, fl.OP_FILTER, 1, inp.ctypes.data_as(_fp), dev.ctypes.data_as(_fp)) != 0
    b.close()


@pytest.mark.parametrize("algo", range(7))
def test_box_filter_equals_create5(algo):
    d3 = ll.builtin3(resx=20, resy=14)
    out = []
    for d in (pl.with_pick(d3, None), fl.with_filter(d3, fl.BOX, 2.0), fl.with_filter(d3, None)):
        r = VertexCM(d, algo, 0.003, 0.75, 31)
        r.mMaxPathLength = 10
        for it in range(2):
            r.RunIteration(it)
        out.append(r.framebuffer_sum())
        r.close()
    assert np.count_nonzero(out[0]) > 0
    for fb in out[1:]:
        assert np.array_equal(fb.view(np.uint32), out[0].view(np.uint32))


@pytest.mark.parametrize("algo", [5, 0, 3, 4])
def test_two_thread_rank_shards_equal_one_context(algo):
    """vcm_create_sharded6, world 2: two rank threads on one device exchanging light records (ShardedVertexCM over the
    thread collectives of test_gpu_dropin_sharded) against one context -- the path tracer bit for bit, the splatting
    algorithms within rounding of the summation order"""
    import threading
    from smallvcm_amd.renderer import ShardedVertexCM
    from test_gpu_dropin_sharded import _ThreadCollectives
    d = fl.builtin_filter(fl.TENT, 1.5, resx=20, resy=14)
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


def test_tracked_contexts_still_work():
    """a filtered VCM context with the technique breakdown, the variance and the robust estimate on: the framebuffer is
    an untracked twin's bit for bit, the planes add up to it within the documented bound (DESIGN.md "Technique
    breakdown": 2 m 2^-24 of the sum for m addends), and the other two images come out"""
    d = fl.builtin_filter(fl.TENT, 1.5, resx=20, resy=14)
    K, buckets = 3, 3
    plain = HipBackend(d, 4, 0.05, 0.75, 1234)
    b = HipBackend(d, 4, 0.05, 0.75, 1234)
    try:
        b.track_parts()
        b.track_variance()
        b.track_robust(buckets)
        splats = 0
        for it in range(K):
            b.run_iteration(it, 0, 10)
            plain.run_iteration(it, 0, 10)
            splats += b.stats()["lightSplats"]
        fb = b.framebuffer_sum()
        assert np.array_equal(fb.view(np.uint32), plain.framebuffer_sum().view(np.uint32)) and fb.any()
        planes = np.stack([b.part(i, 1.0) for i in range(PART_COUNT)])
        assert all(planes[i].max() > 0 for i in range(PART_COUNT))
        m = splats + K * 4 * (1 + 10 * 12)
        S = planes.astype(np.float64).sum(axis=0)
        assert (np.abs(S - fb) <= 2.0 * m * 2.0 ** -24 * fb).all()
        var = b.variance()
        assert np.isfinite(var).all() and var.max() > 0
        st = b.noise_stats()
        assert st["iterations"] == K and st["mean"] > 0
        rob = b.robust()
        assert np.isfinite(rob).all() and rob.max() > 0 and b.robust_stats()["buckets"] == buckets
        emu_fb, _, _ = fl.render(d, 4, K, seed=1234, radius_factor=0.05)
        assert np.array_equal(fb.view(np.uint32), emu_fb.view(np.uint32))
    finally:
        b.close()
        plain.close()


def test_farm_passes_the_filter_on():
    """vcm_farm_render with a filter: two ranks sharing every iteration (thread collectives, one device) against one
    context over the same version-1 scene, within the rounding of the shards' summation order"""
    from smallvcm_amd import farm
    from smallvcm_amd.renderer import cornell_scene
    sc = cornell_scene(1, 20, 14)
    iters = 2
    r = farm.farm_render(sc, 4, iterations=iters, ranks=2, shards=2, inflight=1, devices=[0, 0], collectives="threads",
                         seed=11, pixel_filter=("tent", 1.5))
    box = farm.farm_render(sc, 4, iterations=iters, ranks=2, shards=2, inflight=1, devices=[0, 0], collectives="threads", seed=11)
    d = fl.with_filter(ll.builtin3(mask=ll.SCENE_CONFIGS[1], resx=20, resy=14), fl.TENT, 1.5)
    one = VertexCM(d, 4, 0.003, 0.75, 11)
    one.mMaxPathLength, one.mMinPathLength = 10, 0
    for it in range(iters):
        one.RunIteration(it)
    want = one.framebuffer_sum() / iters
    one.close()
    assert np.count_nonzero(want) > 0
    assert np.allclose(r["image"], want, rtol=2e-6, atol=2e-7)
    assert not np.allclose(box["image"], want, rtol=1e-3, atol=1e-5)
    # one rank: the same context behind the farm's loop; only the final scaling may round differently
    solo = farm.farm_render(sc, 4, iterations=iters, ranks=1, shards=1, inflight=1, devices=[0], collectives="threads", seed=11,
                            pixel_filter=("tent", 1.5))
    assert np.allclose(solo["image"], want, rtol=2.0 ** -22, atol=0)


def test_vcm_render_filter_equals_python(tmp_path):
    from smallvcm_amd.scene_file import load_scene
    (tmp_path / "room.obj").write_text(
        "mtllib room.mtl\nv -1 -1 0\nv 1 -1 0\nv 1 1 0\nv -1 1 0\nv -0.3 -0.3 0\nv 0.3 -0.3 0\nv 0 0.2 0.6\n"
        "usemtl white\nf 1 2 3 4\nusemtl red\nf 5 6 7\n")
    (tmp_path / "room.mtl").write_text("newmtl white\nKd 0.8 0.8 0.8\nnewmtl red\nKd 0.7 0.2 0.2\nKs 0.2 0.2 0.2\nNs 40\n")
    (tmp_path / "s.vcmscene").write_text("obj room.obj\ncamera 0 -4 2  0 1 -0.45  0 0 1  50\nlight background 1.5\n"
                                         "light point 0 0 2  3 3 3\nfilter bspline 2\n")
    res, iters, seed = (24, 18), 2, 4321
    exe = os.path.join(ROOT, "smallvcm_amd", "host", "vcm_render")

    def cli(*args):
        out = tmp_path / "out.pfm"
        p = subprocess.run([exe, "-a", "vcm", "-i", str(iters), "--res", str(res[0]), str(res[1]), "--seed", str(seed),
                            "-o", str(out)] + list(args), capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stderr
        data = out.read_bytes()
        return np.frombuffer(data[len(b"PF\n%d %d\n-1\n" % res):], np.float32).reshape(res[1], res[0], 3)

    def py(scene):
        r = VertexCM(scene, 4, 0.003, 0.75, seed)
        r.mMaxPathLength = 10
        for it in range(iters):
            r.RunIteration(it)
        img = r.GetFramebuffer()
        r.close()
        return img

    d = load_scene(tmp_path / "s.vcmscene", *res)
    want = py(d)
    assert np.count_nonzero(want) > 0
    assert np.array_equal(cli("--scene-file", str(tmp_path / "s.vcmscene")).view(np.uint32), want.view(np.uint32))
    # the flag overrides the file's filter
    other = py(fl.with_filter(d.base, fl.TENT, 1.5))
    assert not np.array_equal(other, want)
    assert np.array_equal(cli("--scene-file", str(tmp_path / "s.vcmscene"), "--filter", "tent", "1.5").view(np.uint32),
                          other.view(np.uint32))
    # a built-in scene
    builtin = py(fl.builtin_filter(fl.TENT, 1.5, mask=ll.SCENE_CONFIGS[1], resx=res[0], resy=res[1]))
    assert np.array_equal(cli("-s", "1", "--filter", "tent", "1.5").view(np.uint32), builtin.view(np.uint32))
    for bad in (["--filter", "gauss", "1"], ["--filter", "tent", "x"], ["--filter", "tent", "0"], ["--filter", "bspline", "17"]):
        p = subprocess.run([exe, "-s", "1", "--res", "8", "8"] + bad, capture_output=True, text=True, timeout=60)
        assert p.returncode == 2 and "filter" in p.stderr, (bad, p.stderr)
