"""The thin-lens camera on the GPU: the WithLens kernels against the host emulation of the same device functions
(tests/host_emul_lens), bit for bit -- framebuffer, random-number tapes and workload counters -- for every algorithm,
scene kind and execution order; lens plus env map; the lens one call at a time (VCM_KAT_LENS); a closed lens against
vcm_create3; two shards against one context; and vcm_render's scene-file path against the Python one."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import envmap_lib as el
import lens_lib as ll
from smallvcm_amd._abi import SceneDesc3
from smallvcm_amd.renderer import HipBackend, VertexCM

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPLAT_ALGOS = (0, 3, 4)
STAT_KEYS = ("lightVertices", "lightRays", "cameraRays", "shadowRays", "mergeQueries", "mergeCandidates",
             "mergeAccepted", "connections", "lightSplats")
R, F = 0.6, 3.2
_fp = C.POINTER(C.c_float)


def _compare(d, algo, strict, seed=77, iters=2):
    emu = ll.Emul4(d, algo, seed=seed)
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
    r.close()
    assert np.count_nonzero(host) > 0
    if strict and algo in SPLAT_ALGOS:   # strict mode splats with fp32 atomics: their order is not defined
        assert np.all(np.abs(gpu - host) <= 2e-5 * np.abs(host) + 2e-7), float(np.abs(gpu - host).max())
    else:
        assert np.array_equal(gpu.view(np.uint32), host.view(np.uint32))


@pytest.mark.parametrize("strict", [False, True])
@pytest.mark.parametrize("kind", ["rects", "list", "bvh"])
@pytest.mark.parametrize("algo", range(7))
def test_gpu_equals_host_emulation(monkeypatch, algo, kind, strict):
    """scene 3's box takes WithLens<SceneRects>; with general pow forced, WithLens<SceneList>; with a BVH forced,
    WithLens<SceneBvh>"""
    if kind == "bvh":
        monkeypatch.setenv("SMALLVCM_AMD_FORCE_BVH", "1")   # read when the scene is built: both sides
    if kind == "list":
        monkeypatch.setenv("SMALLVCM_AMD_GENERAL_POW", "1")
    _compare(ll.builtin_lens(R, F, resx=20, resy=14), algo, strict)


@pytest.mark.parametrize("strict", [False, True])
@pytest.mark.parametrize("algo", [5, 3, 4])
def test_gpu_lens_with_envmap(algo, strict):
    sky = el.sky(48, 24, sun=(0.55, 0.2), sun_size=2, sun_value=(30.0, 27.0, 22.0))
    _compare(ll.with_lens(el.builtin_with_envmap(sky, scale=1.3, resx=20, resy=14), R, F), algo, strict)


def test_device_lens_equals_the_host():
    d = ll.builtin_lens(R, F, resx=64, resy=48)
    n = 50000
    rng = np.random.default_rng(8)
    raster = rng.random((n, 2)) * [64, 48]
    world = np.array(d.camera.position[:]) + rng.normal(size=(n, 3)) * 3.0
    inp = ll.lens_records(raster, rng.random((n, 2)), world)
    b = HipBackend(d, 4, 0.003, 0.75, 1234)
    b.L.vcm_debug_kat.argtypes = [C.c_void_p, C.c_int, C.c_int, _fp, _fp]
    dev = np.zeros_like(inp)
    assert b.L.vcm_debug_kat(b.ctx, ll.OP_LENS, n, inp.ctypes.data_as(_fp), dev.ctypes.data_as(_fp)) == 0, \
        b.L.vcm_last_error()
    b.close()
    host = ll.kat4(d, ll.OP_LENS, inp)
    assert 0.2 * n < np.count_nonzero(host[:, 9]) < n
    assert np.array_equal(dev.view(np.uint32), host.view(np.uint32))
    # a context without a lens refuses the op
    b = HipBackend(ll.builtin3(resx=8, resy=8), 4, 0.003, 0.75, 1)
    assert b.L.vcm_debug_kat(b.ctx, ll.OP_LENS, 1, inp.ctypes.data_as(_fp), dev.ctypes.data_as(_fp)) != 0
    b.close()


@pytest.mark.parametrize("algo", range(7))
def test_closed_lens_equals_create3(algo):
    d3 = ll.builtin3(resx=20, resy=14)
    out = []
    for d in (d3, ll.with_lens(d3, 0.0, 2.0), ll.with_lens(d3, None, None)):
        r = VertexCM(d, algo, 0.003, 0.75, 31)
        r.mMaxPathLength = 10
        for it in range(2):
            r.RunIteration(it)
        out.append(r.framebuffer_sum())
        r.close()
    assert isinstance(d3, SceneDesc3) and np.count_nonzero(out[0]) > 0
    for fb in out[1:]:
        assert np.array_equal(fb.view(np.uint32), out[0].view(np.uint32))


@pytest.mark.parametrize("algo", [5, 0, 3, 4])
def test_two_thread_rank_shards_equal_one_context(algo):
    """vcm_create_sharded4, world 2: two rank threads on one device exchanging light records (ShardedVertexCM over the
    thread collectives of test_gpu_dropin_sharded) against one context -- the path tracer bit for bit, the splatting
    algorithms within rounding of the summation order"""
    import threading
    from smallvcm_amd.renderer import ShardedVertexCM
    from test_gpu_dropin_sharded import _ThreadCollectives
    d = ll.builtin_lens(R, F, resx=20, resy=14)
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
        "mtllib room.mtl\nv -1 -1 0\nv 1 -1 0\nv 1 1 0\nv -1 1 0\nv -0.3 -0.3 0\nv 0.3 -0.3 0\nv 0 0.2 0.6\n"
        "usemtl white\nf 1 2 3 4\nusemtl red\nf 5 6 7\n")
    (tmp_path / "room.mtl").write_text("newmtl white\nKd 0.8 0.8 0.8\nnewmtl red\nKd 0.7 0.2 0.2\nKs 0.2 0.2 0.2\nNs 40\n")
    (tmp_path / "s.vcmscene").write_text("obj room.obj\ncamera 0 -4 2  0 1 -0.45  0 0 1  50\nlight background 1.5\n"
                                         "light point 0 0 2  3 3 3\nlens 0.3 4.2\n")
    res, iters, seed = (24, 18), 2, 4321
    exe = os.path.join(ROOT, "smallvcm_amd", "host", "vcm_render")

    def cli(*extra):
        out = tmp_path / "out.pfm"
        p = subprocess.run([exe, "--scene-file", str(tmp_path / "s.vcmscene"), "-a", "vcm", "-i", str(iters), "--res",
                            str(res[0]), str(res[1]), "--seed", str(seed), "-o", str(out)] + list(extra),
                           capture_output=True, text=True, timeout=300)
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
    assert np.array_equal(cli().view(np.uint32), want.view(np.uint32))
    # the flags override the file's lens
    other = py(ll.with_lens(d.base, 0.1, 3.0))
    assert np.array_equal(cli("--aperture", "0.1", "--focus", "3.0").view(np.uint32), other.view(np.uint32))
    p = subprocess.run([exe, "--scene-file", str(tmp_path / "s.vcmscene"), "--aperture", "0.1"], capture_output=True,
                       text=True, timeout=60)
    assert p.returncode == 2 and "--focus" in p.stderr
