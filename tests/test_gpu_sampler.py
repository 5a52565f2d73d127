"""The Sobol sampler on the GPU: the WithSobol kernels, which a scene with `sampler sobol` launches, against the host
emulation of the same device functions (tests/host_emul_sampler), bit for bit -- framebuffer, random-number tapes and
workload counters -- for every algorithm, scene kind, execution order and two image sizes, five iterations each so that the
sample index crosses a 2^2 block; the sampler beside lens, filter, env map, spot and sphere lights and a pick table; the
sampler one call at a time (VCM_KAT_SAMPLER) and the net property on the device's answers; the default unchanged; two
shards against one context; the tracked images; vcm_render's flag and scene-file path; the farm; and the error against
a converged reference, held to half the measured gain (DESIGN.md "Sampler")."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import envmap_lib as el
import filter_lib as fl
import lens_lib as ll
import lights_lib as lil
import sampler_lib as sl
from smallvcm_amd._abi import PART_COUNT
from smallvcm_amd.renderer import HipBackend, VertexCM

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
SPLAT_ALGOS = (0, 3, 4)
STAT_KEYS = ("lightVertices", "lightRays", "cameraRays", "shadowRays", "mergeQueries", "mergeCandidates",
             "mergeAccepted", "connections", "lightSplats")
_fp = C.POINTER(C.c_float)


def _set_kind(kind, monkeypatch):
    if kind == "bvh":
        monkeypatch.setenv("SMALLVCM_AMD_FORCE_BVH", "1")   # read when the scene is built: both sides
    if kind == "list":
        monkeypatch.setenv("SMALLVCM_AMD_GENERAL_POW", "1")


def _debug_sampler(backend):
    k = C.c_int(-1)
    backend.L.vcm_debug_sampler.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
    assert backend.L.vcm_debug_sampler(backend.ctx, C.byref(k)) == 0
    return k.value


def _compare(d, algo, strict, seed=77, iters=5):
    emu = sl.Emul7(d, algo, seed=seed)
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
    assert _debug_sampler(r.backend) == sl.sampler_params(d) == sl.SOBOL
    r.close()
    assert np.count_nonzero(host) > 0
    if strict and algo in SPLAT_ALGOS:   # strict mode splats with fp32 atomics: their order is not defined (as test_gpu_pixel_filter.py)
        assert np.all(np.abs(gpu - host) <= 2e-5 * np.abs(host) + 2e-7), float(np.abs(gpu - host).max())
    else:
        assert np.array_equal(gpu.view(np.uint32), host.view(np.uint32))


@pytest.mark.parametrize("res", [(20, 14), (67, 45)])
@pytest.mark.parametrize("strict", [False, True])
@pytest.mark.parametrize("kind", ["rects", "list", "bvh"])
@pytest.mark.parametrize("algo", range(7))
def test_gpu_equals_host_emulation(monkeypatch, algo, kind, strict, res):
    """Scene 3's box takes the WithSobol kind over SceneRects; with general pow forced, over SceneList; with a BVH forced,
    over SceneBvh.  20 x 14: a partial workgroup; 67 x 45: no multiple of the wave or the workgroup"""
    _set_kind(kind, monkeypatch)
    _compare(sl.builtin_sampler(sl.SOBOL, resx=res[0], resy=res[1]), algo, strict)


@pytest.mark.parametrize("strict", [False, True])
@pytest.mark.parametrize("algo", [5, 3, 4])
def test_gpu_sobol_beside_every_other_widening(algo, strict):
    _compare(sl.with_kind(fl.with_filter(ll.builtin_lens(0.6, 3.2, resx=20, resy=14), fl.TENT, 1.5), sl.SOBOL), algo, strict, iters=3)
    sky = el.sky(48, 24, sun=(0.55, 0.2), sun_size=2, sun_value=(30.0, 27.0, 22.0))
    _compare(sl.with_kind(fl.with_filter(el.builtin_with_envmap(sky, scale=1.3, resx=20, resy=14), fl.BSPLINE, 2.0), sl.SOBOL),
             algo, strict, iters=3)
    _compare(sl.with_kind(lil.room(pick="power", mix=0.25), sl.SOBOL), algo, strict, iters=3)


@pytest.fixture(scope="module")
def records():
    s, i, p, kind, k = sl.random_records()
    return sl.sampler_records(s, i, p, kind, k)


def _device_kat(backend, inp):
    backend.L.vcm_debug_kat.argtypes = [C.c_void_p, C.c_int, C.c_int, _fp, _fp]
    inp = np.ascontiguousarray(inp, np.float32)
    dev = np.zeros_like(inp)
    assert backend.L.vcm_debug_kat(backend.ctx, sl.OP_SAMPLER, len(inp), inp.ctypes.data_as(_fp), dev.ctypes.data_as(_fp)) == 0, \
        backend.L.vcm_last_error()
    return dev


def test_device_sampler_equals_the_host(records):
    """... in a Sobol context and in one without: the op names the sampler's function, not the context's mode"""
    host = sl.kat7(sl.builtin_sampler(None, resx=8, resy=8), sl.OP_SAMPLER, records)
    assert np.count_nonzero(host[:, 1].view(np.uint32)) > 0.99 * len(host)
    for kind in (sl.SOBOL, None):
        b = HipBackend(sl.builtin_sampler(kind, resx=8, resy=8), 4, 0.003, 0.75, 1234)
        dev = _device_kat(b, records)
        b.close()
        assert np.array_equal(dev.view(np.uint32), host.view(np.uint32))


def test_device_points_are_nets():
    """64 random (seed, path, kind, j), every m = 0..10, the prefix and one random aligned block: one launch, then every
    elementary interval holds one point -- on the 23 bits of the device's floats"""
    rng = np.random.default_rng(11)
    cases, cols = [], [[] for _ in range(5)]
    for _ in range(64):
        seed, path = int(rng.integers(0, 1 << 32)), int(rng.integers(0, 1 << 22))
        kind, j = int(rng.integers(0, 6)), int(rng.integers(0, 64))
        for m in range(11):
            for a in (0, int(rng.integers(1, 1 << (32 - m)))):
                i = (np.arange(1 << m, dtype=np.uint64) + np.uint64(a << m)).astype(np.uint32)
                for c in (0, 1):
                    for col, v in zip(cols, (seed, i, path, kind, 2 * j + c)):
                        col.append(np.broadcast_to(np.uint32(v), i.shape))
                cases.append(m)
    inp = sl.sampler_records(*[np.concatenate(c) for c in cols])
    b = HipBackend(sl.builtin_sampler(sl.SOBOL, resx=8, resy=8), 4, 0.003, 0.75, 1234)
    dev = _device_kat(b, inp)
    b.close()
    w, pos = sl.float_bits23(dev[:, 0]), 0
    for m in cases:
        n = 1 << m
        assert sl.is_net(w[pos:pos + n], w[pos + n:pos + 2 * n], m), (m, pos)
        pos += 2 * n
    assert pos == len(w)


@pytest.mark.parametrize("algo", range(7))
def test_default_is_unchanged(algo):
    """vcm_create7 with sampler NULL and with PHILOX = vcm_create6, bit for bit; vcm_debug_sampler reports what was asked"""
    d6 = sl.as_desc6(ll.builtin3(resx=20, resy=14))
    out = []
    for d, want in ((d6, sl.PHILOX), (sl.with_kind(d6, None), sl.PHILOX), (sl.with_kind(d6, sl.PHILOX), sl.PHILOX),
                    (sl.with_kind(d6, sl.SOBOL), sl.SOBOL)):
        r = VertexCM(d, algo, 0.003, 0.75, 31)
        r.mMaxPathLength = 10
        for it in range(2):
            r.RunIteration(it)
        assert _debug_sampler(r.backend) == want
        out.append((r.framebuffer_sum(), r.backend.rng_counts()))
        r.close()
    assert np.count_nonzero(out[0][0]) > 0
    for fb, (lc, cc) in out[1:3]:
        assert np.array_equal(fb.view(np.uint32), out[0][0].view(np.uint32))
        assert np.array_equal(lc, out[0][1][0]) and np.array_equal(cc, out[0][1][1])
    assert not np.array_equal(out[3][0], out[0][0])


@pytest.mark.parametrize("algo", [5, 0, 3, 4])
def test_two_thread_rank_shards_equal_one_context(algo):
    """vcm_create_sharded7, world 2: two rank threads on one device exchanging light records (ShardedVertexCM over the
    thread collectives of test_gpu_dropin_sharded) against one context -- the path tracer bit for bit, the splatting
    algorithms within rounding of the summation order"""
    import threading
    from smallvcm_amd.renderer import ShardedVertexCM
    from test_gpu_dropin_sharded import _ThreadCollectives
    d = sl.builtin_sampler(sl.SOBOL, resx=20, resy=14)
    world, iters = 2, 5
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
    """a Sobol VCM context with the technique breakdown, the variance and the robust estimate on: the framebuffer is an
    untracked twin's bit for bit, the planes add up to it within the documented bound (DESIGN.md "Technique breakdown":
    2 m 2^-24 of the sum for m addends), and the other two images come out finite"""
    d = sl.builtin_sampler(sl.SOBOL, resx=20, resy=14)
    K, buckets = 5, 3
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
        m = splats + K * 4 * (1 + 10 * 12)
        S = planes.astype(np.float64).sum(axis=0)
        assert (np.abs(S - fb) <= 2.0 * m * 2.0 ** -24 * fb).all()
        var = b.variance()
        assert np.isfinite(var).all() and var.max() > 0
        assert b.noise_stats()["iterations"] == K
        rob = b.robust()
        assert np.isfinite(rob).all() and rob.max() > 0 and b.robust_stats()["buckets"] == buckets
    finally:
        b.close()
        plain.close()


def test_farm_passes_the_sampler_on():
    from smallvcm_amd import farm
    from smallvcm_amd.renderer import cornell_scene
    sc = cornell_scene(1, 20, 14)
    iters = 4
    r = farm.farm_render(sc, 4, iterations=iters, ranks=2, shards=2, inflight=1, devices=[0, 0], collectives="threads",
                         seed=11, sampler="sobol")
    white = farm.farm_render(sc, 4, iterations=iters, ranks=2, shards=2, inflight=1, devices=[0, 0], collectives="threads", seed=11)
    assert r["sampler"] == "sobol" and white["sampler"] == "philox"
    d = sl.builtin_sampler(sl.SOBOL, mask=ll.SCENE_CONFIGS[1], resx=20, resy=14)
    one = VertexCM(d, 4, 0.003, 0.75, 11)
    one.mMaxPathLength, one.mMinPathLength = 10, 0
    for it in range(iters):
        one.RunIteration(it)
    want = one.framebuffer_sum() / iters
    one.close()
    assert np.count_nonzero(want) > 0
    assert np.allclose(r["image"], want, rtol=2e-6, atol=2e-7)
    assert not np.allclose(white["image"], want, rtol=1e-3, atol=1e-5)
    with pytest.raises(ValueError, match="sampler"):
        farm.farm_render(sc, 4, iterations=1, ranks=1, shards=1, inflight=1, devices=[0], collectives="threads", sampler="halton")


def test_vcm_render_sampler_equals_python(tmp_path):
    from smallvcm_amd.scene_file import load_scene
    (tmp_path / "room.obj").write_text(
        "mtllib room.mtl\nv -1 -1 0\nv 1 -1 0\nv 1 1 0\nv -1 1 0\nv -0.3 -0.3 0\nv 0.3 -0.3 0\nv 0 0.2 0.6\n"
        "usemtl white\nf 1 2 3 4\nusemtl red\nf 5 6 7\n")
    (tmp_path / "room.mtl").write_text("newmtl white\nKd 0.8 0.8 0.8\nnewmtl red\nKd 0.7 0.2 0.2\nKs 0.2 0.2 0.2\nNs 40\n")
    (tmp_path / "s.vcmscene").write_text("obj room.obj\ncamera 0 -4 2  0 1 -0.45  0 0 1  50\nlight background 1.5\n"
                                         "light point 0 0 2  3 3 3\nsampler sobol\n")
    res, iters, seed = (24, 18), 5, 4321
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
    # the flag overrides the file's sampler
    other = py(sl.with_kind(d, sl.PHILOX))
    assert not np.array_equal(other, want)
    assert np.array_equal(cli("--scene-file", str(tmp_path / "s.vcmscene"), "--sampler", "philox").view(np.uint32),
                          other.view(np.uint32))
    # a built-in scene
    builtin = py(sl.builtin_sampler(sl.SOBOL, mask=ll.SCENE_CONFIGS[1], resx=res[0], resy=res[1]))
    assert np.array_equal(cli("-s", "1", "--sampler", "sobol").view(np.uint32), builtin.view(np.uint32))
    p = subprocess.run([exe, "-s", "1", "--res", "8", "8", "--sampler", "halton"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 2 and "sampler" in p.stderr, p.stderr


# (case, algorithm, R, P) at 64 iterations as measured (DESIGN.md "Sampler", profiles/r38_sampler_measure.txt): the
# bound t = sqrt(R max(1, P)) is half the measured gain on a log scale, and both cases pass the gate R < 1 / max(1, P)^2
CONVERGENCE = (("s3_pt", 5, 0.457, 1.000), ("s3_vcm", 4, 0.576, 1.012))


@pytest.mark.parametrize("name,algo,R,P", CONVERGENCE)
def test_sobol_converges_faster(name, algo, R, P):
    """Scene 3 at 64 x 64, 64 iterations, mean over two seeds no measurement used: MSE(Sobol) <= t MSE(Philox) against
    the committed reference of 2^14 Philox iterations (seed 90210; written by
    `python tests/sampler_measure.py --make-refs tests/golden`).  A sampler that degenerates to white noise gives a ratio
    near 1 and fails."""
    import sampler_measure as sm
    assert R < 1.0 / max(1.0, P) ** 2
    t = float(np.sqrt(R * max(1.0, P)))
    assert t < 1.0
    ref = np.load(sm.ref_path(GOLDEN, name)).astype(np.float64)
    mse = {}
    for kind in (sl.PHILOX, sl.SOBOL):
        mse[kind] = np.mean([np.mean((sm.render(3, algo, kind, seed, (64,))[0] - ref) ** 2) for seed in (21, 22)])
    print("%s: MSE philox %.5e, sobol %.5e, ratio %.3f, bound %.3f" % (name, mse[sl.PHILOX], mse[sl.SOBOL],
                                                                         mse[sl.SOBOL] / mse[sl.PHILOX], t))
    assert mse[sl.SOBOL] <= t * mse[sl.PHILOX]
