"""Light selection on the GPU: the WithPick kernels against the host emulation of the same device functions
(tests/host_emul_pick), bit for bit -- framebuffer, random-number tapes and workload counters -- for every algorithm,
scene kind and execution order, POWER and CUSTOM, with the light table in LDS (<= 4 lights) and in global memory, with
the pick table in LDS and beyond its room; pick plus lens plus env map; the pick one call at a time
(VCM_KAT_LIGHT_PICK); UNIFORM against vcm_create4; two shards against one context; and vcm_render's scene-file path
against the Python one."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import envmap_lib as el
import lens_lib as ll
import pick_lib as pl
from smallvcm_amd.renderer import HipBackend, VertexCM

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPLAT_ALGOS = (0, 3, 4)
STAT_KEYS = ("lightVertices", "lightRays", "cameraRays", "shadowRays", "mergeQueries", "mergeCandidates",
             "mergeAccepted", "connections", "lightSplats")
_fp = C.POINTER(C.c_float)


def _compare(d, algo, strict, seed=77, iters=2):
    emu = pl.Emul5(d, algo, seed=seed)
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


def _few():
    """scene 3 with three more lights: 4 lights, the light table in LDS"""
    return pl.box_many_lights(3)


def _many():
    """scene 3 with six more lights: 7 lights, the light table in global memory"""
    return pl.box_many_lights(6)


@pytest.mark.parametrize("strict", [False, True])
@pytest.mark.parametrize("kind", ["rects", "list", "bvh"])
@pytest.mark.parametrize("algo", range(7))
def test_gpu_equals_host_emulation(monkeypatch, algo, kind, strict):
    """scene 3's box takes WithPick<SceneRects>; with general pow forced, WithPick<SceneList>; with a BVH forced,
    WithPick<SceneBvh>"""
    if kind == "bvh":
        monkeypatch.setenv("SMALLVCM_AMD_FORCE_BVH", "1")   # read when the scene is built: both sides
    if kind == "list":
        monkeypatch.setenv("SMALLVCM_AMD_GENERAL_POW", "1")
    few, many = _few(), _many()
    assert pl.n_lights(few) == 4 and pl.n_lights(many) == 7
    _compare(pl.with_pick(few, pl.POWER, 0.25), algo, strict)
    _compare(pl.with_pick(few, pl.CUSTOM, 0.0, [1.0, 5.0, 0.5, 2.0]), algo, strict)
    _compare(pl.with_pick(many, pl.POWER), algo, strict)
    _compare(pl.with_pick(many, pl.CUSTOM, 0.1, [3.0, 1.0, 0.25, 8.0, 1.0, 2.0, 0.5]), algo, strict)


@pytest.mark.parametrize("strict", [False, True])
@pytest.mark.parametrize("bvh", [False, True])
@pytest.mark.parametrize("algo", range(7))
def test_gpu_emissive_mesh_equals_host_emulation(monkeypatch, algo, bvh, strict):
    """the case the feature is for: area emitters (a lamp quad, six dim emissive triangles) and a point light, so camera
    paths HIT lights of very different pmf (get_light_radiance and the path tracer's Mis2 with light_pick_prob of the
    hit light's index), as a list and behind a BVH"""
    if bvh:
        monkeypatch.setenv("SMALLVCM_AMD_FORCE_BVH", "1")
    room = pl.lamp_room(resx=20, resy=14, n_dim=6)
    n = pl.n_lights(room)
    assert n == 9
    _compare(pl.with_pick(room, pl.POWER, 0.05), algo, strict)
    _compare(pl.with_pick(room, pl.CUSTOM, 0.0, [5.0, 1.0] + [0.5] * (n - 3) + [2.0]), algo, strict)


@pytest.mark.parametrize("strict", [False, True])
@pytest.mark.parametrize("algo", [5, 3, 4])
def test_gpu_pick_table_beyond_lds(algo, strict):
    """300 lights: more than the LDS room of the pick table (VCM_LDS_PICK = 256), the guided search in global memory"""
    d = pl.box_many_lights(299)
    assert pl.n_lights(d) == 300
    _compare(pl.with_pick(d, pl.POWER, 0.05), algo, strict)


@pytest.mark.parametrize("strict", [False, True])
@pytest.mark.parametrize("algo", [5, 3, 4])
def test_gpu_pick_with_lens_and_envmap(algo, strict):
    sky = el.sky(48, 24, sun=(0.55, 0.2), sun_size=2, sun_value=(30.0, 27.0, 22.0))
    d3 = pl.add_point_lights(el.builtin_with_envmap(sky, scale=1.3, resx=20, resy=14),
                             [((0.3, 0.2, 0.5), (1.0, 0.8, 0.6)), ((-0.4, 0.1, 0.2), (0.1, 0.2, 0.3))])
    _compare(pl.with_pick(ll.with_lens(d3, 0.6, 3.2), pl.POWER, 0.2), algo, strict)


@pytest.mark.parametrize("n", [7, 300])
def test_device_pick_equals_the_host(n):
    """the boundaries of every interval, the generator's extremes and random floats, on the device"""
    rng = np.random.default_rng(n)
    w32 = (10.0 ** rng.uniform(0, 9, n)).astype(np.float32)
    w32[1] = 0.0
    d = pl.with_pick(pl.point_light_scene(w32), pl.CUSTOM, 0.0, w32)
    mode, w, m, pmf, cdf = pl.tables(d)
    live = np.nonzero(m > 0)[0]
    first = (cdf[live].astype(np.float64) + 2.0 ** -24).astype(np.float32)
    last = (cdf[live + 1].astype(np.float64) - 2.0 ** -24).astype(np.float32)
    j = rng.integers(0, pl.Q, 20000)
    rnd = ((2 * j + 1) * 2.0 ** -24).astype(np.float32)
    r = np.concatenate([first, last, np.float32([2.0 ** -24, 1.0 - 2.0 ** -24]), rnd])
    light = np.concatenate([live, live, [live[0], live[-1]], rng.integers(0, n, len(rnd))])
    inp = pl.pick_records(r, light)
    b = HipBackend(d, 4, 0.003, 0.75, 1234)
    b.L.vcm_debug_kat.argtypes = [C.c_void_p, C.c_int, C.c_int, _fp, _fp]
    dev = np.zeros_like(inp)
    assert b.L.vcm_debug_kat(b.ctx, pl.OP_LIGHT_PICK, len(inp), inp.ctypes.data_as(_fp), dev.ctypes.data_as(_fp)) == 0, \
        b.L.vcm_last_error()
    b.close()
    k = len(live)
    assert np.array_equal(dev[:k, 0], live.astype(np.float32)) and np.array_equal(dev[k:2 * k, 0], live.astype(np.float32))
    assert np.array_equal(dev[:k, 1], pmf[live]) and np.array_equal(dev[:2 * k + 2, 2], pmf[light[:2 * k + 2]])
    assert (dev[2 * k, 0], dev[2 * k + 1, 0]) == (live[0], live[-1])
    host = pl.kat5(d, pl.OP_LIGHT_PICK, inp)
    assert np.array_equal(dev.view(np.uint32), host.view(np.uint32))


@pytest.mark.parametrize("algo", range(7))
def test_uniform_equals_create4(algo):
    d4 = pl.as_desc4(_many())
    out = []
    for d in (d4, pl.with_pick(d4, None), pl.with_pick(d4, pl.UNIFORM, 0.4)):
        r = VertexCM(d, algo, 0.003, 0.75, 31)
        r.mMaxPathLength = 10
        for it in range(2):
            r.RunIteration(it)
        out.append((r.framebuffer_sum(), r.backend.rng_counts(), r.stats()))
        r.close()
    assert np.count_nonzero(out[0][0]) > 0
    for fb, counts, stats in out[1:]:
        assert np.array_equal(fb.view(np.uint32), out[0][0].view(np.uint32))
        assert all(np.array_equal(a, b) for a, b in zip(counts, out[0][1]))
        assert all(stats[k] == out[0][2][k] for k in STAT_KEYS)


@pytest.mark.parametrize("algo", [5, 0, 3, 4])
def test_two_thread_rank_shards_equal_one_context(algo):
    """vcm_create_sharded5, world 2: two rank threads on one device exchanging light records against one context -- the
    path tracer bit for bit, the splatting algorithms within rounding of the summation order"""
    import threading
    from smallvcm_amd.renderer import ShardedVertexCM
    from test_gpu_dropin_sharded import _ThreadCollectives
    d = pl.with_pick(_many(), pl.POWER, 0.1)
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
        "v -0.2 -0.2 1.5\nv 0.2 -0.2 1.5\nv 0 0.2 1.5\n"
        "usemtl white\nf 1 2 3 4\nusemtl red\nf 5 6 7\nusemtl lamp\nf 8 10 9\n")
    (tmp_path / "room.mtl").write_text("newmtl white\nKd 0.8 0.8 0.8\nnewmtl red\nKd 0.7 0.2 0.2\nKs 0.2 0.2 0.2\nNs 40\n"
                                       "newmtl lamp\nKe 20 18 15\n")
    (tmp_path / "s.vcmscene").write_text("obj room.obj\ncamera 0 -4 2  0 1 -0.45  0 0 1  50\nlight background 0.2\n"
                                         "light point 0 0 2  0.3 0.3 0.3\nlightpick power 0.1\n")
    res, iters, seed = (24, 18), 2, 4321
    exe = os.path.join(ROOT, "smallvcm_amd", "host", "vcm_render")

    def cli(*extra):
        out = tmp_path / "out.pfm"
        p = subprocess.run([exe, "--scene-file", str(tmp_path / "s.vcmscene"), "-a", "vcm", "-i", str(iters), "--res",
                            str(res[0]), str(res[1]), "--seed", str(seed), "-o", str(out)] + list(extra),
                           capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stderr
        data = out.read_bytes()
        return np.frombuffer(data[len(b"PF\n%d %d\n-1\n" % res):], np.float32).reshape(res[1], res[0], 3), p.stdout

    def py(scene):
        r = VertexCM(scene, 4, 0.003, 0.75, seed)
        r.mMaxPathLength = 10
        for it in range(iters):
            r.RunIteration(it)
        img = r.GetFramebuffer()
        r.close()
        return img

    d = load_scene(tmp_path / "s.vcmscene", *res)
    assert pl.n_lights(d) == 3 and d.pick.contents.mode == pl.POWER
    want = py(d)
    assert np.count_nonzero(want) > 0
    img, text = cli("--light-pick-report")
    assert np.array_equal(img.view(np.uint32), want.view(np.uint32))
    assert "light pick: power" in text and "pmf" in text
    # the flags override the file's directive
    uniform = py(d.base)
    img, text = cli("--light-pick", "uniform")
    assert np.array_equal(img.view(np.uint32), uniform.view(np.uint32))
    assert not np.array_equal(uniform, want)
    other = py(pl.with_pick(d.base, pl.POWER, 0.5))
    assert np.array_equal(cli("--light-pick", "power", "--light-pick-mix", "0.5")[0].view(np.uint32), other.view(np.uint32))
    p = subprocess.run([exe, "--scene-file", str(tmp_path / "s.vcmscene"), "--light-pick", "brightest"], capture_output=True,
                       text=True, timeout=60)
    assert p.returncode == 2 and "--light-pick" in p.stderr
