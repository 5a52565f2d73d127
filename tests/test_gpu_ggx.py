"""The GGX lobe on the GPU: the WithGgx kernels, which a scene with a lobe launches, against the host emulation of the
same device functions (tests/host_emul_ggx), bit for bit -- framebuffer, random-number tapes and workload counters --
for every algorithm, scene kind, execution order and two image sizes; the lobe beside lens, filters, env map, spot and
sphere lights, a pick table and the Sobol sampler; more materials than the LDS table holds; the two known-answer ops;
the default unchanged; two shards against one context, under both exchanges; the tracked images; the feature kernel's albedo; vcm_render on a
scene file with a `Pr` material."""
import ctypes as C
import os
import subprocess
import threading

import numpy as np
import pytest

import envmap_lib as el
import ggx_lib as gl
from smallvcm_amd._abi import with_material_ext
from smallvcm_amd.renderer import HipBackend, VertexCM

pytestmark = pytest.mark.gpu

SPLAT_ALGOS = (0, 3, 4)
STAT_KEYS = ("lightVertices", "lightRays", "cameraRays", "shadowRays", "mergeQueries", "mergeCandidates",
             "mergeAccepted", "connections", "lightSplats")
_fp = C.POINTER(C.c_float)


def _set_kind(kind, monkeypatch):
    if kind == "bvh":
        monkeypatch.setenv("SMALLVCM_AMD_FORCE_BVH", "1")   # read when the scene is built: both sides
    if kind == "list":
        monkeypatch.setenv("SMALLVCM_AMD_GENERAL_POW", "1")


def _debug_ggx(backend):
    n = C.c_int(-1)
    backend.L.vcm_debug_ggx.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
    return backend.L.vcm_debug_ggx(backend.ctx, C.byref(n)), n.value


def _compare(d, algo, strict, seed=77, iters=2, lobes=2, merge=None, rf=0.003):
    """merge: "walk" / "pairs" -- the K4 kernel asked for, and checked to be the one that ran"""
    emu = gl.Emul8(d, algo, seed=seed, radius_factor=rf)
    r = VertexCM(d, algo, rf, 0.75, seed, strict_order=strict)
    r.mMinPathLength, r.mMaxPathLength = 0, 10
    if merge is not None:
        r.backend.set_merge_kernel(merge)
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
    assert _debug_ggx(r.backend) == (1, lobes)
    if merge is not None:
        import capacity_lib as cl
        assert cl.context_info(r.backend)["mergeKernel"] == HipBackend.MERGE_KERNELS[merge]
        assert emu.stats()["mergeAccepted"] > 100   # the lobe is evaluated: the floor and the back wall hold most photons
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
    """The room is a list of axis-aligned rectangles and two spheres: WithGgx over SceneRects; with general pow forced,
    over SceneList; with a BVH forced, over SceneBvh.  20 x 14: a partial workgroup; 67 x 45: no multiple of the wave or
    the workgroup"""
    _set_kind(kind, monkeypatch)
    _compare(gl.room(res[0], res[1]), algo, strict)


@pytest.mark.parametrize("merge", ["walk", "pairs"])
@pytest.mark.parametrize("res", [(20, 14), (67, 45)])
@pytest.mark.parametrize("kind", ["rects", "list", "bvh"])
@pytest.mark.parametrize("algo", [1, 2, 4])
def test_both_merge_kernels_equal_the_host_emulation(monkeypatch, algo, kind, res, merge):
    """the three merging algorithms with k_merge_walk<IP, true> and with k_merge_pairs<IP, true> (the default), integer
    and general Phong exponents (rects / list), the kernel that ran read back; then beside Sobol, lights and a lens"""
    _set_kind(kind, monkeypatch)
    _compare(gl.room(res[0], res[1]), algo, False, merge=merge, iters=3, rf=0.05)   # (a wide radius: hundreds of merges even at 20 x 14)
    if kind == "rects" and res == (20, 14):
        _compare(gl.room(sampler="sobol", lights=True, pick=("power", 0.25), lens=(0.05, 3.2)), algo, False, merge=merge, rf=0.05)


@pytest.mark.parametrize("strict", [False, True])
@pytest.mark.parametrize("algo", [5, 3, 4, 2])
def test_gpu_ggx_beside_every_other_widening(algo, strict):
    _compare(gl.room(lens=(0.05, 3.2), flt=("tent", 1.5)), algo, strict)
    sky = el.sky(48, 24, sun=(0.55, 0.2), sun_size=2, sun_value=(30.0, 27.0, 22.0))
    _compare(gl.room(sky=sky, flt=("bspline", 2.0)), algo, strict)
    _compare(gl.room(lights=True, pick=("power", 0.25)), algo, strict)
    _compare(gl.room(sampler="sobol"), algo, strict)
    _compare(gl.room(sampler="sobol", lights=True, pick=("power", 0.25), lens=(0.05, 3.2)), algo, strict)


@pytest.mark.parametrize("strict", [False, True])
@pytest.mark.parametrize("algo", [4, 5])
def test_gpu_forty_materials(algo, strict):
    """more materials than VCM_LDS_MATERIALS: both tables are read from global memory"""
    d = gl.room(n_materials=40)
    assert int(gl.desc2_of(d).nMaterials) == 41   # (and the emitter's)
    _compare(d, algo, strict, lobes=2 + 33)


def _device_kat(backend, op, inp):
    backend.L.vcm_debug_kat.argtypes = [C.c_void_p, C.c_int, C.c_int, _fp, _fp]
    inp = np.ascontiguousarray(inp, np.float32)
    dev = np.zeros_like(inp)
    assert backend.L.vcm_debug_kat(backend.ctx, op, len(inp), inp.ctypes.data_as(_fp), dev.ctypes.data_as(_fp)) == 0, \
        backend.L.vcm_last_error()
    return dev


def test_device_ops_equal_the_host():
    """VCM_KAT_BSDF_EVAL and VCM_KAT_BSDF_SAMPLE on the 50 000 records of test_ggx.py, bit for bit"""
    d = gl.kat_scene()
    ev, sa = gl.random_records()
    b = HipBackend(d, 4, 0.003, 0.75, 1234)
    for op, rec in ((gl.OP_BSDF_EVAL, ev), (gl.OP_BSDF_SAMPLE, sa)):
        host = gl.kat8(d, op, rec)
        dev = _device_kat(b, op, rec)
        assert np.count_nonzero(host[:, 3]) > 0.3 * len(host)
        assert np.array_equal(dev.view(np.uint32), host.view(np.uint32)), op
    b.close()


@pytest.mark.parametrize("algo", range(7))
def test_default_is_unchanged(algo):
    """vcm_create8 with materialExt NULL and with every ggx zero = vcm_create7, bit for bit, on the kernels of version 7
    (vcm_debug_ggx); a lobe changes the image"""
    d7 = gl.as_desc7(gl.room(phong=True))
    n = int(gl.desc2_of(d7).nMaterials)
    lobe = [(0, 0, 0, 0.0)] * n
    lobe[0] = (0.9, 0.75, 0.5, 0.15)
    out = []
    for d, want in ((d7, (0, 0)), (with_material_ext(d7, None), (0, 0)), (with_material_ext(d7, [(0, 0, 0, 0.5)] * n), (0, 0)),
                    (with_material_ext(d7, lobe), (1, 1))):
        r = VertexCM(d, algo, 0.003, 0.75, 31)
        r.mMaxPathLength = 10
        for it in range(2):
            r.RunIteration(it)
        assert _debug_ggx(r.backend) == want
        out.append((r.framebuffer_sum(), r.backend.rng_counts()))
        r.close()
    assert np.count_nonzero(out[0][0]) > 0
    for fb, (lc, cc) in out[1:3]:
        assert np.array_equal(fb.view(np.uint32), out[0][0].view(np.uint32))
        assert np.array_equal(lc, out[0][1][0]) and np.array_equal(cc, out[0][1][1])
    if algo != 6:   # (eye light shades by the normal alone)
        assert not np.array_equal(out[3][0], out[0][0])


def _two_rank_frames(d, algo, iters=3):
    """the frames of two rank threads on one device exchanging light records (vcm_create_sharded8, world 2)"""
    from smallvcm_amd.renderer import ShardedVertexCM
    from test_gpu_dropin_sharded import _ThreadCollectives
    world = 2
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
    return results


def _check_shards_against_one_context(d, algo, results, iters=3):
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


@pytest.mark.parametrize("algo", [5, 0, 4, 2])
def test_two_thread_rank_shards_equal_one_context(algo):
    """vcm_create_sharded8, world 2: two rank threads on one device exchanging light records against one context -- the
    path tracer bit for bit, the others within rounding of the summation order"""
    d = gl.room()
    _check_shards_against_one_context(d, algo, _two_rank_frames(d, algo))


@pytest.mark.parametrize("algo", [4, 2])
def test_two_thread_rank_shards_unsorted_exchange(monkeypatch, algo):
    """the same with SMALLVCM_AMD_SORTED_EXCHANGE=0 (read in vcm_create*: set before the contexts are made):
    k_compact_records<WithGgx<DScene>> writes the records and k_cell_rank_gather reads them.  What the sorted run
    asserts, and both ranks' frames equal to the sorted run's bit for bit: both exchanges build the same grid
    (test_gpu_dropin_sharded.py test_sorted_and_unsorted_exchange_render_the_same_bits, there without a lobe)"""
    d = gl.room()
    sorted_frames = _two_rank_frames(d, algo)
    monkeypatch.setenv("SMALLVCM_AMD_SORTED_EXCHANGE", "0")
    frames = _two_rank_frames(d, algo)
    _check_shards_against_one_context(d, algo, frames)
    for fb, want in zip(frames, sorted_frames):
        assert np.array_equal(fb.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("algo", [4, 3])
def test_track_parts_still_sums_to_the_framebuffer(algo):
    """a GGX context with the technique breakdown on: the framebuffer is an untracked twin's bit for bit, and the planes
    add up to it within the documented bound (DESIGN.md "Technique breakdown": 2 m 2^-24 of the sum for m addends)"""
    from smallvcm_amd._abi import PART_COUNT
    d = gl.room()
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


def test_feature_albedo_equals_the_emulation():
    """vcm_render_features in a GGX context: albedo = clamp(diffuse + phong + mirror + F0), normal and depth, bit for bit;
    the lobe shows in the albedo of the floor"""
    d = gl.room(67, 45)
    guide, albedo = gl.features(d)
    b = HipBackend(d, 4, 0.003, 0.75, 1234)
    b.render_features()
    got_a, got_n, got_z = b.feature("albedo"), b.feature("normal"), b.feature("depth")
    b.close()
    assert np.array_equal(got_a.view(np.uint32), albedo[:, :, :3].view(np.uint32))
    assert np.array_equal(got_n.view(np.uint32), guide[:, :, :3].view(np.uint32))
    assert np.array_equal(got_z.view(np.uint32), guide[:, :, 3].view(np.uint32))
    floor = np.all(np.isclose(albedo[:, :, :3], np.array([0.9, 0.75, 0.5], np.float32)), axis=2)   # kd = 0: F0 alone
    assert floor.sum() > 200


def test_vcm_render_scene_file_with_pr_equals_python(tmp_path):
    from smallvcm_amd._abi import SceneDesc8
    from smallvcm_amd.scene_file import load_scene
    (tmp_path / "room.obj").write_text(
        "mtllib room.mtl\nv -1 -1 0\nv 1 -1 0\nv 1 1 0\nv -1 1 0\nv -0.3 -0.3 0\nv 0.3 -0.3 0\nv 0 0.2 0.6\n"
        "usemtl glossy\nf 1 2 3 4\nusemtl red\nf 5 6 7\n")
    (tmp_path / "room.mtl").write_text("newmtl glossy\nKd 0.3 0.3 0.3\nKs 0.6 0.5 0.4\nPr 0.4\nnewmtl red\nKd 0.7 0.2 0.2\nKs 0.2 0.2 0.2\nNs 40\n")
    (tmp_path / "s.vcmscene").write_text("obj room.obj\ncamera 0 -4 2  0 1 -0.45  0 0 1  50\nlight background 1.5\n"
                                         "light point 0 0 2  3 3 3\nfilter tent 1.5\n")
    res, iters, seed = (24, 18), 3, 4321
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "smallvcm_amd", "host", "vcm_render")
    out = tmp_path / "out.pfm"
    p = subprocess.run([exe, "-a", "vcm", "-i", str(iters), "--res", str(res[0]), str(res[1]), "--seed", str(seed),
                        "-o", str(out), "--scene-file", str(tmp_path / "s.vcmscene")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    data = out.read_bytes()
    cli = np.frombuffer(data[len(b"PF\n%d %d\n-1\n" % res):], np.float32).reshape(res[1], res[0], 3)
    d = load_scene(tmp_path / "s.vcmscene", *res)
    assert isinstance(d, SceneDesc8)
    r = VertexCM(d, 4, 0.003, 0.75, seed)
    r.mMaxPathLength = 10
    for it in range(iters):
        r.RunIteration(it)
    want = r.GetFramebuffer()
    assert _debug_ggx(r.backend) == (1, 1)
    r.close()
    assert np.count_nonzero(want) > 0
    assert np.array_equal(cli.view(np.uint32), want.view(np.uint32))
