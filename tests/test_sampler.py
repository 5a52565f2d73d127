"""The Owen-scrambled Sobol sampler on the host (no GPU): the known-answer op against a numpy restatement written from
the definition, the net property it is built for, the independence of its scramble seeds from the sample index, the
unchanged default (sampler NULL / PHILOX = version 6, bit for bit), where the draw groups of a path start, and the
`sampler` directive of a scene file in both bindings."""
import numpy as np
import pytest

import sampler_lib as sl
from smallvcm_amd._abi import SceneDesc6, SceneDesc7

ALGOS = range(7)


@pytest.fixture(scope="module")
def records():
    s, i, p, kind, k = sl.random_records()
    return (s, i, p, kind, k), sl.sampler_records(s, i, p, kind, k)


@pytest.fixture(scope="module")
def host_answers(records):
    return sl.kat7(sl.builtin_sampler(None, resx=8, resy=8), sl.OP_SAMPLER, records[1])


def test_host_kat_equals_the_numpy_restatement(records, host_answers):
    (s, i, p, kind, k), _ = records
    assert i.max() == 0xffffffff and k.max() == 127 and set(kind) == set(range(6)) and len(s) == 50000
    want = sl.sobol_words(s, i, p, kind, k)
    got = host_answers[:, 1].copy().view(np.uint32)
    assert np.array_equal(got, want)
    assert np.array_equal(host_answers[:, 0].view(np.uint32), sl.word_to_float(want).view(np.uint32))
    assert not host_answers[:, 2:].any()


def test_second_dimension_is_the_pascal_matrix():
    """brev(T(x)) against Sobol dimension 1 by its bit loop (direction numbers v_b = v_{b-1} ^ (v_{b-1} >> 1))"""
    idx = np.random.default_rng(1).integers(0, 1 << 32, 2000, dtype=np.uint64)
    want = np.zeros_like(idx)
    v = np.uint64(1 << 31)
    for b in range(32):
        want ^= np.where((idx >> np.uint64(b)) & np.uint64(1), v, np.uint64(0))
        v ^= v >> np.uint64(1)
    assert np.array_equal(sl.brev(sl.t_map(idx)), want)


def _net_violations(words_of):
    """64 random (seed, path, kind, j), every m = 0..10, the prefix and one random aligned block"""
    rng = np.random.default_rng(11)
    bad = []
    for _ in range(64):
        seed, path = int(rng.integers(0, 1 << 32)), int(rng.integers(0, 1 << 22))
        kind, j = int(rng.integers(0, 6)), int(rng.integers(0, 64))
        for m in range(11):
            for a in (0, int(rng.integers(1, 1 << (32 - m)))):
                i = (np.arange(1 << m, dtype=np.uint64) + np.uint64(a << m)).astype(np.uint32)
                w0, w1 = words_of(seed, i, path, kind, 2 * j), words_of(seed, i, path, kind, 2 * j + 1)
                if not sl.is_net(w0, w1, m):
                    bad.append((seed, path, kind, j, m, a))
    return bad


def test_net_property_of_the_restatement():
    full = lambda v, i: np.full(len(i), v, np.uint32)   # noqa: E731
    assert not _net_violations(lambda s, i, p, kd, k: sl.sobol_words(full(s, i), i, full(p, i), full(kd, i), full(k, i)))


def test_net_property_of_the_host_floats():
    """the same on what the host function returns, read off the FLOATS (the 23 bits they keep)"""
    sc = sl.builtin_sampler(None, resx=8, resy=8)

    def words(s, i, p, kd, k):
        n = len(i)
        out = sl.kat7(sc, sl.OP_SAMPLER, sl.sampler_records(np.full(n, s, np.uint32), i, np.full(n, p, np.uint32),
                                                            np.full(n, kd, np.uint32), np.full(n, k, np.uint32)))
        return sl.float_bits23(out[:, 0])
    assert not _net_violations(words)


def test_a_white_noise_stream_is_no_net():
    """the check has teeth: Philox words in the sampler's place fail it"""
    rng = np.random.default_rng(3)
    w = rng.integers(0, 1 << 32, (2, 256), dtype=np.uint64).astype(np.uint32)
    assert not sl.is_net(w[0], w[1], 8)


def test_scramble_seeds_are_per_stream_and_pair_not_per_index():
    E = sl.emul_sampler()
    import ctypes as C
    out = (C.c_uint32 * 3)()
    # the library's seeds are the restatement's, and the restatement's take no index at all
    for seed, path, kind, j in ((7, 5, 0, 0), (0xffffffff, 4095, 5, 47), (123456789, 77, 3, 9)):
        E.emul_sampler_seeds(seed, path, kind, j, out)
        assert tuple(out) == tuple(int(x) for x in sl.scramble_seeds(seed, path, kind, j))
    # (scramble_seeds has no index argument, and test_host_kat_equals_the_numpy_restatement holds the library's floats to
    # the words those seeds give for every index.)  With the seeds fixed, indices i and i ^ 1 are the two points of a
    # (0, 1, 2)-net in every component: their words differ in the top bit
    i = np.arange(0, 8192, 2, dtype=np.uint32)
    c = lambda v: np.full(len(i), v, np.uint32)   # noqa: E731
    for k in (0, 1, 6, 7):
        a, b = sl.sobol_words(c(9), i, c(3), c(1), c(k)), sl.sobol_words(c(9), i ^ np.uint32(1), c(3), c(1), c(k))
        assert np.all((a ^ b) >> 31 == 1)
    # distinct (path, kind, j) give distinct seed triples over a 64 x 64 frame, 6 kinds, 48 pairs
    path, kind, j = np.meshgrid(np.arange(64 * 64), np.arange(6), np.arange(48), indexing="ij")
    s0, s1, s2 = sl.scramble_seeds(1234, path.ravel(), kind.ravel(), j.ravel())
    trip = np.stack([s0, s1, s2], axis=1).astype(np.uint32)
    assert len(np.unique(trip, axis=0)) == len(trip)


def test_every_float_is_an_odd_multiple_of_2_to_the_minus_24(host_answers):
    f = host_answers[:, 0].astype(np.float64) * 2.0 ** 24
    assert np.all(f == np.round(f)) and np.all(f.astype(np.int64) % 2 == 1)
    assert host_answers[:, 0].min() > 0 and host_answers[:, 0].max() < 1


def _run(e, iters=2):
    for it in range(iters):
        e.run_iteration(it, 0, 10)
    return e.framebuffer(), e.counts(), e.stats()


@pytest.mark.parametrize("algo", ALGOS)
def test_default_is_unchanged(algo):
    """emul_create7 with sampler NULL and with PHILOX = emul_create6: framebuffer, both tapes, counters"""
    d6 = sl.as_desc6(sl.ll.builtin3(mask=sl.ll.SCENE_CONFIGS[1], resx=20, resy=14))
    want = _run(sl.Emul7(d6, algo, seed=31, version6=True))
    assert np.count_nonzero(want[0]) > 0
    for kind in (None, sl.PHILOX):
        d7 = sl.with_kind(d6, kind)
        assert sl.sampler_params(d7) == sl.PHILOX
        got = _run(sl.Emul7(d7, algo, seed=31))
        assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32))
        assert np.array_equal(got[1][0], want[1][0]) and np.array_equal(got[1][1], want[1][1])
        assert got[2] == want[2]
    sob = _run(sl.Emul7(sl.with_kind(d6, sl.SOBOL), algo, seed=31))
    assert not np.array_equal(sob[0], want[0])


def test_draw_groups_start_on_pair_boundaries():
    """scene 1, VCM, 20 x 14: under Sobol a light path has drawn at least 6 floats where Philox has drawn 5, every direct-
    illumination group starts on an odd position and every scattering group on an even one; under Philox nothing moves"""
    base = sl.ll.builtin3(mask=sl.ll.SCENE_CONFIGS[1], resx=20, resy=14)
    out = {}
    for kind in (sl.PHILOX, sl.SOBOL):
        e = sl.Emul7(sl.with_kind(base, kind), 4, seed=5)
        tr = sl.trace(lambda: [e.run_iteration(it, 0, 10) for it in range(5)])
        out[kind] = (tr, e.counts())
    tr, (lc, cc) = out[sl.SOBOL]
    ptr, (plc, pcc) = out[sl.PHILOX]
    assert plc.min() == 5 and lc.min() >= 6
    g, kd, k0 = tr[:, 0], tr[:, 1], tr[:, 2]
    assert np.count_nonzero(g == sl.GROUP_DI) > 1000 and np.count_nonzero(g == sl.GROUP_SCATTER) > 1000
    assert np.all(k0[g == sl.GROUP_LIGHT] == 1) and np.all(kd[g == sl.GROUP_LIGHT] == 0)
    assert np.all(k0[g == sl.GROUP_DI] % 2 == 1) and np.all(kd[g == sl.GROUP_DI] == 1)
    assert np.all(k0[g == sl.GROUP_SCATTER] % 2 == 0)
    assert np.all(k0[(g == sl.GROUP_SCATTER) & (kd == 0)] >= 6)
    pg, pk0 = ptr[:, 0], ptr[:, 2]
    assert np.all(pk0[pg == sl.GROUP_LIGHT] == 0)
    assert np.any(pk0[pg == sl.GROUP_DI] % 2 == 0) and np.any(pk0[pg == sl.GROUP_SCATTER] % 2 == 1)
    assert cc.max() <= 2 + 8 * 10 and cc.max() > pcc.min()


def _quad(tmp_path):
    (tmp_path / "quad.obj").write_text("mtllib quad.mtl\nv -1 -1 0\nv 1 -1 0\nv 1 1 0\nv -1 1 0\nusemtl white\nf 1 2 3 4\n")
    (tmp_path / "quad.mtl").write_text("newmtl white\nKd 0.8 0.8 0.8\n")


def test_scene_file_sampler_directive(tmp_path):
    from smallvcm_amd.scene_file import load_scene
    _quad(tmp_path)
    (tmp_path / "s.vcmscene").write_text("obj quad.obj\ncamera 0 -4 2  0 1 -0.4  0 0 1  50\nlight background 1\n"
                                         "sampler sobol   # the Owen-scrambled sequence\n")
    d = load_scene(tmp_path / "s.vcmscene", 16, 12)
    assert isinstance(d, SceneDesc7) and d.sampler and d.sampler.contents.kind == sl.SOBOL
    assert not d.base.filter and not d.base.base.pick and d.camera.resolution[0] == 16
    assert sl.sampler_params(d) == sl.SOBOL   # what the C++ scene host makes of the same description
    (tmp_path / "p.vcmscene").write_text("obj quad.obj\nlight background 1\nfilter tent 1.5\nsampler philox\n")
    d = load_scene(tmp_path / "p.vcmscene", 8, 8)
    assert isinstance(d, SceneDesc7) and d.sampler.contents.kind == sl.PHILOX and d.base.filter
    (tmp_path / "plain.vcmscene").write_text("obj quad.obj\nlight background 1\nfilter tent 1.5\n")
    plain = load_scene(tmp_path / "plain.vcmscene", 8, 8)
    assert isinstance(plain, SceneDesc6) and not isinstance(plain, SceneDesc7)
    for bad in ("sampler", "sampler halton", "sampler sobol 2", "sampler sobol\nsampler sobol"):
        (tmp_path / "bad.vcmscene").write_text("obj quad.obj\nlight background 1\n" + bad + "\n")
        with pytest.raises(ValueError, match=r"bad\.vcmscene.*sampler"):
            load_scene(tmp_path / "bad.vcmscene", 8, 8)


def test_builder_and_bad_kinds():
    from smallvcm_amd.scene2 import SceneBuilder
    b = SceneBuilder()
    m = b.material(diffuse=(0.7, 0.7, 0.7))
    b.triangle((-1, -1, 0), (1, -1, 0), (1, 1, 0), m)
    b.point_light((0, 0, 2), (3, 3, 3))
    cam = ((0, -4, 2), (0, 1, -0.4), (0, 0, 1), 50, 8, 8)
    assert not isinstance(b.build(*cam), SceneDesc7)
    b.sampler("sobol")
    d = b.build(*cam)
    assert isinstance(d, SceneDesc7) and sl.sampler_params(d) == sl.SOBOL
    with pytest.raises(ValueError, match="sampler"):
        b.sampler("halton")
    import ctypes as C
    from smallvcm_amd._abi import Sampler
    bad = sl.with_kind(d, None)
    s = Sampler(7)
    bad.sampler = C.pointer(s)
    E = sl.emul_sampler()
    k = C.c_int()
    assert E.emul_sampler_params(C.byref(bad), C.byref(k)) == -1 and b"sampler" in E.emul_sampler_error()
