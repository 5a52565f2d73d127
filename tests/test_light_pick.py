"""Light selection (vcm_scene_desc5) on the CPU: input checks, UNIFORM against the version-4 renderer, exactness of the
table, POWER's weights against the lights' Emit estimators, unbiasedness of every algorithm and the variance gained on a
many-light room (all on the host emulation, tests/host_emul_pick), the random tapes, sharding, and the scene-file /
SceneBuilder surface."""
import ctypes as C

import numpy as np
import pytest

import envmap_lib as el
import lens_lib as ll
import pick_lib as pl
from smallvcm_amd._abi import SceneDesc4, SceneDesc5
from smallvcm_amd.renderer import load_library
from test_thin_lens import _agree, _blocks

Q = pl.Q


@pytest.fixture(scope="module")
def E():
    return pl.emul_pick()   # builds tests/host_emul_pick


# ---------------------------------------------------------------- 1. input checks

def test_create5_rejects_bad_picks(E):
    """the library's checks run before it looks for a device; the emulation shares them (scene_host.h)"""
    L = load_library(require_gpu=False)
    L.vcm_create5.restype = C.c_void_p
    L.vcm_create5.argtypes = [C.POINTER(SceneDesc5), C.c_int, C.c_float, C.c_float, C.c_int]
    L.vcm_last_error.restype = C.c_char_p
    d3 = pl.box_many_lights(2)   # scene 3's background and two point lights: three lights, none of them black
    assert pl.n_lights(d3) == 3
    black = pl.point_light_scene([0, 0])   # two lights that emit nothing
    nan, inf = float("nan"), float("inf")
    # (scene, mode, uniformMix, weights, the words that tell this refusal from the others)
    bad = [(d3, 3, 0.0, None, "mode must be"), (d3, -1, 0.0, None, "mode must be"),
           (d3, pl.POWER, -0.1, None, "uniformMix must be"), (d3, pl.POWER, 1.5, None, "uniformMix must be"),
           (d3, pl.POWER, nan, None, "uniformMix must be"), (d3, pl.UNIFORM, inf, None, "uniformMix must be"),
           (d3, pl.CUSTOM, 0.0, None, "CUSTOM needs weights"),
           (d3, pl.CUSTOM, 0.0, [1.0, -1.0, 1.0], "weights must be finite and >= 0"),
           (d3, pl.CUSTOM, 0.0, [1.0, nan, 1.0], "weights must be finite and >= 0"),
           (d3, pl.CUSTOM, 0.0, [1.0, 1.0, inf], "weights must be finite and >= 0"),
           # one zero among valid weights: nothing but the non-black check can refuse it
           (d3, pl.CUSTOM, 0.0, [0.0, 1.0, 1.0], "zero weight on a light that is not black"),
           (d3, pl.CUSTOM, 0.5, [1.0, 1.0, 0.0], "zero weight on a light that is not black"),
           # only black lights: every zero is acceptable on its own, but the table has nothing to hold
           (black, pl.CUSTOM, 0.0, [0.0, 0.0], "all weights are zero"),
           (black, pl.POWER, 0.0, None, "all weights are zero")]
    for scene, mode, mix, w, words in bad:
        d = pl.with_pick(scene, mode, mix, w)
        assert not L.vcm_create5(C.byref(d), 4, 0.003, 0.75, 1), (mode, mix, w)
        assert words in L.vcm_last_error().decode(), (mode, mix, w, L.vcm_last_error().decode())
        assert not E.emul_create5(C.byref(d), 4, 0.003, 0.75, 1, 0, 1), (mode, mix, w)
        assert words in E.emul_pick_error().decode(), (mode, mix, w, E.emul_pick_error().decode())
    # the same weights are fine once the zero is gone
    assert pl.tables(pl.with_pick(d3, pl.CUSTOM, 0.5, [1.0, 1.0, 2.0]))[0] == pl.CUSTOM
    # a bad version-4 part is still refused
    d = pl.with_pick(ll.builtin_lens(-1.0, 3.0), pl.POWER)
    assert not E.emul_create5(C.byref(d), 4, 0.003, 0.75, 1, 0, 1)
    # a zero weight on a BLACK light is accepted, and that light is never picked
    d = pl.with_pick(pl.point_light_scene([1, 0, 2]), pl.CUSTOM, 0.0, [1.0, 0.0, 2.0])
    mode, w, m, pmf, cdf = pl.tables(d)
    assert mode == pl.CUSTOM and m[1] == 0 and m.sum() == Q
    # with POWER a black light gets pmf 0
    mode, w, m, pmf, cdf = pl.tables(pl.with_pick(pl.point_light_scene([1, 0, 2]), pl.POWER))
    assert list(m) == [Q // 2, 0, Q // 2]


# ---------------------------------------------------------------- 2. UNIFORM is the version-4 renderer

def _state(e):
    return e.framebuffer().view(np.uint32), e.counts(), e.stats()


def _same(a, b):
    (fa, ca, sa), (fb, cb, sb) = _state(a), _state(b)
    return np.array_equal(fa, fb) and all(np.array_equal(x, y) for x, y in zip(ca, cb)) and sa == sb


@pytest.mark.parametrize("scene", ["scene3", "mesh"])
@pytest.mark.parametrize("algo", range(7))
def test_uniform_equals_create4(algo, scene):
    """pick = NULL and mode = UNIFORM: the framebuffer, both tapes and the nine counters of the version-4 description"""
    d4 = pl.as_desc4(ll.builtin3(resx=20, resy=14)) if scene == "scene3" else pl.lamp_room(resx=16, resy=12, n_dim=6)
    assert scene == "scene3" or pl.n_lights(d4) > 4
    ref = ll.Emul4(d4, algo, seed=5)
    emus = [pl.Emul5(pl.with_pick(d4, None), algo, seed=5), pl.Emul5(pl.with_pick(d4, pl.UNIFORM, 0.3), algo, seed=5)]
    for it in range(2):
        ref.run_iteration(it)
        for e in emus:
            e.run_iteration(it)
    assert np.count_nonzero(ref.framebuffer()) > 0
    for e in emus:
        assert _same(e, ref)


# ---------------------------------------------------------------- 3. the table is exact

def _weights(n, rng, zeros, decades):
    w = 10.0 ** rng.uniform(0, decades, n)
    if zeros and n > 1:
        w[rng.random(n) < 0.3] = 0.0
        w[rng.integers(n)] = max(w.max(), 1.0)
    return w.astype(np.float32)


@pytest.mark.parametrize("n", [1, 2, 3, 7, 64, 1000])
def test_table_is_exact(n):
    rng = np.random.default_rng(100 + n)
    for zeros, decades, mix in [(False, 1, 0.0), (True, 3, 0.0), (False, 12, 0.0), (True, 12, 0.0), (False, 6, 0.25)]:
        w32 = _weights(n, rng, zeros, decades)
        d = pl.with_pick(pl.point_light_scene(w32), pl.CUSTOM, mix, w32)
        mode, w, m, pmf, cdf = pl.tables(d)
        assert mode == pl.CUSTOM and np.array_equal(w, w32.astype(np.float64))
        assert int(m.sum()) == Q
        assert np.all(m[w > 0] >= 1) and np.all(m[w == 0] == 0)
        assert cdf[0] == 0.0 and cdf[n] == 1.0
        assert np.array_equal(pmf, (cdf[1:].astype(np.float64) - cdf[:-1]).astype(np.float32))   # exact in binary32
        assert np.array_equal(pmf.astype(np.float64) * Q, m)
        nz = w > 0
        p = np.zeros(n)
        p[nz] = (1 - np.float64(np.float32(mix))) * w[nz] / w.sum() + np.float64(np.float32(mix)) / nz.sum()
        floored = nz & (p * Q < 1.0) & (m == 1)   # the floor of one quantum applied (or would have been met anyway)
        D = int(np.count_nonzero(nz & (np.floor(p * Q + 1e-9) == 0)))
        dev = pmf.astype(np.float64) - p
        # The issue's bound, |pmf - w / sum w| <= 2^-23 "except where the floor of one quantum applies": largest remainder
        # keeps every light within a quantum, and that is asserted as it stands when no light needed the floor (D == 0).
        # With D floored lights the issue's own rule hands each of them a quantum "taken from the largest", so a donor
        # may end up to D quanta further below its share, and nobody gains more than a quantum: that is all that is
        # allowed here, and the total deviation is bounded with it.
        assert np.all(dev[~floored] <= 2.0 ** -23) and np.all(dev[~floored] >= -(D + 1) * 2.0 ** -23)
        if D == 0:
            assert np.all(np.abs(dev) <= 2.0 ** -23)
        assert np.abs(dev).sum() <= (n + 2 * D) * 2.0 ** -23
        # VCM_KAT_LIGHT_PICK: the first and the last float of every non-empty interval, the generator's extremes
        live = np.nonzero(m > 0)[0]
        first = (cdf[live].astype(np.float64) + 2.0 ** -24).astype(np.float32)
        last = (cdf[live + 1].astype(np.float64) - 2.0 ** -24).astype(np.float32)
        assert np.array_equal(first.astype(np.float64), cdf[live].astype(np.float64) + 2.0 ** -24)
        for r in (first, last):
            out = pl.kat5(d, pl.OP_LIGHT_PICK, pl.pick_records(r, live))
            assert np.array_equal(out[:, 0], live.astype(np.float32))
            assert np.array_equal(out[:, 1], pmf[live]) and np.array_equal(out[:, 2], pmf[live])
        ends = pl.kat5(d, pl.OP_LIGHT_PICK, pl.pick_records([2.0 ** -24, 1.0 - 2.0 ** -24]))
        assert (ends[0, 0], ends[1, 0]) == (live[0], live[-1])


def test_exhaustive_count_returns_the_quanta():
    """all 2^23 floats the generator can produce, one n = 7 table with a zero and a weight that needs the floor"""
    w32 = np.array([3.0, 1e-9, 0.0, 7.5, 0.25, 1.0, 2.0], np.float32)
    d = pl.with_pick(pl.point_light_scene(w32), pl.CUSTOM, 0.0, w32)
    mode, w, m, pmf, cdf = pl.tables(d)
    assert m[1] == 1 and m[2] == 0
    assert np.array_equal(pl.pick_counts(d), m.astype(np.int64))
    # UNIFORM counts what int(r * n) gives
    u = pl.pick_counts(pl.with_pick(pl.point_light_scene(w32), None))
    assert u.sum() == Q and np.abs(u - Q / 7.0).max() < 4   # (r * n rounds: a float next to a boundary may cross it)


# ---------------------------------------------------------------- 4. POWER's weights are the lights' flux

def _lum(c):
    return 0.212671 * c[:, 0] + 0.715160 * c[:, 1] + 0.072169 * c[:, 2]


def _five_light_scenes():
    from smallvcm_amd.scene2 import SceneBuilder

    def room(extra):
        b = SceneBuilder()
        m = b.material(diffuse=(0.7, 0.7, 0.7))
        b.triangle((-2, -2, 0), (2, -2, 0), (2, 2, 0), m)
        b.triangle((2, 2, 0), (-2, 2, 0), (-2, -2, 0), m)
        b.emissive_triangle((-0.5, -0.2, 2.0), (0.7, -0.3, 2.1), (0.1, 0.6, 1.9), (3.0, 2.0, 0.5))   # area: light 0
        b.point_light((0.2, 0.1, 1.0), (0.4, 1.1, 2.0))                                             # point: light 1
        b.directional_light((-1.0, 0.5, -1.0), (1.5, 0.7, 0.2))                                     # directional: 2
        extra(b)                                                                                    # background / map: 3
        return pl.as_desc4(b.build((0, -5, 2), (0, 1, -0.3), (0, 0, 1), 50, 8, 8))
    sky = el.sky(32, 16, sun=(0.55, 0.2), sun_size=2, sun_value=(30.0, 27.0, 22.0))
    return room(lambda b: b.background_light(1.7)), room(lambda b: b.envmap_light(sky, 1.3))


def test_power_weights_are_the_lights_flux():
    n = 200000
    rng = np.random.default_rng(4)
    seen = set()
    for d4 in _five_light_scenes():
        d = pl.with_pick(d4, pl.POWER)
        mode, w, m, pmf, cdf = pl.tables(d)
        assert mode == pl.POWER and np.all(w > 0)
        base = d4.base.base
        for i in range(pl.n_lights(d4)):
            inp = np.zeros((n, pl.KAT), np.float32)
            inp[:, 0] = i
            inp[:, 1:5] = rng.random((n, 4))
            out = pl.kat5(d, pl.OP_LIGHT_EMIT, inp).astype(np.float64)
            est = np.where(out[:, 9] > 0, _lum(out[:, 0:3]) / np.where(out[:, 9] > 0, out[:, 9], 1.0), 0.0)
            mean, se = est.mean(), est.std(ddof=1) / np.sqrt(n)
            t = int(base.lights[i].type)
            seen.add(t)
            print("light type %d: estimator %.6g +- %.2g, weight %.6g" % (t, mean, se, w[i]))
            assert abs(mean - w[i]) <= 4 * se + 1e-5 * w[i], (t, mean, se, w[i])
            if t == 2:   # a point light's estimator is a constant
                assert se <= 1e-6 * mean
    assert seen == {0, 1, 2, 3, 4}


# ---------------------------------------------------------------- 5. unbiased in every algorithm

def _estimate(d, algo, iters, seed0, rf=0.003, b=6, min_len=0):
    """mean and standard error per b x b block over 4 independent renders (test_thin_lens._estimate over Emul5)"""
    reps = []
    for k in range(4):
        r = pl.Emul5(d, algo, seed=seed0 + k, radius_factor=rf)
        for it in range(iters):
            r.run_iteration(it, min_len, 10)
        reps.append(_blocks(r.framebuffer() / iters, b))
    reps = np.array(reps)
    return reps.mean(axis=0), reps.std(axis=0, ddof=1) / 2.0


def _variants(d4):
    n = pl.n_lights(d4)
    skew = np.ones(n, np.float32)
    skew[0], skew[1], skew[-1] = 40.0, 10.0, 4.0   # the two lamp triangles unequal, the point light favoured
    return [("power", pl.with_pick(d4, pl.POWER)), ("power mix 0.5", pl.with_pick(d4, pl.POWER, 0.5)),
            ("custom", pl.with_pick(d4, pl.CUSTOM, 0.0, skew))]


@pytest.mark.parametrize("algo,iters", [(5, 24), (3, 40), (4, 10)])
def test_modes_agree_with_uniform(algo, iters):
    """PT, BPT and VCM on the full many-light room: POWER, POWER with a uniform share and a skewed CUSTOM estimate, per
    block, what UNIFORM estimates.  A renderer that uses the pmf where it samples a light and 1 / n where a path hits
    one fails this: PT per block (z = 11.2); BPT, at the 40 iterations it runs here so that the image mean settles
    to about half a percent, by its mean (7.3 to 7.6 % too bright against the bound of 5 %; 0.6 to 0.8 % as built) with
    z = 4.4 to 4.8 per block -- at 12 iterations it was z = 5.18, too close to the bound to rely on."""
    d4 = pl.lamp_room()
    ref = _estimate(pl.with_pick(d4, None), algo, 2 * iters, 900 + algo)
    assert ref[0].mean() > 0.05
    for name, d in _variants(d4):
        _agree(_estimate(d, algo, iters, 300 + algo), ref, (algo, name))


def test_light_tracing_and_bpm_agree_with_the_path_tracer():
    """LT cannot render what is seen through specular objects and BPM's merges only converge as the radius shrinks: as
    in test_thin_lens they are compared with PT (UNIFORM: the yardstick) on the room without the spheres.  That test's
    box has no light in view; this room's emitters are in view, and LT cannot render an emitter the camera sees
    directly, so paths start at length 2 on both sides (mMinPathLength = 2).  Iterations: with 67 lights the per-block
    estimators have heavy tails and four renders give a poor standard error, so this runs 600 (PT, LT) and 160 (BPM)
    iterations; measured max z: LT 3.61 / 3.63 / 2.85, BPM 4.00 / 4.75 / 3.92 (power / mix / custom).  For scale, UNIFORM
    itself measures LT 4.55 and BPM 8.53 against PT at these counts: on this room uniform picks are what converges badly."""
    d4 = pl.lamp_room(specular=False)
    pt = _estimate(pl.with_pick(d4, None), 5, 600, 510, b=3, min_len=2)
    for name, d in _variants(d4):
        _agree(_estimate(d, 0, 600, 10, b=3, min_len=2), pt, ("lt", name))
        _agree(_estimate(d, 2, 160, 210, rf=0.02, b=3, min_len=2), pt, ("bpm", name))


# ---------------------------------------------------------------- 6. it helps

# MSE(UNIFORM) / MSE(POWER) MEASURED on the emulation (lamp_room: 67 lights, 24 x 24, 8 iterations, 4 seeds, paths from
# length 2, reference: UNIFORM with 50 x the iterations): PT 5.22, BPT 5.75.  The test asserts the square root of the
# measured ratio (half-way on a log scale: room for seed-to-seed scatter) and that the scene keeps the measured ratio >= 4.
MEASURED_RATIO = {5: 5.22, 3: 5.75}


@pytest.mark.parametrize("algo", [5, 3])
def test_power_lowers_the_error(algo):
    d4 = pl.lamp_room()
    iters = 8
    ref = pl.Emul5(pl.with_pick(d4, None), algo, seed=77)
    for it in range(50 * iters):
        ref.run_iteration(it, 2, 10)
    want = ref.framebuffer().astype(np.float64) / (50 * iters)

    def mse(d):
        out = []
        for seed in range(4):
            r = pl.Emul5(d, algo, seed=1000 + seed)
            for it in range(iters):
                r.run_iteration(it, 2, 10)   # from length 2: an emitter seen directly is the same in both modes
            out.append(np.mean((r.framebuffer().astype(np.float64) / iters - want) ** 2))
        return float(np.mean(out))
    ratio = mse(pl.with_pick(d4, None)) / mse(pl.with_pick(d4, pl.POWER))
    print("algo %d: MSE(UNIFORM) / MSE(POWER) = %.2f" % (algo, ratio))
    assert MEASURED_RATIO[algo] >= 4.0
    assert ratio >= np.sqrt(MEASURED_RATIO[algo]), ratio


# ---------------------------------------------------------------- 7. the tapes

@pytest.mark.parametrize("algo", range(7))
def test_one_light_scene_is_the_same_in_every_mode(algo):
    """one light: pmf = 1 = 1.f / 1, the same floats drawn, the same image"""
    d4 = pl.as_desc4(ll.builtin3(mask=256 | 4, resx=20, resy=14))   # kGlossyFloor | kLightPoint
    assert pl.n_lights(d4) == 1
    rf = 0.05   # (a radius at which PPM's merges find photons at this size)
    ref = pl.Emul5(pl.with_pick(d4, None), algo, seed=9, radius_factor=rf)
    others = [pl.Emul5(pl.with_pick(d4, pl.POWER, 0.3), algo, seed=9, radius_factor=rf),
              pl.Emul5(pl.with_pick(d4, pl.CUSTOM, 0.0, [2.5]), algo, seed=9, radius_factor=rf)]
    for it in range(2):
        ref.run_iteration(it)
        for e in others:
            e.run_iteration(it)
    assert np.count_nonzero(ref.framebuffer()) > 0
    for e in others:
        assert _same(e, ref)


@pytest.mark.parametrize("algo", [0, 3, 4, 5])
def test_equal_probabilities_draw_the_uniform_tape(algo):
    """a table that gives n = 4 lights a quarter each reaches the lights UNIFORM reaches with the same floats: the same
    number of floats per path, the same image"""
    d3 = pl.add_point_lights(ll.builtin3(resx=20, resy=14), [((0.3, 0.2, 0.5), (1, 1, 1)), ((-0.4, 0.1, 0.2), (2, 1, 1)),
                                                           ((0.1, -0.6, 0.9), (0.5, 0.5, 2))])
    assert pl.n_lights(d3) == 4
    a = pl.Emul5(pl.with_pick(d3, None), algo, seed=2)
    b = pl.Emul5(pl.with_pick(d3, pl.CUSTOM, 0.0, [1.0, 1.0, 1.0, 1.0]), algo, seed=2)
    for it in range(2):
        a.run_iteration(it)
        b.run_iteration(it)
    assert _same(a, b)


# ---------------------------------------------------------------- 8. shards

@pytest.mark.parametrize("algo", range(7))
def test_sharded_emulation_equals_unsharded(algo):
    """as in test_thin_lens: scene 3's box (here with six more lights), where no merge is accepted at this size -- an
    emulated shard merges with the light vertices of its own paths only"""
    d = pl.with_pick(pl.box_many_lights(), pl.POWER, 0.1)
    full = pl.Emul5(d, algo, seed=3)
    shards = [pl.Emul5(d, algo, seed=3, rank=r, world=2) for r in range(2)]
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


# ---------------------------------------------------------------- 9. scene files and SceneBuilder

def test_scene_file_lightpick_directive(tmp_path):
    from smallvcm_amd.scene_file import load_scene
    (tmp_path / "quad.obj").write_text("mtllib quad.mtl\nv -1 -1 0\nv 1 -1 0\nv 1 1 0\nv -1 1 0\nusemtl white\nf 1 2 3 4\n")
    (tmp_path / "quad.mtl").write_text("newmtl white\nKd 0.8 0.8 0.8\n")
    head = "obj quad.obj\ncamera 0 -4 2  0 1 -0.4  0 0 1  50\nlight background 1\nlight point 0 0 2  3 3 3\n"
    (tmp_path / "s.vcmscene").write_text(head + "lightpick power 0.25   # by flux, a quarter uniform\n")
    d = load_scene(tmp_path / "s.vcmscene", 16, 12)
    assert isinstance(d, SceneDesc5) and d.pick
    assert (d.pick.contents.mode, d.pick.contents.uniformMix) == (pl.POWER, 0.25)
    assert not d.base.lens and d.camera.resolution[0] == 16
    assert pl.tables(d)[0] == pl.POWER
    (tmp_path / "u.vcmscene").write_text(head + "lightpick uniform\nlens 0.1 3\n")
    d = load_scene(tmp_path / "u.vcmscene", 8, 8)
    assert isinstance(d, SceneDesc5) and d.pick.contents.mode == pl.UNIFORM and d.base.lens
    (tmp_path / "plain.vcmscene").write_text(head)
    assert not isinstance(load_scene(tmp_path / "plain.vcmscene", 8, 8), SceneDesc5)   # only when asked to
    (tmp_path / "lens.vcmscene").write_text(head + "lens 0.1 3\n")
    assert type(load_scene(tmp_path / "lens.vcmscene", 8, 8)) is SceneDesc4
    for bad in ("lightpick", "lightpick brightest", "lightpick power x", "lightpick power 0.1 7", "lightpick power -0.1",
                "lightpick power 1.5", "lightpick power nan", "lightpick power\nlightpick uniform"):
        (tmp_path / "bad.vcmscene").write_text(head + bad + "\n")
        with pytest.raises(ValueError, match="lightpick"):
            load_scene(tmp_path / "bad.vcmscene", 8, 8)


def test_scene_builder_light_pick():
    from smallvcm_amd.scene2 import SceneBuilder

    def builder():
        b = SceneBuilder()
        m = b.material(diffuse=(0.7, 0.7, 0.7))
        b.triangle((-1, -1, 0), (1, -1, 0), (1, 1, 0), m)
        b.background_light(1.0)
        b.point_light((0, 0, 2), (3, 3, 3))
        return b

    cam = ((0, -4, 2), (0, 1, -0.4), (0, 0, 1), 50, 16, 12)
    b = builder()
    b.light_pick()
    d = b.build(*cam)
    assert isinstance(d, SceneDesc5) and d.pick.contents.mode == pl.POWER and not d.base.lens and not d.base.base.envmap
    plain = builder().build(*cam)
    assert not isinstance(plain, SceneDesc5) and bytes(d.camera) == bytes(plain.camera)
    e = pl.Emul5(d, 5, seed=1)   # the description is complete
    e.run_iteration(0)
    assert np.count_nonzero(e.framebuffer()) > 0
    b = builder()
    b.thin_lens(0.1, 2.0)
    b.light_pick("custom", 0.5, [1.0, 3.0])
    d = b.build(*cam)
    assert isinstance(d, SceneDesc5) and d.base.lens and d.pick.contents.uniformMix == 0.5
    mode, w, m, pmf, cdf = pl.tables(d)
    assert mode == pl.CUSTOM and list(m) == [Q // 2 * 3 // 4, Q - Q // 2 * 3 // 4]   # 0.5 * (1/4, 3/4) + 0.5 * (1/2, 1/2)
    for args in (("brightest",), ("power", -0.1), ("power", float("nan")), ("custom",), ("custom", 0.0, [1.0, -1.0]),
                 ("custom", 0.0, [0.0, 0.0]), ("power", 0.0, [1.0, 1.0])):
        with pytest.raises(ValueError):
            builder().light_pick(*args)
    b = builder()
    b.light_pick("custom", 0.0, [1.0, 2.0, 3.0])
    with pytest.raises(ValueError):
        b.build(*cam)
