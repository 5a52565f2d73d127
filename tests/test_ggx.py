"""The GGX lobe on the CPU (host emulation of the device functions, tests/host_emul_ggx): the known-answer ops against a
binary64 numpy restatement of the model, the identities of the lobe on the ops' outputs, its directional albedo against
quadrature, the degenerate cases (no lobe = version 7, bit for bit) and every refusal of the scene host."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import ggx_lib as gl
from smallvcm_amd._abi import SceneDesc8, with_material_ext

STAT_KEYS = ("lightVertices", "lightRays", "cameraRays", "shadowRays", "mergeQueries", "mergeCandidates",
             "mergeAccepted", "connections", "lightSplats")
TOL = 1e-4    # relative: about forty binary32 roundings are 2.4e-6, a wrong formula is percents
EDGE = 1e-4   # records this close to a branch threshold are left out


@pytest.fixture(scope="module")
def kat():
    """the scene, the 50 000 records of both ops and the emulation's answers: computed once, read-only"""
    d = gl.kat_scene()
    assert isinstance(d, SceneDesc8)
    ev, sa = gl.random_records()
    out = {"scene": d, "ev": ev, "sa": sa, "ev_out": gl.kat8(d, gl.OP_BSDF_EVAL, ev), "sa_out": gl.kat8(d, gl.OP_BSDF_SAMPLE, sa)}
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def _local(rec):
    fr = gl.frame(rec[:, 3:6].astype(np.float64))
    o = gl.to_local(fr, -rec[:, 0:3].astype(np.float64))
    return fr, o, rec[:, 6].astype(int)


def _close(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b) <= TOL * np.maximum(np.abs(a), np.abs(b)) + 1e-30


def test_evaluate_against_numpy(kat):
    rec, out = kat["ev"], kat["ev_out"]
    fr, o, mat = _local(rec)
    i = gl.to_local(fr, rec[:, 7:10].astype(np.float64))
    pr = gl.probabilities(o, mat)
    f, pd, prv, dot_rw, oh = gl.evaluate(o, i, mat, pr)
    keep = ((np.abs(np.abs(o[:, 2]) - gl.EPS_COSINE) > EDGE) & (np.abs(i[:, 2] - gl.EPS_COSINE) > EDGE) & (np.abs(i[:, 2] * o[:, 2]) > EDGE * 1e-2)
            & (np.abs(dot_rw - gl.EPS_PHONG) > EDGE) & ~((oh < EDGE) & (o[:, 2] > 0) & (i[:, 2] > 0)))
    print("left out %.3f %%" % (100 * (1 - keep.mean())))
    assert 1 - keep.mean() <= 0.01
    valid = np.abs(o[:, 2]) >= gl.EPS_COSINE
    assert np.array_equal(out[keep, 0] == 1.0, valid[keep])
    k = keep & valid
    assert np.count_nonzero(k & (f[:, 0] > 0) & (pr["g"] > 0)) > 20000   # the lobe is what most records evaluate
    assert np.all(_close(out[k, 2], pr["cont"][k])), "continuation probability"
    for c in range(3):
        assert np.all(_close(out[k, 3 + c], f[k, c])), "value"
    assert np.all(_close(out[k, 7], pd[k])) and np.all(_close(out[k, 8], prv[k])), "pdfs of Evaluate"
    assert np.all(_close(out[k, 14], o[k, 2]))
    delta = (pr["d"] == 0) & (pr["p"] == 0) & (pr["g"] == 0)
    assert np.array_equal(out[k, 1] == 1.0, delta[k])
    # Pdf() holds no EPS_COSINE guard for the diffuse lobe (the reference's), the GGX lobe keeps its own
    both = k & (o[:, 2] >= gl.EPS_COSINE) & (i[:, 2] >= gl.EPS_COSINE)
    assert np.all(_close(out[both, 9], pd[both])) and np.all(_close(out[both, 10], prv[both])), "Pdf()"


def test_sample_against_numpy(kat):
    rec, out = kat["sa"], kat["sa_out"]
    fr, o, mat = _local(rec)
    kd, ks, n, km, ior, f0, a = gl._materials(mat)
    pr = gl.probabilities(o, mat)
    r0, r1, r2 = (rec[:, 7 + c].astype(np.float64) for c in range(3))
    cum = np.cumsum(np.stack([pr["d"], pr["p"], pr["g"], pr["r"]], axis=1), axis=1)
    branch = (r2[:, None] >= cum).sum(axis=1)   # 0 diffuse, 1 phong, 2 ggx, 3 reflect, 4 refract
    valid = np.abs(o[:, 2]) >= gl.EPS_COSINE
    # the three lobes in numpy; the delta branches belong to the reference and are not restated
    phi = 2 * np.pi * r0
    gen = np.zeros_like(o)
    t2 = np.sqrt(1 - r1)
    gen_d = np.stack([np.cos(phi) * t2, np.sin(phi) * t2, np.sqrt(r1)], axis=1)
    with np.errstate(all="ignore"):
        c2 = r1 ** (1 / (n + 1))
    c3 = np.sqrt(1 - c2 ** 2)
    refl = o * np.array([-1.0, -1.0, 1.0])
    gen_p = gl.to_world(gl.frame(refl), np.stack([np.cos(phi) * c3, np.sin(phi) * c3, c2], axis=1))
    gen_g = gl.ggx_sample(o, a, r0, r1)
    for b, g in ((0, gen_d), (1, gen_p), (2, gen_g)):
        gen[branch == b] = g[branch == b]
    f, pd, _, dot_rw, oh = gl.evaluate(o, gen, mat, pr)
    back = valid & (o[:, 2] < 0) & ((branch == 0) | (branch == 2))
    assert back.sum() > 1000 and np.all(out[back, 7] == 0), "one-sided: nothing is sampled from behind"
    # (SamplePhong from behind, and its samples below the surface, which the reference keeps, are the reference's own business)
    lobe = valid & (branch <= 2) & (o[:, 2] > 0) & ~((branch == 1) & (gen[:, 2] <= 0))
    # Left out, all by rules on the inputs and on numpy's own sample, and all inside the 1 % cap: a branch threshold within
    # EDGE, and GGX samples whose half vector is ill-conditioned in binary32 -- the op's direction is off by ~5e-8, the
    # half vector by that over |o + i| >= o_z + i_z and the lobe's d by that over alpha, so below alpha (o_z + i_z) = 1e-3
    # the op's own rounding exceeds half the tolerance.  Where the lobe is evaluated at a diffuse or Phong sample, whose
    # direction went through sqrt / pow and (Phong) a second frame and is off by ten times as much, the rule is 1e-2.
    near = (np.abs(r2[:, None] - cum) < EDGE).any(axis=1) | (np.abs(gen[:, 2] - gl.EPS_COSINE) < EDGE) | (np.abs(np.abs(o[:, 2]) - gl.EPS_COSINE) < EDGE) \
        | (np.abs(dot_rw - gl.EPS_PHONG) < EDGE) | ((branch == 2) & (oh < EDGE)) | ((branch == 2) & (a * (o[:, 2] + gen[:, 2]) < 1e-3)) \
        | ((branch != 2) & (pr["g"] != 0) & (a * (o[:, 2] + gen[:, 2]) < 1e-2))
    print("left out %.3f %% of the lobe samples" % (100 * (near & lobe).sum() / lobe.sum()))
    assert (near & lobe).sum() <= 0.01 * lobe.sum()
    k = lobe & ~near
    # discarded: the fixed direction below the surface, the sample below it, or (Phong) off the lobe
    gone = (o[:, 2] < gl.EPS_COSINE) | (gen[:, 2] < gl.EPS_COSINE) | ((branch == 1) & (dot_rw <= gl.EPS_PHONG))
    assert np.array_equal((out[k, 7] == 0) & (out[k, 9] == 0), gone[k])
    k &= ~gone
    assert np.count_nonzero(k & (branch == 2)) > 10000
    assert np.array_equal(out[k, 9].astype(int), np.array([gl.K_DIFFUSE, gl.K_PHONG, gl.K_GGX])[branch[k]])
    world = gl.to_world(fr, gen)
    err = np.abs(out[:, 4:7] - world).max(axis=1)
    print("largest direction error %.3g" % err[k].max())
    assert np.all(err[k] <= 1e-4), "the sampled direction, every kept record"
    for c in range(3):
        assert np.all(_close(out[k, 1 + c], f[k, c])), "value"
    assert np.all(_close(out[k, 7], pd[k])), "pdf"
    # (a component of a unit vector: 1e-4 relative, or five binary32 ulps of 1 where it is small)
    assert np.all(_close(out[k, 8], gen[k, 2]) | (np.abs(out[k, 8] - gen[k, 2]) <= 6e-7)), "cosine"
    k2 = k
    # both fixIsLight took part, and the lobe has no adjoint case: the answers do not depend on it
    assert 0.4 < rec[k2, 10].mean() < 0.6
    flipped = np.array(rec)
    flipped[:, 10] = 1 - flipped[:, 10]
    again = gl.kat8(kat["scene"], gl.OP_BSDF_SAMPLE, flipped)
    assert np.array_equal(again[k].view(np.uint32), out[k].view(np.uint32))


def _pure_eval(alpha_mat, o, i):
    """the eval op on material `alpha_mat` for local directions about the normal +z"""
    rec = np.zeros((len(o), gl.KAT), np.float32)
    rec[:, 0:3], rec[:, 3:6], rec[:, 6], rec[:, 7:10] = -o, (0, 0, 1), alpha_mat, i
    return rec


def test_identities_on_the_ops_outputs(kat):
    d = kat["scene"]
    rng = np.random.default_rng(3)
    n = 20000
    o, i = gl._unit(rng, n), gl._unit(rng, n)
    o[:, 2], i[:, 2] = np.abs(o[:, 2]), np.abs(i[:, 2])
    for mat in (0, 1, 2, 3):   # the pure lobes: the component probabilities are 1 in both orders
        a = gl.kat8(d, gl.OP_BSDF_EVAL, _pure_eval(mat, o, i))
        b = gl.kat8(d, gl.OP_BSDF_EVAL, _pure_eval(mat, i, o))
        ok = (a[:, 0] == 1) & (b[:, 0] == 1)
        assert ok.mean() > 0.99
        tol = TOL   # (the frame about +z hands the op the records' own binary32 components in both orders)
        for c in (3, 4, 5):
            assert np.all(np.abs(a[ok, c] - b[ok, c]) <= tol * np.maximum(np.abs(a[ok, c]), np.abs(b[ok, c])) + 1e-30), "f(o, i) = f(i, o)"
        assert np.all(np.abs(a[ok, 7] - b[ok, 8]) <= tol * np.maximum(a[ok, 7], b[ok, 8]) + 1e-30), "direct pdf (o, i) = reverse pdf (i, o)"
    # pure lobes: the sample weight f cos / pdf never exceeds 1; F0 = 1: it is G2 / G1
    rec = np.array(kat["sa"])
    for mat in (0, 1, 2, 3):
        rec[:, 6] = mat
        out = gl.kat8(d, gl.OP_BSDF_SAMPLE, rec)
        hit = out[:, 7] > 0
        assert hit.sum() > 0.3 * len(rec)
        w = out[hit, 1:4].astype(np.float64) * out[hit, 8:9] / out[hit, 7:8]
        assert w.max() <= 1 + 1e-5, w.max()
        if mat == 0:
            fr, ol, _ = _local(rec[hit])
            il = gl.to_local(fr, out[hit, 4:7].astype(np.float64))
            a = gl.KAT_MATERIALS[0][6]
            lo, li = gl.lam(ol, a), gl.lam(il, a)
            assert np.all(np.abs(w[:, 0] - (1 + lo) / (1 + lo + li)) <= 1e-4)


@pytest.mark.parametrize("mat,theta", [(0, 0.5), (1, 0.0), (1, 1.2), (2, 0.5), (2, 1.5), (3, 1.2)])
def test_directional_albedo(kat, mat, theta):
    """the mean sample weight of 10^5 draws against quadrature of f cos (F0 = the material's first channel)"""
    _, _, _, _, _, f0, alpha = gl.KAT_MATERIALS[mat]
    n = 100000
    rng = np.random.default_rng(100 + mat)
    rec = np.zeros((n, gl.KAT), np.float32)
    rec[:, 0:3] = (-np.sin(theta), 0.0, -np.cos(theta))
    rec[:, 3:6], rec[:, 6] = (0, 0, 1), mat
    rec[:, 7:10] = gl.uniforms(rng, (n, 3))
    out = gl.kat8(kat["scene"], gl.OP_BSDF_SAMPLE, rec)
    with np.errstate(all="ignore"):
        w = np.where(out[:, 7] > 0, out[:, 1].astype(np.float64) * out[:, 8] / out[:, 7], 0.0)
    # Schlick is affine in F0: quadrature once at F0 = 1 and once at F0 = 0
    ref = f0[0] * gl.directional_albedo(alpha, theta, 1.0) + (1 - f0[0]) * gl.directional_albedo(alpha, theta, 0.0)
    se = w.std(ddof=1) / np.sqrt(n)
    print("alpha %g theta %g: sampled %.6f +- %.6f, quadrature %.6f" % (alpha, theta, w.mean(), se, ref))
    assert abs(w.mean() - ref) <= 5 * se


def _run(emu, iters, max_len=10):
    tapes = []
    for it in range(iters):
        emu.run_iteration(it, 0, max_len)
        tapes.append(tuple(np.array(t) for t in emu.counts()))
    return emu.framebuffer(), tapes, emu.stats()


@pytest.mark.parametrize("algo", range(7))
def test_no_lobe_is_version_7_bit_for_bit(algo):
    """ext NULL and ext all zero (alpha anything): framebuffer, both tapes, counters"""
    d7 = gl.as_desc7(gl.room(phong=True))
    n = int(gl.desc2_of(d7).nMaterials)
    want = _run(gl.Emul8(d7, algo, seed=5, version7=True), 2)
    assert np.count_nonzero(want[0]) > 0
    for ext in (None, [(0, 0, 0, 0.0)] * n, [(0, 0, 0, 0.3)] * n):
        got = _run(gl.Emul8(with_material_ext(d7, ext), algo, seed=5), 2)
        assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32))
        for (lc, cc), (wl, wc) in zip(got[1], want[1]):
            assert np.array_equal(lc, wl) and np.array_equal(cc, wc)
        for k in STAT_KEYS:
            assert got[2][k] == want[2][k], k


def test_paths_that_never_touch_the_lobe_draw_the_same_tape():
    """the Phong room, and the same room with a lobe on ONE material that no primitive uses: every path's tape and the
    image are those of version 7 (the material table is what changed, the kernels' kind with it)"""
    d7 = gl.as_desc7(gl.room(phong=True, n_materials=9))
    n = int(gl.desc2_of(d7).nMaterials)
    ext = [(0, 0, 0, 0.0)] * n
    ext[7] = (0.5, 0.5, 0.5, 0.2)   # the first padding material: no primitive has it
    for algo in (4, 5):
        want = _run(gl.Emul8(d7, algo, seed=8, version7=True), 2)
        got = _run(gl.Emul8(with_material_ext(d7, ext), algo, seed=8), 2)
        assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32))
        for (lc, cc), (wl, wc) in zip(got[1], want[1]):
            assert np.array_equal(lc, wl) and np.array_equal(cc, wc)




def test_a_used_lobe_leaves_the_paths_that_miss_it_alone():
    """One material IN USE has the lobe: a small plate on the floor of the Phong room.  Path tracing with paths up to
    length 2 (the camera ray and its shadow ray): a pixel whose rays all miss the plate -- by the geometry of its
    footprint, with a margin of a pixel -- draws version 7's tape and gets version 7's value, bit for bit, in a context
    that runs the GGX kind; the pixels wholly on the plate change."""
    d7 = gl.as_desc7(gl.room(24, 24, specular=False, phong=True, n_materials=7))
    n = int(gl.desc2_of(d7).nMaterials)
    ext = [(0, 0, 0, 0.0)] * n
    ext[6] = (0.8, 0.7, 0.6, 0.1)   # the plate's material (ggx_lib.room: the last padding material)
    k = 5
    g = np.linspace(-1.0, 2.0, 3 * k + 1)   # the pixel and a margin of one pixel around it
    yy, xx, v, u = np.meshgrid(np.arange(24), np.arange(24), g, g, indexing="ij")
    org, dirs = gl.camera_rays(d7, np.stack([(xx + u).ravel(), (yy + v).ravel()], axis=1))
    t = (-1.25 + 0.01 - org[2]) / dirs[:, 2]
    p = org + t[:, None] * dirs
    on = ((t > 0) & (np.abs(p[:, 0]) <= 0.2) & (p[:, 1] >= -0.9) & (p[:, 1] <= -0.5)).reshape(24, 24, -1)   # the plate's bounding box
    miss = ~on.any(axis=2)
    want, got = gl.Emul8(d7, 5, seed=8, version7=True), gl.Emul8(with_material_ext(d7, ext), 5, seed=8)
    for it in range(2):
        want.run_iteration(it, 0, 2)
        got.run_iteration(it, 0, 2)
        wc, gc = want.counts()[1].reshape(24, 24), got.counts()[1].reshape(24, 24)
        assert np.array_equal(wc[miss], gc[miss]), "camera tape"
    wf, gf = want.framebuffer().reshape(24, 24, 3), got.framebuffer().reshape(24, 24, 3)
    assert miss.sum() > 500 and np.array_equal(wf[miss].view(np.uint32), gf[miss].view(np.uint32))
    assert np.any(wf[~miss] != gf[~miss]), "the plate is in view and its lobe changes its pixels"

# ---------------------------------------------------------------- images
# (square images throughout: the reference's camera takes ONE field of view for both axes and derives the pixel's solid
# angle from the width alone, so on a non-square image light tracing and the camera estimators differ by the aspect
# ratio -- in the reference and here, with any material)

def _blocks(img, b=4):
    h, w, _ = img.shape
    return img.reshape(h // b, b, w // b, b, 3).mean(axis=(1, 3))


def _seed_means(d, algo, seeds, iters, min_len, max_len, rf=0.003):
    out = []
    for s in seeds:
        e = gl.Emul8(d, algo, seed=s, radius_factor=rf)
        for it in range(iters):
            e.run_iteration(it, min_len, max_len)
        out.append(_blocks(e.framebuffer().astype(np.float64).reshape(e.resy, e.resx, 3) / iters))
    out = np.array(out)
    return out.mean(axis=0), out.std(axis=0, ddof=1) / np.sqrt(len(seeds))


@pytest.fixture(scope="module")
def floor():
    d = gl.floor_scene(24)
    return d, gl.floor_reference(d, 24)


@pytest.mark.parametrize("algo", [0, 5, 3])
def test_floor_against_the_closed_form(floor, algo):
    """A GGX floor under a point light through the pinhole, paths of length 2 only: light tracing, path tracing and BPT
    against f I cos(theta) / d^2, per 4 x 4 block within 5 combined standard errors of 24 seeds and a numpy Monte Carlo of
    the block's footprint; every block counts"""
    d, (ref, ref_se) = floor
    m, se = _seed_means(d, algo, [100 + 17 * k for k in range(24)], 16, 2, 2)
    z = np.abs(m - ref) / np.sqrt(se ** 2 + ref_se ** 2)
    print("algo %d: mean ratio %.4f, worst block %.2f standard errors" % (algo, m.mean() / ref.mean(), z.max()))
    assert ref.min() > 0 and z.max() <= 5.0


ROOM_RES = 56   # at 4 x 4 blocks the two silhouettes cross less than 15 % of the blocks


@pytest.fixture(scope="module")
def room_pt():
    """the path tracer's block means in both rooms under both samplers, computed once: (room with spheres, all path
    lengths) and (room without, paths from length 2 on, as LT cannot see an emitter directly)"""
    return {(spec, smp): _seed_means(gl.room(ROOM_RES, ROOM_RES, specular=spec, sampler=smp), 5, range(12), 24, 0 if spec else 2, 10)
            for spec in (True, False) for smp in (None, "sobol")}


@pytest.mark.parametrize("sampler", [None, "sobol"])
@pytest.mark.parametrize("algo,specular", [(3, True), (4, True), (0, False), (2, False)])
def test_algorithms_agree_with_the_path_tracer(room_pt, algo, specular, sampler):
    """BPT and VCM against PT per 4 x 4 block in the closed room (a sphere light, a GGX floor, a mixed diffuse + GGX wall,
    a glass and a mirror sphere); LT and BPM against PT in the room without spheres.  Within 5 combined standard errors
    of 12 seeds.  The two merging estimators are biased by their radius (the density estimate averages over a disc, and
    at a wall the disc hangs over the edge): BPM runs at radius factor 0.005, a disc of 2 x 0.005 x the scene radius
    (3.4) = 0.034 across, below the 0.045 that one pixel of the 56 covers at the walls, so the blur stays under the
    image's own resolution; both get the 2 % of the block's value that the suite's other estimator comparisons give
    them (test_thin_lens._agree).  The only blocks left out are those a sphere's silhouette crosses."""
    d = gl.room(ROOM_RES, ROOM_RES, specular=specular, sampler=sampler)
    ref, ref_se = room_pt[(specular, sampler)]
    m, se = _seed_means(d, algo, range(100, 112), 12, 0 if specular else 2, 10, rf=0.005 if algo == 2 else 0.003)
    skip = gl.silhouette_blocks(d, ROOM_RES) if specular else np.zeros(ref.shape[:2], bool)
    print("left out (a silhouette crosses them): %.1f %%" % (100 * skip.mean()), np.argwhere(skip).tolist())
    assert skip.mean() <= 0.15
    bias = (0.02 * ref) ** 2 if algo in (2, 4) else 0.0
    z = (np.abs(m - ref) / np.sqrt(se ** 2 + ref_se ** 2 + bias + 1e-30))[~skip]
    print("algo %d: mean ratio %.4f, worst block %.2f standard errors" % (algo, m.mean() / ref.mean(), z.max()))
    assert ref.mean() > 0.05 and z.max() <= 5.0


# ---- the scene host
def _desc(ext, light_material=False):
    from smallvcm_amd.scene2 import SceneBuilder
    b = SceneBuilder()
    m = b.material(diffuse=(0.5, 0.5, 0.5))
    b.triangle((0, 0, 0), (1, 0, 0), (1, 1, 0), m)
    if light_material:
        b.emissive_triangle((0, 0, 2), (1, 1, 2), (1, 0, 2), (1, 1, 1))
    else:
        b.point_light((0, 0, 3), (1, 1, 1))
    d = b.build((0, -3, 1), (0, 1, 0), (0, 0, 1), 45.0, 8, 8)
    n = int(gl.desc2_of(d).nMaterials)
    return with_material_ext(d, [ext] * n if ext is not None else None)


@pytest.mark.parametrize("ext,text", [
    ((float("nan"), 0.5, 0.5, 0.3), "not finite"), ((0.5, 0.5, 0.5, float("inf")), "not finite"),
    ((1.5, 0.5, 0.5, 0.3), "[0, 1]"), ((0.5, -0.1, 0.5, 0.3), "[0, 1]"),
    ((0.5, 0.5, 0.5, 0.005), "alpha"), ((0.5, 0.5, 0.5, 1.5), "alpha"), ((0.0, 0.0, 0.1, 0.0), "alpha")])
def test_refusals(ext, text):
    msg, table = gl.check(_desc(ext))
    assert table is None and text in msg and "materialExt[0]" in msg, msg


def test_a_lobe_on_a_light_is_refused_and_alpha_without_a_lobe_is_not_looked_at():
    msg, _ = gl.check(_desc((0.5, 0.5, 0.5, 0.3), light_material=True))
    assert msg is not None and "light" in msg, msg
    for ext in (None, (0, 0, 0, 0.0), (0, 0, 0, 7.0)):
        msg, table = gl.check(_desc(ext))
        assert msg is None and len(table) == 0   # the version-7 scene
    msg, table = gl.check(_desc((0.25, 0.5, 1.0, 0.01)))
    assert msg is None and np.array_equal(table, np.array([[0.25, 0.5, 1.0, 0.01]], np.float32))


def test_builder_returns_version_8_only_with_a_lobe():
    assert isinstance(gl.room(), SceneDesc8) and not isinstance(gl.room(phong=True), SceneDesc8)
    d = gl.kat_scene()
    msg, table = gl.check(d)
    assert msg is None
    want = np.array([m[5] + (m[6],) for m in gl.KAT_MATERIALS], np.float32)
    assert np.array_equal(table, want)
    assert isinstance(C.cast(d.materialExt, C.c_void_p).value, int)


# ---- .mtl
MTL = ("newmtl floor\nKd 0.1 0.2 0.3\nKs 0.9 0.75 0.5\nNs 40\nPr 0.5\nnewmtl wall\nKd 0.5 0.5 0.5\nKs 0.2 0.3 0.2\nNs 30\n"
       "newmtl shiny\nKs 0.8 0.8 0.8\nPr 0.05\nnewmtl mirror\nKs 1 1 1\nPr 0.3\nillum 3\nnewmtl lamp\nKe 5 5 5\n")
OBJ = ("mtllib m.mtl\nv -1 -1 0\nv 1 -1 0\nv 1 1 0\nv -1 1 0\nusemtl floor\nf 1 2 3 4\nv -1 1 0\nv 1 1 0\nv 1 1 2\nusemtl wall\nf 5 6 7\n"
       "v -1 1 2\nusemtl shiny\nf 5 7 8\nv 0 0 2\nv 1 0 2\nv 0 1 2\nusemtl lamp\nf -3 -1 -2\n")


def _write_scene(tmp_path, mtl=MTL):
    (tmp_path / "m.mtl").write_text(mtl)
    (tmp_path / "m.obj").write_text(OBJ)
    (tmp_path / "s.vcmscene").write_text("obj m.obj\nsphere 0.2 0.2 0.5 0.25 mirror\ncamera 0 -4 1 0 1 0 0 0 1 45\n")
    return str(tmp_path / "s.vcmscene")


def test_pr_in_mtl_equals_the_builder_field_for_field(tmp_path):
    """Pr sends Ks to F0 with alpha = max(Pr^2, 0.01) instead of Phong with Ns; illum 3 stays a mirror"""
    from smallvcm_amd.scene2 import SceneBuilder
    from smallvcm_amd.scene_file import load_scene
    d = load_scene(_write_scene(tmp_path), 8, 8)
    assert isinstance(d, SceneDesc8)
    b = SceneBuilder()
    floor = b.material(diffuse=(0.1, 0.2, 0.3), ggx=(0.9, 0.75, 0.5), alpha=0.25)
    b.triangle((-1, -1, 0), (1, -1, 0), (1, 1, 0), floor); b.triangle((-1, -1, 0), (1, 1, 0), (-1, 1, 0), floor)
    wall = b.material(diffuse=(0.5, 0.5, 0.5), phong=(0.2, 0.3, 0.2), exponent=30.0)
    b.triangle((-1, 1, 0), (1, 1, 0), (1, 1, 2), wall)
    shiny = b.material(ggx=(0.8, 0.8, 0.8), alpha=0.01)   # 0.05^2 is below the floor
    b.triangle((-1, 1, 0), (1, 1, 2), (-1, 1, 2), shiny)
    b.emissive_triangle((0, 0, 2), (0, 1, 2), (1, 0, 2), (5, 5, 5))
    b.sphere((0.2, 0.2, 0.5), 0.25, b.material(mirror=(1, 1, 1)))
    want = b.build((0, -4, 1), (0, 1, 0), (0, 0, 1), 45.0, 8, 8)
    got2, want2 = gl.desc2_of(d), gl.desc2_of(want)
    assert got2.nMaterials == want2.nMaterials == 5
    for m in range(5):
        for f in ("diffuse", "phong", "mirror"):
            assert list(getattr(got2.materials[m], f)) == list(getattr(want2.materials[m], f)), (m, f)
        assert got2.materials[m].ior == want2.materials[m].ior and got2.mat2light[m] == want2.mat2light[m]
        assert got2.materials[m].phongExp == want2.materials[m].phongExp or m in (0, 2)   # (Ns of a Pr material is not looked at)
        assert list(d.materialExt[m].ggx) == list(want.materialExt[m].ggx), m
        if any(d.materialExt[m].ggx):
            assert d.materialExt[m].alpha == want.materialExt[m].alpha, m
    assert gl.check(d)[0] is None
    # without a Pr line in use the file is what it was
    plain = load_scene(_write_scene(tmp_path, MTL.replace("Pr 0.5\n", "").replace("Pr 0.05\n", "")), 8, 8)
    assert not isinstance(plain, SceneDesc8)
    assert list(gl.desc2_of(plain).materials[0].phong) == pytest.approx([0.9, 0.75, 0.5])


@pytest.mark.parametrize("line", ["Pr", "Pr x", "Pr -0.1", "Pr 1.5", "Pr nan", "Pr inf"])
def test_a_malformed_pr_is_named(tmp_path, line):
    from smallvcm_amd.scene_file import load_scene
    with pytest.raises(ValueError, match="m.mtl: bad Pr"):
        load_scene(_write_scene(tmp_path, "newmtl floor\nKs 1 1 1\n" + line + "\n" + MTL.replace("newmtl floor\n", "newmtl floor2\n")), 8, 8)


# ---- host sanitizers
def test_the_ext_checks_and_the_mtl_parse_run_clean_under_the_host_sanitizers(tmp_path):
    """tests/host_emul_ggx/sanitize_ggx: scene_host_set_material_ext on ordinary and hostile tables and the .mtl loader's
    Pr on good and malformed files, in a stand-alone program built with -fsanitize=address,undefined (CPU only)"""
    subprocess.run(["make", "-C", gl.EMUL_DIR, "sanitize_ggx"], check=True, stdout=subprocess.DEVNULL)
    r = subprocess.run([os.path.join(gl.EMUL_DIR, "sanitize_ggx"), str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
