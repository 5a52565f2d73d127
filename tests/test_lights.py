"""Spot and sphere lights on the CPU (DESIGN.md "Spot and sphere lights"): the host emulation of the device functions
against closed forms (a lit floor), the estimators against each other in a room with one light of every finite kind,
known answers of Emit / Illuminate / the emitter hit, the scene host's refusals, the scene-file directives and the
Python builder, and that scenes without the two types are what they were."""
import ctypes as C
import re

import numpy as np
import pytest

import lights_lib as L
import pick_lib as pl
from smallvcm_amd._abi import LIGHT_SPHERE, LIGHT_SPOT, LIGHT_TYPE_NAMES, Light, SceneDesc
from test_thin_lens import _agree, _blocks

LT, BPM, BPT, VCM, PT = 0, 2, 3, 4, 5
SEEDS, ITERS = 24, 12   # per block: the mean of 24 independent renders of 12 iterations, SE = their scatter / sqrt(24)


def _lum(c):
    return 0.212671 * c[..., 0] + 0.715160 * c[..., 1] + 0.072169 * c[..., 2]


def _floor_estimate(d, algo, min_len=2, max_len=2, seed0=100, b=4):
    reps = []
    for k in range(SEEDS):
        e = L.EmulL(d, algo, seed=seed0 + 17 * k)
        for it in range(ITERS):
            e.run_iteration(it, min_len, max_len)
        reps.append(_blocks(e.framebuffer().astype(np.float64) / ITERS, b))
    reps = np.array(reps)
    return reps.mean(axis=0), reps.std(axis=0, ddof=1) / np.sqrt(SEEDS)


# ---------------------------------------------------------------- 1. the analytic floor under a sphere light

@pytest.fixture(scope="module")
def bulb_floor():
    d = L.floor_scene("sphere")
    clean, inside = L.bulb_pixel_masks(d)
    return d, L.floor_reference(d, "sphere"), clean, inside


@pytest.mark.parametrize("algo", [LT, PT, BPT])
def test_floor_under_a_sphere_light_is_lamberts_closed_form(bulb_floor, algo):
    """rho L (r / d)^2 cos theta at every floor point, paths of length 2 only, per 4 x 4 block within 5 combined standard
    errors; the blocks the bulb's silhouette (at 1.3 r) touches are left out -- there the camera sees the bulb itself, a
    path of length 1.  A sphere light rendered as a constant background (what type 6 did before) fails every block."""
    d, (ref, rse, _), clean, _ = bulb_floor
    assert clean.sum() >= 30, int(clean.sum())
    m, se = _floor_estimate(d, algo)
    z = np.abs(m - ref) / np.sqrt(se ** 2 + rse ** 2)
    print("sphere floor, algo %d: %d blocks, max z %.2f, mean ratio %.4f" % (algo, clean.sum(), z[clean].max(), m[clean].mean() / ref[clean].mean()))
    assert ref[clean].min() > 0
    assert z[clean].max() <= 5.0, float(z[clean].max())


@pytest.mark.parametrize("algo", [PT, BPT, VCM])
def test_pixels_that_see_only_the_bulb_show_its_radiance(bulb_floor, algo):
    """paths of length 1: a pixel whose whole footprint lies on the bulb is L, every sample"""
    d, _, _, inside = bulb_floor
    assert inside.sum() >= 4, int(inside.sum())
    e = L.EmulL(d, algo, seed=5)
    for it in range(3):
        e.run_iteration(it, 1, 1)
    fb = e.framebuffer().astype(np.float64) / 3
    want = np.array(L.BULB_L)
    assert np.all(np.abs(fb[inside] - want) <= 1e-6 * want), float(np.abs(fb[inside] / want - 1).max())


# ---------------------------------------------------------------- 2. the analytic floor under a spot light

@pytest.mark.parametrize("light", ["spot", "spot_hard"])
@pytest.mark.parametrize("algo", [LT, PT, BPT])
def test_floor_under_a_spot_light_is_the_closed_form(light, algo):
    """rho / pi I s(c) cos theta / d^2, every block; the blocks wholly outside the cone are exactly 0 for PT"""
    d = L.floor_scene(light)
    ref, rse, dark = L.floor_reference(d, light)
    m, se = _floor_estimate(d, algo, seed0=300)
    lit = ref.max(axis=2) > 0
    assert lit.sum() >= 4 and dark.sum() >= 4, (int(lit.sum()), int(dark.sum()))
    z = np.abs(m - ref) / np.sqrt(se ** 2 + rse ** 2 + 1e-300)
    print("%s floor, algo %d: max z %.2f, mean ratio %.4f" % (light, algo, z.max(), m.mean() / ref.mean()))
    assert z.max() <= 5.0, float(z.max())
    if algo == PT:
        assert np.all(m[dark] == 0.0)


# ---------------------------------------------------------------- 3. the estimators agree

def _estimate(d, algo, iters, seed0, rf=0.003, b=6, min_len=0):
    reps = []
    for k in range(4):
        r = L.EmulL(d, algo, seed=seed0 + k, radius_factor=rf)
        for it in range(iters):
            r.run_iteration(it, min_len, 10)
        reps.append(_blocks(r.framebuffer() / iters, b))
    reps = np.array(reps)
    return reps.mean(axis=0), reps.std(axis=0, ddof=1) / 2.0


@pytest.mark.parametrize("pick", [None, "power"])
def test_estimators_agree_in_the_room(pick):
    """BPT and VCM against PT per block on the closed room (a sphere light, a spot, an emissive triangle; a glass and a
    mirror sphere), all path lengths: the pdfs the MIS weights carry.  The bounds are test_light_pick.py's."""
    d = L.room(24, 24, pick=pick)
    err, info = L.check(d)
    assert err is None and info["new_lights"] == 1 and info["pick_mode"] != 0
    if pick == "power":
        assert len(set(np.round(info["pmf"], 6))) == 3, info["pmf"]
    pt = _estimate(d, PT, 64, 900)
    assert pt[0].mean() > 0.05
    _agree(_estimate(d, BPT, 40, 300), pt, ("bpt", pick))
    _agree(_estimate(d, VCM, 16, 400), pt, ("vcm", pick))


@pytest.mark.parametrize("pick", [None, "power"])
def test_light_tracing_and_bpm_agree_with_the_path_tracer(pick):
    """LT cannot render what is seen through specular objects, nor an emitter the camera sees directly, and BPM's merges
    only converge as the radius shrinks: as in test_light_pick.py both are compared with PT on the room without its two
    spheres, with paths from length 2 on both sides."""
    d = L.room(24, 24, pick=pick, specular=False)
    pt = _estimate(d, PT, 400, 510, b=3, min_len=2)
    _agree(_estimate(d, LT, 400, 10, b=3, min_len=2), pt, ("lt", pick))
    _agree(_estimate(d, BPM, 120, 210, rf=0.02, b=3, min_len=2), pt, ("bpm", pick))


# ---------------------------------------------------------------- 4. known answers

@pytest.fixture(scope="module")
def kat_room():
    d = L.room(8, 8)
    lights = L.desc2_of(d).lights
    types = [lights[i].type for i in range(3)]
    return d, types.index(LIGHT_SPHERE), types.index(LIGHT_SPOT), lights


def _ulps(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.abs(a.astype(np.float64) - b) / np.spacing(np.maximum(np.abs(a), np.abs(b)))


def test_sphere_emit_illuminate_and_hit_agree(kat_room):
    d, bulb, _, lights = kat_room
    c, r = np.array(lights[bulb].p0[:], np.float64), float(lights[bulb].e1[0])
    inv_area = np.float32(lights[bulb].invArea)
    rad = np.array(lights[bulb].intensity[:], np.float32)
    rng = np.random.default_rng(1)
    n = 4000
    u = L.uniforms(rng, (n, 4))
    out = L.kat(d, L.OP_LIGHT_EMIT, L.emit_records(bulb, u))
    pos, dirs, e_pdf, d_pdf, cos = out[:, 3:6].astype(np.float64), out[:, 6:9].astype(np.float64), out[:, 9], out[:, 10], out[:, 11]
    nrm = (pos - c) / r
    assert np.all(np.abs(np.linalg.norm(pos - c, axis=1) - r) <= 4e-7 * (1 + np.abs(c).max()))   # on the sphere
    assert np.all(np.sum(nrm * dirs, axis=1) > 0)                                                # leaving it
    assert np.all(out[:, 12] == 1) and np.all(out[:, 13] == 0)                                   # finite, not delta
    assert np.array_equal(d_pdf, np.full(n, inv_area))
    assert np.all(_ulps(e_pdf, cos * np.float32(1 / np.pi) * inv_area) <= 4)
    assert np.all(_ulps(out[:, 0:3], rad[None, :] * cos[:, None]) <= 1)
    # a receiver along the emitted ray: Illuminate with the same position sample draws the same point
    t = rng.uniform(0.3, 1.0, n)
    recv = (pos + t[:, None] * dirs).astype(np.float32)
    ill = L.kat(d, L.OP_LIGHT_ILLUMINATE, L.illuminate_records(bulb, recv, u[:, 2:4]))
    live = cos > 1e-3   # (the clamp of grazing directions, and cancellation in the cosine, aside)
    assert live.sum() > 0.9 * n
    assert np.array_equal(ill[live, 0:3], np.broadcast_to(rad, (int(live.sum()), 3)))
    to_light = ill[:, 3:6].astype(np.float64)
    assert np.all(np.abs(to_light[live] + dirs[live]) <= 2e-6 / t[live, None])
    dist, dpw, epw, cal = ill[:, 6].astype(np.float64), ill[:, 7], ill[:, 8], ill[:, 9]
    assert np.all(np.abs(dist[live] - t[live]) <= 1e-6)
    assert np.all(np.abs(cal[live] - cos[live]) <= 4e-6 / t[live])
    assert np.all(_ulps(dpw[live], (inv_area * (ill[live, 6] * ill[live, 6]).astype(np.float32)) / cal[live]) <= 4)   # invArea d^2 / cos
    assert np.all(_ulps(epw[live], inv_area * cal[live] * np.float32(1 / np.pi)) <= 4)
    # the emitter hit from that receiver, with the sphere's normal at the point
    hit = L.kat(d, L.OP_LIGHT_RADIANCE_AT, L.radiance_at_records(bulb, ill[:, 3:6], nrm.astype(np.float32)))
    assert np.array_equal(hit[live, 0:3], ill[live, 0:3])
    assert np.array_equal(hit[live, 3], np.full(int(live.sum()), inv_area))
    assert np.all(np.abs(hit[live, 4] / epw[live] - 1) <= 2e-6 / cal[live])   # the same emissionPdfW (the cosine's rounding)
    # the back of the sphere, both ways
    back = L.kat(d, L.OP_LIGHT_RADIANCE_AT, L.radiance_at_records(bulb, ill[:, 3:6], -nrm.astype(np.float32)))
    assert not np.any(back[live, 0:5])
    far = L.kat(d, L.OP_LIGHT_ILLUMINATE, L.illuminate_records(bulb, np.tile(np.float32([3, 3, 3]), (n, 1)), u[:, 0:2]))
    dead = np.all(far[:, 0:3] == 0, axis=1)
    assert 0.45 < dead.mean() < 0.65, float(dead.mean())   # about 55 % of a receiver's samples land on the far side
    # the op without a normal answers a sphere light with zero, as it answers a point light
    assert not np.any(L.kat(d, L.OP_LIGHT_RADIANCE, L.radiance_at_records(bulb, ill[:, 3:6], nrm.astype(np.float32)))[:, 0:5])


def test_spot_emit_and_illuminate_agree(kat_room):
    d, _, spot, lights = kat_room
    l = lights[spot]
    p, axis = np.array(l.p0[:], np.float64), np.array(l.frameZ[:], np.float64)
    cos_outer, cos_inner, pdf = float(l.e1[0]), float(l.e1[1]), np.float32(l.scale)
    assert abs(pdf - 1 / (2 * np.pi * (1 - cos_outer))) <= 1e-7 * pdf
    rng = np.random.default_rng(2)
    n = 4000
    u = L.uniforms(rng, (n, 4))
    out = L.kat(d, L.OP_LIGHT_EMIT, L.emit_records(spot, u))
    dirs = out[:, 6:9].astype(np.float64)
    c = dirs @ axis
    assert np.array_equal(out[:, 3:6], np.broadcast_to(np.float32(l.p0[:]), (n, 3)))
    assert np.all(c >= cos_outer - 1e-6) and np.all(np.abs(np.linalg.norm(dirs, axis=1) - 1) <= 1e-6)
    assert np.all(np.abs(c - (1 - u[:, 0].astype(np.float64) * (1 - cos_outer))) <= 1e-6)   # uniform in the cone
    assert np.array_equal(out[:, 9], np.full(n, pdf)) and np.all(out[:, 10] == 1) and np.all(out[:, 11] == 1)
    assert np.all(out[:, 12] == 1) and np.all(out[:, 13] == 1)   # finite, delta
    s = L.smoothstep_falloff(c, cos_outer, cos_inner)
    want = s[:, None] * np.array(l.intensity[:], np.float64)
    # the falloff's slope is at most 1.5 / (cosInner - cosOuter) per unit of cosine
    tol = 1.5 / (cos_inner - cos_outer) * 2e-6 * np.array(l.intensity[:]).max() + 1e-6
    assert np.all(np.abs(out[:, 0:3] - want) <= tol)
    recv = (p + rng.uniform(0.3, 2.0, n)[:, None] * dirs).astype(np.float32)
    ill = L.kat(d, L.OP_LIGHT_ILLUMINATE, L.illuminate_records(spot, recv, u[:, 0:2]))
    live = np.all(ill[:, 0:3] > 0, axis=1)
    assert live.sum() > 0.8 * n
    assert np.all(np.abs(ill[:, 0:3] - out[:, 0:3]) <= 2 * tol)              # the same radiance both ways
    assert np.array_equal(ill[live, 8], np.full(int(live.sum()), pdf))       # emissionPdfW = the cone's pdf
    assert np.array_equal(ill[live, 7], (ill[live, 6].astype(np.float64) ** 2).astype(np.float32)) or \
        np.all(_ulps(ill[live, 7], ill[live, 6] * ill[live, 6]) <= 2)       # directPdfW = dist^2
    assert np.all(ill[live, 9] == 1)
    # outside the cone: nothing, from either function of a hit
    behind = (p - 0.5 * axis + 0.01 * rng.standard_normal((n, 3))).astype(np.float32)
    assert not np.any(L.kat(d, L.OP_LIGHT_ILLUMINATE, L.illuminate_records(spot, behind, u[:, 0:2]))[:, 0:3])
    hit = L.kat(d, L.OP_LIGHT_RADIANCE_AT, L.radiance_at_records(spot, -dirs.astype(np.float32), dirs.astype(np.float32)))
    assert not np.any(hit[:, 0:5])   # never hit


def test_a_hard_edge_is_one_inside_the_cone():
    d = L.floor_scene("spot_hard", res=8)
    l = L.desc2_of(d).lights[0]
    assert l.e1[0] == l.e1[1] and l.e1[2] == 0.0
    u = L.uniforms(np.random.default_rng(3), (2000, 4))
    out = L.kat(d, L.OP_LIGHT_EMIT, L.emit_records(0, u))
    assert np.array_equal(out[:, 0:3], np.broadcast_to(np.float32(l.intensity[:]), (2000, 3)))


@pytest.mark.parametrize("which", ["sphere", "spot", "spot_hard"])
def test_power_weight_is_the_flux_emit_integrates_to(which):
    """the mean of lum(Emit) / emissionPdfW over 10^6 draws against scene_host_light_power, within 5 standard errors"""
    d = L.floor_scene(which, res=8)
    err, info = L.check(d)
    assert err is None
    n = 1000000
    u = L.uniforms(np.random.default_rng(4), (n, 4))
    out = L.kat(d, L.OP_LIGHT_EMIT, L.emit_records(0, u))
    x = _lum(out[:, 0:3].astype(np.float64)) / out[:, 9]
    mean, se = x.mean(), x.std(ddof=1) / np.sqrt(n)
    w = info["power"][0]
    print("%s: power %.6f, Emit estimates %.6f +- %.6f" % (which, w, mean, se))
    assert w > 0
    # (a hard edge and a sphere are constant estimators up to rounding: their standard error is of the order of 1e-7 w)
    assert abs(mean - w) <= 5 * se + 2e-6 * w, (mean, w, se)
    l = L.desc2_of(d).lights[0]
    lum = float(_lum(np.array(l.intensity[:], np.float64)))
    if which == "sphere":
        assert abs(w - np.pi * lum * 4 * np.pi * L.BULB_RADIUS ** 2) <= 1e-6 * w
    else:
        co, ci = float(l.e1[0]), float(l.e1[1])
        assert w == 2 * np.pi * lum * ((1 - ci) + (ci - co) / 2)


# ---------------------------------------------------------------- 5. input checks, scene files and Python

def _with_lights(d, edit):
    """a copy of the description whose lights (and optionally prims / mat2light / backgroundLight) `edit` has changed"""
    from smallvcm_amd._abi import Prim, SceneDesc2
    b = L.desc2_of(d)
    lights = (Light * b.nLights)(*b.lights[:b.nLights])
    prims = (Prim * b.nPrims)(*b.prims[:b.nPrims])
    m2l = (C.c_int * b.nMaterials)(*b.mat2light[:b.nMaterials])
    out = SceneDesc2.from_buffer_copy(b)
    out.lights, out.prims, out.mat2light = C.cast(lights, C.POINTER(Light)), C.cast(prims, C.POINTER(Prim)), C.cast(m2l, C.POINTER(C.c_int))
    out._keep = (d, lights, prims, m2l)
    edit(out, lights, prims, m2l)
    return out


def _set(field, k, v):
    def edit(d, lights, prims, m2l):
        getattr(lights[0], field)[k] = v
    return edit


REFUSALS = [
    ("spot", _set("p0", 1, float("nan")), "spot light: position and intensity must be finite"),
    ("spot", _set("intensity", 2, float("inf")), "spot light: position and intensity must be finite"),
    ("spot", _set("frameZ", 0, float("nan")), "spot light: direction and angles must be finite"),
    ("spot", _set("e1", 0, 1.0), "spot light: the outer half-angle must be > 0 and <= 180 degrees"),
    ("spot", _set("e1", 0, -1.5), "spot light: the outer half-angle must be > 0 and <= 180 degrees"),
    ("spot", _set("e1", 1, 0.5), "spot light: the inner half-angle must be >= 0 and <= the outer one"),
    ("spot", _set("e1", 1, 1.5), "spot light: the inner half-angle must be >= 0 and <= the outer one"),
    ("spot", lambda d, l, p, m: setattr(l[0], "scale", float("inf")), "spot light: the cone pdf must be finite and > 0"),
    ("spot", lambda d, l, p, m: setattr(d, "backgroundLight", 0), "a spot light cannot be the backgroundLight"),
    ("sphere", _set("e1", 0, 0.0), "sphere light: radius must be finite and > 0"),
    ("sphere", _set("e1", 0, float("inf")), "sphere light: radius must be finite and > 0"),
    ("sphere", _set("p0", 0, float("nan")), "sphere light: centre and intensity must be finite"),
    ("sphere", lambda d, l, p, m: setattr(d, "backgroundLight", 0), "a sphere light cannot be the backgroundLight"),
    ("sphere", lambda d, l, p, m: m.__setitem__(1, -1), "sphere light: exactly one primitive must carry a material mapped to it"),
    ("sphere", lambda d, l, p, m: m.__setitem__(0, 0), "sphere light: exactly one primitive must carry a material mapped to it"),
    ("sphere", lambda d, l, p, m: p[2].p1.__setitem__(0, 0.3), "sphere light: its primitive must be a VCM_PRIM_SPHERE of the same centre and radius"),
    ("sphere", lambda d, l, p, m: p[2].p0.__setitem__(2, 1.0), "sphere light: its primitive must be a VCM_PRIM_SPHERE of the same centre and radius"),
    ("sphere", lambda d, l, p, m: setattr(p[2], "type", 0), "sphere light: its primitive must be a VCM_PRIM_SPHERE of the same centre and radius"),
]


@pytest.mark.parametrize("which,edit,message", REFUSALS)
def test_scene_host_refuses(which, edit, message):
    d = L.floor_scene(which, res=8)
    assert L.check(d)[0] is None
    err, _ = L.check(_with_lights(d, edit))
    assert err == message


def test_version_1_descriptions_are_checked_too():
    """vcm_scene_desc (fixed capacities) takes the same lights and the same refusals"""
    from smallvcm_amd.renderer import cornell_scene
    E = L.emul_lights()
    d1 = cornell_scene(1, 8, 8)
    info = (C.c_int * 3)()
    assert E.emul_lights_check1(C.byref(d1), info) == 0 and info[0] == 0 and info[1] == 0   # no table, as before
    src = L.desc2_of(L.floor_scene("spot", res=8)).lights[0]
    d1.lights[d1.nLights] = src
    d1.nLights += 1
    assert E.emul_lights_check1(C.byref(d1), info) == 0 and info[0] == 1 and info[1] != 0   # now through the table
    d1.lights[d1.nLights - 1].e1[0] = 2.0
    assert E.emul_lights_check1(C.byref(d1), info) == -1
    assert E.emul_lights_error().decode() == "spot light: the outer half-angle must be > 0 and <= 180 degrees"


def test_python_builder_checks_its_arguments():
    from smallvcm_amd.scene2 import SceneBuilder
    b = SceneBuilder()
    for bad in [(0.0, None), (181.0, None), (float("nan"), None), (40.0, 41.0), (40.0, -1.0)]:
        with pytest.raises(ValueError):
            b.spot_light((0, 0, 1), (0, 0, -1), (1, 1, 1), *bad)
    for bad in [0.0, -1.0, float("inf")]:
        with pytest.raises(ValueError):
            b.sphere_light((0, 0, 1), bad, (1, 1, 1))
    assert LIGHT_TYPE_NAMES[LIGHT_SPOT] == "spot" and LIGHT_TYPE_NAMES[LIGHT_SPHERE] == "sphere"


def _fields(s):
    return {name: (list(getattr(s, name)[:]) if hasattr(getattr(s, name), "__len__") else getattr(s, name)) for name, _ in s._fields_}


def test_scene_file_directives_equal_the_builder(tmp_path):
    from smallvcm_amd.scene2 import SceneBuilder
    from smallvcm_amd.scene_file import load_scene
    (tmp_path / "f.obj").write_text("mtllib f.mtl\nv -5 -5 0\nv 5 -5 0\nv 5 5 0\nv -5 5 0\nusemtl floor\nf 1 2 3\nf 3 4 1\n")
    (tmp_path / "f.mtl").write_text("newmtl floor\nKd 0.6 0.6 0.6\n")
    (tmp_path / "s.vcmscene").write_text(
        "obj f.obj\ncamera 0 -2.5 4  0 2.5 -4  0 0 1  45\n"
        "light spot 0.6 0.4 2  -0.6 -0.4 -2  7 6 5  40 25   # a lamp\n"
        "light sphere 0.6 0.4 1.6 0.25  9 8 6\n"
        "light spot -1 0 2  0 0 -1  1 1 1  30 30\n")
    got = L.desc2_of(load_scene(tmp_path / "s.vcmscene", 16, 12))
    b = SceneBuilder()
    m = b.material(diffuse=(0.6, 0.6, 0.6))
    b.triangle((-5, -5, 0), (5, -5, 0), (5, 5, 0), m)
    b.triangle((5, 5, 0), (-5, 5, 0), (-5, -5, 0), m)
    b.spot_light((0.6, 0.4, 2), (-0.6, -0.4, -2), (7, 6, 5), 40, 25)
    b.sphere_light((0.6, 0.4, 1.6), 0.25, (9, 8, 6))
    b.spot_light((-1, 0, 2), (0, 0, -1), (1, 1, 1), 30)
    want = L.desc2_of(b.build((0, -2.5, 4), (0, 2.5, -4), (0, 0, 1), 45, 16, 12))
    assert (got.nPrims, got.nMaterials, got.nLights, got.backgroundLight) == (want.nPrims, want.nMaterials, want.nLights, want.backgroundLight) == (3, 2, 3, -1)
    for k in range(3):
        assert _fields(got.lights[k]) == _fields(want.lights[k]), k
        assert _fields(got.prims[k]) == _fields(want.prims[k]), k
    for k in range(2):
        assert _fields(got.materials[k]) == _fields(want.materials[k]) and got.mat2light[k] == want.mat2light[k]
    assert [got.lights[k].type for k in range(3)] == [LIGHT_SPOT, LIGHT_SPHERE, LIGHT_SPOT]
    assert _fields(got.camera) == _fields(want.camera) and got.sceneRadius == want.sceneRadius
    assert L.check(load_scene(tmp_path / "s.vcmscene", 16, 12))[0] is None


@pytest.mark.parametrize("line,text", [
    ("light spot 0 0 2  0 0 -1  1 1 1  40", "light spot px py pz dx dy dz r g b outerDeg innerDeg"),
    ("light spot 0 0 2  0 0 -1  1 1 1  0 0", "light spot outerDeg must be finite, > 0 and <= 180"),
    ("light spot 0 0 2  0 0 -1  1 1 1  40 50", "light spot innerDeg must be finite, >= 0 and <= outerDeg"),
    ("light sphere 0 0 2  1 1 1", "light sphere cx cy cz radius r g b"),
    ("light sphere 0 0 2 -1  1 1 1", "light sphere radius must be finite and > 0"),
    ("light bulb 0 0 2", "light spot px py pz dx dy dz r g b outerDeg innerDeg, light sphere cx cy cz radius r g b"),
])
def test_a_malformed_directive_names_its_line(tmp_path, line, text):
    from smallvcm_amd.scene_file import load_scene
    (tmp_path / "f.obj").write_text("mtllib f.mtl\nv -5 -5 0\nv 5 -5 0\nv 5 5 0\nusemtl floor\nf 1 2 3\n")
    (tmp_path / "f.mtl").write_text("newmtl floor\nKd 0.6 0.6 0.6\n")
    (tmp_path / "s.vcmscene").write_text("obj f.obj\n# a comment\n%s\n" % line)
    with pytest.raises(Exception) as e:
        load_scene(tmp_path / "s.vcmscene", 8, 8)
    assert "s.vcmscene line 3" in str(e.value) and text in str(e.value), str(e.value)


# ---------------------------------------------------------------- 6. nothing else moved

def test_scenes_without_the_new_types_have_no_table_of_their_own():
    """a scene without a spot or sphere light keeps the uniform choice without a table (the kernels it launched before);
    with one it always has a table -- equal quanta where the caller asked for the uniform choice"""
    for d in (pl.lamp_room(8, 8, n_dim=3), pl.box_many_lights(3, 8, 8)):
        err, info = L.check(d)
        assert err is None and info["new_lights"] == 0 and info["pick_mode"] == 0
    err, info = L.check(pl.with_pick(pl.lamp_room(8, 8, n_dim=3), pl.POWER))
    assert err is None and info["new_lights"] == 0 and info["pick_mode"] == pl.POWER
    for pick in (None, "uniform"):
        err, info = L.check(L.room(8, 8, pick=pick))
        assert err is None and info["new_lights"] == 1 and info["pick_mode"] == pl.CUSTOM
        q = np.round(info["pmf"].astype(np.float64) * pl.Q).astype(np.int64)
        assert q.sum() == pl.Q and q.max() - q.min() <= 1, q
    err, info = L.check(L.room(8, 8, pick="power"))
    assert info["pick_mode"] == pl.POWER


def test_wrapper_rule_is_stated_in_scene_kind_h():
    """the kinds with the new branches exist over the table kinds alone (csrc/scene_kind.h holds the static_asserts)"""
    import os
    src = open(os.path.join(os.path.dirname(L.HERE), "smallvcm_amd", "csrc", "scene_kind.h")).read()
    assert re.search(r"WithLights<WithPick<S>>", src) and "wrappers_valid" in src
    assert not re.search(r"WithLights<(?!WithPick)", src.replace("template <class S> struct WithLights", ""))
