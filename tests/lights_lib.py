"""Spot- and sphere-light scenes for the tests (test infrastructure): the analytic floors, the closed room with one light
of each finite kind, the numpy references of both floors, and the ctypes binding of
tests/host_emul_lights/libemul_lights.so."""
import ctypes as C
import os
import subprocess

import numpy as np

import filter_lib as fl
import lens_lib as ll
import pick_lib as pl
from smallvcm_amd._abi import SceneDesc, SceneDesc6

HERE = os.path.dirname(os.path.abspath(__file__))
EMUL_DIR = os.path.join(HERE, "host_emul_lights")
OP_LIGHT_EMIT, OP_LIGHT_ILLUMINATE, OP_LIGHT_RADIANCE, OP_LIGHT_RADIANCE_AT = 4, 5, 6, 11   # VCM_KAT_*
KAT = 16
LIGHT_SPOT, LIGHT_SPHERE = 5, 6
_fp = C.POINTER(C.c_float)
_E = None

# ---- the analytic floors (the issue's scene): a diffuse floor z = 0, |x|, |y| <= 5, one light above it
RHO = 0.6
FLOOR_CAMERA = ((0.0, -2.5, 4.0), (0.0, 2.5, -4.0), (0.0, 0.0, 1.0), 45.0)
BULB_CENTRE, BULB_RADIUS, BULB_L = (0.6, 0.4, 1.6), 0.25, (9.0, 8.0, 6.0)
SPOT_POS, SPOT_I, SPOT_OUTER, SPOT_INNER = (0.6, 0.4, 2.0), (7.0, 6.0, 5.0), 40.0, 25.0


def as_desc6(d):
    return d if isinstance(d, SceneDesc6) else fl.with_filter(d, None)


def floor_scene(light, res=24):
    """light: "sphere", "spot" (outer 40, inner 25 degrees) or "spot_hard" (inner = outer)"""
    from smallvcm_amd.scene2 import SceneBuilder
    b = SceneBuilder()
    m = b.material(diffuse=(RHO, RHO, RHO))
    b.triangle((-5, -5, 0), (5, -5, 0), (5, 5, 0), m)
    b.triangle((5, 5, 0), (-5, 5, 0), (-5, -5, 0), m)
    if light == "sphere":
        b.sphere_light(BULB_CENTRE, BULB_RADIUS, BULB_L)
    else:
        aim = tuple(-x for x in SPOT_POS)
        b.spot_light(SPOT_POS, aim, SPOT_I, SPOT_OUTER, SPOT_OUTER if light == "spot_hard" else SPOT_INNER)
    pos, fwd, up, fov = FLOOR_CAMERA
    return as_desc6(b.build(pos, fwd, up, fov, res, res))


def room(resx=20, resy=14, pick=None, mix=0.0, lens=None, sky=None, flt=None, fan=False, specular=True):
    """A closed box with one sphere light, one spot and one emissive triangle -- three lights with three different pmf
    under POWER -- a glass sphere and a mirror sphere.  fan: the same room with the bulb replaced by an emissive-triangle
    octahedron of equal area and the spot by a point light (what a scene had to use before; for measurements).
    specular=False: without the two spheres (what light tracing and BPM can be compared on)."""
    from smallvcm_amd.scene2 import SceneBuilder
    b = SceneBuilder()
    white = b.material(diffuse=(0.803922, 0.803922, 0.803922))
    green = b.material(diffuse=(0.156863, 0.803922, 0.172549))
    red = b.material(diffuse=(0.803922, 0.152941, 0.152941))
    lo, hi = -1.25, 1.25
    c = [(lo, hi, lo), (hi, hi, lo), (hi, hi, hi), (lo, hi, hi), (lo, lo, lo), (hi, lo, lo), (hi, lo, hi), (lo, lo, hi)]
    b.triangle(c[0], c[4], c[5], white); b.triangle(c[5], c[1], c[0], white)       # floor
    b.triangle(c[0], c[1], c[2], white); b.triangle(c[2], c[3], c[0], white)       # back wall
    b.triangle(c[3], c[7], c[4], green); b.triangle(c[4], c[0], c[3], green)       # left
    b.triangle(c[1], c[5], c[6], red); b.triangle(c[6], c[2], c[1], red)           # right
    b.triangle(c[2], c[6], c[7], white); b.triangle(c[7], c[3], c[2], white)       # ceiling
    if sky is None:   # closed: the wall behind the camera (facing +y)
        far = -4.5
        f = [(lo, far, lo), (hi, far, lo), (hi, far, hi), (lo, far, hi)]
        b.triangle(f[0], f[2], f[1], white); b.triangle(f[2], f[0], f[3], white)
    if specular:
        b.sphere((-0.55, 0.3, -0.85), 0.4, b.material(mirror=(1, 1, 1)))
        b.sphere((0.55, -0.2, -0.9), 0.35, b.material(mirror=(1, 1, 1), ior=1.6))
    bulb_c, bulb_r, bulb_l = (0.1, 0.1, 0.55), 0.18, (12.0, 11.0, 9.0)
    spot_p, spot_i = (-0.8, -0.6, 1.0), (3.0, 3.0, 4.0)
    if fan:
        s = bulb_r * np.sqrt(4 * np.pi / (4 * np.sqrt(3.0)))   # an octahedron |x| + |y| + |z| = s has the area 4 sqrt(3) s^2
        v = [np.array(bulb_c) + s * np.array(a) for a in [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]]
        for sx in (0, 1):
            for sy in (2, 3):
                for sz in (4, 5):
                    p, q, r = v[sx], v[sy], v[sz]
                    n = np.cross(q - p, r - p)
                    if np.dot(n, (p + q + r) / 3 - np.array(bulb_c)) < 0:
                        q, r = r, q
                    b.emissive_triangle(tuple(p), tuple(q), tuple(r), bulb_l)
        b.point_light(spot_p, spot_i)
    else:
        b.sphere_light(bulb_c, bulb_r, bulb_l)
        b.spot_light(spot_p, (0.9, 0.8, -1.6), spot_i, 50.0, 30.0)
    b.emissive_triangle((-0.3, 0.6, 1.2), (0.3, 0.9, 1.2), (0.3, 0.6, 1.2), (20.0, 20.0, 20.0))   # normal -z
    if sky is not None:
        b.envmap_light(sky, 0.3)
    if lens is not None:
        b.thin_lens(*lens)
    if pick is not None:
        b.light_pick(pick, mix)
    if flt is not None:
        b.pixel_filter(*flt)
    return as_desc6(b.build((-0.0439815, -4.12529, 0.222539), (0.00688625, 0.998505, -0.0542161),
                            (3.73896e-4, 0.0542148, 0.998529), 45.0, resx, resy))


def many_lights_room(n_extra=260, resx=20, resy=14):
    """the room's two new lights among n_extra dim point lights: more lights than the pick table's LDS room (256)"""
    from smallvcm_amd.scene2 import SceneBuilder
    rng = np.random.default_rng(5)
    b = SceneBuilder()
    white = b.material(diffuse=(0.8, 0.8, 0.8))
    b.triangle((-2, -2, 0), (2, -2, 0), (2, 2, 0), white); b.triangle((2, 2, 0), (-2, 2, 0), (-2, -2, 0), white)
    b.triangle((-2, 2, 0), (2, 2, 0), (2, 2, 3), white); b.triangle((2, 2, 3), (-2, 2, 3), (-2, 2, 0), white)
    for k in range(n_extra):
        if k == n_extra // 3:
            b.sphere_light((0.3, 0.2, 0.9), 0.2, (6.0, 5.0, 4.0))
        if k == 2 * n_extra // 3:
            b.spot_light((-0.9, -0.5, 1.6), (0.5, 0.6, -1.0), (2.0, 2.5, 3.0), 45.0, 20.0)
        i = float(10.0 ** rng.uniform(-3, -1))
        b.point_light((rng.uniform(-1.5, 1.5), rng.uniform(-1.5, 1.5), rng.uniform(0.3, 2.5)), (i, i, 0.5 * i))
    b.light_pick("power", 0.05)
    return as_desc6(b.build((0, -4.5, 1.6), (0, 1, -0.2), (0, 0, 1), 45.0, resx, resy))


# ---- the numpy side of the analytic floors
def camera_rays(d, raster):
    """origin [3] and directions [n, 3] of the pinhole rays through raster points [n, 2] (camera.hxx:108-117 in float64)"""
    cam = d.camera
    m = np.array(cam.rasterToWorld[:], np.float64).reshape(4, 4).T   # column-major storage
    p = np.concatenate([raster, np.zeros((len(raster), 1)), np.ones((len(raster), 1))], axis=1) @ m.T
    world = p[:, :3] / p[:, 3:4]
    org = np.array(cam.position[:], np.float64)
    dirs = world - org
    return org, dirs / np.linalg.norm(dirs, axis=1, keepdims=True)


def smoothstep_falloff(c, cos_outer, cos_inner):
    if cos_inner <= cos_outer:
        return (c >= cos_outer).astype(np.float64)
    t = np.clip((c - cos_outer) / (cos_inner - cos_outer), 0.0, 1.0)
    return np.where(c < cos_outer, 0.0, t * t * (3 - 2 * t))


def floor_radiance(light, pts):
    """the closed forms: radiance [n, 3] leaving the floor points pts [n, 3] (z = 0) towards anywhere"""
    if light == "sphere":   # Lambert: rho L (r / d)^2 cos theta, the whole sphere above the horizon
        v = np.array(BULB_CENTRE) - pts
        d = np.linalg.norm(v, axis=1)
        return (RHO * (BULB_RADIUS / d) ** 2 * (v[:, 2] / d))[:, None] * np.array(BULB_L)
    v = np.array(SPOT_POS) - pts
    d = np.linalg.norm(v, axis=1)
    axis = -np.array(SPOT_POS) / np.linalg.norm(SPOT_POS)
    c = (-v / d[:, None]) @ axis
    co = np.cos(np.radians(SPOT_OUTER))
    ci = co if light == "spot_hard" else np.cos(np.radians(SPOT_INNER))
    return (RHO / np.pi * smoothstep_falloff(c, co, ci) * (v[:, 2] / d) / d ** 2)[:, None] * np.array(SPOT_I)


def floor_reference(d, light, res=24, b=4, n=40000, seed=1):
    """per b x b block: mean [B, B, 3] and standard error of the closed form over the block's footprint (Monte Carlo
    over raster points), and whether every sample of the block lies outside the spot's cone (all zero)"""
    rng = np.random.default_rng(seed)
    B = res // b
    mean, se, dark = np.zeros((B, B, 3)), np.zeros((B, B, 3)), np.zeros((B, B), bool)
    for by in range(B):
        for bx in range(B):
            raster = np.array([bx * b, by * b]) + b * rng.random((n, 2))
            org, dirs = camera_rays(d, raster)
            t = -org[2] / dirs[:, 2]
            v = floor_radiance(light, org + t[:, None] * dirs)
            mean[by, bx], se[by, bx] = v.mean(axis=0), v.std(axis=0, ddof=1) / np.sqrt(n)
            dark[by, bx] = not np.any(v)
    return mean, se, dark


def bulb_pixel_masks(d, res=24, b=4):
    """(blocks [B, B] that the bulb's silhouette, taken at 1.3 r, does not touch; pixels [res, res] whose whole footprint
    sees the bulb) -- by a dense grid of rays per pixel, its corners included"""
    k = 9
    g = np.linspace(0.0, 1.0, k)
    yy, xx, v, u = np.meshgrid(np.arange(res), np.arange(res), g, g, indexing="ij")
    raster = np.stack([(xx + u).ravel(), (yy + v).ravel()], axis=1)
    org, dirs = camera_rays(d, raster)
    oc = np.array(BULB_CENTRE) - org
    tca = dirs @ oc
    dist2 = oc @ oc - tca ** 2   # squared distance of the ray from the centre
    near = (dist2 <= (1.3 * BULB_RADIUS) ** 2).reshape(res, res, k * k)
    inside = (dist2 <= (0.999 * BULB_RADIUS) ** 2).reshape(res, res, k * k)
    touched = near.any(axis=2).reshape(res // b, b, res // b, b).any(axis=(1, 3))
    return ~touched, inside.all(axis=2)


# ---- the host emulation
def emul_lights():
    """build (make: a no-op when up to date) and load the lights host emulation"""
    global _E
    if _E is None:
        subprocess.run(["make", "-C", EMUL_DIR], check=True, stdout=subprocess.DEVNULL)
        E = C.CDLL(os.path.join(EMUL_DIR, "libemul_lights.so"))
        P6 = C.POINTER(SceneDesc6)
        E.emul_lights_create.restype = C.c_void_p
        E.emul_lights_create.argtypes = [P6, C.c_int, C.c_float, C.c_float, C.c_int, C.c_int, C.c_int]
        E.emul_destroy.argtypes = [C.c_void_p]
        E.emul_run_iteration.argtypes = [C.c_void_p, C.c_int, C.c_uint, C.c_uint]
        E.emul_get_framebuffer.argtypes = [C.c_void_p, _fp]
        E.emul_get_counts.argtypes = [C.c_void_p, C.POINTER(C.c_ubyte), C.POINTER(C.c_ubyte)]
        E.emul_get_stats.argtypes = [C.c_void_p, C.POINTER(C.c_longlong)]
        E.emul_lights_kat.argtypes = [P6, C.c_int, C.c_int, _fp, _fp]
        E.emul_lights_check.argtypes = [P6, C.POINTER(C.c_int), _fp, C.POINTER(C.c_double)]
        E.emul_lights_check1.argtypes = [C.POINTER(SceneDesc), C.POINTER(C.c_int)]
        E.emul_lights_error.restype = C.c_char_p
        _E = E
    return _E


class EmulL(ll.Emul4):
    """one emulated renderer over any description (rank / world: a shard of it)"""

    def __init__(self, scene, algo, seed=1234, rank=0, world=1, radius_factor=0.003, radius_alpha=0.75):
        self.E = emul_lights()
        scene = as_desc6(scene)
        self.scene = scene
        self.h = self.E.emul_lights_create(C.byref(scene), algo, radius_factor, radius_alpha, seed, rank, world)
        assert self.h, self.E.emul_lights_error().decode()
        self.resx, self.resy = int(scene.camera.resolution[0]), int(scene.camera.resolution[1])
        self.N = self.resx * self.resy
        self.rank, self.world = rank, world


def kat(scene, op, inp):
    scene = as_desc6(scene)
    inp = np.ascontiguousarray(inp, np.float32)
    out = np.zeros_like(inp)
    E = emul_lights()
    assert E.emul_lights_kat(C.byref(scene), op, len(inp), inp.ctypes.data_as(_fp), out.ctypes.data_as(_fp)) == 0, \
        E.emul_lights_error().decode()
    return out


def check(scene):
    """what the scene host says: (None, info dict) when it accepts the description, (message, None) when it refuses"""
    scene = as_desc6(scene)
    n = pl.n_lights(scene)
    info = (C.c_int * 3)()
    pmf, power = np.zeros(max(n, 1), np.float32), np.zeros(max(n, 1), np.float64)
    E = emul_lights()
    if E.emul_lights_check(C.byref(scene), info, pmf.ctypes.data_as(_fp), power.ctypes.data_as(C.POINTER(C.c_double))) != 0:
        return E.emul_lights_error().decode(), None
    return None, {"new_lights": info[0], "pick_mode": info[1], "n": info[2], "pmf": pmf[:n], "power": power[:n]}


def desc2_of(d):
    while hasattr(d, "base"):
        d = d.base
    return d


def uniforms(rng, shape):
    """floats of the generator's form (2j + 1) 2^-24, j < 2^23: in (0, 1), as the device draws them"""
    j = rng.integers(0, 1 << 23, size=shape, dtype=np.int64)
    return ((2 * j + 1).astype(np.float64) * 2.0 ** -24).astype(np.float32)


def emit_records(light, u4):
    inp = np.zeros((len(u4), KAT), np.float32)
    inp[:, 0] = light
    inp[:, 1:5] = u4   # dirRnd2, posRnd2
    return inp


def illuminate_records(light, recv, u2):
    inp = np.zeros((len(recv), KAT), np.float32)
    inp[:, 0] = light
    inp[:, 1:4] = recv
    inp[:, 4:6] = u2
    return inp


def radiance_at_records(light, ray_dir, normal):
    inp = np.zeros((len(ray_dir), KAT), np.float32)
    inp[:, 0] = light
    inp[:, 1:4] = ray_dir
    inp[:, 4:7] = normal
    return inp
