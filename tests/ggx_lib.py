"""GGX materials for the tests (test infrastructure): scenes with the lobe, the ctypes binding of
tests/host_emul_ggx/libemul_ggx.so, the known-answer records, and a binary64 numpy restatement of the lobe written from
its definition (DESIGN.md "Microfacet materials"), not from csrc/vcm_core.h."""
import ctypes as C
import os
import subprocess

import numpy as np

import lens_lib as ll
from smallvcm_amd._abi import SceneDesc7, SceneDesc8, with_material_ext, with_sampler

HERE = os.path.dirname(os.path.abspath(__file__))
EMUL_DIR = os.path.join(HERE, "host_emul_ggx")
OP_BSDF_EVAL, OP_BSDF_SAMPLE = 2, 3   # VCM_KAT_*
KAT = 16
EPS_COSINE, EPS_PHONG = 1e-6, 1e-3
K_DIFFUSE, K_PHONG, K_REFLECT, K_REFRACT, K_GGX = 1, 2, 4, 8, 16
_fp = C.POINTER(C.c_float)
_E = None

# the materials of the known-answer scene: (diffuse, phong, exponent, mirror, ior, F0, alpha).  Pure lobes over the whole
# range of alpha, mixed ones with every other component, and one material without the lobe.
KAT_MATERIALS = [
    ((0, 0, 0), (0, 0, 0), 1.0, (0, 0, 0), -1.0, (1.0, 1.0, 1.0), 0.01),
    ((0, 0, 0), (0, 0, 0), 1.0, (0, 0, 0), -1.0, (0.9, 0.6, 0.3), 0.05),
    ((0, 0, 0), (0, 0, 0), 1.0, (0, 0, 0), -1.0, (0.04, 0.04, 0.04), 0.3),
    ((0, 0, 0), (0, 0, 0), 1.0, (0, 0, 0), -1.0, (1.0, 0.8, 0.5), 1.0),
    ((0.5, 0.3, 0.2), (0, 0, 0), 1.0, (0, 0, 0), -1.0, (0.04, 0.04, 0.04), 0.2),
    ((0.2, 0.3, 0.1), (0.3, 0.2, 0.3), 30.0, (0, 0, 0), -1.0, (0.2, 0.3, 0.25), 0.6),
    ((0.1, 0.1, 0.1), (0.1, 0.1, 0.1), 90.0, (0.3, 0.3, 0.3), -1.0, (0.3, 0.3, 0.3), 0.1),
    ((0.1, 0.1, 0.2), (0, 0, 0), 1.0, (0.2, 0.2, 0.2), 1.5, (0.5, 0.4, 0.3), 0.4),
    ((0.4, 0.4, 0.4), (0.2, 0.2, 0.2), 10.0, (0, 0, 0), -1.0, (0, 0, 0), 1.0),
]


def as_desc8(d, ext=None):
    return d if isinstance(d, SceneDesc8) else with_material_ext(d, ext)


def desc2_of(d):
    while hasattr(d, "base"):
        d = d.base
    return d


def kat_scene(res=8):
    """one floor of every material of KAT_MATERIALS under a point light: the ops look at the materials alone"""
    from smallvcm_amd.scene2 import SceneBuilder
    b = SceneBuilder()
    for k, (kd, ks, n, km, ior, f0, a) in enumerate(KAT_MATERIALS):
        m = b.material(diffuse=kd, phong=ks, exponent=n, mirror=km, ior=ior, ggx=f0, alpha=a)
        b.triangle((k, 0, 0), (k + 1, 0, 0), (k + 1, 1, 0), m)
    b.point_light((0, 0, 3), (1, 1, 1))
    return b.build((4, -6, 3), (0, 1, -0.4), (0, 0, 1), 45.0, res, res)


def room(resx=20, resy=14, specular=True, sampler=None, phong=False, n_materials=0, lens=None, flt=None, sky=None, lights=False, pick=None):
    """A closed box around a sphere light: a GGX floor (alpha 0.15), a mixed diffuse + GGX back wall, diffuse side
    walls, and (specular) a glass and a mirror sphere.  phong=True: the same room with Phong lobes of exponent
    2 / alpha^2 - 2 in place of the GGX ones (the version-7 twin, for measurements).  n_materials: pad the material list
    with unused GGX materials up to that many.  lights: a spot and an emissive triangle beside the bulb."""
    from smallvcm_amd.scene2 import SceneBuilder
    b = SceneBuilder()

    def glossy(kd, f0, alpha):
        if phong:
            return b.material(diffuse=kd, phong=f0, exponent=float(round(2.0 / alpha ** 2 - 2.0)))
        return b.material(diffuse=kd, ggx=f0, alpha=alpha)
    floor = glossy((0, 0, 0), (0.9, 0.75, 0.5), 0.15)
    back = glossy((0.45, 0.45, 0.5), (0.06, 0.06, 0.06), 0.35)
    white = b.material(diffuse=(0.803922, 0.803922, 0.803922))
    green = b.material(diffuse=(0.156863, 0.803922, 0.172549))
    red = b.material(diffuse=(0.803922, 0.152941, 0.152941))
    lo, hi = -1.25, 1.25
    c = [(lo, hi, lo), (hi, hi, lo), (hi, hi, hi), (lo, hi, hi), (lo, lo, lo), (hi, lo, lo), (hi, lo, hi), (lo, lo, hi)]
    b.triangle(c[0], c[4], c[5], floor); b.triangle(c[5], c[1], c[0], floor)       # floor
    b.triangle(c[0], c[1], c[2], back); b.triangle(c[2], c[3], c[0], back)         # back wall
    b.triangle(c[3], c[7], c[4], green); b.triangle(c[4], c[0], c[3], green)       # left
    b.triangle(c[1], c[5], c[6], red); b.triangle(c[6], c[2], c[1], red)           # right
    b.triangle(c[2], c[6], c[7], white); b.triangle(c[7], c[3], c[2], white)       # ceiling
    if sky is None:
        far = -4.5
        f = [(lo, far, lo), (hi, far, lo), (hi, far, hi), (lo, far, hi)]
        b.triangle(f[0], f[2], f[1], white); b.triangle(f[2], f[0], f[3], white)   # the wall behind the camera
    if specular:
        b.sphere(MIRROR_SPHERE[0], MIRROR_SPHERE[1], b.material(mirror=(1, 1, 1)))
        b.sphere(GLASS_SPHERE[0], GLASS_SPHERE[1], b.material(mirror=(1, 1, 1), ior=1.6))
    while len(b.materials) < n_materials:
        k = len(b.materials)
        m = b.material(diffuse=(0.3, 0.3, 0.3), ggx=(0.1 + 0.01 * (k % 7), 0.2, 0.3), alpha=0.05 + 0.02 * (k % 11))
        if k == n_materials - 1:   # the last one is in use: a small plate on the floor
            b.triangle((-0.2, -0.9, lo + 0.01), (0.2, -0.9, lo + 0.01), (0.2, -0.5, lo + 0.01), m)
    b.sphere_light((0.1, 0.1, 0.55), 0.18, (12.0, 11.0, 9.0))
    if lights:
        b.emissive_triangle(*LIGHT_TRIANGLE)   # normal -z
        b.spot_light((-0.8, -0.6, 1.0), (0.9, 0.8, -1.6), (3.0, 3.0, 4.0), 50.0, 30.0)
    if sky is not None:
        b.envmap_light(sky, 0.3)
    if lens is not None:
        b.thin_lens(*lens)
    if pick is not None:
        b.light_pick(*pick)
    if flt is not None:
        b.pixel_filter(*flt)
    if sampler is not None:
        b.sampler(sampler)
    return b.build(*ROOM_CAMERA, resx, resy)


ROOM_CAMERA = ((-0.0439815, -4.12529, 0.222539), (0.00688625, 0.998505, -0.0542161), (3.73896e-4, 0.0542148, 0.998529), 45.0)
LIGHT_TRIANGLE = ((-0.3, 0.6, 1.2), (0.3, 0.9, 1.2), (0.3, 0.6, 1.2), (20.0, 20.0, 20.0))
MIRROR_SPHERE = ((-0.55, 0.3, -0.85), 0.4)
GLASS_SPHERE = ((0.55, -0.2, -0.9), 0.35)


# ---- the analytic floor: a pure GGX floor z = 0, |x|, |y| <= 5, under a point light, seen through the pinhole
FLOOR_F0, FLOOR_ALPHA = (0.9, 0.75, 0.5), 0.3
FLOOR_CAMERA = ((0.0, -2.5, 4.0), (0.0, 2.5, -4.0), (0.0, 0.0, 1.0), 45.0)
FLOOR_LIGHT_POS, FLOOR_LIGHT_I = (0.6, 0.4, 2.0), (7.0, 6.0, 5.0)


def floor_scene(res=24):
    from smallvcm_amd.scene2 import SceneBuilder
    b = SceneBuilder()
    m = b.material(ggx=FLOOR_F0, alpha=FLOOR_ALPHA)
    b.triangle((-5, -5, 0), (5, -5, 0), (5, 5, 0), m)   # normal +z: the local frame is the world's
    b.triangle((5, 5, 0), (-5, 5, 0), (-5, -5, 0), m)
    b.point_light(FLOOR_LIGHT_POS, FLOOR_LIGHT_I)
    pos, fwd, up, fov = FLOOR_CAMERA
    return b.build(pos, fwd, up, fov, res, res)


def camera_rays(d, raster):
    """origin [3] and directions [n, 3] of the pinhole rays through raster points [n, 2] (binary64)"""
    cam = d.camera
    m = np.array(cam.rasterToWorld[:], np.float64).reshape(4, 4).T   # column-major storage
    p = np.concatenate([raster, np.zeros((len(raster), 1)), np.ones((len(raster), 1))], axis=1) @ m.T
    world = p[:, :3] / p[:, 3:4]
    org = np.array(cam.position[:], np.float64)
    dirs = world - org
    return org, dirs / np.linalg.norm(dirs, axis=1, keepdims=True)


def floor_reference(d, res=24, b=4, n=40000, seed=1):
    """per b x b block: mean [B, B, 3] and standard error of the closed form f I cos(theta) / d^2 over the block's
    footprint (Monte Carlo over raster points)"""
    rng = np.random.default_rng(seed)
    B = res // b
    mean, se = np.zeros((B, B, 3)), np.zeros((B, B, 3))
    f0 = np.array(FLOOR_F0, np.float32).astype(np.float64)
    for by in range(B):
        for bx in range(B):
            raster = np.array([bx * b, by * b]) + b * rng.random((n, 2))
            org, dirs = camera_rays(d, raster)
            t = -org[2] / dirs[:, 2]
            p = org + t[:, None] * dirs
            v = np.array(FLOOR_LIGHT_POS) - p
            dist = np.linalg.norm(v, axis=1)
            i = v / dist[:, None]
            f, _, _, _ = ggx_terms(-dirs, i, np.broadcast_to(f0, (n, 3)), float(np.float32(FLOOR_ALPHA)))
            val = f * (i[:, 2] / dist ** 2)[:, None] * np.array(FLOOR_LIGHT_I)
            mean[by, bx], se[by, bx] = val.mean(axis=0), val.std(axis=0, ddof=1) / np.sqrt(n)
    return mean, se


def silhouette_blocks(d, res, b=4, k=7):
    """blocks [B, B] of b x b pixels that a sphere's silhouette crosses -- some ray of the block (a dense grid per pixel,
    the corners included) passes inside the sphere and some ray outside: the geometric rule of the room comparison's
    exclusions"""
    g = np.linspace(0.0, 1.0, k)
    yy, xx, v, u = np.meshgrid(np.arange(res), np.arange(res), g, g, indexing="ij")
    raster = np.stack([(xx + u).ravel(), (yy + v).ravel()], axis=1)
    org, dirs = camera_rays(d, raster)
    touched = np.zeros((res // b, res // b), bool)
    for centre, radius in (MIRROR_SPHERE, GLASS_SPHERE):
        oc = np.array(centre) - org
        dist = np.sqrt(np.maximum(oc @ oc - (dirs @ oc) ** 2, 0.0))
        inside = (dist < radius).reshape(res // b, b, res // b, b, k * k)
        touched |= inside.any(axis=(1, 3, 4)) & ~inside.all(axis=(1, 3, 4))
    return touched


# ---- the host emulation
def emul_ggx():
    """build (make: a no-op when up to date) and load the GGX host emulation"""
    global _E
    if _E is None:
        subprocess.run(["make", "-C", EMUL_DIR], check=True, stdout=subprocess.DEVNULL)
        E = C.CDLL(os.path.join(EMUL_DIR, "libemul_ggx.so"))
        P8, P7 = C.POINTER(SceneDesc8), C.POINTER(SceneDesc7)
        for name, P in (("emul_create8", P8), ("emul_create7", P7)):
            getattr(E, name).restype = C.c_void_p
            getattr(E, name).argtypes = [P, C.c_int, C.c_float, C.c_float, C.c_int, C.c_int, C.c_int]
        E.emul_destroy.argtypes = [C.c_void_p]
        E.emul_run_iteration.argtypes = [C.c_void_p, C.c_int, C.c_uint, C.c_uint]
        E.emul_get_framebuffer.argtypes = [C.c_void_p, _fp]
        E.emul_get_counts.argtypes = [C.c_void_p, C.POINTER(C.c_ubyte), C.POINTER(C.c_ubyte)]
        E.emul_get_stats.argtypes = [C.c_void_p, C.POINTER(C.c_longlong)]
        E.emul_kat8.argtypes = [P8, C.c_int, C.c_int, _fp, _fp]
        E.emul_ggx_check.argtypes = [P8, C.POINTER(C.c_int), _fp]
        E.emul_ggx_error.restype = C.c_char_p
        E.emul_features8.argtypes = [P8, _fp, _fp]
        _E = E
    return _E


class Emul8(ll.Emul4):
    """one emulated renderer over a SceneDesc8 (or, version7=True, over a SceneDesc7 through emul_create7)"""

    def __init__(self, scene, algo, seed=1234, rank=0, world=1, radius_factor=0.003, radius_alpha=0.75, version7=False):
        self.E = emul_ggx()
        self.scene = scene
        create = self.E.emul_create7 if version7 else self.E.emul_create8
        assert isinstance(scene, SceneDesc7 if version7 else SceneDesc8)
        self.h = create(C.byref(scene), algo, radius_factor, radius_alpha, seed, rank, world)
        assert self.h, self.E.emul_ggx_error().decode()
        self.resx, self.resy = int(scene.camera.resolution[0]), int(scene.camera.resolution[1])
        self.N = self.resx * self.resy
        self.rank, self.world = rank, world


def kat8(scene, op, inp):
    inp = np.ascontiguousarray(inp, np.float32)
    out = np.zeros_like(inp)
    E = emul_ggx()
    assert E.emul_kat8(C.byref(scene), op, len(inp), inp.ctypes.data_as(_fp), out.ctypes.data_as(_fp)) == 0, \
        E.emul_ggx_error().decode()
    return out


def features(scene):
    """-> (guide [H, W, 4] = normal.xyz | depth, albedo [H, W, 4] = rgb | 1) of the host emulation"""
    W, H = int(scene.camera.resolution[0]), int(scene.camera.resolution[1])
    g, a = np.zeros((H, W, 4), np.float32), np.zeros((H, W, 4), np.float32)
    E = emul_ggx()
    assert E.emul_features8(C.byref(scene), g.ctypes.data_as(_fp), a.ctypes.data_as(_fp)) == 0, E.emul_ggx_error().decode()
    return g, a


def check(scene):
    """what the scene host says: (None, ext table [n, 4]) when it accepts the description, (message, None) otherwise"""
    n = C.c_int(-1)
    ext = np.zeros((max(int(desc2_of(scene).nMaterials), 1), 4), np.float32)
    E = emul_ggx()
    if E.emul_ggx_check(C.byref(scene), C.byref(n), ext.ctypes.data_as(_fp)) != 0:
        return E.emul_ggx_error().decode(), None
    return None, ext[:n.value]


def as_desc7(d):
    """the version-7 part of any description"""
    if isinstance(d, SceneDesc8):
        d = d.base
    return d if isinstance(d, SceneDesc7) else with_sampler(d, None)


# ---- the known-answer records
def uniforms(rng, shape):
    """floats of the generator's form (2j + 1) 2^-24, j < 2^23: in (0, 1), as the device draws them"""
    j = rng.integers(0, 1 << 23, size=shape, dtype=np.int64)
    return ((2 * j + 1).astype(np.float64) * 2.0 ** -24).astype(np.float32)


def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


RANDOM_FRAME_MIN_COS = 0.1


def random_records(n=50000, seed=9, n_materials=len(KAT_MATERIALS)):
    """(eval records, sample records).  The fixed direction comes from the front side (a tenth from behind), the
    generated one from the whole sphere (four fifths above the surface); three uniforms and both fixIsLight for the
    samples.  Half of the records have an axis as normal: there the local components ARE the record's binary32 numbers,
    and those records reach down to grazing directions, the EPS_COSINE threshold and alpha = 0.01.  The other half have a
    random normal, directions at least RANDOM_FRAME_MIN_COS off the surface and materials of alpha >= 0.1: a direction
    stored in binary32 is off by ~1e-7 in every local component, the half vector by that over |o + i| >= o_z, and the
    lobe's d by that over alpha -- 1e-7 / (0.1 * 0.1) = 1e-5 stays below the tolerance of the comparison, while at
    alpha = 0.01 and o_z = 0.02 the record's own rounding is 5e-4 of the value."""
    rng = np.random.default_rng(seed)
    axis = rng.random(n) < 0.5
    normal = _unit(rng, n)
    eye = np.concatenate([np.eye(3), -np.eye(3)])
    normal[axis] = eye[rng.integers(0, 6, axis.sum())]
    fr = frame(normal)

    def local_dirs(up_share):
        v = _unit(rng, n)
        graze = axis & (rng.random(n) < 0.015)   # (two fifths of them land within 1e-4 of the threshold and are left out)
        v[graze, 2] *= 10.0 ** rng.uniform(-6, -1, graze.sum())
        steep = ~axis & (np.abs(v[:, 2]) < RANDOM_FRAME_MIN_COS)
        v[steep, 2] = np.where(v[steep, 2] < 0, -RANDOM_FRAME_MIN_COS, RANDOM_FRAME_MIN_COS)
        v /= np.linalg.norm(v, axis=1, keepdims=True)
        v[:, 2] = np.abs(v[:, 2]) * np.where(rng.random(n) < up_share, 1.0, -1.0)
        return v
    ray = -to_world(fr, local_dirs(0.9))
    gen = to_world(fr, local_dirs(0.8))
    mat = rng.integers(0, n_materials, n)
    wide = np.array([k for k in range(n_materials) if KAT_MATERIALS[k][6] >= 0.1])
    mat[~axis] = wide[rng.integers(0, len(wide), (~axis).sum())]
    ev = np.zeros((n, KAT), np.float32)
    ev[:, 0:3], ev[:, 3:6], ev[:, 6], ev[:, 7:10] = ray, normal, mat, gen
    sa = ev.copy()
    sa[:, 7:10] = uniforms(rng, (n, 3))
    sa[:, 10] = rng.integers(0, 2, n)
    return ev, sa


# ---- the numpy restatement (binary64)
def frame(normal):
    """Frame::SetFromZ (the public SmallVCM's frame.hxx): the local axes [n, 3] each"""
    z = normal / np.linalg.norm(normal, axis=1, keepdims=True)
    tx = np.where((np.abs(z[:, 0]) > 0.99)[:, None], np.array([0.0, 1.0, 0.0]), np.array([1.0, 0.0, 0.0]))
    y = np.cross(z, tx)
    y /= np.linalg.norm(y, axis=1, keepdims=True)
    return np.cross(y, z), y, z


def to_local(fr, v):
    return np.stack([np.einsum("ij,ij->i", v, a) for a in fr], axis=1)


def to_world(fr, v):
    return fr[0] * v[:, 0:1] + fr[1] * v[:, 1:2] + fr[2] * v[:, 2:3]


def lum(c):
    return 0.212671 * c[..., 0] + 0.715160 * c[..., 1] + 0.072169 * c[..., 2]


def lam(w, a):
    return (-1.0 + np.sqrt(1.0 + a ** 2 * (w[:, 0] ** 2 + w[:, 1] ** 2) / w[:, 2] ** 2)) / 2.0


def schlick(f0, c):
    return f0 + (1.0 - f0) * (1.0 - np.clip(c, 0.0, 1.0))[:, None] ** 5


def ggx_terms(o, i, f0, a):
    """(f [n, 3], direct pdf, reverse pdf, dot(o, h)) of the lobe alone; zero where o_z or i_z < EPS_COSINE"""
    ok = (o[:, 2] >= EPS_COSINE) & (i[:, 2] >= EPS_COSINE)
    with np.errstate(all="ignore"):
        h = o + i
        h = h / np.linalg.norm(h, axis=1, keepdims=True)
        d = a ** 2 * h[:, 2] ** 2 + (h[:, 0] ** 2 + h[:, 1] ** 2)
        D = a ** 2 / (np.pi * d ** 2)
        lo, li = lam(o, a), lam(i, a)
        oh = np.einsum("ij,ij->i", o, h)
        f = schlick(f0, oh) * (D / (1 + lo + li) / (4 * o[:, 2] * i[:, 2]))[:, None]
        pd = D / (1 + lo) / (4 * o[:, 2])
        pr = D / (1 + li) / (4 * i[:, 2])
    z = np.zeros(len(o))
    return np.where(ok[:, None], f, 0.0), np.where(ok, pd, z), np.where(ok, pr, z), oh


def _materials(mat):
    cols = [np.array([np.atleast_1d(np.array(m[k], np.float32).astype(np.float64)) for m in KAT_MATERIALS]) for k in range(7)]
    return [c[mat] if c.shape[1] > 1 else c[mat, 0] for c in cols]


def fresnel_dielectric(cos_i, ior):
    """FresnelDielectric of the public SmallVCM (utils.hxx); ior < 0: 1"""
    cos_i = np.array(cos_i, np.float64)
    ior = np.array(ior, np.float64)
    with np.errstate(all="ignore"):
        neg = cos_i < 0
        eta = np.where(neg, ior, 1.0 / ior)
        ci = np.abs(cos_i)
        sin2 = eta ** 2 * (1 - ci ** 2)
        ct = np.sqrt(np.maximum(0.0, 1 - sin2))
        rs = (ci - eta * ct) / (ci + eta * ct)   # with etaIncident = 1, etaTransmitted = 1 / eta
        rp = (eta * ci - ct) / (eta * ci + ct)
        r = np.where(sin2 > 1, 1.0, (rs ** 2 + rp ** 2) / 2)
    return np.where(ior < 0, 1.0, r)


def probabilities(o, mat):
    """component probabilities and the continuation probability: dict of arrays"""
    kd, ks, n, km, ior, f0, a = _materials(mat)
    rc = fresnel_dielectric(o[:, 2], ior)
    has = np.any(f0 != 0, axis=1)
    fz = schlick(f0, o[:, 2]) * has[:, None]
    alb = {"d": lum(kd), "p": lum(ks), "g": lum(fz), "r": rc * lum(km), "t": (1 - rc) * (ior > 0)}
    tot = sum(alb.values())
    with np.errstate(all="ignore"):
        pr = {k: np.where(tot < 1e-9, 0.0, v / tot) for k, v in alb.items()}
    cont = np.clip((kd + ks + rc[:, None] * km + fz).max(axis=1) + (1 - rc), 0.0, 1.0)
    pr["cont"] = np.where(tot < 1e-9, 0.0, cont)
    pr["rc"] = rc
    return pr


def evaluate(o, i, mat, pr=None):
    """BSDF::Evaluate with the lobe: (f [n, 3], direct pdf, reverse pdf) in the local frame"""
    kd, ks, n, km, ior, f0, a = _materials(mat)
    pr = pr or probabilities(o, mat)
    same = i[:, 2] * o[:, 2] >= 0
    ok = (o[:, 2] >= EPS_COSINE) & (i[:, 2] >= EPS_COSINE)
    f = np.zeros((len(o), 3))
    pd, prv = np.zeros(len(o)), np.zeros(len(o))
    don = ok & (pr["d"] != 0)
    f += np.where(don[:, None], kd / np.pi, 0.0)
    pd += np.where(don, pr["d"] * np.maximum(0, i[:, 2] / np.pi), 0.0)
    prv += np.where(don, pr["d"] * np.maximum(0, o[:, 2] / np.pi), 0.0)
    refl = o * np.array([-1.0, -1.0, 1.0])
    dot = np.einsum("ij,ij->i", refl, i)
    pon = ok & (pr["p"] != 0) & (dot > EPS_PHONG)
    with np.errstate(all="ignore"):
        pw = np.where(pon, np.abs(dot) ** n, 0.0)
    f += np.where(pon[:, None], ks * ((n + 2) * 0.5 / np.pi * pw)[:, None], 0.0)
    ppdf = np.where(pon, pr["p"] * (n + 1) * pw * 0.5 / np.pi, 0.0)
    pd += ppdf
    prv += ppdf
    gf, gd, gr, oh = ggx_terms(o, i, f0, a)
    gon = pr["g"] != 0
    f += np.where(gon[:, None], gf, 0.0)
    pd += np.where(gon, pr["g"] * gd, 0.0)
    prv += np.where(gon, pr["g"] * gr, 0.0)
    return np.where(same[:, None], f, 0.0), np.where(same, pd, 0.0), np.where(same, prv, 0.0), dot, oh


def ggx_sample(o, a, r0, r1):
    """the visible normal by the spherical cap, reflected: the generated local direction [n, 3]"""
    s = np.stack([a * o[:, 0], a * o[:, 1], o[:, 2]], axis=1)
    s /= np.linalg.norm(s, axis=1, keepdims=True)
    z = (1 - r1) * (1 + s[:, 2]) - s[:, 2]
    st = np.sqrt(np.clip(1 - z * z, 0, 1))
    phi = 2 * np.pi * r0
    m = np.stack([st * np.cos(phi), st * np.sin(phi), z], axis=1) + s
    h = np.stack([a * m[:, 0], a * m[:, 1], np.maximum(m[:, 2], 0.0)], axis=1)
    h /= np.linalg.norm(h, axis=1, keepdims=True)
    return 2 * np.einsum("ij,ij->i", o, h)[:, None] * h - o


def directional_albedo(alpha, theta, f0=1.0, n=400):
    """integral of f cos over the upper hemisphere for o at angle theta, by a product Gauss-Legendre rule in
    (mu = cos theta_i in sub-intervals, phi)"""
    o = np.array([[np.sin(theta), 0.0, np.cos(theta)]])
    xs, ws = np.polynomial.legendre.leggauss(n)
    # the lobe is narrow around the mirror direction: split mu and phi where it sits
    total = 0.0
    mu_edges = np.unique(np.clip(np.concatenate([[0.0, 1.0], np.cos(theta) + np.array([-8, -3, -1, 1, 3, 8]) * max(alpha, 0.02) * 0.5]), 0.0, 1.0))
    phi_edges = np.unique(np.clip(np.concatenate([[0.0, np.pi], np.pi - np.array([1, 3, 10, 30]) * max(alpha, 0.02)]), 0.0, np.pi))
    for a0, a1 in zip(mu_edges[:-1], mu_edges[1:]):
        mu = 0.5 * (a1 - a0) * xs + 0.5 * (a1 + a0)
        wm = 0.5 * (a1 - a0) * ws
        for p0, p1 in zip(phi_edges[:-1], phi_edges[1:]):
            ph = 0.5 * (p1 - p0) * xs + 0.5 * (p1 + p0)
            wp = 0.5 * (p1 - p0) * ws
            M, P = np.meshgrid(mu, ph, indexing="ij")
            st = np.sqrt(1 - M ** 2)
            i = np.stack([st * np.cos(P), st * np.sin(P), M], axis=-1).reshape(-1, 3)
            f, _, _, _ = ggx_terms(np.repeat(o, len(i), axis=0), i, np.full((len(i), 3), f0), alpha)
            total += 2.0 * np.sum((f[:, 0] * i[:, 2]).reshape(M.shape) * wm[:, None] * wp[None, :])   # phi in [0, pi] twice
    return total
