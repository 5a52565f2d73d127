"""Camera projections for the tests (test infrastructure): scenes seen through a fisheye or a panorama, the ctypes
binding of tests/host_emul_proj/libemul_proj.so, the known-answer records, and a binary64 numpy restatement of both
projections written from their definition (DESIGN.md "Camera projections"), not from csrc/vcm_core.h."""
import ctypes as C
import os
import subprocess

import numpy as np

import lens_lib as ll
from smallvcm_amd._abi import SceneDesc8, SceneDesc9, with_material_ext, with_projection

HERE = os.path.dirname(os.path.abspath(__file__))
EMUL_DIR = os.path.join(HERE, "host_emul_proj")
OP_PROJECTION = 13   # VCM_KAT_PROJECTION
KAT = 16
PERSPECTIVE, FISHEYE, PANORAMA = 0, 1, 2
_fp = C.POINTER(C.c_float)
_E = None

# the camera of the estimator scenes: inside the box, looking along +y and a little to the side and down
INSIDE_CAMERA = ((0.15, -0.55, 0.1), (0.12, 1.0, -0.15), (0.0, 0.0, 1.0), 60.0)
MIRROR_SPHERE = ((-0.55, 0.45, -0.85), 0.4)


def as_desc9(d, kind=None, fov=0.0):
    return d if isinstance(d, SceneDesc9) else with_projection(d, kind, fov)


def as_desc8(d):
    """the version-8 part of any description"""
    if isinstance(d, SceneDesc9):
        return d.base
    return d if isinstance(d, SceneDesc8) else with_material_ext(d, None)


def box(resx, resy, proj=None, room=False, flt=None, sampler=None, camera=INSIDE_CAMERA, sky=None, lights=False, pick=None, ggx=False,
        exponent=30.0):
    """A closed box [-1.25, 1.25]^3 with the camera inside, so that every direction sees geometry.  room=False: diffuse
    walls, a glossy floor and a point light (nothing emissive in view: what light tracing can render).  room=True: an
    area light under the ceiling and a mirror sphere on the floor.  proj: None, ("fisheye", deg) or ("panorama",).
    sky: an environment map replaces the ceiling.  lights: a spot and a sphere light beside.  ggx: a GGX floor."""
    from smallvcm_amd.scene2 import SceneBuilder
    b = SceneBuilder()
    if ggx:
        floor = b.material(diffuse=(0.2, 0.2, 0.2), ggx=(0.8, 0.7, 0.5), alpha=0.2)
    else:
        floor = b.material(diffuse=(0.3, 0.3, 0.3), phong=(0.5, 0.5, 0.5), exponent=exponent)
    white = b.material(diffuse=(0.803922, 0.803922, 0.803922))
    green = b.material(diffuse=(0.156863, 0.803922, 0.172549))
    red = b.material(diffuse=(0.803922, 0.152941, 0.152941))
    blue = b.material(diffuse=(0.2, 0.3, 0.803922))
    lo, hi = -1.25, 1.25
    c = [(lo, hi, lo), (hi, hi, lo), (hi, hi, hi), (lo, hi, hi), (lo, lo, lo), (hi, lo, lo), (hi, lo, hi), (lo, lo, hi)]
    b.triangle(c[0], c[4], c[5], floor); b.triangle(c[5], c[1], c[0], floor)       # floor
    b.triangle(c[0], c[1], c[2], white); b.triangle(c[2], c[3], c[0], white)       # the wall in front
    b.triangle(c[3], c[7], c[4], green); b.triangle(c[4], c[0], c[3], green)       # left
    b.triangle(c[1], c[5], c[6], red); b.triangle(c[6], c[2], c[1], red)           # right
    b.triangle(c[4], c[7], c[6], blue); b.triangle(c[6], c[5], c[4], blue)         # the wall behind
    if sky is None:
        b.triangle(c[2], c[6], c[7], white); b.triangle(c[7], c[3], c[2], white)   # ceiling
    if room:
        b.sphere(MIRROR_SPHERE[0], MIRROR_SPHERE[1], b.material(mirror=(1, 1, 1)))
        z = hi - 0.02
        b.emissive_triangle((-0.4, -0.1, z), (0.4, 0.7, z), (0.4, -0.1, z), (18.0, 17.0, 15.0))   # normal -z
        b.emissive_triangle((0.4, 0.7, z), (-0.4, -0.1, z), (-0.4, 0.7, z), (18.0, 17.0, 15.0))
    else:
        b.point_light((-0.3, 0.2, 0.9), (1.6, 1.5, 1.3))
    if lights:
        b.spot_light((0.8, -0.6, 1.0), (-0.9, 0.8, -1.6), (3.0, 3.0, 4.0), 50.0, 30.0)
        b.sphere_light((0.6, 0.5, 0.3), 0.15, (9.0, 8.0, 7.0))
    if sky is not None:
        b.envmap_light(sky, 0.5)
    if pick is not None:
        b.light_pick(*pick)
    if flt is not None:
        b.pixel_filter(*flt)
    if sampler is not None:
        b.sampler(sampler)
    if proj is not None:
        b.projection(*proj)
    return b.build(*camera, resx, resy)


# ---- the host emulation
def emul_proj():
    """build (make: a no-op when up to date) and load the projection host emulation"""
    global _E
    if _E is None:
        subprocess.run(["make", "-C", EMUL_DIR], check=True, stdout=subprocess.DEVNULL)
        E = C.CDLL(os.path.join(EMUL_DIR, "libemul_proj.so"))
        P9, P8 = C.POINTER(SceneDesc9), C.POINTER(SceneDesc8)
        for name, P in (("emul_create9", P9), ("emul_create8", P8)):
            getattr(E, name).restype = C.c_void_p
            getattr(E, name).argtypes = [P, C.c_int, C.c_float, C.c_float, C.c_int, C.c_int, C.c_int]
        E.emul_destroy.argtypes = [C.c_void_p]
        E.emul_run_iteration.argtypes = [C.c_void_p, C.c_int, C.c_uint, C.c_uint]
        E.emul_get_framebuffer.argtypes = [C.c_void_p, _fp]
        E.emul_get_counts.argtypes = [C.c_void_p, C.POINTER(C.c_ubyte), C.POINTER(C.c_ubyte)]
        E.emul_get_stats.argtypes = [C.c_void_p, C.POINTER(C.c_longlong)]
        E.emul_kat9.argtypes = [P9, C.c_int, C.c_int, _fp, _fp]
        E.emul_proj_params.argtypes = [P9, _fp]
        E.emul_proj_error.restype = C.c_char_p
        E.emul_features9.argtypes = [P9, _fp, _fp]
        _E = E
    return _E


class Emul9(ll.Emul4):
    """one emulated renderer over a SceneDesc9 (or, version8=True, over a SceneDesc8 through emul_create8)"""

    def __init__(self, scene, algo, seed=1234, rank=0, world=1, radius_factor=0.003, radius_alpha=0.75, version8=False):
        self.E = emul_proj()
        self.scene = scene
        create = self.E.emul_create8 if version8 else self.E.emul_create9
        assert isinstance(scene, SceneDesc8 if version8 else SceneDesc9)
        self.h = create(C.byref(scene), algo, radius_factor, radius_alpha, seed, rank, world)
        assert self.h, self.E.emul_proj_error().decode()
        self.resx, self.resy = int(scene.camera.resolution[0]), int(scene.camera.resolution[1])
        self.N = self.resx * self.resy
        self.rank, self.world = rank, world


def kat9(scene, inp, op=OP_PROJECTION):
    inp = np.ascontiguousarray(inp, np.float32)
    out = np.zeros_like(inp)
    E = emul_proj()
    assert E.emul_kat9(C.byref(scene), op, len(inp), inp.ctypes.data_as(_fp), out.ctypes.data_as(_fp)) == 0, \
        E.emul_proj_error().decode()
    return out


def features(scene):
    """-> (guide [H, W, 4] = normal.xyz | depth, albedo [H, W, 4] = rgb | 1) of the host emulation"""
    W, H = int(scene.camera.resolution[0]), int(scene.camera.resolution[1])
    g, a = np.zeros((H, W, 4), np.float32), np.zeros((H, W, 4), np.float32)
    E = emul_proj()
    assert E.emul_features9(C.byref(scene), g.ctypes.data_as(_fp), a.ctypes.data_as(_fp)) == 0, E.emul_proj_error().decode()
    return g, a


def params(scene):
    """what the scene host says: (None, dict) when it accepts the description, (message, None) otherwise"""
    out = np.zeros(13, np.float32)
    E = emul_proj()
    if E.emul_proj_params(C.byref(scene), out.ctypes.data_as(_fp)) != 0:
        return E.emul_proj_error().decode(), None
    return None, {"kind": int(out[0]), "fov": float(out[1]), "k": float(out[2]), "theta_max": float(out[3]),
                  "f": out[4:7].astype(np.float64), "ex": out[7:10].astype(np.float64), "ey": out[10:13].astype(np.float64)}


# ---- the numpy restatement (binary64)
def camera_frame(cam):
    """(c, f, ex, ey, W, H) from the camera as stored: f = forward, ex = raster +x made orthogonal to f, ey = +-(f x ex)
    along raster +y"""
    m = np.array(cam.rasterToWorld[:], np.float64).reshape(4, 4).T   # column-major storage

    def point(x, y):
        p = m @ np.array([x, y, 0.0, 1.0])
        return p[:3] / p[3]
    o = point(0, 0)
    f = np.array(cam.forward[:], np.float64)
    f /= np.linalg.norm(f)
    ex = point(1, 0) - o
    ex -= (ex @ f) * f
    ex /= np.linalg.norm(ex)
    ey = np.cross(f, ex)
    if ey @ (point(0, 1) - o) < 0:
        ey = -ey
    return np.array(cam.position[:], np.float64), f, ex, ey, float(cam.resolution[0]), float(cam.resolution[1])


class Reference:
    """both maps of one camera in binary64"""

    def __init__(self, scene, kind, fov_deg=0.0):
        self.c, self.f, self.ex, self.ey, self.W, self.H = camera_frame(scene.camera)
        self.kind = kind
        if kind == FISHEYE:
            fov = np.deg2rad(float(np.float32(fov_deg)))
            self.k, self.theta_max = self.W / fov, fov / 2

    def forward(self, raster):
        """raster [n, 2] -> (dir [n, 3], pdfW [n], valid [n], theta [n])"""
        x, y = raster[:, 0].astype(np.float64), raster[:, 1].astype(np.float64)
        with np.errstate(all="ignore"):
            if self.kind == FISHEYE:
                qx, qy = x - self.W / 2, y - self.H / 2
                rho = np.hypot(qx, qy)
                theta = rho / self.k
                ux, uy = np.where(rho > 0, qx / rho, 0.0), np.where(rho > 0, qy / rho, 0.0)
                d = np.sin(theta)[:, None] * (ux[:, None] * self.ex + uy[:, None] * self.ey) + np.cos(theta)[:, None] * self.f
                g = np.where(theta < 1e-3, 1.0, theta / np.maximum(np.sin(theta), 1e-4))
                return d, self.k ** 2 * g, theta <= self.theta_max, theta
            lam, theta = 2 * np.pi * (x / self.W - 0.5), np.pi * y / self.H
            d = np.sin(theta)[:, None] * (np.cos(lam)[:, None] * self.f + np.sin(lam)[:, None] * self.ex) - np.cos(theta)[:, None] * self.ey
            pdf = self.W * self.H / (2 * np.pi ** 2 * np.maximum(np.abs(np.sin(theta)), 1e-4))
            return d, pdf, (y >= 0) & (y < self.H), theta

    def inverse(self, world):
        """world points [n, 3] -> (raster [n, 2], pdfW [n], inside the field of view [n], theta [n])"""
        d = world.astype(np.float64) - self.c
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        a, b, z = d @ self.ex, d @ self.ey, d @ self.f
        with np.errstate(all="ignore"):
            if self.kind == FISHEYE:
                theta = np.arccos(np.clip(z, -1, 1))
                s = np.hypot(a, b)
                t = np.where(s > 0, self.k * theta / s, 0.0)
                g = np.where(theta < 1e-3, 1.0, theta / np.maximum(np.sin(theta), 1e-4))
                return np.stack([self.W / 2 + t * a, self.H / 2 + t * b], axis=1), self.k ** 2 * g, theta <= self.theta_max, theta
            theta = np.arccos(np.clip(-b, -1, 1))
            lam = np.arctan2(a, z)
            r = np.stack([np.mod(self.W * (lam / (2 * np.pi) + 0.5), self.W), np.minimum(self.H * theta / np.pi, self.H)], axis=1)
            pdf = self.W * self.H / (2 * np.pi ** 2 * np.maximum(np.abs(np.sin(theta)), 1e-4))
            return r, pdf, np.ones(len(d), bool), theta

    def raster_error(self, got, want):
        """per record, the distance in pixels (the panorama's x is periodic)"""
        dx = np.abs(got[:, 0].astype(np.float64) - want[:, 0])
        if self.kind == PANORAMA:
            dx = np.minimum(dx, self.W - dx)
        return np.maximum(dx, np.abs(got[:, 1].astype(np.float64) - want[:, 1]))

    def left_out(self, theta):
        """the two rules on the inputs: theta within 1e-4 of theta_max (fisheye), |sin theta| < 0.05"""
        out = np.abs(np.sin(theta)) < 0.05
        if self.kind == FISHEYE:
            out |= np.abs(theta - self.theta_max) < 1e-4
        return out


def records(scene, n=50000, seed=3, margin=2.0):
    """VCM_KAT_PROJECTION input records: raster points uniform over the image grown by `margin` pixels, world points in
    uniformly distributed directions at distances 0.05 .. 50 from the camera"""
    rng = np.random.default_rng(seed)
    W, H = float(scene.camera.resolution[0]), float(scene.camera.resolution[1])
    inp = np.zeros((n, KAT), np.float32)
    inp[:, 0] = rng.uniform(-margin, W + margin, n)
    inp[:, 1] = rng.uniform(-margin, H + margin, n)
    v = rng.normal(size=(n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    inp[:, 2:5] = np.array(scene.camera.position[:], np.float64) + v * (10.0 ** rng.uniform(np.log10(0.05), np.log10(50.0), n))[:, None]
    return inp
