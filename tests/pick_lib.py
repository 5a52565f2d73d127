"""Light-selection scenes for the tests (test infrastructure): version-5 descriptions over the built-in boxes and over
procedural many-light rooms, and the ctypes binding of tests/host_emul_pick/libemul_pick.so."""
import ctypes as C
import os
import subprocess

import numpy as np

import lens_lib as ll
from smallvcm_amd._abi import (Light, LightPick, SceneDesc2, SceneDesc3, SceneDesc4, SceneDesc5, LIGHT_PICK_CUSTOM,
                               LIGHT_PICK_POWER, LIGHT_PICK_UNIFORM)

HERE = os.path.dirname(os.path.abspath(__file__))
EMUL_DIR = os.path.join(HERE, "host_emul_pick")
OP_LIGHT_EMIT = 4    # VCM_KAT_LIGHT_EMIT
OP_LIGHT_PICK = 9    # VCM_KAT_LIGHT_PICK
KAT = 16
Q = 1 << 23          # quanta of the table: pmf[i] = m_i / Q
UNIFORM, POWER, CUSTOM = LIGHT_PICK_UNIFORM, LIGHT_PICK_POWER, LIGHT_PICK_CUSTOM
_fp = C.POINTER(C.c_float)
_E = None


def as_desc4(d):
    """any description up to version 4 as a SceneDesc4 (no lens added)"""
    if isinstance(d, SceneDesc4):
        return d
    if isinstance(d, SceneDesc2):
        d3 = SceneDesc3()
        d3.base = d
        d3._keep = (getattr(d, "_keep", None), d)
        d = d3
    assert isinstance(d, SceneDesc3)
    return ll.with_lens(d, None, None)


def with_pick(d, mode, mix=0.0, weights=None):
    """a description seen with a light-selection setting (mode None: pick = NULL)"""
    d4 = as_desc4(d)
    d5 = SceneDesc5()
    d5.base = d4
    keep = [getattr(d4, "_keep", None), d4]
    if mode is not None:
        w = None if weights is None else np.ascontiguousarray(weights, np.float32)
        pick = LightPick(int(mode), float(mix), w.ctypes.data_as(_fp) if w is not None else None)
        d5.pick = C.pointer(pick)
        keep += [pick, w]
    d5._keep = tuple(keep)
    return d5


def n_lights(d):
    while not isinstance(d, SceneDesc2):
        d = d.base
    return int(d.nLights)


def add_point_lights(d3, lights):
    """a copy of a SceneDesc3 whose light table has the point lights [(position, intensity), ...] appended (the
    geometry, and so the kind of scene the kernels see, stays what it was)"""
    from smallvcm_amd.renderer import load_library
    L = load_library(require_gpu=False)
    L.vcm_make_point_light.argtypes = [_fp, _fp, C.POINTER(Light)]
    L.vcm_make_point_light.restype = None
    b = d3.base
    n = int(b.nLights)
    arr = (Light * (n + len(lights)))(*b.lights[:n])
    for k, (p, i) in enumerate(lights):
        L.vcm_make_point_light((C.c_float * 3)(*p), (C.c_float * 3)(*i), C.byref(arr[n + k]))
    out = SceneDesc3.from_buffer_copy(d3)
    out.base.nLights = n + len(lights)
    out.base.lights = C.cast(arr, C.POINTER(Light))
    out._keep = (getattr(d3, "_keep", None), d3, arr)
    return out


def box_many_lights(n_extra=6, resx=20, resy=14, seed=3):
    """scene 3 (one light: the background) with n_extra point lights of very different intensities inside"""
    rng = np.random.default_rng(seed)
    pts = [((rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(-0.5, 1.0)),
            tuple(float(x) for x in rng.uniform(0.2, 1.0, 3) * 10.0 ** rng.uniform(-2, 0.5))) for _ in range(n_extra)]
    return add_point_lights(ll.builtin3(resx=resx, resy=resy), pts)


def lamp_room(resx=24, resy=24, specular=True, n_dim=64, lamp=25.0, dim=0.25, point=0.02, off=1.2):
    """A box with one bright lamp quad on the ceiling, n_dim small dim emissive triangles of other colours on the walls
    and a weak point light: 2 + n_dim + 1 = 67 lights of which the two lamp triangles carry nearly all the flux."""
    from smallvcm_amd.scene2 import SceneBuilder
    rng = np.random.default_rng(11)
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
    if specular:
        b.sphere((-0.5, 0.3, -0.85), 0.4, b.material(mirror=(1, 1, 1)))
        b.sphere((0.55, -0.2, -0.9), 0.35, b.material(mirror=(1, 1, 1), ior=1.6))
    q = [(-0.3, -0.3, 1.2), (0.3, -0.3, 1.2), (0.3, 0.3, 1.2), (-0.3, 0.3, 1.2)]   # the lamp, facing down
    b.emissive_triangle(q[0], q[2], q[1], (lamp, lamp, lamp))                      # (normal = e1 x e2 = -z)
    b.emissive_triangle(q[2], q[0], q[3], (lamp, lamp, lamp))
    for k in range(n_dim):   # dim triangles just inside the back wall (facing -y) and the side walls (facing inwards)
        u, v = rng.uniform(-1.0, 0.9), rng.uniform(-0.9, 0.9)
        col = tuple(float(x) for x in dim * rng.uniform(0.1, 1.0, 3))
        s = 0.12
        if k % 3 == 0:
            b.emissive_triangle((u, off, v), (u + s, off, v), (u, off, v + s), col)
        elif k % 3 == 1:
            b.emissive_triangle((-off, u, v), (-off, u + s, v), (-off, u, v + s), col)   # normal +x
        else:
            b.emissive_triangle((off, u, v), (off, u, v + s), (off, u + s, v), col)     # normal -x
    b.point_light((0.0, -0.5, 0.6), (point, point, point))
    return as_desc4(b.build((-0.0439815, -4.12529, 0.222539), (0.00688625, 0.998505, -0.0542161),
                            (3.73896e-4, 0.0542148, 0.998529), 45.0, resx, resy))


def point_light_scene(weights, resx=8, resy=8):
    """one floor triangle and len(weights) point lights; a light of weight 0 is black (the only kind CUSTOM accepts a
    zero for), the others emit 1"""
    from smallvcm_amd.scene2 import SceneBuilder
    b = SceneBuilder()
    b.triangle((-1, -1, 0), (1, -1, 0), (0, 1, 0), b.material(diffuse=(0.7, 0.7, 0.7)))
    for k, w in enumerate(weights):
        i = 0.0 if w == 0 else 1.0
        b.point_light((0.3 * np.cos(k), 0.3 * np.sin(k), 1.0), (i, i, i))
    return as_desc4(b.build((0, -4, 2), (0, 1, -0.4), (0, 0, 1), 50, resx, resy))


def emul_pick():
    """build (make: a no-op when up to date) and load the light-selection host emulation"""
    global _E
    if _E is None:
        subprocess.run(["make", "-C", EMUL_DIR], check=True, stdout=subprocess.DEVNULL)
        E = C.CDLL(os.path.join(EMUL_DIR, "libemul_pick.so"))
        P5 = C.POINTER(SceneDesc5)
        E.emul_create5.restype = C.c_void_p
        E.emul_create5.argtypes = [P5, C.c_int, C.c_float, C.c_float, C.c_int, C.c_int, C.c_int]
        E.emul_destroy.argtypes = [C.c_void_p]
        E.emul_run_iteration.argtypes = [C.c_void_p, C.c_int, C.c_uint, C.c_uint]
        E.emul_get_framebuffer.argtypes = [C.c_void_p, _fp]
        E.emul_get_counts.argtypes = [C.c_void_p, C.POINTER(C.c_ubyte), C.POINTER(C.c_ubyte)]
        E.emul_get_stats.argtypes = [C.c_void_p, C.POINTER(C.c_longlong)]
        E.emul_kat5.argtypes = [P5, C.c_int, C.c_int, _fp, _fp]
        E.emul_pick_tables.argtypes = [P5, C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_int), _fp, _fp]
        E.emul_pick_count.argtypes = [P5, C.c_uint, C.c_uint, C.POINTER(C.c_longlong)]
        E.emul_pick_error.restype = C.c_char_p
        _E = E
    return _E


class Emul5(ll.Emul4):
    """one emulated renderer over a SceneDesc5 (rank / world: a shard of it)"""

    def __init__(self, scene, algo, seed=1234, rank=0, world=1, radius_factor=0.003, radius_alpha=0.75):
        self.E = emul_pick()
        self.scene = scene
        self.h = self.E.emul_create5(C.byref(scene), algo, radius_factor, radius_alpha, seed, rank, world)
        assert self.h, self.E.emul_pick_error().decode()
        self.resx, self.resy = int(scene.camera.resolution[0]), int(scene.camera.resolution[1])
        self.N = self.resx * self.resy
        self.rank, self.world = rank, world


def kat5(scene, op, inp):
    inp = np.ascontiguousarray(inp, np.float32)
    out = np.zeros_like(inp)
    E = emul_pick()
    assert E.emul_kat5(C.byref(scene), op, len(inp), inp.ctypes.data_as(_fp), out.ctypes.data_as(_fp)) == 0, \
        E.emul_pick_error().decode()
    return out


def tables(scene):
    """-> (mode, weights before the mix [float64], quanta m_i [int], pmf [float32], cdf [float32]) as the scene host
    builds them; a UNIFORM scene has mode 0 and empty tables"""
    n = n_lights(scene)
    mode = C.c_int(0)
    w, m = np.zeros(n, np.float64), np.zeros(n, np.int32)
    pmf, cdf = np.zeros(n, np.float32), np.zeros(n + 1, np.float32)
    E = emul_pick()
    assert E.emul_pick_tables(C.byref(scene), C.byref(mode), w.ctypes.data_as(C.POINTER(C.c_double)),
                              m.ctypes.data_as(C.POINTER(C.c_int)), pmf.ctypes.data_as(_fp), cdf.ctypes.data_as(_fp)) == 0, \
        E.emul_pick_error().decode()
    if mode.value == UNIFORM:
        return 0, w[:0], m[:0], pmf[:0], cdf[:0]
    return mode.value, w, m, pmf, cdf


def pick_counts(scene, j0=0, j1=Q):
    """how many of the generator's floats (2j + 1) 2^-24, j in [j0, j1), pick each light"""
    counts = np.zeros(n_lights(scene), np.int64)
    E = emul_pick()
    assert E.emul_pick_count(C.byref(scene), j0, j1, counts.ctypes.data_as(C.POINTER(C.c_longlong))) == 0
    return counts


def pick_records(r, light=None):
    """VCM_KAT_LIGHT_PICK input records: the pick's float; a light index for light_pick_prob"""
    r = np.asarray(r, np.float32)
    inp = np.zeros((len(r), KAT), np.float32)
    inp[:, 0] = r
    if light is not None:
        inp[:, 1] = light
    return inp
