"""Version-2 scenes from Python: a SceneBuilder that assembles a `vcm_scene_desc2` (any number of primitives,
materials and lights; include/smallvcm_amd.h) with the library's constructors -- vcm_make_triangle, vcm_make_area_light,
vcm_make_camera, ... each of which computes the derived members exactly as the reference's constructor does
(geometry.hxx:111-123, lights.hxx:116-127, camera.hxx:37-76, scene.hxx:387-398).  Host-only: needs no GPU.

    b = SceneBuilder()
    white = b.material(diffuse=(0.8, 0.8, 0.8))
    b.triangle(p0, p1, p2, white)
    b.emissive_triangle(q0, q1, q2, intensity=(25, 25, 25))
    scene = b.build(position, forward, up, fov_deg=45, resx=512, resy=512)
    r = VertexCM(scene, VertexCM.kVcm, 0.003, 0.75)          # more than 32 primitives: traced through a BVH
"""
import ctypes as C
import math

import numpy as np

from ._abi import (Camera, EnvMap, Light, LightPick, Material, Prim, SceneDesc2, SceneDesc3, SceneDesc4, SceneDesc5, SceneDesc6, ThinLens,
                   PixelFilter, SAMPLERS, with_sampler, with_material_ext, with_projection, PROJECTIONS, PROJ_FISHEYE, FILTER_BOX, FILTER_MAX_RADIUS, LIGHT_PICK_CUSTOM, LIGHT_PICK_MODES, PIXEL_FILTERS)


def _f3(v):
    return (C.c_float * 3)(float(v[0]), float(v[1]), float(v[2]))


class SceneBuilder:
    def __init__(self):
        from .renderer import load_library
        self.L = load_library(require_gpu=False)
        L = self.L
        fp = C.POINTER(C.c_float)
        L.vcm_make_triangle.argtypes = [fp, fp, fp, C.c_int, C.POINTER(Prim)]
        L.vcm_make_triangle.restype = None
        L.vcm_make_sphere.argtypes = [fp, C.c_float, C.c_int, C.POINTER(Prim)]
        L.vcm_make_sphere.restype = None
        L.vcm_make_area_light.argtypes = [fp, fp, fp, fp, C.POINTER(Light)]
        L.vcm_make_area_light.restype = None
        L.vcm_make_directional_light.argtypes = [fp, fp, C.POINTER(Light)]
        L.vcm_make_directional_light.restype = None
        L.vcm_make_point_light.argtypes = [fp, fp, C.POINTER(Light)]
        L.vcm_make_point_light.restype = None
        L.vcm_make_background_light.argtypes = [C.c_float, C.POINTER(Light)]
        L.vcm_make_background_light.restype = None
        L.vcm_make_envmap_light.argtypes = [C.c_float, C.POINTER(Light)]
        L.vcm_make_envmap_light.restype = None
        L.vcm_make_spot_light.argtypes = [fp, fp, fp, C.c_float, C.c_float, C.POINTER(Light)]
        L.vcm_make_spot_light.restype = None
        L.vcm_make_sphere_light.argtypes = [fp, C.c_float, fp, C.POINTER(Light)]
        L.vcm_make_sphere_light.restype = None
        L.vcm_make_material.argtypes = [C.POINTER(Material)]
        L.vcm_make_material.restype = None
        L.vcm_make_camera.argtypes = [fp, fp, fp, C.c_float, C.c_int, C.c_int, C.POINTER(Camera)]
        L.vcm_make_scene_sphere.argtypes = [C.POINTER(Prim), C.c_int, fp, fp, fp]
        L.vcm_make_scene_sphere.restype = None
        self.prims, self.materials, self.mat2light, self.lights = [], [], [], []
        self.background = -1
        self.envmap = None
        self.lens = None
        self.pick = None
        self.filter = None
        self.sampler_kind = None
        self.material_ext = []
        self.camera_model = None

    # ---- materials (materials.hxx:33-65) ----
    def material(self, diffuse=(0, 0, 0), phong=(0, 0, 0), exponent=1.0, mirror=(0, 0, 0), ior=-1.0, ggx=(0, 0, 0), alpha=1.0):
        """ggx, alpha: the optional GGX lobe (include/smallvcm_amd.h vcm_material_ext) -- F0 per channel in [0, 1] and
        the width in [0.01, 1].  build() returns a SceneDesc8 when any material has one."""
        self.material_ext.append(tuple(float(x) for x in ggx) + (float(alpha),))
        m = Material()
        self.L.vcm_make_material(C.byref(m))
        m.diffuse[:] = [float(x) for x in diffuse]
        m.phong[:] = [float(x) for x in phong]
        m.phongExp = float(exponent)
        m.mirror[:] = [float(x) for x in mirror]
        m.ior = float(ior)
        self.materials.append(m)
        self.mat2light.append(-1)
        return len(self.materials) - 1

    # ---- geometry ----
    def triangle(self, p0, p1, p2, material):
        p = Prim()
        self.L.vcm_make_triangle(_f3(p0), _f3(p1), _f3(p2), int(material), C.byref(p))
        self.prims.append(p)
        return len(self.prims) - 1

    def sphere(self, center, radius, material):
        p = Prim()
        self.L.vcm_make_sphere(_f3(center), float(radius), int(material), C.byref(p))
        self.prims.append(p)
        return len(self.prims) - 1

    # ---- lights ----
    def emissive_triangle(self, p0, p1, p2, intensity, diffuse=(0, 0, 0)):
        """a triangle that is an area light: its own material, whose mat2light entry names the light (scene.hxx:333-361)"""
        mat = self.material(diffuse=diffuse)
        light = Light()
        self.L.vcm_make_area_light(_f3(p0), _f3(p1), _f3(p2), _f3(intensity), C.byref(light))
        self.lights.append(light)
        self.mat2light[mat] = len(self.lights) - 1
        return self.triangle(p0, p1, p2, mat)

    def directional_light(self, direction, intensity):
        light = Light()
        self.L.vcm_make_directional_light(_f3(direction), _f3(intensity), C.byref(light))
        self.lights.append(light)

    def point_light(self, position, intensity):
        light = Light()
        self.L.vcm_make_point_light(_f3(position), _f3(intensity), C.byref(light))
        self.lights.append(light)

    def spot_light(self, position, direction, intensity, outer_deg, inner_deg=None):
        """a point light with a cone around `direction` (include/smallvcm_amd.h VCM_LIGHT_SPOT): `intensity` is the radiant
        intensity on the axis, full inside the half-angle inner_deg, smoothly down to zero at outer_deg (0 < outer <=
        180, 0 <= inner <= outer; inner_deg None: a hard edge at outer_deg)"""
        o = float(outer_deg)
        i = o if inner_deg is None else float(inner_deg)
        if not (math.isfinite(o) and 0.0 < o <= 180.0):
            raise ValueError("spot_light: outer_deg must be finite, > 0 and <= 180")
        if not (math.isfinite(i) and 0.0 <= i <= o):
            raise ValueError("spot_light: inner_deg must be finite, >= 0 and <= outer_deg")
        light = Light()
        self.L.vcm_make_spot_light(_f3(position), _f3(direction), _f3(intensity), o, i, C.byref(light))
        self.lights.append(light)

    def sphere_light(self, center, radius, intensity):
        """a sphere that emits the radiance `intensity` outwards (include/smallvcm_amd.h VCM_LIGHT_SPHERE): the sphere
        primitive, a black material of its own and the light its mat2light entry names; returns the primitive's index"""
        r = float(radius)
        if not (math.isfinite(r) and r > 0.0):
            raise ValueError("sphere_light: radius must be finite and > 0")
        mat = self.material()
        light = Light()
        self.L.vcm_make_sphere_light(_f3(center), r, _f3(intensity), C.byref(light))
        self.lights.append(light)
        self.mat2light[mat] = len(self.lights) - 1
        return self.sphere(center, r, mat)

    def background_light(self, scale=1.0):
        light = Light()
        self.L.vcm_make_background_light(float(scale), C.byref(light))
        self.lights.append(light)
        self.background = len(self.lights) - 1

    def envmap_light(self, image, scale=1.0):
        """an environment map as the scene's background: image = float32 [H, W, 3], row 0 = the top of the sky
        (equirectangular, +z up; include/smallvcm_amd.h vcm_envmap).  build() then returns a SceneDesc3."""
        img = np.ascontiguousarray(image, dtype=np.float32)
        if img.ndim != 3 or img.shape[2] != 3:
            raise ValueError("envmap_light: image must be [H, W, 3]")
        light = Light()
        self.L.vcm_make_envmap_light(float(scale), C.byref(light))
        self.lights.append(light)
        self.background = len(self.lights) - 1
        self.envmap = img

    # ---- the camera's lens ----
    def thin_lens(self, aperture_radius, focus_distance):
        """a thin lens instead of the pinhole (include/smallvcm_amd.h vcm_thin_lens): aperture radius >= 0 and focus
        distance > 0 along the camera's forward axis, world units.  build() then returns a SceneDesc4."""
        r, f = float(aperture_radius), float(focus_distance)
        if not (math.isfinite(r) and r >= 0.0):
            raise ValueError("thin_lens: aperture_radius must be finite and >= 0")
        if not (math.isfinite(f) and f > 0.0):
            raise ValueError("thin_lens: focus_distance must be finite and > 0")
        self.lens = (r, f)

    # ---- how lights are chosen ----
    def light_pick(self, mode="power", uniform_mix=0.0, weights=None):
        """how a light is chosen where a path samples one (include/smallvcm_amd.h vcm_light_pick): "uniform", "power"
        (by emitted flux) or "custom" (by `weights`, one per light: finite, >= 0, not all zero), with the share
        uniform_mix in [0, 1] of the uniform choice mixed in.  build() then returns a SceneDesc5."""
        if mode not in LIGHT_PICK_MODES:
            raise ValueError("light_pick: mode must be 'uniform', 'power' or 'custom'")
        a = float(uniform_mix)
        if not (math.isfinite(a) and 0.0 <= a <= 1.0):
            raise ValueError("light_pick: uniform_mix must be finite and in [0, 1]")
        w = None
        if LIGHT_PICK_MODES[mode] == LIGHT_PICK_CUSTOM:
            if weights is None:
                raise ValueError("light_pick: mode 'custom' needs weights")
            w = np.ascontiguousarray(weights, np.float32).reshape(-1)
            if not (np.all(np.isfinite(w)) and np.all(w >= 0) and np.any(w > 0)):
                raise ValueError("light_pick: weights must be finite, >= 0 and not all zero")
        elif weights is not None:
            raise ValueError("light_pick: weights go with mode 'custom'")
        self.pick = (LIGHT_PICK_MODES[mode], a, w)

    # ---- the pixel filter ----
    def pixel_filter(self, kind, radius=0.0):
        """the pixel reconstruction filter (include/smallvcm_amd.h vcm_pixel_filter): "box" (the reference's), "tent" or
        "bspline" with the support `radius` of its offset density in pixels, finite, > 0 and <= 16.  build() then
        returns a SceneDesc6."""
        if kind not in PIXEL_FILTERS:
            raise ValueError("pixel_filter: kind must be 'box', 'tent' or 'bspline'")
        r = float(radius)
        if PIXEL_FILTERS[kind] != FILTER_BOX and not (math.isfinite(r) and 0.0 < r <= FILTER_MAX_RADIUS):
            raise ValueError("pixel_filter: radius must be finite, > 0 and <= %g pixels" % FILTER_MAX_RADIUS)
        self.filter = (PIXEL_FILTERS[kind], r)

    # ---- the sampler ----
    def sampler(self, kind):
        """where the paths' random floats come from (include/smallvcm_amd.h vcm_sampler): "philox" (white noise, the
        default) or "sobol" (the Owen-scrambled Sobol sequence).  build() then returns a SceneDesc7."""
        if kind not in SAMPLERS:
            raise ValueError("sampler: kind must be 'sobol' or 'philox'")
        self.sampler_kind = kind

    # ---- the camera's projection ----
    def projection(self, kind, fov_degrees=0.0):
        """the camera's projection (include/smallvcm_amd.h vcm_camera_model): "perspective" (the pinhole, the default),
        "fisheye" (equidistant; fov_degrees finite and in (0, 360), measured across the image width) or "panorama"
        (equirectangular, 360 x 180 degrees).  The two angular projections keep the camera's position, forward axis and
        raster axes and ignore build()'s fov_deg; a thin lens goes with "perspective" only.  build() then returns a
        SceneDesc9."""
        if kind not in PROJECTIONS:
            raise ValueError("projection: kind must be 'perspective', 'fisheye' or 'panorama'")
        f = float(fov_degrees)
        if PROJECTIONS[kind] == PROJ_FISHEYE and not (math.isfinite(f) and 0.0 < f < 360.0):
            raise ValueError("projection: a fisheye's fov_degrees must be finite and in (0, 360)")
        self.camera_model = (kind, f if PROJECTIONS[kind] == PROJ_FISHEYE else 0.0)

    # ---- the description ----
    def build(self, position, forward, up, fov_deg, resx, resy):
        d = self._build6(position, forward, up, fov_deg, resx, resy)
        if self.sampler_kind is not None:
            d = with_sampler(d, self.sampler_kind)
        if any(e[0] != 0.0 or e[1] != 0.0 or e[2] != 0.0 for e in self.material_ext):
            d = with_material_ext(d, self.material_ext)
        if self.camera_model is not None:
            d = with_projection(d, *self.camera_model)
        return d

    def _build6(self, position, forward, up, fov_deg, resx, resy):
        d = SceneDesc2()
        prims = (Prim * max(len(self.prims), 1))(*self.prims)
        mats = (Material * len(self.materials))(*self.materials)
        m2l = (C.c_int * len(self.mat2light))(*self.mat2light)
        lights = (Light * len(self.lights))(*self.lights)
        d.nPrims, d.prims = len(self.prims), C.cast(prims, C.POINTER(Prim))
        d.nMaterials, d.materials, d.mat2light = len(self.materials), C.cast(mats, C.POINTER(Material)), C.cast(m2l, C.POINTER(C.c_int))
        d.nLights, d.lights = len(self.lights), C.cast(lights, C.POINTER(Light))
        d.backgroundLight = self.background
        r, inv = C.c_float(), C.c_float()
        self.L.vcm_make_scene_sphere(d.prims, d.nPrims, d.sceneCenter, C.byref(r), C.byref(inv))
        d.sceneRadius, d.invSceneRadiusSqr = r.value, inv.value
        if self.L.vcm_make_camera(_f3(position), _f3(forward), _f3(up), float(fov_deg), int(resx), int(resy), C.byref(d.camera)) != 0:
            raise ValueError("bad camera")
        d._keep = (prims, mats, m2l, lights)   # the arrays live as long as the description
        if self.envmap is None and self.lens is None and self.pick is None and self.filter is None:
            return d
        d3 = SceneDesc3()
        d3.base = d
        d3._keep = (d._keep,)
        if self.envmap is not None:
            m = EnvMap()
            m.height, m.width = int(self.envmap.shape[0]), int(self.envmap.shape[1])
            m.rgb = self.envmap.ctypes.data_as(C.POINTER(C.c_float))
            d3.envmap = C.pointer(m)
            d3._keep = (d._keep, self.envmap, m)
        if self.lens is None and self.pick is None and self.filter is None:
            return d3
        d4 = SceneDesc4()
        d4.base = d3
        d4._keep = (d3._keep,)
        if self.lens is not None:
            lens = ThinLens(*self.lens)
            d4.lens = C.pointer(lens)
            d4._keep = (d3._keep, lens)
        if self.pick is None and self.filter is None:
            return d4
        d5 = SceneDesc5()
        d5.base = d4
        d5._keep = (d4._keep,)
        if self.pick is not None:
            mode, mix, w = self.pick
            if w is not None and len(w) != len(self.lights):
                raise ValueError("light_pick: %d weights for %d lights" % (len(w), len(self.lights)))
            pick = LightPick(mode, mix, w.ctypes.data_as(C.POINTER(C.c_float)) if w is not None else None)
            d5.pick = C.pointer(pick)
            d5._keep = (d4._keep, pick, w)
        if self.filter is None:
            return d5
        d6 = SceneDesc6()
        d6.base = d5
        flt = PixelFilter(*self.filter)
        d6.filter = C.pointer(flt)
        d6._keep = (d5._keep, flt)
        return d6
