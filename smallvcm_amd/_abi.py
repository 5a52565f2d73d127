"""ctypes mirror of include/smallvcm_amd.h (the C-ABI PODs).

Field order and sizes must match the header exactly; tests/test_abi.py checks
sizeof() against the values the C library reports.
"""
import ctypes as C

VCM_MAX_PRIMS = 32
VCM_MAX_MATERIALS = 16
VCM_MAX_LIGHTS = 8
VCM_MERGE_RECORD_FLOATS = 13

PRIM_TRIANGLE, PRIM_SPHERE = 0, 1
LIGHT_AREA, LIGHT_DIRECTIONAL, LIGHT_POINT, LIGHT_BACKGROUND = 0, 1, 2, 3
LIGHT_ENVMAP = 4
LIGHT_SPOT, LIGHT_SPHERE = 5, 6
LIGHT_TYPE_NAMES = {LIGHT_AREA: "area", LIGHT_DIRECTIONAL: "directional", LIGHT_POINT: "point", LIGHT_BACKGROUND: "background",
                    LIGHT_ENVMAP: "envmap", LIGHT_SPOT: "spot", LIGHT_SPHERE: "sphere"}

# VertexCM::AlgorithmType (reference src/vertexcm.hxx:182-204)
ALGO_LIGHT_TRACE, ALGO_PPM, ALGO_BPM, ALGO_BPT, ALGO_VCM = 0, 1, 2, 3, 4
ALGO_PATH_TRACE, ALGO_EYE_LIGHT = 5, 6        # PathTracer (src/pathtracer.hxx), EyeLight (src/eyelight.hxx)
ALGO_BY_NAME = {"lt": ALGO_LIGHT_TRACE, "ppm": ALGO_PPM, "bpm": ALGO_BPM,
                "bpt": ALGO_BPT, "vcm": ALGO_VCM, "pt": ALGO_PATH_TRACE, "el": ALGO_EYE_LIGHT}

f3 = C.c_float * 3


class Prim(C.Structure):
    _fields_ = [("type", C.c_int), ("matID", C.c_int),
                ("p0", f3), ("p1", f3), ("p2", f3), ("n", f3)]


class Material(C.Structure):
    _fields_ = [("diffuse", f3), ("phong", f3), ("phongExp", C.c_float),
                ("mirror", f3), ("ior", C.c_float)]


class Light(C.Structure):
    _fields_ = [("type", C.c_int), ("p0", f3), ("e1", f3), ("e2", f3),
                ("frameX", f3), ("frameY", f3), ("frameZ", f3),
                ("intensity", f3), ("invArea", C.c_float), ("scale", C.c_float)]


class Camera(C.Structure):
    _fields_ = [("position", f3), ("forward", f3), ("resolution", C.c_float * 2),
                ("rasterToWorld", C.c_float * 16), ("worldToRaster", C.c_float * 16),
                ("imagePlaneDist", C.c_float)]


class SceneDesc(C.Structure):
    _fields_ = [("nPrims", C.c_int), ("prims", Prim * VCM_MAX_PRIMS),
                ("nMaterials", C.c_int), ("materials", Material * VCM_MAX_MATERIALS),
                ("mat2light", C.c_int * VCM_MAX_MATERIALS),
                ("nLights", C.c_int), ("lights", Light * VCM_MAX_LIGHTS),
                ("backgroundLight", C.c_int),
                ("sceneCenter", f3), ("sceneRadius", C.c_float),
                ("invSceneRadiusSqr", C.c_float),
                ("camera", Camera)]

    def tobytes(self):
        return bytes(memoryview(self))

    @classmethod
    def frombytes(cls, b):
        if len(b) != C.sizeof(cls):
            raise ValueError("scene desc blob has %d bytes, expected %d" % (len(b), C.sizeof(cls)))
        return cls.from_buffer_copy(b)


class SceneDesc2(C.Structure):
    """vcm_scene_desc2: pointer + count for primitives, materials and lights.  The arrays are owned by the Python
    object that built it (SceneBuilder keeps them in `_keep`); the library copies them at vcm_create2."""
    _fields_ = [("nPrims", C.c_int), ("prims", C.POINTER(Prim)),
                ("nMaterials", C.c_int), ("materials", C.POINTER(Material)), ("mat2light", C.POINTER(C.c_int)),
                ("nLights", C.c_int), ("lights", C.POINTER(Light)),
                ("backgroundLight", C.c_int),
                ("sceneCenter", f3), ("sceneRadius", C.c_float), ("invSceneRadiusSqr", C.c_float),
                ("camera", Camera)]


class EnvMap(C.Structure):
    """vcm_envmap: width x height RGB float texels, row 0 = the top (equirectangular, +z up; include/smallvcm_amd.h)"""
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("rgb", C.POINTER(C.c_float))]


class SceneDesc3(C.Structure):
    """vcm_scene_desc3: a version-2 scene and an optional environment map (the light: vcm_make_envmap_light, which
    must be the backgroundLight).  Like SceneDesc2 the arrays are owned by the Python object that built it."""
    _fields_ = [("base", SceneDesc2), ("envmap", C.POINTER(EnvMap))]

    @property
    def camera(self):
        return self.base.camera


class ThinLens(C.Structure):
    """vcm_thin_lens: aperture radius (>= 0; 0 = the pinhole) and focus distance along the camera's forward axis (> 0),
    world units (include/smallvcm_amd.h)"""
    _fields_ = [("apertureRadius", C.c_float), ("focusDistance", C.c_float)]


class SceneDesc4(C.Structure):
    """vcm_scene_desc4: a version-3 scene and an optional thin lens.  Like SceneDesc2 the arrays are owned by the
    Python object that built it."""
    _fields_ = [("base", SceneDesc3), ("lens", C.POINTER(ThinLens))]

    @property
    def camera(self):
        return self.base.base.camera


LIGHT_PICK_UNIFORM, LIGHT_PICK_POWER, LIGHT_PICK_CUSTOM = 0, 1, 2
LIGHT_PICK_MODES = {"uniform": LIGHT_PICK_UNIFORM, "power": LIGHT_PICK_POWER, "custom": LIGHT_PICK_CUSTOM}


class LightPick(C.Structure):
    """vcm_light_pick: how lights are chosen (LIGHT_PICK_UNIFORM / _POWER / _CUSTOM), the share of the uniform choice
    mixed in, and CUSTOM's nLights weights (include/smallvcm_amd.h)"""
    _fields_ = [("mode", C.c_int), ("uniformMix", C.c_float), ("weights", C.POINTER(C.c_float))]


class SceneDesc5(C.Structure):
    """vcm_scene_desc5: a version-4 scene and an optional light-selection setting.  Like SceneDesc2 the arrays are owned
    by the Python object that built it."""
    _fields_ = [("base", SceneDesc4), ("pick", C.POINTER(LightPick))]

    @property
    def camera(self):
        return self.base.base.base.camera


FILTER_BOX, FILTER_TENT, FILTER_BSPLINE = 0, 1, 2
PIXEL_FILTERS = {"box": FILTER_BOX, "tent": FILTER_TENT, "bspline": FILTER_BSPLINE}
FILTER_MAX_RADIUS = 16.0


class PixelFilter(C.Structure):
    """vcm_pixel_filter: the pixel reconstruction filter (FILTER_BOX / _TENT / _BSPLINE) and the support of its offset
    density in pixels (include/smallvcm_amd.h)"""
    _fields_ = [("kind", C.c_int), ("radius", C.c_float)]


class SceneDesc6(C.Structure):
    """vcm_scene_desc6: a version-5 scene and an optional pixel filter.  Like SceneDesc2 the arrays are owned by the
    Python object that built it."""
    _fields_ = [("base", SceneDesc5), ("filter", C.POINTER(PixelFilter))]

    @property
    def camera(self):
        return self.base.base.base.base.camera


SAMPLER_PHILOX, SAMPLER_SOBOL = 0, 1
SAMPLERS = {"philox": SAMPLER_PHILOX, "sobol": SAMPLER_SOBOL}
SAMPLER_NAMES = {v: k for k, v in SAMPLERS.items()}


class Sampler(C.Structure):
    """vcm_sampler: where the paths' random floats come from (SAMPLER_PHILOX: white noise, the default; SAMPLER_SOBOL:
    the Owen-scrambled Sobol sequence; include/smallvcm_amd.h)"""
    _fields_ = [("kind", C.c_int)]


class SceneDesc7(C.Structure):
    """vcm_scene_desc7: a version-6 scene and an optional sampler.  Like SceneDesc2 the arrays are owned by the Python
    object that built it."""
    _fields_ = [("base", SceneDesc6), ("sampler", C.POINTER(Sampler))]

    @property
    def camera(self):
        return self.base.base.base.base.base.camera


def with_sampler(desc, kind):
    """a SceneDesc2 .. SceneDesc6 as a SceneDesc7 with the sampler `kind` ("sobol", "philox" or a SAMPLER_* value; None:
    sampler = NULL); the levels in between get NULL settings.  The result keeps `desc` alive."""
    chain = [SceneDesc2, SceneDesc3, SceneDesc4, SceneDesc5, SceneDesc6, SceneDesc7]
    if isinstance(desc, SceneDesc7):
        desc = desc.base
    if type(desc) not in chain:
        raise TypeError("with_sampler: a SceneDesc2 .. SceneDesc7 is needed (a built-in box: SceneBuilder or a scene file)")
    d = desc
    for cls in chain[chain.index(type(desc)) + 1:]:
        up = cls()
        up.base = d
        up._keep = (getattr(d, "_keep", None), d)
        d = up
    if kind is not None:
        if isinstance(kind, str):
            if kind not in SAMPLERS:
                raise ValueError("sampler: must be 'sobol' or 'philox'")
            kind = SAMPLERS[kind]
        s = Sampler(int(kind))
        d.sampler = C.pointer(s)
        d._keep = d._keep + (s,)
    return d


class MaterialExt(C.Structure):
    """vcm_material_ext: the optional GGX lobe of a material -- F0 per channel in [0, 1] and the width alpha in
    [0.01, 1]; ggx = (0, 0, 0): no lobe (include/smallvcm_amd.h)"""
    _fields_ = [("ggx", C.c_float * 3), ("alpha", C.c_float)]


class SceneDesc8(C.Structure):
    """vcm_scene_desc8: a version-7 scene and one MaterialExt per material.  Like SceneDesc2 the arrays are owned by the
    Python object that built it."""
    _fields_ = [("base", SceneDesc7), ("materialExt", C.POINTER(MaterialExt))]

    @property
    def camera(self):
        return self.base.camera


def with_material_ext(desc, ext):
    """a SceneDesc2 .. SceneDesc7 as a SceneDesc8 with the lobes `ext`: one (r, g, b, alpha) per material, or None
    (materialExt = NULL).  The result keeps `desc` alive."""
    if isinstance(desc, SceneDesc8):
        desc = desc.base
    d7 = desc if isinstance(desc, SceneDesc7) else with_sampler(desc, None)
    d8 = SceneDesc8()
    d8.base = d7
    d8._keep = (getattr(d7, "_keep", None), d7)
    if ext is not None:
        n = int(d7.base.base.base.base.base.nMaterials)
        if len(ext) != n:
            raise ValueError("with_material_ext: %d entries for %d materials" % (len(ext), n))
        arr = (MaterialExt * n)()
        for m, e in enumerate(ext):
            arr[m].ggx[:] = [float(x) for x in e[:3]]
            arr[m].alpha = float(e[3])
        d8.materialExt = C.cast(arr, C.POINTER(MaterialExt))
        d8._keep = d8._keep + (arr,)
    return d8


PROJ_PERSPECTIVE, PROJ_FISHEYE, PROJ_PANORAMA = 0, 1, 2
PROJECTIONS = {"perspective": PROJ_PERSPECTIVE, "fisheye": PROJ_FISHEYE, "panorama": PROJ_PANORAMA}
PROJECTION_NAMES = {v: k for k, v in PROJECTIONS.items()}


class CameraModel(C.Structure):
    """vcm_camera_model: the camera's projection (PROJ_PERSPECTIVE: the pinhole, the default; PROJ_FISHEYE: equidistant,
    fovDegrees in (0, 360) across the image width; PROJ_PANORAMA: equirectangular; include/smallvcm_amd.h)"""
    _fields_ = [("kind", C.c_int), ("fovDegrees", C.c_float)]


class SceneDesc9(C.Structure):
    """vcm_scene_desc9: a version-8 scene and an optional camera model.  Like SceneDesc2 the arrays are owned by the
    Python object that built it."""
    _fields_ = [("base", SceneDesc8), ("model", C.POINTER(CameraModel))]

    @property
    def camera(self):
        return self.base.camera


def with_projection(desc, kind, fov_degrees=0.0):
    """a SceneDesc2 .. SceneDesc8 as a SceneDesc9 with the projection `kind` ("perspective", "fisheye", "panorama" or a
    PROJ_* value; None: model = NULL) and, for a fisheye, its field of view.  The result keeps `desc` alive."""
    if isinstance(desc, SceneDesc9):
        desc = desc.base
    d8 = desc if isinstance(desc, SceneDesc8) else with_material_ext(desc, None)
    d9 = SceneDesc9()
    d9.base = d8
    d9._keep = (getattr(d8, "_keep", None), d8)
    if kind is not None:
        if isinstance(kind, str):
            if kind not in PROJECTIONS:
                raise ValueError("projection: must be 'perspective', 'fisheye' or 'panorama'")
            kind = PROJECTIONS[kind]
        m = CameraModel(int(kind), float(fov_degrees))
        d9.model = C.pointer(m)
        d9._keep = d9._keep + (m,)
    return d9


class DenoiseParams(C.Structure):
    """vcm_denoise_params: a-trous passes (0 .. 12), the three edge-stopping sigmas, and whether the albedo is divided
    out before the first pass and multiplied back after the last (include/smallvcm_amd.h)"""
    _fields_ = [("passes", C.c_int), ("sigmaColor", C.c_float), ("sigmaNormal", C.c_float), ("sigmaDepth", C.c_float),
                ("demodulate", C.c_int)]


class DenoiseParams2(C.Structure):
    """vcm_denoise_params2: vcm_denoise_params, whether the colour stop follows the per-pixel variance, and the number of
    standard deviations it spans (include/smallvcm_amd.h)"""
    _fields_ = DenoiseParams._fields_ + [("varianceGuided", C.c_int), ("sigmaVariance", C.c_float)]


FEATURE_ALBEDO, FEATURE_NORMAL, FEATURE_DEPTH = 0, 1, 2
FEATURES = {"albedo": FEATURE_ALBEDO, "normal": FEATURE_NORMAL, "depth": FEATURE_DEPTH}


class NoiseStats(C.Structure):
    """vcm_noise_stats: the reduction of noise = V / (mean^2 + 0.01) over pixels and channels after `iterations`
    iterations; non-finite elements are counted and left out of mean, max and above (include/smallvcm_amd.h)"""
    _fields_ = [("iterations", C.c_int), ("elements", C.c_longlong), ("above", C.c_longlong), ("nonFinite", C.c_longlong),
                ("mean", C.c_double), ("max", C.c_double)]

    def asdict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


ROBUST_DEFAULT_BUCKETS = 7   # VCM_ROBUST_DEFAULT_BUCKETS


class RobustStats(C.Structure):
    """vcm_robust_stats: what the median-of-means rule decided over the image after `iterations` iterations in `buckets`
    buckets: pixels with a trim t > 0, pixels with a dropped (non-finite) bucket, mean and maximum of the Gini coefficient
    (include/smallvcm_amd.h)"""
    _fields_ = [("iterations", C.c_int), ("buckets", C.c_int), ("pixels", C.c_longlong), ("trimmed", C.c_longlong),
                ("nonFinite", C.c_longlong), ("meanGini", C.c_double), ("maxGini", C.c_double)]

    def asdict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


# VCM_PART_*: the planes of the technique breakdown (vcm_track_parts)
PART_EMISSION, PART_DIRECT, PART_CONNECT, PART_MERGE, PART_LIGHT_TRACE = 0, 1, 2, 3, 4
PART_COUNT = 5
PART_NAMES = ("emission", "direct", "connect", "merge", "lighttrace")
PARTS = {n: i for i, n in enumerate(PART_NAMES)}


class PartsStats(C.Structure):
    """vcm_parts_stats: per plane of the technique breakdown, the luminance summed over the pixels and divided by
    `iterations`; pixels with a non-finite value in any plane are counted and left out (include/smallvcm_amd.h)"""
    _fields_ = [("iterations", C.c_int), ("pixels", C.c_longlong), ("nonFinite", C.c_longlong),
                ("luminance", C.c_double * PART_COUNT)]

    def asdict(self):
        return {"iterations": self.iterations, "pixels": self.pixels, "nonFinite": self.nonFinite,
                "luminance": dict(zip(PART_NAMES, list(self.luminance)))}


# VCM_CURVE_*, VCM_TRANSFER_*, VCM_DISPLAY_*: the display transform (vcm_display)
CURVES = {"clamp": 0, "reinhard": 1, "aces": 2, "hable": 3}
TRANSFERS = {"gamma": 0, "srgb": 1}
DISPLAY_SOURCES = {"framebuffer": 0, "denoised": 1, "robust": 2}
IMAGE_BGR8, IMAGE_RGBE, IMAGE_RGBA8 = 0, 1, 2


class DisplayParams(C.Structure):
    """vcm_display_params: exposure, bloom, tone curve, transfer curve and dither of the display transform
    (include/smallvcm_amd.h)"""
    _fields_ = [("curve", C.c_int), ("whitePoint", C.c_float), ("exposureEV", C.c_float),
                ("autoExposure", C.c_int), ("key", C.c_float), ("lowPercentile", C.c_float), ("highPercentile", C.c_float),
                ("minEV", C.c_float), ("maxEV", C.c_float),
                ("transfer", C.c_int), ("gamma", C.c_float),
                ("bloomStrength", C.c_float), ("bloomLevels", C.c_int),
                ("dither", C.c_int), ("ditherSeed", C.c_uint)]


class DisplayStats(C.Structure):
    """vcm_display_stats: the exposure the histogram picked and the multiplier applied, what the histogram counted and left
    out, and the channels that reached 1.0 after the curve (include/smallvcm_amd.h)"""
    _fields_ = [("autoEV", C.c_double), ("multiplier", C.c_double), ("logAvgLuminance", C.c_double),
                ("counted", C.c_longlong), ("zero", C.c_longlong), ("nonFinite", C.c_longlong),
                ("clampedLow", C.c_longlong), ("clampedHigh", C.c_longlong), ("clipped", C.c_longlong)]

    def asdict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class CompareParams(C.Structure):
    """vcm_compare_params: the epsilon of the relative error, the peak of PSNR and SSIM, the threshold `above` counts
    beyond, SSIM and the error map on or off (include/smallvcm_amd.h)"""
    _fields_ = [("relEpsilon", C.c_float), ("peak", C.c_float), ("threshold", C.c_float), ("ssim", C.c_int), ("writeMap", C.c_int)]


class CompareStats(C.Structure):
    """vcm_compare_stats: an image against a reference image -- the counts, mse, relMse, mae, maxAbs and where, psnr, ssim
    (include/smallvcm_amd.h)"""
    _fields_ = [("iterations", C.c_int), ("pixels", C.c_longlong), ("nonFinite", C.c_longlong), ("above", C.c_longlong),
                ("ssimWindows", C.c_longlong), ("maxPixel", C.c_longlong),
                ("mse", C.c_double), ("relMse", C.c_double), ("mae", C.c_double), ("maxAbs", C.c_double), ("psnr", C.c_double),
                ("ssim", C.c_double)]

    def asdict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class Stats(C.Structure):
    _fields_ = [("lightVertices", C.c_longlong), ("gridVertices", C.c_longlong),
                ("lightRays", C.c_longlong), ("cameraRays", C.c_longlong),
                ("shadowRays", C.c_longlong), ("mergeQueries", C.c_longlong),
                ("mergeCandidates", C.c_longlong), ("mergeAccepted", C.c_longlong),
                ("connections", C.c_longlong), ("lightSplats", C.c_longlong),
                ("msLight", C.c_float), ("msGrid", C.c_float),
                ("msCamera", C.c_float), ("msTotal", C.c_float),
                ("msLightKernel", C.c_float), ("msCameraKernel", C.c_float),
                ("msMergeKernel", C.c_float), ("msQuerySort", C.c_float), ("msConnectKernels", C.c_float),
                ("radius", C.c_float)]

    def asdict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


# Scene::BoxMask (reference src/scene.hxx:112-126)
kLightCeiling, kLightSun, kLightPoint, kLightBackground = 1, 2, 4, 8
kLargeMirrorSphere, kLargeGlassSphere, kSmallMirrorSphere, kSmallGlassSphere = 16, 32, 64, 128
kGlossyFloor = 256
kBothSmallSpheres = kSmallMirrorSphere | kSmallGlassSphere

# g_SceneConfigs (reference src/config.hxx:146-151)
SCENE_CONFIGS = [
    kGlossyFloor | kBothSmallSpheres | kLightSun,
    kGlossyFloor | kLargeMirrorSphere | kLightCeiling,
    kGlossyFloor | kBothSmallSpheres | kLightPoint,
    kGlossyFloor | kBothSmallSpheres | kLightBackground,
]
