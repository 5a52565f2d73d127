"""Scene files (include/smallvcm_amd.h: vcm_scene_load): `.vcmscene` / Wavefront `.obj` + `.mtl` -> SceneDesc2,
SceneDesc3 when the file names an environment map (`light envmap <file> <scale>`), SceneDesc4 when it names a thin
lens (`lens <apertureRadius> <focusDistance>`), SceneDesc5 when it says how lights are chosen (`lightpick
uniform|power [uniformMix]`), SceneDesc6 when it names a pixel filter (`filter tent|bspline <radius>`), SceneDesc7
when it names a sampler (`sampler sobol|philox`), SceneDesc8 when a material in use has a `Pr` line in its `.mtl`
(a GGX lobe), or SceneDesc9 when it names a projection (`projection fisheye <fovDeg>|panorama`).
The parsing happens in the library (smallvcm_amd/csrc/scene_file.cpp documents the format); this is the ctypes binding.

    scene = load_scene("tests/scenes/bumpy_room.vcmscene", 1024, 1024)
    r = VertexCM(scene, VertexCM.kVcm, 0.003, 0.75)
"""
import ctypes as C

from ._abi import SceneDesc2, SceneDesc3, SceneDesc4, SceneDesc5, SceneDesc6, SceneDesc7, SceneDesc8, SceneDesc9


class _Handle:
    def __init__(self, L, h):
        self.L, self.h = L, h

    def __del__(self):
        if self.h:
            self.L.vcm_scene_file_free(self.h)
            self.h = None


def load_scene(path, resx, resy):
    """-> SceneDesc2, SceneDesc3 with an env map, SceneDesc4 with a lens, SceneDesc5 with a `lightpick` directive,
    SceneDesc6 with a `filter` directive, SceneDesc7 with a `sampler` directive, SceneDesc8 with a `Pr` material, or
    SceneDesc9 with a `projection` directive (the
    arrays it points to live as long as the returned object)"""
    from .renderer import load_library
    L = load_library(require_gpu=False)
    L.vcm_scene_load.restype = C.c_void_p
    L.vcm_scene_load.argtypes = [C.c_char_p, C.c_int, C.c_int]
    L.vcm_scene_file_desc.restype = C.POINTER(SceneDesc2)
    L.vcm_scene_file_desc.argtypes = [C.c_void_p]
    L.vcm_scene_file_desc3.restype = C.POINTER(SceneDesc3)
    L.vcm_scene_file_desc3.argtypes = [C.c_void_p]
    L.vcm_scene_file_desc4.restype = C.POINTER(SceneDesc4)
    L.vcm_scene_file_desc4.argtypes = [C.c_void_p]
    L.vcm_scene_file_desc5.restype = C.POINTER(SceneDesc5)
    L.vcm_scene_file_desc5.argtypes = [C.c_void_p]
    L.vcm_scene_file_desc6.restype = C.POINTER(SceneDesc6)
    L.vcm_scene_file_desc6.argtypes = [C.c_void_p]
    L.vcm_scene_file_desc7.restype = C.POINTER(SceneDesc7)
    L.vcm_scene_file_desc7.argtypes = [C.c_void_p]
    L.vcm_scene_file_desc8.restype = C.POINTER(SceneDesc8)
    L.vcm_scene_file_desc8.argtypes = [C.c_void_p]
    L.vcm_scene_file_desc9.restype = C.POINTER(SceneDesc9)
    L.vcm_scene_file_desc9.argtypes = [C.c_void_p]
    L.vcm_scene_file_free.argtypes = [C.c_void_p]
    L.vcm_scene_file_free.restype = None
    L.vcm_scene_load_error.restype = C.c_char_p
    h = L.vcm_scene_load(str(path).encode(), int(resx), int(resy))
    if not h:
        raise ValueError("smallvcm_amd: cannot load %s: %s" % (path, L.vcm_scene_load_error().decode()))
    d4 = L.vcm_scene_file_desc4(h).contents
    d3 = L.vcm_scene_file_desc3(h).contents
    d5 = L.vcm_scene_file_desc5(h).contents
    d6 = L.vcm_scene_file_desc6(h).contents
    d7 = L.vcm_scene_file_desc7(h).contents
    d8 = L.vcm_scene_file_desc8(h).contents
    d9 = L.vcm_scene_file_desc9(h).contents
    if d9.model:
        d = SceneDesc9.from_buffer_copy(d9)   # the struct (pointers into the handle's arrays and settings, the camera model among them)
    elif d8.materialExt:
        d = SceneDesc8.from_buffer_copy(d8)   # the struct (pointers into the handle's arrays and settings, the ext table among them)
    elif d7.sampler:
        d = SceneDesc7.from_buffer_copy(d7)   # the struct (pointers into the handle's arrays, map, lens, pick, filter and sampler)
    elif d6.filter:
        d = SceneDesc6.from_buffer_copy(d6)   # the struct (pointers into the handle's arrays, map, lens, pick and filter)
    elif d5.pick:
        d = SceneDesc5.from_buffer_copy(d5)   # the struct (pointers into the handle's arrays, map, lens and pick)
    elif d4.lens:
        d = SceneDesc4.from_buffer_copy(d4)   # the struct (pointers into the handle's arrays, map and lens)
    elif d3.envmap:
        d = SceneDesc3.from_buffer_copy(d3)   # the struct (pointers into the handle's arrays and map)
    else:
        d = SceneDesc2.from_buffer_copy(L.vcm_scene_file_desc(h).contents)
    d._keep = _Handle(L, h)
    return d
