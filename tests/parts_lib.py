"""The technique breakdown for the tests (test infrastructure): the ctypes binding of
tests/host_emul_parts/libemul_parts.so, built on demand -- a serial host build of the product's wavefront functions and
of the split of smallvcm_amd/csrc/vcm_parts.h."""
import ctypes as C
import os
import subprocess

import numpy as np

from smallvcm_amd._abi import PART_COUNT, PART_NAMES, PartsStats, SceneDesc

HERE = os.path.dirname(os.path.abspath(__file__))
EMUL_DIR = os.path.join(HERE, "host_emul_parts")
DEFAULT_MAX_BLOCKS = 2048    # VCM_PARTS_DEFAULT_MAX_BLOCKS
RADIUS = 0.05                # the radius factor of the merging cases: the default 0.003 accepts 0 - 4 photons in three
                             # iterations at 20 x 14, 0.05 accepts 200 - 1400 in every built-in scene
# the planes an algorithm fills (by VCM_PART_* index); every other plane stays exactly zero
FILLS = {0: {4}, 1: {0, 3}, 2: {0, 3}, 3: {0, 1, 2, 4}, 4: {0, 1, 2, 3, 4}}
_fp = C.POINTER(C.c_float)
_E = None


def emul_parts():
    """build (make: a no-op when up to date) and load the emulation"""
    global _E
    if _E is None:
        subprocess.run(["make", "-C", EMUL_DIR], check=True, stdout=subprocess.DEVNULL)
        E = C.CDLL(os.path.join(EMUL_DIR, "libemul_parts.so"))
        E.emul_parts_create.restype = C.c_void_p
        E.emul_parts_create.argtypes = [C.POINTER(SceneDesc), C.c_int, C.c_float, C.c_float, C.c_int]
        E.emul_parts_destroy.argtypes = [C.c_void_p]
        E.emul_parts_run_iteration.argtypes = [C.c_void_p, C.c_int, C.c_uint, C.c_uint]
        E.emul_parts_get_framebuffer.argtypes = [C.c_void_p, _fp]
        E.emul_parts_get_planes.argtypes = [C.c_void_p, _fp]
        E.emul_parts_get_splat_info.argtypes = [C.c_void_p, C.POINTER(C.c_longlong)]
        E.emul_parts_stats.argtypes = [C.c_void_p, C.c_int, C.POINTER(PartsStats)]
        E.vcm_scene_cornell.argtypes = [C.c_int, C.c_int, C.c_uint, C.POINTER(SceneDesc)]
        _E = E
    return _E


def same_bits(a, b):
    return np.ascontiguousarray(a, np.float32).tobytes() == np.ascontiguousarray(b, np.float32).tobytes()


class PartsEmul:
    """what a context with vcm_track_parts on computes, on the host"""

    def __init__(self, scene, algo, radius_factor=RADIUS, radius_alpha=0.75, seed=1234):
        self.E = emul_parts()
        self.h = self.E.emul_parts_create(C.byref(scene), algo, radius_factor, radius_alpha, seed)
        assert self.h, "emul_parts_create refused the scene or the algorithm"
        self.resx, self.resy = int(scene.camera.resolution[0]), int(scene.camera.resolution[1])
        self.iterations = 0
        self.max_list = 0        # the longest per-pixel splat list of any iteration

    def __del__(self):
        if getattr(self, "h", None):
            self.E.emul_parts_destroy(self.h)
            self.h = None

    def run_iteration(self, it, min_len=0, max_len=10):
        assert self.E.emul_parts_run_iteration(self.h, it, min_len, max_len) == 0
        self.iterations += 1
        self.max_list = max(self.max_list, self.splat_info()[1])

    def framebuffer(self):
        out = np.zeros((self.resy, self.resx, 3), np.float32)
        self.E.emul_parts_get_framebuffer(self.h, out.ctypes.data_as(_fp))
        return out

    def planes(self):
        """[PART_COUNT, H, W, 3]: the raw sums"""
        out = np.zeros((PART_COUNT, self.resy, self.resx, 3), np.float32)
        self.E.emul_parts_get_planes(self.h, out.ctypes.data_as(_fp))
        return out

    def parts(self):
        return dict(zip(PART_NAMES, self.planes()))

    def splat_info(self):
        """(splats of the last iteration, its longest per-pixel list, the most splats of any iteration)"""
        o = (C.c_longlong * 3)()
        self.E.emul_parts_get_splat_info(self.h, o)
        return tuple(o)

    def stats(self, max_blocks=DEFAULT_MAX_BLOCKS):
        st = PartsStats()
        assert self.E.emul_parts_stats(self.h, max_blocks, C.byref(st)) == 0
        return st.asdict()


def rendered(scene, algo, iterations=3, min_len=0, max_len=10, radius_factor=RADIUS):
    e = PartsEmul(scene, algo, radius_factor)
    for it in range(iterations):
        e.run_iteration(it, min_len, max_len)
    return e
