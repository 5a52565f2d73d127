"""The technique breakdown on the GPU: the planes of a context with vcm_track_parts on -- k_resolve_parts of
smallvcm_amd/csrc/vcm_parts.hip and the second pass of the splat kernels -- against the wavefront host emulation
(tests/host_emul_parts), bit for bit; the statistic, the refusals and the command-line host."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import parts_lib as pl
from smallvcm_amd._abi import (ALGO_BPM, ALGO_BPT, ALGO_EYE_LIGHT, ALGO_LIGHT_TRACE, ALGO_PATH_TRACE, ALGO_PPM, ALGO_VCM,
                               PART_COUNT, PART_LIGHT_TRACE, PART_NAMES, PartsStats)
from smallvcm_amd.renderer import HipBackend, cornell_scene, load_library

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VCM_RENDER = os.path.join(ROOT, "smallvcm_amd", "host", "vcm_render")
_fp = C.POINTER(C.c_float)
ALGOS = [ALGO_LIGHT_TRACE, ALGO_PPM, ALGO_BPM, ALGO_BPT, ALGO_VCM]
K = 3
CAP = 2          # workgroups of the small grid: CAP * 256 lanes
_cache = {}


def set_kind(kind, monkeypatch):
    if kind == "list":
        monkeypatch.setenv("SMALLVCM_AMD_NO_ONEPLANE", "1")   # read when the scene is built, on both sides
        monkeypatch.setenv("SMALLVCM_AMD_GENERAL_POW", "1")
    if kind == "bvh":
        monkeypatch.setenv("SMALLVCM_AMD_FORCE_BVH", "1")


def emulated(algo, scene_id, res, lengths=(0, 10), kind="rects"):
    """the emulation after K iterations (under the switches of `kind`, which the caller has set), once per case"""
    key = (algo, scene_id, res, lengths, kind)
    if key not in _cache:
        _cache[key] = pl.rendered(cornell_scene(scene_id, *res), algo, K, *lengths)
    return _cache[key]


def backend(scene_id, res, algo=ALGO_VCM, tracked=True, **kw):
    b = HipBackend(cornell_scene(scene_id, *res), algo, pl.RADIUS, 0.75, 1234, **kw)
    if tracked:
        b.track_parts()
    return b


def device_planes(b):
    """[PART_COUNT, H, W, 3]: the raw sums"""
    return np.stack([b.part(i, 1.0) for i in range(PART_COUNT)])


def check_against_emulation(algo, scene_id, res, lengths=(0, 10), kind="rects"):
    e = emulated(algo, scene_id, res, lengths, kind)
    b = backend(scene_id, res, algo)
    try:
        for it in range(K):
            b.run_iteration(it, *lengths)
        fb, planes, st = b.framebuffer_sum(), device_planes(b), b.parts_stats()
    finally:
        b.close()
    assert pl.same_bits(fb, e.framebuffer())
    for i in range(PART_COUNT):
        assert pl.same_bits(planes[i], e.planes()[i]), PART_NAMES[i]
    return e, planes, st


@pytest.fixture
def small_grid():
    """the kernels' grids capped at CAP workgroups, so that a few hundred pixels reach the grid-stride paths"""
    L = load_library()
    L.vcm_debug_parts_max_blocks(CAP)
    yield CAP
    L.vcm_debug_parts_max_blocks(0)


# ---------------- a tracked context = the emulation, bit for bit ----------------
@pytest.mark.parametrize("res", [(20, 14), (67, 45)])
@pytest.mark.parametrize("kind", ["rects", "list", "bvh"])
@pytest.mark.parametrize("algo", ALGOS)
def test_planes_and_framebuffer_equal_the_emulation(algo, kind, res, monkeypatch):
    """20 x 14: a partial workgroup; 67 x 45: an odd row length across twelve workgroups"""
    set_kind(kind, monkeypatch)
    e, planes, st = check_against_emulation(algo, 1, res, kind=kind)
    for part in pl.FILLS[algo]:
        assert planes[part].max() > 0, part


@pytest.mark.parametrize("scene_id, lengths", [(3, (0, 10)), (2, (0, 10)), (1, (2, 5))])
def test_background_light_point_light_and_short_paths(scene_id, lengths):
    check_against_emulation(ALGO_VCM, scene_id, (20, 14), lengths)


def test_tracking_does_not_disturb_the_framebuffer():
    b, plain = backend(1, (20, 14)), backend(1, (20, 14), tracked=False)
    try:
        for it in range(K):
            b.run_iteration(it, 0, 10)
            plain.run_iteration(it, 0, 10)
            assert pl.same_bits(b.framebuffer_sum(), plain.framebuffer_sum()), it
    finally:
        b.close()
        plain.close()


def test_the_grid_stride_paths_equal_the_emulation(small_grid):
    """67 x 45 = 3015 pixels on 2 x 256 lanes: every lane of k_resolve_parts and of the statistic owns five or six"""
    e, planes, st = check_against_emulation(ALGO_VCM, 1, (67, 45))
    assert st == e.stats(small_grid)


def test_long_splat_lists_take_the_wave_per_pixel_path(tmp_path):
    """SMALLVCM_AMD_SPLAT_LONG=8 (read once per process: a child) sends every list above 8 splats through
    k_splat_apply_long, for the framebuffer and for the LIGHT_TRACE plane"""
    e = emulated(ALGO_VCM, 1, (20, 14))
    assert e.max_list > 8
    out = str(tmp_path / "planes.npy")
    code = r'''
import sys
import numpy as np
sys.path.insert(0, %r)
import parts_lib as pl
from smallvcm_amd.renderer import HipBackend, cornell_scene
b = HipBackend(cornell_scene(1, 20, 14), 4, pl.RADIUS, 0.75, 1234)
b.track_parts()
for it in range(%d):
    b.run_iteration(it, 0, 10)
np.save(%r, np.stack([b.framebuffer_sum()] + [b.part(i, 1.0) for i in range(5)]))
b.close()
''' % (os.path.join(ROOT, "tests"), K, out)
    env = dict(os.environ, SMALLVCM_AMD_SPLAT_LONG="8", PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-600:]
    got = np.load(out)
    assert pl.same_bits(got[0], e.framebuffer())
    assert pl.same_bits(got[1:], e.planes())


# ---------------- what the planes must satisfy ----------------
@pytest.mark.parametrize("algo", ALGOS)
def test_empty_planes_are_zero_and_light_tracing_is_the_framebuffer(algo):
    b = backend(1, (20, 14), algo)
    try:
        for it in range(K):
            b.run_iteration(it, 0, 10)
        fb, planes = b.framebuffer_sum(), device_planes(b)
    finally:
        b.close()
    for part in range(PART_COUNT):
        assert planes[part].any() == (part in pl.FILLS[algo]), part
    if algo == ALGO_LIGHT_TRACE:
        assert pl.same_bits(planes[PART_LIGHT_TRACE], fb)


def test_part_device_is_read_part_with_w_one():
    import torch

    class DevImage:
        def __init__(self, ptr, n):
            self.__cuda_array_interface__ = {"shape": (n, 4), "typestr": "<f4", "data": (ptr, False), "version": 2}

    b = backend(1, (20, 14))
    try:
        for it in range(K):
            b.run_iteration(it, 0, 10)
        for part, scale in ((0, 1.0), (4, 1.0 / K), (2, 0.25)):
            ptr = b.part_device(part, scale)
            b.synchronize()
            img = torch.as_tensor(DevImage(ptr, b.N), device="cuda").cpu().numpy()
            assert pl.same_bits(img[:, :3], b.part(part, scale).reshape(-1, 3))
            assert (img[:, 3] == 1).all()
        assert pl.same_bits(b.part("merge"), b.part(3, 1.0 / K))        # None = 1 / iterations
        assert set(b.parts()) == set(PART_NAMES)
    finally:
        b.close()


def test_the_statistic_is_reproducible_and_equals_the_emulation():
    e = emulated(ALGO_VCM, 1, (67, 45))
    runs = []
    for _ in range(2):
        b = backend(1, (67, 45))
        try:
            for it in range(K):
                b.run_iteration(it, 0, 10)
            runs.append((b.parts_stats(), b.parts_stats()))
        finally:
            b.close()
    ref = e.stats()
    for st in (runs[0][0], runs[0][1], runs[1][0]):
        assert st == ref
        assert all(np.float64(st["luminance"][n]).tobytes() == np.float64(ref["luminance"][n]).tobytes() for n in PART_NAMES)
    assert ref["iterations"] == K and ref["pixels"] == 67 * 45 and ref["nonFinite"] == 0 and min(ref["luminance"].values()) > 0


def test_clear_resets_the_planes():
    """after a clear and one more iteration the planes hold that iteration alone: under light tracing the LIGHT_TRACE plane
    is the (cleared) framebuffer bit for bit, under VCM the planes add up to it within the rounding of m addends"""
    st = PartsStats()
    for algo in (ALGO_LIGHT_TRACE, ALGO_VCM):
        b = backend(1, (20, 14), algo)
        try:
            b.run_iteration(0, 0, 10)
            assert device_planes(b).any()
            b.clear_framebuffer()
            assert b.L.vcm_get_parts_stats(b.ctx, C.byref(st)) == -1 and b"no iteration" in b.L.vcm_last_error()
            b.run_iteration(1, 0, 10)
            fb, planes = b.framebuffer_sum(), device_planes(b)
            assert b.parts_stats()["iterations"] == 1
            if algo == ALGO_LIGHT_TRACE:
                assert pl.same_bits(planes[PART_LIGHT_TRACE], fb) and fb.any()
            else:
                m = b.stats()["lightSplats"] + 4 * (1 + 10 * 12)
                S = planes.astype(np.float64).sum(axis=0)
                assert (np.abs(S - fb) <= 2.0 * m * 2.0 ** -24 * fb).all() and fb.any()
        finally:
            b.close()


# ---------------- refusals ----------------
def test_refusals_of_a_context():
    b = backend(1, (24, 18), tracked=False)
    try:
        L = b.L
        out = np.zeros((18, 24, 3), np.float32)
        st, dev = PartsStats(), C.c_void_p()
        # off: the readers say so
        for rc in (L.vcm_read_part(b.ctx, 0, 1.0, out.ctypes.data_as(_fp)), L.vcm_part_device(b.ctx, 0, 1.0, C.byref(dev)),
                   L.vcm_get_parts_stats(b.ctx, C.byref(st))):
            assert rc == -1 and b"vcm_track_parts is off" in L.vcm_last_error()
        b.track_parts()
        # before the first iteration
        for rc in (L.vcm_read_part(b.ctx, 0, 1.0, out.ctypes.data_as(_fp)), L.vcm_part_device(b.ctx, 0, 1.0, C.byref(dev)),
                   L.vcm_get_parts_stats(b.ctx, C.byref(st))):
            assert rc == -1 and b"no iteration" in L.vcm_last_error()
        # strict order on a tracked context; an iteration that would not be wavefront
        assert L.vcm_set_strict_order(b.ctx, 1) == -1 and b"vcm_track_parts is on" in L.vcm_last_error()
        assert L.vcm_begin_iteration(b.ctx, 0, 0, 32) == -1 and b"would not be wavefront" in L.vcm_last_error()
        b.run_iteration(0, 0, 10)
        # a part outside 0 .. 4, a scale that is not finite
        for part in (-1, 5):
            assert L.vcm_read_part(b.ctx, part, 1.0, out.ctypes.data_as(_fp)) == -1 and b"part must be 0 .. 4" in L.vcm_last_error()
            assert L.vcm_part_device(b.ctx, part, 1.0, C.byref(dev)) == -1 and b"part must be 0 .. 4" in L.vcm_last_error()
        for scale in (float("inf"), float("nan")):
            assert L.vcm_read_part(b.ctx, 0, scale, out.ctypes.data_as(_fp)) == -1 and b"not finite" in L.vcm_last_error()
            assert L.vcm_part_device(b.ctx, 0, scale, C.byref(dev)) == -1 and b"not finite" in L.vcm_last_error()
        # switching on with iterations in the framebuffer
        b.track_parts(False)
        assert L.vcm_track_parts(b.ctx, 1) == -1 and b"holds iterations" in L.vcm_last_error()
        b.clear_framebuffer()
        b.track_parts()
    finally:
        b.close()


def test_strict_order_path_tracing_and_eye_light_are_refused():
    b = backend(1, (24, 18), tracked=False)
    try:
        b.set_strict_order(True)
        assert b.L.vcm_track_parts(b.ctx, 1) == -1 and b"strict order" in b.L.vcm_last_error()
        b.set_strict_order(False)
        b.track_parts()
    finally:
        b.close()
    for algo in (ALGO_PATH_TRACE, ALGO_EYE_LIGHT):
        b = backend(1, (24, 18), algo, tracked=False)
        try:
            assert b.L.vcm_track_parts(b.ctx, 1) == -1 and b"no technique split" in b.L.vcm_last_error()
        finally:
            b.close()


def test_a_sharded_context_is_refused_in_the_words_of_the_denoiser():
    b = backend(1, (24, 18), tracked=False, rank=1, world=3)
    try:
        L = b.L
        pv, st = C.c_void_p(), PartsStats()
        buf = np.zeros((18, 24, 3), np.float32)
        for rc in (L.vcm_track_parts(b.ctx, 1), L.vcm_part_device(b.ctx, 0, 1.0, C.byref(pv)),
                   L.vcm_read_part(b.ctx, 0, 1.0, buf.ctypes.data_as(_fp)), L.vcm_get_parts_stats(b.ctx, C.byref(st))):
            assert rc == -1
            assert b"sharded context: its framebuffer is a shard of the image" in L.vcm_last_error()
    finally:
        b.close()


# ---------------- the command-line host ----------------
def read_pfm(path):
    with open(path, "rb") as f:
        assert f.readline() == b"PF\n"
        w, h = map(int, f.readline().split())
        assert f.readline() == b"-1\n"
        return np.frombuffer(f.read(), np.float32).reshape(h, w, 3)


def test_vcm_render_writes_the_five_parts(tmp_path):
    import json
    prefix = str(tmp_path / "p")
    r = subprocess.run([VCM_RENDER, "-s", "1", "-a", "vcm", "-i", str(K), "--res", "20", "14", "--radius-factor", str(pl.RADIUS),
                        "--parts", prefix, "--json"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-400:]
    b = backend(1, (20, 14))
    try:
        for it in range(K):
            b.run_iteration(it, 0, 10)
        for name in PART_NAMES:
            assert pl.same_bits(read_pfm("%s_%s.pfm" % (prefix, name)), b.part(name)), name
        st = b.parts_stats()
    finally:
        b.close()
    assert json.loads(r.stdout.strip().splitlines()[-1])["parts"] == st
