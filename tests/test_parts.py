"""The technique breakdown without a GPU: the wavefront host emulation (tests/host_emul_parts, the functions of
smallvcm_amd/csrc/vcm_core.h and vcm_parts.h on one host thread) is tied to the strict-order emulation the other tests
rest on, and its five planes are checked against each other and against its framebuffer."""
import os
import subprocess

import numpy as np
import pytest

import parts_lib as pl
from emul_lib import Emul
from smallvcm_amd._abi import ALGO_BPM, ALGO_BPT, ALGO_LIGHT_TRACE, ALGO_PPM, ALGO_VCM, PART_LIGHT_TRACE
from smallvcm_amd.renderer import cornell_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VCM_RENDER = os.path.join(ROOT, "smallvcm_amd", "host", "vcm_render")
ALGOS = [ALGO_LIGHT_TRACE, ALGO_PPM, ALGO_BPM, ALGO_BPT, ALGO_VCM]
LENGTHS = [(0, 10), (2, 5)]
RES = (20, 14)
K = 3
_cache = {}


def rendered(algo, scene_id, lengths=(0, 10)):
    """the emulation after K iterations, computed once per case and left unchanged"""
    key = (algo, scene_id, lengths)
    if key not in _cache:
        _cache[key] = pl.rendered(cornell_scene(scene_id, *RES), algo, K, *lengths)
    return _cache[key]


@pytest.mark.parametrize("lengths", LENGTHS)
@pytest.mark.parametrize("scene_id", [0, 1, 2, 3])
@pytest.mark.parametrize("algo", ALGOS)
def test_the_wavefront_emulation_equals_the_strict_one(algo, scene_id, lengths):
    e = rendered(algo, scene_id, lengths)
    ref = Emul(cornell_scene(scene_id, *RES), algo, pl.RADIUS)
    for it in range(K):
        ref.run_iteration(it, *lengths)
    fb = e.framebuffer()
    assert np.isfinite(fb).all() and fb.max() > 0
    assert pl.same_bits(fb, ref.framebuffer())


@pytest.mark.parametrize("scene_id", [0, 1, 2, 3])
@pytest.mark.parametrize("algo", ALGOS)
def test_planes_an_algorithm_cannot_fill_are_zero(algo, scene_id):
    e = rendered(algo, scene_id)
    planes = e.planes()
    for part in range(5):
        if part not in pl.FILLS[algo]:
            assert not planes[part].any(), part
        elif scene_id == 1:
            assert planes[part].max() > 0, part
    if algo == ALGO_LIGHT_TRACE:
        assert pl.same_bits(planes[PART_LIGHT_TRACE], e.framebuffer())


@pytest.mark.parametrize("lengths", LENGTHS)
@pytest.mark.parametrize("scene_id", [0, 1, 2, 3])
@pytest.mark.parametrize("algo", ALGOS)
def test_the_planes_sum_to_the_framebuffer(algo, scene_id, lengths):
    """two orders over the same m non-negative addends differ by at most 2 m 2^-24 of their sum: loose on purpose, it
    catches a missing or doubled class of addends (the bit comparisons are the sharp test)"""
    e = rendered(algo, scene_id, lengths)
    max_len = lengths[1]
    m = K * (e.splat_info()[2] + 4 * (1 + max_len * (max_len + 2)))
    fb = e.framebuffer().astype(np.float64)
    S = e.planes().astype(np.float64).sum(axis=0)
    assert (e.planes() >= 0).all()
    assert (np.abs(S - fb) <= 2.0 * m * 2.0 ** -24 * fb).all()


def test_the_statistic_is_the_luminance_of_the_planes():
    e = rendered(ALGO_VCM, 1)
    st = e.stats()
    planes = e.planes().astype(np.float64).reshape(5, -1, 3)
    lum = (planes @ np.array([0.212671, 0.715160, 0.072169])).sum(axis=1) / K
    got = np.array(list(st["luminance"].values()))
    assert st["iterations"] == K and st["pixels"] == RES[0] * RES[1] and st["nonFinite"] == 0
    assert (np.abs(got - lum) <= 1e-12 * lum).all() and (got > 0).all()
    assert e.stats(2) != {} and np.abs(np.array(list(e.stats(2)["luminance"].values())) - lum).max() <= 1e-12 * lum.max()


def test_vcm_render_refuses_parts_for_path_tracing_before_any_device_call():
    r = subprocess.run([VCM_RENDER, "-s", "1", "-a", "pt", "-i", "1", "--res", "20", "14", "--parts", "/nonexistent/p"],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--parts wants a VertexCM algorithm" in r.stderr
    r = subprocess.run([VCM_RENDER, "-s", "1", "-a", "vcm", "-i", "1", "--renderers", "2", "--parts", "/nonexistent/p"],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--parts wants one renderer on one GPU" in r.stderr
