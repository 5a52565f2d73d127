"""The widened kernels (environment map, thin lens, light selection) at real launch shapes: 161 x 97 (61 workgroups plus
one lane), 256 x 256 and 3 x 2200 -- where the chunked path refill, the radix sort's multi-tile plan, a hash grid of
thousands of cells, k_merge_pairs' 64-wide rounds, the long-splat kernel and the side streams differ from the trivial
case -- for every kind of scene the launches instantiate them for: rectangles, quads, the list, the BVH of a real mesh,
and the general-pow kinds SceneBvhG / SceneListE / SceneBvhE.  The device against the host emulation of the same device
functions (tests/host_emul_pick), framebuffer bits, both tapes and the nine counters -- the contract of
tests/test_gpu_light_pick.py, with its strict-mode splat tolerance; the kind each context took is asserted through
vcm_debug_context_info, and the emulation's own numbers are asserted non-trivial for every case."""
import time

import numpy as np
import pytest

import capacity_lib as cl
import pick_lib as pl
from smallvcm_amd.renderer import VertexCM

pytestmark = pytest.mark.gpu
_emulation = {"seconds": 0.0, "iterations": 0}
MAX_EMULATED_ITERATIONS = 400   # the whole module: "a few hundred"


@pytest.fixture(scope="module", autouse=True)
def _report_the_emulation_time():
    """after the module's last test, whichever tests ran: what the checker cost"""
    yield
    print("\nhost emulation: %d iterations, %.1f s" % (_emulation["iterations"], _emulation["seconds"]))
    assert _emulation["iterations"] <= MAX_EMULATED_ITERATIONS


def _compare(d, algo, strict, expect, seed=77, iters=2):
    emu = pl.Emul5(d, algo, seed=seed)
    r = VertexCM(d, algo, 0.003, 0.75, seed, strict_order=strict)
    r.mMinPathLength, r.mMaxPathLength = 0, 10
    total = dict.fromkeys(cl.COUNTERS, 0)
    for it in range(iters):
        t0 = time.perf_counter()
        emu.run_iteration(it, 0, 10)
        _emulation["seconds"] += time.perf_counter() - t0
        _emulation["iterations"] += 1
        r.RunIteration(it)
        lc, cc = r.backend.rng_counts()
        elc, ecc = emu.counts()
        assert np.array_equal(lc, elc), ("light tape", it)
        assert np.array_equal(cc, ecc), ("camera tape", it)
        se, sg = emu.stats(), r.stats()
        for k in cl.COUNTERS:
            assert se[k] == sg[k], (it, k, se[k], sg[k])
            total[k] += se[k]
    info = cl.context_info(r.backend)
    gpu, host = r.framebuffer_sum(), emu.framebuffer()
    r.close()
    cl.check_checker(host, total, algo)
    for k, v in expect.items():
        assert info[k] == v, (k, info)
    if strict and algo in cl.SPLATTING:   # strict mode splats with fp32 atomics: their order is not defined
        assert np.all(np.abs(gpu - host) <= 2e-5 * np.abs(host) + 2e-7), float(np.abs(gpu - host).max())
    else:
        assert np.array_equal(gpu.view(np.uint32), host.view(np.uint32))


def _expect(kind, env=True, lens=True, pick=True):
    rects, quads, nodes, int_phong, envmap = cl.KIND_FLAGS[kind]
    return {"rects": rects, "quads": quads, "nodes": nodes, "intPhong": int_phong, "envMap": int(bool(envmap and env)),
            "lens": int(lens), "pick": int(pick)}


@pytest.mark.parametrize("kind,shape,algo,strict", cl.widened_cases())
def test_widened_kernels_at_size_equal_the_host_emulation(monkeypatch, kind, shape, algo, strict):
    for k, v in cl.KIND_ENV.get(kind, {}).items():
        monkeypatch.setenv(k, v)                 # read when the scene is built: both sides
    d = cl.widened_scene(kind, shape)
    assert pl.n_lights(d) > 4
    want = _expect(kind)
    if kind in ("bvh", "bvhG", "bvhE"):
        want["nPrims"] = 2 * 21 * 21 + (6 if kind == "bvhE" else 10) + 2
        assert want["nPrims"] > 800
    _compare(d, algo, strict, want)


@pytest.mark.parametrize("kind,features", cl.FEATURES_ALONE)
@pytest.mark.parametrize("algo", [cl.VCM, cl.PATH_TRACE])
def test_each_feature_alone_at_161_by_97(kind, features, algo):
    _compare(cl.widened_scene(kind, cl.SHAPES[0], **features), algo, False, _expect(kind, **features))


def test_the_case_table_stays_within_the_emulation_budget():
    """by count, whichever tests are selected: two iterations per case"""
    assert 2 * (len(cl.widened_cases()) + 2 * len(cl.FEATURES_ALONE)) <= MAX_EMULATED_ITERATIONS
