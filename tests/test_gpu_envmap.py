"""The environment-map light on the GPU: the kernels of the env-map kinds (SceneRectsE / SceneListE / SceneBvhE) against the host
emulation of the same device functions (tests/host_emul_envmap), bit for bit -- framebuffer, random-number tape and
workload counters -- for every algorithm and kind, wavefront and strict order; the light functions one call at a
time (vcm_debug_kat); and vcm_render's scene-file path against the Python one."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import envmap_lib as el
from smallvcm_amd.renderer import HipBackend, VertexCM

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPLAT_ALGOS = (0, 3, 4)
STAT_KEYS = ("lightVertices", "lightRays", "cameraRays", "shadowRays", "mergeQueries", "mergeCandidates",
             "mergeAccepted", "connections", "lightSplats")
_fp = C.POINTER(C.c_float)


def _scene(resx=20, resy=14):
    return el.builtin_with_envmap(el.sky(48, 24, sun=(0.55, 0.2), sun_size=2, sun_value=(30.0, 27.0, 22.0)), scale=1.3,
                                  resx=resx, resy=resy)


@pytest.mark.parametrize("strict", [False, True])
@pytest.mark.parametrize("kind", ["rects", "list", "bvh"])
@pytest.mark.parametrize("algo", range(7))
def test_gpu_equals_host_emulation(monkeypatch, algo, kind, strict):
    """scene 3's box takes the SceneRectsE kernels; with general pow forced, SceneListE; with a BVH forced, SceneBvhE"""
    if kind == "bvh":
        monkeypatch.setenv("SMALLVCM_AMD_FORCE_BVH", "1")   # read when the scene is built: both sides
    if kind == "list":
        monkeypatch.setenv("SMALLVCM_AMD_GENERAL_POW", "1")
    d = _scene()
    emu = el.Emul3(d, algo, seed=77)
    r = VertexCM(d, algo, 0.003, 0.75, 77, strict_order=strict)
    r.mMinPathLength, r.mMaxPathLength = 0, 10
    for it in range(2):
        emu.run_iteration(it, 0, 10)
        r.RunIteration(it)
        lc, cc = r.backend.rng_counts()
        elc, ecc = emu.counts()
        assert np.array_equal(lc, elc), "light tape"
        assert np.array_equal(cc, ecc), "camera tape"
        se, sg = emu.stats(), r.stats()
        for k in STAT_KEYS:
            assert se[k] == sg[k], (k, se[k], sg[k])
    gpu, host = r.framebuffer_sum(), emu.framebuffer()
    assert np.count_nonzero(host) > 0
    if strict and algo in SPLAT_ALGOS:   # strict mode splats with fp32 atomics: their order is not defined
        assert np.all(np.abs(gpu - host) <= 2e-5 * np.abs(host) + 2e-7), float(np.abs(gpu - host).max())
    else:
        assert np.array_equal(gpu.view(np.uint32), host.view(np.uint32))
    r.close()


@pytest.mark.parametrize("op", [4, 5, 6])   # light_emit, light_illuminate, light_radiance
def test_device_light_functions_equal_the_host(op):
    d = _scene(32, 32)
    n = 50000
    rng = np.random.default_rng(op)
    inp = np.zeros((n, 16), np.float32)
    inp[:, 0] = d.base.backgroundLight
    if op == 6:
        v = rng.normal(size=(n, 3))
        inp[:, 1:4] = v / np.linalg.norm(v, axis=1, keepdims=True)
    elif op == 5:
        inp[:, 1:4] = rng.random((n, 3)) - 0.5
        inp[:, 4:6] = rng.random((n, 2))
    else:
        inp[:, 1:5] = rng.random((n, 4))
    b = HipBackend(d, 4, 0.003, 0.75, 1234)
    b.L.vcm_debug_kat.argtypes = [C.c_void_p, C.c_int, C.c_int, _fp, _fp]
    dev = np.zeros_like(inp)
    assert b.L.vcm_debug_kat(b.ctx, op, n, inp.ctypes.data_as(_fp), dev.ctypes.data_as(_fp)) == 0, b.L.vcm_last_error()
    b.close()
    host = el.kat3(d, op, inp)
    assert np.count_nonzero(host[:, 0]) > 0.9 * n
    assert np.array_equal(dev.view(np.uint32), host.view(np.uint32))


def test_vcm_render_scene_file_equals_python(tmp_path):
    from smallvcm_amd.scene_file import load_scene
    img = el.sky(32, 16)
    (tmp_path / "sky.pfm").write_bytes(b"PF\n32 16\n-1\n" + img[::-1].astype("<f4").tobytes())
    (tmp_path / "room.obj").write_text(
        "mtllib room.mtl\nv -1 -1 0\nv 1 -1 0\nv 1 1 0\nv -1 1 0\nv -0.3 -0.3 0\nv 0.3 -0.3 0\nv 0 0.2 0.6\n"
        "usemtl white\nf 1 2 3 4\nusemtl red\nf 5 6 7\n")
    (tmp_path / "room.mtl").write_text("newmtl white\nKd 0.8 0.8 0.8\nnewmtl red\nKd 0.7 0.2 0.2\nKs 0.2 0.2 0.2\nNs 40\n")
    (tmp_path / "s.vcmscene").write_text("obj room.obj\ncamera 0 -4 2  0 1 -0.45  0 0 1  50\nlight envmap sky.pfm 1.5\n")
    res, iters, seed = (24, 18), 2, 4321
    exe = os.path.join(ROOT, "smallvcm_amd", "host", "vcm_render")
    out = tmp_path / "out.pfm"
    p = subprocess.run([exe, "--scene-file", str(tmp_path / "s.vcmscene"), "-a", "vcm", "-i", str(iters), "--res", str(res[0]),
                        str(res[1]), "--seed", str(seed), "-o", str(out)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    data = out.read_bytes()
    cli = np.frombuffer(data[len(b"PF\n%d %d\n-1\n" % res):], np.float32).reshape(res[1], res[0], 3)
    d = load_scene(tmp_path / "s.vcmscene", *res)
    r = VertexCM(d, 4, 0.003, 0.75, seed)
    r.mMaxPathLength = 10
    for it in range(iters):
        r.RunIteration(it)
    py = r.GetFramebuffer()
    r.close()
    assert np.count_nonzero(py) > 0
    assert np.array_equal(cli.view(np.uint32), py.view(np.uint32))
