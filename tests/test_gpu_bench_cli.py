"""bench.py on the command line: a plain run measures the headline alone, `--steps` sets the timed steps that
`ms_per_step` describes, `--dump-outputs` writes what the timed steps computed (the farm's framebuffer, bit for bit what
vcm_farm_render returns for the same window), and `--full` brings back the legs a plain run leaves out."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RES, STEPS, WARMUP = 256, 3, 1


def _bench(tmp_path, *extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--scene", "1", "--algo", "vcm", "--res", str(RES),
           "--steps", str(STEPS), "--warmup", str(WARMUP)] + list(extra)
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT,
                       env=dict(os.environ, SMALLVCM_AMD_BENCH_DETAIL=str(tmp_path / "bench_detail.json")))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1 and len(lines[0]) < 4096
    return json.loads(lines[0])


def test_plain_run_is_the_headline_alone_and_dumps_its_framebuffer(tmp_path):
    d = _bench(tmp_path, "--dump-outputs", str(tmp_path / "out"))
    assert d["steps"] == STEPS and d["warmup"] == WARMUP and d["n_gpus"] == 1
    assert d["unit"] == "Mpaths/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
    assert d["value"] > 0 and d["ms_per_step"] > 0
    # value and ms_per_step describe the same K timed steps: Mpaths/s = 2 N / (ms per step)
    assert abs(d["value"] - 2.0 * RES * RES / (d["ms_per_step"] / 1e3) / 1e6) < 0.01 * d["value"]
    for leg in ("configs", "cpu_baseline", "dropin", "host_cross_check"):
        assert leg not in d, leg
    fb = np.load(str(tmp_path / "out" / "framebuffer.npy"))
    assert fb.dtype == np.float32 and fb.shape == (RES, RES, 3) and fb.max() > 0
    assert np.allclose(fb.mean(axis=(0, 1)), d["image_mean"], atol=1e-5)
    from smallvcm_amd import farm as F
    from smallvcm_amd._abi import ALGO_BY_NAME
    from smallvcm_amd.renderer import cornell_scene
    r = F.farm_render(cornell_scene(1, RES, RES), ALGO_BY_NAME["vcm"], iterations=STEPS, ranks=1, shards=1, inflight=1, devices=[0],
                      warmup=WARMUP, same_window=True, collectives="threads")
    assert np.array_equal(fb.view(np.uint32), r["image"].view(np.uint32))


def test_full_run_adds_the_other_legs(tmp_path):
    d = _bench(tmp_path, "--full", "--cpu-baseline", "port", "--no-traffic")
    assert d["steps"] == STEPS and d["value"] > 0 and d["ms_per_step"] > 0
    assert d["host_cross_check"]["value"] > 0
    assert d["cpu_baseline"]["value"] > 0
