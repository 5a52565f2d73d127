"""The sweep behind vcm_denoise_defaults2 (DESIGN.md "Variance"; not a test): scenes 0, 1 and 3, path tracing and VCM,
64 x 64, 4 and 16 iterations of the host emulation with variance tracking, denoised with the fixed colour stop
(vcm_denoise_defaults) and with the variance-guided stop over a grid of sigmaVariance, and compared with a 1000-iteration
render of the same emulation.  Prints the relative MSE of every case and the ratio fixed / guided.

    python tests/variance_tune.py [cache_dir]      (the references are kept in cache_dir as .npy, default /tmp; the three
                                                    of tests/golden/denoise_ref_* may be copied there)
"""
import os
import sys
from concurrent.futures import ProcessPoolExecutor

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import denoise_tune as dt  # noqa: E402

SPPS, GRID_V, SEED = (4, 16), (1.0, 2.0, 4.0, 8.0, 16.0), 1234


def case(job):
    import denoise_lib as dl
    import variance_lib as vl
    from smallvcm_amd._abi import DenoiseParams2
    cache, scene, name, algo, spp = job
    ref = dt.reference(cache, scene, name, algo)
    sc = dl.box(scene, dt.RES, dt.RES)
    g, a = dl.features(sc)
    r = vl.TrackedEmul(sc, algo, SEED).run(spp)
    fb = r.framebuffer()
    row = [dl.rel_mse(r.emul.mean(), ref)]
    for guided, sv in [(0, 1.0)] + [(1, v) for v in GRID_V]:
        p = DenoiseParams2(5, 16.0, 32.0, 0.05, 1, guided, sv)
        out = vl.denoise2(fb, a, g, r.mom, vl.var_factor_context(1.0 / spp, spp), p, scale=1.0 / spp)
        row.append(dl.rel_mse(out, ref))
    return (scene, name, spp), row


def main():
    cache = sys.argv[1] if len(sys.argv) > 1 else "/tmp"
    jobs = [(cache, s, name, algo, spp) for s in dt.SCENES for name, algo in dt.ALGOS for spp in SPPS]
    with ProcessPoolExecutor(6) as ex:
        rows = list(ex.map(case, jobs))
    print("case            noisy    fixed   " + "  ".join("sv=%-5g" % v for v in GRID_V) + "   fixed / guided")
    for (s, name, spp), row in rows:
        print("s%d %-3s %2d spp  %.5f  %.5f  " % (s, name, spp, row[0], row[1]) + "  ".join("%.5f" % e for e in row[2:]) +
              "   " + " ".join("%.2f" % (row[1] / e) for e in row[2:]))
    for i, v in enumerate(GRID_V):
        print("sigmaVariance %-4g mean relMSE %.5f (fixed %.5f), geometric mean of fixed / guided %.3f" %
              (v, np.mean([r[2 + i] for _, r in rows]), np.mean([r[1] for _, r in rows]),
               float(np.exp(np.mean([np.log(r[1] / r[2 + i]) for _, r in rows])))))


if __name__ == "__main__":
    main()
