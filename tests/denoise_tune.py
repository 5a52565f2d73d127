"""The sweep that chose vcm_denoise_defaults (DESIGN.md "Denoising"; not a test): scenes 0, 1 and 3, path tracing and
VCM, 64 x 64, 4 iterations of the host emulation, denoised over a grid of the three sigmas and compared with a
1000-iteration render of the same emulation.  Prints the mean relative MSE of every grid point and the winner.

    python tests/denoise_tune.py [cache_dir]      (the references are kept in cache_dir as .npy, default /tmp)
"""
import itertools
import os
import sys
from concurrent.futures import ProcessPoolExecutor

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SCENES, ALGOS, RES, SPP, REF_SPP = (0, 1, 3), (("pt", 5), ("vcm", 4)), 64, 4, 1000
GRID_C, GRID_N, GRID_Z = (0.25, 1.0, 4.0, 16.0, 64.0), (8.0, 32.0, 128.0), (0.02, 0.05, 0.1, 0.3, 1.0)


def render(job):
    import denoise_lib as dl
    scene, algo, n, seed = job
    return dl.Emul(dl.box(scene, RES, RES), algo, seed).run(n).mean()


def reference(cache, scene, name, algo):
    path = os.path.join(cache, "denoise_ref_s%d_%s_%d_%d.npy" % (scene, name, RES, REF_SPP))
    if not os.path.exists(path):
        np.save(path, render((scene, algo, REF_SPP, 777)))
    return np.load(path)


def main():
    import denoise_lib as dl
    from smallvcm_amd._abi import DenoiseParams
    cache = sys.argv[1] if len(sys.argv) > 1 else "/tmp"
    cases = [(s, name, algo) for s in SCENES for name, algo in ALGOS]
    with ProcessPoolExecutor(6) as ex:
        refs = list(ex.map(_ref, [(cache,) + c for c in cases]))
        noisy = list(ex.map(render, [(s, algo, SPP, 1234) for s, _, algo in cases]))
    feats = {s: dl.features(dl.box(s, RES, RES)) for s in SCENES}
    base = [dl.rel_mse(n, r) for n, r in zip(noisy, refs)]
    print("noisy relMSE:", " ".join("s%d/%s %.4f" % (c[0], c[1], b) for c, b in zip(cases, base)))
    best = None
    for sc, sn, sz in itertools.product(GRID_C, GRID_N, GRID_Z):
        p = DenoiseParams(5, sc, sn, sz, 1)
        errs = [dl.rel_mse(dl.denoise(n, feats[c[0]][1], feats[c[0]][0], p), r) for c, n, r in zip(cases, noisy, refs)]
        m = float(np.mean(errs))
        print("sigma c %-5g n %-5g z %-5g  mean relMSE %.5f  ratios %s" % (sc, sn, sz, m, " ".join("%.2f" % (b / e) for b, e in zip(base, errs))))
        if best is None or m < best[0]:
            best = (m, sc, sn, sz)
    print("winner: sigmaColor %g sigmaNormal %g sigmaDepth %g (mean relMSE %.5f; noisy %.5f)" % (best[1], best[2], best[3], best[0], float(np.mean(base))))


def _ref(a):
    return reference(*a)


if __name__ == "__main__":
    main()
