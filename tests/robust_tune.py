"""The sweep behind VCM_ROBUST_DEFAULT_BUCKETS (DESIGN.md "Robust estimate"; not a test): scene 1 under path tracing and
scene 3 under path tracing and VCM, 64 x 64, seeds 11 .. 44, 16 and 64 iterations of the host emulation, the iterations
bucketed for M = 3, 5, 7, 9 and 15 at once, against the committed 1000-iteration renders of the same emulation
(tests/golden/denoise_ref_*).  Prints the relative MSE of the mean and of the estimate for every case, seed and M, and for
every M the mean over the cases of log(estimate / mean): the lowest one is the default.  The trim rule is not swept: it is
the specification.  With --variants it also prints the always-median and never-trim variants of the float64 restatement
for the default M (the figures beside the bounds of tests/test_robust.py).

    python tests/robust_tune.py [--variants]
"""
import os
import sys
from concurrent.futures import ProcessPoolExecutor

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

BUCKETS, SEEDS, LOOKS, RES = (3, 5, 7, 9, 15), (11, 22, 33, 44), (16, 64), 64
CASES = ((1, "pt"), (3, "pt"), (3, "vcm"))


def reference(scene, name):
    return np.load(os.path.join(HERE, "golden", "denoise_ref_s%d_%s_%d_1000.npy" % (scene, name, RES)))


def case(job):
    """one render of max(LOOKS) iterations -> {(look, M): relMSE}, M = 0 for the mean; with variants also (look, "median")
    and (look, "never") for the default M"""
    import denoise_lib as dl
    import robust_lib as rl
    from smallvcm_amd._abi import ALGO_PATH_TRACE, ALGO_VCM
    scene, name, seed, variants = job
    ref = reference(scene, name)
    e = dl.Emul(dl.box(scene, RES, RES), ALGO_PATH_TRACE if name == "pt" else ALGO_VCM, seed)
    images = {M: rl.new_images(RES * RES, M) for M in BUCKETS}
    row = {}
    for k in range(1, max(LOOKS) + 1):
        e.run(1)
        fb = e.framebuffer()
        for M in BUCKETS:
            rl.update(fb, k, *images[M])
        if k in LOOKS:
            row[(k, 0)] = dl.rel_mse(e.mean(), ref)
            for M in BUCKETS:
                row[(k, M)] = dl.rel_mse(rl.resolve(*images[M], k)[:, :3].reshape(RES, RES, 3), ref)
            if variants:
                for v in ("median", "never"):
                    rgb = rl.resolve64(*images[rl.DEFAULT_BUCKETS], k, trim=v)[0]
                    row[(k, v)] = dl.rel_mse(rgb.reshape(RES, RES, 3), ref)
    return (scene, name, seed), row


def main():
    variants = "--variants" in sys.argv[1:]
    jobs = [(s, name, seed, variants) for s, name in CASES for seed in SEEDS]
    with ProcessPoolExecutor(min(12, len(jobs))) as ex:
        rows = dict(ex.map(case, jobs))
    cols = list(BUCKETS) + (["median", "never"] if variants else [])
    logs = {M: [] for M in BUCKETS}
    print("case                    mean      " + "  ".join("M=%-7s" % m for m in cols))
    for s, name in CASES:
        for k in LOOKS:
            for seed in SEEDS:
                row = rows[(s, name, seed)]
                print("s%d %-3s %2d it seed %d  %.5f   " % (s, name, k, seed, row[(k, 0)]) + "  ".join("%.5f  " % row[(k, m)] for m in cols))
            ratios = {m: [rows[(s, name, seed)][(k, m)] / rows[(s, name, seed)][(k, 0)] for seed in SEEDS] for m in cols}
            print("s%d %-3s %2d it estimate / mean: " % (s, name, k) +
                  "; ".join("M=%s %.3f .. %.3f" % (m, min(r), max(r)) for m, r in ratios.items()))
            for M in BUCKETS:
                logs[M].append(float(np.mean(np.log(ratios[M]))))
    for M in BUCKETS:
        print("M = %-2d mean over the six cases of log(estimate / mean) %.4f (geometric mean of the ratio %.4f)" %
              (M, np.mean(logs[M]), np.exp(np.mean(logs[M]))))
    print("lowest: M = %d" % min(BUCKETS, key=lambda M: np.mean(logs[M])))


if __name__ == "__main__":
    main()
