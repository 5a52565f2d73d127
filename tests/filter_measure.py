"""The measurements of DESIGN.md "Pixel filter" (not a test; needs a GPU).

Timing: one VCM iteration of scene 1 at 2048 x 2048 and 512 x 512, host clock around an iteration that ends in a
synchronise, median of 20 after 5 warm-up iterations, one process per run; the runs alternate between the builds and the
filters and every one is repeated, so that the spread of a configuration is seen beside the differences.  `--other-lib
PATH` adds a second build of the library (the parent commit's, for "filter off against the parent") to the rotation.

Error: scene 3 under path tracing at 64 x 64, 16 iterations, box / tent r = 1.5 / B-spline r = 2, the image and the image
through vcm_denoise (the defaults), against 1000 iterations of the host emulation of the SAME filter -- a filtered
image converges to another target than the box's -- over the pixels beside a geometric edge (where a first-hit guide
differs from a neighbour's) and over the whole image.  The box reference is tests/golden/denoise_ref_s3_pt_64_1000.npy,
the other two tests/golden/filter_ref_s3_pt_64_1000_<filter>.npy.

    python tests/filter_measure.py [--other-lib PATH] [--rounds N] [--out FILE]
"""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

FILTERS = {"box": None, "tent1.5": ("tent", 1.5), "bspline2": ("bspline", 2.0)}


def scene(scene_id, res, flt):
    from smallvcm_amd.renderer import cornell_scene
    if flt is None:
        return cornell_scene(scene_id, res, res)   # the version-1 description: what bench.py renders
    import filter_lib as fl
    import lens_lib as ll
    from smallvcm_amd._abi import PIXEL_FILTERS, SCENE_CONFIGS
    return fl.with_filter(ll.builtin3(SCENE_CONFIGS[scene_id], res, res), PIXEL_FILTERS[flt[0]], flt[1])


def child(res, name):
    from smallvcm_amd._abi import ALGO_VCM
    from smallvcm_amd.renderer import HipBackend
    b = HipBackend(scene(1, res, FILTERS[name]), ALGO_VCM, 0.003, 0.75, 1234)
    ts = []
    for it in range(25):
        b.synchronize()
        t = time.perf_counter()
        b.run_iteration(it, 0, 10)
        b.synchronize()
        ts.append((time.perf_counter() - t) * 1e3)
    st = b.stats()
    b.close()
    ts = ts[5:]
    print("RESULT %.4f %.4f %.4f %.4f %.4f" % (np.median(ts), min(ts), max(ts), st["msLightKernel"], st["msCameraKernel"]))


def timing(args, say):
    builds = [("this", None)] + ([("other", args.other_lib)] if args.other_lib else [])
    for res in (2048, 512):
        rows = {}
        for rnd in range(args.rounds):
            for name in FILTERS:
                for tag, lib in builds:
                    if tag == "other" and name != "box":
                        continue   # the other build is there for the filter-off comparison
                    env = dict(os.environ)
                    if lib:
                        env["SMALLVCM_AMD_LIB"] = lib
                    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(res), name], env=env,
                                       capture_output=True, text=True, timeout=600)
                    if p.returncode != 0:
                        say("res %d %s %s: FAILED (exit %d) %s" % (res, tag, name, p.returncode, p.stderr[-300:]))
                        return False
                    v = [float(x) for x in [l for l in p.stdout.splitlines() if l.startswith("RESULT")][0].split()[1:]]
                    rows.setdefault((tag, name), []).append(v)
                    say("res %d round %d build %-5s filter %-8s iteration median %.4f ms (min %.4f max %.4f) = %.1f Mpaths/s; "
                        "last iteration: light kernel %.4f ms, camera kernel %.4f ms" %
                        (res, rnd, tag, name, v[0], v[1], v[2], 2.0 * res * res / v[0] / 1e3, v[3], v[4]))
        for (tag, name), vs in rows.items():
            med = [v[0] for v in vs]
            say("res %d SUMMARY build %-5s filter %-8s medians of %d runs: %s ms; min %.4f max %.4f (spread %.2f %%)" %
                (res, tag, name, len(med), " ".join("%.4f" % m for m in med), min(med), max(med),
                 100.0 * (max(med) - min(med)) / min(med)))
    return True


def error(say):
    import denoise_lib as dl
    from smallvcm_amd._abi import ALGO_PATH_TRACE
    from smallvcm_amd.renderer import HipBackend
    res, spp = 64, 16
    refs = {"box": "denoise_ref_s3_pt_64_1000.npy", "tent1.5": "filter_ref_s3_pt_64_1000_tent1.5.npy",
            "bspline2": "filter_ref_s3_pt_64_1000_bspline2.npy"}
    edge = None
    for name, flt in FILTERS.items():
        ref = np.load(os.path.join(HERE, "golden", refs[name]))
        out = {}
        for seed in (1234, 1235, 1236, 1237):
            b = HipBackend(scene(3, res, flt), ALGO_PATH_TRACE, 0.003, 0.75, seed)
            for it in range(spp):
                b.run_iteration(it, 0, 10)
            noisy = b.framebuffer_sum() / np.float32(spp)
            den = b.denoise(1.0 / spp)
            if edge is None:   # the guides are unfiltered, the same for every filter
                n, z = b.feature("normal"), b.feature("depth")
                g = np.concatenate([n, z[..., None] / max(float(z.max()), 1e-6)], axis=2)
                e = np.zeros((res, res), bool)
                dx = np.abs(g[:, 1:] - g[:, :-1]).max(axis=2) > 0.1
                dy = np.abs(g[1:, :] - g[:-1, :]).max(axis=2) > 0.1
                e[:, 1:] |= dx; e[:, :-1] |= dx; e[1:, :] |= dy; e[:-1, :] |= dy
                edge = e
            b.close()
            for what, img in (("image", noisy), ("denoised", den)):
                out.setdefault(what + " edges", []).append(dl.rel_mse(img[edge], ref[edge]))
                out.setdefault(what + " all", []).append(dl.rel_mse(img, ref))
        say("error scene 3 PT 64x64 %d iterations filter %-8s (%d edge pixels of %d; mean of 4 seeds of the relative MSE "
            "against 1000 iterations of the same filter): %s" %
            (spp, name, int(edge.sum()), res * res, "; ".join("%s %.5f" % (k, float(np.mean(v))) for k, v in out.items())))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", nargs=2)
    ap.add_argument("--other-lib")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out")
    ap.add_argument("--skip-timing", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(int(args.child[0]), args.child[1])
    log = open(args.out, "w") if args.out else None

    def say(s):
        print(s, flush=True)
        if log:
            log.write(s + "\n")
            log.flush()
    if not (args.skip_timing or timing(args, say)):
        sys.exit(1)
    error(say)


if __name__ == "__main__":
    main()
