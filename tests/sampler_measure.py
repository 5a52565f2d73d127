"""The measurements of DESIGN.md "Sampler" (not a test; needs a GPU).

Error: 64 x 64 images after 16, 64 and 256 iterations against a reference of 2^14 iterations of the PHILOX sampler (the
default path, seed 90210, which no test uses), for scene 3 under the path tracer and under VCM -- the two references
committed as tests/golden/sampler_ref_s3_<algo>_64_16384.npy -- and for scene 1 under BPT and the path tracer (rendered
here, not kept).  Per case and iteration count: R = mean MSE(Sobol) / mean MSE(Philox) over seeds 1..8, and P = the same
ratio between Philox seeds 9..16 and Philox seeds 1..8, the spread of the yardstick itself.

    python tests/sampler_measure.py --make-refs DIR      # writes the two reference images into DIR
    python tests/sampler_measure.py [--refs DIR] [--out FILE]
"""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

REF_SEED, REF_ITERS, RES = 90210, 1 << 14, 64
COUNTS = (16, 64, 256)
CASES = (("s3_pt", 3, 5), ("s3_vcm", 3, 4), ("s1_bpt", 1, 3), ("s1_pt", 1, 5))   # name, scene, algorithm
GOLDEN = os.path.join(HERE, "golden")


def ref_path(directory, name):
    return os.path.join(directory, "sampler_ref_%s_%d_%d.npy" % (name, RES, REF_ITERS))


def render(scene_id, algo, sampler, seed, counts):
    """the mean image after each of `counts` iterations (increasing) of one renderer"""
    import lens_lib as ll
    import sampler_lib as sl
    from smallvcm_amd.renderer import VertexCM
    d = sl.builtin_sampler(sampler, mask=ll.SCENE_CONFIGS[scene_id], resx=RES, resy=RES)
    r = VertexCM(d, algo, 0.003, 0.75, seed)
    r.mMinPathLength, r.mMaxPathLength = 0, 10
    out = []
    for it in range(max(counts)):
        r.RunIteration(it)
        if it + 1 in counts:
            out.append(r.framebuffer_sum().astype(np.float64) / (it + 1))
    r.close()
    return out


def reference(scene_id, algo):
    import sampler_lib as sl
    return render(scene_id, algo, sl.PHILOX, REF_SEED, (REF_ITERS,))[0].astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--make-refs")
    ap.add_argument("--refs", default=GOLDEN)
    ap.add_argument("--out")
    args = ap.parse_args()
    import sampler_lib as sl
    if args.make_refs:
        os.makedirs(args.make_refs, exist_ok=True)
        for name, scene_id, algo in CASES[:2]:
            np.save(ref_path(args.make_refs, name), reference(scene_id, algo))
            print("wrote", ref_path(args.make_refs, name), flush=True)
        return
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say("MSE against %d Philox iterations (seed %d), %d x %d, 8 seeds per set; R = Sobol / Philox, P = Philox 9..16 / Philox 1..8"
        % (REF_ITERS, REF_SEED, RES, RES))
    say("%-8s %5s %12s %12s %12s %7s %7s %9s" % ("case", "iters", "mse philox", "mse philox'", "mse sobol", "R", "P", "t"))
    for name, scene_id, algo in CASES:
        ref = np.load(ref_path(args.refs, name)) if os.path.exists(ref_path(args.refs, name)) else reference(scene_id, algo)
        ref = ref.astype(np.float64)
        mse = {"a": [], "b": [], "s": []}
        for seed in range(1, 9):
            mse["a"].append([np.mean((im - ref) ** 2) for im in render(scene_id, algo, sl.PHILOX, seed, COUNTS)])
            mse["b"].append([np.mean((im - ref) ** 2) for im in render(scene_id, algo, sl.PHILOX, seed + 8, COUNTS)])
            mse["s"].append([np.mean((im - ref) ** 2) for im in render(scene_id, algo, sl.SOBOL, seed, COUNTS)])
        a, b, s = (np.mean(np.array(mse[k]), axis=0) for k in "abs")
        for c, n in enumerate(COUNTS):
            R, P = s[c] / a[c], b[c] / a[c]
            gate = R < 1.0 / max(1.0, P) ** 2
            say("%-8s %5d %12.5e %12.5e %12.5e %7.3f %7.3f %9s" % (name, n, a[c], b[c], s[c], R, P,
                                                                    ("%.3f" % np.sqrt(R * max(1.0, P))) if gate else "no gate"))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
