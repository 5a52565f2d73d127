"""The measurement of DESIGN.md "Microfacet materials" (not a test; needs a GPU): the price of the lobe.

The test room (tests/ggx_lib.py room) at 1024 x 1024 under the path tracer and under VCM, 20 timed iterations after 3, two
alternating rounds: the room with its GGX materials against the same room with Phong lobes of exponent 2 / alpha^2 - 2
in their place (the version-7 twin, which launches the kernels of version 7).  Per run: Mpaths/s from the wall time of
the timed iterations and, from vcm_get_stats of the last iteration, the times of K1, K3 and the merge.

--kind list forces the general pow (SceneList) and --kind bvh a BVH on both rooms, --sampler sobol the Sobol sampler: the
forms of wavefront K3 that hold three waves with the lobe and four without.

    python tests/ggx_measure.py [--res 1024] [--kind rects|list|bvh] [--sampler sobol] [--out FILE]
"""
import argparse
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))


def run(phong, algo, res, sampler=None, warm=3, timed=20):
    import ggx_lib as gl
    from smallvcm_amd.renderer import VertexCM
    d = gl.room(res, res, phong=phong, sampler=sampler)
    r = VertexCM(d, algo, 0.003, 0.75, 1234)
    r.mMinPathLength, r.mMaxPathLength = 0, 10
    for it in range(warm):
        r.RunIteration(it)
    r.framebuffer_sum()
    t0 = time.perf_counter()
    for it in range(warm, warm + timed):
        r.RunIteration(it)
    r.framebuffer_sum()   # waits for the last iteration
    wall = time.perf_counter() - t0
    st = r.stats()
    r.close()
    paths = (2 if algo == 4 else 1) * res * res * timed   # VCM: a light and a camera path per pixel
    return paths / wall * 1e-6, st


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=1024)
    ap.add_argument("--kind", default="rects", choices=["rects", "list", "bvh"])
    ap.add_argument("--sampler", default=None, choices=["sobol"])
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.kind == "list":
        os.environ["SMALLVCM_AMD_GENERAL_POW"] = "1"   # read when a context is created
    if args.kind == "bvh":
        os.environ["SMALLVCM_AMD_FORCE_BVH"] = "1"
    lines = ["# tests/ggx_measure.py --kind %s%s: the room at %d^2, 20 timed iterations after 3; ggx = the room's GGX materials, phong = Phong lobes of exponent 2 / alpha^2 - 2 (version 7's kernels)"
             % (args.kind, " --sampler sobol" if args.sampler else "", args.res)]
    for rnd in (1, 2):
        for algo, name in ((5, "pt"), (4, "vcm")):
            for phong in (True, False):
                rate, st = run(phong, algo, args.res, args.sampler)
                lines.append("round %d %-3s %-5s %8.1f Mpaths/s   K1 %.3f ms  K3 %.3f ms  merge %.3f ms  connect %.3f ms  total %.3f ms" % (
                    rnd, name, "phong" if phong else "ggx", rate, st["msLightKernel"], st["msCameraKernel"], st["msMergeKernel"],
                    st["msConnectKernels"], st["msTotal"]))
                print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
