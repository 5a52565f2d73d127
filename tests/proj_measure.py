"""The measurement of DESIGN.md "Camera projections" (not a test; needs a GPU): the price of the projection branch.

The test room (tests/proj_lib.py box, room=True, the camera inside) at 1024 x 1024 under the path tracer and under VCM, 20
timed iterations after 3.  Variants: `persp` (the pinhole: the kernels without the WithLens wrapper), `tent` (the pinhole
with a tent filter: the WithLens kinds, which carry the projection branch without taking it), `fisheye` (180 degrees) and
`panorama`; `sobol` (the pinhole under the Sobol sampler, whose kinds carry the branch too; with SMALLVCM_AMD_GENERAL_POW=1 the
SceneList form of wavefront K3, which the branch takes from four waves per SIMD to three).  Per run: Mpaths/s from the wall time of the timed iterations and, from vcm_get_stats of the last iteration,
the times of K1, K3 and the connection kernels.  SMALLVCM_AMD_LIB selects the library (a build of the parent commit for
`tent`: what carrying the branch costs).

    python tests/proj_measure.py [--res 1024] [--variants tent,persp,fisheye,panorama] [--tag new] [--timed 20] [--out FILE]
"""
import argparse
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

VARIANTS = {"persp": {}, "tent": {"flt": ("tent", 1.5)}, "fisheye": {"proj": ("fisheye", 180.0)}, "panorama": {"proj": ("panorama",)},
            "sobol": {"sampler": "sobol"}}   # (the pinhole under Sobol: its kinds carry every branch; SMALLVCM_AMD_GENERAL_POW=1 for the list kind)


def run(variant, algo, res, warm=3, timed=20):
    import proj_lib as pl
    from smallvcm_amd.renderer import VertexCM
    d = pl.box(res, res, room=True, **VARIANTS[variant])
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
    ap.add_argument("--variants", default="tent,persp,fisheye,panorama")
    ap.add_argument("--tag", default="new")
    ap.add_argument("--timed", type=int, default=20)
    ap.add_argument("--out")
    args = ap.parse_args()
    lines = []
    for algo, name in ((5, "pt"), (4, "vcm")):
        for v in args.variants.split(","):
            rate, st = run(v, algo, args.res, timed=args.timed)
            lines.append("%-6s %-3s %-8s %8.1f Mpaths/s   K1 %.3f ms  K3 %.3f ms  merge %.3f ms  connect %.3f ms  total %.3f ms" % (
                args.tag, name, v, rate, st["msLightKernel"], st["msCameraKernel"], st["msMergeKernel"], st["msConnectKernels"], st["msTotal"]))
            print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
