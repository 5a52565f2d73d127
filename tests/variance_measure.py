"""The timings of DESIGN.md "Variance" (not a test; needs a GPU): k_var_update beside a device-to-device copy of the same
traffic (torch events: median of 20 calls after 3 warm-up calls, and 200 calls back to back between one pair of events),
the noise statistic, a VCM iteration with and without tracking, a default and a guided denoise of the same context (host
clock around work that ends in a synchronise), at 2048 x 2048 and 512 x 512.

    python tests/variance_measure.py
"""
import ctypes as C
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from smallvcm_amd._abi import ALGO_VCM  # noqa: E402
from smallvcm_amd.renderer import (HipBackend, cornell_scene, denoise_params, denoise_params2,  # noqa: E402
                                   noise_stats_tensors, variance_update_tensors)


def events(fn, n=20, warm=3):
    """(median, min, max) ms of n calls timed one by one, and the ms per call of 200 calls back to back"""
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(200):
        fn()
    b.record()
    b.synchronize()
    return np.median(ts), min(ts), max(ts), a.elapsed_time(b) / 200


def wall(fn, n=20, warm=3):
    """(median, min, max) ms of n calls by the host clock, the device idle before and after each"""
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(n):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t) * 1e3)
    return np.median(ts), min(ts), max(ts)


def iteration_ms(b):
    it = [0]

    def iterate():
        b.run_iteration(it[0], 0, 10)
        b.synchronize()
        it[0] += 1
    return wall(iterate, warm=5)


def main():
    for res in (2048, 512):
        n = res * res
        s3 = torch.rand(n, 3, device="cuda")
        prev, mom = torch.zeros(n, 4, device="cuda"), torch.zeros(n, 4, device="cuda")
        k = [1]

        def update():
            k[0] += 1
            variance_update_tensors(s3, k[0], prev, mom)
        m = events(update)
        src = torch.empty(n * 38, dtype=torch.uint8, device="cuda")   # read 38 B, write 38 B per pixel: the update's 76 B
        dst = torch.empty_like(src)
        c = events(lambda: dst.copy_(src))
        print("res %d: k_var_update median %.4f ms (min %.4f max %.4f, back to back %.4f) = %.2f TB/s of 76 B/pixel" %
              (res, *m, 76 * n / m[0] / 1e9))
        print("res %d: device-to-device copy of the same traffic %.4f ms (min %.4f max %.4f, back to back %.4f) = %.2f TB/s; "
              "update / copy %.2f" % (res, *c, 76 * n / c[0] / 1e9, m[0] / c[0]))
        print("res %d: vcm_noise_stats_buffers median %.4f ms (min %.4f max %.4f)" %
              (res, *wall(lambda: noise_stats_tensors(prev, mom, 5, 0.01))))
        del s3, prev, mom, src, dst
        sc = cornell_scene(1, res, res)
        b = HipBackend(sc, ALGO_VCM, 0.003, 0.75, 1234)
        b.track_variance()
        print("res %d: one VCM iteration of scene 1, tracking on: median %.4f ms (min %.4f max %.4f)" % (res, *iteration_ms(b)))
        print("res %d: vcm_get_noise_stats median %.4f ms (min %.4f max %.4f)" % (res, *wall(lambda: b.noise_stats(0.01))))
        p = denoise_params()

        def denoise():
            b.L.vcm_denoise(b.ctx, 0.1, C.byref(p))
            b.synchronize()
        fixed = wall(denoise)
        print("res %d: vcm_denoise with defaults median %.4f ms (min %.4f max %.4f)" % (res, *fixed))
        p2 = denoise_params2(varianceGuided=1)

        def denoise2():
            b.L.vcm_denoise2(b.ctx, 0.1, C.byref(p2))
            b.synchronize()
        guided = wall(denoise2)
        print("res %d: vcm_denoise2, guided defaults, median %.4f ms (min %.4f max %.4f); guided / fixed %.2f" %
              (res, *guided, guided[0] / fixed[0]))
        b.close()
        b = HipBackend(sc, ALGO_VCM, 0.003, 0.75, 1234)
        print("res %d: one VCM iteration of scene 1, tracking off: median %.4f ms (min %.4f max %.4f)" % (res, *iteration_ms(b)))
        b.close()


if __name__ == "__main__":
    main()
