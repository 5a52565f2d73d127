"""The timings of DESIGN.md "Robust estimate" (not a test; needs a GPU): k_robust_update beside a device-to-device copy of
the same 76 B per pixel, k_robust_resolve<M> for M = 5 and 15 beside a copy of (M + 1) x 16 B per pixel (torch events: median
of 20 calls after 3 warm-up calls, and 200 calls back to back between one pair of events), the statistics, and one VCM
iteration of a warm context with robust tracking on and off (host clock around work that ends in a synchronise), at
2048 x 2048 and 512 x 512.

    python tests/robust_measure.py
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from variance_measure import events, iteration_ms, wall  # noqa: E402
from smallvcm_amd._abi import ALGO_VCM, ROBUST_DEFAULT_BUCKETS  # noqa: E402
from smallvcm_amd.renderer import (HipBackend, cornell_scene, robust_resolve_tensors, robust_stats_tensors,  # noqa: E402
                                   robust_update_tensors)


def copy_of(nbytes_moved):
    """a device-to-device copy that moves nbytes_moved in all: half read, half written"""
    src = torch.empty(nbytes_moved // 2, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    return events(lambda: dst.copy_(src))


def main():
    for res in (2048, 512):
        n = res * res
        s3 = torch.rand(n, 3, device="cuda")
        for M in (5, 15):
            prev, buckets = torch.zeros(n, 4, device="cuda"), torch.rand(M, n, 4, device="cuda")
            out = torch.empty(n, 4, device="cuda")
            if M == 5:
                k = [0]

                def update():
                    k[0] += 1
                    robust_update_tensors(s3, k[0], prev, buckets)
                m = events(update)
                c = copy_of(76 * n)
                print("res %d: k_robust_update median %.4f ms (min %.4f max %.4f, back to back %.4f) = %.2f TB/s of 76 B/pixel" %
                      (res, *m, 76 * n / m[0] / 1e9))
                print("res %d: device-to-device copy of the same traffic %.4f ms (min %.4f max %.4f, back to back %.4f) = %.2f TB/s; "
                      "update / copy %.2f" % (res, *c, 76 * n / c[0] / 1e9, m[0] / c[0]))
            kk = 4 * M + 3
            m = events(lambda: robust_resolve_tensors(prev, buckets, kk, out=out))
            c = copy_of((M + 1) * 16 * n)
            print("res %d: k_robust_resolve<%d> median %.4f ms (min %.4f max %.4f, back to back %.4f) = %.2f TB/s of %d B/pixel" %
                  (res, M, *m, (M + 1) * 16 * n / m[0] / 1e9, (M + 1) * 16))
            print("res %d: device-to-device copy of the same traffic %.4f ms (min %.4f max %.4f, back to back %.4f) = %.2f TB/s; "
                  "resolve / copy %.2f" % (res, *c, (M + 1) * 16 * n / c[0] / 1e9, m[0] / c[0]))
            print("res %d: vcm_robust_stats_buffers, M = %d, median %.4f ms (min %.4f max %.4f)" %
                  (res, M, *wall(lambda: robust_stats_tensors(prev, buckets, kk))))
            del prev, buckets, out
        del s3
        sc = cornell_scene(1, res, res)
        for M in (ROBUST_DEFAULT_BUCKETS, 0):
            b = HipBackend(sc, ALGO_VCM, 0.003, 0.75, 1234)
            if M:
                b.track_robust(M)
            print("res %d: one VCM iteration of scene 1, robust tracking %s: median %.4f ms (min %.4f max %.4f)" %
                  (res, "on (M = %d)" % M if M else "off", *iteration_ms(b)))
            if M:
                def read():
                    b.L.vcm_robust_resolve(b.ctx)
                    b.synchronize()
                print("res %d: vcm_robust_resolve + synchronise median %.4f ms (min %.4f max %.4f)" % (res, *wall(read)))
                print("res %d: vcm_get_robust_stats median %.4f ms (min %.4f max %.4f)" % (res, *wall(b.robust_stats)))
            b.close()


if __name__ == "__main__":
    main()
