"""The figures of DESIGN.md "Image comparison" (not a test; needs a GPU).  At 2048 x 2048 and 512 x 512: vcm_compare of a
context (its framebuffer, 12 B per pixel, against its float4 reference) with ssim 0, with ssim 1 and with writeMap 1 -- by
events on the context's stream around vcm_compare (the context is put on torch's current stream with vcm_set_stream; median
of 20 calls after 3 warm-up calls), by the same events around vcm_compare_buffers on the same two images and by the host
clock around the context's call, which waits for its numbers -- and beside them, in the same process, vcm_read_framebuffer of
that context (what a host pays today before it can run numpy) and a device-to-device copy of the bytes the pixel kernel
reads.

    python tests/compare_measure.py

The kernels one by one: --calls RES MAP makes 23 plain calls of vcm_compare (ssim 1, writeMap MAP) and nothing else, for

    rocprofv3 --kernel-trace --stats -d DIR -o cmp --output-format csv -- python tests/compare_measure.py --calls 2048 0
"""
import ctypes as C
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

from smallvcm_amd._abi import ALGO_VCM  # noqa: E402
from smallvcm_amd.renderer import HipBackend, compare_tensors, cornell_scene  # noqa: E402


def events(fn, n=20, warm=3):
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
    return np.median(ts), min(ts), max(ts)


def wall(fn, n=20, warm=3):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(n):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t) * 1e3)
    return np.median(ts), min(ts), max(ts)


def timings(res):
    n = res * res
    b = HipBackend(cornell_scene(1, res, res), ALGO_VCM, 0.003, 0.75, 1234)
    for it in range(2):
        b.run_iteration(it, 0, 10)
    fb = b.framebuffer_sum()
    ref = fb * np.float32(0.5)
    ref[::7, ::5] *= np.float32(1.25)
    b.set_reference(ref)
    b.synchronize()
    b.set_stream(torch.cuda.current_stream(0).cuda_stream)       # the events below are recorded on the context's stream
    timg = torch.from_numpy(fb).cuda()
    tref = torch.from_numpy(np.concatenate([ref, np.ones((res, res, 1), np.float32)], axis=2)).cuda().contiguous()
    tmap = torch.empty(res, res, 4, device="cuda")
    src = torch.empty(n * 28, dtype=torch.uint8, device="cuda")       # the bytes the pixel kernel reads: 12 + 16 per pixel
    dst = torch.empty_like(src)
    cp = events(lambda: dst.copy_(src))
    copy_rate = 2 * 28 * n / cp[0] / 1e6
    print("res %d: device-to-device copy of 28 B per pixel (read and written): median %.4f ms (min %.4f max %.4f) = %.2f GB/s moved" % (res, *cp, copy_rate))
    for name, kw, moved in (("ssim 0", dict(ssim=0), 28), ("ssim 1", dict(ssim=1), 28), ("ssim 0, writeMap 1", dict(ssim=0, writeMap=1), 44),
                            ("ssim 1, writeMap 1", dict(ssim=1, writeMap=1), 44)):
        bkw = {k: v for k, v in kw.items() if k != "writeMap"}
        ev = events(lambda: compare_tensors(timg, tref, map_out=tmap if kw.get("writeMap") else None, scale=0.5, **bkw))
        ec = events(lambda: b.compare(**kw))
        wl = wall(lambda: b.compare(**kw))
        print("res %d, %s: vcm_compare of the context by events on its stream median %.4f ms (min %.4f max %.4f), by the host clock median %.4f ms "
              "(min %.4f max %.4f); vcm_compare_buffers by events median %.4f ms (min %.4f max %.4f); the pixel kernel moves %d B/pixel: over the "
              "context call's events %.2f GB/s, %.2f of the copy's rate" %
              (res, name, *ec, *wl, *ev, moved, moved * n / ec[0] / 1e6, moved * n / ec[0] / 1e6 / copy_rate))
    rd = wall(lambda: b.framebuffer_sum(), n=10)
    print("res %d: vcm_read_framebuffer (12 B/pixel to the host) host clock median %.4f ms (min %.4f max %.4f)" % (res, *rd))
    st = b.compare()
    print("res %d: %s" % (res, st))
    b.close()


def calls(res, write_map):
    b = HipBackend(cornell_scene(1, res, res), ALGO_VCM, 0.003, 0.75, 1234)
    for it in range(2):
        b.run_iteration(it, 0, 10)
    b.set_reference(b.framebuffer_sum() * np.float32(0.45))
    for _ in range(23):
        st = b.compare(ssim=1, writeMap=write_map)
    print("res %d, writeMap %d: %s" % (res, write_map, st))
    b.close()


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--calls":
        calls(int(sys.argv[2]), int(sys.argv[3]))
    else:
        for res in (2048, 512):
            timings(res)
