"""The figures of DESIGN.md "Display transform" (not a test; needs a GPU).  At 2048 x 2048, on a float4 and on a three-float image: curve and
transfer alone, bloom at 5 levels, and the call with auto-exposure on (histogram, read-back, transform), by torch events
around vcm_display_buffers where the call is asynchronous (median of 20 calls after 3 warm-up calls, and 200 calls back to
back between one pair of events) and by the host clock where it waits; vcm_read_image(BGR8) of a context of that size as
the yardstick.  Then what the histogram picks and how much clips on scene 1, scene 3 and an env-map scene at 512 x 512
after 64 VCM iterations.

    python tests/display_measure.py
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
from smallvcm_amd.renderer import HipBackend, cornell_scene, display_params, load_library  # noqa: E402


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
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(200):
        fn()
    b.record()
    b.synchronize()
    return np.median(ts), min(ts), max(ts), a.elapsed_time(b) / 200


def wall(fn, n=20, warm=3):
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


def timings(res=2048):
    L = load_library()
    n = res * res
    for channels in (4, 3):
        img = (torch.rand(res, res, channels, device="cuda") * 4.0).contiguous()
        out = torch.empty(res, res, 4, device="cuda")
        stream = torch.cuda.current_stream(0).cuda_stream

        def call(**kw):
            p = display_params(**kw)

            def fn():
                assert L.vcm_display_buffers(0, res, res, img.data_ptr(), channels, 1.0, C.byref(p), out.data_ptr(), None, stream) == 0, L.vcm_last_error()
            return fn
        rd = 4 * channels
        m = events(call(curve="aces", transfer="srgb"))
        print("res %d, %d floats per pixel: curve + transfer median %.4f ms (min %.4f max %.4f, back to back %.4f) = %.2f TB/s of %d B/pixel" %
              (res, channels, *m, (rd + 16) * n / m[3] / 1e9, rd + 16))
        bl = events(call(curve="aces", transfer="srgb", bloomStrength=0.3, bloomLevels=5))
        # down0 reads the source and writes a quarter float4; the levels (a third of the pixels) are read and written about
        # 16 B x (1 + 2 + 2 + 2 + 2) per level pixel; the final pass reads the source and writes 16 B
        bytes_bloom = (rd + 4) + (rd + 16) + (16.0 / 3.0) * 9
        print("res %d, %d floats per pixel: with bloom at 5 levels median %.4f ms (min %.4f max %.4f, back to back %.4f) = %.2f TB/s of about %.0f B/pixel" %
              (res, channels, *bl, bytes_bloom * n / bl[3] / 1e9, bytes_bloom))
        au = wall(call(curve="aces", transfer="srgb", autoExposure=1))
        pl = wall(call(curve="aces", transfer="srgb"))
        print("res %d, %d floats per pixel: with auto-exposure (histogram, 2 KB read-back, transform) host clock median %.4f ms (min %.4f max %.4f); "
              "the same call without it %.4f ms; the difference %.4f ms = %.2f TB/s of the histogram's %d B/pixel" %
              (res, channels, *au, pl[0], au[0] - pl[0], rd * n / max(au[0] - pl[0], 1e-6) / 1e9, rd))
    src = torch.empty(n * 16, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    cp = events(lambda: dst.copy_(src))
    print("res %d: device-to-device copy, 16 B read + 16 B written per pixel: median %.4f ms (back to back %.4f) = %.2f TB/s" %
          (res, cp[0], cp[3], 32 * n / cp[3] / 1e9))
    del src, dst
    b = HipBackend(cornell_scene(1, res, res), ALGO_VCM, 0.003, 0.75, 1234)
    b.run_iteration(0, 0, 10)
    b.synchronize()
    print("res %d: vcm_read_image(BGR8) of a context (allocation, encode, 3 B/pixel to the host) host clock median %.4f ms (min %.4f max %.4f)" %
          (res, *wall(lambda: b.read_image(0, 1.0, 2.2), n=10)))

    def shown():
        b.display(curve="aces", transfer="srgb")
        b.read_display_image(0)
    print("res %d: vcm_display + vcm_read_display + vcm_read_display_image(BGR8) of the same context host clock median %.4f ms (min %.4f max %.4f)" %
          (res, *wall(shown, n=10)))
    b.close()


def image_statistics(res=512, iterations=64):
    import denoise_lib as dl
    import envmap_lib as el
    scenes = {"scene 1": dl.box(1, res, res), "scene 3": dl.box(3, res, res),
              "env map": el.builtin_with_envmap(el.sky(64, 32), resx=res, resy=res)}
    for name, sc in scenes.items():
        b = HipBackend(dl.desc5(sc), ALGO_VCM, 0.003, 0.75, 1234)
        for it in range(iterations):
            b.run_iteration(it, 0, 10)
        b.display()
        clamp = b.display_stats()
        b.display(curve="aces", autoExposure=1)
        aces = b.display_stats()
        print("%s, VCM, %d x %d, %d iterations: autoEV %+.3f (log2 of the trimmed mean luminance %.3f, %d pixels counted, %d black); "
              "clipped channels under CLAMP at exposure 0: %.2f %%; under ACES with auto-exposure: %.2f %%" %
              (name, res, res, iterations, aces["autoEV"], aces["logAvgLuminance"], aces["counted"], aces["zero"],
               100.0 * clamp["clipped"] / (3 * res * res), 100.0 * aces["clipped"] / (3 * res * res)))
        b.close()


if __name__ == "__main__":
    timings()
    image_statistics()
