#!/usr/bin/env python3
"""What the auxiliary lines (halo_consumer_view_overlay: horizon, grid, sun circles, zenith / nadir rings, sun marker) cost next to
halo_consumer_view_filtered, on the GPU, in one process and on one consumer.

A dense 1920 x 1080 consumer accumulated under a dual-fisheye-equal-area render with overlap 0.1 (a log-normal image: every pixel lit) is
looked at through a 1920 x 1080 linear lens, fov 60, az 180, el 25.  rgb only, nearest and bilinear:

  halo_consumer_view_filtered                    the gather and the copy back (this code is the parent commit's, unchanged)
  halo_consumer_view_overlay, no layer on        the gather with its dir output (12 more bytes written per pixel), the overlay pass, the copy back
  halo_consumer_view_overlay, all five layers    the same with every layer drawn

Per way the median (min) over --calls calls after --warmup of

  device ms   HIP events on the backend's stream around the call's stream work (the kernels and the copy back to pageable host memory)
  wall ms     host clock around the call (it ends in the call's one stream synchronise)
  copy ms     the same bytes copied back from a device buffer by hipMemcpyAsync alone, between the same events
  kernel ms   device ms - copy ms: the kernels with the copy taken out

The overlay pass alone is the difference of the overlay call and the filtered call: the pass itself and the 12 bytes per pixel of directions the
gather writes for it (they stay on the device: rgb_out alone is asked of every call).
Every call goes to the C entry point with host buffers allocated once (tools/view_cost.py says why).

With --parent-tree DIR (a built checkout of the parent commit) the headline follows: `bench.py --gpus 1 --steps 20 --warmup 5` in DIR and in this
tree, alternating, --ab-rounds times each.

  python tools/view_overlay_cost.py [--calls 40] [--warmup 10] [--parent-tree DIR] [--out profiles/view_overlay_cost.txt]
"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from view_cost import headline, hip_runtime   # noqa: E402  (the protocol's two helpers: one definition)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--parent-tree", default="")
    ap.add_argument("--ab-rounds", type=int, default=3)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.calls < 20:
        ap.error("--calls must be at least 20")
    import numpy as np
    from ice_halo_sim_amd import abi, backend, scenes
    L = backend.load_library()
    if L.halo_device_count() <= 0:
        sys.exit("view_overlay_cost: no GPU — this is a measurement, it does not fall back")
    hb = backend.HipTraceBackend(device=0, seed=1)
    hip = hip_runtime()
    stream, e0, e1 = C.c_void_p(), C.c_void_p(), C.c_void_p()
    assert hip.hipStreamCreate(C.byref(stream)) == 0 and hip.hipEventCreate(C.byref(e0)) == 0 and hip.hipEventCreate(C.byref(e1)) == 0
    hb.set_stream(stream.value)

    def timed(fn):
        dev, wall = [], []
        for k in range(args.warmup + args.calls):
            hip.hipEventRecord(e0, stream)
            t = time.perf_counter()
            fn()
            w = (time.perf_counter() - t) * 1e3
            hip.hipEventRecord(e1, stream)
            hip.hipEventSynchronize(e1)
            ms = C.c_float()
            hip.hipEventElapsedTime(C.byref(ms), e0, e1)
            if k >= args.warmup:
                dev.append(ms.value)
                wall.append(w)
        return statistics.median(dev), min(dev), statistics.median(wall), min(wall)

    sw, sh = 1920, 1080
    n = sw * sh
    dbuf = C.c_void_p()
    assert hip.hipMalloc(C.byref(dbuf), C.c_size_t(3 * n)) == 0
    host = np.empty(3 * n, np.uint8)

    def copy_alone():
        hip.hipMemcpyAsync(host.ctypes.data_as(C.c_void_p), dbuf, C.c_size_t(host.nbytes), 2, stream)
        hip.hipStreamSynchronize(stream)

    src = scenes.render(abi.LENS_DUAL_FISHEYE_EQUAL_AREA, sw, sh, visible=abi.VISIBLE_FULL, az=0.0, el=0.0, overlap=0.1)
    xyz = np.exp(np.random.default_rng(5).normal(0.0, 1.0, (sh, sw, 3))).astype(np.float32)
    hb.Consume(xyz, 0.01 * sw * sh)
    rgb = np.zeros(3 * n, np.uint8)
    rgb_p = rgb.ctypes.data_as(C.POINTER(C.c_uint8))
    dsp = abi.HaloDisplay(1.0, (C.c_float * 3)(-1.0, -1.0, -1.0), (C.c_float * 3)(0.0, 0.0, 0.0))
    view = scenes.render(abi.LENS_LINEAR, sw, sh, fov=60.0, az=180.0, el=25.0, visible=abi.VISIBLE_FULL)
    spec = abi.HaloViewSpec()
    spec.view, spec.has_source, spec.source, spec.display = view, 1, src, dsp
    off = backend.view_overlay(60.0, (25.0, 180.0))
    on = backend.view_overlay(60.0, (25.0, 180.0), ("horizon", "grid", "circles", "zenith", "sun"))
    fmt = "  %-58s device %7.3f (%7.3f) ms   wall %7.3f (%7.3f) ms   copy %7.3f ms   kernel %7.3f ms"
    lines = ["rgb-only view calls on a %d x %d dual-fisheye-equal-area consumer, overlap 0.1, through a %d x %d linear view, fov 60, az 180, el 25: median (min) over "
             "%d calls after %d warm-up calls; device ms = HIP events around the call's stream work, copy ms = the same bytes by hipMemcpyAsync alone, "
             "kernel ms = device - copy" % (sw, sh, sw, sh, args.calls, args.warmup)]
    c = timed(copy_alone)[0]
    changed = hb.ViewOverlay(view, on, src)["rgb"] != hb.View(view, src)["rgb"]
    lines.append("all five layers change %.2f %% of the view's pixels" % (100.0 * float(changed.any(axis=-1).mean())))
    for fname, fval in (("nearest", abi.VIEW_NEAREST), ("bilinear", abi.VIEW_BILINEAR)):
        f = abi.HaloViewFilter(fval, 0)

        def filtered():
            assert L.halo_consumer_view_filtered(hb._h, C.byref(spec), C.byref(f), rgb_p, None, None, None, None) == abi.HALO_OK

        def overlay(o):
            assert L.halo_consumer_view_overlay(hb._h, C.byref(spec), C.byref(f), C.byref(o), rgb_p, None, None, None, None, None) == abi.HALO_OK

        lines.append("")
        d0, dm, wl, wm = timed(filtered)
        lines.append(fmt % ("halo_consumer_view_filtered, %s" % fname, d0, dm, wl, wm, c, d0 - c))
        for name, o in (("halo_consumer_view_overlay, %s, no layer on" % fname, off), ("halo_consumer_view_overlay, %s, all five layers" % fname, on)):
            d, dm, wl, wm = timed(lambda: overlay(o))
            lines.append(fmt % (name, d, dm, wl, wm, c, d - c))
            lines.append("    -> against halo_consumer_view_filtered: the call %.2f x (+%.3f ms), the kernels %.2f x" % (d / d0, d - d0, (d - c) / (d0 - c)))
    hb.close()
    if args.parent_tree:
        lines += ["", "headline: bench.py --gpus 1 --steps 20 --warmup 5, the parent commit's tree and this one alternating, a fresh process each"]
        ms = {"parent": [], "this": []}
        for k in range(args.ab_rounds):
            for who, tree in (("parent", args.parent_tree), ("this", ROOT)):
                m, v = headline(tree)
                ms[who].append(m)
                lines.append("  %-6s run %d   ms_per_step %8.4f   rays/s %.4e" % (who, k + 1, m, v))
        pm, tm = statistics.median(ms["parent"]), statistics.median(ms["this"])
        lines.append("  parent median %.4f ms (its runs span %.4f .. %.4f: %.3f %%), this median %.4f ms: %+.3f %% against the parent"
                     % (pm, min(ms["parent"]), max(ms["parent"]), 100.0 * (max(ms["parent"]) - min(ms["parent"])) / pm, tm, 100.0 * (tm - pm) / pm))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
