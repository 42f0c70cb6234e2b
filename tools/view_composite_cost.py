#!/usr/bin/env python3
"""What the class composite through a view (halo_consumer_view_composite) and the class lanes through a view (halo_consumer_view_lanes) cost, on the
GPU, in one process and on one handle — on the protocol of tools/view_filter_cost.py.

A dense 1920 x 1080 lane set (log-normal: every pixel lit in every class) under a dual-fisheye-equal-area render with overlap 0.1 is looked at
through a 1920 x 1080 linear lens, fov 60, az 180, el 0 (the horizon, and the band around it, run through the middle of the view).  For nearest,
bilinear and bilinear + blend, per call the median (min) over --calls calls after --warmup of

  device ms   HIP events on the backend's stream around the call's stream work — for the composite calls that includes the host's three waits
              inside the P99 select, which the stream sits out idle
  wall ms     host clock around the call (it ends in the call's last stream synchronise)

and the split of the srgb-only composite view, from calls that share its parts:

  stage 1     halo_consumer_composite with srgb_out only (the select's three histogram passes with their round trips, the composite kernel, the
              copy of the source-sized bytes) less that copy alone: what the view call runs before its gather
  copy        the view's 3 bytes per pixel copied back from a device buffer by hipMemcpyAsync alone, between the same events
  gather      the view call less stage 1 less copy: halo_view_composite_kernel

Next to them halo_consumer_view_filtered (rgb only) on a consumer of the same size, and the lanes call at 3 and at 16 classes with its own copy.
Every call goes to the C entry point with host buffers allocated once (tools/view_cost.py says why).

With --parent-tree DIR (a built checkout of the parent commit) the headline follows: `bench.py --gpus 1 --steps 20 --warmup 5` in DIR and in this
tree, alternating, --ab-rounds times each.

  python tools/view_composite_cost.py [--calls 40] [--warmup 10] [--parent-tree DIR] [--ab-rounds 5] [--out profiles/view_composite_cost.txt]
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
    ap.add_argument("--ab-rounds", type=int, default=5)
    ap.add_argument("--out", default="")
    ap.add_argument("--filters", default="nearest,bilinear,bilinear + blend", help="the filters to time (one alone under a kernel trace: a kernel's name does not say its filter)")
    args = ap.parse_args()
    if args.calls < 20:
        ap.error("--calls must be at least 20")
    import numpy as np
    from ice_halo_sim_amd import abi, backend, scenes
    L = backend.load_library()
    if L.halo_device_count() <= 0:
        sys.exit("view_composite_cost: no GPU — this is a measurement, it does not fall back")
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
    big = 16
    dbuf = C.c_void_p()
    assert hip.hipMalloc(C.byref(dbuf), C.c_size_t(4 * big * n)) == 0
    host = np.empty(4 * big * n, np.uint8)

    def copy_alone(nbytes):
        def fn():
            hip.hipMemcpyAsync(host.ctypes.data_as(C.c_void_p), dbuf, C.c_size_t(nbytes), 2, stream)
            hip.hipStreamSynchronize(stream)
        return fn

    src = scenes.render(abi.LENS_DUAL_FISHEYE_EQUAL_AREA, sw, sh, visible=abi.VISIBLE_FULL, az=0.0, el=0.0, overlap=0.1)
    view = scenes.render(abi.LENS_LINEAR, sw, sh, fov=60.0, az=180.0, el=0.0, visible=abi.VISIBLE_FULL)
    spec = abi.HaloViewSpec()
    spec.view, spec.has_source, spec.source = view, 1, src
    spec.display = abi.HaloDisplay(1.0, (C.c_float * 3)(-1.0, -1.0, -1.0), (C.c_float * 3)(0.0, 0.0, 0.0))
    g = np.random.default_rng(5)
    lanes16 = np.exp(g.normal(0.0, 1.0, (big, sh, sw))).astype(np.float32)
    colors = [{"color": c} for c in ((1.0, 0.2, 0.1), (0.1, 1.0, 0.3), (0.2, 0.4, 1.0))]
    comp = abi.composite(colors, "painter", 1.0, 1.0)
    hb.Consume(np.exp(g.normal(0.0, 1.0, (sh, sw, 3))).astype(np.float32), 0.01 * n)   # the consumer halo_consumer_view_filtered reads
    rgb = np.zeros(3 * n, np.uint8)
    rgb_p = rgb.ctypes.data_as(C.POINTER(C.c_uint8))
    out_l = np.zeros(big * n, np.float32)
    out_lp = out_l.ctypes.data_as(C.POINTER(C.c_float))
    p99, produced = C.c_float(), C.c_int32()
    filters = [(name, f) for name, f in (("nearest", abi.HaloViewFilter(abi.VIEW_NEAREST, 0)), ("bilinear", abi.HaloViewFilter(abi.VIEW_BILINEAR, 0)),
                                         ("bilinear + blend", abi.HaloViewFilter(abi.VIEW_BILINEAR, 1))) if name in args.filters.split(",")]

    def classes(k):
        hb.set_color([], [scenes.color_class([c]) for c in range(k)])
        hb.LoadClassLanes(lanes16[:k], 0.01 * n)

    def view_composite(f):
        def fn():
            assert L.halo_consumer_view_composite(hb._h, C.byref(spec), C.byref(f), C.byref(comp), rgb_p, None, None, None, C.byref(p99), C.byref(produced)) == abi.HALO_OK
            assert produced.value == 1
        return fn

    def flat_composite():
        assert L.halo_consumer_composite(hb._h, C.byref(comp), None, rgb_p, C.byref(p99), C.byref(produced)) == abi.HALO_OK and produced.value == 1

    def view_filtered(f):
        def fn():
            assert L.halo_consumer_view_filtered(hb._h, C.byref(spec), C.byref(f), rgb_p, None, None, None, None) == abi.HALO_OK
        return fn

    def view_lanes(f):
        def fn():
            assert L.halo_consumer_view_lanes(hb._h, C.byref(spec), C.byref(f), out_lp, None, None) == abi.HALO_OK
        return fn

    tap = hb.View(view, src, want=("tap",), filter="bilinear", blend=True)["tap"]
    fmt = "  %-58s device %7.3f (%7.3f) ms   wall %7.3f (%7.3f) ms"
    lines = ["library: %s" % os.path.basename(backend.LIB_PATH),
             "%d x %d dual-fisheye-equal-area lanes, overlap 0.1, through a %d x %d linear view, fov 60, az 180, el 0 (%.1f %% of its pixels lie in the "
             "overlap band): median (min) over %d calls after %d warm-up calls" % (sw, sh, sw, sh, 100.0 * float((tap[..., 4] > 0.0).mean()), args.calls, args.warmup)]
    c3 = timed(copy_alone(3 * n))
    lines += ["", fmt % ("copy of %d bytes alone (3 per pixel)" % (3 * n), *c3)]
    classes(3)
    flat = timed(flat_composite)
    stage1 = flat[0] - c3[0]
    lines += [fmt % ("halo_consumer_composite, srgb only, 3 classes", *flat), "    -> stage 1 (select + composite kernel) = that less the copy: %.3f ms" % stage1]
    for name, f in filters:
        v = timed(view_composite(f))
        lines += [fmt % ("halo_consumer_view_composite, srgb only, " + name, *v),
                  "    -> stage 1 %.3f + gather kernel %.3f + copy %.3f ms" % (stage1, v[0] - stage1 - c3[0], c3[0])]
        o = timed(view_filtered(f))
        lines += [fmt % ("halo_consumer_view_filtered, rgb only, " + name, *o), "    -> its kernel (the call less the copy): %.3f ms" % (o[0] - c3[0])]
    for k in (3, big):
        classes(k)
        ck = timed(copy_alone(4 * k * n))
        lines += ["", fmt % ("copy of %d bytes alone (%d classes x 4 per pixel)" % (4 * k * n, k), *ck)]
        for name, f in filters:
            v = timed(view_lanes(f))
            lines += [fmt % ("halo_consumer_view_lanes, %d classes, %s" % (k, name), *v), "    -> kernel (the call less the copy): %.3f ms" % (v[0] - ck[0])]
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
