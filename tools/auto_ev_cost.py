#!/usr/bin/env python3
"""What halo_consumer_auto_ev costs next to the snapshot it accompanies, on the GPU, in one process.

A 1920 x 1080 consumer is loaded with a sparse (2 % lit) and a dense Y plane of the tests' integer recipe (values in three exponents: the first
radix digit lands in a handful of bins, like a halo image).  Per image, the median over --calls calls (after --warmup) of

  device ms   HIP events on the backend's stream around the call's stream work (value kernel, select, the 32-byte copy back)
  wall ms     host clock around the call (it ends in the call's one stream synchronise)

for f = 8 (32 400 box sums, one workgroup's select) and f = 1 (2 073 600 values, the multi-block select), each with plain LDS adds in the
histogram passes (the product) and with wave-aggregated adds (option auto_ev_hist = 1); f = 8 also through the multi-block select.  A third
image, every pixel the same value, is the plain adds' worst case: all 64 lanes of every wave meet in one bin on all three digits.  Beside them
halo_consumer_snapshot (rgb out) on the same consumer.  Every variant must return the same record.

  python tools/auto_ev_cost.py [--calls 40] [--warmup 10] [--out profiles/auto_ev_cost.txt]
"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def hip_runtime():
    """The HIP runtime the library itself is linked to (the one already mapped into this process)."""
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            return C.CDLL(line.split()[-1])
    sys.exit("auto_ev_cost: the HIP runtime is not loaded")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.calls < 20:
        ap.error("--calls must be at least 20")
    import numpy as np
    from ice_halo_sim_amd import backend
    from tests import _ev_auto_model as M
    L = backend.load_library()
    if L.halo_device_count() <= 0:
        sys.exit("auto_ev_cost: no GPU — this is a measurement, it does not fall back")
    hb = backend.HipTraceBackend(device=0, seed=1)
    hip = hip_runtime()
    stream, e0, e1 = C.c_void_p(), C.c_void_p(), C.c_void_p()
    assert hip.hipStreamCreate(C.byref(stream)) == 0 and hip.hipEventCreate(C.byref(e0)) == 0 and hip.hipEventCreate(C.byref(e1)) == 0
    hb.set_stream(stream.value)

    def timed(fn):
        dev, wall, last = [], [], None
        for k in range(args.warmup + args.calls):
            hip.hipEventRecord(e0, stream)
            t = time.perf_counter()
            last = fn()
            w = (time.perf_counter() - t) * 1e3
            hip.hipEventRecord(e1, stream)
            hip.hipEventSynchronize(e1)
            ms = C.c_float()
            hip.hipEventElapsedTime(C.byref(ms), e0, e1)
            if k >= args.warmup:
                dev.append(ms.value)
                wall.append(w)
        return statistics.median(dev), min(dev), statistics.median(wall), min(wall), last

    w, h = 1920, 1080
    lines = ["halo_consumer_auto_ev at %d x %d: median (min) over %d calls after %d warm-up calls; device ms = HIP events around the call's stream work, "
             "wall ms = host clock around the call" % (w, h, args.calls, args.warmup)]
    for name, density in (("sparse (2 % lit)", 0.02), ("dense", 1.0), ("flat (every pixel 0.75)", None)):
        y = np.full((h, w), 0.75, np.float32) if density is None else M.recipe_image(w, h, 19, density, 0.0 if density == 1.0 else 0.1, -2, 0)
        xyz = np.zeros((h, w, 3), np.float32)
        xyz[..., 1] = y
        hb.ResetConsumer()
        hb.Consume(xyz, 0.01 * w * h)
        lines.append("")
        lines.append("image: %s" % name)
        d, dm, wl, wm, _ = timed(lambda: hb.Snapshot(want_xyz=False))
        lines.append("  %-58s device %7.3f (%7.3f) ms   wall %7.3f (%7.3f) ms" % ("halo_consumer_snapshot (rgb out, 6.2 MB copied back)", d, dm, wl, wm))
        for f in (8, 1):
            ref = None
            for label, select, agg in (("plain LDS adds", -1, 0), ("wave-aggregated adds", -1, 1)) + \
                    ((("multi-block select, plain LDS adds", 0, 0), ("multi-block select, wave-aggregated adds", 0, 1)) if f == 8 else ()):
                hb.set_option("auto_ev_select", select)
                hb.set_option("auto_ev_hist", agg)
                d, dm, wl, wm, a = timed(lambda: hb.AutoEv(f))
                ref = ref or a
                assert a == ref, (a, ref)
                lines.append("  %-58s device %7.3f (%7.3f) ms   wall %7.3f (%7.3f) ms" % ("auto_ev f = %d, %s" % (f, label), d, dm, wl, wm))
            lines.append("    -> %d values, p99_y %.9g, ev_auto %+.4f" % (ref["value_count"], ref["p99_y"], ref["ev_auto"]))
        hb.set_option("auto_ev_select", -1)
        hb.set_option("auto_ev_hist", 0)
    hb.close()
    # where one workgroup's select stops paying: the same dense values through both selects, fine path on small images (plain adds)
    lines.append("")
    lines.append("one workgroup's select against the multi-block select, dense values, f = 1 (the threshold kAevSmallMax of halo_launch.h comes from here)")
    for sw, sh in ((32, 32), (64, 64), (128, 64), (128, 128), (240, 135), (256, 256)):   # 1 Ki .. 64 Ki values
        hs = backend.HipTraceBackend(device=0, seed=1)
        hs.set_stream(stream.value)
        xyz = np.zeros((sh, sw, 3), np.float32)
        xyz[..., 1] = M.recipe_image(sw, sh, 23, 1.0, 0.0, -2, 0)
        hs.Consume(xyz, 0.01 * sw * sh)
        res = []
        for select in (1, 0):
            hs.set_option("auto_ev_select", select)
            res.append(timed(lambda: hs.AutoEv(1)))
        assert res[0][4] == res[1][4]
        lines.append("  %7d values: one workgroup device %7.3f (%7.3f) ms   multi-block device %7.3f (%7.3f) ms" % (sw * sh, res[0][0], res[0][1], res[1][0], res[1][1]))
        hs.close()
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
