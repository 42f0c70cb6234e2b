#!/usr/bin/env python3
"""What halo_consumer_view costs next to halo_consumer_snapshot, on the GPU, in one process.

A 1920 x 1080 consumer accumulated under a dual-fisheye-equal-area render (a dense log-normal image: every pixel lit) is looked at through a linear
lens, fov 60, az 180, el 25, at 1920 x 1080 and at 960 x 540.  Per view, the median (min) over --calls calls after --warmup of

  device ms   HIP events on the backend's stream around the call's stream work (the kernel and the copies back to pageable host memory)
  wall ms     host clock around the call (it ends in the call's one stream synchronise)
  copy ms     the same bytes copied back from a device buffer by hipMemcpyAsync alone, between the same events
  kernel ms   device ms - copy ms: the kernel with the copies taken out

for the rgb-only call and for the call with all four outputs (rgb + xyz + map + dir), and for halo_consumer_snapshot (rgb out) on the same
consumer.  Every call goes to the C entry point with host buffers allocated once (the Python wrappers allocate their arrays per call, and a
copy into 30 MB of pages no one has touched yet measures the host's page faults).  The bytes the algorithm moves (computed from the shapes:
per view pixel 24 B gathered from sum / comp, plus what is stored) over the kernel time give the achieved rate.

With --parent-tree DIR (a built checkout of the parent commit) the headline follows: `bench.py --gpus 1 --steps 20 --warmup 5` in DIR and in this
tree, alternating, --ab-rounds times each.

  python tools/view_cost.py [--calls 40] [--warmup 10] [--parent-tree DIR] [--out profiles/view_cost.txt]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def hip_runtime():
    """The HIP runtime the library itself is linked to (the one already mapped into this process)."""
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            return C.CDLL(line.split()[-1])
    sys.exit("view_cost: the HIP runtime is not loaded")


def headline(tree):
    """One bench.py run in `tree`, a fresh process: (ms per step, rays / s)."""
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5"], cwd=tree, capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        sys.exit("view_cost: bench.py failed in %s\n%s" % (tree, r.stderr[-2000:]))
    doc = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    return doc["ms_per_step"], doc["value"]


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
        sys.exit("view_cost: no GPU — this is a measurement, it does not fall back")
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

    dbuf = C.c_void_p()
    assert hip.hipMalloc(C.byref(dbuf), C.c_size_t(1920 * 1080 * 40)) == 0

    def copy_ms(sizes):
        """The copies of a call on their own: one hipMemcpyAsync per output, device to pageable host memory, then the synchronise."""
        hosts = [np.empty(n, np.uint8) for n in sizes]

        def go():
            for a in hosts:
                hip.hipMemcpyAsync(a.ctypes.data_as(C.c_void_p), dbuf, C.c_size_t(a.nbytes), 2, stream)
            hip.hipStreamSynchronize(stream)
        return timed(go)[0]

    sw, sh = 1920, 1080
    src = scenes.render(abi.LENS_DUAL_FISHEYE_EQUAL_AREA, sw, sh, visible=abi.VISIBLE_FULL, az=0.0, el=0.0)
    xyz = np.exp(np.random.default_rng(5).normal(0.0, 1.0, (sh, sw, 3))).astype(np.float32)
    hb.Consume(xyz, 0.01 * sw * sh)
    fmt = "  %-52s device %7.3f (%7.3f) ms   wall %7.3f (%7.3f) ms   copy %7.3f ms   kernel %7.3f ms   %6.1f MB moved: %7.1f GB/s"
    lines = ["halo_consumer_view on a %d x %d dual-fisheye-equal-area consumer: median (min) over %d calls after %d warm-up calls; device ms = HIP events "
             "around the call's stream work, copy ms = the same bytes by hipMemcpyAsync alone, kernel ms = device - copy" % (sw, sh, args.calls, args.warmup), ""]
    n = sw * sh
    bufs = {"rgb": np.zeros(3 * n, np.uint8), "xyz": np.zeros(3 * n, np.float32), "map": np.zeros(n, np.int32), "dir": np.zeros(3 * n, np.float32)}
    ptr = {"rgb": bufs["rgb"].ctypes.data_as(C.POINTER(C.c_uint8)), "xyz": bufs["xyz"].ctypes.data_as(C.POINTER(C.c_float)),
           "map": bufs["map"].ctypes.data_as(C.POINTER(C.c_int32)), "dir": bufs["dir"].ctypes.data_as(C.POINTER(C.c_float))}
    dsp = abi.HaloDisplay(1.0, (C.c_float * 3)(-1.0, -1.0, -1.0), (C.c_float * 3)(0.0, 0.0, 0.0))

    def snapshot():
        assert L.halo_consumer_snapshot(hb._h, C.byref(dsp), ptr["rgb"], None, None) == abi.HALO_OK

    def look(view, want):
        spec = abi.HaloViewSpec()
        spec.view, spec.has_source, spec.source, spec.display = view, 1, src, dsp
        assert L.halo_consumer_view(hb._h, C.byref(spec), *[ptr[k] if k in want else None for k in ("rgb", "xyz", "map", "dir")]) == abi.HALO_OK

    d, dm, wl, wm = timed(snapshot)
    c = copy_ms([3 * n])
    snap_call, snap_kernel = d, d - c
    mb = n * (24 + 3) / 1e6
    lines.append(fmt % ("halo_consumer_snapshot (rgb out)", d, dm, wl, wm, c, d - c, mb, mb / (d - c)))
    for vw, vh in ((1920, 1080), (960, 540)):
        view = scenes.render(abi.LENS_LINEAR, vw, vh, fov=60.0, az=180.0, el=25.0, visible=abi.VISIBLE_FULL)
        m = vw * vh
        lines += ["", "view: linear, fov 60, az 180, el 25, %d x %d" % (vw, vh)]
        for name, want, out_bytes in (("rgb only", ("rgb",), [3 * m]), ("rgb + xyz + map + dir", ("rgb", "xyz", "map", "dir"), [3 * m, 12 * m, 4 * m, 12 * m])):
            d, dm, wl, wm = timed(lambda: look(view, want))
            c = copy_ms(out_bytes)
            mb = (24 * m + sum(out_bytes)) / 1e6
            lines.append(fmt % ("halo_consumer_view, " + name, d, dm, wl, wm, c, d - c, mb, mb / (d - c)))
            if name == "rgb only" and (vw, vh) == (sw, sh):
                lines.append("    -> against the snapshot: the call %.2f x, the kernel %.2f x" % (d / snap_call, (d - c) / snap_kernel))
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
