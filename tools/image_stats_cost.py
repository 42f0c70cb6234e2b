#!/usr/bin/env python3
"""What halo_consumer_stats costs next to the calls it stands beside, on the GPU, in one process.

A 1920 x 1080 consumer is loaded with a sparse (2 % lit) and a dense Y plane of the tests' integer recipe (values in three exponents, like a halo
image: the percentiles' ranks share a handful of prefixes) and with a dense log-normal plane (sigma = 4: the ranks spread over
more than a dozen first-digit bins, the select's many-groups case).  Per image, the median over --calls calls (after --warmup) of

  device ms   HIP events on the backend's stream around the call's stream work (kernels, the one record copied back)
  wall ms     host clock around the call (it ends in the call's one stream synchronise)

for the reference tool's eleven-percentile call, a call with no percentile (moments only: the first sweep and one pick), halo_consumer_auto_ev
at f = 1 and halo_consumer_snapshot (rgb out), all on the same consumer.  Then the one-workgroup form against the multi-block form on 1 Ki ..
64 Ki values (option stats_select; the threshold kStatsSmallMax of halo_launch.h comes from here); both must return the same result.

With --parent-tree DIR (a built checkout of the parent commit) the headline follows: `bench.py --gpus 1 --steps 20 --warmup 5 --repeats 5` in
DIR and in this tree, alternating, --ab-rounds times each.

  python tools/image_stats_cost.py [--calls 40] [--warmup 10] [--parent-tree DIR] [--out profiles/image_stats_cost.txt]
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
    sys.exit("image_stats_cost: the HIP runtime is not loaded")


def headline(tree):
    """One bench.py run in `tree`, a fresh process: (ms per step, rays / s, CoV of the repeats)."""
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5", "--repeats", "5"], cwd=tree, capture_output=True, text=True,
                       timeout=600)
    if r.returncode != 0:
        sys.exit("image_stats_cost: bench.py failed in %s\n%s" % (tree, r.stderr[-2000:]))
    doc = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    return doc["ms_per_step"], doc["value"], doc["repeats"]["cov"], doc["repeats"]["ms_per_step_all"]


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
    from ice_halo_sim_amd import abi, backend
    from tests import _ev_auto_model as M
    L = backend.load_library()
    if L.halo_device_count() <= 0:
        sys.exit("image_stats_cost: no GPU — this is a measurement, it does not fall back")
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

    def lognormal(w, h, seed):
        return np.exp(np.random.default_rng(seed).normal(0.0, 4.0, (h, w))).astype(np.float32)

    def groups(s):
        """Distinct prefixes among the distinct ranks after the first and after the second digit: the histograms of the second and third."""
        pats = {np.float32(v).view(np.uint32) for v in s["lo"] + s["hi"]}
        return len({int(p) >> 21 for p in pats}), len({int(p) >> 10 for p in pats})

    eleven = abi.STATS_TOOL_PERCENTILES
    w, h = 1920, 1080
    fmt = "  %-58s device %7.3f (%7.3f) ms   wall %7.3f (%7.3f) ms"
    lines = ["halo_consumer_stats at %d x %d: median (min) over %d calls after %d warm-up calls; device ms = HIP events around the call's stream work, "
             "wall ms = host clock around the call" % (w, h, args.calls, args.warmup)]
    for name, y in (("sparse (2 % lit)", M.recipe_image(w, h, 19, 0.02, 0.1, -2, 0)), ("dense", M.recipe_image(w, h, 19, 1.0, 0.0, -2, 0)),
                    ("dense log-normal, sigma = 4", lognormal(w, h, 5))):
        xyz = np.zeros((h, w, 3), np.float32)
        xyz[..., 1] = y
        hb.ResetConsumer()
        hb.Consume(xyz, 0.01 * w * h)
        lines += ["", "image: %s" % name]
        d, dm, wl, wm, _ = timed(lambda: hb.Snapshot(want_xyz=False))
        lines.append(fmt % ("halo_consumer_snapshot (rgb out, 6.2 MB copied back)", d, dm, wl, wm))
        d, dm, wl, wm, a = timed(lambda: hb.AutoEv(1))
        lines.append(fmt % ("halo_consumer_auto_ev f = 1", d, dm, wl, wm))
        d, dm, wl, wm, s0 = timed(lambda: hb.ImageStats(()))
        lines.append(fmt % ("halo_consumer_stats, no percentile (moments only)", d, dm, wl, wm))
        d, dm, wl, wm, s = timed(lambda: hb.ImageStats(eleven))
        lines.append(fmt % ("halo_consumer_stats, the tool's eleven percentiles", d, dm, wl, wm))
        assert (s0["sum"], s0["sum_sq"], s0["positive_count"]) == (s["sum"], s["sum_sq"], s["positive_count"]) and s["positive_count"] == a["value_count"]
        g1, g2 = groups(s)
        lines.append("    -> %d positive values, %d + %d groups on the second / third digit: 1 + %d + %d sweeps; P50 %.6g P99 %.6g P99.5 %.6g (of norm), mean %.6g, cv %.4g"
                     % (s["positive_count"], g1, g2, -(-g1 // 7), -(-g2 // 14), s["percentiles"][0], s["percentiles"][4], s["percentiles"][6], s["mean"], s["cv"]))
    hb.close()
    lines += ["", "one workgroup against the multi-block form, dense values, the eleven percentiles (the threshold kStatsSmallMax of halo_launch.h comes from here)"]
    for sw, sh in ((32, 32), (64, 64), (128, 64), (128, 128), (240, 135), (256, 256)):   # 1 Ki .. 64 Ki values
        for name, y in (("recipe", M.recipe_image(sw, sh, 23, 1.0, 0.0, -2, 0)), ("log-normal", lognormal(sw, sh, 6))):
            hs = backend.HipTraceBackend(device=0, seed=1)
            hs.set_stream(stream.value)
            xyz = np.zeros((sh, sw, 3), np.float32)
            xyz[..., 1] = y
            hs.Consume(xyz, 0.01 * sw * sh)
            res = []
            for select in (1, 0):
                hs.set_option("stats_select", select)
                res.append(timed(lambda: hs.ImageStats(eleven)))
            assert res[0][4] == res[1][4]
            lines.append("  %7d values, %-10s: one workgroup device %7.3f (%7.3f) ms   multi-block device %7.3f (%7.3f) ms"
                         % (sw * sh, name, res[0][0], res[0][1], res[1][0], res[1][1]))
            hs.close()
    if args.parent_tree:
        lines += ["", "headline: bench.py --gpus 1 --steps 20 --warmup 5 --repeats 5, the parent commit's tree and this one alternating, a fresh process each"]
        ms = {"parent": [], "this": []}
        for k in range(args.ab_rounds):
            for who, tree in (("parent", args.parent_tree), ("this", ROOT)):
                m, v, cov, every = headline(tree)
                ms[who].append(m)
                lines.append("  %-6s run %d   ms_per_step %8.4f   rays/s %.4e   CoV of 5 repeats %.5f   repeats %s" % (who, k + 1, m, v, cov, " ".join("%.4f" % x for x in every)))
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
