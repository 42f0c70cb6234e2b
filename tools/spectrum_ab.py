#!/usr/bin/env python3
"""A/B of the two ways to trace a discrete spectrum, on the GPU, in one process:

  (a) one session per wavelength — what `bench.py --config 4d` measures and `cli.run_job` does by default;
  (b) one spectrum session for the whole list (HipTraceBackend.BeginSpectrumSession, `cli --spectrum-session`).

Scene: configs[4]'s — the stochastic prism entry of examples/bench_config_stoch.json, full-sphere axis, max_hits 8, rectangular 2048 x 1024,
full sky.  Spectrum: 31 entries 380..780 nm weighted by the D65 SPD (halo_host_illuminant_spd), 806 452 roots per entry and step — the
numbers of bench.py's 4d.  Both variants run on ONE backend with the options bench.py gives its tracer (dist.ShardedTracer: async = 1, a bound
accumulator with defer_fold = 1, one drain per step), take turns step by step in the warm-up (until two chunks of each agree within 5 %) and
region by region in the timed part (>= 5 regions each, every region closed by a device synchronise), and report median, min, max and CoV of the
regions' ms per step, the ratio of the medians, the launches per step, and how the two images compare (same spectrum, same seed, other rays per
entry: the block of entry k starts at another counter — a statistical comparison, not a bitwise one).

  python tools/spectrum_ab.py [--steps 10] [--regions 7] [--rays-per-wl 806452] [--out profiles/spectrum_session_ab.txt]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10, help="steps per timed region")
    ap.add_argument("--regions", type=int, default=7, help="timed regions per variant (at least 5)")
    ap.add_argument("--rays-per-wl", type=int, default=-(-25_000_000 // 31))
    ap.add_argument("--out", default="", help="also write the report here")
    args = ap.parse_args()
    if args.regions < 5:
        ap.error("--regions must be at least 5")
    import numpy as np
    import torch
    from ice_halo_sim_amd import abi, backend, scenes
    from ice_halo_sim_amd.dist import ShardedTracer
    if not torch.cuda.is_available():
        sys.exit("spectrum_ab: no GPU — this is a measurement, it does not fall back")
    L = backend.load_library()
    lam = [380.0 + 400.0 * i / 30.0 for i in range(31)]
    wls = [scenes.wl_discrete(w, float(L.halo_host_illuminant_spd(abi.ILLUM["D65"], w))) for w in lam]
    sc = scenes.scene([(0.0, [scenes.stochastic_prism_entry()])], max_hits=8)
    rd = scenes.render(abi.LENS_RECTANGULAR, 2048, 1024, el=0.0, visible=abi.VISIBLE_FULL)
    n = args.rays_per_wl
    tracer = ShardedTracer(sc, rd, seed=42, device=0, rank=0, world=1, **{"async": 1})
    b = tracer.backend
    routes = {}

    def step_a():
        for wl in wls:
            tracer.trace_session_layers(wl, n)
        routes["a"] = b.last_route()
        tracer.reduce_to_root()

    def step_b():
        b.BeginSpectrumSession(sc, rd, wls, len(wls) * n)
        b.TraceLayer(len(wls) * n)
        b.EndSession()
        routes["b"] = b.last_route()
        tracer.reduce_to_root()

    variants = {"a": step_a, "b": step_b}

    def region(name):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            variants[name]()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.steps * 1e3

    # warm-up: both variants in turn, until two consecutive chunks of EACH agree within 5 % (at least 1 s, at most 8 s in all)
    t_w, last, warm = time.perf_counter(), {}, 0
    while True:
        ok = True
        for name in variants:
            ms = region(name)
            ok = ok and name in last and abs(ms - last[name]) <= 0.05 * ms
            last[name] = ms
        warm += 1
        el = time.perf_counter() - t_w
        if (ok and el >= 1.0) or el > 8.0:
            break
    # one step of each on a clean accumulator: the images and the tallies of a step
    images, tallies = {}, {}
    for name in variants:
        tracer.zero()
        b.collect_stats()
        b.collect_timing()
        variants[name]()
        torch.cuda.synchronize()
        st = b.collect_stats()
        trace_ms, post_ms, launches = b.collect_timing()
        images[name] = tracer.total()[: rd.width * rd.height * 3].double().cpu().numpy().reshape(rd.height, rd.width, 3)
        tallies[name] = dict(roots=int(st.root_count), exits=int(st.exit_count), pixel_hits=int(st.pixel_hits), launches=int(st.launches), trace_ms=trace_ms, post_ms=post_ms,
                             timed_dispatches=int(launches), landed=tracer.backend.take_landed())
    tracer.zero()
    times = {name: [] for name in variants}
    for _ in range(args.regions):
        for name in variants:          # a, b, a, b, ...: the two see the same machine
            times[name].append(region(name))
    lines = []
    out = lines.append
    rays = len(wls) * n
    out("spectrum session A/B: configs[4]'s scene (stochastic prism, full-sphere axis, max_hits 8, rectangular 2048x1024 full sky), 31 entries 380..780 nm x D65 SPD,")
    out("%d roots per entry = %d roots per step; one backend, options of bench.py's tracer (async = 1, bound accumulator, defer_fold = 1), one drain per step" % (n, rays))
    out("warm-up: %d rounds of %d steps of each variant (until two rounds agree within 5 %%); timed: %d regions of %d steps each, alternating a, b" % (warm, args.steps, args.regions, args.steps))
    out("")
    med = {}
    for name, what in (("a", "31 discrete sessions (bench.py --config 4d's path)"), ("b", "one spectrum session")):
        t = times[name]
        med[name] = statistics.median(t)
        out("(%s) %-52s ms/step median %.3f  min %.3f  max %.3f  CoV %.2f %%  -> %.3f G rays/s   regions: %s" % (
            name, what, med[name], min(t), max(t), 100.0 * statistics.pstdev(t) / statistics.mean(t), rays / med[name] / 1e6, " ".join("%.3f" % x for x in t)))
    out("(b)/(a) time per step: %.3f   (a)/(b) = speed-up of the spectrum session: %.2fx" % (med["b"] / med["a"], med["a"] / med["b"]))
    out("")
    for name in variants:
        r, y = routes[name], tallies[name]
        out("(%s) one step: roots %d, exits %d, pixel hits %d, kernel launches %d (trace kernels %d per session, route of the last session: accum_mask 0x%x, planes %d, geom_mask 0x%x, spec_mask 0x%x), "
            "last-layer trace kernels %.3f ms + accumulation passes %.3f ms over %d timed dispatches, landed %.6g" % (
                name, y["roots"], y["exits"], y["pixel_hits"], y["launches"], r.launches, r.accum_mask, r.plane_cnt, r.geom_mask, r.spec_mask, y["trace_ms"], y["post_ms"],
                y["timed_dispatches"], y["landed"]))
    ia, ib = images["a"], images["b"]
    k = 8
    bm = lambda im: im[: im.shape[0] // k * k, : im.shape[1] // k * k].reshape(im.shape[0] // k, k, im.shape[1] // k, k, 3).mean(axis=(1, 3))
    out("images of one step (other rays per entry, so statistical): channel sums b/a  X %.5f  Y %.5f  Z %.5f;  8x8 block-mean rel L2 %.4f;  landed b/a %.6f" % (
        ib[..., 0].sum() / ia[..., 0].sum(), ib[..., 1].sum() / ia[..., 1].sum(), ib[..., 2].sum() / ia[..., 2].sum(),
        float(np.linalg.norm(bm(ib) - bm(ia)) / np.linalg.norm(bm(ia))), tallies["b"]["landed"] / tallies["a"]["landed"]))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
