"""Price of canonical continuation order (option cont_order = 1) on configs[2]'s step: plate at prob 1 over a random column, 9 wavelengths x
--rays root rays, fisheye 1920x1080 upper — bench.py --config 2's work, traced here directly because bench.py has no option for it.

  python tools/canonical_order_probe.py [--rays 50000000] [--steps 3] [--orders 0,1]
  rocprofv3 --kernel-trace --stats -d DIR -o probe -- python tools/canonical_order_probe.py --orders 1 --steps 1

Each order runs on its own backend: one untimed warm-up step, then --steps timed steps (host wall time, synchronised at the end of each step),
alternating between the orders step by step so drift hits both alike.  Prints ms per step (median) and the difference."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ice_halo_sim_amd import scenes  # noqa: E402
from ice_halo_sim_amd.backend import HipTraceBackend  # noqa: E402


def step(hb, sc, rd, wls, n):
    cont = 0
    for wl in wls:
        hb.BeginSession(sc, rd, wl, n)
        for li in range(sc.layer_count):
            s = hb.TraceLayer(n if li == 0 else 0)
            if li + 1 < sc.layer_count:
                cont += s.continuation_count
                hb.Recombine(True)
        hb.EndSession()
    hb.sync()
    return cont


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=50_000_000)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--orders", default="0,1")
    a = ap.parse_args()
    sc, rd = scenes.config3_scene(), scenes.config2_render()
    wls = [scenes.wl_discrete(w) for w in scenes.CONFIG_WAVELENGTHS_9]
    orders = [int(x) for x in a.orders.split(",")]
    bes = {o: HipTraceBackend(device=0, seed=42, cont_order=o) for o in orders}
    for o in orders:
        step(bes[o], sc, rd, wls, a.rays)
    ms = {o: [] for o in orders}
    conts = {}
    for _ in range(a.steps):
        for o in orders:
            t = time.perf_counter()
            conts[o] = step(bes[o], sc, rd, wls, a.rays)
            ms[o].append(1e3 * (time.perf_counter() - t))
    for o in orders:
        print("cont_order=%d: %.2f ms per step (median of %s), %d continuations per step" % (o, statistics.median(ms[o]), ["%.2f" % x for x in ms[o]], conts[o]))
        bes[o].close()
    if len(orders) == 2:
        m0, m1 = statistics.median(ms[orders[0]]), statistics.median(ms[orders[1]])
        print("difference: %+.2f ms per step (%+.1f %%)" % (m1 - m0, 100.0 * (m1 - m0) / m0))


if __name__ == "__main__":
    main()
