"""Price of option deterministic = 1 (fixed-point accumulation: bit-reproducible images) on the benchmark's steps: configs[1], configs[2] with
cont_order = 1 (a deterministic multi-layer session needs it, so both sides run it) and configs[4] — bench.py's work, traced here directly
because bench.py has no option for it.

  python tools/deterministic_probe.py [--configs 1,2,4] [--steps 5] [--scale 1.0] [--out profiles/deterministic_cost.txt]

Each side runs on its own backend in one process: one untimed warm-up step, then --steps timed steps (host wall time, synchronised at the end
of each step), alternating between off and on step by step so drift hits both alike.  Prints ms per step (median) and the difference, and the
sha256 of the image of the last deterministic step (equal from run to run; the float side's differs)."""
import argparse
import hashlib
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench import workload  # noqa: E402
from ice_halo_sim_amd.backend import HipTraceBackend  # noqa: E402


def step(hb, w, n):
    sc = w["scene"]
    for wl in w["wls"]:
        hb.BeginSession(sc, w["render"], wl, n)
        for li in range(sc.layer_count):
            hb.TraceLayer(n if li == 0 else 0)
            if li + 1 < sc.layer_count:
                hb.Recombine(True)
        hb.EndSession()
    hb.sync()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="1,2,4")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of the configuration's rays per session")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []
    for cfg in a.configs.split(","):
        w = workload(cfg)
        n = max(1, int(w["rays"] * a.scale))
        multi = w["scene"].layer_count > 1
        bes = {d: HipTraceBackend(device=0, seed=42, cont_order=int(multi), deterministic=d) for d in (0, 1)}
        for d in (0, 1):
            bes[d].set_option("ray_base", 0)
            step(bes[d], w, n)
            bes[d].ReadbackXyzAccum()
        ms = {0: [], 1: []}
        for _ in range(a.steps):
            for d in (0, 1):
                t = time.perf_counter()
                step(bes[d], w, n)
                ms[d].append(1e3 * (time.perf_counter() - t))
        sha = {}
        for d in (0, 1):
            img, _ = bes[d].ReadbackXyzAccum()
            sha[d] = hashlib.sha256(img.tobytes()).hexdigest()[:16]
            mask = bes[d].last_route().accum_mask
            lines.append("configs[%s]%s deterministic=%d: %.2f ms per step (median of %s), %d sessions x %d rays, accum_mask 0x%x, xyz sha256 %s" %
                         (cfg, " cont_order=1" if multi else "", d, statistics.median(ms[d]), ["%.2f" % x for x in ms[d]], len(w["wls"]), n, mask, sha[d]))
            bes[d].close()
        m0, m1 = statistics.median(ms[0]), statistics.median(ms[1])
        lines.append("configs[%s] difference: %+.2f ms per step (%+.1f %%)" % (cfg, m1 - m0, 100.0 * (m1 - m0) / m0))
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
