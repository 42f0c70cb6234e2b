"""Price of option deterministic = 1 (fixed-point accumulation: bit-reproducible images) on the benchmark's steps: configs[1], configs[2] with
cont_order = 1 (a deterministic multi-layer session needs it, so both sides run it) and configs[4] — bench.py's work, traced here directly
because bench.py has no option for it.

  python tools/deterministic_probe.py [--configs 1,2,4] [--steps 5] [--scale 1.0] [--readings off,direct,log,auto] [--out profiles/deterministic_cost.txt]

Readings: off = deterministic 0; direct = deterministic 1 with hit_log 0 (every miss a 64-bit integer atomic); log = deterministic 1 with
hit_log 1 (misses leave as records, the integer per-tile passes sum them); auto = deterministic 1 with hit_log -1 (the backend's own choice).
Each reading runs on its own backend in one process: one untimed warm-up step, then --steps timed steps (host wall time, synchronised at the
end of each step), alternating between the readings step by step so drift hits all alike.  Prints ms per step (median, min .. max) and the
difference to the first reading, and the sha256 of the image of the last step (equal between the deterministic readings and from run to run;
the float side's differs)."""
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


READINGS = {"off": dict(deterministic=0), "direct": dict(deterministic=1, hit_log=0), "log": dict(deterministic=1, hit_log=1), "auto": dict(deterministic=1, hit_log=-1)}


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
    ap.add_argument("--readings", default="off,direct,log", help="comma list of off, direct, log, auto")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []
    for cfg in a.configs.split(","):
        w = workload(cfg)
        n = max(1, int(w["rays"] * a.scale))
        multi = w["scene"].layer_count > 1
        names = a.readings.split(",")
        bes = {r: HipTraceBackend(device=0, seed=42, cont_order=int(multi), **READINGS[r]) for r in names}
        for r in names:
            bes[r].set_option("ray_base", 0)
            step(bes[r], w, n)
            bes[r].ReadbackXyzAccum()
        ms = {r: [] for r in names}
        for _ in range(a.steps):
            for r in names:
                t = time.perf_counter()
                step(bes[r], w, n)
                ms[r].append(1e3 * (time.perf_counter() - t))
        for r in names:
            img, _ = bes[r].ReadbackXyzAccum()
            sha = hashlib.sha256(img.tobytes()).hexdigest()[:16]
            mask = bes[r].last_route().accum_mask
            lines.append("configs[%s]%s %s: %.3f ms per step (median; %.3f .. %.3f over %d steps), %d sessions x %d rays, accum_mask 0x%x, xyz sha256 %s" %
                         (cfg, " cont_order=1" if multi else "", r, statistics.median(ms[r]), min(ms[r]), max(ms[r]), len(ms[r]), len(w["wls"]), n, mask, sha))
            bes[r].close()
        m0 = statistics.median(ms[names[0]])
        for r in names[1:]:
            m1 = statistics.median(ms[r])
            lines.append("configs[%s] %s against %s: %+.3f ms per step (%+.1f %%)" % (cfg, r, names[0], m1 - m0, 100.0 * (m1 - m0) / m0))
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
