"""Measures the margins and bar constants of tests/_hit_model.py and writes tests/golden/HIT_MARGINS.md.

    python -m tests.golden.make_hit_margins

Both oracle builds (uncontracted, FMA-contracted) against the float64 model with every margin at zero, on batches several times the tests':
per crystal and hit budget MEASURE_SEEDS directed probe sets of MEASURE_PER_CLASS per class and MEASURE_RANDOM rays of random incidence,
under both next-face strategies.  A ray whose record set (seq, path length, path bytes) differs from the model's is charged to the decision
it came closest to; the largest such distance per kind is MEASURED[kind].  The worst error of an exit of an agreeing ray, in units of the
model's conditioning (units()), is MEASURED_BAR.  Copy the two dicts into tests/_hit_model.py; tests/test_hit_model.py holds them equal."""
import os
import time

import numpy as np

from tests import _hit_model as M
from tests import _libs

ZERO = {k: -1.0 for k in M.KINDS}


def up(x):
    """x rounded up to three significant digits."""
    if x <= 0.0:
        return 0.0
    e = int(np.floor(np.log10(x))) - 2
    return float("%.3g" % (np.ceil(x / 10.0 ** e) * 10.0 ** e))


def main():
    L = _libs.oracle()
    n_idx = M.refractive_index(L)
    worst = {k: 0.0 for k in M.KINDS}
    bar = {"dir": 0.0, "weight": 0.0}
    rows = []
    t0 = time.time()
    for name, cr in M.crystals():
        g = M.geometry_of(cr, L)
        sets = [("probes seed %d" % s, M.probes(g, n_idx, s, M.MEASURE_PER_CLASS, plate_tir=(name == "plate"))) for s in M.MEASURE_SEEDS]
        sets.append(("random seed 21", M.random_rays(g, M.MEASURE_RANDOM, 21)))
        for mh in M.budgets(name):
            for strategy in (1, 0):
                n_rays = n_bad = n_exits = 0
                w_case = {k: 0.0 for k in M.KINDS}
                b_case = {"dir": 0.0, "weight": 0.0}
                for label, rays in sets:
                    R = M.trace(g, n_idx, rays["d"], rays["p"], rays["w"], rays["face"], mh, strategy)
                    ud, uw = M.units(R.exits)
                    for fma in (False, True):
                        c = M.compare(R, M.oracle_records(fma, cr, g, rays, mh, strategy))
                        bad = c["bad_root"]
                        for k, v in M.charge(R, bad).items():
                            w_case[k] = max(w_case[k], v)
                        ok = ~R.unstable[R.exits.root[c["im"]]]
                        im = c["im"][ok]
                        with np.errstate(invalid="ignore", divide="ignore"):
                            rd, rw = c["err_dir"][ok] / ud[im], np.where(c["err_w"][ok] > 0, c["err_w"][ok] / uw[im], 0.0)
                        b_case["dir"] = max(b_case["dir"], float(rd.max(initial=0.0)))
                        b_case["weight"] = max(b_case["weight"], float(rw.max(initial=0.0)))
                        n_rays += R.n
                        n_bad += int(bad.sum())
                        n_exits += len(im)
                for k in M.KINDS:
                    worst[k] = max(worst[k], w_case[k])
                for k in bar:
                    bar[k] = max(bar[k], b_case[k])
                rows.append("| %s | %d | %d | %d | %d | %d | %s | %.3g | %.3g |" % (name, mh, strategy, n_rays, n_bad, n_exits,
                                                                                 " ".join("%.3g" % w_case[k] for k in M.KINDS), b_case["dir"], b_case["weight"]))
                print(rows[-1], "%.0f s" % (time.time() - t0), flush=True)
    measured = {k: up(worst[k]) for k in M.KINDS}
    measured_bar = {k: up(bar[k]) for k in bar}
    out = ["# Hit-loop margins", "",
           "Measured by `python -m tests.golden.make_hit_margins`: both oracle builds against the float64 model of `tests/_hit_model.py`, every margin at zero.",
           "Batches per crystal, hit budget and strategy: directed probes with seeds %s at %d per class, and %d rays of random incidence (seed 21), each under the uncontracted and the FMA-contracted build." %
           (", ".join(str(s) for s in M.MEASURE_SEEDS), M.MEASURE_PER_CLASS, M.MEASURE_RANDOM),
           "The tests' own batch is seed %d at %d per class.  `rays` counts ray x build; `differ` the rays whose record set is not the model's; `exits` the compared exits." % (M.TEST_SEED, M.TEST_PER_CLASS),
           "A differing ray is charged to the kind it came closest to, each distance divided by that kind's scale: CHARGE_SCALE = %r." % M.CHARGE_SCALE,
           "", "The constants (rounded up to three digits); DELTA and K are %g times these:" % M.FACTOR, "", "```",
           "MEASURED = %r" % measured, "MEASURED_BAR = %r" % measured_bar, "```", "",
           "| crystal | max_hits | rehit_strategy | rays | differ | exits | largest distance of a differing ray: %s | dir err / unit | weight err / unit |" % " ".join(M.KINDS),
           "|---|---|---|---|---|---|---|---|---|"] + rows
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "HIT_MARGINS.md")
    with open(path, "w") as f:
        f.write("\n".join(out) + "\n")
    print("MEASURED = %r\nMEASURED_BAR = %r" % (measured, measured_bar))


if __name__ == "__main__":
    main()
