"""The float64 model of the interaction loop (tests/_hit_model.py) against the fp32 code that is the truth on the host: both builds of the
oracle (uncontracted and FMA-contracted), under both next-face strategies, on directed probes of every class on every crystal and hit budget.

No fraction anywhere: every probe the model calls decidable has the model's exit set — seq, path length, path bytes — in both builds, and
every exit of such a probe the model's direction and weight within the model's bar.  The margins and the two bar constants the model commits
are four times what this comparison measures on batches several times this size (tests/golden/make_hit_margins.py, recorded in
tests/golden/HIT_MARGINS.md), and what they leave out is capped here, on the host, where the reference side alone decides it.
tests/test_gpu_hit_loop.py then holds the device to the same model."""
import ast
import os
import re

import numpy as np
import pytest

from tests import _hit_model as M
from tests import _libs

CRYSTALS = M.crystals()
NAMES = [c[0] for c in CRYSTALS]
CASES = [(name, mh, s) for name in NAMES for mh in M.budgets(name) for s in (1, 0)]

_cache = {}


def _probes(name):
    if ("p", name) not in _cache:
        cr = dict(CRYSTALS)[name]
        L = _libs.oracle()
        g = M.geometry_of(cr, L)
        _cache["p", name] = (cr, g, M.probes(g, M.refractive_index(L), M.TEST_SEED, M.TEST_PER_CLASS, plate_tir=(name == "plate")))
    return _cache["p", name]


def _batch(name, strategy):
    """(crystal, tables, probes) that strategy is held on: everything under rehit_strategy 1; under 0 the classes of M.STRATEGY0_CLASSES,
    narrowed to the probes whose own outgoing-child decision is a margin clear by construction (scope0 in M.probes())."""
    cr, g, pr = _probes(name)
    if strategy == 0:
        pr = {k: v[pr["scope0"]] for k, v in pr.items()}
        pr["must"] = pr["must0"]
    return cr, g, pr


def _model(name, mh, strategy):
    if (name, mh, strategy) not in _cache:
        cr, g, pr = _batch(name, strategy)
        _cache[name, mh, strategy] = M.trace(g, M.refractive_index(_libs.oracle()), pr["d"], pr["p"], pr["w"], pr["face"], mh, strategy)
    return _cache[name, mh, strategy]


def _describe(R, pr, k):
    return (int(k), M.CLASSES[pr["cls"][k]], {q: float("%.3g" % R.dist[q][k]) for q in M.KINDS})


@pytest.mark.parametrize("name,mh,strategy", CASES, ids=["%s-%d-s%d" % c for c in CASES])
def test_both_oracle_builds_have_the_models_exits_on_every_decidable_probe(name, mh, strategy):
    cr, g, pr = _batch(name, strategy)
    R = _model(name, mh, strategy)
    ok = R.decidable()
    E = R.exits
    bd, bw = M.bars(E)
    worst = {k: 0.0 for k in M.KINDS}
    for fma in (False, True):
        c = M.compare(R, M.oracle_records(fma, cr, g, pr, mh, strategy))
        bad = np.flatnonzero(c["bad_root"] & ok)
        assert len(bad) == 0, (fma, [_describe(R, pr, k) for k in bad[:6]])
        # direction and weight of every exit of a decidable probe, within the model's bar
        sel = ok[E.root[c["im"]]]
        im = c["im"][sel]
        over = np.flatnonzero((c["err_dir"][sel] > bd[im]) | (c["err_w"][sel] > bw[im]))
        assert len(over) == 0, (fma, [(_describe(R, pr, E.root[im[j]]), int(E.seq[im[j]]), float(c["err_dir"][sel][j]), float(bd[im[j]]), float(c["err_w"][sel][j]),
                                       float(bw[im[j]])) for j in over[:6]])
        # an entry face outside the body's, and nothing else, gives no record
        none = np.bincount(c["rec"]["root"].astype(np.int64), minlength=R.n) == 0
        assert none[pr["cls"] == M.CLASSES.index("badface")].all()
        for k, v in M.charge(R, c["bad_root"]).items():
            worst[k] = max(worst[k], v)
    # the margins are what was measured: every disagreement lies within MEASURED (a quarter of DELTA) of a decision of its kind
    for k in M.KINDS:
        assert worst[k] <= M.MEASURED[k], (k, worst[k], M.MEASURED[k])
    print("%s max_hits %d strategy %d: %d probes, %d left out %s" % (name, mh, strategy, R.n, int((~ok).sum()), _left_out(R)))
    # what may be left out, under either strategy: at most one third of the batch, and no probe built well away from the boundary its class probes
    assert (~ok).mean() <= 1.0 / 3.0, (~ok).mean()
    lost = np.flatnonzero(pr["must"] & ~ok)
    assert len(lost) == 0, [_describe(R, pr, k) for k in lost[:6]]
    assert pr["must"].sum() >= 150 and len(pr["w"]) >= 300


def _left_out(R):
    """{kind: probes within that kind's margin}; a probe near two decisions counts under both."""
    out = {k: int((R.dist[k] <= M.DELTA[k]).sum()) for k in M.KINDS}
    out["unstable"] = int(R.unstable.sum())
    return out


def test_margins_and_bar_constants_are_four_times_what_was_measured_and_recorded():
    assert M.FACTOR == 4.0 and set(M.DELTA) == set(M.KINDS) == set(M.MEASURED)
    for k in M.KINDS:
        assert M.DELTA[k] == 4.0 * M.MEASURED[k]
    assert M.K_DIR == 4.0 * M.MEASURED_BAR["dir"] and M.K_W == 4.0 * M.MEASURED_BAR["weight"]
    text = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "HIT_MARGINS.md")).read()
    rec = {name: ast.literal_eval(body) for name, body in re.findall(r"^(MEASURED(?:_BAR)?) = (\{[^}]*\})$", text, re.M)}
    assert rec == {"MEASURED": M.MEASURED, "MEASURED_BAR": M.MEASURED_BAR}, rec
    assert "CHARGE_SCALE = %r" % M.CHARGE_SCALE in text
    # the record names the batches it was measured on
    for s in M.MEASURE_SEEDS:
        assert str(s) in text
    assert "%d per class" % M.MEASURE_PER_CLASS in text and "%d rays of random incidence" % M.MEASURE_RANDOM in text
    assert M.MEASURE_PER_CLASS * len(M.MEASURE_SEEDS) >= 4 * M.TEST_PER_CLASS


def test_bars_are_never_looser_than_the_projects_where_nothing_loses_digits():
    """An exit whose conditioning terms are zero — an external reflection, a path through well-conditioned refractions — is held tighter than
    the project's per-ray bars (direction 2e-5 per component, weight 2e-4 relative)."""
    for name in ("regular", "pyramid"):
        R = _model(name, 8, 1)
        E = R.exits
        bd, bw = M.bars(E)
        first = (E.depth == 1) & (E.weight > 0)
        assert first.any() and (E.cond_dir[first] == 0).all()            # an external reflection's direction takes nothing from dd
        assert (bd[first] <= 2e-5 / 8).all()
        # "zero" for a weight: at the level of its own rounding (a reflected weight does take R from dd, to a few ulp when dd is well known)
        calm = (E.cond_dir <= 1e-6) & (E.cond_w + E.aw <= 2e-6 * np.abs(E.weight)) & (E.weight > 1e-3) & R.decidable()[E.root]
        assert calm.mean() > 0.2 and (calm & first).sum() > 100
        assert (bd[calm] <= 2e-5).all() and (bw[calm] <= 2e-4 * np.abs(E.weight[calm])).all(), (bd[calm].max(), (bw[calm] / E.weight[calm]).max())


def test_probe_sets_cover_their_classes():
    for name in NAMES:
        cr, g, pr = _probes(name)
        Gm = M.Geom(g)
        cnt = np.bincount(pr["cls"], minlength=len(M.CLASSES))
        assert (cnt > 0).all(), (name, dict(zip(M.CLASSES, cnt.tolist())))
        assert 800 <= len(pr["w"]) <= 4000
        normal = pr["face"][pr["cls"] == M.CLASSES.index("normal")]
        assert set(normal.tolist()) == set(range(Gm.F))                       # normal incidence on every face
        R8 = _model(name, 8, 1)
        # grazing: both sides of the margin; critical: TIR and not, decidably; parallel: den either side of the gate, decidably
        gz = pr["cls"] == M.CLASSES.index("grazing")
        assert (R8.dist["entry"][gz] < 1e-3).any() and (pr["must"] & gz).sum() >= 20
        ok = R8.decidable()
        E = R8.exits
        cr_ = np.flatnonzero((pr["cls"] == M.CLASSES.index("critical")) & ok)
        has3 = np.isin(cr_, E.root[E.seq == 3])
        assert has3.any() and (~has3).any(), name                          # the second interaction refracts out, or reflects totally
        # off-plane entries: both sides of the stray threshold, and under strategy 0 parked children that go on to leave
        off = pr["cls"] == M.CLASSES.index("offplane")
        sides = (pr["p"][off].astype(np.float64) * Gm.n[pr["face"][off]]).sum(1) + Gm.c[pr["face"][off]]
        assert (sides > 1.2 * M.EPS).any() and (sides < -1.2 * M.EPS).any() and (np.abs(sides) < 0.8 * M.EPS).any()
        R0 = _model(name, 8, 0)                                            # (on the scoped batch: its roots count within scope0)
        at = np.cumsum(pr["scope0"]) - 1
        offs = np.flatnonzero(off & pr["scope0"])
        parted = [k for k in offs if sorted(R8.exits.key()[R8.exits.root == k] & 0xFFFFFF) != sorted(R0.exits.key()[R0.exits.root == at[k]] & 0xFFFFFF)]
        assert len(parted) >= 4, name                                      # the two strategies part ways on this class
        # every class has its `must` subset, both sides of its decision where it has two
        for c, least in (("normal", Gm.F), ("random", 100), ("grazing", 20), ("critical", 5), ("edge", 10), ("vertex", 5), ("parallel", 10), ("offplane", 16),
                         ("badface", 8), ("zero_weight", 4)):
            sel = pr["must"] & (pr["cls"] == M.CLASSES.index(c))
            assert sel.sum() >= least, (name, c, int(sel.sum()))
            if c in ("critical", "edge", "parallel", "offplane"):
                assert {-1, 1} <= set(pr["side"][sel].tolist()), (name, c)
        # ... and the decidable probes of the aimed classes do reach their decision: an edge of the next face from both sides and a vertex, within
        # 30 margins of the face kind; a skimmed face with n.d within a fifth of 1e-5 on both sides of it
        for c, kind, reach in (("edge", "face", 30 * M.DELTA["face"]), ("vertex", "face", 30 * M.DELTA["face"]), ("parallel", "gate", 0.2 * M.EPS)):
            sel = ok & (pr["cls"] == M.CLASSES.index(c)) & (R8.dist[kind] <= reach)
            assert {-1, 1} <= set(pr["side"][sel].tolist()), (name, c, int(sel.sum()))
        assert (pr["must0"] & pr["scope0"] & off).sum() >= 8 and {-1, 1} <= set(pr["side"][pr["must0"] & off].tolist()), name
    # the plate's long budget crosses the 16 faces of the path register
    Rp = _model("plate", M.PLATE_BUDGET, 1)
    Ep = Rp.exits
    okp = Rp.decidable()[Ep.root]
    assert (Ep.path_len[okp] == 16).any() and (Ep.path_len[okp] == 17).any() and (Ep.path_len[okp] >= 20).any()


@pytest.mark.ref
@pytest.mark.parametrize("name", NAMES)
def test_models_face_distance_and_reflect_ratio_equal_the_references_on_the_probes_own_operands(name):
    """ref_slab_face_t and ref_reflect_ratio (the reference's shared-math headers) on the operands of the probes' first search and split:
    the model's t and R within fp32 rounding of them (err(t) of the model's `face` distance; a few ulp of R), the den <= 1e-5 gate exactly."""
    if not _libs.have_ref():
        pytest.skip("oracle/_ref is not built here (the reference's sources are absent)")
    Rf = _libs.ref()
    cr, g, pr = _probes(name)
    Gm = M.Geom(g)
    n_idx = float(M.refractive_index(_libs.oracle()))
    rng = np.random.default_rng(3)
    checked = 0
    for k in rng.choice(len(pr["w"]), 300, replace=False):
        f = int(pr["face"][k])
        if f >= Gm.F:
            continue
        d, p = np.ascontiguousarray(pr["d"][k]), np.ascontiguousarray(pr["p"][k])
        for fi in range(Gm.F):
            nf = np.ascontiguousarray(Gm.n[fi], np.float32)
            t_ref = Rf.ref_slab_face_t(_libs.fptr(d), _libs.fptr(p), _libs.fptr(nf), float(Gm.c[fi]))
            den = float(d.astype(np.float64) @ Gm.n[fi])
            if abs(den - M.EPS) <= 4 * M.U:
                continue
            if den <= M.EPS:
                assert t_ref == np.float32(1e30), (k, fi, den, t_ref)
                continue
            t = -(p.astype(np.float64) @ Gm.n[fi] + Gm.c[fi]) / den
            err = (2 * M.U * (np.abs(p * Gm.n[fi]).sum() + abs(Gm.c[fi])) + abs(t) * 2 * M.U * np.abs(d * Gm.n[fi]).sum()) / den
            assert abs(t_ref - t) <= 2.0 * err + abs(t) * 2 * M.U, (k, fi, t_ref, t, err)
            checked += 1
        cos = float(d.astype(np.float64) @ Gm.n[f])
        rr = n_idx if cos > 0 else float(np.float32(1.0) / np.float32(n_idx))
        dd = (1 - rr * rr) / (cos * cos) + rr * rr
        if dd > 0 and np.isfinite(np.float32(dd)):
            sq = np.sqrt(dd)
            R = (((rr - sq) / (rr + sq)) ** 2 + ((1 - rr * sq) / (1 + rr * sq)) ** 2) * 0.5
            got = Rf.ref_reflect_ratio(float(np.float32(dd)), float(np.float32(rr)))
            # (the argument is dd rounded once: half an ulp of dd moves sqrt by a quarter ulp, R by dR/dsq of that)
            assert abs(got - R) <= 16 * M.U * max(R, 1e-3) + 4 * M.U * dd / sq * 4 / (rr + sq), (k, got, R)
    assert checked > 1000
