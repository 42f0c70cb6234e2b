"""The device's interaction loop (trace_one, csrc/halo_trace.inl), ray by ray, at its edges, on every kernel route — with no fractional bar.

Every ray is a directed probe of tests/_hit_model.py: host-injected on an injected crystal, aimed at a decision of the loop (a grazing entry,
a critical angle, an edge or a vertex of the next face, a face the ray skims with n.d either side of 1e-5, an entry point off its plane, a bad
entry face, zero weight, hit budgets of 1, 2 and 8, paths either side of the 16 faces of the path register).  The float64 model says what
each ray must emit and whether fp32 code may decide otherwise (closer than the measured margin DELTA to a decision: left out).  The host side
of that bargain — the model against both builds of the oracle, the margins, the bar constants, how little they leave out — is
tests/test_hit_model.py; this file holds the device to the same model:

  capture     capture_exits = 1 (the table-driven search over slabs and singles): for every decidable probe the model's exit set, seq,
              path_len and path bytes exactly, every exit's direction and weight within the model's bar; both next-face strategies
  production  the read-back image per pixel against the float64 scatter-add of the MODEL's weights at the pixels the capture records carry:
              the literal search of the regular prism (direct and hit-log kernels), the table search inside a production kernel
              (hex_fast = 0, the irregular prism, the pyramid), and the fast filter with the regular prism's path numbering
  pool        the same image check on the sampled-prism pool kernels (geom_mask bit 2; under the hit log the SlotFast::hexn search), after
              showing that the device-generated records are the host builder's bit for bit
"""
import numpy as np
import pytest

from ice_halo_sim_amd import abi, scenes
from tests import _hit_model as M
from tests import _lens_model as LM

pytestmark = pytest.mark.gpu

CRYSTALS = dict(M.crystals())
NAMES = list(CRYSTALS)
HOST = 1 << 2                 # HaloRouteInfo.source_mask: host-injected rays
GEOM_ONE, GEOM_PRISM_POOL, GEOM_HEX = 1 << 0, 1 << 2, 1 << 3


def hip_backend(**kw):
    from ice_halo_sim_amd.backend import HipTraceBackend
    return HipTraceBackend(device=0, **kw)


_cache = {}


def _probes(name):
    if ("p", name) not in _cache:
        g = M.geometry_of(CRYSTALS[name])               # the product's host builder: the tables the device gets
        _cache["p", name] = (g, M.probes(g, M.refractive_index(), M.TEST_SEED, M.TEST_PER_CLASS, plate_tir=(name == "plate")))
    return _cache["p", name]


def _capture(name, mh, strategy=1):
    """The capture route on crystal `name`, once: model, records, comparison, stats, route, landed weight."""
    key = ("c", name, mh, strategy)
    if key in _cache:
        return _cache[key]
    g, pr = _probes(name)
    if strategy == 0:      # the classes rehit_strategy 0 is held on, narrowed to the probes whose own outgoing-child decision is clear (M.probes(): scope0)
        pr = {k: v[pr["scope0"]] for k, v in pr.items()}
        pr["must"] = pr["must0"]
    R = M.trace(g, M.refractive_index(), pr["d"], pr["p"], pr["w"], pr["face"], mh, strategy)
    hb = hip_backend(seed=1, capture_exits=1, rehit_strategy=strategy)
    st = M.session(hb, CRYSTALS[name], g, pr, mh)
    route = hb.last_route()
    rec = hb.DrainExits()
    img, landed = hb.ReadbackXyzAccum()
    hb.close()
    _cache[key] = dict(g=g, pr=pr, R=R, st=st, route=route, rec=rec, cmp=M.compare(R, rec), img=img, landed=landed)
    return _cache[key]


def _describe(R, pr, k):
    return (int(k), M.CLASSES[pr["cls"][k]], {q: float("%.3g" % R.dist[q][k]) for q in M.KINDS})


def _hold_to_model(c):
    """Every decidable probe: the model's record set exactly; every exit of one: direction and weight within the model's bar."""
    R, pr, cm = c["R"], c["pr"], c["cmp"]
    ok = R.decidable()
    E = R.exits
    bad = np.flatnonzero(cm["bad_root"] & ok)
    assert len(bad) == 0, [(_describe(R, pr, k), [(int(s), int(l)) for s, l in zip(E.seq[E.root == k], E.path_len[E.root == k])],
                            [(int(r["seq"]), int(r["path_len"])) for r in cm["rec"][cm["rec"]["root"] == k]]) for k in bad[:6]]
    bd, bw = M.bars(E)
    sel = ok[E.root[cm["im"]]]
    im = cm["im"][sel]
    print("%d probes, %d decidable, %d exits compared; worst direction error %.3g of its bar, weight %.3g" % (
        R.n, int(ok.sum()), len(im), float((cm["err_dir"][sel] / bd[im]).max()), float(np.where(cm["err_w"][sel] > 0, cm["err_w"][sel] / np.maximum(bw[im], 1e-300), 0).max())))
    over = np.flatnonzero((cm["err_dir"][sel] > bd[im]) | (cm["err_w"][sel] > bw[im]))
    assert len(over) == 0, [(_describe(R, pr, E.root[im[j]]), int(E.seq[im[j]]), float(cm["err_dir"][sel][j]), float(bd[im[j]]), float(cm["err_w"][sel][j]), float(bw[im[j]]))
                            for j in over[:6]]
    return ok


CAPTURE = [(name, mh) for name in NAMES for mh in M.budgets(name)]


@pytest.mark.parametrize("name,mh", CAPTURE, ids=["%s-%d" % c for c in CAPTURE])
def test_capture_route_has_the_models_exits_for_every_decidable_probe(name, mh):
    c = _capture(name, mh)
    R, pr, rec, route, st = c["R"], c["pr"], c["rec"], c["route"], c["st"]
    assert route.mode_mask == abi.MODE_CAPTURE and route.geom_mask == GEOM_ONE and route.source_mask == HOST, (route.mode_mask, route.geom_mask, route.source_mask)
    ok = _hold_to_model(c)
    lost = np.flatnonzero(pr["must"] & ~ok)
    assert len(lost) == 0 and (~ok).mean() <= 1.0 / 3.0, ([_describe(R, pr, k) for k in lost[:6]], (~ok).mean())
    # an entry face outside the body's gives no record; every other probe at least its first one
    per_root = np.bincount(rec["root"].astype(np.int64), minlength=R.n)
    invalid = pr["cls"] == M.CLASSES.index("badface")
    assert (per_root[invalid] == 0).all() and (per_root[~invalid & ok] > 0).all()
    assert (rec["layer"] == 0).all() and (rec["wl_idx"] == 0).all()
    # the layer's tallies are the records'
    assert st.root_count == R.n and st.exit_count == len(rec)
    w = rec["weight"].astype(np.float64)
    assert st.exit_w_sum == pytest.approx(w.sum(), rel=1e-5)
    assert c["landed"] == pytest.approx(w[rec["pixel"] >= 0].sum(), rel=1e-6, abs=1e-12)


@pytest.mark.parametrize("name", NAMES)
def test_capture_route_parks_the_child_that_re_hits_under_the_first_strategy(name):
    """rehit_strategy = 0 on the whole batch (its off-plane class is where the strategies part): the same model, told the strategy."""
    c0, c1 = _capture(name, 8, 0), _capture(name, 8, 1)
    assert c0["route"].mode_mask == abi.MODE_CAPTURE and c0["route"].geom_mask == GEOM_ONE
    ok0 = _hold_to_model(c0)
    pr0, pr1 = c0["pr"], c1["pr"]
    # what may be left out under this strategy too: at most a third of its batch, no `must` probe
    lost = np.flatnonzero(pr0["must"] & ~ok0)
    assert len(lost) == 0 and (~ok0).mean() <= 1.0 / 3.0 and pr0["must"].sum() >= 150, ([_describe(c0["R"], pr0, k) for k in lost[:6]], (~ok0).mean())
    # decidable off-plane probes on which the device's records differ between the strategies, as the model's do
    where = np.flatnonzero(pr1["scope0"])                        # root of the scoped batch -> root of the whole one
    ok1 = c1["R"].decidable()
    differ = 0
    for k0 in np.flatnonzero((pr0["cls"] == M.CLASSES.index("offplane")) & ok0):
        k1 = where[k0]
        if not ok1[k1]:
            continue
        r0, r1 = c0["rec"][c0["rec"]["root"] == k0], c1["rec"][c1["rec"]["root"] == k1]
        dev = sorted(zip(r0["seq"].tolist(), r0["path_len"].tolist())) != sorted(zip(r1["seq"].tolist(), r1["path_len"].tolist()))
        mod = sorted((c0["R"].exits.key()[c0["R"].exits.root == k0] & 0xFFFFFF).tolist()) != sorted((c1["R"].exits.key()[c1["R"].exits.root == k1] & 0xFFFFFF).tolist())
        assert dev == mod, (int(k0), int(k1))
        differ += dev
    assert differ >= 4, differ


# ---------------------------------------------------------------------------------------------------------------------------------
# production routes: the image
# ---------------------------------------------------------------------------------------------------------------------------------
def _cmf():
    import ctypes as C
    from ice_halo_sim_amd.backend import load_library
    wl = scenes.wl_discrete(M.WL)
    buf = np.zeros((1, 5), np.float32)
    assert load_library().halo_host_wl_pool(C.byref(wl), buf.ctypes.data_as(C.POINTER(C.c_float)), 1) == 1
    return buf[0, 2:5].astype(np.float64)


def _expected(name, keep=None):
    """(rays, sum per pixel, bar per pixel, addends per pixel, unsure pixels, landed bounds) of the production batch of crystal `name`: the
    capture batch with the weight of every undecidable probe set to zero — it is traced, and whatever it decides adds exactly nothing — and
    the float64 scatter-add of the MODEL's weights of the others at the pixels their capture records carry.  `keep`: a mask over the model's
    exits (the filter case).  An exit whose pixel the projection's own margins (tests/_lens_model.py) leave open, widened by what the exit's
    direction bar can move it, makes the four pixels around it unsure."""
    c = _capture(name, 8)
    R, cm, pr = c["R"], c["cmp"], c["pr"]
    ok = _hold_to_model(c)
    E = R.exits
    P = LM.proj_of(M.full_sky())
    sel = ok[E.root[cm["im"]]]
    im, ir = cm["im"][sel], cm["ir"][sel]
    assert len(im) == int(ok[E.root].sum())                  # every exit of a decidable probe has its record
    if keep is not None:
        k = keep[im]
        im, ir = im[k], ir[k]
    rec = cm["rec"][ir]
    bd, bw = M.bars(E)
    d = rec["dir"].astype(np.float64)
    H = LM.project(P, d)
    assert (H.primary_pixel(P.w)[H.decidable()] == rec["pixel"][H.decidable()]).all()
    px_per_unit = P.w / (2.0 * np.pi) / np.maximum(np.sqrt(np.maximum(1.0 - d[:, 2] ** 2, 0.0)), 1e-3) + P.h / np.pi / np.maximum(np.sqrt(np.maximum(1.0 - d[:, 2] ** 2, 0.0)), 1e-3)
    open_px = ~H.decidable() | (H.dist["px"] <= LM.DELTA["px"] + 2.0 * bd[im] * px_per_unit)
    npix = P.w * P.h
    acc, bar, cnt, unsure = np.zeros(npix), np.zeros(npix), np.zeros(npix, np.int64), np.zeros((P.h, P.w), bool)
    sure = ~open_px & (rec["pixel"] >= 0)                   # (the full sky takes every exit but one straight down: the projection's matter, pinned elsewhere)
    np.add.at(acc, rec["pixel"][sure], E.weight[im][sure])
    np.add.at(bar, rec["pixel"][sure], bw[im][sure])
    np.add.at(cnt, rec["pixel"][sure], 1)
    for j in np.flatnonzero(open_px):
        fx, fy = H.f[j, 0]
        for x in {int(np.floor(fx - 0.5)), int(np.floor(fx + 0.5))}:
            for y in {int(np.floor(fy - 0.5)), int(np.floor(fy + 0.5))}:
                if 0 <= y < P.h:
                    unsure[y, x % P.w] = True
    assert unsure.mean() <= 1.0 / 3.0, unsure.mean()          # at least two thirds of the image is compared (in fact nearly all of it)
    rays = dict(pr)
    rays["w"] = np.where(ok, pr["w"], np.float32(0.0)).astype(np.float32)
    lands = (rec["pixel"] >= 0) | open_px
    total, slack = E.weight[im][sure].sum(), bw[im][lands].sum() + E.weight[im][open_px].sum()
    return rays, acc.reshape(P.h, P.w), bar.reshape(P.h, P.w), cnt.reshape(P.h, P.w), unsure, (total - slack, total + slack)


FIX_HALF_QUANTUM = 2.0 ** -33   # the hit log's per-tile pass sums weight x 2^F rounded to nearest, F = 32 for unit-weight launches under 2^28 rays (csrc/halo_kernels.hip)


def _check_image(exp, img, landed, fixed_point=False):
    """Per pixel: the model's sum within the sum of its addends' weight bars, the fp32 roundings of the adds and of the colour-matching
    products, and — where the route sums in fixed point — half a quantum per addend."""
    rays, acc, bar, cnt, unsure, (lo, hi) = exp
    cmf = _cmf()[None, None, :]
    want = acc[:, :, None] * cmf
    tol = (bar + (cnt + 8) * 2.0 ** -23 * acc + (cnt * FIX_HALF_QUANTUM if fixed_point else 0.0))[:, :, None] * cmf
    err = np.abs(img.astype(np.float64) - want)
    bad = (err > tol) & ~unsure[:, :, None]
    assert not bad.any(), [(int(y), int(x), img[y, x].tolist(), want[y, x].tolist(), tol[y, x].tolist(), int(cnt[y, x])) for y, x in np.argwhere(bad.any(axis=2))[:8]]
    empty = (cnt == 0) & ~unsure
    assert not img[empty].any(), [(int(y), int(x), img[y, x].tolist()) for y, x in np.argwhere(empty & img.any(axis=2))[:8]]
    assert lo * (1 - 1e-6) - 1e-12 <= landed <= hi * (1 + 1e-6) + 1e-12, (lo, landed, hi)
    print("%d of %d pixels compared, %d of them lit" % (int((~unsure).sum()), unsure.size, int(((cnt > 0) & ~unsure).sum())))


def _production(name, exp, filters=None, filter_id=0, crystal=None, **opts):
    """`crystal`: the scene's own crystal takes the rays (nothing injected); default: the crystal's tables injected with the rays."""
    g = None if crystal is not None else _probes(name)[0]
    hb = hip_backend(seed=1, **opts)
    if filters:
        hb.set_filters(filters)
    rays = exp[0]
    sc = scenes.scene([(0.0, [scenes.entry(crystal if crystal is not None else CRYSTALS[name], scenes.axis(), filter_id=filter_id)])], max_hits=8)
    hb.BeginSession(sc, M.full_sky(), scenes.wl_discrete(M.WL), len(rays["w"]))
    st = hb.TraceLayer(host_rays=(rays["d"], rays["p"], rays["w"], rays["face"]) + ((g,) if g is not None else ()))
    hb.EndSession()
    route = hb.last_route()
    img, landed = hb.ReadbackXyzAccum()
    hb.close()
    assert st.root_count == len(rays["w"]) and route.source_mask == HOST, (st.root_count, route.source_mask)
    return route, img, landed


ROUTES = [("regular", dict(hit_log=0), GEOM_HEX),            # the literal search of the regular prism
          ("regular", dict(hit_log=1), GEOM_HEX),            # ... in the lens-constant last-layer kernel of the hit log
          ("regular", dict(hit_log=0, hex_fast=0), GEOM_ONE),     # the table search inside a production kernel
          ("irregular", dict(hit_log=0), GEOM_ONE),
          ("pyramid", dict(hit_log=0), GEOM_ONE),
          ("plate", dict(hit_log=0), GEOM_HEX),              # a regular prism whose basal and prism faces have different plane constants
          ("column", dict(hit_log=1), GEOM_HEX)]


@pytest.mark.parametrize("name,opts,geom", ROUTES, ids=["%s-%s" % (r[0], "-".join("%s%d" % kv for kv in r[1].items())) for r in ROUTES])
def test_production_route_image_equals_the_models_scatter_add(name, opts, geom):
    exp = _expected(name)
    route, img, landed = _production(name, exp, **opts)
    assert route.mode_mask == abi.MODE_PLAIN and route.geom_mask == geom, (route.mode_mask, route.geom_mask)
    if opts["hit_log"]:
        both = abi.SPEC_LENS | abi.SPEC_VIS
        assert route.accum_mask == abi.ACCUM_LOG, route.accum_mask             # 512 x 256: the hit log serves it (tests/test_gpu_lens_edges.py)
        assert route.spec_mask & both == both and route.spec_mask & abi.SPEC_LAST and route.generic_launches == 0, (route.spec_mask, route.generic_launches)
    else:
        assert route.accum_mask in (abi.ACCUM_XYZ, abi.ACCUM_SCALAR), route.accum_mask
    _check_image(exp, img, landed, fixed_point=bool(opts["hit_log"]))


def test_fast_filter_on_the_regular_prism_keeps_exactly_the_models_exits_of_one_path():
    """A raypath filter without symmetry for the two-face path 3-5 on the regular prism (the fast filter, mode_mask bit 1, on the literal search:
    its path register numbers a face `face + 1`): the image is the model's exits with exactly that path, nothing else."""
    c = _capture("regular", 8)
    E = c["R"].exits
    path = (3, 5)
    keep = (E.path_len == 2) & (E.path[:, 0] == path[0]) & (E.path[:, 1] == path[1])
    assert keep.sum() >= 20, int(keep.sum())
    exp = _expected("regular", keep)
    flt = [scenes.simple_filter(scenes.filter_term("raypath", raypath=list(path)), "")]
    route, img, landed = _production("regular", exp, filters=flt, filter_id=1, hit_log=0)
    assert route.mode_mask == abi.MODE_FILTER and route.geom_mask == GEOM_HEX, (route.mode_mask, route.geom_mask)
    _check_image(exp, img, landed)


@pytest.mark.parametrize("hit_log", [0, 1])
@pytest.mark.parametrize("name", ["regular", "irregular"])
def test_sampled_prism_pool_search_image_equals_the_models_scatter_add(name, hit_log):
    """The pool kernels' literal search with a plane constant per face (SlotFast::hexn, geom_mask bit 2).  A crystal whose six face distances
    carry a distribution of zero width is not deterministic for the backend, so its dispatch samples a pool on the device — of records that
    are, every one, the host builder's tables bit for bit (shown first) — and the host rays of the batch run on that route.  The irregular
    prism has the regular one's normals and a different plane constant on every face: the two faces of a slab must not be confused.
    (The pool kernels of the hit log are the ones that build SlotFast per half-wave; the direct ones run the table search on pool records.)"""
    import copy
    cr = copy.deepcopy(CRYSTALS[name])
    for i in range(6):
        cr.face_dist[i].type, cr.face_dist[i].spread = abi.DIST_UNIFORM, 0.0
    g, _ = _probes(name)
    hb = hip_backend(seed=1)
    recs = hb.generate_shapes(cr, 0, 8, on_device=2)
    hb.close()
    for k in range(8):
        assert bytes(recs[k]) == bytes(g), k
    exp = _expected(name)
    route, img, landed = _production(name, exp, crystal=cr, hit_log=hit_log)
    assert route.mode_mask == abi.MODE_PLAIN and route.geom_mask == GEOM_PRISM_POOL, (route.mode_mask, route.geom_mask)
    assert (route.accum_mask == abi.ACCUM_LOG) == bool(hit_log), route.accum_mask
    _check_image(exp, img, landed, fixed_point=bool(hit_log))
