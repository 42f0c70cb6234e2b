"""The device's lens projection, ray by ray, at its edges, on every kernel route.

project_exit, exit_may_land and the bounds test of land_exit (csrc/halo_trace.inl) decide which pixel an exit lands on, or whether it lands
at all.  Here every exit is a directed probe of tests/_lens_model.py: a host-injected ray on the unit prism with max_hits = 1 leaves only its
external reflection, so the exit direction is chosen — to the bit on the four faces with exact normals.  The float64 model says, per
direction, which pixels it must reach and whether fp32 code may decide otherwise (closer than the measured margin DELTA to a decision:
left out).  The host side of that bargain — the model against the reference's own fp32 code, the margins, how little they leave out — is
tests/test_lens_model.py; this file holds the device to the same model with no fractional bar anywhere:

  capture     capture_exits = 1 (MODE 2, generic lens from the dispatch record): every record's pixel, against the model on the record's own dir
  direct      production kernels, hit_log = 0: the read-back image per pixel against the float64 scatter-add of the captured weights at the
              model's pixels (second hits of the dual lenses included), empty pixels exactly 0, landed weight
  hit log     the same with hit_log = 1: for linear, fisheye equal area, dual fisheye equal area and rectangular under VISIBLE_UPPER / FULL these
              are the compile-time lens instantiations reading the projection from LDS (spec_mask), for the others the generic one
"""
import ctypes as C

import numpy as np
import pytest

from ice_halo_sim_amd import abi, scenes
from tests import _lens_model as M
from tests._oracle_backend import OracleBackend

pytestmark = pytest.mark.gpu

RENDERS = M.renders()
IDS = [r[0] for r in RENDERS]
WL = 550.0


def hip_backend(**kw):
    from ice_halo_sim_amd.backend import HipTraceBackend
    return HipTraceBackend(device=0, **kw)


def _scene():
    return scenes.scene([(0.0, [scenes.entry(scenes.prism_crystal(1.0), scenes.axis())])], max_hits=1)


def _run(b, rd, rays):
    n = len(rays[2])
    b.BeginSession(_scene(), rd, scenes.wl_discrete(WL), n)
    st = b.TraceLayer(host_rays=rays[:4])
    b.EndSession()
    return st


def _cmf():
    from ice_halo_sim_amd.backend import load_library
    wl = scenes.wl_discrete(WL)
    buf = np.zeros((1, 5), np.float32)
    assert load_library().halo_host_wl_pool(C.byref(wl), buf.ctypes.data_as(C.POINTER(C.c_float)), 1) == 1
    return buf[0, 2:5].astype(np.float64)    # {n, spd weight, cmf x, y, z}


def _records(b, n):
    ex = b.DrainExits()
    ex = ex[np.argsort(ex["root"], kind="stable")]
    assert len(ex) == n and (ex["root"] == np.arange(n)).all(), (len(ex), n)      # one exit per injected ray:
    assert (ex["seq"] == 0).all() and (ex["path_len"] == 1).all()                   # ... its external reflection
    return ex


_cache = {}


def _capture(i):
    """Route a of render i, once: (P, probes, rays, records, model on the records' own directions, decidable, image, landed)."""
    if i in _cache:
        return _cache[i]
    rd = RENDERS[i][1]
    P = M.proj_of(rd)
    pr = M.probes(rd)
    rays = M.entry_rays(pr["dir"])
    hb = hip_backend(seed=1, capture_exits=1)
    _run(hb, rd, rays)
    route = hb.last_route()
    ex = _records(hb, len(pr))
    img, landed = hb.ReadbackXyzAccum()
    hb.close()
    assert route.mode_mask == abi.MODE_CAPTURE and route.source_mask == 1 << 2, (route.mode_mask, route.source_mask)
    H = M.project(P, ex["dir"].astype(np.float64))
    _cache[i] = dict(P=P, pr=pr, rays=rays, ex=ex, H=H, ok=H.decidable(), img=img, landed=landed)
    return _cache[i]


def _expected_image(c):
    """(float64 sum per pixel, addends per pixel, pixels an undecidable probe may touch) from the captured weights at the model's pixels."""
    P, H, ok, w = c["P"], c["H"], c["ok"], c["ex"]["weight"].astype(np.float64)
    npix = P.w * P.h
    acc, cnt, unsure = np.zeros(npix), np.zeros(npix, np.int64), np.zeros((P.h, P.w), bool)
    A = M.project(P, c["ex"]["dir"].astype(np.float64), cull=False)      # where a hit would land if a cull went the other way
    for hit in (0, 1):
        sel = ok & H.inframe[:, hit]
        pix = H.pix[sel, hit, 1] * P.w + H.pix[sel, hit, 0]
        np.add.at(acc, pix, w[sel])
        np.add.at(cnt, pix, 1)
        for k in np.flatnonzero(~ok & A.near[:, hit]):         # an undecidable probe lands within half a pixel of where the model puts it (the
            fx, fy = A.f[k, hit]                                # widest margin there is, next to an acos pole), or not at all: at most four pixels
            for x in {int(np.floor(fx - 0.5)), int(np.floor(fx + 0.5))}:
                for y in {int(np.floor(fy - 0.5)), int(np.floor(fy + 0.5))}:
                    x = x % P.w if P.t == abi.LENS_RECTANGULAR else x
                    if 0 <= x < P.w and 0 <= y < P.h:
                        unsure[y, x] = True
    # what is left out stays small: at least two thirds of the image is compared on every render
    assert unsure.mean() <= 1.0 / 3.0, unsure.mean()
    return acc.reshape(P.h, P.w), cnt.reshape(P.h, P.w), unsure


def _landed_bounds(c):
    """Landed weight of a production route: the in-frame primaries.  Only a probe whose LANDING is in doubt widens the bound: one within a
    margin of a cull that decides its primary hit (wz, cz), or whose primary hit is within half a pixel of a frame edge; every other
    undecidable probe (a pixel edge inside the frame, a pole, the overlap band) lands or not as the model says."""
    P, H, ok = c["P"], c["H"], c["ok"]
    w = c["ex"]["weight"].astype(np.float64)
    A = M.project(P, c["ex"]["dir"].astype(np.float64), cull=False)
    fx, fy = A.f[:, 0, 0], A.f[:, 0, 1]
    at_frame = (np.minimum(np.abs(fy), np.abs(fy - P.h)) < 0.5) | ((P.t != abi.LENS_RECTANGULAR) & (np.minimum(np.abs(fx), np.abs(fx - P.w)) < 0.5))
    at_cull = (H.dist["cz"] < M.DELTA["cz"]) | ((H.dist["wz"] < M.DELTA["wz"]) & (P.t in M.SINGLE))
    doubt = ~ok & (at_cull | at_frame)
    sure = w[~doubt & H.inframe[:, 0]].sum()
    return sure, sure + w[doubt].sum()


@pytest.mark.parametrize("i", range(len(RENDERS)), ids=IDS)
def test_capture_route_records_the_models_pixel_for_every_decidable_probe(i):
    c = _capture(i)
    P, pr, ex, H, ok = c["P"], c["pr"], c["ex"], c["H"], c["ok"]
    exact = c["rays"][4]
    assert (ex["dir"][exact] == pr["dir"][exact]).all()       # exact normals: the wanted direction to the bit (but for the sign of a zero, which d - 2 (d.n) n does not keep)
    assert np.abs(ex["dir"].astype(np.float64) - pr["dir"]).max() < 1e-6
    assert ok[pr["must"]].all(), int((~ok[pr["must"]]).sum())      # no probe built k >= 1 margins from its boundary drops out on the device either
    print("%s: %d probes, %d decidable, %d land" % (IDS[i], len(pr), int(ok.sum()), int((ex["pixel"] >= 0).sum())))
    want = H.primary_pixel(P.w)
    bad = np.flatnonzero(ok & (ex["pixel"] != want))
    assert len(bad) == 0, [(M.CLASSES[pr["cls"][k]], ex["dir"][k].tolist(), int(ex["pixel"][k]), int(want[k]), {q: float(H.dist[q][k]) for q in M.KINDS}) for k in bad[:8]]
    # landed weight: the in-frame primaries (an undecidable probe counts as the device itself recorded it)
    w = ex["weight"].astype(np.float64)
    landed = w[ok & H.inframe[:, 0]].sum() + w[~ok & (ex["pixel"] >= 0)].sum()
    assert c["landed"] == pytest.approx(landed, rel=1e-6, abs=1e-12)
    # the capture session's own image: the same per-pixel check as the production routes
    _check_image(c, c["img"], c["landed"])
    # the oracle on the same rays: same records, same verdict — what ties this file to tests/test_lens_model.py
    ob = OracleBackend(seed=1, capture_exits=1)
    _run(ob, RENDERS[i][1], c["rays"])
    eo = _records(ob, len(pr))
    ob.close()
    Ho = M.project(P, eo["dir"].astype(np.float64))
    oko = Ho.decidable()
    assert (eo["pixel"][oko] == Ho.primary_pixel(P.w)[oko]).all()
    same = (eo["dir"].view(np.uint32) == ex["dir"].view(np.uint32)).all(axis=1)
    assert (eo["dir"][exact] == ex["dir"][exact]).all() and (eo["pixel"][same & ok] == ex["pixel"][same & ok]).all()


def _check_image(c, img, landed):
    P = c["P"]
    acc, cnt, unsure = _expected_image(c)
    exp = acc[:, :, None] * _cmf()[None, None, :]
    tol = (2e-4 + cnt * 2.0 ** -24)[:, :, None] * np.abs(exp)
    err = np.abs(img.astype(np.float64) - exp)
    bad = (err > tol) & ~unsure[:, :, None]
    assert not bad.any(), [(int(y), int(x), img[y, x].tolist(), exp[y, x].tolist(), int(cnt[y, x])) for y, x in np.argwhere(bad.any(axis=2))[:8]]
    empty = (cnt == 0) & ~unsure
    assert not img[empty].any(), [(int(y), int(x), img[y, x].tolist()) for y, x in np.argwhere(empty & img.any(axis=2))[:8]]
    lo, hi = _landed_bounds(c)
    assert lo * (1 - 1e-6) - 1e-12 <= landed <= hi * (1 + 1e-6) + 1e-12, (lo, landed, hi)


def _production(i, hit_log):
    c = _capture(i)
    hb = hip_backend(seed=1, hit_log=hit_log)
    st = _run(hb, RENDERS[i][1], c["rays"])
    route = hb.last_route()
    img, landed = hb.ReadbackXyzAccum()
    hb.close()
    assert st.root_count == len(c["pr"]) == st.exit_count
    assert route.mode_mask == abi.MODE_PLAIN and route.source_mask == 1 << 2, (route.mode_mask, route.source_mask)
    return c, route, img, landed


@pytest.mark.parametrize("i", range(len(RENDERS)), ids=IDS)
def test_direct_route_image_equals_the_models_scatter_add(i):
    c, route, img, landed = _production(i, 0)
    assert route.accum_mask in (abi.ACCUM_XYZ, abi.ACCUM_SCALAR), route.accum_mask
    _check_image(c, img, landed)


@pytest.mark.parametrize("i", range(len(RENDERS)), ids=IDS)
def test_hit_log_route_image_equals_the_models_scatter_add(i):
    c, route, img, landed = _production(i, 1)
    P = c["P"]
    if route.accum_mask != abi.ACCUM_LOG:
        # the log's tile layout has limits (plan_route): the backend says which route it took
        assert (P.w, P.h) != (512, 256), "the hit log must serve a 512 x 256 session"
        pytest.skip("halo_last_route: accum_mask %d, the hit log does not serve %d x %d" % (route.accum_mask, P.w, P.h))
    both = abi.SPEC_LENS | abi.SPEC_VIS
    if P.t in M.SPECIALISED and P.vr in (abi.VISIBLE_UPPER, abi.VISIBLE_FULL):
        assert route.spec_mask & both == both and route.spec_mask & abi.SPEC_LAST and route.generic_launches == 0, (route.spec_mask, route.generic_launches)
    else:
        assert route.spec_mask & both == 0, route.spec_mask        # the generic-lens instantiation
    _check_image(c, img, landed)


def test_every_specialised_lens_has_a_512_render_for_the_hit_log_route():
    """... on which test_hit_log_route_image_equals_the_models_scatter_add may not skip."""
    for lens in M.SPECIALISED:
        assert any(rd.lens_type == lens and (rd.width, rd.height) == (512, 256) and rd.visible in (abi.VISIBLE_UPPER, abi.VISIBLE_FULL) for _, rd in RENDERS), lens
