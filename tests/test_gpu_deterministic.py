"""Deterministic sessions (option deterministic = 1): pixel sums and the landed weight are 64-bit fixed-point integers from the first add to the
fold, so they depend on the SET of rays alone.  Every comparison below is integer or byte equality — no tolerance anywhere.  Every run uses one
seed, one ray_base and a fresh handle; what varies is how the same rays are cut into launches, workgroups, streams and sessions.

halo_peek_fixed hands out the pending planes as integers (before the fold), ReadbackXyzAccum the folded image."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

from ice_halo_sim_amd import abi, scenes
from tests import _fixed_model as fm
from tests._oracle_backend import run_session

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED, RAY_BASE, WL = 11, 3 << 20, 550.0
FULL = {"type": "uniform", "mean": 0.0, "std": 360.0}


def hip_backend(**kw):
    from ice_halo_sim_amd.backend import HipTraceBackend
    return HipTraceBackend(device=0, **kw)


def _prism(filter_id=0):
    return scenes.entry(scenes.prism_crystal(1.0), scenes.axis(zenith=FULL, azimuth=FULL, roll=FULL), 1.0, 1, filter_id=filter_id)


def _base_scene():
    """A regular prism in random orientation, max_hits 7, sun at 20 degrees: a third of the exits are rays that crossed two parallel faces and
    land on the few pixels of the sun's disc."""
    return scenes.scene([(0.0, [_prism()])], max_hits=7, sun_altitude=20.0)


def _fisheye(w, h):
    return scenes.render(abi.LENS_FISHEYE_EQUAL_AREA, w, h, fov=180.0, el=30.0, visible=abi.VISIBLE_UPPER)


def _run(scene, render, n, wl=None, parts=1, filters=(), det=1, **opts):
    """Trace `n` roots as `parts` sessions on a fresh handle.  Returns the peeked integers (det = 1) or the captured exits (capture_exits = 1),
    the image bytes and what the route says."""
    wl = wl or scenes.wl_discrete(WL)
    hb = hip_backend(seed=SEED, **opts)
    hb.set_option("deterministic", det)
    hb.set_option("ray_base", RAY_BASE)
    hb.set_filters(list(filters))
    cuts = [n // parts] * (parts - 1) + [n - (parts - 1) * (n // parts)]
    stats, mask, modes, geoms = [], 0, 0, 0
    for m in cuts:
        stats += [(int(s.root_count), int(s.continuation_count)) for s in run_session(hb, scene, render, wl, m)]
        r = hb.last_route()
        mask, modes, geoms = mask | r.accum_mask, modes | r.mode_mask, geoms | r.geom_mask
    out = dict(stats=stats, mask=mask, modes=modes, geoms=geoms, planes=hb.last_route().plane_cnt)
    if det:
        hb.sync()
        peeks = [hb.peek_fixed(p) for p in range(out["planes"])]
        out.update(sums=[p[0] for p in peeks], F=peeks[0][1], landed_q=int(peeks[0][2]), FL=peeks[0][3])
    if opts.get("capture_exits"):
        out["ex"] = hb.DrainExits()
    img, landed = hb.ReadbackXyzAccum()
    out.update(img=img.tobytes(), landed=landed, sha=hashlib.sha256(img.tobytes()).hexdigest())
    hb.close()
    return out


def _same(a, b, what):
    assert a["F"] == b["F"] and a["FL"] == b["FL"], what
    for p, (x, y) in enumerate(zip(a["sums"], b["sums"])):
        bad = np.flatnonzero(x.ravel() != y.ravel())
        assert bad.size == 0, "%s: plane %d differs in %d pixels, first %d: %d vs %d" % (what, p, bad.size, bad[0], x.ravel()[bad[0]], y.ravel()[bad[0]])
    assert a["landed_q"] == b["landed_q"], what
    assert a["img"] == b["img"], what
    assert a["landed"] == b["landed"], what


PLANS = [("chunk", dict(chunk=1 << 18)), ("blocks_per_cu", dict(blocks_per_cu=1)), ("overlap", dict(overlap=0)), ("aggregate", dict(aggregate=0)),
         ("mono_copies", dict(mono_copies=1)), ("async", {"async": 1}), ("four sessions", dict(parts=4))]


# ---- 1. the plan does not matter ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,n", [(256, 128, (1 << 20) + 37), (17, 13, (1 << 20) + 37), (1920, 1080, 1 << 18)])
def test_plane_sums_landed_integer_and_image_do_not_depend_on_the_plan(w, h, n):
    """256 x 128: 32 Ki pixels against 1024 cache slots, so most hits miss the cache and the sun's pixels are hot; 17 x 13: every pixel lives in
    the cache; 1920 x 1080: a plane of 2 Mi slots, few hits per pixel."""
    sc, rd = _base_scene(), _fisheye(w, h)
    ref = _run(sc, rd, n)
    assert ref["mask"] == abi.ACCUM_FIXED and ref["planes"] == 1 and ref["modes"] == abi.MODE_PLAIN and ref["geoms"] == 1 << 3
    total = int(ref["sums"][0].sum(dtype=np.uint64))
    assert ref["landed_q"] > 0 and total > 0
    assert int(ref["sums"][0].max()) > 50 * (total // (w * h) + 1) or w * h < 1024, "the sun's disc is in the frame: its pixels are hot"
    assert ref["F"] == 29 and ref["FL"] == 27      # unit weights: 2^30 rays per plane set, 2^32 for the landed integer
    for name, kw in PLANS:
        got = _run(sc, rd, n, **kw)
        assert got["mask"] == abi.ACCUM_FIXED, name
        _same(ref, got, name)


# ---- 2. every kernel family ---------------------------------------------------------------------------------------------------------------------
def _families():
    pyr = scenes.pyramid_crystal(0.3, 1.0, 0.2)
    pyr_s = scenes.pyramid_crystal({"type": "gauss", "mean": 0.3, "std": 0.05}, 1.0, {"type": "gauss", "mean": 0.2, "std": 0.05})
    ax = scenes.axis(zenith=FULL, azimuth=FULL, roll=FULL)
    one = lambda e, hits=7: scenes.scene([(0.0, [e])], max_hits=hits, sun_altitude=20.0)
    rd = _fisheye(256, 128)
    flt = [scenes.simple_filter(scenes.filter_term("raypath", raypath=[3, 5]), "PBD")]
    dual = scenes.render(abi.LENS_DUAL_FISHEYE_EQUAL_AREA, 256, 128, visible=abi.VISIBLE_FULL, overlap=0.0872)
    d65 = scenes.wl_illuminant("D65", 31)
    return {
        "fixed pyramid": dict(scene=one(scenes.entry(pyr, ax, 1.0, 2)), render=rd, geoms=1 << 0, planes=1),
        "sampled prisms": dict(scene=one(scenes.stochastic_prism_entry(), 8), render=rd, geoms=1 << 2, planes=1),
        "sampled pyramids": dict(scene=one(scenes.entry(pyr_s, ax, 1.0, 4)), render=rd, geoms=1 << 1, planes=1),
        "D65 regular prism": dict(scene=_base_scene(), render=rd, wl=d65, geoms=1 << 3, planes=3),
        "D65 sampled prisms": dict(scene=one(scenes.stochastic_prism_entry(), 8), render=rd, wl=d65, geoms=1 << 2, planes=3),
        "raypath filter": dict(scene=one(_prism(filter_id=1)), render=rd, filters=flt, geoms=1 << 3, planes=1, modes=abi.MODE_FILTER),
        "dual lens overlap": dict(scene=_base_scene(), render=dual, geoms=1 << 3, planes=1),
    }


@pytest.mark.parametrize("family", sorted(_families()))
def test_every_kernel_family_is_plan_invariant(family):
    f = _families()[family]
    kw = dict(wl=f.get("wl"), filters=f.get("filters", ()))
    n = 1 << 18
    a = _run(f["scene"], f["render"], n, **kw)
    b = _run(f["scene"], f["render"], n, chunk=1 << 16, blocks_per_cu=1, **kw)
    for r in (a, b):
        assert r["mask"] == abi.ACCUM_FIXED and r["geoms"] == f["geoms"] and r["planes"] == f["planes"] and r["modes"] == f.get("modes", abi.MODE_PLAIN), family
    assert all(int(s.sum(dtype=np.uint64)) > 0 for s in a["sums"]) and a["landed_q"] > 0
    _same(a, b, family)


# ---- 3. against the rays themselves -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("crystal", ["regular prism", "fixed pyramid"])
def test_plane_sums_are_the_quantised_weights_of_the_captured_rays(crystal):
    """Capture (option off) hands out every exit's weight and primary pixel; the deterministic run of the same seed must hold, pixel by pixel,
    exactly the sum of q(weight) over them — the capture kernels and the production kernels trace bit-identical rays."""
    c = scenes.prism_crystal(1.0) if crystal == "regular prism" else scenes.pyramid_crystal(0.3, 1.0, 0.2)
    sc = scenes.scene([(0.0, [scenes.entry(c, scenes.axis(zenith=FULL, azimuth=FULL, roll=FULL), 1.0, 1)])], max_hits=7, sun_altitude=20.0)
    rd = scenes.render(abi.LENS_LINEAR, 128, 64, fov=90.0, el=30.0, visible=abi.VISIBLE_UPPER)
    n = 1 << 16
    ex = _run(sc, rd, n, det=0, capture_exits=1)["ex"]
    assert (ex["pixel"] >= 0).sum() > 1000
    det = _run(sc, rd, n)
    want = fm.plane_sums(ex["pixel"], ex["weight"], 128 * 64, det["F"]).reshape(64, 128)
    bad = np.flatnonzero(want.ravel() != det["sums"][0].ravel())
    assert bad.size == 0, "%d pixels differ, first %d: captured %d, plane %d" % (bad.size, bad[0], want.ravel()[bad[0]], det["sums"][0].ravel()[bad[0]])
    assert det["landed_q"] == int(fm.q(ex["weight"][ex["pixel"] >= 0], det["FL"]).sum(dtype=np.uint64))


# ---- 4. multi-layer, with canonical continuation order ---------------------------------------------------------------------------------------------
def test_two_layers_are_plan_invariant_with_canonical_order():
    plate = scenes.entry(scenes.prism_crystal(0.3), scenes.axis(zenith={"type": "gauss", "mean": 0, "std": 0.8}), 1.0, 6)
    col = scenes.entry(scenes.prism_crystal(1.3, [1.0] * 6), scenes.axis(zenith={"type": "uniform", "mean": 90, "std": 360}, azimuth=FULL), 1.0, 3)
    sc = scenes.scene([(0.5, [plate]), (0.0, [col])], max_hits=7)
    rd, n = _fisheye(256, 128), 1 << 16
    a = _run(sc, rd, n, cont_order=1)
    b = _run(sc, rd, n, cont_order=1, chunk=1 << 14, blocks_per_cu=1)
    assert a["mask"] == abi.ACCUM_FIXED and b["mask"] == abi.ACCUM_FIXED
    assert a["stats"][0][1] > 0 and a["stats"] == b["stats"]          # per-layer roots and continuation counts
    _same(a, b, "two layers")


# ---- 5. what is refused, and the default ----------------------------------------------------------------------------------------------------------
def test_refusals_name_the_option_and_leave_the_backend_usable():
    from ice_halo_sim_amd.backend import BackendError
    rd, wl = _fisheye(64, 32), scenes.wl_discrete(WL)
    two = scenes.scene([(0.5, [_prism()]), (0.0, [_prism()])], max_hits=7)
    T = scenes.filter_term

    def refused(hb, scene, why):
        with pytest.raises(BackendError, match="deterministic") as e:
            hb.BeginSession(scene, rd, wl, 1000)
        assert why in str(e.value), str(e.value)
        # ... and the handle goes on: a session it does cover
        hb.set_option("capture_exits", 0)
        hb.set_option("rehit_strategy", 1)
        hb.set_color([], [])
        hb.set_filters([])
        assert run_session(hb, _base_scene(), rd, wl, 1000)[0].root_count == 1000
        assert hb.last_route().accum_mask == abi.ACCUM_FIXED
        hb.close()

    refused(hip_backend(seed=SEED, deterministic=1), two, "cont_order")
    hb = hip_backend(seed=SEED, deterministic=1)
    hb.set_color([scenes.color_set([(T("raypath", raypath=[3, 5]), "PBD", 0)])], [scenes.color_class([0])])
    refused(hb, _base_scene(), "colour")
    refused(hip_backend(seed=SEED, deterministic=1, capture_exits=1), _base_scene(), "capture_exits")
    refused(hip_backend(seed=SEED, deterministic=1, rehit_strategy=0), _base_scene(), "rehit_strategy")
    hb = hip_backend(seed=SEED, deterministic=1, filter_fast=0)      # the filter would run the generic filter kernels
    hb.set_filters([scenes.simple_filter(T("raypath", raypath=[3, 5]), "PBD")])
    refused(hb, scenes.scene([(0.0, [_prism(filter_id=1)])], max_hits=7), "generic filter kernels")
    # the option itself: 0 / 1, not inside a session
    hb = hip_backend(seed=SEED)
    with pytest.raises(BackendError, match="deterministic"):
        hb.set_option("deterministic", 2)
    hb.BeginSession(_base_scene(), rd, wl, 1000)
    with pytest.raises(BackendError, match="inside a session"):
        hb.set_option("deterministic", 1)
    hb.EndSession()
    with pytest.raises(BackendError, match="no fixed-point planes"):
        hb.peek_fixed()
    hb.close()


@pytest.mark.parametrize("route,opts,n", [("direct", dict(hit_log=0), 1 << 16), ("hit log", dict(hit_log=1), 1 << 16)])
def test_default_never_takes_the_fixed_route(route, opts, n):
    r = _run(_base_scene(), _fisheye(256, 128), n, det=0, **opts)
    assert r["mask"] & abi.ACCUM_FIXED == 0 and r["mask"] == (abi.ACCUM_SCALAR if route == "direct" else abi.ACCUM_LOG), (route, r["mask"])


# ---- 6. run to run ------------------------------------------------------------------------------------------------------------------------------
_CHILD = """
import sys
sys.path.insert(0, %r)
from tests.test_gpu_deterministic import _run, _base_scene, _fisheye
print("sha256", _run(_base_scene(), _fisheye(256, 128), (1 << 20) + 37)["sha"])
"""


def test_two_runs_and_a_fresh_process_give_the_same_bytes():
    n = (1 << 20) + 37
    a = _run(_base_scene(), _fisheye(256, 128), n)
    b = _run(_base_scene(), _fisheye(256, 128), n)
    assert a["sha"] == b["sha"] and a["landed_q"] == b["landed_q"]
    out = subprocess.run([sys.executable, "-c", _CHILD % ROOT], capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    assert out.stdout.split("sha256")[-1].strip() == a["sha"]
