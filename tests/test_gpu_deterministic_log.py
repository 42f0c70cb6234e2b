"""Deterministic sessions under the hit log (options deterministic = 1, hit_log = 1): a hit that loses the cache claim leaves as a raw record and
the integer twins of the split and per-tile passes quantise it with the session's F — so a logged deterministic launch must leave, bit for bit,
the integers the direct deterministic launch (hit_log = 0) leaves.  Every comparison below is integer or byte equality on the peeked planes, the
landed integer with F and F_L, and the image bytes with the landed weight.  No tolerance anywhere.

Scenes, lens, seed and ray_base are those of tests/test_gpu_deterministic.py."""
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
DIRECT, LOGGED, LOGGED_XYZ = abi.ACCUM_FIXED, abi.ACCUM_FIXED | abi.ACCUM_LOG, abi.ACCUM_FIXED | abi.ACCUM_LOG_XYZ


def hip_backend(**kw):
    from ice_halo_sim_amd.backend import HipTraceBackend
    return HipTraceBackend(device=0, **kw)


def _prism(filter_id=0):
    return scenes.entry(scenes.prism_crystal(1.0), scenes.axis(zenith=FULL, azimuth=FULL, roll=FULL), 1.0, 1, filter_id=filter_id)


def _base_scene():
    return scenes.scene([(0.0, [_prism()])], max_hits=7, sun_altitude=20.0)


def _fisheye(w, h):
    return scenes.render(abi.LENS_FISHEYE_EQUAL_AREA, w, h, fov=180.0, el=30.0, visible=abi.VISIBLE_UPPER)


def _run(scene, render, n, wl=None, parts=1, filters=(), det=1, part_opts=None, **opts):
    """Trace `n` roots as `parts` sessions on a fresh handle (part_opts: options set before session k, cycled).  Returns the peeked integers
    (det = 1) or the captured exits, the image bytes, the per-layer counts, the pixel hits and what the routes say."""
    wl = wl or scenes.wl_discrete(WL)
    hb = hip_backend(seed=SEED, **opts)
    hb.set_option("deterministic", det)
    hb.set_option("ray_base", RAY_BASE)
    hb.set_filters(list(filters))
    cuts = [n // parts] * (parts - 1) + [n - (parts - 1) * (n // parts)]
    stats, masks, modes, geoms, hits = [], [], 0, 0, 0
    for k, m in enumerate(cuts):
        for key, v in (part_opts[k % len(part_opts)] if part_opts else {}).items():
            hb.set_option(key, v)
        st = run_session(hb, scene, render, wl, m)
        stats += [(int(s.root_count), int(s.continuation_count)) for s in st]
        hits += sum(int(s.pixel_hits) for s in st)
        r = hb.last_route()
        masks.append(r.accum_mask)
        modes, geoms = modes | r.mode_mask, geoms | r.geom_mask
    mask = 0
    for m in masks:
        mask |= m
    out = dict(stats=stats, mask=mask, masks=masks, modes=modes, geoms=geoms, planes=hb.last_route().plane_cnt, hits=hits)
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
    assert len(a["sums"]) == len(b["sums"]), what
    for p, (x, y) in enumerate(zip(a["sums"], b["sums"])):
        bad = np.flatnonzero(x.ravel() != y.ravel())
        assert bad.size == 0, "%s: plane %d differs in %d pixels, first %d: %d vs %d" % (what, p, bad.size, bad[0], x.ravel()[bad[0]], y.ravel()[bad[0]])
    assert a["landed_q"] == b["landed_q"], what
    assert a["img"] == b["img"], what
    assert a["landed"] == b["landed"], what


LOG_PLANS = [("default", {}), ("chunk", dict(chunk=1 << 16)), ("blocks_per_cu", dict(blocks_per_cu=1)), ("overlap", dict(overlap=0)), ("async", {"async": 1}),
             ("four sessions", dict(parts=4)), ("aggregate 0", dict(aggregate=0))]


# ---- 1. logged equals direct --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,n", [(256, 128, (1 << 18) + 37), (17, 13, (1 << 18) + 37), (1920, 1080, 1 << 18)])
def test_logged_launches_leave_the_integers_of_direct_launches(w, h, n):
    """256 x 128: 32 Ki pixels meet 1024 cache slots, most hits become records, the sun's pixels are hot; 17 x 13: every pixel is cached — empty
    tile lists, near-empty regions; 1920 x 1080: 2 Mi slots, 16 Ki-slot tiles, few records per tile."""
    sc, rd = _base_scene(), _fisheye(w, h)
    ref = _run(sc, rd, n, hit_log=0)
    assert ref["mask"] == DIRECT and ref["planes"] == 1 and ref["modes"] == abi.MODE_PLAIN and ref["geoms"] == 1 << 3
    assert ref["landed_q"] > 0 and int(ref["sums"][0].sum(dtype=np.uint64)) > 0 and ref["F"] == 29 and ref["FL"] == 27
    for name, kw in LOG_PLANS:
        got = _run(sc, rd, n, hit_log=1, **kw)
        assert got["mask"] == LOGGED and got["geoms"] == ref["geoms"] and got["modes"] == ref["modes"], (name, got["mask"])
        _same(ref, got, name)


def test_direct_and_logged_sessions_share_one_pending_plane_set():
    """Four sessions under lazy_fold alternate hit_log 0 / 1 into one pending plane set with one F: the bytes of either route alone."""
    sc, rd, n = _base_scene(), _fisheye(256, 128), (1 << 18) + 37
    ref = _run(sc, rd, n, hit_log=0, parts=4)
    log = _run(sc, rd, n, hit_log=1, parts=4)
    mix = _run(sc, rd, n, parts=4, part_opts=[dict(hit_log=0), dict(hit_log=1)])
    assert ref["masks"] == [DIRECT] * 4 and log["masks"] == [LOGGED] * 4 and mix["masks"] == [DIRECT, LOGGED, DIRECT, LOGGED]
    _same(ref, log, "logged alone")
    _same(ref, mix, "alternating")


def test_auto_takes_the_log_on_a_chip_filling_scalar_launch():
    """Default options (hit_log = -1): 8 Mi rays over the upper sky pass the scalar threshold of 2 Mi, so the launch is logged — 128 contiguous
    tiles, the integer twin of halo_bin_accumulate_range_kernel — and leaves the bytes of the same run on the direct route."""
    sc, rd, n = _base_scene(), _fisheye(256, 128), 8 << 20
    auto = _run(sc, rd, n)
    assert auto["mask"] == LOGGED, auto["mask"]
    ref = _run(sc, rd, n, hit_log=0)
    assert ref["mask"] == DIRECT
    _same(ref, auto, "auto")


# ---- 2. both overflow fallbacks -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("illum", ["scalar", "D65"])
def test_full_regions_and_full_tile_lists_add_the_same_integers(illum):
    """hit_log_cap = 2048 records per region, every hit a record (aggregate = 0), the launch held to 32 workgroups: the landed hits outnumber all
    the regions' room by more than two, so the trace kernel's own fallback runs; the tile lists get half their even share of what the regions
    hold, so the split pass's runs too."""
    blocks, cap = 32, 2048
    wl = scenes.wl_illuminant("D65", 31) if illum == "D65" else None
    sc, rd, n = _base_scene(), _fisheye(256, 128), 1 << 18
    ref = _run(sc, rd, n, wl=wl, hit_log=0)
    got = _run(sc, rd, n, wl=wl, hit_log=1, aggregate=0, hit_log_cap=cap, blocks_cap=blocks)
    assert got["hits"] > 2 * cap * blocks, (got["hits"], cap * blocks)
    assert ref["mask"] == DIRECT and got["mask"] == (LOGGED_XYZ if illum == "D65" else LOGGED)
    assert ref["planes"] == got["planes"] == (3 if illum == "D65" else 1)
    _same(ref, got, illum)
    # ... and with the cache on: cached pixels never leave as records, the rest still overflows
    _same(ref, _run(sc, rd, n, wl=wl, hit_log=1, hit_log_cap=cap, blocks_cap=blocks), illum + ", cache on")


# ---- 3. every kernel family ---------------------------------------------------------------------------------------------------------------------
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
def test_every_kernel_family_logged_against_direct(family):
    f = _families()[family]
    kw = dict(wl=f.get("wl"), filters=f.get("filters", ()))
    n = 1 << 18
    a = _run(f["scene"], f["render"], n, hit_log=0, **kw)
    b = _run(f["scene"], f["render"], n, hit_log=1, **kw)
    assert a["mask"] == DIRECT and b["mask"] == (LOGGED_XYZ if f["planes"] == 3 else LOGGED), (family, a["mask"], b["mask"])
    for r in (a, b):
        assert r["geoms"] == f["geoms"] and r["planes"] == f["planes"] and r["modes"] == f.get("modes", abi.MODE_PLAIN), family
    assert b["geoms"] == a["geoms"] and b["modes"] == a["modes"]
    assert all(int(s.sum(dtype=np.uint64)) > 0 for s in a["sums"]) and a["landed_q"] > 0
    _same(a, b, family)


# ---- 4. against the rays themselves -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("crystal", ["regular prism", "fixed pyramid"])
def test_every_hit_through_the_passes_sums_to_the_captured_rays(crystal):
    """aggregate = 0 under the log: every hit is a record, so the planes are what the split and the per-tile sums made of the records alone.  They
    must hold, pixel by pixel, the sum of q(weight) over the exits the capture kernels hand out for the same seed."""
    c = scenes.prism_crystal(1.0) if crystal == "regular prism" else scenes.pyramid_crystal(0.3, 1.0, 0.2)
    sc = scenes.scene([(0.0, [scenes.entry(c, scenes.axis(zenith=FULL, azimuth=FULL, roll=FULL), 1.0, 1)])], max_hits=7, sun_altitude=20.0)
    rd = scenes.render(abi.LENS_LINEAR, 128, 64, fov=90.0, el=30.0, visible=abi.VISIBLE_UPPER)
    n = 1 << 16
    ex = _run(sc, rd, n, det=0, capture_exits=1)["ex"]
    assert (ex["pixel"] >= 0).sum() > 1000
    det = _run(sc, rd, n, hit_log=1, aggregate=0)
    assert det["mask"] == LOGGED
    want = fm.plane_sums(ex["pixel"], ex["weight"], 128 * 64, det["F"]).reshape(64, 128)
    bad = np.flatnonzero(want.ravel() != det["sums"][0].ravel())
    assert bad.size == 0, "%d pixels differ, first %d: captured %d, plane %d" % (bad.size, bad[0], want.ravel()[bad[0]], det["sums"][0].ravel()[bad[0]])
    assert det["landed_q"] == int(fm.q(ex["weight"][ex["pixel"] >= 0], det["FL"]).sum(dtype=np.uint64))


# ---- 5. two layers ------------------------------------------------------------------------------------------------------------------------------
def test_two_layers_log_the_last_layer_over_the_continuation_pool():
    plate = scenes.entry(scenes.prism_crystal(0.3), scenes.axis(zenith={"type": "gauss", "mean": 0, "std": 0.8}), 1.0, 6)
    col = scenes.entry(scenes.prism_crystal(1.3, [1.0] * 6), scenes.axis(zenith={"type": "uniform", "mean": 90, "std": 360}, azimuth=FULL), 1.0, 3)
    sc = scenes.scene([(0.5, [plate]), (0.0, [col])], max_hits=7)
    rd, n = _fisheye(256, 128), 1 << 16
    a = _run(sc, rd, n, cont_order=1, hit_log=0)
    b = _run(sc, rd, n, cont_order=1, hit_log=1)
    assert a["mask"] == DIRECT and b["mask"] == LOGGED     # the first layer runs the CANON direct twin, the last layer the log
    assert a["stats"][0][1] > 0 and a["stats"] == b["stats"]
    _same(a, b, "two layers")


# ---- 6. what must not change --------------------------------------------------------------------------------------------------------------------
def test_float_sessions_keep_their_routes():
    sc, rd, n = _base_scene(), _fisheye(256, 128), 1 << 16
    r = _run(sc, rd, n, det=0, hit_log=1)
    assert r["mask"] == abi.ACCUM_LOG
    r = _run(sc, rd, n, det=0, hit_log=1, aggregate=0)      # the float route's log needs the cache: direct, as before
    assert r["mask"] == abi.ACCUM_SCALAR
    r = _run(sc, rd, n, hit_log=-1)                          # below the auto thresholds: the direct deterministic route
    assert r["mask"] == DIRECT
    r = _run(sc, rd, n, hit_log=-1, aggregate=0)
    assert r["mask"] == DIRECT


@pytest.mark.parametrize("hit_log", [0, 1])
def test_refusals_do_not_depend_on_hit_log(hit_log):
    from ice_halo_sim_amd.backend import BackendError
    rd, wl = _fisheye(64, 32), scenes.wl_discrete(WL)
    T = scenes.filter_term

    def refused(hb, scene, why):
        with pytest.raises(BackendError, match="deterministic") as e:
            hb.BeginSession(scene, rd, wl, 1000)
        assert why in str(e.value), str(e.value)
        hb.close()

    hb = hip_backend(seed=SEED, deterministic=1, hit_log=hit_log)
    hb.set_color([scenes.color_set([(T("raypath", raypath=[3, 5]), "PBD", 0)])], [scenes.color_class([0])])
    refused(hb, _base_scene(), "deterministic = 1: raypath-colour tables are set (the class lanes are fp64 atomics)")
    refused(hip_backend(seed=SEED, deterministic=1, hit_log=hit_log, capture_exits=1), _base_scene(),
            "deterministic = 1: capture_exits = 1 is not supported (the capture kernels have no fixed-point route)")
    refused(hip_backend(seed=SEED, deterministic=1, hit_log=hit_log, rehit_strategy=0), _base_scene(),
            "deterministic = 1: rehit_strategy = 0 is not supported (the legacy strategy lives in the generic kernels)")
    hb = hip_backend(seed=SEED, deterministic=1, hit_log=hit_log, filter_fast=0)
    hb.set_filters([scenes.simple_filter(T("raypath", raypath=[3, 5]), "PBD")])
    refused(hb, scenes.scene([(0.0, [_prism(filter_id=1)])], max_hits=7),
            "deterministic = 1: a filter of this scene needs the generic filter kernels (filter_fast = 0, max_hits > 16, or tables that do not fit the fast form)")


# ---- 7. run to run ------------------------------------------------------------------------------------------------------------------------------
_CHILD = """
import sys
sys.path.insert(0, %r)
from tests.test_gpu_deterministic_log import _run, _base_scene, _fisheye
r = _run(_base_scene(), _fisheye(256, 128), (1 << 18) + 37, hit_log=1)
print("mask", r["mask"], "sha256", r["sha"])
"""


def test_two_logged_runs_and_a_fresh_process_give_the_same_bytes():
    n = (1 << 18) + 37
    a = _run(_base_scene(), _fisheye(256, 128), n, hit_log=1)
    b = _run(_base_scene(), _fisheye(256, 128), n, hit_log=1)
    assert a["mask"] == LOGGED and a["sha"] == b["sha"] and a["landed_q"] == b["landed_q"]
    out = subprocess.run([sys.executable, "-c", _CHILD % ROOT], capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    assert out.stdout.split("mask")[-1].split()[0] == str(LOGGED)
    assert out.stdout.split("sha256")[-1].strip() == a["sha"]
