"""Root profiles: the last-layer plain hit-log kernels of one regular hexagonal prism with their root generation as compile-time constants
(`halo_trace_kernel<0,3,true,kAccLogFinal,LENS,VIS,true,false,ROOT>`, halo_trace.inl kRoot*) against the same launch with the run-time form
(option spec_root = 0).  The two trace the SAME rays — same draws, same stream slots, same expressions — so the device tallies that are sums of
integers (roots, exits, pixel hits) are equal exactly, the weight sums within the suite's 1e-4 relative bar for landed weight,
and the image within the 2e-5 bar of test_hit_log_route_equals_the_direct_route: the only difference allowed is the order of the fp32 adds
inside a workgroup's pixel cache, which that bar is sized for.  `halo_last_root_profile` says which form ran.

Every case runs 2^21 rays (the smallest launch that takes the hit log on an upper-hemisphere render) on a 480 x 270 fisheye equal-area image."""
import os
import re

import numpy as np
import pytest

from ice_halo_sim_amd import abi, scenes
from tests._oracle_backend import run_session

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 1 << 21
FULL = {"type": "uniform", "mean": 0.0, "std": 360.0}
SPEC_ALL = abi.SPEC_LAST | abi.SPEC_LENS | abi.SPEC_VIS | abi.SPEC_NOGATE


def rel_l2(a, b):
    return float(np.linalg.norm(a.astype(np.float64) - b) / max(np.linalg.norm(b.astype(np.float64)), 1e-30))


def _host_rays(n):
    """Crystal-local rays onto the top basal face of the h = 1.3 column (the construction of test_gpu_production_routes' queued sessions)."""
    g = np.random.default_rng(5)
    d = g.normal(size=(n, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d[:, 2] = -np.abs(d[:, 2]) - 0.2
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    p = np.zeros((n, 3), np.float32)
    p[:, 2] = 0.65
    p[:, :2] = g.uniform(-0.3, 0.3, size=(n, 2)).astype(np.float32)
    return d, p, np.ones(n, np.float32), np.zeros(n, np.uint32)


def _run(scene, wl, spec_root, host_rays=None, **opts):
    from ice_halo_sim_amd.backend import HipTraceBackend
    hb = HipTraceBackend(device=0, seed=61, spec_root=spec_root, **opts)
    rd = scenes.config2_render(480, 270)
    if host_rays is None:
        st = run_session(hb, scene, rd, wl, N)
    else:
        hb.BeginSession(scene, rd, wl, N)
        st = [hb.TraceLayer(N, host_rays=host_rays)]
        hb.EndSession()
    route, root = hb.last_route(), hb.last_root_profile()
    img, landed = hb.ReadbackXyzAccum()
    hb.close()
    return {"st": st, "route": route, "root": root, "img": img, "landed": landed}


def _same_rays_same_image(on, off, what):
    """The issue's bars: integer tallies exact, weights rel 1e-4, image rel L2 2e-5 (figures printed before they are held to them)."""
    so, sf = on["st"][-1], off["st"][-1]
    err = rel_l2(on["img"], off["img"])
    print("%s: roots %d / %d, exits %d / %d, pixel hits %d / %d, landed %.9g / %.9g, exit weight %.9g / %.9g, image rel L2 %.2e, root profile %d / %d, generic launches %d / %d"
          % (what, so.root_count, sf.root_count, so.exit_count, sf.exit_count, so.pixel_hits, sf.pixel_hits, on["landed"], off["landed"], so.exit_w_sum, sf.exit_w_sum,
             err, on["root"], off["root"], on["route"].generic_launches, off["route"].generic_launches))
    for a, b in zip(on["st"], off["st"]):
        assert (a.root_count, a.exit_count, a.pixel_hits, a.continuation_count) == (b.root_count, b.exit_count, b.pixel_hits, b.continuation_count)
        assert a.exit_w_sum == pytest.approx(b.exit_w_sum, rel=1e-4)
    assert off["img"].sum() > 0 and sf.pixel_hits > 0
    assert on["landed"] == pytest.approx(off["landed"], rel=1e-4)
    assert err <= 2e-5, err
    for f in ("launches", "mode_mask", "geom_mask", "accum_mask", "source_mask", "spec_mask", "generic_launches"):   # the option moves none of them
        assert getattr(on["route"], f) == getattr(off["route"], f), f


def test_spec_root_is_a_known_option_and_defaults_to_on():
    """No GPU needed: the option is a row of the option table that stores a boolean, the options start with it on, and the header documents both.
    (tests/test_cpp_options.py checks the first two by running the table: the key is accepted, 0 / 1 / 7 / -3 store 0 / 1 / 1 / 1, the default is 1.)"""
    src = open(os.path.join(ROOT, "ice_halo_sim_amd", "csrc", "halo_options.h")).read()
    assert re.search(r'^\s*\{"spec_root", &Options::spec_root, kOptBool, 0, ', src, re.M)
    assert re.search(r"^\s*int spec_root = 1;", src, re.M)
    header = open(os.path.join(ROOT, "include", "halo_trace.h")).read()
    assert '"spec_root" (1 [default]' in header


@pytest.mark.gpu
def test_generated_roots_profile_traces_the_same_rays_to_the_same_image():
    """The benchmark scene's crystal and axis (configs[1]: column, latitude by the LUT, azimuth and roll uniform), one discrete wavelength."""
    sc, wl = scenes.config2_scene(), scenes.wl_discrete(550.0)
    on, off = _run(sc, wl, 1), _run(sc, wl, 0)
    _same_rays_same_image(on, off, "generated roots")
    r = on["route"]
    assert (r.mode_mask, r.geom_mask, r.accum_mask, r.launches) == (abi.MODE_PLAIN, 1 << 3, abi.ACCUM_LOG, 1), (r.mode_mask, r.geom_mask, r.accum_mask, r.launches)
    assert r.spec_mask == SPEC_ALL and r.generic_launches == 0
    assert on["root"] == abi.ROOT_GEN and off["root"] == 0


@pytest.mark.gpu
def test_transit_profile_traces_the_same_rays_to_the_same_image():
    """configs[2]: plate at prob 1 over a column whose axis is LUT latitude, uniform azimuth and roll — the last layer reads the continuation pool.
    Canonical continuation order (cont_order = 1) hands both runs the pool in the same order, so the last layer traces the same rays in both
    and the exact bars mean something (in append order, wave scheduling decides which ray meets which draw)."""
    sc, wl = scenes.config3_scene(), scenes.wl_discrete(550.0)
    on, off = _run(sc, wl, 1, cont_order=1), _run(sc, wl, 0, cont_order=1)
    assert on["st"][0].continuation_count == off["st"][0].continuation_count == on["st"][1].root_count >= N   # first layer: equal exactly
    _same_rays_same_image(on, off, "continuation pool")
    r = on["route"]
    assert r.mode_mask == abi.MODE_PLAIN and r.geom_mask == 1 << 3 and r.source_mask == 0b011 and r.accum_mask & abi.ACCUM_LOG, (r.mode_mask, r.geom_mask, r.source_mask, r.accum_mask)
    assert r.spec_mask & SPEC_ALL == SPEC_ALL
    assert on["root"] == abi.ROOT_TRANSIT and off["root"] == 0   # the last layer alone: the first one is no last-layer kernel


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["gauss_azimuth", "full_sphere_axis", "two_entry_pool", "host_rays"])
def test_what_matches_no_profile_runs_the_generic_root_generation(case):
    """One step off the profile each: none may report it, and the option changes nothing."""
    col, wl, rays = scenes.prism_crystal(1.3, [1.0] * 6), scenes.wl_discrete(550.0), None
    if case == "gauss_azimuth":
        ax = scenes.axis(zenith={"type": "gauss", "mean": 90, "std": 0.3}, azimuth={"type": "gauss", "mean": 0, "std": 40}, roll=FULL)
    elif case == "full_sphere_axis":
        ax = scenes.axis(zenith=FULL, azimuth=FULL, roll=FULL)
    else:
        ax = scenes.column_crystal_entry().axis
    if case == "two_entry_pool":
        wl = scenes.wl_illuminant("D65", 2)
    if case == "host_rays":
        rays = _host_rays(N)
    sc = scenes.scene([(0.0, [scenes.entry(col, ax, 10.0, 3)])], max_hits=7)
    on, off = _run(sc, wl, 1, host_rays=rays), _run(sc, wl, 0, host_rays=rays)
    _same_rays_same_image(on, off, case)
    assert on["root"] == 0 and off["root"] == 0
    assert on["route"].source_mask == (0b100 if case == "host_rays" else 0b001)
