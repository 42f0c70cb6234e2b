"""Whole sessions with and without the per-tile append (option tile_append): the trace kernel of a launch that closes its session
directly appends its records to per-tile chunks of each workgroup, and the closing pass reads the chunks — no split pass.

Every case traces the same sessions twice, tile_append = 1 against 0, on the shapes of tests/test_gpu_direct_close_sessions.py: a 480 x 270
upper-sky fisheye, config2_scene, 2^18 rays per session, the hit log forced on with one plane copy, and close_direct = 1 (the append exists where
a launch closes directly).  The two runs trace the SAME rays (monotone ray counters), so root, exit and pixel-hit counts agree exactly and the
landed weight to rel 1e-12; the images agree within the project's bars for "same rays, float order differs": sum rel 2e-6, max abs 2e-5 x max.
halo_tile_appends says how many launches took the new route: all of the eligible ones, none of the others; the route info does not change.
"""
import numpy as np
import pytest

from ice_halo_sim_amd import abi, scenes
from tests._oracle_backend import run_session

pytestmark = pytest.mark.gpu

W, H = 480, 270
BASE = {"hit_log": 1, "mono_copies": 1, "close_direct": 1}
N = 1 << 18


def _stats(sts):
    return [(int(st.root_count), int(st.exit_count), int(st.pixel_hits)) for st in sts]


def _sessions(hb, sc, rd, wls, n=N):
    sts = []
    for wl in wls:
        sts += _stats(run_session(hb, sc, rd, scenes.wl_discrete(wl), n))
    return sts


def _run(sc, rd, wls, **opts):
    from ice_halo_sim_amd.backend import HipTraceBackend
    hb = HipTraceBackend(device=0, seed=23, **{**BASE, **opts})
    sts = _sessions(hb, sc, rd, wls)
    img, landed = hb.ReadbackXyzAccum(rd.width, rd.height)
    out = (sts, img, landed, hb.tile_appends(), hb.direct_closes(), hb.last_route().accum_mask)
    hb.close()
    return out


def _same(a, b):
    (sts_a, img_a, la, _, closes_a, mask_a), (sts_b, img_b, lb, _, closes_b, mask_b) = a, b
    assert sts_a == sts_b, (sts_a, sts_b)
    assert closes_a == closes_b and mask_a == mask_b   # a launch that appends per tile closes directly and is a logged launch like any other
    assert img_b.max() > 0 and lb > 0
    assert la == pytest.approx(lb, rel=1e-12)
    assert img_a.sum(dtype=np.float64) == pytest.approx(img_b.sum(dtype=np.float64), rel=2e-6)
    assert np.abs(img_a - img_b).max() <= 2e-5 * float(img_b.max())


def _both(sc, rd, wls, **opts):
    on, off = _run(sc, rd, wls, tile_append=1, **opts), _run(sc, rd, wls, tile_append=0, **opts)
    assert off[3] == 0, off[3]
    _same(on, off)
    return on


def test_six_sessions_alternating_two_wavelengths_all_append_per_tile():
    on = _both(scenes.config2_scene(), scenes.config2_render(W, H), [450.0, 610.0] * 3)
    assert on[3] == 6 and on[4] == 6 and on[5] == abi.ACCUM_LOG
    img = on[1]   # both colours are there
    assert img[..., 2].sum() > 0.2 * img[..., 1].sum() and img[..., 0].sum() > 0.2 * img[..., 1].sum()


def test_auto_mode_takes_launches_that_fill_the_chip_and_leaves_small_ones():
    """tile_append = -1 beside close_direct = -1: a launch of <= 2^alt_log2 rays keeps the fold and the split; alt_log2 = 17 puts the 2^18-ray
    launches of this test on the chip-filling side"""
    sc, rd, wls = scenes.config2_scene(), scenes.config2_render(W, H), [450.0, 610.0, 450.0, 610.0]
    auto = {"close_direct": -1, "tile_append": -1}
    small, filling = _run(sc, rd, wls, **auto), _run(sc, rd, wls, alt_log2=17, **auto)
    never = _run(sc, rd, wls, alt_log2=17, close_direct=-1, tile_append=0)
    assert small[3] == 0 and filling[3] == 4 and never[3] == 0
    assert filling[4] == 4 and never[4] == 4 and small[4] == 0
    _same(filling, never)
    assert small[0] == never[0]


def test_chunks_that_overflow_into_the_twin():
    """hit_log_cap = 256: two records per chunk, most records find their chunk full and go to the fp64 twin, which the closing pass takes in and zeroes,
    session after session"""
    on = _both(scenes.config2_scene(), scenes.config2_render(W, H), [450.0, 610.0, 610.0, 450.0], hit_log_cap=256)
    assert on[3] == 4


def test_two_layer_scene_whose_last_layer_reads_the_continuation_pool():
    """a plate layer whose every exit continues over a column layer of one launch: the last layer's roots come from the pool (the transit root
    form of the kernel); canonical continuation order, so that both runs trace the same rays on the second layer too"""
    on = _both(scenes.config3_scene(), scenes.config2_render(W, H), [450.0, 610.0], cont_order=1)
    assert on[3] == 2 and on[5] == abi.ACCUM_NONE | abi.ACCUM_LOG


def test_a_lens_without_an_instantiation_keeps_the_split():
    """the equidistant fisheye is no template constant of the last-layer kernels: the launch closes directly over the split pass's lists"""
    rd = scenes.render(abi.LENS_FISHEYE_EQUIDISTANT, W, H, fov=180.0, el=30.0, visible=abi.VISIBLE_UPPER)
    on = _both(scenes.config2_scene(), rd, [450.0, 610.0])
    assert on[3] == 0 and on[4] == 2
