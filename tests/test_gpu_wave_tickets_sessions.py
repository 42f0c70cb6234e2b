"""Whole sessions with and without wave tickets (option tile_ticket): the trace kernel of a launch that appends its records per tile
runs one resident round of workgroups whose WAVES draw their passes of the ray loop — 64 rays each — from a counter, instead of every workgroup
striding over its static share.

Every case traces the same sessions on the shapes of tests/test_gpu_tile_append_sessions.py — a 480 x 270 upper-sky fisheye, config2_scene, the
hit log forced on with one plane copy, close_direct = 1 and tile_append = 1 — with tile_ticket = 1 against 0.  The two runs trace the SAME rays (a
ray keeps its counter whoever traces it), so root, exit and pixel-hit counts agree exactly; the images agree within the project's bars for "same
rays, float order differs": sum rel 2e-6, max abs 2e-5 x max.  halo_tile_tickets says how many launches took tickets: all that append per tile
with the option on, none with it off; appends, direct closes and the route info do not change.

The landed weight, tickets on against off: both are sums of the same non-negative fp32 terms — a lane of the static loop sums its rays of the
whole launch in fp32, a lane of the ticketed loop whatever rays it drew in fp64.  A sum of k non-negative fp32 terms is within k x 2^-24 of the
exact one, relatively; a ray adds at most max_hits + 1 terms, so with K = (max_hits + 1) x the passes a lane of the static run sums in fp32 the two
agree to rel 2 K 2^-24 (the fp64 side's own error, k x 2^-53, is far inside the factor 2).  K comes from n and the static grid (1e-6 at 2^18 rays).
Tickets on against tickets on, in a second handle: which wave traces which ray, and where one ticket ends and the next begins, changes from run to
run; the fp64 lane sums differ by the order of adds only — rel 1e-12.  The shapes of the issue all draw tickets of the smallest size (a range of 64
passes and 128 for the rule's divisor at 2^18 rays), so a case of 2^22 rays with ticket_min = 1 and ticket_div = 1 — tickets of 12 passes down to
1, their sizes following racy reads of the counters — and a case with the options at their defaults, on launches whose static grid lies on either side of one resident round, stand beside them.
"""
import numpy as np
import pytest

from ice_halo_sim_amd import abi, backend, scenes
from tests._oracle_backend import run_session

pytestmark = pytest.mark.gpu

W, H = 480, 270
BASE = {"hit_log": 1, "mono_copies": 1, "close_direct": 1, "tile_append": 1}
N = 1 << 18
LO, HI, DIV, GROUPS = 4, 64, 2, 64   # the ticket rule's defaults and the counters of a launch (halo_device.h)


def _stats(sts):
    return [(int(st.root_count), int(st.exit_count), int(st.pixel_hits)) for st in sts]


def _run(sc, rd, wls, n=N, **opts):
    hb = backend.HipTraceBackend(device=0, seed=23, **{**BASE, **opts})
    sts = []
    for wl in wls:
        sts += _stats(run_session(hb, sc, rd, scenes.wl_discrete(wl), n))
    img, landed = hb.ReadbackXyzAccum(rd.width, rd.height)
    out = (sts, img, landed, hb.tile_appends(), hb.direct_closes(), hb.last_route().accum_mask, hb.tile_tickets())
    hb.close()
    return out


def _cus():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _landed_rel(sc, n_launch):
    """2 K 2^-24 for launches of n_launch rays: the static grid (halo_backend.cpp blocks_of: small launches spread over five workgroups per CU
    before a workgroup takes a second pass, 24 per CU at the most)."""
    cus = _cus()
    cap = min(24 * cus, max(5 * cus, n_launch // (256 * 32)))
    blocks = max(1, min((n_launch + 255) // 256, cap))
    static_passes = -(-n_launch // (256 * blocks))
    k = (sc.max_hits + 1) * max(static_passes, 1)
    return 2.0 * k * 2.0 ** -24


def _first_ticket(n_launch, lo=LO, div=DIV):
    """the size of the first ticket a wave draws in a ticketed launch of n_launch rays: the passes are cut into GROUPS ranges with a counter each,
    and the rule runs per range with the waves at home on it"""
    cus = _cus()
    cap = min(24 * cus, max(5 * cus, n_launch // (256 * 32)))
    blocks = max(1, min((n_launch + 255) // 256, cap, 6 * cus))
    per = backend.host_ticket_range(-(-n_launch // 64), 0)[1]
    return backend.host_ticket_size(per, 0, max(div * 4 * blocks // GROUPS, 1), lo, HI)


def _same(a, b, landed_rel, lit=True):
    (sts_a, img_a, la, app_a, closes_a, mask_a, _), (sts_b, img_b, lb, app_b, closes_b, mask_b, _) = a, b
    assert sts_a == sts_b, (sts_a, sts_b)
    assert app_a == app_b and closes_a == closes_b and mask_a == mask_b
    if lit:
        assert img_b.max() > 0 and lb > 0
    print("landed", la, lb, "rel", abs(la - lb) / max(abs(lb), 1e-300), "bar", landed_rel)
    assert la == pytest.approx(lb, rel=landed_rel, abs=0.0)
    assert img_a.sum(dtype=np.float64) == pytest.approx(img_b.sum(dtype=np.float64), rel=2e-6, abs=0.0)
    assert np.abs(img_a - img_b).max() <= 2e-5 * float(img_b.max())


def _three(sc, rd, wls, n=N, n_last=None, lit=True, **opts):
    """tickets on, off, and on again in a second handle"""
    on, off, again = _run(sc, rd, wls, n, tile_ticket=1, **opts), _run(sc, rd, wls, n, tile_ticket=0, **opts), _run(sc, rd, wls, n, tile_ticket=1, **opts)
    assert off[6] == 0, off[6]
    assert on[6] == on[3] == again[6], (on[6], on[3], again[6])   # every launch that appends per tile takes tickets
    _same(on, off, _landed_rel(sc, n_last if n_last is not None else n), lit)
    _same(again, on, 1e-12, lit)
    return on


@pytest.mark.parametrize("n", [1, 65, (1 << 12) + 1, (1 << 18) - 1, 1 << 18])
def test_ray_counts_at_the_edges_of_the_loop(n):
    """fewer tickets than waves (1, 65), a ragged last wave (65, 2^12 + 1, 2^18 - 1), a last ticket of one pass (2^12 + 1: 65 passes in ranges of two)"""
    on = _three(scenes.config2_scene(), scenes.config2_render(W, H), [450.0, 610.0], n=n, lit=n > 4096)
    assert on[3] == 2 and on[4] == 2 and on[6] == 2 and on[5] == abi.ACCUM_LOG
    assert [s[0] for s in on[0]] == [n, n]


def test_guided_tickets_whose_sizes_follow_the_counters():
    """2^22 rays with ticket_min = 1 and ticket_div = 1: a range holds 1024 passes and the first tickets are several passes long (12 on 256 CUs), the
    later ones shorter, each sized from a read of its counter that races with the other waves' adds — boundaries that differ from run to run"""
    n = 1 << 22
    assert _first_ticket(n, lo=1, div=1) > LO and _first_ticket(N) == LO   # this case draws guided tickets; the 2^18-ray cases do not
    on = _three(scenes.config2_scene(), scenes.config2_render(W, H), [450.0, 610.0], n=n, ticket_min=1, ticket_div=1)
    assert on[3] == 2 and on[6] == 2 and on[5] == abi.ACCUM_LOG
    assert [s[0] for s in on[0]] == [n, n]


def test_default_options_take_tickets_beyond_one_resident_round_only():
    """tile_ticket at its default (-2) beside close_direct and tile_append at theirs, 2^20 rays with alt_log2 = 17 (the chip-filling side).  Spread
    over eight workgroups per CU (small_blocks_per_cu = 8) the static grid is 2048 workgroups on 256 CUs, more than the 1536 of one resident
    round: the launches take tickets.  At the default five per CU it is 1280: they append per tile and keep the static loop — and with it the
    split route's landed weight to rel 1e-12, as do the 2^18-ray launches of tests/test_gpu_tile_append_sessions.py."""
    sc, rd, wls = scenes.config2_scene(), scenes.config2_render(W, H), [450.0, 610.0, 450.0]
    n = 1 << 20
    cus = _cus()
    assert 5 * cus < 6 * cus < min(8 * cus, n // 256)   # the two static grids lie on either side of one resident round
    auto = {"close_direct": -1, "tile_append": -1, "alt_log2": 17}
    wide, wide_again = _run(sc, rd, wls, n, small_blocks_per_cu=8, **auto), _run(sc, rd, wls, n, small_blocks_per_cu=8, **auto)
    wide_off = _run(sc, rd, wls, n, small_blocks_per_cu=8, tile_ticket=0, **auto)
    assert wide[3] == 3 and wide[4] == 3 and wide[6] == 3 and wide_again[6] == 3, (wide[3:], wide_again[3:])
    assert wide_off[3] == 3 and wide_off[6] == 0
    _same(wide, wide_off, 2.0 * (sc.max_hits + 1) * -(-n // (256 * min(8 * cus, n // 256))) * 2.0 ** -24)
    _same(wide_again, wide, 1e-12)
    narrow, narrow_split = _run(sc, rd, wls, n, **auto), _run(sc, rd, wls, n, close_direct=-1, tile_append=0, alt_log2=17)
    assert narrow[3] == 3 and narrow[6] == 0 and narrow_split[3] == 0
    _same_but_appends(narrow, narrow_split)


def _same_but_appends(a, b):
    (sts_a, img_a, la, _, closes_a, mask_a, _), (sts_b, img_b, lb, _, closes_b, mask_b, _) = a, b
    assert sts_a == sts_b and closes_a == closes_b and mask_a == mask_b
    assert la == pytest.approx(lb, rel=1e-12, abs=0.0)
    assert np.abs(img_a - img_b).max() <= 2e-5 * float(img_b.max())


def test_six_sessions_alternating_two_wavelengths_on_one_handle():
    """the counters are back at zero for every launch, and the two log sets — each with counters of its own — take turns"""
    on = _three(scenes.config2_scene(), scenes.config2_render(W, H), [450.0, 610.0] * 3)
    assert on[3] == 6 and on[4] == 6 and on[6] == 6 and on[5] == abi.ACCUM_LOG
    img = on[1]   # both colours are there
    assert img[..., 2].sum() > 0.2 * img[..., 1].sum() and img[..., 0].sum() > 0.2 * img[..., 1].sum()


def test_chunks_that_overflow_into_the_twin():
    """hit_log_cap = 256: two records per chunk, most records find their chunk full and go to the fp64 twin"""
    on = _three(scenes.config2_scene(), scenes.config2_render(W, H), [450.0, 610.0, 610.0, 450.0], hit_log_cap=256)
    assert on[6] == 4


def test_two_layer_scene_whose_last_layer_reads_the_continuation_pool():
    """the last layer's roots come from the pool (the transit root form of the ticketed kernel); canonical continuation order, so that all runs trace
    the same rays on the second layer too"""
    sc = scenes.config3_scene()
    probe = _run(sc, scenes.config2_render(W, H), [450.0], tile_ticket=0, cont_order=1)
    n_last = probe[0][-1][0]   # the rays of the last layer's launch
    assert 0 < n_last
    on = _three(sc, scenes.config2_render(W, H), [450.0, 610.0], n_last=n_last, cont_order=1)
    assert on[6] == 2 and on[5] == abi.ACCUM_NONE | abi.ACCUM_LOG


def test_auto_mode_takes_launches_that_fill_the_chip_and_leaves_small_ones():
    """tile_ticket = -1 follows tile_append's auto rule: alt_log2 = 17 puts the 2^18-ray launches of this test on the chip-filling side, and without
    it none of them takes tickets — not even with the append itself forced on"""
    sc, rd, wls = scenes.config2_scene(), scenes.config2_render(W, H), [450.0, 610.0, 450.0, 610.0]
    auto = {"close_direct": -1, "tile_append": -1, "tile_ticket": -1}
    small, filling = _run(sc, rd, wls, **auto), _run(sc, rd, wls, alt_log2=17, **auto)
    forced_append = _run(sc, rd, wls, tile_ticket=-1)
    never = _run(sc, rd, wls, alt_log2=17, close_direct=-1, tile_append=-1, tile_ticket=0)
    assert small[6] == 0 and small[3] == 0
    assert filling[6] == 4 and filling[3] == 4 and filling[4] == 4
    assert forced_append[6] == 0 and forced_append[3] == 4
    assert never[6] == 0 and never[3] == 4 and never[4] == 4
    _same(filling, never, _landed_rel(sc, N))
    assert small[0] == never[0]
