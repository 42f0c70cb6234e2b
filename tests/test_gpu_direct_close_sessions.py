"""Whole sessions with and without the direct close (option close_direct): a hit-log launch that is its whole session adds its tile
sums to the XYZ image in its own per-tile pass instead of writing the plane for a closing fold on the auxiliary stream.

Every case traces the same sessions twice, close_direct = 1 against 0, on a 480 x 270 upper-sky fisheye with the hit log forced on (hit_log = 1,
one plane copy).  The two runs trace the SAME rays (monotone ray counters), so root, exit and pixel-hit counts agree exactly and the landed weight
to rel 1e-12; the images agree within the bars the project uses for "same rays, float order differs"
(tests/test_gpu_production_routes.py::test_many_small_sessions_fold_once_and_equal_the_eager_fold): sum rel 2e-6, max abs 2e-5 x max — a pixel
whose cache flushes and log records arrive in another order rounds differently, nothing else moves.  halo_direct_closes says how many launches
took the new path: all of the eligible ones, none of the others.
"""
import numpy as np
import pytest

from ice_halo_sim_amd import abi, scenes
from tests._oracle_backend import run_session

pytestmark = pytest.mark.gpu

W, H = 480, 270
BASE = {"hit_log": 1, "mono_copies": 1}


def _stats(sts):
    return [(int(st.root_count), int(st.exit_count), int(st.pixel_hits)) for st in sts]


def _both(program, **opts):
    """program(hb) -> (list of (image, landed), list of stats tuples); run with close_direct 1 and 0.  Returns the direct run's close count and images."""
    from ice_halo_sim_amd.backend import HipTraceBackend
    out = {}
    for direct in (1, 0):
        hb = HipTraceBackend(device=0, seed=23, close_direct=direct, **{**BASE, **opts})
        imgs, sts = program(hb)
        out[direct] = (imgs, sts, hb.direct_closes(), hb.last_route().accum_mask)
        hb.close()
    (imgs1, sts1, closes1, mask1), (imgs0, sts0, closes0, mask0) = out[1], out[0]
    assert closes0 == 0, closes0
    assert sts1 == sts0, (sts1, sts0)
    assert mask1 == mask0, (mask1, mask0)   # the route info does not tell the two apart: halo_direct_closes does
    assert len(imgs1) == len(imgs0) > 0
    for (a, la), (b, lb) in zip(imgs1, imgs0):
        assert b.max() > 0 and la > 0
        assert la == pytest.approx(lb, rel=1e-12)
        assert a.sum(dtype=np.float64) == pytest.approx(b.sum(dtype=np.float64), rel=2e-6)
        assert np.abs(a - b).max() <= 2e-5 * float(b.max())
    return closes1, [a for a, _ in imgs1], mask1


def _sessions(hb, sc, rd, wls, n):
    sts = []
    for wl in wls:
        sts += _stats(run_session(hb, sc, rd, scenes.wl_discrete(wl), n))
    return sts


def test_six_sessions_alternating_two_wavelengths_all_close_directly():
    sc, rd = scenes.config2_scene(), scenes.config2_render(W, H)

    def program(hb):
        sts = _sessions(hb, sc, rd, [450.0, 610.0] * 3, 1 << 18)
        return [hb.ReadbackXyzAccum(W, H)], sts

    closes, (img,), mask = _both(program)
    assert closes == 6 and mask == abi.ACCUM_LOG
    # both colours are there (a close with the wrong CMF would tint everything one way)
    assert img[..., 2].sum() > 0.2 * img[..., 1].sum() and img[..., 0].sum() > 0.2 * img[..., 1].sum()


def test_auto_mode_takes_launches_that_fill_the_chip_and_leaves_small_ones():
    """close_direct = -1: a launch that alternates between the two trace streams (<= 2^alt_log2 rays) keeps the fold it starts its successor
    under; one above that size closes directly.  alt_log2 = 17 puts the 2^18-ray launches of this test on the chip-filling side."""
    from ice_halo_sim_amd.backend import HipTraceBackend
    sc, rd = scenes.config2_scene(), scenes.config2_render(W, H)
    res = {}
    for name, opts in (("small", {}), ("filling", {"alt_log2": 17}), ("never", {"alt_log2": 17, "close_direct": 0})):
        hb = HipTraceBackend(device=0, seed=23, **{**BASE, **opts})
        sts = _sessions(hb, sc, rd, [450.0, 610.0, 450.0, 610.0], 1 << 18)
        res[name] = (sts, hb.ReadbackXyzAccum(W, H), hb.direct_closes())
        hb.close()
    assert res["small"][2] == 0 and res["filling"][2] == 4 and res["never"][2] == 0
    (a, la), (b, lb) = res["filling"][1], res["never"][1]
    assert res["filling"][0] == res["never"][0] == res["small"][0]
    assert la == pytest.approx(lb, rel=1e-12)
    assert a.sum(dtype=np.float64) == pytest.approx(b.sum(dtype=np.float64), rel=2e-6)
    assert np.abs(a - b).max() <= 2e-5 * float(b.max())


def test_queued_sessions_on_a_bound_tensor_with_the_fold_deferred():
    """async = 1, the caller's tensor, defer_fold: nothing waits on the host until the one flush at the end.  The direct closes write the tensor
    from the trace streams; the flush joins them as it joins the auxiliary stream's folds."""
    import torch
    sc, rd = scenes.config2_scene(), scenes.config2_render(W, H)

    def program(hb):
        ext = torch.zeros(W * H * 3 + 4, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        hb.bind_accumulator(ext.data_ptr(), ext.numel())
        hb.collect_stats()
        for wl, n in ((450.0, 1 << 18), (610.0, 1 << 20), (610.0, 1 << 18), (450.0, 1 << 19), (530.0, 1 << 18)):
            run_session(hb, sc, rd, scenes.wl_discrete(wl), n)
        hb.flush()
        st = hb.collect_stats()
        hb.sync()
        torch.cuda.synchronize()
        img = ext[: W * H * 3].reshape(H, W, 3).cpu().numpy().copy()
        assert not ext[W * H * 3:].any().item()
        landed = hb.take_landed()
        hb.bind_accumulator(0, 0)
        return [(img, landed)], _stats([st])

    closes, _, _ = _both(program, **{"async": 1, "defer_fold": 1})
    assert closes == 5


def test_own_accumulator_under_lazy_fold_with_a_readback_in_the_middle():
    """equal sessions on the backend's own image: without the direct close their planes add up and fold once per readback; with it every session
    closes itself and the readers find nothing pending"""
    sc, rd = scenes.config2_scene(), scenes.config2_render(W, H)

    def program(hb):
        sts = _sessions(hb, sc, rd, [550.0, 550.0], 1 << 18)
        imgs = [hb.ReadbackXyzAccum(W, H)]
        sts += _sessions(hb, sc, rd, [550.0, 550.0, 480.0], 1 << 18)
        imgs.append(hb.ReadbackXyzAccum(W, H))
        return imgs, sts

    closes, _, _ = _both(program, lazy_fold=1)
    assert closes == 5


def test_log_regions_and_tile_lists_that_overflow_into_the_twin():
    """hit_log_cap = 2048: most records find their region or their tile list full and go to the fp64 twin, which the closing pass takes in and
    zeroes, session after session, on the twin half it shares with its successor"""
    sc, rd = scenes.config2_scene(), scenes.config2_render(W, H)

    def program(hb):
        sts = _sessions(hb, sc, rd, [450.0, 610.0, 610.0, 450.0], 1 << 18)
        return [hb.ReadbackXyzAccum(W, H)], sts

    closes, _, _ = _both(program, hit_log_cap=2048)
    assert closes == 4


def test_a_direct_session_then_a_small_unlogged_one_of_the_same_wavelength():
    """the second session adds to the plane with atomics and leaves it for the fold: the image holds the direct close's light and the fold's"""
    sc, rd = scenes.config2_scene(), scenes.config2_render(W, H)

    def program(hb):
        sts = _sessions(hb, sc, rd, [550.0], 1 << 19)
        hb.set_option("hit_log", 0)
        sts += _sessions(hb, sc, rd, [550.0], 1 << 16)
        return [hb.ReadbackXyzAccum(W, H)], sts

    closes, _, _ = _both(program)
    assert closes == 1


def _two_entry_scene():
    plate = scenes.entry(scenes.prism_crystal(0.3), scenes.axis(zenith={"type": "gauss", "mean": 0, "std": 0.8}), 1.0, 6)
    return scenes.scene([(0.0, [scenes.column_crystal_entry(), plate])], max_hits=7)


@pytest.mark.parametrize("case", ["two_entries", "chunked", "deterministic", "full_sky"])
def test_launches_that_are_not_their_whole_session_keep_the_fold(case):
    sc, rd, opts = scenes.config2_scene(), scenes.config2_render(W, H), {}
    if case == "two_entries":
        sc = _two_entry_scene()
    elif case == "chunked":
        opts = {"chunk": 1 << 17}
    elif case == "deterministic":
        opts = {"deterministic": 1}
    else:
        rd = scenes.render(abi.LENS_RECTANGULAR, 512, 256, fov=360.0, el=0.0, visible=abi.VISIBLE_FULL)

    def program(hb):
        sts = _sessions(hb, sc, rd, [450.0, 610.0], 1 << 18)
        return [hb.ReadbackXyzAccum(rd.width, rd.height)], sts

    closes, _, mask = _both(program, **opts)
    assert closes == 0
    assert mask == (abi.ACCUM_FIXED_LOG if case == "deterministic" else abi.ACCUM_LOG)


def test_two_layer_scene_whose_last_layer_closes_directly():
    """a plate layer whose every exit continues (the no-accumulation kernels: nothing on the planes) over a column layer of one launch; canonical
    continuation order, so that both runs trace the same rays on the second layer too"""
    sc, rd = scenes.config3_scene(), scenes.config2_render(W, H)

    def program(hb):
        sts = _sessions(hb, sc, rd, [450.0, 610.0], 1 << 18)
        return [hb.ReadbackXyzAccum(W, H)], sts

    closes, _, mask = _both(program, cont_order=1)
    assert closes == 2 and mask == abi.ACCUM_NONE | abi.ACCUM_LOG
