"""halo_consumer_auto_ev — the reference GUI's P99-anchored auto EV as a device-side consumer stage — against the float32 model of the reference's
own functions (tests/_ev_auto_model.py, itself held to the reference's header by tests/test_ev_auto_model.py).

Images are fed exactly: halo_consumer_consume from a reset consumer makes `sum` the image and `comp` zero.  Every case compares p99_y and the
per-pixel intensity BIT FOR BIT, value_count, coarse_w / coarse_h and produced exactly, against the model applied to the image that
Snapshot(want_xyz=True) hands out; the EV to 1e-6 absolute (powf / log2f of two libms, each under one ulp; one float ulp at |ev| <= 6 is 4.8e-7)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from ice_halo_sim_amd import abi, scenes
from tests import _ev_auto_model as M
from tests._oracle_backend import run_session

pytestmark = pytest.mark.gpu
F32 = np.float32
EV_TOL = 1e-6
HERE = os.path.dirname(os.path.abspath(__file__))
_BACKENDS = {}


def hip_backend(**kw):
    from ice_halo_sim_amd.backend import HipTraceBackend
    return HipTraceBackend(device=0, **kw)


@pytest.fixture(scope="module", autouse=True)
def _close_backends():
    yield
    for hb in _BACKENDS.values():
        hb.close()
    _BACKENDS.clear()


def backend_for(w, h):
    """One handle per image size (a consumer keeps the size of its first image)."""
    if (w, h) not in _BACKENDS:
        _BACKENDS[(w, h)] = hip_backend(seed=3)
    return _BACKENDS[(w, h)]


def feed(y, landed=1.0, more=()):
    """A reset consumer that has consumed Y plane `y` (X and Z carry other numbers: only channel 1 may be read) with landed weight `landed`, then
    every (y, landed) of `more`."""
    y = np.asarray(y, F32)
    h, w = y.shape
    hb = backend_for(w, h)
    hb.ResetConsumer()
    for yy, ll in [(y, landed)] + list(more):
        xyz = np.empty((h, w, 3), F32)
        xyz[..., 0], xyz[..., 1], xyz[..., 2] = 3.0, np.asarray(yy, F32), -2.0
        hb.Consume(xyz, ll)
    return hb


def check(hb, f, tw=135.0):
    """AutoEv(f, tw) against the model on the snapshot's own Y.  Returns (result dict, model p99, Y)."""
    a = hb.AutoEv(f, tw)
    _, xyz, total = hb.Snapshot(want_xyz=True)
    y = xyz[..., 1]
    p, n, wc, hc = M.p99_y(y, f)
    pp = M.per_pixel_intensity(total, y.size)
    print("f=%d %dx%d: p99 %r (model %r), count %d (model %d), grid %dx%d, per-pixel %r, ev %r (model %r)"
          % (f, y.shape[1], y.shape[0], a["p99_y"], float(p), a["value_count"], n, a["coarse_w"], a["coarse_h"], a["per_pixel_intensity"], a["ev_auto"],
             float(M.ev_auto(p, pp, tw))))
    assert M.bits(a["p99_y"]) == M.bits(p)
    assert a["value_count"] == n and (a["coarse_w"], a["coarse_h"]) == (wc, hc)
    assert M.bits(a["per_pixel_intensity"]) == M.bits(pp)
    assert a["produced"] == bool(p > 0 and pp > 0)
    assert abs(a["ev_auto"] - float(M.ev_auto(p, pp, tw))) <= EV_TOL
    if not a["produced"]:
        assert a["ev_auto"] == 0.0
    return a, p, y


def strip(vals, width=772, fill=0.0, seed=1):
    """`vals` scattered over a 16-pixel-high strip (16 x width >= len(vals)), `fill` elsewhere — positions from the integer recipe's hash."""
    vals = np.asarray(vals, F32)
    n = 16 * width
    assert vals.size <= n
    order = np.argsort(M._mix(np.arange(n), seed, 0), kind="stable")
    y = np.full(n, fill, F32)
    y[order[:vals.size]] = vals
    return y.reshape(16, width)


# ---- 1, 2: the dropped strip -----------------------------------------------------------------------------------------------------------------------
def test_positives_only_in_the_dropped_strip_give_no_data_and_no_fine_fallback():
    y = np.zeros((13, 19), F32)     # f = 8: 2 x 1 bins; columns 16..18 and rows 8..12 fill no bin
    y[:, 16:] = 2.0
    y[8:, :] = 3.0
    a, p, _ = check(feed(y), 8)
    assert (a["p99_y"], a["produced"], a["value_count"], a["coarse_w"], a["coarse_h"], a["ev_auto"]) == (0.0, False, 0, 2, 1, 0.0)
    assert check(feed(y), 1)[0]["p99_y"] == 3.0      # the fine path does see them


def test_trailing_rows_and_columns_stay_dropped():
    y = M.recipe_image(19, 13, 11, 1.0, 0.0, -2, 0)
    y[:, 16:] *= 1000.0
    y[8:, :] *= 1000.0              # were they read, every bin sum would show it
    a, p, _ = check(feed(y), 8)
    assert a["value_count"] == 2 and a["p99_y"] < 4.0


# ---- 3, 4: the fine path ---------------------------------------------------------------------------------------------------------------------------
def test_collapsed_grid_takes_the_fine_path():
    a, _, _ = check(feed(M.recipe_image(7, 20, 12, 0.5, 0.2, -3, 1)), 8)     # 7 / 8 = 0 columns
    assert (a["coarse_w"], a["coarse_h"]) == (0, 0) and a["value_count"] > 0
    a, _, _ = check(feed(np.full((1, 1), 7.5, F32)), 8)
    assert a["p99_y"] == 7.5 and a["value_count"] == 1


@pytest.mark.parametrize("f", [1, 0, -3])
def test_fine_path_by_request(f):
    a, _, _ = check(feed(M.recipe_image(33, 17, 13, 0.5, 0.2, -3, 1)), f)
    assert (a["coarse_w"], a["coarse_h"]) == (0, 0) and a["value_count"] > 100


# ---- 5, 6: no data -----------------------------------------------------------------------------------------------------------------------------------
def test_all_zeros():
    a, _, _ = check(feed(np.zeros((8, 8), F32)), 8)
    assert (a["p99_y"], a["produced"], a["ev_auto"], a["value_count"], a["coarse_w"], a["coarse_h"]) == (0.0, False, 0.0, 0, 1, 1)


def test_no_landed_intensity_reports_the_p99_and_no_ev():
    a, _, _ = check(feed(np.full((8, 8), 0.5, F32), landed=0.0), 8)
    assert a["p99_y"] == 0.5 and a["per_pixel_intensity"] == 0.0 and a["ev_auto"] == 0.0 and not a["produced"]


# ---- 7: the fp32 index rule ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 100, 101, 199, 200, 12345])
def test_index_rule(n):
    """n distinct positive values k = 1..n: the order statistic at index idx is idx + 1.  idx = (size_t)((float)n * 0.99f), e.g. 99 for n = 100
    (the fp32 product rounds to 99.0), and n - 1 at most."""
    a, p, _ = check(feed(strip(np.arange(1, n + 1), seed=n)), 1)
    idx = min(int(F32(n) * F32(0.99)), n - 1)
    assert a["value_count"] == n and a["p99_y"] == float(idx + 1)


# ---- 8: ties ---------------------------------------------------------------------------------------------------------------------------------------------
def test_ties():
    v = np.concatenate([np.full(500, 1.0), np.full(495, 2.0), np.full(5, 3.0)])    # index 990 of 1000 lies inside the run of twos (500..994)
    a, _, _ = check(feed(strip(v, seed=5)), 1)
    assert a["p99_y"] == 2.0 and a["value_count"] == 1000
    a, _, _ = check(feed(strip(np.full(777, 0.625), seed=6)), 1)
    assert a["p99_y"] == 0.625 and a["value_count"] == 777
    y = np.repeat(np.repeat(np.asarray([[1.0, 1.0, 2.0], [1.0, 2.0, 2.0]], F32), 8, 0), 8, 1) / 64.0    # coarse: six bins, three levels of two
    a, _, _ = check(feed(y), 8)
    assert a["value_count"] == 6 and a["p99_y"] == 2.0 / 64.0


# ---- 9: each radix digit decides once ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["low10", "mid11", "top11"])
def test_each_digit_decides(which):
    one = 0x3F800000
    if which == "low10":
        bits = one | np.arange(1024, dtype=np.uint32)
    elif which == "mid11":
        bits = one | (np.arange(2048, dtype=np.uint32) << 10)
    else:      # sign, exponent and the two highest mantissa bits: 2^-20 .. 2^20 times 1, 1.25, 1.5, 1.75
        bits = np.asarray([((127 + e) << 23) | (q << 21) for e in range(-20, 21) for q in range(4)], np.uint32)
    v = bits.view(F32)
    a, _, _ = check(feed(strip(v, seed=9)), 1)
    want = np.sort(v)[min(int(F32(v.size) * F32(0.99)), v.size - 1)]
    assert M.bits(a["p99_y"]) == M.bits(want) and a["value_count"] == v.size


# ---- 10: negatives, zeros, a bin that sums to <= 0 ----------------------------------------------------------------------------------------------------
def test_negatives_and_zeros_are_skipped():
    y = M.recipe_image(64, 48, 14, 0.4, 0.3, -3, 1)
    assert (y < 0).sum() > 500 and (y == 0).sum() > 500
    for f in (8, 1):
        check(feed(y), f)
    y = np.zeros((8, 16), F32)
    y[0, 0], y[3, 3] = 1.0, -5.0          # bin 0 sums to -4 although a pixel in it is positive
    y[2, 9], y[7, 15] = 4.0, 6.0          # bin 1 sums to 10
    a, _, _ = check(feed(y), 8)
    assert a["value_count"] == 1 and a["p99_y"] == 10.0 / 64.0
    y[3, 3] = -1.0                        # ... and to exactly 0: still skipped
    a, _, _ = check(feed(y), 8)
    assert a["value_count"] == 1


# ---- 11: the summation order ---------------------------------------------------------------------------------------------------------------------------
def test_bins_are_summed_one_pixel_after_another():
    y = np.ones((8, 8), F32)
    y[0, 0] = 2.0 ** 24                   # then 63 ones, each absorbed: a pairwise tree would end at 2^24 + 64
    a, _, _ = check(feed(y), 8)
    assert a["p99_y"] == 2.0 ** 24 / 64.0
    y = M.recipe_image(16, 16, 15, 1.0, 0.0, -12, 12)        # magnitudes spread over 2^24 within every bin
    pairwise = y.reshape(2, 8, 2, 8).transpose(0, 2, 1, 3).reshape(2, 2, 64)
    while pairwise.shape[-1] > 1:
        pairwise = (pairwise[..., 0::2] + pairwise[..., 1::2]).astype(F32)
    assert (pairwise[..., 0] != M.box_sum_y(y, 8)).any()     # the two orders do differ on this image
    check(feed(y), 8)


# ---- 12: Y is sum + comp -------------------------------------------------------------------------------------------------------------------------------
def test_source_is_sum_plus_compensation():
    """Three consumes: a = m * 2^24, b of order 1, then -a.  The running sum keeps what survives next to 2^24 (multiples of 2), the compensation
    holds the rest: sum + comp is b again (exactly where b has few bits), sum alone is not."""
    w, h = 64, 48
    big = (np.ldexp(1.0 + (M._mix(np.arange(w * h), 16, 0) % np.uint64(3)).astype(np.float64), 24)).astype(F32).reshape(h, w)
    b = M.recipe_image(w, h, 17, 1.0, 0.0, -1, 1)
    hb = feed(big, 1.0, more=[(b, 1.0), (-big, 1.0)])
    s, c = np.zeros((h, w), F32), np.zeros((h, w), F32)      # the fold's Neumaier step (accum_shared.h:70-74), in fp32
    for d in (big, b, -big):
        ns = (s + d).astype(F32)
        c = (c + np.where(np.abs(d) < np.abs(s), ((s - ns).astype(F32) + d).astype(F32), ((d - ns).astype(F32) + s).astype(F32))).astype(F32)
        s = ns
    for f in (8, 1):
        a, p, y = check(hb, f)
        assert (y.view(np.uint32) == (s + c).astype(F32).view(np.uint32)).all() and (c != 0).sum() > 1000
        assert M.bits(M.p99_y(s, f)[0]) != M.bits(p)         # the sum alone would give another answer


# ---- 13: the clamp ---------------------------------------------------------------------------------------------------------------------------------------
def test_clamp():
    y = M.recipe_image(64, 48, 18, 0.5, 0.0, -2, 0)
    a, _, _ = check(feed(y, landed=1e6 * y.size), 8)
    assert a["ev_auto"] == 6.0 and a["produced"]
    a, _, _ = check(feed(y, landed=1e-6 * y.size), 8)
    assert a["ev_auto"] == -6.0 and a["produced"]
    a, _, _ = check(feed(y, landed=0.02 * y.size), 8)
    assert 0.0 < abs(a["ev_auto"]) < 6.0


# ---- 14: the production shape --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("density", [0.02, 1.0])
def test_full_size(density):
    """1920 x 1080: f = 8 is 32 400 values (one workgroup's select), f = 1 is 2 073 600 (the multi-block select); values in three exponents."""
    y = M.recipe_image(1920, 1080, 19, density, 0.0 if density == 1.0 else 0.1, -2, 0)
    hb = feed(y, landed=0.01 * y.size)
    for f, tw in ((8, 135.0), (1, 11.0)):
        a, _, _ = check(hb, f, tw)
        assert a["produced"] and (a["coarse_w"], a["coarse_h"]) == ((240, 135) if f == 8 else (0, 0))


# ---- every route: the select's size threshold, both selects and both histogram forms on the same values ---------------------------------------------
@pytest.mark.parametrize("w,h", [(256, 128), (32769, 1)])
def test_select_threshold(w, h):
    """32 768 values are one workgroup's, 32 769 the multi-block select's (kAevSmallMax, halo_launch.h)."""
    check(feed(M.recipe_image(w, h, 20, 0.7, 0.1, -4, 2), landed=0.01 * w * h), 1)


def test_every_route_gives_the_same_record():
    small, large = M.recipe_image(33, 17, 21, 0.6, 0.2, -3, 1), M.recipe_image(400, 300, 22, 0.6, 0.2, -3, 1)
    one = np.zeros((17, 33), F32)
    one[5, 7] = 0.375
    for y in (small, large, one, np.zeros((17, 33), F32)):
        hb = feed(y)
        got = []
        try:
            for select in (-1, 0, 1):
                for agg in (0, 1):
                    hb.set_option("auto_ev_select", select)
                    hb.set_option("auto_ev_hist", agg)
                    got.append(check(hb, 1)[0])
        finally:
            hb.set_option("auto_ev_select", -1)
            hb.set_option("auto_ev_hist", 0)
        assert all(g == got[0] for g in got)


# ---- 15, 16: a live consumer -----------------------------------------------------------------------------------------------------------------------------
def _traced():
    hb = hip_backend(seed=42)
    rd = scenes.config2_render(64, 48)
    run_session(hb, scenes.config2_scene(), rd, scenes.wl_discrete(550.0), 1 << 16)
    hb.ConsumeDeviceFused()
    return hb


def test_on_a_traced_consumer_twice_and_nothing_is_modified():
    hb = _traced()
    before = hb.Snapshot(intensity_factor=1.7)
    a, _, _ = check(hb, 8)
    b = hb.AutoEv(8)
    after = hb.Snapshot(intensity_factor=1.7)
    hb.close()
    assert a == b and a["produced"] and a["value_count"] > 0
    assert before[0].tobytes() == after[0].tobytes() and before[1].tobytes() == after[1].tobytes() and before[2] == after[2]


def test_snapshot_auto_ev_applies_the_factor():
    hb = _traced()
    plain = hb.Snapshot(intensity_factor=0.8)
    assert len(plain) == 3
    rgb, xyz, total, ev = hb.Snapshot(intensity_factor=0.8, auto_ev=True, target_white=120.0)
    a = hb.AutoEv(8, 120.0)
    by_hand = hb.Snapshot(intensity_factor=0.8 * 2.0 ** a["ev_auto"])
    hb.close()
    assert ev == a["ev_auto"] and ev != 0.0
    assert rgb.tobytes() == by_hand[0].tobytes() and xyz.tobytes() == by_hand[1].tobytes() and total == by_hand[2]
    assert rgb.tobytes() != plain[0].tobytes()


# ---- 17: the command line --------------------------------------------------------------------------------------------------------------------------------
def test_cli_auto_ev(tmp_path, capsys):
    from ice_halo_sim_amd import cli, config
    doc = json.load(open(os.path.join(HERE, "golden", "ref_e2e_configs.json")))["multi_lens"]
    doc["render"] = [dict(doc["render"][1], resolution=[64, 48])]      # the fisheye entry, id 2
    doc["scene"]["ray_num"] = 1 << 16
    cfg = tmp_path / "tiny.json"
    cfg.write_text(json.dumps(doc))
    base = ["-f", str(cfg), "--deterministic", "--seed", "7"]           # fixed-point sums: the same XYZ bytes on every run

    def run(*extra):
        out = tmp_path / ("img%d.ppm" % len(extra))
        assert cli.main(base + ["--out-rgb", str(out)] + list(extra)) == 0
        return out.read_bytes(), capsys.readouterr().out

    plain, log0 = run()
    auto, log1 = run("--auto-ev")
    auto2, log2 = run("--auto-ev", "--target-white", "60")
    assert "ev_auto" not in log0
    line = [ln for ln in log1.splitlines() if ln.startswith("ev_auto (render 2): ")]
    assert len(line) == 1 and " EV (p99_y=" in line[0] and "per_pixel_intensity=" in line[0] and line[0][len("ev_auto (render 2): ")] in "+-"
    assert auto != plain and auto2 != auto and len(auto) == len(plain)
    # without the flag the image is what the same calls gave before the flag existed; with it, the snapshot at factor x 2^ev
    job = config.load_config(str(cfg))
    res = cli.run_job(job, 2, seed=7, deterministic=True)
    be, factor = res["backend"], job.render_meta.get(2, {}).get("intensity_factor", 1.0)
    rgb = be.Snapshot(intensity_factor=factor)[0]
    ev = be.AutoEv(8, 135.0)["ev_auto"]
    rgb_auto = be.Snapshot(intensity_factor=factor * 2.0 ** ev)[0]
    be.close()
    assert plain.endswith(rgb.tobytes()) and auto.endswith(rgb_auto.tobytes())
    assert ("%+.2f EV" % ev) in line[0]
    assert cli.main(base + ["--auto-ev", "--target-white", "0"]) == 2


# ---- 18: errors ------------------------------------------------------------------------------------------------------------------------------------------
def test_errors_leave_the_handle_usable():
    from ice_halo_sim_amd.backend import BackendError
    hb = hip_backend(seed=1)
    L, out = hb._L, abi.HaloAutoEv()
    with pytest.raises(BackendError, match="before consumer_fold"):
        hb.AutoEv()
    xyz = np.zeros((8, 8, 3), F32)
    xyz[..., 1] = 0.25
    hb.Consume(xyz, 2.0)
    assert L.halo_consumer_auto_ev(hb._h, 8, 135.0, None) == abi.HALO_FATAL and b"NULL" in L.halo_last_error(hb._h)
    for tw in (0.0, 256.0, -1.0, float("nan")):
        assert L.halo_consumer_auto_ev(hb._h, 8, tw, C.byref(out)) == abi.HALO_FATAL and b"target_white" in L.halo_last_error(hb._h)
        with pytest.raises(BackendError, match="target_white"):
            hb.AutoEv(8, tw)
    a = hb.AutoEv(8, 255.0)                 # the upper end is inside
    assert a["p99_y"] == 0.25 and a["produced"] and a["value_count"] == 1
    hb.close()
