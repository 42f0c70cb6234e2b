"""halo_consumer_stats — exact percentiles and moments of the consumer's image on the device — against the float64 model
(tests/_image_stats_model.py, itself held to numpy by tests/test_image_stats_model.py).

Images are fed exactly, as tests/test_gpu_auto_ev.py feeds them: halo_consumer_consume into a reset consumer makes `sum` the image and `comp`
zero.  Truth is the model on the Y that Snapshot(want_xyz=True) hands out (or on the loaded lane).  Per case, with the reference tool's eleven
percentiles plus 0 and 100: counts and ranks are exact integers; lo, hi, max and frac are compared BIT FOR BIT; the interpolated value to
4 * 2^-52 relative (three float64 roundings on either side); sum and sum_sq must EQUAL math.fsum of the float64 values and of their float64
squares (a float32 squared is exact in float64, so both are the exact sums rounded once).  Every case runs by size and through both forms
(option stats_select: one workgroup, many workgroups), which must return the same bytes.

Sizes sit on both sides of a workgroup (1 x 1, 7 x 5 below 1024 values; 64 x 48 above), of the form threshold kStatsSmallMax = 2^13
(128 x 64 on it, 8193 x 1 over it) and of 2^15 and 2^16 (256 x 160, 300 x 219: more than one workgroup's stride, several workgroups)."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest

from ice_halo_sim_amd import abi, scenes
from tests import _image_stats_model as M

pytestmark = pytest.mark.gpu
F32 = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
SIZES = [(1, 1), (7, 5), (64, 48), (128, 64), (8193, 1), (256, 160), (300, 219)]
SOME_SIZES = [(7, 5), (64, 48), (300, 219)]
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
    y = np.asarray(y, F32)
    h, w = y.shape
    hb = backend_for(w, h)
    hb.ResetConsumer()
    for yy, ll in [(y, landed)] + list(more):
        xyz = np.empty((h, w, 3), F32)
        xyz[..., 0], xyz[..., 1], xyz[..., 2] = 3.0, np.asarray(yy, F32), -2.0       # X and Z carry other numbers: only channel 1 may be read
        hb.Consume(xyz, ll)
    return hb


def raw(hb, pcts, plane=None, norm=None):
    """The struct itself, by the C entry point."""
    spec, r = abi.HaloStatsSpec(), abi.HaloImageStats()
    spec.plane = abi.STATS_PLANE_Y if plane is None else plane
    spec.percentile_count = len(pcts)
    for j, p in enumerate(pcts):
        spec.percentiles[j] = p
    spec.norm = 0.0 if norm is None else norm
    assert hb._L.halo_consumer_stats(hb._h, C.byref(spec), C.byref(r)) == abi.HALO_OK, hb._L.halo_last_error(hb._h)
    return r


def same(a, b):
    return a == b or (isinstance(a, float) and isinstance(b, float) and math.isnan(a) and math.isnan(b))


def check(hb, pcts=M.THIRTEEN, norm=None, plane=None, truth=None):
    """ImageStats against the model on the snapshot's own Y (or on `truth`), by size and through both forms.  Returns (result, model)."""
    got = []
    try:
        for select in (-1, 0, 1):
            hb.set_option("stats_select", select)
            got.append((hb.ImageStats(pcts, plane=plane, norm=norm), bytes(raw(hb, pcts, plane, norm))))
    finally:
        hb.set_option("stats_select", -1)
    assert got[0][1] == got[1][1] == got[2][1], "the two forms differ"
    s = got[0][0]
    y = hb.Snapshot(want_xyz=True)[1][..., 1] if truth is None else truth
    m = M.stats(y, pcts, s["norm"])
    print("%s, %d percentiles: n %d (model %d), saturated %s (%s), sum %r (%r), sum_sq %r (%r), max %r (%r)"
          % (y.shape, len(pcts), s["positive_count"], m["positive_count"], s["saturated_count"], m.get("saturated_count"), s["sum"], m.get("sum"),
             s["sum_sq"], m.get("sum_sq"), s["max_raw"], m.get("max")))
    assert s["pixel_count"] == m["pixel_count"] and s["positive_count"] == m["positive_count"] and s["produced"] == m["produced"]
    if not m["produced"]:
        assert (s["saturated_count"], s["sum"], s["sum_sq"], s["max_raw"]) == (0, 0.0, 0.0, 0.0)
        assert s["rank"] == [0] * len(pcts) and s["lo"] == s["hi"] == s["value"] == s["frac"] == [0.0] * len(pcts)
        return s, m
    assert s["saturated_count"] == m["saturated_count"]
    assert M.bits32(s["max_raw"]) == M.bits32(m["max"])
    assert s["sum"] == m["sum"] and s["sum_sq"] == m["sum_sq"]
    assert s["rank"] == m["rank"]
    for j, q in enumerate(pcts):
        print("  p%-6g rank %d frac %r lo %r hi %r value %r (model %r)" % (q, s["rank"][j], s["frac"][j], s["lo"][j], s["hi"][j], s["value"][j], m["value"][j]))
        assert M.bits32(s["lo"][j]) == M.bits32(m["lo"][j]) and M.bits32(s["hi"][j]) == M.bits32(m["hi"][j])
        assert M.bits64(s["frac"][j]) == M.bits64(m["frac"][j])
        v, w = s["value"][j], m["value"][j]
        assert same(v, w) or abs(v - w) <= M.VALUE_RTOL * abs(w)
    return s, m


def lognormal(w, h, seed=1, sigma=4.0):
    return np.exp(np.random.default_rng(seed).normal(0.0, sigma, (h, w))).astype(F32)


def narrow(w, h, seed=2):
    """All of it in [1, 1 + 2^-13): one first-digit bin, one second-digit bin, the ranks part in the last ten bits."""
    return (np.uint32(0x3F800000) | np.random.default_rng(seed).integers(0, 1024, (h, w), dtype=np.uint32)).view(F32)


def holes(w, h, seed=3):
    """Log-normal with three pixels in ten zero and two in ten negative."""
    rng = np.random.default_rng(seed)
    y, u = lognormal(w, h, seed), rng.random((h, w))
    y[u < 0.3] = 0.0
    y[(u >= 0.3) & (u < 0.5)] *= F32(-1.0)
    return y


def extremes(w, h):
    """A denormal, 1e-30, 1.0 and 1e30 in turn: exponent bins at both ends, 1e60 among the squares."""
    return np.resize(np.asarray([1e-45, 1e-30, 1.0, 1e30], F32), h * w).reshape(h, w)


# ---- the images ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", SIZES)
def test_lognormal(w, h):
    """sigma = 4: the ranks spread over more than a dozen first-digit bins."""
    s, _ = check(feed(lognormal(w, h, seed=w), landed=0.5 * w * h), norm=5.0)
    if w * h >= 3072:
        assert len({M.bits32(v) >> 21 for v in s["lo"]}) >= 10 and 0 < s["saturated_count"] < s["positive_count"]


@pytest.mark.parametrize("w,h", SIZES)
def test_narrow_band(w, h):
    s, _ = check(feed(narrow(w, h)), norm=1.00003)
    assert len({M.bits32(v) >> 10 for v in s["lo"]}) == 1


@pytest.mark.parametrize("w,h", SOME_SIZES)
def test_one_value_everywhere(w, h):
    s, _ = check(feed(np.full((h, w), 0.625, F32)), norm=0.5)
    assert s["lo"] == s["hi"] == s["value"] == [0.625] * 13 and s["saturated_count"] == w * h and s["sum"] == 0.625 * w * h


@pytest.mark.parametrize("w,h", SOME_SIZES)
def test_one_positive_pixel(w, h):
    y = np.zeros((h, w), F32)
    y[h // 2, w // 3] = 0.375
    s, _ = check(feed(y), norm=1.0)
    assert s["positive_count"] == 1 and s["rank"] == [0] * 13 and s["value"] == [0.375] * 13 and s["sum_sq"] == 0.375 ** 2


@pytest.mark.parametrize("w,h", SOME_SIZES)
def test_no_positive_pixel(w, h):
    y = np.zeros((h, w), F32)
    y[::2] = -1.5
    s, _ = check(feed(y), norm=1.0)
    assert not s["produced"] and s["positive_count"] == 0 and s["pixel_count"] == w * h and s["norm"] == 1.0
    assert s["percentiles"] == [0.0] * 13 and s["mean"] == s["std"] == s["max"] == s["saturation_rate"] == 0.0


@pytest.mark.parametrize("w,h", SOME_SIZES)
def test_both_ends_of_the_exponent_range(w, h):
    s, m = check(feed(extremes(w, h)), norm=1.0)
    assert s["sum_sq"] > 1e59 and M.bits32(s["lo"][0]) == 1


@pytest.mark.parametrize("w,h", SOME_SIZES)
def test_zeros_and_negatives_among_the_positives(w, h):
    y = holes(w, h)
    s, _ = check(feed(y), norm=2.0)
    assert s["positive_count"] == int((y > 0).sum()) < w * h


def test_source_is_sum_plus_compensation():
    """Three consumes, as in tests/test_gpu_auto_ev.py: a = m * 2^24, b of order 1, then -a.  sum + comp is b again, sum alone is not."""
    w, h = 64, 48
    rng = np.random.default_rng(16)
    big = np.ldexp(1.0 + rng.integers(0, 3, (h, w)), 24).astype(F32)
    b = np.ldexp(rng.integers(1, 1 << 12, (h, w)).astype(np.float64), -12).astype(F32)
    hb = feed(big, 1.0, more=[(b, 1.0), (-big, 1.0)])
    s, _ = check(hb, norm=0.5)
    y = hb.Snapshot(want_xyz=True)[1][..., 1]
    assert (y == b).all() and s["sum"] == math.fsum(b.astype(np.float64).ravel())


# ---- the wrapper's normalised view -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,w,h", [("lognormal", 300, 219), ("holes", 64, 48), ("narrow-wide", 256, 160)])
def test_std_from_the_exact_sums(name, w, h):
    """Population std from sum and sum_sq (one pass: var = E[v^2] - mean^2) against numpy's two-pass float64 std.  The one-pass formula cancels:
    its relative error is bounded by 8 * 2^-53 * (1 + mean^2 / var).  Images with cv >= 0.1."""
    y = {"lognormal": lognormal(w, h, 7, 1.0), "holes": holes(w, h, 8),
         "narrow-wide": (narrow(w, h, 9).astype(np.float64) * np.random.default_rng(9).choice([1.0, 2.0], (h, w))).astype(F32)}[name]
    s = feed(y).ImageStats(norm=1.0)
    p = y[y > 0].astype(np.float64)
    mean, std = float(np.mean(p)), float(np.std(p))
    assert std / mean >= 0.1
    bound = 8.0 * 2.0 ** -53 * (1.0 + mean * mean / (std * std))
    print("%s: std %r (numpy %r), relative difference %.3g, bound %.3g" % (name, s["std"], std, abs(s["std"] - std) / std, bound))
    assert abs(s["std"] - std) <= bound * std
    assert s["mean"] == math.fsum(p) / p.size and abs(s["mean"] - mean) <= 1e-14 * mean and abs(s["cv"] - std / mean) <= 2.0 * bound * std / mean
    assert s["max"] == float(p.max()) and s["non_zero_count"] == p.size and s["saturation_rate"] == float((p.astype(F32) > 1).sum()) / p.size


def test_normalised_view_divides_by_the_norm():
    hb = feed(lognormal(64, 48, 11, 1.0), landed=0.02 * 64 * 48)
    a, b = hb.ImageStats(norm=1.0), hb.ImageStats(norm=4.0)
    assert b["percentiles"] == [v / 4.0 for v in a["percentiles"]] and b["mean"] == a["mean"] / 4.0 and b["max"] == a["max"] / 4.0
    assert b["cv"] == a["cv"] and b["value"] == a["value"] and b["saturated_count"] < a["saturated_count"]


# ---- percentile lists ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pcts", [(), tuple(100.0 * k / 15 for k in range(16)), (99.0, 99.0, 50.0, 99.0, 0.0, 50.0), (99.99, 0.0, 50.0, 100.0, 12.5, 99.0)],
                         ids=["empty", "sixteen", "repeated", "unsorted"])
def test_percentile_lists(pcts):
    for w, h in ((64, 48), (300, 219)):
        s, m = check(feed(lognormal(w, h, 12)), pcts=pcts, norm=1.0)
        assert len(s["value"]) == len(pcts) and s["positive_count"] == w * h and s["sum"] == m["sum"]
    with pytest.raises(ValueError):
        feed(lognormal(7, 5, 12)).ImageStats(percentiles=range(17))


# ---- the divisor -------------------------------------------------------------------------------------------------------------------------------------
def test_default_norm_is_the_per_pixel_intensity():
    y = lognormal(64, 48, 13, 1.0)
    hb = feed(y, landed=0.3 * y.size)
    s, _ = check(hb)
    pp = hb.AutoEv(1)["per_pixel_intensity"]
    assert M.bits32(s["norm"]) == M.bits32(pp) and pp > 0
    t, _ = check(hb, norm=1.0)
    assert t["saturated_count"] == int((y > 1.0).sum()) != s["saturated_count"] and t["value"] == s["value"] and t["norm"] == 1.0
    hb = feed(y, landed=0.0)                  # no landed intensity to divide by: nothing produced
    z = hb.ImageStats()
    assert not z["produced"] and z["norm"] == 0.0 and z["positive_count"] == 0 and z["pixel_count"] == y.size
    assert hb.ImageStats(norm=2.0)["produced"]


# ---- class lanes, and +inf ----------------------------------------------------------------------------------------------------------------------------
def test_class_lanes_and_infinity():
    from ice_halo_sim_amd.backend import BackendError
    w, h = 150, 113           # 16 950 values: the multi-block form by size
    lanes = np.stack([holes(w, h, 14), lognormal(w, h, 15, 2.0)])
    lanes[1, 5, 7] = np.inf
    lanes[1, 6, 7] = np.nan
    hb = hip_backend(seed=1)
    with pytest.raises(BackendError, match="class lane"):
        hb.ImageStats(plane=0)               # no lanes yet
    hb.set_color([], [scenes.color_class([i]) for i in range(2)])
    hb.LoadClassLanes(lanes, 0.1 * w * h)
    s0, _ = check(hb, plane=0, truth=lanes[0])
    s1, m1 = check(hb, plane=1, truth=lanes[1], norm=3.0)
    assert s1["max_raw"] == math.inf and s1["sum"] == math.inf and s1["sum_sq"] == math.inf and s1["hi"][-1] == math.inf
    assert s1["positive_count"] == w * h - 1 and math.isfinite(s1["lo"][-2]) and s0["max_raw"] < math.inf
    with pytest.raises(BackendError, match="class lane"):
        hb.ImageStats(plane=2)
    with pytest.raises(BackendError, match="before consumer_fold"):
        hb.ImageStats()                      # lanes alone are no image
    hb.close()


# ---- reproducible, read-only --------------------------------------------------------------------------------------------------------------------------
def test_twice_the_same_bytes_and_nothing_is_modified():
    y = holes(300, 219, 17)
    hb = feed(y, landed=0.05 * y.size)
    before, ev0 = hb.Snapshot(intensity_factor=1.7), hb.AutoEv(8)
    a = bytes(raw(hb, M.THIRTEEN))
    b = bytes(raw(hb, M.THIRTEEN))
    after, ev1 = hb.Snapshot(intensity_factor=1.7), hb.AutoEv(8)
    assert a == b and ev0 == ev1 and ev0["produced"]
    assert before[0].tobytes() == after[0].tobytes() and before[1].tobytes() == after[1].tobytes() and before[2] == after[2]


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_usable():
    from ice_halo_sim_amd.backend import BackendError
    hb = hip_backend(seed=1)
    L, spec, out = hb._L, abi.HaloStatsSpec(), abi.HaloImageStats()
    spec.plane, spec.percentile_count, spec.norm = abi.STATS_PLANE_Y, 1, 1.0
    spec.percentiles[0] = 50.0
    with pytest.raises(BackendError, match="before consumer_fold"):
        hb.ImageStats()
    xyz = np.zeros((8, 8, 3), F32)
    xyz[..., 1] = 0.25
    hb.Consume(xyz, 2.0)
    assert L.halo_consumer_stats(hb._h, None, C.byref(out)) == abi.HALO_FATAL and b"NULL" in L.halo_last_error(hb._h)
    assert L.halo_consumer_stats(hb._h, C.byref(spec), None) == abi.HALO_FATAL and b"NULL" in L.halo_last_error(hb._h)
    for bad in (-0.5, 100.5, float("nan"), float("inf")):
        spec.percentiles[0] = bad
        assert L.halo_consumer_stats(hb._h, C.byref(spec), C.byref(out)) == abi.HALO_FATAL and b"[0, 100]" in L.halo_last_error(hb._h)
        with pytest.raises(BackendError, match="percentile"):
            hb.ImageStats(percentiles=(50.0, bad))
    spec.percentiles[0] = 50.0
    for cnt in (-1, 17):
        spec.percentile_count = cnt
        assert L.halo_consumer_stats(hb._h, C.byref(spec), C.byref(out)) == abi.HALO_FATAL and b"percentile_count" in L.halo_last_error(hb._h)
    spec.percentile_count, spec.plane = 1, -2
    assert L.halo_consumer_stats(hb._h, C.byref(spec), C.byref(out)) == abi.HALO_FATAL and b"plane" in L.halo_last_error(hb._h)
    with pytest.raises(BackendError, match="class lane"):
        hb.ImageStats(plane=0)
    s = hb.ImageStats((0.0, 100.0), norm=1.0)          # both ends are inside
    assert s["value"] == [0.25, 0.25] and s["positive_count"] == 64 and s["produced"]
    hb.close()


# ---- the command line -----------------------------------------------------------------------------------------------------------------------------------
def test_cli_stats(tmp_path):
    from ice_halo_sim_amd import cli, config
    doc = json.load(open(os.path.join(HERE, "golden", "ref_e2e_configs.json")))["multi_lens"]
    doc["render"] = [dict(doc["render"][1], resolution=[128, 96])]      # the fisheye entry, id 2
    doc["scene"]["ray_num"] = 1 << 18
    cfg = tmp_path / "tiny.json"
    cfg.write_text(json.dumps(doc))
    base = ["-f", str(cfg), "--deterministic", "--seed", "7"]           # fixed-point sums: the same image on every run
    assert cli.main(base + ["--stats", str(tmp_path / "a.json")]) == 0
    assert cli.main(base + ["--auto-ev", "--stats", str(tmp_path / "b.json")]) == 0
    a, b = json.load(open(tmp_path / "a.json")), json.load(open(tmp_path / "b.json"))
    assert a == b                                                       # the exposure does not touch what is described
    assert list(a) == ["scene", "config", "pixel_count", "non_zero_count", "percentiles", "mean", "std", "cv", "max", "saturation_rate"]
    assert list(a["percentiles"]) == ["p50", "p70", "p90", "p95", "p99", "p99_3", "p99_5", "p99_7", "p99_9", "p99_95", "p99_99"]
    assert a["scene"] == "tiny" and a["config"] == str(cfg) and a["pixel_count"] == 128 * 96 and 0 < a["non_zero_count"] <= 128 * 96
    job = config.load_config(str(cfg))
    be = cli.run_job(job, 2, seed=7, deterministic=True)["backend"]
    s = be.ImageStats()
    y = be.Snapshot(want_xyz=True)[1][..., 1]
    be.close()
    assert a["percentiles"] == dict(zip(abi.STATS_TOOL_KEYS, s["percentiles"])) and a["non_zero_count"] == s["non_zero_count"] == int((y > 0).sum())
    assert (a["mean"], a["std"], a["cv"], a["max"], a["saturation_rate"]) == (s["mean"], s["std"], s["cv"], s["max"], s["saturation_rate"])
    vals = list(a["percentiles"].values())
    assert vals == sorted(vals) and 0 < vals[0] and vals[-1] <= a["max"]
    assert cli.main(base + ["-o", str(tmp_path), "--stats", str(tmp_path / "c.json")]) == 2
