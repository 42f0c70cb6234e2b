"""The image-statistics model (tests/_image_stats_model.py) against numpy, and the host halves of halo_consumer_stats against the model.  No GPU.

Tolerances.  The interpolated value is lo + (hi - lo) * frac in float64, the same three roundings numpy makes (for frac >= 0.5 numpy evaluates
hi - (hi - lo) * (1 - frac), three roundings of the same size): the two agree to 4 * 2^-52 relative.  halo_host_percentile_rank is the model's
own expression — one division, one product, one floor, one subtraction, all IEEE — so it is compared bit for bit; halo_host_binned_sum is an
exact sum rounded once, so it equals float(Fraction) of the same integers."""
import ctypes as C
import math
import random

import numpy as np
import pytest

from ice_halo_sim_amd import abi, backend
from tests import _image_stats_model as M

F32 = np.float32


def host_rank(q, n):
    L, r, f = backend.load_library(), C.c_uint64(), C.c_double()
    assert L.halo_host_percentile_rank(float(q), int(n), C.byref(r), C.byref(f)) == abi.HALO_OK
    return r.value, f.value


def host_sum(bins, squares):
    L, out = backend.load_library(), C.c_double()
    arr = (C.c_uint64 * len(bins))(*bins)
    assert L.halo_host_binned_sum(arr, 1 if squares else 0, C.byref(out)) == abi.HALO_OK
    return out.value


@pytest.mark.parametrize("n", [1, 2, 3, 7, 100, 101, 4097, 65700, 2073600])
def test_model_value_agrees_with_numpy(n):
    rng = np.random.default_rng(n)
    y = np.exp(rng.normal(0.0, 4.0, n)).astype(F32)
    s = M.stats(y, M.THIRTEEN)
    want = np.percentile(y.astype(np.float64), M.THIRTEEN)
    worst = 0.0
    for v, w in zip(s["value"], want):
        worst = max(worst, abs(v - w) / abs(w))
    print("n = %d: worst relative difference to np.percentile %.3g (bar %.3g)" % (n, worst, M.VALUE_RTOL))
    assert worst <= M.VALUE_RTOL
    assert s["positive_count"] == n and s["max"] == float(y.max())
    assert s["sum"] == math.fsum(y.astype(np.float64))


@pytest.mark.parametrize("n", [1, 2, 3, 7, 100, 101, 1 << 25])
def test_host_rank_is_the_model_bit_for_bit(n):
    qs = list(M.THIRTEEN)
    for k in (1, n // 3, n // 2, n - 2):          # percentiles whose product lands on an integer rank, and their float64 neighbours
        if 0 < k < n - 1:
            q = 100.0 * k / (n - 1)
            qs += [q, math.nextafter(q, 0.0), math.nextafter(q, 100.0)]
    if n == 101:
        qs += [50.0, math.nextafter(50.0, 0.0), math.nextafter(50.0, 100.0)]
        assert M.rank_rule(50.0, 101) == (50, 0.0)
    for q in qs:
        r, f = host_rank(q, n)
        mr, mf = M.rank_rule(q, n)
        assert r == mr and M.bits64(f) == M.bits64(mf), (q, n, r, f, mr, mf)
        assert 0 <= r <= n - 1 and 0.0 <= f < 1.0


def test_host_rank_refusals():
    L, r, f = backend.load_library(), C.c_uint64(), C.c_double()
    for q, n in ((-0.001, 10), (100.001, 10), (float("nan"), 10), (50.0, 0)):
        assert L.halo_host_percentile_rank(q, n, C.byref(r), C.byref(f)) == abi.HALO_FATAL
    assert L.halo_host_percentile_rank(50.0, 10, None, C.byref(f)) == abi.HALO_FATAL
    assert L.halo_host_percentile_rank(50.0, 10, C.byref(r), None) == abi.HALO_FATAL


def test_binned_sum_random_bins():
    rnd = random.Random(5)
    for trial in range(40):
        bins = [0] * 512
        for _ in range(rnd.randrange(1, 40)):
            e = rnd.randrange(0, 255)
            bins[e] = rnd.randrange(1, 1 << 49)
            bins[256 + e] = rnd.randrange(0, 1 << 49)
        assert host_sum(bins[:256], False) == M.binned_float(bins[:256], False)
        assert host_sum(bins, True) == M.binned_float(bins, True)


def test_binned_sum_of_real_values():
    rng = np.random.default_rng(6)
    y = np.exp(rng.normal(0.0, 4.0, 5000)).astype(F32)
    y[:3] = [1e-45, 1e-30, 1e30]        # a denormal; 1e60 among the squares
    b = M.bins_of(y)
    y64 = y.astype(np.float64)
    assert host_sum(b[:256], False) == math.fsum(y64) == M.binned_float(b[:256], False)
    assert host_sum(b[256:], True) == math.fsum(y64 * y64) == M.binned_float(b[256:], True)


@pytest.mark.parametrize("k,low,up", [(6, 0, False), (7, 0, True), (6, 1, True), (7, 1, True)])
def test_binned_sum_rounds_ties_to_even(k, low, up):
    """A * 2^59 with A = 2^54 + 4 k + 2: 55 bits, the 53 kept are 2^52 + k, the guard bit is set and nothing lies below — a tie, broken to the even
    neighbour; one unit in exponent bin 1 (2^0) below it is no tie any more."""
    a = (1 << 54) | (k << 2) | 2
    bins = [0] * 256
    bins[60], bins[1] = a, low             # exponent field 60: shift 59
    kept = (1 << 52) + k + (1 if up else 0)
    want = math.ldexp(float(kept), 2 + 59 - 149)
    assert host_sum(bins, False) == want == M.binned_float(bins, False)
    sq = [0] * 512                         # the same integer in the squares' low set: exponent field 30 is shift 2 * 29 = 58
    sq[30], sq[1] = a << 1, low
    assert host_sum(sq, True) == math.ldexp(float(kept), 2 + 59 - 298) == M.binned_float(sq, True)


def test_binned_sum_edges():
    assert host_sum([0] * 256, False) == 0.0 and host_sum([0] * 512, True) == 0.0
    top = [0] * 512
    top[254], top[256 + 254] = (1 << 49) - 1, (1 << 49) - 3        # the top finite exponent, as full as 2^25 values can make it
    assert host_sum(top[:256], False) == M.binned_float(top[:256], False) > 2.0 ** 152      # 2^49 x 2^(254 - 150)
    assert host_sum(top, True) == M.binned_float(top, True) > 2.0 ** 280                    # 2^49 x 2^24 x 2^(2 x 253 - 298)
    one = [0] * 256
    one[0] = 1                                                     # the smallest denormal
    assert host_sum(one, False) == 2.0 ** -149
    inf = [0] * 512
    inf[255] = 0x800000
    assert host_sum(inf[:256], False) == math.inf
    inf = [0] * 512
    inf[256 + 255] = 1 << 22
    assert host_sum(inf, True) == math.inf
    L, out = backend.load_library(), C.c_double()
    assert L.halo_host_binned_sum(None, 0, C.byref(out)) == abi.HALO_FATAL
    assert L.halo_host_binned_sum((C.c_uint64 * 256)(), 0, None) == abi.HALO_FATAL


def test_abi_mirrors():
    L = backend.load_library()
    assert L.halo_abi_sizeof(13) == C.sizeof(abi.HaloStatsSpec) == 144
    assert L.halo_abi_sizeof(14) == C.sizeof(abi.HaloImageStats) == 568
    assert abi.HaloImageStats.value.offset == 440 and abi.HaloStatsSpec.norm.offset == 136
