"""Float64 model of halo_consumer_stats (include/halo_trace.h): the statistics of the positive values of one float32 plane, the way the reference's
scripts/dump_xyz_stats.py takes them with numpy — np.percentile's default ("linear") rule, exact sums — written out with math.floor, np.sort and
math.fsum so that every rounding is in view.  tests/test_image_stats_model.py holds it to numpy and holds the host halves of the stage
(halo_host_percentile_rank, halo_host_binned_sum) to it; tests/test_gpu_image_stats.py holds the device stage to it."""
import math
import struct
from fractions import Fraction

import numpy as np

F32 = np.float32
TOOL_PERCENTILES = (50.0, 70.0, 90.0, 95.0, 99.0, 99.3, 99.5, 99.7, 99.9, 99.95, 99.99)     # scripts/dump_xyz_stats.py PERCENTILE_VALUES
THIRTEEN = (0.0,) + TOOL_PERCENTILES + (100.0,)
VALUE_RTOL = 4.0 * 2.0 ** -52


def bits32(x):
    return struct.unpack("<I", struct.pack("<f", float(x)))[0]


def bits64(x):
    return struct.unpack("<Q", struct.pack("<d", float(x)))[0]


def rank_rule(q, n):
    """(rank, frac) of percentile q among n values: vi = (q / 100) * (n - 1), the quotient first, then one float64 product."""
    vi = (float(q) / 100.0) * float(n - 1)
    r = math.floor(vi)
    return int(r), vi - r


def lerp(lo, hi, frac):
    """lo + (hi - lo) * frac in float64, three roundings."""
    lo, hi = float(lo), float(hi)
    with np.errstate(invalid="ignore"):
        return float(np.float64(lo) + (np.float64(hi) - np.float64(lo)) * np.float64(frac))


def stats(y, percentiles=THIRTEEN, norm=1.0):
    """The model of HaloImageStats for plane `y` (any shape, float32) and divisor `norm` (float32)."""
    y = np.asarray(y, F32).ravel()
    pos = np.sort(y[y > 0.0])            # (NaN fails the test; +inf sorts last)
    n = int(pos.size)
    out = {"pixel_count": int(y.size), "positive_count": n, "produced": n > 0}
    if n == 0:
        return out
    y64 = pos.astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        out["saturated_count"] = int(((pos / F32(norm)) > F32(1.0)).sum())      # the float32 quotient, like the tool's norm_y > 1.0
        out["sum"] = math.fsum(y64)
        out["sum_sq"] = math.fsum(y64 * y64)       # a float32 squared is exact in float64 (48 bits, exponent in range)
    out["max"] = float(pos[-1])
    out["rank"], out["frac"], out["lo"], out["hi"], out["value"] = [], [], [], [], []
    for q in percentiles:
        r, f = rank_rule(q, n)
        lo, hi = pos[r], pos[min(r + 1, n - 1)]
        out["rank"].append(r)
        out["frac"].append(f)
        out["lo"].append(float(lo))
        out["hi"].append(float(hi))
        out["value"].append(lerp(lo, hi, f))
    return out


def split(v):
    """(exponent field, 24-bit significand) of a positive float32: v = m * 2^(max(e, 1) - 150)."""
    u = bits32(v)
    e = (u >> 23) & 255
    return e, (u & 0x7FFFFF) | (0x800000 if e else 0)


def bins_of(values):
    """The three bin sets of the device's first sweep, as Python integers: per exponent field the sums of m, of (m * m) & 0xFFFFFF, of (m * m) >> 24."""
    b = [0] * 768
    for v in np.asarray(values, F32).ravel():
        if not v > 0:
            continue
        e, m = split(v)
        b[e] += m
        b[256 + e] += (m * m) & 0xFFFFFF
        b[512 + e] += (m * m) >> 24
    return b


def binned_fraction(bins, squares):
    """The exact value of a bin set (squares: bins[0:256] low halves, bins[256:512] high halves) as a Fraction."""
    tot = 0
    for e in range(255):
        s = max(e, 1) - 1
        if squares:
            tot += (bins[e] + (bins[256 + e] << 24)) << (2 * s)
        else:
            tot += bins[e] << s
    return Fraction(tot, 1 << (298 if squares else 149))


def binned_float(bins, squares):
    """... rounded once to float64 (Fraction -> float is correctly rounded); +inf when exponent field 255 holds anything."""
    if bins[255] or (squares and bins[256 + 255]):
        return math.inf
    return float(binned_fraction(bins, squares))
