"""float32 numpy model of the reference GUI's auto-exposure functions (src/gui/gui_ev_auto.hpp: DownsampleBoxSumY, ComputeP99Y, ComputeEvAuto)
and of the per-pixel landed intensity (src/server/render.cpp:584-593), restated — every operation rounds to fp32 where the reference's does.
tests/golden/ev_auto_vectors.json holds what the reference's own header returns on the inputs `recipe_image` makes (the fixture keeps only the
recipe's parameters); tests/test_ev_auto_model.py holds this model to it, tests/test_gpu_auto_ev.py holds halo_consumer_auto_ev to this model.
"""
import numpy as np

F32 = np.float32
_M64 = (1 << 64) - 1


def _mix(i, seed, stream):
    """One LCG step on uint64 per index — x = (i + (2 seed + stream) * 0x9E3779B97F4A7C15) * 6364136223846793005 + 1442695040888963407 (mod 2^64)
    — and its upper 32 bits folded down once (an LCG's low bits are poor): a closed form of the index, so no generator state and no order."""
    i = np.asarray(i, np.uint64)
    off = np.uint64(((2 * int(seed) + int(stream)) * 0x9E3779B97F4A7C15) & _M64)
    with np.errstate(over="ignore"):
        x = (i + off) * np.uint64(6364136223846793005) + np.uint64(1442695040888963407)
        x ^= x >> np.uint64(32)
        x = x * np.uint64(6364136223846793005) + np.uint64(1442695040888963407)
    return x >> np.uint64(32)   # 32 good bits


def recipe_image(w, h, seed, density, neg, exp_lo, exp_hi):
    """Y plane float32[h, w] from integers alone.  Pixel i (row-major): a = bits of stream 0 (24 of them, as a fraction of 2^24): a < density -> lit,
    density <= a < density + neg -> the same magnitude negated, else 0.  Magnitude = (2^23 + 23 bits of stream 1) * 2^(e - 23) with
    e = exp_lo + (stream 0's next 8 bits) % (exp_hi - exp_lo + 1): every value is an exact float32, no libm call."""
    n = int(w) * int(h)
    i = np.arange(n, dtype=np.uint64)
    r0, r1 = _mix(i, seed, 0), _mix(i, seed, 1)
    a = (r0 & np.uint64(0xFFFFFF)).astype(np.float64) / float(1 << 24)
    e = int(exp_lo) + ((r0 >> np.uint64(24)) & np.uint64(0xFF)).astype(np.int64) % (int(exp_hi) - int(exp_lo) + 1)
    mant = ((r1 & np.uint64(0x7FFFFF)) | np.uint64(0x800000)).astype(np.float64)
    mag = np.ldexp(mant, (e - 23).astype(np.int32)).astype(F32)
    y = np.zeros(n, F32)
    lit, minus = a < float(density), (a >= float(density)) & (a < float(density) + float(neg))
    y[lit] = mag[lit]
    y[minus] = -mag[minus]
    return y.reshape(int(h), int(w))


def box_sum_y(y, f):
    """DownsampleBoxSumY (:31-57): float32[hc, wc] box sums, or None where the reference returns an empty vector.  Each bin adds its f x f pixels one
    after another from 0.0f, rows outside, columns inside, every add rounded to fp32: here one strided plane per (dr, dc), all bins at once."""
    y = np.asarray(y, F32)
    h, w = y.shape
    if f <= 0 or w <= 0 or h <= 0:
        return None
    wc, hc = w // f, h // f
    if wc <= 0 or hc <= 0:
        return None
    acc = np.zeros((hc, wc), F32)
    for dr in range(f):
        for dc in range(f):
            acc = (acc + y[dr:hc * f:f, dc:wc * f:f]).astype(F32)
    return acc


def order_statistic(vals):
    """(the exact order statistic the reference takes with nth_element, count): over the values > 0, index (size_t)((float)count * 0.99f) clamped
    to count - 1 (:106-111, :132-137); (0, 0) when there is none."""
    v = np.asarray(vals, F32).ravel()
    v = np.sort(v[v > 0])
    n = int(v.size)
    if n == 0:
        return F32(0.0), 0
    idx = min(int(F32(n) * F32(0.99)), n - 1)
    return F32(v[idx]), n


def p99_y(y, f=1):
    """ComputeP99Y (:92-138) of a Y plane float32[h, w]: (p99 as float32 — the fine-equivalent one on the coarse path, count of positive values the
    percentile was taken over, coarse_w, coarse_h) with (0, 0) for the fine path.  A coarse grid without a positive bin gives 0, not the fine path."""
    y = np.asarray(y, F32)
    if f > 1:
        coarse = box_sum_y(y, f)
        if coarse is not None:
            p, n = order_statistic(coarse)
            if n:
                p = F32(p / (F32(f) * F32(f)))
            return p, n, coarse.shape[1], coarse.shape[0]
    p, n = order_statistic(y)
    return p, n, 0, 0


def per_pixel_intensity(total_intensity, n_pix):
    """RenderConsumer::GetRawXyzResult (render.cpp:586-587): snapshot_intensity_ (float) / (kNormScale * total_pix)."""
    return F32(F32(total_intensity) / (F32(0.08) * F32(n_pix))) if n_pix > 0 else F32(0.0)


def ev_auto(p99, per_pixel, target_white=135.0):
    """ComputeEvAuto (:143-155) in float32."""
    p99, per_pixel, tw = F32(p99), F32(per_pixel), F32(target_white)
    if per_pixel <= 0 or p99 <= 0:
        return F32(0.0)
    p99_norm = F32(p99 / per_pixel)
    t = F32(tw / F32(255.0))
    if t <= F32(0.04045):
        target_linear = F32(t / F32(12.92))
    else:
        target_linear = F32(np.power(F32(F32(t + F32(0.055)) / F32(1.055)), F32(2.4)))
    if target_linear <= 0 or p99_norm <= 0:
        return F32(0.0)
    ev = F32(np.log2(F32(target_linear / p99_norm)))
    return F32(min(max(ev, F32(-6.0)), F32(6.0)))


def bits(x):
    return int(np.asarray(x, F32).view(np.uint32))


def case_image(case):
    """The Y plane of a fixture case (tests/golden/ev_auto_vectors.json)."""
    r = case["recipe"]
    if r["id"] == "literal":
        return np.asarray(r["y"], F32).reshape(case["h"], case["w"])
    return recipe_image(case["w"], case["h"], r["seed"], r["density"], r["neg"], r["exp_lo"], r["exp_hi"])
