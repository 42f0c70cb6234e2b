"""The bit-equality claim behind the deterministic route's hit log, in numpy (tests/_fixed_model.py).  No GPU.

A deterministic launch adds q(v, F) per hit, v the fp32 weight on a scalar plane or the fp32 product cmf * weight on X, Y, Z.  Under the hit log
the same hit reaches the plane by one of four paths — the workgroup's integer cache, a record summed by the per-tile pass, a record added by the
trace kernel because its region was full, a record added by the split pass because its tile list was full — and every path quantises the SAME
fp32 value with the SAME F and adds integers.  So the plane holds sum q(v) whatever path each hit took and in whatever order the adds ran: the
per-tile pass may skip a product whose CMF entry is 0 (it adds q(0 * w) = 0, also for a NaN weight), nothing else differs.  This file pins that
for the model the GPU tests compare against; tests/test_gpu_deterministic_log.py holds the device to it."""
import numpy as np
import pytest

from tests import _fixed_model as fm

D65_MAX = np.float32(118.0)   # the largest spd weight of the D65 pool


def _weights(rng, n):
    """fp32 weights as the kernels see them: mostly (0, 1] x spd, with zeros, negatives, NaN, denormals and the largest D65 weight mixed in."""
    w = (rng.random(n, dtype=np.float32) * rng.choice(np.array([1.0, 1e-3, 31.5, 118.0], np.float32), n)).astype(np.float32)
    special = np.array([0.0, -0.0, -1.0, -1e-30, np.nan, 1e-45, np.finfo(np.float32).tiny, 118.0, 1.0, 2.0 ** -33], np.float32)
    at = rng.choice(n, size=n // 8, replace=False)
    w[at] = rng.choice(special, at.size)
    return w


def _four_paths(rng, pix, v, n_pix, F):
    """Sum q(v) as a logged launch does: every hit takes one of the four paths at random, each path adds in an order of its own."""
    out = np.zeros(n_pix, np.uint64)
    path = rng.integers(0, 4, pix.size)
    for k in range(4):
        idx = np.flatnonzero(path == k)
        idx = idx[rng.permutation(idx.size)]
        if k == 0:   # the cache: summed per pixel first, flushed as one integer per pixel
            part = np.zeros(n_pix, np.uint64)
            np.add.at(part, pix[idx], fm.q(v[idx], F))
            out += part
        else:        # records and fallbacks: one integer add per hit
            np.add.at(out, pix[idx], fm.q(v[idx], F))
    return out


@pytest.mark.parametrize("F", [22, 29, 32])
@pytest.mark.parametrize("seed", [1, 2])
def test_scalar_records_sum_to_plane_sums_in_any_order(F, seed):
    rng = np.random.default_rng(seed)
    n, n_pix = 50_000, 257
    pix, w = rng.integers(0, n_pix, n), _weights(rng, n)
    want = fm.plane_sums(pix, w, n_pix, F)
    assert (_four_paths(rng, pix, w, n_pix, F) == want).all()
    # ... and plainly: any order of the quantised addends
    p = rng.permutation(n)
    assert (fm.plane_sums(pix[p], w[p], n_pix, F) == want).all()
    assert int(want.sum(dtype=np.uint64)) == int(fm.q(w, F).sum(dtype=np.uint64))


@pytest.mark.parametrize("F", [22, 25])
def test_xyz_records_quantise_the_fp32_product_like_the_direct_route(F):
    """The per-tile pass forms cmf * w as one fp32 multiply from the pool's row and the record's raw weight and skips a zero CMF entry; the direct
    route multiplies the same two floats and always adds.  Same q, channel by channel."""
    rng = np.random.default_rng(7)
    n, n_pix, pool = 40_000, 129, 31
    cmf = rng.random((pool, 3), dtype=np.float32) * np.float32(1.8)
    cmf[rng.integers(0, pool, 6), rng.integers(0, 3, 6)] = 0.0   # rows with a zero entry (the ends of the visible range)
    cmf[3] = 0.0
    code, pix, w = rng.integers(0, pool, n), rng.integers(0, n_pix, n), _weights(rng, n)
    w[:64] = D65_MAX
    for c in range(3):
        prod = (cmf[code, c] * w).astype(np.float32)            # one fp32 multiply, as accumulate_fixed and the pass both do
        direct = fm.plane_sums(pix, prod, n_pix, F)
        keep = cmf[code, c] != 0.0                               # the pass: `if (c4.x != 0.0f)`
        logged = _four_paths(rng, pix[keep], prod[keep], n_pix, F)
        assert (logged == direct).all(), c
        # a product is not the double product rounded later: the claim is about the fp32 value
        assert fm.q(prod, F).dtype == np.uint64


def test_what_adds_nothing_adds_nothing_on_every_path():
    f32 = np.float32
    nothing = np.array([0.0, -0.0, -1.0, -np.inf, np.nan], f32)
    with np.errstate(invalid="ignore"):
        zero_row, some_row = (f32(0.0) * nothing).astype(f32), (f32(1.5) * nothing).astype(f32)   # (0 * inf is a NaN: still nothing)
    for F in (22, 29, 32):
        assert fm.q(nothing, F).tolist() == [0] * nothing.size
        assert fm.q(zero_row, F).tolist() == [0] * nothing.size     # a zero CMF entry times anything
        assert fm.q(some_row, F).tolist() == [0] * nothing.size
    # the largest D65 weight at the scale its session gets: exact, and 2^30 of them cannot wrap a slot
    from ice_halo_sim_amd.backend import host_fixed_frac_bits
    F = host_fixed_frac_bits(float(D65_MAX), 1 << 30)
    assert fm.q(D65_MAX, F) == int(118.0 * 2 ** F) and int(fm.q(D65_MAX, F)) * (1 << 30) * 4 < 1 << 62
