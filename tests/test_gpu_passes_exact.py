"""The accumulation and reorder passes of halo_kernels.hip, record by record and bit for bit.

Synthetic records go to the launchers themselves (tests/cpp/passes_shim.cpp), the references are plain numpy in int64 / float64 (tests/_passes.py):
the per-tile sums are 64-bit fixed point, so a plane slot after a pass is exactly

    float32(plane_before + float32(float64(sum over its records of floor(float64(w) * 2^F + 0.5)) * 2^-F))

whatever the order of the adds, and the canonical reorder is integer work.  Where a record may fall to the fp64 twin or to fp32 atomics (a tile list
that overflows; the two workgroups per tile of the plain binned pass) the weights are dyadic (k * 2^-12), so every partial sum is exact in any order.
Every buffer lies between guard bands that are checked after the run; planes start non-zero; what a pass must not read holds poison.

The one comparison here that is not bit for bit is the fold over 31 planes of random values: its bound, (n_planes + 2) * 2^-24 * sum |coef * t| per
pixel and channel, is one rounding per multiply-add of the chain however it is contracted, plus the final add to the image.
"""
import ctypes as C

import numpy as np
import pytest

from tests import _passes as P

pytestmark = pytest.mark.gpu

U32 = np.uint32


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(U32)


def assert_bits_equal(got, want, what):
    g, w = bits(got).ravel(), bits(want).ravel()
    if not np.array_equal(g, w):
        bad = np.flatnonzero(g != w)
        raise AssertionError("%s: %d of %d slots differ, first at %d: got %r want %r" % (what, len(bad), len(g), bad[0], np.ravel(got)[bad[0]], np.ravel(want)[bad[0]]))


def round_up(n, k):
    return (int(n) + k - 1) // k * k


def start_plane(rng, n, dyadic):
    return P.dyadic_plane(rng, n) if dyadic else (0.5 + rng.random(n, dtype=np.float32)).astype(np.float32)


# ---- the hit-log routes ---------------------------------------------------------------------------------------------------------------------

def run_log(rng, lay, x, w, *, tiles, planes=1, s, interleaved, frac_bits=32, cap2, dyadic, twin=True, copies_log2=0, xyz=None):
    """One launch_log_route (xyz = None) or launch_log_route_xyz (xyz = (pool rows [n, 3], codes)) over the records {x, w}, and every check that does
    not depend on the case: guard bands, inputs untouched, the lists the split left, the counts, the planes, the twin and its flag."""
    L = P.shim()
    stride = P.const("kBinCntStride")
    n_slots = lay.n_slots
    ch = 3 if xyz is not None else 1
    plane_stride = n_slots << copies_log2
    plane0 = start_plane(rng, ch * plane_stride, dyadic)
    fills, reported = P.region_fills(len(x), P.CAP1)
    slot_mask = (1 << P.const("kLogWlShift")) - 1 if xyz is not None else 0xFFFFFFFF
    rec_x = x if xyz is None else (x | (xyz[1].astype(U32) << U32(P.const("kLogWlShift")))).astype(U32)
    log0 = P.deal_log(rng, rec_x, w, P.CAP1, fills, rec_x[:1000])
    b_plane, b_log, b_cnt1 = P.Buf(plane0), P.Buf(log0), P.Buf(reported)
    b_list2 = P.Buf(np.full((lay.n_lists * cap2, 2), P.POISON_U32, dtype=U32))
    b_cnt2 = P.Buf(P.counters(lay.n_lists, stride))
    b_twin = P.Buf(np.zeros(ch * n_slots, dtype=np.float64)) if twin else None
    b_flag = P.Buf(np.zeros(1, dtype=U32)) if twin else None
    if xyz is None:
        rc = L.pt_log_route(b_plane.ref(), b_log.ref(), P.CAP1, b_cnt1.ref(), len(fills), b_list2.ref(), cap2, b_cnt2.ref(), tiles, planes, s, int(interleaved), frac_bits,
                            P.ref_of(b_twin), P.ref_of(b_flag), copies_log2)
        contrib = [(x, w)]
    else:
        rows = np.asarray(xyz[0], dtype=np.float32)
        pool_size = len(rows)
        pool = np.full((pool_size, P.const("sizeof_WlEntryDev") // 4), 7.0, dtype=np.float32)   # (n_idx, spd_weight and the pads must not matter)
        for c, name in enumerate("xyz"):
            pool[:, P.const("offsetof_cmf_" + name) // 4] = rows[:, c]
        b_pool = P.Buf(pool)
        rc = L.pt_log_route_xyz(b_plane.ref(), plane_stride, b_log.ref(), P.CAP1, b_cnt1.ref(), len(fills), b_list2.ref(), cap2, b_cnt2.ref(), tiles, s, b_pool.ref(), pool_size,
                                frac_bits, P.ref_of(b_twin), P.ref_of(b_flag), copies_log2)
        assert b_pool.guards_intact() and np.array_equal(b_pool.a.view(U32), pool.view(U32))
        table = np.concatenate([rows, np.eye(3, dtype=np.float32)])   # pool entries, then the three unit rows
        with np.errstate(invalid="ignore"):
            contrib = [(x, (table[xyz[1], c] * w).astype(np.float32)) for c in range(3)]   # one fp32 product per channel
    assert rc == P.HIP_SUCCESS, "HIP status %d" % rc
    for name, b in (("plane", b_plane), ("log", b_log), ("cnt1", b_cnt1), ("list2", b_list2), ("cnt2", b_cnt2), ("twin", b_twin), ("flag", b_flag)):
        assert b is None or b.guards_intact(), "a guard band of %s was written" % name
    assert np.array_equal(b_log.a, log0) and np.array_equal(b_cnt1.a, reported)
    cnt2 = P.check_lists(b_list2.a, b_cnt2.a, cap2, stride, lay, rec_x, w, code_mask=slot_mask)
    assert int(cnt2.sum()) == int(np.minimum(reported.astype(np.int64), P.CAP1).sum()) == len(x)
    overflowed = bool((cnt2 > cap2).any())
    after = b_plane.a.reshape(ch, 1 << copies_log2, n_slots)
    before = plane0.reshape(ch, 1 << copies_log2, n_slots)
    assert_bits_equal(after[:, 1:], before[:, 1:], "the other copies of the planes")
    for c, (sl, v) in enumerate(contrib):
        if not overflowed:
            assert_bits_equal(after[c, 0], P.expected_plane(before[c, 0], sl, v, frac_bits), "plane %d" % c)
        else:
            assert dyadic, "an overflowing case needs dyadic weights"
            P.assert_dyadic_exact(before[c, 0], sl, v, bits=15 if xyz is not None else P.DYADIC_BITS)
            with np.errstate(invalid="ignore"):
                exact = before[c, 0].astype(np.float64) + np.bincount(sl.astype(np.int64), weights=v.astype(np.float64), minlength=n_slots)
            got = after[c, 0].astype(np.float64) + (b_twin.a[c * n_slots:(c + 1) * n_slots] if twin else 0.0)
            bad = np.flatnonzero(got != exact)
            assert len(bad) == 0, "plane + twin, channel %d: %d slots differ, first at %d: got %r want %r" % (c, len(bad), bad[0], got[bad[0]], exact[bad[0]])
    if twin:
        assert int(b_flag.a[0]) == (1 if overflowed else 0), "the overflow flag is set if and only if a list overflowed"
        assert overflowed or not b_twin.a.any(), "the twin was written without an overflow"
    return cnt2, overflowed


def scalar_records(rng, lay, edges, dyadic):
    lens = P.list_lengths(rng, lay.n_lists, edges, sum(P.REGION_COUNTS) + P.CAP1)
    x = P.records_for(rng, lay, lens)
    w = P.dyadic_weights(rng, len(x)) if dyadic else P.arbitrary_weights(rng, len(x))
    return lens, x, w


def scalar_layout(T, s, form, planes=1):
    t = T.bit_length() - 1
    if form == "contiguous":
        return P.Layout(T, tile_log2=s + 10 - t, interleaved=False)
    return P.Layout(T * planes, s=s, t=t)


# T = 128, 256: both forms; T = 512 (and planes > 1) takes the 512-list split and is interleaved always.  s = 6..11: t <= s and t > s.
SCALAR_SHAPES = [(T, s, form) for T in (128, 256) for s in range(6, 12) for form in ("contiguous", "interleaved")] + [(512, s, "interleaved") for s in range(6, 12)]


@pytest.mark.parametrize("T,s,form", SCALAR_SHAPES)
def test_scalar_log_route_every_shape(T, s, form):
    rng = np.random.default_rng(1000 * T + 10 * s + len(form))
    lay = scalar_layout(T, s, form)
    lens, x, w = scalar_records(rng, lay, P.LIST_EDGES_SHORT, dyadic=False)
    frac_bits = (32, 28)[s % 2]
    _, overflowed = run_log(rng, lay, x, w, tiles=T, s=s, interleaved=form == "interleaved", frac_bits=frac_bits, cap2=round_up(lens.max() + 1, 16), dyadic=False)
    assert not overflowed


@pytest.mark.parametrize("T,s,form,planes", [(128, 9, "contiguous", 1), (128, 6, "interleaved", 1), (512, 7, "interleaved", 1), (128, 6, "interleaved", 4)])
def test_scalar_log_route_long_lists(T, s, form, planes):
    """lists either side of kListOnceMin (65536 records), where the non-temporal load loop takes over; planes = 4: per-entry planes back to back"""
    rng = np.random.default_rng(77 + T + s + planes)
    lay = scalar_layout(T, s, form, planes)
    lens, x, w = scalar_records(rng, lay, P.LIST_EDGES_LONG, dyadic=False)
    _, overflowed = run_log(rng, lay, x, w, tiles=T, planes=planes, s=s, interleaved=form == "interleaved", cap2=round_up(lens.max() + 1, 16), dyadic=False)
    assert not overflowed


def test_scalar_log_route_sum_above_2_to_53_at_frac_bits_20():
    """weights of a few thousand at the F that fix_frac_bits gives such a session (20): one slot's fixed-point sum passes 2^53 and the uint64 -> double
    conversion rounds — to nearest even on the device as in numpy, so the comparison stays bit for bit"""
    rng = np.random.default_rng(53)
    frac_bits = P.fix_frac_bits(3072.0, 1 << 28)
    assert frac_bits == 20
    lay = P.Layout(2, tile_log2=14, interleaved=False)
    n_hot = 4_500_000
    lens = np.array([150_000, n_hot + 1000])
    x = P.records_for(rng, lay, lens)
    hot_slot = U32(lay.n_slots - 3)
    x[np.flatnonzero(x >> U32(14) == 1)[:n_hot]] = hot_slot
    w = (np.float32(2048.0) + np.float32(1024.0) * rng.random(len(x), dtype=np.float32)).astype(np.float32)
    hot = np.flatnonzero(x == hot_slot)
    w[hot[:5000]] = P.arbitrary_weights(rng, 5000)   # (weights of that size alone are multiples of 2^-12: the sum's low bits come from small ones)
    w[hot[5000]] = 0.0
    if int(P.slot_sums(x, P.fix(w, frac_bits), lay.n_slots)[hot_slot]) % 2 == 0:
        w[hot[5000]] = 2.0 ** -20                    # one unit of the fixed point: the sum is odd
    total = int(P.slot_sums(x, P.fix(w, frac_bits), lay.n_slots)[hot_slot])
    assert (1 << 53) < total < (1 << 54) and total % 2 == 1   # not a float64: the conversion has to round
    _, overflowed = run_log(rng, lay, x, w, tiles=2, s=5, interleaved=False, frac_bits=frac_bits, cap2=round_up(lens.max() + 1, 16), dyadic=False)
    assert not overflowed


OVERFLOW_EDGES = [0, 1, 2, 3, 2047, 4095, 4096, 4097, 8191, 8193, 8194]   # cap2 = 4096: a list one short of full, full, and one over (position cap2 exactly)


@pytest.mark.parametrize("T,s,form,twin,copies_log2", [(128, 7, "contiguous", True, 0), (256, 6, "interleaved", True, 0), (512, 8, "interleaved", True, 0),
                                                      (128, 7, "contiguous", False, 0), (256, 7, "interleaved", False, 0), (512, 6, "interleaved", False, 0),
                                                      (128, 8, "contiguous", True, 3), (256, 6, "interleaved", True, 3)])
def test_scalar_log_route_overflowing_lists(T, s, form, twin, copies_log2):
    """cap2 below the longest lists: what does not fit goes to the fp64 twin (copy 0's, TwinOffset) and raises the flag, or — no twin — to fp32 atomics on
    the plane; plane + twin is the exact sum, nothing lands past cap2 in any list or outside the buffers"""
    rng = np.random.default_rng(4096 + T + s + copies_log2 + int(twin))
    lay = scalar_layout(T, s, form)
    lens, x, w = scalar_records(rng, lay, OVERFLOW_EDGES, dyadic=True)
    cnt2, overflowed = run_log(rng, lay, x, w, tiles=T, s=s, interleaved=form == "interleaved", cap2=4096, dyadic=True, twin=twin, copies_log2=copies_log2)
    assert overflowed and cnt2[-1] == 8194 and {4095, 4096, 4097} <= set(cnt2.tolist())


def test_scalar_log_route_with_room_leaves_twin_and_flag_alone_on_dyadic_weights():
    rng = np.random.default_rng(11)
    lay = scalar_layout(256, 7, "interleaved")
    lens, x, w = scalar_records(rng, lay, P.LIST_EDGES_SHORT, dyadic=True)
    _, overflowed = run_log(rng, lay, x, w, tiles=256, s=7, interleaved=True, cap2=round_up(lens.max(), 16), dyadic=True, copies_log2=3)
    assert not overflowed


def xyz_case(rng, T, s, pool_size, dyadic, edges):
    lay = P.Layout(T, s=s, t=T.bit_length() - 1)
    assert lay.slots_per_list <= 4096 and s + 10 <= P.const("kLogWlShift")
    lens, x, w = scalar_records(rng, lay, edges, dyadic)
    if dyadic:
        rows = (rng.integers(0, 8, size=(pool_size, 3)) / 8.0).astype(np.float32)
    else:
        rows = (2.0 * rng.random((pool_size, 3), dtype=np.float32)).astype(np.float32)
    rows[rng.random((pool_size, 3)) < 0.2] = 0.0   # a CMF component that is exactly 0 adds nothing to its channel
    if pool_size == 1:
        rows[0] = (0.0, rows[0, 1] or 0.5, 0.0)
    codes = rng.integers(0, pool_size + 3, size=len(x))
    codes[:pool_size + 3] = np.arange(pool_size + 3)    # every pool entry and the three unit rows
    return lay, lens, x, w, rows, codes


@pytest.mark.parametrize("T,s,pool_size", [(128, 6, 1), (256, 8, 31), (512, 11, None), (512, 6, 31), (128, 9, None)])
def test_xyz_log_route(T, s, pool_size):
    pool_size = P.const("HALO_WL_POOL_MAX") if pool_size is None else pool_size
    rng = np.random.default_rng(3 * T + s + pool_size)
    lay, lens, x, w, rows, codes = xyz_case(rng, T, s, pool_size, False, P.LIST_EDGES_SHORT)
    _, overflowed = run_log(rng, lay, x, w, tiles=T, s=s, interleaved=True, frac_bits=(32, 28)[s % 2], cap2=round_up(lens.max() + 1, 16), dyadic=False, xyz=(rows, codes))
    assert not overflowed


def test_xyz_log_route_long_lists():
    rng = np.random.default_rng(65536)
    lay, lens, x, w, rows, codes = xyz_case(rng, 128, 8, 31, False, P.LIST_EDGES_LONG)
    _, overflowed = run_log(rng, lay, x, w, tiles=128, s=8, interleaved=True, cap2=round_up(lens.max() + 1, 16), dyadic=False, xyz=(rows, codes))
    assert not overflowed


@pytest.mark.parametrize("T,s,pool_size,twin,copies_log2", [(256, 8, 31, True, 0), (512, 9, 255, True, 3), (128, 7, 1, False, 0)])
def test_xyz_log_route_overflowing_lists(T, s, pool_size, twin, copies_log2):
    rng = np.random.default_rng(5 * T + s + pool_size)
    lay, lens, x, w, rows, codes = xyz_case(rng, T, s, pool_size, True, OVERFLOW_EDGES)
    cnt2, overflowed = run_log(rng, lay, x, w, tiles=T, s=s, interleaved=True, cap2=4096, dyadic=True, twin=twin, copies_log2=copies_log2, xyz=(rows, codes))
    assert overflowed and cnt2[-1] == 8194


# ---- the binned routes ----------------------------------------------------------------------------------------------------------------------

BIN_EDGES = [0, 1, 2, 3, 2047, 2048, 2049, 8191, 8192, 8193, 16383, 16384, 16385, 16386]   # kBinSplit = 2 parts of 8 x 1024 records per unrolled iteration


@pytest.mark.parametrize("dyadic", [False, True])
def test_bin_accumulate(dyadic):
    """two workgroups per tile, each adds its half of the list with fp32 atomics: the plane starts from 0 (arbitrary weights: the two addends of a slot
    commute, and which records make up each is fixed by the kernel's split n * part / 2), or non-zero with dyadic values"""
    L = P.shim()
    rng = np.random.default_rng(20 + int(dyadic))
    stride, tile_log2 = P.const("kBinCntStride"), P.const("kBinTileLog2")
    tiles, t = 32, 5
    cap = 16400
    lens = P.list_lengths(rng, tiles, BIN_EDGES + [cap], 0)
    lens[lens > cap] = cap // 3
    lens[-1] = cap
    assert set(BIN_EDGES) <= set(lens.tolist())
    tile = np.repeat(np.arange(tiles, dtype=U32), lens)
    pos = np.concatenate([np.arange(n) for n in lens])
    local = rng.integers(0, 1 << tile_log2, size=len(tile)).astype(U32)
    x = (local << U32(t)) | tile                # the plane slot: local << tiles_log2 | tile
    w = P.dyadic_weights(rng, len(x)) if dyadic else P.arbitrary_weights(rng, len(x))
    n_slots = tiles << tile_log2
    plane0 = P.dyadic_plane(rng, n_slots) if dyadic else np.zeros(n_slots, dtype=np.float32)
    lists = np.zeros((tiles, cap, 2), dtype=U32)
    lists[:, :, 0] = (U32(5) << U32(t)) | np.arange(tiles, dtype=U32)[:, None]    # behind a list's fill: poison records, a valid slot and weight 1e6
    lists[:, :, 1] = np.float32(1e6).view(U32)
    lists[tile, pos, 0] = x
    lists[tile, pos, 1] = w.view(U32)
    reported = lens.astype(U32)
    reported[-1] = cap + 50                     # must be clamped to cap
    cnt0 = P.counters(tiles, stride, reported)
    b_plane, b_list, b_cnt = P.Buf(plane0), P.Buf(lists), P.Buf(cnt0)
    rc = L.pt_bin_accumulate(b_plane.ref(), b_list.ref(), cap, b_cnt.ref(), tiles, 32)
    assert rc == P.HIP_SUCCESS, "HIP status %d" % rc
    assert b_plane.guards_intact() and b_list.guards_intact() and b_cnt.guards_intact()
    assert np.array_equal(b_list.a, lists) and np.array_equal(b_cnt.a, cnt0)
    if dyadic:
        P.assert_dyadic_exact(plane0, x, w)
        want = (plane0.astype(np.float64) + np.bincount(x.astype(np.int64), weights=w.astype(np.float64), minlength=n_slots)).astype(np.float32)
    else:
        first = pos < (lens[tile] // 2)         # part 0 takes records [0, n / 2), part 1 the rest
        halves = [P.unfix(P.slot_sums(x[m], P.fix(w[m], 32), n_slots), 32) for m in (first, ~first)]
        want = (halves[0] + halves[1]).astype(np.float32)
    assert_bits_equal(b_plane.a, want, "plane")


@pytest.mark.parametrize("lists1,fan,edges,cap2", [(8, 2, P.LIST_EDGES_SHORT, None), (2, 32, P.LIST_EDGES_SHORT, None), (4, 8, P.LIST_EDGES_LONG, None), (4, 4, OVERFLOW_EDGES, 4096)])
def test_bin_two_level(lists1, fan, edges, cap2):
    """coarse lists (counters kBinCntStride apart, 8 workgroups each) dealt out to `fan` tile lists of 16 Ki consecutive slots, then summed per tile"""
    L = P.shim()
    rng = np.random.default_rng(100 * lists1 + fan)
    stride, tile_log2 = P.const("kBinCntStride"), P.const("kBinTileLog2")
    tiles, fan_log2 = lists1 * fan, fan.bit_length() - 1
    lay = P.Layout(tiles, tile_log2=tile_log2, interleaved=False)
    dyadic = cap2 is not None
    lens = P.list_lengths(rng, tiles, edges, 0)
    x = P.records_for(rng, lay, lens)
    w = P.dyadic_weights(rng, len(x)) if dyadic else P.arbitrary_weights(rng, len(x))
    cap2 = round_up(lens.max() + 1, 16) if cap2 is None else cap2
    coarse = (x >> U32(tile_log2 + fan_log2)).astype(np.int64)
    fills = np.bincount(coarse, minlength=lists1)
    cap1 = int(fills.max())                     # the fullest coarse list is full, and reports more than it can hold
    reported = fills.astype(U32)
    reported[np.argmax(fills)] = cap1 + 77
    order = np.argsort(coarse, kind="stable")
    pos = np.arange(len(x)) - np.repeat(np.cumsum(fills) - fills, fills)
    list1 = np.zeros((lists1, cap1, 2), dtype=U32)
    list1[:, :, 0] = (np.arange(lists1, dtype=U32)[:, None] << U32(tile_log2 + fan_log2)) | U32(9)   # poison behind the fill: a slot of that list, weight 1e6
    list1[:, :, 1] = np.float32(1e6).view(U32)
    list1[coarse[order], pos, 0] = x[order]
    list1[coarse[order], pos, 1] = w[order].view(U32)
    plane0 = start_plane(rng, lay.n_slots, dyadic)
    cnt1_0 = P.counters(lists1, stride, reported)
    b_plane, b_list1, b_cnt1 = P.Buf(plane0), P.Buf(list1), P.Buf(cnt1_0)
    b_list2 = P.Buf(np.full((tiles * cap2, 2), P.POISON_U32, dtype=U32))
    b_cnt2 = P.Buf(P.counters(tiles, stride))
    b_twin, b_flag = P.Buf(np.zeros(lay.n_slots, dtype=np.float64)), P.Buf(np.zeros(1, dtype=U32))
    rc = L.pt_bin_two_level(b_plane.ref(), b_list1.ref(), cap1, b_cnt1.ref(), lists1, b_list2.ref(), cap2, b_cnt2.ref(), tiles, fan_log2, 32, b_twin.ref(), b_flag.ref())
    assert rc == P.HIP_SUCCESS, "HIP status %d" % rc
    for b in (b_plane, b_list1, b_cnt1, b_list2, b_cnt2, b_twin, b_flag):
        assert b.guards_intact()
    assert np.array_equal(b_list1.a, list1) and np.array_equal(b_cnt1.a, cnt1_0)
    cnt2 = P.check_lists(b_list2.a, b_cnt2.a, cap2, stride, lay, x, w)
    assert int(cnt2.sum()) == int(np.minimum(reported.astype(np.int64), cap1).sum()) == len(x)
    overflowed = bool((cnt2 > cap2).any())
    assert overflowed == dyadic and int(b_flag.a[0]) == int(overflowed)
    if not overflowed:
        assert not b_twin.a.any()
        assert_bits_equal(b_plane.a, P.expected_plane(plane0, x, w, 32), "plane")
    else:
        P.assert_dyadic_exact(plane0, x, w)
        exact = plane0.astype(np.float64) + np.bincount(x.astype(np.int64), weights=w.astype(np.float64), minlength=lay.n_slots)
        assert np.array_equal(b_plane.a.astype(np.float64) + b_twin.a, exact)


# ---- the fold -------------------------------------------------------------------------------------------------------------------------------

def fold_s_log2(n_pix):
    s = 6
    while (P.const("kMonoRows") << s) < n_pix:
        s += 1
    return s


def fold_tile_height(s):
    """launch_fold's choice: the tallest of 64 / 16 / 4 rows that gives the launch >= 512 workgroups"""
    tiles_c, rows = (1 << s) // 64, P.const("kMonoRows")
    return 64 if tiles_c * (rows // 64) >= 512 else 16 if tiles_c * (rows // 16) >= 512 else 4


def run_fold(rng, width, height, n_planes, copies, twin, values):
    """twin: None (absent), 0 (present, flag 0: must be ignored) or 1 (present, flag 1: taken in and zeroed).  values: "dyadic" (bit for bit),
    "one" (one plane of arbitrary values, bit for bit) or "random" (float64 reference and the derived bound)."""
    L = P.shim()
    n_pix = width * height
    s = fold_s_log2(n_pix)
    plane = P.const("kMonoRows") << s
    slot = P.mono_slot(np.arange(n_pix), s).astype(np.int64)
    in_image = np.zeros(plane, dtype=bool)
    in_image[slot] = True
    assert in_image.sum() == n_pix
    if values == "dyadic":
        t = rng.integers(0, 256, size=(n_planes, copies, n_pix), dtype=np.uint8).astype(np.float32) * np.float32(2.0 ** -12)
        o = rng.integers(1, 256, size=(n_planes, n_pix), dtype=np.uint8).astype(np.float64) * 2.0 ** -12
        coef = (rng.integers(0, 8, size=(n_planes, 3)) / 4.0).astype(np.float32)
        xyz0 = (rng.integers(1, 4096, size=(n_pix, 3)) * 2.0 ** -14).astype(np.float32)
    else:
        t = rng.random((n_planes, copies, n_pix), dtype=np.float32)
        o = rng.random((n_planes, n_pix)) * 3.0
        coef = (0.5 * rng.random((n_planes, 3), dtype=np.float32)).astype(np.float32)
        xyz0 = (0.25 + 0.75 * rng.random((n_pix, 3), dtype=np.float32)).astype(np.float32)
    t[rng.integers(0, 4, size=t.shape, dtype=np.uint8) == 0] = 0.0   # slots nothing landed on
    t[:, :, rng.random(n_pix) < 0.1] = 0.0                           # ... and pixels nothing landed on in any plane
    o[rng.integers(0, 10, size=o.shape, dtype=np.uint8) < 7] = 0.0   # the twin is mostly empty; some of what it holds sits where the plane has nothing
    planes0 = np.full((n_planes, copies, plane), 1e30, dtype=np.float32)   # poison on the slots of pixels >= n_pix
    planes0[:, :, slot] = t
    b_xyz, b_planes = P.Buf(xyz0), P.Buf(planes0)
    b_twin = b_flag = None
    if twin is not None:
        twin0 = np.full((n_planes, plane), 1e30, dtype=np.float64)
        twin0[:, slot] = o
        b_twin, b_flag = P.Buf(twin0), P.Buf(np.array([twin], dtype=U32))
    coef_c = np.ascontiguousarray(coef)
    rc = L.pt_fold(b_xyz.ref(), b_planes.ref(), n_pix, s, copies, n_planes, coef_c.ctypes.data_as(C.POINTER(C.c_float)), P.ref_of(b_twin), P.ref_of(b_flag))
    assert rc == P.HIP_SUCCESS, "HIP status %d" % rc
    for b in (b_xyz, b_planes, b_twin, b_flag):
        assert b is None or b.guards_intact()
    assert not b_planes.a[:, :, in_image].any(), "a plane slot of an in-image pixel was left non-zero"
    if twin is not None:
        assert int(b_flag.a[0]) == twin
        if twin:
            assert not b_twin.a[:, in_image].any(), "a twin slot that was taken in was left non-zero"
        else:
            assert np.array_equal(b_twin.a, twin0), "the twin was touched with its flag at 0"
    take = twin == 1
    if values == "random":
        assert not take
        term = coef.astype(np.float64)[:, None, :] * t.astype(np.float64).sum(axis=1)[:, :, None]   # [plane, pixel, channel]
        want = xyz0.astype(np.float64) + term.sum(axis=0)
        bound = (n_planes + 2) * 2.0 ** -24 * np.abs(term).sum(axis=0)
        err = np.abs(b_xyz.a.astype(np.float64) - want)
        lit = bound > 0.0
        print("fold %dx%d, %d planes: largest error %.3e, largest error / bound %.3f over %d values" % (width, height, n_planes, err.max(), (err[lit] / bound[lit]).max(), lit.sum()))
        worst = np.unravel_index(np.argmax(err - bound), err.shape)
        assert (err <= bound).all(), (worst, err[worst], bound[worst])
        return
    tsum = t.astype(np.float64).sum(axis=1)                        # copies: dyadic, exact in any order (copies = 1: the value itself)
    if values == "dyadic":
        assert (tsum * 2.0 ** 12 < (1 << 24)).all()
    if take:
        tsum = (tsum + o).astype(np.float32).astype(np.float64)    # float32(float64(t) + o)
    if values == "one":
        assert n_planes == 1 and copies == 1
        add = (coef[0][None, :] * tsum[0].astype(np.float32)[:, None]).astype(np.float32)   # one fp32 product per channel
        want = (xyz0 + add).astype(np.float32)
    else:
        x = (coef.astype(np.float64)[:, None, :] * tsum[:, :, None]).sum(axis=0)
        total = (xyz0.astype(np.float64) + x) * 2.0 ** 14
        assert (total == np.floor(total)).all() and total.max() < (1 << 24)   # every partial sum of the chain is exact
        want = (xyz0.astype(np.float64) + x).astype(np.float32)
    assert_bits_equal(b_xyz.a, want, "xyz")


FOLD_SMALL = [(1, 1), (3, 1), (31, 1), (64, 1), (1, 8), (3, 8)]   # (n_planes, copies): privatised copies belong to sessions of few planes


@pytest.mark.parametrize("width,height,tile_rows", [(256, 128, 4), (480, 270, 4)])
@pytest.mark.parametrize("n_planes,copies", FOLD_SMALL)
def test_fold_small_images(width, height, tile_rows, n_planes, copies):
    """480 x 270: the pixel count is no multiple of 1024 and the last column lies partly outside the image"""
    assert fold_tile_height(fold_s_log2(width * height)) == tile_rows
    rng = np.random.default_rng(width + 7 * n_planes + copies)
    for twin in (None, 0, 1):
        run_fold(rng, width, height, n_planes, copies, twin, "dyadic")


@pytest.mark.parametrize("width,height,tile_rows,n_planes,copies,twin", [(800, 600, 16, 1, 1, 1), (800, 600, 16, 31, 1, 0), (800, 600, 16, 3, 8, 1), (800, 600, 16, 64, 1, None),
                                                                        (1920, 1080, 64, 1, 8, 1), (1920, 1080, 64, 3, 1, 0), (1920, 1080, 64, 31, 1, None)])
def test_fold_larger_images(width, height, tile_rows, n_planes, copies, twin):
    assert fold_tile_height(fold_s_log2(width * height)) == tile_rows
    run_fold(np.random.default_rng(height + n_planes + copies), width, height, n_planes, copies, twin, "dyadic")


@pytest.mark.parametrize("width,height", [(256, 128), (480, 270), (800, 600), (1920, 1080)])
@pytest.mark.parametrize("twin", [None, 0, 1])
def test_fold_one_plane_of_arbitrary_values(width, height, twin):
    run_fold(np.random.default_rng(width + (twin or 0)), width, height, 1, 1, twin, "one")


@pytest.mark.parametrize("width,height", [(480, 270), (800, 600)])
def test_fold_31_planes_of_random_values_within_the_derived_bound(width, height):
    run_fold(np.random.default_rng(31 + width), width, height, 31, 1, None, "random")


# ---- the canonical reorder ------------------------------------------------------------------------------------------------------------------

def make_pool(rng, n_roots, dense):
    """masks of 0-6 bits per root (sparse: about 0.2 bits per root), one record per set bit in canonical (root, seq) order, dealt at random over the shards"""
    shards, cstride, planes = P.const("kContShards"), P.const("kContCntStride"), 9
    if dense:
        k = rng.integers(0, 7, size=n_roots)
    else:
        k = np.where(rng.random(n_roots) < 0.15, rng.integers(1, 3, size=n_roots), 0)
    k[-3:] = np.array([2, 1, 3])[-min(3, n_roots):]                                           # the last roots — behind the last carry of the tiles scan — have records
    cand = rng.integers(0, 128, size=(n_roots, 6), dtype=np.uint8)
    pick = np.arange(6)[None, :] < k[:, None]
    roots = np.broadcast_to(np.arange(n_roots, dtype=np.int64)[:, None], cand.shape)[pick]
    seqs = cand[pick].astype(np.int64)
    edge_roots = rng.integers(0, n_roots, size=min(n_roots, 8))
    roots = np.concatenate([roots, np.repeat(edge_roots, 4)])       # bits 0, 63, 64 and 127
    seqs = np.concatenate([seqs, np.tile(np.array([0, 63, 64, 127]), len(edge_roots))])
    key = np.unique(roots * 128 + seqs)                             # canonical order; a seq drawn twice is one bit
    roots, seqs = key // 128, key % 128
    n_cont = len(key)
    mask = np.zeros(n_roots * 4, dtype=U32)
    np.bitwise_or.at(mask, roots * 4 + seqs // 32, (U32(1) << (seqs % 32).astype(U32)))
    vals = np.empty((planes, n_cont), dtype=U32)
    for p in range(planes):
        vals[p] = (np.arange(n_cont, dtype=np.uint64) * np.uint64(planes) + np.uint64(p)).astype(U32) ^ U32(0x5BD1E995)   # unique to the record and the plane
    vals[P.const("kContPlaneRoot")] = roots
    vals[P.const("kContPlaneSeq")] = seqs
    region = max(1, n_cont // 100)
    full, empty = 37, rng.permutation(np.delete(np.arange(shards), 37))[:10]
    fills = np.zeros(shards, dtype=np.int64)
    fills[full] = min(region, n_cont)
    open_ = np.setdiff1d(np.arange(shards), np.concatenate([[full], empty]))
    left = n_cont - fills[full]
    assert left <= len(open_) * region
    fills[open_] = np.minimum(rng.multinomial(left, np.full(len(open_), 1.0 / len(open_))), region)
    while fills.sum() < n_cont:                                     # what the clamp cut off goes where there is room
        room = open_[fills[open_] < region]
        fills[room[0]] += min(region - fills[room[0]], n_cont - fills.sum())
    in_stride = shards * region + 5
    pool = np.full((planes, in_stride), P.POISON_U32, dtype=U32)    # (a poison root is >= n_roots: reading one raises kContErrKey)
    where = np.concatenate([sh * region + np.arange(f) for sh, f in enumerate(fills)])[np.argsort(rng.permutation(n_cont))]
    pool[:, where] = vals                                           # record i of the canonical order sits at where[i]
    reported = fills.astype(U32)
    reported[full] += 9                                             # the full shard's counter ran past its region: clamped
    return dict(n_roots=n_roots, n_cont=n_cont, mask=mask, vals=vals, pool=pool, where=where, region=region, in_stride=in_stride, planes=planes,
                cnt=P.counters(shards, cstride, reported), max_fill=int(fills.max()), popcount=np.bincount(roots, minlength=n_roots))


def run_reorder(c, n_cont=None):
    L = P.shim()
    n_cont = c["n_cont"] if n_cont is None else n_cont
    out_stride = max(c["n_cont"], n_cont) + 8
    tiles = (c["n_roots"] + 2047) // 2048
    b_in, b_cnt, b_mask = P.Buf(c["pool"]), P.Buf(c["cnt"]), P.Buf(c["mask"])
    b_sum, b_base = P.Buf(np.full(tiles, P.POISON_U32, dtype=U32)), P.Buf(np.full(c["n_roots"], P.POISON_U32, dtype=U32))
    b_out, b_err = P.Buf(np.full((c["planes"], out_stride), P.POISON_U32, dtype=U32)), P.Buf(np.zeros(1, dtype=U32))
    rc = L.pt_cont_reorder(b_in.ref(), c["in_stride"], c["region"], b_cnt.ref(), c["max_fill"], b_mask.ref(), c["n_roots"], b_sum.ref(), b_base.ref(), b_out.ref(),
                           out_stride, n_cont, c["planes"], b_err.ref())
    assert rc == P.HIP_SUCCESS, "HIP status %d" % rc
    for b in (b_in, b_cnt, b_mask, b_sum, b_base, b_out, b_err):
        assert b.guards_intact()
    assert np.array_equal(b_in.a, c["pool"]) and np.array_equal(b_cnt.a, c["cnt"]) and np.array_equal(b_mask.a, c["mask"])
    want_base = np.cumsum(c["popcount"]) - c["popcount"]
    assert np.array_equal(b_base.a.astype(np.int64), want_base), "first slot of every root"
    return b_out.a, int(b_err.a[0])


@pytest.mark.parametrize("n_roots", [1, 7, 2047, 2048, 2049, 2048 * 64 + 1, 2048 * 2048 + 3])
def test_cont_reorder_sorts_the_pool_by_root_and_seq(n_roots):
    """2048 * 2048 + 3 roots: more than one pass of the tiles scan (2048 tile sums per pass), the carry between two passes"""
    c = make_pool(np.random.default_rng(n_roots), n_roots, dense=n_roots <= 2048 * 64 + 1)
    out, err = run_reorder(c)
    assert err == 0
    n = c["n_cont"]
    bad = np.flatnonzero((out[:, :n] != c["vals"]).any(axis=0))
    assert len(bad) == 0, "%d of %d records are not in their canonical slot, first at %d" % (len(bad), n, bad[0])
    assert (out[:, n:] == P.POISON_U32).all()


def test_cont_reorder_flags_inconsistent_pools():
    """a record whose bit is not in its root's mask, or whose root or seq lies outside the layer, sets kContErrKey and is not placed; an n_cont that is not
    the masks' popcount sets kContErrSum — an error word, never a fault: every index stays inside the buffers"""
    key, total = P.const("kContErrKey"), P.const("kContErrSum")
    rng = np.random.default_rng(99)
    base = make_pool(rng, 2049, dense=True)
    n, vals = base["n_cont"], base["vals"]
    victim = n // 2
    root, seq = int(vals[7, victim]), int(vals[8, victim])
    held = set(vals[8, vals[7] == root].tolist())
    stray = next(b for b in range(128) if b not in held)
    for plane, value in ((8, stray), (7, base["n_roots"]), (7, 0xFFFFFFFF), (8, 128)):
        c = dict(base, pool=base["pool"].copy())
        c["pool"][plane, base["where"][victim]] = value
        out, err = run_reorder(c)
        assert err == key, (plane, value, err)
        others = np.delete(np.arange(n), victim)
        assert np.array_equal(out[:, others], vals[:, others]) and (out[:, victim] == P.POISON_U32).all() and (out[:, n:] == P.POISON_U32).all()
    out, err = run_reorder(base, n_cont=n + 1)
    assert err == total and np.array_equal(out[:, :n], vals) and (out[:, n:] == P.POISON_U32).all()
    out, err = run_reorder(base, n_cont=n - 1)   # ... and the record whose slot would be n_cont - 1 is refused, not written
    assert err == total | key and np.array_equal(out[:, :n - 1], vals[:, :n - 1]) and (out[:, n - 1:] == P.POISON_U32).all()
