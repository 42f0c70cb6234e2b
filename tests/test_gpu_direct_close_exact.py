"""The closing form of the scalar per-tile pass (launch_log_route_close: halo_split_kernel, then halo_bin_accumulate_range_kernel<false, true>), record
by record and bit for bit.

A launch that is its whole session adds its tile sums to the XYZ image itself instead of writing the plane for the fold to read back.  With

    t = float32(float64(sum over the slot's records of floor(float64(w) * 2^F + 0.5)) * 2^-F)      (the pass's fixed point, tests/_passes.py)
    t = float32(float64(t) + o)    where the twin's flag is up and the twin holds o != 0            (the fold's way with the twin)

the image after the pass is exactly float32(xyz_before + float32(coef_c * t)) at the pixel of every slot with t != 0 — product and add rounded
separately, which is what the fold's chain gives for one plane — and untouched everywhere else.  Where records fall to the twin (a tile list that
overflows) the weights are dyadic (k * 2^-12), so the sum is exact however it is shared between the list and the twin.

Set-up as in tests/test_gpu_passes_exact.py: every buffer between guard bands, the image non-zero before, poison where nothing may be read.  The
image buffer has a row for EVERY slot of the plane: rows from n_pix on must come back as they were (a pixel test that failed would be a failed
assertion here, not a write outside the buffer).  The launcher is not given the plane at all; a poisoned one travels along and must come back
untouched.  Every case runs the launcher TWICE on one stream, on fresh records, with no host reset between: the second run sees the counters,
the twin and its flag as the first one left them.
"""
import ctypes as C

import numpy as np
import pytest

from tests import _close as K
from tests import _passes as P

pytestmark = pytest.mark.gpu

U32 = np.uint32
COEF = np.array([0.43351, 0.99495, 0.00875], dtype=np.float32)
# (s, tiles, width, height): 4 tiles of 16 Ki slots (256 rows x 64 columns each: runs of eight rows); 256 tiles of 512 slots (4 rows x 128 columns:
# runs of four); 128 tiles of 16 Ki slots (8 rows x 2048 columns).  None of the pixel counts is a multiple of 1024.
SHAPES = [(6, 4, 100, 70), (7, 256, 481, 269), (11, 128, 1921, 999)]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(U32)


def assert_bits_equal(got, want, what):
    g, w = bits(got).ravel(), bits(want).ravel()
    if not np.array_equal(g, w):
        bad = np.flatnonzero(g != w)
        raise AssertionError("%s: %d of %d floats differ, first at %d: got %r want %r" % (what, len(bad), len(g), bad[0], np.ravel(got)[bad[0]], np.ravel(want)[bad[0]]))


class Shape:
    def __init__(self, s, tiles, width, height):
        self.s, self.tiles, self.n_pix = s, tiles, width * height
        self.n_slots = 1024 << s
        self.tile_log2 = s + 10 - (tiles.bit_length() - 1)
        assert (s == 6 or (1024 << (s - 1)) < self.n_pix) and self.n_pix <= self.n_slots and self.n_pix % 1024 != 0 and self.tile_log2 <= P.const("kBinTileLog2")
        self.pix_slots = P.mono_slot(np.arange(self.n_pix), s)   # the slots that are pixels
        assert len(np.unique(self.pix_slots)) == self.n_pix

    def tile_of(self, slots):
        return np.asarray(slots, dtype=U32) >> U32(self.tile_log2)


def make_records(rng, sh, n, dyadic, empty_tile=None):
    """n records: nine in ten on pixels, the rest anywhere on the plane (most of those map to no pixel: they must be summed and dropped).  A hot
    slot with 5000 records, a slot whose records sum to zero (zero, negative and NaN weights), no record in `empty_tile`."""
    x = np.where(rng.random(n) < 0.9, sh.pix_slots[rng.integers(0, sh.n_pix, size=n)], rng.integers(0, sh.n_slots, size=n).astype(U32)).astype(U32)
    w = P.dyadic_weights(rng, n) if dyadic else P.arbitrary_weights(rng, n)
    hot, zero = sh.pix_slots[sh.n_pix // 3], sh.pix_slots[sh.n_pix // 2 + 1]
    if not dyadic:
        x[rng.choice(n, size=5000, replace=False)] = hot
    at = np.flatnonzero(x == zero)
    x[at] = hot if not dyadic else sh.pix_slots[5]
    at = rng.choice(n, size=40, replace=False)
    x[at] = zero
    w[at] = np.array([0.0, -1.0, -0.0, np.nan], dtype=np.float32)[rng.integers(0, 4, size=40)]
    if dyadic:   # (at most 2^12 hits and a numerator below 2^24 per slot: assert_dyadic_exact in run_close)
        w[at] = 0.0
    if empty_tile is not None:
        keep = sh.tile_of(x) != empty_tile
        x, w = x[keep], w[keep]
    return x, w


def run_close(rng, sh, runs, *, cap2, frac_bits, dyadic, twin0, flag0):
    """One ct_close over `runs` (one or two (x, w) pairs) and every check.  twin0: the twin before the first run; flag0: its flag."""
    L = K.shim()
    stride = P.const("kBinCntStride")
    img0 = (0.5 + rng.random((sh.n_slots, 3), dtype=np.float32)).astype(np.float32)   # rows >= n_pix: no pixel, must stay
    logs = []
    for x, w in runs:
        fills, reported = P.region_fills(len(x), P.CAP1)
        logs.append((P.Buf(P.deal_log(rng, x, w, P.CAP1, fills, x[:1000])), P.Buf(reported), len(fills)))
    b_img, b_mid = P.Buf(img0), P.Buf(np.zeros_like(img0))
    b_list2 = P.Buf(np.full((sh.tiles * cap2, 2), P.POISON_U32, dtype=U32))
    b_cnt2 = P.Buf(P.counters(sh.tiles, stride))
    b_twin, b_flag = P.Buf(twin0), P.Buf(np.array([flag0], dtype=U32))
    plane0 = np.full(sh.n_slots, P.POISON_U32, dtype=U32)
    b_plane = P.Buf(plane0)
    two = len(runs) == 2
    log_in = [(b.a.copy(), c.a.copy()) for b, c, _ in logs]
    rc = L.ct_close(b_img.ref(), sh.n_pix, COEF.ctypes.data_as(C.POINTER(C.c_float)), logs[0][0].ref(), logs[0][1].ref(), logs[0][2],
                    logs[1][0].ref() if two else None, logs[1][1].ref() if two else None, logs[1][2] if two else 0, P.CAP1, b_list2.ref(), cap2, b_cnt2.ref(),
                    sh.tiles, sh.s, frac_bits, b_twin.ref(), b_flag.ref(), b_plane.ref(), b_mid.ref() if two else None)
    assert rc == P.HIP_SUCCESS, "HIP status %d" % rc
    named = [("image", b_img), ("list2", b_list2), ("cnt2", b_cnt2), ("twin", b_twin), ("flag", b_flag), ("plane", b_plane), ("mid", b_mid)]
    named += [("log %d" % i, b) for i, (b, _, _) in enumerate(logs)] + [("cnt1 %d" % i, c) for i, (_, c, _) in enumerate(logs)]
    for name, b in named:
        assert b is None or b.guards_intact(), "a guard band of %s was written" % name
    for (b, c, _), (l0, c0) in zip(logs, log_in):
        assert np.array_equal(b.a, l0) and np.array_equal(c.a, c0), "the log or its counts were written"
    assert np.array_equal(b_plane.a, plane0), "the plane was written"
    # the route's own resets: every tile counter zero (the words between them as they were), the flag clear
    assert not b_cnt2.a[::stride][:sh.tiles].any(), "a tile counter was left non-zero"
    assert (np.delete(b_cnt2.a, np.arange(0, sh.tiles * stride, stride)) == P.POISON_U32).all(), "a word between the tile counters was written"
    assert int(b_flag.a[0]) == 0, "the twin's flag was left up"
    # expected sums of each run, the twin taken in where its flag was up when the pass read it
    want, twin, flag, took_twin = img0, np.asarray(twin0, dtype=np.float64), bool(flag0), False
    mids = []
    for x, w in runs:
        over = bool((np.bincount(sh.tile_of(x), minlength=sh.tiles) > cap2).any())
        if over:
            assert dyadic, "an overflowing case needs dyadic weights"
            P.assert_dyadic_exact(np.zeros(sh.n_slots), x, w)
            assert not flag or (twin * 4096.0 == np.floor(twin * 4096.0)).all()
            with np.errstate(invalid="ignore"):
                t = (np.bincount(x.astype(np.int64), weights=w.astype(np.float64), minlength=sh.n_slots) + (twin if flag else 0.0)).astype(np.float32)
            flag = True   # the split raised it
        else:
            t = K.tile_sums(x, w, sh.n_slots, frac_bits)
            if flag:
                t = K.with_twin(t, twin)
        if flag:
            took_twin, twin, flag = True, np.zeros(sh.n_slots), False   # consumed and zeroed, the flag cleared behind the pass
        want = K.expected_image(want, t, COEF, sh.n_pix, sh.s)
        mids.append(want)
    if two:
        assert_bits_equal(b_mid.a, mids[0], "the image after the first run")
    assert_bits_equal(b_img.a, want, "the image")
    if took_twin:
        assert not b_twin.a.any(), "a consumed slot of the twin was left non-zero"
    else:
        assert np.array_equal(b_twin.a.view(np.uint64), np.asarray(twin0, dtype=np.float64).view(np.uint64)), "the twin was touched with its flag down"


def n_records(sh):
    return 200_000 if sh.s < 11 else 400_000


@pytest.mark.parametrize("s,tiles,width,height", SHAPES)
def test_close_adds_the_tile_sums_to_the_image_and_never_reads_a_twin_whose_flag_is_down(s, tiles, width, height):
    rng = np.random.default_rng(100 * s + tiles)
    sh = Shape(s, tiles, width, height)
    runs = [make_records(rng, sh, n_records(sh), dyadic=False) for _ in range(2)]
    cap2 = (max(int(np.bincount(sh.tile_of(x), minlength=tiles).max()) for x, _ in runs) + 16) // 16 * 16
    run_close(rng, sh, runs, cap2=cap2, frac_bits=(32, 28)[s % 2], dyadic=False, twin0=np.full(sh.n_slots, 1e30), flag0=0)


@pytest.mark.parametrize("s,tiles,width,height", SHAPES)
def test_close_takes_the_twin_in_even_where_a_tile_has_no_record(s, tiles, width, height):
    """flag up, twin values on pixels of a tile without a single record (and on others, and on slots that are no pixel): all of it reaches the
    image or is dropped, all of it is zeroed; the second run finds the flag down"""
    rng = np.random.default_rng(200 * s + tiles)
    sh = Shape(s, tiles, width, height)
    empty = tiles // 2 + 1 if tiles > 4 else 2
    runs = [make_records(rng, sh, n_records(sh), dyadic=False, empty_tile=empty) for _ in range(2)]
    twin0 = np.zeros(sh.n_slots)
    in_empty = sh.pix_slots[sh.tile_of(sh.pix_slots) == empty]
    assert len(in_empty) >= 4
    twin0[in_empty[: max(4, len(in_empty) // 2)]] = 3.0 + rng.random(max(4, len(in_empty) // 2))
    twin0[rng.integers(0, sh.n_slots, size=5000)] = rng.random(5000) * 1e-3
    cap2 = (max(int(np.bincount(sh.tile_of(x), minlength=tiles).max()) for x, _ in runs) + 16) // 16 * 16
    run_close(rng, sh, runs, cap2=cap2, frac_bits=32, dyadic=False, twin0=twin0, flag0=1)


@pytest.mark.parametrize("s,tiles,width,height", SHAPES)
def test_close_with_tile_lists_that_overflow_into_the_twin(s, tiles, width, height):
    """cap2 far below the lists: the split sends what does not fit to the twin and raises the flag, the pass takes it back in — in both runs, the
    second starting from the flag, twin and counters the first one left"""
    rng = np.random.default_rng(300 * s + tiles)
    sh = Shape(s, tiles, width, height)
    runs = [make_records(rng, sh, n_records(sh), dyadic=True) for _ in range(2)]
    cap2 = 256 if tiles == 256 else 2048
    assert all((np.bincount(sh.tile_of(x), minlength=tiles) > cap2).any() for x, _ in runs)
    run_close(rng, sh, runs, cap2=cap2, frac_bits=32, dyadic=True, twin0=np.zeros(sh.n_slots), flag0=0)
