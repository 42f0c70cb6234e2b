"""The closing per-tile pass over per-tile chunks (launch_tile_route_close: halo_tile_close_kernel), record by record and bit for bit.

A trace kernel of the per-tile append leaves chunk[tile][workgroup][cap] and cnt[tile][workgroup] (records MET: above cap where a chunk overflowed,
and then the chunk holds cap of them).  With

    t = float32(float64(sum over the slot's held records of floor(float64(w) * 2^F + 0.5)) * 2^-F)      (the pass's fixed point, tests/_passes.py)
    t = float32(float64(t) + o)    where the twin's flag is up and the twin holds o != 0                 (the fold's way with the twin)

the image after the pass is exactly float32(xyz_before + float32(coef_c * t)) at the pixel of every slot with t != 0 and untouched everywhere else
— the integer sums do not depend on the order of the adds, so numpy's are the reference, bit for bit.

Shapes: 8 tiles x 5 workgroups with cap 24 — chunk counts 0, 1, an odd count, cap and cap + 7 (clamped), one tile without a record; and 8 tiles x 70
workgroups with cap 600 — more chunks than one wave's 64 counts, chunks past the 128 pairs a lane pair loads at once (129, 256, 257, 258 records),
odd and clamped ones.  Every buffer lies between guard bands; what lies behind a chunk's fill is a record of weight 1e6 that must not be read.  The
launcher runs TWICE on one stream, on fresh chunks, with no host reset between: the second run sees the twin and its flag as the first left them.
"""
import ctypes as C

import numpy as np
import pytest

from tests import _close as K
from tests import _passes as P
from tests import _tile as T

pytestmark = pytest.mark.gpu

U32 = np.uint32
COEF = np.array([0.43351, 0.99495, 0.00875], dtype=np.float32)
S, TILES, WIDTH, HEIGHT = 6, 8, 250, 201   # 64 Ki slots, 8 tiles of 8 Ki; 50 250 pixels (no multiple of 1024)
TILE_LOG2 = S + 10 - 3
EMPTY = 5                                   # the tile without a record
# (workgroups, cap, counts every run must contain)
SHAPES = {"small": (5, 24, [0, 1, 7, 24, 24 + 7]), "long": (70, 600, [0, 1, 129, 256, 257, 258, 599, 600, 607])}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(U32)


def assert_bits_equal(got, want, what):
    g, w = bits(got).ravel(), bits(want).ravel()
    if not np.array_equal(g, w):
        bad = np.flatnonzero(g != w)
        raise AssertionError("%s: %d of %d floats differ, first at %d: got %r want %r" % (what, len(bad), len(g), bad[0], np.ravel(got)[bad[0]], np.ravel(want)[bad[0]]))


def make_counts(rng, wgs, cap, wanted):
    counts = rng.integers(0, cap + 1, size=(TILES, wgs))
    counts[EMPTY, :] = 0
    free = [(t, g) for t in range(TILES) if t != EMPTY for g in range(wgs)]
    for (t, g), c in zip([free[i] for i in rng.permutation(len(free))[:len(wanted)]], wanted):
        counts[t, g] = c
    assert all((counts == c).any() for c in wanted) and not counts[EMPTY].any()
    return counts


@pytest.mark.parametrize("flag0", [0, 1])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_tile_close_sums_the_chunks_exactly(shape, flag0):
    wgs, cap, wanted = SHAPES[shape]
    assert TILES <= T.shim().tt_tiles_max()
    rng = np.random.default_rng(1000 * wgs + flag0)
    n_slots, n_pix, frac_bits = 1024 << S, WIDTH * HEIGHT, (32, 28)[flag0]
    pix_slots = P.mono_slot(np.arange(n_pix), S)
    img0 = (0.5 + rng.random((n_slots, 3), dtype=np.float32)).astype(np.float32)   # rows >= n_pix: no pixel, must stay
    runs = []
    for _ in range(2):
        chunk, cnt, x, w = T.deal_chunks(rng, make_counts(rng, wgs, cap, wanted), cap, TILE_LOG2, lambda n: P.arbitrary_weights(rng, n))
        runs.append((P.Buf(chunk), P.Buf(cnt), x, w))
        assert not ((x >> U32(TILE_LOG2)) == EMPTY).any()
    if flag0:   # twin values on pixels of the tile without a record, on other pixels and on slots that are no pixel
        twin0 = np.zeros(n_slots)
        in_empty = pix_slots[(pix_slots >> U32(TILE_LOG2)) == EMPTY]
        assert len(in_empty) >= 4
        twin0[in_empty[: len(in_empty) // 2]] = 3.0 + rng.random(len(in_empty) // 2)
        twin0[rng.integers(0, n_slots, size=3000)] = rng.random(3000) * 1e-3
    else:
        twin0 = np.full(n_slots, 1e30)   # flag down: never read
    b_img, b_mid = P.Buf(img0), P.Buf(np.zeros_like(img0))
    b_twin, b_flag = P.Buf(twin0), P.Buf(np.array([flag0], dtype=U32))
    kept = [(c.a.copy(), n.a.copy()) for c, n, _, _ in runs]
    rc = T.shim().tt_close(b_img.ref(), n_pix, COEF.ctypes.data_as(C.POINTER(C.c_float)), runs[0][0].ref(), runs[0][1].ref(), runs[1][0].ref(), runs[1][1].ref(),
                           wgs, cap, TILES, S, frac_bits, b_twin.ref(), b_flag.ref(), b_mid.ref())
    assert rc == P.HIP_SUCCESS, "HIP status %d" % rc
    for name, b in [("image", b_img), ("mid", b_mid), ("twin", b_twin), ("flag", b_flag)] + [("chunks %d" % i, r[0]) for i, r in enumerate(runs)] + \
                   [("counts %d" % i, r[1]) for i, r in enumerate(runs)]:
        assert b.guards_intact(), "a guard band of %s was written" % name
    for (c, n, _, _), (c0, n0) in zip(runs, kept):
        assert np.array_equal(c.a, c0) and np.array_equal(n.a, n0), "the chunks or their counts were written"
    assert int(b_flag.a[0]) == 0, "the twin's flag was left up"
    want, flag, mids = img0, bool(flag0), []
    for _, _, x, w in runs:
        t = K.tile_sums(x, w, n_slots, frac_bits)
        if flag:
            t = K.with_twin(t, twin0)
            flag = False   # consumed and zeroed, the flag cleared behind the pass
        want = K.expected_image(want, t, COEF, n_pix, S)
        mids.append(want)
    assert_bits_equal(b_mid.a, mids[0], "the image after the first run")
    assert_bits_equal(b_img.a, want, "the image")
    if flag0:
        assert not b_twin.a.any(), "a consumed slot of the twin was left non-zero"
    else:
        assert np.array_equal(b_twin.a.view(np.uint64), twin0.view(np.uint64)), "the twin was touched with its flag down"


def test_tile_close_refuses_shapes_it_cannot_take():
    """an odd cap (a chunk would not start on 16 bytes), more tiles than the trace kernel has counters, more records than its 32-bit index spans"""
    L = T.shim()
    one = P.Buf(np.zeros(64, dtype=np.float32))
    args = lambda wgs, cap, tiles: (one.ref(), 4, COEF.ctypes.data_as(C.POINTER(C.c_float)), one.ref(), one.ref(), None, None, wgs, cap, tiles, S, 32, one.ref(), one.ref(), None)
    for wgs, cap, tiles in ((5, 23, 8), (5, 24, 2 * L.tt_tiles_max()), (5, 24, 6), (1 << 14, 1 << 14, 8)):
        assert L.tt_close(*args(wgs, cap, tiles)) == 1, (wgs, cap, tiles)   # hipErrorInvalidValue, before anything is launched
