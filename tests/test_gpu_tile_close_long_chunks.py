"""The closing pass over per-tile chunks (launch_tile_route_close: halo_tile_close_kernel) on LONG chunks — few workgroups, thousands of records
a chunk, what a small trace grid leaves — record by record and bit for bit, through the shim and the helpers of
tests/test_gpu_tile_route_exact.py.

The reader walks a chunk in steps of 64 x kLoads pairs of records per wave, kChunksInFlight chunks side by side, the next step's loads in the air
before this step's adds, the counts of 32 chunks held one per lane, an odd last record riding in the chunk's last 16 bytes.  So the shapes are
its edges: one workgroup, 63 and 65 (a batch of counts not full; the second and third batch, on the next waves), 1536 (six workgroups per CU: the
counts of more than one round of the workgroup's waves, all kept from the pre-pass) and 2100 (more rounds than the pre-pass keeps: the later
ones are read when their turn comes, as on the headline's 6103 workgroups); cap 4096; in ONE tile chunks of 0, 1 and cap records and one
whose count exceeds cap (clamped); and chunks of 2 x 64 x L - 1, 2 x 64 x L and 2 x 64 x L + 1 records — one record short of a whole step, a whole
step, one over: odd and even lengths — for the kept L = kLoads = 1 and for 2, 3 and 4 beside it, so that the file still holds its edges should the
pair move.  Every other chunk is random and short, as a trace kernel's mostly are.  What lies behind a chunk's fill is a record of weight 1e6 that
must not be summed; every buffer lies between guard bands.  The launcher runs TWICE on one stream with no host reset between, once with the
twin's flag up: the second run sees the twin and its flag as the first left them.

The reference is numpy's: the pass sums integers, floor(float64(w) * 2^F + 0.5), whose sum does not depend on the order of the adds.
"""
import ctypes as C

import numpy as np
import pytest

from tests import _close as K
from tests import _passes as P
from tests import _tile as T
from tests.test_gpu_tile_route_exact import COEF, assert_bits_equal

pytestmark = pytest.mark.gpu

U32 = np.uint32
CAP = 4096
STEP_EDGES = [2 * 64 * loads + d for loads in (1, 2, 3, 4) for d in (-1, 0, 1)]   # 127 128 129 (the kept pair's) | 255 256 257 | 383 .. | 511 ..
WANTED = [0, 1, CAP, CAP + 9] + STEP_EDGES
# workgroups -> (tiles, s): 16 tiles for one workgroup (a tile has ONE chunk there: the wanted counts take a tile each); 2 tiles of 8 Ki slots for
# the large grids (100 - 140 MB of chunks per run)
SHAPES = {1: (16, 6), 63: (8, 6), 65: (8, 6), 1536: (2, 4), 2100: (2, 4)}
WIDTH, HEIGHT = {6: 250, 4: 125}, {6: 201, 4: 101}   # no multiple of 1024 pixels, fewer pixels than slots


def make_counts(rng, tiles, wgs):
    """random short chunks (a quarter of them empty); the wanted counts all in tile 0 where it has the chunks, else one tile each"""
    counts = rng.integers(0, 700, size=(tiles, wgs))
    counts[rng.random((tiles, wgs)) < 0.25] = 0
    if wgs >= len(WANTED):
        counts[0, rng.permutation(wgs)[:len(WANTED)]] = WANTED
        assert all((counts[0] == c).any() for c in WANTED)
    else:
        assert tiles * wgs >= len(WANTED)
        counts.ravel()[:len(WANTED)] = WANTED
    assert all((counts == c).any() for c in WANTED)
    return counts


@pytest.mark.parametrize("flag0", [0, 1])
@pytest.mark.parametrize("wgs", sorted(SHAPES))
def test_tile_close_sums_long_chunks_exactly(wgs, flag0):
    tiles, s = SHAPES[wgs]
    tile_log2 = s + 10 - (tiles.bit_length() - 1)
    assert tiles <= T.shim().tt_tiles_max()
    rng = np.random.default_rng(77 * wgs + flag0)
    n_slots, n_pix, frac_bits = 1024 << s, WIDTH[s] * HEIGHT[s], (32, 28)[flag0]
    img0 = (0.5 + rng.random((n_slots, 3), dtype=np.float32)).astype(np.float32)   # rows >= n_pix: no pixel, must stay
    runs = []
    for _ in range(2):
        chunk, cnt, x, w = T.deal_chunks(rng, make_counts(rng, tiles, wgs), CAP, tile_log2, lambda n: P.arbitrary_weights(rng, n))
        runs.append((P.Buf(chunk), P.Buf(cnt), x, w))
    if flag0:   # twin values on slots all over the plane, pixels and others
        twin0 = np.zeros(n_slots)
        twin0[rng.integers(0, n_slots, size=3000)] = rng.random(3000) * 1e-3
    else:
        twin0 = np.full(n_slots, 1e30)   # flag down: never read
    b_img, b_mid = P.Buf(img0), P.Buf(np.zeros_like(img0))
    b_twin, b_flag = P.Buf(twin0), P.Buf(np.array([flag0], dtype=U32))
    rc = T.shim().tt_close(b_img.ref(), n_pix, COEF.ctypes.data_as(C.POINTER(C.c_float)), runs[0][0].ref(), runs[0][1].ref(), runs[1][0].ref(), runs[1][1].ref(),
                           wgs, CAP, tiles, s, frac_bits, b_twin.ref(), b_flag.ref(), b_mid.ref())
    assert rc == P.HIP_SUCCESS, "HIP status %d" % rc
    for name, b in [("image", b_img), ("mid", b_mid), ("twin", b_twin), ("flag", b_flag)] + [("chunks %d" % i, r[0]) for i, r in enumerate(runs)] + \
                   [("counts %d" % i, r[1]) for i, r in enumerate(runs)]:
        assert b.guards_intact(), "a guard band of %s was written" % name
    assert int(b_flag.a[0]) == 0, "the twin's flag was left up"
    want, flag, mids = img0, bool(flag0), []
    for _, _, x, w in runs:
        t = K.tile_sums(x, w, n_slots, frac_bits)
        if flag:
            t = K.with_twin(t, twin0)
            flag = False   # consumed and zeroed, the flag cleared behind the pass
        want = K.expected_image(want, t, COEF, n_pix, s)
        mids.append(want)
    assert_bits_equal(b_mid.a, mids[0], "the image after the first run")
    assert_bits_equal(b_img.a, want, "the image")
    if flag0:
        assert not b_twin.a.any(), "a consumed slot of the twin was left non-zero"
    else:
        assert np.array_equal(b_twin.a.view(np.uint64), twin0.view(np.uint64)), "the twin was touched with its flag down"
