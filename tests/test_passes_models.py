"""CPU side of tests/test_gpu_passes_exact.py: the shim builds, links and reports "no device" cleanly, and the Python models the GPU tests
judge the kernels by (TileMap, MonoSlot, TwinOffset, the fixed-point sums) are right in themselves."""
import ctypes as C

import numpy as np
import pytest

from tests import _passes as P

# every (s_log2, tiles_log2) the GPU tests cut a plane with: T = 128, 256, 512 over s = 6..11 (scalar route; X/Y/Z where a tile has <= 4 Ki slots)
ST_PAIRS = [(s, t) for t in (7, 8, 9) for s in range(6, 12)]


def test_shim_builds_links_and_reports_no_device():
    L = P.shim()
    for name in ("pt_log_route", "pt_log_route_xyz", "pt_bin_accumulate", "pt_bin_two_level", "pt_fold", "pt_cont_reorder"):
        getattr(L, name)
    if L.pt_device_count() != 0:
        return   # (a GPU is present: tests/test_gpu_passes_exact.py runs the entry points)
    one = P.Buf(np.zeros(16, dtype=np.uint32))
    coef = (C.c_float * 3)(1.0, 1.0, 1.0)
    r = one.ref()
    assert L.pt_log_route(r, r, 1, r, 0, r, 16, r, 128, 1, 7, 1, 32, None, None, 0) == P.HIP_NO_DEVICE
    assert L.pt_log_route_xyz(r, 0, r, 1, r, 0, r, 16, r, 128, 7, r, 1, 32, None, None, 0) == P.HIP_NO_DEVICE
    assert L.pt_bin_accumulate(r, r, 1, r, 1, 32) == P.HIP_NO_DEVICE
    assert L.pt_bin_two_level(r, r, 1, r, 1, r, 16, r, 2, 1, 32, None, None) == P.HIP_NO_DEVICE
    assert L.pt_fold(r, r, 1, 6, 1, 1, coef, None, None) == P.HIP_NO_DEVICE
    assert L.pt_cont_reorder(r, 1, 1, r, 1, r, 1, r, r, r, 1, 1, 9, r) == P.HIP_NO_DEVICE
    assert one.guards_intact() and not one.a.any()


def test_shim_exports_the_constants_of_the_device_header():
    import re
    src = open(P.SHIM_DEPS[2]).read() + open(P.SHIM_DEPS[3]).read()
    for name in ("kBinCntStride", "kBinTileLog2", "kLogWlShift", "kMonoRows", "kFoldGroup", "kContShards", "kContCntStride", "kContPlaneRoot", "kContPlaneSeq",
                 "kContMaskWords", "kContErrKey", "kContErrSum"):
        m = re.search(r"\b%s\s*=\s*(\d+)" % name, src)
        assert m and P.const(name) == int(m.group(1)), name
    assert P.const("HALO_WL_POOL_MAX") == int(re.search(r"#define\s+HALO_WL_POOL_MAX\s+(\d+)", src).group(1))
    assert P.const("sizeof_WlEntryDev") == 32 and P.const("sizeof_HitRec") == 8
    assert [P.const("offsetof_cmf_" + c) for c in "xyz"] == [8, 12, 16]
    assert P.shim().pt_const(b"no_such_constant") == -1


@pytest.mark.parametrize("s,t", ST_PAIRS)
def test_tile_map_model_is_a_bijection(s, t):
    n = 1024 << s
    slot = np.arange(n, dtype=np.uint32)
    tile, local = P.tile_split(slot, s, t)
    assert tile.max() == (1 << t) - 1 and local.max() == (n >> t) - 1
    pair = tile.astype(np.uint64) * np.uint64(n >> t) + local
    assert len(np.unique(pair)) == n                                   # slot -> (tile, local) is one to one, hence onto
    assert np.array_equal(P.tile_slot_of(tile, local, s, t), slot)     # ... and slot_of inverts it
    assert np.bincount(tile).min() == np.bincount(tile).max() == n >> t


def test_layout_finds_its_own_slots():
    rng = np.random.default_rng(5)
    for lay in (P.Layout(256, s=7, t=7), P.Layout(512, s=6, t=9), P.Layout(128, tile_log2=9, interleaved=False), P.Layout(64, tile_log2=14, interleaved=False)):
        lst = rng.integers(0, lay.n_lists, size=5000).astype(np.uint32)
        local = rng.integers(0, lay.slots_per_list, size=5000).astype(np.uint32)
        slot = lay.slot(lst, local)
        assert slot.max() < lay.n_slots and np.array_equal(lay.list_of(slot), lst)


def test_mono_slot_model_matches_the_header():
    L = P.shim()
    rows = P.const("kMonoRows")
    rng = np.random.default_rng(6)
    for s in (6, 7, 9, 11, 13):
        pix = np.concatenate([np.arange(0, 2100), rng.integers(0, rows << s, size=2000), [(rows << s) - 1]]).astype(np.uint32)
        pix = pix[pix < (rows << s)]
        want = np.array([L.pt_mono_slot(int(p), s) for p in pix], dtype=np.uint32)
        assert np.array_equal(P.mono_slot(pix, s), want)
        every = P.mono_slot(np.arange(rows << s, dtype=np.uint32), s) if s <= 9 else None
        assert every is None or len(np.unique(every)) == rows << s   # a bijection on the plane


def test_twin_offset_model_matches_the_header():
    L = P.shim()
    rng = np.random.default_rng(7)
    for plane_log2, copies_log2 in ((16, 0), (16, 3), (21, 3), (0, 0)):
        off = rng.integers(0, 3 << (plane_log2 + copies_log2), size=500).astype(np.uint64)
        want = np.array([L.pt_twin_offset(int(o), plane_log2, copies_log2) for o in off], dtype=np.uint64)
        assert np.array_equal(P.twin_offset(off, plane_log2, copies_log2), want)


@pytest.mark.parametrize("frac_bits", [32, 28, 20])
def test_expected_plane_agrees_with_a_per_record_loop(frac_bits):
    rng = np.random.default_rng(frac_bits)
    n_slots, n = 64, 3000
    slots = rng.integers(0, n_slots - 4, size=n)          # (the last slots get nothing)
    w = P.arbitrary_weights(rng, n)
    w[:8] = np.array([0.5 * 2.0 ** -frac_bits, 1.5 * 2.0 ** -frac_bits, 2.5 * 2.0 ** -frac_bits, 1.0, np.float32(1.0) - np.float32(2.0 ** -24), 2.0 ** -24, 3e-39, np.nan], dtype=np.float32)
    if frac_bits == 20:   # one slot's sum above 2^53, where uint64 -> float64 rounds
        hot = rng.integers(0, n, size=1200)
        slots[hot] = 7
        w[hot] = (np.float32(4e9) * (1.0 + rng.random(len(hot), dtype=np.float32))).astype(np.float32)
        assert int(P.slot_sums(slots, P.fix(w, frac_bits), n_slots)[7]) > (1 << 53)
    before = (0.5 + rng.random(n_slots, dtype=np.float32)).astype(np.float32)
    fast = P.expected_plane(before, slots, w, frac_bits)
    slow = P.slow_expected_plane(before, slots, w, frac_bits)
    assert np.array_equal(fast.view(np.uint32), slow.view(np.uint32))
    assert np.array_equal(fast[-4:].view(np.uint32), before[-4:].view(np.uint32))
    assert np.array_equal(P.fix(w, frac_bits), np.array([P.slow_fix(x, frac_bits) for x in w], dtype=np.uint64))


def test_fix_rounds_to_nearest_and_drops_nan_and_negative_weights():
    w = np.array([np.nan, -1.0, -0.0, 0.0, 1e-40, 1.0, 0.5 * 2.0 ** -32, 0.75 * 2.0 ** -32, 0.25 * 2.0 ** -32], dtype=np.float32)
    assert P.fix(w, 32).tolist() == [0, 0, 0, 0, 0, 1 << 32, 1, 1, 0]
    assert P.fix_frac_bits(1.0, (1 << 28) - 1) == 32 and P.fix_frac_bits(60.0, 1 << 26) == 28 and P.fix_frac_bits(1500.0, 1 << 29) == 20


def test_generated_records_reach_the_wanted_list_and_region_lengths():
    rng = np.random.default_rng(8)
    lay = P.Layout(128, s=6, t=7)
    fills_min = sum(P.REGION_COUNTS) + P.CAP1
    lens = P.list_lengths(rng, lay.n_lists, P.LIST_EDGES_LONG, fills_min)
    assert set(P.LIST_EDGES_LONG) <= set(lens.tolist()) and lens[-1] == 65537 and (lens == 0).sum() >= 3
    x = P.records_for(rng, lay, lens)
    assert np.array_equal(np.bincount(lay.list_of(x), minlength=lay.n_lists), lens)
    fills, reported = P.region_fills(len(x), P.CAP1)
    assert fills.sum() == len(x) and fills.max() == P.CAP1 and reported.max() > P.CAP1 and set(P.REGION_COUNTS) <= set(fills.tolist())
    assert np.minimum(reported, P.CAP1).sum() == len(x)
    w = P.dyadic_weights(rng, len(x))
    log = P.deal_log(rng, x, w, P.CAP1, fills, x[:100])
    live = np.concatenate([log[r * P.CAP1: r * P.CAP1 + f] for r, f in enumerate(fills)])
    assert np.array_equal(live[:, 0], x) and np.array_equal(live[:, 1], w.view(np.uint32))
    P.assert_dyadic_exact(P.dyadic_plane(rng, lay.n_slots), x, w)
