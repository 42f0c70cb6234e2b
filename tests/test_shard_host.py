"""halo_host_shard_slice — which rays of a crystal entry's share a shard takes (halo_set_shard) — against Python integers.  No GPU."""
import ctypes as C

import pytest

from ice_halo_sim_amd import abi, backend

SHARES = [0, 1, 31, 32, 33, (1 << 18) + 37, (1 << 32) - 17, (1 << 32) + 5]
CLOCKS = [1, 32, 48]
COUNTS = [1, 2, 3, 5, 16]


def _rule(share, clock, k, n):
    u = -(-share // clock)
    lo, hi = min(clock * (k * u // n), share), min(clock * ((k + 1) * u // n), share)
    return lo, hi - lo


@pytest.mark.parametrize("clock", CLOCKS)
@pytest.mark.parametrize("count", COUNTS)
def test_slices_are_the_rule_and_tile_the_share(clock, count):
    for share in SHARES:
        got = [backend.host_shard_slice(share, clock, k, count) for k in range(count)]
        assert got == [_rule(share, clock, k, count) for k in range(count)], (share, clock, count)
        end = 0
        for first, n in got:                       # disjoint, in index order, covering [0, share)
            assert first == end or n == 0, (share, clock, count, got)
            assert first % clock == 0 and first <= share
            if n:
                end = first + n
        assert end == share
        assert sum(n for _, n in got) == share
        units = [-(-n // clock) for _, n in got]   # sizes differ by at most one clock: whole units, the last one of the share may be short
        assert max(units) - min(units) <= 1
        assert max(n for _, n in got) - min(n for _, n in got) <= clock
        for first, n in got:                       # only the slice that ends the share may end inside a unit
            assert n % clock == 0 or first + n == share


@pytest.mark.parametrize("clock", CLOCKS)
def test_one_shard_is_the_whole_share(clock):
    for share in SHARES:
        assert backend.host_shard_slice(share, clock, 0, 1) == (0, share)


def test_bad_arguments_are_refused():
    L = backend.load_library()
    first, n = C.c_uint64(), C.c_uint64()
    ok = lambda *a: L.halo_host_shard_slice(*a)
    assert ok(100, 32, 0, 2, C.byref(first), C.byref(n)) == abi.HALO_OK
    assert ok(100, 32, 2, 2, C.byref(first), C.byref(n)) == abi.HALO_FATAL       # index >= count
    assert ok(100, 32, 0, 0, C.byref(first), C.byref(n)) == abi.HALO_FATAL       # count == 0
    assert ok(100, 0, 0, 2, C.byref(first), C.byref(n)) == abi.HALO_FATAL        # clock == 0
    assert ok(100, 32, 0, 2, None, C.byref(n)) == abi.HALO_FATAL
    assert ok(100, 32, 0, 2, C.byref(first), None) == abi.HALO_FATAL
    for bad in ((100, 32, 2, 2), (100, 32, 0, 0), (100, 0, 0, 2), (-1, 32, 0, 2), (100, 32, 0, 1 << 32)):
        with pytest.raises(ValueError):
            backend.host_shard_slice(*bad)


def test_the_new_entry_points_are_exported():
    L = backend.load_library()
    for sym in ("halo_set_shard", "halo_host_shard_slice", "halo_export_fixed", "halo_import_fixed"):
        assert sym in backend.EXPORTED_SYMBOLS and getattr(L, sym)
