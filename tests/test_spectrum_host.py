"""Spectrum sessions, host side (no GPU): which root takes which spectrum entry.

halo_begin_spectrum fixes the rule: root r (0-based within a crystal entry's share of m roots, counted across launches) takes entry
min(r // ceil(m / count), count - 1).  halo_host_spectrum_entry evaluates the function the kernels call, with the per-launch constants the host
hands them, for two different cuts of the share into launches.  It is compared with Python's integers, exactly, at every block edge."""
import numpy as np
import pytest

from ice_halo_sim_amd import backend

MS = [1, 2, 254, 255, 256, 10007, (1 << 20) + 37, (1 << 32) - 1, (1 << 32) + 5]
COUNTS = [1, 2, 3, 31, 255]


def want_entry(m, count, r):
    per = -(-m // count)
    return min(r // per, count - 1)


def edge_rays(m, count):
    """Every r within 2 of every block edge (k * per for k = 0 .. count), of the share's end and of the 32-bit wraps, inside [0, m)."""
    per = -(-m // count)
    marks = {k * per for k in range(count + 1)} | {0, m, 1 << 31, 1 << 32, 65521, 2 * 65521, (1 << 32) - 2}
    rs = set()
    for e in marks:
        for d in range(-2, 3):
            if 0 <= e + d < m:
                rs.add(e + d)
    return sorted(rs)


@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("m", MS)
def test_entry_of_every_ray_around_every_block_edge(m, count):
    rs = edge_rays(m, count)
    assert rs
    got = [backend.host_spectrum_entry(m, count, r) for r in rs]
    want = [want_entry(m, count, r) for r in rs]
    bad = [(r, g, w) for r, g, w in zip(rs, got, want) if g != w]
    assert not bad, "m %d count %d: (r, got, want) %s" % (m, count, bad[:5])
    assert max(got) <= count - 1                       # a short last block never names an entry past the table
    if count > m:                                      # blocks of one root: entries >= m get no ray
        assert got == list(range(m))


@pytest.mark.parametrize("m,count", [(10007, 3), (10007, 31), (256, 255), (254, 255), ((1 << 20) + 37, 31)])
def test_every_ray_of_a_small_share(m, count):
    """Exhaustive where the share is small enough: block sizes and the monotone order, not just the edges."""
    step = 1 if m <= 20000 else 97
    rs = np.arange(0, m, step, dtype=np.int64)
    got = np.array([backend.host_spectrum_entry(m, count, int(r)) for r in rs])
    per = -(-m // count)
    assert (got == np.minimum(rs // per, count - 1)).all()
    assert (np.diff(got) >= 0).all()
    if step == 1:
        sizes = np.bincount(got, minlength=count)
        assert sizes.sum() == m and sizes.max() == per and (sizes[: (m - 1) // per] == per).all()


def test_random_rays_against_python_integers():
    rng = np.random.default_rng(20)
    for m in MS:
        for count in COUNTS:
            for r in rng.integers(0, m, 40):
                assert backend.host_spectrum_entry(m, count, int(r)) == want_entry(m, count, int(r)), (m, count, int(r))
