"""The ticket rule of the ticketed trace kernels (option tile_ticket; halo_device.h TicketSize, exported as halo_host_ticket_size): waves that
draw tickets in any interleaving tile the launch's wave-passes exactly once, with few enough adds on the counter's line and short last tickets.
No GPU.

The model of a wave is the kernel's loop: read the counter (`seen`), leave if it says the launch is handed out, ask halo_host_ticket_size for a
size, add it to the counter with a returning add (`old`), leave if old >= total, otherwise trace passes [old, min(old + size, total)).  Between a
wave's read and its add any number of other waves may read and add — the interleavings below are random — so `seen` <= `old`, and the size is
at least the one the rule gives for what is left at the add.

The bound on the adds that this implies.  Let D = div x waves be the rule's divisor and R = total - old > 0 what is left at a successful add.
  floor(R / D) >= hi: the size is hi                                      -> at most ceil(total / hi) such adds
  floor(R / D) = s, lo <= s < hi: R lies in an interval D long, size >= s  -> at most ceil(D / s) such adds, for each s
  floor(R / D) < lo: R < lo x D, size >= lo                               -> at most D such adds
and a wave adds in vain at most once per counter (it turns away at once), `waves` adds more.  The kernel cuts a launch into 64 ranges with a
counter each and runs the rule per range with the waves at home on it: for the headline's launch — 12 208 passes and 96 waves per range, the
defaults 4 / 64 / 2 — the bound is 1063 adds per counter line, against a budget of 30 000.  The cases below give the rule whole
launches on ONE counter, the hardest case for it: 781 250 passes and 6144 waves are bounded by 66 241 adds there.

"Last tickets": the tail of a launch is made of the tickets still being traced when the counter passes `total`.  With div = 2 a ticket of s passes
is drawn while at least 2 s x waves are left, which the other waves need 2 s passes' time for: only tickets of the rule's last phase — size lo —
are still running at the end, whatever the grid.
"""
import math
import random

import pytest

from ice_halo_sim_amd import backend
from ice_halo_sim_amd.build import build

TOTALS = [0, 1, 2, 63, 4096, 781250]
GRIDS = [1, 4, 6144]
LO, HI, DIV = 4, 64, 2   # the defaults (halo_device.h kTicketMin / kTicketMax / kTicketDiv)


@pytest.fixture(scope="module")
def size_of():
    build()
    fn = backend.host_ticket_size
    cache = {}

    def cached(total, seen, waves, lo, hi):
        key = (total, seen, waves, lo, hi)
        if key not in cache:
            cache[key] = fn(*key)
        return cache[key]
    return cached


def bound(total, waves, lo, hi, div):
    d = div * waves
    return math.ceil(total / hi) + sum(math.ceil(d / s) for s in range(lo, hi)) + d + waves


def draw_all(size_of, total, waves, lo, hi, div, rng, speeds=None):
    """Every wave runs the kernel's loop; which wave steps next is random (speeds: a time-ordered run instead, wave w taking speeds[w] per pass).
    Returns the tickets as (old, size, start time, end time) and the number of adds."""
    counter, adds, tickets = 0, 0, []
    if speeds is None:
        # state per wave: None = about to read, an int = has read that value and is about to add
        pending = {w: None for w in range(waves)}
        alive = list(pending)
        while alive:
            i = rng.randrange(len(alive))
            w = alive[i]
            if pending[w] is None:
                if counter >= total:
                    alive[i] = alive[-1]
                    alive.pop()
                else:
                    pending[w] = counter
                continue
            size = size_of(total, pending[w], div * waves, lo, hi)
            assert size >= 1
            old, counter, adds = counter, counter + size, adds + 1
            pending[w] = None
            if old >= total:
                alive[i] = alive[-1]
                alive.pop()
            else:
                tickets.append((old, size, 0.0, 0.0))
        return tickets, adds
    import heapq
    heap = [(rng.random() * 1e-3, w) for w in range(waves)]
    heapq.heapify(heap)
    while heap:
        t, w = heapq.heappop(heap)
        if counter >= total:
            continue
        size = size_of(total, counter, div * waves, lo, hi)
        assert size >= 1
        old, counter, adds = counter, counter + size, adds + 1
        n = min(old + size, total) - old
        tickets.append((old, size, t, t + n * speeds[w]))
        heapq.heappush(heap, (t + n * speeds[w], w))
    return tickets, adds


def check_tiling(tickets, total):
    at = 0
    for old, size, _, _ in sorted(tickets):
        assert old == at and size >= 1, (old, at, size)
        at = old + size
    assert (at >= total) if total else (at == 0 and not tickets)
    if tickets:
        assert max(old for old, _, _, _ in tickets) < total   # a ticket that starts past the end is nobody's


@pytest.mark.parametrize("waves", GRIDS)
@pytest.mark.parametrize("total", TOTALS)
def test_random_interleavings_tile_the_launch_once_within_the_budget(size_of, total, waves):
    for seed in range(3):
        tickets, adds = draw_all(size_of, total, waves, LO, HI, DIV, random.Random(1000 * seed + waves))
        check_tiling(tickets, total)
        assert adds <= bound(total, waves, LO, HI, DIV), (adds, bound(total, waves, LO, HI, DIV))


def test_the_headline_launch_holds_the_budget_of_adds_per_counter_line(size_of):
    """50 M rays are 781 250 passes in 64 ranges of 12 208 (the last 12 146), with the 96 waves of 6144 at home on each counter.  One range under its
    home waves, and — the worst a line can see — one range with ALL 6144 waves drawing on it at the kernel's divisor (2 x 96: thieves use the
    same rule): at most about 30 000 returning adds on the line either way."""
    groups = backend.host_ticket_groups()
    assert groups == 64 and backend.host_ticket_range(781250, 0) == (0, 12208) and backend.host_ticket_range(781250, 63) == (63 * 12208, 12146)
    assert bound(12208, 96, LO, HI, DIV) <= 30000
    for seed in range(3):
        tickets, adds = draw_all(size_of, 12208, 96, LO, HI, DIV, random.Random(seed))
        check_tiling(tickets, 12208)
        assert adds <= bound(12208, 96, LO, HI, DIV) <= 30000
    # all waves of the grid on one line: sizes from the divisor of 96 home waves, adds bounded by the tickets plus one vain add per wave
    counter, adds, rng = 0, 0, random.Random(5)
    waves = list(range(6144))
    while waves:
        i = rng.randrange(len(waves))
        if counter >= 12208:
            waves[i] = waves[-1]
            waves.pop()
            continue
        counter, adds = counter + size_of(12208, counter, DIV * 96, LO, HI), adds + 1
    assert adds <= 30000, adds


@pytest.mark.parametrize("all_passes", [0, 1, 2, 63, 64, 65, 4096, 4097, 781250, 2 ** 26])
def test_ranges_tile_the_launch_and_stealing_waves_finish_it(size_of, all_passes):
    """the kernel's range and steal logic (halo_host_ticket_range, halo_host_ticket_next): the ranges tile [0, all) in order; waves that run the
    kernel's loop over them — a range in hand until it is handed out, then the first open range at or after home — trace every pass exactly once"""
    groups = backend.host_ticket_groups()
    ranges = [backend.host_ticket_range(all_passes, g) for g in range(groups)]
    at = 0
    for first, n in ranges:
        assert first == at and n <= -(-all_passes // groups)
        at += n
    assert at == all_passes
    for mask, home in [(1, 0), (1, 5), (1 << 63, 0), (1 << 63, 63), ((1 << 7) | (1 << 3), 4), ((1 << 7) | (1 << 3), 8), (2 ** 64 - 1, 70)]:
        want = next(g % groups for g in range(home % groups, home % groups + groups) if mask >> (g % groups) & 1)
        assert backend.host_ticket_next(mask, home) == want
    assert backend.host_ticket_next(0, 3) == groups
    if all_passes > 4097:
        return   # (the ranges are checked above; the walk below is for launches a Python loop can trace)
    rng = random.Random(all_passes)
    blocks = 7   # fewer workgroups than ranges: most ranges are finished by thieves alone
    counters, traced = [0] * groups, []
    hand = {w: None for w in range(4 * blocks)}
    alive = list(hand)
    while alive:
        i = rng.randrange(len(alive))
        w = alive[i]
        if hand[w] is None:
            mask = sum(1 << g for g in range(groups) if counters[g] < ranges[g][1])
            if not mask:
                alive[i] = alive[-1]
                alive.pop()
                continue
            hand[w] = backend.host_ticket_next(mask, w // 4)
            continue
        g = hand[w]
        first, n = ranges[g]
        seen = counters[g]
        if seen >= n:
            hand[w] = None
            continue
        size = size_of(n, seen, max(DIV * 4 * blocks // groups, 1), LO, HI)
        old, counters[g] = counters[g], counters[g] + size
        if old >= n:
            hand[w] = None
            continue
        traced += range(first + old, first + min(old + size, n))
    assert sorted(traced) == list(range(all_passes))


@pytest.mark.parametrize("lo,hi,div", [(1, 16, 2), (2, 32, 2), (4, 64, 1), (2, 64, 1), (3, 3, 1)])
def test_other_bounds_of_the_rule(size_of, lo, hi, div):
    for total, waves in [(4096, 4), (63, 6144), (781250, 6144)]:
        tickets, adds = draw_all(size_of, total, waves, lo, hi, div, random.Random(7))
        check_tiling(tickets, total)
        assert all(lo <= s <= hi for _, s, _, _ in tickets)
        assert adds <= bound(total, waves, lo, hi, div)


@pytest.mark.parametrize("waves", GRIDS)
@pytest.mark.parametrize("total", TOTALS)
def test_last_tickets_are_short(size_of, total, waves):
    """A run in time: waves whose passes take 0.8 .. 1.2 of the mean (the spread profiles/resident_grid_ab.txt points to).  The tail of the launch is
    made of the tickets still being traced when the counter passes `total`: each is at most 4 passes long."""
    rng = random.Random(waves + 17 * total)
    speeds = [0.8 + 0.4 * rng.random() for _ in range(waves)]
    tickets, adds = draw_all(size_of, total, waves, LO, HI, DIV, rng, speeds)
    check_tiling(tickets, total)
    assert adds <= bound(total, waves, LO, HI, DIV)
    if not tickets:
        return
    t_out = min(t0 for old, size, t0, _ in tickets if old + size >= total)
    last = [min(old + size, total) - old for old, size, _, t1 in tickets if t1 > t_out]
    # (one wave alone has no tail to speak of: its last ticket is the launch's end whatever its length, and the rule shrinks it all the same)
    assert max(last) <= 4, sorted(last)[-5:]


def test_degenerate_arguments(size_of):
    assert size_of(10, 20, 4, 2, 64) == 2       # a counter past the end: the smallest ticket (the add that follows finds nothing)
    assert size_of(1000, 0, 0, 0, 0) == 1       # waves = 0 counts as 1, lo = 0 as 1, hi < lo as lo
    assert size_of(2 ** 26, 0, 1, 1, 1024) == 1024
