"""Synthetic records for the accumulation and reorder passes (halo_kernels.hip), through tests/cpp/passes_shim.cpp.

  build_shim() / shim()   the host-only shim (libpasses_shim.so, linked against libhalo_hip.so) and its ctypes signatures
  Buf                     a numpy array between two guard bands, as the shim's PtBuf
  tile_split / tile_slot_of / mono_slot / twin_offset   Python models of TileMap, MonoSlot and TwinOffset (halo_kernels.hip, halo_device.h)
  fix / unfix / slot_sums / expected_plane              the 64-bit fixed point of the per-tile sums (FixQ), in int64 / float64 numpy
  slow_* functions        the same, one record at a time with Python integers: what the fast forms are checked against on the CPU

Everything here is numpy and ctypes; nothing needs a GPU until a pt_* launcher entry point is called.
"""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "ice_halo_sim_amd")
SHIM_SRC = os.path.join(ROOT, "tests", "cpp", "passes_shim.cpp")
SHIM_SO = os.path.join(ROOT, "tests", "cpp", "libpasses_shim.so")
SHIM_DEPS = [SHIM_SRC, os.path.join(PKG, "csrc", "halo_launch.h"), os.path.join(PKG, "csrc", "halo_device.h"), os.path.join(ROOT, "include", "halo_trace.h")]

HIP_SUCCESS = 0
HIP_NO_DEVICE = 100        # hipErrorNoDevice
GUARD = 4096               # bytes of guard band on either side of a buffer (a multiple of 256: device pointers keep their alignment)
GUARD_BYTE = 0xA5
POISON_U32 = 0xDEADBEEF    # never a valid slot of the planes used here (bit 31 set), NaN-free as a weight is irrelevant: it must never be read


def build_shim(force=False):
    """Compile the shim the way halo_backend.cpp is compiled (hipcc as a host compiler, no device code), when it is missing or older than its sources."""
    from ice_halo_sim_amd import build as hip_build
    if not force and os.path.exists(SHIM_SO) and all(os.path.getmtime(d) <= os.path.getmtime(SHIM_SO) for d in SHIM_DEPS):
        return SHIM_SO
    if not os.path.exists(hip_build.LIB):
        raise ImportError("libhalo_hip.so is not built — run `python -m ice_halo_sim_amd.build` (needs hipcc)")
    cmd = [hip_build.hipcc(), "-O2", "-ffp-contract=off", "-fno-fast-math", "-D__HIP_PLATFORM_AMD__", "-std=c++17", "-fPIC", "-shared",
           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(PKG, "csrc"), SHIM_SRC, "-o", SHIM_SO,
           "-L" + PKG, "-lhalo_hip", "-Wl,-rpath," + PKG]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("passes_shim.cpp failed to build:\n" + r.stdout + r.stderr)
    return SHIM_SO


class PtBuf(C.Structure):
    _fields_ = [("host", C.c_void_p), ("bytes", C.c_uint64), ("lead", C.c_uint64)]


_shim = None


def shim():
    global _shim
    if _shim is not None:
        return _shim
    L = C.CDLL(build_shim())
    B, u32 = C.POINTER(PtBuf), C.c_uint32
    L.pt_device_count.restype = C.c_int; L.pt_device_count.argtypes = []
    L.pt_const.restype = C.c_int64; L.pt_const.argtypes = [C.c_char_p]
    L.pt_mono_slot.restype = u32; L.pt_mono_slot.argtypes = [u32, u32]
    L.pt_twin_offset.restype = C.c_uint64; L.pt_twin_offset.argtypes = [C.c_uint64, u32, u32]
    L.pt_log_route.restype = C.c_int
    L.pt_log_route.argtypes = [B, B, u32, B, u32, B, u32, B, u32, u32, u32, C.c_int, u32, B, B, u32]
    L.pt_log_route_xyz.restype = C.c_int
    L.pt_log_route_xyz.argtypes = [B, u32, B, u32, B, u32, B, u32, B, u32, u32, B, u32, u32, B, B, u32]
    L.pt_bin_accumulate.restype = C.c_int
    L.pt_bin_accumulate.argtypes = [B, B, u32, B, u32, u32]
    L.pt_bin_two_level.restype = C.c_int
    L.pt_bin_two_level.argtypes = [B, B, u32, B, u32, B, u32, B, u32, u32, u32, B, B]
    L.pt_fold.restype = C.c_int
    L.pt_fold.argtypes = [B, B, u32, u32, u32, u32, C.POINTER(C.c_float), B, B]
    L.pt_cont_reorder.restype = C.c_int
    L.pt_cont_reorder.argtypes = [B, u32, u32, B, u32, B, u32, B, B, B, u32, u32, u32, B]
    _shim = L
    return L


def const(name):
    v = shim().pt_const(name.encode())
    assert v >= 0, "the shim exports no constant " + name
    return int(v)


class Buf:
    """A C-contiguous array `a` with GUARD bytes of GUARD_BYTE before and behind it; .pt is the shim's view of it."""

    def __init__(self, a):
        a = np.ascontiguousarray(a)
        self.raw = np.full(GUARD + a.nbytes + GUARD, GUARD_BYTE, dtype=np.uint8)
        self.a = self.raw[GUARD:GUARD + a.nbytes].view(a.dtype).reshape(a.shape)
        self.a[...] = a
        self.pt = PtBuf(self.raw.ctypes.data, self.raw.nbytes, GUARD)

    def ref(self):
        return C.byref(self.pt)

    def guards_intact(self):
        return bool((self.raw[:GUARD] == GUARD_BYTE).all() and (self.raw[self.raw.nbytes - GUARD:] == GUARD_BYTE).all())


def ref_of(buf):
    return buf.ref() if buf is not None else None


# ---- index maps -------------------------------------------------------------------------------------------------------------------------

def tile_split(slot, s, t):
    """TileMap::split: slot of a plane of 1024 rows x 2^s columns -> (tile of 2^t, local)"""
    slot = np.asarray(slot, dtype=np.uint32)
    row, col = slot >> np.uint32(s), slot & np.uint32((1 << s) - 1)
    if t <= s:
        tile = (col + row) & np.uint32((1 << t) - 1)
        local = (row << np.uint32(s - t)) | (col >> np.uint32(t))
    else:
        d = t - s
        tile = ((row & np.uint32((1 << d) - 1)) << np.uint32(s)) | ((col + (row >> np.uint32(d))) & np.uint32((1 << s) - 1))
        local = row >> np.uint32(d)
    return tile.astype(np.uint32), local.astype(np.uint32)


def tile_slot_of(tile, local, s, t):
    """TileMap::slot_of, written from the description (tile = (column + row) mod T ...), not transcribed: the bijection test ties the two together"""
    tile, local = np.asarray(tile, dtype=np.int64), np.asarray(local, dtype=np.int64)
    S, T = 1 << s, 1 << t
    if t <= s:
        row, chi = local >> (s - t), local & ((1 << (s - t)) - 1)
        col = (chi << t) | ((tile - row) % T)
    else:
        d = t - s
        row = (local << d) | (tile >> s)
        col = ((tile & (S - 1)) - local) % S
    return ((row << s) | col).astype(np.uint32)


def mono_slot(pix, s):
    """MonoSlot: pixel -> slot of the plane (row = pixel mod kMonoRows, column = a multiplicative hash of pixel / kMonoRows)"""
    pix = np.asarray(pix, dtype=np.uint64)
    rows = np.uint64(1024)
    col = ((pix // rows) * np.uint64(0x9E3779B1)) & np.uint64((1 << s) - 1)
    return (((pix % rows) << np.uint64(s)) + col).astype(np.uint32)


def twin_offset(off, plane_log2, copies_log2):
    off = np.asarray(off, dtype=np.uint64)
    return ((off >> np.uint64(plane_log2 + copies_log2)) << np.uint64(plane_log2)) | (off & np.uint64((1 << plane_log2) - 1))


class Layout:
    """Which tile list a record's slot belongs to.  interleaved: `planes` planes of 1024 << s slots back to back, T interleaved tiles each
    (list = plane << t | tile); contiguous: lists of 2^tile_log2 consecutive slots."""

    def __init__(self, n_lists, s=None, t=None, tile_log2=None, interleaved=True):
        self.n_lists, self.s, self.t, self.tile_log2, self.interleaved = n_lists, s, t, tile_log2, interleaved
        self.slots_per_list = 1 << (s + 10 - t) if interleaved else 1 << tile_log2
        self.n_slots = n_lists * self.slots_per_list

    def slot(self, lst, local):
        lst, local = np.asarray(lst, dtype=np.uint32), np.asarray(local, dtype=np.uint32)
        if not self.interleaved:
            return (lst << np.uint32(self.tile_log2)) | local
        plane, tile = lst >> np.uint32(self.t), lst & np.uint32((1 << self.t) - 1)
        return (plane << np.uint32(self.s + 10)) | tile_slot_of(tile, local, self.s, self.t)

    def list_of(self, slot):
        slot = np.asarray(slot, dtype=np.uint32)
        if not self.interleaved:
            return slot >> np.uint32(self.tile_log2)
        tile, _ = tile_split(slot & np.uint32((1 << (self.s + 10)) - 1), self.s, self.t)
        return ((slot >> np.uint32(self.s + 10)) << np.uint32(self.t)) | tile


# ---- the fixed-point sums ---------------------------------------------------------------------------------------------------------------

def fix(w, frac_bits):
    """FixQ::fix: floor(float64(w) * 2^F + 0.5); NaN and negative weights (and -0.0) contribute 0"""
    v = np.asarray(w, dtype=np.float32).astype(np.float64)
    v = np.where(np.isnan(v) | (v < 0.0), 0.0, v)
    return np.floor(v * 2.0 ** frac_bits + 0.5).astype(np.uint64)


def unfix(a, frac_bits):
    """FixQ::unfix: float32(float64(uint64 sum) * 2^-F) — numpy's uint64 -> float64 rounds to nearest even, like the device's"""
    return (np.asarray(a, dtype=np.uint64).astype(np.float64) * 2.0 ** -frac_bits).astype(np.float32)


def slot_sums(slots, q, n_slots):
    """exact uint64 sum of q per slot (three 21-bit limbs through bincount: every limb sum stays far below 2^53; q < 2^63, sums < 2^64)"""
    slots = np.asarray(slots, dtype=np.int64)
    q = np.asarray(q, dtype=np.uint64)
    assert len(q) < (1 << 30) and (len(q) == 0 or int(q.max()) < (1 << 63))
    out = np.zeros(n_slots, dtype=np.uint64)
    for k in range(3):
        limb = ((q >> np.uint64(21 * k)) & np.uint64((1 << 21) - 1)).astype(np.float64)
        out += np.bincount(slots, weights=limb, minlength=n_slots).astype(np.uint64) << np.uint64(21 * k)
    return out


def expected_plane(before, slots, w, frac_bits):
    """float32(plane_before + float32(float64(sum of fix(w)) * 2^-F)) per slot"""
    before = np.asarray(before, dtype=np.float32)
    return (before + unfix(slot_sums(slots, fix(w, frac_bits), before.size), frac_bits)).astype(np.float32)


def slow_fix(w, frac_bits):
    """one weight, with Python's exact integers and fractions"""
    import math
    from fractions import Fraction
    w = float(np.float32(w))
    if math.isnan(w) or w < 0.0:
        return 0
    v = float(Fraction(w) * (1 << frac_bits) + Fraction(1, 2))   # one rounding to float64, like the device's fma
    return int(math.floor(v))


def slow_expected_plane(before, slots, w, frac_bits):
    acc = [0] * len(before)
    for s, x in zip(slots, w):
        acc[int(s)] += slow_fix(x, frac_bits)
    out = np.array(before, dtype=np.float32)
    for i, a in enumerate(acc):
        assert a < (1 << 64)
        v = np.float32(float(a) * 2.0 ** -frac_bits)   # int -> float rounds to nearest even
        out[i] = np.float32(out[i] + v)
    return out


def fix_frac_bits(max_w, m):
    """halo_backend.cpp fix_frac_bits: the largest F <= 32 with 4 x max_w x m x 2^F below 2^62"""
    import math
    _, e = math.frexp(4.0 * max(max_w, 1e-30) * float(max(m, 1)))
    return min(32, max(0, 62 - e))


# ---- weights ----------------------------------------------------------------------------------------------------------------------------

def arbitrary_weights(rng, n):
    """random float32 in (0, 1] with a sprinkling of NaN, -1, -0.0, denormals and 0"""
    w = (1.0 - rng.random(n, dtype=np.float32)).astype(np.float32)
    special = np.array([np.nan, -1.0, -0.0, 1e-40, 0.0], dtype=np.float32)
    if n:
        at = rng.choice(n, size=max(1, n // 50) if n >= 5 else 0, replace=False)
        w[at] = special[rng.integers(0, len(special), size=len(at))]
    return w


DYADIC_BITS = 12


def dyadic_weights(rng, n):
    """k * 2^-12, k in 1..255"""
    return (rng.integers(1, 256, size=n).astype(np.float32) * np.float32(2.0 ** -DYADIC_BITS)).astype(np.float32)


def dyadic_plane(rng, n):
    """non-zero starting values on the same grid"""
    return (rng.integers(1, 1000, size=n).astype(np.float32) * np.float32(2.0 ** -DYADIC_BITS)).astype(np.float32)


def assert_dyadic_exact(before, slots, w, bits=DYADIC_BITS):
    """the generated inputs keep every slot's numerator (on the 2^-bits grid) below 2^24 and its hits at most 2^12: every partial sum, in any
    order and however it is shared between the plane and its twin, is exact in fp32 and in fp64"""
    before = np.asarray(before, dtype=np.float64).ravel()
    slots = np.asarray(slots, dtype=np.int64)
    num = np.bincount(slots, weights=np.asarray(w, dtype=np.float64) * 2.0 ** bits, minlength=before.size)
    hits = np.bincount(slots, minlength=before.size)
    assert len(num) == before.size and hits.max(initial=0) <= (1 << 12), hits.max(initial=0)
    total = num + before * 2.0 ** bits
    assert (total == np.floor(total)).all() and total.max(initial=0) < (1 << 24), total.max(initial=0)


# ---- dealing records to lists and regions ------------------------------------------------------------------------------------------------

LIST_EDGES_SHORT = [0, 1, 2, 3, 2047, 2048, 2049, 8191, 8192, 8193, 8194]
LIST_EDGES_LONG = LIST_EDGES_SHORT + [65535, 65536, 65537]
REGION_COUNTS = [0, 1, 2, 16383, 16384, 16385, 32769]
CAP1 = 32784   # records per region of the log


def list_lengths(rng, n_lists, edges, at_least):
    """per-list record counts: the edges on lists spread over the range (the LAST list gets the longest edge), two more lists empty, the rest random
    so that the total is at least `at_least`"""
    assert n_lists >= len(edges) + 4
    lens = np.full(n_lists, -1, dtype=np.int64)
    where = rng.permutation(n_lists - 1)[:len(edges) + 1]
    order = list(edges[:-1])
    for i, e in zip(where[:-2], order):
        lens[i] = e
    lens[n_lists - 1] = edges[-1]
    for i in where[-2:]:
        lens[i] = 0
    free = np.flatnonzero(lens < 0)
    need = max(at_least - int(lens[lens >= 0].sum()), 0) + 4 * len(free)
    lens[free] = rng.multinomial(need, np.full(len(free), 1.0 / len(free)))
    return lens


def records_for(rng, layout, lens):
    """a shuffled array of slots with lens[l] records in list l"""
    lst = np.repeat(np.arange(layout.n_lists, dtype=np.uint32), lens)
    local = rng.integers(0, layout.slots_per_list, size=len(lst)).astype(np.uint32)
    slots = layout.slot(lst, local)
    assert (layout.list_of(slots) == lst).all()
    return slots[rng.permutation(len(slots))]


def region_fills(n, cap1, wanted=REGION_COUNTS):
    """fill counts of the log's regions for n records: the wanted counts, one region full to cap1 (reported ABOVE cap1), empty ones, the remainder"""
    fills = list(wanted) + [cap1, 0]
    left = n - sum(fills)
    assert left >= 0, "too few records for the wanted region counts"
    while left > 0:
        k = min(left, cap1 - 5)
        fills.append(k)
        left -= k
    fills.append(0)
    reported = list(fills)
    reported[len(wanted)] = cap1 + 77   # must be clamped to cap1
    return np.array(fills, dtype=np.int64), np.array(reported, dtype=np.uint32)


def deal_log(rng, x, w, cap1, fills, poison_slots):
    """the log: region r holds fills[r] records at r * cap1; what is left of every region holds poison records (a valid slot, weight 1e6)"""
    regions = len(fills)
    log = np.zeros((regions * cap1, 2), dtype=np.uint32)
    log[:, 0] = poison_slots[rng.integers(0, len(poison_slots), size=len(log))]
    log[:, 1] = np.float32(1e6).view(np.uint32)
    at = np.concatenate([r * cap1 + np.arange(f, dtype=np.int64) for r, f in enumerate(fills)]) if regions else np.zeros(0, dtype=np.int64)
    assert len(at) == len(x)
    log[at, 0] = x
    log[at, 1] = np.asarray(w, dtype=np.float32).view(np.uint32)
    return log


def counters(n, stride, values=None):
    """n counters `stride` words apart; the words between them hold POISON_U32 and must stay"""
    c = np.full(n * stride, POISON_U32, dtype=np.uint32)
    c[::stride] = 0 if values is None else values
    return c


def check_lists(list2, cnt2, cap2, stride, layout, x, w, code_mask=0xFFFFFFFF):
    """what the split pass left: every list's count is its records' number; its first min(count, cap2) entries are records of that list — all of them,
    as a multiset, when none overflowed — and everything behind is untouched"""
    n_lists = layout.n_lists
    cnt = cnt2[::stride][:n_lists].astype(np.int64)
    gaps = np.delete(cnt2[:n_lists * stride], np.arange(0, n_lists * stride, stride))
    assert (gaps == POISON_U32).all(), "a word between the list counters was written"
    lst = layout.list_of(np.asarray(x, dtype=np.uint32) & np.uint32(code_mask)).astype(np.int64)
    want = np.bincount(lst, minlength=n_lists)
    assert (cnt == want).all(), "list counts: first difference at list %d" % int(np.flatnonzero(cnt != want)[0])
    rec = list2.reshape(n_lists, cap2, 2)
    held = np.minimum(cnt, cap2)
    col = np.arange(cap2)[None, :]
    valid = col < held[:, None]
    assert (rec[~valid] == POISON_U32).all(), "an entry past a list's fill was written"
    got_list = np.broadcast_to(np.arange(n_lists)[:, None], valid.shape)[valid]
    got = rec[valid]
    assert (layout.list_of(got[:, 0] & np.uint32(code_mask)) == got_list).all(), "a record sits in another tile's list"
    key_in = (np.asarray(x, dtype=np.uint64) << np.uint64(32)) | np.asarray(w, dtype=np.float32).view(np.uint32).astype(np.uint64)
    key_out = (got[:, 0].astype(np.uint64) << np.uint64(32)) | got[:, 1].astype(np.uint64)
    if (cnt <= cap2).all():
        assert np.array_equal(np.sort(key_in), np.sort(key_out)), "the lists do not hold exactly the log's records"
    else:
        uo, co = np.unique(key_out, return_counts=True)
        ui, ci = np.unique(key_in, return_counts=True)
        pos = np.searchsorted(ui, uo)
        assert (pos < len(ui)).all() and (ui[np.minimum(pos, len(ui) - 1)] == uo).all() and (co <= ci[pos]).all(), "a list holds a record the log did not"
    return cnt
