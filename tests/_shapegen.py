"""Whole shape records of the crystal generators (halo_shapegen.hip) and of the host builder (halo_geom.h), through tests/cpp/shapegen_shim.cpp.

  build_shim() / shim()      the host-only shim (libshapegen_shim.so, linked against libhalo_hip.so) and its ctypes signatures
  SHAPE_DEV / SHAPE_PRISM    numpy structured dtypes of ShapeDev / ShapePrism (float rows as uint32: everything is compared as bits);
                             check_layout() holds them against the sizeof / offsetof the shim exports
  host_records / device_records   n records per crystal from geom::MakeShapeDev / from launch_shapegen between poisoned guard records
  live_mismatch              which records differ on their LIVE rows: the four counts, face / face_number up to face_cnt, slab (all eight words) up
                             to slab_cnt, single up to single_cnt, tri_v / tri_na / tri_face up to tri_cnt.  Rows beyond the counts are unspecified
                             by design (geom::ClearShape) and never looked at.
  slab_model                 the slab rule of halo_device.h (the comment above ShapeDev), in plain numpy, from its statement:
                                 face i pairs with the first later unpaired face whose three normal floats are its exact negatives (float
                                 comparison: -0.0 equals +0.0); the slab row is {n_i, d_i, d_mate, i, mate, 0} (ids as integer bits), rows in order
                                 of i; unpaired faces go to `single` in order of i.
  table_errors               the model against a record's own slab / single tables, and the invariants that follow from the rule
  golden_pools / fixed_crystal / jitter_crystal   the reference's 807 fixed pyramid samples (tests/golden/ref_pyramid_goldens.npz) as recipes

Everything here is numpy and ctypes; nothing needs a GPU until device_records is called.
"""
import ctypes as C
import os
import subprocess

import numpy as np

from ice_halo_sim_amd import abi, scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "ice_halo_sim_amd")
SHIM_SRC = os.path.join(ROOT, "tests", "cpp", "shapegen_shim.cpp")
SHIM_SO = os.path.join(ROOT, "tests", "cpp", "libshapegen_shim.so")
SHIM_DEPS = [SHIM_SRC] + [os.path.join(PKG, "csrc", h) for h in ("halo_launch.h", "halo_device.h", "halo_geom.h", "halo_host.hpp")] + \
            [os.path.join(ROOT, "include", "halo_trace.h")]

HIP_SUCCESS = 0
POISON_BYTE = 0xA5   # counts of 0xA5A5A5A5 are negative, floats of it are -2.87e-16: nothing a generator writes

MAX_FACES, MAX_SLABS, MAX_TRIS = 20, 10, 64
SHAPE_DEV = np.dtype([("face_cnt", "<i4"), ("tri_cnt", "<i4"), ("slab_cnt", "<i4"), ("single_cnt", "<i4"), ("face", "<u4", (MAX_FACES, 4)),
                      ("slab", "<u4", (MAX_SLABS, 8)), ("tri_v", "<u4", (MAX_TRIS, 9)), ("tri_na", "<u4", (MAX_TRIS, 4)), ("tri_face", "u1", (MAX_TRIS,)),
                      ("face_number", "u1", (MAX_FACES,)), ("single", "u1", (MAX_FACES,)), ("pad2", "u1", (8,))])
SHAPE_PRISM = np.dtype([("face_cnt", "<i4"), ("tri_cnt", "<i4"), ("slab_cnt", "<i4"), ("single_cnt", "<i4"), ("face", "<u4", (8, 4)), ("slab", "<u4", (4, 8)),
                        ("tri_v", "<u4", (20, 9)), ("tri_na", "<u4", (20, 4)), ("tri_face", "u1", (20,)), ("face_number", "u1", (8,)), ("single", "u1", (8,)),
                        ("pad", "u1", (12,))])
COUNTS = ("face_cnt", "tri_cnt", "slab_cnt", "single_cnt")
# live rows: field -> the count that bounds it
LIVE = (("face", "face_cnt"), ("face_number", "face_cnt"), ("slab", "slab_cnt"), ("single", "single_cnt"), ("tri_v", "tri_cnt"), ("tri_na", "tri_cnt"),
        ("tri_face", "tri_cnt"))


def build_shim(force=False):
    """Compile the shim the way halo_host.cpp is compiled (hipcc as a host compiler, no contraction: the host builder inside it must round like the
    library's), when it is missing or older than its sources."""
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
        raise RuntimeError("shapegen_shim.cpp failed to build:\n" + r.stdout + r.stderr)
    return SHIM_SO


_shim = None


def shim():
    global _shim
    if _shim is None:
        L = C.CDLL(build_shim())
        u32, cp = C.c_uint32, C.POINTER(abi.HaloCrystal)
        L.sg_device_count.restype = C.c_int; L.sg_device_count.argtypes = []
        L.sg_guard_records.restype = u32; L.sg_guard_records.argtypes = []
        L.sg_layout.restype = C.c_char_p; L.sg_layout.argtypes = [C.c_int]
        L.sg_host.restype = C.c_int; L.sg_host.argtypes = [cp, u32, u32, C.c_uint64, u32, C.c_int, C.c_void_p]
        L.sg_device.restype = C.c_int; L.sg_device.argtypes = [cp, u32, u32, C.c_uint64, u32, C.c_int, C.c_int, u32, C.c_void_p]
        _shim = L
    return _shim


def dtype_of(prism_records):
    return SHAPE_PRISM if prism_records else SHAPE_DEV


def cxx_layout(prism_records):
    """{member: (offset, size)} and sizeof of the C++ struct, as the shim's compiler sees it"""
    items = [x.split(":") for x in shim().sg_layout(int(bool(prism_records))).decode().split(";") if x]
    members = {i[0]: (int(i[1]), int(i[2])) for i in items if i[0] != "sizeof"}
    return members, int(dict((i[0], i[1]) for i in items)["sizeof"])


def check_layout():
    for prism in (0, 1):
        dt = dtype_of(prism)
        members, size = cxx_layout(prism)
        assert dt.itemsize == size, (prism, dt.itemsize, size)
        assert set(members) == set(dt.names), set(members) ^ set(dt.names)
        for name in dt.names:
            sub, off = dt.fields[name][:2]
            assert (off, sub.itemsize) == members[name], (prism, name, off, sub.itemsize, members[name])


def crystal_array(crystals):
    crystals = list(crystals)
    return (abi.HaloCrystal * max(len(crystals), 1))(*crystals)


def host_records(crystals, seed, first_index, n, prism_records=0):
    """records [case, k] of geom::MakeShapeDev(seed, MakeRecipe(crystal), first_index + k)"""
    crystals = list(crystals)
    out = np.zeros((len(crystals), n), dtype=dtype_of(prism_records))
    assert shim().sg_host(crystal_array(crystals), len(crystals), seed, first_index, n, int(bool(prism_records)), out.ctypes.data) == 0
    return out


def device_records(crystals, seed, first_index, n, prism_records=0, serial=0):
    """(HIP status, records [case, guard + n + guard]) as the device buffer stood after one launch_shapegen per case"""
    crystals = list(crystals)
    g = shim().sg_guard_records()
    out = np.zeros((len(crystals), n + 2 * g), dtype=dtype_of(prism_records))
    status = shim().sg_device(crystal_array(crystals), len(crystals), seed, first_index, n, int(bool(prism_records)), int(bool(serial)), POISON_BYTE, out.ctypes.data)
    return status, out


def pool_of(status, buf, n):
    """the pools [case, n] of device_records' result, with the status and the guard records in front and behind checked"""
    assert status == HIP_SUCCESS, "HIP status %d" % status
    g = shim().sg_guard_records()
    guards = np.concatenate([buf[:, :g], buf[:, g + n:]], axis=1)
    assert guards.shape[1] == 2 * g and (guards.view(np.uint8) == POISON_BYTE).all(), "a guard record was written"
    return buf[:, g:g + n]


def device_pool(crystals, seed, first_index, n, prism_records=0, serial=0):
    return pool_of(*device_records(crystals, seed, first_index, n, prism_records, serial), n)


def live_mismatch(a, b):
    """{field: indices of the records (flattened) that differ there on live rows}; empty = equal.  Counts are compared whole; a row is live by the
    counts of `b` (the expectation)."""
    a, b = np.ascontiguousarray(a).ravel(), np.ascontiguousarray(b).ravel()
    assert a.dtype == b.dtype and a.shape == b.shape
    out = {}
    for c in COUNTS:
        bad = np.flatnonzero(a[c] != b[c])
        if len(bad):
            out[c] = bad
    for field, cnt in LIVE:
        x, y = a[field], b[field]
        ne = x != y
        if ne.ndim == 3:
            ne = ne.any(axis=2)
        live = np.arange(x.shape[1])[None, :] < b[cnt][:, None]
        bad = np.flatnonzero((ne & live).any(axis=1))
        if len(bad):
            out[field] = bad
    return out


def assert_live_equal(a, b, what):
    bad = live_mismatch(a, b)
    if bad:
        k = int(min(v[0] for v in bad.values()))
        x, y = np.ravel(a)[k], np.ravel(b)[k]
        raise AssertionError("%s: records differ on live rows: %s; first record %d has counts %s, expected %s" % (
            what, {f: len(v) for f, v in bad.items()}, k, [int(x[c]) for c in COUNTS], [int(y[c]) for c in COUNTS]))


def slab_model(face, face_cnt):
    """face: uint32 [R, F, 4] face rows {nx, ny, nz, d} as bits, face_cnt: int [R].  Returns (slab uint32 [R, F // 2, 8], slab_cnt [R], single uint8 [R, F],
    single_cnt [R]) by the rule in this module's docstring; rows beyond the counts are zero."""
    face = np.ascontiguousarray(face, dtype=np.uint32)
    R, F = face.shape[:2]
    nrm = face[..., :3].view(np.float32)
    nf = np.asarray(face_cnt, dtype=np.int64)
    mate = np.full((R, F), -1, dtype=np.int64)     # mate[r, i] = j: face i is the plus face of a slab whose minus face is j
    paired = np.zeros((R, F), dtype=bool)          # face is in a slab already, on either side
    for i in range(F):
        looking = (i < nf) & ~paired[:, i]
        for j in range(i + 1, F):
            hit = looking & (j < nf) & ~paired[:, j] & (nrm[:, i, :] == -nrm[:, j, :]).all(axis=1)
            mate[hit, i] = j
            paired[hit, i] = paired[hit, j] = True
            looking &= ~hit
    plus = mate >= 0
    single_of = (np.arange(F)[None, :] < nf[:, None]) & ~paired
    slab = np.zeros((R, F // 2, 8), dtype=np.uint32)
    single = np.zeros((R, F), dtype=np.uint8)
    r, i = np.nonzero(plus)                        # row-major: in order of i within a record
    k = (np.cumsum(plus, axis=1) - 1)[r, i]
    j = mate[r, i]
    slab[r, k, 0:4] = face[r, i, 0:4]
    slab[r, k, 4] = face[r, j, 3]
    slab[r, k, 5] = i
    slab[r, k, 6] = j
    r, i = np.nonzero(single_of)
    single[r, (np.cumsum(single_of, axis=1) - 1)[r, i]] = i
    return slab, plus.sum(axis=1), single, single_of.sum(axis=1)


def table_errors(rec):
    """The slab / single tables of records `rec` against the model on their own face rows, and the derived invariants.  Returns a list of strings."""
    rec = np.ascontiguousarray(rec).ravel()
    F = rec["face"].shape[1]
    nf, ns, n1 = rec["face_cnt"].astype(np.int64), rec["slab_cnt"].astype(np.int64), rec["single_cnt"].astype(np.int64)
    errors = []
    sane = (nf >= 0) & (nf <= F) & (ns >= 0) & (ns <= F // 2) & (n1 >= 0) & (n1 <= F)
    if not sane.all():
        return ["%d records with counts out of range, first %d" % ((~sane).sum(), np.flatnonzero(~sane)[0])]
    slab, m_ns, single, m_n1 = slab_model(rec["face"], nf)
    for name, bad in (("slab_cnt", ns != m_ns), ("single_cnt", n1 != m_n1),
                      ("slab rows", ((rec["slab"] != slab).any(axis=2) & (np.arange(F // 2)[None, :] < m_ns[:, None])).any(axis=1)),
                      ("single", ((rec["single"] != single) & (np.arange(F)[None, :] < m_n1[:, None])).any(axis=1))):
        if bad.any():
            k = int(np.flatnonzero(bad)[0])
            errors.append("%s: %d records differ from the model, first %d: slab %s single %s, model slab %s single %s" % (
                name, bad.sum(), k, rec["slab"][k, :max(ns[k], 0), 5:7].tolist(), rec["single"][k, :max(n1[k], 0)].tolist(), slab[k, :m_ns[k], 5:7].tolist(),
                single[k, :m_n1[k]].tolist()))
    # the invariants, from the record's own tables alone: every face id below face_cnt exactly once over plus ids, minus ids and single
    seen = np.zeros((len(rec), 256), dtype=np.int64)
    rows = np.arange(len(rec))[:, None]
    live_s, live_1 = np.arange(F // 2)[None, :] < ns[:, None], np.arange(F)[None, :] < n1[:, None]
    for ids, live in ((rec["slab"][:, :, 5], live_s), (rec["slab"][:, :, 6], live_s), (rec["single"].astype(np.uint32), live_1)):
        if (ids[live] > 255).any():
            errors.append("a face id above 255")
            return errors
        np.add.at(seen, (np.broadcast_to(rows, ids.shape)[live], ids[live]), 1)
    want = (np.arange(256)[None, :] < nf[:, None]).astype(np.int64)
    if (seen != want).any():
        errors.append("face ids: %d records do not list every face exactly once, first %d" % ((seen != want).any(axis=1).sum(), np.flatnonzero((seen != want).any(axis=1))[0]))
    if (ns + n1 + ns != nf).any():
        errors.append("slab_cnt + single_cnt + slab_cnt != face_cnt in %d records" % (ns + n1 + ns != nf).sum())
    if (rec["slab"][:, :, 7][live_s] != 0).any():
        errors.append("a slab row's last word is not 0")
    return errors


# ---- the reference's fixed pyramid samples as recipes ----------------------------------------------------------------------------------------------
GOLDEN = os.path.join(ROOT, "tests", "golden", "ref_pyramid_goldens.npz")
POOLS = ("wc", "miller", "flat85", "flat87", "flat875", "flat88", "flat89", "flat895", "degenerate030", "degenerate050")
_pools = None


def golden_pools():
    """{pool: (params float [n, 11] = upper wedge, lower wedge (degrees), h1, h2, h3, six face distances; topology int [n, 3] = vertices, face mask,
    path tag — or None for the degenerate pools, which have no topology goldens)}; Miller rows go through scenes.miller_wedge_deg"""
    global _pools
    if _pools is None:
        G = np.load(GOLDEN)
        _pools = {}
        for name in POOLS:
            s = np.asarray(G[name + "_samples"], dtype=np.float32)
            if name == "miller":
                wedges = [[scenes.miller_wedge_deg(int(r[0]), int(r[1])), scenes.miller_wedge_deg(int(r[2]), int(r[3]))] for r in s]
                s = np.concatenate([np.asarray(wedges, dtype=np.float32), s[:, 4:]], axis=1)
            topo = np.asarray(G[name + "_topology"]) if name + "_topology" in G.files else None
            _pools[name] = (np.ascontiguousarray(s, dtype=np.float32), topo)
        assert sum(len(p) for p, _ in _pools.values()) == 807 and sum(len(t) for _, t in _pools.values() if t is not None) == 728
    return _pools


def fixed_crystal(p):
    """nine fixed scalars"""
    return scenes.pyramid_crystal(float(p[2]), float(p[3]), float(p[4]), upper_wedge=float(p[0]), lower_wedge=float(p[1]), face_distance=[float(x) for x in p[5:11]])


def jitter_crystal(p, spread=2e-4):
    """every scalar uniform with `spread` around the sample (uniform draws use no libm: host and device draw the same floats)"""
    u = lambda m: {"type": "uniform", "mean": float(m), "std": spread}
    return scenes.pyramid_crystal(u(p[2]), u(p[3]), u(p[4]), upper_wedge=float(p[0]), lower_wedge=float(p[1]), face_distance=[u(x) for x in p[5:11]])
