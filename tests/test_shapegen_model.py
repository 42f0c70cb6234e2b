"""The numpy model of the slab rule (tests/_shapegen.py slab_model) proved on the CPU before it judges the device generators
(tests/test_gpu_shapegen_records.py): against hand-made face tables whose pairing is written out here, and against the host builder's records
(geom::FinalizeSlabs through geom::MakeShapeDev) of the reference's 807 fixed pyramid samples.  Also the shim's layout check: the numpy dtypes of
ShapeDev / ShapePrism against the C++ sizeof / offsetof."""
import numpy as np

from tests import _shapegen as SG

S3 = np.float32(0.86602540378443864676)
SIDES = [(1.0, 0.0), (0.5, S3), (-0.5, S3), (-1.0, 0.0), (-0.5, -S3), (0.5, -S3)]


def faces(rows, width=8):
    """[R = 1, width, 4] uint32 from a list of (nx, ny, nz, d)"""
    f = np.zeros((1, width, 4), dtype=np.float32)
    f[0, :len(rows)] = np.asarray(rows, dtype=np.float32)
    return f.view(np.uint32), np.array([len(rows)])


def model(rows, width=8):
    slab, ns, single, n1 = SG.slab_model(*faces(rows, width))
    pairs = [(int(r[5]), int(r[6])) for r in slab[0, :ns[0]]]
    return slab[0, :ns[0]], pairs, single[0, :n1[0]].tolist()


def prism_rows(present=range(6)):
    return [(0, 0, 1, -0.5), (0, 0, -1, -0.6)] + [(SIDES[i][0], SIDES[i][1], 0, -0.4 - 0.01 * i) for i in present]


def test_layout_of_the_numpy_records_is_the_cxx_layout():
    SG.check_layout()
    assert SG.SHAPE_DEV.itemsize == 4096 and SG.SHAPE_PRISM.itemsize == 1360


def test_model_on_hand_made_face_tables():
    # a full prism: basal pair, sides i / i + 3 — 4 slabs, no single face
    slab, pairs, single = model(prism_rows())
    assert pairs == [(0, 1), (2, 5), (3, 6), (4, 7)] and single == []
    rows = np.asarray(prism_rows(), dtype=np.float32)
    for r, (i, j) in zip(slab, pairs):   # {n_i, d_i, d_mate, i, mate, 0}
        assert r[:4].tobytes() == rows[i].tobytes() and r[4:5].tobytes() == rows[j, 3:4].tobytes() and r[7] == 0
    # side 1 gone: its opposite (side 4, now face 5) is single; ids are compact
    slab, pairs, single = model(prism_rows([0, 2, 3, 4, 5]))
    assert pairs == [(0, 1), (2, 4), (3, 6)] and single == [5]
    # two faces with equal normals: the first takes the one opposite, the second stays single; and two candidates for one face: the FIRST later one
    assert model([(1, 0, 0, -1), (1, 0, 0, -2), (-1, 0, 0, -3)])[1:] == ([(0, 2)], [1])
    assert model([(1, 0, 0, -1), (-1, 0, 0, -2), (-1, 0, 0, -3)])[1:] == ([(0, 1)], [2])
    assert model([(1, 0, 0, -1), (1, 0, 0, -2), (-1, 0, 0, -3), (-1, 0, 0, -4)])[1:] == ([(0, 2), (1, 3)], [])
    # -0.0 against +0.0: float comparison, so (+0, +0, 1) and (+0, +0, -1) are opposite although the bits of -(+0) and +0 differ
    assert model([(0.0, 0.0, 1, -1), (0.0, 0.0, -1, -1)])[1:] == ([(0, 1)], [])
    assert model([(-0.0, 0.0, 1, -1), (-0.0, -0.0, -1, -1)])[1:] == ([(0, 1)], [])
    # a normal that differs in its last bit is not opposite
    assert model([(1, 0, 0, -1), (np.nextafter(np.float32(-1), np.float32(0)), 0, 0, -1)])[1:] == ([], [0, 1])
    # nothing beyond face_cnt is looked at
    f, _ = faces([(1, 0, 0, -1), (-1, 0, 0, -1)])
    slab, ns, single, n1 = SG.slab_model(f, np.array([1]))
    assert (int(ns[0]), int(n1[0]), int(single[0, 0])) == (0, 1, 0)
    # several records at once: each by its own count
    f2 = np.concatenate([faces(prism_rows())[0], faces(prism_rows([0, 2, 3, 4, 5]))[0]])
    slab, ns, single, n1 = SG.slab_model(f2, np.array([8, 7]))
    assert ns.tolist() == [4, 3] and n1.tolist() == [0, 1] and single[1, 0] == 5 and slab[1, 1, 5:7].tolist() == [2, 4]


def test_table_errors_sees_a_wrong_table():
    rec = np.zeros(1, dtype=SG.SHAPE_PRISM)
    f, _ = faces(prism_rows([0, 2, 3, 4, 5]))
    rec["face"], rec["face_cnt"] = f, 7
    slab, ns, single, n1 = SG.slab_model(f, np.array([7]))
    rec["slab"], rec["slab_cnt"], rec["single"], rec["single_cnt"] = slab[:, :4], ns, single, n1
    assert SG.table_errors(rec) == []
    for field, at, value in (("slab", (0, 1, 6), 2), ("slab", (0, 1, 5), 4), ("single", (0, 0), 6), ("slab_cnt", (0,), 2), ("slab", (0, 2, 7), 1)):
        bad = rec.copy()
        bad[field][at] = value
        assert SG.table_errors(bad), (field, at)
    swapped = rec.copy()   # d_plus / d_minus exchanged
    swapped["slab"][0, 1, 3], swapped["slab"][0, 1, 4] = rec["slab"][0, 1, 4], rec["slab"][0, 1, 3]
    assert SG.table_errors(swapped)


def test_model_equals_the_host_builder_on_the_reference_pools():
    """All 807 samples as recipes of nine fixed scalars through geom::MakeShapeDev: none is empty, the tables stay inside what the kernels' slots
    hold, and the host's slab / single tables are the model's."""
    total, most = 0, dict.fromkeys(SG.COUNTS, 0)
    for name, (params, _) in SG.golden_pools().items():
        rec = SG.host_records([SG.fixed_crystal(p) for p in params], 1234, 0, 1).ravel()
        total += len(rec)
        assert (rec["face_cnt"] >= 4).all() and (rec["tri_cnt"] >= 4).all(), name
        assert (rec["face_cnt"] <= 20).all() and (rec["tri_cnt"] <= 44).all() and (rec["slab_cnt"] <= 10).all(), name
        assert SG.table_errors(rec) == [], name
        for c in SG.COUNTS:
            most[c] = max(most[c], int(rec[c].max()))
    assert total == 807
    assert most["face_cnt"] == 20 and most["tri_cnt"] == 44   # the pools reach the full solid: 20 faces, 24 corners
    assert most["slab_cnt"] >= 4 and most["single_cnt"] >= 1   # both tables are exercised


def test_shim_host_builder_is_the_librarys():
    """The shim compiles halo_geom.h itself; its records must be the ones libhalo_hip.so's own host builder makes (halo_host_pyramid_geometry: faces
    and triangles — the library hands out no more), bit for bit, or the GPU tests would hold the device to a third builder."""
    import ctypes as C
    from ice_halo_sim_amd import abi, backend
    L = backend.load_library()
    for name, (params, _) in SG.golden_pools().items():
        rec = SG.host_records([SG.fixed_crystal(p) for p in params], 99, 5, 1).ravel()
        for p, r in zip(params, rec):
            g = abi.HaloGeomTables()
            L.halo_host_pyramid_geometry(*[float(x) for x in p[:5]], np.ascontiguousarray(p[5:11]).ctypes.data_as(C.POINTER(C.c_float)), C.byref(g))
            nf, nt = g.face_cnt, g.tri_cnt
            assert (nf, nt) == (int(r["face_cnt"]), int(r["tri_cnt"])), name
            face = np.concatenate([np.frombuffer(g.face_n, np.uint32).reshape(-1, 3)[:nf], np.frombuffer(g.face_d, np.uint32)[:nf, None]], axis=1)
            tri_na = np.concatenate([np.frombuffer(g.tri_n, np.uint32).reshape(-1, 3)[:nt], np.frombuffer(g.tri_area, np.uint32)[:nt, None]], axis=1)
            assert (face == r["face"][:nf]).all() and (tri_na == r["tri_na"][:nt]).all(), name
            assert (np.frombuffer(g.tri_v, np.uint32).reshape(-1, 9)[:nt] == r["tri_v"][:nt]).all(), name
            assert list(g.face_number[:nf]) == r["face_number"][:nf].tolist() and list(g.tri_face[:nt]) == r["tri_face"][:nt].tolist(), name
