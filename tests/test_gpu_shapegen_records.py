"""The device crystal generators (halo_shapegen.hip) held to WHOLE records: every live row of what launch_shapegen leaves in the pool — counts, faces,
face numbers, the slab and single tables the next-face search walks, fan triangles — against the host builder (geom::MakeShapeDev) bit for bit,
and the slab / single tables against a plain model of the slab rule (tests/_shapegen.py, proved on the CPU by tests/test_shapegen_model.py).

  reference pools, fixed      the reference's 807 fixed pyramid samples as recipes of nine fixed scalars, n = 9 (one live team and seven dead ones in
                              the last block), both pyramid routes (team kernel, serial kernel); the reference's topology goldens where it has them
  reference pools, jittered   every scalar uniform with spread 2e-4 around the sample, 16 shapes from index 2^32 - 8 (the index carries into its
                              high word inside the launch); no empty record, nothing beyond 20 faces / 44 triangles / 10 slabs (ShapeSlot48 stages
                              48 triangle rows: stage_shape's clamp never bites)
  prisms                      uniform, wild (sides vanish: single faces) and sync-group recipes on the ShapePrism team kernel, the ShapePrism
                              serial kernel and the ShapeDev serial kernel
  launch edges                n around the team, block and wave sizes between poisoned guard records; n = 0 touches nothing
  refused recipes             illegal wedges, vanishing heights: counts and live rows are the host's, an empty crystal is four zero counts
  hard pyramids, traced       four reference samples through the pool trace kernels against the one-shape kernel, ray by ray

The pool is NOT cleared before a launch (production does not either: tests/cpp/shapegen_shim.cpp), so a row a generator should have written and
did not shows as poison.  Rows beyond the counts are unspecified by design and never compared.

Shown once on a scratch build that these tests see a wrong table: with r[3] and r[4] (d_plus / d_minus) exchanged in the team kernel's slab row, all 28
"team" cases of the reference-pool, launch-edge (n >= 1) and refused-recipe tests failed, on the slab rows against the host AND against the model; the
38 serial and prism cases passed.
"""
import ctypes as C

import numpy as np
import pytest

from ice_halo_sim_amd import abi, backend, scenes
from tests import _shapegen as SG
from tests.test_gpu_parity import block_mean, hip_backend, match_exits, rel_l2
from tests._oracle_backend import run_session

pytestmark = pytest.mark.gpu

SEED = 1234
ROUTES = {"team": 0, "serial": 1}   # launch_shapegen's serial_pyramid
CARRY = 2**32 - 8                   # 16 shapes from here: eight below 2^32, eight above


def popcount(x):
    return bin(int(x)).count("1")


def assert_records(dev, host, what):
    """live rows against the host builder AND the slab / single tables against the model: both judged before either fails, so a wrong table
    shows under both"""
    bad = {f: len(v) for f, v in SG.live_mismatch(dev, host).items()}
    errors = SG.table_errors(dev)
    assert not bad and not errors, "%s: records that differ from the host's on live rows, by field: %s; against the model: %s" % (what, bad, errors)


@pytest.mark.parametrize("route", sorted(ROUTES))
@pytest.mark.parametrize("pool", SG.POOLS)
def test_reference_pools_fixed(pool, route):
    params, topo = SG.golden_pools()[pool]
    crystals = [SG.fixed_crystal(p) for p in params]
    n = 9
    host = SG.host_records(crystals, SEED, 0, n)
    dev = SG.device_pool(crystals, SEED, 0, n, serial=ROUTES[route])
    assert_records(dev, host, "%s, %s" % (pool, route))
    if topo is not None:
        dropped = 0
        for k, t in enumerate(topo):
            vertices, mask, tag = int(t[0]), int(t[1]), int(t[2])
            if tag & 0x40:   # the reference's own marker that its result lost a face (tests/test_host_tables.py): here the face must be there
                dropped += 1
                assert (dev["face_cnt"][k] > popcount(mask)).all(), (pool, k)
            else:
                assert (dev["face_cnt"][k] == popcount(mask)).all() and (dev["tri_cnt"][k] == 2 * vertices - 4).all(), (pool, k, dev["face_cnt"][k], dev["tri_cnt"][k], t)
        assert dropped == (1 if pool == "flat895" else 0)


@pytest.mark.parametrize("route", sorted(ROUTES))
@pytest.mark.parametrize("pool", SG.POOLS)
def test_reference_pools_jittered_across_the_index_carry(pool, route):
    params, _ = SG.golden_pools()[pool]
    crystals = [SG.jitter_crystal(p) for p in params]
    n = 16
    host = SG.host_records(crystals, SEED, CARRY, n)
    dev = SG.device_pool(crystals, SEED, CARRY, n, serial=ROUTES[route])
    assert_records(dev, host, "%s, %s" % (pool, route))
    assert (dev["face_cnt"] >= 4).all() and (dev["tri_cnt"] >= 4).all(), "an empty record"
    assert (dev["tri_cnt"] <= 44).all() and (dev["face_cnt"] <= 20).all() and (dev["slab_cnt"] <= 10).all()
    # the draws differ from shape to shape, across the carry too: the records are not one record sixteen times
    assert (dev["face"][:, 7, 0, 3] != dev["face"][:, 8, 0, 3]).any()


def prism_recipes():
    u = lambda m, s: {"type": "uniform", "mean": m, "std": s}
    return {"uniform": scenes.prism_crystal(u(1.0, 1.2), [u(1.0, 0.9)] * 6),
            "wild": scenes.prism_crystal(u(0.4, 0.6), [u(0.9, 1.8)] * 6),   # sides vanish
            "sync": scenes.prism_crystal(u(1.0, 0.5), [u(1.0, 0.8)] * 6, sync_group=[0, 0, 0, 1, 2, 1, 2, 1, 2])}


# (prism_records, serial): the ShapePrism team kernel, the ShapePrism serial kernel, the ShapeDev serial kernel
PRISM_ROUTES = {"prism_team": (1, 0), "prism_serial": (1, 1), "general_serial": (0, 1)}


@pytest.mark.parametrize("route", sorted(PRISM_ROUTES))
def test_prism_records(route):
    prism_records, serial = PRISM_ROUTES[route]
    names = sorted(prism_recipes())
    crystals = [prism_recipes()[k] for k in names]
    n, first = 400, 2**32 - 250
    host = SG.host_records(crystals, SEED, first, n, prism_records)
    dev = SG.device_pool(crystals, SEED, first, n, prism_records, serial)
    assert_records(dev, host, route)
    wild = dev[names.index("wild")]
    assert (wild["single_cnt"] > 0).sum() >= 20 and (wild["face_cnt"] == 8).any()   # sides vanish: faces without an opposite
    assert (dev[names.index("uniform")]["slab_cnt"] == 4).any()


@pytest.mark.parametrize("route", sorted(ROUTES))
@pytest.mark.parametrize("n", [0, 1, 7, 8, 9, 63, 64, 65])
def test_launch_edges_pyramid(n, route):
    u = lambda m, s: {"type": "uniform", "mean": m, "std": s}
    cr = scenes.pyramid_crystal(u(0.3, 0.4), u(1.0, 0.8), u(0.3, 0.4), face_distance=[u(1.0, 0.5)] * 6)
    check_launch_edge([cr], n, 0, ROUTES[route])


@pytest.mark.parametrize("n", [0, 1, 15, 16, 17])
def test_launch_edges_prism_team(n):
    check_launch_edge([prism_recipes()["uniform"], prism_recipes()["wild"]], n, 1, 0)


def check_launch_edge(crystals, n, prism_records, serial):
    status, buf = SG.device_records(crystals, SEED, CARRY, n, prism_records, serial)
    assert status == SG.HIP_SUCCESS
    g = SG.shim().sg_guard_records()
    assert buf.shape == (len(crystals), n + 2 * g)
    if n == 0:
        assert (buf.view(np.uint8) == SG.POISON_BYTE).all()   # success, and nothing touched
        return
    pool = SG.pool_of(status, buf, n)   # (checks the guard records in front and behind)
    host = SG.host_records(crystals, SEED, CARRY, n, prism_records)
    SG.assert_live_equal(pool[:, :1], host[:, :1], "record 0, n = %d" % n)   # whatever the number of dead teams that alias it
    assert_records(pool, host, "n = %d" % n)


REFUSED = {   # (upper wedge, lower wedge, h1, h2, h3): what is left of the crystal
    "upper_wedge_0.05": (0.05, 28.0, 0.3, 1.0, 0.3),
    "lower_wedge_89.95": (28.0, 89.95, 0.3, 1.0, 0.3),
    "h1_0": (28.0, 28.0, 0.0, 1.0, 0.3),
    "h3_0": (28.0, 28.0, 0.3, 1.0, 0.0),
    "all_heights_0": (28.0, 28.0, 0.0, 0.0, 0.0),
}


@pytest.mark.parametrize("route", sorted(ROUTES))
def test_refused_and_half_refused_recipes(route):
    names = sorted(REFUSED)
    u = lambda m: {"type": "uniform", "mean": m, "std": 0.2}
    crystals = [scenes.pyramid_crystal(r[2], r[3], r[4], upper_wedge=r[0], lower_wedge=r[1], face_distance=[u(1.0)] * 6) for r in (REFUSED[k] for k in names)]
    n = 9
    host = SG.host_records(crystals, SEED, CARRY, n)
    dev = SG.device_pool(crystals, SEED, CARRY, n, serial=ROUTES[route])
    assert_records(dev, host, route)
    for k, name in enumerate(names):
        counts = np.stack([dev[k][c] for c in SG.COUNTS])
        if name == "all_heights_0":
            assert (counts == 0).all() and all((host[k][c] == 0).all() for c in SG.COUNTS)   # the empty crystal: four zero counts on both sides
        else:   # one cone gone (its face numbers 13..18 / 23..28 do not appear), the prism and the other cone stay
            gone = range(13, 19) if name in ("upper_wedge_0.05", "h1_0") else range(23, 29)
            for r in dev[k]:
                numbers = set(r["face_number"][:r["face_cnt"]].tolist())
                assert r["face_cnt"] >= 8 and not numbers & set(gone) and numbers & set(range(13, 29)), (name, sorted(numbers))


# ---- hard pyramids through the trace kernels --------------------------------------------------------------------------------------------------------
# (pool, index): 20 faces / 44 fan triangles with unequal cones; a 89.5-degree flat tail whose equal cones pair up across the crystal (10 slabs);
# a Miller sample with unequal cones (wedges 28.0 over 14.9 degrees: 19 faces, 13 of them single); a sample of the reference's degenerate050 pool
TRACED = {"tri44": ("wc", 17), "flat895": ("flat895", 1), "miller_unequal": ("miller", 9), "degenerate050": ("degenerate050", 0)}


@pytest.mark.parametrize("case", sorted(TRACED))
def test_hard_pyramid_pool_route_equals_the_one_shape_route(case):
    """tests/test_gpu_parity.py::test_pool_path_with_frozen_geometry_equals_the_one_shape_path on the reference's hard pyramids: the fixed crystal
    takes the one-shape kernel with the host builder's tables, the same crystal with gauss(d, 1e-7) face distances the device generator, the pool
    and the pool trace kernels with their slab walk.  Same ray streams: the same exits ray for ray, up to the 1e-7 wobble."""
    pool, index = TRACED[case]
    p = SG.golden_pools()[pool][0][index]
    fixed = SG.fixed_crystal(p)
    frozen = scenes.pyramid_crystal(float(p[2]), float(p[3]), float(p[4]), upper_wedge=float(p[0]), lower_wedge=float(p[1]),
                                    face_distance=[{"type": "gauss", "mean": float(x), "std": 1e-7} for x in p[5:11]])
    # the sample was chosen so that the wobble does not change its topology: held here for the first 16 draws, on the CPU
    L = backend.load_library()
    f32p = C.POINTER(C.c_float)

    def counts(sc):
        g = abi.HaloGeomTables()
        dist = np.ascontiguousarray(sc[3:9], dtype=np.float32)
        L.halo_host_pyramid_geometry(fixed.wedge_upper_deg, fixed.wedge_lower_deg, abs(float(sc[0])), abs(float(sc[1])), abs(float(sc[2])), dist.ctypes.data_as(f32p), C.byref(g))
        return g.face_cnt, g.tri_cnt

    want = counts(np.asarray(p[2:11], dtype=np.float32))
    assert want[0] >= 4
    if case == "tri44":
        assert want == (20, 44)
    for idx in range(16):
        sc = np.zeros(9, np.float32)
        assert L.halo_host_shape_scalars(C.byref(frozen), 47, idx, 0, sc.ctypes.data_as(f32p)) == 0
        assert counts(sc) == want, (case, idx)
    full = {"type": "uniform", "mean": 0.0, "std": 360.0}
    ax = scenes.axis(zenith=full, azimuth=full, roll=full)
    rd = scenes.render(abi.LENS_DUAL_FISHEYE_EQUAL_AREA, 512, 256, visible=abi.VISIBLE_FULL)
    out = []
    for cr in (fixed, frozen):
        hb = hip_backend(seed=47, capture_exits=1)
        run_session(hb, scenes.scene([(0.0, [scenes.entry(cr, ax, 1.0, 1)])], max_hits=6), rd, scenes.wl_discrete(550.0), 150_000)
        ex = hb.DrainExits()
        img, landed = hb.ReadbackXyzAccum()
        hb.close()
        out.append((ex, img, landed))
    frac, pix, path = match_exits(out[1][0], out[0][0])
    print("%s: matched %.5f, same pixel %.5f, same path %.5f, landed %.6g against %.6g, block-mean rel L2 %.3e" % (
        case, frac, pix, path, out[1][2], out[0][2], rel_l2(block_mean(out[1][1]), block_mean(out[0][1]))))
    assert len(out[0][0]) > 100_000
    assert frac >= 0.995 and pix >= 0.99 and path >= 0.997
    assert out[1][2] == pytest.approx(out[0][2], rel=2e-3)
