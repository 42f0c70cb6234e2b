"""Spectrum sessions (halo_begin_spectrum / HipTraceBackend.BeginSpectrumSession): one session for a whole list of discrete wavelengths.

The rule that makes the tests exact: root r of a crystal entry's share of m roots takes spectrum entry min(r // ceil(m / K), K - 1) — blocks of
consecutive roots, no draw, every other stream untouched.  So, with one crystal entry and ray_base = B, block k of a spectrum session IS entry
k's discrete session at ray_base B + k * per, ray for ray and bit for bit.  Tests 1-7 below are integer / byte equality; 8-10 carry bounds that
are derived where they stand (fp32 summation, the oracle's statistical bars for multi-scattering), not measured."""
import ctypes as C
import functools

import numpy as np
import pytest

from ice_halo_sim_amd import abi, scenes
from tests import _fixed_model as fm
from tests._oracle_backend import OracleBackend, run_session
from tests.test_gpu_parity import block_mean, match_exits

pytestmark = pytest.mark.gpu

SEED, RAY_BASE, PER = 11, 3 << 20, 10007
FULL = {"type": "uniform", "mean": 0.0, "std": 360.0}
WLS3 = [(420.0, 1.0), (550.0, 0.5), (680.0, 0.25)]
EXACT_FIELDS = ("dir", "weight", "root", "seq", "layer", "path_len", "path", "pixel", "crystal_id", "color_mask")


def hip_backend(**kw):
    from ice_halo_sim_amd.backend import HipTraceBackend
    return HipTraceBackend(device=0, **kw)


def _wls(pairs):
    return [scenes.wl_discrete(w, s) for w, s in pairs]


def _cmf(pairs):
    """Rows {n, weight, cmf_x, cmf_y, cmf_z} of the session's pool, from the host hook the backend itself uses (float32[K, 5])."""
    from ice_halo_sim_amd.backend import load_library
    out = np.zeros((len(pairs), 5), np.float32)
    for k, wl in enumerate(_wls(pairs)):
        assert load_library().halo_host_wl_pool(C.byref(wl), out[k].ctypes.data_as(C.POINTER(C.c_float)), 1) == 1
    return out


def _crystal(kind):
    return scenes.prism_crystal(1.0) if kind == "prism" else scenes.pyramid_crystal(0.3, 1.0, 0.2)


def _one_entry(kind="prism"):
    return scenes.scene([(0.0, [scenes.entry(_crystal(kind), scenes.axis(zenith=FULL, azimuth=FULL, roll=FULL), 1.0, 1)])], max_hits=7, sun_altitude=20.0)


def _linear():
    return scenes.render(abi.LENS_LINEAR, 128, 64, fov=90.0, el=30.0, visible=abi.VISIBLE_UPPER)


def _fisheye(w=256, h=128):
    return scenes.render(abi.LENS_FISHEYE_EQUAL_AREA, w, h, fov=180.0, el=30.0, visible=abi.VISIBLE_UPPER)


def _two_layers():
    plate = scenes.entry(scenes.prism_crystal(0.3), scenes.axis(zenith={"type": "gauss", "mean": 0, "std": 0.8}), 1.0, 6)
    col = scenes.entry(scenes.prism_crystal(1.3, [1.0] * 6), scenes.axis(zenith={"type": "uniform", "mean": 90, "std": 360}, azimuth=FULL), 1.0, 3)
    return scenes.scene([(0.5, [plate]), (0.0, [col])], max_hits=7)


def _spectrum_session(hb, scene, render, wls, n, shuffle=True):
    hb.BeginSpectrumSession(scene, render, wls, n)
    stats = []
    for li in range(scene.layer_count):
        stats.append(hb.TraceLayer(n if li == 0 else 0))
        if li + 1 < scene.layer_count:
            hb.Recombine(shuffle)
    hb.EndSession()
    return stats


def _by_key(ex):
    return ex[np.lexsort((ex["seq"], ex["root"], ex["layer"]))]


def _assert_same_records(a, b, what, fields=EXACT_FIELDS):
    assert len(a) == len(b), "%s: %d records against %d" % (what, len(a), len(b))
    for f in fields:
        x, y = np.ascontiguousarray(a[f]), np.ascontiguousarray(b[f])
        if x.dtype == np.float32:
            x, y = x.view(np.uint32), y.view(np.uint32)      # bitwise: -0.0 is not 0.0, a NaN equals itself
        bad = np.flatnonzero((x != y).reshape(len(a), -1).any(axis=1))
        assert bad.size == 0, "%s: field %s differs in %d of %d records, first: root %d seq %d: %s vs %s" % (
            what, f, bad.size, len(a), a["root"][bad[0]], a["seq"][bad[0]], a[f][bad[0]], b[f][bad[0]])


def _blocks(n, k):
    per = -(-n // k)
    return per, [max(0, min(per, n - i * per)) for i in range(k)]


# ---- the capture runs tests 3 and 8 share -----------------------------------------------------------------------------------------------------
CASES = [("prism", 3 * PER, 0), ("prism", 3 * PER, 1 << 12), ("prism", 3 * PER - 5, 1 << 12), ("pyramid", 3 * PER, 0)]


@functools.lru_cache(maxsize=None)
def _spectrum_capture(kind, n, chunk):
    hb = hip_backend(seed=SEED, capture_exits=1)
    if chunk:
        hb.set_option("chunk", chunk)
    hb.set_option("ray_base", RAY_BASE)
    st = _spectrum_session(hb, _one_entry(kind), _linear(), _wls(WLS3), n)
    ex, route = hb.DrainExits(), hb.last_route()
    img, landed = hb.ReadbackXyzAccum()
    hb.close()
    ex.setflags(write=False)
    img.setflags(write=False)
    return dict(ex=ex, img=img, landed=landed, launches=route.launches, planes=route.plane_cnt, roots=int(st[0].root_count))


# ---- 2. argument refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_argument_and_leave_the_handle_usable():
    from ice_halo_sim_amd.backend import BackendError
    sc, rd = _one_entry(), _linear()
    hb = hip_backend(seed=SEED)
    with pytest.raises(BackendError, match=r"count 0 "):
        hb.BeginSpectrumSession(sc, rd, [], 100)
    with pytest.raises(BackendError, match=r"count 256 "):
        hb.BeginSpectrumSession(sc, rd, _wls([(400.0 + k, 1.0) for k in range(256)]), 100)
    with pytest.raises(BackendError, match=r"entries\[1\].*illuminant"):
        hb.BeginSpectrumSession(sc, rd, [scenes.wl_discrete(500.0), scenes.wl_illuminant("D65", 8), scenes.wl_discrete(600.0)], 100)
    with pytest.raises(BackendError, match=r"entries is NULL"):
        hb._check(hb._L.halo_begin_spectrum(hb._h, C.byref(sc), C.byref(rd), None, 3, 100))
    # ... none of them opened a session, and the handle goes on: the largest table there is, then a discrete session
    st = _spectrum_session(hb, sc, rd, _wls([(380.0 + 1.5 * k, 1.0) for k in range(255)]), 1000)
    assert st[0].root_count == 1000
    assert run_session(hb, sc, rd, scenes.wl_discrete(550.0), 1000)[0].root_count == 1000
    hb.close()


# ---- 3. ray for ray against separate discrete sessions ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,n,chunk", CASES)
def test_blocks_are_the_discrete_sessions_ray_for_ray(kind, n, chunk):
    sp = _spectrum_capture(kind, n, chunk)
    per, sizes = _blocks(n, 3)
    assert sp["roots"] == n and sp["planes"] == 3 and sp["launches"] == (-(-n // chunk) if chunk else 1)
    got = _by_key(sp["ex"])
    assert got["root"].max() < n and len(got) > n
    np.testing.assert_array_equal(got["wl_idx"], np.minimum(got["root"] // per, 2))        # the block of every exit's root
    hb = hip_backend(seed=SEED, capture_exits=1)
    sc, rd, parts = _one_entry(kind), _linear(), []
    for k, wl in enumerate(_wls(WLS3)):
        hb.set_option("ray_base", RAY_BASE + k * per)
        assert run_session(hb, sc, rd, wl, sizes[k])[0].root_count == sizes[k]
        e = hb.DrainExits()
        assert (e["wl_idx"] == 0).all() and e["root"].max() < sizes[k]
        e["root"] += k * per
        parts.append(e)
    hb.close()
    _assert_same_records(got, _by_key(np.concatenate(parts)), "%s n %d chunk %d" % (kind, n, chunk))


def test_block_zero_against_the_oracles_discrete_session():
    """The bars test_gpu_parity.py holds a one-layer fixed prism to (its test_single_scatter_parity_all_lenses)."""
    sp = _spectrum_capture("prism", 3 * PER, 0)
    ob = OracleBackend(seed=SEED, capture_exits=1, threads=8)
    ob.set_option("ray_base", RAY_BASE)
    run_session(ob, _one_entry("prism"), _linear(), _wls(WLS3)[0], PER)
    eo = ob.DrainExits()
    ob.close()
    frac, pix, path = match_exits(sp["ex"][sp["ex"]["root"] < PER], eo)
    assert frac >= 0.998 and pix >= 0.995 and path >= 0.999, (frac, pix, path)


# ---- 4. nothing else moves ----------------------------------------------------------------------------------------------------------------------
def test_three_identical_entries_trace_the_discrete_sessions_rays_on_every_layer():
    ax = scenes.axis(zenith=FULL, azimuth=FULL, roll=FULL)
    layer0 = [scenes.entry(scenes.prism_crystal(1.0), ax, 1.0, 7), scenes.stochastic_prism_entry()]
    layer0[1].proportion = 2.0
    col = scenes.entry(scenes.prism_crystal(1.3, [1.0] * 6), scenes.axis(zenith={"type": "uniform", "mean": 90, "std": 360}, azimuth=FULL), 1.0, 3)
    sc, rd, n = scenes.scene([(0.5, layer0), (0.0, [col])], max_hits=7), _fisheye(), 30011
    runs = []
    for spectrum in (False, True):
        hb = hip_backend(seed=SEED, capture_exits=1, cont_order=1, chunk=1 << 13)
        hb.set_option("ray_base", RAY_BASE)
        if spectrum:
            st = _spectrum_session(hb, sc, rd, _wls([(550.0, 1.0)] * 3), n)
        else:
            st = run_session(hb, sc, rd, scenes.wl_discrete(550.0), n)
        runs.append(dict(ex=_by_key(hb.DrainExits()), st=[(int(s.root_count), int(s.continuation_count)) for s in st], src=hb.last_route().source_mask))
        hb.close()
    one, sp = runs
    assert one["st"] == sp["st"] and one["st"][0][0] == n and one["st"][0][1] > 0 and one["st"][1][0] == one["st"][0][1]
    assert one["src"] == sp["src"] == 0b011
    assert (sp["ex"]["layer"] == 1).sum() > 1000
    _assert_same_records(sp["ex"], one["ex"], "two layers")
    assert set(np.unique(sp["ex"]["wl_idx"])) == {0, 1, 2} and (one["ex"]["wl_idx"] == 0).all()
    # layer 1 carries the entry its root was given in layer 0: the three of them in every crystal entry's share, in block order
    from ice_halo_sim_amd.backend import load_library
    l0 = sp["ex"][sp["ex"]["layer"] == 0]
    props, carry, counts = (C.c_float * 2)(1.0, 2.0), (C.c_double * 2)(0.0, 0.0), (C.c_uint64 * 2)()
    assert load_library().halo_host_partition(props, 2, n, carry, counts) == 0
    m0 = int(counts[0])                                            # entry 0's share: roots [0, m0), entry 1's [m0, n)
    assert 0 < m0 < n and int(counts[1]) == n - m0 and (l0["crystal_id"][l0["root"] < m0] == 7).all() and (l0["crystal_id"][l0["root"] >= m0] == 1).all()
    per0, per1 = -(-m0 // 3), -(-(n - m0) // 3)
    want = np.where(l0["root"] < m0, np.minimum(l0["root"] // per0, 2), np.minimum((l0["root"].astype(np.int64) - m0) // per1, 2))
    np.testing.assert_array_equal(l0["wl_idx"], want)


# ---- 5. one entry is the discrete session ---------------------------------------------------------------------------------------------------------
def test_one_entry_is_halo_begin():
    sc, rd, n, wl = _one_entry(), _fisheye(), 1 << 16, scenes.wl_discrete(610.0, 0.75)
    out = []
    for spectrum in (False, True):
        hb = hip_backend(seed=SEED, deterministic=1)
        hb.set_option("ray_base", RAY_BASE)
        if spectrum:
            _spectrum_session(hb, sc, rd, [wl], n)
        else:
            run_session(hb, sc, rd, wl, n)
        route = bytes(hb.last_route())
        hb.sync()
        sums, f, landed_q, fl = hb.peek_fixed(0)
        img, landed = hb.ReadbackXyzAccum()
        out.append((route, sums.tobytes(), f, int(landed_q), fl, img.tobytes(), landed))
        hb.close()
    assert out[0] == out[1]
    r = abi.HaloRouteInfo.from_buffer_copy(out[1][0])
    assert r.plane_cnt == 1 and r.accum_mask == abi.ACCUM_FIXED and np.frombuffer(out[1][5], np.float32).sum() > 0


# ---- 6. deterministic spectrum sessions ---------------------------------------------------------------------------------------------------------
def _wls31():
    from ice_halo_sim_amd.backend import load_library
    lam = [380.0 + 400.0 * k / 30.0 for k in range(31)]
    spd = [load_library().halo_host_illuminant_spd(abi.ILLUM["D65"], float(x)) for x in lam]
    return [(x, s / max(spd)) for x, s in zip(lam, spd)]


def _det_run(scene, render, pairs, n, **opts):
    hb = hip_backend(seed=SEED, deterministic=1, **opts)
    hb.set_option("ray_base", RAY_BASE)
    st = _spectrum_session(hb, scene, render, _wls(pairs), n)
    r = hb.last_route()
    hb.sync()
    peeks = [hb.peek_fixed(p) for p in range(3)]
    img, landed = hb.ReadbackXyzAccum()
    hb.close()
    return dict(sums=[p[0] for p in peeks], F=peeks[0][1], landed_q=int(peeks[0][2]), FL=peeks[0][3], img=img.tobytes(), landed=landed, mask=r.accum_mask,
                planes=r.plane_cnt, launches=r.launches, st=[(int(s.root_count), int(s.continuation_count)) for s in st])


def _assert_same_integers(a, b, what):
    assert a["F"] == b["F"] and a["FL"] == b["FL"], what
    for p, (x, y) in enumerate(zip(a["sums"], b["sums"])):
        bad = np.flatnonzero(x.ravel() != y.ravel())
        assert bad.size == 0, "%s: plane %d differs in %d pixels, first %d: %d vs %d" % (what, p, bad.size, bad[0], x.ravel()[bad[0]], y.ravel()[bad[0]])
    assert a["landed_q"] == b["landed_q"] and a["img"] == b["img"] and a["landed"] == b["landed"], what


DET_PLANS = [("chunk", dict(chunk=1 << 14)), ("blocks_per_cu", dict(blocks_per_cu=1)), ("overlap", dict(overlap=0)), ("aggregate", dict(aggregate=0)),
             ("async", {"async": 1}), ("hit_log 0", dict(hit_log=0)), ("hit_log 1", dict(hit_log=1))]


@functools.lru_cache(maxsize=None)
def _det_reference():
    return _det_run(_one_entry(), _fisheye(), tuple(_wls31()), 31 * 8501)


@pytest.mark.parametrize("plan", [p[0] for p in DET_PLANS])
def test_deterministic_spectrum_does_not_depend_on_the_plan(plan):
    ref = _det_reference()
    assert ref["planes"] == 3 and ref["mask"] & abi.ACCUM_FIXED and ref["launches"] == 1
    assert all(int(s.sum(dtype=np.uint64)) > 0 for s in ref["sums"]) and ref["landed_q"] > 0
    got = _det_run(_one_entry(), _fisheye(), tuple(_wls31()), 31 * 8501, **dict(DET_PLANS)[plan])
    assert got["mask"] & abi.ACCUM_FIXED and (plan != "chunk" or got["launches"] == -(-31 * 8501 // (1 << 14)))
    assert plan != "hit_log 1" or got["mask"] == abi.ACCUM_FIXED_LOG_XYZ
    _assert_same_integers(ref, got, plan)


def test_deterministic_two_layer_spectrum_does_not_depend_on_the_plan():
    sc, rd, pairs, n = _two_layers(), _fisheye(), tuple(_wls31()), 31 * 2111
    a = _det_run(sc, rd, pairs, n, cont_order=1)
    b = _det_run(sc, rd, pairs, n, cont_order=1, chunk=1 << 12, blocks_per_cu=1, hit_log=1)
    assert a["st"] == b["st"] and a["st"][0][1] > 0 and b["launches"] > a["launches"]
    _assert_same_integers(a, b, "two layers")


def test_deterministic_planes_are_the_quantised_products_of_the_captured_rays():
    """X, Y, Z of a hit are the fp32 products cmf_c[entry] * weight, each quantised on its own (include/halo_trace.h, option "deterministic")."""
    pairs, n, rd = _wls31(), 31 * 8501, _fisheye()
    hb = hip_backend(seed=SEED, capture_exits=1)
    hb.set_option("ray_base", RAY_BASE)
    _spectrum_session(hb, _one_entry(), rd, _wls(pairs), n)
    ex = hb.DrainExits()
    hb.close()
    ref, cmf = _det_reference(), _cmf(pairs)
    np.testing.assert_array_equal(ex["wl_idx"], np.minimum(ex["root"] // 8501, 30))
    assert len(np.unique(ex["wl_idx"][ex["pixel"] >= 0])) == 31
    for c in range(3):
        v = cmf[ex["wl_idx"], 2 + c] * ex["weight"]          # float32 * float32, rounded once
        assert v.dtype == np.float32
        want = fm.plane_sums(ex["pixel"], v, rd.width * rd.height, ref["F"]).reshape(rd.height, rd.width)
        bad = np.flatnonzero(want.ravel() != ref["sums"][c].ravel())
        assert bad.size == 0, "plane %d: %d pixels differ, first %d: captured %d, plane %d" % (c, bad.size, bad[0], want.ravel()[bad[0]], ref["sums"][c].ravel()[bad[0]])
    assert ref["landed_q"] == int(fm.q(ex["weight"][ex["pixel"] >= 0], ref["FL"]).sum(dtype=np.uint64))


# ---- 7. the production routes really run ----------------------------------------------------------------------------------------------------------
WLS5 = [(440.0, 0.6), (500.0, 0.8), (560.0, 1.0), (620.0, 0.9), (680.0, 0.7)]


def _full_sky(w, h):
    return scenes.render(abi.LENS_RECTANGULAR, w, h, el=0.0, visible=abi.VISIBLE_FULL)


def test_large_spectrum_session_takes_the_xyz_hit_log():
    sc, rd, n = _one_entry(), _full_sky(1056, 512), (2 << 20) + 37
    assert rd.width * rd.height > 512 << 10
    hb = hip_backend(seed=SEED)
    st = _spectrum_session(hb, sc, rd, _wls(WLS5), n)
    r = hb.last_route()
    img, landed = hb.ReadbackXyzAccum()
    hb.close()
    assert st[0].root_count == n and r.accum_mask == abi.ACCUM_LOG_XYZ and r.plane_cnt == 3 and r.mode_mask == abi.MODE_PLAIN
    assert landed > 0.5 * n * min(s for _, s in WLS5) and img.sum() > 0
    a = _det_run(sc, rd, tuple(WLS5), n, hit_log=1)
    b = _det_run(sc, rd, tuple(WLS5), n, hit_log=0)
    assert a["mask"] == abi.ACCUM_FIXED_LOG_XYZ and b["mask"] == abi.ACCUM_FIXED
    _assert_same_integers(a, b, "hit_log 1 vs 0")


def test_very_large_spectrum_session_takes_one_plane_per_entry():
    """8 Mi roots on a small image: one scalar plane per spectrum entry.  The same rays as on X, Y, Z planes (lambda_planes = 0): equal exit and
    pixel-hit counts."""
    sc, rd, n = _one_entry(), _fisheye(), 8 << 20
    tot = []
    for lp in (-1, 0):
        hb = hip_backend(seed=SEED, lambda_planes=lp)
        st = _spectrum_session(hb, sc, rd, _wls(WLS5), n)
        r = hb.last_route()
        img, landed = hb.ReadbackXyzAccum()
        hb.close()
        assert r.plane_cnt == (len(WLS5) if lp < 0 else 3), lp
        tot.append((img.sum(axis=(0, 1), dtype=np.float64), landed, int(st[0].exit_count), int(st[0].pixel_hits)))
    assert (tot[0][0] > 0).all() and (tot[1][0] > 0).all() and tot[0][1] > 0 and tot[1][1] > 0
    assert tot[0][2] == tot[1][2] and tot[0][3] == tot[1][3]


def test_per_entry_planes_hold_each_entrys_own_light():
    """One plane per spectrum entry, folded with that entry's CMF row (lambda_planes = 1 asks for the layout at a size where the rays can be
    captured): the image against its own rays, within the bound of test 8."""
    hb = hip_backend(seed=SEED, capture_exits=1, lambda_planes=1)
    hb.set_option("ray_base", RAY_BASE)
    _spectrum_session(hb, _one_entry(), _linear(), _wls(WLS5), 5 * PER - 3)
    ex, r = hb.DrainExits(), hb.last_route()
    img, landed = hb.ReadbackXyzAccum()
    hb.close()
    assert r.plane_cnt == len(WLS5) and r.accum_mask == abi.ACCUM_SCALAR
    per = -(-(5 * PER - 3) // 5)
    np.testing.assert_array_equal(ex["wl_idx"], np.minimum(ex["root"] // per, 4))
    hit = _image_bound_check(img, ex, _cmf(WLS5), "per-entry planes")
    assert len(np.unique(hit["wl_idx"])) == 5 and landed > 0


# ---- 8. the float image against its own rays ------------------------------------------------------------------------------------------------------
def _image_bound_check(img, ex, cmf, what):
    """Each pixel channel against the float64 sum of cmf_c[entry] * w over the pixel's captured primary hits, within (n_p + 16) * 2^-23 * sum |terms|:
    the fp32 recursive-summation bound (n_p - 1) * 2^-24 * sum |terms|, in any order, with a factor 2 of slack for the rounding of each product and the fold."""
    h, w, _ = img.shape
    hit = ex[ex["pixel"] >= 0]
    n_p = np.bincount(hit["pixel"], minlength=w * h).astype(np.float64)
    for c in range(3):
        terms = cmf[hit["wl_idx"], 2 + c].astype(np.float64) * hit["weight"].astype(np.float64)
        want = np.bincount(hit["pixel"], weights=terms, minlength=w * h)
        mag = np.bincount(hit["pixel"], weights=np.abs(terms), minlength=w * h)
        err = np.abs(img[..., c].ravel().astype(np.float64) - want)
        bound = (n_p + 16.0) * 2.0 ** -23 * mag
        bad = np.flatnonzero(err > bound)
        assert bad.size == 0, "%s: channel %d, %d pixels outside the bound, first %d: image %r, rays %r, bound %r" % (
            what, c, bad.size, bad[0], img[..., c].ravel()[bad[0]], want[bad[0]], bound[bad[0]])
    return hit


@pytest.mark.parametrize("kind,n,chunk", CASES)
def test_float_image_is_the_sum_over_its_own_rays(kind, n, chunk):
    sp = _spectrum_capture(kind, n, chunk)
    hit = _image_bound_check(sp["img"], sp["ex"], _cmf(WLS3), "%s n %d chunk %d" % (kind, n, chunk))
    assert len(hit) > 1000 and len(np.unique(hit["wl_idx"])) == 3


@pytest.mark.parametrize("kind,n,chunk", CASES)
def test_landed_weight_is_the_sum_of_its_own_rays_weights(kind, n, chunk):
    """The landed weight against the float64 sum of the captured primary hits' weights, to 1e-9 relative.  The capture kernels tally the landed
    weight in fp64 from the first add (RaySums::landed64 in halo_trace.inl): what is left is the order of some thousand fp64 adds, ~1e-13.
    (The production kernels add a thread's and a wave's landed weights in fp32 and only the waves' sums in fp64: the same sessions read
    2.9e-9 .. 3.8e-9 off when the capture kernels still tallied that way.)"""
    sp = _spectrum_capture(kind, n, chunk)
    hit = sp["ex"][sp["ex"]["pixel"] >= 0]
    want = hit["weight"].astype(np.float64).sum()
    print("landed %r, rays %r, relative difference %.3e" % (sp["landed"], want, abs(sp["landed"] / want - 1.0)))
    assert sp["landed"] == pytest.approx(want, rel=1e-9)


# ---- 9. statistical parity of a multi-layer spectrum ----------------------------------------------------------------------------------------------
def test_two_layer_spectrum_against_the_oracles_three_sessions():
    """The multi-scatter bars of test_gpu_parity.py::test_multi_scatter_parity — landed weight 5e-3, 4 x 4 block-mean Pearson 0.95, channel-sum
    ratio 5 % — on X, Y and Z separately: a continuation that lost its entry would shift the channel ratios (400 nm is nearly all Z, 700 nm all X)."""
    sc = scenes.config3_scene()
    rd = scenes.render(abi.LENS_DUAL_FISHEYE_EQUAL_AREA, 512, 256, visible=abi.VISIBLE_FULL)
    pairs, per = [(400.0, 1.0), (550.0, 1.0), (700.0, 1.0)], 40_000
    hb, ob = hip_backend(seed=SEED), OracleBackend(seed=SEED, threads=8)
    st = _spectrum_session(hb, sc, rd, _wls(pairs), 3 * per)
    assert st[0].continuation_count > 0 and st[1].root_count == st[0].continuation_count
    for wl in _wls(pairs):
        run_session(ob, sc, rd, wl, per)
    ih, lh = hb.ReadbackXyzAccum()
    io, lo = ob.ReadbackXyzAccum()
    hb.close()
    ob.close()
    assert lh == pytest.approx(lo, rel=5e-3)
    a, b = block_mean(ih, 4), block_mean(io, 4)
    for c in range(3):
        assert np.corrcoef(a[..., c].ravel(), b[..., c].ravel())[0, 1] >= 0.95, c
        assert abs(ih[..., c].sum(dtype=np.float64) / io[..., c].sum(dtype=np.float64) - 1) <= 0.05, c


# ---- 10. the command-line path ----------------------------------------------------------------------------------------------------------------------
WLS9 = [(w, 1.0 - 0.05 * k) for k, w in enumerate(scenes.CONFIG_WAVELENGTHS_9)]


@functools.lru_cache(maxsize=None)
def _cli_runs():
    """run_job on a one-entry fixed-shape document, 9 wavelengths x 20 000 rays: the default path, then spectrum_session = True."""
    from ice_halo_sim_amd import cli, config
    per, rd = 20_000, _fisheye()
    job = config.TraceJob()
    job.scene, job.renders, job.wavelengths, job.ray_num = _one_entry(), {1: rd}, _wls(WLS9), 9 * per
    out = []
    for spectrum in (False, True):
        res = cli.run_job(job, seed=SEED, spectrum_session=spectrum)
        assert res["rays"] == 9 * per
        planes = res["backend"].last_route().plane_cnt
        _, xyz, total = res["backend"].Snapshot()
        res["backend"].close()
        out.append((xyz, total, planes))
    return job, rd, out


def test_cli_spectrum_session_images_are_sums_over_the_same_rays():
    job, rd, out = _cli_runs()
    assert out[0][2] == 1 and out[1][2] == 3                    # nine discrete sessions; one spectrum session on X, Y, Z planes
    # both images are sums over the SAME rays: those of a session at the counter run_job's 1024 warm-up rays leave behind, captured here
    hb = hip_backend(seed=SEED, capture_exits=1)
    hb.set_option("ray_base", 1024)
    _spectrum_session(hb, job.scene, rd, job.wavelengths, 9 * 20_000)
    ex = hb.DrainExits()
    hb.close()
    for xyz, _, _ in out:
        hit = _image_bound_check(xyz, ex, _cmf(WLS9), "cli")
        assert len(np.unique(hit["wl_idx"])) == 9


def test_cli_spectrum_session_lands_the_default_runs_weight():
    """The same rays, so the landed weight of the two runs to 1e-9 relative (production kernels: a thread and its wave add in fp32, the waves'
    sums in fp64 — nine launches and one group the same weights differently; measured 5.8e-10)."""
    _, _, out = _cli_runs()
    print("landed: default %r, spectrum session %r, relative difference %.3e" % (out[0][1], out[1][1], abs(out[1][1] / out[0][1] - 1.0)))
    assert out[1][1] == pytest.approx(out[0][1], rel=1e-9)
