"""Deterministic sessions across shards (halo_set_shard, halo_export_fixed, halo_import_fixed): N handles on device 0 trace one session's rays
between them; their exported 64-bit words, added as integers, are the one-handle run's plane sums and landed integer, and imported into one
handle they fold to its image bytes.  Every comparison is integer or byte equality — no tolerance anywhere.  One seed, one ray_base, fresh handles."""
import ctypes as C

import numpy as np
import pytest

from ice_halo_sim_amd import abi, scenes
from ice_halo_sim_amd.backend import host_shard_slice, load_library
from tests._oracle_backend import run_session

pytestmark = pytest.mark.gpu

SEED, RAY_BASE, WL = 11, 3 << 20, 550.0
FULL = {"type": "uniform", "mean": 0.0, "std": 360.0}
AX = dict(zenith=FULL, azimuth=FULL, roll=FULL)
W, H = 256, 128


def hip_backend(**kw):
    from ice_halo_sim_amd.backend import HipTraceBackend
    return HipTraceBackend(device=0, **kw)


def _prism(proportion=1.0, filter_id=0):
    return scenes.entry(scenes.prism_crystal(1.0), scenes.axis(**AX), proportion, 1, filter_id=filter_id)


def _one(*entries, hits=7):
    return scenes.scene([(0.0, list(entries))], max_hits=hits, sun_altitude=20.0)


def _fisheye(w=W, h=H):
    return scenes.render(abi.LENS_FISHEYE_EQUAL_AREA, w, h, fov=180.0, el=30.0, visible=abi.VISIBLE_UPPER)


def _families():
    """name -> scene, wl (a HaloWl, or a list = a spectrum session), n, planes, sampled (per crystal entry), options, filters."""
    pyr = scenes.entry(scenes.pyramid_crystal(0.3, 1.0, 0.2), scenes.axis(**AX), 0.3, 2)
    stoch = _one(scenes.stochastic_prism_entry(), hits=8)
    flt = [scenes.simple_filter(scenes.filter_term("raypath", raypath=[3, 5]), "PBD")]
    spectrum = [scenes.wl_discrete(l, w) for l, w in ((450.0, 1.0), (500.0, 0.8), (550.0, 1.0), (600.0, 0.9), (650.0, 0.7))]
    one = scenes.wl_discrete(WL)
    return {
        "regular prism": dict(scene=_one(_prism()), wl=one, n=(1 << 18) + 37, planes=1, sampled=[False]),
        "two entries": dict(scene=_one(_prism(0.7), pyr), wl=one, n=(1 << 17) + 5, planes=1, sampled=[False, False]),
        "sampled prisms clock 32": dict(scene=stoch, wl=one, n=(1 << 17) + 5, planes=1, sampled=[True], opts=dict(geom_clock=32)),
        "sampled prisms clock 48": dict(scene=stoch, wl=one, n=(1 << 17) + 5, planes=1, sampled=[True], opts=dict(geom_clock=48)),
        "D65": dict(scene=_one(_prism()), wl=scenes.wl_illuminant("D65", 31), n=1 << 17, planes=3, sampled=[False]),
        "spectrum of 5": dict(scene=_one(_prism()), wl=spectrum, n=(1 << 17) + 3, planes=3, sampled=[False]),
        "raypath filter": dict(scene=_one(_prism(filter_id=1)), wl=one, n=1 << 17, planes=1, sampled=[False], filters=flt),
    }


def _session(hb, scene, render, wl, n):
    if isinstance(wl, list):
        hb.BeginSpectrumSession(scene, render, wl, n)
        st = hb.TraceLayer(n)
        hb.EndSession()
        return st
    return run_session(hb, scene, render, wl, n)[0]


def _handle(f, det=1, **more):
    hb = hip_backend(seed=SEED, **dict(f.get("opts", {}), **more))
    hb.set_option("deterministic", det)
    hb.set_option("ray_base", RAY_BASE)
    hb.set_filters(list(f.get("filters", ())))
    return hb


def _shares(f):
    """The rays each crystal entry of the (one) layer gets of the session's n: the backend's partition, fresh carry."""
    L = f["scene"].layers[0]
    k = L.entry_count
    props = (C.c_float * k)(*[L.entries[i].proportion for i in range(k)])
    carry, out = (C.c_double * k)(), (C.c_uint64 * k)()
    assert load_library().halo_host_partition(props, k, f["n"], carry, out) == abi.HALO_OK
    return list(out)


def _slice_total(f, index, count):
    clock = f.get("opts", {}).get("geom_clock", 32)
    return sum(host_shard_slice(m, clock if s else 1, index, count)[1] for m, s in zip(_shares(f), f["sampled"]))


_WHOLE = {}


def _whole(name):
    """The one-handle run of a family: peeked integers, landed integer, sample counts, then the image bytes.  Traced once, shared, never changed."""
    if name not in _WHOLE:
        f = _families()[name]
        hb = _handle(f)
        st = _session(hb, f["scene"], _fisheye(), f["wl"], f["n"])
        assert int(st.root_count) == f["n"]
        route = hb.last_route()
        assert route.accum_mask & abi.ACCUM_FIXED and route.plane_cnt == f["planes"]
        peeks = [hb.peek_fixed(p) for p in range(f["planes"])]
        out = dict(sums=[p[0].copy() for p in peeks], F=peeks[0][1], landed_q=int(peeks[0][2]), FL=peeks[0][3], samples=hb.last_sample_counts())
        img, landed = hb.ReadbackXyzAccum()
        out.update(img=img.tobytes(), landed=landed)
        hb.close()
        assert out["landed_q"] > 0 and all(int(s.sum(dtype=np.uint64)) > 0 for s in out["sums"])
        _WHOLE[name] = out
    return _WHOLE[name]


def _export(hb):
    import torch
    words = torch.empty(hb.fixed_words(), dtype=torch.int64, device="cuda:0")
    layout = hb.export_fixed(words)
    return words, layout


def _trace_shards(f, count, **more):
    """The family's session on `count` sharded handles, each exported.  Returns (handles, exported tensors, layouts, root counts, sample counts)."""
    hbs, words, layouts, roots, samples = [], [], [], [], []
    for k in range(count):
        hb = _handle(f, **more)
        hb.set_shard(k, count)
        st = _session(hb, f["scene"], _fisheye(), f["wl"], f["n"])       # the WHOLE count on every shard
        roots.append(int(st.root_count))
        samples.append(hb.last_sample_counts())
        w, l = _export(hb)
        hbs.append(hb), words.append(w), layouts.append(l)
    return hbs, words, layouts, roots, samples


def _check_merge(name, count, **more):
    import torch
    f, ref = _families()[name], _whole(name)
    hbs, words, layouts, roots, samples = _trace_shards(f, count, **more)
    npix = W * H
    assert all(l == (f["planes"], ref["F"], ref["FL"]) for l in layouts), layouts
    total = torch.stack(words).sum(0)                                     # int64 adds wrap: the sum modulo 2^64
    host = total.cpu().numpy().view(np.uint64)
    for p in range(f["planes"]):
        got = host[p * npix:(p + 1) * npix].reshape(H, W)
        bad = np.flatnonzero(got.ravel() != ref["sums"][p].ravel())
        assert bad.size == 0, "%s, %d shards: plane %d differs in %d pixels, first %d" % (name, count, p, bad.size, bad[0])
    assert int(host[-1]) == ref["landed_q"], (name, count)
    assert sum(roots) == f["n"] and roots == [_slice_total(f, k, count) for k in range(count)], (name, count, roots)
    assert tuple(sum(s[i] for s in samples) for i in range(2)) == tuple(ref["samples"]), (name, count)
    # ... and a shard that has exported holds nothing: a second export has nothing pending
    from ice_halo_sim_amd.backend import BackendError
    with pytest.raises(BackendError, match="no fixed-point planes"):
        hbs[1].export_fixed(words[1])
    torch.cuda.synchronize()                                              # (the sum was made on torch's stream; the handles have their own)
    hbs[0].import_fixed(total, *layouts[0], f["n"])
    hbs[0].flush()
    img, landed = hbs[0].ReadbackXyzAccum()
    assert img.tobytes() == ref["img"], (name, count)
    assert landed == ref["landed"], (name, count)
    for hb in hbs:
        hb.close()


# ---- 1. integers and bytes, family by family ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", [2, 3, 5])
@pytest.mark.parametrize("family", sorted(_families()))
def test_shards_sum_to_the_whole_runs_integers_and_fold_to_its_bytes(family, count):
    _check_merge(family, count)


@pytest.mark.parametrize("family", ["sampled prisms clock 32", "two entries"])
def test_shards_cut_into_small_launches_through_the_hit_log_give_the_same_integers(family):
    """chunk 2^14 cuts every slice into several launches (and the slices fall inside launches of the whole plan), blocks_per_cu 1 and the forced hit
    log take other kernels and another summation order: the same integers."""
    _check_merge(family, 3, chunk=1 << 14, blocks_per_cu=1, hit_log=1)


# ---- 2. more shards than units -----------------------------------------------------------------------------------------------------------------
def test_more_shards_than_units():
    import torch
    f = dict(_families()["sampled prisms clock 32"], n=70)
    hb = _handle(f)
    assert int(_session(hb, f["scene"], _fisheye(), f["wl"], 70).root_count) == 70
    want_samples = hb.last_sample_counts()
    want_img, want_landed = hb.ReadbackXyzAccum()
    hb.close()
    hbs, words, layouts, roots, samples = _trace_shards(f, 5)
    assert roots == [0, 32, 0, 32, 6]                                    # three units of 32 rays over five shards
    for k in (0, 2):
        assert not words[k].any().item() and samples[k] == (0, 0)        # nothing traced: zeros exported, landed word included
    assert tuple(sum(s[i] for s in samples) for i in range(2)) == tuple(want_samples)
    total = torch.stack(words).sum(0)
    torch.cuda.synchronize()
    hbs[0].import_fixed(total, *layouts[0], 70)
    img, landed = hbs[0].ReadbackXyzAccum()
    assert img.tobytes() == want_img.tobytes() and landed == want_landed and want_landed > 0
    for h in hbs:
        h.close()


# ---- 3. exchange points ------------------------------------------------------------------------------------------------------------------------
def test_exchanges_where_one_handle_folds_give_its_bytes():
    import torch
    from ice_halo_sim_amd.backend import BackendError
    f = _families()["regular prism"]
    sc, rd, n = f["scene"], _fisheye(), 1 << 16
    # (weights 1.0, 0.8 and 2.0 give the landed integer the scales 27, 28 and 26: one handle converts what it holds when the scale changes)
    seq = [scenes.wl_discrete(l, w) for l, w in ((530.0, 1.0), (530.0, 1.0), (610.0, 0.8), (530.0, 2.0))]
    one = _handle(f)                                                      # default lazy_fold: folds before the third and fourth session and at the readback
    for wl in seq:
        run_session(one, sc, rd, wl, n)
    want_img, want_landed = one.ReadbackXyzAccum()
    one.close()

    hbs = [_handle(f) for _ in range(3)]
    for k, hb in enumerate(hbs):
        hb.set_shard(k, 3)
    state = dict(key=None, rays=0, exchanges=0)

    def exchange():
        parts = [_export(hb) for hb in hbs]
        total = torch.stack([w for w, _ in parts]).sum(0)
        torch.cuda.synchronize()
        hbs[0].import_fixed(total, *parts[0][1], state["rays"])
        hbs[0].flush()
        state.update(rays=0, exchanges=state["exchanges"] + 1)

    for wl in seq:                                                        # the rule of dist.ExactShardedTracer.trace_session
        key = (wl.wavelength, wl.weight, wl.illuminant, wl.pool_size, rd.width, rd.height)
        if state["rays"] and (key != state["key"] or state["rays"] + n > abi.FIX_BUDGET_RAYS):
            exchange()
        for hb in hbs:
            run_session(hb, sc, rd, wl, n)
        state.update(key=key, rays=state["rays"] + n)
    # a shard asked for its image without an exchange: refused, by name, and still usable
    for ask in (hbs[1].ReadbackXyzAccum, hbs[1].flush, hbs[1].take_landed):
        with pytest.raises(BackendError, match="halo_export_fixed"):
            ask()
    with pytest.raises(BackendError, match="halo_export_fixed"):          # ... nor does a session with other planes fold them
        hbs[2].BeginSession(sc, rd, scenes.wl_discrete(450.0), n)
    # ... nor may it start a session that changes the landed integer's scale while it holds landed weight of its own: refused before a counter moves
    hbs[1].BeginSession(sc, rd, scenes.wl_discrete(530.0, 0.8), n)
    with pytest.raises(BackendError, match="F_landed.*halo_export_fixed"):
        hbs[1].TraceLayer(n)
    hbs[1].EndSession()
    exchange()
    assert state["exchanges"] == 3
    img, landed = hbs[0].ReadbackXyzAccum()
    assert img.tobytes() == want_img.tobytes() and landed == want_landed
    for hb in hbs[1:]:                                                    # the others kept nothing
        im, l = hb.ReadbackXyzAccum()
        assert not im.any() and l == 0.0
    for hb in hbs:
        hb.close()


# ---- 4. the same rays without determinism ------------------------------------------------------------------------------------------------------
def test_float_shards_trace_exactly_the_whole_runs_rays():
    f = dict(_families()["regular prism"], n=30021)
    rd = _fisheye()

    def exits(index, count):
        hb = _handle(f, det=0, capture_exits=1)
        hb.set_shard(index, count)
        st = _session(hb, f["scene"], rd, f["wl"], f["n"])
        ex = hb.DrainExits()
        hb.close()
        return int(st.root_count), ex

    n_whole, whole = exits(0, 1)
    parts = [exits(k, 3) for k in range(3)]
    assert n_whole == 30021 and [p[0] for p in parts] == [10007, 10007, 10007]
    for k, (_, ex) in enumerate(parts):                                   # each shard's roots are its slice of the layer
        assert ex["root"].min() >= 10007 * k and ex["root"].max() < 10007 * (k + 1)
    got = np.concatenate([p[1] for p in parts])
    assert got.shape == whole.shape and whole.shape[0] > 1000
    order = lambda a: a[np.lexsort((a["seq"], a["root"]))]
    got, whole = order(got), order(whole)
    for field in whole.dtype.names:
        assert np.array_equal(got[field], whole[field]), field
    assert got.tobytes() == whole.tobytes()


# ---- 5. refusals, each by name, handle usable afterwards ---------------------------------------------------------------------------------------
def test_refusals_name_what_they_refuse_and_leave_the_handle_usable():
    import torch
    from ice_halo_sim_amd.backend import BackendError
    f = _families()["regular prism"]
    sc, rd, wl = f["scene"], _fisheye(64, 32), scenes.wl_discrete(WL)

    def covered(hb, index, count):
        """a session the handle covers, on the same handle: it traces its slice and exports"""
        assert int(run_session(hb, sc, rd, wl, 1000)[0].root_count) == host_shard_slice(1000, 1, index, count)[1]
        assert hb.last_route().accum_mask == abi.ACCUM_FIXED
        return _export(hb)

    hb = _handle(f)
    hb.BeginSession(sc, rd, wl, 1000)
    with pytest.raises(BackendError, match="halo_set_shard inside a session"):
        hb.set_shard(0, 2)
    hb.EndSession()
    for index, count in ((2, 2), (0, 0), (5, 3)):
        with pytest.raises(BackendError, match="halo_set_shard: index"):
            hb.set_shard(index, count)
    covered(hb, 0, 1)

    hb.set_shard(1, 2)
    hb.set_option("cont_order", 1)
    two = scenes.scene([(0.5, [_prism()]), (0.0, [_prism()])], max_hits=7)
    with pytest.raises(BackendError, match="halo_set_shard count > 1: a multi-layer scene"):
        hb.BeginSession(two, rd, wl, 1000)
    covered(hb, 1, 2)

    hb.BeginSession(sc, rd, wl, 4)
    rays = (np.tile([0.0, 0.0, -1.0], (4, 1)), np.zeros((4, 3)), np.ones(4), np.zeros(4, np.uint32))
    with pytest.raises(BackendError, match="halo_set_shard count > 1: host-injected rays"):
        hb.TraceLayer(host_rays=rays)
    hb.EndSession()
    covered(hb, 1, 2)

    with pytest.raises(BackendError, match="rank"):
        hb.set_option("rank", 1)
    covered(hb, 1, 2)
    hb.set_shard(0, 1)
    hb.set_option("rank", 1)
    with pytest.raises(BackendError, match="option rank"):
        hb.set_shard(1, 2)
    hb.set_option("ray_base", RAY_BASE)                                   # (takes the rank's counter range back)
    hb.set_shard(1, 2)
    covered(hb, 1, 2)

    # a sampled entry cut into launches that do not start on shapes
    g = _families()["sampled prisms clock 48"]
    hs = _handle(g, chunk=1 << 14)
    hs.set_shard(0, 2)
    hs.BeginSession(g["scene"], rd, wl, 1 << 16)
    with pytest.raises(BackendError, match="multiples of geom_clock"):
        hs.TraceLayer(1 << 16)
    hs.EndSession()
    hs.set_option("chunk", 48 << 9)
    assert int(run_session(hs, g["scene"], rd, wl, 1 << 16)[0].root_count) == host_shard_slice(1 << 16, 48, 0, 2)[1]
    hs.close()

    # export with nothing pending
    words, layout = covered(hb, 1, 2)
    with pytest.raises(BackendError, match="halo_export_fixed: no fixed-point planes are pending"):
        hb.export_fixed(words)
    fresh = _handle(f)
    with pytest.raises(BackendError, match="halo_export_fixed: no fixed-point planes are pending"):
        fresh.export_fixed(words)
    with pytest.raises(BackendError, match="halo_import_fixed"):          # no deterministic session before it
        fresh.import_fixed(words, *layout, 1000)
    fresh.close()

    # import with a layout that is not the handle's
    planes, frac, frac_landed = layout
    with pytest.raises(BackendError, match="halo_import_fixed: plane count"):
        hb.import_fixed(words, 3, frac, frac_landed, 1000)
    other = torch.zeros(3 * 64 * 32 + 1, dtype=torch.int64, device="cuda:0")
    with pytest.raises(BackendError, match="halo_import_fixed: n_words"):
        hb.import_fixed(other, planes, frac, frac_landed, 1000)
    with pytest.raises(BackendError, match=r"halo_import_fixed: frac_bits \(F\)"):
        hb.import_fixed(words, planes, frac - 1, frac_landed, 1000)
    with pytest.raises(BackendError, match=r"halo_import_fixed: landed_frac_bits"):
        hb.import_fixed(words, planes, frac, frac_landed + 1, 1000)
    # ... and past the budget of one plane set
    with pytest.raises(BackendError, match="budget of 2\\^30 rays"):
        hb.import_fixed(words, planes, frac, frac_landed, (1 << 30) + 1)
    zeros = torch.zeros_like(words)
    hb.import_fixed(zeros, planes, frac, frac_landed, (1 << 30) - 10)
    with pytest.raises(BackendError, match="budget of 2\\^30 rays"):
        hb.import_fixed(words, planes, frac, frac_landed, 11)
    hb.import_fixed(words, planes, frac, frac_landed, 10)                 # what fits is taken
    img, landed = hb.ReadbackXyzAccum()
    assert landed > 0 and img.any()
    covered(hb, 1, 2)
    hb.close()


# ---- 6. default untouched ------------------------------------------------------------------------------------------------------------------------
def test_shard_zero_of_one_is_the_default():
    f, ref = _families()["two entries"], _whole("two entries")
    hb = _handle(f)
    hb.set_shard(0, 1)
    assert int(_session(hb, f["scene"], _fisheye(), f["wl"], f["n"]).root_count) == f["n"]
    peek = hb.peek_fixed(0)
    assert np.array_equal(peek[0], ref["sums"][0]) and int(peek[2]) == ref["landed_q"] and (peek[1], peek[3]) == (ref["F"], ref["FL"])
    img, landed = hb.ReadbackXyzAccum()                                   # one shard of one folds its own planes, as ever
    assert img.tobytes() == ref["img"] and landed == ref["landed"]
    hb.close()


# ---- 7. dist.ExactShardedTracer on one device: landed scales and the budget -------------------------------------------------------------------------
def _tracer_against_one_handle(sessions, scene, **opts):
    """`sessions` = [(HaloWl, n)] through ExactShardedTracer (one rank: it exports, imports and folds its own words) and on one plain handle."""
    from ice_halo_sim_amd.dist import ExactShardedTracer
    rd = _fisheye(64, 32)
    one = hip_backend(seed=SEED, **opts)
    one.set_option("deterministic", 1)
    one.set_option("ray_base", RAY_BASE)
    for wl, n in sessions:
        run_session(one, scene, rd, wl, n)
    want_img, want_landed = one.ReadbackXyzAccum()
    one.close()
    tr = ExactShardedTracer(scene, rd, seed=SEED, device=0, rank=0, world=1, ray_base=RAY_BASE, **opts)
    for wl, n in sessions:
        assert int(tr.trace_session(wl, n).root_count) == n
    img, landed = tr.readback()
    tr.backend.close()
    assert img.tobytes() == want_img.tobytes() and landed == want_landed and landed > 0
    return tr.exchanges


def test_tracer_carries_the_landed_weight_across_scales():
    """Sessions of weights 1.0, 0.8, 2.0, 2.0, 1.0: F_landed 27, 28, 26, 26, 27.  The imported landed integer is converted where one handle converts
    its own, the export leaves that double with the handle: bytes and landed weight of the one-handle run."""
    from ice_halo_sim_amd.backend import host_fixed_frac_bits
    assert [host_fixed_frac_bits(w, 1 << 32) for w in (1.0, 0.8, 2.0)] == [27, 28, 26]
    f = _families()["two entries"]
    sessions = [(scenes.wl_discrete(l, w), (1 << 15) + 3) for l, w in ((530.0, 1.0), (610.0, 0.8), (450.0, 2.0), (450.0, 2.0), (530.0, 1.0))]
    assert _tracer_against_one_handle(sessions, f["scene"]) == 4


def test_tracer_exchanges_where_the_budget_makes_one_handle_fold():
    """Four sessions of 2^28 rays fill the 2^30-ray budget of one plane set; one handle folds before the launch of the fifth, the tracer exchanges
    before the fifth session.  A session of several launches that would straddle the budget is refused."""
    from ice_halo_sim_amd.dist import ExactShardedTracer
    f = _families()["regular prism"]
    wl = scenes.wl_discrete(WL)
    sessions = [(wl, 1 << 28)] * 4 + [(wl, 1 << 16)]
    assert _tracer_against_one_handle(sessions, f["scene"], hit_log=0) == 2
    two = _families()["two entries"]
    tr = ExactShardedTracer(two["scene"], _fisheye(64, 32), seed=SEED, device=0, rank=0, world=1, ray_base=RAY_BASE)
    tr._rays, tr._key = (1 << 30) - 100, tr._session_key(wl)              # (as after sessions of that many rays)
    with pytest.raises(ValueError, match="straddle"):
        tr.trace_session(wl, 1000)
    tr.backend.close()
