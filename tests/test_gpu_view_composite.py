"""halo_consumer_view_composite and halo_consumer_view_lanes — the class composite and the class lanes through any lens — on the device.

No ray is traced: lanes come in through halo_consumer_load_lanes (float -> double -> float is exact), classes through halo_set_color.  S is
halo_consumer_composite's srgb_out of the same lanes on the same handle; the geometry reference is halo_consumer_view_filtered on a handle whose
consumer holds a zero image of the source's size.  Per (source, view) pair of tests/_view_filter_model.py:
  1. nearest, no blend: srgb_view[p] == S[map[p]] byte for byte, (0, 0, 0) elsewhere; p99 and produced are the composite call's; map and tap are
     halo_consumer_view_filtered's, bit for bit;
  2. quantisation: srgb_out == floor(float32(value_out) + float32(0.5)), evaluated in fp32, on every pixel, under every filter;
  3. values: value_out against _view_filter_model.view64(S as float32, the device's own tap, ...), |delta| <= BAR x the largest tap value — the
     three-lerp-and-blend chain that bar was derived for (_view_filter_model.py), on taps that are bytes (BAR is 8 x 2^-24; measured on an
     MI355X: 2.25 x 2^-24 for the composite, 2.53 x 2^-24 for the lanes);
  4. exact anchors: constant lanes, the two constants across a dual source's band (fma(t, b - a, a) to the bit), a single lit source pixel;
  5. the lanes view: nearest is the loaded lane at map, bilinear and the blend against view64 per class, class counts 1, 3 and 16;
  6. the three cases that stop before a composite; 7. the refusals by name; 8. the Python wrappers, the CLI and a C++ host program."""
import ctypes as C
import functools
import json
import os
import subprocess

import numpy as np
import pytest

from ice_halo_sim_amd import abi, scenes
from tests import _lens_model as lm
from tests import _view_filter_model as fm
from tests import _view_model as vm

pytestmark = pytest.mark.gpu
F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCES = fm.sources()
IDS = [s[0] for s in SOURCES]
COMBOS = (("nearest", False), ("nearest", True), ("bilinear", False), ("bilinear", True))
ALL4 = ("srgb", "value", "map", "tap")
TOTAL = 1000.0
_handles = {}


def handle(key):
    if key not in _handles:
        from ice_halo_sim_amd.backend import HipTraceBackend
        _handles[key] = HipTraceBackend(device=0, seed=5)
    return _handles[key]


@pytest.fixture(scope="module", autouse=True)
def _close_handles():
    yield
    for hb in _handles.values():
        hb.close()
    _handles.clear()


def pairs_of(sid):
    return [(vid, view) for s2, _, vid, view in fm.gpu_pairs() if s2 == sid]


def has_band(src):
    return lm.proj_of(src).mad > 0.0


def bit_classes(n, bits=True):
    return [scenes.color_class([c] if bits else []) for c in range(n)]


def display(n, solo=(), hidden=(), z=None):
    g = np.random.default_rng(100 + n)
    cols = g.uniform(0.1, 1.0, (n, 3)).round(3)
    return [{"color": tuple(float(v) for v in cols[c]), "visible": c not in hidden, "solo": c in solo, "z_order": c if z is None else z[c]} for c in range(n)]


def random_lanes(n, src, seed=3):
    """Lanes over four decades with a fifth of the pixels dark: the composite holds bytes from 0 to 255."""
    g = np.random.default_rng(seed)
    v = 10.0 ** g.uniform(-3.0, 1.0, (n, src.height, src.width))
    return np.ascontiguousarray((v * (g.random((n, src.height, src.width)) > 0.2)).astype(F32))


def load(hb, lanes, total=TOTAL, bits=True):
    hb.set_color([], bit_classes(len(lanes), bits))
    hb.LoadClassLanes(lanes, total)
    return lanes


def drained(hb, like):
    """halo_readback_class_lanes: the device lanes as floats (the call zeroes them: the last thing a test does with its lanes)."""
    out = np.zeros_like(like)
    n, h, w = like.shape
    hb._check(hb._L.halo_readback_class_lanes(hb._h, out.ctypes.data_as(C.POINTER(C.c_float)), w, h, n))
    return out


def composite(hb, disp, mode, scale=1.0, intensity=1.0):
    """halo_consumer_composite on the handle: (produced, S uint8[h, w, 3], p99)."""
    ok, _, srgb, p99 = hb.CompositeColorClasses(disp, mode, scale, intensity)
    return ok, srgb, p99


@functools.lru_cache(maxsize=None)
def geometry(sid_k, vid):
    """halo_consumer_view_filtered's (map, tap) for the pair: the consumer holds a zero image of the source's size."""
    sid, src = SOURCES[sid_k]
    view = dict(pairs_of(sid))[vid]
    hb = handle("geo-%dx%d" % (src.width, src.height))
    if not getattr(hb, "_cons_size", None):
        hb.Consume(np.zeros((src.height, src.width, 3), F32), 1.0)
    out = hb.View(view, src, want=("map", "tap"), filter="bilinear", blend=True)
    return out["map"].tobytes(), out["tap"].tobytes()


def check_quantised(out, name):
    want = np.floor(out["value"].astype(F32) + F32(0.5))
    assert want.dtype == F32 and (want >= 0).all() and (want <= 255).all(), name
    assert (out["srgb"] == want.astype(np.uint8)).all(), (name, int((out["srgb"] != want.astype(np.uint8)).sum()))


def check_values(S, out, src, bilinear, blend, name, key="value"):
    """out[key] float[h, w, 3] against the float64 model from the device's tap; returns the worst |delta| / largest tap value."""
    mp, val, tap = out["map"].ravel(), out[key].reshape(-1, 3), out["tap"].reshape(-1, 5)
    hit = mp >= 0
    assert (val[~hit] == 0.0).all() and (tap[~hit] == 0.0).all(), name
    if not hit.any():
        return 0.0
    want, big = fm.view64(S.astype(F32), tap[hit], src, bilinear, blend)
    err = np.abs(val[hit].astype(np.float64) - want)
    bar = fm.BAR * big[:, None]
    assert (err <= bar).all(), (name, float((err / np.maximum(bar, 1e-300)).max()))
    return float((err / np.maximum(big[:, None], 1e-300)).max())


# the composite each source is shown with: the three modes on random lanes of 3 classes, 1 class, 16 classes, solo and z-order
CASES = [("dominant", 3, {}), ("additive", 3, {}), ("painter", 3, {}), ("painter", 1, {}), ("additive", 16, {}), ("painter", 3, {"solo": (1, 2)}),
         ("painter", 3, {"z": (2, 0, 1)}), ("dominant", 3, {"hidden": (0,), "z": (1, 2, 0)})]
assert len(CASES) == len(SOURCES)


def prepared(k, case=None):
    sid, src = SOURCES[k]
    mode, n, kw = CASES[k] if case is None else case
    hb = handle(sid)
    lanes = load(hb, random_lanes(n, src, seed=3 + k))
    disp = display(n, **kw)
    ok, S, p99 = composite(hb, disp, mode)
    assert ok and p99 > 0.0 and len(np.unique(S)) > 64, (sid, mode)      # (not a black or a saturated frame)
    return hb, src, lanes, disp, mode, S, p99


# ---------------------------------------------------------------------------------------------------------------------------------
# 1: nearest is the composite's byte
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(len(SOURCES)), ids=IDS)
def test_nearest_is_the_composites_byte(k):
    hb, src, lanes, disp, mode, S, p99 = prepared(k)
    flat = S.reshape(-1, 3)
    n_hit = 0
    for vid, view in pairs_of(SOURCES[k][0]):
        name = "%s %s -> %s" % (mode, SOURCES[k][0], vid)
        out = hb.ViewComposite(view, disp, mode, source=src, want=ALL4)
        assert out["produced"] is True and F32(out["p99"]).tobytes() == F32(p99).tobytes(), name
        mp = out["map"].ravel()
        hit = mp >= 0
        got = out["srgb"].reshape(-1, 3)
        assert (got[hit] == flat[mp[hit]]).all(), (name, int((got[hit] != flat[mp[hit]]).any(axis=1).sum()))
        assert (got[~hit] == 0).all() and (out["value"].reshape(-1, 3)[~hit] == 0.0).all(), name
        assert (out["value"].reshape(-1, 3)[hit] == flat[mp[hit]].astype(F32)).all(), name
        assert (out["map"].tobytes(), out["tap"].tobytes()) == geometry(k, vid), name
        n_hit += int(hit.sum())
    assert n_hit > 1000
    assert drained(hb, lanes).tobytes() == lanes.tobytes()      # the lanes were read where they lie, and left as they were


@pytest.mark.parametrize("c", range(len(CASES)), ids=["%s-%d-%s" % (m, n, "-".join(kw) or "plain") for m, n, kw in CASES])
def test_every_composite_case_on_one_source(c):
    hb, src, lanes, disp, mode, S, p99 = prepared(1, CASES[c])
    flat = S.reshape(-1, 3)
    for vid, view in pairs_of(SOURCES[1][0])[::7]:
        out = hb.ViewComposite(view, disp, mode, source=src, want=("srgb", "map"))
        mp = out["map"].ravel()
        assert out["produced"] and out["p99"] == p99 and (out["srgb"].reshape(-1, 3)[mp >= 0] == flat[mp[mp >= 0]]).all(), (CASES[c], vid)
        assert (out["srgb"].reshape(-1, 3)[mp < 0] == 0).all(), (CASES[c], vid)


# ---------------------------------------------------------------------------------------------------------------------------------
# 2, 3: quantisation, values
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(len(SOURCES)), ids=IDS)
def test_quantisation_is_exact_and_values_meet_the_float64_model(k):
    hb, src, lanes, disp, mode, S, p99 = prepared(k)
    worst = 0.0
    moved = 0
    for vid, view in pairs_of(SOURCES[k][0]):
        outs = {}
        for filt, blend in COMBOS:
            name = "%s -> %s %s blend %d" % (SOURCES[k][0], vid, filt, blend)
            out = outs[filt, blend] = hb.ViewComposite(view, disp, mode, source=src, filter=filt, blend=blend, want=ALL4)
            assert out["produced"] and out["p99"] == p99, name
            assert (out["map"].tobytes(), out["tap"].tobytes()) == geometry(k, vid), name
            check_quantised(out, name)                                                               # 2: no pixel is excepted
            worst = max(worst, check_values(S, out, src, filt == "bilinear", blend, name))         # 3
        if not has_band(src):      # blend = 1 on a source without a band is accepted and changes nothing
            for filt in ("nearest", "bilinear"):
                assert outs[filt, True]["value"].tobytes() == outs[filt, False]["value"].tobytes(), vid
        moved += int((outs["bilinear", False]["srgb"] != outs["nearest", False]["srgb"]).sum())
    assert moved > 0
    print("%s: worst |delta| / max tap value = %.3g x 2^-24" % (SOURCES[k][0], worst * 2.0 ** 24))


def test_the_view_whose_tiles_outnumber_the_grid():
    sid, src, vid, view = vm.BIG_PAIR      # 8160 tiles of 16 x 16 pixels over a 1920 x 1080 source: workgroups stride over tiles
    small = scenes.render(abi.LENS_DUAL_FISHEYE_EQUAL_AREA, 128, 64, visible=vm.F, overlap=0.1, **vm.FLAT)
    hb = handle(SOURCES[1][0])
    lanes = load(hb, random_lanes(3, small, seed=41))
    disp = display(3)
    ok, S, p99 = composite(hb, disp, "additive")
    near = hb.ViewComposite(view, disp, "additive", source=small, want=("srgb", "map"))
    mp = near["map"].ravel()
    assert ok and (mp >= 0).mean() > 0.99 and (near["srgb"].reshape(-1, 3)[mp >= 0] == S.reshape(-1, 3)[mp[mp >= 0]]).all()
    out = hb.ViewComposite(view, disp, "additive", source=small, filter="bilinear", blend=True, want=ALL4)
    assert out["map"].tobytes() == near["map"].tobytes()
    check_quantised(out, "big")
    check_values(S, out, small, True, True, "big")
    assert (out["tap"][..., 4] > 0.0).any()
    lv = hb.ViewLanes(view, source=small, filter="bilinear", blend=True, want=("lanes", "map", "tap"))
    assert lv["map"].tobytes() == out["map"].tobytes() and lv["tap"].tobytes() == out["tap"].tobytes()
    check_lanes(lanes, lv, small, True, True, "big lanes")


# ---------------------------------------------------------------------------------------------------------------------------------
# 4: exact anchors
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(len(SOURCES)), ids=IDS)
def test_constant_lanes_stay_that_constant(k):
    sid, src = SOURCES[k]
    hb = handle(sid)
    lanes = np.empty((3, src.height, src.width), F32)
    lanes[0], lanes[1], lanes[2] = 0.5, 0.125, 2.0
    load(hb, lanes)
    disp = display(3)
    ok, S, _ = composite(hb, disp, "additive")
    const = S[0, 0].copy()
    assert ok and (S == const).all() and const.min() > 0 and len(set(const.tolist())) > 1, const
    for vid, view in pairs_of(sid):
        for filt, blend in COMBOS:
            out = hb.ViewComposite(view, disp, "additive", source=src, filter=filt, blend=blend, want=("srgb", "value", "map"))
            hit = out["map"].ravel() >= 0
            val, got = out["value"].reshape(-1, 3), out["srgb"].reshape(-1, 3)
            assert (val[hit] == const.astype(F32)).all() and (val[~hit] == 0.0).all(), (sid, vid, filt, blend)      # every b - a is 0
            assert (got[hit] == const).all() and (got[~hit] == 0).all(), (sid, vid, filt, blend)


BANDED = [k for k, (sid, src) in enumerate(SOURCES) if src.lens_type in vm.DUAL and src.overlap > 0.0 and src.lens_type != abi.LENS_DUAL_FISHEYE_ORTHOGRAPHIC]


@pytest.mark.parametrize("k", BANDED, ids=[IDS[k] for k in BANDED])
def test_the_band_blends_two_constants_exactly(k):
    sid, src = SOURCES[k]
    assert has_band(src)
    hb = handle(sid)
    w, h = src.width, src.height
    lanes = np.zeros((3, h, w), F32)
    lanes[0, :, :w // 2], lanes[0, :, w // 2:] = 1.0, 0.25      # the upper hemisphere's circle is the left one
    lanes[1, :, :w // 2], lanes[1, :, w // 2:] = 0.125, 1.0
    lanes[2] = 0.5
    load(hb, lanes)
    disp = display(3)
    ok, S, _ = composite(hb, disp, "additive")
    a, b = S[0, 0].astype(np.float64), S[0, w - 1].astype(np.float64)
    assert ok and (S[:, :w // 2] == S[0, 0]).all() and (S[:, w // 2:] == S[0, w - 1]).all() and (np.abs(a - b) > 8).any(), (a, b)
    checked = 0
    for vid, view in pairs_of(sid):
        for filt in ("nearest", "bilinear"):
            name = "%s -> %s %s" % (sid, vid, filt)
            plain = hb.ViewComposite(view, disp, "additive", source=src, filter=filt, blend=False, want=ALL4)
            blent = hb.ViewComposite(view, disp, "additive", source=src, filter=filt, blend=True, want=ALL4)
            mp, tap = plain["map"].ravel(), plain["tap"].reshape(-1, 5)
            v_p, v_b = plain["value"].reshape(-1, 3), blent["value"].reshape(-1, 3)
            two = (mp >= 0) & (tap[:, 4] > 0.0)
            assert (v_b[~two].view(np.uint32) == v_p[~two].view(np.uint32)).all(), name
            if not two.any():
                continue
            bil = filt == "bilinear"
            side = []
            for j in (0, 2):      # the taps of the primary and of the second sample: all left of the middle, or all right of it
                x0, x1, _, _, _, _ = fm.taps_of(tap[two, j], tap[two, j + 1], w, h, False, bil)
                lo, hi = np.minimum(x0, x1 if bil else x0), np.maximum(x0, x1 if bil else x0)
                side.append(np.where(hi < w // 2, -1, np.where(lo >= w // 2, 1, 0)))
            pure = side[0] * side[1] == -1
            t = tap[two, 4][pure].astype(np.float64)[:, None]
            first = np.where((side[0][pure] == -1)[:, None], a, b)
            second = np.where((side[1][pure] == -1)[:, None], a, b)
            want = (t * (second - first) + first).astype(F32)      # t (24 bits) x a difference of bytes (9) + a byte: exact in float64, one rounding
            assert (v_b[two][pure].view(np.uint32) == want.view(np.uint32)).all(), (name, int((v_b[two][pure] != want).any(axis=1).sum()))
            assert (v_p[two][pure] == first.astype(F32)).all(), name
            check_quantised(blent, name)
            checked += int(pure.sum())
    assert checked > 200, checked


def quadrupled(src, shift):
    """test_gpu_view_filter's: the source's own lens at four times the size, a single-view lens shifted by one view pixel."""
    r = abi.HaloRender()
    C.memmove(C.byref(r), C.byref(src), C.sizeof(r))
    r.width, r.height = 4 * src.width, 4 * src.height
    r.lens_shift[0], r.lens_shift[1] = shift
    return r


@pytest.mark.parametrize("k", [2, 4, 0], ids=[IDS[2], IDS[4], IDS[0]])
def test_a_single_lit_pixel_shows_only_where_a_tap_is_that_pixel(k):
    sid, src = SOURCES[k]
    hb = handle(sid)
    w, h = src.width, src.height
    single = src.lens_type in vm.SINGLE
    views = [("itself", src), ("quadrupled", quadrupled(src, (1, 1) if single else (0, 0)))] + pairs_of(sid)[:4]
    spots = [(0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1), (w - 1, h // 2), (0, h // 2), (w // 2, 0), (w // 2, h - 1), (w // 3, h // 2)]
    disp = display(1)
    clamped = {"left": 0, "right": 0, "top": 0, "bottom": 0, "wrap": 0}
    for sx, sy in spots:
        lanes = np.zeros((1, h, w), F32)
        lanes[0, sy, sx] = 2.5
        load(hb, lanes)
        ok, S, _ = composite(hb, disp, "painter")
        assert ok and S[sy, sx].max() > 32 and int((S != 0).any(axis=2).sum()) == 1
        for vid, view in views:
            name = "%s spot %d,%d -> %s" % (sid, sx, sy, vid)
            out = hb.ViewComposite(view, disp, "painter", source=src, filter="bilinear", blend=False, want=ALL4)
            check_values(S, out, src, True, False, name)
            mp, val, tap = out["map"].ravel(), out["value"].reshape(-1, 3), out["tap"].reshape(-1, 5)
            lit = (val != 0.0).any(axis=1)
            x0, x1, y0, y1, ax, ay = fm.taps_of(tap[:, 0], tap[:, 1], w, h, fm.is_rect(src))
            among = (((x0 == sx) | (x1 == sx)) & ((y0 == sy) | (y1 == sy))) & (mp >= 0)
            assert (among[lit]).all(), (name, int((lit & ~among).sum()))
            fx, fy = tap[:, 0].astype(np.float64), tap[:, 1].astype(np.float64)
            clamped["left"] += int((lit & (fx < 0.0)).sum())
            clamped["right"] += int((lit & (fx > w - 1) & ~np.bool_(fm.is_rect(src))).sum())
            clamped["top"] += int((lit & (fy < 0.0)).sum())
            clamped["bottom"] += int((lit & (fy > h - 1)).sum())
            clamped["wrap"] += int((lit & (x0 == w - 1) & (x1 == 0) & (ax > 0.0)).sum()) if fm.is_rect(src) else 0
    if src.lens_type == abi.LENS_LINEAR:      # its frame is all image: the quadrupled view reaches beyond all four edges, where the taps clamp
        assert min(clamped["left"], clamped["right"], clamped["top"], clamped["bottom"]) > 0, clamped
    if fm.is_rect(src):
        assert clamped["wrap"] > 0 and clamped["bottom"] > 0, clamped


# ---------------------------------------------------------------------------------------------------------------------------------
# 5: the lanes view
# ---------------------------------------------------------------------------------------------------------------------------------
def check_lanes(lanes, out, src, bilinear, blend, name):
    worst = 0.0
    for c in range(len(lanes)):      # one class at a time: the bar is that class's largest tap, not the largest of three
        one = {"map": out["map"], "tap": out["tap"], "v": np.repeat(out["lanes"][c][..., None], 3, axis=2)}
        worst = max(worst, check_values(np.repeat(lanes[c][..., None], 3, axis=2), one, src, bilinear, blend, "%s class %d" % (name, c), key="v"))
    return worst


@pytest.mark.parametrize("n", [1, 3, 16])
@pytest.mark.parametrize("k", [1, 2, 3], ids=[IDS[1], IDS[2], IDS[3]])
def test_the_lanes_view(k, n):
    sid, src = SOURCES[k]
    hb = handle(sid)
    lanes = load(hb, random_lanes(n, src, seed=50 + n))
    disp = display(n)
    worst = 0.0
    for vid, view in pairs_of(sid)[::(1 if n == 3 else 5)]:
        name = "%s -> %s x%d" % (sid, vid, n)
        near = hb.ViewLanes(view, source=src, want=("lanes", "map", "tap"))
        assert near["lanes"].shape == (n, view.height, view.width) and near["lanes"].dtype == F32
        comp = hb.ViewComposite(view, disp, "painter", source=src, want=("map", "tap"))
        assert near["map"].tobytes() == comp["map"].tobytes() and near["tap"].tobytes() == comp["tap"].tobytes(), name
        mp = near["map"].ravel()
        hit = mp >= 0
        for c in range(n):
            got = near["lanes"][c].ravel()
            assert (got[hit].view(np.uint32) == lanes[c].ravel()[mp[hit]].view(np.uint32)).all() and (got[~hit] == 0.0).all(), (name, c)
        for filt, blend in COMBOS[1:]:
            out = hb.ViewLanes(view, source=src, filter=filt, blend=blend, want=("lanes", "map", "tap"))
            assert out["map"].tobytes() == near["map"].tobytes() and out["tap"].tobytes() == near["tap"].tobytes(), name
            worst = max(worst, check_lanes(lanes, out, src, filt == "bilinear", blend, name))
            alone = hb.ViewLanes(view, source=src, filter=filt, blend=blend)
            assert set(alone) == {"lanes"} and alone["lanes"].tobytes() == out["lanes"].tobytes(), name
    assert drained(hb, lanes).tobytes() == lanes.tobytes()      # read where they lie, left as they were
    print("%s x%d: worst |delta| / max tap value = %.3g x 2^-24" % (sid, n, worst * 2.0 ** 24))


# ---------------------------------------------------------------------------------------------------------------------------------
# 6, 7: the cases without a composite, the refusals
# ---------------------------------------------------------------------------------------------------------------------------------
def _spec(view, source=None):
    s = abi.HaloViewSpec()
    s.view = view
    s.has_source = 0 if source is None else 1
    if source is not None:
        s.source = source
    return s


def _ptr(a, t):
    return a.ctypes.data_as(C.POINTER(t)) if a is not None else None


def raw_composite(hb, spec, filt, comp, srgb=None, value=None, mp=None, tap=None, want_produced=True):
    p99, produced = C.c_float(-7.0), C.c_int32(-7)
    rc = hb._L.halo_consumer_view_composite(hb._h, C.byref(spec) if spec is not None else None, C.byref(filt) if filt is not None else None,
                                            C.byref(comp) if comp is not None else None, _ptr(srgb, C.c_uint8), _ptr(value, C.c_float), _ptr(mp, C.c_int32),
                                            _ptr(tap, C.c_float), C.byref(p99), C.byref(produced) if want_produced else None)
    return rc, (hb._L.halo_last_error(hb._h) or b"").decode(), p99.value, produced.value


def raw_lanes(hb, spec, filt, lanes=None, mp=None, tap=None):
    rc = hb._L.halo_consumer_view_lanes(hb._h, C.byref(spec) if spec is not None else None, C.byref(filt) if filt is not None else None, _ptr(lanes, C.c_float),
                                        _ptr(mp, C.c_int32), _ptr(tap, C.c_float))
    return rc, (hb._L.halo_last_error(hb._h) or b"").decode()


def _buffers(view):
    n = view.width * view.height
    return np.full((n, 3), 77, np.uint8), np.full((n, 3), 77.0, F32), np.full(n, -5, np.int32), np.full((n, 5), 77.0, F32)


def test_the_three_cases_that_stop_before_a_composite():
    k = 1
    sid, src = SOURCES[k]
    vid, view = pairs_of(sid)[0]
    hb = handle(sid)
    lanes = random_lanes(3, src)
    filt = abi.HaloViewFilter(abi.VIEW_BILINEAR, 1)
    geo = geometry(k, vid)
    # no class references a raypath bit: nothing of the composite is written
    load(hb, lanes, bits=False)
    srgb, value, mp, tap = _buffers(view)
    rc, msg, p99, produced = raw_composite(hb, _spec(view, src), filt, abi.composite(display(3), "painter"), srgb, value, mp, tap)
    assert rc == abi.HALO_OK and produced == 0 and p99 == -7.0, msg
    assert (srgb == 77).all() and (value == 77.0).all() and (mp.tobytes(), tap.tobytes()) == geo
    assert not hb.CompositeColorClasses(display(3), "painter")[0]
    # no active class: a black composite, still a valid one
    load(hb, lanes)
    srgb, value, mp, tap = _buffers(view)
    rc, msg, p99, produced = raw_composite(hb, _spec(view, src), filt, abi.composite(display(3, hidden=(0, 1, 2)), "painter"), srgb, value, mp, tap)
    assert rc == abi.HALO_OK and produced == 1 and p99 == 0.0, msg
    assert (srgb == 0).all() and (value == 0.0).all() and (mp.tobytes(), tap.tobytes()) == geo
    ok, S, p99c = composite(hb, display(3, hidden=(0, 1, 2)), "painter")
    assert ok and p99c == 0.0 and (S == 0).all()
    # the exposure scale is not positive (no landed intensity): P99 published, the bytes untouched, the value image zeroed
    load(hb, lanes, total=0.0)
    srgb, value, mp, tap = _buffers(view)
    rc, msg, p99, produced = raw_composite(hb, _spec(view, src), filt, abi.composite(display(3), "painter"), srgb, value, mp, tap)
    ok, _, p99c = composite(hb, display(3), "painter")
    assert rc == abi.HALO_OK and produced == 0 and not ok and p99 > 0.0 and F32(p99).tobytes() == F32(p99c).tobytes(), msg
    assert (srgb == 77).all() and (value == 0.0).all() and (mp.tobytes(), tap.tobytes()) == geo
    out = hb.ViewComposite(view, display(3), "painter", source=src, filter="bilinear", blend=True, want=ALL4)
    assert out["produced"] is False and out["srgb"] is None and out["p99"] == p99 and out["map"].tobytes() == geo[0]


def test_refusals_come_back_by_name_and_leave_the_handle_usable():
    from ice_halo_sim_amd.backend import HipTraceBackend
    sid, src = SOURCES[1]
    vid, view = pairs_of(sid)[0]
    lanes = random_lanes(3, src)
    disp = display(3)
    good, comp = abi.HaloViewFilter(abi.VIEW_BILINEAR, 1), abi.composite(disp, "additive")
    srgb, value, mp, tap = _buffers(view)
    lout = np.zeros((3, view.height, view.width), F32)
    hb = HipTraceBackend(device=0, seed=9)
    try:
        def both(spec, filt, text, rc_want=abi.HALO_FATAL, c=comp):
            rc, msg, _, _ = raw_composite(hb, spec, filt, c, srgb=srgb)
            assert rc == rc_want and "consumer_view_composite" in msg and text in msg, (text, rc, msg)
            rc, msg = raw_lanes(hb, spec, filt, lanes=lout)
            assert rc == rc_want and "consumer_view_lanes" in msg and text in msg, (text, rc, msg)
        hb.set_color([], bit_classes(3))
        both(_spec(view, src), good, "no lanes")
        hb.LoadClassLanes(lanes, TOTAL)
        both(None, good, "spec is NULL")
        for f in (2, -1, 7):
            both(_spec(view, src), abi.HaloViewFilter(f, 0), "unknown filter")
        for bl in (2, -1):
            both(_spec(view, src), abi.HaloViewFilter(abi.VIEW_BILINEAR, bl), "blend must be 0 or 1")
        for j in (0, 1):
            f = abi.HaloViewFilter(abi.VIEW_NEAREST, 0)
            f.reserved[j] = 1
            both(_spec(view, src), f, "reserved")
        both(_spec(view, None), good, "has had no session")
        both(_spec(view, scenes.render(src.lens_type, src.width // 2, src.height, visible=src.visible)), good, "size is not the lanes'")
        for w, h in ((0, 5), (5, 0), (-1, 3)):
            both(_spec(scenes.render(abi.LENS_LINEAR, w, h, fov=60.0), src), good, "empty view")
        both(_spec(scenes.render(abi.LENS_LINEAR, 8192, 4097, fov=60.0), src), good, "2^25", abi.HALO_UNAVAILABLE)
        bad = _spec(view, src)
        bad.source.lens_type = 11
        both(bad, good, "unknown lens type")
        bad = _spec(view, src)
        bad.view.lens_type = -1
        both(bad, good, "unknown lens type")
        # every output NULL: participating_p99_y and produced do not count
        rc, msg, _, _ = raw_composite(hb, _spec(view, src), good, comp)
        assert rc == abi.HALO_FATAL and "every output is NULL" in msg
        rc, msg = raw_lanes(hb, _spec(view, src), good)
        assert rc == abi.HALO_FATAL and "every output is NULL" in msg
        # the composite call's own
        rc, msg, _, _ = raw_composite(hb, _spec(view, src), good, comp, srgb=srgb, want_produced=False)
        assert rc == abi.HALO_FATAL and "produced is NULL" in msg
        rc, msg, _, _ = raw_composite(hb, _spec(view, src), good, None, srgb=srgb)
        assert rc == abi.HALO_FATAL and "composite is NULL" in msg
        for m in (-1, 3):
            rc, msg, _, _ = raw_composite(hb, _spec(view, src), good, abi.composite(disp, m), srgb=srgb)
            assert rc == abi.HALO_FATAL and "unknown mode" in msg
        for n in (2, 4):
            rc, msg, _, _ = raw_composite(hb, _spec(view, src), good, abi.composite(display(n), "additive"), srgb=srgb)
            assert rc == abi.HALO_FATAL and "class_count differs" in msg
        # the lanes call's own: 16 classes x 2^24 view pixels is more than 2^27 floats (nothing is allocated for it)
        hb.set_color([], bit_classes(16))
        hb.LoadClassLanes(random_lanes(16, src), TOTAL)
        rc, msg = raw_lanes(hb, _spec(scenes.render(abi.LENS_LINEAR, 4096, 4096, fov=60.0), src), good, mp=mp)
        assert rc == abi.HALO_UNAVAILABLE and "2^27" in msg
        hb.set_color([], bit_classes(3))
        hb.LoadClassLanes(lanes, TOTAL)
        with pytest.raises(ValueError):
            hb.ViewComposite(view, disp, source=src, filter="cubic")
        with pytest.raises(ValueError):
            hb.ViewLanes(view, source=src, want=("lane",))
        sc = scenes.config2_scene()
        hb.set_color([], [])      # (a plain session)
        hb.BeginSession(sc, src, scenes.wl_discrete(550.0), 64)
        both(_spec(view, src), good, "inside a session")
        hb.TraceLayer(64)
        hb.EndSession()
        # ... and the handle works, giving a fresh handle's bytes; the default source is now the session's render; filter NULL is nearest, no blend
        hb.set_color([], bit_classes(3))
        hb.LoadClassLanes(lanes, TOTAL)
        rc, msg, p99, produced = raw_composite(hb, _spec(view, None), good, comp, srgb, value, mp, tap)
        assert rc == abi.HALO_OK and produced == 1, msg
        rc, msg = raw_lanes(hb, _spec(view, None), good, lanes=lout)
        assert rc == abi.HALO_OK, msg
        s2 = np.zeros_like(srgb)
        rc, msg, _, _ = raw_composite(hb, _spec(view, src), None, comp, srgb=s2)
        assert rc == abi.HALO_OK, msg
        fresh = HipTraceBackend(device=0, seed=9)
        try:
            load(fresh, lanes)
            want = fresh.ViewComposite(view, disp, "additive", source=src, filter="bilinear", blend=True, want=ALL4)
            for key, a in zip(ALL4, (srgb, value, mp, tap)):
                assert want[key].tobytes() == a.tobytes(), key
            assert want["p99"] == p99
            assert fresh.ViewLanes(view, source=src, filter="bilinear", blend=True)["lanes"].tobytes() == lout.tobytes()
            assert fresh.ViewComposite(view, disp, "additive", source=src)["srgb"].tobytes() == s2.tobytes()
        finally:
            fresh.close()
    finally:
        hb.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# 8: the wrappers
# ---------------------------------------------------------------------------------------------------------------------------------
def test_the_python_wrappers_are_the_c_calls():
    hb, src, lanes, disp, mode, S, p99 = prepared(2)
    vid, view = vm.mid_views()[0]
    srgb, value, mp, tap = _buffers(view)
    rc, msg, p, produced = raw_composite(hb, _spec(view, src), abi.HaloViewFilter(abi.VIEW_BILINEAR, 0), abi.composite(disp, mode, 1.5, 0.75), srgb, value, mp, tap)
    assert rc == abi.HALO_OK and produced == 1, msg
    out = hb.ViewComposite(view, disp, mode, 1.5, 0.75, source=src, filter="bilinear", want=ALL4)
    assert out["srgb"].shape == (view.height, view.width, 3) and out["tap"].shape == (view.height, view.width, 5) and out["map"].shape == (view.height, view.width)
    for key, a in zip(ALL4, (srgb, value, mp, tap)):
        assert out[key].tobytes() == a.tobytes(), key
    assert out["p99"] == p and out["produced"] is True
    assert set(hb.ViewComposite(view, disp, mode, source=src)) == {"srgb", "produced", "p99"}
    lout = np.zeros((len(lanes), view.height, view.width), F32)
    m2, t2 = np.zeros_like(mp), np.zeros_like(tap)
    rc, msg = raw_lanes(hb, _spec(view, src), abi.HaloViewFilter(abi.VIEW_BILINEAR, 1), lout, m2, t2)
    assert rc == abi.HALO_OK, msg
    got = hb.ViewLanes(view, source=src, filter="bilinear", blend=True, want=("lanes", "map", "tap"))
    assert got["lanes"].tobytes() == lout.tobytes() and got["map"].tobytes() == m2.tobytes() and got["tap"].tobytes() == t2.tobytes()


def test_the_cli_writes_the_composite_views_bytes(tmp_path, capsys):
    from ice_halo_sim_amd import cli, config
    cfg = json.load(open(os.path.join(ROOT, "tests", "golden", "ref_e2e_configs.json")))["painter_default_overlap"]
    cfg["scene"]["ray_num"] = 60000
    cfg["render"][0]["overlap"] = 0.1
    path = str(tmp_path / "colour.json")
    json.dump(cfg, open(path, "w"))
    ppm, flat, npy = str(tmp_path / "vc.ppm"), str(tmp_path / "c.ppm"), str(tmp_path / "lanes.npy")
    common = ["-f", path, "--view-lens", "linear", "--view-fov", "90", "--view-az", "0", "--view-el", "0", "--view-size", "80x45", "--display-ev", "0.5"]
    # one run writes the view, the flat composite and then the lanes both were made from (the view is taken before the lanes are drained)
    assert cli.main(common + ["--out-view-composite", ppm, "--out-composite", flat, "--out-lanes", npy, "--view-filter", "bilinear", "--view-blend"]) == 0
    head = b"P6\n80 45\n255\n"
    data = open(ppm, "rb").read()
    assert data[:len(head)] == head and len(data) == len(head) + 80 * 45 * 3
    job = config.load_config(path)
    src = job.renders[sorted(job.renders)[0]]
    lanes = np.load(npy)
    assert src.overlap > 0.0 and lanes.shape == (len(job.color_meta), src.height, src.width) and lanes.max() > 0.0
    hb = handle("cli")
    load(hb, lanes)      # (any positive total intensity: the composite's exposure is anchored to its own P99)
    view = scenes.render(abi.LENS_LINEAR, 80, 45, fov=90.0, az=0.0, el=0.0, ro=0.0, visible=abi.VISIBLE_FULL)
    out = hb.ViewComposite(view, job.color_meta, job.color_mode, 2.0 ** 0.5, 1.0, source=src, filter="bilinear", blend=True, want=("srgb", "tap"))
    assert out["produced"] and out["srgb"].tobytes() == data[len(head):]
    assert len(np.unique(out["srgb"])) > 8 and (out["tap"][..., 4] > 0.0).any()      # (not a black frame; the band is on screen)
    near = hb.ViewComposite(view, job.color_meta, job.color_mode, 2.0 ** 0.5, 1.0, source=src)
    assert near["srgb"].tobytes() != out["srgb"].tobytes()
    whole = open(flat, "rb").read()
    assert whole[-src.width * src.height * 3:] == hb.CompositeColorClasses(job.color_meta, job.color_mode, 2.0 ** 0.5, 1.0)[2].tobytes()
    # where the reference's function returns false the CLI says so and writes no file: an intensity factor of zero leaves no exposure scale
    cfg["render"][0]["intensity_factor"] = 0.0
    json.dump(cfg, open(path, "w"))
    gone = str(tmp_path / "none.ppm")
    capsys.readouterr()
    assert cli.main(common + ["--out-view-composite", gone]) == 0
    assert "no composite" in capsys.readouterr().err and not os.path.exists(gone)


def test_a_cpp_host_drives_both_calls():
    from ice_halo_sim_amd import backend
    backend.load_library()
    exe = os.path.join(ROOT, "tests", "cpp", "view_composite_main")
    libdir = os.path.join(ROOT, "ice_halo_sim_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-o", exe, os.path.join(ROOT, "tests", "cpp", "view_composite_main.cpp"), "-L" + libdir, "-lhalo_hip", "-ldl",
                           "-Wl,-rpath," + libdir])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    said = dict(line.split() for line in r.stdout.strip().splitlines())

    def fnv1a(a):
        h = 1469598103934665603
        for byte in a.tobytes():
            h = ((h ^ byte) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
        return "%016x" % h
    W, H, N = 128, 64, 3
    i = np.arange(N * W * H, dtype=np.uint64)
    lanes = ((((i * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)) >> np.uint64(12)) & np.uint64(0xFFFF)).astype(F32) / F32(65536.0)
    src = scenes.render(abi.LENS_DUAL_FISHEYE_EQUAL_AREA, W, H, fov=180.0, az=0.0, el=0.0, ro=0.0, visible=abi.VISIBLE_FULL, overlap=0.1)
    view = scenes.render(abi.LENS_LINEAR, 37, 23, fov=90.0, az=40.0, el=5.0, ro=10.0, visible=abi.VISIBLE_FULL)
    disp = [{"color": c, "visible": True, "solo": False, "z_order": j} for j, c in enumerate(((1.0, 0.25, 0.125), (0.125, 1.0, 0.5), (0.25, 0.5, 1.0)))]
    hb = handle("cpp")
    load(hb, lanes.reshape(N, H, W))
    out = hb.ViewComposite(view, disp, "additive", source=src, filter="bilinear", blend=True, want=ALL4)
    lv = hb.ViewLanes(view, source=src, filter="bilinear", blend=True)
    assert said["produced"] == "1" and out["produced"]
    assert said["p99"] == "%08x" % int(np.array(out["p99"], F32).view(np.uint32))
    for key in ALL4:
        assert said[key] == fnv1a(out[key]), key
    assert said["lanes"] == fnv1a(lv["lanes"])
    assert len(np.unique(out["srgb"])) > 8 and (out["tap"][..., 4] > 0.0).any()
