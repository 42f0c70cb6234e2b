"""halo_consumer_view_filtered — bilinear taps and the overlap-band blend of the view stage — on the device, held part by part.

Images are loaded with halo_consumer_consume; the consumer's raw snapshot (sum + compensation, what a tap reads) is the image every value is
compared against.  Per (source, view) pair of tests/_view_filter_model.py:
  1. filter = nearest, blend = 0 gives halo_consumer_view's rgb, xyz, map and dir byte for byte;
  2. tap: floor(fx0 + 0.5), floor(fy0 + 0.5), taken in fp32, is map's pixel on EVERY pixel that has a source (the rectangular lens after its wrap),
     zeros elsewhere; the record equals halo_host_view_source_pos fed the device's dir — bit for bit where no libm call (and no v_rsq_f32) lies
     between: the linear, orthographic and globe sources, and t everywhere; within _lens_model.DELTA["px"] for the others;
  3. values: xyz against the float64 model (_view_filter_model.view64) evaluated from the device's own tap record,
     |delta| <= 8 x 2^-24 x the largest tap value of the pixel, per channel (derivation: _view_filter_model.py), for a random image with a
     compensation term, a ramp in x of integers below 2^24 and a ramp in y;
  4. exact anchors: a constant image, single-pixel images at the frame's edges and the rectangular wrap column, a two-valued image across a dual
     source's band (the blend is fma(t, b - a, a) to the bit, blend = 0 shows the step), continuity where the band ends;
  5. rgb: the call's xyz_out, loaded into a second handle of the view's size, has rgb_out as its snapshot under the same display, byte for byte;
  6. every output alone, two calls one record, the refusals by name, the Python wrapper against the C call, the CLI."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from ice_halo_sim_amd import abi, scenes
from tests import _lens_model as lm
from tests import _view_filter_model as fm
from tests import _view_model as vm
from tests.test_gpu_view import DISPLAYS

pytestmark = pytest.mark.gpu
F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = ("rgb", "xyz", "map", "dir")
ALL5 = ALL + ("tap",)
SOURCES = fm.sources()
IDS = [s[0] for s in SOURCES]
EXACT_ON_HOST = (abi.LENS_LINEAR, abi.LENS_FISHEYE_ORTHOGRAPHIC, abi.LENS_DUAL_FISHEYE_ORTHOGRAPHIC, abi.LENS_GLOBE)
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


def load(hb, images, landed=None):
    """Replace the consumer's image by the sum of `images`; returns the raw snapshot float32[h, w, 3]."""
    if getattr(hb, "_cons_size", None):
        hb.ResetConsumer()
    h, w = images[0].shape[:2]
    hb.Consume(images[0], 0.08 * w * h * 2.0 * float(images[0][..., 1].mean()) if landed is None else landed)
    for img in images[1:]:
        hb.Consume(img, 0.0)
    return hb.Snapshot(want_xyz=True)[1].copy()


def random_images(src, seed=11):
    g = np.random.default_rng(seed)
    a = g.uniform(0.5, 2.0, (src.height, src.width, 3)).astype(F32)
    b = (g.uniform(0.5, 2.0, (src.height, src.width, 3)) * 1e-4).astype(F32)     # a second fold whose low bits the sum drops: comp != 0
    return a, b


def ramp_x(src):
    v = (np.arange(src.width, dtype=np.float64) + 1.0) * 130001.0               # integers below 2^24 = 16777216
    img = np.broadcast_to(np.stack([v, v + 1.0, v + 2.0], 1)[None, :, :], (src.height, src.width, 3)).astype(F32)
    assert img.max() < 2.0 ** 24 and (img == np.round(img)).all()
    return np.ascontiguousarray(img)


def ramp_y(src):
    v = (np.arange(src.height, dtype=np.float64) + 1.0) * 0.37
    return np.ascontiguousarray(np.broadcast_to(np.stack([v, 2.0 * v, 0.5 * v], 1)[:, None, :], (src.height, src.width, 3)).astype(F32))


def pairs_of(sid):
    return [(vid, view) for s2, _, vid, view in fm.gpu_pairs() if s2 == sid]


def floor_half(v):
    return np.floor(np.asarray(v, F32) + F32(0.5)).astype(np.int64)


def has_band(src):
    return lm.proj_of(src).mad > 0.0


def check_values(raw, out, src, bilinear, blend, name):
    mp, xyz, tap = out["map"].ravel(), out["xyz"].reshape(-1, 3), out["tap"].reshape(-1, 5)
    hit = mp >= 0
    assert (xyz[~hit] == 0.0).all() and (tap[~hit] == 0.0).all(), name
    if not hit.any():
        return 0.0
    want, big = fm.view64(raw, tap[hit], src, bilinear, blend)
    err = np.abs(xyz[hit].astype(np.float64) - want)
    bar = fm.BAR * big[:, None]
    assert (err <= bar).all(), (name, float((err / np.maximum(bar, 1e-300)).max()))
    return float((err / np.maximum(big[:, None], 1e-300)).max())


# ---------------------------------------------------------------------------------------------------------------------------------
# 1, 2: the old call, the tap record
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(len(SOURCES)), ids=IDS)
def test_nearest_is_the_old_call_and_the_tap_record_is_project_exit(k):
    sid, src = SOURCES[k]
    hb = handle(sid)
    load(hb, random_images(src))
    P = lm.proj_of(src)
    n_hit = n_two = 0
    for vid, view in pairs_of(sid):
        name = sid + " -> " + vid
        old = hb.View(view, src, want=ALL, **DISPLAYS[2])
        new = hb.View(view, src, want=ALL5, filter="nearest", blend=False, **DISPLAYS[2])
        for key in ALL:
            assert new[key].tobytes() == old[key].tobytes(), (name, key)
        mp, tap, dirs = new["map"].ravel(), new["tap"].reshape(-1, 5), new["dir"].reshape(-1, 3)
        hit = mp >= 0
        assert (tap[~hit] == 0.0).all(), name
        if not hit.any():
            continue
        px, py = floor_half(tap[hit, 0]), floor_half(tap[hit, 1])
        if fm.is_rect(src):
            px = np.mod(px, src.width)
        assert (px == mp[hit] % src.width).all() and (py == mp[hit] // src.width).all(), (name, int(((px != mp[hit] % src.width) | (py != mp[hit] // src.width)).sum()))
        cnt, pos = fm.host_source_pos(src, dirs[hit])
        assert (cnt >= 1).all() and ((tap[hit, 4] > 0.0) == (cnt == 2)).all(), name
        assert (tap[hit, 4].view(np.uint32) == pos[:, 4].view(np.uint32)).all(), name      # t: one difference, one product, one quotient
        if src.lens_type in EXACT_ON_HOST:
            assert (tap[hit].view(np.uint32) == pos.view(np.uint32)).all(), (name, int((tap[hit] != pos).any(axis=1).sum()))
        else:
            dev = np.abs(tap[hit, :4].astype(np.float64) - pos[:, :4].astype(np.float64)).max()
            assert dev <= lm.DELTA["px"], (name, float(dev))
        n_hit += int(hit.sum())
        n_two += int((cnt == 2).sum())
    assert n_hit > 1000 and (n_two > 100) == has_band(src), (n_hit, n_two)


# ---------------------------------------------------------------------------------------------------------------------------------
# 3: values
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(len(SOURCES)), ids=IDS)
def test_values_against_the_float64_model(k):
    sid, src = SOURCES[k]
    hb = handle(sid)
    worst = 0.0
    for label, images in (("random", random_images(src)), ("ramp-x", (ramp_x(src),)), ("ramp-y", (ramp_y(src),))):
        raw = load(hb, images)
        if label == "random":
            assert (raw.astype(np.float64) - images[0].astype(np.float64) > 0).all()      # the compensation term is in the taps
        for vid, view in pairs_of(sid):
            name = "%s %s -> %s" % (label, sid, vid)
            plain = hb.View(view, src, want=("xyz", "map", "tap"), filter="bilinear", blend=False)
            worst = max(worst, check_values(raw, plain, src, True, False, name))
            blent = hb.View(view, src, want=("xyz", "map", "tap"), filter="bilinear", blend=True)
            assert blent["tap"].tobytes() == plain["tap"].tobytes() and blent["map"].tobytes() == plain["map"].tobytes(), name
            if has_band(src):
                worst = max(worst, check_values(raw, blent, src, True, True, name + " blend"))
                one = plain["tap"].reshape(-1, 5)[:, 4] == 0.0
                assert (blent["xyz"].reshape(-1, 3)[one].view(np.uint32) == plain["xyz"].reshape(-1, 3)[one].view(np.uint32)).all(), name
            else:       # blend = 1 on a source without a band is accepted and changes nothing
                assert blent["xyz"].tobytes() == plain["xyz"].tobytes(), name
    print("%s: worst |delta| / max |tap value| = %.3g x 2^-24" % (sid, worst * 2.0 ** 24))


def test_the_pair_whose_tiles_outnumber_the_grid():
    sid, src, vid, view = vm.BIG_PAIR      # 8160 tiles of 16 x 16 pixels: workgroups stride over tiles
    hb = handle("big")
    raw = load(hb, random_images(src))
    old = hb.View(view, src, want=("xyz", "map"))
    out = hb.View(view, src, want=("xyz", "map", "tap"), filter="bilinear", blend=True)
    assert out["map"].tobytes() == old["map"].tobytes() and (out["map"] >= 0).mean() > 0.99
    check_values(raw, out, src, True, True, sid + " -> " + vid)
    mp, tap = out["map"].ravel(), out["tap"].reshape(-1, 5)
    assert (floor_half(tap[:, 0]) == mp % src.width)[mp >= 0].all() and (floor_half(tap[:, 1]) == mp // src.width)[mp >= 0].all()
    near = hb.View(view, src, want=("xyz",), filter="nearest", blend=False)
    assert near["xyz"].tobytes() == old["xyz"].tobytes()
    hb.close()
    del _handles["big"]


# ---------------------------------------------------------------------------------------------------------------------------------
# 4: exact anchors
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(len(SOURCES)), ids=IDS)
def test_a_constant_image_stays_that_constant(k):
    sid, src = SOURCES[k]
    hb = handle(sid)
    const = np.array([1.5, 2.25, 0.7], F32)
    load(hb, (np.broadcast_to(const, (src.height, src.width, 3)).copy(),))
    for vid, view in pairs_of(sid):
        out = hb.View(view, src, want=("xyz", "map"), filter="bilinear", blend=True)
        hit = out["map"].ravel() >= 0
        xyz = out["xyz"].reshape(-1, 3)
        assert (xyz[hit] == const).all() and (xyz[~hit] == 0.0).all(), sid + " -> " + vid      # every b - a is 0


def quadrupled(src, shift):
    """The source's own lens at four times the size: with a lens shift of one view pixel the centres of a single-view lens fall on
    (p - 1) / 4 of the source — a quarter pixel beyond its first centre and beyond its last, inside the frame's outermost half pixels, where
    the taps clamp; a rectangular source is read at p / 4, up to its wrap column and its last row."""
    r = abi.HaloRender()
    C.memmove(C.byref(r), C.byref(src), C.sizeof(r))
    r.width, r.height = 4 * src.width, 4 * src.height
    r.lens_shift[0], r.lens_shift[1] = shift
    return r


@pytest.mark.parametrize("k", [2, 3, 4, 0], ids=[IDS[2], IDS[3], IDS[4], IDS[0]])
def test_a_single_pixel_shows_only_where_a_tap_is_that_pixel(k):
    sid, src = SOURCES[k]
    hb = handle(sid)
    w, h = src.width, src.height
    single = src.lens_type in vm.SINGLE
    views = [("itself", src), ("quadrupled", quadrupled(src, (1, 1) if single else (0, 0)))] + pairs_of(sid)[:6]
    spots = [(0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1), (w - 1, h // 2), (0, h // 2), (w // 2, 0), (w // 2, h - 1), (w // 3, h // 2)]
    clamped = {"left": 0, "right": 0, "top": 0, "bottom": 0, "wrap": 0}
    for sx, sy in spots:
        img = np.zeros((h, w, 3), F32)
        img[sy, sx] = (3.0, 5.0, 7.0)
        raw = load(hb, (img,), landed=1.0)
        for vid, view in views:
            name = "%s spot %d,%d -> %s" % (sid, sx, sy, vid)
            out = hb.View(view, src, want=("xyz", "map", "tap"), filter="bilinear", blend=False)
            check_values(raw, out, src, True, False, name)
            mp, xyz, tap = out["map"].ravel(), out["xyz"].reshape(-1, 3), out["tap"].reshape(-1, 5)
            lit = (xyz != 0.0).any(axis=1)
            x0, x1, y0, y1, ax, ay = fm.taps_of(tap[:, 0], tap[:, 1], w, h, fm.is_rect(src))
            among = (((x0 == sx) | (x1 == sx)) & ((y0 == sy) | (y1 == sy))) & (mp >= 0)
            assert (among[lit]).all(), (name, int((lit & ~among).sum()))
            fx, fy = tap[:, 0].astype(np.float64), tap[:, 1].astype(np.float64)
            clamped["left"] += int((lit & (fx < 0.0)).sum())
            clamped["right"] += int((lit & (fx > w - 1) & ~np.bool_(fm.is_rect(src))).sum())
            clamped["top"] += int((lit & (fy < 0.0)).sum())
            clamped["bottom"] += int((lit & (fy > h - 1)).sum())
            clamped["wrap"] += int((lit & (x0 == w - 1) & (x1 == 0) & (ax > 0.0)).sum()) if fm.is_rect(src) else 0
    print(sid, clamped)
    if src.lens_type == abi.LENS_LINEAR:      # its frame is all image: the quadrupled view reaches a quarter of a source pixel beyond all four edges
        # (a fisheye's image circle touches the frame at four points, which its rim culls)
        assert min(clamped["left"], clamped["right"], clamped["top"], clamped["bottom"]) > 0, clamped
    if fm.is_rect(src):      # (no latitude lies above the first row's centre: the top edge clamps on the single-view sources)
        assert clamped["wrap"] > 0 and clamped["bottom"] > 0, clamped


BANDED = [k for k, (sid, src) in enumerate(SOURCES) if src.lens_type in vm.DUAL and src.overlap > 0.0 and src.lens_type != abi.LENS_DUAL_FISHEYE_ORTHOGRAPHIC]


@pytest.mark.parametrize("k", BANDED, ids=[IDS[k] for k in BANDED])
def test_the_band_blends_two_hemispheres_exactly(k):
    sid, src = SOURCES[k]
    assert has_band(src)
    hb = handle(sid)
    w, h = src.width, src.height
    a, b = np.array([1.0, 2.0, 0.5], F32), np.array([3.0, 6.0, 1.5], F32)      # b - a: powers of two, so fma(t, b - a, a) is one rounding of an exact float64
    img = np.zeros((h, w, 3), F32)
    img[:, :w // 2], img[:, w // 2:] = a, b      # the upper hemisphere's circle is the left one
    raw = load(hb, (img,), landed=1.0)
    assert (raw == img).all()
    checked = steps = 0
    for vid, view in pairs_of(sid):
        for filt in ("nearest", "bilinear"):
            name = "%s -> %s %s" % (sid, vid, filt)
            plain = hb.View(view, src, want=("xyz", "map", "tap"), filter=filt, blend=False)
            blent = hb.View(view, src, want=("xyz", "map", "tap"), filter=filt, blend=True)
            mp, tap = plain["map"].ravel(), plain["tap"].reshape(-1, 5)
            x_p, x_b = plain["xyz"].reshape(-1, 3), blent["xyz"].reshape(-1, 3)
            two = (mp >= 0) & (tap[:, 4] > 0.0)
            assert (x_b[~two].view(np.uint32) == x_p[~two].view(np.uint32)).all(), name
            if filt == "nearest":      # blend = 0 shows the step: every pixel is its primary pixel's value, a on one side of the horizon and b on the other
                assert (x_p[mp >= 0] == raw.reshape(-1, 3)[mp[mp >= 0]]).all(), name
                steps += int((x_p[two] == a).all(axis=1).any() and (x_p[two] == b).all(axis=1).any())
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
            first = np.where((side[0][pure] == -1)[:, None], a, b).astype(np.float64)
            second = np.where((side[1][pure] == -1)[:, None], a, b).astype(np.float64)
            want = (t * (second - first) + first).astype(F32)
            assert (x_b[two][pure].view(np.uint32) == want.view(np.uint32)).all(), (name, int((x_b[two][pure] != want).any(axis=1).sum()))
            assert (x_p[two][pure] == first.astype(F32)).all(), name
            checked += int(pure.sum())
            # where the band ends (t -> 0) the blend is the primary sample: |blent - plain| <= t |c2 - c1| + the bar of the values test
            d = np.abs(x_b[two].astype(np.float64) - x_p[two].astype(np.float64))
            assert (d <= tap[two, 4].astype(np.float64)[:, None] * 6.0 + fm.BAR * 6.0).all(), name
    assert checked > 200 and steps > 0, (checked, steps)


# ---------------------------------------------------------------------------------------------------------------------------------
# 5: rgb is the snapshot's transform of the filtered value
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 2, 4], ids=[IDS[1], IDS[2], IDS[4]])
def test_rgb_is_the_snapshot_of_the_filtered_xyz(k):
    sid, src = SOURCES[k]
    hb = handle(sid)
    images = random_images(src, seed=23)
    chosen = [pv for pv in pairs_of(sid) if pv[1].width * pv[1].height > 1][::9] + [pairs_of(sid)[-1]]
    n_src = src.width * src.height
    for di, d in enumerate(DISPLAYS):
        # a total intensity that makes the exposure scale, ((intensity_factor * 0.08f) * npix) / total in fp32, exactly 1/4 on both handles
        c = F32(d["intensity_factor"]) * F32(0.08)
        load(hb, images, landed=float(c * F32(n_src)) * 4.0)
        for vid, view in chosen:
            name = "%s -> %s display %d" % (sid, vid, di)
            out = hb.View(view, src, want=("rgb", "xyz", "map"), filter="bilinear", blend=True, **d)
            second = handle("second-%dx%d" % (view.width, view.height))
            load(second, (out["xyz"],), landed=float(c * F32(view.width * view.height)) * 4.0)
            snap = second.Snapshot(want_xyz=False, **d)[0]
            assert out["rgb"].tobytes() == snap.tobytes(), (name, int((out["rgb"] != snap).any(axis=2).sum()))
            assert len(np.unique(out["rgb"][out["map"] >= 0])) > 8 or (out["map"] >= 0).sum() < 8, name      # (not a black or a white frame)


# ---------------------------------------------------------------------------------------------------------------------------------
# 6: the rest
# ---------------------------------------------------------------------------------------------------------------------------------
def test_two_calls_one_record_and_every_output_alone():
    sid, src = SOURCES[1]
    hb = handle(sid)
    load(hb, random_images(src))
    for vid, view in (vm.small_views()[0], vm.mid_views()[5], vm.mid_views()[11]):
        one = hb.View(view, src, want=ALL5, filter="bilinear", blend=True, **DISPLAYS[2])
        two = hb.View(view, src, want=ALL5, filter="bilinear", blend=True, **DISPLAYS[2])
        for key in ALL5:
            assert one[key].tobytes() == two[key].tobytes(), (vid, key)
            alone = hb.View(view, src, want=(key,), filter="bilinear", blend=True, **DISPLAYS[2])
            assert set(alone) == {key} and alone[key].tobytes() == one[key].tobytes(), (vid, key)
        assert one["tap"].shape == (view.height, view.width, 5) and one["tap"].dtype == F32


def _spec(view, source=None):
    s = abi.HaloViewSpec()
    s.view = view
    s.has_source = 0 if source is None else 1
    if source is not None:
        s.source = source
    s.display = abi.HaloDisplay(1.0, (C.c_float * 3)(-1.0, -1.0, -1.0), (C.c_float * 3)(0.0, 0.0, 0.0))
    return s


def _raw_call(hb, spec, filt, rgb=None, xyz=None, mp=None, d=None, tap=None):
    def ptr(a, t):
        return a.ctypes.data_as(C.POINTER(t)) if a is not None else None
    rc = hb._L.halo_consumer_view_filtered(hb._h, C.byref(spec) if spec is not None else None, C.byref(filt) if filt is not None else None, ptr(rgb, C.c_uint8),
                                           ptr(xyz, C.c_float), ptr(mp, C.c_int32), ptr(d, C.c_float), ptr(tap, C.c_float))
    return rc, (hb._L.halo_last_error(hb._h) or b"").decode()


def test_refusals_come_back_by_name_and_leave_the_handle_usable():
    from ice_halo_sim_amd.backend import HipTraceBackend
    sid, src = SOURCES[0]
    view = vm.small_views()[0][1]
    rgb = np.zeros((view.height, view.width, 3), np.uint8)
    good = abi.HaloViewFilter(abi.VIEW_BILINEAR, 1)
    hb = HipTraceBackend(device=0, seed=9)
    try:
        rc, msg = _raw_call(hb, _spec(view, src), good, rgb=rgb)
        assert rc == abi.HALO_FATAL and "consumer_view_filtered before consumer_fold" in msg
        hb.Consume(random_images(src)[0], 1.0)
        # the filter's own
        rc, msg = _raw_call(hb, _spec(view, src), None, rgb=rgb)
        assert rc == abi.HALO_FATAL and "filter is NULL" in msg
        for f in (2, -1, 7):
            rc, msg = _raw_call(hb, _spec(view, src), abi.HaloViewFilter(f, 0), rgb=rgb)
            assert rc == abi.HALO_FATAL and "unknown filter" in msg
        for bl in (2, -1):
            rc, msg = _raw_call(hb, _spec(view, src), abi.HaloViewFilter(abi.VIEW_BILINEAR, bl), rgb=rgb)
            assert rc == abi.HALO_FATAL and "blend must be 0 or 1" in msg
        for j in (0, 1):
            f = abi.HaloViewFilter(abi.VIEW_NEAREST, 0)
            f.reserved[j] = 1
            rc, msg = _raw_call(hb, _spec(view, src), f, rgb=rgb)
            assert rc == abi.HALO_FATAL and "reserved" in msg
        # halo_consumer_view's
        rc, msg = _raw_call(hb, _spec(view, src), good)
        assert rc == abi.HALO_FATAL and "every output is NULL" in msg
        rc, msg = _raw_call(hb, _spec(view, None), good, rgb=rgb)
        assert rc == abi.HALO_FATAL and "has had no session" in msg
        other = scenes.render(src.lens_type, src.width // 2, src.height, visible=src.visible)
        rc, msg = _raw_call(hb, _spec(view, other), good, rgb=rgb)
        assert rc == abi.HALO_FATAL and "size is not the consumer's" in msg
        for w, h in ((0, 5), (5, 0), (-1, 3)):
            rc, msg = _raw_call(hb, _spec(scenes.render(abi.LENS_LINEAR, w, h, fov=60.0), src), good, rgb=rgb)
            assert rc == abi.HALO_FATAL and "empty view" in msg
        rc, msg = _raw_call(hb, _spec(scenes.render(abi.LENS_LINEAR, 8192, 4097, fov=60.0), src), good, rgb=rgb)
        assert rc == abi.HALO_UNAVAILABLE and "2^25" in msg
        bad = _spec(view, src)
        bad.source.lens_type = 11
        rc, msg = _raw_call(hb, bad, good, rgb=rgb)
        assert rc == abi.HALO_FATAL and "unknown lens type" in msg
        rc, msg = _raw_call(hb, None, good, rgb=rgb)
        assert rc == abi.HALO_FATAL and "spec is NULL" in msg
        with pytest.raises(ValueError):
            hb.View(view, src, filter="cubic")
        with pytest.raises(ValueError):
            hb.View(view, src, want=("taps",))
        sc = scenes.config2_scene()
        hb.BeginSession(sc, src, scenes.wl_discrete(550.0), 64)
        rc, msg = _raw_call(hb, _spec(view, src), good, rgb=rgb)
        assert rc == abi.HALO_FATAL and "inside a session" in msg
        hb.TraceLayer(64)
        hb.EndSession()
        # ... and the handle works: the default source is now the session's render; a tap record alone is an output
        tap = np.zeros((view.height, view.width, 5), F32)
        rc, msg = _raw_call(hb, _spec(view, None), good, rgb=rgb, tap=tap)
        assert rc == abi.HALO_OK, msg
        want = hb.View(view, src, want=("rgb", "tap"), filter="bilinear", blend=True)
        assert rgb.tobytes() == want["rgb"].tobytes() and tap.tobytes() == want["tap"].tobytes()
    finally:
        hb.close()


def test_the_python_wrapper_is_the_c_call():
    sid, src = SOURCES[2]
    hb = handle(sid)
    load(hb, random_images(src))
    vid, view = vm.mid_views()[0]
    n = view.width * view.height
    rgb, xyz, mp, d, tap = np.zeros((n, 3), np.uint8), np.zeros((n, 3), F32), np.zeros(n, np.int32), np.zeros((n, 3), F32), np.zeros((n, 5), F32)
    rc, msg = _raw_call(hb, _spec(view, src), abi.HaloViewFilter(abi.VIEW_BILINEAR, 0), rgb, xyz, mp, d, tap)
    assert rc == abi.HALO_OK, msg
    out = hb.View(view, src, want=ALL5, filter="bilinear")
    assert out["tap"].shape == (view.height, view.width, 5) and out["map"].shape == (view.height, view.width)
    for key, a in zip(ALL5, (rgb, xyz, mp, d, tap)):
        assert out[key].tobytes() == a.tobytes(), key
    # the defaults are the old call: no "tap", nearest, no blend
    old = hb.View(view, src, want=ALL)
    near = hb.View(view, src, want=ALL5, filter="nearest", blend=False)
    for key in ALL:
        assert old[key].tobytes() == near[key].tobytes(), key
    assert (out["xyz"] != old["xyz"]).any()


def test_the_cli_writes_the_filtered_views_bytes(tmp_path):
    from ice_halo_sim_amd import cli, config
    cfg = json.load(open(os.path.join(ROOT, "tests", "golden", "exact_shards_config.json")))
    cfg["scene"]["ray_num"] = 20000
    cfg["render"] = [{"id": 1, "lens": {"type": "dual_fisheye_equal_area", "fov": 180}, "resolution": [256, 128], "visible": "full", "overlap": 0.1}]
    path = str(tmp_path / "view.json")
    json.dump(cfg, open(path, "w"))
    ppm = str(tmp_path / "v.ppm")
    common = ["-f", path, "--deterministic", "--view-lens", "linear", "--view-fov", "60", "--view-az", "180", "--view-el", "0", "--view-size", "160x90", "--auto-ev"]
    assert cli.main(common + ["--out-view", ppm, "--view-filter", "bilinear", "--view-blend"]) == 0
    head = b"P6\n160 90\n255\n"
    data = open(ppm, "rb").read()
    assert data[:len(head)] == head and len(data) == len(head) + 160 * 90 * 3
    res = cli.run_job(config.load_config(path), None, 42, 0, None, deterministic=True)
    be = res["backend"]
    try:
        assert res["render"].overlap > 0.0
        view = scenes.render(abi.LENS_LINEAR, 160, 90, fov=60.0, az=180.0, el=0.0, ro=0.0, visible=abi.VISIBLE_FULL)
        factor = 1.0 * 2.0 ** be.AutoEv(8, 135.0)["ev_auto"]
        out = be.View(view, want=("rgb", "tap"), intensity_factor=factor, filter="bilinear", blend=True)
        assert out["rgb"].tobytes() == data[len(head):]
        assert (out["tap"][..., 4] > 0.0).any()      # the band is on screen
        old = be.View(view, want=("rgb",), intensity_factor=factor)
        assert old["rgb"].tobytes() != out["rgb"].tobytes()
    finally:
        be.close()
