"""halo_consumer_view — the consumer's image through any lens, gathered on the device — held half by half, exactly.

The source image is loaded with halo_consumer_consume into a fresh consumer: pixel i holds X = i + 1, Y = 2 (i + 1), Z = 3 (i + 1), exact in
fp32, so a gathered value names the pixel it came from.  Per (source, view) pair of tests/_view_model.py:
  1. inverse half   dir_out against the float64 model of the inverses: validity equal outside the domain margins, every returned direction
                    lands (under the forward lens model) within EPS of its pixel's centre (tests/test_view_model.py says where the acos allowance
                    of the single-view equidistant / stereographic lenses comes from), zeros where there is no direction;
  2. source half    map_out == the lens model's primary pixel of the DEVICE's fp32 direction under the source render, on every pixel the model
                    calls decidable — no fraction may disagree, and at most 1 % may be undecidable;
  3. values         xyz_out is the raw value of pixel map_out bit for bit (zeros at -1); rgb_out is the snapshot's byte of that pixel under three
                    displays (at -1: the snapshot's value of a zero pixel).
Then: view = source for all eleven lenses (map_out[p] == p), a random image with a non-zero compensation term, the 1920 x 1080 pair whose tiles
outnumber the grid, two calls giving one record, every output alone, every refusal by name, the Python wrapper against the C call, the CLI."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from ice_halo_sim_amd import abi, scenes
from tests import _lens_model as lm
from tests import _view_model as vm

pytestmark = pytest.mark.gpu
F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DISPLAYS = [dict(intensity_factor=1.0, ray_color=(-1.0, -1.0, -1.0), background=(0.0, 0.0, 0.0)),        # true colour
            dict(intensity_factor=1.0, ray_color=(0.9, 0.5, 0.2), background=(0.0, 0.0, 0.0)),           # a ray colour
            dict(intensity_factor=3.0, ray_color=(-1.0, -1.0, -1.0), background=(0.05, 0.1, 0.2))]       # a background, exposed 3 x
ALL = ("rgb", "xyz", "map", "dir")
MEASURE = bool(os.environ.get("HALO_VIEW_MEASURE"))
_handles = {}
_worst = {"px": 0.0, "rim": 0.0, "wz": 0.0, "share": 0.0}


def ramp(render):
    n = render.width * render.height
    i = np.arange(1, n + 1, dtype=np.float64)
    return np.stack([i, 2.0 * i, 3.0 * i], 1).astype(F32).reshape(render.height, render.width, 3)


def loaded(key, render, image=None, more=()):
    """A handle whose consumer holds `image` (default: the ramp) under `render`, with a total intensity that puts the ramp's Y across the display
    range (scale = 1 / (2 n) at intensity_factor 1) — made once per key."""
    if key not in _handles:
        from ice_halo_sim_amd.backend import HipTraceBackend
        hb = HipTraceBackend(device=0, seed=5)
        n = render.width * render.height
        hb.Consume(ramp(render) if image is None else image, 0.08 * n * 2.0 * n)
        for img in more:
            hb.Consume(img, 0.0)
        raw = hb.Snapshot(want_xyz=True)[1].reshape(-1, 3).copy()
        snaps = [hb.Snapshot(want_xyz=False, **d)[0].reshape(-1, 3).copy() for d in DISPLAYS]
        _handles[key] = (hb, raw, snaps)
    return _handles[key]


@pytest.fixture(scope="module", autouse=True)
def _close_handles():
    yield
    for hb, _, _ in _handles.values():
        hb.close()
    _handles.clear()
    if MEASURE:
        print("device, worst over all pairs:", _worst)


def zero_pixel(hb, display):
    """What the snapshot gives a pixel that holds zero: the view's value where it has no source."""
    key = ("zero", json.dumps(display, sort_keys=True))
    if key not in _handles:
        from ice_halo_sim_amd.backend import HipTraceBackend
        z = HipTraceBackend(device=0, seed=5)
        img = np.zeros((1, 2, 3), F32)
        img[0, 1] = 1.0
        z.Consume(img, 1.0)
        _handles[key] = (z, None, z.Snapshot(want_xyz=False, **display)[0].reshape(-1, 3)[0].copy())
    return _handles[key][2]


def check_pair(hb, raw, snaps, src, view, name):
    P_src, P = lm.proj_of(src), lm.proj_of(view)
    x, y = vm.pixel_grid(P)
    out = hb.View(view, src, want=ALL, **DISPLAYS[0])
    dirs, mp, xyz = out["dir"].reshape(-1, 3), out["map"].ravel(), out["xyz"].reshape(-1, 3)
    has = (dirs != 0.0).any(axis=1)
    # 1. the inverse half
    I = vm.inverse64(P, x, y)
    fig = vm.compare(P, _all_decided(I) if MEASURE else I, x, y, has, dirs)      # (HALO_VIEW_MEASURE=1: margins at zero, figures instead of bars)
    for k in ("px", "rim", "wz"):
        _worst[k] = max(_worst[k], fig[k])
    if not MEASURE:
        ok = I.decided()
        assert (has[ok] == I.valid[ok]).all(), (name, int((has[ok] != I.valid[ok]).sum()))
        assert fig["px"] <= vm.EPS, (name, fig["px"])
    assert (mp[~has] == -1).all() and (xyz[~has] == 0.0).all(), name
    # 2. the source half: the lens model on the device's own directions
    if has.any():
        H = lm.project(P_src, dirs[has].astype(np.float64))
        dec = H.decidable()
        want = H.primary_pixel(P_src.w)
        assert (mp[has][dec] == want[dec]).all(), (name, int((mp[has][dec] != want[dec]).sum()))
        _worst["share"] = max(_worst["share"], float((~dec).mean()))
        assert (~dec).mean() <= 0.01, (name, float((~dec).mean()))
    assert ((mp >= -1) & (mp < P_src.w * P_src.h)).all(), name
    # 3. the values
    hit = mp >= 0
    assert (xyz[hit].view(np.uint32) == raw[mp[hit]].view(np.uint32)).all() and (xyz[~hit] == 0.0).all(), name
    for k, d in enumerate(DISPLAYS):
        rgb = out["rgb"].reshape(-1, 3) if k == 0 else hb.View(view, src, want=("rgb",), **d)["rgb"].reshape(-1, 3)
        assert (rgb[hit] == snaps[k][mp[hit]]).all(), (name, k)
        assert (rgb[~hit] == zero_pixel(hb, d)).all(), (name, k)
    return out


def _all_decided(I):
    I.decided = lambda delta=None: np.ones(len(I.valid), bool)
    return I


SOURCES = vm.sources()


@pytest.mark.parametrize("k", range(len(SOURCES)), ids=[s[0] for s in SOURCES])
def test_every_view_of_a_source(k):
    sid, src = SOURCES[k]
    hb, raw, snaps = loaded(sid, src)
    n = 0
    for s2, _, vid, view in vm.pairs():
        if s2 == sid:
            check_pair(hb, raw, snaps, src, view, sid + " -> " + vid)
            n += 1
    assert n >= len(vm.small_views()) + len(vm.mid_views()) // 3


def test_the_pair_whose_tiles_outnumber_the_grid():
    sid, src, vid, view = vm.BIG_PAIR      # 8160 tiles of 16 x 16 pixels: the launcher's grid is capped below that, workgroups stride over tiles
    hb, raw, snaps = loaded(sid, src)
    out = check_pair(hb, raw, snaps, src, view, sid + " -> " + vid)
    assert (out["map"] >= 0).mean() > 0.99


def test_identity_for_all_eleven_lenses():
    seen = set()
    for name, r in vm.identity_renders():
        hb, raw, snaps = loaded("id-%dx%d" % (r.width, r.height), r)     # (the ramp depends on the size alone: one handle per size)
        out = hb.View(r, r, want=ALL, **DISPLAYS[0])
        dirs, mp = out["dir"].reshape(-1, 3), out["map"].ravel()
        has = (dirs != 0.0).any(axis=1)
        assert has.any(), name
        assert (mp[has] == np.flatnonzero(has)).all(), (name, int((mp[has] != np.flatnonzero(has)).sum()))
        assert (out["xyz"].reshape(-1, 3)[has].view(np.uint32) == raw[has].view(np.uint32)).all(), name
        assert (out["rgb"].reshape(-1, 3)[has] == snaps[0][has]).all(), name
        seen.add(r.lens_type)
    assert seen == set(range(11))


def test_random_image_with_a_compensation_term():
    sid, src = SOURCES[0]
    g = np.random.default_rng(11)
    a = g.uniform(0.5, 2.0, (src.height, src.width, 3)).astype(F32)
    b = (g.uniform(0.5, 2.0, (src.height, src.width, 3)) * 1e-4).astype(F32)     # a second fold whose low bits the sum drops: comp != 0
    hb, raw, snaps = loaded("random", src, image=a, more=(b,))
    assert (raw.astype(np.float64) - a.reshape(-1, 3).astype(np.float64) > 0).all()
    for vid, view in vm.small_views()[:6] + vm.mid_views()[:3]:
        check_pair(hb, raw, snaps, src, view, "random -> " + vid)


def test_two_calls_one_record_and_every_output_alone():
    sid, src = SOURCES[1]
    hb, raw, snaps = loaded(sid, src)
    for vid, view in (vm.small_views()[0], vm.mid_views()[5], vm.mid_views()[11]):
        one = hb.View(view, src, want=ALL, **DISPLAYS[2])
        two = hb.View(view, src, want=ALL, **DISPLAYS[2])
        for k in ALL:
            assert one[k].tobytes() == two[k].tobytes(), (vid, k)
            alone = hb.View(view, src, want=(k,), **DISPLAYS[2])
            assert set(alone) == {k} and alone[k].tobytes() == one[k].tobytes(), (vid, k)


def _raw_call(hb, spec, rgb=None, xyz=None, mp=None, d=None):
    def ptr(a, t):
        return a.ctypes.data_as(C.POINTER(t)) if a is not None else None
    rc = hb._L.halo_consumer_view(hb._h, C.byref(spec) if spec is not None else None, ptr(rgb, C.c_uint8), ptr(xyz, C.c_float), ptr(mp, C.c_int32), ptr(d, C.c_float))
    return rc, (hb._L.halo_last_error(hb._h) or b"").decode()


def _spec(view, source=None):
    s = abi.HaloViewSpec()
    s.view = view
    s.has_source = 0 if source is None else 1
    if source is not None:
        s.source = source
    s.display = abi.HaloDisplay(1.0, (C.c_float * 3)(-1.0, -1.0, -1.0), (C.c_float * 3)(0.0, 0.0, 0.0))
    return s


def test_refusals_come_back_by_name_and_leave_the_handle_usable():
    from ice_halo_sim_amd.backend import HipTraceBackend
    sid, src = SOURCES[0]
    view = vm.small_views()[0][1]
    rgb = np.zeros((view.height, view.width, 3), np.uint8)
    hb = HipTraceBackend(device=0, seed=9)
    try:
        rc, msg = _raw_call(hb, _spec(view, src), rgb=rgb)
        assert rc == abi.HALO_FATAL and "before consumer_fold" in msg
        hb.Consume(ramp(src), 1.0)
        rc, msg = _raw_call(hb, _spec(view, src))
        assert rc == abi.HALO_FATAL and "every output is NULL" in msg
        rc, msg = _raw_call(hb, _spec(view, None), rgb=rgb)
        assert rc == abi.HALO_FATAL and "has had no session" in msg
        other = scenes.render(src.lens_type, src.width // 2, src.height, visible=src.visible)
        rc, msg = _raw_call(hb, _spec(view, other), rgb=rgb)
        assert rc == abi.HALO_FATAL and "size is not the consumer's" in msg
        for w, h in ((0, 5), (5, 0), (-1, 3)):
            rc, msg = _raw_call(hb, _spec(scenes.render(abi.LENS_LINEAR, w, h, fov=60.0), src), rgb=rgb)
            assert rc == abi.HALO_FATAL and "empty view" in msg
        rc, msg = _raw_call(hb, _spec(scenes.render(abi.LENS_LINEAR, 8192, 4097, fov=60.0), src), rgb=rgb)
        assert rc == abi.HALO_UNAVAILABLE and "2^25" in msg
        rc, msg = _raw_call(hb, None, rgb=rgb)
        assert rc == abi.HALO_FATAL
        # inside a session (on a handle whose consumer has the session's size, so nothing else refuses first)
        sc = scenes.config2_scene()
        hb.BeginSession(sc, src, scenes.wl_discrete(550.0), 64)
        rc, msg = _raw_call(hb, _spec(view, src), rgb=rgb)
        assert rc == abi.HALO_FATAL and "inside a session" in msg
        hb.TraceLayer(64)
        hb.EndSession()
        # ... and the handle works: the default source is now the session's render
        rc, msg = _raw_call(hb, _spec(view, None), rgb=rgb)
        assert rc == abi.HALO_OK, msg
        want = hb.View(view, src, want=("rgb",))["rgb"]
        assert rgb.tobytes() == want.tobytes()
    finally:
        hb.close()


def test_the_python_wrapper_is_the_c_call():
    sid, src = SOURCES[2]
    hb, raw, snaps = loaded(sid, src)
    vid, view = vm.mid_views()[0]
    n = view.width * view.height
    rgb, xyz, mp, d = np.zeros((n, 3), np.uint8), np.zeros((n, 3), F32), np.zeros(n, np.int32), np.zeros((n, 3), F32)
    s = _spec(view, src)
    rc, msg = _raw_call(hb, s, rgb, xyz, mp, d)
    assert rc == abi.HALO_OK, msg
    out = hb.View(view, src, want=ALL)
    assert out["rgb"].shape == (view.height, view.width, 3) and out["map"].shape == (view.height, view.width) and out["map"].dtype == np.int32
    for k, a in zip(ALL, (rgb, xyz, mp, d)):
        assert out[k].tobytes() == a.tobytes(), k


def test_the_cli_writes_the_views_bytes(tmp_path):
    from ice_halo_sim_amd import cli, config
    cfg = json.load(open(os.path.join(ROOT, "tests", "golden", "exact_shards_config.json")))
    cfg["scene"]["ray_num"] = 20000
    cfg["render"] = [{"id": 1, "lens": {"type": "dual_fisheye_equal_area", "fov": 180}, "resolution": [256, 128], "visible": "full"}]
    path = str(tmp_path / "view.json")
    json.dump(cfg, open(path, "w"))
    ppm, whole = str(tmp_path / "v.ppm"), str(tmp_path / "whole.ppm")
    argv = ["-f", path, "--deterministic", "--out-view", ppm, "--out-rgb", whole, "--view-lens", "linear", "--view-fov", "60", "--view-az", "180",
            "--view-el", "25", "--view-size", "160x90", "--auto-ev"]
    assert cli.main(argv) == 0
    head = b"P6\n160 90\n255\n"
    data = open(ppm, "rb").read()
    assert data[:len(head)] == head and len(data) == len(head) + 160 * 90 * 3
    # the same deterministic trace again, here: its view must be the file's bytes
    res = cli.run_job(config.load_config(path), None, 42, 0, None, deterministic=True)
    be = res["backend"]
    try:
        view = scenes.render(abi.LENS_LINEAR, 160, 90, fov=60.0, az=180.0, el=25.0, ro=0.0, visible=abi.VISIBLE_FULL)
        factor = 1.0 * 2.0 ** be.AutoEv(8, 135.0)["ev_auto"]       # --auto-ev: the EV of the consumer's image, not of the view
        out = be.View(view, want=("rgb", "map"), intensity_factor=factor)      # (source: the handle's last session's render)
        assert out["rgb"].tobytes() == data[len(head):]
        assert (out["map"] >= 0).all()
        snap = be.Snapshot(want_xyz=False, auto_ev=True)[0]
        assert open(whole, "rb").read().endswith(snap.tobytes())
        assert (out["rgb"].reshape(-1, 3) == snap.reshape(-1, 3)[out["map"].ravel()]).all()
    finally:
        be.close()
