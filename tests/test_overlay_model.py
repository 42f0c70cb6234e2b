"""The rule of the view stage's auxiliary lines on the host (halo_host_view_sky, halo_host_view_overlay_pixel, halo_host_view_overlay_defaults:
ice_halo_sim_amd/csrc/halo_overlay.h, the code the device pass runs) against the float64 model of tests/_overlay_model.py.  No GPU.
HALO_OVERLAY_MEASURE=1 prints the figures _overlay_model.MEASURED is made of instead of asserting them."""
import ctypes as C
import os

import numpy as np
import pytest

from ice_halo_sim_amd import abi, backend, scenes

from tests import _overlay_model as om
from tests import _view_model as vm

MEASURE = bool(os.environ.get("HALO_OVERLAY_MEASURE"))
SUN = (25.0, 10.0)


@pytest.fixture(scope="module")
def view_dirs():
    """{view id: (view, dir float32[h, w, 3], has bool[h, w])} of every test view, by the host's own view_direction."""
    return {vid: (view,) + om.host_dirs(view) for vid, view in vm.all_views()}


def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v)


def _special_dirs(sun):
    """The poles, the horizon, the azimuth seam on both sides, and directions within 1e-6 of the sun and of its antipode."""
    out = [(0, 0, -1), (0, 0, 1), (-1, 0, 0), (0, -1, 0), (1, 0, 0), (1, 1e-7, 0), (1, -1e-7, 0), (1, 0.0, 1e-7), (1e-7, 0, -1), (0, -1e-7, 1),
           (-0.6, 0.8, 0.0), (-0.6, 0.8, 1e-8), (-0.6, 0.8, -1e-8)]
    s = np.asarray(sun, np.float64)
    a = _unit(np.cross(s, (0.0, 0.0, 1.0)))
    b = np.cross(s, a)
    for sign in (1.0, -1.0):
        out.append(sign * s)
        for eps in (1e-6, 3e-7, 1e-7):
            for t in (a, -a, b, -b, _unit(a + b)):
                out.append(_unit(sign * s + eps * t))
    return np.array(out, np.float64).astype(np.float32)


def test_sky_coordinates_against_the_model(view_dirs):
    sun = om.overlay(60.0, SUN).sun_dir
    sun = np.array(list(sun), np.float32)
    dirs = [d[has] for _, d, has in view_dirs.values()] + [_special_dirs(sun)]
    worst = 0.0
    for d in dirs:
        if len(d):
            worst = max(worst, om.sky_deviation(om.host_sky(d, sun), om.sky64(d, sun)))
    if MEASURE:
        print("\nhost sky deviation: %.3g degrees over %d directions" % (worst, sum(len(d) for d in dirs)))
        return
    assert worst <= om.DELTA["sky"], worst
    assert om.host_sky([(0, 0, -1)], sun)[0, 0] == pytest.approx(90.0, abs=1e-4) and om.host_sky([(0, 0, 1)], sun)[0, 0] == pytest.approx(-90.0, abs=1e-4)
    assert abs(om.host_sky([sun], sun)[0, 2]) < 1e-4 and abs(om.host_sky([-sun], sun)[0, 2] - 180.0) < 1e-4


def _view_case(view, d, has, o):
    """Everything a pixel test needs of one view: base bytes, the host's fp32 sky6, pixel coordinates, marks — of the pixels that have a direction."""
    h, w = has.shape
    sun = np.array(list(o.sun_dir), np.float32)
    sky3 = np.zeros((h, w, 3), np.float32)
    sky3[has] = om.host_sky(d[has], sun)
    sky6 = np.concatenate([sky3, om.footprint32(sky3, has)], -1)
    ys, xs = np.mgrid[0:h, 0:w]
    xy = np.stack([xs, ys], -1).astype(np.float32)
    rng = np.random.default_rng(w * 1000 + h)
    base = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    return base[has], sky6[has], xy[has], om.host_marks(view, sun)


def test_pixel_values_against_the_model(view_dirs):
    worst, n = 0.0, 0
    for vid, (view, d, has) in view_dirs.items():
        if not has.any():
            continue
        for o in (om.overlay(view.fov, SUN), om.overlay(view.fov, (-40.0, 200.0), grid_step_deg=7.5, sun_circle_count=3, sun_circle_deg=(9.0, 22.0, 120.0),
                                                          zenith_nadir_radius_px=3.0, sun_marker_radius_px=2.5)):
            base, sky6, xy, marks = _view_case(view, d, has, o)
            got = om.host_pixels(base, sky6, xy, marks, o)
            worst = max(worst, float(np.abs(got - om.value64(base, sky6, xy, marks, o)).max()))
            n += len(base)
            assert (om.rgb_of(got) == np.floor(np.clip(got.astype(np.float64), 0, 255) + 0.5)).all()
    if MEASURE:
        print("\nhost value deviation: %.3g byte units over %d pixels" % (worst, n))
        return
    assert worst <= om.DELTA["value"], worst


def test_footprints_of_the_model_rule():
    """footprint32 itself, on cases worked by hand: a lone pixel, the seam's wrap, a missing partner's fallback, a missing pixel."""
    f32 = np.float32
    one = om.footprint32(np.zeros((1, 1, 3), f32), np.ones((1, 1), bool))
    assert (one == f32(1e-4)).all()
    sky = np.zeros((1, 3, 3), f32)
    sky[0, :, 1] = (179.5, -179.75, -179.0)
    fw = om.footprint32(sky, np.ones((1, 3), bool))
    assert fw[0, 0, 1] == f32(0.75) and fw[0, 1, 1] == f32(0.75)          # wrapped: 179.5 -> -179.75 is 0.75, not 359.25
    assert fw[0, 2, 1] == f32(0.75)                                         # x = 2 is even, its partner x = 3 lies outside: the fallback x = 1
    has = np.array([[True, False, True]])
    fw = om.footprint32(sky, has)
    assert fw[0, 0, 1] == f32(1e-4) and (fw[0, 1] == 0).all()               # x = 0: partner without a direction, no x = -1: the lower clamp
    assert fw[0, 2, 1] == f32(1e-4)                                         # x = 2: partner outside, fallback x = 1 without a direction
    sky = np.zeros((2, 2, 3), f32)
    sky[..., 0] = [[0.0, 1.0], [3.0, 9.0]]
    fw = om.footprint32(sky, np.ones((2, 2), bool))
    assert fw[0, 0, 0] == f32(2.0) and fw[1, 1, 0] == f32(2.0) and fw[0, 1, 0] == f32(2.0)   # 1 + 3 clamped to 2; 6 + 8; 1 + 8


def test_exact_cases(view_dirs):
    view, d, has = view_dirs["l0-96-flat-upper"]
    o = om.overlay(view.fov, (8.0, 3.0), sun_marker_alpha=1.0, sun_marker_radius_px=6.0)
    base, sky6, xy, marks = _view_case(view, d, has, o)
    assert marks[8] == 1.0
    got = om.host_pixels(base, sky6, xy, marks, o)
    far = ~om.reach(sky6, xy, marks, o, margin=1e-3)
    assert far.any() and (~far).any()
    assert (got[far] == base[far].astype(np.float32)).all()       # at least 1.5 fw from every line, radius + 1.5 from every mark: the base, to the bit
    r = np.hypot(xy[:, 0] - marks[6], xy[:, 1] - marks[7])
    inside = r <= 6.0 - 1.5 - 1e-3
    m = (np.array(list(o.sun_marker_color), np.float32) * np.float32(255.0)).astype(np.float32)
    assert inside.any() and (got[inside] == m[None, :]).all()     # the marker at alpha 1: its colour, to the bit
    # k = 0 and k = 1 by the layers' alphas: every alpha 0 leaves c; the horizon alone at alpha 1, on the horizon itself, gives m
    zero = om.overlay(view.fov, (8.0, 3.0), horizon_alpha=0.0, grid_alpha=0.0, sun_circles_alpha=0.0, zenith_nadir_alpha=0.0, sun_marker_alpha=0.0)
    assert (om.host_pixels(base, sky6, xy, marks, zero) == base.astype(np.float32)).all()
    off = om.overlay(view.fov, (8.0, 3.0), layers=())
    assert (om.host_pixels(base, sky6, xy, marks, off) == base.astype(np.float32)).all()
    hor = om.overlay(view.fov, (8.0, 3.0), layers=("horizon",), horizon_alpha=1.0)
    on = sky6.copy()
    on[:, 0] = 0.0
    hm = (np.array(list(hor.horizon_color), np.float32) * np.float32(255.0)).astype(np.float32)
    assert (om.host_pixels(base, on, xy, marks, hor) == hm[None, :]).all()


def test_defaults_and_layout():
    L = backend.load_library()
    for fov, step in ((120.0, 30.0), (119.99, 20.0), (60.0, 20.0), (59.99, 10.0), (30.0, 10.0), (29.99, 5.0), (15.0, 5.0), (14.99, 2.0), (6.0, 2.0), (5.99, 1.0),
                      (2.0, 1.0), (1.99, 0.5), (180.0, 30.0), (0.1, 0.5)):
        assert backend.view_overlay(fov).grid_step_deg == step == om.grid_step(fov), fov
    o = backend.view_overlay(60.0, SUN)
    assert [o.show_horizon, o.show_grid, o.show_sun_circles, o.show_zenith_nadir, o.show_sun_marker] == [0] * 5
    assert o.sun_circle_count == 2 and list(o.sun_circle_deg)[:3] == [22.0, 46.0, 0.0]
    f32 = np.float32

    def col(c):
        return [f32(v) for v in c]
    assert col(o.horizon_color) == col((0.8, 0.2, 0.2)) and o.horizon_alpha == f32(0.6)
    assert col(o.grid_color) == col((1, 1, 1)) and o.grid_alpha == f32(0.3)
    assert col(o.sun_circles_color) == col((1, 0.9, 0.3)) and o.sun_circles_alpha == f32(0.5)
    assert col(o.zenith_nadir_color) == col((0.8, 0.2, 0.2)) and o.zenith_nadir_alpha == f32(0.6) and o.zenith_nadir_radius_px == 8.0
    assert col(o.sun_marker_color) == col((1, 0.9, 0.3)) and o.sun_marker_alpha == f32(0.75) and o.sun_marker_radius_px == 5.0
    assert list(o.reserved) == [0, 0]
    assert np.abs(np.array(list(o.sun_dir)) - om.sun_dir64(*SUN)).max() < 2e-7
    assert list(backend.view_overlay(60.0).sun_dir) == [0.0, 0.0, -1.0]
    # the layout: 200 bytes, the library's size, the offsets of the header's fields
    assert C.sizeof(abi.HaloViewOverlay) == 200 == L.halo_host_view_overlay_defaults(60.0, None, C.byref(abi.HaloViewOverlay()))
    off = {n: getattr(abi.HaloViewOverlay, n).offset for n, _ in abi.HaloViewOverlay._fields_}
    assert off == {"show_horizon": 0, "show_grid": 4, "show_sun_circles": 8, "show_zenith_nadir": 12, "show_sun_marker": 16, "grid_step_deg": 20, "sun_dir": 24,
                   "sun_circle_count": 36, "sun_circle_deg": 40, "horizon_color": 104, "horizon_alpha": 116, "grid_color": 120, "grid_alpha": 132,
                   "sun_circles_color": 136, "sun_circles_alpha": 148, "zenith_nadir_color": 152, "zenith_nadir_alpha": 164, "sun_marker_color": 168,
                   "sun_marker_alpha": 180, "zenith_nadir_radius_px": 184, "sun_marker_radius_px": 188, "reserved": 192}
    assert L.halo_host_view_overlay_defaults(60.0, None, None) == 0
    assert L.halo_abi_sizeof(17) == 0 and L.halo_abi_version() == 6   # the struct has no index in the size table; the ABI stays


def test_the_margins_are_what_was_measured():
    assert om.FACTOR == 4.0 and set(om.DELTA) == set(om.MEASURED) == {"sky", "value"}
    for k in om.DELTA:
        assert om.DELTA[k] == 4.0 * om.MEASURED[k]


def test_the_wrappers_refuse_what_they_cannot_pass_on():
    with pytest.raises(ValueError):
        backend.view_overlay(60.0, SUN, layers=("halo",))
    with pytest.raises(ValueError):
        backend.view_overlay(60.0, SUN, circles=[1.0] * 17)
    o = backend.view_overlay(60.0, SUN, layers=("grid", "sun"), circles=(9, 22, 46), grid_step=2.5)
    assert (o.show_grid, o.show_sun_marker, o.show_horizon, o.sun_circle_count, o.grid_step_deg) == (1, 1, 0, 3, 2.5)
    o.sun_circle_count = 17
    with pytest.raises(ValueError):
        backend.host_view_overlay_pixel((1, 2, 3), np.zeros(6), (0, 0), np.zeros(9), o)
