"""A float64 model of the view stage's auxiliary lines (halo_consumer_view_overlay, ice_halo_sim_amd/csrc/halo_overlay.h) and what its tests share.

Written from the rule, not from any shader.  Per view pixel with travel direction w (sky position -w), the sun's travel direction s, D = 57.29578f:
    sky        alt = atan2(-wz, sqrt(wx^2 + wy^2)) D;  az = atan2(-wy, -wx) D in [-180, 180];  dist = atan2(|w x s|, w . s) D
    footprint  fw(q) = |q(x ^ 1, y) - q| + |q(x, y ^ 1) - q|; a partner outside the view or without a direction is replaced by the pixel's other
               neighbour on that axis (x - 1 for even x, x + 1 for odd x), a term with neither is 0; the azimuth difference is wrapped once
               (d > 180: d - 360; d < -180: d + 360); fw_alt, fw_dist in [1e-4, 2], fw_az in [1e-4, 5]
    coverage   smoothstep(e0, e1, x) = t t (3 - 2 t), t = clamp((x - e0) / (e1 - e0), 0, 1);  cover(d, fw) = 1 - smoothstep(0, 1.5 fw, d)
    mixing     c = float(byte), m = colour 255, c <- m k + c (1 - k); layers: grid, circles in list order, horizon, zenith ring, nadir ring, marker
sky64 and value64 evaluate this in float64 (the inputs promoted, every operation in float64: no rounding shared with the fp32 code);
footprint32 evaluates the footprint rule in numpy fp32, operation for operation as the header spells it: the device's sky_out[3:6] must equal it
to the bit.

MEASURED holds the largest deviations of the fp32 code from the model; the tests hold the code to DELTA = 4 x MEASURED (_lens_model.py's rule: libm
differs between host and device by a few ulp).  HALO_OVERLAY_MEASURE=1 makes tests/test_overlay_model.py (host) and tests/test_gpu_view_overlay.py
(device) print their figures instead of asserting them.
#                 host        device (MI355X)   MEASURED (the larger)
#   sky (deg)     1.97e-5     2.51e-5           2.51e-5     |alt|, |az| (around the circle) and |dist| against sky64 at the same fp32 direction: an ulp
#                                                            of 180 is 1.5e-5; near the sun and its antipode the fp32 cross product carries 1e-7 rad
#   value (byte)  8.28e-4     2.75e-2           2.75e-2     value_out against value64 fed the same fp32 sky6 and bytes.  az + 180 + step / 2 is rounded
#                                                            to an ulp of 256 (3e-5 degrees) before the modulo; the coverage falls from 1 to 0 over
#                                                            1.5 footprints, so the finer the view's pixels the more of a byte that ulp is: the host's
#                                                            views have footprints of a degree, the device's include a 1920 x 1080 view at 0.03 degrees
"""
import ctypes as C

import numpy as np

from ice_halo_sim_amd import abi

MEASURED = {"sky": 2.51e-5, "value": 2.75e-2}
FACTOR = 4.0
DELTA = {k: FACTOR * v for k, v in MEASURED.items()}

D32 = np.float32(57.29578)
D = float(D32)
ZENITH, NADIR = (0.0, 0.0, -1.0), (0.0, 0.0, 1.0)   # travel directions


def sky64(dirs, sun):
    """dirs[n, 3], sun[3] -> float64[n, 3] = alt, az, dist in degrees."""
    w = np.asarray(dirs, np.float64).reshape(-1, 3)
    s = np.asarray(sun, np.float64).reshape(3)
    alt = np.arctan2(-w[:, 2], np.hypot(w[:, 0], w[:, 1])) * D
    az = np.arctan2(-w[:, 1], -w[:, 0]) * D
    dist = np.arctan2(np.linalg.norm(np.cross(w, s[None, :]), axis=1), w @ s) * D
    return np.stack([alt, az, dist], 1)


def sky_deviation(got, want):
    """The largest |difference| of fp32 sky coordinates got[n, 3] from the model's want[n, 3]; the azimuth's taken around the circle (-180 is 180)."""
    d = np.abs(np.asarray(got, np.float64) - want)
    d[:, 1] = np.minimum(d[:, 1], 360.0 - d[:, 1])
    return float(d.max()) if d.size else 0.0


def footprint32(sky3, has):
    """sky3 float32[h, w, 3], has bool[h, w] -> float32[h, w, 3] = fw_alt, fw_az, fw_dist (zeros where has is False): the header's fp32 operations."""
    sky3 = np.asarray(sky3, np.float32)
    h, w = has.shape
    f32 = np.float32
    ys, xs = np.mgrid[0:h, 0:w]

    def term(nx, ny, fx, fy):
        """|q(neighbour) - q| with the partner (nx, ny), else the fallback (fx, fy), else 0"""
        out = np.zeros((h, w, 3), f32)
        done = np.zeros((h, w), bool)
        for ax, ay in ((nx, ny), (fx, fy)):
            ok = (ax >= 0) & (ax < w) & (ay >= 0) & (ay < h)
            cx, cy = np.clip(ax, 0, w - 1), np.clip(ay, 0, h - 1)
            ok &= has[cy, cx] & ~done
            d = sky3[cy, cx] - sky3          # (fp32 - fp32: one rounding)
            daz = d[..., 1]
            daz = np.where(daz > f32(180.0), daz - f32(360.0), np.where(daz < f32(-180.0), daz + f32(360.0), daz))
            d = np.stack([d[..., 0], daz, d[..., 2]], -1)
            out[ok] = np.abs(d)[ok]
            done |= ok
        return out
    odd_x, odd_y = (xs & 1) == 1, (ys & 1) == 1
    tx = term(xs ^ 1, ys, np.where(odd_x, xs + 1, xs - 1), ys)
    ty = term(xs, ys ^ 1, xs, np.where(odd_y, ys + 1, ys - 1))
    fw = tx + ty
    hi = np.array([2.0, 5.0, 2.0], f32)
    fw = np.minimum(np.maximum(fw, f32(1e-4)), hi[None, None, :])
    fw[~has] = 0.0
    assert fw.dtype == np.float32
    return fw


def _smoothstep(e0, e1, x):
    t = np.clip((x - e0) / (e1 - e0), 0.0, 1.0)
    return t * t * (3.0 - 2.0 * t)


def _cover(d, fw):
    return 1.0 - _smoothstep(0.0, 1.5 * fw, d)


def _mod(x, g):
    return x - g * np.floor(x / g)


def _f(v):
    return float(np.float32(v))


def layers(sky6, xy, marks, o):
    """The layers of the record `o` (abi.HaloViewOverlay) in drawing order, in float64: [(name, colour[3] in byte units, k[n], reach[n])] — k the
    mixing weight, reach the distance in units of the layer's fade (< 1: the layer can touch the pixel; >= 1: its weight is exactly 0)."""
    sky6 = np.asarray(sky6, np.float64).reshape(-1, 6)
    xy = np.asarray(xy, np.float64).reshape(-1, 2)
    marks = np.asarray(marks, np.float64).reshape(3, 3)
    alt, az, dist, fw_alt, fw_az, fw_dist = sky6.T
    out = []

    def colour(c):
        return np.array([_f(v) for v in c], np.float64) * 255.0
    if o.show_grid:
        step = _f(o.grid_step_deg)
        h = step / 2.0
        d_alt = np.abs(_mod(np.abs(alt) + h, step) - h)
        d_az = np.abs(_mod(az + 180.0 + h, step) - h)
        low = np.abs(alt) < 85.0
        t = np.maximum(_cover(d_alt, fw_alt), np.where(low, _cover(d_az, fw_az), 0.0))
        reach = np.minimum(d_alt / (1.5 * fw_alt), np.where(low, d_az / (1.5 * fw_az), np.inf))
        out.append(("grid", colour(o.grid_color), t * _f(o.grid_alpha), reach))
    if o.show_sun_circles:
        for i in range(o.sun_circle_count):
            d = np.abs(dist - _f(o.sun_circle_deg[i]))
            out.append(("circle%d" % i, colour(o.sun_circles_color), _cover(d, fw_dist) * _f(o.sun_circles_alpha), d / (1.5 * fw_dist)))
    if o.show_horizon:
        out.append(("horizon", colour(o.horizon_color), _cover(np.abs(alt), fw_alt) * _f(o.horizon_alpha), np.abs(alt) / (1.5 * fw_alt)))
    if o.show_zenith_nadir:
        radius = _f(o.zenith_nadir_radius_px)
        for m, name in ((0, "zenith"), (1, "nadir")):
            if marks[m, 2] == 0.0:
                continue
            r = np.hypot(xy[:, 0] - marks[m, 0], xy[:, 1] - marks[m, 1])
            d = np.abs(r - radius)
            out.append((name, colour(o.zenith_nadir_color), (1.0 - _smoothstep(0.0, 1.5, d)) * _f(o.zenith_nadir_alpha), d / 1.5))
    if o.show_sun_marker and marks[2, 2] != 0.0:
        radius = _f(o.sun_marker_radius_px)
        r = np.hypot(xy[:, 0] - marks[2, 0], xy[:, 1] - marks[2, 1])
        out.append(("sun", colour(o.sun_marker_color), (1.0 - _smoothstep(radius - 1.5, radius + 1.5, r)) * _f(o.sun_marker_alpha), (r - (radius - 1.5)) / 3.0))
    return out


def value64(base, sky6, xy, marks, o):
    """base uint8[n, 3], sky6[n, 6], xy[n, 2] (pixel coordinates), marks[9], o -> float64[n, 3]: the colour after the last layer of pixels that
    HAVE a direction."""
    c = np.asarray(base).reshape(-1, 3).astype(np.float64)
    for _, m, k, _ in layers(sky6, xy, marks, o):
        c = m[None, :] * k[:, None] + c * (1.0 - k[:, None])
    return c


def reach(sky6, xy, marks, o, margin=0.0):
    """bool[n]: some layer of `o` with a positive alpha can touch the pixel — it lies nearer than (1 + margin) fades to a line or a mark."""
    sky6 = np.asarray(sky6, np.float64).reshape(-1, 6)
    hit = np.zeros(len(sky6), bool)
    alphas = {"grid": o.grid_alpha, "circle": o.sun_circles_alpha, "horizon": o.horizon_alpha, "zenith": o.zenith_nadir_alpha, "nadir": o.zenith_nadir_alpha,
              "sun": o.sun_marker_alpha}
    for name, _, _, r in layers(sky6, xy, marks, o):
        if alphas[name.rstrip("0123456789")] > 0.0:
            hit |= r < 1.0 + margin
    return hit


def rgb_of(value):
    """uint8 of fp32 values: floor(clamp(value, 0, 255) + 0.5), in fp32."""
    v = np.asarray(value, np.float32)
    return np.floor(np.minimum(np.maximum(v, np.float32(0.0)), np.float32(255.0)) + np.float32(0.5)).astype(np.uint8)


def sun_dir64(alt_deg, az_deg):
    a, z = np.radians(alt_deg), np.radians(az_deg)
    return np.array([-np.cos(a) * np.cos(z), -np.cos(a) * np.sin(z), -np.sin(a)])


def grid_step(fov):
    for bound, step in ((120.0, 30.0), (60.0, 20.0), (30.0, 10.0), (15.0, 5.0), (6.0, 2.0), (2.0, 1.0)):
        if fov >= bound:
            return step
    return 0.5


# ---- the host functions over arrays ----------------------------------------------------------------------------------------------------
def host_sky(dirs, sun):
    """float32[n, 3] of halo_host_view_sky over dirs[n, 3] float32."""
    from ice_halo_sim_amd import backend
    fn = backend.load_library().halo_host_view_sky
    dirs = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
    s = np.ascontiguousarray(sun, np.float32)
    out = np.zeros((len(dirs), 3), np.float32)
    f32p = C.POINTER(C.c_float)
    sp, bd, bo = s.ctypes.data_as(f32p), dirs.ctypes.data, out.ctypes.data
    for i in range(len(dirs)):
        fn(C.cast(bd + 12 * i, f32p), sp, C.cast(bo + 12 * i, f32p))
    return out


def host_pixels(base, sky6, xy, marks, o):
    """float32[n, 3] of halo_host_view_overlay_pixel over base uint8[n, 3], sky6 float32[n, 6], xy float32[n, 2]."""
    from ice_halo_sim_amd import backend
    fn = backend.load_library().halo_host_view_overlay_pixel
    base = np.ascontiguousarray(base, np.uint8).reshape(-1, 3)
    sky6 = np.ascontiguousarray(sky6, np.float32).reshape(-1, 6)
    xy = np.ascontiguousarray(xy, np.float32).reshape(-1, 2)
    m = np.ascontiguousarray(marks, np.float32).reshape(9)
    out = np.zeros((len(base), 3), np.float32)
    f32p, u8p = C.POINTER(C.c_float), C.POINTER(C.c_uint8)
    mp, ref = m.ctypes.data_as(f32p), C.byref(o)
    bb, bs, bx, bo = base.ctypes.data, sky6.ctypes.data, xy.ctypes.data, out.ctypes.data
    for i in range(len(base)):
        assert fn(C.cast(bb + 3 * i, u8p), C.cast(bs + 24 * i, f32p), C.cast(bx + 8 * i, f32p), mp, ref, C.cast(bo + 12 * i, f32p)) == 1
    return out


def host_dirs(view):
    """(dir float32[h, w, 3], has bool[h, w]) of halo_host_view_direction over every pixel of the HaloRender `view`."""
    from ice_halo_sim_amd import backend
    fn = backend.load_library().halo_host_view_direction
    h, w = int(view.height), int(view.width)
    d = np.zeros((h, w, 3), np.float32)
    has = np.zeros((h, w), bool)
    f32p = C.POINTER(C.c_float)
    ref, bd = C.byref(view), d.ctypes.data
    for y in range(h):
        for x in range(w):
            has[y, x] = fn(ref, x, y, C.cast(bd + 12 * (y * w + x), f32p)) != 0
    return d, has


def host_marks(view, sun):
    """float32[9]: {x, y, present} of zenith, nadir and sun under `view` by halo_host_view_source_pos."""
    from ice_halo_sim_amd import backend
    out = np.zeros(9, np.float32)
    for m, d in enumerate((ZENITH, NADIR, tuple(float(v) for v in sun))):
        n, pos = backend.host_view_source_pos(view, d)
        if n > 0:
            out[3 * m:3 * m + 3] = pos[0], pos[1], 1.0
    return out


def overlay(fov, sun_alt_az=(25.0, 10.0), layers=("horizon", "grid", "circles", "zenith", "sun"), **fields):
    """backend.view_overlay with fields of the record overwritten (colours and arrays as sequences)."""
    from ice_halo_sim_amd import backend
    o = backend.view_overlay(fov, sun_alt_az, layers)
    for k, v in fields.items():
        if isinstance(v, (tuple, list)):
            arr = getattr(o, k)
            for i, x in enumerate(v):
                arr[i] = x
        else:
            setattr(o, k, v)
    return o
