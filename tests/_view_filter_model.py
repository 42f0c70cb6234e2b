"""What the filtered view's tests share (halo_consumer_view_filtered, halo_host_view_source_pos): a float64 model of the bilinear sample and the
overlap-band blend, evaluated from a tap record {fx0, fy0, fx1, fy1, t} and the image the consumer holds, and the (source, view) pairs.

The model takes the tap record as given — where the taps lie is checked against the lens model (tests/_lens_model.py) and against project_exit's
map by the tests themselves — and evaluates in float64 what the kernel evaluates in fp32:
    x0 = floor(fx), ax = fx - x0 (exact in both), columns x0, x0 + 1 clamped to the frame (a rectangular source: modulo the width), rows clamped,
    top = v00 + ax (v10 - v00), bot = v01 + ax (v11 - v01), c = top + ay (bot - top);  blend: c = c1 + t (c2 - c1).
BAR is the fp32 code's distance from it, for images without negative values (M = the largest tap value of the pixel, u = 2^-24): a lerp is one
difference and one fma, two roundings of values no larger than M: 2 u M.  The second level inherits (1 - ay) e_top + ay e_bot <= 2 u M and adds
its own 2 u M; the blend inherits (1 - t) e_1 + t e_2 <= 4 u M and adds 2 u M: 6 u M, held to 8 u M."""
import ctypes as C

import numpy as np

from ice_halo_sim_amd import abi, scenes

from tests import _view_model as vm

BAR = 8.0 * 2.0 ** -24
T_BAR = 4.0 * 2.0 ** -24      # t: one difference, one product, one quotient of values <= 1
F, FLAT = vm.F, vm.FLAT


def sources():
    """[(id, HaloRender)]: _view_model's sources and, at 128 x 64 with an overlap band, the other three dual lenses."""
    return vm.sources() + [
        ("dual-ed-128-overlap0.1", scenes.render(abi.LENS_DUAL_FISHEYE_EQUIDISTANT, 128, 64, visible=F, overlap=0.1, **FLAT)),
        ("dual-st-128-overlap0.12", scenes.render(abi.LENS_DUAL_FISHEYE_STEREOGRAPHIC, 128, 64, visible=F, overlap=0.12, **FLAT)),
        ("dual-or-128-overlap0.15", scenes.render(abi.LENS_DUAL_FISHEYE_ORTHOGRAPHIC, 128, 64, visible=F, overlap=0.15, **FLAT)),
    ]


# The overlaps are the ones, of 0.10 .. 0.15 in steps of 0.01, at which the model alone calls at most 1 % of every view's source lookups
# undecidable (at the others one or more 37 x 23 views put 2 .. 20 % of their centres on source pixel edges).  (source id, view id) pairs left
# out: the orthographic source under the two 37 x 23 rectangular views, 4.9 % at every one of those overlaps.
# tests/test_view_filter_model.py::test_the_model_alone_keeps_every_pair_decidable holds the rest to the cap.
DROPPED = {("dual-or-128-overlap0.15", "l7-37-flat"), ("dual-or-128-overlap0.15", "l7-37-rot")}


def cpu_pairs():
    """[(source id, source, view id, view)]: every view of _view_model.all_views against every source."""
    return [(sid, src, vid, view) for sid, src in sources() for vid, view in vm.all_views() if (sid, vid) not in DROPPED]


def gpu_pairs():
    """Every source with every small view (37 x 23, 1 x 1, 5 x 300) and a third of the 96 x 54 ones (a different third per source)."""
    out = []
    mids = vm.mid_views()
    for k, (sid, src) in enumerate(sources()):
        for vid, view in vm.small_views():
            if (sid, vid) not in DROPPED:
                out.append((sid, src, vid, view))
        for j, (vid, view) in enumerate(mids):
            if j % 3 == k % 3 and (sid, vid) not in DROPPED:
                out.append((sid, src, vid, view))
    return out


def is_rect(render):
    return render.lens_type == abi.LENS_RECTANGULAR


def is_dual(render):
    return render.lens_type in vm.DUAL


def taps_of(fx, fy, w, h, wrap, bilinear=True):
    """(x0, x1, y0, y1, ax, ay) of the sample at (fx, fy): integer arrays inside the frame, float64 weights."""
    fx, fy = np.asarray(fx, np.float64), np.asarray(fy, np.float64)
    bx, by = (np.floor(fx), np.floor(fy)) if bilinear else (np.floor(fx.astype(np.float32) + np.float32(0.5)).astype(np.float64),
                                                           np.floor(fy.astype(np.float32) + np.float32(0.5)).astype(np.float64))
    ix, iy = bx.astype(np.int64), by.astype(np.int64)
    if wrap:
        x0, x1 = np.mod(ix, w), np.mod(ix + 1, w)
    else:
        x0, x1 = np.clip(ix, 0, w - 1), np.clip(ix + 1, 0, w - 1)
    y0, y1 = np.clip(iy, 0, h - 1), np.clip(iy + 1, 0, h - 1)
    return x0, x1, y0, y1, fx - bx, fy - by


def sample64(img, fx, fy, wrap, bilinear=True):
    """img float[h, w, 3] (the consumer's raw snapshot) -> (value[n, 3] float64, largest |tap|[n])."""
    h, w = img.shape[:2]
    img = img.astype(np.float64)
    x0, x1, y0, y1, ax, ay = taps_of(fx, fy, w, h, wrap, bilinear)
    v00 = img[y0, x0]
    if not bilinear:
        return v00, np.abs(v00).max(axis=1)
    v10, v01, v11 = img[y0, x1], img[y1, x0], img[y1, x1]
    top = v00 + ax[:, None] * (v10 - v00)
    bot = v01 + ax[:, None] * (v11 - v01)
    big = np.max(np.abs(np.stack([v00, v10, v01, v11], 0)), axis=(0, 2))
    return top + ay[:, None] * (bot - top), big


def view64(img, tap, source, bilinear=True, blend=False):
    """The filtered view's xyz from the tap record tap[n, 5] of pixels that have a source: (value[n, 3] float64, largest |tap value|[n])."""
    tap = np.asarray(tap, np.float64).reshape(-1, 5)
    c, big = sample64(img, tap[:, 0], tap[:, 1], is_rect(source), bilinear)
    if blend and is_dual(source):
        two = tap[:, 4] > 0.0      # (a second hit has |sz| < max_abs_dz: t > 0)
        if two.any():
            c2, big2 = sample64(img, tap[two, 2], tap[two, 3], False, bilinear)
            c[two] = c[two] + tap[two, 4][:, None] * (c2 - c[two])
            big[two] = np.maximum(big[two], big2)
    return c, big


def host_source_pos(source, dirs):
    """(count[n], pos[n, 5] float32) of halo_host_view_source_pos over dirs[n, 3] float32."""
    from ice_halo_sim_amd import backend
    fn = backend.load_library().halo_host_view_source_pos
    dirs = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
    n = len(dirs)
    cnt, pos = np.zeros(n, np.int64), np.zeros((n, 5), np.float32)
    f32p = C.POINTER(C.c_float)
    base_d, base_p = dirs.ctypes.data, pos.ctypes.data
    ref = C.byref(source)
    for i in range(n):
        cnt[i] = fn(ref, C.cast(base_d + 12 * i, f32p), C.cast(base_p + 20 * i, f32p))
    return cnt, pos
