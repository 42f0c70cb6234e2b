"""A float64 model of the lens projection (world exit direction -> 0, 1 or 2 pixels) and a generator of directed probes for it.

The model is written from the lens definitions, with the reference's projection_shared.h read as the specification: which culls
exist, which constants are floats (pi, pi/2, the equal-area clamp -1 + 1e-6, the globe's camera distance 4), where the +0.5 and
the lens shift enter.  It takes the 19 four-byte fields of a ProjParams (halo_host_build_proj_params, pinned to the reference by
tests/test_host_tables.py and tests/test_ref_expectations.py) promoted to float64 and evaluates everything else in float64, so it
shares no rounding with the fp32 code it checks.  Besides the pixels it returns, per direction, how far the direction is from every
DECISION the projection makes (a pixel or frame edge, a cull, the overlap band, the seam, a pole branch): a direction closer than
the margin DELTA to one of them is *undecidable* — fp32 code may legitimately take the other side — and is left out of comparisons.

DELTA is measured, not chosen (tests/test_lens_model.py::test_margins_are_four_times_the_measured_disagreement): with the margin at
zero, the largest distance of each kind at which the fp32 oracle and this model disagree, over every probe and 200 k random
directions per render, times four (the device's FMA contraction and libm differ from the host's by a few ulp on top).
"""
import ctypes as C

import numpy as np

from ice_halo_sim_amd import abi, scenes

KINDS = ("px", "wz", "cz", "sz", "lon", "rho", "acos")
# kind: what the distance is                                                       unit
#   px   to the nearest pixel edge (a frame edge is one) of any hit in or next to the frame        pixels
#   wz   |wz|: the visible-range cull of the single-view lenses, the dual lenses' hemisphere        direction cosine
#   cz   |cz| (single-view rim), |cz + 1/4| (globe)                                                  direction cosine
#   sz   ||sz| - max_abs_dz|: the dual lenses' overlap band                                          direction cosine
#   lon  pi - |lon_rel|: the rectangular lens's wrap                                                 radians
#   rho  hypot of the two components across the lens axis: the `rho < 1e-10` branch of the equidistant and stereographic
#        forms, the rectangular lens's atan2 of two zeros                                            direction cosine
#   acos px / |d r / d cz|, single-view equidistant and stereographic lenses only: how far the ROTATED axis component cz is from
#        moving the hit over a pixel edge.  These two forms take theta = acos(cz), whose slope is 1 / sin(theta): half an ulp of
#        cz (3e-8 .. 6e-8 next to 1, plus the rounding of the three products) is 0.02 px half a pixel off the centre of a
#        1920 x 1080 image, against 1e-4 px anywhere else.  The six kinds above had no place for this; measured, it needed one.
#        (The dual lenses take acos of an INPUT, sz, and have no such term.)                         direction cosine

# Measured on the host (fp32 oracle and, where built, the reference's own code against this model; margin zero): the largest distance
# at which the two disagree.  wz and sz compare an INPUT with a constant — no arithmetic, no disagreement at any distance, exact
# zeros included.  lon: the wrap moves a hit by a whole turn, the pixel does not change.
# rho: no direction ever came within 1e-10 of a pole without being exactly on it, where both sides take the branch.
#                 measured   x 4 = DELTA
#   px            9.95e-5    3.98e-4 px     (worst: rectangular 1920 x 1080; 1e-5 .. 9e-5 elsewhere at that size, < 2e-5 at 512 x 256)
#   cz            1.72e-8    6.88e-8        (rim of the single-view lenses under a rotated view, the globe's -1/4)
#   acos          4.20e-8    1.68e-7        (equidistant / stereographic 1920 x 1080 under the rotated view; 0.04 px half a pixel off the centre)
#   wz sz lon rho 0          0
MEASURED = {"px": 9.95e-5, "wz": 0.0, "cz": 1.72e-8, "sz": 0.0, "lon": 0.0, "rho": 0.0, "acos": 4.20e-8}
FACTOR = 4.0
DELTA = {k: FACTOR * v for k, v in MEASURED.items()}

PI_F = float(np.float32(3.14159265358979323846))       # LM_PI_F / LM_PI_2F: float constants of the specification
PI_2F = float(np.float32(1.57079632679489661923))
EA_CLAMP = float(np.float32(-1.0) + np.float32(1e-6))  # -1.0f + 1e-6f
GLOBE_D = 4.0
SINGLE = (abi.LENS_LINEAR, abi.LENS_FISHEYE_EQUAL_AREA, abi.LENS_FISHEYE_EQUIDISTANT, abi.LENS_FISHEYE_STEREOGRAPHIC, abi.LENS_FISHEYE_ORTHOGRAPHIC)
DUAL = (abi.LENS_DUAL_FISHEYE_EQUAL_AREA, abi.LENS_DUAL_FISHEYE_EQUIDISTANT, abi.LENS_DUAL_FISHEYE_STEREOGRAPHIC, abi.LENS_DUAL_FISHEYE_ORTHOGRAPHIC)
FORM = {abi.LENS_FISHEYE_EQUAL_AREA: "ea", abi.LENS_FISHEYE_EQUIDISTANT: "ed", abi.LENS_FISHEYE_STEREOGRAPHIC: "st", abi.LENS_FISHEYE_ORTHOGRAPHIC: "or",
        abi.LENS_DUAL_FISHEYE_EQUAL_AREA: "ea", abi.LENS_DUAL_FISHEYE_EQUIDISTANT: "ed", abi.LENS_DUAL_FISHEYE_STEREOGRAPHIC: "st",
        abi.LENS_DUAL_FISHEYE_ORTHOGRAPHIC: "or"}
GUARD = 2   # pixels around the frame inside which a hit's pixel is compared; farther out only "not in frame" is


class Proj:
    """ProjParams, promoted."""

    def __init__(self, pp):
        self.pp = pp
        self.t, self.w, self.h, self.vr = int(pp.proj_type), int(pp.img_w), int(pp.img_h), int(pp.visible_range)
        self.shx, self.shy = float(pp.lens_shift_x), float(pp.lens_shift_y)
        self.scale, self.az0, self.rs, self.mad = float(pp.scale), float(pp.az0), float(pp.r_scale), float(pp.max_abs_dz)
        self.rot = np.array([float(v) for v in pp.rot], np.float64)


def proj_of(render):
    from ice_halo_sim_amd import backend
    pp = abi.ProjParams()
    assert backend.load_library().halo_host_build_proj_params(C.byref(render), C.byref(pp)) == 0
    return Proj(pp)


class Hits:
    """count[n]; f[n, hit, xy] continuous image coordinates (the argument of the floor); pix[n, hit, xy]; inframe[n, hit]; near[n, hit]: the
    hit exists and lies within GUARD pixels of the frame (its pixel is compared); dist[kind][n].  Hit 0 is the primary (the one landed
    weight counts), hit 1 the dual lenses' overlap write."""

    def decidable(self, delta=None):
        delta = DELTA if delta is None else delta
        ok = np.ones(len(self.count), bool)
        for k in KINDS:
            ok &= self.dist[k] >= delta[k]
        return ok

    def primary_pixel(self, w):
        """What an exit record's `pixel` holds: row-major index of the primary hit, -1 when it does not land."""
        return np.where(self.inframe[:, 0], self.pix[:, 0, 1] * w + self.pix[:, 0, 0], -1)


def _forward(form, dx, dy, dz, rs, cull=True):
    """The four fisheye forms: (x, y, rho or None).  rho is returned where the form has a pole branch."""
    if form == "ea":
        k = rs / np.sqrt(1.0 + np.clip(dz, EA_CLAMP, 1.0))
        return k * dx, k * dy, None
    if form == "or":
        ok = (dz >= 0.0) | (not cull)
        return np.where(ok, rs * dx, 0.0), np.where(ok, rs * dy, 0.0), None
    rho = np.hypot(dx, dy)
    pole = rho < 1e-10
    theta = np.arccos(np.clip(dz, -1.0, 1.0))
    with np.errstate(divide="ignore", invalid="ignore"):
        sc = rs * theta / (PI_2F * rho) if form == "ed" else rs * np.tan(theta / 2.0) / rho
    sc = np.where(pole, 0.0, sc)
    return sc * dx, sc * dy, rho


def project(P, d, cull=True):
    """cull=False: every cull passes and the overlap band is everywhere — where a hit WOULD land if fp32 code decided a cull the other way."""
    d = np.asarray(d, np.float64).reshape(-1, 3)
    n = len(d)
    wx, wy, wz = d[:, 0], d[:, 1], d[:, 2]
    H = Hits()
    H.count = np.zeros(n, np.int64)
    H.f = np.zeros((n, 2, 2))
    H.dist = {k: np.full(n, np.inf) for k in KINDS}
    t, w, h = P.t, P.w, P.h
    if t in SINGLE or t == abi.LENS_GLOBE:
        r = P.rot
        cx = r[0] * -wx + r[3] * -wy + r[6] * -wz
        cy = r[1] * -wx + r[4] * -wy + r[7] * -wz
        cz = r[2] * -wx + r[5] * -wy + r[8] * -wz
    if t in SINGLE:
        live = np.ones(n, bool)
        if P.vr in (abi.VISIBLE_UPPER, abi.VISIBLE_LOWER):
            H.dist["wz"] = np.abs(wz)
            live = ~(wz > 0.0) if P.vr == abi.VISIBLE_UPPER else ~(wz < 0.0)
        H.dist["cz"] = np.where(live, np.abs(cz), np.inf)
        live &= cz > 0.0
        if not cull:
            live[:] = True
        with np.errstate(divide="ignore", invalid="ignore"):
            if t == abi.LENS_LINEAR:
                x, y, rho = cx / cz, cy / cz, None
            else:
                x, y, rho = _forward(FORM[t], cx, cy, cz, 1.0, cull)
        amp = None
        if rho is not None:
            H.dist["rho"] = np.where(live, rho, np.inf)
            # |d r / d cz| in pixels: r = scale theta / (pi/2) or scale tan(theta / 2), d theta / d cz = -1 / sin(theta)
            with np.errstate(divide="ignore", invalid="ignore"):
                amp = P.scale / (PI_2F * rho) if FORM[t] == "ed" else P.scale / ((1.0 + cz) * rho)
        H.f[:, 0, 0] = np.where(live, -x * P.scale + w / 2.0 + 0.5 + P.shx, 0.0)
        H.f[:, 0, 1] = np.where(live, y * P.scale + h / 2.0 + 0.5 + P.shy, 0.0)
        H.count = live.astype(np.int64)
    elif t == abi.LENS_GLOBE:
        H.dist["cz"] = np.abs(cz + 1.0 / GLOBE_D)
        live = ~(cz >= -1.0 / GLOBE_D) | (not cull)
        den = GLOBE_D + cz
        H.f[:, 0, 0] = np.where(live, -cx / den * P.scale + w / 2.0 + 0.5 + P.shx, 0.0)
        H.f[:, 0, 1] = np.where(live, cy / den * P.scale + h / 2.0 + 0.5 + P.shy, 0.0)
        H.count = live.astype(np.int64)
    elif t == abi.LENS_RECTANGULAR:
        lon = np.arctan2(-wy, -wx) - P.az0
        lat = np.arcsin(np.clip(-wz, -1.0, 1.0))
        for _ in range(8):
            lon = np.where(lon < -PI_F, lon + 2.0 * PI_F, lon)
        for _ in range(8):
            lon = np.where(lon > PI_F, lon - 2.0 * PI_F, lon)
        H.dist["lon"] = PI_F - np.abs(lon)
        H.dist["rho"] = np.hypot(wx, wy)
        H.f[:, 0, 0] = lon * P.scale + w / 2.0 + 0.5
        H.f[:, 0, 1] = -lat * P.scale + h / 2.0 + 0.5
        H.count[:] = 1
    elif t in DUAL:
        sx, sy, sz = -wx, -wy, -wz
        upper = sz >= 0.0
        zh = np.where(upper, sz, -sz)
        H.dist["wz"] = np.abs(sz)
        half = min(w // 2, h) / 2.0

        def to_pixel(x, y, up):
            return np.where(up, -y, y) * half + np.where(up, w / 2.0 - half, w / 2.0 + half) + 0.5, x * half + h / 2.0 + 0.5
        x, y, rho = _forward(FORM[t], sx, sy, zh, P.rs)
        if rho is not None:
            H.dist["rho"] = rho
        H.f[:, 0, 0], H.f[:, 0, 1] = to_pixel(x, y, upper)
        H.count[:] = 1
        if P.mad > 0.0:
            H.dist["sz"] = np.abs(np.abs(sz) - P.mad)
            two = (np.abs(sz) < P.mad) | (not cull)
            x2, y2, _ = _forward(FORM[t], sx, sy, -zh, P.rs)
            fx2, fy2 = to_pixel(x2, y2, ~upper)
            H.f[:, 1, 0], H.f[:, 1, 1] = np.where(two, fx2, 0.0), np.where(two, fy2, 0.0)
            H.count = np.where(two, 2, 1)
    exists = np.arange(2)[None, :] < H.count[:, None]
    f = np.where(np.isfinite(H.f), H.f, 1e30)
    fl = np.floor(np.clip(f, -2.0 ** 40, 2.0 ** 40)).astype(np.int64)
    if t == abi.LENS_RECTANGULAR:
        fl[:, :, 0] = np.mod(fl[:, :, 0], w)
    H.pix = np.where(exists[:, :, None], fl, 0)
    H.inframe = exists & (fl[:, :, 0] >= 0) & (fl[:, :, 0] < w) & (fl[:, :, 1] >= 0) & (fl[:, :, 1] < h)
    H.near = exists & (fl[:, :, 0] >= -GUARD) & (fl[:, :, 0] < w + GUARD) & (fl[:, :, 1] >= -GUARD) & (fl[:, :, 1] < h + GUARD)
    edge = np.abs(f - np.round(f)).min(axis=2)
    H.dist["px"] = np.where(H.near, edge, np.inf).min(axis=1)
    H.amp = np.zeros(n)
    if t in SINGLE and amp is not None:
        H.amp = np.where(live, amp, 0.0)
        with np.errstate(divide="ignore", invalid="ignore"):
            H.dist["acos"] = np.where(H.near[:, 0] & (H.amp > 0.0), H.dist["px"] / H.amp, np.inf)
    return H


# ---------------------------------------------------------------------------------------------------------------------------------
# renders
# ---------------------------------------------------------------------------------------------------------------------------------
SPECIALISED = (abi.LENS_LINEAR, abi.LENS_FISHEYE_EQUAL_AREA, abi.LENS_DUAL_FISHEYE_EQUAL_AREA, abi.LENS_RECTANGULAR)   # lens as a template constant
ROTATED = dict(az=42.0, el=60.0, ro=15.0)   # the rotated view of tests/test_ref_expectations.py


def renders():
    """[(id, HaloRender)]: all eleven lenses x {512x256, 17x13 with a lens shift, 1920x1080} x {default view, the rotated view, straight up,
    straight down} where the lens has a view; the four specialised lenses appear under VISIBLE_UPPER and VISIBLE_FULL."""
    U, Lo, F = abi.VISIBLE_UPPER, abi.VISIBLE_LOWER, abi.VISIBLE_FULL
    out = []
    for lens in SINGLE:
        wide = 90.0 if lens == abi.LENS_LINEAR else 180.0
        out.append(("l%d-512-default-upper" % lens, scenes.render(lens, 512, 256, fov=wide, el=30.0, visible=U)))
        out.append(("l%d-17-up-shift-full" % lens, scenes.render(lens, 17, 13, fov=60.0, el=90.0, visible=F, lens_shift=(2, -1))))
        out.append(("l%d-1080-rotated-full" % lens, scenes.render(lens, 1920, 1080, fov=wide, visible=F, **ROTATED)))
        out.append(("l%d-512-down-lower" % lens, scenes.render(lens, 512, 256, fov=wide, el=-90.0, visible=Lo)))
    for lens in DUAL:
        out.append(("l%d-512-full" % lens, scenes.render(lens, 512, 256, el=0.0, visible=F)))     # no overlap, circles as high as the frame: a primary hit can leave it at the bottom
        out.append(("l%d-17-overlap-upper" % lens, scenes.render(lens, 17, 13, el=0.0, visible=U, overlap=0.0872)))
        out.append(("l%d-1080-overlap-upper" % lens, scenes.render(lens, 1920, 1080, el=0.0, visible=U, overlap=0.0872)))
    out.append(("l4-512-overlap1.5-full", scenes.render(abi.LENS_DUAL_FISHEYE_EQUAL_AREA, 512, 256, el=0.0, visible=F, overlap=1.5)))   # the antipode clamp is reachable
    lens = abi.LENS_RECTANGULAR
    out.append(("l7-512-az0-full", scenes.render(lens, 512, 256, fov=360.0, az=0.0, el=0.0, visible=F)))
    out.append(("l7-17-az170-upper", scenes.render(lens, 17, 13, fov=360.0, az=170.0, el=0.0, visible=U)))          # lon - az0 leaves [-pi, pi]: the wrap loops run
    out.append(("l7-1080-az-120-full", scenes.render(lens, 1920, 1080, fov=360.0, az=-120.0, el=0.0, visible=F)))
    lens = abi.LENS_GLOBE
    out.append(("l10-512-default", scenes.render(lens, 512, 256, fov=60.0, el=30.0, visible=F)))
    # (fov 20: the globe's disc, radius 0.258 scale, is wider than the frame: frame edges on all four sides of 17 x 13, top and bottom of 1920 x 1080)
    out.append(("l10-17-rotated-shift", scenes.render(lens, 17, 13, fov=20.0, visible=F, lens_shift=(2, -1), **ROTATED)))
    out.append(("l10-1080-up", scenes.render(lens, 1920, 1080, fov=20.0, el=90.0, visible=F)))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# probes
# ---------------------------------------------------------------------------------------------------------------------------------
CLASSES = ("pixel_edge", "frame_edge", "horizon", "rim", "pole", "seam", "band", "second_edge", "grid")
PROBE_DTYPE = np.dtype([("dir", np.float32, 3), ("cls", np.int8), ("must", bool), ("side", np.int8)])
# must: built k >= 1 margins from its boundary on every count — may not be undecidable.  side: -1 / +1 which side of its boundary, 0 n/a.


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _sphere(n):
    i = np.arange(n) + 0.5
    z = 1.0 - 2.0 * i / n
    ph = i * np.pi * (3.0 - np.sqrt(5.0))
    s = np.sqrt(1.0 - z * z)
    return np.stack([s * np.cos(ph), s * np.sin(ph), z], 1)


def _basis(u):
    a = np.where((np.abs(u[:, 2]) < 0.9)[:, None], np.array([0.0, 0.0, 1.0]), np.array([1.0, 0.0, 0.0]))
    e1 = _unit(np.cross(u, a))
    return e1, np.cross(u, e1)


def _invert(P, targets, hit, seeds, seed_f, seed_ok):
    """Directions whose hit `hit` has the continuous coordinates `targets`: Newton on the model from the nearest seed, in the tangent plane
    (the steps run along great circles).  Returns (directions, converged)."""
    T = np.asarray(targets, np.float64).reshape(-1, 2)
    if not seed_ok.any() or len(T) == 0:
        return np.zeros((len(T), 3)), np.zeros(len(T), bool)
    sf, sd = seed_f[seed_ok], seeds[seed_ok]
    start = np.empty(len(T), np.int64)
    for a in range(0, len(T), 256):
        start[a:a + 256] = ((T[a:a + 256, None, :] - sf[None, :, :]) ** 2).sum(2).argmin(1)
    u = sd[start].copy()
    step = 1e-6

    def f_of(v):
        Hv = project(P, v)
        return np.where((Hv.count > hit)[:, None], Hv.f[:, hit, :], np.nan)
    for _ in range(25):
        e1, e2 = _basis(u)
        f0 = f_of(u)
        j1 = (f_of(_unit(u + step * e1)) - f_of(_unit(u - step * e1))) / (2 * step)
        j2 = (f_of(_unit(u + step * e2)) - f_of(_unit(u - step * e2))) / (2 * step)
        r = T - f0
        det = j1[:, 0] * j2[:, 1] - j1[:, 1] * j2[:, 0]
        with np.errstate(all="ignore"):
            a = (r[:, 0] * j2[:, 1] - r[:, 1] * j2[:, 0]) / det
            b = (j1[:, 0] * r[:, 1] - j1[:, 1] * r[:, 0]) / det
        bad = ~np.isfinite(a) | ~np.isfinite(b)
        a, b = np.where(bad, 0.0, a), np.where(bad, 0.0, b)
        ln = np.hypot(a, b)
        k = np.minimum(1.0, 0.2 / np.maximum(ln, 1e-300))   # at most 0.2 rad per step
        u = _unit(u + (k * a)[:, None] * e1 + (k * b)[:, None] * e2)
    with np.errstate(all="ignore"):
        ok = np.abs(f_of(u) - T).max(axis=1) < 1e-7
    return u, ok


def _f32(v):
    return np.asarray(v, np.float64).astype(np.float32)


def probes(render, delta=None, seed=1, stats=None):
    """The directed probes of one render: a PROBE_DTYPE array of wanted exit directions (fp32).  stats (a dict) receives, per edge class, how many
    spots were asked for and how many the lens cannot reach (the Newton iteration found no direction that lands there: outside the image
    circle, behind the rim or the visible-range cull) — coverage that is absent is then visible, not silent."""
    delta = DELTA if delta is None else delta
    P = proj_of(render)
    w, h, t = P.w, P.h, P.t
    rng = np.random.default_rng(seed)
    seeds = _sphere(30000)
    Hs = project(P, seeds)
    out = []

    def add(dirs, cls, must=False, side=0):
        dirs = _f32(dirs).reshape(-1, 3)
        if len(dirs) == 0:
            return
        a = np.zeros(len(dirs), PROBE_DTYPE)
        a["dir"], a["cls"], a["must"] = dirs, CLASSES.index(cls), must
        a["side"] = side
        out.append(a)

    def settled(dirs, coord, want, margin):
        """Of the fp32 directions `dirs`: those the model calls decidable and whose signed coordinate `coord` lies on the wanted side,
        at least `margin` out."""
        d32 = _f32(dirs).astype(np.float64)
        Hd = project(P, d32)
        c = coord(Hd, d32)
        return Hd.decidable(delta) & (np.sign(want) * c >= margin)

    def edge_pairs(cls, spots, hit, seed_ok):
        """spots: (axis, edge value, centre of the pixel along the other axis).  Four probes per spot: the edge -/+ k margins, k in 1, 10."""
        u0, ok0 = _invert(P, np.array([(e, c) if ax == 0 else (c, e) for ax, e, c in spots], np.float64).reshape(-1, 2), hit, seeds, Hs.f[:, hit, :], seed_ok)
        amp0 = project(P, _f32(u0).astype(np.float64)).amp if hit == 0 else np.zeros(len(spots))
        if stats is not None:
            stats[cls] = dict(spots=len(spots), unreachable=int((~ok0).sum()), kept=0)
        spots = [s + (delta["px"] + delta["acos"] * a,) for s, a, o in zip(spots, amp0, ok0) if o]    # + the margin in pixels AT the spot
        for k in (1, 10):
            for sgn in (-1, 1):
                todo = np.ones(len(spots), bool)
                grow = 2.0      # (one margin to spare: a reflection off an inexact face moves the exit by ~1e-7, up to 1e-4 px)
                for _ in range(4):
                    if not todo.any():
                        break
                    S = [s for s, m in zip(spots, todo) if m]
                    T = np.array([(e + sgn * k * m * grow, c) if ax == 0 else (c, e + sgn * k * m * grow) for ax, e, c, m in S], np.float64).reshape(-1, 2)
                    u, ok = _invert(P, T, hit, seeds, Hs.f[:, hit, :], seed_ok)
                    ax = np.array([s[0] for s in S], np.int64)
                    ev = np.array([s[1] for s in S], np.float64)
                    mg = np.array([s[3] for s in S], np.float64)
                    good = ok & settled(u, lambda Hd, d: Hd.f[np.arange(len(d)), hit, ax] - ev, sgn, k * mg)
                    add(u[good], cls, must=True, side=sgn)
                    if stats is not None:
                        stats[cls]["kept"] += int(good.sum())
                    idx = np.flatnonzero(todo)
                    todo[idx[good]] = False
                    todo[idx[~ok]] = False      # not reachable under this lens (outside the image circle, behind the rim)
                    grow *= 1.5

    # --- pixel edges and frame edges of the primary hit
    cxp, cyp = w // 2, h // 2
    rows, cols = sorted({0, 1, h // 4, cyp, 3 * h // 4, h - 2, h - 1}), sorted({0, 1, w // 4, cxp, 3 * w // 4, w - 2, w - 1})   # (w/4, 3w/4: through the dual lenses' circles)
    spots = [(0, float(cxp), cyp + 0.5), (1, float(cyp), cxp + 0.5), (0, float(cxp + 2), cyp + 2.5), (1, float(cyp + 2), cxp + 2.5)]
    spots += [(0, float(e), r + 0.5) for e in (1, w - 1) for r in rows] + [(1, float(e), c + 0.5) for e in (1, h - 1) for c in cols]
    for _ in range(40):
        x, y = int(rng.integers(1, w)), int(rng.integers(1, h))
        spots += [(0, float(x), min(y, h - 1) + 0.5), (1, float(y), min(x, w - 1) + 0.5)]
    edge_pairs("pixel_edge", spots, 0, Hs.count >= 1)
    frame = [(0, float(e), r + 0.5) for e in (0, w) for r in rows] + [(1, float(e), c + 0.5) for e in (0, h) for c in cols]
    edge_pairs("frame_edge", frame, 0, Hs.count >= 1)

    # --- interior grid: pixel centres
    gx, gy = np.meshgrid(np.linspace(0, w - 1, min(w, 18)).round() + 0.5, np.linspace(0, h - 1, min(h, 12)).round() + 0.5)
    u, ok = _invert(P, np.stack([gx.ravel(), gy.ravel()], 1), 0, seeds, Hs.f[:, 0, :], Hs.count >= 1)
    add(u[ok], "grid")

    # --- horizon: wz = +-0 and a ladder of small values, round the compass
    az = np.deg2rad(np.arange(12) * 30.0 + 7.0)
    for wz in (0.0, -0.0, 1e-30, -1e-30, 1e-7, -1e-7, 1e-5, -1e-5, 1e-3, -1e-3):
        for j in range(4):
            a = az + 1e-3 * j
            d = np.stack([np.cos(a), np.sin(a), np.full(len(a), wz)], 1)
            good = settled(d, lambda Hd, dd: np.zeros(len(dd)), 1, 0.0)
            add(d[good], "horizon", must=True, side=int(np.sign(wz)) if wz != 0 else (-1 if np.signbit(wz) else 1))
            az = az[~good]
            if len(az) == 0:
                break
        az = np.deg2rad(np.arange(12) * 30.0 + 7.0)

    # --- rim: cz around 0 (single-view lenses), around -1/4 (globe)
    if t in SINGLE or t == abi.LENS_GLOBE:
        R = P.rot.reshape(3, 3)          # c = R^T (-w)  =>  w = -R c
        c0 = 0.0 if t in SINGLE else -1.0 / GLOBE_D
        dc = delta["cz"]
        phis = np.deg2rad(np.arange(12) * 30.0 + 11.0)

        def cz_of(Hd, dd):
            r = P.rot
            return (r[2] * -dd[:, 0] + r[5] * -dd[:, 1] + r[8] * -dd[:, 2]) - c0
        for k, sgn in ((0, 0), (1, -1), (1, 1), (10, -1), (10, 1), (1000, -1), (1000, 1)):
            ph = phis.copy()
            for j in range(6):
                czt = c0 + sgn * k * max(dc, 1e-7) * (3.0 + 0.5 * j)      # (two margins to spare: a reflection off an inexact face moves cz by ~6e-8)
                s = np.sqrt(1.0 - czt * czt)
                c = np.stack([s * np.cos(ph), s * np.sin(ph), np.full(len(ph), czt)], 1)
                d = -(c @ R.T)
                if k == 0:
                    add(d, "rim")
                    break
                good = settled(d, cz_of, sgn, k * dc)
                add(d[good], "rim", must=True, side=sgn)
                ph = ph[~good] + 1e-3
                if len(ph) == 0:
                    break

    # --- poles: along +- the view axis and +- z, and a ladder of small tilts off them
    axes = [np.array([0.0, 0.0, 1.0]), np.array([0.0, 0.0, -1.0])]
    if t in SINGLE or t == abi.LENS_GLOBE:
        ax = P.rot.reshape(3, 3) @ np.array([0.0, 0.0, 1.0])
        axes += [-ax, ax]
    for a in axes:
        add(a, "pole")
        e1, e2 = _basis(a[None, :])
        for tilt in (1e-7, 1e-6, 1e-5, 1e-4, 1e-3, 1e-2):
            for ph in np.deg2rad([13.0, 103.0, 193.0, 283.0]):
                add(_unit(a + tilt * (np.cos(ph) * e1[0] + np.sin(ph) * e2[0])), "pole")
    if t == abi.LENS_RECTANGULAR:
        for sx in (0.0, -0.0):
            for sy in (0.0, -0.0):
                for sz in (1.0, -1.0):
                    add(np.array([sx, sy, sz]), "pole")

    # --- seam of the rectangular lens: lon_rel = +-(pi - eps)
    if t == abi.LENS_RECTANGULAR:
        dl = delta["lon"]
        for eps in (0.0, 1e-7, 3e-7, 1e-6, 1e-5, 1e-4, 1e-3):
            for sgn in (-1, 1):
                for lat in np.deg2rad([-80.0, -33.0, -0.4, 12.0, 61.0, 88.0]):
                    for j in range(4):
                        lon = P.az0 + sgn * (np.pi - eps) + 0.0
                        la = lat + 1e-3 * j
                        d = -np.array([[np.cos(lon) * np.cos(la), np.sin(lon) * np.cos(la), np.sin(la)]])
                        must = eps >= max(dl, 1e-6)
                        if not must:
                            add(d, "seam", side=sgn)
                            break
                        if settled(d, lambda Hd, dd: Hd.dist["lon"], 1, dl)[0]:
                            add(d, "seam", must=True, side=sgn)
                            break

    # --- overlap band of the dual lenses: |sz| either side of max_abs_dz, second hits in and out of the frame, their pixel edges
    if t in DUAL and 0.0 < P.mad < 1.0:
        ds = delta["sz"]
        phis = np.deg2rad(np.arange(16) * 22.5 + 5.0)
        for k, sgn in ((1, -1), (1, 1), (10, -1), (10, 1)):
            for hemi in (-1.0, 1.0):
                ph = phis.copy()
                for j in range(6):
                    z = P.mad + sgn * k * max(ds, 1e-7) * (1.25 + 0.5 * j)
                    s = np.sqrt(1.0 - z * z)
                    d = np.stack([s * np.cos(ph), s * np.sin(ph), np.full(len(ph), hemi * z)], 1)
                    good = settled(d, lambda Hd, dd: np.abs(dd[:, 2]) - P.mad, sgn, k * ds)
                    add(d[good], "band", must=True, side=sgn)
                    ph = ph[~good] + 1e-3
                    if len(ph) == 0:
                        break
        for z in (0.5 * P.mad, -0.5 * P.mad, 0.9 * P.mad, -0.1 * P.mad):      # a ring of second hits: part of it leaves the frame
            ph = np.deg2rad(np.arange(48) * 7.5 + 1.0)
            s = np.sqrt(1.0 - z * z)
            add(np.stack([s * np.cos(ph), s * np.sin(ph), np.full(len(ph), z)], 1), "band")
        two = np.flatnonzero((Hs.count == 2) & Hs.inframe[:, 1])
        if len(two):
            pick = two[rng.permutation(len(two))[:24]]
            f1 = Hs.f[pick, 1, :]
            spots2 = [(0, float(np.round(x)), np.floor(y) + 0.5) for x, y in f1] + [(1, float(np.round(y)), np.floor(x) + 0.5) for x, y in f1]
            edge_pairs("second_edge", spots2, 1, Hs.count == 2)
    elif t in DUAL and P.mad >= 1.0:
        ph = np.deg2rad(np.arange(48) * 7.5 + 1.0)
        for z in (0.3, -0.3, 0.9, -0.9, 0.999, -0.999):
            s = np.sqrt(1.0 - z * z)
            add(np.stack([s * np.cos(ph), s * np.sin(ph), np.full(len(ph), z)], 1), "band")
    return np.concatenate(out)


def cone_directions(P, n, seed, half_angle=0.03):
    """n directions whose light arrives within `half_angle` of the view axis of a single-view lens: the neighbourhood of the image centre,
    where the acos forms are ill-conditioned (kind acos) and uniformly random directions almost never fall."""
    g = np.random.default_rng(seed)
    ax = -(P.rot.reshape(3, 3) @ np.array([0.0, 0.0, 1.0]))
    e1, e2 = _basis(ax[None, :])
    t, ph = half_angle * np.sqrt(g.uniform(0.0, 1.0, n)), g.uniform(0.0, 2.0 * np.pi, n)
    return _f32(_unit(ax + (t * np.cos(ph))[:, None] * e1 + (t * np.sin(ph))[:, None] * e2))


def random_directions(n, seed):
    g = np.random.default_rng(seed)
    d = g.normal(size=(n, 3))
    return _f32(_unit(d))


# ---------------------------------------------------------------------------------------------------------------------------------
# the rays that produce the probes: external reflections off the unit prism
# ---------------------------------------------------------------------------------------------------------------------------------
EXACT_FACES = (0, 1, 2, 5)    # +z, -z, +x, -x: normals of zeros and ones — the reflection d - 2 (d.n) n is exact there


def unit_prism_faces():
    """(normals[8, 3], points[8, 3]) of the regular unit prism from the product's host builder: face order = the entry-face index of a host ray."""
    from ice_halo_sim_amd import backend
    g = abi.HaloGeomTables()
    fd = (C.c_float * 6)(*[1.0] * 6)
    assert backend.load_library().halo_host_prism_geometry(1.0, fd, C.byref(g)) == 0 and g.face_cnt == 8
    nrm = np.array(g.face_n[:24], np.float32).reshape(8, 3)
    dist = np.array(g.face_d[:8], np.float32)
    return nrm, (-dist[:, None] * nrm).astype(np.float32)


def entry_rays(dirs):
    """Host rays (d, p, w, face) whose external reflection off the unit prism leaves along `dirs` (fp32).  The face is the one whose outward
    normal is closest to the wanted direction — incidence below 60 degrees — except that one of the four faces with exact normals is
    taken whenever it is within 60 degrees: the exit is then the wanted direction to the bit (returned as `exact`)."""
    nrm, pts = unit_prism_faces()
    e = np.asarray(dirs, np.float32).astype(np.float64)
    n64 = nrm.astype(np.float64)
    dots = e @ n64.T
    ex = np.array(EXACT_FACES)
    best_exact = ex[dots[:, ex].argmax(1)]
    use_exact = dots[np.arange(len(e)), best_exact] >= 0.5
    face = np.where(use_exact, best_exact, dots.argmax(1))
    nf = n64[face]
    dn = (e * nf).sum(1, keepdims=True)
    d_in = e - 2.0 * dn * nf
    return d_in.astype(np.float32), pts[face], np.ones(len(e), np.float32), face.astype(np.uint32), use_exact


# ---------------------------------------------------------------------------------------------------------------------------------
# comparison with fp32 code that returns {count, px0, py0, px1, py1} per direction (the oracle's and the reference's batch hooks)
# ---------------------------------------------------------------------------------------------------------------------------------
def disagreements(P, H, out5):
    """(count_bad[n], pixel_bad[n]): the hit count differs; a hit within GUARD pixels of the frame has another pixel, or a hit lands on one side
    and not on the other."""
    out5 = np.asarray(out5, np.int64).reshape(-1, 5)
    count_bad = out5[:, 0] != H.count
    code_pix = out5[:, 1:5].reshape(-1, 2, 2)
    code_in = (np.arange(2)[None, :] < out5[:, 0:1]) & (code_pix[:, :, 0] >= 0) & (code_pix[:, :, 0] < P.w) & (code_pix[:, :, 1] >= 0) & (code_pix[:, :, 1] < P.h)
    pix_bad = (H.near & (code_pix != H.pix).any(axis=2)).any(axis=1) | (code_in != H.inframe).any(axis=1)
    return count_bad, pix_bad & ~count_bad


def charge(P, H, count_bad, pix_bad, px_floor=np.inf):
    """{kind: largest distance of that kind among the disagreements charged to it} with the margin at zero.  A wrong count is charged to the
    nearest cull (wz, cz, sz); a wrong pixel to px — except that a single-view acos lens's wrong pixel farther than `px_floor` from its edge
    (what px explains everywhere else) is charged to acos."""
    worst = {k: 0.0 for k in KINDS}
    if count_bad.any():
        culls = np.stack([H.dist[k][count_bad] for k in ("wz", "cz", "sz")], 1)
        which = culls.argmin(1)
        for j, k in enumerate(("wz", "cz", "sz")):
            if (which == j).any():
                worst[k] = float(culls[which == j, j].max())
    if pix_bad.any():
        a = pix_bad & np.isfinite(H.dist["acos"]) & (H.dist["px"] > px_floor)
        if a.any():
            worst["acos"] = float(H.dist["acos"][a].max())
        if (pix_bad & ~a).any():
            worst["px"] = float(H.dist["px"][pix_bad & ~a].max())
    return worst
