"""A float64 model of the view stage's inverse half (pixel centre -> world exit direction) and the cases the view tests share.

The inverses are written from the lens definitions, against the forward model of tests/_lens_model.py (which is pinned to the oracle and to the
reference): same ProjParams fields promoted to float64 (_lens_model.Proj), same float constants of the specification (pi, pi/2, the globe's
camera distance 4), everything else evaluated in float64, so it shares no rounding with the fp32 code it checks (halo_view.h view_direction, on
the host through halo_host_view_direction and on the device as halo_consumer_view's dir_out).

Coordinates: pixel (px, py) here means the continuous coordinates project_exit computes BEFORE its floor(. + 0.5) — integer (px, py) is the centre
of that pixel, and the forward model's `f` (the argument of the floor) is (px + 0.5, py + 0.5) there.  inverse64 takes real-valued (px, py), so
the tests can also ask it where a forward hit came from.

Besides the direction and the validity flag it returns, per pixel, how far the centre is from every DOMAIN decision the inverse makes:
    rim   pixels: to the rim of a fisheye's image circle (cz = 0), of a dual lens's disc, to the globe's limb, to the rectangular lens's
          |lon| = pi and |lat| = pi/2 lines
    wz    direction cosine |wz|: the view's own visible-range cull (single-view lenses)
A centre closer than the margin DELTA to one of them is one where fp32 code may legitimately decide the other way; validity is compared only
outside the margins.  The margins and the pixel tolerance are measured, not chosen — see MEASURED below.
"""
import numpy as np

from ice_halo_sim_amd import abi, scenes

from tests import _lens_model as lm

KINDS = ("rim", "wz")

# Measured with the margins at zero (HALO_VIEW_MEASURE=1 makes tests/test_view_model.py::test_host_code_against_the_model, for the host function
# over every test view below, and tests/test_gpu_view.py, for the device's dir_out over every pair the GPU tests use, print the figures instead of
# asserting them): the largest deviation |project(P_view, dir).f - pixel centre| of a direction the fp32 code returned (less the forward model's
# own acos allowance, see acos_allowance), and the largest distance from a decision at which the fp32 code and this model disagree about
# validity.  DELTA = 4 x MEASURED, _lens_model.py's rule and reason (libm and contraction differ between host and device by a few ulp).
#            host       device (MI355X)   MEASURED (the larger)   x 4 = DELTA
#   px       1.12e-5    2.39e-4           2.39e-4                 9.56e-4 px   (device: the 1920 x 1080 linear view, 935 px per unit of tangent:
#                                                                               s = R c with an fp32 R that is orthonormal to 6e-8; the 96 x 54
#                                                                               and 37 x 23 views stay below 3e-5 on both sides)
#   rim      2.19e-7    2.19e-7           2.19e-7                 8.77e-7 px   (the rectangular lens's pole rows: pi/2 against the float LM_PI_2F)
#   wz       0          0                 0                       0            (no centre of these views came nearer the horizon than it could
#                                                                               be told; an exact zero is compared as undecided)
MEASURED = {"px": 2.39e-4, "rim": 2.1920e-7, "wz": 0.0}
FACTOR = 4.0
DELTA = {k: FACTOR * v for k, v in MEASURED.items()}
EPS = DELTA["px"]

SINGLE, DUAL, FORM = lm.SINGLE, lm.DUAL, lm.FORM


class Inv:
    """dir[n, 3] (zeros where invalid), valid[n], dist[kind][n]."""

    def decided(self, delta=None):
        delta = DELTA if delta is None else delta
        ok = np.ones(len(self.valid), bool)
        for k in KINDS:
            ok &= self.dist[k] > delta[k]
        return ok


def _form_inverse(form, x, y, rs):
    """Inverse of _lens_model._forward: (dx, dy, dz, defined) of the unit direction whose form is (x, y)."""
    xn, yn = x / rs, y / rs
    r2 = xn * xn + yn * yn
    r = np.sqrt(r2)
    ok = np.ones(len(r), bool)
    with np.errstate(invalid="ignore", divide="ignore"):
        if form == "ea":        # r^2 = 1 - dz
            dz = 1.0 - r2
            ok = dz >= -1.0
            k = np.sqrt(np.maximum(1.0 + dz, 0.0))
        elif form == "ed":      # r = theta / (pi/2)
            theta = r * lm.PI_2F
            ok = theta <= np.pi
            dz = np.cos(theta)
            k = np.where(r > 0.0, np.sin(theta) / np.where(r > 0.0, r, 1.0), 0.0)
        elif form == "st":      # r = tan(theta / 2)
            dz = (1.0 - r2) / (1.0 + r2)
            k = 2.0 / (1.0 + r2)
        else:                   # orthographic: r = rho
            ok = r2 <= 1.0
            dz = np.sqrt(np.maximum(1.0 - r2, 0.0))
            k = np.ones(len(r))
    return k * xn, k * yn, dz, ok


def inverse64(P, px, py):
    px, py = np.asarray(px, np.float64).ravel(), np.asarray(py, np.float64).ravel()
    n = len(px)
    I = Inv()
    I.dist = {k: np.full(n, np.inf) for k in KINDS}
    t, w, h = P.t, P.w, P.h
    if t in SINGLE or t == abi.LENS_GLOBE:
        u = -(px - w / 2.0 - P.shx) / P.scale
        v = (py - h / 2.0 - P.shy) / P.scale
        r = np.hypot(u, v)
        if t == abi.LENS_GLOBE:
            q = u * u + v * v
            disc = 1.0 - 15.0 * q
            valid = disc > 0.0
            cz = -(lm.GLOBE_D * q + np.sqrt(np.maximum(disc, 0.0))) / (q + 1.0)
            cx, cy = u * (lm.GLOBE_D + cz), v * (lm.GLOBE_D + cz)
            I.dist["rim"] = np.abs(r - 1.0 / np.sqrt(15.0)) * P.scale
        elif t == abi.LENS_LINEAR:
            nrm = 1.0 / np.sqrt(u * u + v * v + 1.0)
            cx, cy, cz = u * nrm, v * nrm, nrm
            valid = np.ones(n, bool)
        else:
            cx, cy, cz, ok = _form_inverse(FORM[t], u, v, 1.0)
            valid = ok & (cz > 0.0)
            r_rim = (np.pi / 2.0) / lm.PI_2F if FORM[t] == "ed" else 1.0
            I.dist["rim"] = np.abs(r - r_rim) * P.scale
        # c = R^T s  =>  s = R^-T c: the EXACT inverse of the fp32 matrix as it stands (orthonormal only to 6e-8; the fp32 code takes s = R c)
        s = np.linalg.solve(P.rot.reshape(3, 3).T, np.stack([cx, cy, cz], 0)).T
        if t in SINGLE and P.vr in (abi.VISIBLE_UPPER, abi.VISIBLE_LOWER):
            wz = -s[:, 2]
            I.dist["wz"] = np.where(valid, np.abs(wz), np.inf)
            valid = valid & ~((wz > 0.0) if P.vr == abi.VISIBLE_UPPER else (wz < 0.0))
        d = -s
    elif t == abi.LENS_RECTANGULAR:
        lon = (px - w / 2.0) / P.scale
        lat = -(py - h / 2.0) / P.scale
        # the forward's range: asin gives |lat| <= pi/2, the wrap loops leave |lon| <= PI_F (the float constant)
        valid = (np.abs(lon) <= lm.PI_F) & (np.abs(lat) <= np.pi / 2.0)
        I.dist["rim"] = np.minimum(np.abs(lm.PI_F - np.abs(lon)), np.abs(np.pi / 2.0 - np.abs(lat))) * P.scale
        a = lon + P.az0
        cl = np.maximum(np.cos(lat), 0.0)
        d = -np.stack([cl * np.cos(a), cl * np.sin(a), np.sin(lat)], 1)
    else:
        rad = min(w // 2, h) / 2.0
        with np.errstate(invalid="ignore", divide="ignore"):
            xn = (py - h / 2.0) / rad
            yl = -(px - (w / 2.0 - rad)) / rad
            yr = (px - (w / 2.0 + rad)) / rad
            rl, rr = np.hypot(xn, yl), np.hypot(xn, yr)
            left = rl <= 1.0
            valid = left | (rr <= 1.0)
            I.dist["rim"] = np.minimum(np.abs(rl - 1.0), np.abs(rr - 1.0)) * rad
            I.dist["rim"] = np.where(np.isfinite(I.dist["rim"]), I.dist["rim"], np.inf)
            dx, dy, dz, ok = _form_inverse(FORM[t], xn, np.where(left, yl, yr), P.rs)
        # ... and the forward lands there: the horizon itself is the left circle's (sz >= 0 is "upper"), the overlap write needs |sz| < max_abs_dz
        valid = valid & ok & ((dz > 0.0) | (np.abs(dz) < P.mad) | (left & (dz == 0.0)))
        d = np.stack([-dx, -dy, np.where(left, -dz, dz)], 1)
    I.valid = valid
    I.dir = np.where(valid[:, None], d, 0.0)
    return I


def pixel_grid(P):
    y, x = np.mgrid[0:P.h, 0:P.w]
    return x.ravel().astype(np.float64), y.ravel().astype(np.float64)


def wrap_slip(P):
    """Pixels by which the forward model itself moves a hit of the rectangular lens whose lon + az0 leaves (-pi, pi]: its atan2 comes back a TRUE
    turn away, its wrap loop adds a turn of 2 PI_F (the float constant) — 1.7e-7 rad more.  No inverse can undo a step in the forward."""
    return (2.0 * lm.PI_F - 2.0 * np.pi) * P.scale if P.t == abi.LENS_RECTANGULAR else 0.0


def acos_allowance(P, dirs):
    """Pixels by which the forward model's hit moves when the rotated axis component cz moves by _lens_model.DELTA["acos"]: the single-view
    equidistant and stereographic forms take theta = acos(cz), and next to cz = 1 (the image centre) that is not a matter of the inverse — an
    fp32 direction cannot hold the angle (see _lens_model.py, kind acos: measured there, committed there).  Zero for every other lens."""
    dirs = np.asarray(dirs, np.float64).reshape(-1, 3)
    if P.t not in (abi.LENS_FISHEYE_EQUIDISTANT, abi.LENS_FISHEYE_STEREOGRAPHIC):
        return np.zeros(len(dirs))
    cz = np.clip(-(dirs @ P.rot.reshape(3, 3)[:, 2]), -1.0, 1.0)

    def radius(c):
        th = np.arccos(np.clip(c, -1.0, 1.0))
        return P.scale * (th / lm.PI_2F if lm.FORM[P.t] == "ed" else np.tan(th / 2.0))
    return np.abs(radius(cz - lm.DELTA["acos"]) - radius(cz))


def landing_error(P, dirs, px, py):
    """Per direction: how far (pixels, the larger of |dx|, |dy|) the forward model lands it from the centre of pixel (px, py) — the nearer of
    its hits, so that a dual lens's overlap write counts; inf where it does not land at all."""
    H = lm.project(P, dirs)
    tgt = np.stack([np.asarray(px, np.float64) + 0.5, np.asarray(py, np.float64) + 0.5], 1)
    f = H.f
    if P.t == abi.LENS_RECTANGULAR:     # the forward wraps columns modulo the width
        f = f.copy()
        f[:, :, 0] = tgt[:, None, 0] + (np.mod(f[:, :, 0] - tgt[:, None, 0] + P.w / 2.0, P.w) - P.w / 2.0)
    err = np.abs(f - tgt[:, None, :]).max(axis=2)
    err = np.where(np.arange(2)[None, :] < H.count[:, None], err, np.inf)
    return err.min(axis=1)


def compare(P, I, x, y, has, dirs):
    """The figures of one view: the largest landing error (less the acos allowance) of a direction returned outside the margins, and per decision
    kind the largest distance at which the code's validity is not the model's (a disagreement is charged to the nearer decision, in margins)."""
    out = {"px": 0.0, "rim": 0.0, "wz": 0.0}
    dis = has != I.valid
    if dis.any():
        rim, wz = I.dist["rim"][dis], I.dist["wz"][dis]
        to_wz = np.isfinite(wz) & ((wz * 1e6 < rim) | ~np.isfinite(rim))    # (1 px of rim ~ 1e-6 of wz: neither kind hides the other)
        if to_wz.any():
            out["wz"] = float(wz[to_wz].max())
        if (~to_wz).any():
            out["rim"] = float(rim[~to_wz].max())
    m = has & I.valid & I.decided()
    if m.any():
        d64 = dirs[m].astype(np.float64)
        out["px"] = float((landing_error(P, d64, x[m], y[m]) - acos_allowance(P, d64)).max())
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------------------------------------
ROT = dict(az=40.0, el=25.0, ro=10.0)
FLAT = dict(az=0.0, el=0.0, ro=0.0)
U, LO, F = abi.VISIBLE_UPPER, abi.VISIBLE_LOWER, abi.VISIBLE_FULL
ALL_LENSES = tuple(range(11))


def _wide(lens):
    return {abi.LENS_LINEAR: 90.0, abi.LENS_GLOBE: 60.0, abi.LENS_RECTANGULAR: 360.0}.get(lens, 180.0)   # orthographic 180: the lens's limit


def small_views():
    """[(id, HaloRender)] at 37 x 23 (odd, no multiple of the 16-pixel tile), 1 x 1 and 5 x 300."""
    out = []
    for lens in SINGLE:
        fov = _wide(lens)
        out.append(("l%d-37-rot-shift-full" % lens, scenes.render(lens, 37, 23, fov=fov, visible=F, lens_shift=(3, -2), **ROT)))
        out.append(("l%d-37-flat-upper" % lens, scenes.render(lens, 37, 23, fov=fov, visible=U, **FLAT)))
        out.append(("l%d-37-up-upper" % lens, scenes.render(lens, 37, 23, fov=fov, visible=U, az=0.0, el=90.0)))
        out.append(("l%d-37-down-lower-shift" % lens, scenes.render(lens, 37, 23, fov=fov, visible=LO, az=0.0, el=-90.0, lens_shift=(3, -2))))
    for lens in DUAL:
        # (the dual equidistant lens at this size takes overlaps 0.1 and 0.15: at 0 and at 0.2 sixteen of its 512 centres fall 2e-5 px from a row
        #  edge of the dual equal-area sources — 3 % undecidable source lookups, a case that would test little; its overlap 0 is among mid_views)
        a, b = (0.1, 0.15) if lens == abi.LENS_DUAL_FISHEYE_EQUIDISTANT else (0.0, 0.2)
        out.append(("l%d-37-overlap%g" % (lens, a), scenes.render(lens, 37, 23, visible=F, overlap=a, **FLAT)))
        out.append(("l%d-37-overlap%g-rot" % (lens, b), scenes.render(lens, 37, 23, visible=U, overlap=b, **ROT)))
    out.append(("l7-37-flat", scenes.render(abi.LENS_RECTANGULAR, 37, 23, fov=360.0, visible=F, **FLAT)))
    out.append(("l7-37-rot", scenes.render(abi.LENS_RECTANGULAR, 37, 23, fov=360.0, visible=U, **ROT)))
    out.append(("l10-37-rot-shift", scenes.render(abi.LENS_GLOBE, 37, 23, fov=60.0, visible=F, lens_shift=(3, -2), **ROT)))
    out.append(("l10-37-flat-fov90", scenes.render(abi.LENS_GLOBE, 37, 23, fov=90.0, visible=LO, **FLAT)))   # the globe's widest field
    out.append(("l0-1x1", scenes.render(abi.LENS_LINEAR, 1, 1, fov=60.0, visible=F, **ROT)))
    out.append(("l4-1x1", scenes.render(abi.LENS_DUAL_FISHEYE_EQUAL_AREA, 1, 1, visible=F, **FLAT)))   # no circle fits: no pixel has a direction
    out.append(("l1-5x300", scenes.render(abi.LENS_FISHEYE_EQUAL_AREA, 5, 300, fov=180.0, visible=F, **ROT)))
    out.append(("l7-5x300", scenes.render(abi.LENS_RECTANGULAR, 5, 300, fov=360.0, visible=F, **FLAT)))
    return out


def mid_views():
    """[(id, HaloRender)] at 96 x 54."""
    out = []
    for lens in SINGLE:
        fov = _wide(lens)
        out.append(("l%d-96-rot-shift-lower" % lens, scenes.render(lens, 96, 54, fov=fov, visible=LO, lens_shift=(3, -2), **ROT)))
        # (el = 0 under VISIBLE_UPPER: the horizon runs through the centres of row 27 — the visible-range cull is decided on a wz of ~1e-8)
        out.append(("l%d-96-flat-upper" % lens, scenes.render(lens, 96, 54, fov=fov if lens != abi.LENS_LINEAR else 60.0, visible=U, **FLAT)))
    for lens in DUAL:
        out.append(("l%d-96-overlap0" % lens, scenes.render(lens, 96, 54, visible=U, **ROT)))
        out.append(("l%d-96-overlap0.1" % lens, scenes.render(lens, 96, 54, visible=F, overlap=0.1, **FLAT)))
    out.append(("l7-96-az-120", scenes.render(abi.LENS_RECTANGULAR, 96, 54, fov=360.0, visible=F, az=-120.0, el=0.0)))
    out.append(("l10-96-up", scenes.render(abi.LENS_GLOBE, 96, 54, fov=60.0, visible=F, az=0.0, el=90.0)))
    return out


def all_views():
    return small_views() + mid_views()


def sources():
    """[(id, HaloRender)]: the renders the GPU tests accumulate their image under."""
    return [
        ("dual-ea-128", scenes.render(abi.LENS_DUAL_FISHEYE_EQUAL_AREA, 128, 64, visible=F, **FLAT)),
        ("dual-ea-128-overlap0.1", scenes.render(abi.LENS_DUAL_FISHEYE_EQUAL_AREA, 128, 64, visible=F, overlap=0.1, **FLAT)),
        ("rect-128", scenes.render(abi.LENS_RECTANGULAR, 128, 64, fov=360.0, visible=F, **FLAT)),
        ("ea-96-upper-rot", scenes.render(abi.LENS_FISHEYE_EQUAL_AREA, 96, 96, fov=180.0, visible=U, az=42.0, el=60.0, ro=15.0)),   # covers part of the sky
        ("linear-96x54-fov60", scenes.render(abi.LENS_LINEAR, 96, 54, fov=60.0, visible=F, az=0.0, el=30.0)),
    ]


def pairs():
    """[(source id, source, view id, view)]: every source with every small view and with a third of the 96 x 54 views (a different third per source)."""
    out = []
    mids = mid_views()
    for k, (sid, src) in enumerate(sources()):
        for vid, view in small_views():
            out.append((sid, src, vid, view))
        for j, (vid, view) in enumerate(mids):
            if j % 3 == k % 3:
                out.append((sid, src, vid, view))
    return out


def identity_renders():
    """[(id, HaloRender)]: all eleven lenses as source AND view, at 37 x 23 and at 96 x 54.  No overlap: a band pixel of a dual view shows the other
    hemisphere, whose primary hit lies in the other circle.  The single-view equidistant and stereographic lenses take 95 x 53 for 96 x 54: at an
    even size one pixel's centre IS the view axis, where the lens model calls every lookup undecidable (kind acos)."""
    out = []
    for lens in ALL_LENSES:
        for w, h in ((37, 23), (95, 53) if lens in (abi.LENS_FISHEYE_EQUIDISTANT, abi.LENS_FISHEYE_STEREOGRAPHIC) else (96, 54)):
            kw = dict(ROT) if lens in SINGLE or lens == abi.LENS_GLOBE else dict(FLAT)
            shift = (3, -2) if (lens in SINGLE or lens == abi.LENS_GLOBE) and w == 37 else (0, 0)
            out.append(("l%d-%dx%d" % (lens, w, h), scenes.render(lens, w, h, fov=_wide(lens), visible=F, lens_shift=shift, **kw)))
    return out


BIG_PAIR = ("dual-ea-1080", scenes.render(abi.LENS_DUAL_FISHEYE_EQUAL_AREA, 1920, 1080, visible=F, **FLAT),
            "l0-1080-rot", scenes.render(abi.LENS_LINEAR, 1920, 1080, fov=60.0, visible=F, az=180.0, el=25.0, ro=0.0))


def undecidable_share(P_src, dirs, has_dir):
    """Of the pixels that have a direction: the share whose source lookup the lens model calls undecidable."""
    if not has_dir.any():
        return 0.0
    H = lm.project(P_src, dirs[has_dir])
    return float((~H.decidable()).mean())
