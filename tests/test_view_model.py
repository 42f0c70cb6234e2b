"""The float64 model of the view stage's inverse half (tests/_view_model.py) against the forward lens model it inverts (tests/_lens_model.py, pinned
to the oracle and the reference), and the product's fp32 inverse on the host (halo_host_view_direction: halo_view.h, the code halo_view_kernel
runs) against the model — on every pixel of every test view.  No GPU.

What is compared where:
  * Outside the domain margins (_view_model.DELTA, kinds rim and wz) the fp32 code's validity is the model's.  A centre inside a margin lies on
    a decision (a disc's rim, the limb, the rectangular lens's pole rows and seam, the view's horizon): fp32 code may decide either way there, and
    where it gives no direction there is nothing to land — so the landing check, too, is made outside the margins.
  * A direction the fp32 code returns lands, under the forward MODEL, within EPS = DELTA["px"] of the pixel's centre — plus, for the single-view
    equidistant and stereographic lenses only, what the forward model's own theta = acos(cz) moves the hit when cz moves by
    _lens_model.DELTA["acos"] (the margin that model already commits for exactly this: next to the image centre an fp32 direction cannot hold the
    angle, whatever inverse produced it; half a pixel off the centre of these views it is 1e-5 px, ON the centre pixel of an even-sized view 6e-3 px).
  * The float64 round trip holds to 1e-9 px farther than 1e-3 px from a rim; closer, the forward model's own asin / acos at 1 - 1e-15 keeps only
    1e-5 px (the rectangular lens's pole rows: their centres are the pole itself).  The rectangular lens gets its forward's own step on top:
    _view_model.wrap_slip.
HALO_VIEW_MEASURE=1 prints the figures MEASURED is made of instead of asserting them."""
import ctypes as C
import os

import numpy as np
import pytest

from ice_halo_sim_amd import backend
from tests import _lens_model as lm
from tests import _view_model as vm

VIEWS = vm.all_views() + [("identity-" + k, r) for k, r in vm.identity_renders()]
MEASURE = bool(os.environ.get("HALO_VIEW_MEASURE"))
RIM_NEAR = 1e-3     # pixels
_cache = {}


def _case(i):
    if i not in _cache:
        P = lm.proj_of(VIEWS[i][1])
        x, y = vm.pixel_grid(P)
        _cache[i] = (P, x, y, vm.inverse64(P, x, y))
    return _cache[i]


def host_directions(render):
    """(has[n], dir[n, 3] float32) of every pixel, row-major, from halo_host_view_direction."""
    fn = backend.load_library().halo_host_view_direction
    n = render.width * render.height
    has, d = np.zeros(n, bool), np.zeros((n, 3), np.float32)
    buf = (C.c_float * 3)()
    for p in range(n):
        has[p] = fn(C.byref(render), p % render.width, p // render.width, buf) == 1
        d[p] = buf[:]
    return has, d


@pytest.mark.parametrize("i", range(len(VIEWS)), ids=[v[0] for v in VIEWS])
def test_round_trip_in_float64(i):
    P, x, y, I = _case(i)
    if I.valid.any():
        err = vm.landing_error(P, I.dir[I.valid], x[I.valid], y[I.valid])
        near = I.dist["rim"][I.valid] <= RIM_NEAR
        assert (err[~near] <= 1e-9 + vm.wrap_slip(P)).all(), float(err[~near].max())
        assert (err[near] <= 1e-5 + vm.wrap_slip(P)).all(), float(err[near].max())
    # ... and the other way round: whatever the forward model lands in the frame comes from the direction the inverse gives for that spot
    d = lm.random_directions(20_000, 7 + i).astype(np.float64)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    H = lm.project(P, d)
    for hit in range(2):
        sel = H.inframe[:, hit]
        if not sel.any():
            continue
        fx, fy = H.f[sel, hit, 0] - 0.5, H.f[sel, hit, 1] - 0.5
        J = vm.inverse64(P, fx, fy)
        far = J.dist["rim"] > RIM_NEAR
        assert J.valid[far].all(), (hit, int((~J.valid[far]).sum()))
        # (a coarse bar, 1e-4: this direction is about the right spot of the sky — mirror images, swapped circles and wrong hemispheres are what
        #  it catches.  The fp32 rotation matrix is orthonormal to 6e-8 only, so "d is a unit vector" and "R^T d is a unit vector", what the forward
        #  and the inverse each take for granted, cannot both hold, and the forward's acos next to the axis turns 6e-8 of cz into 1e-5 of angle.)
        dev = np.abs(J.dir - d[sel]).max(axis=1)[far & J.valid]
        assert (dev <= 1e-4).all(), (hit, float(dev.max()))


def test_host_code_against_the_model():
    worst = {"px": 0.0, "rim": 0.0, "wz": 0.0}
    for i, (name, render) in enumerate(VIEWS):
        P, x, y, I = _case(i)
        has, dirs = host_directions(render)
        assert (dirs[~has] == 0.0).all(), name
        if MEASURE:
            I2 = vm.inverse64(P, x, y)
            I2.decided = lambda delta=None: np.ones(len(x), bool)   # margins at zero
            fig = vm.compare(P, I2, x, y, has, dirs)
            print("%-34s px %.3e  rim %.3e  wz %.3e" % (name, fig["px"], fig["rim"], fig["wz"]))
        else:
            fig = vm.compare(P, I, x, y, has, dirs)
            ok = I.decided()
            assert (has[ok] == I.valid[ok]).all(), (name, int((has[ok] != I.valid[ok]).sum()))
            assert fig["px"] <= vm.EPS, (name, fig["px"])
        for k in worst:
            worst[k] = max(worst[k], fig[k])
    print("host, worst over all views:", worst)
    for k in worst:   # what is committed as measured is no less than what the host shows
        assert MEASURE or worst[k] <= vm.MEASURED[k], (k, worst[k])


def test_margins_are_four_times_the_measured_disagreement():
    assert vm.FACTOR == 4.0 and set(vm.DELTA) == set(vm.MEASURED) == {"px"} | set(vm.KINDS)
    for k in vm.DELTA:
        assert vm.DELTA[k] == 4.0 * vm.MEASURED[k]
    assert vm.EPS == vm.DELTA["px"] <= 0.01     # a lens that needed more would have an ill-conditioned inverse


def test_view_spec_layout():
    L = backend.load_library()
    assert L.halo_abi_sizeof(15) == C.sizeof(vm.abi.HaloViewSpec) == 120
    assert vm.abi.HaloViewSpec.has_source.offset == 44 and vm.abi.HaloViewSpec.source.offset == 48 and vm.abi.HaloViewSpec.display.offset == 92
    assert L.halo_abi_version() == 6
    d = (C.c_float * 3)(1.0, 1.0, 1.0)
    assert L.halo_host_view_direction(None, 0, 0, d) == 0 and L.halo_host_view_direction(C.byref(VIEWS[0][1]), 0, 0, None) == 0
    has, w = backend.host_view_direction(VIEWS[0][1], 5, 5)
    assert has and abs(float(np.linalg.norm(w.astype(np.float64))) - 1.0) < 1e-6
    has, w = backend.host_view_direction(VIEWS[0][1], -1, 5)     # outside the frame
    assert not has and (w == 0.0).all()


def _share(src, view):
    P_src, P = lm.proj_of(src), lm.proj_of(view)
    x, y = vm.pixel_grid(P)
    I = vm.inverse64(P, x, y)
    return vm.undecidable_share(P_src, I.dir, I.valid)


def test_source_lookups_are_decidable_for_the_cases_the_gpu_tests_use():
    """From the MODEL's directions: the share of view pixels whose source lookup the lens model calls undecidable.  With DELTA["px"] = 3.98e-4 px
    of the lens model about 4 x 3.98e-4 = 0.16 % are expected; a case with more than 1 % would test little.  The identity pairs must show none."""
    worst = 0.0
    for sid, src, vid, view in vm.pairs():
        s = _share(src, view)
        worst = max(worst, s)
        assert s <= 0.01, (sid, vid, s)
    for name, r in vm.identity_renders():
        assert _share(r, r) == 0.0, name
    sid, src, vid, view = vm.BIG_PAIR
    s = _share(src, view)
    print("undecidable share: worst pair %.4f %%, %s -> %s %.4f %%" % (100 * worst, sid, vid, 100 * s))
    assert s <= 0.01
