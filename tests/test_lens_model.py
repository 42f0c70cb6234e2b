"""The float64 lens model (tests/_lens_model.py) against the fp32 code that is the truth: the oracle's ho_project_exit_to_pixel and, when
oracle/_ref is built, the reference's own lm_proj::ProjectExitToPixel — on every directed probe and 200 k uniformly random directions per
render (plus, for the single-view lenses, 50 k around the view axis).  No fraction anywhere: every direction the model calls decidable
must agree in hit count, every pixel next to or in the frame, and in-frame flag.  The margins the model commits are checked to be four
times what this very comparison measures, and the share of directions they leave out is capped here, on the host, where the reference
alone decides it (tests/test_gpu_lens_edges.py then holds the device to the same model)."""
import ctypes as C

import numpy as np
import pytest

from tests import _lens_model as M
from tests import _libs

RENDERS = M.renders()


def _code(which):
    if which == "oracle":
        return lambda P, d, out: _libs.oracle_project_batch(P.pp, d, out)
    if not _libs.have_ref():
        pytest.skip("oracle/_ref is not built here (the reference's sources are absent)")
    R = _libs.ref()
    assert R.ref_proj_params_size() == C.sizeof(M.abi.ProjParams)
    return lambda P, d, out: R.ref_project_exit_batch(C.addressof(P.pp), _libs.fptr(d), len(d), _libs.i32ptr(out))


_cache = {}


def _case(i):
    """(P, probes, directions, model hits) of render i — made once, shared by both arms and all tests."""
    if i not in _cache:
        P = M.proj_of(RENDERS[i][1])
        st = {}
        pr = M.probes(RENDERS[i][1], stats=st)
        print("%s: %s" % (RENDERS[i][0], st))
        parts = [pr["dir"], M.random_directions(200_000, 100 + i)]
        if P.t in M.SINGLE:
            parts.append(M.cone_directions(P, 50_000, 300 + i))
        d = np.ascontiguousarray(np.concatenate(parts), np.float32)
        _cache[i] = (P, pr, d, M.project(P, d.astype(np.float64)))
    return _cache[i]


@pytest.mark.parametrize("which", ["oracle", "ref"])
@pytest.mark.parametrize("i", range(len(RENDERS)), ids=[r[0] for r in RENDERS])
def test_model_equals_the_fp32_projection_on_every_decidable_direction(i, which):
    run = _code(which)
    P, pr, d, H = _case(i)
    out = np.zeros((len(d), 5), np.int32)
    run(P, d, out)
    count_bad, pix_bad = M.disagreements(P, H, out)
    ok = H.decidable()
    bad = np.flatnonzero(ok & (count_bad | pix_bad))
    assert len(bad) == 0, [(d[k].tolist(), out[k].tolist(), int(H.count[k]), H.pix[k].tolist(), {q: float(H.dist[q][k]) for q in M.KINDS}) for k in bad[:5]]
    # the margins are what was measured: every disagreement lies within MEASURED (a quarter of DELTA) of a decision of its kind
    worst = M.charge(P, H, count_bad, pix_bad, px_floor=M.MEASURED["px"])
    for k in M.KINDS:
        assert worst[k] <= M.MEASURED[k], (k, worst[k], M.MEASURED[k])
    # what may be left out: no probe built k >= 1 margins from its boundary, at most 1 % of the random directions
    n = len(pr)
    assert ok[:n][pr["must"]].all(), int((~ok[:n][pr["must"]]).sum())
    assert (~ok[n:n + 200_000]).mean() <= 0.01, (~ok[n:n + 200_000]).mean()


def test_margins_are_four_times_the_measured_disagreement():
    assert M.FACTOR == 4.0 and set(M.DELTA) == set(M.KINDS) == set(M.MEASURED)
    for k in M.KINDS:
        assert M.DELTA[k] == 4.0 * M.MEASURED[k]
    # an input compared with a constant involves no arithmetic: exact zeros are decidable
    assert M.DELTA["wz"] == 0.0 and M.DELTA["sz"] == 0.0


def test_probe_sets_cover_their_classes():
    """Every probe class is present where the lens has it, with both sides of its boundary, and each probe has a well-conditioned
    reflection to produce it (incidence below 60 degrees)."""
    seen = set()
    for i, (name, rd) in enumerate(RENDERS):
        P, pr, d, H = _case(i)
        cls = {M.CLASSES[c] for c in np.unique(pr["cls"])}
        seen |= {(P.t, c) for c in cls}
        assert {"horizon", "pole"} <= cls, (name, cls)
        assert 300 <= len(pr) <= 5000, (name, len(pr))
        for c in ("pixel_edge", "frame_edge", "rim", "band", "second_edge", "seam"):
            sel = (pr["cls"] == M.CLASSES.index(c)) & pr["must"]
            if sel.any() and c != "frame_edge":      # (a frame edge may be reachable from the inside only)
                assert {-1, 1} <= set(pr["side"][sel].tolist()), (name, c)
        d_in, p, w, face, exact = M.entry_rays(pr["dir"])
        nrm, _ = M.unit_prism_faces()
        cos_i = -(d_in.astype(np.float64) * nrm[face].astype(np.float64)).sum(1) / np.linalg.norm(d_in.astype(np.float64), axis=1)
        assert (cos_i > 0.5 - 1e-6).all(), (name, float(cos_i.min()))
        assert exact.mean() > 0.5, (name, exact.mean())
    for t in range(11):
        assert (t, "pixel_edge") in seen and (t, "grid") in seen, t
    for t in M.SINGLE + (M.abi.LENS_GLOBE,):
        assert (t, "rim") in seen and (t, "frame_edge") in seen, t
    for t in M.DUAL:
        assert (t, "frame_edge") in seen, t
    # (the dual orthographic lens has no overlap band: the parameter builder, like the reference's, leaves its max_abs_dz at 0 whatever the overlap)
    for t in (M.abi.LENS_DUAL_FISHEYE_EQUAL_AREA, M.abi.LENS_DUAL_FISHEYE_EQUIDISTANT, M.abi.LENS_DUAL_FISHEYE_STEREOGRAPHIC):
        assert (t, "band") in seen and (t, "second_edge") in seen, t
    assert (M.abi.LENS_RECTANGULAR, "seam") in seen and (M.abi.LENS_RECTANGULAR, "frame_edge") in seen

