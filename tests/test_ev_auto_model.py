"""The auto-exposure model (tests/_ev_auto_model.py) and halo_host_ev_auto against what the reference's own header returned
(tests/golden/ev_auto_vectors.json, made by tests/golden/make_ev_auto_fixture.py).  No GPU.

Tolerances.  p99 and the per-pixel intensity are sums, a selection and one division in fp32: bit-exact.  The EV passes through powf and log2f of
whichever libm is present, each good to under one ulp; one float ulp at |ev| <= 6 is 4.8e-7, so the EV is held to 1e-6 absolute (two ulps)."""
import json
import os

import numpy as np
import pytest

from ice_halo_sim_amd import abi, backend
from tests import _ev_auto_model as M

HERE = os.path.dirname(os.path.abspath(__file__))
FX = json.load(open(os.path.join(HERE, "golden", "ev_auto_vectors.json")))
EV_TOL = 1e-6
F32 = np.float32


def f32_from_bits(b):
    return np.asarray([b], np.uint32).view(np.float32)[0]


def case_id(c):
    return "%dx%d-f%d-%s" % (c["w"], c["h"], c["f"], c["recipe"]["id"] + str(c["recipe"].get("seed", "")))


@pytest.mark.parametrize("case", FX["cases"], ids=case_id)
def test_model_reproduces_the_reference(case):
    y = M.case_image(case)
    p99, count, wc, hc = M.p99_y(y, case["f"])
    assert M.bits(p99) == case["p99_bits"], (float(p99), float(f32_from_bits(case["p99_bits"])))
    pp = M.per_pixel_intensity(case["total_intensity"], case["w"] * case["h"])
    want = float(f32_from_bits(case["ev_bits"]))
    assert abs(float(M.ev_auto(p99, pp, case["target_white"])) - want) <= EV_TOL
    assert abs(backend.host_ev_auto(p99, pp, case["target_white"]) - want) <= EV_TOL


def test_fixture_holds_the_reference_tests_literals():
    lits = [c for c in FX["cases"] if c["recipe"]["id"] == "literal"]
    got = {(c["w"], c["h"], c["f"]): float(f32_from_bits(c["p99_bits"])) for c in lits}
    assert got == {(4, 4, 2): 13.5, (8, 8, 8): 0.0, (1, 1, 8): 7.5}
    # every branch is in the fixture: both sides of the sRGB knee, an EV at each clamp and one inside, coarse / collapsed / fine grids
    evs = [float(f32_from_bits(c["ev_bits"])) for c in FX["cases"]]
    assert 6.0 in evs and -6.0 in evs and any(0.0 < abs(e) < 6.0 for e in evs)
    assert {10.0, 11.0} <= {c["target_white"] for c in FX["cases"]}


def test_box_sum_is_sequential_and_drops_the_trailing_strip():
    y = np.arange(1, 17, dtype=F32).reshape(4, 4)
    assert M.box_sum_y(y, 2).tolist() == [[14.0, 22.0], [46.0, 54.0]]
    assert M.box_sum_y(np.ones((13, 19), F32), 8).shape == (1, 2)
    assert M.box_sum_y(np.ones((1, 1), F32), 8) is None
    # 2^24 first, then 63 ones: added one after another every 1 is absorbed; a pairwise tree would keep them
    y = np.ones((8, 8), F32)
    y[0, 0] = F32(2.0 ** 24)
    assert float(M.box_sum_y(y, 8)[0, 0]) == 2.0 ** 24
    # positives only in the dropped strip: the coarse grid exists and is empty -> 0, no fine fallback
    y = np.zeros((13, 19), F32)
    y[:, 16:] = 1.0
    y[8:, :] = 1.0
    assert M.p99_y(y, 8) == (0.0, 0, 2, 1)
    assert M.p99_y(y, 1)[0] == 1.0


def test_index_rule_and_clamp():
    # 0.99f is 0.9900000095...: 100 of them round to 99.0 in fp32 (the exact product 99.00000095 lies within half an ulp of 99), so 100 values
    # take index 99, the largest — not the 98 that floor(100 * 0.99) suggests; the products below are exact in fp64 and rounded once
    for n, want in [(1, 0), (2, 1), (100, 99), (101, 99), (199, 197), (200, 198), (12345, 12221)]:
        idx = min(int(F32(n) * F32(0.99)), n - 1)
        assert idx == want == int(F32(float(n) * float(F32(0.99)))), (n, idx)
        v = np.arange(1, n + 1, dtype=F32)[::-1].copy()
        assert M.order_statistic(v) == (float(want + 1), n)


def test_host_ev_auto_guards_clamp_and_knee():
    ev = backend.host_ev_auto
    assert ev(0.0, 1.0) == 0.0 and ev(-1.0, 1.0) == 0.0 and ev(1.0, 0.0) == 0.0 and ev(1.0, -2.0) == 0.0
    assert ev(1e-9, 1.0) == 6.0 and ev(1e9, 1.0) == -6.0
    for tw in (10.0, 11.0, 135.0, 255.0):   # t <= 0.04045 for 10 (linear segment), above it for 11 (power segment)
        t = tw / 255.0
        lin = t / 12.92 if F32(t) <= F32(0.04045) else ((t + 0.055) / 1.055) ** 2.4
        for p99, pp in ((0.37, 1.9), (4.0, 0.5)):
            want = min(max(np.log2(lin / (p99 / pp)), -6.0), 6.0)
            assert abs(ev(p99, pp, tw) - want) <= 1e-5     # (the fp64 formula against an fp32 evaluation — a dozen roundings of 6e-8 — : a check of the branch, not the bar)
            assert abs(ev(p99, pp, tw) - float(M.ev_auto(p99, pp, tw))) <= EV_TOL
    assert (F32(10.0) / F32(255.0)) <= F32(0.04045) < (F32(11.0) / F32(255.0))


def test_abi_mirror():
    L = backend.load_library()
    import ctypes as C
    assert L.halo_abi_sizeof(12) == C.sizeof(abi.HaloAutoEv) == 28
