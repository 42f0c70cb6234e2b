"""The fixed-point rule of option "deterministic" on the host: the numpy model of q() that the GPU tests sum captured rays with
(tests/_fixed_model.py), and halo_host_fixed_frac_bits against its own statement.  No GPU."""
import numpy as np
import pytest

from tests import _fixed_model as fm


def test_q_rounds_to_nearest_and_drops_what_is_not_a_weight():
    f32 = np.float32
    assert fm.q(0.0, 32) == 0
    assert fm.q(-0.0, 32) == 0
    # denormals and the smallest normal: far below half a unit at any F <= 32
    assert fm.q(np.array([1e-45, 1e-40, np.finfo(f32).tiny], f32), 32).tolist() == [0, 0, 0]
    # halves round up (floor(x + 0.5)), just below a half rounds down
    assert fm.q(f32(0.5), 0) == 1 and fm.q(f32(1.5), 0) == 2 and fm.q(f32(2.5), 0) == 3
    assert fm.q(np.nextafter(f32(0.5), f32(0.0)), 0) == 0
    assert fm.q(f32(2.0) ** -33, 32) == 1 and fm.q(np.nextafter(f32(2.0) ** -33, f32(0.0)), 32) == 0
    # a float32 is an integer multiple of 2^-F once it is >= 2^(24 - F): exact, nothing to round
    v = np.array([1.0, 0.75, 1.0 / 3.0, 31.5], f32)
    assert fm.q(v, 32).tolist() == [int(float(x) * 2 ** 32 + 0.5) for x in v]
    assert fm.q(f32(1.0), 29) == 1 << 29
    # NaN and negative values add nothing
    assert fm.q(np.array([np.nan, -1.0, -1e-30, -np.inf], f32), 32).tolist() == [0, 0, 0, 0]
    # the largest weight a session may declare (an illuminant's spd, tens) at the scale its 2^30-ray budget gives it
    from ice_halo_sim_amd.backend import host_fixed_frac_bits
    F = host_fixed_frac_bits(31.5, 1 << 30)
    assert fm.q(f32(31.5), F) == int(31.5 * 2 ** F) and int(fm.q(f32(31.5), F)) * (1 << 30) * 4 < 1 << 62
    assert fm.q(f32(1.0), 32).dtype == np.uint64


def test_plane_sums_groups_by_pixel():
    pix = np.array([0, 2, 2, -1, 0], np.int32)
    w = np.array([0.5, 0.25, 0.25, 9.0, 1.0], np.float32)
    assert fm.plane_sums(pix, w, 3, 2).tolist() == [6, 0, 2]


@pytest.mark.parametrize("max_w", [1e-30, 1e-3, 1.0, 31.5])
@pytest.mark.parametrize("hits", [1, 1 << 20, 1 << 28, 1 << 40])
def test_host_fixed_frac_bits_is_the_largest_scale_that_cannot_wrap(max_w, hits):
    from ice_halo_sim_amd.backend import host_fixed_frac_bits
    F = host_fixed_frac_bits(max_w, hits)
    assert 0 <= F <= 32
    assert fm.frac_bits_bound_holds(max_w, hits, F)
    assert F == 32 or not fm.frac_bits_bound_holds(max_w, hits, F + 1)
