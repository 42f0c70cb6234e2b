"""The fixed-point rule of option "deterministic" (include/halo_trace.h) in numpy: what a hit adds to a plane or to the landed integer.

    q(v, F) = floor(double(v) * 2^F + 0.5)   as an unsigned 64-bit integer; a NaN or a negative value adds nothing

`v` is the fp32 value the kernel holds (the weight on a scalar plane, the fp32 product cmf * weight on X, Y, Z).  double(v) * 2^F is exact (a
power-of-two scale of a 24-bit significand), the + 0.5 is one correctly rounded fp64 add — what the device's fma computes — so the model is
the device's rule bit for bit, not an approximation of it."""
import numpy as np


def q(v, frac_bits):
    """uint64 array of q(v, F) for an array (or scalar) of float32 values."""
    v = np.asarray(v, dtype=np.float32).astype(np.float64)
    v = np.where(np.isnan(v) | (v < 0.0), 0.0, v)
    return np.floor(v * np.float64(2.0) ** int(frac_bits) + 0.5).astype(np.uint64)


def frac_bits_bound_holds(max_w, hits, frac_bits):
    """The statement of halo_host_fixed_frac_bits: 4 * max(max_w, 1e-30) * max(hits, 1) * 2^F < 2^62, evaluated exactly (rationals)."""
    from fractions import Fraction
    bound = 4 * Fraction(max(float(max_w), 1e-30)) * max(int(hits), 1) * Fraction(2) ** int(frac_bits)
    return bound < Fraction(2) ** 62


def plane_sums(pixels, values, n_pix, frac_bits):
    """Per-pixel sum of q(values) over the records with that pixel (records with pixel < 0 land nowhere): uint64[n_pix]."""
    pixels = np.asarray(pixels, dtype=np.int64)
    keep = pixels >= 0
    out = np.zeros(int(n_pix), np.uint64)
    np.add.at(out, pixels[keep], q(np.asarray(values)[keep], frac_bits))
    return out
