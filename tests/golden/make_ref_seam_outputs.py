#!/usr/bin/env python3
"""Outputs of the reference's own pieces (oracle/_ref/libref_shared.so) on the fixed inputs of two vector groups of
tests/golden/ref_test_vectors.json, so that tests/test_ref_seam_vectors.py checks them wherever it runs:

  scatter_*        the image + landed weight ScatterOutgoingToXyz makes of the twelve `scatter_outgoing` rays (ProjectExitToPixel + SpectrumToXyz)
  post_snapshot_*  the image of the four `post_snapshot_fusion` rays, and per case the sRGB bytes of the chain rebuilt from GamutClipXyz /
                   XyzToLinearRgb / LinearToSrgb (real colour: also how many channels were clamped)

Needs the reference build (oracle/_ref, made by build() where the reference checkout lies); where it exists the tests also recompute
every array live and require it to equal the stored one.  `python tests/golden/make_ref_seam_outputs.py` writes ref_seam_outputs.npz."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import _libs  # noqa: E402
from tests import test_ref_seam_vectors as T  # noqa: E402


def main():
    assert _libs.have_ref(), "oracle/_ref/libref_shared.so is missing: run build() where the reference checkout lies"
    out = {}
    for key, fn in T.LIVE_REF_OUTPUTS.items():
        for name, arr in fn().items():
            out[key + "_" + name] = arr
    path = os.path.join(ROOT, "tests", "golden", "ref_seam_outputs.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, sorted(out))


if __name__ == "__main__":
    main()
