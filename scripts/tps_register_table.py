#!/usr/bin/env python3
"""GPU-box helper: the defaults of sift3d_amd_register_tps on the pair of tests/test_gpu_tps.py::test_regSift3D_tps_end_to_end
(synth.blobs(128, 112, 96, 5000, 21) against its copy deformed by a smooth field of 2.5 voxels amplitude).  regSift3D --tps over
lambda in {100, 1000, 10^4} at the default control-point threshold (4 x err_thresh = 20) and at sqrt(20) = 4.47: control
points, mean |warped - reference| over [6:-6]^3, and its ratio to the affine run's.

    python scripts/tps_register_table.py > profiles/tps_register.txt
"""
import os
import sys
import tempfile
import pathlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import tps_cases as tc                                        # noqa: E402

print("regSift3D --tps on blobs(128, 112, 96, 5000, 21) against its deformed copy (unit spacing)")
print(f"{'--tps_thresh':>12} {'--tps_lambda':>12} {'ctrl points':>12} {'affine err':>11} {'spline err':>11} {'ratio':>7}")
with tempfile.TemporaryDirectory() as d:
    for thresh in (None, 4.47):
        for lam in (100, 1000, 10000):
            extra = ("--tps_lambda", str(lam)) + (("--tps_thresh", str(thresh)) if thresh else ())
            e_aff, e_tps, csv = tc.e2e_run(pathlib.Path(d), extra=extra)
            print(f"{thresh or 'default (20)':>12} {lam:>12} {csv.shape[0] - 4:>12} {e_aff:>11.4f} {e_tps:>11.4f} {e_tps / e_aff:>7.3f}", flush=True)
