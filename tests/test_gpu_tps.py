"""Thin-plate-spline registration on the device: s3d_k_inv_tps and im_inv_transform against the reference's warp
(tests/tps_cases.py; the CPU counterpart is tests/test_tps.py), and regSift3D --tps end to end on a deformed pair."""
import os

import numpy as np
import pytest

import sift3d_amd
from tests import tps_cases as tc
from tests.test_cli import BIN, run

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def host():
    return tc.bind(sift3d_amd.load())


@pytest.fixture(scope="module")
def dev():
    return sift3d_amd.load_device()


@pytest.mark.parametrize("interp,nc", [(0, 1), (0, 3), (1, 1)])
@pytest.mark.parametrize("n", tc.N_CTRL)
def test_warp_kernel_vs_reference(dev, reference, n, interp, nc):
    src, ctrl, params = tc.warp_inputs(n, nc)
    want = tc.reference_warp(reference, n, nc, interp)
    got = tc.warp_through_kernel(dev, src, ctrl, params, interp)
    tc.check_warp(got, want, src, ctrl, params, interp)


def test_warp_kernel_partial_workgroup_and_three_tiles(dev, reference):
    """70 x 9 x 5 destination (a row is no multiple of the workgroup), 300 control points (two full tiles and a part)"""
    dd = (70, 9, 5)
    assert 2 * tc.TILE < 300 < 3 * tc.TILE
    src, ctrl, params = tc.warp_inputs(300, 1, dd)
    want = tc.reference_warp(reference, 300, 1, 0, dd)
    got = tc.warp_through_kernel(dev, src, ctrl, params, 0, dd)
    tc.check_warp(got, want, src, ctrl, params, 0, dd)


@pytest.mark.parametrize("n", [0, 197])
def test_im_inv_transform_vs_reference(host, reference, n):
    src, ctrl, params = tc.warp_inputs(n, 1)
    got = tc.warp_through_api(host, src, ctrl, params, 0)
    tc.check_warp(got, tc.reference_warp(reference, n, 1, 0), src, ctrl, params, 0)


def test_warp_entry_point_failures(dev):
    src, ctrl, params = tc.warp_inputs(7, 1)
    bufs = [dev.upload(a) for a in (src, np.zeros(tc.DST_DIMS[::-1], np.float32), params, ctrl)]
    (sx, sy, sz), (dx, dy, dz) = tc.SRC_DIMS, tc.DST_DIMS
    for sd, nc, dd, interp in (((0, sy, sz), 1, (dx, dy, dz), 0), ((sx, sy, sz), 1, (dx, 0, dz), 0), ((sx, sy, sz), 0, (dx, dy, dz), 0),
                               ((sx, sy, sz), 1, (dx, 65536, dz), 0), ((sx, sy, sz), 1, (dx, dy, dz), 2)):
        assert dev.L.s3d_k_inv_tps(bufs[0], *sd, nc, bufs[1], *dd, bufs[3], bufs[2], 7, interp, None) != 0 and dev.err()
    assert not dev.download(bufs[1], tc.DST_DIMS[::-1]).any()            # nothing was launched
    for b in bufs:
        dev.free(b)


def test_regSift3D_tps_end_to_end(tmp_path):
    e_aff, e_tps, csv = tc.e2e_run(tmp_path)
    n = csv.shape[0] - 4
    print(f"regSift3D --tps: {n} control points, mean |warped - ref| affine {e_aff:.4f}, spline {e_tps:.4f}, ratio {e_tps / e_aff:.3f}")
    assert csv.shape[1] == 6 and n >= 150 and not csv[n:, :3].any()
    assert e_tps <= 0.6 * e_aff
    exe = os.path.join(BIN, "regSift3D")
    ref_exe = os.path.join(tc.ROOT, "oracle", "_ref", "bin", "regSift3D")
    mine = run(exe, "--help")
    assert mine.returncode == 0 and "--tps_lambda" in mine.stdout.split("Other options:")[0]
    if os.path.exists(ref_exe):                                           # the reference's program text, linked against this library
        assert mine.stdout.split("Other options:")[1] == run(ref_exe, "--help").stdout.split("Other options:")[1]
    r = run(exe, "--type", "tps", "--matches", "m.csv", "a", "b")
    assert r.returncode == 1 and "Unrecognized transformation type: tps" in r.stderr
