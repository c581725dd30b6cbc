"""RANSAC hypotheses scored on the device, on the device: s3d_k_ransac_count against the numpy restatement, and
find_tform_ransac DEVICE against HOST bit for bit (tests/ransac_cases.py; the CPU counterpart is tests/test_ransac_device.py).
regSift3D end to end is tests/test_reg.py::test_regSift3D_end_to_end."""
import numpy as np
import pytest

import sift3d_amd
from tests import ransac_cases as rc
from tests.ransac_cases import AUTO, DEVICE
from tests.test_reg import A_TRUE, _points

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def host():
    return rc.bind_ransac(sift3d_amd.load())


@pytest.fixture(scope="module")
def dev():
    return sift3d_amd.load_device()


@pytest.fixture(scope="module")
def pair_17874():
    """the match count of tests/golden/pair512.npz, half of them outliers, coordinates of a 512^3 volume"""
    src, ref = _points(17874, 8937, 11, A_TRUE)
    return src * 5, ref * 5


@pytest.mark.parametrize("npts", rc.NPTS)
def test_kernel_counts_equal_numpy(dev, npts):
    rc.check_kernel_grid(dev, npts)


def test_kernel_counts_equal_numpy_35000_by_1000(dev):
    src, ref = _points(35000, 17500, 13, A_TRUE)
    rng = np.random.default_rng(13)
    models = (A_TRUE[None] + rng.standard_normal((1000, 3, 4)) * np.array([0.01, 0.01, 0.01, 3.0])).reshape(1000, 12)
    want = rc.np_counts(src, ref, models, 25.0)
    assert 0 < want.min() < want.max() < 35000
    assert np.array_equal(rc.device_counts(dev, src, ref, models, 25.0), want)


def test_kernel_does_not_contract(dev):
    """matches whose residual falls on the other side of thr2 when a multiply-add is fused"""
    rc.check_no_contraction(dev)


def test_kernel_refuses_empty_sizes(dev):
    src, ref, models = rc.kernel_inputs(8, 3, 25.0)
    bufs = [dev.upload(a) for a in (src, ref, models, np.zeros(3, np.int32))]
    for npts, nm in ((0, 3), (8, 0), (8, 65535 * rc.TILE + 1)):
        assert dev.L.s3d_k_ransac_count(bufs[0], bufs[1], npts, bufs[2], nm, 25.0, bufs[3], None) != 0
    for b in bufs:
        dev.free(b)


@pytest.mark.parametrize("case", ["200", "duplicate-rows"])
def test_device_equals_host(host, case, capfd):
    src, ref = _points(200, 120, 2, A_TRUE) if case == "200" else rc.duplicate_rows_case()
    rc.check_device_equals_host(host, src, ref)
    capfd.readouterr()


def test_device_equals_host_on_failure(host, capfd):
    src, ref = rc.no_consensus_case()
    h, _ = rc.check_device_equals_host(host, src, ref, want_rc=-1, err_thresh=0.5)
    capfd.readouterr()
    assert np.abs(h[1]).max() > 0                                       # the best sample's model is left in tform


@pytest.mark.parametrize("num_iter", [500, 5000])
def test_device_equals_host_17874(host, pair_17874, num_iter, capfd):
    src, ref = pair_17874
    h, _ = rc.check_device_equals_host(host, src, ref, num_iter=num_iter)
    capfd.readouterr()
    assert np.abs(h[1] - A_TRUE * np.array([1, 1, 1, 5.0])).max() < 1.0


def test_profiling_times_the_device_path_and_changes_nothing(host, pair_17874, capfd):
    src, ref = pair_17874
    plain = rc.run_ransac(host, src, ref, DEVICE)
    host.imutil.sift3d_amd_set_ransac_profile(1)
    try:
        timed = rc.run_ransac(host, src, ref, DEVICE)
        ms = host.imutil.sift3d_amd_ransac_last_device_ms()
    finally:
        host.imutil.sift3d_amd_set_ransac_profile(0)
    capfd.readouterr()
    assert 0.0 < ms < 1000.0
    assert timed[0] == plain[0] == 0 and np.array_equal(timed[1], plain[1]) and timed[2] == plain[2] and timed[3] == 1


def test_auto_path(host, pair_17874, capfd):
    src, ref = pair_17874
    big = rc.run_ransac(host, src, ref, AUTO)
    src, ref = _points(60, 20, 1, A_TRUE)
    small = rc.run_ransac(host, src, ref, AUTO)
    capfd.readouterr()
    assert big[0] == 0 and big[3] == 1
    assert small[0] == 0 and small[3] == 0
