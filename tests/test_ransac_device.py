"""RANSAC hypotheses scored on the device (s3d_k_ransac_count, find_tform_ransac's DEVICE path), on the CPU: the kernel and
the host's device path run through the SIMT emulator build of the library (tests/emu), against a numpy restatement of the
count, against the host path, and against the reference estimator with the same rand() seed.  The GPU counterpart is
tests/test_gpu_ransac.py."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import sift3d_amd
from sift3d_amd import abi
from sift3d_amd.device import DeviceLib, bind_extensions
from tests import ransac_cases as rc
from tests.ransac_cases import AUTO, DEVICE, HOST
from tests.test_reg import A_TRUE, _points

EMU_DIR = os.path.join(rc.ROOT, "tests", "emu")
EMU_LIB = os.path.join(EMU_DIR, "libsift3d_emu.so")


@pytest.fixture(scope="module")
def emu_cdll():
    subprocess.run(["sh", os.path.join(EMU_DIR, "build_emu.sh")], check=True, capture_output=True)
    L = C.CDLL(EMU_LIB)
    bind_extensions(L)
    return L


@pytest.fixture(scope="module")
def emu(emu_cdll):
    return rc.bind_ransac(abi.Sift3dLib(emu_cdll, None, "emulated"))


@pytest.fixture(scope="module")
def emu_dev(emu_cdll):
    return DeviceLib(emu_cdll)


# ---- the kernel ----------------------------------------------------------------------------------------------------------
def test_case_grid_covers_the_model_tile():
    assert {rc.TILE - 1, rc.TILE, rc.TILE + 1} <= set(rc.NMODELS) and {1, 2, 63, 64, 65, 257} <= set(rc.NMODELS)


@pytest.mark.parametrize("npts", rc.NPTS)
def test_kernel_counts_equal_numpy(emu_dev, npts):
    rc.check_kernel_grid(emu_dev, npts)


def test_kernel_does_not_contract(emu_dev):
    """matches whose residual falls on the other side of thr2 when a multiply-add is fused"""
    rc.check_no_contraction(emu_dev)


def test_kernel_refuses_empty_sizes(emu_dev):
    src, ref, models = rc.kernel_inputs(8, 3, 25.0)
    bufs = [emu_dev.upload(a) for a in (src, ref, models, np.zeros(3, np.int32))]
    L = emu_dev.L
    for npts, nm in ((0, 3), (8, 0), (0, 0)):
        assert L.s3d_k_ransac_count(bufs[0], bufs[1], npts, bufs[2], nm, 25.0, bufs[3], None) != 0
        assert emu_dev.err()
    assert L.s3d_k_ransac_count(bufs[0], bufs[1], 8, bufs[2], (65535 * rc.TILE) + 1, 25.0, bufs[3], None) != 0   # grid overflow
    for b in bufs:
        emu_dev.free(b)


# ---- find_tform_ransac: DEVICE against HOST against the reference ---------------------------------------------------------
API_CASES = {
    "60": lambda: _points(60, 20, 1, A_TRUE),
    "200": lambda: _points(200, 120, 2, A_TRUE),
    "12": lambda: _points(12, 2, 3, A_TRUE),
    "5": lambda: _points(5, 0, 4, A_TRUE),
    "duplicate-rows": rc.duplicate_rows_case,
}


@pytest.mark.parametrize("case", list(API_CASES))
def test_find_tform_ransac_device_equals_host_and_matches_reference(emu, reference, case, capfd):
    rc.bind_ransac(reference)
    src, ref = API_CASES[case]()
    h, d = rc.check_device_equals_host(emu, src, ref)
    r = rc.run_ransac(reference, src, ref)
    capfd.readouterr()
    assert r[0] == 0
    for got in (h, d):
        assert np.abs(got[1] - r[1]).max() <= 1e-9
    assert h[2] == r[2]                                                # the reference has consumed the same rand() stream


def test_no_consensus_fails_alike_and_leaves_the_best_sample(emu, reference, capfd):
    rc.bind_ransac(reference)
    src, ref = rc.no_consensus_case()
    h, d = rc.check_device_equals_host(emu, src, ref, want_rc=-1, err_thresh=0.5)
    r = rc.run_ransac(reference, src, ref, err_thresh=0.5)
    capfd.readouterr()
    assert r[0] == -1
    for got in (h, d):                                                 # what the failed call leaves in tform: the reference's matrix
        assert np.abs(got[1] - r[1]).max() <= 1e-9
    assert h[2] == r[2]
    # the four sampled points fit their own model, so some hypothesis had a count: its model is what the call leaves behind
    assert np.abs(h[1]).max() > 0
    assert 4 <= rc.np_counts(src, ref, h[1].reshape(1, 12), 0.25)[0] < 5


@pytest.mark.parametrize("num_iter", [1, rc.BATCH - 1, rc.BATCH, rc.BATCH + 1])
def test_batch_edges(emu, num_iter, capfd):
    src, ref = _points(12, 2, 3, A_TRUE)
    h, _ = rc.check_device_equals_host(emu, src, ref, want_rc=None, num_iter=num_iter)   # (a single draw may hit an outlier)
    capfd.readouterr()
    assert h[0] == (0 if num_iter > 1 else -1)


def test_profiling_times_the_device_path_and_changes_nothing(emu, emu_cdll, capfd):
    src, ref = _points(200, 120, 2, A_TRUE)
    plain = rc.run_ransac(emu, src, ref, DEVICE, num_iter=rc.BATCH + 5)     # two batches
    emu_cdll.sift3d_amd_set_ransac_profile(1)
    try:
        timed = rc.run_ransac(emu, src, ref, DEVICE, num_iter=rc.BATCH + 5)
        ms = emu_cdll.sift3d_amd_ransac_last_device_ms()
        on_host = rc.run_ransac(emu, src, ref, HOST, num_iter=rc.BATCH + 5)
        ms_host = emu_cdll.sift3d_amd_ransac_last_device_ms()
    finally:
        emu_cdll.sift3d_amd_set_ransac_profile(0)
    capfd.readouterr()
    assert ms >= 0.0 and ms_host == 0.0
    for got in (timed, on_host):
        assert got[0] == plain[0] == 0 and np.array_equal(got[1], plain[1]) and got[2] == plain[2]
    assert (plain[3], timed[3], on_host[3]) == (1, 1, 0)


# ---- the knob ------------------------------------------------------------------------------------------------------------
def test_knob_round_trip_and_invalid_mode(emu_cdll):
    L = emu_cdll
    L.sift3d_amd_last_error.restype = C.c_char_p
    try:
        for m in (HOST, DEVICE, AUTO):
            assert L.sift3d_amd_set_ransac_device(m) == 0 and L.sift3d_amd_get_ransac_device() == m
        assert L.sift3d_amd_set_ransac_device(DEVICE) == 0
        for bad in (2, -2, 7):
            assert L.sift3d_amd_set_ransac_device(bad) == -1
            assert b"sift3d_amd_set_ransac_device" in L.sift3d_amd_last_error()
            assert L.sift3d_amd_get_ransac_device() == DEVICE          # left as it was
    finally:
        L.sift3d_amd_set_ransac_device(AUTO)


_CHILD = """
import ctypes as C, sys
L = C.CDLL(sys.argv[1])
print(L.sift3d_amd_get_ransac_device())
assert L.sift3d_amd_set_ransac_device(0) == 0
print(L.sift3d_amd_get_ransac_device())
"""


@pytest.mark.parametrize("value,want", [("1", 1), ("0", 0), ("-1", -1), (None, -1), ("", -1), ("2", -1), ("device", -1), ("1x", -1)])
def test_environment_variable_sets_the_default(emu_cdll, value, want):
    env = {k: v for k, v in os.environ.items() if k != "SIFT3D_RANSAC_DEVICE"}
    if value is not None:
        env["SIFT3D_RANSAC_DEVICE"] = value
    p = subprocess.run([sys.executable, "-c", _CHILD, EMU_LIB], env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    assert p.stdout.split() == [str(want), "0"]                        # a call overrides the environment


def test_auto_takes_the_host_path_below_the_threshold_and_the_device_above(emu, capfd):
    """the emulator reports one device, so AUTO's choice depends on npts * num_iter alone"""
    src, ref = _points(60, 20, 1, A_TRUE)
    small = rc.run_ransac(emu, src, ref, AUTO)
    src, ref = _points(2048, 1024, 5, A_TRUE)
    k = rc.AUTO_MIN_WORK // 2048                                       # 2048 * k is the threshold exactly
    below = rc.run_ransac(emu, src, ref, AUTO, num_iter=k - 1)
    big = rc.run_ransac(emu, src, ref, AUTO, num_iter=k)
    ref_big = rc.run_ransac(emu, src, ref, HOST, num_iter=k)
    capfd.readouterr()
    assert small[0] == 0 and small[3] == 0 and below[0] == 0 and below[3] == 0
    assert big[0] == 0 and big[3] == 1
    assert np.array_equal(big[1], ref_big[1]) and big[2] == ref_big[2]


def test_product_library_without_a_device(capfd):
    """AUTO falls back to the host path silently, DEVICE fails with a message"""
    if sift3d_amd.load_device().device_count() > 0:
        pytest.skip("this machine has a device")
    host = rc.bind_ransac(sift3d_amd.load())
    src, ref = _points(2048, 1024, 5, A_TRUE)
    k = rc.AUTO_MIN_WORK // 2048
    a = rc.run_ransac(host, src, ref, AUTO, num_iter=k)                # at the AUTO threshold: the device is looked for
    h = rc.run_ransac(host, src, ref, HOST, num_iter=k)
    assert a[0] == h[0] == 0 and a[3] == 0 and np.array_equal(a[1], h[1]) and a[2] == h[2]
    d = rc.run_ransac(host, src, ref, DEVICE, num_iter=k)
    capfd.readouterr()
    assert d[0] == -1 and d[3] == 0
    assert b"find_tform_ransac" in host.imutil.sift3d_amd_last_error()
