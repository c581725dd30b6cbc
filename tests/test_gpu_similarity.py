"""Similarity scores of a registration on the device: the cases of tests/similarity_cases.py (the CPU counterpart is
tests/test_similarity.py) against the numpy restatement, run-to-run determinism, the device-pointer entry point against the host
form, and regSift3D --tps --metrics end to end."""
import ctypes as C
import gzip
import os

import numpy as np
import pytest

import sift3d_amd
from sift3d_amd import abi, synth
from tests import similarity_cases as sc
from tests import tps_cases as tc
from tests.test_cli import BIN, _csv, run
from tests.test_host_io import nifti1_bytes

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def host():
    return sc.bind(sift3d_amd.load())


@pytest.fixture(scope="module")
def dev():
    return sift3d_amd.load_device()


@pytest.mark.parametrize("bins", sc.BINS)
@pytest.mark.parametrize("shape", list(sc.SHAPES))
def test_affine_linear_histogram_and_sums(dev, shape, bins):
    sc.case_affine_linear(dev, shape, bins)


@pytest.mark.parametrize("shape,bins", [("70x33x9", 64), ("257x19x5", 37)])
def test_aggregated_histogram_update(dev, shape, bins):
    sc.case_aggregated(dev, shape, bins)


@pytest.mark.parametrize("shape,bins", [("70x33x9", 37), ("257x19x5", 128)])
def test_public_entry_statistics(host, shape, bins):
    sc.case_api(host, shape, bins)


def test_kept_voxel_counts(host):
    sc.case_counts(host)


def test_identity(host):
    sc.case_identity(host)


def test_degenerate_volumes(host):
    sc.case_degenerate(host)


@pytest.mark.parametrize("n", [0, 1, tc.TILE + 1])
def test_consistent_with_the_spline_warp(host, dev, n):
    sc.case_consistency_tps(host, dev, n)


def test_consistent_with_the_lanczos_warp(host, dev):
    sc.case_consistency_lanczos(host, dev)


def test_meaning(host):
    sc.case_meaning(host)


def test_refusals(host, capfd):
    sc.case_refusals(host)
    capfd.readouterr()


def test_two_calls_return_the_same_bits(dev):
    ref, src = sc.volumes("257x19x5")
    w = sc.want_affine("257x19x5", sc.A_FIXED, 64)
    h1, s1 = sc.kernel_affine(dev, src, ref, sc.A_FIXED, 64, w)
    h2, s2 = sc.kernel_affine(dev, src, ref, sc.A_FIXED, 64, w)
    assert np.array_equal(h1, h2) and np.array_equal(s1.view(np.uint64), s2.view(np.uint64))
    assert s1.any()


def test_device_form_equals_the_host_form(host, dev):
    ref, src = sc.volumes("70x33x9")
    t = sc.make_affine(host, sc.A_FIXED)
    opts = sc.make_opts(37)
    want = sc.similarity(host, t, src, ref, opts, 37)
    bufs = [dev.upload(src), dev.upload(ref)]
    out, joint = abi.Similarity(), np.zeros(37 * 37, np.uint64)
    try:
        rc = host.sift.sift3d_amd_similarity_dev(C.addressof(t), bufs[0], *src.shape[::-1], bufs[1], *ref.shape[::-1], C.byref(opts),
                                                 C.byref(out), joint.ctypes.data, None)
    finally:
        for b in bufs:
            dev.free(b)
        host.imutil.cleanup_tform(C.byref(t))
    assert rc == 0 and want.rc == 0 and want.n > 0
    assert bytes(out) == bytes(want.out) and np.array_equal(joint.reshape(37, 37), want.hist)


def test_regSift3D_metrics_end_to_end(tmp_path):
    """the synthetic 96 x 80 x 64 pair of tests/test_reg.py: three rows (identity, affine, spline) of seven columns"""
    a = synth.blobs(96, 80, 64, 500, 21)
    b = np.roll(a, (3, -2, 1), axis=(2, 1, 0)).copy()
    for name, v in (("src", a), ("ref", b)):
        with gzip.open(str(tmp_path / f"{name}.nii.gz"), "wb") as f:
            f.write(nifti1_bytes(np.ascontiguousarray(v.transpose(2, 1, 0)), (1.0, 1.0, 1.5)))
    mp = str(tmp_path / "m.csv")
    r = run(os.path.join(BIN, "regSift3D"), "--tps", "--metrics", mp, str(tmp_path / "src.nii.gz"), str(tmp_path / "ref.nii.gz"))
    assert r.returncode == 0, r.stderr
    m = np.array(_csv(mp), np.float64)
    print(m)
    assert m.shape == (3, 7)
    assert (m[:, 0] <= m[:, 1]).all() and (m[:, 1] == 96 * 80 * 64).all() and m[0, 0] == 96 * 80 * 64
    assert m[1, 4] > m[0, 4]                                            # ncc: the affine row above the identity row
