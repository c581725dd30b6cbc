"""Intensity-based refinement of an affine registration on the device: the cases of tests/refine_cases.py (the CPU counterpart is
tests/test_refine.py) against the numpy restatement, run-to-run determinism, the device-pointer entry point against the host
form, and regSift3D --refine --metrics end to end."""
import ctypes as C
import gzip
import os

import numpy as np
import pytest

import sift3d_amd
from sift3d_amd import abi, synth
from tests import refine_cases as rc
from tests import similarity_cases as sc
from tests.test_cli import BIN, _csv, run
from tests.test_host_io import nifti1_bytes

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def host():
    return sc.bind(sift3d_amd.load())


@pytest.fixture(scope="module")
def dev():
    return sift3d_amd.load_device()


@pytest.mark.parametrize("consts", [rc.RAW, rc.SCALED])
@pytest.mark.parametrize("shape", list(sc.SHAPES))
def test_kernel_sums_and_count(dev, shape, consts):
    rc.case_kernel(dev, shape, consts)


def test_shifted_lattice(dev):
    rc.case_shifted_lattice(dev)


def test_identity(dev):
    rc.case_identity(dev)


def test_no_overlap(host, dev, capfd):
    rc.case_no_overlap(dev, host)


def test_scratch_bounds(dev):
    rc.case_scratch_guard(dev)


def test_flat_entry_refuses_bad_arguments(dev):
    rc.case_flat_refusals(dev)


def test_two_calls_return_the_same_bits(dev):
    rc.case_determinism(dev)


def test_consistent_with_the_score(host, dev):
    rc.case_consistent_with_the_score(host, dev)


def test_clean_mid_start_one_level(host):
    rc.case_starts()
    rc.case_clean_mid(host)


def test_clean_large_start_two_levels(host):
    rc.case_clean_large(host)


def test_noisy_reference(host):
    rc.case_noisy(host)


def test_gain_and_offset(host):
    rc.case_gain_offset(host)


def test_already_optimal(host):
    rc.case_already_optimal(host)


def test_unrelated_volumes(host):
    rc.case_unrelated(host)


def test_public_entry_refusals(host, capfd):
    rc.case_refusals(host)
    capfd.readouterr()


def test_device_form_equals_the_host_form(host, dev):
    ref, src = sc.meaning_volumes()
    opts = rc.make_opts(levels=2)
    want = rc.refine(host, src, ref, sc.A_FIXED + rc.MID, opts)
    t, info = sc.make_affine(host, sc.A_FIXED + rc.MID), abi.RefineInfo()
    bufs = [dev.upload(src), dev.upload(ref)]
    try:
        got_rc = host.sift.sift3d_amd_refine_affine_dev(bufs[0], *src.shape[::-1], bufs[1], *ref.shape[::-1], C.byref(opts), C.byref(t),
                                                        C.byref(info), None)
        got = rc.affine_bytes(t)
    finally:
        for b in bufs:
            dev.free(b)
        host.imutil.cleanup_tform(C.byref(t))
    assert got_rc == 0 and want.rc == 0 and want.info.status != abi.REFINE_UNCHANGED and want.info.levels_run == 2
    assert got == want.after and bytes(info) == bytes(want.info)


def test_regSift3D_refine_metrics_end_to_end(tmp_path):
    """the synthetic 96 x 80 x 64 rolled pair of tests/test_gpu_similarity.py: three rows (identity, affine, refined) of seven
    columns, the refined row no worse than the affine row"""
    a = synth.blobs(96, 80, 64, 500, 21)
    b = np.roll(a, (3, -2, 1), axis=(2, 1, 0)).copy()
    for name, v in (("src", a), ("ref", b)):
        with gzip.open(str(tmp_path / f"{name}.nii.gz"), "wb") as f:
            f.write(nifti1_bytes(np.ascontiguousarray(v.transpose(2, 1, 0)), (1.0, 1.0, 1.5)))
    mp = str(tmp_path / "m.csv")
    r = run(os.path.join(BIN, "regSift3D"), "--refine", "--metrics", mp, str(tmp_path / "src.nii.gz"), str(tmp_path / "ref.nii.gz"))
    assert r.returncode == 0, r.stderr
    m = np.array(_csv(mp), np.float64)
    print(m)
    assert m.shape == (3, 7)
    assert m[2, 2] <= m[1, 2]                                           # mse: the refined row no worse than the affine row
    assert m[2, 0] >= 0.5 * m[1, 0]
