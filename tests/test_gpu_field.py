"""The inverse of a displacement field's map and its Jacobian determinant on the device: the cases of tests/field_cases.py (the CPU
counterpart is tests/test_field.py) against the numpy restatement -- every entry, status byte and determinant bit for bit, the
statistics, the meaning of the inverse, the host forms against the device forms -- and regSift3D --demons_inverse /
--demons_jacobian end to end."""
import gzip
import os
import re

import numpy as np
import pytest

import sift3d_amd
from sift3d_amd import synth
from tests import field_cases as fc
from tests import similarity_cases as sc
from tests.test_cli import BIN, run
from tests.test_gpu_demons import _nii
from tests.test_host_io import nifti1_bytes

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def host():
    return sc.bind(sift3d_amd.load())


@pytest.fixture(scope="module")
def dev():
    return sift3d_amd.load_device()


@pytest.mark.parametrize("amp", fc.AMPS)
@pytest.mark.parametrize("grid", list(fc.GRIDS))
def test_invert_per_voxel(dev, grid, amp):
    fc.case_invert(dev, grid, amp)


@pytest.mark.parametrize("shape", list(sc.SHAPES))
def test_invert_non_finite_entries(dev, shape):
    fc.case_invert_nonfinite(dev, shape)


@pytest.mark.parametrize("grid", list(fc.GRIDS))
def test_invert_zero_field(dev, grid):
    fc.case_zero_field(dev, grid)


def test_invert_constant_field(dev):
    fc.case_constant_field(dev)


def test_invert_without_updates_and_without_status(dev):
    fc.case_max_iter_zero(dev)


def test_invert_bounds(dev):
    fc.case_invert_guard(dev)


def test_invert_refuses_bad_arguments(dev):
    fc.case_invert_refusals(dev)


def test_inverse_composed_with_the_map_is_the_identity(dev):
    fc.case_meaning(dev)


@pytest.mark.parametrize("amp", fc.AMPS)
@pytest.mark.parametrize("grid", list(fc.GRIDS))
def test_jacobian_per_voxel(dev, grid, amp):
    fc.case_jacobian(dev, grid, amp)


@pytest.mark.parametrize("shape", list(sc.SHAPES))
def test_jacobian_non_finite_entries(dev, shape):
    fc.case_jacobian_nonfinite(dev, shape)


@pytest.mark.parametrize("base", ["fixed", "identity"])
@pytest.mark.parametrize("name", list(fc.LINEAR_G))
def test_jacobian_of_a_linear_field(dev, name, base):
    fc.case_jacobian_linear(dev, name, sc.A_FIXED if base == "fixed" else sc.A_IDENTITY)


def test_jacobian_bounds_and_refusals(dev):
    fc.case_jacobian_guard_and_refusals(dev)


def test_forms_agree_and_the_pair_is_a_map(host, dev):
    fc.case_forms_agree(host, dev)


def test_public_entry_refusals(host, capfd):
    fc.case_refusals(host)
    capfd.readouterr()


def test_regSift3D_inverse_and_jacobian_end_to_end(tmp_path):
    """the synthetic 96 x 80 x 64 rolled pair of tests/test_gpu_demons.py: the inverse field is a 4-D image on the source grid, the
    determinant a 3-D image on the reference grid, and the folded count the program prints is the number of values <= 0 in the map
    it wrote"""
    a = synth.blobs(96, 80, 64, 500, 21)
    b = np.roll(a, (3, -2, 1), axis=(2, 1, 0)).copy()
    for name, v in (("src", a), ("ref", b)):
        with gzip.open(str(tmp_path / f"{name}.nii.gz"), "wb") as f:
            f.write(nifti1_bytes(np.ascontiguousarray(v.transpose(2, 1, 0)), (1.0, 1.0, 1.5)))
    exe, s, r = os.path.join(BIN, "regSift3D"), str(tmp_path / "src.nii.gz"), str(tmp_path / "ref.nii.gz")
    inv, jac = str(tmp_path / "inv.nii.gz"), str(tmp_path / "jac.nii.gz")
    got = run(exe, "--refine", "--demons", "--demons_inverse", inv, "--demons_jacobian", jac, s, r)
    assert got.returncode == 0, got.stderr
    dim, body = _nii(inv)
    assert dim == (4, 96, 80, 64, 3) and len(body) == 4 * 3 * 96 * 80 * 64
    dim, body = _nii(jac)
    assert dim == (3, 96, 80, 64, 1) and len(body) == 4 * 96 * 80 * 64
    det = np.frombuffer(body, "<f4")
    m = re.search(r"Deformation: (\d+) folded voxels of (\d+), minimum determinant (\S+); inverse: (\d+) converged, (\d+) not "
                  r"converged of (\d+)", got.stdout)
    assert m, got.stdout
    print(m.group(0))
    assert int(m.group(1)) == int((det <= 0).sum()) and int(m.group(2)) == det.size == int(m.group(6))
    assert abs(float(m.group(3)) - float(det.min())) <= 1e-5 * max(1.0, abs(float(det.min())))      # printed with "%g"
    assert int(m.group(4)) + int(m.group(5)) <= det.size
