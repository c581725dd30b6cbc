"""The inverse of a displacement field's map and its Jacobian determinant (s3d_k_field_invert, s3d_k_field_jacobian,
sift3d_amd_invert_field, sift3d_amd_field_jacobian, sift3d_amd_field_apply_points) on the CPU: the kernels and the entry points run
through the SIMT emulator build of the library (tests/emu) against the numpy restatement of tests/field_cases.py, and regSift3D's
two new options are checked up to the point where an image would be read.  The GPU counterpart is tests/test_gpu_field.py."""
import ctypes as C
import os
import subprocess

import pytest

from sift3d_amd import abi, build as _b
from sift3d_amd.device import DeviceLib, bind_extensions
from tests import field_cases as fc
from tests import similarity_cases as sc
from tests.test_cli import BIN, run

EMU_DIR = os.path.join(sc.ROOT, "tests", "emu")


@pytest.fixture(scope="module")
def emu_cdll():
    subprocess.run(["sh", os.path.join(EMU_DIR, "build_emu.sh")], check=True, capture_output=True)
    L = C.CDLL(os.path.join(EMU_DIR, "libsift3d_emu.so"))
    bind_extensions(L)
    return L


@pytest.fixture(scope="module")
def emu(emu_cdll):
    return sc.bind(abi.Sift3dLib(emu_cdll, None, "emulated"))


@pytest.fixture(scope="module")
def emu_dev(emu_cdll):
    return DeviceLib(emu_cdll)


def test_struct_layouts(tmp_path):
    fc.case_struct_layouts(tmp_path)


@pytest.mark.parametrize("amp", fc.AMPS)
@pytest.mark.parametrize("grid", list(fc.GRIDS))
def test_invert_per_voxel(emu_dev, grid, amp):
    fc.case_invert(emu_dev, grid, amp)


@pytest.mark.parametrize("shape", list(sc.SHAPES))
def test_invert_non_finite_entries(emu_dev, shape):
    fc.case_invert_nonfinite(emu_dev, shape)


@pytest.mark.parametrize("grid", list(sc.SHAPES))          # (the emulator takes 20 s per launch on 48x44x40: the GPU suite has it)
def test_invert_zero_field(emu_dev, grid):
    fc.case_zero_field(emu_dev, grid)


def test_invert_constant_field(emu_dev):
    fc.case_constant_field(emu_dev)


def test_invert_without_updates_and_without_status(emu_dev):
    fc.case_max_iter_zero(emu_dev)


def test_invert_bounds(emu_dev):
    fc.case_invert_guard(emu_dev)


def test_invert_refuses_bad_arguments(emu_dev):
    fc.case_invert_refusals(emu_dev)


def test_inverse_composed_with_the_map_is_the_identity(emu_dev):
    fc.case_meaning(emu_dev)


@pytest.mark.parametrize("amp", fc.AMPS)
@pytest.mark.parametrize("grid", list(fc.GRIDS))
def test_jacobian_per_voxel(emu_dev, grid, amp):
    fc.case_jacobian(emu_dev, grid, amp)


@pytest.mark.parametrize("shape", list(sc.SHAPES))
def test_jacobian_non_finite_entries(emu_dev, shape):
    fc.case_jacobian_nonfinite(emu_dev, shape)


@pytest.mark.parametrize("base", ["fixed", "identity"])
@pytest.mark.parametrize("name", list(fc.LINEAR_G))
def test_jacobian_of_a_linear_field(emu_dev, name, base):
    fc.case_jacobian_linear(emu_dev, name, sc.A_FIXED if base == "fixed" else sc.A_IDENTITY)


def test_jacobian_bounds_and_refusals(emu_dev):
    fc.case_jacobian_guard_and_refusals(emu_dev)


def test_forms_agree_and_the_pair_is_a_map(emu, emu_dev):
    fc.case_forms_agree(emu, emu_dev)


def test_public_entry_refusals(emu, capfd):
    fc.case_refusals(emu)
    capfd.readouterr()


def test_regSift3D_field_options():
    """--help shows the two options inside "Deformable options:" and leaves the text below "Other options:" alone; each is refused
    without --demons before any image is read (the files do not exist)"""
    _b.build()
    exe = os.path.join(BIN, "regSift3D")
    r = run(exe, "--help")
    assert r.returncode == 0
    head, tail = r.stdout.split("Other options:")
    block = head[head.index("Deformable options:"):]
    for opt in ("--demons_inverse [filename]", "--demons_jacobian [filename]"):
        assert opt in block, opt
    assert "--demons" not in tail and tail.lstrip().startswith("--nn_thresh [value]")
    for args, msg in ((["--demons_inverse", "i.nii", "--warped", "w.nii", "a", "b"], "--demons_inverse needs --demons."),
                      (["--demons_jacobian", "j.nii", "a", "b"], "--demons_jacobian needs --demons."),
                      (["--refine", "--demons_inverse", "i.nii", "--demons_jacobian", "j.nii", "a", "b"], "--demons_inverse needs --demons.")):
        r = run(exe, *args)
        assert r.returncode == 1 and msg in r.stderr and "Failed to read" not in r.stderr, (args, r.stderr)
    r = run(exe, "--demons", "--demons_inverse", "i.nii", "--demons_jacobian", "j.nii", "a", "b")   # accepted: fails at the missing file
    assert r.returncode == 1 and "Failed to read the source image" in r.stderr
