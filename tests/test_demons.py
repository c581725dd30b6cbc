"""Deformable registration (sift3d_amd_register_demons, s3d_k_demons_step, s3d_k_inv_field, s3d_k_field_upsample2) on the CPU:
the kernels and the driver run through the SIMT emulator build of the library (tests/emu) against the numpy restatement of
tests/demons_cases.py, and regSift3D's --demons options are checked up to the point where an image would be read.  The GPU
counterpart is tests/test_gpu_demons.py."""
import ctypes as C
import os
import subprocess

import pytest

from sift3d_amd import abi, build as _b
from sift3d_amd.device import DeviceLib, bind_extensions
from tests import demons_cases as dc
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
    """the ctypes mirrors against the C definitions: sizes and offsets as the compiler lays them out"""
    dc.case_struct_layouts()
    fields = {"sift3d_amd_demons_opts": ("levels", "max_iter", "sigma", "max_step", "tol", "min_overlap", "normalize"),
              "sift3d_amd_demons_info": ("status", "levels_run", "iters", "passes", "n_before", "n_after", "cost_before",
                                         "cost_after", "mean_disp", "max_disp")}
    body = "".join(f'printf("%zu", sizeof({t}));' + "".join(f'printf(" %zu", offsetof({t}, {f}));' for f in fs) + 'printf("\\n");'
                   for t, fs in fields.items())
    (tmp_path / "layout.c").write_text(f'#include <stddef.h>\n#include <stdio.h>\n#include "sift3d_amd.h"\nint main(void) {{ {body} return 0; }}\n')
    subprocess.run(["gcc", "-std=gnu11", "-I", os.path.join(sc.ROOT, "include"), str(tmp_path / "layout.c"), "-o", str(tmp_path / "layout")],
                   check=True)
    out = subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout.split("\n")
    for line, cls in zip(out, (abi.DemonsOpts, abi.DemonsInfo)):
        assert [int(v) for v in line.split()] == [C.sizeof(cls)] + [getattr(cls, f).offset for f, _ in cls._fields_]


@pytest.mark.parametrize("setting", list(dc.STEP_SETTINGS))
@pytest.mark.parametrize("shape", list(sc.SHAPES))
def test_step_per_voxel(emu_dev, shape, setting):
    dc.case_step(emu_dev, shape, setting)


def test_step_scratch_bounds(emu_dev):
    dc.case_step_scratch_guard(emu_dev)


def test_flat_entries_refuse_bad_arguments(emu_dev):
    dc.case_flat_refusals(emu_dev)


@pytest.mark.parametrize("nc", [1, 2])
@pytest.mark.parametrize("interp", [0, 1])
def test_warp_through_a_zero_field(emu_dev, interp, nc):
    dc.case_warp_zero_field(emu_dev, interp, nc)


@pytest.mark.parametrize("interp", [0, 1])
def test_warp_through_a_constant_field(emu_dev, interp):
    dc.case_warp_constant_field(emu_dev, interp)


@pytest.mark.parametrize("shape", list(sc.SHAPES))
def test_warp_through_a_random_field(emu_dev, shape):
    dc.case_warp_random_field(emu_dev, shape)


@pytest.mark.parametrize("fdims", [(70, 33, 9), (71, 32, 8)])
def test_upsample(emu_dev, fdims):
    dc.case_upsample(emu_dev, fdims)


@pytest.mark.parametrize("shape", list(sc.SHAPES))
def test_field_norm(emu_dev, shape):
    dc.case_field_norm(emu_dev, shape)


def test_nothing_to_do(emu, emu_dev):
    dc.case_nothing_to_do(emu, emu_dev)


def test_recovery_of_a_known_deformation(emu):
    dc.case_recovery(emu, "emulator")


def test_no_transform_is_the_identity(emu):
    dc.case_no_transform(emu)


def test_normalized_intensities(emu):
    dc.case_normalized(emu)


def test_hopeless_pair(emu, emu_dev):
    dc.case_hopeless(emu, emu_dev)


def test_forms_agree(emu, emu_dev, tmp_path):
    """(six passes per level, enough to reach the stopping rule: a whole call of the recovery case takes the emulator a minute,
    and the GPU suite compares the forms on that)"""
    dc.case_forms_agree(emu, emu_dev, tmp_path, dc.recovery_opts(max_iter=6))


def test_public_entry_refusals(emu, capfd):
    dc.case_refusals(emu)
    capfd.readouterr()


def test_regSift3D_demons_options():
    """--help shows the new block between "Refinement options:" and "Other options:" and leaves the text below as it was; bad
    values and forbidden combinations fail with their messages before any image is read (the files do not exist)"""
    _b.build()
    exe = os.path.join(BIN, "regSift3D")
    r = run(exe, "--help")
    assert r.returncode == 0
    head, tail = r.stdout.split("Other options:")
    for opt in ("Deformable options:", " --demons - ", "--demons_levels [value]", "--demons_iter [value]", "--demons_sigma [value]",
                "--demons_field [filename]"):
        assert opt in head, opt
    assert head.index("Refinement options:") < head.index("Deformable options:")
    assert "--demons" not in tail and tail.lstrip().startswith("--nn_thresh [value]")
    for args, msg in ((["--demons", "--demons_levels", "0", "--warped", "w.nii", "a", "b"], "Invalid value for demons_levels."),
                      (["--demons", "--demons_iter", "-3", "--warped", "w.nii", "a", "b"], "Invalid value for demons_iter."),
                      (["--demons", "--demons_sigma", "0.2", "--warped", "w.nii", "a", "b"], "Invalid value for demons_sigma."),
                      (["--demons", "--demons_sigma", "9", "--warped", "w.nii", "a", "b"], "Invalid value for demons_sigma."),
                      (["--demons", "--tps", "--warped", "w.nii", "a", "b"], "--demons cannot be combined with --tps."),
                      (["--demons", "--resample", "--warped", "w.nii", "a", "b"], "--demons cannot be combined with --resample."),
                      (["--demons_field", "f.nii", "--warped", "w.nii", "a", "b"], "--demons_field needs --demons.")):
        r = run(exe, *args)
        assert r.returncode == 1 and msg in r.stderr and "Failed to read" not in r.stderr, (args, r.stderr)
    r = run(exe, "--refine", "--demons", "--demons_field", "f.nii", "a", "b")       # accepted: fails only at the missing file
    assert r.returncode == 1 and "Failed to read the source image" in r.stderr
