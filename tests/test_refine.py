"""Intensity-based refinement of an affine registration (sift3d_amd_refine_affine, s3d_k_affine_normal_eq) on the CPU: the kernel
and the optimiser run through the SIMT emulator build of the library (tests/emu) against the numpy restatement of
tests/refine_cases.py, and regSift3D's --refine options are checked up to the point where an image would be read.  The GPU
counterpart is tests/test_gpu_refine.py."""
import ctypes as C
import os
import subprocess

import pytest

from sift3d_amd import abi, build as _b
from sift3d_amd.device import DeviceLib, bind_extensions
from tests import refine_cases as rc
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
    rc.case_struct_layouts()
    fields = {"sift3d_amd_refine_opts": ("levels", "max_iter", "tol", "min_overlap", "normalize"),
              "sift3d_amd_refine_info": ("status", "levels_run", "iters", "passes", "n_before", "n_after", "cost_before",
                                         "cost_after", "max_corner_shift")}
    body = "".join(f'printf("%zu", sizeof({t}));' + "".join(f'printf(" %zu", offsetof({t}, {f}));' for f in fs) + 'printf("\\n");'
                   for t, fs in fields.items())
    (tmp_path / "layout.c").write_text(f'#include <stddef.h>\n#include <stdio.h>\n#include "sift3d_amd.h"\nint main(void) {{ {body} return 0; }}\n')
    subprocess.run(["gcc", "-std=gnu11", "-I", os.path.join(sc.ROOT, "include"), str(tmp_path / "layout.c"), "-o", str(tmp_path / "layout")],
                   check=True)
    out = subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout.split("\n")
    for line, cls in zip(out, (abi.RefineOpts, abi.RefineInfo)):
        assert [int(v) for v in line.split()] == [C.sizeof(cls)] + [getattr(cls, f).offset for f, _ in cls._fields_]


def test_the_starts_are_as_far_off_as_stated():
    rc.case_starts()


@pytest.mark.parametrize("consts", [rc.RAW, rc.SCALED])
@pytest.mark.parametrize("shape", list(sc.SHAPES))
def test_kernel_sums_and_count(emu_dev, shape, consts):
    rc.case_kernel(emu_dev, shape, consts)


def test_shifted_lattice(emu_dev):
    rc.case_shifted_lattice(emu_dev)


def test_identity(emu_dev):
    rc.case_identity(emu_dev)


def test_no_overlap(emu, emu_dev, capfd):
    rc.case_no_overlap(emu_dev, emu)


def test_scratch_bounds(emu_dev):
    rc.case_scratch_guard(emu_dev)


def test_flat_entry_refuses_bad_arguments(emu_dev):
    rc.case_flat_refusals(emu_dev)


def test_two_calls_return_the_same_bits(emu_dev):
    rc.case_determinism(emu_dev)


def test_consistent_with_the_score(emu, emu_dev):
    rc.case_consistent_with_the_score(emu, emu_dev)


def test_clean_mid_start_one_level(emu):
    rc.case_clean_mid(emu)


def test_clean_large_start_two_levels(emu):
    rc.case_clean_large(emu)


def test_noisy_reference(emu):
    rc.case_noisy(emu)


def test_gain_and_offset(emu):
    rc.case_gain_offset(emu)


def test_already_optimal(emu):
    rc.case_already_optimal(emu)


def test_unrelated_volumes(emu):
    rc.case_unrelated(emu)


def test_public_entry_refusals(emu, capfd):
    rc.case_refusals(emu)
    capfd.readouterr()


def test_regSift3D_refine_options():
    """--help shows the new block between "Similarity options:" and "Other options:" and leaves the text below as it was; bad
    values and forbidden combinations fail with their messages before any image is read (the files do not exist)"""
    _b.build()
    exe = os.path.join(BIN, "regSift3D")
    r = run(exe, "--help")
    assert r.returncode == 0
    head, tail = r.stdout.split("Other options:")
    for opt in ("Refinement options:", " --refine - ", "--refine_levels [value]", "--refine_iter [value]", " --refine_normalize - "):
        assert opt in head, opt
    assert head.index("Similarity options:") < head.index("Refinement options:")
    assert "--refine" not in tail and tail.lstrip().startswith("--nn_thresh [value]")
    ref_exe = os.path.join(sc.ROOT, "oracle", "_ref", "bin", "regSift3D")
    if os.path.exists(ref_exe):
        assert tail == run(ref_exe, "--help").stdout.split("Other options:")[1]
    for args, msg in ((["--refine", "--refine_levels", "0", "--transform", "t.csv", "a", "b"], "Invalid value for refine_levels."),
                      (["--refine", "--refine_levels", "-2", "--transform", "t.csv", "a", "b"], "Invalid value for refine_levels."),
                      (["--refine", "--refine_iter", "0", "--transform", "t.csv", "a", "b"], "Invalid value for refine_iter."),
                      (["--refine", "--refine_iter", "x", "--transform", "t.csv", "a", "b"], "Invalid value for refine_iter."),
                      (["--refine", "--resample", "--transform", "t.csv", "a", "b"], "--refine cannot be combined with --resample."),
                      (["--refine", "--tps", "--transform", "t.csv", "a", "b"], "--refine cannot be combined with --tps."),
                      (["--refine", "--type", "tps", "--transform", "t.csv", "a", "b"], "Unrecognized transformation type: tps")):
        r = run(exe, *args)
        assert r.returncode == 1 and msg in r.stderr and "Failed to read" not in r.stderr, (args, r.stderr)
    r = run(exe, "--refine", "--refine_normalize", "--transform", "t.csv", "a", "b")    # accepted: fails only at the missing file
    assert r.returncode == 1 and "Failed to read the source image" in r.stderr
