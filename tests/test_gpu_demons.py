"""Deformable registration on the device: the cases of tests/demons_cases.py (the CPU counterpart is tests/test_demons.py) against
the numpy restatement -- the per-voxel update, the warp through a field, the upsampling, the driver on a known deformation and on
a hopeless pair, the device-pointer entry point against the host form -- and regSift3D --demons end to end."""
import ctypes as C
import gzip
import os
import struct

import numpy as np
import pytest

import sift3d_amd
from sift3d_amd import synth
from tests import demons_cases as dc
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


@pytest.mark.parametrize("setting", list(dc.STEP_SETTINGS))
@pytest.mark.parametrize("shape", list(sc.SHAPES))
def test_step_per_voxel(dev, shape, setting):
    dc.case_step(dev, shape, setting)


def test_step_scratch_bounds(dev):
    dc.case_step_scratch_guard(dev)


def test_flat_entries_refuse_bad_arguments(dev):
    dc.case_flat_refusals(dev)


@pytest.mark.parametrize("nc", [1, 2])
@pytest.mark.parametrize("interp", [0, 1])
def test_warp_through_a_zero_field(dev, interp, nc):
    dc.case_warp_zero_field(dev, interp, nc)


@pytest.mark.parametrize("interp", [0, 1])
def test_warp_through_a_constant_field(dev, interp):
    dc.case_warp_constant_field(dev, interp)


@pytest.mark.parametrize("shape", list(sc.SHAPES))
def test_warp_through_a_random_field(dev, shape):
    dc.case_warp_random_field(dev, shape)


@pytest.mark.parametrize("fdims", [(70, 33, 9), (71, 32, 8)])
def test_upsample(dev, fdims):
    dc.case_upsample(dev, fdims)


@pytest.mark.parametrize("shape", list(sc.SHAPES))
def test_field_norm(dev, shape):
    dc.case_field_norm(dev, shape)


def test_nothing_to_do(host, dev):
    dc.case_nothing_to_do(host, dev)


def test_recovery_of_a_known_deformation(host):
    dc.case_recovery(host, "device")


def test_no_transform_is_the_identity(host):
    dc.case_no_transform(host)


def test_normalized_intensities(host):
    dc.case_normalized(host)


def test_hopeless_pair(host, dev):
    dc.case_hopeless(host, dev)


def test_forms_agree(host, dev, tmp_path):
    dc.case_forms_agree(host, dev, tmp_path, dc.recovery_opts())


def test_public_entry_refusals(host, capfd):
    dc.case_refusals(host)
    capfd.readouterr()


def _nii(path):
    """(dim[0 .. 5), the voxel bytes) of a gzipped NIfTI-1 file"""
    with gzip.open(path, "rb") as f:
        raw = f.read()
    return struct.unpack_from("<8h", raw, 40)[:5], raw[352:]


def _through_the_written_map(host, t_csv, src, warped):
    """the largest difference between a --warped volume and the library's own im_inv_transform of src through the map --transform
    wrote beside it, and the bound on it.  The file holds the map to six decimals ("%f"), so each entry is within 5e-7 of the one
    the program warped with: a coordinate moves by at most 5e-7 (nx + ny + nz + 1) voxels, and the tri-linear interpolant by at
    most that times the sum over the axes of the largest difference between neighbouring source voxels (its slope along an axis
    is a convex combination of such differences), plus a rounding of the float result.  Voxels whose coordinate is within 1e-3 of
    the source's faces, where the rounded map may decide inside against outside differently, are left out."""
    A = np.array(_csv(t_csv), np.float64)[:3, :4]
    nz, ny, nx = src.shape
    t = sc.make_affine(host, A)
    try:
        own = sc.warp(host, t, src, (nx, ny, nz), 0)
    finally:
        host.imutil.cleanup_tform(C.byref(t))
    coords = sc.affine_coords(A, (nx, ny, nz))
    clear = np.ones(src.shape, bool)
    for c, n in zip(coords, (nx, ny, nz)):
        clear &= (np.abs(c) > 1e-3) & (np.abs(c - (n - 1)) > 1e-3)
    slope = sum(float(np.abs(np.diff(src.astype(np.float64), axis=ax)).max()) for ax in range(3))
    bound = 5e-7 * (nx + ny + nz + 1) * slope + 4 * float(np.spacing(np.abs(src).max()))
    return float(np.abs(own.astype(np.float64) - warped)[clear].max()), bound, int(clear.sum())


def test_regSift3D_demons_end_to_end(host, tmp_path):
    """the synthetic 96 x 80 x 64 rolled pair of tests/test_gpu_refine.py: the field is a 4-D image on the reference grid, --tps is
    refused, and without --demons the warped image is the affine warp through the map the run wrote, whatever the other new
    options say"""
    a = synth.blobs(96, 80, 64, 500, 21)
    b = np.roll(a, (3, -2, 1), axis=(2, 1, 0)).copy()
    for name, v in (("src", a), ("ref", b)):
        with gzip.open(str(tmp_path / f"{name}.nii.gz"), "wb") as f:
            f.write(nifti1_bytes(np.ascontiguousarray(v.transpose(2, 1, 0)), (1.0, 1.0, 1.5)))
    exe, s, r = os.path.join(BIN, "regSift3D"), str(tmp_path / "src.nii.gz"), str(tmp_path / "ref.nii.gz")
    f, w, w0, w1 = (str(tmp_path / n) for n in ("f.nii.gz", "w.nii.gz", "w0.nii.gz", "w1.nii.gz"))
    got = run(exe, "--refine", "--demons", "--demons_field", f, "--warped", w, s, r)
    assert got.returncode == 0, got.stderr
    dim, body = _nii(f)
    assert dim == (4, 96, 80, 64, 3) and len(body) == 4 * 3 * 96 * 80 * 64
    assert _nii(w)[0] == (3, 96, 80, 64, 1)
    got = run(exe, "--demons", "--tps", "--warped", w, s, r)
    assert got.returncode == 1 and "--demons cannot be combined with --tps." in got.stderr
    # Without --demons nothing of the new path runs.  Each of the two runs below -- one plain, one with the other new options,
    # which are inert without --demons -- must have written the affine warp through the map it wrote with --transform.  (The two
    # files are not compared with each other: find_tform_ransac does not return the same map, to the last bit, in every run on
    # one set of matches, so two registrations of one pair may warp through maps that print alike and differ below 1e-6.)
    for k, (path, extra) in enumerate(((w0, ()), (w1, ("--demons_levels", "2", "--demons_iter", "5", "--demons_sigma", "2")))):
        t = str(tmp_path / f"t{k}.csv")
        got = run(exe, "--refine", *extra, "--transform", t, "--warped", path, s, r)
        assert got.returncode == 0, got.stderr
        dim, body = _nii(path)
        assert dim == (3, 96, 80, 64, 1)
        worst, bound, n = _through_the_written_map(host, t, a, np.frombuffer(body, "<f4").reshape(64, 80, 96).astype(np.float64))
        print(f"run {k}: largest difference from the warp through the written map {worst:.3e}, bound {bound:.3e}, over {n} voxels")
        assert n > 0.9 * a.size and worst <= bound
