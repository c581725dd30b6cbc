"""Similarity scores of a registration (sift3d_amd_im_similarity, s3d_k_similarity_*, s3d_k_minmax_finite) on the CPU: the
kernels and the host entry points run through the SIMT emulator build of the library (tests/emu) against the numpy restatement of
tests/similarity_cases.py, and regSift3D's --metrics options are checked up to the point where an image would be read.  The GPU
counterpart is tests/test_gpu_similarity.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from sift3d_amd import abi, build as _b
from sift3d_amd.device import DeviceLib, bind_extensions
from tests import similarity_cases as sc
from tests import tps_cases as tc
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


def test_struct_layouts():
    assert C.sizeof(abi.Similarity) == 2 * 8 + 12 * 8 and abi.Similarity.mean_ref.offset == 16 and abi.Similarity.nmi.offset == 104
    assert C.sizeof(abi.SimilarityOpts) == 40 and abi.SimilarityOpts.ref_range.offset == 8 and abi.SimilarityOpts.src_range.offset == 24


@pytest.mark.parametrize("bins", sc.BINS)
@pytest.mark.parametrize("shape", list(sc.SHAPES))
def test_affine_linear_histogram_and_sums(emu_dev, shape, bins):
    sc.case_affine_linear(emu_dev, shape, bins)


@pytest.mark.parametrize("shape,bins", [("70x33x9", 64), ("257x19x5", 37)])
def test_aggregated_histogram_update(emu_dev, shape, bins):
    sc.case_aggregated(emu_dev, shape, bins)


@pytest.mark.parametrize("shape,bins", [("70x33x9", 37), ("257x19x5", 128)])
def test_public_entry_statistics(emu, shape, bins, capfd):
    sc.case_api(emu, shape, bins)


def test_kept_voxel_counts(emu, capfd):
    sc.case_counts(emu)


def test_identity(emu, capfd):
    sc.case_identity(emu)


def test_degenerate_volumes(emu, capfd):
    sc.case_degenerate(emu)


@pytest.mark.parametrize("n", [0, 1, tc.TILE + 1])
def test_consistent_with_the_spline_warp(emu, emu_dev, n, capfd):
    sc.case_consistency_tps(emu, emu_dev, n)


def test_consistent_with_the_lanczos_warp(emu, emu_dev, capfd):
    sc.case_consistency_lanczos(emu, emu_dev)


def test_meaning(emu, capfd):
    sc.case_meaning(emu)


def test_refusals(emu, capfd):
    sc.case_refusals(emu)
    capfd.readouterr()


@pytest.mark.parametrize("case", ["plain", "nan", "inf", "negative", "none-finite", "one"])
def test_minmax_finite(emu_dev, case):
    rng = np.random.default_rng(4)
    v = rng.standard_normal(5000).astype(np.float32)
    if case == "nan":
        v[[0, 17, 4999]] = np.nan
    elif case == "inf":
        v[[3, 4]] = [np.inf, -np.inf]
    elif case == "negative":
        v = -np.abs(v) - 1
    elif case == "none-finite":
        v = np.array([np.nan, np.inf, -np.inf] * 100, np.float32)
    elif case == "one":
        v = np.array([np.nan, -0.0, np.inf], np.float32)
    d = emu_dev.upload(v)
    try:
        lo, hi = emu_dev.minmax_finite(d, v.size)
    finally:
        emu_dev.free(d)
    f = v[np.isfinite(v)]
    if f.size == 0:
        assert np.isnan(lo) and np.isnan(hi)
    else:
        assert (lo, hi) == (float(f.min()), float(f.max()))


def test_flat_entry_refuses_bad_arguments(emu_dev):
    ref, src = sc.volumes("70x33x9", clean=True)
    w = sc.want_affine("70x33x9", sc.A_FIXED, 64, clean=True)
    L = emu_dev.L
    assert L.s3d_k_similarity_scratch_bytes(70, 33, 9, 64) > 0
    for bad in ((0, 33, 9, 64), (70, 33, 9, 1), (70, 33, 9, 129)):
        assert L.s3d_k_similarity_scratch_bytes(*bad) == 0
    bufs = [emu_dev.upload(a) for a in (src, ref, np.zeros(128 * 128, np.uint64), np.zeros(7), np.zeros(7 * 2048))]
    A = np.ascontiguousarray(sc.A_FIXED).ctypes.data_as(C.POINTER(C.c_double))
    tail = (w.rr[0], 1.0, w.sr[0], 1.0, w.c[0], w.c[1], bufs[2], bufs[3], bufs[4], None)
    try:
        for sd, rd, interp, bins in (((0, 37, 11), (70, 33, 9), 0, 64), ((61, 37, 11), (70, 0, 9), 0, 64), ((61, 37, 11), (70, 33, 9), 2, 64),
                                     ((61, 37, 11), (70, 33, 9), 0, 1), ((61, 37, 11), (70, 33, 9), 0, 129),
                                     ((61, 37, 11), (70, 65536, 32768), 0, 64)):   # more rows than the grid's 32-bit index holds
            assert L.s3d_k_similarity_affine(bufs[0], *sd, bufs[1], *rd, A, interp, bins, *tail) != 0 and emu_dev.err()
        assert L.s3d_k_similarity_tps(bufs[0], 61, 37, 11, bufs[1], 70, 33, 9, None, None, 0, 0, 64, *tail) != 0 and emu_dev.err()
    finally:
        for b in bufs:
            emu_dev.free(b)


def test_regSift3D_metrics_options():
    """--help shows the new block above "Other options:" and leaves the text below as it was; bad values and --metrics with
    --resample fail with their messages before any image is read (the files do not exist)"""
    _b.build()
    exe = os.path.join(BIN, "regSift3D")
    r = run(exe, "--help")
    assert r.returncode == 0
    head, tail = r.stdout.split("Other options:")
    assert "Similarity options:" in head and "--metrics [filename]" in head and "--metric_bins [value]" in head
    assert head.index("Thin-plate-spline options:") < head.index("Similarity options:")
    assert "--metric" not in tail and tail.lstrip().startswith("--nn_thresh [value]")
    ref_exe = os.path.join(sc.ROOT, "oracle", "_ref", "bin", "regSift3D")
    if os.path.exists(ref_exe):
        assert tail == run(ref_exe, "--help").stdout.split("Other options:")[1]
    for args, msg in ((["--metric_bins", "1", "--metrics", "m.csv", "a", "b"], "Invalid value for metric_bins."),
                      (["--metric_bins", "129", "--metrics", "m.csv", "a", "b"], "Invalid value for metric_bins."),
                      (["--metrics", "m.csv", "--resample", "a", "b"], "--metrics cannot be combined with --resample.")):
        r = run(exe, *args)
        assert r.returncode == 1 and msg in r.stderr and "Failed to read" not in r.stderr, (args, r.stderr)
    r = run(exe, "--metrics", "m.csv", "a")                             # --metrics alone is an output
    assert r.returncode == 1 and "Not enough arguments." in r.stderr
