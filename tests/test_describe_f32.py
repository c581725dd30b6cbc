"""CPU, emulator: the f32 / f64 forms of the descriptor kernel's back end (tests/describe_f32.py) on the volume the
emulator's redo test uses, blobs(40, 36, 32, 120, seed 4) with unit voxels."""
import ctypes as C
import os
import subprocess

import pytest

from sift3d_amd import abi, synth
from sift3d_amd.device import bind_extensions
from tests import describe_f32 as df

EMU_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu")
DIMS, NBLOBS, SEED = (40, 36, 32), 120, 4


@pytest.fixture(scope="module")
def emu():
    subprocess.run(["sh", os.path.join(EMU_DIR, "build_emu.sh")], check=True, capture_output=True)
    L = C.CDLL(os.path.join(EMU_DIR, "libsift3d_emu.so"))
    lib = abi.Sift3dLib(L, None, "emulated")
    bind_extensions(L)
    return lib


@pytest.fixture(scope="module")
def plain(emu, oracle):
    sc = df.Scene(emu, oracle, synth.blobs(*DIMS, NBLOBS, SEED), (1, 1, 1))
    yield sc
    sc.close()


def test_path_independence_bitwise(plain):
    """f32 limit x 1, 2^-6, 2^-10 and 0 (every voxel through the f64 form): byte-identical descriptors; 2^-6 mixes the
    two forms inside the windows of this volume."""
    df.check_path_independence(plain)


@pytest.mark.parametrize("est_factor", [1.0, 1e-3, 64.0])
def test_oracle_parity_mixed_path(plain, est_factor):
    """Both forms inside one window, on the estimated grid, on one a thousand times too fine and on one 64 times too
    coarse (both redone by every window): the oracle's descriptors within the contract."""
    df.check_mixed_path_parity(plain, est_factor)


def test_outliers_at_product_setting(emu, oracle):
    """Three voxels at 50 x the volume's maximum: their neighbourhoods exceed 2^24 grid units and take the f64 form at
    the product's limit; detection and descriptors stay the oracle's."""
    vol, spots = df.outlier_volume(synth.blobs(*DIMS, NBLOBS, SEED))
    sc = df.Scene(emu, oracle, vol, (1, 1, 1))
    try:
        df.check_outliers(sc, spots)
    finally:
        sc.close()


def test_slow_path_share(plain):
    """At most one voxel in a thousand may need the f64 form on a plain volume: one such lane sends its whole wave
    through the f64 block.  (0 of 234 175 here with DW_GRID_K = 2; 2.7e-3 with K = 1.)"""
    df.check_slow_share(plain)


def test_error_headroom(plain, emu, oracle):
    """Worst |got - want| / (1e-4 |want| + 1e-7) over this volume and the anisotropic one of the emulator's parity tests:
    at most 0.25 of the band (a 512^3 run has ~70 x as many keypoints and a longer tail).  Measured, iso / aniso, for the
    grid DW_GRID_K times coarser than the 32-bit fields could take: K = 16: 0.809 / 0.841, K = 8: 0.421 / 0.412,
    K = 4: 0.255 / 0.185, K = 2 (the kernel's): 0.137 / 0.079, K = 1: 0.064 / 0.044 (0.096 before the f32 products)."""
    r_iso = df.error_ratio(plain.describe(1.0)["bins"], plain.want)
    sc = df.Scene(emu, oracle, synth.blobs(36, 32, 28, 60, 3), (1, 0.8, 2))
    try:
        r_aniso = df.error_ratio(sc.describe(1.0)["bins"], sc.want)
    finally:
        sc.close()
    print(f"worst error ratio: iso {r_iso:.4f}, aniso {r_aniso:.4f}")
    assert max(r_iso, r_aniso) <= 0.25, (r_iso, r_aniso)
