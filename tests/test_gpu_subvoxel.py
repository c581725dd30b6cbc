"""GPU: sub-voxel keypoints through the product library on an MI355X -- the bodies of tests/test_subvoxel.py on the device (the
kernel's buffers and the oracle's pyramid levels go through HBM), and a 128^3 volume whose list spans many workgroups."""
import numpy as np
import pytest

from sift3d_amd import synth
from tests import test_subvoxel as S

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def no_environment_switch(monkeypatch):
    monkeypatch.delenv("SIFT3D_SUBVOXEL", raising=False)


# ---- 1, 2: the kernel ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("length", S.LENGTHS)
@pytest.mark.parametrize("i", range(5))
def test_kernel_against_the_restatement(hip, oracle, i, length):
    S.check_kernel(hip, oracle, i, length, gpu=True)


def test_records_that_cannot_be_refined(hip, oracle):
    S.check_unrefinable(hip, oracle, gpu=True)


def test_isolated_blobs(hip, oracle):
    S.check_isolated_blobs(hip, oracle, gpu=True)


# ---- 3: the contract -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(5))
def test_refined_detect_is_the_integer_detect_moved(hip, oracle, i):
    S.check_contract(hip, oracle, i)


def test_mask_and_budget_compose(hip, oracle):
    S.check_with_mask_and_budget(hip, oracle)


def test_lifecycle(hip, oracle, monkeypatch):
    S.check_lifecycle(hip, oracle, monkeypatch)


def test_two_loopback_ranks_refuse_refinement(hip):
    S.check_loopback_ranks(hip)


# ---- 4, 5, 6 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", [1, 3, 4])
def test_descriptors_at_refined_keys(hip, oracle, i):
    S.check_describe(hip, oracle, i)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_shift_recovery(hip, oracle, seed):
    S.check_shift_recovery(hip, oracle, seed)


def test_kpSift3D_subvoxel(hip, tmp_path, oracle):
    S.check_cli(hip, tmp_path, None, oracle)


# ---- 7: a list of many workgroups -------------------------------------------------------------------------------------------------------
def test_128_cubed(hip, oracle):
    """128^3: several hundred keypoints behind more than twice as many candidates (the grid's bound), the kernel launched by the
    detect on the count the compaction left on the device."""
    vol = synth.blobs(128, 128, 128, synth.default_nblobs(128, 128, 128), 0)
    st = S.snapshot(oracle, vol, S.UNIT, key=("128",))
    K = len(st["xyzos"])
    assert K > 300 and len(st["cands"]) > 2 * K
    ok = S.usable(st, st["xyzos"])
    base = S.run(hip, vol, S.UNIT, subvoxel=False)
    S.assert_integer_list(base, st, what="128^3 off")
    got = S.run(hip, vol, S.UNIT, subvoxel=True)
    # (records the condition on the inputs excludes are compared in everything but their position)
    sel = dict(got, xyz=got["xyz"][ok], o=got["o"][ok], s=got["s"][ok], sd=got["sd"][ok], R=got["R"][ok])
    off, flags = S.assert_refined_list(dict(sel, counts=_counts(st, ok)), None, st, ok, "128^3 on")
    w_flags = S.restate(st, st["xyzos"])[1]
    assert got["counts"] == (int((w_flags == 1).sum()), int((w_flags == 2).sum())) and sum(got["counts"]) == K
    assert got["R"].tobytes() == base["R"].tobytes() and np.array_equal(got["o"], base["o"]) and np.array_equal(got["s"], base["s"])
    assert np.abs(got["xyz"] - base["xyz"]).max() <= 0.5


def _counts(st, ok):
    f = S.restate(st, st["xyzos"][ok])[1]
    return int((f == 1).sum()), int((f == 2).sum())
