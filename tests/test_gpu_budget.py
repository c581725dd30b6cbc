"""GPU: a keypoint budget through the product library on an MI355X -- the bodies of tests/test_budget.py on the device, the
selection kernel at the multi-workgroup size the compaction tests use, and a 256^3 volume with a budget of 2 000."""
import numpy as np
import pytest

from sift3d_amd import synth
from tests import test_budget as B

pytestmark = pytest.mark.gpu


# ---- 1: the selection kernel ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", B.PATTERNS)
@pytest.mark.parametrize("num", B.SELECT_SIZES + [70001])
def test_select_strongest_against_numpy(hip, num, pattern):
    B.check_select(hip, num, pattern, gpu=True)


def test_select_strongest_arguments(hip):
    B.check_select_arguments(hip)


# ---- 2, 3: strengths, budgeted detect == filtered unbudgeted detect -----------------------------------------------------------------
@pytest.mark.parametrize("i", range(5))
def test_strengths_are_the_oracles_dog(hip, oracle, i):
    B.check_strengths(hip, oracle, i)


@pytest.mark.parametrize("which", B.BUDGETS)
@pytest.mark.parametrize("i", range(5))
def test_budgeted_detect_is_the_filtered_unbudgeted_detect(hip, oracle, i, which):
    B.check_volume_budget(hip, oracle, i, which)


def test_selection_spans_orientation_chunks(hip, oracle):
    B.check_volume_budget(hip, oracle, 2, "7", orient_chunk=16)


# ---- 4, 5, 6, 7 ---------------------------------------------------------------------------------------------------------------------
def test_mask_then_budget(hip, oracle):
    B.check_mask_plus_budget(hip, oracle)


def test_typed_input_plus_budget(hip):
    B.check_typed_plus_budget(hip)


def test_nonfinite_volume_with_a_budget(hip, oracle):
    B.check_nonfinite_budget(hip, oracle, *B.NONFINITE)


def test_lifecycle(hip):
    B.check_lifecycle(hip)


def test_two_loopback_ranks_refuse_a_budget(hip):
    B.check_loopback_ranks(hip)


# ---- 8: the command line ------------------------------------------------------------------------------------------------------------
def test_kpSift3D_max_keypoints(tmp_path, oracle):
    B.check_cli(tmp_path, None, oracle, (96, 80, 64), 900, 5)


# ---- 9: a volume of a size users run ------------------------------------------------------------------------------------------------
def test_256_cubed_budget_2000(hip, oracle):
    """256^3, budget 2 000: the budgeted run against the product's own unbudgeted run restricted by numpy (records, every GSS
    level, descriptors bit for bit) and against the oracle's list restricted by the oracle's own DoG."""
    n = 2000
    vol = synth.blobs(256, 256, 256, synth.default_nblobs(256, 256, 256), 0)
    base = B.run(hip, vol, B.UNIT)
    w_xyzos, w_sd, w_R = oracle.detect(vol, B.UNIT)
    w_strength = B.oracle_strengths(oracle, w_xyzos)
    assert 0 < n < len(w_xyzos) - 100
    assert np.array_equal(base["xyzos"], w_xyzos) and base["strength"].tobytes() == w_strength.tobytes()
    keep = B.top_n(w_strength, n)
    assert int(keep.sum()) == n and len(np.unique(w_xyzos[keep, 3])) > 1
    got = B.run(hip, vol, B.UNIT, n)
    B.assert_is_filtered(got, base, keep, "256^3 budget 2000")
    assert np.array_equal(got["xyzos"], w_xyzos[keep]) and np.array_equal(got["sd"], w_sd[keep])
    assert np.abs(got["R"] - w_R[keep]).max(initial=0) <= 1e-5
