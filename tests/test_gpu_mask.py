"""GPU: keypoints inside a region of interest only, through the product library on an MI355X -- the bodies of
tests/test_mask.py on the device (host form and device-resident form of the mask), a 256^3 volume, and two loop-back Z-slab
ranks whose gathered list is filtered on the host."""
import ctypes as C

import numpy as np
import pytest

from sift3d_amd import synth
from tests import test_mask as M
from tests import test_typed_input as T

pytestmark = pytest.mark.gpu
FORMS = ["host", "device"]


# ---- 1, 2: the kernels ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", M.PACK_DIMS + [(130, 128, 96)])
def test_mask_pack_against_packbits(hip, dims):
    M.check_mask_pack(hip, dims, gpu=True)


def test_mask_pack_of_a_mask_that_is_not_16_byte_aligned(hip):
    M.check_mask_pack(hip, (21, 19, 17), gpu=True, misalign=3)


@pytest.mark.parametrize("nseg,nwords", [(1, 1), (1, 1500), (3, 1500), (3, 2049), (3, 1), (3, 70001)])
def test_compact_bits_multi_and_against_numpy(hip, nseg, nwords):
    M.check_compact_and(hip, nseg, nwords, gpu=True)


# ---- 3, 4: masked detect == filtered unmasked detect ------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", M.MASK_NAMES)
@pytest.mark.parametrize("i", range(len(T.VOLUMES)))
def test_masked_detect_is_the_filtered_unmasked_detect(hip, oracle, i, name, form):
    M.check_volume_mask(hip, oracle, i, name, form)


def test_octave_mapping(hip, oracle):
    M.check_octave_mapping(hip, oracle)


# ---- 5, 6, 7 --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
def test_lifecycle(hip, form):
    M.check_lifecycle(hip, form)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("i", [2, 3], ids=["fused_route", "conversion_route"])
def test_typed_input_plus_mask(hip, i, form):
    M.check_typed_plus_mask(hip, i, form)


@pytest.mark.parametrize("base,name", M.REFERENCE_FAILS)
def test_masked_background_stops_being_fatal(hip, base, name):
    M.check_nonfinite_fatal_case(hip, base, name)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("base,name,mask_name,total,n_kept", M.NONFINITE_MASKED)
def test_nonfinite_volumes_with_a_mask(hip, base, name, mask_name, total, n_kept, form):
    M.check_nonfinite_masked_case(hip, base, name, mask_name, total, n_kept, form)


# ---- a volume of a size users run -----------------------------------------------------------------------------------------------
def test_256_cubed_ball(hip, oracle):
    """256^3, `ball`: the masked run against the product's own unmasked run filtered (records, every GSS level, descriptors bit
    for bit) and against the oracle's list filtered."""
    vol = synth.blobs(256, 256, 256, synth.default_nblobs(256, 256, 256), 0)
    mask = M.make_mask("ball", vol.shape)
    base = M.run(hip, vol, M.UNIT)
    w_xyzos, w_sd, w_R = oracle.detect(vol, M.UNIT)
    cand = oracle.candidates()[0]
    wk = M.kept(w_xyzos, mask)
    for form in FORMS:
        got = M.run(hip, vol, M.UNIT, mask, form)
        keep = M.assert_masked_is_filtered(got, base, mask, f"256^3 ball, {form} form")
        assert 100 < int(keep.sum()) < len(keep) - 100
        assert np.array_equal(got["xyzos"], w_xyzos[wk]) and np.array_equal(got["sd"], w_sd[wk])
        assert np.abs(got["R"] - w_R[wk]).max(initial=0) <= 1e-5
        assert got["ncand"] == int(M.kept(cand, mask).sum())
    assert base["ncand"] == len(cand)


# ---- several GPUs ------------------------------------------------------------------------------------------------------------
def test_two_loopback_ranks_with_a_mask(hip):
    M.check_loopback_ranks(hip)


# ---- 8: the command line ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mask_dtype", [np.uint8, np.int16])
def test_kpSift3D_mask(tmp_path, mask_dtype):
    M.check_cli(tmp_path, None, (96, 80, 64), 900, 5, mask_dtype)
