"""CPU: keypoints inside a region of interest only (sift3d_amd_set_mask, s3d_k_mask_pack, s3d_k_compact_bits_multi_and).

The product's sources run on the SIMT emulator (tests/emu).  The contract every test here uses: the masked detect returns
exactly the unmasked keypoint list with the masked-out records deleted -- a keypoint of octave o at octave coordinates
(x, y, z) is kept iff mask[z << o, y << o, x << o] != 0 -- byte for byte and in the same order, on a pyramid that is bit for bit
the unmasked one; the descriptors of the survivors are those of the unmasked run.  tests/test_gpu_mask.py runs the same
bodies on the device (`gpu=True`: buffers go through HBM)."""
import ctypes as C
import gzip
import os
import subprocess

import numpy as np
import pytest

from sift3d_amd import abi, synth
from sift3d_amd.device import DeviceLib, bind_extensions
from tests import parity
from tests import test_typed_input as T
from tests.test_host_io import nifti1_bytes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")
P = C.POINTER
UNIT = (1.0, 1.0, 1.0)

# The oracle's counts for T.VOLUMES: total, then kept under half_x / ball / rand50 (no case is vacuous)
COUNTS = [(21, 11, 3, 7), (15, 8, 5, 6), (41, 25, 14, 21), (42, 22, 13, 25), (47, 17, 17, 24)]
MASK_NAMES = ("half_x", "ball", "rand50")


@pytest.fixture(scope="module")
def emu():
    subprocess.run(["sh", os.path.join(EMU_DIR, "build_emu.sh")], check=True, capture_output=True)
    L = C.CDLL(os.path.join(EMU_DIR, "libsift3d_emu.so"))
    lib = abi.Sift3dLib(L, None, "emulated")
    bind_extensions(L)
    return lib


# ---- helpers (shared with the GPU file) ------------------------------------------------------------------------------------
def make_mask(name, shape):
    """uint8 [nz, ny, nx]; inside = 1."""
    nz, ny, nx = shape
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    if name == "half_x":
        m = x < nx // 2
    elif name == "half_z":
        m = z < nz // 2
    elif name == "ball":
        m = (x - nx // 2) ** 2 + (y - ny // 2) ** 2 + (z - nz // 2) ** 2 <= (0.35 * min(shape)) ** 2
    elif name == "rand50":
        m = np.random.default_rng(7).random(shape) < 0.5
    elif name == "even":
        m = (x % 2 == 0) & (y % 2 == 0) & (z % 2 == 0)
    elif name == "odd":
        m = ~((x % 2 == 0) & (y % 2 == 0) & (z % 2 == 0))
    elif name == "ones":
        m = np.ones(shape, bool)
    elif name == "zeros":
        m = np.zeros(shape, bool)
    else:
        raise KeyError(name)
    return np.ascontiguousarray(m.astype(np.uint8))


def kept(xyzos, mask):
    """The rule: which rows of an x, y, z, o, s list survive `mask` [nz, ny, nx]."""
    c = np.asarray(xyzos, np.int64).reshape(-1, 5)
    o = c[:, 3]
    return mask[c[:, 2] << o, c[:, 1] << o, c[:, 0] << o] != 0


def record_rows(kp):
    """One row of bytes per keypoint record, without the pointer it holds and the padding in front of it (T.key_records)."""
    k = int(kp.slab.num)
    raw = np.ctypeslib.as_array(C.cast(kp.buf, P(C.c_uint8)), shape=(k, C.sizeof(abi.Keypoint))).copy() if k else \
        np.zeros((0, C.sizeof(abi.Keypoint)), np.uint8)
    off = abi.Keypoint.R.offset
    return np.concatenate([raw[:, :abi.Keypoint.r_data.size], raw[:, off + 8:]], axis=1)


def set_mask(lib, s, mask, form="host"):
    """Host form, or the device-resident form: the mask lies in HBM, is read in place and is free again after the call."""
    if form == "host" or mask is None:
        rc = abi.set_mask(lib.sift, s, mask)
    else:
        dev = DeviceLib(lib.sift)
        d_m = dev.upload(mask)
        try:
            rc = abi.set_mask(lib.sift, s, d_m, shape=mask.shape)
        finally:
            dev.free(d_m)
    return rc


def descriptors(lib, s, kp):
    d = abi.SIFT3D_Descriptor_store()
    lib.sift.init_SIFT3D_Descriptor_store(C.byref(d))
    assert lib.sift.SIFT3D_extract_descriptors(C.byref(s), C.byref(kp), C.byref(d)) == 0
    bins, xyzs = lib.descriptors_to_numpy(d)
    lib.sift.cleanup_SIFT3D_Descriptor_store(C.byref(d))
    return bins, xyzs


def run(lib, vol, units, mask=None, form="host", params=None, describe=True, levels=True):
    """One detect (+ describe) on a fresh struct: dict of record rows, xyzos / sd / R, candidate count, GSS level bytes and
    descriptor bins."""
    s = T.new_sift(lib)
    for k, v in (params or {}).items():
        assert getattr(lib.sift, f"set_{k}_SIFT3D")(C.byref(s), v) == 0
    if mask is not None:
        assert set_mask(lib, s, mask, form) == 0, lib.sift.sift3d_amd_last_error()
    assert lib.sift.sift3d_amd_have_mask(C.byref(s)) == (mask is not None)
    kp = T.float_detect(lib, s, vol, units)
    xyzos, sd, R = lib.keypoints_to_numpy(kp)
    out = dict(rows=record_rows(kp), xyzos=xyzos, sd=sd, R=R, ncand=lib.sift.sift3d_amd_last_num_candidates(C.byref(s)),
               dims=(kp.nx, kp.ny, kp.nz))
    if levels:
        out["gss"] = T.gss_bytes(lib, s)
    if describe:
        out["bins"], out["xyzs"] = descriptors(lib, s, kp) if len(xyzos) else (np.zeros((0, 768), np.float32), np.zeros((0, 4)))
    lib.sift.cleanup_Keypoint_store(C.byref(kp))
    lib.sift.cleanup_SIFT3D(C.byref(s))
    return out


def assert_masked_is_filtered(got, base, mask, what=""):
    """`got` (masked run) against `base` (unmasked run of the same library): records, pyramid, descriptors.  Returns the
    boolean selection."""
    keep = kept(base["xyzos"], mask)
    assert len(got["rows"]) == int(keep.sum()), f"{what}: {len(got['rows'])} keypoints, the filtered list has {int(keep.sum())}"
    assert got["rows"].tobytes() == base["rows"][keep].tobytes(), f"{what}: keypoint records differ"
    assert got["dims"] == base["dims"]
    if "gss" in got and "gss" in base:
        assert len(got["gss"]) == len(base["gss"])
        for i, (a, b) in enumerate(zip(got["gss"], base["gss"])):
            assert a == b, f"{what}: GSS level {i} differs from the unmasked run's"
    if "bins" in got and "bins" in base:
        # bit-equal: the descriptor of a keypoint is a function of its record and the pyramid alone (an order-free fixed-point
        # histogram per keypoint), not of which other keypoints share the launch
        assert got["bins"].tobytes() == base["bins"][keep].tobytes(), f"{what}: descriptors differ from the unmasked run's rows"
        assert np.array_equal(got["xyzs"], base["xyzs"][keep])
    return keep


_unmasked = {}


def unmasked(lib, oracle, i):
    """The unmasked run of T.VOLUMES[i] on `lib` and the oracle's answer, once per library."""
    key = (lib.name, i)
    if key not in _unmasked:
        dims, units, nblobs, seed, _ = T.VOLUMES[i]
        vol = synth.blobs(*dims, nblobs, seed)
        want = oracle.detect(vol, units)
        cand = oracle.candidates()[0].copy()
        _unmasked[key] = (vol, units, run(lib, vol, units), want, cand)
    return _unmasked[key]


def check_volume_mask(lib, oracle, i, name, form="host"):
    vol, units, base, (w_xyzos, w_sd, w_R), cand = unmasked(lib, oracle, i)
    mask = make_mask(name, vol.shape)
    got = run(lib, vol, units, mask, form)
    keep = assert_masked_is_filtered(got, base, mask, f"{T.VOLUMES[i][0]} {name}")
    wk = kept(w_xyzos, mask)
    total, want_kept = COUNTS[i][0], COUNTS[i][1 + MASK_NAMES.index(name)]
    assert len(w_xyzos) == total and int(wk.sum()) == want_kept, "the oracle's counts moved"
    assert 0 < int(keep.sum()) < len(keep), "the mask must keep a keypoint and remove one"
    assert np.array_equal(got["xyzos"], w_xyzos[wk]) and np.array_equal(got["sd"], w_sd[wk])
    assert np.abs(got["R"] - w_R[wk]).max(initial=0) <= 1e-5          # parity.check_detect_describe's bound
    assert got["ncand"] == int(kept(cand, mask).sum()), "candidates are counted after masking"
    assert base["ncand"] == len(cand)
    return int(keep.sum())


# ---- 1: s3d_k_mask_pack ---------------------------------------------------------------------------------------------------
def octave_dims(lib, dims, shifts=4):
    """(onx, ony, onz) per shift from a planned pyramid; shifts past its last octave halve on as the pyramid would."""
    s = T.new_sift(lib)
    lib.sift.sift3d_amd_plan.argtypes = [P(abi.SIFT3D), C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double]
    assert lib.sift.sift3d_amd_plan(C.byref(s), *dims, 1.0, 1.0, 1.0) == 0
    out = []
    for o in range(s.gpyr.num_octaves):
        lv = s.gpyr.levels[o * s.gpyr.num_levels]
        out.append((lv.nx, lv.ny, lv.nz))
    lib.sift.cleanup_SIFT3D(C.byref(s))
    assert out[0] == tuple(dims)
    while len(out) < shifts:
        out.append(tuple(d // 2 for d in out[-1]))
    return out[:shifts]


def packed(mask, odims, shift):
    onx, ony, onz = odims
    sub = mask[::1 << shift, ::1 << shift, ::1 << shift][:onz, :ony, :onx]
    assert sub.shape == (onz, ony, onx)
    nwords = (onx * ony * onz + 63) // 64
    b = np.packbits(sub.ravel() != 0, bitorder="little")
    return np.concatenate([b, np.zeros(nwords * 8 - len(b), np.uint8)]).view(np.uint64)


def check_mask_pack(lib, dims, gpu, misalign=0):
    dev = DeviceLib(lib.sift)
    nx, ny, nz = dims
    rng = np.random.default_rng(nx * 1000 + ny)
    mask = rng.choice(np.array([0, 1, 2, 128, 255], np.uint8), size=(nz, ny, nx), p=[0.5, 0.125, 0.125, 0.125, 0.125])
    buf = np.zeros(mask.size + 32, np.uint8)
    if not gpu:                                           # start on a 16-byte boundary (device allocations do), plus `misalign`
        misalign += -buf.ctypes.data % 16
    buf[misalign:misalign + mask.size] = mask.ravel()
    d_buf = dev.upload(buf) if gpu else buf.ctypes.data
    for shift, od in enumerate(octave_dims(lib, dims)):
        want = packed(mask, od, shift)
        got = np.full(len(want) + 1, 0xFFFFFFFFFFFFFFFF, np.uint64)      # ones: an unwritten word or a non-zero tail shows
        d_bits = dev.upload(got) if gpu else got.ctypes.data
        dev.mask_pack(d_buf + misalign, nx, ny, od, shift, d_bits)
        dev.sync()
        if gpu:
            got = dev.download(d_bits, got.shape, np.uint64)
            dev.free(d_bits)
        assert got[-1] == 0xFFFFFFFFFFFFFFFF, "wrote past the last word"
        assert np.array_equal(got[:-1], want), (dims, shift, misalign)
    if gpu:
        dev.free(d_buf)


PACK_DIMS = [(21, 19, 17), (64, 40, 36), (66, 64, 64), (23, 9, 11)]       # 21*19*17 % 64 = 63, 23*9*11 % 64 = 37


@pytest.mark.parametrize("dims", PACK_DIMS)
def test_mask_pack_against_packbits(emu, dims):
    check_mask_pack(emu, dims, gpu=False)


def test_mask_pack_of_a_mask_that_is_not_16_byte_aligned(emu):
    check_mask_pack(emu, (21, 19, 17), gpu=False, misalign=3)


# ---- 2: s3d_k_compact_bits_multi_and -----------------------------------------------------------------------------------------
def check_compact_and(lib, nseg, nwords, gpu, seed=0):
    dev = DeviceLib(lib.sift)
    rng = np.random.default_rng(seed + nseg * 100003 + nwords)
    stride = nwords + 5
    bits = np.zeros(nseg * stride, np.uint64)
    for s in range(nseg):
        b = rng.random(nwords * 64) < 0.03
        bits[s * stride:s * stride + nwords] = np.packbits(b, bitorder="little").view(np.uint64)
        bits[s * stride + nwords:(s + 1) * stride] = 0xFFFFFFFFFFFFFFFF          # the gap between segments is not read
    band = np.packbits(rng.random(nwords * 64) < 0.5, bitorder="little").view(np.uint64)
    base, tag0, start = 1000, (2 << 8) | 1, 5

    def expect(use_and):
        idx, tag = [], []
        for s in range(nseg):
            w = bits[s * stride:s * stride + nwords]
            if use_and:
                w = w & band
            on = np.flatnonzero(np.unpackbits(w.view(np.uint8), bitorder="little"))
            idx.append(on + base)
            tag.append(np.full(len(on), tag0 + s))
        return np.concatenate(idx).astype(np.uint32), np.concatenate(tag).astype(np.uint32)

    def call(which):
        want_idx, want_tag = expect(which == "and")
        cap = start + len(want_idx) + 7
        idx = np.full(cap, 0xDEADBEEF, np.uint32)
        tag = np.full(cap, 0xDEADBEEF, np.uint32)
        count = np.array([start], np.uint32)
        scratch = np.zeros(nseg * ((nwords + 1023) // 1024) + 8, np.uint32)
        arrs = [bits, band, idx, tag, count, scratch]
        ptr = [dev.upload(a) for a in arrs] if gpu else [a.ctypes.data for a in arrs]
        if which == "plain":
            rc = dev.L.s3d_k_compact_bits_multi(ptr[0], nwords, nseg, stride, base, ptr[2], ptr[3], tag0, cap, ptr[4], ptr[5],
                                                None)
            assert rc == 0
        else:
            dev.compact_bits_multi_and(ptr[0], nwords, nseg, stride, base, ptr[2], ptr[3], tag0, cap, ptr[4], ptr[5],
                                       ptr[1] if which == "and" else None)
        dev.sync()
        if gpu:
            idx, tag, count = (dev.download(ptr[k], arrs[k].shape, np.uint32) for k in (2, 3, 4))
            for p in ptr:
                dev.free(p)
        assert int(count[0]) == start + len(want_idx), "the count advances by the (masked) population"
        assert np.array_equal(idx[start:start + len(want_idx)], want_idx) and np.array_equal(tag[start:start + len(want_idx)], want_tag)
        assert (idx[:start] == 0xDEADBEEF).all() and (idx[start + len(want_idx):] == 0xDEADBEEF).all()
        return idx.tobytes() + tag.tobytes() + count.tobytes()

    masked = call("and")
    null = call("null")
    assert null == call("plain"), "d_and = NULL is s3d_k_compact_bits_multi"
    assert masked != null


@pytest.mark.parametrize("nseg,nwords", [(1, 1), (1, 1500), (3, 1500), (3, 2049), (3, 1)])
def test_compact_bits_multi_and_against_numpy(emu, nseg, nwords):
    check_compact_and(emu, nseg, nwords, gpu=False)


# ---- 3: masked detect == filtered unmasked detect ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MASK_NAMES)
@pytest.mark.parametrize("i", range(len(T.VOLUMES)))
def test_masked_detect_is_the_filtered_unmasked_detect(emu, oracle, i, name):
    check_volume_mask(emu, oracle, i, name)


# ---- 4: the octave mapping ---------------------------------------------------------------------------------------------------
def check_octave_mapping(lib, oracle):
    vol, units, base, (w_xyzos, _, _), _ = unmasked(lib, oracle, 2)            # (68, 64, 62) seed 1
    o = base["xyzos"][:, 3]
    assert np.array_equal(base["xyzos"], w_xyzos) and int((o >= 1).sum()) == 23
    odd = run(lib, vol, units, make_mask("odd", vol.shape), describe=False, levels=False)
    assert_masked_is_filtered(odd, base, make_mask("odd", vol.shape), "odd")
    assert len(odd["xyzos"]) == 15 and (odd["xyzos"][:, 3] == 0).all()        # octaves >= 1 sit on even voxels of the input
    even = run(lib, vol, units, make_mask("even", vol.shape), describe=False, levels=False)
    assert_masked_is_filtered(even, base, make_mask("even", vol.shape), "even")
    eo = even["xyzos"][:, 3]
    assert int((eo >= 1).sum()) == 23
    assert int((eo == 0).sum()) == int(((o == 0) & (base["xyzos"][:, :3] % 2 == 0).all(axis=1)).sum())
    assert len(even["xyzos"]) + len(odd["xyzos"]) == len(base["xyzos"])


def test_octave_mapping(emu, oracle):
    check_octave_mapping(emu, oracle)


# ---- 5: lifecycle --------------------------------------------------------------------------------------------------------------
def check_lifecycle(lib, form="host"):
    L = lib.sift
    dims = (48, 48, 48)
    vol = synth.blobs(*dims, 120, 0)
    base = run(lib, vol, UNIT, levels=False)
    half = make_mask("half_x", vol.shape)
    keep = kept(base["xyzos"], half)
    assert 0 < keep.sum() < len(keep)

    def detect(s, v=vol):
        im = lib.image_from_numpy(v, UNIT)
        kp = T.new_kp(lib)
        rc = L.SIFT3D_detect_keypoints(C.byref(s), C.byref(im), C.byref(kp))
        rows = record_rows(kp) if rc == 0 else None
        lib.free_image(im)
        return rc, rows, kp

    s = T.new_sift(lib)
    assert L.sift3d_amd_have_mask(C.byref(s)) == 0
    # all ones: the unmasked records
    assert set_mask(lib, s, make_mask("ones", vol.shape), form) == 0 and L.sift3d_amd_have_mask(C.byref(s)) == 1
    rc, rows, kp = detect(s)
    assert rc == 0 and rows.tobytes() == base["rows"].tobytes()
    L.cleanup_Keypoint_store(C.byref(kp))
    # all zeros: success, no keypoints, and the descriptor call on the empty store does what it does without a mask
    s0 = T.new_sift(lib)
    rc, rows, kp0 = detect(s0, np.zeros_like(vol))                             # an unmasked detect that finds nothing
    assert rc == 0 and len(rows) == 0
    d0 = abi.SIFT3D_Descriptor_store()
    L.init_SIFT3D_Descriptor_store(C.byref(d0))
    want_rc = L.SIFT3D_extract_descriptors(C.byref(s0), C.byref(kp0), C.byref(d0))
    assert set_mask(lib, s, make_mask("zeros", vol.shape), form) == 0
    rc, rows, kp = detect(s)
    assert rc == 0 and len(rows) == 0 and L.sift3d_amd_last_num_candidates(C.byref(s)) == 0
    d = abi.SIFT3D_Descriptor_store()
    L.init_SIFT3D_Descriptor_store(C.byref(d))
    assert L.SIFT3D_extract_descriptors(C.byref(s), C.byref(kp), C.byref(d)) == want_rc
    assert int(d.num) == int(d0.num) == 0
    for st in (d, d0):
        L.cleanup_SIFT3D_Descriptor_store(C.byref(st))
    L.cleanup_Keypoint_store(C.byref(kp))
    L.cleanup_Keypoint_store(C.byref(kp0))
    L.cleanup_SIFT3D(C.byref(s0))
    # a mask stays in force: two detects
    assert set_mask(lib, s, half, form) == 0
    for _ in range(2):
        rc, rows, kp = detect(s)
        assert rc == 0 and rows.tobytes() == base["rows"][keep].tobytes()
        L.cleanup_Keypoint_store(C.byref(kp))
    # bad nx: failure, the mask that was set stays
    assert L.sift3d_amd_set_mask(C.byref(s), C.c_void_p(half.ctypes.data), 0, 0, 48, 48) != 0
    assert L.sift3d_amd_last_error()
    assert L.sift3d_amd_set_mask(C.byref(s), C.c_void_p(half.ctypes.data), 0, 48, -1, 48) != 0
    assert L.sift3d_amd_set_mask(C.byref(s), C.c_void_p(half.ctypes.data), 0, 4, 48, 48) != 0      # too small for a detect
    assert L.sift3d_amd_have_mask(C.byref(s)) == 1
    rc, rows, kp = detect(s)
    assert rc == 0 and rows.tobytes() == base["rows"][keep].tobytes()
    L.cleanup_Keypoint_store(C.byref(kp))
    # copy_SIFT3D carries it
    L.copy_SIFT3D.argtypes = [P(abi.SIFT3D), P(abi.SIFT3D)]
    s2 = T.new_sift(lib)
    assert L.copy_SIFT3D(C.byref(s), C.byref(s2)) == 0 and L.sift3d_amd_have_mask(C.byref(s2)) == 1
    rc, rows, kp = detect(s2)
    assert rc == 0 and rows.tobytes() == base["rows"][keep].tobytes()
    L.cleanup_Keypoint_store(C.byref(kp))
    # ... as a copy: clearing the copy's leaves the source's
    assert set_mask(lib, s2, None) == 0 and L.sift3d_amd_have_mask(C.byref(s2)) == 0 and L.sift3d_amd_have_mask(C.byref(s)) == 1
    L.cleanup_SIFT3D(C.byref(s2))
    # a volume of other dimensions fails, naming both, until the mask is reset or cleared
    other = synth.blobs(40, 48, 48, 100, 1)
    rc, _, kp = detect(s, other)
    msg = L.sift3d_amd_last_error().decode()
    assert rc != 0 and "40 x 48 x 48" in msg and "48 x 48 x 48" in msg, msg
    L.cleanup_Keypoint_store(C.byref(kp))
    rc, rows, kp = detect(s)                                                    # the struct still works on the mask's dimensions
    assert rc == 0 and rows.tobytes() == base["rows"][keep].tobytes()
    L.cleanup_Keypoint_store(C.byref(kp))
    obase = run(lib, other, UNIT, describe=False, levels=False)
    omask = make_mask("half_x", other.shape)
    assert set_mask(lib, s, omask, form) == 0                                  # reset to the new dimensions
    rc, rows, kp = detect(s, other)
    assert rc == 0 and rows.tobytes() == obase["rows"][kept(obase["xyzos"], omask)].tobytes()
    L.cleanup_Keypoint_store(C.byref(kp))
    rc, _, kp = detect(s)
    assert rc != 0
    L.cleanup_Keypoint_store(C.byref(kp))
    # NULL restores the unmasked detect
    assert set_mask(lib, s, None) == 0 and L.sift3d_amd_have_mask(C.byref(s)) == 0
    rc, rows, kp = detect(s)
    assert rc == 0 and rows.tobytes() == base["rows"].tobytes()
    L.cleanup_Keypoint_store(C.byref(kp))
    L.cleanup_SIFT3D(C.byref(s))
    # bool arrays and the wrong types
    sb = T.new_sift(lib)
    assert abi.set_mask(L, sb, half.astype(bool)) == 0
    with pytest.raises(TypeError):
        abi.set_mask(L, sb, half.astype(np.int16))
    with pytest.raises(TypeError):
        abi.set_mask(L, sb, 12345)
    L.cleanup_SIFT3D(C.byref(sb))


def test_lifecycle(emu):
    check_lifecycle(emu)


def test_device_resident_mask_form(emu):
    """on_device = 1 (on the emulator device memory is host memory): the same bits as the host form."""
    vol = synth.blobs(48, 48, 48, 120, 0)
    mask = make_mask("ball", vol.shape)
    a = run(emu, vol, UNIT, mask, "host", describe=False, levels=False)
    b = run(emu, vol, UNIT, mask, "device", describe=False, levels=False)
    assert len(a["rows"]) > 0 and a["rows"].tobytes() == b["rows"].tobytes()


# ---- 6: typed input plus mask -----------------------------------------------------------------------------------------------------
def check_typed_plus_mask(lib, i, form="host"):
    dims, units, nblobs, seed, fused = T.VOLUMES[i]
    q = T.quantise(synth.blobs(*dims, nblobs, seed), np.int16)
    slope, inter = 0.01171875, -7.25
    assert T.route_is_fused(lib, q, units) == fused
    vol = T.converted(q, slope, inter)
    mask = make_mask("half_x", vol.shape)
    base = run(lib, vol, units, describe=False)
    want = run(lib, vol, units, mask, form, describe=False)
    keep = assert_masked_is_filtered(want, base, mask, "float + mask")
    assert 0 < keep.sum() < len(keep)
    s = T.new_sift(lib)
    assert set_mask(lib, s, mask, form) == 0
    kp = T.typed_detect(lib, s, q, units, slope, inter)
    assert record_rows(kp).tobytes() == want["rows"].tobytes()
    assert T.gss_bytes(lib, s) == base["gss"]
    lib.sift.cleanup_Keypoint_store(C.byref(kp))
    # other dimensions fail on the typed entry point too
    q2 = T.quantise(synth.blobs(40, 40, 40, 50, 1), np.int16)
    kp = T.new_kp(lib)
    assert abi.detect_keypoints_typed(lib.sift, s, q2, kp, units, slope, inter) != 0
    lib.sift.cleanup_Keypoint_store(C.byref(kp))
    lib.sift.cleanup_SIFT3D(C.byref(s))


@pytest.mark.parametrize("i", [2, 3], ids=["fused_route", "conversion_route"])
def test_typed_input_plus_mask(emu, i):
    check_typed_plus_mask(emu, i)


# ---- 7: non-finite volumes -----------------------------------------------------------------------------------------------------
REFERENCE_FAILS = [("iso48", "nan_first"), ("aniso40", "nan_first"), ("iso72", "nan_center"), ("slab64", "nan_rank0")]
NONFINITE_MASKED = [("iso48", "nan_interior2", "half_x", 7, 6), ("iso48", "nan_interior", "half_z", 7, 3),
                    ("iso72", "nan_far_edge", "half_x", 31, 18)]


def masked_detect_describe_or_fail(lib, vol, units, params, mask, form="host"):
    """parity.detect_describe_or_fail with a mask set first."""
    L = lib.sift
    s = T.new_sift(lib)
    for k, v in (params or {}).items():
        assert getattr(L, f"set_{k}_SIFT3D")(C.byref(s), v) == 0
    assert set_mask(lib, s, mask, form) == 0
    im = lib.image_from_numpy(vol, units)
    kp = T.new_kp(lib)
    out = None
    try:
        if L.SIFT3D_detect_keypoints(C.byref(s), C.byref(im), C.byref(kp)) == 0:
            xyzos, sd, R = lib.keypoints_to_numpy(kp)
            bins = descriptors(lib, s, kp)[0].copy() if len(xyzos) else np.zeros((0, 768), np.float32)
            out = (xyzos.copy(), sd.copy(), R.copy(), bins)
    finally:
        L.cleanup_Keypoint_store(C.byref(kp))
        lib.free_image(im)
        L.cleanup_SIFT3D(C.byref(s))
    return out


def _edits(base, name):
    return next(e for b, n, e in parity.NONFINITE_CASES if (b, n) == (base, name))


def check_nonfinite_fatal_case(lib, base, name, form="host"):
    """A volume the reference's detect fails on (a NaN gradient in a candidate's orientation window): it fails unmasked, and an
    all-zero mask -- every candidate removed before orientation assignment -- succeeds with no keypoints."""
    want, g = parity.nonfinite_golden()
    assert want[(base, name)] is None
    vol, units, params = parity.nonfinite_input_checked(g, base, name, _edits(base, name))
    assert parity.detect_describe_or_fail(lib, vol, units, params) is None
    got = masked_detect_describe_or_fail(lib, vol, units, params, make_mask("zeros", vol.shape), form)
    assert got is not None and len(got[0]) == 0


def check_nonfinite_masked_case(lib, base, name, mask_name, total, n_kept, form="host"):
    want, g = parity.nonfinite_golden()
    vol, units, params = parity.nonfinite_input_checked(g, base, name, _edits(base, name))
    w = want[(base, name)]
    mask = make_mask(mask_name, vol.shape)
    keep = kept(w[0], mask)
    assert (len(keep), int(keep.sum())) == (total, n_kept)
    got = masked_detect_describe_or_fail(lib, vol, units, params, mask, form)
    assert parity.assert_same_nonfinite_result(got, tuple(a[keep] for a in w), f"{base}/{name} {mask_name}") == n_kept


@pytest.mark.parametrize("base,name", REFERENCE_FAILS)
def test_masked_background_stops_being_fatal(emu, base, name):
    check_nonfinite_fatal_case(emu, base, name)


@pytest.mark.parametrize("base,name,mask_name,total,n_kept", NONFINITE_MASKED)
def test_nonfinite_volumes_with_a_mask(emu, base, name, mask_name, total, n_kept):
    check_nonfinite_masked_case(emu, base, name, mask_name, total, n_kept)


# ---- several GPUs: the gathered list filtered on the host ------------------------------------------------------------------------
def check_loopback_ranks(lib, ranks=2):
    """Two loop-back Z-slab ranks (the volume and parameters tests/test_gpu_slab.py runs on two ranks): the single-GPU masked
    list, descriptors included."""
    L = lib.sift
    L.sift3d_amd_set_num_gpus.argtypes = [P(abi.SIFT3D), C.c_int, C.c_int]
    dims, units, nblobs, seed, params = parity.NONFINITE_BASES["slab64"]
    vol = synth.blobs(*dims, nblobs, seed)
    mask = make_mask("half_x", vol.shape)
    base = run(lib, vol, units, params=params, levels=False)
    want = run(lib, vol, units, mask, params=params, levels=False)
    keep = assert_masked_is_filtered(want, base, mask, "single GPU")
    assert 0 < keep.sum() < len(keep)
    s = T.new_sift(lib)
    for k, v in params.items():
        assert getattr(L, f"set_{k}_SIFT3D")(C.byref(s), v) == 0
    assert L.sift3d_amd_set_num_gpus(C.byref(s), ranks, 1) == 0                # 1 = SIFT3D_AMD_SLAB_LOOPBACK
    assert set_mask(lib, s, mask) == 0
    for _ in range(2):                                                          # the host copy of the bits is fetched once
        kp = T.float_detect(lib, s, vol, units)
        assert record_rows(kp).tobytes() == want["rows"].tobytes()
        bins, xyzs = descriptors(lib, s, kp)
        assert bins.tobytes() == want["bins"].tobytes() and np.array_equal(xyzs, want["xyzs"])
        L.cleanup_Keypoint_store(C.byref(kp))
    # other dimensions fail here too
    im = lib.image_from_numpy(synth.blobs(32, 32, 48, 60, 1), units)
    kp = T.new_kp(lib)
    assert L.SIFT3D_detect_keypoints(C.byref(s), C.byref(im), C.byref(kp)) != 0
    lib.free_image(im)
    L.cleanup_Keypoint_store(C.byref(kp))
    L.cleanup_SIFT3D(C.byref(s))


def test_two_loopback_ranks_with_a_mask(emu, monkeypatch):
    monkeypatch.setenv("S3D_EMU_DEVICES", "2")
    check_loopback_ranks(emu)


# ---- 8: kpSift3D --mask ------------------------------------------------------------------------------------------------------------
def check_cli(tmp_path, env, dims, nblobs, seed, mask_dtype):
    prog = os.path.join(ROOT, "sift3d_amd", "bin", "kpSift3D")
    if not os.path.exists(prog):
        from sift3d_amd import build as _b
        _b.build()
    nx, ny, nz = dims
    vol = synth.blobs(nx, ny, nz, nblobs, seed)
    mask = make_mask("half_x", vol.shape) * (7 if mask_dtype != np.uint8 else 128)        # non-zero, bit 0 clear for uint8
    src, msk, bad = (str(tmp_path / n) for n in ("vol.nii.gz", "mask.nii", "bad.nii"))
    with gzip.open(src, "wb") as f:
        f.write(nifti1_bytes(np.ascontiguousarray(vol.transpose(2, 1, 0)), UNIT))
    open(msk, "wb").write(nifti1_bytes(np.ascontiguousarray(mask.astype(mask_dtype).transpose(2, 1, 0)), UNIT))
    open(bad, "wb").write(nifti1_bytes(np.ones((nx - 1, ny, nz), np.uint8), UNIT))
    e = None if env is None else dict(os.environ, **env)

    def kp_run(*args):
        return subprocess.run([prog, "--peak_thresh", "0.08", *args, src], capture_output=True, text=True, timeout=600, env=e)

    def rows(path):
        return [line.split(",") for line in open(path).read().splitlines()]

    plain, masked = str(tmp_path / "k0.csv"), str(tmp_path / "k1.csv")
    r = kp_run("--keys", plain)
    assert r.returncode == 0, r.stderr
    r = kp_run("--keys", masked, "--mask", msk)
    assert r.returncode == 0, r.stderr
    all_rows, got = rows(plain), rows(masked)
    xyzo = np.array([[float(v) for v in r_[:4]] for r_ in all_rows]).astype(np.int64)
    keep = kept(np.concatenate([xyzo, np.zeros((len(xyzo), 1), np.int64)], axis=1), mask)
    assert 0 < keep.sum() < len(keep)
    assert got == [r_ for r_, k in zip(all_rows, keep) if k]
    r = kp_run("--keys", masked, "--mask", bad)
    assert r.returncode == 1 and f"The mask is {nx - 1} x {ny} x {nz} but the image is {nx} x {ny} x {nz}." in r.stderr
    r = kp_run("--keys", masked, "--mask", str(tmp_path / "none.nii"))
    assert r.returncode == 1 and "Could not read the mask." in r.stderr
    r = subprocess.run([prog, "--help"], capture_output=True, text=True, timeout=60)
    assert r.stdout.startswith("Usage: kpSift3D [image.nii]") and " --mask [filename] " in r.stdout


@pytest.mark.parametrize("mask_dtype", [np.uint8, np.int16, np.float32])
def test_kpSift3D_mask_emulated(emu, tmp_path, mask_dtype):
    check_cli(tmp_path, {"LD_PRELOAD": os.path.join(EMU_DIR, "libsift3d_emu.so")}, (40, 36, 32), 120, 3, mask_dtype)      # 13 keypoints, 6 kept
