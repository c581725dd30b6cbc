"""CPU: keypoints on 8- and 16-bit integer volumes as stored (sift3d_amd_detect_keypoints_typed, sift3d_amd_read_nii_native).

The product's sources run on the SIMT emulator (tests/emu).  The contract: the typed detect gives what SIFT3D_detect_keypoints
gives on the float volume (float)((double)raw * slope + inter) -- the same keypoint records and the same pyramid bytes --
whichever way the volume takes: the first filter converting as it loads (unit voxels, nx % 4 == 0) or a conversion pass
in front of the float path (ragged rows, other spacings)."""
import ctypes as C
import gzip
import json
import os
import subprocess

import numpy as np
import pytest

from sift3d_amd import abi, codeobj, synth
from sift3d_amd.device import DeviceLib, bind_extensions
from tests.test_host_io import nifti1_bytes
from tests.util import rel_close

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")
P = C.POINTER

INT_TYPES = [np.uint8, np.int8, np.uint16, np.int16]
RANGES = {np.uint8: (0, 255), np.int8: (-128, 127), np.uint16: (0, 65535), np.int16: (-1024, 3071)}
SCALINGS = [(1.0, 0.0), (0.01171875, -7.25), (0.0, 3.0)]
# (dims, units, blobs, seed, the first filter reads the stored elements)
VOLUMES = [
    ((64, 40, 36), (1.0, 1.0, 1.0), 100, 0, True),        # <= 64^3
    ((48, 48, 48), (1.0, 1.0, 1.0), 120, 0, True),        # <= 64^3
    ((68, 64, 62), (1.0, 1.0, 1.0), 150, 1, True),        # > 64^3, unit voxels, nx % 4 == 0: the fused typed filter
    ((66, 64, 64), (1.0, 1.0, 1.0), 150, 2, False),       # nx % 4 != 0: conversion pass, then the ragged float kernels
    ((68, 64, 62), (0.7, 0.7, 1.5), 150, 3, False),       # other spacings: conversion pass, then the table-driven x pass
]


@pytest.fixture(scope="module")
def emu():
    subprocess.run(["sh", os.path.join(EMU_DIR, "build_emu.sh")], check=True, capture_output=True)
    L = C.CDLL(os.path.join(EMU_DIR, "libsift3d_emu.so"))
    lib = abi.Sift3dLib(L, None, "emulated")
    bind_extensions(L)
    return lib


def quantise(vol, dtype):
    """`vol` scaled into the type's range and rounded."""
    lo, hi = RANGES[dtype]
    v = vol.astype(np.float64)
    v = (v - v.min()) / (v.max() - v.min())
    return np.rint(lo + v * (hi - lo)).astype(dtype)


def converted(q, slope, inter):
    """The float volume the typed entry point stands for (slope 0 counts as 1)."""
    s = 1.0 if slope == 0.0 else slope
    return (q.astype(np.float64) * s + inter).astype(np.float32)


def key_records(kp):
    """The keypoint records without the one pointer they hold (Keypoint.R.data points into the record itself) and the padding
    in front of it."""
    k = int(kp.slab.num)
    raw = np.ctypeslib.as_array(C.cast(kp.buf, P(C.c_uint8)), shape=(k, C.sizeof(abi.Keypoint))).copy() if k else \
        np.zeros((0, C.sizeof(abi.Keypoint)), np.uint8)
    off = abi.Keypoint.R.offset
    return raw[:, :abi.Keypoint.r_data.size].tobytes() + raw[:, off + 8:].tobytes()


def gss_bytes(lib, s):
    assert lib.sift.sift3d_amd_download_pyramid(C.byref(s), 0) == 0
    out = []
    for i in range(s.gpyr.num_octaves * s.gpyr.num_levels):
        out.append(lib.image_to_numpy(s.gpyr.levels[i]).tobytes())
    return out


def new_sift(lib):
    s = abi.SIFT3D()
    assert lib.sift.init_SIFT3D(C.byref(s)) == 0
    return s


def new_kp(lib):
    kp = abi.Keypoint_store()
    lib.sift.init_Keypoint_store(C.byref(kp))
    return kp


def float_detect(lib, s, vol, units):
    im = lib.image_from_numpy(vol, units)
    kp = new_kp(lib)
    assert lib.sift.SIFT3D_detect_keypoints(C.byref(s), C.byref(im), C.byref(kp)) == 0
    lib.free_image(im)
    return kp


def typed_detect(lib, s, q, units, slope, inter):
    kp = new_kp(lib)
    rc = abi.detect_keypoints_typed(lib.sift, s, q, kp, units, slope, inter)
    assert rc == 0, lib.sift.sift3d_amd_last_error()
    return kp


def check_typed_equals_float(lib, q, units, slope, inter):
    """Typed detect == float detect on the converted volume: keypoint records and GSS level bytes.  Returns the count."""
    sf, st = new_sift(lib), new_sift(lib)
    kf = float_detect(lib, sf, converted(q, slope, inter), units)
    kt = typed_detect(lib, st, q, units, slope, inter)
    n = int(kt.slab.num)
    assert n == int(kf.slab.num)
    assert key_records(kt) == key_records(kf)
    assert (kt.nx, kt.ny, kt.nz) == (kf.nx, kf.ny, kf.nz)
    lf, lt = gss_bytes(lib, sf), gss_bytes(lib, st)
    assert len(lf) == len(lt)
    for i, (a, b) in enumerate(zip(lf, lt)):
        assert a == b, f"GSS level {i} differs"
    assert lib.sift.SIFT3D_have_gpyr(C.byref(st))
    for s, k in ((sf, kf), (st, kt)):
        lib.sift.cleanup_Keypoint_store(C.byref(k))
        lib.sift.cleanup_SIFT3D(C.byref(s))
    return n


def route_is_fused(lib, q, units):
    """Whether the first filter of this volume reads the stored elements (seam: s3d_k_sep_fir_div_typed_eligible)."""
    dev = DeviceLib(lib.sift)
    g = abi.Gauss_filter()
    assert lib.imutil.init_Gauss_filter(C.byref(g), float(np.sqrt(1.6 ** 2 - 1.15 ** 2)), 3) == 0
    uf = np.asarray([np.float32(1.0 / u) for u in units], np.float32)
    nz, ny, nx = q.shape
    r = dev.L.s3d_k_sep_fir_div_typed_eligible(C.c_void_p(q.ctypes.data), abi.TYPED_DTYPES[q.dtype], nx, ny, nz,
                                               uf.ctypes.data_as(P(C.c_float)), g.f.width)
    lib.imutil.cleanup_Gauss_filter(C.byref(g))
    return bool(r)


# ---- 1: typed == float, every route -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("slope,inter", SCALINGS)
@pytest.mark.parametrize("dtype", INT_TYPES)
@pytest.mark.parametrize("dims,units,nblobs,seed,fused", VOLUMES)
def test_typed_detect_equals_float_detect(emu, dims, units, nblobs, seed, fused, dtype, slope, inter):
    nx, ny, nz = dims
    q = quantise(synth.blobs(nx, ny, nz, nblobs, seed), dtype)
    assert route_is_fused(emu, q, units) == fused
    n = check_typed_equals_float(emu, q, units, slope, inter)
    assert n > 0, "degenerate volume: no keypoints"


def test_quantised_volumes_keep_their_keypoints(emu):
    """The counts the quantised volumes were chosen for: 15 at 48^3 / 120 blobs and 21 at 64 x 40 x 36 / 100 blobs."""
    for dims, nblobs, want in (((48, 48, 48), 120, 15), ((64, 40, 36), 100, 21)):
        q = quantise(synth.blobs(*dims, nblobs, 0), np.int16)
        s = new_sift(emu)
        kp = typed_detect(emu, s, q, (1.0, 1.0, 1.0), 0.01171875, -7.25)
        assert int(kp.slab.num) == want
        emu.sift.cleanup_Keypoint_store(C.byref(kp))
        emu.sift.cleanup_SIFT3D(C.byref(s))


# ---- 2: against the oracle -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,slope,inter", [(np.int16, 0.01171875, -7.25), (np.uint8, 0.0, 3.0), (np.uint16, 1.0, 0.0),
                                               (np.int8, 0.01171875, -7.25)])
@pytest.mark.parametrize("dims,units,nblobs,seed", [((48, 48, 48), (1.0, 1.0, 1.0), 120, 0),
                                                    ((42, 40, 36), (0.7, 0.7, 1.5), 100, 1)])
def test_typed_detect_describe_against_oracle(emu, oracle, dims, units, nblobs, seed, dtype, slope, inter):
    nx, ny, nz = dims
    q = quantise(synth.blobs(nx, ny, nz, nblobs, seed), dtype)
    want_xyzos, want_sd, want_R = oracle.detect(converted(q, slope, inter), units)
    s = new_sift(emu)
    kp = typed_detect(emu, s, q, units, slope, inter)
    xyzos, sd, R = emu.keypoints_to_numpy(kp)
    assert len(xyzos) > 0
    assert np.array_equal(xyzos, want_xyzos)
    assert np.array_equal(sd, want_sd)
    assert np.abs(R - want_R).max(initial=0) <= 1e-5
    d = abi.SIFT3D_Descriptor_store()
    emu.sift.init_SIFT3D_Descriptor_store(C.byref(d))
    assert emu.sift.SIFT3D_extract_descriptors(C.byref(s), C.byref(kp), C.byref(d)) == 0
    bins, xyzs = emu.descriptors_to_numpy(d)
    wb, wx = oracle.describe(xyzos[:, :3].astype(np.float64), xyzos[:, 3:5], sd, R)
    assert np.array_equal(xyzs, wx)
    ok = rel_close(bins, wb, rtol=1e-4, atol=1e-7)
    assert ok.all(), f"{(~ok).sum()} descriptor floats beyond 1e-4 relative"
    emu.sift.cleanup_SIFT3D_Descriptor_store(C.byref(d))
    emu.sift.cleanup_Keypoint_store(C.byref(kp))
    emu.sift.cleanup_SIFT3D(C.byref(s))


# ---- the kernels on their own (the GPU file repeats this on the device) ---------------------------------------------------------
@pytest.mark.parametrize("dtype", INT_TYPES)
@pytest.mark.parametrize("n,offset", [(1, 0), (5, 1), (4099, 0), (4099, 3), (2 * 1024 * 4 * 4 + 7, 2)])
def test_convert_and_maximum_kernels(emu, dtype, n, offset):
    dev = DeviceLib(emu.sift)
    info = np.iinfo(dtype)
    rng = np.random.default_rng(n + offset)
    buf = rng.integers(info.min, info.max, n + offset, dtype=dtype, endpoint=True)
    v = buf[offset:]                                      # a start that is not aligned to four elements
    v[rng.integers(0, n)] = info.min
    v[rng.integers(0, n)] = info.max
    for slope, inter in ((1.0, 0.0), (0.01171875, -7.25), (-3.5, 100.0), (1e300, 0.0)):
        with np.errstate(over="ignore"):
            want = (v.astype(np.float64) * slope + inter).astype(np.float32)
        got = np.full(n + 1, -1.0, np.float32)
        dev.convert_f32(v.ctypes.data, dtype, n, slope, inter, got.ctypes.data)
        assert got[n] == -1.0
        assert got[:n].tobytes() == want.tobytes()
        m = np.zeros(1, np.float32)
        dev.absmax_typed(v.ctypes.data, dtype, n, slope, inter, m.ctypes.data)
        assert m.tobytes() == np.abs(want).max().tobytes()


# ---- 3: a file with its elements as stored -------------------------------------------------------------------------------------
def _read_nii(lib, path):
    lib.imutil.read_nii.argtypes = [C.c_char_p, P(abi.Image)]
    im = abi.Image()
    lib.imutil.init_im(C.byref(im))
    assert lib.imutil.read_nii(path.encode(), C.byref(im)) == 0
    arr = lib.image_to_numpy(im)
    units = (im.ux, im.uy, im.uz)
    lib.imutil.im_free(C.byref(im))
    return arr, units


def _write(path, raw, gz):
    with (gzip.open(path, "wb") if gz else open(path, "wb")) as f:
        f.write(raw)


@pytest.mark.parametrize("slope,inter", [(0.37, -11.5), (0.0, 4.0)])
@pytest.mark.parametrize("endian,gz", [("<", False), (">", False), ("<", True), (">", True)])
@pytest.mark.parametrize("dtype", INT_TYPES)
def test_read_nii_native_keeps_integers(emu, tmp_path, dtype, endian, gz, slope, inter):
    rng = np.random.default_rng(7)
    info = np.iinfo(dtype)
    data = rng.integers(info.min, info.max, (9, 6, 5), dtype=dtype, endpoint=True)      # [x, y, z]
    path = str(tmp_path / ("v.nii.gz" if gz else "v.nii"))
    _write(path, nifti1_bytes(data, (0.5, 1.25, 3.0), slope, inter, endian, vox_offset=400 if gz else 352), gz)
    v = abi.Volume()
    assert emu.sift.sift3d_amd_read_nii_native(path.encode(), C.byref(v)) == 0
    assert v.dtype == abi.TYPED_DTYPES[np.dtype(dtype)]
    assert (v.nx, v.ny, v.nz) == (9, 6, 5) and (v.ux, v.uy, v.uz) == (0.5, 1.25, 3.0)
    q = abi.volume_to_numpy(v)
    assert np.array_equal(q, data.transpose(2, 1, 0))     # the stored elements, in the host's byte order
    want, units = _read_nii(emu, path)
    assert units == (v.ux, v.uy, v.uz)
    assert (q.astype(np.float64) * v.slope + v.inter).astype(np.float32).tobytes() == want.tobytes()
    if slope == 0.0:
        assert v.slope == 1.0
    emu.sift.sift3d_amd_free_volume(C.byref(v))
    assert not v.data


@pytest.mark.parametrize("dtype", [np.float64, np.int32, np.float32])
def test_read_nii_native_other_types_come_back_as_float(emu, tmp_path, dtype):
    rng = np.random.default_rng(8)
    data = (rng.standard_normal((7, 5, 4)) * 1000).astype(dtype)
    path = str(tmp_path / "v.nii")
    _write(path, nifti1_bytes(data, (1.0, 1.0, 2.0), 0.37, -11.5, ">"), False)
    v = abi.Volume()
    assert emu.sift.sift3d_amd_read_nii_native(path.encode(), C.byref(v)) == 0
    assert v.dtype == abi.SIFT3D_AMD_F32 and (v.slope, v.inter) == (1.0, 0.0)
    want, _ = _read_nii(emu, path)
    assert abi.volume_to_numpy(v).tobytes() == want.tobytes()
    emu.sift.sift3d_amd_free_volume(C.byref(v))


def test_read_nii_native_refuses_channels_and_missing_files(emu, tmp_path):
    data = np.arange(4 * 3 * 2 * 3, dtype=np.int16).reshape(4, 3, 2, 3)
    path = str(tmp_path / "c.nii")
    _write(path, nifti1_bytes(data, (1.0, 1.0, 1.0, 0.0)), False)
    v = abi.Volume()
    assert emu.sift.sift3d_amd_read_nii_native(path.encode(), C.byref(v)) != 0
    assert not v.data
    assert emu.sift.sift3d_amd_read_nii_native(str(tmp_path / "none.nii").encode(), C.byref(v)) != 0


def test_read_analyze_pair_native(emu, tmp_path):
    data = np.arange(5 * 4 * 3, dtype=np.int16).reshape(5, 4, 3) - 17
    raw = nifti1_bytes(data, (1.0, 2.0, 3.0), 2.0, 1.0, "<", vox_offset=0, magic=b"ni1\0")
    (tmp_path / "p.hdr").write_bytes(raw[:348])
    (tmp_path / "p.img").write_bytes(raw[348:])
    v = abi.Volume()
    assert emu.sift.sift3d_amd_read_nii_native(str(tmp_path / "p.img").encode(), C.byref(v)) == 0
    assert np.array_equal(abi.volume_to_numpy(v), data.transpose(2, 1, 0)) and (v.slope, v.inter) == (2.0, 1.0)
    emu.sift.sift3d_amd_free_volume(C.byref(v))


def test_file_to_keypoints_without_a_float_copy(emu, tmp_path):
    """read_nii_native -> typed detect == read_nii -> SIFT3D_detect_keypoints."""
    q = quantise(synth.blobs(40, 36, 32, 80, 4), np.int16)
    path = str(tmp_path / "ct.nii.gz")
    _write(path, nifti1_bytes(np.ascontiguousarray(q.transpose(2, 1, 0)), (1.0, 1.0, 1.0), 0.5, -100.0, ">"), True)
    v = abi.Volume()
    assert emu.sift.sift3d_amd_read_nii_native(path.encode(), C.byref(v)) == 0
    st, sf = new_sift(emu), new_sift(emu)
    kt = new_kp(emu)
    assert emu.sift.sift3d_amd_detect_keypoints_typed(C.byref(st), v.data, v.dtype, 0, v.nx, v.ny, v.nz, v.ux, v.uy, v.uz,
                                                      v.slope, v.inter, C.byref(kt)) == 0
    vol, units = _read_nii(emu, path)
    kf = float_detect(emu, sf, vol, units)
    assert int(kt.slab.num) > 0 and key_records(kt) == key_records(kf)
    emu.sift.sift3d_amd_free_volume(C.byref(v))
    for s, k in ((sf, kf), (st, kt)):
        emu.sift.cleanup_Keypoint_store(C.byref(k))
        emu.sift.cleanup_SIFT3D(C.byref(s))


# ---- 4: arguments, and the struct afterwards ------------------------------------------------------------------------------------
def test_argument_errors_leave_the_struct_usable(emu):
    vol = synth.blobs(32, 32, 32, 40, 0)
    q = quantise(vol, np.int16)
    s = new_sift(emu)
    kp = new_kp(emu)
    f = emu.sift.sift3d_amd_detect_keypoints_typed
    good = (C.c_void_p(q.ctypes.data), abi.SIFT3D_AMD_I16, 0, 32, 32, 32, 1.0, 1.0, 1.0, 1.0, 0.0)

    def call(**kw):
        names = ("vol", "dtype", "on_device", "nx", "ny", "nz", "ux", "uy", "uz", "slope", "inter")
        a = dict(zip(names, good))
        a.update(kw)
        return f(C.byref(s), *[a[k] for k in names], C.byref(kp))

    for bad in (dict(dtype=8), dict(dtype=0), dict(vol=None), dict(slope=float("nan")), dict(slope=float("inf")),
                dict(inter=float("-inf")), dict(nx=0), dict(nz=-3)):
        assert call(**bad) != 0, bad
        assert emu.sift.sift3d_amd_last_error(), bad
    qf = converted(q, 1.0, 0.0)
    assert call(vol=C.c_void_p(qf.ctypes.data), dtype=abi.SIFT3D_AMD_F32, slope=2.0) != 0       # float32 takes no scaling
    assert b"float32" in emu.sift.sift3d_amd_last_error()
    # ... and the struct still detects: float, then typed, equal to each other
    kf = float_detect(emu, s, qf, (1.0, 1.0, 1.0))
    assert call() == 0
    assert int(kp.slab.num) > 0 and key_records(kp) == key_records(kf)
    # float32 through the typed entry point is the float path
    k32 = new_kp(emu)
    assert abi.detect_keypoints_typed(emu.sift, s, qf, k32) == 0
    assert key_records(k32) == key_records(kf)
    for k in (kp, kf, k32):
        emu.sift.cleanup_Keypoint_store(C.byref(k))
    emu.sift.cleanup_SIFT3D(C.byref(s))


def test_struct_reuse_typed_float_typed(emu):
    """typed -> float -> typed on one SIFT3D, same and new dims: every result equals a fresh struct's."""
    s = new_sift(emu)
    steps = [("t", (40, 32, 28), np.int16, 5), ("f", (40, 32, 28), np.int16, 6), ("t", (40, 32, 28), np.uint8, 7),
             ("t", (36, 36, 30), np.uint16, 8), ("f", (32, 30, 34), np.int8, 9), ("t", (32, 30, 34), np.int8, 10)]
    for how, dims, dtype, seed in steps:
        q = quantise(synth.blobs(*dims, 60, seed), dtype)
        fresh = new_sift(emu)
        want = float_detect(emu, fresh, converted(q, 0.5, -3.0), (1.0, 1.0, 1.0))
        got = typed_detect(emu, s, q, (1.0, 1.0, 1.0), 0.5, -3.0) if how == "t" else \
            float_detect(emu, s, converted(q, 0.5, -3.0), (1.0, 1.0, 1.0))
        assert int(got.slab.num) > 0 and key_records(got) == key_records(want), (how, dims, dtype)
        assert gss_bytes(emu, s) == gss_bytes(emu, fresh)
        emu.sift.cleanup_Keypoint_store(C.byref(got))
        emu.sift.cleanup_Keypoint_store(C.byref(want))
        emu.sift.cleanup_SIFT3D(C.byref(fresh))
    emu.sift.cleanup_SIFT3D(C.byref(s))


def test_overflowing_slope_takes_the_verbatim_pass(emu):
    """A slope that overflows the conversion to infinities: the repeat on the literal kernels, as for such a float volume."""
    q = quantise(synth.blobs(24, 24, 24, 20, 1), np.int16)
    with np.errstate(over="ignore"):
        vol = (q.astype(np.float64) * 1e300 + 0.0).astype(np.float32)
    assert np.isinf(vol).any()
    sf, st = new_sift(emu), new_sift(emu)
    im = emu.image_from_numpy(vol, (1.0, 1.0, 1.0))
    kf, kt = new_kp(emu), new_kp(emu)
    rf = emu.sift.SIFT3D_detect_keypoints(C.byref(sf), C.byref(im), C.byref(kf))
    rt = abi.detect_keypoints_typed(emu.sift, st, q, kt, (1.0, 1.0, 1.0), 1e300, 0.0)
    assert rt == rf
    if rf == 0:
        assert key_records(kt) == key_records(kf)
        assert gss_bytes(emu, st) == gss_bytes(emu, sf)
    emu.free_image(im)
    for s, k in ((sf, kf), (st, kt)):
        emu.sift.cleanup_Keypoint_store(C.byref(k))
        emu.sift.cleanup_SIFT3D(C.byref(s))


# ---- 5: the measured Gaussian is still the measured Gaussian ----------------------------------------------------------------------
def test_gauss_kernels_isa_digest_unchanged():
    """bench.py takes the Gaussian's HBM traffic from profiles/pmc_gauss.json only while the machine code of the k_gauss_xy* /
    k_gauss_z* kernels is the code it was measured on: the typed first filter shares their body and must not move them."""
    so = os.path.join(ROOT, "sift3d_amd", "lib", "libsift3d_amd.so")
    if not os.path.exists(so):
        pytest.skip("sift3d_amd/lib/libsift3d_amd.so is not built")
    want = json.load(open(os.path.join(ROOT, "profiles", "pmc_gauss.json")))["gauss_kernels_isa_sha256"]
    assert codeobj.kernel_isa_sha256(so, codeobj.GAUSS_KERNELS) == want
    typed = codeobj.kernel_isa(so, ("k_first_xy_typed", "k_convert_f32", "k_absmax_typed"))
    assert len(typed) == 8 * 4 + 4 + 4                    # half widths 1..8 x four element types, and the two streaming kernels
    assert not any(g in name for name in typed for g in codeobj.GAUSS_KERNELS)
