"""GPU: keypoints on 8- and 16-bit integer volumes as stored, through the product library on an MI355X -- the checks of
tests/test_typed_input.py on the device, the host form and the device-resident form, plus 256^3 volumes on the fused route
with bit-equal descriptors (the same kernels on the same pyramid bits)."""
import ctypes as C
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

from sift3d_amd import abi, synth
from sift3d_amd.device import DeviceLib
from tests import test_typed_input as T
from tests.util import rel_close

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def typed_detect_dev(lib, s, q, units, slope, inter):
    """The device-resident form: the volume lies in HBM (the library's own allocator) and is read in place."""
    dev = DeviceLib(lib.sift)
    d_q = dev.upload(q)
    kp = T.new_kp(lib)
    try:
        rc = abi.detect_keypoints_typed(lib.sift, s, d_q, kp, units, slope, inter, dtype=q.dtype, shape=q.shape)
        assert rc == 0, lib.sift.sift3d_amd_last_error()
    finally:
        dev.free(d_q)
    return kp


def descriptors(lib, s, kp):
    d = abi.SIFT3D_Descriptor_store()
    lib.sift.init_SIFT3D_Descriptor_store(C.byref(d))
    assert lib.sift.SIFT3D_extract_descriptors(C.byref(s), C.byref(kp), C.byref(d)) == 0
    bins, xyzs = lib.descriptors_to_numpy(d)
    lib.sift.cleanup_SIFT3D_Descriptor_store(C.byref(d))
    return bins, xyzs


def sha(levels):
    return [hashlib.sha256(b).hexdigest() for b in levels]


def check_forms_equal_float(lib, q, units, slope, inter, bit_equal_descriptors=True):
    """Host form and device form against the float detect on the converted volume: keypoint records, every GSS level (SHA-256)
    and the descriptors.  Returns the keypoint count."""
    sf = T.new_sift(lib)
    kf = T.float_detect(lib, sf, T.converted(q, slope, inter), units)
    want_keys, want_levels = T.key_records(kf), sha(T.gss_bytes(lib, sf))
    want_bins, want_xyzs = descriptors(lib, sf, kf) if int(kf.slab.num) else (None, None)
    n = int(kf.slab.num)
    for form in (T.typed_detect, typed_detect_dev):
        st = T.new_sift(lib)
        kt = form(lib, st, q, units, slope, inter)
        assert int(kt.slab.num) == n, form.__name__
        assert T.key_records(kt) == want_keys, form.__name__
        assert sha(T.gss_bytes(lib, st)) == want_levels, form.__name__
        if n:
            bins, xyzs = descriptors(lib, st, kt)
            assert np.array_equal(xyzs, want_xyzs)
            if bit_equal_descriptors:
                assert bins.tobytes() == want_bins.tobytes(), form.__name__
        lib.sift.cleanup_Keypoint_store(C.byref(kt))
        lib.sift.cleanup_SIFT3D(C.byref(st))
    lib.sift.cleanup_Keypoint_store(C.byref(kf))
    lib.sift.cleanup_SIFT3D(C.byref(sf))
    return n


# ---- 6: items 1 and 2 on the device -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("slope,inter", T.SCALINGS)
@pytest.mark.parametrize("dtype", T.INT_TYPES)
@pytest.mark.parametrize("dims,units,nblobs,seed,fused", T.VOLUMES)
def test_typed_detect_equals_float_detect(hip, dims, units, nblobs, seed, fused, dtype, slope, inter):
    nx, ny, nz = dims
    q = T.quantise(synth.blobs(nx, ny, nz, nblobs, seed), dtype)
    assert T.route_is_fused(hip, q, units) == fused
    assert check_forms_equal_float(hip, q, units, slope, inter) > 0


@pytest.mark.parametrize("dtype,slope,inter", [(np.int16, 0.01171875, -7.25), (np.uint8, 0.0, 3.0), (np.uint16, 1.0, 0.0),
                                               (np.int8, 0.01171875, -7.25)])
@pytest.mark.parametrize("dims,units,nblobs,seed", [((48, 48, 48), (1.0, 1.0, 1.0), 120, 0),
                                                    ((64, 40, 36), (1.0, 1.0, 1.0), 100, 0),
                                                    ((68, 64, 62), (0.7, 0.7, 1.5), 150, 3)])
@pytest.mark.parametrize("form", ["host", "device"])
def test_typed_detect_describe_against_oracle(hip, oracle, form, dims, units, nblobs, seed, dtype, slope, inter):
    nx, ny, nz = dims
    q = T.quantise(synth.blobs(nx, ny, nz, nblobs, seed), dtype)
    want_xyzos, want_sd, want_R = oracle.detect(T.converted(q, slope, inter), units)
    s = T.new_sift(hip)
    kp = (T.typed_detect if form == "host" else typed_detect_dev)(hip, s, q, units, slope, inter)
    xyzos, sd, R = hip.keypoints_to_numpy(kp)
    assert len(xyzos) > 0
    assert np.array_equal(xyzos, want_xyzos)
    assert np.array_equal(sd, want_sd)
    assert np.abs(R - want_R).max(initial=0) <= 1e-5
    bins, xyzs = descriptors(hip, s, kp)
    wb, wx = oracle.describe(xyzos[:, :3].astype(np.float64), xyzos[:, 3:5], sd, R)
    assert np.array_equal(xyzs, wx)
    ok = rel_close(bins, wb, rtol=1e-4, atol=1e-7)
    assert ok.all(), f"{(~ok).sum()} descriptor floats beyond 1e-4 relative"
    hip.sift.cleanup_Keypoint_store(C.byref(kp))
    hip.sift.cleanup_SIFT3D(C.byref(s))


@pytest.mark.parametrize("dtype,slope,inter", [(np.int16, 0.01171875, -7.25), (np.uint8, 1.0, 0.0)])
def test_256_cubed_on_the_fused_route(hip, dtype, slope, inter):
    """256^3, unit voxels: the first filter reads the stored elements.  Keypoint records and every GSS level equal the float
    path's by SHA-256; descriptors bit-equal (the order-free fixed-point histogram on identical pyramid bits)."""
    q = T.quantise(synth.blobs(256, 256, 256, 4000, 11), dtype)
    assert T.route_is_fused(hip, q, (1.0, 1.0, 1.0))
    assert check_forms_equal_float(hip, q, (1.0, 1.0, 1.0), slope, inter) > 0


# The device form on a torch tensor's data_ptr().  In a process of its own, torch imported first, as every torch process of
# this suite is (tests/test_gpu_slab.py): torch brings its own copy of the HIP runtime, and the test process, which has the
# library's loaded already, does not take a second one in.
TORCH_WORKER = r'''
import ctypes as C, hashlib, sys
import numpy as np, torch
sys.path.insert(0, sys.argv[1])
import sift3d_amd
from sift3d_amd import abi
lib = sift3d_amd.load()
data = np.load(sys.argv[2])
out = {}
for name in data["names"]:
    q = data[name]
    slope, inter = (float(v) for v in data[name + "_scale"])
    units = tuple(float(v) for v in data[name + "_units"])
    t = torch.from_numpy(q.view(np.int16) if q.dtype == np.uint16 else q).to("cuda")
    torch.cuda.synchronize()
    s = abi.SIFT3D()
    assert lib.sift.init_SIFT3D(C.byref(s)) == 0
    kp = abi.Keypoint_store()
    lib.sift.init_Keypoint_store(C.byref(kp))
    rc = abi.detect_keypoints_typed(lib.sift, s, t.data_ptr(), kp, units, slope, inter, dtype=q.dtype, shape=q.shape)
    assert rc == 0, lib.sift.sift3d_amd_last_error()
    xyzos, sd, R = lib.keypoints_to_numpy(kp)
    assert lib.sift.sift3d_amd_download_pyramid(C.byref(s), 0) == 0
    levels = [hashlib.sha256(lib.image_to_numpy(s.gpyr.levels[i]).tobytes()).hexdigest()
              for i in range(s.gpyr.num_octaves * s.gpyr.num_levels)]
    d = abi.SIFT3D_Descriptor_store()
    lib.sift.init_SIFT3D_Descriptor_store(C.byref(d))
    assert lib.sift.SIFT3D_extract_descriptors(C.byref(s), C.byref(kp), C.byref(d)) == 0
    out[name + "_xyzos"], out[name + "_sd"], out[name + "_R"] = xyzos, sd, R
    out[name + "_levels"] = np.array(levels)
    out[name + "_bins"] = lib.descriptors_to_numpy(d)[0]
    lib.sift.cleanup_SIFT3D_Descriptor_store(C.byref(d))
    lib.sift.cleanup_Keypoint_store(C.byref(kp))
    lib.sift.cleanup_SIFT3D(C.byref(s))
    del t
np.savez(sys.argv[3], **out)
'''


def test_device_form_on_a_torch_tensor(hip, tmp_path):
    """on_device = 1 with torch.Tensor.data_ptr(): fused route, conversion route and a 16-bit unsigned volume, against the float
    detect of this process -- keypoints, every GSS level by SHA-256, descriptors bit-equal."""
    cases = {"fused_i16": ((68, 64, 62), (1.0, 1.0, 1.0), np.int16, 1, 0.01171875, -7.25),
             "ragged_u8": ((66, 64, 64), (1.0, 1.0, 1.0), np.uint8, 2, 0.0, 3.0),
             "units_u16": ((68, 64, 62), (0.7, 0.7, 1.5), np.uint16, 3, 1.0, 0.0),
             "fused_i8": ((48, 48, 48), (1.0, 1.0, 1.0), np.int8, 0, 0.01171875, -7.25)}
    arrays = {"names": np.array(list(cases))}
    for name, (dims, units, dtype, seed, slope, inter) in cases.items():
        arrays[name] = T.quantise(synth.blobs(*dims, 150, seed), dtype)
        arrays[name + "_scale"] = np.array([slope, inter])
        arrays[name + "_units"] = np.array(units)
    src, out = str(tmp_path / "in.npz"), str(tmp_path / "out.npz")
    np.savez(src, **arrays)
    script = tmp_path / "torch_worker.py"
    script.write_text(TORCH_WORKER)
    r = subprocess.run([sys.executable, str(script), ROOT, src, out], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       timeout=600)
    assert r.returncode == 0, r.stdout.decode()[-3000:]
    got = np.load(out)
    for name, (dims, units, dtype, seed, slope, inter) in cases.items():
        s = T.new_sift(hip)
        kf = T.float_detect(hip, s, T.converted(arrays[name], slope, inter), units)
        xyzos, sd, R = hip.keypoints_to_numpy(kf)
        assert len(xyzos) > 0, name
        assert np.array_equal(got[name + "_xyzos"], xyzos) and np.array_equal(got[name + "_sd"], sd), name
        assert got[name + "_R"].tobytes() == R.tobytes(), name
        assert list(got[name + "_levels"]) == sha(T.gss_bytes(hip, s)), name
        assert got[name + "_bins"].tobytes() == descriptors(hip, s, kf)[0].tobytes(), name
        hip.sift.cleanup_Keypoint_store(C.byref(kf))
        hip.sift.cleanup_SIFT3D(C.byref(s))


# ---- 7: the streaming kernels on their own ------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", T.INT_TYPES)
@pytest.mark.parametrize("n,offset", [(1, 0), (5, 1), (4099, 0), (4099, 3), (256 * 1024 * 4 * 4 * 3 + 7, 2), (1 << 24, 0)])
def test_convert_and_maximum_kernels(hip, dtype, n, offset):
    dev = DeviceLib(hip.sift)
    info = np.iinfo(dtype)
    es = np.dtype(dtype).itemsize
    rng = np.random.default_rng(n + offset)
    buf = rng.integers(info.min, info.max, n + offset, dtype=dtype, endpoint=True)
    v = buf[offset:]
    v[rng.integers(0, n)] = info.min                      # the extreme values of the type
    v[rng.integers(0, n)] = info.max
    d_buf = dev.upload(buf)
    d_out = dev.malloc(4 * (n + 1))
    d_max = dev.malloc(4)
    try:
        for slope, inter in ((1.0, 0.0), (0.01171875, -7.25), (-3.5, 100.0), (1e300, 0.0)):
            with np.errstate(over="ignore"):
                want = (v.astype(np.float64) * slope + inter).astype(np.float32)
            dev.check(dev.L.s3d_rt_memset(C.c_void_p(d_out), 0xFF, 4 * (n + 1), None))
            dev.convert_f32(d_buf + offset * es, dtype, n, slope, inter, d_out)
            got = dev.download(d_out, (n + 1,))
            assert got[n:].tobytes() == b"\xff\xff\xff\xff"          # nothing behind the volume is written
            assert got[:n].tobytes() == want.tobytes()
            dev.absmax_typed(d_buf + offset * es, dtype, n, slope, inter, d_max)
            assert dev.download(d_max, (1,)).tobytes() == np.abs(want).max().tobytes()
    finally:
        for p in (d_buf, d_out, d_max):
            dev.free(p)


# ---- 8: one struct, typed and float in turn -----------------------------------------------------------------------------------------
def test_struct_reuse_typed_float_typed(hip):
    s = T.new_sift(hip)
    steps = [("t", (72, 64, 60), np.int16, 5), ("f", (72, 64, 60), np.int16, 6), ("d", (72, 64, 60), np.uint8, 7),
             ("t", (66, 70, 64), np.uint16, 8), ("f", (48, 44, 52), np.int8, 9), ("d", (48, 44, 52), np.int8, 10),
             ("t", (72, 64, 60), np.int16, 5)]
    for how, dims, dtype, seed in steps:
        q = T.quantise(synth.blobs(*dims, 150, seed), dtype)
        fresh = T.new_sift(hip)
        want = T.float_detect(hip, fresh, T.converted(q, 0.5, -3.0), (1.0, 1.0, 1.0))
        if how == "t":
            got = T.typed_detect(hip, s, q, (1.0, 1.0, 1.0), 0.5, -3.0)
        elif how == "d":
            got = typed_detect_dev(hip, s, q, (1.0, 1.0, 1.0), 0.5, -3.0)
        else:
            got = T.float_detect(hip, s, T.converted(q, 0.5, -3.0), (1.0, 1.0, 1.0))
        assert int(got.slab.num) > 0 and T.key_records(got) == T.key_records(want), (how, dims, dtype)
        assert sha(T.gss_bytes(hip, s)) == sha(T.gss_bytes(hip, fresh))
        if int(got.slab.num):
            assert descriptors(hip, s, got)[0].tobytes() == descriptors(hip, fresh, want)[0].tobytes()
        hip.sift.cleanup_Keypoint_store(C.byref(got))
        hip.sift.cleanup_Keypoint_store(C.byref(want))
        hip.sift.cleanup_SIFT3D(C.byref(fresh))
    hip.sift.cleanup_SIFT3D(C.byref(s))


def test_argument_errors_do_no_device_work(hip):
    q = T.quantise(synth.blobs(32, 32, 32, 40, 0), np.int16)
    s = T.new_sift(hip)
    kp = T.new_kp(hip)
    f = hip.sift.sift3d_amd_detect_keypoints_typed
    p = C.c_void_p(q.ctypes.data)
    assert f(C.byref(s), p, 8, 0, 32, 32, 32, 1.0, 1.0, 1.0, 1.0, 0.0, C.byref(kp)) != 0
    assert f(C.byref(s), None, 4, 1, 32, 32, 32, 1.0, 1.0, 1.0, 1.0, 0.0, C.byref(kp)) != 0
    assert f(C.byref(s), p, 4, 0, 32, 32, 32, 1.0, 1.0, 1.0, float("nan"), 0.0, C.byref(kp)) != 0
    assert hip.sift.sift3d_amd_last_error()
    assert not hip.sift.SIFT3D_have_gpyr(C.byref(s))
    assert f(C.byref(s), p, 4, 0, 32, 32, 32, 1.0, 1.0, 1.0, 1.0, 0.0, C.byref(kp)) == 0
    assert int(kp.slab.num) > 0
    hip.sift.cleanup_Keypoint_store(C.byref(kp))
    hip.sift.cleanup_SIFT3D(C.byref(s))
