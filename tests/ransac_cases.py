"""Shared by tests/test_ransac_device.py (CPU: the SIMT emulator) and tests/test_gpu_ransac.py (the device): inputs, the numpy
restatement of the consensus count, and the driver that runs find_tform_ransac under one scoring mode."""
import ctypes as C
import os
import re

import numpy as np

from sift3d_amd import abi
from sift3d_amd.device import DeviceLib
from tests.test_reg import A_TRUE, _affine, _bind, _mat, _mat_np, _points

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = C.POINTER
libc = C.CDLL(None)
AUTO, HOST, DEVICE = -1, 0, 1


def _define(path, name):
    with open(os.path.join(ROOT, path)) as f:
        return int(re.search(rf"#define\s+{name}\s+\(?(\d+)", f.read()).group(1))


TILE = _define("include/s3d_device.h", "S3D_RANSAC_TILE")             # models per workgroup of the kernel
BATCH = _define("sift3d_amd/csrc/host/s3d_host.h", "S3D_RANSAC_BATCH")  # models per draw batch of find_tform_ransac

with open(os.path.join(ROOT, "sift3d_amd/csrc/host/s3d_host_reg.c")) as _f:    # AUTO: the device from this npts * num_iter on
    AUTO_MIN_WORK = 1 << int(re.search(r"#define\s+S3D_RANSAC_AUTO_MIN_WORK\s+\(1L << (\d+)\)", _f.read()).group(1))

NPTS = [1, 63, 64, 65, 255, 256, 257, 1000]
NMODELS = sorted({1, 2, 63, 64, 65, 257, TILE - 1, TILE, TILE + 1})
THR2 = [25.0, 0.0]
# an integer model: with ref (10, 20, 30) it gives (12, 17, 31) exactly
M_INT = np.array([[1.0, 0.0, 0.0, 2.0], [0.0, 1.0, 0.0, -3.0], [0.0, 0.0, 1.0, 1.0]])


def kernel_inputs(npts, nmodels, thr2, seed=0):
    """Matches around A_TRUE, models that are perturbations of A_TRUE (model 0: M_INT), and as far as npts allows: row 0 with
    e == thr2 exactly under model 0 (3-4-5 for 25, a perfect fit for 0), row 1 with a NaN, row 2 with an infinity."""
    rng = np.random.default_rng(seed + 7919 * npts + nmodels)
    src, ref = _points(npts, npts // 2, seed + npts, A_TRUE)
    models = A_TRUE[None] + rng.standard_normal((nmodels, 3, 4)) * np.array([0.01, 0.01, 0.01, 3.0])
    models[0] = M_INT
    ref[0] = (10.0, 20.0, 30.0)
    src[0] = (15.0, 21.0, 31.0) if thr2 == 25.0 else (12.0, 17.0, 31.0)
    if npts > 1:
        src[1, 0] = np.nan
    if npts > 2:
        ref[2, 0] = np.inf
    return np.ascontiguousarray(src), np.ascontiguousarray(ref), np.ascontiguousarray(models.reshape(nmodels, 12))


def residuals(src, ref, A):
    """e of every match under the 12 coefficients A, in the host loop's operation order: numpy's elementwise f64 operations
    round separately, like the C expression without contraction, so this is exact."""
    x, y, z = ref[:, 0], ref[:, 1], ref[:, 2]
    with np.errstate(all="ignore"):
        xo = ((A[0] * x + A[1] * y) + A[2] * z) + A[3]
        yo = ((A[4] * x + A[5] * y) + A[6] * z) + A[7]
        zo = ((A[8] * x + A[9] * y) + A[10] * z) + A[11]
        d0, d1, d2 = src[:, 0] - xo, src[:, 1] - yo, src[:, 2] - zo
        return (d0 * d0 + d1 * d1) + d2 * d2


def np_counts(src, ref, models, thr2):
    with np.errstate(all="ignore"):
        return np.array([np.count_nonzero(~(residuals(src, ref, A) > thr2)) for A in models], np.int32)


def device_counts(dev: DeviceLib, src, ref, models, thr2):
    """s3d_k_ransac_count on dev; the counts buffer is filled with garbage first (the launcher zeroes it)."""
    npts, nm = src.shape[0], models.shape[0]
    bufs = [dev.upload(a) for a in (src, ref, models, np.full(nm, 0x55555555, np.int32))]
    try:
        dev.ransac_count(bufs[0], bufs[1], npts, bufs[2], nm, thr2, bufs[3])
        return dev.download(bufs[3], (nm,), np.int32)
    finally:
        for b in bufs:
            dev.free(b)


def check_kernel_grid(dev: DeviceLib, npts):
    for nm in NMODELS:
        for thr2 in THR2:
            src, ref, models = kernel_inputs(npts, nm, thr2)
            want = np_counts(src, ref, models, thr2)
            e0 = residuals(src, ref, models[0])
            assert e0[0] == thr2                                   # the boundary match sits on the threshold exactly ...
            assert want[0] >= 1 + (npts > 1)                       # ... and counts, like the NaN row
            got = device_counts(dev, src, ref, models, thr2)
            assert np.array_equal(got, want), (npts, nm, thr2, got[:8], want[:8])


def _fl(fr):
    return float(fr)                                                   # Fraction -> nearest double (ties to even)


def residual_contracted(s, r, A):
    """e of one match as a compiler that contracts a * b + c into fused multiply-adds would compute it (every product that
    feeds an addition fused into it, the expression's association kept): exact rationals rounded once per fused operation"""
    from fractions import Fraction as F
    s, r, A = [F(float(v)) for v in s], [F(float(v)) for v in r], [F(float(v)) for v in A]
    d = []
    for k in range(3):
        a = A[4 * k: 4 * k + 4]
        t = F(_fl(a[0] * r[0]))
        t = F(_fl(a[1] * r[1] + t))
        t = F(_fl(a[2] * r[2] + t))
        t = F(_fl(t + a[3]))
        d.append(F(_fl(s[k] - t)))
    e = F(_fl(d[0] * d[0]))
    e = F(_fl(d[1] * d[1] + e))
    return _fl(d[2] * d[2] + e)


def contraction_cases(n_each=3, seed=17):
    """Single matches under a perturbed A_TRUE whose residual differs between the separately rounded expression and its
    contracted form, each with the thr2 that separates the two: the smaller of the two residuals, which counts (e == thr2)
    where the larger one does not.  -> [(src 1x3, ref 1x3, model 1x12, thr2, want)], want from the uncontracted form; n_each
    cases where contraction would turn an inlier into an outlier and n_each the other way round."""
    rng = np.random.default_rng(seed)
    A = (A_TRUE + rng.standard_normal((3, 4)) * np.array([0.01, 0.01, 0.01, 3.0])).reshape(12)
    up, down = [], []
    while len(up) < n_each or len(down) < n_each:
        ref = rng.random((1, 3)) * 100
        src = ref @ A.reshape(3, 4)[:, :3].T + A.reshape(3, 4)[:, 3] + rng.standard_normal((1, 3)) * 2
        eu, ef = float(residuals(src, ref, A)[0]), residual_contracted(src[0], ref[0], A)
        if ef > eu and len(up) < n_each:
            up.append((src, ref, A.reshape(1, 12), eu, 1))             # uncontracted: e == thr2, counts; contracted: above
        elif ef < eu and len(down) < n_each:
            down.append((src, ref, A.reshape(1, 12), ef, 0))           # uncontracted: above; contracted: e == thr2, counts
    return up + down


def check_no_contraction(dev: DeviceLib):
    for src, ref, model, thr2, want in contraction_cases():
        assert np_counts(src, ref, model, thr2)[0] == want
        assert int(not residual_contracted(src[0], ref[0], model[0]) > thr2) == 1 - want   # a contracted kernel gives the other count
        got = device_counts(dev, np.ascontiguousarray(src), np.ascontiguousarray(ref), np.ascontiguousarray(model), thr2)
        assert got[0] == want, (thr2, got)


def duplicate_rows_case():
    """rows 0-11 of both arrays are one row: a sample holding two of them is singular and is redrawn"""
    src, ref = _points(40, 10, 7, A_TRUE)
    src[:12], ref[:12] = src[0], ref[0]
    return src, ref


def no_consensus_case():
    """the second case of test_ransac_failures_like_the_reference (with err_thresh 0.5)"""
    rng = np.random.default_rng(0)
    rng.random((3, 3)), rng.random((3, 3))
    return rng.random((30, 3)) * 100, rng.random((30, 3)) * 100


def bind_ransac(L):
    _bind(L)
    u = L.imutil
    if hasattr(u, "sift3d_amd_last_error"):
        u.sift3d_amd_last_error.restype = C.c_char_p
    return L


def run_ransac(L, src, ref, mode=None, err_thresh=5.0, num_iter=500):
    """find_tform_ransac of library L after srand(1) -> (rc, the 3 x 4 matrix left in tform, the next rand(), last_path).
    mode None: a library without the knob (the reference).  The mode is put back to AUTO afterwards."""
    u = L.imutil
    ran = abi.Ransac()
    u.init_Ransac(C.byref(ran))
    ran.err_thresh, ran.num_iter = err_thresh, num_iter
    ms, mr = _mat(L, src), _mat(L, ref)
    t = _affine(L)
    if mode is not None:
        assert u.sift3d_amd_set_ransac_device(mode) == 0
    try:
        libc.srand(1)
        rc = u.find_tform_ransac(C.byref(ran), C.byref(ms), C.byref(mr), C.byref(t))
        nxt = libc.rand()
        path = u.sift3d_amd_ransac_last_path() if mode is not None else None
    finally:
        if mode is not None:
            u.sift3d_amd_set_ransac_device(AUTO)
    A = _mat_np(t.A)
    u.cleanup_Mat_rm(C.byref(ms)), u.cleanup_Mat_rm(C.byref(mr)), u.cleanup_tform(C.byref(t))
    return rc, A, nxt, path


def check_device_equals_host(L, src, ref, want_rc=0, **kw):
    """DEVICE against HOST, bit for bit: return code (want_rc None: whichever, but the same), the matrix left in tform, the next
    rand(), and the paths taken"""
    h = run_ransac(L, src, ref, HOST, **kw)
    d = run_ransac(L, src, ref, DEVICE, **kw)
    assert h[0] == d[0] and (want_rc is None or h[0] == want_rc), (h[0], d[0])
    assert np.array_equal(h[1], d[1]), np.abs(h[1] - d[1]).max()
    assert h[2] == d[2]
    assert (h[3], d[3]) == (0, 1)
    return h, d
