"""Shared by tests/test_tps.py (CPU: host C, the SIMT emulator, the reference) and tests/test_gpu_tps.py (the device): the
thin-plate-spline cases, their numpy restatement, and the drivers that run the warp through the reference, the flat kernel
entry and im_inv_transform."""
import ctypes as C
import os
import re

import numpy as np

from sift3d_amd import abi
from sift3d_amd.device import DeviceLib
from tests.util import nbitdiff

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = C.POINTER


def _define(path, name):
    with open(os.path.join(ROOT, path)) as f:
        return int(re.search(rf"#define\s+{name}\s+\(?(\d+)", f.read()).group(1))


TILE = _define("include/s3d_device.h", "S3D_TPS_TILE")                  # control points per LDS tile of the kernel
N_CTRL = [0, 1, TILE - 1, TILE, TILE + 1, 197]
SRC_DIMS, DST_DIMS = (18, 16, 14), (22, 20, 12)                         # (x, y, z)
A_WARP = np.array([[0.9, 0.1, 0.05, 1.3], [-0.08, 1.05, 0.02, -0.7], [0.03, -0.06, 0.95, 2.2]])
FIELD_DIMS = np.array([96.0, 80.0, 64.0])


def bind(L):
    """the Tps entry points of a library that speaks the C API (product, emulated or reference)"""
    u = L.imutil
    u.init_Mat_rm.argtypes = [P(abi.Mat_rm), C.c_int, C.c_int, C.c_int, C.c_int]
    u.cleanup_Mat_rm.argtypes = [P(abi.Mat_rm)]
    u.cleanup_Mat_rm.restype = None
    u.init_Tps.argtypes = [P(abi.Tps), C.c_int, C.c_int]
    u.resize_Tps.argtypes = [P(abi.Tps), C.c_int, C.c_int]
    u.init_tform.argtypes = [C.c_void_p, C.c_int]
    u.cleanup_tform.argtypes = [C.c_void_p]
    u.cleanup_tform.restype = None
    u.copy_tform.argtypes = [C.c_void_p, C.c_void_p]
    u.write_tform.argtypes = [C.c_char_p, C.c_void_p]
    u.tform_get_size.argtypes = [C.c_void_p]
    u.tform_get_size.restype = C.c_size_t
    u.tform_type_get_size.argtypes = [C.c_int]
    u.tform_type_get_size.restype = C.c_size_t
    u.tform_get_type.argtypes = [C.c_void_p]
    u.apply_tform_xyz.argtypes = [C.c_void_p, C.c_double, C.c_double, C.c_double] + [P(C.c_double)] * 3
    u.apply_tform_xyz.restype = None
    u.apply_tform_Mat_rm.argtypes = [C.c_void_p, P(abi.Mat_rm), P(abi.Mat_rm)]
    u.im_inv_transform.argtypes = [C.c_void_p, P(abi.Image), C.c_int, C.c_int, P(abi.Image)]
    if hasattr(u, "sift3d_amd_fit_tps"):
        u.sift3d_amd_fit_tps.argtypes = [P(abi.Mat_rm), P(abi.Mat_rm), C.c_double, P(abi.Tps)]
        u.sift3d_amd_last_error.restype = C.c_char_p
    return L


def mat(L, a):
    a = np.ascontiguousarray(a, np.float64)
    m = abi.Mat_rm()
    assert L.imutil.init_Mat_rm(C.byref(m), a.shape[0], a.shape[1], 0, 0) == 0
    if a.size:
        C.memmove(m.data, a.ctypes.data, a.nbytes)
    return m


def mat_np(m):
    if m.num_rows * m.num_cols == 0:
        return np.zeros((m.num_rows, m.num_cols))
    return np.ctypeslib.as_array(C.cast(m.data, P(C.c_double)), (m.num_rows, m.num_cols)).copy()


def make_tps(L, ctrl, params):
    """a Tps of library L (its own init_Tps, so its own vtable) holding ctrl (N x 3) and params (3 x (N + 4))"""
    n = ctrl.shape[0]
    assert params.shape == (3, n + 4)
    t = abi.Tps()
    assert L.imutil.init_Tps(C.byref(t), 3, n + 4) == 0
    assert (t.params.num_rows, t.params.num_cols, t.kp_src.num_rows, t.kp_src.num_cols, t.dim) == (3, n + 4, n, 3, 3)
    params, ctrl = np.ascontiguousarray(params, np.float64), np.ascontiguousarray(ctrl, np.float64)
    C.memmove(t.params.data, params.ctypes.data, params.nbytes)
    if n:
        C.memmove(t.kp_src.data, ctrl.ctypes.data, ctrl.nbytes)
    return t


# ---- numpy restatement ------------------------------------------------------------------------------------------------------
def U(r2):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(r2 == 0, 0.0, r2 * np.log(r2))


def np_fit(ref, src, lam):
    """[K + lam I, P; P^T, 0] [w; a] = [src; 0] by numpy's LU -> params 3 x (N + 4)"""
    n = len(ref)
    K = U(((ref[:, None] - ref[None]) ** 2).sum(-1)) + lam * np.eye(n)
    Pm = np.c_[np.ones(n), ref]
    M = np.block([[K, Pm], [Pm.T, np.zeros((4, 4))]])
    return np.ascontiguousarray(np.linalg.solve(M, np.r_[src, np.zeros((4, 3))]).T)


def np_apply(ctrl, params, pts):
    """f(pts) -> (values M x 3, B M x 3): B = sum |U_n w_n| + |tail terms|, the magnitude every rounding is relative to"""
    n = len(ctrl)
    K = U(((pts[:, None] - ctrl[None]) ** 2).sum(-1)) if n else np.zeros((len(pts), 0))
    Q = np.c_[np.ones(len(pts)), pts]
    return K @ params[:, :n].T + Q @ params[:, n:].T, np.abs(K) @ np.abs(params[:, :n]).T + np.abs(Q) @ np.abs(params[:, n:]).T


def disp(p):
    """the smooth deformation field of the spline tests (amplitude 2.5 voxels over a 96 x 80 x 64 volume)"""
    amp = 2.5
    x, y, z = p.T
    nx, ny, nz = FIELD_DIMS
    return np.stack([amp * np.sin(2 * np.pi * y / ny) * np.cos(np.pi * z / nz) + 1.0,
                     amp * np.sin(2 * np.pi * z / nz) * np.cos(np.pi * x / nx) - 0.5,
                     0.6 * amp * np.sin(2 * np.pi * x / nx)], 1)


def fit_points(n, sigma, seed):
    """distinct integer ref points, src = ref + field + noise"""
    rng = np.random.default_rng(seed)
    ref = np.unique(np.floor(rng.random((n, 3)) * FIELD_DIMS), axis=0)
    rng.shuffle(ref)
    return ref + disp(ref) + rng.standard_normal(ref.shape) * sigma, ref


# ---- warp cases -------------------------------------------------------------------------------------------------------------
_CACHE = {}


def warp_inputs(n, nc, ddims=DST_DIMS, seed=3):
    """source volume [z, y, x(, c)], control points (distinct integer voxels of the destination grid) and params: a lambda = 100
    fit to A_WARP plus 0.8-voxel noise; below 5 points A_WARP with small random weights"""
    key = (n, nc, ddims, seed)
    if key not in _CACHE:
        rng = np.random.default_rng(seed + 1000 * n + nc)
        sx, sy, sz = SRC_DIMS
        src = rng.standard_normal((sz, sy, sx) if nc == 1 else (sz, sy, sx, nc)).astype(np.float32)
        flat = rng.choice(ddims[0] * ddims[1] * ddims[2], n, replace=False)
        ctrl = np.stack([flat % ddims[0], flat // ddims[0] % ddims[1], flat // (ddims[0] * ddims[1])], 1).astype(np.float64)
        if n < 5:
            params = np.c_[rng.standard_normal((3, n)) * 1e-3, A_WARP[:, 3:], A_WARP[:, :3]]
        else:
            params = np_fit(ctrl, ctrl @ A_WARP[:, :3].T + A_WARP[:, 3] + rng.standard_normal((n, 3)) * 0.8, 100.0)
        for a in (src, ctrl, params):
            a.setflags(write=False)
        _CACHE[key] = (src, ctrl, params)
    return _CACHE[key]


def warp_through_api(L, src, ctrl, params, interp, ddims=DST_DIMS):
    """im_inv_transform of library L on a Tps built with L's own init_Tps -> [z, y, x(, c)]"""
    nc = 1 if src.ndim == 3 else src.shape[3]
    t = make_tps(L, ctrl, params)
    im = L.image_from_numpy(src, (1, 1, 1))
    shape = (ddims[2], ddims[1], ddims[0]) + (() if nc == 1 else (nc,))
    dst = L.image_from_numpy(np.full(shape, 7.0, np.float32), (1, 1, 1))
    try:
        assert L.imutil.im_inv_transform(C.byref(t), C.byref(im), interp, 0, C.byref(dst)) == 0
        return L.image_to_numpy(dst)
    finally:
        L.free_image(im), L.free_image(dst), L.imutil.cleanup_tform(C.byref(t))


_WANT = {}


def reference_warp(reference, n, nc, interp, ddims=DST_DIMS):
    """the reference's im_inv_transform on the case, computed once"""
    key = (n, nc, interp, ddims)
    if key not in _WANT:
        want = warp_through_api(bind(reference), *warp_inputs(n, nc, ddims), interp, ddims)
        want.setflags(write=False)
        _WANT[key] = want
    return _WANT[key]


def warp_through_kernel(dev: DeviceLib, src, ctrl, params, interp, ddims=DST_DIMS):
    """s3d_k_inv_tps on dev; the destination is filled with garbage first"""
    nc = 1 if src.ndim == 3 else src.shape[3]
    n = ctrl.shape[0]
    shape = (ddims[2], ddims[1], ddims[0]) + (() if nc == 1 else (nc,))
    bufs = [dev.upload(src), dev.upload(np.full(shape, 7.0, np.float32)), dev.upload(params)]
    if n:
        bufs.append(dev.upload(ctrl))
    try:
        dev.inv_tps(bufs[0], SRC_DIMS, nc, bufs[1], ddims, bufs[3] if n else None, bufs[2], n, interp)
        return dev.download(bufs[1], shape, np.float32)
    finally:
        for b in bufs:
            dev.free(b)


def check_warp(got, want, src, ctrl, params, interp, ddims=DST_DIMS):
    """the bound of the warp.  Linear, N = 0: no differing bit.  Linear, N > 0: per voxel B = sum |U_n w_n| + |tail terms| and
    Delta = (N + 8) 2^-52 B (one rounding per accumulated term plus an ulp-accurate log);
    |got - want| <= 2^-23 |want| + 6 max|src| Delta (tri-linear interpolation moves by at most 2 max|src| per unit of
    each coordinate); voxels whose coordinate lies within Delta of a source boundary plane may flip between inside and outside
    and are excluded: none for the committed seeds.  Lanczos: 1e-6 absolute."""
    n = ctrl.shape[0]
    assert got.shape == want.shape
    assert np.abs(want).max() > 0.1 and (want == 0).any()               # part of the output falls outside the source
    if interp == 1:
        err = np.abs(got.astype(np.float64) - want).max()
        print(f"lanczos N={n}: max abs error {err:.3e}")
        assert err <= 1e-6
        return
    if n == 0:
        assert nbitdiff(got, want) == 0
        return
    z, y, x = np.meshgrid(*(np.arange(d, dtype=np.float64) for d in ddims[::-1]), indexing="ij")
    t, B = np_apply(ctrl, params, np.stack([x.ravel(), y.ravel(), z.ravel()], 1))
    delta = (n + 8) * 2.0 ** -52 * B                                     # per voxel and coordinate
    hi = np.array(SRC_DIMS, np.float64) - 1
    near = (np.abs(t) <= delta) | (np.abs(t - hi) <= delta)
    excluded = near.any(1).reshape(x.shape)
    margin = np.minimum(np.abs(t), np.abs(t - hi)).min()
    tol = 6 * float(np.abs(src).max()) * delta.max(1).reshape(x.shape)
    if got.ndim == 4:
        excluded, tol = excluded[..., None], tol[..., None]
    err = np.abs(got.astype(np.float64) - want)
    bound = 2.0 ** -23 * np.abs(want) + tol
    worst = (err / bound).max()
    print(f"linear N={n}: Delta max {delta.max():.2e}, nearest boundary {margin:.2e}, excluded {int(excluded.sum())}, "
          f"max err {err.max():.3e}, worst err/bound {worst:.3g}, differing voxels {nbitdiff(got, want)}")
    assert excluded.sum() == 0
    assert excluded.mean() <= 1e-3
    assert (err <= bound)[np.broadcast_to(~excluded, err.shape)].all()


# ---- regSift3D --tps end to end ---------------------------------------------------------------------------------------------
E2E_DIMS = (128, 112, 96)


def e2e_volumes():
    """synth.blobs(128, 112, 96, 5000, 21) and its copy deformed by the smooth field scaled to the volume: ref(p) = src(p + d(p))"""
    from scipy.ndimage import map_coordinates
    from sift3d_amd import synth
    nx, ny, nz = E2E_DIMS
    a = synth.blobs(nx, ny, nz, 5000, 21)                                 # [z, y, x]
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    p = np.stack([x.ravel(), y.ravel(), z.ravel()], 1) * (FIELD_DIMS / np.array(E2E_DIMS, np.float64))
    d = disp(p).T.reshape(3, nz, ny, nx)
    b = map_coordinates(a, [z + d[2], y + d[1], x + d[0]], order=1, mode="constant").astype(np.float32)
    return a, b


def e2e_run(tmp_path, env=None, extra=()):
    """regSift3D with and without --tps on the deformed pair -> (mean |warped - ref| over [6:-6]^3 of the affine run, of the
    spline run, the spline's CSV)"""
    import gzip
    from tests.test_cli import BIN, _csv, _nii_f32, run
    from tests.test_host_io import nifti1_bytes
    a, b = e2e_volumes()
    for name, v in (("src", a), ("ref", b)):
        with gzip.open(str(tmp_path / f"{name}.nii.gz"), "wb") as f:
            f.write(nifti1_bytes(np.ascontiguousarray(v.transpose(2, 1, 0)), (1.0, 1.0, 1.0)))
    core = tuple(slice(6, -6) for _ in range(3))
    want = b.transpose(2, 1, 0)[core]
    errs, csv = [], None
    for tag, args in (("affine", ()), ("tps", ("--tps", *extra))):
        tf, wp = str(tmp_path / f"{tag}.csv"), str(tmp_path / f"{tag}.nii.gz")
        r = run(os.path.join(BIN, "regSift3D"), *args, "--transform", tf, "--warped", wp, str(tmp_path / "src.nii.gz"),
                str(tmp_path / "ref.nii.gz"), env=env)
        assert r.returncode == 0, r.stderr
        w, _ = _nii_f32(wp)
        assert w.shape == E2E_DIMS
        errs.append(float(np.abs(w[core] - want).mean()))
        csv = np.array(_csv(tf), np.float64)
    return errs[0], errs[1], csv
