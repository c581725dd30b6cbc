"""Thin-plate-spline registration on the CPU: the Tps type and its host apply against the reference, the fit against its
defining equations, the warp kernel and the registration entry through the SIMT emulator build of the library (tests/emu).
The GPU counterpart is tests/test_gpu_tps.py; the cases are in tests/tps_cases.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import sift3d_amd
from sift3d_amd import abi
from sift3d_amd.device import DeviceLib, bind_extensions
from tests import tps_cases as tc
from tests.test_cli import _csv

EMU_DIR = os.path.join(tc.ROOT, "tests", "emu")
libc = C.CDLL(None)


@pytest.fixture(scope="module")
def host():
    return tc.bind(sift3d_amd.load())


@pytest.fixture(scope="module")
def emu_cdll():
    subprocess.run(["sh", os.path.join(EMU_DIR, "build_emu.sh")], check=True, capture_output=True)
    L = C.CDLL(os.path.join(EMU_DIR, "libsift3d_emu.so"))
    bind_extensions(L)
    return L


@pytest.fixture(scope="module")
def emu(emu_cdll):
    return tc.bind(abi.Sift3dLib(emu_cdll, None, "emulated"))


@pytest.fixture(scope="module")
def emu_dev(emu_cdll):
    return DeviceLib(emu_cdll)


# ---- layout and host apply --------------------------------------------------------------------------------------------------
def test_layout_equals_the_reference(host, reference):
    tc.bind(reference)
    for L in (host, reference):
        assert L.imutil.tform_type_get_size(1) == C.sizeof(abi.Tps) == 88
        assert L.imutil.tform_type_get_size(0) == C.sizeof(abi.Affine)
        t = abi.Tps()
        C.memset(C.byref(t), 0xAB, C.sizeof(t))
        # the fields land where this struct has them: params at 16, kp_src at 48, dim at 80
        assert L.imutil.init_Tps(C.byref(t), 3, 11) == 0
        assert (t.tform.type, t.dim) == (1, 3) and L.imutil.tform_get_size(C.byref(t)) == 88
        assert (t.params.num_rows, t.params.num_cols, t.params.type, t.params.size) == (3, 11, 0, 3 * 11 * 8)
        assert (t.kp_src.num_rows, t.kp_src.num_cols, t.kp_src.type, t.kp_src.size) == (7, 3, 0, 7 * 3 * 8)
        assert not tc.mat_np(t.params).any() and not tc.mat_np(t.kp_src).any()
        assert L.imutil.resize_Tps(C.byref(t), 30, 3) == 0
        assert (t.params.num_rows, t.params.num_cols, t.kp_src.num_rows, t.kp_src.num_cols, t.dim) == (3, 34, 30, 3, 3)
        assert (t.params.size, t.kp_src.size) == (3 * 34 * 8, 30 * 3 * 8)
        assert L.imutil.init_Tps(C.byref(abi.Tps()), 1, 5) != 0
        L.imutil.cleanup_tform(C.byref(t))
    assert (abi.Tps.params.offset, abi.Tps.kp_src.offset, abi.Tps.dim.offset) == (16, 48, 80)


def _apply_case(n, seed=0):
    rng = np.random.default_rng(seed + n)
    ctrl = np.floor(rng.random((n, 3)) * 50)
    params = np.c_[rng.standard_normal((3, n)) * 1e-3, rng.standard_normal((3, 1)) * 5, np.eye(3) + rng.standard_normal((3, 3)) * 0.05]
    pts = rng.random((40, 3)) * 50
    pts[5] = np.floor(pts[5])
    if n:
        pts[0], pts[1] = ctrl[0], ctrl[n // 2]                            # exactly on a control point: U = 0
    return ctrl, params, pts


@pytest.mark.parametrize("n", [0, 1, 7, 200])
def test_host_apply_is_bit_identical_to_the_reference(host, reference, n):
    tc.bind(reference)
    ctrl, params, pts = _apply_case(n)
    outs = []
    for L in (host, reference):
        t = tc.make_tps(L, ctrl, params)
        xyz = np.empty((len(pts), 3))
        o = [C.c_double() for _ in range(3)]
        for i, p in enumerate(pts):
            L.imutil.apply_tform_xyz(C.byref(t), p[0], p[1], p[2], *[C.byref(v) for v in o])
            xyz[i] = [v.value for v in o]
        mi, mo = tc.mat(L, pts.T), tc.mat(L, np.full((3, len(pts)), np.nan))   # one point per column
        assert L.imutil.apply_tform_Mat_rm(C.byref(t), C.byref(mi), C.byref(mo)) == 0
        outs.append((xyz, tc.mat_np(mo)))
        L.imutil.cleanup_Mat_rm(C.byref(mi)), L.imutil.cleanup_Mat_rm(C.byref(mo)), L.imutil.cleanup_tform(C.byref(t))
    (gx, gm), (wx, wm) = outs
    assert np.isfinite(wx).all() and np.abs(wx - pts).max() > 0.1
    assert np.array_equal(gx.view(np.uint64), wx.view(np.uint64))
    assert np.array_equal(gm.view(np.uint64), wm.view(np.uint64))
    assert np.array_equal(gm.T.copy().view(np.uint64), gx.view(np.uint64))
    assert np.abs(gx - tc.np_apply(ctrl, params, pts)[0]).max() <= 1e-9


def test_copy_is_deep_and_write_gives_the_documented_csv(host, tmp_path, capfd):
    ctrl, params, pts = _apply_case(7)
    t = tc.make_tps(host, ctrl, params)
    d = abi.Tps()
    assert host.imutil.init_Tps(C.byref(d), 3, 4) == 0
    assert host.imutil.copy_tform(C.byref(t), C.byref(d)) == 0
    assert d.params.data != t.params.data and d.kp_src.data != t.kp_src.data and d.dim == 3
    assert np.array_equal(tc.mat_np(d.params), params) and np.array_equal(tc.mat_np(d.kp_src), ctrl)
    C.memset(t.params.data, 0, t.params.size)                            # the copy does not follow the original
    assert np.array_equal(tc.mat_np(d.params), params)
    path = str(tmp_path / "sub" / "tps.csv")
    assert host.imutil.write_tform(path.encode(), C.byref(d)) == 0
    m = np.array(_csv(path), np.float64)
    assert m.shape == (7 + 4, 6)
    assert np.array_equal(m[:7, :3], ctrl) and np.abs(m[:7, 3:] - params[:, :7].T).max() <= 5e-7   # "%f"
    assert not m[7:, :3].any() and np.abs(m[7:, 3:] - params[:, 7:].T).max() <= 5e-7
    host.imutil.cleanup_tform(C.byref(t)), host.imutil.cleanup_tform(C.byref(d))
    # init_tform has no point count to allocate with: it keeps failing, as the reference's does
    assert host.imutil.init_tform(C.byref(abi.Tps()), 1) != 0
    capfd.readouterr()


# ---- the fit ----------------------------------------------------------------------------------------------------------------
def _fit(host, src, ref, lam):
    ms, mr = tc.mat(host, src), tc.mat(host, ref)
    t = abi.Tps()
    assert host.imutil.init_Tps(C.byref(t), 3, 4) == 0
    rc = host.imutil.sift3d_amd_fit_tps(C.byref(ms), C.byref(mr), lam, C.byref(t))
    out = (tc.mat_np(t.kp_src), tc.mat_np(t.params)) if rc == 0 else None
    host.imutil.cleanup_Mat_rm(C.byref(ms)), host.imutil.cleanup_Mat_rm(C.byref(mr)), host.imutil.cleanup_tform(C.byref(t))
    return rc, out


@pytest.mark.parametrize("lam", [0.0, 100.0])
@pytest.mark.parametrize("n", [40, 200, 500])
def test_fit_satisfies_the_defining_equations(host, n, lam):
    src, ref = tc.fit_points(n, 0.5, 5 + n)
    rc, (ctrl, params) = _fit(host, src, ref, lam)
    assert rc == 0 and np.array_equal(ctrl, ref) and params.shape == (3, len(ref) + 4)
    n = len(ref)
    w, a = params[:, :n].T, params[:, n:].T
    K = tc.U(((ref[:, None] - ref[None]) ** 2).sum(-1))
    Pm = np.c_[np.ones(n), ref]
    r1 = np.abs((K + lam * np.eye(n)) @ w + Pm @ a - src).max()
    r2 = np.abs(Pm.T @ w).max()
    print(f"N={n} lambda={lam}: |(K + lambda I) w + P a - src| {r1:.2e}, |P^T w| {r2:.2e} (bound {1e-8 * np.abs(w).sum() * np.abs(Pm).max():.2e})")
    assert r1 <= 1e-8
    assert r2 <= 1e-8 * np.abs(w).sum() * np.abs(Pm).max()


def test_fit_beats_the_affine_at_held_out_points(host):
    src, ref = tc.fit_points(200, 0.5, 11)
    rc, (ctrl, params) = _fit(host, src, ref, 100.0)
    assert rc == 0
    test = np.random.default_rng(12).random((2000, 3)) * tc.FIELD_DIMS
    truth = test + tc.disp(test)
    A, *_ = np.linalg.lstsq(np.c_[np.ones(len(ref)), ref], src, rcond=None)
    e_aff = np.linalg.norm(np.c_[np.ones(len(test)), test] @ A - truth, axis=1).mean()
    e_tps = np.linalg.norm(tc.np_apply(ctrl, params, test)[0] - truth, axis=1).mean()
    print(f"held-out mean error: spline {e_tps:.3f}, affine {e_aff:.3f}, ratio {e_tps / e_aff:.3f}")
    assert e_tps <= 0.5 * e_aff


def test_fit_drops_duplicate_rows(host):
    src, ref = tc.fit_points(60, 0.5, 13)
    rc, plain = _fit(host, src, ref, 100.0)
    # rows 0, 7 and 30 again, with other src points, behind and between the others: the earlier row wins
    ref2 = np.r_[ref[:40], ref[[7]], ref[40:], ref[[0, 30]]]
    src2 = np.r_[src[:40], src[[7]] + 3.0, src[40:], src[[0, 30]] - 2.0]
    rc2, dup = _fit(host, src2, ref2, 100.0)
    assert rc == rc2 == 0
    assert np.array_equal(dup[0], plain[0]) and np.array_equal(dup[1], plain[1])


def test_fit_failures(host):
    src, ref = tc.fit_points(60, 0.5, 17)
    flat = ref.copy()
    flat[:, 2] = flat[:, 0] + 2 * flat[:, 1]                              # one plane, not an axis plane
    for s, r, lam, msg in ((src[:3], ref[:3], 100.0, b"at least 4"), (src, flat, 100.0, b"singular"),
                           (np.r_[src[:3], src[:3]], np.r_[ref[:3], ref[:3]], 100.0, b"at least 4"),
                           (src, ref, -1.0, b"lambda"), (src, ref, float("nan"), b"lambda"),
                           (src[:, :2], ref, 100.0, b"n x 3"), (src[:50], ref, 100.0, b"n x 3")):
        rc, _ = _fit(host, s, r, lam)
        assert rc == -1 and msg in host.imutil.sift3d_amd_last_error(), (msg, host.imutil.sift3d_amd_last_error())
    ms, mr = tc.mat(host, src), tc.mat(host, ref)
    ms.type = 1                                                           # SIFT3D_FLOAT
    t = abi.Tps()
    assert host.imutil.init_Tps(C.byref(t), 3, 4) == 0
    assert host.imutil.sift3d_amd_fit_tps(C.byref(ms), C.byref(mr), 100.0, C.byref(t)) == -1
    assert b"type double" in host.imutil.sift3d_amd_last_error()


# ---- the warp kernel through the emulator -----------------------------------------------------------------------------------
def test_case_grid_covers_the_control_point_tile():
    assert {0, 1, tc.TILE - 1, tc.TILE, tc.TILE + 1, 197} == set(tc.N_CTRL)


@pytest.mark.parametrize("interp,nc", [(0, 1), (0, 3), (1, 1)])
@pytest.mark.parametrize("n", tc.N_CTRL)
def test_warp_kernel_emulated_vs_reference(emu_dev, reference, n, interp, nc):
    src, ctrl, params = tc.warp_inputs(n, nc)
    want = tc.reference_warp(reference, n, nc, interp)
    got = tc.warp_through_kernel(emu_dev, src, ctrl, params, interp)
    tc.check_warp(got, want, src, ctrl, params, interp)


@pytest.mark.parametrize("n", [0, 197])
def test_im_inv_transform_emulated_vs_reference(emu, reference, n):
    src, ctrl, params = tc.warp_inputs(n, 1)
    got = tc.warp_through_api(emu, src, ctrl, params, 0)
    tc.check_warp(got, tc.reference_warp(reference, n, 1, 0), src, ctrl, params, 0)


def test_numpy_restatement_reproduces_the_reference_warp(reference):
    """the coordinates check_warp excludes voxels by are the reference's: tri-linear sampling of them gives its bits"""
    from scipy.ndimage import map_coordinates
    src, ctrl, params = tc.warp_inputs(197, 1)
    want = tc.reference_warp(reference, 197, 1, 0)
    z, y, x = np.meshgrid(*(np.arange(d, dtype=np.float64) for d in tc.DST_DIMS[::-1]), indexing="ij")
    t, _ = tc.np_apply(ctrl, params, np.stack([x.ravel(), y.ravel(), z.ravel()], 1))
    inside = ((t >= 0) & (t <= np.array(tc.SRC_DIMS) - 1.0)).all(1)
    got = np.where(inside, map_coordinates(src.astype(np.float64), [t[:, 2], t[:, 1], t[:, 0]], order=1, mode="nearest"), 0.0)
    assert np.array_equal(inside.reshape(want.shape), want != 0)
    assert np.abs(got.reshape(want.shape) - want).max() <= 1e-5


def test_warp_entry_point_failures(emu, emu_dev):
    src, ctrl, params = tc.warp_inputs(7, 1)
    bufs = [emu_dev.upload(a) for a in (src, np.zeros(tc.DST_DIMS[::-1], np.float32), params, ctrl)]
    L, (sx, sy, sz), (dx, dy, dz) = emu_dev.L, tc.SRC_DIMS, tc.DST_DIMS

    def call(sd=(sx, sy, sz), nc=1, dd=(dx, dy, dz), interp=0, c=bufs[3], p=bufs[2]):
        return L.s3d_k_inv_tps(bufs[0], *sd, nc, bufs[1], *dd, c, p, 7, interp, None)

    assert call() == 0
    before = emu_dev.download(bufs[1], tc.DST_DIMS[::-1])
    for kw in (dict(sd=(0, sy, sz)), dict(dd=(dx, 0, dz)), dict(dd=(dx, dy, -1)), dict(nc=0), dict(dd=(dx, 65536, dz)),
               dict(interp=2), dict(interp=-1), dict(p=None), dict(c=None)):
        emu_dev.check(emu_dev.L.s3d_rt_memset(bufs[1], 0, before.nbytes, None), "memset")
        assert call(**kw) != 0 and emu_dev.err(), kw
        assert not emu_dev.download(bufs[1], tc.DST_DIMS[::-1]).any()     # nothing was launched
    for b in bufs:
        emu_dev.free(b)
    # im_inv_transform: a spline of another dimension fails as every unsupported transform does
    t = abi.Tps()
    assert emu.imutil.init_Tps(C.byref(t), 2, 8) == 0
    im = emu.image_from_numpy(src)
    assert emu.imutil.im_inv_transform(C.byref(t), C.byref(im), 0, 0, C.byref(im)) != 0


# ---- the registration entry on hand-made descriptor stores ------------------------------------------------------------------
def _reg_case():
    from tests.test_reg import A_TRUE
    from tests.util import match_sets, rand_desc
    rng = np.random.default_rng(5)
    d1 = rand_desc(90, 7)
    d2 = match_sets(d1, 8)                                                # rows 0..89: a permutation of d1 with noise
    perm = np.random.default_rng(8).permutation(90)
    x2 = np.c_[rng.random((d2.shape[0], 3)) * tc.FIELD_DIMS, np.full(d2.shape[0], 1.6)]
    x1 = np.c_[np.zeros((90, 3)), np.full(90, 1.6)]
    r = x2[:90, :3]
    x1[perm, :3] = r @ A_TRUE[:, :3].T + A_TRUE[:, 3] + tc.disp(r)        # affine + the smooth field
    return d1, x1, d2, x2


def _register(emu, opts, with_tps):
    d1, x1, d2, x2 = _reg_case()
    reg = abi.Reg_SIFT3D()
    assert emu.reg.init_Reg_SIFT3D(C.byref(reg)) == 0
    s1, keep1 = abi.Sift3dLib.descriptor_store_from_numpy(d1, x1)
    s2, keep2 = abi.Sift3dLib.descriptor_store_from_numpy(d2, x2)
    reg.desc_src, reg.desc_ref = s1, s2
    for k in range(3):
        reg.src_units[k], reg.ref_units[k] = (1.0, 1.0, 2.0)[k], (1.0, 0.8, 2.0)[k]
    reg.ran.err_thresh = 2.0
    a, t = abi.Affine(), abi.Tps()
    assert emu.imutil.init_tform(C.byref(a), 0) == 0 and emu.imutil.init_Tps(C.byref(t), 3, 4) == 0
    libc.srand(1)
    if with_tps:
        rc = emu.imutil.sift3d_amd_register_tps(C.byref(reg), C.byref(opts) if opts is not None else None, C.byref(a), C.byref(t))
    else:
        rc = emu.reg.register_SIFT3D(C.byref(reg), C.byref(a))
    assert rc == 0, emu.imutil.sift3d_amd_last_error()
    out = (tc.mat_np(a.A), tc.mat_np(reg.match_src), tc.mat_np(reg.match_ref), tc.mat_np(t.kp_src), tc.mat_np(t.params))
    reg.desc_src = abi.SIFT3D_Descriptor_store()                          # numpy owns those buffers
    reg.desc_ref = abi.SIFT3D_Descriptor_store()
    emu.reg.cleanup_Reg_SIFT3D(C.byref(reg)), emu.imutil.cleanup_tform(C.byref(a)), emu.imutil.cleanup_tform(C.byref(t))
    return out


def _mm_residual(A, ms, mr):
    return np.linalg.norm((ms - (mr @ A[:, :3].T + A[:, 3])) * np.array([1.0, 1.0, 2.0]), axis=1)


def test_register_tps_on_given_descriptors(emu, capfd):
    from tests.test_reg import _bind
    _bind(emu)
    emu.imutil.sift3d_amd_register_tps.argtypes = [C.POINTER(abi.Reg_SIFT3D), C.POINTER(abi.TpsOpts), C.POINTER(abi.Affine),
                                                   C.POINTER(abi.Tps)]
    A0, ms0, mr0, _, _ = _register(emu, None, False)
    # every match under ctrl_thresh is a control point, in match order
    opts = abi.TpsOpts(100.0, 3.0, 0)
    A, ms, mr, ctrl, params = _register(emu, opts, True)
    assert np.array_equal(A, A0) and np.array_equal(ms, ms0) and np.array_equal(mr, mr0) and len(ms) >= 60
    e = _mm_residual(A, ms, mr)
    assert np.abs(e - 3.0).min() > 1e-6 and 20 <= (e <= 3.0).sum() < len(ms)    # some matches are left out, none on the edge
    assert np.array_equal(ctrl, mr[e <= 3.0]) and params.shape == (3, len(ctrl) + 4)
    # defaults: 4 x err_thresh, lambda 1000, at most 512 points
    _, _, _, ctrl_d, _ = _register(emu, None, True)
    assert np.array_equal(ctrl_d, mr[e <= 8.0]) and len(ctrl_d) > len(ctrl)
    # every second match under the threshold is a control point; the others are held out
    under = np.flatnonzero(e <= 8.0)
    opts = abi.TpsOpts(100.0, 0.0, (len(under) + 1) // 2)
    _, _, _, ctrl_h, params_h = _register(emu, opts, True)
    capfd.readouterr()
    assert np.array_equal(ctrl_h, mr[under[::2]])
    held = under[1::2]
    e_tps = np.linalg.norm(tc.np_apply(ctrl_h, params_h, mr[held])[0] - ms[held], axis=1).mean()
    e_aff = np.linalg.norm(mr[held] @ A[:, :3].T + A[:, 3] - ms[held], axis=1).mean()
    print(f"held-out matches: spline {e_tps:.3f}, affine {e_aff:.3f} voxels")
    assert e_tps < e_aff


# ---- the program's options (no device needed: they fail or print before any image is read) ---------------------------------
def test_regSift3D_tps_options():
    from sift3d_amd import build as _b
    from tests.test_cli import BIN, run
    _b.build()
    exe = os.path.join(BIN, "regSift3D")
    r = run(exe, "--help")
    above, below = r.stdout.split("Other options:")
    assert r.returncode == 0 and below.lstrip().startswith("--nn_thresh")
    for opt in ("--tps ", "--tps_lambda", "--tps_thresh", "--tps_max_points", "(default: 1000)", "(default: 512)"):
        assert opt in above and opt not in below, opt
    for args, msg in ((["--tps", "--tps_lambda", "-1"], "Invalid value for tps_lambda."),
                      (["--tps", "--tps_lambda", "nan"], "Invalid value for tps_lambda."),
                      (["--tps", "--tps_thresh", "0"], "Invalid value for tps_thresh."),
                      (["--tps", "--tps_max_points", "3"], "Invalid value for tps_max_points."),
                      (["--tps", "--resample"], "--tps cannot be combined with --resample."),
                      (["--tps", "--type", "tps"], "Unrecognized transformation type: tps")):
        r = run(exe, *args, "--transform", "t.csv", "a.nii", "b.nii")
        assert r.returncode == 1 and msg in r.stderr, (args, r.stderr)
