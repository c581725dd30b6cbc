"""Shared bodies of tests/test_describe_f32.py (CPU, emulator) and tests/test_gpu_describe_f32.py (testing library on
the GPU): the descriptor kernel's back end forms a voxel's 24 histogram contributions as f32 products whose subnormal
bit patterns are the fixed-point integers, and as f64 fused multiply-adds for the few voxels the f32 form cannot take
(s3d_keypoint.hip, (2) in the kernel's header).  Both forms must give the same integers, so a descriptor may not depend
on which form a voxel took."""
from __future__ import annotations

import ctypes as C

import numpy as np

from sift3d_amd import abi, synth
from tests import parity
from tests.util import rel_close

DESC_SIG_FCTR, DESC_RAD_FCTR = 7.071067812, 2.0          # sift.c:45-46
OUTLIER_FACTOR = 50.0


def bind(lib):
    L = lib.sift
    L.s3d_k_set_describe_est_factor.argtypes = [C.c_float]
    L.s3d_k_set_describe_f32_limit.argtypes = [C.c_float]
    L.s3d_k_describe_redo_stats.argtypes = [C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong), C.c_int]
    L.s3d_k_describe_path_stats.argtypes = [C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong), C.c_int]
    return L


class Scene:
    """One volume: detected once by the library and once by the oracle (keypoints must agree), the oracle's descriptors
    computed once and kept; describe() runs the library's descriptor kernel under a given hook setting."""

    def __init__(self, lib, oracle, vol, units):
        self.lib, self.L = lib, bind(lib)
        self.vol, self.units = vol, units
        want_xyzos, want_sd, want_R = oracle.detect(vol, units)
        self.s, self.im, self.kp = parity.run_detect(lib, vol, units)
        self.xyzos, self.sd, self.R = lib.keypoints_to_numpy(self.kp)
        assert np.array_equal(self.xyzos, want_xyzos) and len(self.xyzos) > 0, "detection differs from the oracle's"
        assert np.array_equal(self.sd, want_sd) and np.abs(self.R - want_R).max() <= 1e-5
        self.want, _ = oracle.describe(self.xyzos[:, :3].astype(np.float64), self.xyzos[:, 3:5], self.sd, self.R)
        self.want.setflags(write=False)
        self._runs = {}

    @property
    def k(self):
        return len(self.xyzos)

    def describe(self, limit=1.0, est_factor=1.0):
        """-> dict(bins, fast, slow, described, redone); each (limit, est_factor) is run once and kept."""
        key = (float(limit), float(est_factor))
        if key in self._runs:
            return self._runs[key]
        L = self.L
        a, b, f, s = C.c_ulonglong(), C.c_ulonglong(), C.c_ulonglong(), C.c_ulonglong()
        d = abi.SIFT3D_Descriptor_store()
        L.init_SIFT3D_Descriptor_store(C.byref(d))
        try:
            assert L.s3d_k_set_describe_f32_limit(limit) == 0
            assert L.s3d_k_set_describe_est_factor(est_factor) == 0
            assert L.s3d_k_describe_redo_stats(C.byref(a), C.byref(b), 1) == 0
            assert L.s3d_k_describe_path_stats(C.byref(f), C.byref(s), 1) == 0
            assert L.SIFT3D_extract_descriptors(C.byref(self.s), C.byref(self.kp), C.byref(d)) == 0
            bins, _ = self.lib.descriptors_to_numpy(d)
            assert L.s3d_k_describe_redo_stats(C.byref(a), C.byref(b), 1) == 0
            assert L.s3d_k_describe_path_stats(C.byref(f), C.byref(s), 1) == 0
        finally:
            L.s3d_k_set_describe_f32_limit(1.0)
            L.s3d_k_set_describe_est_factor(1.0)
            L.cleanup_SIFT3D_Descriptor_store(C.byref(d))
        bins.setflags(write=False)
        r = dict(bins=bins, fast=int(f.value), slow=int(s.value), described=int(a.value), redone=int(b.value))
        self._runs[key] = r
        return r

    def close(self):
        self.L.cleanup_Keypoint_store(C.byref(self.kp))
        self.lib.free_image(self.im)
        self.L.cleanup_SIFT3D(C.byref(self.s))


def error_ratio(got, want):
    """worst |got - want| / (1e-4 |want| + 1e-7): 1 is the edge of the contract"""
    g, w = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float((np.abs(g - w) / (1e-4 * np.abs(w) + 1e-7)).max())


def outlier_volume(vol):
    """The volume with three interior voxels raised to 50 x its maximum, and their (x, y, z)."""
    nz, ny, nx = vol.shape
    spots = [(nx // 4, ny // 4, nz // 4), (nx // 2, ny // 2 + 3, nz // 2 - 2), (3 * nx // 4 - 1, 3 * ny // 4, 3 * nz // 4)]
    out = vol.copy()
    for x, y, z in spots:
        out[z, y, x] = OUTLIER_FACTOR * float(vol.max())
    return out, spots


def keypoints_seeing(spots, xyzos, sd, units):
    """How many keypoints certainly have one of `spots` in their descriptor window: the window is the cube of half width
    rad / sqrt(2) (any orientation) cut by the sphere of radius rad = 2 * 7.07 * sd around the keypoint, so the sphere of
    0.9 rad / sqrt(2) lies inside it."""
    u = np.asarray(units, np.float64)
    n = 0
    for (x, y, z, o, _), s in zip(xyzos, sd):
        c = np.array([x, y, z], np.float64) * (2.0 ** o) * u
        r = 0.9 * DESC_RAD_FCTR * DESC_SIG_FCTR * s / np.sqrt(2.0)
        n += any(np.linalg.norm(np.array(p, np.float64) * u - c) <= r for p in spots)
    return n


# ---- the test bodies -------------------------------------------------------------------------------------------------
MIX_LIMIT = 2.0 ** -6


def check_path_independence(scene):
    ref = scene.describe(1.0)
    for lim in (MIX_LIMIT, 2.0 ** -10, 0.0):
        r = scene.describe(lim)
        assert r["bins"].tobytes() == ref["bins"].tobytes(), f"descriptors differ between f32 limit 1 and {lim}"
    z = scene.describe(0.0)
    assert z["fast"] == 0 and z["slow"] > 0, z
    m = scene.describe(MIX_LIMIT)
    assert m["fast"] > 0 and m["slow"] > 0, (m["fast"], m["slow"])
    assert ref["fast"] + ref["slow"] == z["slow"] == m["fast"] + m["slow"]     # the same live voxels whichever form they take


def check_mixed_path_parity(scene, est_factor):
    r = scene.describe(MIX_LIMIT, est_factor)
    ok = rel_close(r["bins"], scene.want, rtol=1e-4, atol=1e-7)
    assert ok.all(), f"{(~ok).sum()} descriptor floats beyond 1e-4 relative (est_factor {est_factor})"
    assert r["described"] == scene.k, (r["described"], scene.k)
    assert r["fast"] > 0 and r["slow"] > 0
    if est_factor != 1.0:                        # a grid that far off is noticed by every window's proof
        assert r["redone"] == scene.k, (r["redone"], scene.k)
    print(f"est_factor {est_factor}: {r['redone']} of {scene.k} windows redone, {r['slow']} of {r['fast'] + r['slow']} voxels in the f64 form")


def check_outliers(scene, spots, min_seeing=5):
    assert keypoints_seeing(spots, scene.xyzos, scene.sd, scene.units) >= min_seeing
    r = scene.describe(1.0)
    assert r["slow"] > 0, "no voxel took the f64 form although the windows hold 50x outliers"
    ok = rel_close(r["bins"], scene.want, rtol=1e-4, atol=1e-7)
    assert ok.all(), f"{(~ok).sum()} descriptor floats beyond 1e-4 relative"
    return r


def check_slow_share(scene, cap=1e-3):
    r = scene.describe(1.0)
    share = r["slow"] / float(r["fast"] + r["slow"])
    print(f"f64-form share at the product setting: {r['slow']} of {r['fast'] + r['slow']} voxels = {share:.3g}")
    assert share <= cap, share
    return share
