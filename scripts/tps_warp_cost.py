#!/usr/bin/env python3
"""GPU-box helper: what the thin-plate-spline warp costs.  s3d_k_inv_tps at 256^3 -> 256^3, tri-linear, one channel, with
N in {0, 64, 512} control points, and s3d_k_inv_affine at the same shape: HIP events around every launch, medians of --steps
launches, ns per (voxel x control point), and the f64 instruction rate as a fraction of the 39.3 Tops/s issue rate DESIGN.md
uses (--f64-per-point: the kernel's f64 VALU instructions per voxel and control point, read from the disassembly).
Against it the reference's host loop: im_inv_transform of oracle/_ref/libimutil.so through a Tps on a 64^3 output with N = 64,
wall clock, on this box's host (the loop is single-threaded).

    python scripts/tps_warp_cost.py [--steps 20] > profiles/tps_warp_cost.txt
"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import sift3d_amd                                                        # noqa: E402
from sift3d_amd import abi                                               # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--size", type=int, default=256)
ap.add_argument("--f64-per-point", type=float, default=84.0)
ap.add_argument("--peak-tops", type=float, default=39.3)
args = ap.parse_args()
med = statistics.median
_vp = C.c_void_p


def spline(n, dims, rng):
    """n distinct integer control points of the grid and the parameters of a lambda = 100 fit to a near-identity affine map
    plus half a voxel of noise (numpy; n = 0: the affine map alone)"""
    A = np.array([[0.99, 0.01, 0.0, 1.5], [-0.01, 1.01, 0.01, -0.5], [0.0, -0.01, 0.98, 2.0]])
    if n == 0:
        return np.zeros((0, 3)), np.ascontiguousarray(np.c_[A[:, 3:], A[:, :3]])
    flat = rng.choice(dims[0] * dims[1] * dims[2], n, replace=False)
    c = np.stack([flat % dims[0], flat // dims[0] % dims[1], flat // (dims[0] * dims[1])], 1).astype(np.float64)
    r2 = ((c[:, None] - c[None]) ** 2).sum(-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        K = np.where(r2 == 0, 0.0, r2 * np.log(r2)) + 100.0 * np.eye(n)
    Pm = np.c_[np.ones(n), c]
    M = np.block([[K, Pm], [Pm.T, np.zeros((4, 4))]])
    rhs = np.r_[c @ A[:, :3].T + A[:, 3] + rng.standard_normal((n, 3)) * 0.5, np.zeros((4, 3))]
    return c, np.ascontiguousarray(np.linalg.solve(M, rhs).T)


def timed(dev, launch):
    ev = [_vp(), _vp()]
    for e in ev:
        dev.check(dev.L.s3d_rt_event_create(C.byref(e)), "event")
    ms = []
    for i in range(args.warmup + args.steps):
        dev.check(dev.L.s3d_rt_event_record(ev[0], None), "record")
        launch()
        dev.check(dev.L.s3d_rt_event_record(ev[1], None), "record")
        dev.sync()
        t = C.c_float()
        dev.check(dev.L.s3d_rt_event_elapsed_ms(ev[0], ev[1], C.byref(t)), "elapsed")
        if i >= args.warmup:
            ms.append(t.value)
    for e in ev:
        dev.L.s3d_rt_event_destroy(e)
    return ms


def device_part():
    dev = sift3d_amd.load_device()
    if dev.device_count() < 1:
        sys.exit("no HIP device")
    L, n = dev.L, args.size
    L.s3d_k_inv_affine.argtypes = [_vp, C.c_int, C.c_int, C.c_int, C.c_int, _vp, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double),
                                   C.c_int, _vp]
    rng = np.random.default_rng(1)
    d_src = dev.upload(rng.standard_normal((n, n, n)).astype(np.float32))
    d_dst = dev.malloc(4 * n ** 3)
    vox = float(n) ** 3
    print(f"s3d_k_inv_tps / s3d_k_inv_affine, {n}^3 -> {n}^3, tri-linear, 1 channel; HIP events, {args.steps} launches after {args.warmup}")
    print(f"{'kernel':<22}{'median ms':>10}{'min':>9}{'max':>9}{'ns/(vox x pt)':>15}{'f64 Tops/s':>12}{'of issue rate':>15}")
    A = np.array([0.99, 0.01, 0.0, 1.5, -0.01, 1.01, 0.01, -0.5, 0.0, -0.01, 0.98, 2.0])
    ms = timed(dev, lambda: dev.check(L.s3d_k_inv_affine(d_src, n, n, n, 1, d_dst, n, n, n, A.ctypes.data_as(C.POINTER(C.c_double)), 0, None),
                                      "s3d_k_inv_affine"))
    print(f"{'inv_affine':<22}{med(ms):>10.3f}{min(ms):>9.3f}{max(ms):>9.3f}{'-':>15}{'-':>12}{'-':>15}")
    base = None
    for nc in (0, 64, 512):
        c, p = spline(nc, (n, n, n), rng)
        d_p = dev.upload(p)
        d_c = dev.upload(c) if nc else None
        ms = timed(dev, lambda: dev.inv_tps(d_src, (n, n, n), 1, d_dst, (n, n, n), d_c, d_p, nc, 0))
        if nc == 0:
            base = med(ms)
            print(f"{'inv_tps N=0':<22}{med(ms):>10.3f}{min(ms):>9.3f}{max(ms):>9.3f}{'-':>15}{'-':>12}{'-':>15}")
        else:
            per = (med(ms) - base) * 1e6 / (vox * nc)                   # the control-point loop alone
            tops = args.f64_per_point / per * 1e-3
            print(f"{'inv_tps N=' + str(nc):<22}{med(ms):>10.3f}{min(ms):>9.3f}{max(ms):>9.3f}{per:>15.5f}{tops:>12.2f}"
                  f"{tops / args.peak_tops:>14.1%}")
        dev.free(d_p)
        if d_c:
            dev.free(d_c)
    print(f"(ns per voxel and control point: (median - median at N = 0) / ({n}^3 N); f64 rate: {args.f64_per_point:g} f64 VALU "
          f"instructions per voxel and control point x 64 lanes counted as operations, against {args.peak_tops} Tops/s)")
    dev.free(d_src), dev.free(d_dst)


def reference_part():
    from oracle import oracle as orc
    if not orc.have_ref():
        print("reference: oracle/_ref not built, host loop not timed")
        return
    ref = orc.load_ref()
    u = ref.imutil
    u.init_Tps.argtypes = [C.POINTER(abi.Tps), C.c_int, C.c_int]
    u.im_inv_transform.argtypes = [_vp, C.POINTER(abi.Image), C.c_int, C.c_int, C.POINTER(abi.Image)]
    n, nc = 64, 64
    rng = np.random.default_rng(2)
    c, p = spline(nc, (n, n, n), rng)
    t = abi.Tps()
    assert u.init_Tps(C.byref(t), 3, nc + 4) == 0
    C.memmove(t.params.data, p.ctypes.data, p.nbytes)
    C.memmove(t.kp_src.data, c.ctypes.data, c.nbytes)
    src = ref.image_from_numpy(rng.standard_normal((n, n, n)).astype(np.float32))
    dst = ref.image_from_numpy(np.zeros((n, n, n), np.float32))
    ts = []
    for _ in range(3):
        t0 = time.perf_counter()
        assert u.im_inv_transform(C.byref(t), C.byref(src), 0, 0, C.byref(dst)) == 0
        ts.append(time.perf_counter() - t0)
    per = med(ts) * 1e9 / (n ** 3 * nc)
    print(f"reference im_inv_transform (host loop), {n}^3 output, N = {nc}: median of 3 {med(ts) * 1e3:.1f} ms = {per:.2f} ns per "
          f"(voxel x control point); 256^3 x 512 at that rate: {per * 256 ** 3 * 512 * 1e-9:.0f} s")


if __name__ == "__main__":
    reference_part()                                                     # before this process opens the GPU
    device_part()
