#!/usr/bin/env python3
"""GPU-box helper: what refining an affine registration on the intensities costs.  One normal-equation pass
(s3d_k_affine_normal_eq: its kernel and the finish launch) against one similarity pass (s3d_k_similarity_affine at 64 bins: its
memset and both launches) on the same 256^3 and 512^3 volumes, resident in HBM -- both read the reference once and gather the
source; the normal equations add a second eight-corner gather for the gradient and 74 f64 sums per voxel where the score has
seven and an LDS atomic.  HIP events around every launch, medians and min - max of --steps launches after --warmup, the two
alternated in one process.  Then a whole sift3d_amd_refine_affine_dev call at 256^3 with the default options from a start about
2 voxels off: the reference is the blob volume warped on the device by the map of tests/similarity_cases.py, the start that map
plus the perturbation `mid` of tests/refine_cases.py scaled to the volume.

    python scripts/refine_cost.py [--steps 20] > profiles/refine_cost.txt
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
from sift3d_amd import abi, synth                                        # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--sizes", type=int, nargs="+", default=[256, 512])
ap.add_argument("--call-size", type=int, default=256)
args = ap.parse_args()
med = statistics.median
_vp = C.c_void_p
_dp = C.POINTER(C.c_double)
A = np.array([0.97, 0.05, -0.02, 1.5, -0.04, 1.02, 0.03, -2.25, 0.01, -0.03, 0.95, 0.75])
MID = np.array([[0.01, -0.008, 0.006, 1.2], [0.007, 0.012, -0.009, -0.8], [-0.006, 0.008, -0.01, 0.6]])


class Timer:
    def __init__(self, dev):
        self.dev, self.ev = dev, [_vp(), _vp()]
        for e in self.ev:
            dev.check(dev.L.s3d_rt_event_create(C.byref(e)), "event")

    def __call__(self, launch):
        dev = self.dev
        dev.check(dev.L.s3d_rt_event_record(self.ev[0], None), "record")
        launch()
        dev.check(dev.L.s3d_rt_event_record(self.ev[1], None), "record")
        dev.sync()
        t = C.c_float()
        dev.check(dev.L.s3d_rt_event_elapsed_ms(self.ev[0], self.ev[1], C.byref(t)), "elapsed")
        return t.value


def alternate(timer, launches):
    """every launch once per round, --warmup + --steps rounds -> the timed rounds' ms per launch"""
    ms = [[] for _ in launches]
    for i in range(args.warmup + args.steps):
        for k, f in enumerate(launches):
            t = timer(f)
            if i >= args.warmup:
                ms[k].append(t)
    return ms


def row(name, ms, base=None):
    r = f"{med(ms) / base:>9.2f}" if base else f"{'-':>9}"
    print(f"  {name:<34}{med(ms):>10.3f}{min(ms):>9.3f}{max(ms):>9.3f}{r}")


def corner_error(P, Q, n):
    p = np.array([[x, y, z, 1.0] for x in (0, n - 1) for y in (0, n - 1) for z in (0, n - 1)])
    return float(np.sqrt((((P - Q) @ p.T) ** 2).sum(0)).max())


def main():
    dev = sift3d_amd.load_device()
    if dev.device_count() < 1:
        sys.exit("no HIP device")
    L = dev.L
    L.s3d_k_inv_affine.argtypes = [_vp, C.c_int, C.c_int, C.c_int, C.c_int, _vp, C.c_int, C.c_int, C.c_int, _dp, C.c_int, _vp]
    timer = Timer(dev)
    Ap = A.ctypes.data_as(_dp)
    print(f"s3d_k_affine_normal_eq against s3d_k_similarity_affine (64 bins), tri-linear, 1 channel, source and reference n^3; HIP "
          f"events, medians of {args.steps} launches after {args.warmup}, alternated; ratio = normal equations / score")
    for n in args.sizes:
        vol = synth.blobs(n, n, n, synth.default_nblobs(n, n, n), 0)
        lo, hi = float(vol.min()), float(vol.max())
        d_vol = dev.upload(vol)
        del vol
        d_hist, d_sums, d_neq = dev.malloc(64 * 64 * 8), dev.malloc(56), dev.malloc(74 * 8)
        d_scr = dev.malloc(max(int(L.s3d_k_similarity_scratch_bytes(n, n, n, 64)), int(L.s3d_k_affine_normal_eq_scratch_bytes(n, n, n))))
        ctr = np.full(3, (n - 1) / 2)
        s = 64 / (hi - lo)

        def score():
            dev.check(L.s3d_k_similarity_affine(d_vol, n, n, n, d_vol, n, n, n, Ap, 0, 64, lo, s, lo, s, 0.5 * (lo + hi),
                                                0.5 * (lo + hi), d_hist, d_sums, d_scr, None), "s3d_k_similarity_affine")

        def neq():
            dev.check(L.s3d_k_affine_normal_eq(d_vol, n, n, n, d_vol, n, n, n, Ap, ctr.ctypes.data_as(_dp), 1.0, 0.0, 1.0, 0.0, d_neq,
                                               d_scr, None), "s3d_k_affine_normal_eq")

        ms = alternate(timer, [score, neq])
        got = dev.download(d_neq, (74,), np.float64)
        print(f"{n}^3 blobs (n = {int(got[73])} of {n ** 3} voxels counted){'median ms':>10}{'min':>9}{'max':>9}{'ratio':>9}")
        row("similarity 64 bins", ms[0])
        row("normal equations", ms[1], med(ms[0]))
        for p in (d_vol, d_hist, d_sums, d_neq, d_scr):
            dev.free(p)
    # ---- a whole call, device volumes -------------------------------------------------------------------------------------------
    n = args.call_size
    host = sift3d_amd.load()
    u = host.imutil
    u.init_tform.argtypes = [_vp, C.c_int]
    u.init_Mat_rm.argtypes = [C.POINTER(abi.Mat_rm), C.c_int, C.c_int, C.c_int, C.c_int]
    u.Affine_set_mat.argtypes = [C.POINTER(abi.Mat_rm), C.POINTER(abi.Affine)]
    vol = synth.blobs(n, n, n, synth.default_nblobs(n, n, n), 0)
    d_src, d_ref = dev.upload(vol), dev.malloc(4 * n ** 3)
    del vol
    dev.check(L.s3d_k_inv_affine(d_src, n, n, n, 1, d_ref, n, n, n, Ap, 0, None), "s3d_k_inv_affine")
    dev.sync()
    true = A.reshape(3, 4)
    pert = MID.copy()
    pert[:, :3] *= 44.0 / n                                              # the same corner displacement as on the 48 x 44 x 40 pair
    start = true + pert
    t, m = abi.Affine(), abi.Mat_rm()
    assert u.init_tform(C.byref(t), 0) == 0 and u.init_Mat_rm(C.byref(m), 3, 4, 0, 0) == 0
    info, ts = abi.RefineInfo(), []
    for i in range(1 + 5):
        C.memmove(m.data, np.ascontiguousarray(start).ctypes.data, 96)
        assert u.Affine_set_mat(C.byref(m), C.byref(t)) == 0
        t0 = time.perf_counter()
        rc = host.sift.sift3d_amd_refine_affine_dev(d_src, n, n, n, d_ref, n, n, n, None, C.byref(t), C.byref(info), None)
        if i >= 1:
            ts.append((time.perf_counter() - t0) * 1e3)
        assert rc == 0, u.sift3d_amd_last_error()
    got = np.frombuffer(C.string_at(t.A.data, 96), np.float64).reshape(3, 4)
    print(f"sift3d_amd_refine_affine_dev, device volumes {n}^3, default options (3 levels), start {corner_error(start, true, n):.3f} "
          f"voxels off: median of 5 calls {med(ts):.2f} ms wall clock (min {min(ts):.2f}, max {max(ts):.2f}); status {info.status}, "
          f"{info.levels_run} levels, {info.iters} accepted steps, {info.passes} passes, cost {info.cost_before:.4g} -> "
          f"{info.cost_after:.4g}, result {corner_error(got, true, n):.2e} voxels off")
    dev.free(d_src)
    dev.free(d_ref)


if __name__ == "__main__":
    main()
