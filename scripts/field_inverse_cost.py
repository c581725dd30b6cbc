#!/usr/bin/env python3
"""GPU-box helper: what inverting a displacement field and mapping its Jacobian determinant cost.  On n^3 grids resident in HBM
(source and reference grids alike), the sine field of tests/demons_cases.py at --amp voxels under the map of
tests/similarity_cases.py; HIP events around every form, medians and min - max of --steps rounds after --warmup, the forms
alternated in one process:

  s3d_k_field_invert (the clearing of its partials and its one launch; 30 updates at most, tol 1e-3), with the status bytes;
  s3d_k_field_jacobian, with the determinant map;
  s3d_k_inv_field, tri-linear, of a one-channel blob volume through the same field: the yardstick, the warp a caller of the
  inverse would make next.

    python scripts/field_inverse_cost.py [--steps 20] > profiles/field_inverse_cost.txt
"""
import argparse
import ctypes as C
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import sift3d_amd                                                        # noqa: E402
from sift3d_amd import synth                                             # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--sizes", type=int, nargs="+", default=[256, 512])
ap.add_argument("--amp", type=float, nargs="+", default=[1.5, 10.0])
args = ap.parse_args()
med = statistics.median
_vp = C.c_void_p
_dp = C.POINTER(C.c_double)
A = np.array([0.97, 0.05, -0.02, 1.5, -0.04, 1.02, 0.03, -2.25, 0.01, -0.03, 0.95, 0.75])
MAX_ITER, TOL = 30, 1e-3


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


def row(name, ms, base, nbytes):
    print(f"  {name:<34}{med(ms):>10.3f}{min(ms):>9.3f}{max(ms):>9.3f}{med(ms) / base:>9.2f}{nbytes / med(ms) / 1e9:>9.2f}")


def sine_field(n, amp):
    g = np.arange(n, dtype=np.float32)
    z, y, x = g[:, None, None], g[None, :, None], g[None, None, :]
    one = np.ones((n, n, n), np.float32)
    return np.stack([amp * np.sin(2 * np.pi * y / n) * np.cos(np.pi * z / n) * one, amp * np.sin(2 * np.pi * z / n) * one,
                     amp * np.cos(2 * np.pi * x / n) * np.sin(np.pi * y / n) * one]).astype(np.float32)


def main():
    dev = sift3d_amd.load_device()
    if dev.device_count() < 1:
        sys.exit("no HIP device")
    L = dev.L
    timer = Timer(dev)
    A34 = A.reshape(3, 4)
    Linv = np.linalg.inv(A34[:, :3])
    B = np.ascontiguousarray(np.hstack([Linv, -(Linv @ A34[:, 3:])])).reshape(12)
    Ap, Bp = A.ctypes.data_as(_dp), B.ctypes.data_as(_dp)
    islots, istats = int(L.s3d_k_field_invert_slots()), int(L.s3d_k_field_invert_stats())
    jslots, jstats = int(L.s3d_k_field_jacobian_slots()), int(L.s3d_k_field_jacobian_stats())
    print(f"s3d_k_field_invert (max_iter {MAX_ITER}, tol {TOL}, status bytes written), s3d_k_field_jacobian (map written) and "
          f"s3d_k_inv_field (tri-linear, 1 channel) on one n^3 grid in HBM, the sine field under the test map; HIP events, medians of "
          f"{args.steps} rounds after {args.warmup}, alternated; ratio = to the warp; TB/s = compulsory bytes (inversion: 13 B written "
          f"per voxel, the field gathers not counted; determinant: 12 B read + 4 B written; warp: 12 B read + 4 B written, the "
          f"source gathers not counted) per second")
    for n in args.sizes:
        nvox = n ** 3
        vol = synth.blobs(n, n, n, synth.default_nblobs(n, n, n), 0)
        d_src = dev.upload(vol)
        del vol
        d_w, d_st, d_det, d_dst = dev.malloc(12 * nvox), dev.malloc(nvox), dev.malloc(4 * nvox), dev.malloc(4 * nvox)
        d_ip, d_jp = dev.malloc(islots * istats * 8), dev.malloc(jslots * jstats * 8)
        for amp in args.amp:
            field = sine_field(n, amp)
            d_u = dev.upload(field)
            del field

            def invert():
                dev.check(L.s3d_k_field_invert(d_u, n, n, n, Ap, Bp, d_w, n, n, n, MAX_ITER, TOL, d_st, d_ip, None), "s3d_k_field_invert")

            def jacobian():
                dev.check(L.s3d_k_field_jacobian(d_u, n, n, n, Ap, d_det, d_jp, None), "s3d_k_field_jacobian")

            def warp():
                dev.check(L.s3d_k_inv_field(d_src, n, n, n, 1, d_dst, n, n, n, Ap, d_u, 0, None), "s3d_k_inv_field")

            ms = alternate(timer, [warp, invert, jacobian])
            ip = dev.download(d_ip, (islots, istats), np.float64)
            jp = dev.download(d_jp, (jslots, jstats), np.float64)
            counts = [int(ip[:, k].sum()) for k in range(4)]
            used = jp[jp[:, 1] > 0]
            print(f"{n}^3, amplitude {amp:g}: {ip[:, 4].sum() / nvox:.2f} updates per voxel; status 0 / 1 / 2 / 3: {counts[0]} / "
                  f"{counts[1]} / {counts[2]} / {counts[3]}; largest residual {ip[:, 6].max():.3g}; {int(used[:, 2].sum())} folded, "
                  f"determinant {used[:, 3].min():.3f} .. {used[:, 4].max():.3f}")
            print(f"  {'':<34}{'median ms':>10}{'min':>9}{'max':>9}{'ratio':>9}{'TB/s':>9}")
            row("warp through the field", ms[0], med(ms[0]), 16 * nvox)
            row("field inversion", ms[1], med(ms[0]), 13 * nvox)
            row("Jacobian determinant", ms[2], med(ms[0]), 16 * nvox)
            dev.free(d_u)
        for p in (d_src, d_w, d_st, d_det, d_dst, d_ip, d_jp):
            dev.free(p)


if __name__ == "__main__":
    main()
