#!/usr/bin/env python3
"""GPU-box helper: what the deformable registration costs.  On 256^3 and 512^3 volumes resident in HBM, HIP events around every
form, medians and min - max of --steps rounds after --warmup, the forms alternated in one process:

  one s3d_k_demons_step (its kernel and the finish launch) from a smooth non-zero field;
  one iteration: that step plus the three Gaussians of sigma 1.5 (s3d_k_sep_fir, one channel, unit spacing) over the components;
  one similarity pass (s3d_k_similarity_affine at 64 bins), the yardstick of profiles/refine_cost.txt.

Then a whole sift3d_amd_register_demons_dev call with the default options at each size, wall clock: the reference is the blob
volume warped on the device by the map of tests/similarity_cases.py plus a sine field of amplitude 1.5 voxels.

    python scripts/demons_cost.py [--steps 20] > profiles/demons_cost.txt
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
ap.add_argument("--calls", type=int, default=20)
args = ap.parse_args()
med = statistics.median
_vp = C.c_void_p
_dp = C.POINTER(C.c_double)
_fp = C.POINTER(C.c_float)
A = np.array([0.97, 0.05, -0.02, 1.5, -0.04, 1.02, 0.03, -2.25, 0.01, -0.03, 0.95, 0.75])
SIGMA = 1.5


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


def row(name, ms, base=None, nbytes=None):
    r = f"{med(ms) / base:>9.2f}" if base else f"{'-':>9}"
    bw = f"{nbytes / med(ms) / 1e9:>9.2f}" if nbytes else f"{'-':>9}"
    print(f"  {name:<34}{med(ms):>10.3f}{min(ms):>9.3f}{max(ms):>9.3f}{r}{bw}")


def gauss_taps(sigma):
    hw = int(np.ceil(3 * sigma))
    k = np.exp(-0.5 * ((np.arange(2 * hw + 1) - hw) / (sigma + np.finfo(np.float64).eps)) ** 2).astype(np.float32)
    return (k / np.float32(k.sum(dtype=np.float32))).astype(np.float32)


def sine_field(n, amp=1.5):
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
    host = sift3d_amd.load()
    u_ = host.imutil
    u_.init_tform.argtypes = [_vp, C.c_int]
    u_.init_Mat_rm.argtypes = [C.POINTER(abi.Mat_rm), C.c_int, C.c_int, C.c_int, C.c_int]
    u_.Affine_set_mat.argtypes = [C.POINTER(abi.Mat_rm), C.POINTER(abi.Affine)]
    u_.sift3d_amd_last_error.restype = C.c_char_p
    L.s3d_k_sep_fir.argtypes = [_vp, _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, _fp, _fp, C.c_int, _vp]
    t, m = abi.Affine(), abi.Mat_rm()
    assert u_.init_tform(C.byref(t), 0) == 0 and u_.init_Mat_rm(C.byref(m), 3, 4, 0, 0) == 0
    C.memmove(m.data, A.ctypes.data, 96)
    assert u_.Affine_set_mat(C.byref(m), C.byref(t)) == 0
    timer = Timer(dev)
    Ap = A.ctypes.data_as(_dp)
    taps = gauss_taps(SIGMA)
    uf = np.ones(3, np.float32)
    print(f"s3d_k_demons_step, one demons iteration (the step and three Gaussians of sigma {SIGMA}, {taps.size} taps) and "
          f"s3d_k_similarity_affine (64 bins); tri-linear, 1 channel, source and reference n^3 in HBM; HIP events, medians of "
          f"{args.steps} rounds after {args.warmup}, alternated; ratio = to the score; TB/s = compulsory bytes (step: 4 B reference + "
          f"12 B field read + 12 B field written per voxel, the source gathers not counted; iteration: the step + 3 x 8 B) per second")
    for n in args.sizes:
        nvox = n ** 3
        vol = synth.blobs(n, n, n, synth.default_nblobs(n, n, n), 0)
        lo, hi = float(vol.min()), float(vol.max())
        d_src = dev.upload(vol)
        del vol
        field = sine_field(n)
        d_true = dev.upload(field)
        del field
        d_ref = dev.malloc(4 * nvox)
        dev.inv_field(d_src, (n, n, n), 1, d_ref, (n, n, n), A, d_true)
        d_u, d_v, d_tmp = dev.malloc(12 * nvox), dev.malloc(12 * nvox), dev.malloc(4 * nvox)
        dev.check(L.s3d_rt_d2d(d_u, d_true, 12 * nvox, None), "d2d")
        d_hist, d_sums7, d_sums3 = dev.malloc(64 * 64 * 8), dev.malloc(56), dev.malloc(24)
        d_scr = dev.malloc(max(int(L.s3d_k_similarity_scratch_bytes(n, n, n, 64)), int(L.s3d_k_demons_step_scratch_bytes(n, n, n))))
        s = 64 / (hi - lo)

        def score():
            dev.check(L.s3d_k_similarity_affine(d_src, n, n, n, d_ref, n, n, n, Ap, 0, 64, lo, s, lo, s, 0.5 * (lo + hi),
                                                0.5 * (lo + hi), d_hist, d_sums7, d_scr, None), "s3d_k_similarity_affine")

        def step():
            dev.check(L.s3d_k_demons_step(d_src, n, n, n, d_ref, n, n, n, Ap, d_u, d_v, 1.0, 0.0, 1.0, 0.0, 0.25, d_sums3, d_scr, None),
                      "s3d_k_demons_step")

        d_w = dev.malloc(12 * nvox)                                      # the smoothed field of a timed iteration (u stays as it is)

        def iteration():
            step()
            for c in range(3):
                dev.check(L.s3d_k_sep_fir(d_v + 4 * c * nvox, d_w + 4 * c * nvox, d_tmp, n, n, n, 1, uf.ctypes.data_as(_fp),
                                          taps.ctypes.data_as(_fp), taps.size, None), "s3d_k_sep_fir")

        ms = alternate(timer, [score, step, iteration])
        got = dev.download(d_sums3, (3,), np.float64)
        print(f"{n}^3 blobs (n = {int(got[1])} of {nvox} voxels counted){'median ms':>10}{'min':>9}{'max':>9}{'ratio':>9}{'TB/s':>9}")
        row("similarity 64 bins", ms[0])
        row("demons step", ms[1], med(ms[0]), 28 * nvox)
        row("demons iteration", ms[2], med(ms[0]), (28 + 24) * nvox)
        for p in (d_u, d_v, d_w, d_tmp, d_hist, d_sums7, d_sums3, d_scr, d_true):
            dev.free(p)
        # ---- a whole call, device volumes, default options ------------------------------------------------------------------------
        d_field = dev.malloc(12 * nvox)
        info, ts = abi.DemonsInfo(), []
        for i in range(1 + args.calls):
            t0 = time.perf_counter()
            rc = host.sift.sift3d_amd_register_demons_dev(d_src, n, n, n, d_ref, n, n, n, C.addressof(t), None, d_field, C.byref(info), None)
            if i >= 1:
                ts.append((time.perf_counter() - t0) * 1e3)
            assert rc == 0, u_.sift3d_amd_last_error()
        print(f"  sift3d_amd_register_demons_dev, default options: median of {args.calls} calls {med(ts):.1f} ms wall clock (min "
              f"{min(ts):.1f}, max {max(ts):.1f}); status {info.status}, {info.levels_run} levels, {info.iters} updates, {info.passes} "
              f"passes, cost {info.cost_before:.4g} -> {info.cost_after:.4g} (ratio {info.cost_after / info.cost_before:.4f}), n "
              f"{info.n_before} -> {info.n_after}, |u| mean {info.mean_disp:.3f} max {info.max_disp:.3f}")
        for p in (d_src, d_ref, d_field):
            dev.free(p)


if __name__ == "__main__":
    main()
