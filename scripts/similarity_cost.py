#!/usr/bin/env python3
"""GPU-box helper: what scoring a registration costs.  s3d_k_similarity_affine against s3d_k_inv_affine on the same volumes --
the warp does the same gathers and stores 4 B/voxel where the score reads 4 B/voxel, so what the score costs beyond it is the
price of the joint histogram and the reductions.  256^3 and 512^3, resident in HBM, the affine map of tests/similarity_cases.py,
tri-linear, 64 and 128 bins; HIP events around every launch (the score: its memset and both kernels), medians of --steps launches
after --warmup, the two kernels alternated in one process.  On the bench's blob volume, on uniform noise, where the bins are
spread, and on a volume that is one background value but for 2 % of its voxels, where nearly every voxel falls into one bin: the
difference between the ratios is the contention of the LDS atomics; each with every lane's own atomic and with the
wave-aggregated update (s3d_k_similarity_set_aggregate).  Then one spline figure, 256^3 x 512 control points against
s3d_k_inv_tps, and the host form sift3d_amd_im_similarity API to API at 256^3 (two uploads).

    python scripts/similarity_cost.py [--steps 20] > profiles/similarity_cost.txt
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
args = ap.parse_args()
med = statistics.median
_vp = C.c_void_p
_dp = C.POINTER(C.c_double)
A = np.array([0.97, 0.05, -0.02, 1.5, -0.04, 1.02, 0.03, -2.25, 0.01, -0.03, 0.95, 0.75])


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


def main():
    dev = sift3d_amd.load_device()
    if dev.device_count() < 1:
        sys.exit("no HIP device")
    L = dev.L
    L.s3d_k_inv_affine.argtypes = [_vp, C.c_int, C.c_int, C.c_int, C.c_int, _vp, C.c_int, C.c_int, C.c_int, _dp, C.c_int, _vp]
    timer = Timer(dev)
    Ap = A.ctypes.data_as(_dp)
    print(f"s3d_k_similarity_affine against s3d_k_inv_affine, tri-linear, 1 channel, source and reference n^3; HIP events, medians of "
          f"{args.steps} launches after {args.warmup}, alternated; ratio = score / warp")
    rng = np.random.default_rng(1)
    for n in args.sizes:
        d_dst = dev.malloc(4 * n ** 3)
        d_hist, d_sums = dev.malloc(128 * 128 * 8), dev.malloc(56)
        d_scr = dev.malloc(max(int(L.s3d_k_similarity_scratch_bytes(n, n, n, b)) for b in (64, 128)))
        for content in ("blobs", "noise", "background"):
            if content == "blobs":
                vol = synth.blobs(n, n, n, synth.default_nblobs(n, n, n), 0)
            elif content == "noise":
                vol = rng.random((n, n, n), dtype=np.float32)
            else:                                                        # one background value but for 2 % of the voxels
                vol = rng.random((n, n, n), dtype=np.float32)
                vol[vol < 0.98] = 0.0
            lo, hi = float(vol.min()), float(vol.max())
            top = np.bincount(np.minimum(((vol.astype(np.float64) - lo) * (64 / (hi - lo))).astype(np.int64), 63).ravel(),
                              minlength=64).max() / vol.size
            d_vol = dev.upload(vol)
            del vol
            print(f"{n}^3 {content} (fullest of 64 bins holds {top:.1%} of the voxels)"
                  f"{'median ms':>10}{'min':>9}{'max':>9}{'ratio':>9}")

            def warp():
                dev.check(L.s3d_k_inv_affine(d_vol, n, n, n, 1, d_dst, n, n, n, Ap, 0, None), "s3d_k_inv_affine")

            def score(bins):
                s = bins / (hi - lo)
                return lambda: dev.check(L.s3d_k_similarity_affine(d_vol, n, n, n, d_vol, n, n, n, Ap, 0, bins, lo, s, lo, s,
                                                                   0.5 * (lo + hi), 0.5 * (lo + hi), d_hist, d_sums, d_scr, None),
                                         "s3d_k_similarity_affine")

            for agg in (0, 1):
                L.s3d_k_similarity_set_aggregate(agg)
                ms = alternate(timer, [warp, score(64), score(128)])
                tag = "wave-aggregated" if agg else "own atomics"
                row("inv_affine", ms[0])
                row(f"similarity 64 bins, {tag}", ms[1], med(ms[0]))
                row(f"similarity 128 bins, {tag}", ms[2], med(ms[0]))
            L.s3d_k_similarity_set_aggregate(-1)
            dev.free(d_vol)
        for p in (d_dst, d_hist, d_sums, d_scr):
            dev.free(p)
    # ---- the spline form -------------------------------------------------------------------------------------------------------
    n, nc = 256, 512
    flat = rng.choice(n ** 3, nc, replace=False)
    c = np.stack([flat % n, flat // n % n, flat // (n * n)], 1).astype(np.float64)
    p = np.ascontiguousarray(np.c_[rng.standard_normal((3, nc)) * 1e-6, A.reshape(3, 4)[:, 3:], A.reshape(3, 4)[:, :3]])
    vol = synth.blobs(n, n, n, synth.default_nblobs(n, n, n), 0)
    lo, hi = float(vol.min()), float(vol.max())
    d_vol, d_dst, d_c, d_p = dev.upload(vol), dev.malloc(4 * n ** 3), dev.upload(c), dev.upload(p)
    d_hist, d_sums, d_scr = dev.malloc(64 * 64 * 8), dev.malloc(56), dev.malloc(int(L.s3d_k_similarity_scratch_bytes(n, n, n, 64)))
    s = 64 / (hi - lo)
    ms = alternate(timer, [lambda: dev.inv_tps(d_vol, (n, n, n), 1, d_dst, (n, n, n), d_c, d_p, nc, 0),
                           lambda: dev.check(L.s3d_k_similarity_tps(d_vol, n, n, n, d_vol, n, n, n, d_c, d_p, nc, 0, 64, lo, s, lo, s,
                                                                    0.5 * (lo + hi), 0.5 * (lo + hi), d_hist, d_sums, d_scr, None),
                                             "s3d_k_similarity_tps")])
    print(f"{n}^3 blobs, spline of {nc} control points{'median ms':>10}{'min':>9}{'max':>9}{'ratio':>9}")
    row("inv_tps", ms[0])
    row("similarity_tps 64 bins", ms[1], med(ms[0]))
    for q in (d_vol, d_dst, d_c, d_p, d_hist, d_sums, d_scr):
        dev.free(q)
    # ---- the host form, API to API ---------------------------------------------------------------------------------------------
    host = sift3d_amd.load()
    im = host.image_from_numpy(vol, (1, 1, 1))
    t, m = abi.Affine(), abi.Mat_rm()
    u = host.imutil
    u.init_tform.argtypes = [_vp, C.c_int]
    u.init_Mat_rm.argtypes = [C.POINTER(abi.Mat_rm), C.c_int, C.c_int, C.c_int, C.c_int]
    u.Affine_set_mat.argtypes = [C.POINTER(abi.Mat_rm), C.POINTER(abi.Affine)]
    assert u.init_tform(C.byref(t), 0) == 0 and u.init_Mat_rm(C.byref(m), 3, 4, 0, 0) == 0
    C.memmove(m.data, A.ctypes.data, A.nbytes)
    assert u.Affine_set_mat(C.byref(m), C.byref(t)) == 0
    out, ts = abi.Similarity(), []
    for i in range(2 + 5):
        t0 = time.perf_counter()
        assert u.sift3d_amd_im_similarity(C.addressof(t), C.byref(im), C.byref(im), None, C.byref(out), None) == 0
        if i >= 2:
            ts.append((time.perf_counter() - t0) * 1e3)
    print(f"sift3d_amd_im_similarity, host volumes {n}^3 (two uploads of {4 * n ** 3 / 2 ** 20:.0f} MiB, two min / max passes, the "
          f"score, 64 bins): median of 5 calls {med(ts):.2f} ms wall clock (min {min(ts):.2f}, max {max(ts):.2f}); n = {out.n} of "
          f"{out.n_total}, ncc {out.ncc:.4f}, mi {out.mi:.4f}")


if __name__ == "__main__":
    main()
