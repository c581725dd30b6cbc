#!/usr/bin/env python3
"""GPU-box helper: what a caller saves by handing a volume over as stored (sift3d_amd_detect_keypoints_typed) instead of as
float32.  One process, the benchmark's 512^3 volume quantised to int16 and to uint8, the forms alternated step by step after a
warm-up, host clock around calls that end synchronised (every detect returns with its keypoints on the host):

  (a) SIFT3D_detect_keypoints on the float volume      -- the existing path, the baseline
  (b) typed, host form, int16        (c) typed, host form, uint8
  (d) sift3d_amd_detect_keypoints_dev on the float volume in HBM      (e) typed, on_device, int16

and the host-to-device rate of a plain copy of the float volume, to set the differences against.

    python scripts/typed_input_cost.py [--n 512] [--steps 20] [--warmup 3] > profiles/typed_input_cost.txt
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
import sift3d_amd                                  # noqa: E402
from sift3d_amd import abi, synth                  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=512)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
args = ap.parse_args()
n = args.n

lib = sift3d_amd.load()
dev = sift3d_amd.load_device()
vol = synth.blobs(n, n, n, synth.default_nblobs(n, n, n), 0)


def quantise(v, dtype, lo, hi):
    v = v.astype(np.float64)
    v = (v - v.min()) / (v.max() - v.min())
    return np.rint(lo + v * (hi - lo)).astype(dtype)


q16 = quantise(vol, np.int16, -1024, 3071)
q8 = quantise(vol, np.uint8, 0, 255)
units = (1.0, 1.0, 1.0)
im = lib.image_from_numpy(vol)
d_f32 = dev.upload(vol)
d_i16 = dev.upload(q16)
kp = abi.Keypoint_store()
lib.sift.init_Keypoint_store(C.byref(kp))


def struct():
    s = abi.SIFT3D()
    assert lib.sift.init_SIFT3D(C.byref(s)) == 0
    return s


def typed(s, v, on_device=False, dtype=None):
    if on_device:
        return abi.detect_keypoints_typed(lib.sift, s, v, kp, units, dtype=dtype, shape=(n, n, n))
    return abi.detect_keypoints_typed(lib.sift, s, v, kp, units)


forms = [
    ("a", "SIFT3D_detect_keypoints, float32 host", vol.nbytes,
     lambda s: lib.sift.SIFT3D_detect_keypoints(C.byref(s), C.byref(im), C.byref(kp))),
    ("b", "typed, int16 host", q16.nbytes, lambda s: typed(s, q16)),
    ("c", "typed, uint8 host", q8.nbytes, lambda s: typed(s, q8)),
    ("d", "sift3d_amd_detect_keypoints_dev, float32 in HBM", 0,
     lambda s: lib.sift.sift3d_amd_detect_keypoints_dev(C.byref(s), C.c_void_p(d_f32), n, n, n, 1.0, 1.0, 1.0, C.byref(kp))),
    ("e", "typed on_device, int16 in HBM", 0, lambda s: typed(s, d_i16, True, np.int16)),
]
structs = {k: struct() for k, *_ in forms}               # one struct per form: each keeps its own buffers, as a caller's would
times = {k: [] for k, *_ in forms}
counts = {}
for step in range(args.warmup + args.steps):
    for k, _, _, call in forms:
        t0 = time.perf_counter()
        rc = call(structs[k])
        t1 = time.perf_counter()
        assert rc == 0, (k, lib.sift.sift3d_amd_last_error())
        counts[k] = int(kp.slab.num)
        if step >= args.warmup:
            times[k].append((t1 - t0) * 1e3)

# host-to-device rate of the float volume from the same pageable buffer, for scale
d_tmp = dev.malloc(vol.nbytes)
h2d = []
for i in range(5):
    t0 = time.perf_counter()
    dev.check(dev.L.s3d_rt_h2d(C.c_void_p(d_tmp), C.c_void_p(vol.ctypes.data), vol.nbytes, None))
    dev.sync()
    h2d.append(time.perf_counter() - t0)
rate = vol.nbytes / min(h2d[1:]) / 1e9

print(f"typed input cost: {n}^3, {args.steps} alternated steps per form after {args.warmup} warm-up steps; ms per detect call")
print(f"{'form':<52} {'bytes up':>12} {'median':>8} {'min':>8} {'max':>8} {'keypoints':>10}")
for k, name, up, _ in forms:
    t = times[k]
    print(f"({k}) {name:<48} {up:>12d} {statistics.median(t):>8.2f} {min(t):>8.2f} {max(t):>8.2f} {counts[k]:>10d}")
med = {k: statistics.median(v) for k, v in times.items()}
print(f"host-to-device copy of the float volume (pageable): {rate:.1f} GB/s -> {vol.nbytes / rate / 1e6:.2f} ms for "
      f"{vol.nbytes} bytes")
for k, up in (("b", q16.nbytes), ("c", q8.nbytes)):
    print(f"(a) - ({k}) = {med['a'] - med[k]:.2f} ms; the {vol.nbytes - up} bytes no longer sent take "
          f"{(vol.nbytes - up) / rate / 1e6:.2f} ms at that rate")
print(f"(e) - (d) = {med['e'] - med['d']:+.2f} ms; spread of (d) over its own repeats: {max(times['d']) - min(times['d']):.2f} ms")
assert len(set(counts.values())) <= 3                     # (a) = (d); (b) = (e); (c): one count per volume
assert counts["a"] == counts["d"] and counts["b"] == counts["e"]
