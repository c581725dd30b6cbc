#!/usr/bin/env python3
"""GPU-box helper: what a region of interest (sift3d_amd_set_mask) saves, and what it costs.  One process, the benchmark's
512^3 volume resident in HBM, one struct per form with its mask set once, the forms alternated step by step after a warm-up;
host clock around calls that end synchronised (the detect returns with its keypoints on the host, the descriptor call is
followed by a stream synchronise):

  (a) no mask      (b) all-ones mask      (c) `ball` (centre, radius 0.35 n: ~18 % of the voxels)      (d) `half_x`

detect ms, describe ms (sift3d_amd_extract_descriptors_dev: records stay in HBM), candidates and keypoints of each; then
sift3d_amd_set_mask itself for a host mask and for a device mask, and the pack kernel of octave 0 alone (HIP events around
`--pack-reps` launches) against the time its read takes at the copy ceiling measured for this project (6.29 TB/s).

With --parent-lib the unmasked detect of this build and of another build of the library (the parent commit's) are first
alternated in child processes of their own (SIFT3D_AMD_LIB names the library; the loop of scripts/detect_ab.py), before this
process opens the GPU.

    python scripts/masked_detect_cost.py [--n 512] [--steps 20] [--warmup 3] [--parent-lib PATH] > profiles/masked_detect_cost.txt
"""
import argparse
import ctypes as C
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=512)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--pack-reps", type=int, default=50)
ap.add_argument("--parent-lib", default=None, help="libsift3d_amd.so of the parent commit: alternate the unmasked detect with it")
ap.add_argument("--ab-rounds", type=int, default=3)
ap.add_argument("--ab-child", action="store_true", help=argparse.SUPPRESS)
args = ap.parse_args()
n = args.n
COPY_CEILING = 6.29e12                                   # bytes/s, VERDICT.md

if args.parent_lib:
    this_lib = os.path.join(ROOT, "sift3d_amd", "lib", "libsift3d_amd.so")
    print(f"unmasked detect, this build against the parent's: {args.ab_rounds} alternated pairs of child processes "
          f"({n}^3 in HBM, 10 timed calls each after 2 dropped)")
    for r in range(args.ab_rounds):
        for who, path in (("parent", os.path.abspath(args.parent_lib)), ("this", this_lib)):
            env = dict(os.environ, SIFT3D_AMD_LIB=path)
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--ab-child", "--n", str(n)], env=env,
                               capture_output=True, text=True, timeout=600)
            if p.returncode != 0:
                sys.exit(f"the child process ({who}) failed:\n{p.stdout}{p.stderr}")
            print(f"  round {r} {who:<6} {p.stdout.strip()}")
    print()

import sift3d_amd                                  # noqa: E402
from sift3d_amd import abi, synth                  # noqa: E402

lib = sift3d_amd.load()
dev = sift3d_amd.load_device()
L = lib.sift
vol = synth.blobs(n, n, n, synth.default_nblobs(n, n, n), 0)
d_vol = dev.upload(vol)
if args.ab_child:
    # the unmasked detect of the library SIFT3D_AMD_LIB names, as scripts/detect_ab.py times it: 12 calls, the first two dropped
    s = abi.SIFT3D()
    assert L.init_SIFT3D(C.byref(s)) == 0
    kp = abi.Keypoint_store()
    L.init_Keypoint_store(C.byref(kp))
    ts = []
    for i in range(12):
        dev.sync()
        t0 = time.perf_counter()
        assert L.sift3d_amd_detect_keypoints_dev(C.byref(s), C.c_void_p(d_vol), n, n, n, 1.0, 1.0, 1.0, C.byref(kp)) == 0
        dev.sync()
        ts.append((time.perf_counter() - t0) * 1e3)
    t = ts[2:]
    print(f"detect median {statistics.median(t):.3f} ms, min {min(t):.3f}, max {max(t):.3f}, keypoints {int(kp.slab.num)}")
    sys.exit(0)
z, y, x = np.ogrid[:n, :n, :n]
masks = {
    "a": ("no mask", None),
    "b": ("all-ones mask", np.ones((n, n, n), np.uint8)),
    "c": ("ball", ((x - n // 2) ** 2 + (y - n // 2) ** 2 + (z - n // 2) ** 2 <= (0.35 * n) ** 2).astype(np.uint8)),
    "d": ("half_x", np.ascontiguousarray(np.broadcast_to(x < n // 2, (n, n, n)).astype(np.uint8))),
}
kp = abi.Keypoint_store()
L.init_Keypoint_store(C.byref(kp))
structs = {}
for k, (_, m) in masks.items():
    s = abi.SIFT3D()
    assert L.init_SIFT3D(C.byref(s)) == 0
    if m is not None:
        assert abi.set_mask(L, s, m) == 0, L.sift3d_amd_last_error()
    structs[k] = s

det = {k: [] for k in masks}
des = {k: [] for k in masks}
cand, keys = {}, {}
d_desc = C.c_void_p()
for step in range(args.warmup + args.steps):
    for k in masks:
        s = structs[k]
        t0 = time.perf_counter()
        rc = L.sift3d_amd_detect_keypoints_dev(C.byref(s), C.c_void_p(d_vol), n, n, n, 1.0, 1.0, 1.0, C.byref(kp))
        t1 = time.perf_counter()
        assert rc == 0, (k, L.sift3d_amd_last_error())
        rc = L.sift3d_amd_extract_descriptors_dev(C.byref(s), C.byref(kp), C.byref(d_desc))
        dev.sync()
        t2 = time.perf_counter()
        assert rc == 0, (k, L.sift3d_amd_last_error())
        cand[k], keys[k] = L.sift3d_amd_last_num_candidates(C.byref(s)), int(kp.slab.num)
        if step >= args.warmup:
            det[k].append((t1 - t0) * 1e3)
            des[k].append((t2 - t1) * 1e3)

print(f"masked detect cost: {n}^3 in HBM, {args.steps} alternated steps per form after {args.warmup} warm-up steps; ms per call")
print(f"{'form':<20} {'inside':>7} {'detect med':>10} {'min':>7} {'max':>7} {'describe med':>12} {'min':>7} {'max':>7} "
      f"{'candidates':>10} {'keypoints':>9}")
for k, (name, m) in masks.items():
    inside = 1.0 if m is None else float(m.mean())
    print(f"({k}) {name:<16} {inside:>7.3f} {statistics.median(det[k]):>10.3f} {min(det[k]):>7.3f} {max(det[k]):>7.3f} "
          f"{statistics.median(des[k]):>12.3f} {min(des[k]):>7.3f} {max(des[k]):>7.3f} {cand[k]:>10d} {keys[k]:>9d}")
md = {k: statistics.median(v) for k, v in det.items()}
ms = {k: statistics.median(v) for k, v in des.items()}
print(f"detect (b) - (a) = {md['b'] - md['a']:+.3f} ms; spread of (a) over its own repeats: {max(det['a']) - min(det['a']):.3f} ms")
for k in ("c", "d"):
    print(f"describe ({k}) / (a) = {ms[k] / ms['a']:.3f}; keypoints ({k}) / (a) = {keys[k] / keys['a']:.3f}; "
          f"detect ({k}) - (a) = {md[k] - md['a']:+.3f} ms; detect + describe: {md['a'] + ms['a']:.2f} -> {md[k] + ms[k]:.2f} ms")
assert cand["a"] == cand["b"] and keys["a"] == keys["b"]

# sift3d_amd_set_mask itself: a host mask (upload of n^3 bytes through a staging buffer + pack) and a mask already in HBM
ball = masks["c"][1]
d_ball = dev.upload(ball)
s = structs["c"]
for form, arg, shape in (("host mask", ball, None), ("device mask", d_ball, ball.shape)):
    t = []
    for i in range(6):
        t0 = time.perf_counter()
        assert abi.set_mask(L, s, arg, shape) == 0
        t.append((time.perf_counter() - t0) * 1e3)
    print(f"sift3d_amd_set_mask, {form}: median {statistics.median(t[1:]):.3f} ms, min {min(t[1:]):.3f}, max {max(t[1:]):.3f} "
          f"(5 calls after one warm-up; the bitmaps of all octaves, returns synchronised)")

# the pack kernel of octave 0 alone
nwords = (n ** 3 + 63) // 64
d_bits = dev.malloc(nwords * 8)
ev = [C.c_void_p(), C.c_void_p()]
for e in ev:
    dev.check(dev.L.s3d_rt_event_create(C.byref(e)))
# three masks in turn (3 n^3 bytes: at 512^3 more than the 256 MB last-level cache holds), so that no launch reads what the
# one before left there
d_srcs = [dev.upload(masks["b"][1]), d_ball, dev.upload(masks["d"][1])]
for i in range(3):
    dev.mask_pack(d_srcs[i], n, n, (n, n, n), 0, d_bits)
dev.sync()
dev.check(dev.L.s3d_rt_event_record(ev[0], None))
for i in range(args.pack_reps):
    dev.mask_pack(d_srcs[i % 3], n, n, (n, n, n), 0, d_bits)
dev.check(dev.L.s3d_rt_event_record(ev[1], None))
el = C.c_float()
dev.check(dev.L.s3d_rt_event_elapsed_ms(ev[0], ev[1], C.byref(el)))
us = max(el.value, 1e-6) * 1e3 / args.pack_reps
floor = n ** 3 / COPY_CEILING * 1e6
print(f"s3d_k_mask_pack, octave 0 ({n ** 3} bytes read, {nwords * 8} written): {us:.1f} us per launch over {args.pack_reps} "
      f"back-to-back launches over three masks in turn = {n ** 3 / us / 1e6:.2f} TB/s read; the read alone at the copy ceiling (6.29 TB/s): {floor:.1f} us "
      f"-> {floor / us:.2f} of it")
dev.mask_pack(d_ball, n, n, (n, n, n), 0, d_bits)
got = dev.download(d_bits, (nwords,), np.uint64)
assert np.array_equal(got.view(np.uint8), np.packbits(ball.ravel() != 0, bitorder="little")), "pack kernel result"
