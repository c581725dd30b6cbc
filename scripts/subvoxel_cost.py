#!/usr/bin/env python3
"""GPU-box helper: what sub-voxel refinement (sift3d_amd_set_subvoxel) costs.  One process, the benchmark's 512^3 volume
resident in HBM, one struct per form with its setting made once, the forms alternated step by step after a warm-up; host
clock around calls that end synchronised (the detect returns with its keypoints on the host, the descriptor call is followed
by a stream synchronise):

  (a) refinement off      (b) refinement on

detect ms and describe ms (sift3d_amd_extract_descriptors_dev: records stay in HBM) of each -- refined keypoints leave the
descriptor kernel's integer-centre weight table, so (b)'s describe is expected to rise -- and from the same calls the time of
s3d_k_refine_keys by HIP events on the detect's stream (sift3d_amd_set_subvoxel_events).

With --parent-lib the unrefined detect of this build and of another build of the library (the parent commit's) are first
alternated in child processes of their own (SIFT3D_AMD_LIB names the library), before this process opens the GPU.

    python scripts/subvoxel_cost.py [--n 512] [--steps 20] [--warmup 3] [--parent-lib PATH] [--out profiles/subvoxel_cost.txt]
"""
import argparse
import ctypes as C
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=512)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--parent-lib", default=None, help="libsift3d_amd.so of the parent commit: alternate the unrefined detect with it")
ap.add_argument("--ab-rounds", type=int, default=3)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "subvoxel_cost.txt"))
ap.add_argument("--ab-child", action="store_true", help=argparse.SUPPRESS)
args = ap.parse_args()
n = args.n
lines = []


def say(text=""):
    print(text, flush=True)
    lines.append(text)


if args.parent_lib:
    this_lib = os.path.join(ROOT, "sift3d_amd", "lib", "libsift3d_amd.so")
    say(f"unrefined detect, this build against the parent's: {args.ab_rounds} alternated pairs of child processes "
        f"({n}^3 in HBM, 10 timed calls each after 2 dropped)")
    for r in range(args.ab_rounds):
        for who, path in (("parent", os.path.abspath(args.parent_lib)), ("this", this_lib)):
            env = dict(os.environ, SIFT3D_AMD_LIB=path)
            env.pop("SIFT3D_SUBVOXEL", None)
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--ab-child", "--n", str(n)], env=env,
                               capture_output=True, text=True, timeout=600)
            if p.returncode != 0:
                sys.exit(f"the child process ({who}) failed:\n{p.stdout}{p.stderr}")
            say(f"  round {r} {who:<6} {p.stdout.strip()}")
    say()

import sift3d_amd                                  # noqa: E402
from sift3d_amd import abi, synth                  # noqa: E402

lib = sift3d_amd.load()
dev = sift3d_amd.load_device()
L = lib.sift
vol = synth.blobs(n, n, n, synth.default_nblobs(n, n, n), 0)
d_vol = dev.upload(vol)
if args.ab_child:
    # the unrefined detect of the library SIFT3D_AMD_LIB names: 12 calls, the first two dropped
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

forms = {"a": ("refinement off", False), "b": ("refinement on", True)}
kp = abi.Keypoint_store()
L.init_Keypoint_store(C.byref(kp))
structs = {}
for k, (_, on) in forms.items():
    s = abi.SIFT3D()
    assert L.init_SIFT3D(C.byref(s)) == 0
    assert abi.set_subvoxel(L, s, on) == 0, L.sift3d_amd_last_error()
    structs[k] = s
ev = [C.c_void_p(), C.c_void_p()]
for e in ev:
    dev.check(dev.L.s3d_rt_event_create(C.byref(e)))
L.sift3d_amd_set_subvoxel_events.argtypes = [C.c_void_p] * 2
L.sift3d_amd_set_subvoxel_events.restype = None

det, des = ({k: [] for k in forms} for _ in range(2))
ref = []
cand, keys, fits = {}, {}, {}
d_desc = C.c_void_p()
el = C.c_float()
for step in range(args.warmup + args.steps):
    for k in forms:
        s = structs[k]
        L.sift3d_amd_set_subvoxel_events(ev[0], ev[1])
        t0 = time.perf_counter()
        rc = L.sift3d_amd_detect_keypoints_dev(C.byref(s), C.c_void_p(d_vol), n, n, n, 1.0, 1.0, 1.0, C.byref(kp))
        t1 = time.perf_counter()
        L.sift3d_amd_set_subvoxel_events(None, None)
        assert rc == 0, (k, L.sift3d_amd_last_error())
        rc = L.sift3d_amd_extract_descriptors_dev(C.byref(s), C.byref(kp), C.byref(d_desc))
        dev.sync()
        t2 = time.perf_counter()
        assert rc == 0, (k, L.sift3d_amd_last_error())
        cand[k], keys[k], fits[k] = L.sift3d_amd_last_num_candidates(C.byref(s)), int(kp.slab.num), abi.last_subvoxel_counts(L, s)
        if step >= args.warmup:
            det[k].append((t1 - t0) * 1e3)
            des[k].append((t2 - t1) * 1e3)
            if forms[k][1]:
                dev.check(dev.L.s3d_rt_event_elapsed_ms(ev[0], ev[1], C.byref(el)))
                ref.append(el.value)

med = statistics.median
say(f"sub-voxel refinement cost: {n}^3 in HBM, {args.steps} alternated steps per form after {args.warmup} warm-up steps; ms per call; "
    f"refine kernel: HIP events on the detect's stream, inside the same calls")
say(f"{'form':<20} {'detect med':>10} {'min':>7} {'max':>7} {'describe med':>12} {'min':>7} {'max':>7} {'candidates':>10} "
    f"{'keypoints':>9} {'3-D fits':>9} {'fallback':>9}")
for k, (name, _) in forms.items():
    say(f"({k}) {name:<16} {med(det[k]):>10.3f} {min(det[k]):>7.3f} {max(det[k]):>7.3f} {med(des[k]):>12.3f} {min(des[k]):>7.3f} "
        f"{max(des[k]):>7.3f} {cand[k]:>10d} {keys[k]:>9d} {fits[k][0]:>9d} {fits[k][1]:>9d}")
say(f"s3d_k_refine_keys (grid over {cand['b']} candidate slots, {keys['b']} records): median {med(ref):.4f} ms, min {min(ref):.4f}, "
    f"max {max(ref):.4f}")
say(f"spread of (a)'s detect over its own repeats: {max(det['a']) - min(det['a']):.3f} ms")
say(f"(b): detect - (a) = {med(det['b']) - med(det['a']):+.3f} ms; describe / (a) = {med(des['b']) / med(des['a']):.3f}; "
    f"detect + describe: {med(det['a']) + med(des['a']):.2f} -> {med(det['b']) + med(des['b']):.2f} ms")
assert cand["a"] == cand["b"] and keys["a"] == keys["b"], "refinement does not change the list"
assert fits["a"] == (0, 0) and sum(fits["b"]) == keys["b"]
os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
