#!/usr/bin/env python3
"""GPU-box helper: what a keypoint budget (sift3d_amd_set_max_keypoints) saves, and what it costs.  One process, the
benchmark's 512^3 volume resident in HBM, one struct per form with its budget set once, the forms alternated step by step
after a warm-up; host clock around calls that end synchronised (the detect returns with its keypoints on the host, the
descriptor call is followed by a stream synchronise):

  (a) no budget      (b) a budget of `--all` (everything survives)      (c) 10 000      (d) 5 000      (e) 1 000

detect ms and describe ms (sift3d_amd_extract_descriptors_dev: records stay in HBM) of each, and from the same calls the time
of the orientation step and of the strength + selection kernels behind it by HIP events on the detect's stream
(sift3d_amd_set_orient_events).

With --parent-lib the unbudgeted detect of this build and of another build of the library (the parent commit's) are first
alternated in child processes of their own (SIFT3D_AMD_LIB names the library), before this process opens the GPU.

    python scripts/keypoint_budget_cost.py [--n 512] [--steps 20] [--warmup 3] [--parent-lib PATH] > profiles/keypoint_budget_cost.txt
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
ap.add_argument("--all", type=int, default=31207, help="the budget of form (b): the keypoint count of the unbudgeted detect")
ap.add_argument("--parent-lib", default=None, help="libsift3d_amd.so of the parent commit: alternate the unbudgeted detect with it")
ap.add_argument("--ab-rounds", type=int, default=3)
ap.add_argument("--ab-child", action="store_true", help=argparse.SUPPRESS)
args = ap.parse_args()
n = args.n

if args.parent_lib:
    this_lib = os.path.join(ROOT, "sift3d_amd", "lib", "libsift3d_amd.so")
    print(f"unbudgeted detect, this build against the parent's: {args.ab_rounds} alternated pairs of child processes "
          f"({n}^3 in HBM, 10 timed calls each after 2 dropped)")
    for r in range(args.ab_rounds):
        for who, path in (("parent", os.path.abspath(args.parent_lib)), ("this", this_lib)):
            env = dict(os.environ, SIFT3D_AMD_LIB=path)
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--ab-child", "--n", str(n)], env=env,
                               capture_output=True, text=True, timeout=600)
            if p.returncode != 0:
                sys.exit(f"the child process ({who}) failed:\n{p.stdout}{p.stderr}")
            print(f"  round {r} {who:<6} {p.stdout.strip()}", flush=True)
    print()

import sift3d_amd                                  # noqa: E402
from sift3d_amd import abi, synth                  # noqa: E402

lib = sift3d_amd.load()
dev = sift3d_amd.load_device()
L = lib.sift
vol = synth.blobs(n, n, n, synth.default_nblobs(n, n, n), 0)
d_vol = dev.upload(vol)
if args.ab_child:
    # the unbudgeted detect of the library SIFT3D_AMD_LIB names: 12 calls, the first two dropped
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

forms = {"a": ("no budget", 0), "b": (f"budget {args.all}", args.all), "c": ("budget 10000", 10000), "d": ("budget 5000", 5000),
         "e": ("budget 1000", 1000)}
kp = abi.Keypoint_store()
L.init_Keypoint_store(C.byref(kp))
structs = {}
for k, (_, budget) in forms.items():
    s = abi.SIFT3D()
    assert L.init_SIFT3D(C.byref(s)) == 0
    assert abi.set_max_keypoints(L, s, budget) == 0, L.sift3d_amd_last_error()
    structs[k] = s
ev = [C.c_void_p(), C.c_void_p(), C.c_void_p()]
for e in ev:
    dev.check(dev.L.s3d_rt_event_create(C.byref(e)))
L.sift3d_amd_set_orient_events.argtypes = [C.c_void_p] * 3
L.sift3d_amd_set_orient_events.restype = None

det, des, ori, sel = ({k: [] for k in forms} for _ in range(4))
cand, keys = {}, {}
d_desc = C.c_void_p()
el = C.c_float()
for step in range(args.warmup + args.steps):
    for k in forms:
        s = structs[k]
        L.sift3d_amd_set_orient_events(ev[0], ev[1], ev[2])
        t0 = time.perf_counter()
        rc = L.sift3d_amd_detect_keypoints_dev(C.byref(s), C.c_void_p(d_vol), n, n, n, 1.0, 1.0, 1.0, C.byref(kp))
        t1 = time.perf_counter()
        L.sift3d_amd_set_orient_events(None, None, None)
        assert rc == 0, (k, L.sift3d_amd_last_error())
        rc = L.sift3d_amd_extract_descriptors_dev(C.byref(s), C.byref(kp), C.byref(d_desc))
        dev.sync()
        t2 = time.perf_counter()
        assert rc == 0, (k, L.sift3d_amd_last_error())
        cand[k], keys[k] = L.sift3d_amd_last_num_candidates(C.byref(s)), int(kp.slab.num)
        if step >= args.warmup:
            det[k].append((t1 - t0) * 1e3)
            des[k].append((t2 - t1) * 1e3)
            dev.check(dev.L.s3d_rt_event_elapsed_ms(ev[0], ev[1], C.byref(el)))
            ori[k].append(el.value)
            dev.check(dev.L.s3d_rt_event_elapsed_ms(ev[1], ev[2], C.byref(el)))
            sel[k].append(el.value)

med = statistics.median
print(f"keypoint budget cost: {n}^3 in HBM, {args.steps} alternated steps per form after {args.warmup} warm-up steps; ms per call; "
      f"orientation and selection: HIP events on the detect's stream, inside the same calls")
print(f"{'form':<20} {'detect med':>10} {'min':>7} {'max':>7} {'describe med':>12} {'min':>7} {'max':>7} {'orient med':>10} "
      f"{'select med':>10} {'min':>7} {'max':>7} {'candidates':>10} {'keypoints':>9}")
for k, (name, _) in forms.items():
    print(f"({k}) {name:<16} {med(det[k]):>10.3f} {min(det[k]):>7.3f} {max(det[k]):>7.3f} {med(des[k]):>12.3f} {min(des[k]):>7.3f} "
          f"{max(des[k]):>7.3f} {med(ori[k]):>10.3f} {med(sel[k]):>10.4f} {min(sel[k]):>7.4f} {max(sel[k]):>7.4f} {cand[k]:>10d} "
          f"{keys[k]:>9d}")
md = {k: med(v) for k, v in det.items()}
ms = {k: med(v) for k, v in des.items()}
print(f"spread of (a)'s detect over its own repeats: {max(det['a']) - min(det['a']):.3f} ms")
for k in ("b", "c", "d", "e"):
    print(f"({k}): detect - (a) = {md[k] - md['a']:+.3f} ms; selection / orientation = {med(sel[k]) / med(ori[k]):.3f}; "
          f"describe / (a) = {ms[k] / ms['a']:.3f} for keypoints / (a) = {keys[k] / keys['a']:.3f}; "
          f"detect + describe: {md['a'] + ms['a']:.2f} -> {md[k] + ms[k]:.2f} ms")
assert len(set(cand.values())) == 1, "the budget does not change the candidates"
assert keys["b"] == keys["a"] and all(keys[k] == min(forms[k][1], keys["a"]) for k in "cde")
