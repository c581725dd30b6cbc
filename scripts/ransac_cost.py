#!/usr/bin/env python3
"""GPU-box helper: what scoring the RANSAC hypotheses on the device saves, and where it starts to pay.  find_tform_ransac on
synthetic matches (as tests/test_reg.py::_points: noisy images of random points under one affine map, 50 % outliers) over the grid

    npts in {60, 200, 2000, 12485, 17874, 35000}  x  num_iter in {500, 5000, 50000},   err_thresh 5, srand(1) before every call

Part 1 (with --parent-lib): the default form of this build (AUTO) against another build of the library (the parent commit's),
each in child processes of its own (SIFT3D_AMD_LIB names the library), alternated round by round.  This is the yardstick for
what a caller gains.
Part 2: the forms of this build -- forced HOST, forced DEVICE -- alternated call by call in one process, with the device-side
share of the DEVICE form (HIP events inside the call: sift3d_amd_set_ransac_profile).  The AUTO threshold is read off this part:
the smallest npts * num_iter at which DEVICE beats HOST by more than HOST's own min-max spread, rounded up to a power of two.

Host clock around the call; medians and min-max over --steps repeats per form, fewer where one call is long: a grid point gets at
most --budget seconds per form (never fewer than 3 repeats), and the table says how many it got.

    python scripts/ransac_cost.py [--steps 20] [--budget 3] [--parent-lib PATH] > profiles/ransac_cost.txt
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--budget", type=float, default=3.0, help="seconds per grid point and form")
ap.add_argument("--npts", type=int, nargs="*", default=[60, 200, 2000, 12485, 17874, 35000])
ap.add_argument("--num-iter", type=int, nargs="*", default=[500, 5000, 50000])
ap.add_argument("--parent-lib", default=None, help="libsift3d_amd.so of the parent commit")
ap.add_argument("--ab-rounds", type=int, default=2)
ap.add_argument("--ab-child", action="store_true", help=argparse.SUPPRESS)
args = ap.parse_args()
args.warmup = max(1, args.warmup)
GRID = [(n, k) for n in args.npts for k in args.num_iter]
A_TRUE = np.array([[1.02, 0.03, -0.01, 4.0], [-0.02, 0.97, 0.05, -3.0], [0.01, -0.04, 1.01, 2.5]])
med = statistics.median


def points(n, seed):
    rng = np.random.default_rng(seed)
    ref = rng.random((n, 3)) * 100
    src = ref @ A_TRUE[:, :3].T + A_TRUE[:, 3] + rng.standard_normal((n, 3)) * 0.3
    bad = rng.choice(n, n // 2, replace=False)
    src[bad] = rng.random((n // 2, 3)) * 100
    return src, ref


def fmt(ts):
    return f"{med(ts):>10.3f} {min(ts):>9.3f} {max(ts):>9.3f}"


if args.parent_lib and not args.ab_child:
    # before this process opens the GPU
    this_lib = os.path.join(ROOT, "sift3d_amd", "lib", "libsift3d_amd.so")
    per_round = max(1, args.steps // args.ab_rounds)
    res = {"parent": {}, "this": {}}
    paths = {}
    for r in range(args.ab_rounds):
        for who, path in (("parent", os.path.abspath(args.parent_lib)), ("this", this_lib)):
            env = dict(os.environ, SIFT3D_AMD_LIB=path)
            env.pop("SIFT3D_RANSAC_DEVICE", None)
            cmd = [sys.executable, os.path.abspath(__file__), "--ab-child", "--steps", str(per_round), "--warmup", str(args.warmup),
                   "--budget", str(args.budget / args.ab_rounds), "--npts", *map(str, args.npts), "--num-iter", *map(str, args.num_iter)]
            p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=1100)
            if p.returncode != 0:
                sys.exit(f"the child process ({who}, round {r}) failed:\n{p.stdout[-2000:]}{p.stderr[-2000:]}")
            for line in p.stdout.splitlines():
                if line.startswith("{"):
                    rec = json.loads(line)
                    key = (rec["npts"], rec["num_iter"])
                    res[who].setdefault(key, []).extend(rec["ms"])
                    if who == "this":
                        paths[key] = rec["path"]
    print(f"part 1: find_tform_ransac of this build as a caller gets it (AUTO) against the parent's, {args.ab_rounds} alternated pairs of "
          f"child processes; ms per call")
    print(f"{'npts':>6} {'num_iter':>8} {'n':>3} {'parent med':>10} {'min':>9} {'max':>9} {'this med':>10} {'min':>9} {'max':>9} "
          f"{'path':>6} {'this - parent':>13} {'larger spread':>13}")
    for key in GRID:
        a, b = res["parent"][key], res["this"][key]
        spread = max(max(a) - min(a), max(b) - min(b))
        print(f"{key[0]:>6d} {key[1]:>8d} {len(a):>3d} {fmt(a)} {fmt(b)} {'device' if paths[key] else 'host':>6} "
              f"{med(b) - med(a):>+13.3f} {spread:>13.3f}")
    print(flush=True)

import sift3d_amd                                  # noqa: E402
from sift3d_amd import abi                         # noqa: E402

lib = sift3d_amd.load()
u = lib.imutil
libc = C.CDLL(None)
P = C.POINTER
u.init_Mat_rm.argtypes = [P(abi.Mat_rm), C.c_int, C.c_int, C.c_int, C.c_int]
u.init_tform.argtypes = [C.c_void_p, C.c_int]
u.init_Ransac.argtypes = [P(abi.Ransac)]
u.init_Ransac.restype = None
u.find_tform_ransac.argtypes = [P(abi.Ransac), P(abi.Mat_rm), P(abi.Mat_rm), C.c_void_p]
have_knob = hasattr(u, "sift3d_amd_set_ransac_device")


def mat(a):
    a = np.ascontiguousarray(a, np.float64)
    m = abi.Mat_rm()
    assert u.init_Mat_rm(C.byref(m), a.shape[0], a.shape[1], 0, 0) == 0
    C.memmove(m.data, a.ctypes.data, a.nbytes)
    return m


def call(ran, ms, mr, t, mode):
    if mode is not None:
        assert u.sift3d_amd_set_ransac_device(mode) == 0
    libc.srand(1)
    t0 = time.perf_counter()
    rc = u.find_tform_ransac(C.byref(ran), C.byref(ms), C.byref(mr), C.byref(t))
    dt = (time.perf_counter() - t0) * 1e3
    assert rc == 0, (mode, u.sift3d_amd_last_error())
    A = np.ctypeslib.as_array(C.cast(t.A.data, P(C.c_double)), (3, 4)).copy()
    return dt, A


def measure(npts, num_iter, modes, steps, budget):
    """the forms alternated call by call -> {mode: [ms]}, {mode: [device ms]}, {mode: last_path}, repeats"""
    src, ref = points(npts, npts)
    ms, mr = mat(src), mat(ref)
    t = abi.Affine()
    assert u.init_tform(C.byref(t), 0) == 0
    ran = abi.Ransac()
    u.init_Ransac(C.byref(ran))
    ran.num_iter = num_iter
    ts, dev_ms, path, mats = ({m: [] for m in modes} for _ in range(4))
    first = {}
    for _ in range(args.warmup):
        for m in modes:
            first[m], mats[m] = call(ran, ms, mr, t, m)
    n = max(3, min(steps, int(budget * 1e3 / max(first.values()))))
    for _ in range(n):
        for m in modes:
            dt, A = call(ran, ms, mr, t, m)
            ts[m].append(dt)
            assert np.array_equal(A, mats[m]), "the same seed gives the same transform"
            if have_knob:
                dev_ms[m].append(u.sift3d_amd_ransac_last_device_ms())
                path[m] = u.sift3d_amd_ransac_last_path()
    ref_m = modes[0]
    for m in modes[1:]:
        assert np.array_equal(mats[m], mats[ref_m]), "the forms return the same transform, bit for bit"
    u.cleanup_Mat_rm(C.byref(ms)), u.cleanup_Mat_rm(C.byref(mr)), u.cleanup_tform(C.byref(t))
    return ts, dev_ms, path, n


if args.ab_child:
    # the default form of the library SIFT3D_AMD_LIB names (the parent has no knob: its only form)
    for npts, num_iter in GRID:
        ts, _, path, n = measure(npts, num_iter, [None], args.steps, args.budget)
        print(json.dumps({"npts": npts, "num_iter": num_iter, "ms": ts[None],
                          "path": u.sift3d_amd_ransac_last_path() if have_knob else 0}), flush=True)
    sys.exit(0)

HOST, DEVICE = 0, 1
u.sift3d_amd_set_ransac_profile(1)
print(f"part 2: this build, forced HOST and forced DEVICE alternated call by call in one process (up to {args.steps} repeats per form "
      f"after {args.warmup} warm-up, at most {args.budget:g} s per grid point and form); ms per call; device ms: HIP events around the "
      f"transfers and kernels inside the DEVICE calls")
print(f"{'npts':>6} {'num_iter':>8} {'work':>11} {'n':>3} {'HOST med':>10} {'min':>9} {'max':>9} {'DEVICE med':>10} {'min':>9} {'max':>9} "
      f"{'device ms':>9} {'HOST - DEVICE':>13} {'HOST spread':>11} {'pays':>4}")
pays = []
for npts, num_iter in sorted(GRID, key=lambda g: g[0] * g[1]):
    ts, dev_ms, path, n = measure(npts, num_iter, [HOST, DEVICE], args.steps, args.budget)
    assert path[HOST] == 0 and path[DEVICE] == 1
    gain, spread = med(ts[HOST]) - med(ts[DEVICE]), max(ts[HOST]) - min(ts[HOST])
    if gain > spread:
        pays.append(npts * num_iter)
    print(f"{npts:>6d} {num_iter:>8d} {npts * num_iter:>11d} {n:>3d} {fmt(ts[HOST])} {fmt(ts[DEVICE])} {med(dev_ms[DEVICE]):>9.3f} "
          f"{gain:>+13.3f} {spread:>11.3f} {'yes' if gain > spread else 'no':>4}", flush=True)
u.sift3d_amd_set_ransac_device(-1)
u.sift3d_amd_set_ransac_profile(0)
if pays:
    w = min(pays)
    print(f"\nsmallest measured npts * num_iter at which DEVICE beats HOST by more than HOST's spread: {w}; "
          f"rounded up to a power of two: {1 << (w - 1).bit_length()} = 2^{(w - 1).bit_length()}")
else:
    print("\nDEVICE beats HOST by more than HOST's spread nowhere on this grid")
