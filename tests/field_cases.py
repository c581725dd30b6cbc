"""Shared by tests/test_field.py (CPU: the SIMT emulator build of the library) and tests/test_gpu_field.py (the device): the inputs
of the field inversion and of the Jacobian determinant (s3d_k_field_invert, s3d_k_field_jacobian, sift3d_amd_invert_field,
sift3d_amd_field_jacobian, sift3d_amd_field_apply_points), a numpy restatement of both kernels' definitions
(include/s3d_device.h) and the checks both suites apply.

The restatement forms every term with the operation order the header states, as element-wise f64 numpy operations: each is
rounded once and nothing is fused, as in the kernels (compiled without contraction), so an inverse field entry, a status byte and
a determinant are reproduced bit for bit, the counts exactly, and the f64 sums obey the bound of any summation order,
n * 2^-53 * sum |term|.  The meaning of the inverse -- phi(psi(y)) = y -- is checked apart from the restatement, by composing the
two maps in numpy."""
import ctypes as C
import math
import os
import subprocess

import numpy as np

from sift3d_amd import abi
from tests import demons_cases as dc
from tests import similarity_cases as sc

P = C.POINTER
MAX_ITER, TOL = 30, 1e-3
# (reference dims, source dims): the project's two awkward shapes and the demons pair
GRIDS = {"70x33x9": sc.SHAPES["70x33x9"][:2], "257x19x5": sc.SHAPES["257x19x5"][:2], "48x44x40": (dc.RDIMS, dc.RDIMS)}
AMPS = (1.5, 10.0)
NAN_WORD = 0x7FC00000
_CACHE = {}


def inverse34(A):
    """the inverse of a 3 x 4 map as a 3 x 4 map (numpy's; the kernel takes whatever inverse its caller computed)"""
    A = np.asarray(A, np.float64)
    L = np.linalg.inv(A[:, :3])
    return np.ascontiguousarray(np.hstack([L, -(L @ A[:, 3:])]))


def sine(grid, amp):
    """demons_cases.sine_field over the grid's reference, rounded to f32: three [z, y, x] components"""
    key = ("sine", grid, amp)
    if key not in _CACHE:
        u = tuple(np.ascontiguousarray(c, np.float32) for c in dc.sine_field(GRIDS[grid][0], amp))
        for c in u:
            c.setflags(write=False)
        _CACHE[key] = u
    return _CACHE[key]


# ---- numpy restatement of the kernels ---------------------------------------------------------------------------------------
def trilinear_f64(comp, q):
    """s3d_sample_store<linear>'s expression at q (inside the grid) in f64, before its rounding to float"""
    tx, ty, tz = q
    fx, fy, fz = (np.floor(c).astype(np.int64) for c in (tx, ty, tz))
    cx, cy, cz = (np.ceil(c).astype(np.int64) for c in (tx, ty, tz))
    dx, dy, dz = tx - fx, ty - fy, tz - fz
    s = comp.astype(np.float64)
    c0, c1, c2, c3 = s[fz, fy, fx], s[fz, cy, fx], s[fz, fy, cx], s[fz, cy, cx]
    c4, c5, c6, c7 = s[cz, fy, fx], s[cz, cy, fx], s[cz, fy, cx], s[cz, cy, cx]
    with np.errstate(invalid="ignore", over="ignore"):
        return (c0 * (1.0 - dx) * (1.0 - dy) * (1.0 - dz) + c1 * (1.0 - dx) * dy * (1.0 - dz) +
                c2 * dx * (1.0 - dy) * (1.0 - dz) + c3 * dx * dy * (1.0 - dz) +
                c4 * (1.0 - dx) * (1.0 - dy) * dz + c5 * (1.0 - dx) * dy * dz +
                c6 * dx * (1.0 - dy) * dz + c7 * dx * dy * dz)


def clamp(p, rdims):
    return tuple(np.where(c < 0, 0.0, np.where(c > n - 1, float(n - 1), c)) for c, n in zip(p, rdims))


class InvertWant:
    """s3d_k_field_invert restated, steps 1 to 7 of the header: w (3 x n float32, its bits), status (n bytes), k per voxel, the
    residual sqrt(e2) of the voxels that are not invalid"""

    def __init__(self, u, A, B, sdims, max_iter=MAX_ITER, tol=TOL):
        A, B = np.asarray(A, np.float64), np.asarray(B, np.float64)
        rdims = u[0].shape[::-1]
        n = sdims[0] * sdims[1] * sdims[2]
        p0 = np.stack([c.reshape(-1) for c in sc.affine_coords(B, sdims)])
        w, k, st, e2_end = np.zeros((3, n)), np.zeros(n, np.int64), np.full(n, 255, np.uint8), np.zeros(n)
        act = np.arange(n)
        tol2 = tol * tol
        with np.errstate(invalid="ignore", over="ignore"):
            while act.size:
                wa = w[:, act]
                p = p0[:, act] + wa
                fin = np.isfinite(p).all(0)
                q = tuple(np.where(fin, c, 0.0) for c in clamp(p, rdims))
                s = np.stack([trilinear_f64(u[c], q) for c in range(3)])
                valid = fin & np.isfinite(s).all(0)
                r = [((A[i, 0] * wa[0] + A[i, 1] * wa[1]) + A[i, 2] * wa[2]) + s[i] for i in range(3)]
                e2 = (r[0] * r[0] + r[1] * r[1]) + r[2] * r[2]
                conv = valid & (e2 <= tol2)
                inside = (q[0] == p[0]) & (q[1] == p[1]) & (q[2] == p[2])
                stop = valid & ~conv & (k[act] == max_iter)
                go = valid & ~conv & ~stop
                st[act[~valid]] = 3
                st[act[conv]] = np.where(inside[conv], 0, 1)
                st[act[stop]] = 2
                e2_end[act[conv | stop]] = e2[conv | stop]
                for i in range(3):
                    w[i, act[go]] = -((B[i, 0] * s[0] + B[i, 1] * s[1]) + B[i, 2] * s[2])[go]
                k[act[go]] += 1
                act = act[go]
            wf = w.astype(np.float32)
        bits = wf.view(np.uint32).copy()
        bits[:, st == 3] = NAN_WORD
        self.bits, self.status, self.k = bits, st, k
        self.counts = tuple(int((st == v).sum()) for v in range(4))
        self.updates = int(k.sum())
        self.e2 = e2_end[st != 3]
        self.res = np.sqrt(self.e2)
        self.n = n

    @property
    def w(self):
        return self.bits.view(np.float32)


def invert_want(grid, amp):
    key = ("invert", grid, amp)
    if key not in _CACHE:
        _CACHE[key] = InvertWant(sine(grid, amp), sc.A_FIXED, inverse34(sc.A_FIXED), GRIDS[grid][1])
    return _CACHE[key]


def axis_diff(c, axis):
    """central differences times 0.5 inside, one-sided on the two faces; c f64 [z, y, x], axis 0 = x"""
    c = np.moveaxis(c, 2 - axis, 0)
    g = np.empty_like(c)
    g[1:-1] = (c[2:] - c[:-2]) * 0.5
    g[0] = c[1] - c[0]
    g[-1] = c[-1] - c[-2]
    return np.moveaxis(g, 0, 2 - axis)


class JacobianWant:
    """s3d_k_field_jacobian restated: the determinant as f64 and as the stored float, and the statistics over the finite ones"""

    def __init__(self, u, A):
        A = np.asarray(A, np.float64)
        with np.errstate(invalid="ignore", over="ignore"):
            J = [[A[i, a] + axis_diff(np.asarray(u[i], np.float32).astype(np.float64), a) for a in range(3)] for i in range(3)]
            det = ((J[0][0] * (J[1][1] * J[2][2] - J[1][2] * J[2][1]) - J[0][1] * (J[1][0] * J[2][2] - J[1][2] * J[2][0])) +
                   J[0][2] * (J[1][0] * J[2][1] - J[1][1] * J[2][0]))
            self.map = det.astype(np.float32)
        fin = np.isfinite(det)
        f = det[fin]
        self.det, self.n_finite, self.n_folded = det, int(fin.sum()), int((f <= 0).sum())
        self.sum, self.mag = math.fsum(f), math.fsum(np.abs(f))
        self.min, self.max = (float(f.min()), float(f.max())) if f.size else (math.nan, math.nan)


def jacobian_want(grid, amp):
    key = ("jacobian", grid, amp)
    if key not in _CACHE:
        _CACHE[key] = JacobianWant(sine(grid, amp), sc.A_FIXED)
    return _CACHE[key]


# ---- drivers of the kernels -------------------------------------------------------------------------------------------------
def kernel_invert(dev, u, A, B, sdims, max_iter=MAX_ITER, tol=TOL, with_status=True):
    """s3d_k_field_invert on dev -> (w bits 3 x n uint32, status bytes or None, the statistics of DeviceLib.field_invert)"""
    rd = u[0].shape[::-1]
    n = sdims[0] * sdims[1] * sdims[2]
    flat = dc.planar(u)
    bufs = [dev.upload(flat), dev.upload(np.full(3 * n, -3.5, np.float32))]
    if with_status:
        bufs.append(dev.upload(np.full(n, 0xEE, np.uint8)))
    try:
        stats = dev.field_invert(bufs[0], rd, A, B, bufs[1], sdims, max_iter, tol, bufs[2] if with_status else None)
        w = dev.download(bufs[1], (3, n), np.float32).view(np.uint32)
        st = dev.download(bufs[2], (n,), np.uint8) if with_status else None
        assert np.array_equal(dc.bits(dev.download(bufs[0], flat.shape, np.float32)), dc.bits(flat))     # u is only read
        return w, st, stats
    finally:
        for b in bufs:
            dev.free(b)


def kernel_jacobian(dev, u, A, with_map=True):
    """s3d_k_field_jacobian on dev -> (the map [z, y, x] float32 or None, the statistics of DeviceLib.field_jacobian)"""
    rd = u[0].shape[::-1]
    n = rd[0] * rd[1] * rd[2]
    bufs = [dev.upload(dc.planar(u))]
    if with_map:
        bufs.append(dev.upload(np.full(n, -3.5, np.float32)))
    try:
        stats = dev.field_jacobian(bufs[0], rd, A, bufs[1] if with_map else None)
        return (dev.download(bufs[1], rd[::-1], np.float32) if with_map else None), stats
    finally:
        for b in bufs:
            dev.free(b)


def check_invert_stats(stats, w, label=""):
    """the four counts and the updates exactly; the residual sum within n * 2^-53 * sum |term| of math.fsum; the maximum to the
    rounding of one square root"""
    want_sum = math.fsum(w.res)
    bound = w.n * 2.0 ** -53 * want_sum
    want_max = float(w.res.max()) if w.res.size else 0.0
    print(f"{label} counts {stats['counts']} want {w.counts}; updates {stats['updates']} want {w.updates}; residual sum "
          f"{stats['sum_residual']!r} fsum {want_sum!r} bound {bound:.3e}; max {stats['max_residual']!r} want {want_max!r}")
    assert stats["counts"] == w.counts and sum(stats["counts"]) == w.n
    assert stats["updates"] == w.updates
    assert abs(stats["sum_residual"] - want_sum) <= bound
    assert abs(stats["max_residual"] - want_max) <= np.spacing(want_max)


def check_jacobian_stats(stats, w, label=""):
    n = w.det.size
    bound = n * 2.0 ** -53 * w.mag
    print(f"{label} finite {stats['n_finite']} want {w.n_finite}; folded {stats['n_folded']} want {w.n_folded}; sum {stats['sum']!r} "
          f"fsum {w.sum!r} bound {bound:.3e}; min {stats['min']!r} want {w.min!r}; max {stats['max']!r} want {w.max!r}")
    assert (stats["n_finite"], stats["n_folded"]) == (w.n_finite, w.n_folded)
    assert abs(stats["sum"] - w.sum) <= bound
    assert stats["min"] == w.min and stats["max"] == w.max


# ---- the cases both suites run (L: the library behind the C API, dev: its flat device entry points) --------------------------
def case_invert(dev, grid, amp):
    """the sine field under A_FIXED: every entry, every status byte and the statistics against the restatement, twice"""
    u, sdims = sine(grid, amp), GRIDS[grid][1]
    w = invert_want(grid, amp)
    present = set(np.unique(w.status).tolist())
    print(f"{grid} amp {amp}: most updates {int(w.k.max())}, counts {w.counts}")
    assert present == ({0, 1} if amp == 1.5 else {0, 1, 2})                  # conditions on the input
    B = inverse34(sc.A_FIXED)
    bits, st, stats = kernel_invert(dev, u, sc.A_FIXED, B, sdims)
    assert np.array_equal(st, w.status)
    assert np.array_equal(bits, w.bits)
    check_invert_stats(stats, w, f"{grid} amp {amp}")
    bits2, st2, stats2 = kernel_invert(dev, u, sc.A_FIXED, B, sdims)
    assert np.array_equal(bits, bits2) and np.array_equal(st, st2)
    assert stats == stats2 and np.float64(stats["sum_residual"]).tobytes() == np.float64(stats2["sum_residual"]).tobytes()


def case_invert_nonfinite(dev, shape):
    """demons_cases.random_field, with a NaN, an inf and a 1000 planted: the voxels whose iteration touches a non-finite entry are
    status 3 with NaN words, the same voxels as in the restatement; everything else bit for bit as well"""
    u, sdims = dc.random_field(shape), sc.SHAPES[shape][1]
    B = inverse34(sc.A_FIXED)
    key = ("nonfinite", shape)
    if key not in _CACHE:
        _CACHE[key] = InvertWant(u, sc.A_FIXED, B, sdims)
    w = _CACHE[key]
    bits, st, stats = kernel_invert(dev, u, sc.A_FIXED, B, sdims)
    bad = st == 3
    print(f"{shape}: {int(bad.sum())} invalid voxels, counts {stats['counts']}")
    assert 0 < int(bad.sum()) < st.size and np.array_equal(bad, w.status == 3)
    assert (bits[:, bad] == NAN_WORD).all() and np.isfinite(bits.view(np.float32)[:, ~bad]).all()
    assert np.array_equal(st, w.status) and np.array_equal(bits, w.bits)
    check_invert_stats(stats, w, shape)


def case_zero_field(dev, grid):
    """u == 0: all-zero bits, no update, every voxel converged"""
    rd, sd = GRIDS[grid]
    zero = tuple(np.zeros(rd[::-1], np.float32) for _ in range(3))
    for tol in (TOL, 0.0):
        bits, st, stats = kernel_invert(dev, zero, sc.A_FIXED, inverse34(sc.A_FIXED), sd, tol=tol)
        assert not bits.any() and stats["updates"] == 0 and set(np.unique(st).tolist()) <= {0, 1}
        assert stats["counts"][2] == 0 and stats["counts"][3] == 0 and stats["sum_residual"] == 0.0 and stats["max_residual"] == 0.0
        assert stats["counts"][0] > 0 and stats["counts"][1] > 0


def case_constant_field(dev):
    """the constant field (3, -2, 1) on the identity: every w is exactly (-3, 2, -1) after one update"""
    rd, sd = GRIDS["70x33x9"]
    const = tuple(np.full(rd[::-1], c, np.float32) for c in (3.0, -2.0, 1.0))
    n = sd[0] * sd[1] * sd[2]
    bits, st, stats = kernel_invert(dev, const, sc.A_IDENTITY, sc.A_IDENTITY, sd)
    w = bits.view(np.float32)
    assert (w[0] == -3.0).all() and (w[1] == 2.0).all() and (w[2] == -1.0).all()
    assert stats["updates"] == n and stats["counts"][2] == 0 and stats["counts"][3] == 0 and stats["max_residual"] == 0.0
    assert set(np.unique(st).tolist()) == {0, 1}


def case_max_iter_zero(dev):
    """max_iter = 0: w is zero bits, the status 2 wherever |u(B y)| > tol; d_status = NULL is accepted and changes nothing"""
    grid = "70x33x9"
    u, sd = sine(grid, 1.5), GRIDS[grid][1]
    B = inverse34(sc.A_FIXED)
    w = InvertWant(u, sc.A_FIXED, B, sd, max_iter=0)
    bits, st, stats = kernel_invert(dev, u, sc.A_FIXED, B, sd, max_iter=0)
    assert not bits.any() and stats["updates"] == 0
    far = w.e2 > TOL * TOL                                                  # (no voxel is invalid: e2 is per voxel)
    assert np.array_equal(st, w.status) and (st[far] == 2).all() and int((st == 2).sum()) == int(far.sum()) > 0
    check_invert_stats(stats, w, "max_iter 0")
    full = invert_want(grid, 1.5)
    bits, st, stats = kernel_invert(dev, u, sc.A_FIXED, B, sd, with_status=False)
    assert st is None and np.array_equal(bits, full.bits)
    check_invert_stats(stats, full, "no status")


def case_invert_guard(dev):
    """dirty buffers: nothing is written behind d_w, d_status or the partials, and the dirt does not reach the statistics"""
    grid = "257x19x5"
    u, (rd, sd) = sine(grid, 1.5), GRIDS[grid]
    L = dev.L
    n, guard = sd[0] * sd[1] * sd[2], 4096
    slots, nstat = int(L.s3d_k_field_invert_slots()), int(L.s3d_k_field_invert_stats())
    assert (slots, nstat) == (2048, 7)
    pbytes = slots * nstat * 8
    bufs = [dev.upload(dc.planar(u)), dev.malloc(12 * n + guard), dev.malloc(n + guard), dev.malloc(pbytes + guard)]
    dp = P(C.c_double)
    A, B = np.ascontiguousarray(sc.A_FIXED), inverse34(sc.A_FIXED)
    try:
        for b, size in zip(bufs[1:], (12 * n + guard, n + guard, pbytes + guard)):
            dev.check(L.s3d_rt_memset(b, 0xA5, size, None))
        dev.check(L.s3d_k_field_invert(bufs[0], *rd, A.ctypes.data_as(dp), B.ctypes.data_as(dp), bufs[1], *sd, MAX_ITER, TOL, bufs[2],
                                       bufs[3], None))
        dev.sync()
        bits = dev.download(bufs[1], (3, n), np.float32).view(np.uint32)
        st = dev.download(bufs[2], (n,), np.uint8)
        part = dev.download(bufs[3], (slots, nstat), np.float64)
        tails = [dev.download(b + size, (guard,), np.uint8) for b, size in zip(bufs[1:], (12 * n, n, pbytes))]
    finally:
        for b in bufs:
            dev.free(b)
    assert all((t == 0xA5).all() for t in tails)
    w = invert_want(grid, 1.5)
    assert np.array_equal(bits, w.bits) and np.array_equal(st, w.status)
    rows = sd[1] * sd[2]
    assert not part[rows:].any()                                            # the slots not used hold zeros
    assert tuple(int(part[:, k].sum()) for k in range(4)) == w.counts and int(part[:, 4].sum()) == w.updates


def case_invert_refusals(dev):
    """each refusal of the header: non-zero, a message, the outputs untouched"""
    grid = "70x33x9"
    u, (rd, sd) = sine(grid, 1.5), GRIDS[grid]
    L = dev.L
    n = sd[0] * sd[1] * sd[2]
    pbytes = int(L.s3d_k_field_invert_slots()) * int(L.s3d_k_field_invert_stats()) * 8
    bufs = [dev.upload(dc.planar(u)), dev.upload(np.full(3 * n, -7.5, np.float32)), dev.upload(np.full(n, 0xEE, np.uint8)),
            dev.upload(np.full(pbytes // 8, -7.5))]
    dp = P(C.c_double)
    A_, B_ = np.ascontiguousarray(sc.A_FIXED), inverse34(sc.A_FIXED)
    A, B = A_.ctypes.data_as(dp), B_.ctypes.data_as(dp)
    d_u, d_w, d_s, d_p = bufs
    try:
        for args in ((d_u, (0, 33, 9), A, B, d_w, sd, 30, 1e-3, d_s, d_p), (d_u, rd, A, B, d_w, (61, 0, 11), 30, 1e-3, d_s, d_p),
                     (d_u, rd, A, B, d_w, (61, 37, -1), 30, 1e-3, d_s, d_p), (None, rd, A, B, d_w, sd, 30, 1e-3, d_s, d_p),
                     (d_u, rd, None, B, d_w, sd, 30, 1e-3, d_s, d_p), (d_u, rd, A, None, d_w, sd, 30, 1e-3, d_s, d_p),
                     (d_u, rd, A, B, None, sd, 30, 1e-3, d_s, d_p), (d_u, rd, A, B, d_w, sd, 30, 1e-3, d_s, None),
                     (d_u, rd, A, B, d_w, sd, -1, 1e-3, d_s, d_p), (d_u, rd, A, B, d_w, sd, 30, -1e-3, d_s, d_p),
                     (d_u, rd, A, B, d_w, sd, 30, math.nan, d_s, d_p), (d_u, rd, A, B, d_w, (61, 65536, 11), 30, 1e-3, d_s, d_p),
                     (d_u, rd, A, B, d_w, (61, 37, 65536), 30, 1e-3, d_s, d_p)):
            a_u, a_rd, a_A, a_B, a_w, a_sd, a_it, a_tol, a_s, a_p = args
            assert L.s3d_k_field_invert(a_u, *a_rd, a_A, a_B, a_w, *a_sd, a_it, a_tol, a_s, a_p, None) != 0 and dev.err(), args
        dev.sync()
        assert (dev.download(d_w, (3 * n,), np.float32) == -7.5).all()
        assert (dev.download(d_s, (n,), np.uint8) == 0xEE).all()
        assert (dev.download(d_p, (pbytes // 8,), np.float64) == -7.5).all()
    finally:
        for b in bufs:
            dev.free(b)


def compose(u, A, B, wf, sdims):
    """phi(psi(y)) - y in numpy f64 for every source voxel: psi(y) = B y + (double)w, phi(x) = A x + the clamped tri-linear sample
    of u at x.  Independent of the restatement's iteration: plain matrix arithmetic on the returned float field."""
    A, B = np.asarray(A, np.float64), np.asarray(B, np.float64)
    rd = u[0].shape[::-1]
    z, y, x = np.meshgrid(*(np.arange(n, dtype=np.float64) for n in sdims[::-1]), indexing="ij")
    Y = np.stack([x.reshape(-1), y.reshape(-1), z.reshape(-1)])
    X = B[:, :3] @ Y + B[:, 3:] + wf.astype(np.float64)
    q = clamp(tuple(X), rd)
    s = np.stack([trilinear_f64(u[c], q) for c in range(3)])
    return A[:, :3] @ X + A[:, 3:] + s - Y, Y


def rounding_slack(u, A, wf):
    """What rounding w to float adds to |phi(psi(y)) - y|.  A component of w moves by at most h, half an ulp of the largest |w|.
    Component i of phi then moves by at most sum_a (|A_ia| + D_ia) h, D_ia the largest difference between neighbours of u_i along
    axis a (the slope of the tri-linear interpolant along an axis is a convex combination of such differences); the slack is the
    Euclidean length of these three bounds."""
    h = 0.5 * float(np.spacing(np.float32(np.abs(wf).max())))
    A = np.asarray(A, np.float64)
    per = [sum(abs(A[i, a]) + float(np.abs(np.diff(u[i].astype(np.float64), axis=2 - a)).max()) for a in range(3)) * h
           for i in range(3)]
    return math.sqrt(sum(v * v for v in per))


def case_meaning(dev):
    """48 x 44 x 40 at amp 1.5: the returned float field composed with the map, in numpy, is the identity to tol"""
    grid = "48x44x40"
    u, sd = sine(grid, 1.5), GRIDS[grid][1]
    B = inverse34(sc.A_FIXED)
    bits, st, _ = kernel_invert(dev, u, sc.A_FIXED, B, sd)
    wf = bits.view(np.float32)
    ok = st == 0
    assert ok.sum() > 0.5 * st.size and (st <= 1).all()
    r, _ = compose(u, sc.A_FIXED, B, np.where(np.isfinite(wf), wf, np.float32(0)), sd)
    err = np.sqrt((r * r).sum(0))[ok]
    none, _ = compose(u, sc.A_FIXED, B, np.zeros_like(wf), sd)               # the error of no inverse field at all
    err_none = float(np.sqrt((none * none).sum(0))[ok].mean())
    slack = rounding_slack(u, sc.A_FIXED, wf[:, ok])
    print(f"round trip over {int(ok.sum())} voxels: max {err.max()!r} against tol {TOL} + slack {slack:.3e} = {TOL + slack!r}; mean "
          f"{err.mean()!r}; no inverse field: mean {err_none!r}")
    assert err.max() <= TOL + slack
    assert err.mean() < 1e-3 and err.mean() < 1e-3 * err_none


def case_jacobian(dev, grid, amp):
    u = sine(grid, amp)
    w = jacobian_want(grid, amp)
    assert w.n_finite == w.det.size and (w.n_folded == 0 if amp == 1.5 else w.n_folded > 0)
    got, stats = kernel_jacobian(dev, u, sc.A_FIXED)
    assert np.array_equal(dc.bits(got), dc.bits(w.map))
    check_jacobian_stats(stats, w, f"{grid} amp {amp}")
    assert (stats["n_folded"] == 0) if amp == 1.5 else (stats["n_folded"] > 0)
    _, only = kernel_jacobian(dev, u, sc.A_FIXED, with_map=False)            # d_det = NULL: the same statistics
    assert only == stats
    _, again = kernel_jacobian(dev, u, sc.A_FIXED)
    assert again == stats


def case_jacobian_nonfinite(dev, shape):
    """random_field's NaN and inf entries: those determinants are stored as computed and left out of every statistic"""
    u = dc.random_field(shape)
    w = JacobianWant(u, sc.A_FIXED)
    assert 0 < w.n_finite < w.det.size
    got, stats = kernel_jacobian(dev, u, sc.A_FIXED)
    fin = np.isfinite(w.det)
    assert np.array_equal(dc.bits(got)[fin], dc.bits(w.map)[fin]) and np.array_equal(np.isnan(got), np.isnan(w.map))
    assert np.array_equal(np.isinf(got), np.isinf(w.map))
    check_jacobian_stats(stats, w, shape)


LINEAR_G = {"stretch": np.array([[0.25, -0.125, 0.0], [0.5, 0.375, -0.25], [0.125, 0.0, -0.5]]),
            "fold": np.array([[-2.5, 0.125, 0.0], [0.25, 0.5, 0.125], [0.0, -0.375, 0.25]])}


def case_jacobian_linear(dev, name, A):
    """u = G x, G's entries multiples of 1/8, so every entry and every difference is exact: every voxel, faces included, holds
    the float of the scalar formula on A + G"""
    G = LINEAR_G[name]
    rd = GRIDS["257x19x5"][0]
    z, y, x = np.meshgrid(*(np.arange(n, dtype=np.float64) for n in rd[::-1]), indexing="ij")
    u64 = tuple(G[i, 0] * x + G[i, 1] * y + G[i, 2] * z for i in range(3))
    u = tuple(c.astype(np.float32) for c in u64)
    assert all(np.array_equal(a.astype(np.float64), b) for a, b in zip(u, u64))
    J = np.asarray(A, np.float64)[:, :3] + G
    det = ((J[0, 0] * (J[1, 1] * J[2, 2] - J[1, 2] * J[2, 1]) - J[0, 1] * (J[1, 0] * J[2, 2] - J[1, 2] * J[2, 0])) +
           J[0, 2] * (J[1, 0] * J[2, 1] - J[1, 1] * J[2, 0]))
    assert (det < 0) == (name == "fold")
    got, stats = kernel_jacobian(dev, u, A)
    n = got.size
    assert (dc.bits(got) == dc.bits(np.float32(det))).all()
    assert stats["n_finite"] == n and stats["n_folded"] == (n if det <= 0 else 0) and stats["min"] == det and stats["max"] == det
    assert abs(stats["sum"] - n * det) <= n * 2.0 ** -53 * n * abs(det)


def case_jacobian_guard_and_refusals(dev):
    """dirty buffers: nothing behind d_det or the partials is written; a dimension of 1, NULL buffers and too many rows are refused
    with the outputs untouched"""
    grid = "257x19x5"
    u, rd = sine(grid, 10.0), GRIDS[grid][0]
    L = dev.L
    n, guard = rd[0] * rd[1] * rd[2], 4096
    slots, nstat = int(L.s3d_k_field_jacobian_slots()), int(L.s3d_k_field_jacobian_stats())
    assert (slots, nstat) == (2048, 5)
    pbytes = slots * nstat * 8
    bufs = [dev.upload(dc.planar(u)), dev.malloc(4 * n + guard), dev.malloc(pbytes + guard)]
    A_ = np.ascontiguousarray(sc.A_FIXED)
    A = A_.ctypes.data_as(P(C.c_double))
    d_u, d_d, d_p = bufs
    try:
        dev.check(L.s3d_rt_memset(d_d, 0xA5, 4 * n + guard, None))
        dev.check(L.s3d_rt_memset(d_p, 0xA5, pbytes + guard, None))
        for args in ((d_u, (1, 19, 5), A, d_d, d_p), (d_u, (257, 1, 5), A, d_d, d_p), (d_u, (257, 19, 1), A, d_d, d_p),
                     (d_u, (257, 19, 0), A, d_d, d_p), (None, rd, A, d_d, d_p), (d_u, rd, None, d_d, d_p), (d_u, rd, A, d_d, None),
                     (d_u, (257, 65536, 5), A, d_d, d_p), (d_u, (257, 19, 65536), A, d_d, d_p)):
            a_u, a_rd, a_A, a_d, a_p = args
            assert L.s3d_k_field_jacobian(a_u, *a_rd, a_A, a_d, a_p, None) != 0 and dev.err(), args
        dev.sync()
        assert (dev.download(d_d, (4 * n,), np.uint8) == 0xA5).all() and (dev.download(d_p, (pbytes,), np.uint8) == 0xA5).all()
        dev.check(L.s3d_k_field_jacobian(d_u, *rd, A, d_d, d_p, None))
        dev.sync()
        got = dev.download(d_d, rd[::-1], np.float32)
        part = dev.download(d_p, (slots, nstat), np.float64)
        tails = [dev.download(d_d + 4 * n, (guard,), np.uint8), dev.download(d_p + pbytes, (guard,), np.uint8)]
    finally:
        for b in bufs:
            dev.free(b)
    assert all((t == 0xA5).all() for t in tails)
    w = jacobian_want(grid, 10.0)
    assert np.array_equal(dc.bits(got), dc.bits(w.map))
    assert not part[rd[1] * rd[2]:].any() and int(part[:, 1].sum()) == w.n_finite and int(part[:, 2].sum()) == w.n_folded


# ---- the public entry points ------------------------------------------------------------------------------------------------
def make_opts(max_iter=0, tol=0.0):
    o = abi.FieldInverseOpts()
    o.max_iter, o.tol = max_iter, tol
    return o


def interleaved(u):
    """three [z, y, x] components -> [z, y, x, 3]"""
    return np.ascontiguousarray(np.stack([np.asarray(c, np.float32) for c in u], axis=-1))


def mat_from(L, a):
    """a Mat_rm of doubles holding the 2-D array a"""
    m = abi.Mat_rm()
    a = np.ascontiguousarray(a, np.float64)
    assert L.imutil.init_Mat_rm(C.byref(m), a.shape[0], a.shape[1], 0, 0) == 0
    C.memmove(m.data, a.ctypes.data, a.nbytes)
    return m


def mat_to(m):
    out = np.empty((m.num_rows, m.num_cols))
    C.memmove(out.ctypes.data, m.data, out.nbytes)
    return out


def affine_matrix(t):
    out = np.empty((3, 4))
    C.memmove(out.ctypes.data, t.A.data, out.nbytes)
    return out


def apply_points(L, t, field_im, pts):
    """sift3d_amd_field_apply_points on 3 x n points -> 3 x n"""
    m_in, m_out = mat_from(L, pts), abi.Mat_rm()
    assert L.imutil.init_Mat_rm(C.byref(m_out), 0, 0, 0, 0) == 0
    try:
        rc = L.sift.sift3d_amd_field_apply_points(None if t is None else C.addressof(t), C.byref(field_im), C.byref(m_in), C.byref(m_out))
        assert rc == 0, L.imutil.sift3d_amd_last_error()
        return mat_to(m_out)
    finally:
        L.imutil.cleanup_Mat_rm(C.byref(m_in))
        L.imutil.cleanup_Mat_rm(C.byref(m_out))


def case_struct_layouts(tmp_path):
    """the ctypes mirrors against the C definitions: sizes and offsets as the compiler lays them out"""
    classes = {"sift3d_amd_field_inverse_opts": abi.FieldInverseOpts, "sift3d_amd_field_inverse_info": abi.FieldInverseInfo,
               "sift3d_amd_field_jacobian_info": abi.FieldJacobianInfo}
    body = "".join(f'printf("%zu", sizeof({t}));' + "".join(f'printf(" %zu", offsetof({t}, {f}));' for f, _ in cls._fields_) +
                   'printf("\\n");' for t, cls in classes.items())
    (tmp_path / "layout.c").write_text(f'#include <stddef.h>\n#include <stdio.h>\n#include "sift3d_amd.h"\nint main(void) {{ {body} return 0; }}\n')
    subprocess.run(["gcc", "-std=gnu11", "-I", os.path.join(sc.ROOT, "include"), str(tmp_path / "layout.c"), "-o", str(tmp_path / "layout")],
                   check=True)
    out = subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout.split("\n")
    for line, cls in zip(out, classes.values()):
        assert [int(v) for v in line.split()] == [C.sizeof(cls)] + [getattr(cls, f).offset for f, _ in cls._fields_]
    assert (C.sizeof(abi.FieldInverseOpts), C.sizeof(abi.FieldInverseInfo), C.sizeof(abi.FieldJacobianInfo)) == (16, 64, 48)


def case_forms_agree(L, dev):
    """the host forms against the device forms and the kernels' restatement on 70x33x9 at amp 1.5; the returned pair is a map:
    inv_tform . tform is the identity, sift3d_amd_im_warp_field through the pair is the restated warp, and points pushed through
    (tform, field) come home through the pair"""
    grid = "70x33x9"
    u, (rd, sd) = sine(grid, 1.5), GRIDS[grid]
    want = invert_want(grid, 1.5)
    n = sd[0] * sd[1] * sd[2]
    t = sc.make_affine(L, sc.A_FIXED)
    inv_t = abi.Affine()
    assert L.imutil.init_tform(C.byref(inv_t), 0) == 0
    f_im = L.image_from_numpy(interleaved(u), (1, 1, 1.5))
    inv_im, det_im, warped = abi.Image(), abi.Image(), abi.Image()
    for im in (inv_im, det_im, warped):
        L.imutil.init_im(C.byref(im))
    info, info_d = abi.FieldInverseInfo(), abi.FieldInverseInfo()
    jinfo, jinfo_d, jinfo_s = abi.FieldJacobianInfo(), abi.FieldJacobianInfo(), abi.FieldJacobianInfo()
    units = (C.c_double * 3)(0.5, 0.75, 2.0)
    opts = make_opts(MAX_ITER, TOL)
    bufs = [dev.upload(dc.planar(u)), dev.upload(np.full(3 * n, -3.5, np.float32)), dev.upload(np.full(rd[0] * rd[1] * rd[2], -3.5, np.float32))]
    ref_vol = sc.volumes(grid, clean=True)[0]                                # a volume on the reference grid, to pull back
    r_im = L.image_from_numpy(ref_vol, (1, 1, 1))
    try:
        # -- the inversion
        rc = L.sift.sift3d_amd_invert_field(C.addressof(t), C.byref(f_im), *sd, units, C.byref(opts), C.byref(inv_t), C.byref(inv_im),
                                            C.byref(info))
        assert rc == 0, L.imutil.sift3d_amd_last_error()
        assert (inv_im.nx, inv_im.ny, inv_im.nz, inv_im.nc) == (*sd, 3) and (inv_im.ux, inv_im.uy, inv_im.uz) == (0.5, 0.75, 2.0)
        got = L.image_to_numpy(inv_im)                                      # [z, y, x, 3]
        inv_A = (C.c_double * 12)()
        rc = L.sift.sift3d_amd_invert_field_dev(bufs[0], *rd, C.addressof(t), bufs[1], *sd, None, inv_A, C.byref(info_d), None)
        assert rc == 0, L.imutil.sift3d_amd_last_error()                    # (opts NULL: the defaults, which MAX_ITER and TOL are)
        flat = dev.download(bufs[1], (3, n), np.float32)
        assert np.array_equal(dc.bits(flat), dc.bits(dc.planar(dc.field_components(got)))) and bytes(info) == bytes(info_d)
        Binv = affine_matrix(inv_t)
        assert np.array_equal(Binv, np.array(inv_A[:]).reshape(3, 4))
        M = np.vstack([Binv, [0, 0, 0, 1]]) @ np.vstack([sc.A_FIXED, [0, 0, 0, 1]])
        assert np.abs(M - np.eye(4)).max() <= 1e-12
        # the library's cofactor inverse differs from numpy's in the last bits, so the restatement runs on the library's own
        w = want if np.array_equal(Binv, inverse34(sc.A_FIXED)) else InvertWant(u, sc.A_FIXED, Binv, sd)
        assert np.array_equal(flat.view(np.uint32), w.bits)
        assert (info.n, info.n_converged, info.n_outside, info.n_not_converged, info.n_invalid, info.updates) == (n, *w.counts, w.updates)
        mean = math.fsum(w.res) / w.res.size                               # (the summation bound and the division's rounding)
        assert abs(info.mean_residual - mean) <= (n * 2.0 ** -53 + 2.0 ** -52) * mean and info.max_residual <= TOL
        assert abs(info.max_residual - w.res.max()) <= np.spacing(w.res.max())
        # -- pulling the reference onto the source grid through the returned pair: the restated warp
        for interp in (0, 1):
            assert L.sift.sift3d_amd_im_warp_field(C.addressof(inv_t), C.byref(inv_im), C.byref(r_im), interp, C.byref(warped)) == 0
            assert (warped.nx, warped.ny, warped.nz, warped.nc) == (*sd, 1)
            pulled = L.image_to_numpy(warped)
            assert np.array_equal(dc.bits(pulled), dc.bits(dc.kernel_warp(dev, ref_vol, sd, Binv, dc.field_components(got), interp)))
        assert np.isfinite(pulled).all() and (pulled != 0).sum() > 0.5 * pulled.size
        # -- the determinant
        assert L.sift.sift3d_amd_field_jacobian(C.addressof(t), C.byref(f_im), C.byref(det_im), C.byref(jinfo)) == 0
        assert (det_im.nx, det_im.ny, det_im.nz, det_im.nc) == (*rd, 1) and (det_im.ux, det_im.uy, det_im.uz) == (1.0, 1.0, 1.5)
        jw = jacobian_want(grid, 1.5)
        assert np.array_equal(dc.bits(L.image_to_numpy(det_im)), dc.bits(jw.map))
        assert L.sift.sift3d_amd_field_jacobian_dev(bufs[0], *rd, C.addressof(t), bufs[2], C.byref(jinfo_d), None) == 0
        assert np.array_equal(dc.bits(dev.download(bufs[2], rd[::-1], np.float32)), dc.bits(jw.map)) and bytes(jinfo) == bytes(jinfo_d)
        assert L.sift.sift3d_amd_field_jacobian(C.addressof(t), C.byref(f_im), None, C.byref(jinfo_s)) == 0 and bytes(jinfo_s) == bytes(jinfo)
        assert L.sift.sift3d_amd_field_jacobian(C.addressof(t), C.byref(f_im), C.byref(det_im), None) == 0
        assert (jinfo.n, jinfo.n_finite, jinfo.n_folded, jinfo.min_det, jinfo.max_det) == (jw.det.size, jw.n_finite, 0, jw.min, jw.max)
        assert abs(jinfo.mean_det - jw.sum / jw.n_finite) <= (jw.n_finite * 2.0 ** -53 + 2.0 ** -52) * jw.mag / jw.n_finite
        # -- points: at integer in-grid points T(x) + u(x) to the bit, outside the clamped sample, and there and back
        rng = np.random.default_rng(5)
        ints = np.stack([rng.integers(0, m, 64) for m in rd]).astype(np.float64)
        ints[:, 0], ints[:, 1] = 0, np.array(rd) - 1
        out = apply_points(L, t, f_im, ints)
        ix, iy, iz = ints.astype(np.int64)
        A = sc.A_FIXED
        for i in range(3):
            tx = A[i, 0] * ints[0] + A[i, 1] * ints[1] + A[i, 2] * ints[2] + A[i, 3]
            assert np.array_equal(out[i], tx + u[i][iz, iy, ix].astype(np.float64)), i
        far = np.array([[-3.5, 100.25, 10.5, 69.0], [5.0, -2.0, 40.0, 32.75], [12.0, 3.5, -1.0, 8.0]])
        out = apply_points(L, t, f_im, far)
        q = clamp(tuple(far), rd)
        for i in range(3):
            tx = A[i, 0] * far[0] + A[i, 1] * far[1] + A[i, 2] * far[2] + A[i, 3]
            assert np.array_equal(out[i], tx + trilinear_f64(u[i], q)), i
        none = apply_points(L, None, f_im, far)                              # no transform: the identity
        for i in range(3):
            assert np.array_equal(none[i], far[i] + trilinear_f64(u[i], q)), i
        # reference points whose images are voxel centres of the source that converged inside: through (tform, field), then
        # back through the returned pair (whose field is sampled at those voxel centres: the float w itself)
        ok = np.flatnonzero(w.status == 0)[:: max(1, int((w.status == 0).sum()) // 200)]
        z_, y_, x_ = np.unravel_index(ok, sd[::-1])
        Y = np.stack([x_, y_, z_]).astype(np.float64)
        X = apply_points(L, inv_t, inv_im, Y)                               # psi(y)
        home = apply_points(L, t, f_im, X)                                  # phi(psi(y))
        err = np.sqrt(((home - Y) ** 2).sum(0))
        slack = rounding_slack(u, sc.A_FIXED, flat[:, ok])
        print(f"{ok.size} points there and back: max {err.max()!r} against {TOL + slack!r}")
        assert err.max() <= TOL + slack
        # and the other way round from the reference points x = psi(y): through (tform, field), which lands within eps = TOL +
        # slack of y, and back through the pair, which is psi(y) = x at y to the bit and moves by at most
        # sum_a (|B_ia| + the largest neighbour difference of w_i along a) eps per component over that distance
        back = apply_points(L, inv_t, inv_im, home)
        wc = dc.field_components(got)
        per = [sum(abs(Binv[i, a]) + float(np.abs(np.diff(wc[i].astype(np.float64), axis=2 - a)).max()) for a in range(3)) *
               (TOL + slack) for i in range(3)]
        bound = math.sqrt(sum(v * v for v in per))
        err = np.sqrt(((back - X) ** 2).sum(0))
        print(f"and back again, in reference voxels: max {err.max()!r} against {bound!r}")
        assert err.max() <= bound
    finally:
        for b in bufs:
            dev.free(b)
        for tf in (t, inv_t):
            L.imutil.cleanup_tform(C.byref(tf))
        for im in (f_im, inv_im, det_im, warped, r_im):
            L.free_image(im)


def case_refusals(L):
    """each failure returns SIFT3D_FAILURE with its message and leaves the outputs untouched"""
    from tests import tps_cases as tc
    lib, last = L.sift, L.imutil.sift3d_amd_last_error
    tc.bind(L)
    rd, sd = GRIDS["70x33x9"]
    u = sine("70x33x9", 1.5)
    good = sc.make_affine(L, sc.A_FIXED)
    singular = sc.make_affine(L, np.array([[1.0, 2.0, 3.0, 0.5], [2.0, 4.0, 6.0, 1.0], [0.0, 1.0, 0.0, 0.0]]))
    nonfinite = sc.make_affine(L, np.array([[1.0, 0.0, 0.0, math.inf], [0.0, 1.0, 0.0, 0.0], [0.0, 0.0, 1.0, 0.0]]))
    ctrl, params = tc.warp_inputs(4, 1, rd)[1:]
    tps = tc.make_tps(L, ctrl, params)
    f_im = L.image_from_numpy(interleaved(u), (1, 1, 1))
    nc1 = L.image_from_numpy(np.zeros(rd[::-1], np.float32), (1, 1, 1))
    thin = L.image_from_numpy(np.zeros((1, 33, 70, 3), np.float32), (1, 1, 1))
    out_im = L.image_from_numpy(np.full((2, 3, 4, 3), 5.0, np.float32), (1, 1, 1))
    inv_t = sc.make_affine(L, sc.A_SHIFT)
    info, jinfo = abi.FieldInverseInfo(), abi.FieldJacobianInfo()
    m_in, m_out = mat_from(L, np.zeros((3, 2))), mat_from(L, np.full((1, 1), 7.0))
    m_bad = mat_from(L, np.zeros((2, 3)))

    def state():
        return (bytes(C.string_at(C.addressof(out_im), C.sizeof(out_im))) + bytes(C.string_at(out_im.data, 4 * 72)) + bytes(info) +
                bytes(jinfo) + affine_matrix(inv_t).tobytes() + bytes(C.string_at(C.addressof(m_out), C.sizeof(m_out))))

    def invert(t, f, dims=sd, opts=None, it=inv_t, out=out_im, units=None):
        return lib.sift3d_amd_invert_field(None if t is None else C.addressof(t), None if f is None else C.byref(f), *dims, units,
                                           None if opts is None else C.byref(opts), None if it is None else C.byref(it),
                                           None if out is None else C.byref(out), C.byref(info))

    try:
        C.memset(C.byref(info), 0xAB, C.sizeof(info))
        C.memset(C.byref(jinfo), 0xAB, C.sizeof(jinfo))
        before = state()
        for label, call, msg in (
                ("a singular map", lambda: invert(singular, f_im), b"singular"),
                ("a map that is not finite", lambda: invert(nonfinite, f_im), b"not finite"),
                ("a Tps", lambda: invert(tps, f_im), b"Tps"),
                ("nc = 1", lambda: invert(good, nc1), b"three channels"),
                ("a NULL field", lambda: invert(good, None), b"NULL"),
                ("a NULL inverse field", lambda: invert(good, f_im, out=None), b"NULL"),
                ("a NULL inverse transform", lambda: invert(good, f_im, it=None), b"NULL"),
                ("a source dimension of 0", lambda: invert(good, f_im, dims=(61, 0, 11)), b"bad dimensions"),
                ("max_iter -1", lambda: invert(good, f_im, opts=make_opts(max_iter=-1)), b"max_iter"),
                ("tol -1", lambda: invert(good, f_im, opts=make_opts(tol=-1.0)), b"tol"),
                ("tol NaN", lambda: invert(good, f_im, opts=make_opts(tol=math.nan)), b"tol"),
                ("units 0", lambda: invert(good, f_im, units=(C.c_double * 3)(1.0, 0.0, 1.0)), b"units")):
            assert call() == -1, label
            assert b"sift3d_amd_invert_field" in last() and msg in last(), (label, last())
            assert state() == before, label
        inv_A = (C.c_double * 12)(*([7.0] * 12))
        assert lib.sift3d_amd_invert_field_dev(None, *rd, C.addressof(good), None, *sd, None, inv_A, C.byref(info), None) == -1
        assert b"NULL data" in last() and list(inv_A) == [7.0] * 12 and state() == before
        for label, call, msg in (
                ("a Tps", lambda: lib.sift3d_amd_field_jacobian(C.addressof(tps), C.byref(f_im), C.byref(out_im), C.byref(jinfo)), b"Tps"),
                ("nc = 1", lambda: lib.sift3d_amd_field_jacobian(C.addressof(good), C.byref(nc1), C.byref(out_im), C.byref(jinfo)), b"three channels"),
                ("a dimension of 1", lambda: lib.sift3d_amd_field_jacobian(C.addressof(good), C.byref(thin), C.byref(out_im), C.byref(jinfo)), b"at least 2"),
                ("a NULL field", lambda: lib.sift3d_amd_field_jacobian(C.addressof(good), None, C.byref(out_im), C.byref(jinfo)), b"NULL"),
                ("no output", lambda: lib.sift3d_amd_field_jacobian(C.addressof(good), C.byref(f_im), None, None), b"neither")):
            assert call() == -1, label
            assert b"sift3d_amd_field_jacobian" in last() and msg in last(), (label, last())
            assert state() == before, label
        assert lib.sift3d_amd_field_jacobian_dev(None, *rd, C.addressof(good), None, C.byref(jinfo), None) == -1 and state() == before
        for label, call, msg in (
                ("a Tps", lambda: lib.sift3d_amd_field_apply_points(C.addressof(tps), C.byref(f_im), C.byref(m_in), C.byref(m_out)), b"Tps"),
                ("nc = 1", lambda: lib.sift3d_amd_field_apply_points(C.addressof(good), C.byref(nc1), C.byref(m_in), C.byref(m_out)), b"three channels"),
                ("2 x 3 points", lambda: lib.sift3d_amd_field_apply_points(C.addressof(good), C.byref(f_im), C.byref(m_bad), C.byref(m_out)), b"3 x n"),
                ("NULL points", lambda: lib.sift3d_amd_field_apply_points(C.addressof(good), C.byref(f_im), None, C.byref(m_out)), b"NULL")):
            assert call() == -1, label
            assert b"sift3d_amd_field_apply_points" in last() and msg in last(), (label, last())
            assert state() == before, label
    finally:
        for t in (good, singular, nonfinite, tps, inv_t):
            L.imutil.cleanup_tform(C.byref(t))
        for im in (f_im, nc1, thin, out_im):
            L.free_image(im)
        for m in (m_in, m_out, m_bad):
            L.imutil.cleanup_Mat_rm(C.byref(m))
