"""Shared by tests/test_demons.py (CPU: the SIMT emulator build of the library) and tests/test_gpu_demons.py (the device): the
inputs of the deformable registration (sift3d_amd_register_demons, s3d_k_demons_step, s3d_k_inv_field, s3d_k_field_upsample2),
a numpy restatement of the kernels' definitions (include/s3d_device.h) and of the driver (include/sift3d_amd.h), and the checks
both suites apply.

The kernels' restatement forms every term with the operation order the header states, as element-wise f64 numpy operations:
each is rounded once and nothing is fused, as in the kernels (compiled without contraction), so an updated field entry, a warped
voxel and an upsampled entry are reproduced bit for bit and the sums obey the bound of any summation order,
n * 2^-53 * sum |term|.  The driver's restatement follows the schedule of the header with a plain `reflect`-boundary Gaussian in
f64 where the library's mirrors asymmetrically and rounds every axis pass to f32, so it is compared with a margin.

One deviation between the suites: the device-pointer entry is compared with the host form on the whole recovery case on the GPU
only; on the emulator, where one such call takes a minute, the two forms are compared on the same pair with six passes per
level (case_forms_agree's opts)."""
import ctypes as C
import math
import os

import numpy as np

from sift3d_amd import abi
from tests import refine_cases as rcs
from tests import similarity_cases as sc

P = C.POINTER
RAW, SCALED = rcs.RAW, rcs.SCALED
# (constants, max_step): kstep = 1 / (4 max_step^2)
STEP_SETTINGS = {"raw": (RAW, 1.0), "scaled": (SCALED, 0.5)}
RDIMS = (48, 44, 40)
_CACHE = {}


def kstep_of(max_step):
    return 1.0 / (4.0 * max_step * max_step)


def planar(u):
    """three [z, y, x] components -> the device layout, component c of voxel i at [c * N + i]"""
    return np.ascontiguousarray(np.stack([np.asarray(c, np.float32) for c in u]).reshape(3, -1))


def components(flat, rdims):
    return tuple(np.asarray(flat).reshape(3, rdims[2], rdims[1], rdims[0]))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def random_field(shape_key):
    """seeded, standard deviation 1.5 voxels, a few entries NaN, +inf and 1000 (far outside the source)"""
    key = ("field", shape_key)
    if key not in _CACHE:
        rd = sc.SHAPES[shape_key][0]
        n = rd[0] * rd[1] * rd[2]
        u = (np.random.default_rng(7).standard_normal((3, n)) * 1.5).astype(np.float32)
        for k, (c, i) in enumerate(((0, n // 3), (1, n // 2 + 5), (2, n // 5), (0, n // 7), (1, 2 * n // 3), (2, n // 2 + 40),
                                    (0, n // 2 + 77), (1, n // 4), (2, 3 * n // 4))):
            u[c, i] = (np.nan, np.inf, 1000.0)[k % 3]
        u.setflags(write=False)
        _CACHE[key] = components(u, rd)
    return _CACHE[key]


# ---- numpy restatement of the kernels ---------------------------------------------------------------------------------------
def field_coords(A, rdims, u):
    """(tx, ty, tz) = A [x y z 1]^T + (double)u, each operation rounded"""
    return tuple(a + np.asarray(b, np.float32).astype(np.float64) for a, b in zip(sc.affine_coords(A, rdims), u))


class StepWant:
    """s3d_k_demons_step restated: v bit for bit, the exact count, math.fsum of the two f64 sums and the magnitudes their
    rounding is relative to (tests/refine_cases.Want extended by u, D and m)"""

    def __init__(self, ref, src, A, consts, kstep, u):
        sa, ma, sb, mb = consts
        rd, sd = ref.shape[::-1], src.shape[::-1]
        with np.errstate(invalid="ignore", over="ignore"):
            t = field_coords(A, rd, u)
        inside = sc.inside_mask(t, sd)
        b = sc.trilinear(src, t, inside)
        tx, ty, tz = (np.where(inside, c, 0.0) for c in t)
        X0, Y0, Z0 = (np.minimum(np.floor(c).astype(np.int64), n - 2) for c, n in zip((tx, ty, tz), sd))
        fx, fy, fz = tx - X0, ty - Y0, tz - Z0
        ux, uy, uz = 1.0 - fx, 1.0 - fy, 1.0 - fz
        s = src.astype(np.float64)
        c000, c100, c010, c110 = s[Z0, Y0, X0], s[Z0, Y0, X0 + 1], s[Z0, Y0 + 1, X0], s[Z0, Y0 + 1, X0 + 1]
        c001, c101, c011, c111 = s[Z0 + 1, Y0, X0], s[Z0 + 1, Y0, X0 + 1], s[Z0 + 1, Y0 + 1, X0], s[Z0 + 1, Y0 + 1, X0 + 1]
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            gx = ((c100 - c000) * uy + (c110 - c010) * fy) * uz + ((c101 - c001) * uy + (c111 - c011) * fy) * fz
            gy = ((c010 - c000) * ux + (c110 - c100) * fx) * uz + ((c011 - c001) * ux + (c111 - c101) * fx) * fz
            gz = ((c001 - c000) * ux + (c101 - c100) * fx) * uy + ((c011 - c010) * ux + (c111 - c110) * fx) * fy
            gx, gy, gz = sb * gx, sb * gy, sb * gz
            ok = inside & np.isfinite(ref) & np.isfinite(b) & np.isfinite(gx) & np.isfinite(gy) & np.isfinite(gz)
            r = sb * (b.astype(np.float64) - mb) - sa * (ref.astype(np.float64) - ma)
            D = ((gx * gx + gy * gy) + gz * gz) + kstep * (r * r)
            moved = ok & (D > 0) & np.isfinite(D)
            m = (-r) / np.where(moved, D, 1.0)
            d = tuple(np.where(moved, m * g, 0.0) for g in (gx, gy, gz))
            self.v = tuple(np.where(moved, (np.asarray(uc, np.float32).astype(np.float64) + dc).astype(np.float32),
                                    np.asarray(uc, np.float32)) for uc, dc in zip(u, d))
        self.inside, self.ok, self.moved, self.n = inside, ok, moved, int(ok.sum())
        terms = ((r * r)[ok], ((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])[ok])
        self.sums = np.array([math.fsum(t) for t in terms])
        self.mags = np.array([math.fsum(np.abs(t)) for t in terms])


def step_want(shape, setting):
    key = ("step", shape, setting)
    if key not in _CACHE:
        ref, src = sc.volumes(shape)
        consts, max_step = STEP_SETTINGS[setting]
        _CACHE[key] = StepWant(ref, src, sc.A_FIXED, consts, kstep_of(max_step), random_field(shape))
    return _CACHE[key]


def check_step_sums(got, w, label=""):
    """n exactly, the two sums within n * 2^-53 * sum |term| of the correctly rounded sum (refine_cases.check_sums' bound)"""
    bound = w.n * 2.0 ** -53 * w.mags
    err = np.abs(got[[0, 2]] - w.sums)
    print(f"{label} n: got {got[1]!r}, want {w.n}; sum r^2 {got[0]!r} fsum {w.sums[0]!r} error {err[0]:.3e} bound {bound[0]:.3e}; "
          f"sum |d|^2 {got[2]!r} fsum {w.sums[1]!r} error {err[1]:.3e} bound {bound[1]:.3e}")
    assert got[1] == w.n
    assert np.isfinite(got).all()
    assert (err <= bound).all()


def upsample_want(coarse, fdims):
    """s3d_k_field_upsample2 restated: the tri-linear sample at (min(x / 2.0, cn - 1), ..), doubled in f64"""
    fnx, fny, fnz = fdims
    out = []
    for c in coarse:
        cz, cy, cx = c.shape
        idx = [np.minimum(np.arange(n, dtype=np.float64) / 2.0, m - 1) for n, m in ((fnz, cz), (fny, cy), (fnx, cx))]
        Z, Y, X = np.meshgrid(*idx, indexing="ij")
        b = sc.trilinear(c, (X, Y, Z), np.ones((fnz, fny, fnx), bool))
        out.append((2.0 * b.astype(np.float64)).astype(np.float32))
    return tuple(out)


# ---- drivers of the kernels -------------------------------------------------------------------------------------------------
def kernel_step(dev, src, ref, A, u, consts, kstep, in_place=False):
    """s3d_k_demons_step on dev -> (v as three [z, y, x] components, the 3 sums)"""
    rd = ref.shape[::-1]
    flat = planar(u)
    bufs = [dev.upload(src), dev.upload(ref), dev.upload(flat)]
    bufs.append(bufs[2] if in_place else dev.upload(np.full(flat.shape, -3.5, np.float32)))
    try:
        sums = dev.demons_step(bufs[0], src.shape[::-1], bufs[1], rd, A, bufs[2], bufs[3], consts, kstep)
        v = dev.download(bufs[3], flat.shape, np.float32)
        if not in_place:
            assert np.array_equal(bits(dev.download(bufs[2], flat.shape, np.float32)), bits(flat))   # u is only read
        return components(v, rd), sums
    finally:
        for b in bufs[:3] + ([] if in_place else [bufs[3]]):
            dev.free(b)


def kernel_warp(dev, src, rdims, A, u, interp, affine_only=False):
    """s3d_k_inv_field (or s3d_k_inv_affine) on dev; src [z, y, x] or [z, y, x, c] -> the same layout over rdims"""
    L = dev.L
    nc = 1 if src.ndim == 3 else src.shape[3]
    sd = src.shape[:3][::-1]
    n = rdims[0] * rdims[1] * rdims[2]
    bufs = [dev.upload(src), dev.upload(np.full(n * nc, 7.0, np.float32))]
    a = np.ascontiguousarray(A, np.float64).reshape(12)
    try:
        if affine_only:
            L.s3d_k_inv_affine.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                           P(C.c_double), C.c_int, C.c_void_p]
            dev.check(L.s3d_k_inv_affine(bufs[0], *sd, nc, bufs[1], *rdims, a.ctypes.data_as(P(C.c_double)), interp, None))
        else:
            bufs.append(dev.upload(planar(u)))
            dev.inv_field(bufs[0], sd, nc, bufs[1], rdims, A, bufs[2], interp)
        out = dev.download(bufs[1], (rdims[2], rdims[1], rdims[0], nc), np.float32)
        return out[..., 0] if nc == 1 else out
    finally:
        for b in bufs:
            dev.free(b)


def kernel_upsample(dev, coarse, fdims):
    cd = coarse[0].shape[::-1]
    n = fdims[0] * fdims[1] * fdims[2]
    bufs = [dev.upload(planar(coarse)), dev.upload(np.full(3 * n, -3.5, np.float32))]
    try:
        dev.field_upsample2(bufs[0], cd, bufs[1], fdims)
        return components(dev.download(bufs[1], (3 * n,), np.float32), fdims)
    finally:
        for b in bufs:
            dev.free(b)


# ---- the public entry points ------------------------------------------------------------------------------------------------
def make_opts(levels=0, max_iter=0, sigma=0.0, max_step=0.0, tol=0.0, min_overlap=0.0, normalize=0):
    o = abi.DemonsOpts()
    o.levels, o.max_iter, o.sigma, o.max_step, o.tol, o.min_overlap, o.normalize = \
        levels, max_iter, sigma, max_step, tol, min_overlap, normalize
    return o


class Registered:
    def __init__(self, rc, field, info, err):
        self.rc, self.field, self.info, self.err = rc, field, info, err          # field: [z, y, x, 3] or None


def register(L, src, ref, A, opts=None, units=(1, 1, 1)):
    """sift3d_amd_register_demons of library L on numpy volumes [z, y, x] under the map A (None: no transform)"""
    ims = [L.image_from_numpy(src, (1, 1, 1)), L.image_from_numpy(ref, units)]
    field, info = abi.Image(), abi.DemonsInfo()
    L.imutil.init_im(C.byref(field))
    C.memset(C.byref(info), 0xAB, C.sizeof(info))
    t = None if A is None else sc.make_affine(L, A)
    try:
        rc = L.sift.sift3d_amd_register_demons(C.byref(ims[0]), C.byref(ims[1]), None if t is None else C.addressof(t),
                                               None if opts is None else C.byref(opts), C.byref(field), C.byref(info))
        out = None
        if rc == 0:
            assert (field.nx, field.ny, field.nz, field.nc) == (ref.shape[2], ref.shape[1], ref.shape[0], 3)
            assert (field.ux, field.uy, field.uz) == tuple(float(v) for v in units)
            out = L.image_to_numpy(field)
        return Registered(rc, out, info, L.imutil.sift3d_amd_last_error() or b"")
    finally:
        if t is not None:
            L.imutil.cleanup_tform(C.byref(t))
        for im in ims + [field]:
            L.free_image(im)


def field_components(field):
    """[z, y, x, 3] -> three [z, y, x] components"""
    return tuple(np.ascontiguousarray(field[..., c]) for c in range(3))


def check_contract(g, min_overlap=0.5):
    """success, and either a field that is no worse at level 0 or the zero field, bit for bit"""
    i = g.info
    print(f"status {i.status}, levels {i.levels_run}, iters {i.iters}, passes {i.passes}, n {i.n_before} -> {i.n_after}, cost "
          f"{i.cost_before!r} -> {i.cost_after!r}, |u| mean {i.mean_disp!r} max {i.max_disp!r}")
    assert g.rc == 0, g.err
    assert i.cost_after <= i.cost_before and i.n_after >= min_overlap * i.n_before
    if i.status == abi.DEMONS_UNCHANGED:
        assert not bits(g.field).any() and i.mean_disp == 0.0 and i.max_disp == 0.0
    else:
        assert i.status in (abi.DEMONS_CONVERGED, abi.DEMONS_MAX_ITER)


# ---- numpy restatement of the driver ----------------------------------------------------------------------------------------
def gauss_taps(sigma):
    hw = int(math.ceil(3 * sigma))
    k = np.exp(-0.5 * ((np.arange(2 * hw + 1) - hw) / (sigma + np.finfo(np.float64).eps)) ** 2).astype(np.float32)
    return (k / np.float32(k.sum(dtype=np.float32))).astype(np.float64)


def smooth(f, sigma):
    """separable Gaussian, numpy's `reflect` boundary, f64"""
    k = gauss_taps(sigma)
    hw = len(k) // 2
    f = f.astype(np.float64)
    for ax in range(3):
        pad = [(0, 0)] * 3
        pad[ax] = (hw, hw)
        g = np.pad(f, pad, mode="reflect")
        out = np.zeros_like(f)
        for i, w in enumerate(k):
            sl = [slice(None)] * 3
            sl[ax] = slice(i, i + f.shape[ax])
            out += w * g[tuple(sl)]
        f = out
    return f


def restated_register(src, ref, A, levels=2, max_iter=50, sigma=1.5, max_step=1.0, tol=1e-3, min_dim=16):
    """the driver of include/sift3d_amd.h (raw SSD) -> (field components, cost_before, cost_after, levels_run)"""
    pyr = [(src, ref)]
    while len(pyr) < levels and all(n // 2 >= min_dim for v in pyr[-1] for n in v.shape):
        pyr.append(tuple(smooth(v, 1.0)[::2, ::2, ::2][:v.shape[0] // 2, :v.shape[1] // 2, :v.shape[2] // 2].astype(np.float32)
                         for v in pyr[-1]))
    k = kstep_of(max_step)
    zero = tuple(np.zeros(ref.shape, np.float32) for _ in range(3))
    w0 = StepWant(ref, src, A, RAW, k, zero)
    assert w0.n > 0
    u, levels_run = None, 0
    for l in range(len(pyr) - 1, -1, -1):
        s_, r_ = pyr[l]
        Al = np.array(A, np.float64)
        Al[:, 3] = Al[:, 3] / 2.0 ** l
        u = tuple(np.zeros(r_.shape, np.float32) for _ in range(3)) if u is None else upsample_want(u, r_.shape[::-1])
        hist = []
        for it in range(max_iter):
            w = StepWant(r_, s_, Al, RAW, k, u)
            if it == 0:
                if w.n == 0:
                    break
                levels_run += 1
            hist.append(w.sums[0] / w.n)
            if it >= 5 and hist[it] > (1.0 - tol) * hist[it - 5]:
                break
            u = tuple(smooth(c, sigma).astype(np.float32) for c in w.v)
    w1 = StepWant(ref, src, A, RAW, k, u)
    return u, w0.sums[0] / w0.n, w1.sums[0] / w1.n, levels_run


def sine_field(rdims=RDIMS, amp=1.5):
    nx, ny, nz = rdims
    z, y, x = np.meshgrid(np.arange(nz, dtype=np.float64), np.arange(ny, dtype=np.float64), np.arange(nx, dtype=np.float64),
                          indexing="ij")
    return (amp * np.sin(2 * np.pi * y / ny) * np.cos(np.pi * z / nz), amp * np.sin(2 * np.pi * z / nz),
            amp * np.cos(2 * np.pi * x / nx) * np.sin(np.pi * y / ny))


def recovery_pair():
    """(src, ref, the true field): src the blob volume, ref its restated tri-linear warp by A_FIXED plus the sine field"""
    if "recovery" not in _CACHE:
        src = sc._blobby(RDIMS, 21)
        true = sine_field()
        t = tuple(a + b for a, b in zip(sc.affine_coords(sc.A_FIXED, RDIMS), true))
        inside = sc.inside_mask(t, RDIMS)
        ref = np.where(inside, sc.trilinear(src, t, inside), np.float32(0)).astype(np.float32)
        for a in (src, ref):
            a.setflags(write=False)
        _CACHE["recovery"] = (src, ref, true)
    return _CACHE["recovery"]


def restated_recovery():
    if "restated" not in _CACHE:
        src, ref, _ = recovery_pair()
        _CACHE["restated"] = restated_register(src, ref, sc.A_FIXED)
    return _CACHE["restated"]


def library_recovery(L):
    """the library on the recovery pair, once per library"""
    key = ("library", id(L))
    if key not in _CACHE:
        src, ref, _ = recovery_pair()
        _CACHE[key] = register(L, src, ref, sc.A_FIXED, recovery_opts())
    return _CACHE[key]


def recovery_opts(max_iter=50):
    """the settings of the recovery case: two levels, sigma 1.5, max_step 1, tol 1e-3, at most 50 passes per level"""
    return make_opts(levels=2, max_iter=max_iter, sigma=1.5, max_step=1.0, tol=1e-3)


def field_error(u, true, margin=6):
    inter = (slice(margin, -margin),) * 3
    return float(np.sqrt(sum((np.asarray(a, np.float64) - b) ** 2 for a, b in zip(u, true)))[inter].mean())


# ---- the cases both suites run (L: the library behind the C API, dev: its flat device entry points) --------------------------
def case_step(dev, shape, setting):
    ref, src = sc.volumes(shape)
    consts, max_step = STEP_SETTINGS[setting]
    u = random_field(shape)
    w = step_want(shape, setting)
    assert 0 < w.n < int(w.inside.sum()) < ref.size                          # non-finite voxels dropped, part outside
    assert int(w.moved.sum()) > 0.9 * w.n
    for c in u:                                                             # the NaN, inf and 1000 entries are not inside
        assert not w.inside[~np.isfinite(c) | (c == 1000.0)].any()
    v, sums = kernel_step(dev, src, ref, sc.A_FIXED, u, consts, kstep_of(max_step))
    for c in range(3):
        assert np.array_equal(bits(v[c]), bits(w.v[c])), c
    check_step_sums(sums, w, f"{shape} {setting}")
    # no update longer than max_step but for the rounding of v to f32: half an ulp of the largest entry per component
    with np.errstate(invalid="ignore"):                                     # (the inf and NaN entries are not among the moved)
        step = np.sqrt(sum((a.astype(np.float64) - np.asarray(b, np.float32).astype(np.float64)) ** 2 for a, b in zip(v, u)))[w.moved]
    slack = float(np.spacing(np.float32(max(float(np.abs(c[w.moved]).max()) for c in v))))
    print("longest update", float(step.max()), "max_step", max_step, "slack", slack)
    assert step.max() <= max_step + slack
    for c in range(3):                                                      # an entry that is not updated keeps its bits
        assert np.array_equal(bits(v[c])[~w.moved], bits(u[c])[~w.moved])
    v2, sums2 = kernel_step(dev, src, ref, sc.A_FIXED, u, consts, kstep_of(max_step), in_place=True)
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(v, v2))      # two calls, and d_v == d_u: the same bits
    assert np.array_equal(sums.view(np.uint64), sums2.view(np.uint64))


def case_step_scratch_guard(dev):
    """a dirty scratch does not reach the sums, and nothing is written behind its stated size or behind the field"""
    shape = "257x19x5"
    ref, src = sc.volumes(shape)
    rd, sd = ref.shape[::-1], src.shape[::-1]
    L = dev.L
    n = ref.size
    nbytes, guard = int(L.s3d_k_demons_step_scratch_bytes(*rd)), 4096
    assert nbytes > 0 and nbytes % (3 * 8) == 0
    flat = planar(random_field(shape))
    bufs = [dev.upload(src), dev.upload(ref), dev.upload(flat), dev.malloc(12 * n + guard), dev.malloc(3 * 8),
            dev.malloc(nbytes + guard)]
    A = np.ascontiguousarray(sc.A_FIXED).ctypes.data_as(P(C.c_double))
    try:
        dev.check(L.s3d_rt_memset(bufs[3], 0xA5, 12 * n + guard, None))
        dev.check(L.s3d_rt_memset(bufs[5], 0xA5, nbytes + guard, None))
        dev.check(L.s3d_k_demons_step(bufs[0], *sd, bufs[1], *rd, A, bufs[2], bufs[3], *RAW, 0.25, bufs[4], bufs[5], None))
        got = dev.download(bufs[4], (3,), np.float64)
        v = dev.download(bufs[3], (3, n), np.float32)
        tails = [dev.download(bufs[3] + 12 * n, (guard,), np.uint8), dev.download(bufs[5] + nbytes, (guard,), np.uint8)]
    finally:
        for b in bufs:
            dev.free(b)
    assert all((t == 0xA5).all() for t in tails)
    w = step_want(shape, "raw")
    check_step_sums(got, w, "dirty scratch")
    assert np.array_equal(bits(v), bits(planar(w.v)))                        # every entry of v is written


def case_flat_refusals(dev):
    """a zero dimension, a source dimension of 1, NULL buffers, too many rows: non-zero, a message, the outputs untouched"""
    ref, src = sc.volumes("70x33x9", clean=True)
    L = dev.L
    assert L.s3d_k_demons_step_scratch_bytes(70, 33, 9) > 0
    for bad in ((0, 33, 9), (70, 0, 9), (70, 33, -1)):
        assert L.s3d_k_demons_step_scratch_bytes(*bad) == 0
    n = ref.size
    mark = np.full(3, -7.5)
    bufs = [dev.upload(src), dev.upload(ref), dev.upload(np.zeros(3 * n, np.float32)), dev.upload(np.full(3 * n, -7.5, np.float32)),
            dev.upload(mark), dev.upload(np.full(3 * 2048, -7.5))]
    A = np.ascontiguousarray(sc.A_FIXED).ctypes.data_as(P(C.c_double))
    sd, rd = (61, 37, 11), (70, 33, 9)
    s, r, u, v, o, w = bufs
    try:
        for args in ((s, (0, 37, 11), r, rd, A, u, v, o, w), (s, sd, r, (70, 0, 9), A, u, v, o, w), (s, (61, 37, 1), r, rd, A, u, v, o, w),
                     (s, (1, 37, 11), r, rd, A, u, v, o, w), (s, (61, 1, 11), r, rd, A, u, v, o, w), (None, sd, r, rd, A, u, v, o, w),
                     (s, sd, None, rd, A, u, v, o, w), (s, sd, r, rd, None, u, v, o, w), (s, sd, r, rd, A, None, v, o, w),
                     (s, sd, r, rd, A, u, None, o, w), (s, sd, r, rd, A, u, v, None, w), (s, sd, r, rd, A, u, v, o, None),
                     (s, sd, r, (70, 65536, 32768), A, u, v, o, w)):         # more rows than the grid's 32-bit index holds
            a_s, a_sd, a_r, a_rd, a_A, a_u, a_v, a_o, a_w = args
            assert L.s3d_k_demons_step(a_s, *a_sd, a_r, *a_rd, a_A, a_u, a_v, *RAW, 0.25, a_o, a_w, None) != 0 and dev.err()
        # the warp and the upsampling: NULL buffers, an unknown interpolation, dimensions that are not halves
        assert L.s3d_k_inv_field(s, *sd, 1, v, *rd, A, None, 0, None) != 0 and dev.err()
        assert L.s3d_k_inv_field(s, *sd, 1, v, *rd, A, u, 2, None) != 0 and dev.err()
        assert L.s3d_k_inv_field(s, *sd, 0, v, *rd, A, u, 0, None) != 0 and dev.err()
        assert L.s3d_k_field_upsample2(u, 35, 16, 5, v, 70, 33, 9, None) != 0 and dev.err()
        assert L.s3d_k_field_upsample2(u, 35, 16, 4, v, 70, 34, 9, None) != 0 and dev.err()
        assert L.s3d_k_field_upsample2(None, 35, 16, 4, v, 70, 33, 9, None) != 0 and dev.err()
        assert L.s3d_k_field_upsample2(u, 0, 16, 4, v, 1, 33, 9, None) != 0 and dev.err()
        dev.sync()
        assert np.array_equal(dev.download(o, (3,), np.float64), mark)
        assert (dev.download(w, (3 * 2048,), np.float64) == -7.5).all()
        assert (dev.download(v, (3 * n,), np.float32) == -7.5).all()
    finally:
        for b in bufs:
            dev.free(b)


def case_warp_zero_field(dev, interp, nc):
    """u == 0: s3d_k_inv_affine bit for bit"""
    rd = sc.SHAPES["70x33x9"][0]
    _, src = sc.volumes("70x33x9")
    if nc == 2:
        src = np.ascontiguousarray(np.stack([src, src[::-1] * np.float32(0.5)], axis=-1))
    zero = tuple(np.zeros(rd[::-1], np.float32) for _ in range(3))
    got = kernel_warp(dev, src, rd, sc.A_FIXED, zero, interp)
    want = kernel_warp(dev, src, rd, sc.A_FIXED, None, interp, affine_only=True)
    assert np.array_equal(bits(got), bits(want)) and np.isfinite(got).any() and (got != 7.0).all()


def case_warp_constant_field(dev, interp):
    """the constant field (3, -2, 1) on the identity: s3d_k_inv_affine with A_SHIFT bit for bit"""
    rd = sc.SHAPES["70x33x9"][0]
    _, src = sc.volumes("70x33x9", clean=True)
    const = tuple(np.full(rd[::-1], c, np.float32) for c in (3.0, -2.0, 1.0))
    got = kernel_warp(dev, src, rd, sc.A_IDENTITY, const, interp)
    want = kernel_warp(dev, src, rd, sc.A_SHIFT, None, interp, affine_only=True)
    assert np.array_equal(bits(got), bits(want)) and int((want != 0).sum()) > sc.KEPT_SHIFT // 2


def case_warp_random_field(dev, shape):
    """tri-linear through the random field of the step cases: similarity_cases.trilinear at the restated coordinates, zero outside"""
    rd = sc.SHAPES[shape][0]
    _, src = sc.volumes(shape, clean=True)
    u = random_field(shape)
    with np.errstate(invalid="ignore"):
        t = field_coords(sc.A_FIXED, rd, u)
    inside = sc.inside_mask(t, src.shape[::-1])
    want = np.where(inside, sc.trilinear(src, t, inside), np.float32(0)).astype(np.float32)
    got = kernel_warp(dev, src, rd, sc.A_FIXED, u, 0)
    assert 0 < int(inside.sum()) < inside.size
    assert np.array_equal(bits(got), bits(want))


def case_upsample(dev, fdims):
    cd = (35, 16, 4)
    assert tuple(n // 2 for n in fdims) == cd
    coarse = components((np.random.default_rng(3).standard_normal(3 * 35 * 16 * 4) * 2).astype(np.float32), cd)
    got, want = kernel_upsample(dev, coarse, fdims), upsample_want(coarse, fdims)
    for c in range(3):
        assert np.array_equal(bits(got[c]), bits(want[c])), c
    assert np.array_equal(bits(got[0][::2, ::2, ::2][:4, :16, :35]), bits((2.0 * coarse[0].astype(np.float64)).astype(np.float32)))


def case_field_norm(dev, shape):
    """the lengths of a field's entries: the count exactly, the sum within the bound of any summation order, the maximum to the
    rounding of one square root; the NaN and inf entries are left out, the entries of 1000 are not"""
    flat = planar(random_field(shape))
    n = flat.shape[1]
    with np.errstate(invalid="ignore", over="ignore"):
        x, y, z = (c.astype(np.float64) for c in flat)
        m = np.sqrt((x * x + y * y) + z * z)
    fin = np.isfinite(m)
    buf = dev.upload(flat)
    try:
        total, count, big = dev.field_norm(buf, n)
        again = dev.field_norm(buf, n)
    finally:
        dev.free(buf)
    want = math.fsum(m[fin])
    print(f"{shape}: sum {total!r} fsum {want!r}, count {count} of {n}, max {big!r} numpy {m[fin].max()!r}")
    assert count == int(fin.sum()) == n - 6 and m[fin].max() >= 1000.0
    assert abs(total - want) <= count * 2.0 ** -53 * want
    assert abs(big - m[fin].max()) <= np.spacing(m[fin].max())
    assert again == (total, count, big)


def case_nothing_to_do(L, dev):
    """ref is src warped by the map given: no residual, no update, the zero field"""
    ref, src = sc.meaning_volumes()
    zero = tuple(np.zeros(ref.shape, np.float32) for _ in range(3))
    v, sums = kernel_step(dev, src, ref, sc.A_FIXED, zero, RAW, 0.25)
    assert sums[0] == 0.0 and sums[2] == 0.0 and sums[1] > 0 and not any(bits(c).any() for c in v)
    g = register(L, src, ref, sc.A_FIXED, make_opts(max_iter=6))
    check_contract(g)
    assert g.info.cost_before == 0.0 and g.info.cost_after == 0.0 and g.info.n_before == int(sums[1])
    assert not bits(g.field).any()


def case_recovery(L, where):
    """the library against the numpy restatement of the whole driver on a known smooth deformation"""
    src, ref, true = recovery_pair()
    u_w, before_w, after_w, levels_w = restated_recovery()
    g = library_recovery(L)
    check_contract(g)
    i = g.info
    ratio, ratio_w = i.cost_after / i.cost_before, after_w / before_w
    err = field_error(field_components(g.field), true)
    err_w, err_0 = field_error(u_w, true), field_error(tuple(np.zeros_like(c) for c in true), true)
    text = (f"{where}: cost_after / cost_before {ratio:.5f} (restatement {ratio_w:.5f}); mean field error 6 voxels inside the border "
            f"{err:.4f} voxel (restatement {err_w:.4f}, zero field {err_0:.4f}); status {i.status}, {i.levels_run} levels, {i.iters} "
            f"updates, {i.passes} passes")
    print(text)
    out = os.environ.get("SIFT3D_DEMONS_RECORD")
    if out:
        with open(out, "a") as f:
            f.write(text + "\n")
    assert levels_w == 2 and abs(i.cost_before - before_w) <= 1e-9 * before_w
    assert ratio <= 1.25 * ratio_w
    assert err <= err_w + 0.05
    assert i.levels_run == 2                                                # 12 x 11 x 10 is below 16: no third level
    assert i.status != abi.DEMONS_UNCHANGED and i.cost_after <= i.cost_before and i.n_after >= 0.5 * i.n_before


def case_no_transform(L):
    """tform == NULL is the identity: the same field bits and info bytes as the identity passed as an Affine, and a field that
    helps on a pair that differs by the sine field alone"""
    src, _, true = recovery_pair()
    t = tuple(a + b for a, b in zip(sc.affine_coords(sc.A_IDENTITY, RDIMS), true))
    inside = sc.inside_mask(t, RDIMS)
    ref = np.where(inside, sc.trilinear(src, t, inside), np.float32(0)).astype(np.float32)
    opts = make_opts(levels=1, max_iter=6)
    g, want = register(L, src, ref, None, opts), register(L, src, ref, sc.A_IDENTITY, opts)
    check_contract(g)
    check_contract(want)
    assert np.array_equal(bits(g.field), bits(want.field)) and bytes(g.info) == bytes(want.info)
    assert g.info.status == abi.DEMONS_MAX_ITER and g.info.levels_run == 1 and g.info.iters == 6 and g.info.passes == 8
    assert g.info.cost_after < g.info.cost_before
    zero = tuple(np.zeros_like(c) for c in true)
    assert field_error(field_components(g.field), true) < field_error(zero, true)


def case_normalized(L):
    """a reference with a gain and an offset: z-scored intensities (normalize = 1) still recover the deformation"""
    src, ref, true = recovery_pair()
    scaled = (ref * np.float32(2.5) + np.float32(10)).astype(np.float32)
    g = register(L, src, scaled, sc.A_FIXED, make_opts(levels=1, max_iter=6, normalize=1))
    check_contract(g)
    zero = tuple(np.zeros_like(c) for c in true)
    err, err_0 = field_error(field_components(g.field), true), field_error(zero, true)
    print("field error, z-scored", err, "zero field", err_0)
    # (six passes at one level do not finish the job; what is asserted is that the z-scored cost is usable: the field it
    # finds lowers the cost and is nearer the true field than no field)
    assert g.info.status != abi.DEMONS_UNCHANGED and g.info.cost_after < g.info.cost_before and err < err_0


def case_hopeless(L, dev):
    """unrelated volumes: a field with a lower cost or the zero field, and info is what one more pass measures"""
    src, ref = sc._blobby(RDIMS, 21), sc._blobby(RDIMS, 99)
    g = register(L, src, ref, sc.A_FIXED, make_opts(levels=2, max_iter=6))
    check_contract(g)
    u = field_components(g.field)
    _, sums = kernel_step(dev, src, ref, sc.A_FIXED, u, RAW, 0.25)
    assert sums[1] == g.info.n_after and sums[0] / sums[1] == g.info.cost_after
    norm = np.sqrt(sum(c.astype(np.float64) ** 2 for c in u))
    assert abs(g.info.mean_disp - norm.mean()) <= 1e-12 * max(1.0, norm.mean())
    assert abs(g.info.max_disp - norm.max()) <= np.spacing(norm.max())


def case_forms_agree(L, dev, tmp_path, opts):
    """the device-pointer entry against the host form on the recovery pair (opts: the recovery case's, whose host-form result is
    shared with it, or the same with fewer passes where a call is slow); the field through write_nii / read_nii; the field warp
    against the kernel"""
    src, ref, _ = recovery_pair()
    want = library_recovery(L) if opts.max_iter == 50 else register(L, src, ref, sc.A_FIXED, opts)
    assert want.rc == 0 and want.info.status != abi.DEMONS_UNCHANGED and want.info.levels_run == 2
    n = ref.size
    info, t = abi.DemonsInfo(), sc.make_affine(L, sc.A_FIXED)
    bufs = [dev.upload(src), dev.upload(ref), dev.upload(np.full(3 * n, -3.5, np.float32))]
    try:
        rc = L.sift.sift3d_amd_register_demons_dev(bufs[0], *src.shape[::-1], bufs[1], *ref.shape[::-1], C.addressof(t), C.byref(opts),
                                                   bufs[2], C.byref(info), None)
        flat = dev.download(bufs[2], (3, n), np.float32)
    finally:
        for b in bufs:
            dev.free(b)
    u = field_components(want.field)
    assert rc == 0 and np.array_equal(bits(flat), bits(planar(u))) and bytes(info) == bytes(want.info)
    # the field as a 4-D NIfTI and back
    u_ = L.imutil
    u_.im_write.argtypes = [C.c_char_p, P(abi.Image)]
    u_.im_read.argtypes = [C.c_char_p, P(abi.Image)]
    im, back, warped = L.image_from_numpy(want.field, (1, 1, 1)), abi.Image(), abi.Image()
    u_.init_im(C.byref(back))
    u_.init_im(C.byref(warped))
    s_im = L.image_from_numpy(src, (1, 1, 1))
    path = str(tmp_path / "field.nii.gz").encode()
    try:
        assert u_.im_write(path, C.byref(im)) == 0 and u_.im_read(path, C.byref(back)) == 0
        assert (back.nx, back.ny, back.nz, back.nc) == (RDIMS[0], RDIMS[1], RDIMS[2], 3)
        assert np.array_equal(bits(L.image_to_numpy(back)), bits(want.field))
        for interp in (0, 1):
            assert L.sift.sift3d_amd_im_warp_field(C.addressof(t), C.byref(back), C.byref(s_im), interp, C.byref(warped)) == 0
            assert (warped.nx, warped.ny, warped.nz, warped.nc) == (RDIMS[0], RDIMS[1], RDIMS[2], 1)
            got = L.image_to_numpy(warped)
            assert np.array_equal(bits(got), bits(kernel_warp(dev, src, RDIMS, sc.A_FIXED, u, interp)))
        # the warp through the field agrees with ref better than the warp through the affine map alone
        lin = kernel_warp(dev, src, RDIMS, sc.A_FIXED, u, 0).astype(np.float64)
        aff = kernel_warp(dev, src, RDIMS, sc.A_FIXED, None, 0, affine_only=True).astype(np.float64)
        assert ((lin - ref) ** 2).mean() < 0.5 * ((aff - ref) ** 2).mean()
    finally:
        u_.cleanup_tform(C.byref(t))
        for i_ in (im, back, warped, s_im):
            L.free_image(i_)


def case_refusals(L):
    """each failure returns SIFT3D_FAILURE with a message and leaves the field and info untouched"""
    u = L.imutil
    ref, src = sc.volumes("70x33x9", clean=True)
    ims = {"src": L.image_from_numpy(src, (1, 1, 1)), "ref": L.image_from_numpy(ref, (1, 1, 1)),
           "nc2": L.image_from_numpy(np.zeros((14, 15, 16, 2), np.float32), (1, 1, 1)),
           "thin": L.image_from_numpy(np.ascontiguousarray(src[:1]), (1, 1, 1)),
           "small": L.image_from_numpy(np.ascontiguousarray(ref[:6]), (1, 1, 1))}
    good = sc.make_affine(L, sc.A_FIXED)
    from tests import tps_cases as tc
    tc.bind(L)
    ctrl, params = tc.warp_inputs(4, 1, (70, 33, 9))[1:]
    tps = tc.make_tps(L, ctrl, params)
    flat = abi.Affine()
    u.init_Affine.argtypes = [P(abi.Affine), C.c_int]
    assert u.init_Affine(C.byref(flat), 2) == 0                         # a 2-D affine
    nan = math.nan
    field = L.image_from_numpy(np.full((2, 3, 4, 3), 5.0, np.float32), (1, 1, 1))
    cases = [("a Tps", tps, "src", "ref", make_opts(), True), ("a 2-D affine", flat, "src", "ref", make_opts(), True),
             ("nc 2 source", good, "nc2", "ref", make_opts(), True), ("nc 2 reference", good, "src", "nc2", make_opts(), True),
             ("70 x 33 x 1 source", good, "thin", "ref", make_opts(), True),
             ("a reference of 6 planes under a Gaussian of half width 5", good, "src", "small", make_opts(), True),
             ("sigma 0.2", good, "src", "ref", make_opts(sigma=0.2), True), ("sigma 9", good, "src", "ref", make_opts(sigma=9.0), True),
             ("sigma NaN", good, "src", "ref", make_opts(sigma=nan), True),
             ("max_step -1", good, "src", "ref", make_opts(max_step=-1.0), True),
             ("max_step NaN", good, "src", "ref", make_opts(max_step=nan), True),
             ("tol NaN", good, "src", "ref", make_opts(tol=nan), True), ("min_overlap -1", good, "src", "ref", make_opts(min_overlap=-1.0), True),
             ("levels -1", good, "src", "ref", make_opts(levels=-1), True), ("max_iter -2", good, "src", "ref", make_opts(max_iter=-2), True),
             ("normalize 2", good, "src", "ref", make_opts(normalize=2), True),
             ("a NULL field", good, "src", "ref", make_opts(), False)]
    try:
        for label, t, s, r, opts, with_field in cases:
            info = abi.DemonsInfo()
            C.memset(C.byref(info), 0xAB, C.sizeof(info))
            before = bytes(C.string_at(C.addressof(field), C.sizeof(field))) + bytes(C.string_at(field.data, 4 * 72))
            rc = L.sift.sift3d_amd_register_demons(C.byref(ims[s]), C.byref(ims[r]), C.addressof(t), C.byref(opts),
                                                   C.byref(field) if with_field else None, C.byref(info))
            assert rc == -1, label
            assert b"sift3d_amd_register_demons" in u.sift3d_amd_last_error(), label
            after = bytes(C.string_at(C.addressof(field), C.sizeof(field))) + bytes(C.string_at(field.data, 4 * 72))
            assert after == before and bytes(info) == b"\xab" * C.sizeof(info), label
        # no overlap under the map as given
        far = sc.make_affine(L, sc.A_FAR)
        info = abi.DemonsInfo()
        C.memset(C.byref(info), 0xAB, C.sizeof(info))
        rc = L.sift.sift3d_amd_register_demons(C.byref(ims["src"]), C.byref(ims["ref"]), C.addressof(far), None, C.byref(field),
                                               C.byref(info))
        u.cleanup_tform(C.byref(far))
        assert rc == -1 and b"overlap" in u.sift3d_amd_last_error() and bytes(info) == b"\xab" * C.sizeof(info)
        # the field warp: a Tps, a field of two channels
        dst = abi.Image()
        u.init_im(C.byref(dst))
        assert L.sift.sift3d_amd_im_warp_field(C.addressof(tps), C.byref(field), C.byref(ims["src"]), 0, C.byref(dst)) == -1
        assert b"sift3d_amd_im_warp_field" in u.sift3d_amd_last_error()
        assert L.sift.sift3d_amd_im_warp_field(C.addressof(good), C.byref(ims["nc2"]), C.byref(ims["src"]), 0, C.byref(dst)) == -1
        assert L.sift.sift3d_amd_im_warp_field(C.addressof(good), C.byref(field), C.byref(ims["src"]), 2, C.byref(dst)) == -1
        assert not dst.data
    finally:
        for t in (good, tps, flat):
            u.cleanup_tform(C.byref(t))
        for im in list(ims.values()) + [field]:
            L.free_image(im)


def case_struct_layouts():
    o, i = abi.DemonsOpts, abi.DemonsInfo
    assert C.sizeof(o) == 48 and (o.levels.offset, o.max_iter.offset, o.sigma.offset, o.max_step.offset, o.tol.offset,
                                  o.min_overlap.offset, o.normalize.offset) == (0, 4, 8, 16, 24, 32, 40)
    assert C.sizeof(i) == 64 and (i.status.offset, i.levels_run.offset, i.iters.offset, i.passes.offset, i.n_before.offset,
                                  i.n_after.offset, i.cost_before.offset, i.cost_after.offset, i.mean_disp.offset,
                                  i.max_disp.offset) == (0, 4, 8, 12, 16, 24, 32, 40, 48, 56)
