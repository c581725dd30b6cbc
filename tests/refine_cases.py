"""Shared by tests/test_refine.py (CPU: the SIMT emulator build of the library) and tests/test_gpu_refine.py (the device): the
inputs of the intensity-based affine refinement (sift3d_amd_refine_affine, s3d_k_affine_normal_eq), a numpy restatement of the
kernel's definition (include/s3d_device.h) and the checks both suites apply.

The restatement forms every term with the operation order the header states, as element-wise f64 numpy operations: each is
rounded once and nothing is fused, as in the kernel (compiled without contraction), so a term is reproduced bit for bit and the
sums obey the bound of any summation order, n * 2^-53 * sum |term| (similarity_cases.check_sums), with no widening (k = 0)."""
import ctypes as C
import math

import numpy as np

from sift3d_amd import abi
from tests import similarity_cases as sc

P = C.POINTER
RAW = (1.0, 0.0, 1.0, 0.0)
SCALED = (1.7, 0.3, 0.6, -0.2)
MID = np.array([[0.01, -0.008, 0.006, 1.2], [0.007, 0.012, -0.009, -0.8], [-0.006, 0.008, -0.01, 0.6]])
LARGE = np.array([[0.02, -0.015, 0.01, 2.5], [0.012, 0.02, -0.015, -1.8], [-0.01, 0.015, -0.02, 1.4]])
SUM_NAMES = tuple(f"H[{g}][{q}]" for g in ("xx", "xy", "xz", "yy", "yz", "zz")
                  for q in ("00", "01", "02", "03", "11", "12", "13", "22", "23", "33")) + \
    tuple(f"grad[{i}{k}]" for i in "xyz" for k in "0123") + ("sum r^2",)
_CACHE = {}


def centre(rdims):
    return tuple((n - 1) / 2 for n in rdims)


# ---- numpy restatement ------------------------------------------------------------------------------------------------------
class Want:
    """the 73 sums (math.fsum of the terms), the magnitude each sum's rounding is relative to, and the exact count"""

    def __init__(self, ref, src, A, consts, ctr=None):
        sa, ma, sb, mb = consts
        rd, sd = ref.shape[::-1], src.shape[::-1]
        cx, cy, cz = ctr if ctr is not None else centre(rd)
        t = sc.affine_coords(A, rd)
        inside = sc.inside_mask(t, sd)
        b = sc.trilinear(src, t, inside)
        tx, ty, tz = (np.where(inside, c, 0.0) for c in t)
        X0, Y0, Z0 = (np.minimum(np.floor(c).astype(np.int64), n - 2) for c, n in zip((tx, ty, tz), sd))
        fx, fy, fz = tx - X0, ty - Y0, tz - Z0
        ux, uy, uz = 1.0 - fx, 1.0 - fy, 1.0 - fz
        s = src.astype(np.float64)
        c000, c100, c010, c110 = s[Z0, Y0, X0], s[Z0, Y0, X0 + 1], s[Z0, Y0 + 1, X0], s[Z0, Y0 + 1, X0 + 1]
        c001, c101, c011, c111 = s[Z0 + 1, Y0, X0], s[Z0 + 1, Y0, X0 + 1], s[Z0 + 1, Y0 + 1, X0], s[Z0 + 1, Y0 + 1, X0 + 1]
        with np.errstate(invalid="ignore", over="ignore"):
            gx = ((c100 - c000) * uy + (c110 - c010) * fy) * uz + ((c101 - c001) * uy + (c111 - c011) * fy) * fz
            gy = ((c010 - c000) * ux + (c110 - c100) * fx) * uz + ((c011 - c001) * ux + (c111 - c101) * fx) * fz
            gz = ((c001 - c000) * ux + (c101 - c100) * fx) * uy + ((c011 - c010) * ux + (c111 - c110) * fx) * fy
            gx, gy, gz = sb * gx, sb * gy, sb * gz
        ok = inside & np.isfinite(ref) & np.isfinite(b) & np.isfinite(gx) & np.isfinite(gy) & np.isfinite(gz)
        self.inside, self.ok, self.n = inside, ok, int(ok.sum())
        self.dropped = int(inside.sum()) - self.n
        z, y, x = np.meshgrid(np.arange(rd[2], dtype=np.float64), np.arange(rd[1], dtype=np.float64),
                              np.arange(rd[0], dtype=np.float64), indexing="ij")
        qx, qy, qz = (x - cx)[ok], (y - cy)[ok], (z - cz)[ok]
        gx, gy, gz = gx[ok], gy[ok], gz[ok]
        a, bb = ref[ok].astype(np.float64), b[ok].astype(np.float64)
        r = sb * (bb - mb) - sa * (a - ma)
        gg = (gx * gx, gx * gy, gx * gz, gy * gy, gy * gz, gz * gz)
        qq = (qx * qx, qx * qy, qx * qz, qx, qy * qy, qy * qz, qy, qz * qz, qz, None)    # None: q_3 * q_3 = 1
        terms = [g if q is None else g * q for g in gg for q in qq]
        for rg in (r * gx, r * gy, r * gz):
            terms += [rg * qx, rg * qy, rg * qz, rg]
        terms.append(r * r)
        self.sums = np.array([math.fsum(v) for v in terms])
        self.mags = np.array([math.fsum(np.abs(v)) for v in terms])


def want(shape, A, consts, clean=False):
    key = (shape, np.asarray(A).tobytes(), consts, clean)
    if key not in _CACHE:
        ref, src = sc.volumes(shape, clean)
        _CACHE[key] = Want(ref, src, A, consts)
    return _CACHE[key]


def check_sums(got, w, label=""):
    """n exactly, each of the 73 sums within n * 2^-53 * sum |term| of the correctly rounded sum"""
    bound = w.n * 2.0 ** -53 * w.mags
    err = np.abs(got[:73] - w.sums)
    worst = int(np.argmax(err - bound))
    print(f"{label} n: got {got[73]!r}, want {w.n}; closest to its bound: {SUM_NAMES[worst]} got {got[worst]!r}, fsum "
          f"{w.sums[worst]!r}, error {err[worst]:.3e}, bound {bound[worst]:.3e}")
    assert got[73] == w.n
    assert np.isfinite(got).all()
    assert (err <= bound).all(), [(SUM_NAMES[k], err[k], bound[k]) for k in np.nonzero(err > bound)[0]]


# ---- drivers ----------------------------------------------------------------------------------------------------------------
def kernel(dev, src, ref, A, consts=RAW, ctr=None):
    """s3d_k_affine_normal_eq on dev -> the 74 sums"""
    bufs = [dev.upload(src), dev.upload(ref)]
    try:
        return dev.affine_normal_eq(bufs[0], src.shape[::-1], bufs[1], ref.shape[::-1], A,
                                    ctr if ctr is not None else centre(ref.shape[::-1]), consts)
    finally:
        for b in bufs:
            dev.free(b)


def make_opts(levels=0, max_iter=0, tol=0.0, min_overlap=0.0, normalize=0):
    o = abi.RefineOpts()
    o.levels, o.max_iter, o.tol, o.min_overlap, o.normalize = levels, max_iter, tol, min_overlap, normalize
    return o


def affine_bytes(t):
    return C.string_at(t.A.data, 96)


class Refined:
    def __init__(self, rc, before, after, info, err):
        self.rc, self.before, self.after, self.info, self.err = rc, before, after, info, err
        self.A = np.frombuffer(after, np.float64).reshape(3, 4)


def refine(L, src, ref, A, opts=None):
    """sift3d_amd_refine_affine of library L on numpy volumes [z, y, x] from the map A"""
    ims = [L.image_from_numpy(v, (1, 1, 1)) for v in (src, ref)]
    t, info = sc.make_affine(L, A), abi.RefineInfo()
    C.memset(C.byref(info), 0xAB, C.sizeof(info))
    before = affine_bytes(t)
    try:
        rc = L.sift.sift3d_amd_refine_affine(C.byref(ims[0]), C.byref(ims[1]), None if opts is None else C.byref(opts),
                                             C.byref(t), C.byref(info))
        return Refined(rc, before, affine_bytes(t), info, L.imutil.sift3d_amd_last_error() or b"")
    finally:
        L.imutil.cleanup_tform(C.byref(t))
        for im in ims:
            L.free_image(im)


def corner_error(A, B, rdims):
    """the largest displacement of a corner of the reference volume between the maps A and B"""
    nx, ny, nz = rdims
    p = np.array([[x, y, z, 1.0] for x in (0, nx - 1) for y in (0, ny - 1) for z in (0, nz - 1)])
    return float(np.sqrt((((np.asarray(A) - np.asarray(B)) @ p.T) ** 2).sum(0)).max())


def check_contract(g, min_overlap=0.5):
    """success, and either a map that is no worse at level 0 or the map as given, bit for bit"""
    i = g.info
    print(f"status {i.status}, levels {i.levels_run}, iters {i.iters}, passes {i.passes}, n {i.n_before} -> {i.n_after}, cost "
          f"{i.cost_before!r} -> {i.cost_after!r}, shift {i.max_corner_shift!r}")
    assert g.rc == 0, g.err
    if i.status == abi.REFINE_UNCHANGED:
        assert g.after == g.before
    else:
        assert i.cost_after <= i.cost_before and i.n_after >= min_overlap * i.n_before


# ---- the cases both suites run (L: the library behind the C API, dev: its flat device entry points) --------------------------
def case_kernel(dev, shape, consts):
    ref, src = sc.volumes(shape)
    w = want(shape, sc.A_FIXED, consts)
    assert int(w.inside.sum()) == sc.SHAPES[shape][2]
    assert 2 < w.dropped <= 2 + 2 * 27                                  # two of ref; a source voxel is a corner of up to 27 cells
    check_sums(kernel(dev, src, ref, sc.A_FIXED, consts), w, f"{shape} {consts}")


def case_shifted_lattice(dev):
    """every sample on a lattice point: floor == ceil in the sample, the gradient one-sided"""
    ref, src = sc.volumes("70x33x9", clean=True)
    w = want("70x33x9", sc.A_SHIFT, RAW, clean=True)
    got = kernel(dev, src, ref, sc.A_SHIFT)
    assert got[73] == sc.KEPT_SHIFT == w.n
    check_sums(got, w, "shift")
    assert got[:60].any()


def case_identity(dev):
    """the reference against itself: no residual, and the last planes count through the clipped cell"""
    ref, _ = sc.volumes("70x33x9", clean=True)
    got = kernel(dev, ref, ref, sc.A_IDENTITY)
    assert got[73] == ref.size
    assert got[72] == 0.0 and (got[60:72] == 0.0).all()
    check_sums(got, Want(ref, ref, sc.A_IDENTITY, RAW), "identity")
    assert all(got[k] > 0 for k in (0, 30, 50))                         # H[xx][00], H[yy][00], H[zz][00]


def case_no_overlap(dev, L):
    ref, src = sc.volumes("70x33x9", clean=True)
    got = kernel(dev, src, ref, sc.A_FAR)
    assert (got == 0.0).all()
    g = refine(L, src, ref, sc.A_FAR)
    assert g.rc == -1 and b"sift3d_amd_refine_affine" in g.err and b"overlap" in g.err
    assert g.after == g.before and bytes(g.info) == b"\xab" * C.sizeof(g.info)


def case_scratch_guard(dev):
    """a dirty scratch does not reach the sums, and nothing is written behind its stated size"""
    ref, src = sc.volumes("257x19x5")
    rd, sd = ref.shape[::-1], src.shape[::-1]
    L = dev.L
    nbytes, guard = int(L.s3d_k_affine_normal_eq_scratch_bytes(*rd)), 4096
    assert nbytes > 0 and nbytes % (74 * 8) == 0
    bufs = [dev.upload(src), dev.upload(ref), dev.malloc(74 * 8), dev.malloc(nbytes + guard)]
    A = np.ascontiguousarray(sc.A_FIXED).ctypes.data_as(P(C.c_double))
    ctr = np.array(centre(rd)).ctypes.data_as(P(C.c_double))
    try:
        dev.check(L.s3d_rt_memset(bufs[3], 0xA5, nbytes + guard, None))
        dev.check(L.s3d_k_affine_normal_eq(bufs[0], *sd, bufs[1], *rd, A, ctr, *RAW, bufs[2], bufs[3], None))
        got = dev.download(bufs[2], (74,), np.float64)
        tail = dev.download(bufs[3] + nbytes, (guard,), np.uint8)
    finally:
        for b in bufs:
            dev.free(b)
    assert (tail == 0xA5).all()
    check_sums(got, want("257x19x5", sc.A_FIXED, RAW), "dirty scratch")


def case_flat_refusals(dev):
    """a zero dimension, a source dimension of 1 and NULL buffers: non-zero, a message, the outputs untouched"""
    ref, src = sc.volumes("70x33x9", clean=True)
    L = dev.L
    assert L.s3d_k_affine_normal_eq_scratch_bytes(70, 33, 9) > 0
    for bad in ((0, 33, 9), (70, 0, 9), (70, 33, -1)):
        assert L.s3d_k_affine_normal_eq_scratch_bytes(*bad) == 0
    mark = np.full(74, -7.5)
    bufs = [dev.upload(src), dev.upload(ref), dev.upload(mark), dev.upload(np.full(74 * 2048, -7.5))]
    A = np.ascontiguousarray(sc.A_FIXED).ctypes.data_as(P(C.c_double))
    ctr = np.array(centre((70, 33, 9))).ctypes.data_as(P(C.c_double))
    sd, rd = (61, 37, 11), (70, 33, 9)
    s, r, o, w = bufs
    try:
        for args in ((s, (0, 37, 11), r, rd, A, ctr, o, w), (s, sd, r, (70, 0, 9), A, ctr, o, w), (s, (61, 37, 1), r, rd, A, ctr, o, w),
                     (s, (1, 37, 11), r, rd, A, ctr, o, w), (s, (61, 1, 11), r, rd, A, ctr, o, w), (None, sd, r, rd, A, ctr, o, w),
                     (s, sd, None, rd, A, ctr, o, w), (s, sd, r, rd, None, ctr, o, w), (s, sd, r, rd, A, None, o, w),
                     (s, sd, r, rd, A, ctr, None, w), (s, sd, r, rd, A, ctr, o, None),
                     (s, sd, r, (70, 65536, 32768), A, ctr, o, w)):           # more rows than the grid's 32-bit index holds
            a_s, a_sd, a_r, a_rd, a_A, a_c, a_o, a_w = args
            assert L.s3d_k_affine_normal_eq(a_s, *a_sd, a_r, *a_rd, a_A, a_c, *RAW, a_o, a_w, None) != 0 and dev.err()
        dev.sync()
        assert np.array_equal(dev.download(o, (74,), np.float64), mark)
        assert (dev.download(w, (74 * 2048,), np.float64) == -7.5).all()
    finally:
        for b in bufs:
            dev.free(b)


def case_determinism(dev):
    ref, src = sc.volumes("257x19x5")
    s1, s2 = kernel(dev, src, ref, sc.A_FIXED, SCALED), kernel(dev, src, ref, sc.A_FIXED, SCALED)
    assert np.array_equal(s1.view(np.uint64), s2.view(np.uint64)) and s1.any()


def case_consistent_with_the_score(L, dev):
    ref, src = sc.volumes("70x33x9", clean=True)
    got = kernel(dev, src, ref, sc.A_FIXED)
    t = sc.make_affine(L, sc.A_FIXED)
    g = sc.similarity(L, t, src, ref, None, 64)
    L.imutil.cleanup_tform(C.byref(t))
    assert g.rc == 0 and got[73] == g.n > 0
    assert abs(got[72] / got[73] - g.stats["mse"]) <= 1e-9 * g.stats["mse"]


RDIMS = (48, 44, 40)


def case_starts():
    assert abs(corner_error(sc.A_FIXED + MID, sc.A_FIXED, RDIMS) - 2.075) < 5e-4
    assert abs(corner_error(sc.A_FIXED + LARGE, sc.A_FIXED, RDIMS) - 4.244) < 5e-4


def case_clean_mid(L):
    ref, src = sc.meaning_volumes()
    g = refine(L, src, ref, sc.A_FIXED + MID, make_opts(levels=1))
    check_contract(g)
    err = corner_error(g.A, sc.A_FIXED, RDIMS)
    print("error", err)
    i = g.info
    assert err < 0.01 and i.cost_after < 1e-3 * i.cost_before and i.n_after >= i.n_before
    assert i.status == abi.REFINE_CONVERGED and i.iters <= 10 and i.levels_run == 1 and i.passes >= i.iters + 1
    assert abs(i.max_corner_shift - corner_error(g.A, sc.A_FIXED + MID, RDIMS)) < 1e-9


def case_clean_large(L):
    ref, src = sc.meaning_volumes()
    g = refine(L, src, ref, sc.A_FIXED + LARGE, make_opts(levels=2))
    check_contract(g)
    err = corner_error(g.A, sc.A_FIXED, RDIMS)
    print("error", err)
    assert err < 0.01 and g.info.levels_run == 2


def case_noisy(L):
    ref, src = sc.meaning_volumes()
    noisy = (ref + np.float32(0.1 * src.std()) * np.random.default_rng(5).standard_normal(ref.shape).astype(np.float32))
    g = refine(L, src, noisy.astype(np.float32), sc.A_FIXED + MID, make_opts(levels=1))
    check_contract(g)
    err = corner_error(g.A, sc.A_FIXED, RDIMS)
    print("error", err)
    assert err < 0.1


def case_gain_offset(L):
    ref, src = sc.meaning_volumes()
    scaled = (ref * np.float32(2.5) + np.float32(10)).astype(np.float32)
    g = refine(L, src, scaled, sc.A_FIXED + MID, make_opts(levels=1, normalize=1))
    check_contract(g)
    err = corner_error(g.A, sc.A_FIXED, RDIMS)
    print("error, z-scored", err)
    assert err < 0.5 and g.info.status != abi.REFINE_UNCHANGED
    # raw SSD runs away on this pair (the restatement ends 53 voxels off): the contract only.  It holds wherever the loop stops,
    # so three accepted steps, which meet accepted and rejected steps alike, check what thirty would
    check_contract(refine(L, src, scaled, sc.A_FIXED + MID, make_opts(levels=1, max_iter=3)))


def case_already_optimal(L):
    ref, src = sc.meaning_volumes()
    g = refine(L, src, ref, sc.A_FIXED)
    check_contract(g)
    assert g.info.max_corner_shift < 1e-6 and g.info.cost_after <= g.info.cost_before and g.info.iters <= 2


def case_unrelated(L):
    ref, src = sc.volumes("70x33x9", clean=True)
    g = refine(L, src, ref, sc.A_FIXED, make_opts(max_iter=5))           # (the contract does not depend on where the loop stops)
    check_contract(g)
    assert g.info.n_before == sc.SHAPES["70x33x9"][2] and g.info.n_after >= 0.5 * g.info.n_before


def case_refusals(L):
    """each failure returns SIFT3D_FAILURE with a message and leaves the affine and info untouched"""
    u = L.imutil
    ref, src = sc.volumes("70x33x9", clean=True)
    ims = {"src": L.image_from_numpy(src, (1, 1, 1)), "ref": L.image_from_numpy(ref, (1, 1, 1)),
           "nc2": L.image_from_numpy(np.zeros((4, 5, 6, 2), np.float32), (1, 1, 1)),
           "thin": L.image_from_numpy(np.ascontiguousarray(src[:1]), (1, 1, 1))}
    assert (ims["thin"].nx, ims["thin"].ny, ims["thin"].nz) == (61, 37, 1)
    good = sc.make_affine(L, sc.A_FIXED)
    from tests import tps_cases as tc
    tc.bind(L)
    ctrl, params = tc.warp_inputs(4, 1, (70, 33, 9))[1:]
    tps = tc.make_tps(L, ctrl, params)
    nan = math.nan
    cases = [("nc 2 source", good, "nc2", "ref", make_opts()), ("nc 2 reference", good, "src", "nc2", make_opts()),
             ("70 x 33 x 1 source", good, "thin", "ref", make_opts()), ("a Tps", tps, "src", "ref", make_opts()),
             ("tol NaN", good, "src", "ref", make_opts(tol=nan)), ("min_overlap -1", good, "src", "ref", make_opts(min_overlap=-1.0)),
             ("min_overlap NaN", good, "src", "ref", make_opts(min_overlap=nan)), ("tol -1", good, "src", "ref", make_opts(tol=-1.0)),
             ("levels -1", good, "src", "ref", make_opts(levels=-1)), ("max_iter -2", good, "src", "ref", make_opts(max_iter=-2)),
             ("normalize -1", good, "src", "ref", make_opts(normalize=-1))]
    try:
        for label, t, s, r, opts in cases:
            info = abi.RefineInfo()
            C.memset(C.byref(info), 0xAB, C.sizeof(info))
            before = bytes(C.string_at(C.addressof(t), C.sizeof(t))) + (affine_bytes(t) if t is good else b"")
            rc = L.sift.sift3d_amd_refine_affine(C.byref(ims[s]), C.byref(ims[r]), C.byref(opts), C.cast(C.pointer(t), P(abi.Affine)),
                                                 C.byref(info))
            assert rc == -1, label
            assert b"sift3d_amd_refine_affine" in u.sift3d_amd_last_error(), label
            after = bytes(C.string_at(C.addressof(t), C.sizeof(t))) + (affine_bytes(t) if t is good else b"")
            assert after == before and bytes(info) == b"\xab" * C.sizeof(info), label
    finally:
        u.cleanup_tform(C.byref(good))
        u.cleanup_tform(C.byref(tps))
        for im in ims.values():
            L.free_image(im)


def case_struct_layouts():
    o, i = abi.RefineOpts, abi.RefineInfo
    assert C.sizeof(o) == 32 and (o.levels.offset, o.max_iter.offset, o.tol.offset, o.min_overlap.offset, o.normalize.offset) == \
        (0, 4, 8, 16, 24)
    assert C.sizeof(i) == 56 and (i.status.offset, i.levels_run.offset, i.iters.offset, i.passes.offset, i.n_before.offset,
                                  i.n_after.offset, i.cost_before.offset, i.cost_after.offset, i.max_corner_shift.offset) == \
        (0, 4, 8, 12, 16, 24, 32, 40, 48)
