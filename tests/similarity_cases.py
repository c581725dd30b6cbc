"""Shared by tests/test_similarity.py (CPU: the SIMT emulator build of the library) and tests/test_gpu_similarity.py (the
device): the inputs of the similarity scores (sift3d_amd_im_similarity), a numpy restatement of their definition
(include/sift3d_amd.h) and the checks both suites apply.

The restatement is exact where the definition is: the affine coordinates and the tri-linear sample are element-wise f64
operations in the kernels' order (s3d_affine_xyz, s3d_sample_store in sift3d_amd/csrc/s3d_resample.hip), which numpy evaluates
with the same roundings; the bin rule likewise; the seven sums are math.fsum, correctly rounded."""
import ctypes as C
import math
import os

import numpy as np

from sift3d_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = C.POINTER

A_FIXED = np.array([[0.97, 0.05, -0.02, 1.5], [-0.04, 1.02, 0.03, -2.25], [0.01, -0.03, 0.95, 0.75]])
A_IDENTITY = np.array([[1.0, 0, 0, 0], [0, 1.0, 0, 0], [0, 0, 1.0, 0]])
A_SHIFT = np.array([[1.0, 0, 0, 3.0], [0, 1.0, 0, -2.0], [0, 0, 1.0, 1.0]])
A_FAR = np.array([[1.0, 0, 0, 1000.0], [0, 1.0, 0, 0], [0, 0, 1.0, 0]])
# (reference dims, source dims) as (nx, ny, nz), and how many reference voxels A_FIXED keeps inside the source (counted with
# numpy when the cases were chosen): rows that are no multiple of 64, and a row that crosses 256
SHAPES = {"70x33x9": ((70, 33, 9), (61, 37, 11), 15677), "257x19x5": ((257, 19, 5), (250, 21, 6), 12215)}
KEPT_SHIFT = 16182                                                     # A_SHIFT on the first shape
BINS = [2, 37, 64, 128]
SUM_NAMES = ("sum a'", "sum b'", "sum a'^2", "sum b'^2", "sum a'b'", "sum (a-b)^2", "sum |a-b|")
FIELDS = ("mean_ref", "mean_src", "var_ref", "var_src", "mse", "mae", "ncc", "h_ref", "h_src", "h_joint", "mi", "nmi")


# ---- inputs -----------------------------------------------------------------------------------------------------------------
_CACHE = {}


def _blobby(dims, seed):
    """seeded noise plus a few Gaussian blobs, [z, y, x] float32"""
    nx, ny, nz = dims
    rng = np.random.default_rng(seed)
    v = rng.standard_normal((nz, ny, nx)) * 0.1
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    for _ in range(5):
        c = rng.random(3) * (nx, ny, nz)
        s = 2.0 + 3.0 * rng.random()
        v += (0.5 + rng.random()) * np.exp(-((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2) / (2 * s * s))
    return v.astype(np.float32)


def volumes(shape, clean=False):
    """(ref, src) of a shape of SHAPES.  Unless clean: one NaN and one +inf voxel on each side, inside the overlap under A_FIXED,
    and the reference's largest finite voxel at its centre, which A_FIXED maps inside the source (it sits exactly on ref_hi)."""
    key = (shape, clean)
    if key not in _CACHE:
        rd, sd, _ = SHAPES[shape]
        ref, src = _blobby(rd, 11), _blobby(sd, 12)
        if not clean:
            cz, cy, cx = rd[2] // 2, rd[1] // 2, rd[0] // 2
            ref[cz, cy, cx] = np.float32(3.25)                         # above everything else: the finite maximum
            ref[cz, cy - 3, cx + 4] = np.nan
            ref[cz - 1, cy + 2, cx - 5] = np.inf
            src[sd[2] // 2, sd[1] // 2, sd[0] // 2] = np.nan
            src[sd[2] // 2 + 1, sd[1] // 2 - 4, sd[0] // 2 + 6] = np.inf
        for a in (ref, src):
            a.setflags(write=False)
        _CACHE[key] = (ref, src)
    return _CACHE[key]


def meaning_volumes():
    """48 x 44 x 40 blob volume as the source; the reference is the source warped by A_FIXED (restated tri-linear warp)"""
    if "meaning" not in _CACHE:
        from sift3d_amd import synth
        src = synth.blobs(48, 44, 40, 500, 21)
        t = affine_coords(A_FIXED, (48, 44, 40))
        inside = inside_mask(t, (48, 44, 40))
        ref = np.where(inside, trilinear(src, t, inside), np.float32(0)).astype(np.float32)
        for a in (ref, src):
            a.setflags(write=False)
        _CACHE["meaning"] = (ref, src)
    return _CACHE["meaning"]


# ---- numpy restatement ------------------------------------------------------------------------------------------------------
def affine_coords(A, rdims):
    """(tx, ty, tz), each [z, y, x] float64: A [x y z 1]^T left to right, every operation rounded"""
    nx, ny, nz = rdims
    z, y, x = np.meshgrid(np.arange(nz, dtype=np.float64), np.arange(ny, dtype=np.float64), np.arange(nx, dtype=np.float64),
                          indexing="ij")
    A = np.asarray(A, np.float64)
    return tuple(A[r, 0] * x + A[r, 1] * y + A[r, 2] * z + A[r, 3] for r in range(3))


def inside_mask(t, sdims):
    tx, ty, tz = t
    outside = (tx < 0) | (tx > sdims[0] - 1) | (ty < 0) | (ty > sdims[1] - 1) | (tz < 0) | (tz > sdims[2] - 1)
    return ~(outside | np.isnan(tx) | np.isnan(ty) | np.isnan(tz))


def trilinear(src, t, inside):
    """the float32 that s3d_sample_store<linear> stores at the inside voxels (anything elsewhere)"""
    tx, ty, tz = (np.where(inside, c, 0.0) for c in t)
    fx, fy, fz = (np.floor(c).astype(np.int64) for c in (tx, ty, tz))
    cx, cy, cz = (np.ceil(c).astype(np.int64) for c in (tx, ty, tz))
    dx, dy, dz = tx - fx, ty - fy, tz - fz
    s = src.astype(np.float64)
    c0, c1, c2, c3 = s[fz, fy, fx], s[fz, cy, fx], s[fz, fy, cx], s[fz, cy, cx]
    c4, c5, c6, c7 = s[cz, fy, fx], s[cz, cy, fx], s[cz, fy, cx], s[cz, cy, cx]
    with np.errstate(invalid="ignore", over="ignore"):
        v = (c0 * (1.0 - dx) * (1.0 - dy) * (1.0 - dz) + c1 * (1.0 - dx) * dy * (1.0 - dz) +
             c2 * dx * (1.0 - dy) * (1.0 - dz) + c3 * dx * dy * (1.0 - dz) +
             c4 * (1.0 - dx) * (1.0 - dy) * dz + c5 * (1.0 - dx) * dy * dz +
             c6 * dx * (1.0 - dy) * dz + c7 * dx * dy * dz)
        return v.astype(np.float32)


def finite_range(v):
    f = v[np.isfinite(v)]
    return float(f.min()), float(f.max())


def bin_index(v, lo, hi, bins):
    scale = bins / (hi - lo) if hi > lo else 0.0
    t = (v.astype(np.float64) - lo) * scale
    return np.where(t < 0, 0, np.where(t >= bins, bins - 1, np.minimum(t, bins - 1).astype(np.int64)))


class Want:
    """the definition applied to the pairs (a, b) of the voxels in `mask`: histogram, exact sums, the magnitude each sum's
    rounding is relative to, and the derived statistics"""

    def __init__(self, ref, b, mask, bins, ref_range=None, src_range=None, src=None):
        ok = mask & np.isfinite(ref) & np.isfinite(b)
        self.rr = ref_range or finite_range(ref)
        self.sr = src_range or finite_range(src)
        self.bins, self.ok = bins, ok
        a, bb = ref[ok].astype(np.float64), b[ok].astype(np.float64)
        self.n, self.n_total = int(ok.sum()), ref.size
        self.ia, self.ib = bin_index(ref[ok], *self.rr, bins), bin_index(b[ok], *self.sr, bins)
        self.hist = np.zeros((bins, bins), np.uint64)
        np.add.at(self.hist, (self.ia, self.ib), 1)
        self.c = (0.5 * (self.rr[0] + self.rr[1]), 0.5 * (self.sr[0] + self.sr[1]))
        ap, bp, d = a - self.c[0], bb - self.c[1], a - bb
        terms = (ap, bp, ap * ap, bp * bp, ap * bp, d * d, np.abs(d))
        self.sums = np.array([math.fsum(t) for t in terms])
        self.mags = np.array([math.fsum(np.abs(t)) for t in terms])
        self.stats = derive(self.hist, self.sums, self.c)


def entropy(counts, n):
    p = counts[counts > 0].astype(np.float64) / n
    return float(-(p * np.log(p)).sum())


def derive(hist, sums, c):
    """the statistics of include/sift3d_amd.h from a histogram and seven sums"""
    n = int(hist.sum())
    if n == 0:
        return dict.fromkeys(FIELDS, math.nan)
    ma, mb = sums[0] / n, sums[1] / n
    va, vb = sums[2] / n - ma * ma, sums[3] / n - mb * mb
    cov = sums[4] / n - ma * mb
    h_ref, h_src, h_joint = entropy(hist.sum(1), n), entropy(hist.sum(0), n), entropy(hist.ravel(), n)
    return {"mean_ref": c[0] + ma, "mean_src": c[1] + mb, "var_ref": va, "var_src": vb, "mse": sums[5] / n, "mae": sums[6] / n,
            "ncc": cov / math.sqrt(va * vb) if va > 0 and vb > 0 else math.nan, "h_ref": h_ref, "h_src": h_src,
            "h_joint": h_joint, "mi": h_ref + h_src - h_joint, "nmi": (h_ref + h_src) / h_joint if h_joint != 0 else math.nan}


def want_affine(shape, A, bins, clean=False):
    key = ("want", shape, np.asarray(A).tobytes(), bins, clean)
    if key not in _CACHE:
        ref, src = volumes(shape, clean)
        rd, sd, _ = SHAPES[shape]
        t = affine_coords(A, rd)
        inside = inside_mask(t, sd)
        w = Want(ref, trilinear(src, t, inside), inside, bins, src=src)
        w.inside = inside
        _CACHE[key] = w
    return _CACHE[key]


# ---- drivers ----------------------------------------------------------------------------------------------------------------
def bind(L):
    u = L.imutil
    u.init_Mat_rm.argtypes = [P(abi.Mat_rm), C.c_int, C.c_int, C.c_int, C.c_int]
    u.cleanup_Mat_rm.argtypes = [P(abi.Mat_rm)]
    u.cleanup_Mat_rm.restype = None
    u.init_tform.argtypes = [C.c_void_p, C.c_int]
    u.Affine_set_mat.argtypes = [P(abi.Mat_rm), P(abi.Affine)]
    u.cleanup_tform.argtypes = [C.c_void_p]
    u.cleanup_tform.restype = None
    u.init_Tps.argtypes = [P(abi.Tps), C.c_int, C.c_int]
    u.im_inv_transform.argtypes = [C.c_void_p, P(abi.Image), C.c_int, C.c_int, P(abi.Image)]
    u.sift3d_amd_last_error.restype = C.c_char_p
    return L


def make_affine(L, A):
    t, m = abi.Affine(), abi.Mat_rm()
    A = np.ascontiguousarray(A, np.float64)
    assert L.imutil.init_tform(C.byref(t), 0) == 0 and L.imutil.init_Mat_rm(C.byref(m), 3, 4, 0, 0) == 0
    C.memmove(m.data, A.ctypes.data, A.nbytes)
    assert L.imutil.Affine_set_mat(C.byref(m), C.byref(t)) == 0
    L.imutil.cleanup_Mat_rm(C.byref(m))
    return t


def make_opts(bins=0, interp=0, ref_range=(0.0, 0.0), src_range=(0.0, 0.0)):
    o = abi.SimilarityOpts()
    o.bins, o.interp = bins, interp
    o.ref_range[0], o.ref_range[1] = ref_range
    o.src_range[0], o.src_range[1] = src_range
    return o


class Got:
    def __init__(self, rc, out, joint, bins):
        self.rc, self.out, self.hist = rc, out, joint.reshape(bins, bins)
        self.n, self.n_total = out.n, out.n_total
        self.stats = {f: getattr(out, f) for f in FIELDS}


def similarity(L, tform, src, ref, opts=None, bins=64):
    """sift3d_amd_im_similarity of library L on numpy volumes [z, y, x]; tform: None or a ctypes transform of L"""
    ims = [L.image_from_numpy(v, (1, 1, 1)) for v in (src, ref)]
    out, joint = abi.Similarity(), np.full(bins * bins, 0xDEADBEEF, np.uint64)
    try:
        rc = L.imutil.sift3d_amd_im_similarity(None if tform is None else C.addressof(tform), C.byref(ims[0]), C.byref(ims[1]),
                                               None if opts is None else C.byref(opts), C.byref(out), joint.ctypes.data)
    finally:
        for im in ims:
            L.free_image(im)
    return Got(rc, out, joint, bins)


def warp(L, tform, src, rdims, interp, nc_fill=7.0):
    """the library's own im_inv_transform of src onto a grid of rdims -> [z, y, x]"""
    im = L.image_from_numpy(src, (1, 1, 1))
    dst = L.image_from_numpy(np.full(rdims[::-1], nc_fill, np.float32), (1, 1, 1))
    try:
        assert L.imutil.im_inv_transform(C.addressof(tform), C.byref(im), interp, 0, C.byref(dst)) == 0
        return L.image_to_numpy(dst)
    finally:
        L.free_image(im), L.free_image(dst)


# ---- checks -----------------------------------------------------------------------------------------------------------------
def check_sums(got_sums, want, label=""):
    """each of the seven sums within n * 2^-53 * sum |term| of the correctly rounded sum: the bound of ANY order of summation
    (every partial sum is at most sum |term| in magnitude and each of the n - 1 additions rounds once, to half an ulp)"""
    bound = want.n * 2.0 ** -53 * want.mags
    err = np.abs(np.asarray(got_sums) - want.sums)
    for k, name in enumerate(SUM_NAMES):
        print(f"{label} {name}: got {got_sums[k]!r}, fsum {want.sums[k]!r}, error {err[k]:.3e}, bound {bound[k]:.3e}")
    assert (err <= bound).all()


def check_stats(got, want_stats, hist):
    """derived statistics within 1e-9 relative of the same formulas on the exact sums; entropies, mi and nmi within 1e-10 of
    numpy's on the same integer histogram (B^2 * eps * 0.37, the largest |p log p|, with two orders of margin)"""
    for f in FIELDS:
        g, w = got.stats[f], want_stats[f]
        print(f"{f}: got {g!r}, want {w!r}")
        if math.isnan(w):
            assert math.isnan(g), f
        elif f in ("h_ref", "h_src", "h_joint", "mi", "nmi"):
            assert abs(g - w) <= 1e-10, f
        else:
            assert abs(g - w) <= 1e-9 * abs(w), f
    n = int(hist.sum())
    assert abs(got.stats["h_joint"] - entropy(hist.ravel(), n)) <= 1e-10


def check_against(got, want, label=""):
    """a result of the public entry point against the restatement: counts and histogram exactly, the sums through the flat
    entry elsewhere, the statistics to their bounds"""
    assert got.rc == 0
    assert (got.n, got.n_total) == (want.n, want.n_total), label
    assert int(got.hist.sum()) == got.n
    assert np.array_equal(got.hist, want.hist), label
    check_stats(got, want.stats, want.hist)


def kernel_affine(dev, src, ref, A, bins, want, interp=0):
    """s3d_k_similarity_affine on dev with the restatement's ranges and pivots -> (hist, sums)"""
    bufs = [dev.upload(src), dev.upload(ref)]
    try:
        rs = bins / (want.rr[1] - want.rr[0]) if want.rr[1] > want.rr[0] else 0.0
        ss = bins / (want.sr[1] - want.sr[0]) if want.sr[1] > want.sr[0] else 0.0
        return dev.similarity_affine(bufs[0], src.shape[::-1], bufs[1], ref.shape[::-1], A, interp, bins, want.rr[0], rs,
                                     want.sr[0], ss, want.c[0], want.c[1])
    finally:
        for b in bufs:
            dev.free(b)


def kernel_tps(dev, src, ref, ctrl, params, bins, want, interp=0):
    n = ctrl.shape[0]
    bufs = [dev.upload(src), dev.upload(ref), dev.upload(params)] + ([dev.upload(ctrl)] if n else [])
    try:
        rs = bins / (want.rr[1] - want.rr[0]) if want.rr[1] > want.rr[0] else 0.0
        ss = bins / (want.sr[1] - want.sr[0]) if want.sr[1] > want.sr[0] else 0.0
        return dev.similarity_tps(bufs[0], src.shape[::-1], bufs[1], ref.shape[::-1], bufs[3] if n else None, bufs[2], n, interp,
                                  bins, want.rr[0], rs, want.sr[0], ss, want.c[0], want.c[1])
    finally:
        for b in bufs:
            dev.free(b)


# ---- the cases both suites run (L: the library behind the C API, dev: its flat device entry points) --------------------------
def case_affine_linear(dev, shape, bins):
    """the joint histogram equals numpy's exactly and the seven sums are within the bound of any summation order"""
    ref, src = volumes(shape)
    w = want_affine(shape, A_FIXED, bins)
    rd = SHAPES[shape][0]
    assert int(w.inside.sum()) == SHAPES[shape][2]
    assert 2 < SHAPES[shape][2] - w.n <= 2 + 2 * 8                      # the NaN and inf voxels: two of ref, up to 8 samples each of src
    assert w.ok[rd[2] // 2, rd[1] // 2, rd[0] // 2] and w.hist[bins - 1].sum() >= 1   # the voxel on ref_hi is in bin B - 1
    hist, sums = kernel_affine(dev, src, ref, A_FIXED, bins, w)
    assert int(hist.sum()) == w.n
    assert np.array_equal(hist, w.hist)
    check_sums(sums, w, f"{shape} bins {bins}")


def case_aggregated(dev, shape, bins):
    """the wave-aggregated form of the histogram update counts the same: on the case above, and on a reference that is one
    background value but for a few voxels (every lane of most waves on one counter)"""
    dev.L.s3d_k_similarity_set_aggregate(1)
    try:
        case_affine_linear(dev, shape, bins)
        ref, src = volumes(shape)
        rd, sd, _ = SHAPES[shape]
        flat = np.zeros_like(ref)
        flat[::2, ::5, ::7] = ref[::2, ::5, ::7]
        t = affine_coords(A_IDENTITY, rd)
        inside = inside_mask(t, rd)
        w = Want(flat, trilinear(flat, t, inside), inside, bins, src=flat)
        hist, sums = kernel_affine(dev, flat, flat, A_IDENTITY, bins, w)
        assert np.array_equal(hist, w.hist) and w.hist.max() > w.n // 2
        check_sums(sums, w)
    finally:
        dev.L.s3d_k_similarity_set_aggregate(-1)


def case_api(L, shape, bins):
    """the public entry point on the same case: default ranges found on the device, the statistics to their bounds"""
    ref, src = volumes(shape)
    t = make_affine(L, A_FIXED)
    try:
        check_against(similarity(L, t, src, ref, make_opts(bins), bins), want_affine(shape, A_FIXED, bins), shape)
    finally:
        L.imutil.cleanup_tform(C.byref(t))


def case_counts(L):
    """how many voxels the transforms keep, against the counts fixed when the cases were chosen: a kernel that drops or invents
    voxels cannot pass by agreeing with itself"""
    for shape, (rd, sd, kept) in SHAPES.items():
        ref, src = volumes(shape, clean=True)
        assert int(inside_mask(affine_coords(A_FIXED, rd), sd).sum()) == kept
        t = make_affine(L, A_FIXED)
        g = similarity(L, t, src, ref, make_opts(2), 2)
        L.imutil.cleanup_tform(C.byref(t))
        assert g.rc == 0 and (g.n, g.n_total) == (kept, rd[0] * rd[1] * rd[2]) and int(g.hist.sum()) == kept
    ref, src = volumes("70x33x9", clean=True)
    for A, kept in ((A_SHIFT, KEPT_SHIFT), (A_FAR, 0)):
        t = make_affine(L, A)
        g = similarity(L, t, src, ref, make_opts(2), 2)
        L.imutil.cleanup_tform(C.byref(t))
        assert g.rc == 0 and (g.n, g.n_total) == (kept, 20790) and int(g.hist.sum()) == kept
        if kept == 0:                                                   # no overlap is a success with NaN statistics
            assert all(math.isnan(v) for v in g.stats.values()) and not g.hist.any()
        else:
            check_against(g, want_affine("70x33x9", A, 2, clean=True))


def case_identity(L):
    """T == NULL with src == ref"""
    ref, _ = volumes("70x33x9", clean=True)
    g = similarity(L, None, ref, ref, None, 64)
    assert g.rc == 0 and g.n == g.n_total == ref.size
    assert g.stats["mse"] == 0.0 and g.stats["mae"] == 0.0 and abs(g.stats["ncc"] - 1.0) <= 1e-12
    assert abs(g.stats["mi"] - g.stats["h_ref"]) <= 1e-10 and abs(g.stats["mi"] - g.stats["h_src"]) <= 1e-10
    assert g.stats["h_ref"] > 1.0                                       # the volume spreads over many bins
    assert not (g.hist - np.diag(np.diag(g.hist))).any()                # a == b: only the diagonal
    check_against(g, Want(ref, ref, np.ones(ref.shape, bool), 64, src=ref))


def case_degenerate(L):
    """a 1 x 1 x 1 pair; a constant volume: an empty range, everything in bin 0, NaN ncc"""
    one = np.full((1, 1, 1), 2.5, np.float32)
    g = similarity(L, None, one, one, make_opts(2), 2)
    assert g.rc == 0 and (g.n, g.n_total) == (1, 1) and g.hist[0, 0] == 1 and g.hist.sum() == 1
    assert g.stats["mse"] == 0.0 and g.stats["mean_ref"] == 2.5 and math.isnan(g.stats["ncc"]) and math.isnan(g.stats["nmi"])
    ref, src = volumes("70x33x9", clean=True)
    const = np.full(ref.shape, -1.5, np.float32)
    t = make_affine(L, A_FIXED)
    g = similarity(L, t, src, const, make_opts(37), 37)
    L.imutil.cleanup_tform(C.byref(t))
    assert g.rc == 0 and g.n == SHAPES["70x33x9"][2] and g.hist[0].sum() == g.n and not g.hist[1:].any()
    assert g.stats["var_ref"] == 0.0 and g.stats["mean_ref"] == -1.5 and math.isnan(g.stats["ncc"]) and g.stats["h_ref"] == 0.0
    assert abs(g.stats["mi"]) <= 1e-10 and g.stats["var_src"] > 0


CONSISTENCY_RDIMS = (40, 21, 7)


def _consistency(L, dev, tform, src, interp, run_kernel, bins=37):
    """the histogram and the sums of the numpy restatement fed by the library's own im_inv_transform output; the overlap is the
    non-zero voxels of the same warp of an all-ones source"""
    ref = _blobby(CONSISTENCY_RDIMS, 13)
    b = warp(L, tform, src, CONSISTENCY_RDIMS, interp)
    mask = warp(L, tform, np.ones_like(src), CONSISTENCY_RDIMS, interp) != 0
    w = Want(ref, b, mask, bins, src=src)
    assert 0 < w.n < ref.size                                            # part of the reference falls outside the source
    g = similarity(L, tform, src, ref, make_opts(bins, interp), bins)
    check_against(g, w)
    hist, sums = run_kernel(ref, w)
    assert np.array_equal(hist, w.hist)
    check_sums(sums, w)


def case_consistency_tps(L, dev, n):
    from tests import tps_cases as tc
    tc.bind(L)
    src, ctrl, params = tc.warp_inputs(n, 1, CONSISTENCY_RDIMS)
    t = tc.make_tps(L, ctrl, params)
    try:
        _consistency(L, dev, t, src, 0, lambda ref, w: kernel_tps(dev, src, ref, ctrl, params, w.bins, w))
    finally:
        L.imutil.cleanup_tform(C.byref(t))


def case_consistency_lanczos(L, dev):
    _, src = volumes("70x33x9", clean=True)
    t = make_affine(L, A_FIXED)
    try:
        _consistency(L, dev, t, src, 1, lambda ref, w: kernel_affine(dev, src, ref, A_FIXED, w.bins, w, 1))
    finally:
        L.imutil.cleanup_tform(C.byref(t))


def case_meaning(L):
    """the reference is the source warped by A_FIXED: under that map the images agree more than under the identity"""
    ref, src = meaning_volumes()
    t = make_affine(L, A_FIXED)
    good, bad = similarity(L, t, src, ref, None, 64), similarity(L, None, src, ref, None, 64)
    L.imutil.cleanup_tform(C.byref(t))
    assert good.rc == 0 and bad.rc == 0
    print({f: (good.stats[f], bad.stats[f]) for f in ("ncc", "mi", "mse")})
    assert good.stats["ncc"] > bad.stats["ncc"] and good.stats["mi"] > bad.stats["mi"] and good.stats["mse"] < bad.stats["mse"]
    assert good.stats["mse"] == 0.0 and abs(good.stats["ncc"] - 1.0) <= 1e-12   # the warp restated bit for bit


def case_refusals(L):
    """each failure returns SIFT3D_FAILURE with a message and leaves out and joint untouched"""
    u = L.imutil
    ref, src = volumes("70x33x9", clean=True)
    ims = {"src": L.image_from_numpy(src, (1, 1, 1)), "ref": L.image_from_numpy(ref, (1, 1, 1)),
           "nc2": L.image_from_numpy(np.zeros((4, 5, 6, 2), np.float32), (1, 1, 1))}
    null = abi.Image()
    u.init_im(C.byref(null))
    null.nx, null.ny, null.nz, null.nc = 6, 5, 4, 1
    u.im_default_stride(C.byref(null))
    good = make_affine(L, A_FIXED)
    odd = make_affine(L, A_FIXED)
    odd.tform.type = 5                                                  # neither AFFINE nor TPS
    flat = abi.Affine()
    u.init_Affine.argtypes = [P(abi.Affine), C.c_int]
    assert u.init_Affine(C.byref(flat), 2) == 0                         # a 2-D affine
    nan = math.nan
    cases = [("bins 1", good, "src", "ref", make_opts(1)), ("bins 129", good, "src", "ref", make_opts(129)),
             ("bins -4", good, "src", "ref", make_opts(-4)), ("unknown transform type", odd, "src", "ref", make_opts()),
             ("2-D affine", flat, "src", "ref", make_opts()), ("nc 2 source", good, "nc2", "ref", make_opts()),
             ("nc 2 reference", good, "src", "nc2", make_opts()), ("NULL data", good, "src", "null", make_opts()),
             ("unknown interp", good, "src", "ref", make_opts(0, 2)),
             ("NaN reference range", good, "src", "ref", make_opts(0, 0, (nan, 1.0))),
             ("NaN source range", good, "src", "ref", make_opts(0, 0, (0.0, 0.0), (0.0, nan)))]
    ims["null"] = null
    try:
        for label, t, s, r, opts in cases:
            out, joint = abi.Similarity(), np.full(129 * 129, 0xDEADBEEF, np.uint64)
            C.memset(C.byref(out), 0xAB, C.sizeof(out))
            before = bytes(out)
            rc = u.sift3d_amd_im_similarity(C.addressof(t), C.byref(ims[s]), C.byref(ims[r]), C.byref(opts), C.byref(out),
                                            joint.ctypes.data)
            assert rc == -1, label
            assert b"sift3d_amd_im_similarity" in u.sift3d_amd_last_error(), label
            assert bytes(out) == before and (joint == 0xDEADBEEF).all(), label
    finally:
        odd.tform.type = 0
        for t in (good, odd, flat):
            u.cleanup_tform(C.byref(t))
        for k in ("src", "ref", "nc2"):
            L.free_image(ims[k])
