"""ctypes mirror of the SIFT3D C ABI (x86-64 SysV) that this repo's drop-in library exports.

The struct layouts below are the ones declared in ``include/sift3d_abi.h`` (which is layout
compatible with the reference's ``imutil/imtypes.h:136-334`` -- sizes/offsets are asserted both
in the header and in ``tests/test_abi.py``).  Because the layouts are identical, the very same
bindings can drive

* ``sift3d_amd/lib/libsift3d_amd.so``   -- the MI355X/HIP implementation (the product), and
* ``oracle/_ref/libsift3D.so``          -- the unmodified reference compiled as an oracle
                                           (tests / cpu_baseline only),

which is what lets the parity tests read like the reference's own usage
(``examples/featuresC.c:26-102``): init_SIFT3D -> SIFT3D_detect_keypoints ->
SIFT3D_extract_descriptors.

Nothing in here computes anything; it is plumbing.
"""
from __future__ import annotations

import ctypes as C
import numpy as np

IM_NDIMS = 3
ICOS_NFACES = 20
ICOS_NVERT = 12
NHIST_PER_DIM = 4
HIST_NUMEL = ICOS_NVERT
DESC_NUM_TOTAL_HIST = NHIST_PER_DIM ** 3
DESC_NUMEL = DESC_NUM_TOTAL_HIST * HIST_NUMEL

SIFT3D_SUCCESS = 0
SIFT3D_FAILURE = -1


class Mat_rm(C.Structure):
    _fields_ = [("data", C.c_void_p), ("size", C.c_size_t), ("num_cols", C.c_int),
                ("num_rows", C.c_int), ("static_mem", C.c_int), ("type", C.c_int)]


class Image(C.Structure):
    _fields_ = [("data", C.POINTER(C.c_float)), ("cl_image", C.c_int), ("s", C.c_double),
                ("size", C.c_size_t), ("nx", C.c_int), ("ny", C.c_int), ("nz", C.c_int),
                ("ux", C.c_double), ("uy", C.c_double), ("uz", C.c_double),
                ("xs", C.c_size_t), ("ys", C.c_size_t), ("zs", C.c_size_t),
                ("nc", C.c_int), ("cl_valid", C.c_int)]


class Sep_FIR_filter(C.Structure):
    _fields_ = [("cl_apply_unrolled", C.c_int), ("kernel", C.POINTER(C.c_float)),
                ("dim", C.c_int), ("width", C.c_int), ("symmetric", C.c_int)]


class Gauss_filter(C.Structure):
    _fields_ = [("sigma", C.c_double), ("f", Sep_FIR_filter)]


class GSS_filters(C.Structure):
    _fields_ = [("first_gauss", Gauss_filter), ("gauss_octave", C.POINTER(Gauss_filter)),
                ("num_filters", C.c_int), ("first_level", C.c_int)]


class SIFT_cl_kernels(C.Structure):
    _fields_ = [("downsample_2", C.c_int)]


class Pyramid(C.Structure):
    _fields_ = [("levels", C.POINTER(Image)), ("sigma_n", C.c_double), ("sigma0", C.c_double),
                ("num_kp_levels", C.c_int), ("first_octave", C.c_int), ("num_octaves", C.c_int),
                ("first_level", C.c_int), ("num_levels", C.c_int)]


class Cvec(C.Structure):
    _fields_ = [("x", C.c_float), ("y", C.c_float), ("z", C.c_float)]


class Slab(C.Structure):
    _fields_ = [("buf", C.c_void_p), ("num", C.c_size_t), ("buf_size", C.c_size_t)]


class Keypoint(C.Structure):
    _fields_ = [("r_data", C.c_float * 9), ("R", Mat_rm), ("xd", C.c_double), ("yd", C.c_double),
                ("zd", C.c_double), ("sd", C.c_double), ("o", C.c_int), ("s", C.c_int)]


class Keypoint_store(C.Structure):
    _fields_ = [("buf", C.POINTER(Keypoint)), ("slab", Slab), ("nx", C.c_int), ("ny", C.c_int),
                ("nz", C.c_int)]


class Hist(C.Structure):
    _fields_ = [("bins", C.c_float * HIST_NUMEL)]


class SIFT3D_Descriptor(C.Structure):
    _fields_ = [("hists", Hist * DESC_NUM_TOTAL_HIST), ("xd", C.c_double), ("yd", C.c_double),
                ("zd", C.c_double), ("sd", C.c_double)]


class SIFT3D_Descriptor_store(C.Structure):
    _fields_ = [("buf", C.POINTER(SIFT3D_Descriptor)), ("num", C.c_size_t), ("nx", C.c_int),
                ("ny", C.c_int), ("nz", C.c_int)]


class Tri(C.Structure):
    _fields_ = [("v", Cvec * 3), ("idx", C.c_int * 3)]


class Mesh(C.Structure):
    _fields_ = [("tri", C.POINTER(Tri)), ("num", C.c_int)]


class SIFT3D(C.Structure):
    _fields_ = [("mesh", Mesh), ("gss", GSS_filters), ("kernels", SIFT_cl_kernels),
                ("gpyr", Pyramid), ("dog", Pyramid), ("im", Image), ("peak_thresh", C.c_double),
                ("corner_thresh", C.c_double), ("dense_rotate", C.c_int)]


class Ransac(C.Structure):
    _fields_ = [("err_thresh", C.c_double), ("num_iter", C.c_int)]


class Tform(C.Structure):
    _fields_ = [("type", C.c_int), ("vtable", C.c_void_p)]


class Affine(C.Structure):
    _fields_ = [("tform", Tform), ("A", Mat_rm)]


class Tps(C.Structure):
    """Thin-plate spline: ``params`` dim x (N + dim + 1), ``kp_src`` N x dim (imtypes.h:380-385)."""
    _fields_ = [("tform", Tform), ("params", Mat_rm), ("kp_src", Mat_rm), ("dim", C.c_int)]


class TpsOpts(C.Structure):
    """``sift3d_amd_tps_opts``; a field <= 0 (lambda < 0) takes its default."""
    _fields_ = [("lambda_", C.c_double), ("ctrl_thresh", C.c_double), ("max_points", C.c_int)]


class Similarity(C.Structure):
    """``sift3d_amd_similarity``: the scores of a source under a transform against a reference, over their overlap."""
    _fields_ = [("n", C.c_longlong), ("n_total", C.c_longlong)] + \
               [(f, C.c_double) for f in ("mean_ref", "mean_src", "var_ref", "var_src", "mse", "mae", "ncc", "h_ref", "h_src",
                                          "h_joint", "mi", "nmi")]


class SimilarityOpts(C.Structure):
    """``sift3d_amd_similarity_opts``; bins 0: 64, interp 0 tri-linear / 1 Lanczos-2, a range is used when [1] > [0]."""
    _fields_ = [("bins", C.c_int), ("interp", C.c_int), ("ref_range", C.c_double * 2), ("src_range", C.c_double * 2)]


class RefineOpts(C.Structure):
    """``sift3d_amd_refine_opts``; a zero field takes its default (levels 3, max_iter 30, tol 1e-3, min_overlap 0.5)."""
    _fields_ = [("levels", C.c_int), ("max_iter", C.c_int), ("tol", C.c_double), ("min_overlap", C.c_double),
                ("normalize", C.c_int)]


class RefineInfo(C.Structure):
    """``sift3d_amd_refine_info``: how sift3d_amd_refine_affine ended; costs and counts are level 0's."""
    _fields_ = [("status", C.c_int), ("levels_run", C.c_int), ("iters", C.c_int), ("passes", C.c_int),
                ("n_before", C.c_longlong), ("n_after", C.c_longlong), ("cost_before", C.c_double),
                ("cost_after", C.c_double), ("max_corner_shift", C.c_double)]


REFINE_CONVERGED, REFINE_MAX_ITER, REFINE_STALLED, REFINE_UNCHANGED = 0, 1, 2, 3


class DemonsOpts(C.Structure):
    """``sift3d_amd_demons_opts``; a zero field takes its default (levels 3, max_iter 50, sigma 1.5, max_step 1, tol 1e-3,
    min_overlap 0.5)."""
    _fields_ = [("levels", C.c_int), ("max_iter", C.c_int), ("sigma", C.c_double), ("max_step", C.c_double), ("tol", C.c_double),
                ("min_overlap", C.c_double), ("normalize", C.c_int)]


class DemonsInfo(C.Structure):
    """``sift3d_amd_demons_info``: how sift3d_amd_register_demons ended; costs and counts are level 0's, the displacements
    those of the returned field."""
    _fields_ = [("status", C.c_int), ("levels_run", C.c_int), ("iters", C.c_int), ("passes", C.c_int),
                ("n_before", C.c_longlong), ("n_after", C.c_longlong), ("cost_before", C.c_double),
                ("cost_after", C.c_double), ("mean_disp", C.c_double), ("max_disp", C.c_double)]


DEMONS_CONVERGED, DEMONS_MAX_ITER, DEMONS_UNCHANGED = 0, 1, 3


class FieldInverseOpts(C.Structure):
    """``sift3d_amd_field_inverse_opts``; a zero field takes its default (max_iter 30, tol 1e-3 source voxel)."""
    _fields_ = [("max_iter", C.c_int), ("tol", C.c_double)]


class FieldInverseInfo(C.Structure):
    """``sift3d_amd_field_inverse_info``: the source voxels by how their iteration ended, the updates made, and the residual
    |phi(psi(y)) - y| in source voxels over the voxels that are not invalid."""
    _fields_ = [("n", C.c_longlong), ("n_converged", C.c_longlong), ("n_outside", C.c_longlong),
                ("n_not_converged", C.c_longlong), ("n_invalid", C.c_longlong), ("updates", C.c_longlong),
                ("mean_residual", C.c_double), ("max_residual", C.c_double)]


class FieldJacobianInfo(C.Structure):
    """``sift3d_amd_field_jacobian_info``: the determinant of the map's Jacobian over the reference voxels; n_folded counts the
    finite ones <= 0."""
    _fields_ = [("n", C.c_longlong), ("n_finite", C.c_longlong), ("n_folded", C.c_longlong), ("min_det", C.c_double),
                ("max_det", C.c_double), ("mean_det", C.c_double)]


# s3d_k_field_invert's status byte per source voxel
FIELD_INV_CONVERGED, FIELD_INV_OUTSIDE, FIELD_INV_NOT_CONVERGED, FIELD_INV_INVALID = 0, 1, 2, 3


class Reg_SIFT3D(C.Structure):
    _fields_ = [("src_units", C.c_double * 3), ("ref_units", C.c_double * 3), ("sift3d", SIFT3D), ("ran", Ransac),
                ("desc_src", SIFT3D_Descriptor_store), ("desc_ref", SIFT3D_Descriptor_store), ("match_src", Mat_rm),
                ("match_ref", Mat_rm), ("nn_thresh", C.c_double), ("verbose", C.c_int)]


class Volume(C.Structure):
    """``sift3d_amd_volume``: a volume with its elements as stored (sift3d_amd_read_nii_native)."""
    _fields_ = [("data", C.c_void_p), ("dtype", C.c_int), ("nx", C.c_int), ("ny", C.c_int), ("nz", C.c_int),
                ("ux", C.c_double), ("uy", C.c_double), ("uz", C.c_double), ("slope", C.c_double),
                ("inter", C.c_double)]


# element types of the typed entry points: their NIfTI-1 datatype codes (include/sift3d_amd.h)
SIFT3D_AMD_U8, SIFT3D_AMD_I16, SIFT3D_AMD_F32, SIFT3D_AMD_I8, SIFT3D_AMD_U16 = 2, 4, 16, 256, 512
TYPED_DTYPES = {np.dtype(np.uint8): SIFT3D_AMD_U8, np.dtype(np.int8): SIFT3D_AMD_I8,
                np.dtype(np.uint16): SIFT3D_AMD_U16, np.dtype(np.int16): SIFT3D_AMD_I16,
                np.dtype(np.float32): SIFT3D_AMD_F32}


def detect_keypoints_typed(L: C.CDLL, sift3d, vol, kp, units=(1.0, 1.0, 1.0), slope: float = 1.0, inter: float = 0.0,
                           dtype=None, shape=None) -> int:
    """sift3d_amd_detect_keypoints_typed on ``vol``: a numpy array [nz, ny, nx] of uint8 / int8 / uint16 / int16 / float32
    (host form), or a device address -- e.g. ``torch.Tensor.data_ptr()`` -- with ``dtype`` (numpy dtype) and ``shape``
    (nz, ny, nx) given (device form).  ``L`` must have been through ``device.bind_extensions``.  Returns the C status."""
    if isinstance(vol, np.ndarray):
        if vol.dtype not in TYPED_DTYPES:
            raise TypeError(f"unsupported element type {vol.dtype}")
        vol = np.ascontiguousarray(vol)
        nz, ny, nx = vol.shape
        return L.sift3d_amd_detect_keypoints_typed(C.byref(sift3d), C.c_void_p(vol.ctypes.data), TYPED_DTYPES[vol.dtype], 0,
                                                   nx, ny, nz, units[0], units[1], units[2], slope, inter, C.byref(kp))
    if dtype is None or shape is None:
        raise TypeError("a device address needs dtype and shape")
    nz, ny, nx = shape
    return L.sift3d_amd_detect_keypoints_typed(C.byref(sift3d), C.c_void_p(int(vol)), TYPED_DTYPES[np.dtype(dtype)], 1,
                                               nx, ny, nz, units[0], units[1], units[2], slope, inter, C.byref(kp))


def set_mask(L: C.CDLL, sift3d, mask, shape=None) -> int:
    """sift3d_amd_set_mask: keypoints of the following detects on ``sift3d`` inside the region of interest only.  ``mask``: a
    numpy uint8 / bool array [nz, ny, nx] (host form; non-zero = inside), a device address -- e.g. a ``torch.uint8`` tensor's
    ``data_ptr()`` -- with ``shape`` (nz, ny, nx) given (device form; any address, 16-byte aligned ones are packed with wide
    loads, an offset view that is not with byte loads), or None to clear.  ``L`` must have been through
    ``device.bind_extensions``.  Returns the C status."""
    if mask is None:
        return L.sift3d_amd_set_mask(C.byref(sift3d), None, 0, 0, 0, 0)
    if isinstance(mask, np.ndarray):
        if mask.dtype not in (np.dtype(np.uint8), np.dtype(np.bool_)) or mask.ndim != 3:
            raise TypeError("a mask is a uint8 or bool array [nz, ny, nx]")
        mask = np.ascontiguousarray(mask)                 # (a bool array stores one byte per element, 0 or 1)
        nz, ny, nx = mask.shape
        return L.sift3d_amd_set_mask(C.byref(sift3d), C.c_void_p(mask.ctypes.data), 0, nx, ny, nz)
    if shape is None:
        raise TypeError("a device address needs shape")
    nz, ny, nx = shape
    return L.sift3d_amd_set_mask(C.byref(sift3d), C.c_void_p(int(mask)), 1, nx, ny, nz)


def set_max_keypoints(L: C.CDLL, sift3d, n: int) -> int:
    """sift3d_amd_set_max_keypoints: the following detects on ``sift3d`` return the ``n`` strongest keypoints only (strength:
    |DoG| of the keypoint's own voxel), in the reference's order; 0 = no budget.  Returns the C status (n < 0 fails and leaves
    the previous value)."""
    L.sift3d_amd_set_max_keypoints.argtypes = [C.POINTER(SIFT3D), C.c_long]
    L.sift3d_amd_set_max_keypoints.restype = C.c_int
    return L.sift3d_amd_set_max_keypoints(C.byref(sift3d), int(n))


def get_max_keypoints(L: C.CDLL, sift3d) -> int:
    L.sift3d_amd_get_max_keypoints.argtypes = [C.POINTER(SIFT3D)]
    L.sift3d_amd_get_max_keypoints.restype = C.c_long
    return int(L.sift3d_amd_get_max_keypoints(C.byref(sift3d)))


def keypoint_strengths(L: C.CDLL, sift3d, kp) -> np.ndarray:
    """sift3d_amd_keypoint_strengths: float32 [K], the strength of each record of ``kp`` from the pyramid ``sift3d`` holds on the
    device after a detect.  Raises RuntimeError with the library's message on failure (no pyramid, a record outside its level,
    an empty store, a pyramid spread over several GPUs)."""
    L.sift3d_amd_keypoint_strengths.argtypes = [C.POINTER(SIFT3D), C.POINTER(Keypoint_store), C.POINTER(C.c_float)]
    L.sift3d_amd_keypoint_strengths.restype = C.c_int
    L.sift3d_amd_last_error.restype = C.c_char_p
    out = np.zeros(int(kp.slab.num), np.float32)
    if L.sift3d_amd_keypoint_strengths(C.byref(sift3d), C.byref(kp), out.ctypes.data_as(C.POINTER(C.c_float))) != 0:
        raise RuntimeError((L.sift3d_amd_last_error() or b"").decode())
    return out


def set_subvoxel(L: C.CDLL, sift3d, on: bool) -> int:
    """sift3d_amd_set_subvoxel: the following detects on ``sift3d`` refine every keypoint's position within its voxel and its
    scale within its level by a quadratic fit to the DoG (same list, same order, same o, s and R); False restores integer
    keypoints.  Overrides SIFT3D_SUBVOXEL of the environment.  Returns the C status."""
    L.sift3d_amd_set_subvoxel.argtypes = [C.POINTER(SIFT3D), C.c_int]
    L.sift3d_amd_set_subvoxel.restype = C.c_int
    return L.sift3d_amd_set_subvoxel(C.byref(sift3d), 1 if on else 0)


def get_subvoxel(L: C.CDLL, sift3d) -> bool:
    L.sift3d_amd_get_subvoxel.argtypes = [C.POINTER(SIFT3D)]
    L.sift3d_amd_get_subvoxel.restype = C.c_int
    return bool(L.sift3d_amd_get_subvoxel(C.byref(sift3d)))


def last_subvoxel_counts(L: C.CDLL, sift3d) -> tuple:
    """sift3d_amd_last_subvoxel_counts: (keypoints that took the 3-D fit, keypoints that took the per-axis fallback) of the last
    detect on ``sift3d``; (0, 0) after an unrefined one."""
    L.sift3d_amd_last_subvoxel_counts.argtypes = [C.POINTER(SIFT3D), C.POINTER(C.c_long)]
    L.sift3d_amd_last_subvoxel_counts.restype = C.c_int
    out = (C.c_long * 2)()
    if L.sift3d_amd_last_subvoxel_counts(C.byref(sift3d), out) != 0:
        raise RuntimeError("sift3d_amd_last_subvoxel_counts failed")
    return int(out[0]), int(out[1])


def refined_keypoints_to_numpy(kp) -> tuple:
    """(xyz float64 [K, 3] in octave voxels, o int32 [K], s int32 [K], sd float64 [K], R float32 [K, 3, 3]) of a store whose
    positions may carry fractions (``Sift3dLib.keypoints_to_numpy`` is for integer records)."""
    k = int(kp.slab.num)
    xyz, o, s = np.zeros((k, 3), np.float64), np.zeros(k, np.int32), np.zeros(k, np.int32)
    sd, R = np.zeros(k, np.float64), np.zeros((k, 3, 3), np.float32)
    for i in range(k):
        key = kp.buf[i]
        xyz[i] = (key.xd, key.yd, key.zd)
        o[i], s[i], sd[i] = key.o, key.s, key.sd
        R[i] = np.array(key.r_data[:], dtype=np.float32).reshape(3, 3)
    return xyz, o, s, sd, R


def volume_to_numpy(v: Volume) -> np.ndarray:
    """A copy of a ``Volume``'s elements as [nz, ny, nx] in their stored type."""
    dt = {code: d for d, code in TYPED_DTYPES.items()}[v.dtype]
    n = v.nx * v.ny * v.nz
    buf = (C.c_char * (n * dt.itemsize)).from_address(v.data)
    return np.frombuffer(buf, dtype=dt).copy().reshape(v.nz, v.ny, v.nx)


# (struct, sizeof, {field: offset}) measured on the compiled reference.
ABI_LAYOUT = [
    (Image, 104, {"data": 0, "cl_image": 8, "s": 16, "size": 24, "nx": 32, "ux": 48, "xs": 72,
                  "nc": 96, "cl_valid": 100}),
    (Mat_rm, 32, {}),
    (Keypoint, 112, {"r_data": 0, "R": 40, "xd": 72, "sd": 96, "o": 104, "s": 108}),
    (Slab, 24, {}),
    (Keypoint_store, 48, {}),
    (Hist, 48, {}),
    (SIFT3D_Descriptor, 3104, {"xd": 3072}),
    (SIFT3D_Descriptor_store, 32, {}),
    (Sep_FIR_filter, 32, {}),
    (Gauss_filter, 40, {}),
    (GSS_filters, 56, {}),
    (Pyramid, 48, {}),
    (Tri, 48, {}),
    (Mesh, 16, {}),
    (Ransac, 16, {"num_iter": 8}),
    (Tform, 16, {"vtable": 8}),
    (Affine, 48, {"A": 16}),
    (Tps, 88, {"params": 16, "kp_src": 48, "dim": 80}),
    (Reg_SIFT3D, 512, {"ref_units": 24, "sift3d": 48, "ran": 352, "desc_src": 368, "desc_ref": 400, "match_src": 432,
                       "match_ref": 464, "nn_thresh": 496, "verbose": 504}),
    (SIFT3D, 304, {"gss": 16, "gpyr": 80, "dog": 128, "im": 176, "peak_thresh": 280,
                   "dense_rotate": 296}),
]


class Sift3dLib:
    """A loaded library that speaks the SIFT3D C API (product or reference oracle).

    ``imutil`` may be a second CDLL when the L1 functions live in a separate shared object (the
    reference splits libimutil / libsift3D; the product exports both layers from one library).
    """

    def __init__(self, sift: C.CDLL, imutil: C.CDLL | None = None, name: str = "?", reg: C.CDLL | None = None):
        self.sift = sift
        self.imutil = imutil if imutil is not None else sift
        self.reg = reg if reg is not None else sift          # registration layer (libreg in the reference)
        self.name = name
        s, u = self.sift, self.imutil
        P = C.POINTER
        u.init_im.argtypes = [P(Image)]
        u.init_im.restype = None
        u.im_free.argtypes = [P(Image)]
        u.im_free.restype = None
        u.im_resize.argtypes = [P(Image)]
        u.im_default_stride.argtypes = [P(Image)]
        u.im_default_stride.restype = None
        u.init_Gauss_filter.argtypes = [P(Gauss_filter), C.c_double, C.c_int]
        u.init_Gauss_incremental_filter.argtypes = [P(Gauss_filter), C.c_double, C.c_double, C.c_int]
        u.cleanup_Gauss_filter.argtypes = [P(Gauss_filter)]
        u.cleanup_Gauss_filter.restype = None
        u.apply_Sep_FIR_filter.argtypes = [P(Image), P(Image), P(Sep_FIR_filter), C.c_double]
        s.init_SIFT3D.argtypes = [P(SIFT3D)]
        s.cleanup_SIFT3D.argtypes = [P(SIFT3D)]
        s.cleanup_SIFT3D.restype = None
        for f in ("set_peak_thresh_SIFT3D", "set_corner_thresh_SIFT3D", "set_sigma_n_SIFT3D",
                  "set_sigma0_SIFT3D"):
            getattr(s, f).argtypes = [P(SIFT3D), C.c_double]
        s.set_num_kp_levels_SIFT3D.argtypes = [P(SIFT3D), C.c_uint]
        s.init_Keypoint_store.argtypes = [P(Keypoint_store)]
        s.init_Keypoint_store.restype = None
        s.cleanup_Keypoint_store.argtypes = [P(Keypoint_store)]
        s.cleanup_Keypoint_store.restype = None
        s.resize_Keypoint_store.argtypes = [P(Keypoint_store), C.c_size_t]
        s.init_SIFT3D_Descriptor_store.argtypes = [P(SIFT3D_Descriptor_store)]
        s.init_SIFT3D_Descriptor_store.restype = None
        s.cleanup_SIFT3D_Descriptor_store.argtypes = [P(SIFT3D_Descriptor_store)]
        s.cleanup_SIFT3D_Descriptor_store.restype = None
        s.SIFT3D_detect_keypoints.argtypes = [P(SIFT3D), P(Image), P(Keypoint_store)]
        s.SIFT3D_extract_descriptors.argtypes = [P(SIFT3D), P(Keypoint_store),
                                                 P(SIFT3D_Descriptor_store)]
        s.SIFT3D_extract_raw_descriptors.argtypes = [P(SIFT3D), P(Image), P(Keypoint_store),
                                                     P(SIFT3D_Descriptor_store)]
        s.SIFT3D_extract_dense_descriptors.argtypes = [P(SIFT3D), P(Image), P(Image)]
        s.SIFT3D_assign_orientations.argtypes = [P(SIFT3D), P(Image), P(Keypoint_store),
                                                 P(P(C.c_double))]
        s.SIFT3D_have_gpyr.argtypes = [P(SIFT3D)]

    # -- helpers that only marshal data ------------------------------------------------------
    def image_from_numpy(self, vol: np.ndarray, units=(1.0, 1.0, 1.0)) -> Image:
        """Make an ``Image`` owning a malloc'd copy of ``vol`` (shape [nz, ny, nx] or
        [nz, ny, nx, nc], float32; x fastest like ``im_default_stride``, imutil.c:1453)."""
        vol = np.ascontiguousarray(vol, dtype=np.float32)
        if vol.ndim == 3:
            vol = vol[..., None]
        nz, ny, nx, nc = vol.shape
        im = Image()
        self.imutil.init_im(C.byref(im))
        im.nx, im.ny, im.nz, im.nc = nx, ny, nz, nc
        im.ux, im.uy, im.uz = units
        self.imutil.im_default_stride(C.byref(im))
        if self.imutil.im_resize(C.byref(im)) != 0:
            raise RuntimeError("im_resize failed")
        C.memmove(im.data, vol.ctypes.data, vol.nbytes)
        return im

    def image_to_numpy(self, im: Image) -> np.ndarray:
        n = im.nx * im.ny * im.nz * im.nc
        a = np.ctypeslib.as_array(im.data, shape=(n,)).copy()
        a = a.reshape(im.nz, im.ny, im.nx, im.nc)
        return a[..., 0] if im.nc == 1 else a

    def free_image(self, im: Image) -> None:
        self.imutil.im_free(C.byref(im))
        im.data = None

    @staticmethod
    def descriptor_store_from_numpy(bins: np.ndarray, xyzs: np.ndarray | None = None):
        """A SIFT3D_Descriptor_store over a numpy-owned buffer (returned too: keep it alive)."""
        k = bins.shape[0]
        raw = np.zeros((k, C.sizeof(SIFT3D_Descriptor)), np.uint8)
        if k:
            raw[:, :DESC_NUMEL * 4] = np.ascontiguousarray(bins, np.float32).view(np.uint8).reshape(k, -1)
        if xyzs is not None and k:
            raw[:, DESC_NUMEL * 4:] = np.ascontiguousarray(xyzs, np.float64).view(np.uint8).reshape(k, -1)
        st = SIFT3D_Descriptor_store()
        st.buf = C.cast(raw.ctypes.data, C.POINTER(SIFT3D_Descriptor))
        st.num = k
        return st, raw

    @staticmethod
    def keypoints_to_numpy(kp: Keypoint_store):
        """Return (coords int64 [K,5] = x,y,z,o,s ; sd float64 [K] ; R float32 [K,3,3])."""
        k = int(kp.slab.num)
        xyzos = np.zeros((k, 5), dtype=np.int64)
        xyz_d = np.zeros((k, 3), dtype=np.float64)
        sd = np.zeros(k, dtype=np.float64)
        R = np.zeros((k, 3, 3), dtype=np.float32)
        for i in range(k):
            key = kp.buf[i]
            xyz_d[i] = (key.xd, key.yd, key.zd)
            xyzos[i] = (int(key.xd), int(key.yd), int(key.zd), key.o, key.s)
            sd[i] = key.sd
            R[i] = np.array(key.r_data[:], dtype=np.float32).reshape(3, 3)
        assert np.all(xyz_d == xyzos[:, :3]), "keypoint coordinates are integers stored as double"
        return xyzos, sd, R

    @staticmethod
    def descriptors_to_numpy(desc: SIFT3D_Descriptor_store):
        """Return (bins float32 [K,768] in memory order 12*(cx+4cy+16cz)+v ; xyzs float64 [K,4])."""
        k = int(desc.num)
        raw = np.ctypeslib.as_array(C.cast(desc.buf, C.POINTER(C.c_uint8)),
                                    shape=(k, C.sizeof(SIFT3D_Descriptor))).copy()
        bins = raw[:, :DESC_NUMEL * 4].copy().view(np.float32).reshape(k, DESC_NUMEL)
        xyzs = raw[:, DESC_NUMEL * 4:].copy().view(np.float64).reshape(k, 4)
        return bins, xyzs
