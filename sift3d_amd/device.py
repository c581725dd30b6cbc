"""ctypes bindings of the flat device C-ABI (include/s3d_device.h) and of the sift3d_amd_* extension
entry points (include/sift3d_amd.h).  Plumbing only: pointers are plain integers (device addresses,
e.g. ``torch.Tensor.data_ptr()``) or numpy buffers for host data."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import abi

_vp = C.c_void_p
_f32p = C.POINTER(C.c_float)


def bind_extensions(L: C.CDLL) -> None:
    P = C.POINTER
    L.sift3d_amd_detect_keypoints_dev.argtypes = [P(abi.SIFT3D), _vp, C.c_int, C.c_int, C.c_int, C.c_double,
                                                  C.c_double, C.c_double, P(abi.Keypoint_store)]
    L.sift3d_amd_extract_descriptors_dev.argtypes = [P(abi.SIFT3D), P(abi.Keypoint_store), P(_vp)]
    L.sift3d_amd_extract_dense_dev.argtypes = [P(abi.SIFT3D), _vp, C.c_int, C.c_int, C.c_int, C.c_double,
                                               C.c_double, C.c_double, P(C.c_double), _vp]
    L.sift3d_amd_gauss_dev.argtypes = [_vp, _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, P(C.c_double), _f32p,
                                       C.c_int, C.c_double]
    L.sift3d_amd_download_pyramid.argtypes = [P(abi.SIFT3D), C.c_int]
    L.sift3d_amd_last_num_candidates.argtypes = [P(abi.SIFT3D)]
    L.sift3d_amd_last_num_candidates.restype = C.c_long
    L.sift3d_amd_set_stream.argtypes = [P(abi.SIFT3D), _vp]
    L.sift3d_amd_nn_match_dev.argtypes = [_vp, C.c_size_t, C.c_long, _vp, C.c_size_t, C.c_long, C.c_float,
                                          P(C.c_int), _vp]
    L.sift3d_amd_last_error.restype = C.c_char_p
    L.sift3d_amd_detect_keypoints_typed.argtypes = [P(abi.SIFT3D), _vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                                    C.c_double, C.c_double, C.c_double, C.c_double, C.c_double,
                                                    P(abi.Keypoint_store)]
    L.sift3d_amd_read_nii_native.argtypes = [C.c_char_p, P(abi.Volume)]
    L.sift3d_amd_free_volume.argtypes = [P(abi.Volume)]
    L.sift3d_amd_free_volume.restype = None
    # (an older build of the library, loaded through SIFT3D_AMD_LIB for an A/B run, has no masks: nothing is bound for it, and
    # a caller that asks for one fails on the missing symbol)
    if hasattr(L, "sift3d_amd_set_mask"):
        L.sift3d_amd_set_mask.argtypes = [P(abi.SIFT3D), _vp, C.c_int, C.c_int, C.c_int, C.c_int]
        L.sift3d_amd_have_mask.argtypes = [P(abi.SIFT3D)]
    if hasattr(L, "sift3d_amd_set_ransac_device"):        # (absent from builds older than the device-scored RANSAC)
        L.sift3d_amd_set_ransac_device.argtypes = [C.c_int]
        L.sift3d_amd_get_ransac_device.argtypes = []
        L.sift3d_amd_ransac_last_path.argtypes = []
        L.sift3d_amd_set_ransac_profile.argtypes = [C.c_int]
        L.sift3d_amd_set_ransac_profile.restype = None
        L.sift3d_amd_ransac_last_device_ms.argtypes = []
        L.sift3d_amd_ransac_last_device_ms.restype = C.c_double
    if hasattr(L, "sift3d_amd_set_subvoxel"):             # (absent from builds older than the sub-voxel refinement)
        L.sift3d_amd_set_subvoxel.argtypes = [P(abi.SIFT3D), C.c_int]
        L.sift3d_amd_get_subvoxel.argtypes = [P(abi.SIFT3D)]
        L.sift3d_amd_last_subvoxel_counts.argtypes = [P(abi.SIFT3D), P(C.c_long)]
    if hasattr(L, "sift3d_amd_fit_tps"):                  # (absent from builds older than the thin-plate spline)
        L.init_Tps.argtypes = [P(abi.Tps), C.c_int, C.c_int]
        L.resize_Tps.argtypes = [P(abi.Tps), C.c_int, C.c_int]
        L.sift3d_amd_fit_tps.argtypes = [P(abi.Mat_rm), P(abi.Mat_rm), C.c_double, P(abi.Tps)]
        L.sift3d_amd_register_tps.argtypes = [P(abi.Reg_SIFT3D), P(abi.TpsOpts), P(abi.Affine), P(abi.Tps)]
    if hasattr(L, "sift3d_amd_im_similarity"):            # (absent from builds older than the similarity scores)
        L.sift3d_amd_im_similarity.argtypes = [_vp, P(abi.Image), P(abi.Image), P(abi.SimilarityOpts), P(abi.Similarity), _vp]
        L.sift3d_amd_similarity_dev.argtypes = [_vp, _vp, C.c_int, C.c_int, C.c_int, _vp, C.c_int, C.c_int, C.c_int,
                                                P(abi.SimilarityOpts), P(abi.Similarity), _vp, _vp]
    if hasattr(L, "sift3d_amd_refine_affine"):            # (absent from builds older than the intensity-based refinement)
        L.sift3d_amd_refine_affine.argtypes = [P(abi.Image), P(abi.Image), P(abi.RefineOpts), P(abi.Affine), P(abi.RefineInfo)]
        L.sift3d_amd_refine_affine_dev.argtypes = [_vp, C.c_int, C.c_int, C.c_int, _vp, C.c_int, C.c_int, C.c_int,
                                                   P(abi.RefineOpts), P(abi.Affine), P(abi.RefineInfo), _vp]
    if hasattr(L, "sift3d_amd_register_demons"):          # (absent from builds older than the deformable registration)
        L.sift3d_amd_register_demons.argtypes = [P(abi.Image), P(abi.Image), _vp, P(abi.DemonsOpts), P(abi.Image),
                                                 P(abi.DemonsInfo)]
        L.sift3d_amd_register_demons_dev.argtypes = [_vp, C.c_int, C.c_int, C.c_int, _vp, C.c_int, C.c_int, C.c_int, _vp,
                                                     P(abi.DemonsOpts), _vp, P(abi.DemonsInfo), _vp]
        L.sift3d_amd_im_warp_field.argtypes = [_vp, P(abi.Image), P(abi.Image), C.c_int, P(abi.Image)]
    if hasattr(L, "sift3d_amd_invert_field"):             # (absent from builds older than the field inversion)
        L.sift3d_amd_invert_field.argtypes = [_vp, P(abi.Image), C.c_int, C.c_int, C.c_int, P(C.c_double), P(abi.FieldInverseOpts),
                                              P(abi.Affine), P(abi.Image), P(abi.FieldInverseInfo)]
        L.sift3d_amd_invert_field_dev.argtypes = [_vp, C.c_int, C.c_int, C.c_int, _vp, _vp, C.c_int, C.c_int, C.c_int,
                                                  P(abi.FieldInverseOpts), P(C.c_double), P(abi.FieldInverseInfo), _vp]
        L.sift3d_amd_field_jacobian.argtypes = [_vp, P(abi.Image), P(abi.Image), P(abi.FieldJacobianInfo)]
        L.sift3d_amd_field_jacobian_dev.argtypes = [_vp, C.c_int, C.c_int, C.c_int, _vp, _vp, P(abi.FieldJacobianInfo), _vp]
        L.sift3d_amd_field_apply_points.argtypes = [_vp, P(abi.Image), P(abi.Mat_rm), P(abi.Mat_rm)]


class DeviceLib:
    def __init__(self, L: C.CDLL):
        self.L = L
        L.s3d_rt_last_error.restype = C.c_char_p
        L.s3d_rt_device_count.argtypes = [C.POINTER(C.c_int)]
        L.s3d_rt_malloc.argtypes = [C.POINTER(_vp), C.c_size_t]
        L.s3d_rt_free.argtypes = [_vp]
        L.s3d_rt_mem_info.argtypes = [C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
        L.s3d_rt_h2d.argtypes = [_vp, _vp, C.c_size_t, _vp]
        L.s3d_rt_d2h.argtypes = [_vp, _vp, C.c_size_t, _vp]
        L.s3d_rt_d2d.argtypes = [_vp, _vp, C.c_size_t, _vp]
        L.s3d_rt_memset.argtypes = [_vp, C.c_int, C.c_size_t, _vp]
        L.s3d_rt_sync.argtypes = [_vp]
        L.s3d_rt_event_create.argtypes = [C.POINTER(_vp)]
        L.s3d_rt_event_destroy.argtypes = [_vp]
        L.s3d_rt_event_record.argtypes = [_vp, _vp]
        L.s3d_rt_event_elapsed_ms.argtypes = [_vp, _vp, C.POINTER(C.c_float)]
        L.s3d_k_absmax.argtypes = [_vp, C.c_size_t, _vp, _vp]
        L.s3d_k_scale_div.argtypes = [_vp, C.c_size_t, _vp, _vp]
        L.s3d_k_decimate2.argtypes = [_vp, C.c_int, C.c_int, C.c_int, _vp, _vp]
        L.s3d_k_subtract.argtypes = [_vp, _vp, _vp, C.c_size_t, _vp]
        L.s3d_k_conv_axis.argtypes = [_vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _f32p, C.c_int,
                                      C.c_float, _vp]
        L.s3d_k_sep_fir_path.argtypes = [_vp, _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, _f32p, _f32p, C.c_int,
                                         C.c_int, _vp]
        L.s3d_k_gauss_set_chunks.argtypes = [C.c_int, C.c_int]
        L.s3d_k_gauss_set_chunks.restype = None
        L.s3d_k_gauss_set_events.argtypes = [_vp, _vp, _vp]
        L.s3d_k_gauss_set_events.restype = None
        L.s3d_k_dogmax.argtypes = [_vp, _vp, C.c_size_t, _vp, _vp]
        # volumes of 8- / 16-bit integers as stored: (src, dtype code, ...)
        L.s3d_k_typed_elem_size.argtypes = [C.c_int]
        L.s3d_k_convert_f32.argtypes = [_vp, C.c_int, C.c_size_t, C.c_double, C.c_double, _vp, _vp]
        L.s3d_k_absmax_typed.argtypes = [_vp, C.c_int, C.c_size_t, C.c_double, C.c_double, _vp, _vp]
        L.s3d_k_sep_fir_div_typed_eligible.argtypes = [_vp, C.c_int, C.c_int, C.c_int, C.c_int, _f32p, C.c_int]
        L.s3d_k_sep_fir_div_typed.argtypes = [_vp, C.c_int, C.c_double, C.c_double, _vp, _vp, C.c_int, C.c_int, C.c_int,
                                              _f32p, _f32p, C.c_int, _vp, _vp]
        # region of interest: (bits, nwords, nseg, seg_stride, idx_base, idx, tag, tag0, capacity, count, scratch[, and], stream)
        L.s3d_k_compact_bits_multi.argtypes = [_vp, C.c_size_t, C.c_int, C.c_size_t, C.c_uint32, _vp, _vp, C.c_uint32,
                                               C.c_uint32, _vp, _vp, _vp]
        if hasattr(L, "s3d_k_mask_pack"):                 # (absent from builds older than the region of interest, see above)
            L.s3d_k_compact_bits_multi_and.argtypes = [_vp, C.c_size_t, C.c_int, C.c_size_t, C.c_uint32, _vp, _vp, C.c_uint32,
                                                       C.c_uint32, _vp, _vp, _vp, _vp]
            L.s3d_k_mask_pack.argtypes = [_vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _vp]
        if hasattr(L, "s3d_k_select_strongest"):          # (absent from builds older than the keypoint budget)
            L.s3d_k_key_strength.argtypes = [_vp, _vp, _vp, _vp, C.c_uint32, _vp, _vp]
            L.s3d_k_select_scratch_bytes.argtypes = [C.c_uint32]
            L.s3d_k_select_scratch_bytes.restype = C.c_size_t
            L.s3d_k_select_strongest.argtypes = [_vp, _vp, C.c_uint32, C.c_uint32, _vp, _vp]
        if hasattr(L, "s3d_k_ransac_count"):              # (absent from builds older than the device-scored RANSAC)
            L.s3d_k_ransac_count.argtypes = [_vp, _vp, C.c_uint32, _vp, C.c_uint32, C.c_double, _vp, _vp]
        if hasattr(L, "s3d_k_refine_keys"):               # (absent from builds older than the sub-voxel refinement)
            L.s3d_k_refine_keys.argtypes = [_vp, _vp, _vp, C.c_uint32, _vp, _vp, _vp, _vp]
        if hasattr(L, "s3d_k_inv_tps"):                   # (absent from builds older than the thin-plate spline)
            L.s3d_k_inv_tps.argtypes = [_vp, C.c_int, C.c_int, C.c_int, C.c_int, _vp, C.c_int, C.c_int, C.c_int, _vp, _vp,
                                        C.c_uint32, C.c_int, _vp]
        if hasattr(L, "s3d_k_similarity_affine"):         # (absent from builds older than the similarity scores)
            _sim_tail = [C.c_int, C.c_int] + [C.c_double] * 6 + [_vp, _vp, _vp, _vp]   # interp, bins, range / scale / pivots, ...
            L.s3d_k_similarity_scratch_bytes.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int]
            L.s3d_k_similarity_scratch_bytes.restype = C.c_size_t
            L.s3d_k_similarity_affine.argtypes = [_vp, C.c_int, C.c_int, C.c_int, _vp, C.c_int, C.c_int, C.c_int,
                                                  C.POINTER(C.c_double)] + _sim_tail
            L.s3d_k_similarity_tps.argtypes = [_vp, C.c_int, C.c_int, C.c_int, _vp, C.c_int, C.c_int, C.c_int, _vp, _vp,
                                               C.c_uint32] + _sim_tail
            L.s3d_k_minmax_finite.argtypes = [_vp, C.c_size_t, _vp, _vp]
            L.s3d_k_similarity_set_aggregate.argtypes = [C.c_int]
            L.s3d_k_similarity_set_aggregate.restype = None
        if hasattr(L, "s3d_k_affine_normal_eq"):          # (absent from builds older than the intensity-based refinement)
            L.s3d_k_affine_normal_eq_scratch_bytes.argtypes = [C.c_int, C.c_int, C.c_int]
            L.s3d_k_affine_normal_eq_scratch_bytes.restype = C.c_size_t
            L.s3d_k_affine_normal_eq.argtypes = [_vp, C.c_int, C.c_int, C.c_int, _vp, C.c_int, C.c_int, C.c_int,
                                                 C.POINTER(C.c_double), C.POINTER(C.c_double)] + [C.c_double] * 4 + [_vp, _vp, _vp]
        if hasattr(L, "s3d_k_demons_step"):               # (absent from builds older than the deformable registration)
            L.s3d_k_demons_step_scratch_bytes.argtypes = [C.c_int, C.c_int, C.c_int]
            L.s3d_k_demons_step_scratch_bytes.restype = C.c_size_t
            L.s3d_k_demons_step.argtypes = [_vp, C.c_int, C.c_int, C.c_int, _vp, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double),
                                            _vp, _vp] + [C.c_double] * 5 + [_vp, _vp, _vp]
            L.s3d_k_inv_field.argtypes = [_vp, C.c_int, C.c_int, C.c_int, C.c_int, _vp, C.c_int, C.c_int, C.c_int,
                                          C.POINTER(C.c_double), _vp, C.c_int, _vp]
            L.s3d_k_field_upsample2.argtypes = [_vp, C.c_int, C.c_int, C.c_int, _vp, C.c_int, C.c_int, C.c_int, _vp]
            L.s3d_k_field_norm.argtypes = [_vp, C.c_size_t, _vp, _vp]
        if hasattr(L, "s3d_k_field_invert"):              # (absent from builds older than the field inversion)
            _dp = C.POINTER(C.c_double)
            L.s3d_k_field_invert.argtypes = [_vp, C.c_int, C.c_int, C.c_int, _dp, _dp, _vp, C.c_int, C.c_int, C.c_int, C.c_int,
                                             C.c_double, _vp, _vp, _vp]
            L.s3d_k_field_jacobian.argtypes = [_vp, C.c_int, C.c_int, C.c_int, _dp, _vp, _vp, _vp]
        L.s3d_mesh_table.argtypes = [_f32p]
        L.s3d_mesh_table.restype = None

    def err(self) -> str:
        return (self.L.s3d_rt_last_error() or b"").decode()

    def check(self, rc: int, what: str = "device call") -> None:
        if rc != 0:
            raise RuntimeError(f"{what} failed: {self.err()}")

    def device_count(self) -> int:
        n = C.c_int(0)
        rc = self.L.s3d_rt_device_count(C.byref(n))
        return n.value if rc == 0 else 0

    def mem_info(self) -> tuple:
        """(free, total) bytes of device memory on the current device (hipMemGetInfo)."""
        free, total = C.c_size_t(0), C.c_size_t(0)
        self.check(self.L.s3d_rt_mem_info(C.byref(free), C.byref(total)), "s3d_rt_mem_info")
        return free.value, total.value

    # --- memory helpers (numpy <-> HBM) -----------------------------------------------------------
    def malloc(self, nbytes: int) -> int:
        p = _vp()
        self.check(self.L.s3d_rt_malloc(C.byref(p), nbytes), "s3d_rt_malloc")
        return p.value

    def free(self, p: int) -> None:
        self.L.s3d_rt_free(_vp(p))

    def upload(self, a: np.ndarray, stream=None) -> int:
        a = np.ascontiguousarray(a)
        p = self.malloc(a.nbytes)
        self.check(self.L.s3d_rt_h2d(_vp(p), _vp(a.ctypes.data), a.nbytes, _vp(stream)), "h2d")
        self.check(self.L.s3d_rt_sync(_vp(stream)), "sync")
        return p

    def download(self, p: int, shape, dtype=np.float32, stream=None) -> np.ndarray:
        out = np.empty(shape, dtype=dtype)
        self.check(self.L.s3d_rt_d2h(_vp(out.ctypes.data), _vp(p), out.nbytes, _vp(stream)), "d2h")
        self.check(self.L.s3d_rt_sync(_vp(stream)), "sync")
        return out

    def sync(self, stream=None) -> None:
        self.check(self.L.s3d_rt_sync(_vp(stream)), "sync")

    # --- one Gaussian application on device buffers ------------------------------------------------
    def sep_fir(self, d_src: int, d_dst: int, d_tmp: int, nx, ny, nz, nc, uf, taps: np.ndarray, path=0,
                stream=None) -> None:
        t = np.ascontiguousarray(taps, np.float32)
        u = np.asarray(uf, np.float32)
        self.check(self.L.s3d_k_sep_fir_path(_vp(d_src), _vp(d_dst), _vp(d_tmp), nx, ny, nz, nc,
                                             u.ctypes.data_as(_f32p), t.ctypes.data_as(_f32p), t.size, path,
                                             _vp(stream)), "s3d_k_sep_fir_path")

    def conv_axis(self, d_src, d_dst, nx, ny, nz, nc, axis, taps, uf, stream=None) -> None:
        t = np.ascontiguousarray(taps, np.float32)
        self.check(self.L.s3d_k_conv_axis(_vp(d_src), _vp(d_dst), nx, ny, nz, nc, axis, t.ctypes.data_as(_f32p),
                                          t.size, float(uf), _vp(stream)), "s3d_k_conv_axis")

    def nn_match(self, d_a: int, na: int, d_b: int, nb: int, thr: float = 0.8, stride: int = 768,
                 stream=None) -> np.ndarray:
        """SIFT3D_nn_match on device-resident descriptor rows (sift3d_amd_nn_match_dev)."""
        m = np.empty(na, np.int32)
        rc = self.L.sift3d_amd_nn_match_dev(d_a, stride, na, d_b, stride, nb, thr,
                                            m.ctypes.data_as(C.POINTER(C.c_int)), stream)
        self.check(rc, "sift3d_amd_nn_match_dev")
        return m

    # --- volumes of 8- / 16-bit integers as stored ----------------------------------------------------
    def convert_f32(self, d_src: int, dtype, n: int, slope: float, inter: float, d_dst: int, stream=None) -> None:
        """d_dst[i] = (float)((double)d_src[i] * slope + inter); dtype: a numpy dtype of the four integer types."""
        self.check(self.L.s3d_k_convert_f32(_vp(d_src), abi.TYPED_DTYPES[np.dtype(dtype)], n, slope, inter, _vp(d_dst),
                                            _vp(stream)), "s3d_k_convert_f32")

    def absmax_typed(self, d_src: int, dtype, n: int, slope: float, inter: float, d_max: int, stream=None) -> None:
        """*d_max = max |converted d_src[i]| (s3d_k_absmax_typed)."""
        self.check(self.L.s3d_k_absmax_typed(_vp(d_src), abi.TYPED_DTYPES[np.dtype(dtype)], n, slope, inter, _vp(d_max),
                                             _vp(stream)), "s3d_k_absmax_typed")

    # --- region of interest ------------------------------------------------------------------------------
    def mask_pack(self, d_mask: int, nx: int, ny: int, odims, shift: int, d_bits: int, stream=None) -> None:
        """One bit per voxel of the octave ``odims`` = (onx, ony, onz) from the byte mask of an nx x ny x . volume
        (s3d_k_mask_pack): ceil(onx * ony * onz / 64) words at d_bits."""
        self.check(self.L.s3d_k_mask_pack(_vp(d_mask), nx, ny, odims[0], odims[1], odims[2], shift, _vp(d_bits), _vp(stream)),
                   "s3d_k_mask_pack")

    def compact_bits_multi_and(self, d_bits: int, nwords: int, nseg: int, seg_stride: int, idx_base: int, d_idx: int,
                               d_tag: int, tag: int, capacity: int, d_count: int, d_scratch: int, d_and: int | None,
                               stream=None) -> None:
        """s3d_k_compact_bits_multi over d_bits[w] & d_and[w]; d_and None: no AND."""
        self.check(self.L.s3d_k_compact_bits_multi_and(_vp(d_bits), nwords, nseg, seg_stride, idx_base, _vp(d_idx), _vp(d_tag),
                                                       tag, capacity, _vp(d_count), _vp(d_scratch), _vp(d_and), _vp(stream)),
                   "s3d_k_compact_bits_multi_and")

    # --- keypoint budget ---------------------------------------------------------------------------------
    def select_scratch_bytes(self, num: int) -> int:
        return int(self.L.s3d_k_select_scratch_bytes(num))

    def select_strongest(self, d_strength: int, d_keep: int, num: int, budget: int, d_scratch: int, stream=None) -> None:
        """Clears d_keep[i] (uint32) of every kept entry that is not among the ``budget`` kept entries of largest d_strength
        (float32, non-negative); ties go to the lower i (s3d_k_select_strongest)."""
        self.check(self.L.s3d_k_select_strongest(_vp(d_strength), _vp(d_keep), num, budget, _vp(d_scratch), _vp(stream)),
                   "s3d_k_select_strongest")

    # --- sub-voxel refinement ----------------------------------------------------------------------------
    def refine_keys(self, pyr_desc, d_xyzos: int, d_num: int, max_num: int, d_off: int, d_flags: int, d_counters: int,
                    stream=None) -> None:
        """Offsets (4 float64 per record: dx, dy, dz in octave voxels, ds in levels), flag words (uint32) and the two
        counters of the *d_num <= max_num records d_xyzos (int32 x, y, z, o, s) -- s3d_k_refine_keys.  ``pyr_desc``: a
        ctypes image of s3d_pyramid_desc (include/s3d_device.h), passed by reference."""
        self.check(self.L.s3d_k_refine_keys(C.byref(pyr_desc), _vp(d_xyzos), _vp(d_num), max_num, _vp(d_off), _vp(d_flags),
                                            _vp(d_counters), _vp(stream)), "s3d_k_refine_keys")

    # --- RANSAC consensus counts -------------------------------------------------------------------------
    def ransac_count(self, d_src: int, d_ref: int, npts: int, d_models: int, nmodels: int, thr2: float, d_counts: int,
                     stream=None) -> None:
        """d_counts[m] (int32) = number of matches i with !(|src_i - M_m [ref_i 1]^T|^2 > thr2), f64 (s3d_k_ransac_count):
        d_src, d_ref npts x 3 and d_models nmodels x 12 doubles on the device."""
        self.check(self.L.s3d_k_ransac_count(_vp(d_src), _vp(d_ref), npts, _vp(d_models), nmodels, thr2, _vp(d_counts),
                                             _vp(stream)), "s3d_k_ransac_count")

    # --- thin-plate-spline warp -----------------------------------------------------------------------------
    def inv_tps(self, d_src: int, sdims, nc: int, d_dst: int, ddims, d_ctrl: int | None, d_params: int, n_ctrl: int,
                interp: int = 0, stream=None) -> None:
        """d_dst (ddims = (nx, ny, nz), nc channels, float32) = d_src (sdims) sampled at the spline of every output voxel
        (s3d_k_inv_tps): d_ctrl n_ctrl x 3 and d_params 3 x (n_ctrl + 4) doubles on the device; interp 0 tri-linear,
        1 Lanczos-2."""
        self.check(self.L.s3d_k_inv_tps(_vp(d_src), sdims[0], sdims[1], sdims[2], nc, _vp(d_dst), ddims[0], ddims[1], ddims[2],
                                        _vp(d_ctrl), _vp(d_params), n_ctrl, interp, _vp(stream)), "s3d_k_inv_tps")

    # --- similarity of a source under a transform against a reference ---------------------------------------
    def minmax_finite(self, d_v: int, n: int, stream=None) -> tuple:
        """(min, max) over the finite elements of the n float32 at d_v; both NaN when none is (s3d_k_minmax_finite)."""
        d_mm = self.malloc(8)
        try:
            self.check(self.L.s3d_k_minmax_finite(_vp(d_v), n, _vp(d_mm), _vp(stream)), "s3d_k_minmax_finite")
            mm = self.download(d_mm, (2,), np.float32, stream)
        finally:
            self.free(d_mm)
        return float(mm[0]), float(mm[1])

    def _similarity(self, launch, rdims, bins: int, stream):
        nbytes = int(self.L.s3d_k_similarity_scratch_bytes(rdims[0], rdims[1], rdims[2], bins))
        if nbytes == 0:
            raise RuntimeError("s3d_k_similarity_scratch_bytes: bad dimensions or bins")
        d_hist, d_sums, d_scr = self.malloc(bins * bins * 8), self.malloc(7 * 8), self.malloc(nbytes)
        try:
            launch(d_hist, d_sums, d_scr)
            return (self.download(d_hist, (bins, bins), np.uint64, stream), self.download(d_sums, (7,), np.float64, stream))
        finally:
            for p in (d_hist, d_sums, d_scr):
                self.free(p)

    def similarity_affine(self, d_src: int, sdims, d_ref: int, rdims, A, interp: int, bins: int, ref_lo: float,
                          ref_scale: float, src_lo: float, src_scale: float, c_ref: float, c_src: float, stream=None) -> tuple:
        """(joint histogram uint64 [bins, bins], row = reference bin; the seven float64 sums) of d_src (sdims = (nx, ny, nz),
        float32, one channel) sampled at A [x y z 1]^T of every voxel of d_ref (rdims) -- s3d_k_similarity_affine; A: 12
        doubles, 3 x 4 row major."""
        a = np.ascontiguousarray(A, np.float64).reshape(12)
        return self._similarity(lambda h, s, w: self.check(self.L.s3d_k_similarity_affine(
            _vp(d_src), sdims[0], sdims[1], sdims[2], _vp(d_ref), rdims[0], rdims[1], rdims[2],
            a.ctypes.data_as(C.POINTER(C.c_double)), interp, bins, ref_lo, ref_scale, src_lo, src_scale, c_ref, c_src, _vp(h),
            _vp(s), _vp(w), _vp(stream)), "s3d_k_similarity_affine"), rdims, bins, stream)

    def similarity_tps(self, d_src: int, sdims, d_ref: int, rdims, d_ctrl: int | None, d_params: int, n_ctrl: int, interp: int,
                       bins: int, ref_lo: float, ref_scale: float, src_lo: float, src_scale: float, c_ref: float, c_src: float,
                       stream=None) -> tuple:
        """The same through a spline (s3d_k_similarity_tps): d_ctrl n_ctrl x 3 and d_params 3 x (n_ctrl + 4) doubles on the
        device, as for inv_tps."""
        return self._similarity(lambda h, s, w: self.check(self.L.s3d_k_similarity_tps(
            _vp(d_src), sdims[0], sdims[1], sdims[2], _vp(d_ref), rdims[0], rdims[1], rdims[2], _vp(d_ctrl), _vp(d_params),
            n_ctrl, interp, bins, ref_lo, ref_scale, src_lo, src_scale, c_ref, c_src, _vp(h), _vp(s), _vp(w), _vp(stream)),
            "s3d_k_similarity_tps"), rdims, bins, stream)

    # --- normal equations of an intensity-based affine fit ---------------------------------------------------
    def affine_normal_eq(self, d_src: int, sdims, d_ref: int, rdims, A, centre, consts=(1.0, 0.0, 1.0, 0.0),
                         stream=None) -> np.ndarray:
        """The 74 float64 sums of s3d_k_affine_normal_eq (layout: include/s3d_device.h) for d_src (sdims = (nx, ny, nz),
        float32, one channel) sampled at A [x y z 1]^T of every voxel of d_ref (rdims); centre: 3 doubles, consts:
        (sa, ma, sb, mb)."""
        nbytes = int(self.L.s3d_k_affine_normal_eq_scratch_bytes(rdims[0], rdims[1], rdims[2]))
        if nbytes == 0:
            raise RuntimeError("s3d_k_affine_normal_eq_scratch_bytes: bad dimensions")
        a = np.ascontiguousarray(A, np.float64).reshape(12)
        c = np.ascontiguousarray(centre, np.float64).reshape(3)
        dp = C.POINTER(C.c_double)
        d_sums, d_scr = self.malloc(74 * 8), self.malloc(nbytes)
        try:
            self.check(self.L.s3d_k_affine_normal_eq(_vp(d_src), sdims[0], sdims[1], sdims[2], _vp(d_ref), rdims[0], rdims[1],
                                                     rdims[2], a.ctypes.data_as(dp), c.ctypes.data_as(dp), *map(float, consts),
                                                     _vp(d_sums), _vp(d_scr), _vp(stream)), "s3d_k_affine_normal_eq")
            return self.download(d_sums, (74,), np.float64, stream)
        finally:
            self.free(d_sums)
            self.free(d_scr)

    # --- deformable registration: fields are planar, component c of voxel i at [c * N + i] -----------------------
    def demons_step(self, d_src: int, sdims, d_ref: int, rdims, A, d_u: int, d_v: int, consts=(1.0, 0.0, 1.0, 0.0),
                    kstep: float = 0.25, stream=None) -> np.ndarray:
        """One demons update of the planar field d_u into d_v (which may be d_u) and the three float64 sums (sum r^2, n,
        sum |update|^2) of s3d_k_demons_step (include/s3d_device.h); consts: (sa, ma, sb, mb), kstep = 1 / (4 max_step^2)."""
        nbytes = int(self.L.s3d_k_demons_step_scratch_bytes(rdims[0], rdims[1], rdims[2]))
        if nbytes == 0:
            raise RuntimeError("s3d_k_demons_step_scratch_bytes: bad dimensions")
        a = np.ascontiguousarray(A, np.float64).reshape(12)
        d_sums, d_scr = self.malloc(3 * 8), self.malloc(nbytes)
        try:
            self.check(self.L.s3d_k_demons_step(_vp(d_src), sdims[0], sdims[1], sdims[2], _vp(d_ref), rdims[0], rdims[1], rdims[2],
                                                a.ctypes.data_as(C.POINTER(C.c_double)), _vp(d_u), _vp(d_v), *map(float, consts),
                                                float(kstep), _vp(d_sums), _vp(d_scr), _vp(stream)), "s3d_k_demons_step")
            return self.download(d_sums, (3,), np.float64, stream)
        finally:
            self.free(d_sums)
            self.free(d_scr)

    def inv_field(self, d_src: int, sdims, nc: int, d_dst: int, ddims, A, d_u: int, interp: int = 0, stream=None) -> None:
        """d_dst (ddims, nc channels) = d_src (sdims) sampled at A [x y z 1]^T + u of every output voxel, d_u a planar field
        over ddims (s3d_k_inv_field); interp 0 tri-linear, 1 Lanczos-2."""
        a = np.ascontiguousarray(A, np.float64).reshape(12)
        self.check(self.L.s3d_k_inv_field(_vp(d_src), sdims[0], sdims[1], sdims[2], nc, _vp(d_dst), ddims[0], ddims[1], ddims[2],
                                          a.ctypes.data_as(C.POINTER(C.c_double)), _vp(d_u), interp, _vp(stream)),
                   "s3d_k_inv_field")

    def field_upsample2(self, d_coarse: int, cdims, d_fine: int, fdims, stream=None) -> None:
        """The planar field d_coarse (cdims = fdims // 2) one pyramid level up into d_fine, displacements doubled
        (s3d_k_field_upsample2)."""
        self.check(self.L.s3d_k_field_upsample2(_vp(d_coarse), cdims[0], cdims[1], cdims[2], _vp(d_fine), fdims[0], fdims[1],
                                                fdims[2], _vp(stream)), "s3d_k_field_upsample2")

    def field_norm(self, d_u: int, nvox: int, stream=None) -> tuple:
        """(sum, count, maximum) of the lengths of the planar field's entries, those that are not finite left out
        (s3d_k_field_norm; its per-workgroup partials added here in slot order)."""
        slots = int(self.L.s3d_k_field_norm_slots())
        d_part = self.malloc(slots * 3 * 8)
        try:
            self.check(self.L.s3d_k_field_norm(_vp(d_u), nvox, _vp(d_part), _vp(stream)), "s3d_k_field_norm")
            part = self.download(d_part, (slots, 3), np.float64, stream)
        finally:
            self.free(d_part)
        total = 0.0
        for v in part[:, 0]:
            total += float(v)
        return total, int(part[:, 1].sum()), float(part[:, 2].max())

    def field_invert(self, d_u: int, rdims, A, B, d_w: int, sdims, max_iter: int = 30, tol: float = 1e-3,
                     d_status: int | None = None, stream=None) -> dict:
        """The inverse of the map A [x 1]^T + u(x) as the planar field d_w over sdims, B the inverse of A (s3d_k_field_invert;
        d_status: one byte per source voxel or None).  Returns the statistics, the per-workgroup partials added here in slot
        order: counts (four, by status), updates, sum_residual, max_residual."""
        slots, stats = int(self.L.s3d_k_field_invert_slots()), int(self.L.s3d_k_field_invert_stats())
        a = np.ascontiguousarray(A, np.float64).reshape(12)
        b = np.ascontiguousarray(B, np.float64).reshape(12)
        dp = C.POINTER(C.c_double)
        d_part = self.malloc(slots * stats * 8)
        try:
            self.check(self.L.s3d_k_field_invert(_vp(d_u), rdims[0], rdims[1], rdims[2], a.ctypes.data_as(dp), b.ctypes.data_as(dp),
                                                 _vp(d_w), sdims[0], sdims[1], sdims[2], int(max_iter), float(tol), _vp(d_status),
                                                 _vp(d_part), _vp(stream)), "s3d_k_field_invert")
            part = self.download(d_part, (slots, stats), np.float64, stream)
        finally:
            self.free(d_part)
        total = 0.0
        for v in part[:, 5]:
            total += float(v)
        return {"counts": tuple(int(part[:, k].sum()) for k in range(4)), "updates": int(part[:, 4].sum()),
                "sum_residual": total, "max_residual": float(part[:, 6].max())}

    def field_jacobian(self, d_u: int, rdims, A, d_det: int | None = None, stream=None) -> dict:
        """det(A's linear part + grad u) per voxel of the planar field d_u to d_det (float32, or None: statistics only) --
        s3d_k_field_jacobian.  Returns the statistics over the finite determinants, the partials added here in slot order: sum,
        n_finite, n_folded (those <= 0), min, max (NaN when none is finite)."""
        slots, stats = int(self.L.s3d_k_field_jacobian_slots()), int(self.L.s3d_k_field_jacobian_stats())
        a = np.ascontiguousarray(A, np.float64).reshape(12)
        d_part = self.malloc(slots * stats * 8)
        try:
            self.check(self.L.s3d_k_field_jacobian(_vp(d_u), rdims[0], rdims[1], rdims[2], a.ctypes.data_as(C.POINTER(C.c_double)),
                                                   _vp(d_det), _vp(d_part), _vp(stream)), "s3d_k_field_jacobian")
            part = self.download(d_part, (slots, stats), np.float64, stream)
        finally:
            self.free(d_part)
        used = part[part[:, 1] > 0]
        total = 0.0
        for v in used[:, 0]:
            total += float(v)
        return {"sum": total, "n_finite": int(used[:, 1].sum()), "n_folded": int(used[:, 2].sum()),
                "min": float(used[:, 3].min()) if len(used) else float("nan"),
                "max": float(used[:, 4].max()) if len(used) else float("nan")}

    def mesh_table(self) -> np.ndarray:
        out = np.zeros(20 * 16 + 32, np.float32)      # S3D_MESH_FLOATS: face table + 32-word face LUT
        self.L.s3d_mesh_table(out.ctypes.data_as(_f32p))
        return out
