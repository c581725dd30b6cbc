/* s3d_device.h -- the thin C-ABI seam between the host C code and the hand-written HIP kernels.
 *
 * Plain pointers and sizes only (no HIP or torch types): every `d_*` pointer is device (HBM)
 * memory, every other pointer is host memory.  All launches are asynchronous on `stream`
 * (an opaque hipStream_t; NULL = the default stream) and return 0 on success, -1 on a HIP error
 * (text via s3d_rt_last_error()).  Nothing here falls back to the CPU: without a usable gfx950
 * device every call fails.
 *
 * Each kernel cites the reference routine whose arithmetic it reproduces (paths relative to the
 * reference tree, bbrister/SIFT3D v1.4.6).
 */
#ifndef S3D_DEVICE_H
#define S3D_DEVICE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void *s3d_stream;

#define S3D_MAX_TAPS 129     /* widest separable filter accepted (half width 64) */
#define S3D_MAX_OCTAVES 16
#define S3D_MAX_LEVELS 16    /* GSS levels per octave (num_kp_levels + 3) */
#define S3D_DESC_NUMEL 768
#define S3D_NFACES 20
#define S3D_NVERT 12

/* ---- runtime ----------------------------------------------------------------------------------- */
int s3d_rt_device_count(int *count);
int s3d_rt_set_device(int dev);
int s3d_rt_get_device(int *dev);
int s3d_rt_malloc(void **d_ptr, size_t bytes);
int s3d_rt_mem_info(size_t *free_bytes, size_t *total_bytes);   /* hipMemGetInfo of the current device */
int s3d_rt_free(void *d_ptr);
int s3d_rt_h2d(void *d_dst, const void *src, size_t bytes, s3d_stream stream);
int s3d_rt_d2h(void *dst, const void *d_src, size_t bytes, s3d_stream stream);
int s3d_rt_d2d(void *d_dst, const void *d_src, size_t bytes, s3d_stream stream);
int s3d_rt_memset(void *d_ptr, int value, size_t bytes, s3d_stream stream);
int s3d_rt_sync(s3d_stream stream);
int s3d_rt_sync_timeout(s3d_stream stream, double timeout_s);   /* 0 drained, 1 still busy after timeout_s, -1 error */
int s3d_rt_stream_create(s3d_stream *stream);
int s3d_rt_stream_create_nonblocking(s3d_stream *stream);   /* does not synchronise with the NULL stream */
int s3d_rt_stream_destroy(s3d_stream stream);
/* HIP events on `stream`, for timing the kernels where they run (bench.py) */
int s3d_rt_event_create(void **ev);
int s3d_rt_event_destroy(void *ev);
int s3d_rt_event_record(void *ev, s3d_stream stream);
int s3d_rt_event_elapsed_ms(void *ev_start, void *ev_stop, float *ms); /* synchronises on ev_stop */
int s3d_rt_event_sync(void *ev);
int s3d_rt_stream_wait_event(s3d_stream stream, void *ev);   /* work queued on stream after this waits for ev */
/* pinned host memory: page-lock a caller's buffer / allocate a page-locked staging buffer */
int s3d_rt_host_register(void *p, size_t bytes);
int s3d_rt_host_unregister(void *p);
int s3d_rt_host_alloc(void **p, size_t bytes);
int s3d_rt_host_free(void *p);
const char *s3d_rt_last_error(void);

/* ---- image ops ---------------------------------------------------------------------------------- */
/* *d_max = max |v[i]|     (im_max_abs, imutil/imutil.c:1959-1973).  d_max is overwritten.  Order-free reduction over the
 * bit patterns of |v|: exact for finite values and infinities; if any v[i] is a NaN the result is a NaN ("sticky") -- the
 * reference's sequential scan then gives something else, see s3d_k_seqmax. */
int s3d_k_absmax(const float *d_v, size_t n, float *d_max, s3d_stream stream);
/* The reference's maximum whatever the input holds: max |a[i]| (d_b == NULL) or max |a[i] - b[i]| as the SEQUENTIAL scan
 * max = (max > samp ? max : samp) computes it (imutil/imutil.c:1959-1973, sift3d/sift.c:1161-1166, immacros.h:36): a NaN
 * replaces the running maximum and the next sample replaces the NaN, so the result is the maximum of the samples behind the
 * last NaN in index order (0 if none follow), and that NaN itself if it is the last sample.  Without a NaN: s3d_k_absmax /
 * s3d_k_dogmax plus three launches that return at once.  d_rec16: 16 bytes of device scratch (8-byte aligned) owned by the
 * call until it has run.  s3d_k_seqmax_parts leaves there { sticky max bits, max bits behind the last NaN, index + 1 of the
 * last NaN as 64 bits (0: none) } for callers that combine several index ranges (the Z-slab ranks). */
int s3d_k_seqmax(const float *d_a, const float *d_b, size_t n, float *d_max, void *d_rec16, s3d_stream stream);
/* The same for the three DoG levels between four consecutive GSS levels, d_max3[s] = s3d_k_seqmax(d_levels[s], d_levels[s + 1]):
 * the sticky maxima and last NaNs of all three from one pass over the four levels.  d_rec48: 48 bytes, 8-byte aligned. */
int s3d_k_seqmax3(const float *const *d_levels, size_t n, float *d_max3, void *d_rec48, s3d_stream stream);
int s3d_k_seqmax_parts(const float *d_a, const float *d_b, size_t n, void *d_rec16, s3d_stream stream);
/* v[i] = v[i] / *d_max unless *d_max == 0   (im_scale, imutil/imutil.c:1977-1991; true division) */
int s3d_k_scale_div(float *d_v, size_t n, const float *d_max, s3d_stream stream);
/* dst(x,y,z) = src(2x,2y,2z), dst dims = floor(n/2)   (im_downsample_2x, imutil/imutil.c:1742-1768) */
int s3d_k_decimate2(const float *d_src, int nx, int ny, int nz, float *d_dst, s3d_stream stream);
/* the same for nc interleaved channels (im_downsample_2x on a multi-channel Image) */
int s3d_k_decimate2_nc(const float *d_src, int nx, int ny, int nz, int nc, float *d_dst, s3d_stream stream);
/* dst = a - b   (im_subtract, imutil/imutil.c:1997-2017) */
int s3d_k_subtract(const float *d_a, const float *d_b, float *d_dst, size_t n, s3d_stream stream);

/* ---- separable FIR / Gaussian  (apply_Sep_FIR_filter imutil.c:3459-3544,
 *      convolve_sep_gen imutil.c:2274-2393) ------------------------------------------------------- */
/* One axis pass with the reference's exact per-element arithmetic: tap spacing `uf` voxels
 * (unit / units[axis] as float), 2-point interpolation, asymmetric mirror boundary.  Any nc. */
int s3d_k_conv_axis(const float *d_src, float *d_dst, int nx, int ny, int nz, int nc, int axis,
                    const float *taps, int width, float uf, s3d_stream stream);
/* All three axes (x, y, z; each pass rounded to f32).  d_tmp: scratch of the same size.
 * d_src may equal d_dst.  Uses the fused streaming kernels when uf == (1,1,1) and nc == 1
 * (octave 0 of a unit-voxel volume: the roofline configuration), the generic pass otherwise. */
int s3d_k_sep_fir(const float *d_src, float *d_dst, float *d_tmp, int nx, int ny, int nz, int nc,
                  const float uf[3], const float *taps, int width, s3d_stream stream);
/* The same for one channel, plus s3d_k_absmax of the result into *d_max (the z pass keeps the maximum: no pass of its own).
 * Returns 1 without doing anything where the fused unit-spacing kernels do not apply; the caller then runs the two steps. */
int s3d_k_sep_fir_max(const float *d_src, float *d_dst, float *d_tmp, int nx, int ny, int nz, const float uf[3],
                      const float *taps, int width, float *d_max, s3d_stream stream);
/* Z-slab form: the pointers are VIEWS addressed by global z -- element (x,y,z)
 * at view[(z*ny + y)*nx + x] -- of which only the caller's planes plus halos are backed by memory.
 * Produces dst planes [z0, z1) from src planes [z0-h, z1+h) clamped to [0, nz), h = ceil(hw*uf[2]) + 1 (the
 * extra plane: the reference's drifting tap coordinate, see s3d_gauss.hip; fused unit-spacing path: hw):
 * the halo planes come from the Z-neighbours; the global ends use the reference's mirror rule.
 * dst / tmp planes in that range are scratch.  nc == 1. */
int s3d_k_sep_fir_slab(const float *d_src, float *d_dst, float *d_tmp, int nx, int ny, int nz, int z0,
                       int z1, const float uf[3], const float *taps, int width, s3d_stream stream);
/* im_scale (imutil.c:1977) folded into the filter that follows it: dst planes [z0, z1) = filter(src / *d_div), every
 * source voxel divided as it is loaded (*d_div == 0: not divided), so the scaled image is never written.  For the
 * configurations the fused unit-spacing kernels take and those whose x pass is table-driven (any spacing, any row
 * length, volumes above 64^3) -- s3d_k_sep_fir_div_eligible() != 0 -- and an error otherwise. */
int s3d_k_sep_fir_div_eligible(int nx, int ny, int nz, const float uf[3], int width);
int s3d_k_sep_fir_div(const float *d_src, float *d_dst, float *d_tmp, int nx, int ny, int nz, int z0, int z1,
                      const float uf[3], const float *taps, int width, const float *d_div, s3d_stream stream);
/* ---- volumes of 8- and 16-bit integers, read as stored ---------------------------------------------------------------
 * Element types by their NIfTI-1 datatype code.  The value of a voxel is (float)((double)raw * slope + inter) everywhere:
 * two separately rounded f64 operations and one conversion, what the host reader computes (s3d_host_io.c).  d_src must be
 * aligned to its element size; slope and inter finite. */
#define S3D_DT_U8 2
#define S3D_DT_I16 4
#define S3D_DT_I8 256
#define S3D_DT_U16 512
/* bytes per element; 0: not one of the four */
int s3d_k_typed_elem_size(int dtype);
/* d_dst[i] = value of d_src[i] (d_dst dword aligned): afterwards the volume is an ordinary float volume */
int s3d_k_convert_f32(const void *d_src, int dtype, size_t n, double slope, double inter, float *d_dst, s3d_stream stream);
/* *d_max = max |value of d_src[i]|, the bits s3d_k_absmax gives on the converted volume, from 1 or 2 bytes per voxel.
 * (The value is monotone in the raw element, roundings included, so the maximum is taken over the raw elements' minimum and
 * maximum and only those two are converted.) */
int s3d_k_absmax_typed(const void *d_src, int dtype, size_t n, double slope, double inter, float *d_max, s3d_stream stream);
/* s3d_k_sep_fir_div over the whole volume with the conversion folded into the loads as well: dst = filter(value(src) / *d_div)
 * on the fused unit-spacing kernels.  Eligible: where s3d_k_sep_fir_div takes those kernels, nx % 4 == 0, d_src aligned to
 * four elements and a filter of at most 17 taps; an error otherwise (callers convert first: s3d_k_convert_f32). */
int s3d_k_sep_fir_div_typed_eligible(const void *d_src, int dtype, int nx, int ny, int nz, const float uf[3], int width);
int s3d_k_sep_fir_div_typed(const void *d_src, int dtype, double slope, double inter, float *d_dst, float *d_tmp, int nx,
                            int ny, int nz, const float uf[3], const float *taps, int width, const float *d_div,
                            s3d_stream stream);
/* Force a code path (tests / profiling): 0 = auto, 1 = generic per-axis passes, 2 = fused fast path
 * (fails if the configuration is not eligible). */
/* The three knobs below are per calling thread (thread_local): tests and bench.py set them on the thread that then
 * makes the calls; other threads' SIFT3D objects are not affected. */
/* rows (planes) per marching chunk of the fused kernels: occupancy vs warm-up re-reads */
void s3d_k_gauss_set_chunks(int chunk_xy, int chunk_z);
/* record HIP events (from s3d_rt_event_create) before k_gauss_xy, between, and after k_gauss_z of the
 * next fused applications; NULLs switch it off.  For bench.py's per-kernel timing. */
void s3d_k_gauss_set_events(void *before_xy, void *between, void *after_z);
/* profiling knobs, see s3d_gauss.hip -- and mode 64, "verbatim", which is not one: every axis pass on the per-element
 * kernel that evaluates both samples of every tap as the reference does (0 * NaN is NaN).  The host pipelines select it
 * for volumes that hold non-finite voxels and restore what s3d_k_gauss_get_mode returned before. */
void s3d_k_gauss_set_mode(int mode);
int s3d_k_gauss_get_mode(void);
/* Volumes of up to max_voxels output voxels run the three passes of an application in one launch (k_gauss3_tile: the
 * coarse octaves of a pyramid, bound by launch and L2 latency); 0 = never, < 0 = the default (64^3, or S3D_TILE3_MAX).
 * Per calling thread.  s3d_k_gauss_tile3_launches: how many such launches the calling thread has made (tests). */
void s3d_k_gauss_set_tile3(long max_voxels);
long s3d_k_gauss_tile3_launches(void);
/* The table-driven axis passes (s3d_gauss_tab.hip: any tap spacing, any row length; chosen by the library for volumes
 * above 64^3 wherever the unit-spacing and dyadic kernels do not apply).  Outputs per marching chunk, the number of such
 * passes the calling thread has launched (tests), and the release of the tap tables of every device. */
void s3d_k_gauss_tab_set_chunk(int chunk);
long s3d_k_gauss_tab_launches(void);
void s3d_k_tap_tables_release(void);
int s3d_k_sep_fir_path(const float *d_src, float *d_dst, float *d_tmp, int nx, int ny, int nz,
                       int nc, const float uf[3], const float *taps, int width, int path,
                       s3d_stream stream);

/* ---- DoG + extrema  (build_dog sift3d/sift.c:1052-1071, detect_extrema sift.c:1074-1212) -------- */
/* *d_max = max |a - b|  : per-level `dogmax` (sift.c:1161-1166) without materialising the DoG (sticky like s3d_k_absmax). */
int s3d_k_dogmax(const float *d_a, const float *d_b, size_t n, float *d_max, s3d_stream stream);
/* d_max3[k] = max |d_levels4[k] - d_levels4[k+1]|, k = 0..2, in one pass (16-byte aligned levels; the host array
 * of four device pointers is read at call time). */
int s3d_k_dogmax3(const float *const *d_levels4, size_t n, float *d_max3, s3d_stream stream);
/* Extrema of DoG(s) = L1 - L2 against DoG(s-1) = L0 - L1 and DoG(s+1) = L2 - L3 for one level:
 * bit i of d_bits (64-bit words, little-endian bit order) is set iff linear voxel i is a candidate
 * (strict 6-neighbour + prev/next centre test, |v| > (float)(peak_thresh * *d_dogmax)).
 * d_bits must hold ceil(n/64) words; every word is written. */
int s3d_k_extrema(const float *d_l0, const float *d_l1, const float *d_l2, const float *d_l3,
                  int nx, int ny, int nz, double peak_thresh, const float *d_dogmax,
                  unsigned long long *d_bits, s3d_stream stream);
/* The same for the planes [z0, z1) of a level given as views addressed by global z (needs one halo
 * plane on each interior side); bit i of d_bits <-> voxel z0*nx*ny + i. */
int s3d_k_extrema_slab(const float *d_l0, const float *d_l1, const float *d_l2, const float *d_l3,
                       int nx, int ny, int nz, int z0, int z1, double peak_thresh, const float *d_dogmax,
                       unsigned long long *d_bits, s3d_stream stream);
/* All nkp keypoint levels of one octave in a single pass over the nkp+3 GSS levels d_levels[0..nkp+2]
 * (d_levels[0] = L(s-1) of the first keypoint level).  d_dogmax[k] / d_bits[k] belong to keypoint level k.
 * Planes [z0, z1).  Returns 1 and does nothing when the configuration is not eligible (use the per-level
 * call), 0 on success, -1 on error. */
#define S3D_FUSED_KP_MAX 3
int s3d_k_extrema_fused(const float *const *d_levels, int nkp, int nx, int ny, int nz, int z0, int z1,
                        double peak_thresh, const float *d_dogmax, unsigned long long *const *d_bits,
                        s3d_stream stream);
/* The same with every neighbour test written as its own comparison (no maximum / minimum of neighbours in between): the bitmaps
 * of s3d_k_extrema_slab per level bit for bit also on levels that hold NaNs or infinities (a comparison with a NaN is false; the
 * maximum of the other neighbours would still be compared).  The verbatim pass of volumes with non-finite voxels. */
int s3d_k_extrema_fused_literal(const float *const *d_levels, int nkp, int nx, int ny, int nz, int z0, int z1,
                                double peak_thresh, const float *d_dogmax, unsigned long long *const *d_bits,
                                s3d_stream stream);
/* The same without the DoG maxima being known beforehand, as two calls (a Z-slab rank all-reduces d_dogmax in between):
 * s3d_k_extrema_fused_runmax zeroes d_dogmax[0..nkp), finds a superset of the extrema of planes [z0, z1) under a running
 * lower bound of the maxima and leaves the exact maxima of those planes in d_dogmax; s3d_k_extrema_refilter applies the
 * exact thresholds to the bitmaps.  Bitmaps identical to s3d_k_dogmax3 + s3d_k_extrema_fused, one pass over four GSS
 * levels less.  Returns 1 (nothing done) where s3d_k_extrema_fused would. */
int s3d_k_extrema_fused_runmax(const float *const *d_levels, int nkp, int nx, int ny, int nz, int z0, int z1,
                               double peak_thresh, float *d_dogmax, unsigned long long *const *d_bits, s3d_stream stream);
int s3d_k_extrema_refilter(const float *const *d_levels, int nkp, int nx, int ny, int nz, int z0, int z1,
                           double peak_thresh, const float *d_dogmax, unsigned long long *const *d_bits, s3d_stream stream);
/* Ordered compaction of a bitmap: appends the indices of set bits, ascending, to d_idx starting at
 * position *d_count, tags each with `tag` in d_tag, and advances *d_count.  Entries past `capacity`
 * are dropped (the count still advances, so overflow is detectable).  d_scratch: >= nwords/1024+2
 * uint32. */
int s3d_k_compact_bits(const unsigned long long *d_bits, size_t nwords, uint32_t *d_idx,
                       uint32_t *d_tag, uint32_t tag, uint32_t capacity, uint32_t *d_count,
                       uint32_t *d_scratch, s3d_stream stream);
/* as above with bit i <-> voxel idx_base + i */
int s3d_k_compact_bits_base(const unsigned long long *d_bits, size_t nwords, uint32_t idx_base,
                            uint32_t *d_idx, uint32_t *d_tag, uint32_t tag, uint32_t capacity,
                            uint32_t *d_count, uint32_t *d_scratch, s3d_stream stream);
/* The same for nseg bitmaps of nwords words lying seg_stride words apart (the keypoint levels of one octave), appended
 * one after the other with tags tag, tag + 1, ..: one count / scan / emit triple instead of nseg.  d_scratch: nseg *
 * ceil(nwords / 1024) counters. */
int s3d_k_compact_bits_multi(const unsigned long long *d_bits, size_t nwords, int nseg, size_t seg_stride, uint32_t idx_base,
                             uint32_t *d_idx, uint32_t *d_tag, uint32_t tag, uint32_t capacity, uint32_t *d_count,
                             uint32_t *d_scratch, s3d_stream stream);

/* s3d_k_compact_bits_multi over d_bits[w] & d_and[w]: d_and holds nwords words shared by all nseg segments (the octave's
 * region-of-interest bitmap, s3d_k_mask_pack); d_and == NULL is s3d_k_compact_bits_multi.  The count advances by the
 * population of the ANDed words. */
int s3d_k_compact_bits_multi_and(const unsigned long long *d_bits, size_t nwords, int nseg, size_t seg_stride, uint32_t idx_base,
                                 uint32_t *d_idx, uint32_t *d_tag, uint32_t tag, uint32_t capacity, uint32_t *d_count,
                                 uint32_t *d_scratch, const unsigned long long *d_and, s3d_stream stream);
/* A byte mask of the input volume (rows of nx bytes, planes of nx * ny) as one bit per voxel of the octave it was decimated
 * to `shift` times (dims onx x ony x onz, from the pyramid): bit i = x + onx * (y + ony * z) of d_bits is set iff the byte at
 * (x << shift, y << shift, z << shift) is non-zero -- the voxel of the input that octave voxel is (im_downsample_2x takes
 * voxel (2x, 2y, 2z), imutil.c:1742-1768).  Writes ceil(onx * ony * onz / 64) words, every one of them, once; bits past the
 * last voxel are zero. */
int s3d_k_mask_pack(const unsigned char *d_mask, int nx, int ny, int onx, int ony, int onz, int shift,
                    unsigned long long *d_bits, s3d_stream stream);

/* ---- keypoints ----------------------------------------------------------------------------------- */
typedef struct {
    const float *d_level[S3D_MAX_OCTAVES * S3D_MAX_LEVELS]; /* GSS level data, [o*num_levels + (s-first_level)] */
    int dims[S3D_MAX_OCTAVES][3];                           /* per octave nx, ny, nz */
    float unitsf[S3D_MAX_OCTAVES][3];                       /* per octave (float) ux, uy, uz */
    int num_octaves, num_levels, first_level;
} s3d_pyramid_desc;

/* assign_eig_ori (sift.c:1354-1514) + assign_orientation_thresh (sift.c:1331-1342) for `num`
 * candidates with tag = o<<8 | (s - first_level) (d_tag == NULL: all in level 0).  Window centre: the
 * voxel of linear index d_idx[i] (d_idx == NULL: voxel i, the dense case) when d_center == NULL (detected candidates; d_sigma is then indexed per level,
 * [o*num_levels + k], = 1.5 * level scale), else the float triple d_center[3i..] (raw-image
 * variant, sift.c:1534-1604; d_sigma is then per candidate).
 * Outputs: d_R[9*i] row-major rotation, d_keep[i] = 1 iff not rejected and conf >= corner_thresh,
 * d_conf[i] (optional) = corner score, 0 when rejected.  Three launches per chunk: window sums (a wave per
 * candidate), decisions (a thread per candidate), the ordered sum for the few the bound left undecided.
 * d_fail (optional): one word the call sets to 1 (and never clears) when some candidate's window holds a NaN gradient --
 * the reference's eigen_Mat_rm fails on the NaN structure tensor (LAPACK dsyevd, info > 0) and with it the whole
 * SIFT3D_detect_keypoints / SIFT3D_assign_orientations call (sift.c:1430-1431, 1293-1296); such a candidate is not kept. */
int s3d_k_orient(const s3d_pyramid_desc *pyr, const uint32_t *d_idx, const uint32_t *d_tag,
                 const float *d_center, uint32_t num, const double *d_sigma, double corner_thresh,
                 float *d_R, uint32_t *d_keep, double *d_conf,
                 void *d_scratch /* s3d_k_orient_scratch_bytes(num) bytes */, uint32_t *d_fail, s3d_stream stream);
/* The same with the levels' window tables: d_tabs = s3d_k_orient_tab_bytes(pyr) bytes of device memory the call fills
 * (one launch, a wave per level) and the window sums then replay -- the window of a candidate with an integer centre
 * away from the faces of the volume is a property of its level, whatever the units are (which
 * voxels, in which order, with which weights), so the row intervals, scans and weights need not be redone per
 * candidate.  Same results, bit for bit; d_tabs == NULL is s3d_k_orient. */
#define S3D_ORI_TAB_TURNS 128                /* turns of 64 lanes a table holds (default parameters: 11-27) */
typedef struct { int off, nval, pad0, pad1; float w[4]; } s3d_ori_ent;   /* a lane's four x-consecutive voxels of one turn */
typedef struct {
    int n_turns;                             /* 0: no table for this level (the general path serves it) */
    int rb[6];                               /* the window's bounding box relative to the centre: xs xe ys ye zs ze */
    int pad;
    s3d_ori_ent ent[S3D_ORI_TAB_TURNS * 64];
} s3d_ori_tab;
size_t s3d_k_orient_tab_bytes(const s3d_pyramid_desc *pyr);
/* Nonzero when s3d_k_orient_tab will use d_tabs for this pyramid: the knob below asks for it, or the levels' units are not
 * one power of two (no per-wave weight table: the replayed weights then save an expf per window voxel). */
int s3d_k_orient_wants_tab(const s3d_pyramid_desc *pyr);
int s3d_k_orient_tab(const s3d_pyramid_desc *pyr, const uint32_t *d_idx, const uint32_t *d_tag,
                     const float *d_center, uint32_t num, const double *d_sigma, double corner_thresh,
                     float *d_R, uint32_t *d_keep, double *d_conf, void *d_scratch, void *d_tabs, uint32_t *d_fail,
                     s3d_stream stream);
/* The two halves of s3d_k_orient_tab for callers that overlap them with other work: the tables depend on the pyramid's geometry
 * (dims, units) and the levels' sigmas only, not on the voxels, so SIFT3D_detect_keypoints builds them on its extrema stream
 * while the pyramid is being filtered (a wave per level for ~0.2 ms: off the critical path), and the window sums then run with
 * tables that are already there.  The build must be complete, or ordered before `stream`, when s3d_k_orient_tab_built runs. */
int s3d_k_orient_tab_build(const s3d_pyramid_desc *pyr, const double *d_sigma, void *d_tabs, s3d_stream stream);
int s3d_k_orient_tab_built(const s3d_pyramid_desc *pyr, const uint32_t *d_idx, const uint32_t *d_tag,
                           const float *d_center, uint32_t num, const double *d_sigma, double corner_thresh,
                           float *d_R, uint32_t *d_keep, double *d_conf, void *d_scratch, void *d_tabs, uint32_t *d_fail,
                           s3d_stream stream);
/* Test / profiling knob of the calling thread: how s3d_k_orient_tab uses the tables -- 0 not at all, 1 one kernel that
 * replays or enumerates per candidate, 2 a table-walk kernel plus the general kernel for the candidates it flags; anything
 * else restores the default (S3D_ORI_MODE, else 0: measured at 512^3, the tables do not pay -- profiles/r03_orient_experiments.txt). */
void s3d_k_set_orient_mode(int mode);
int s3d_k_orient_mode(void);                 /* what the calling thread's next s3d_k_orient_tab will do */
/* Candidates are processed in chunks of S3D_ORIENT_CHUNK; the scratch holds one chunk's window sums. */
#define S3D_ORIENT_CHUNK (1u << 20)
#define S3D_ORIENT_SCRATCH_BYTES 128u
size_t s3d_k_orient_scratch_bytes(uint32_t num);
/* Test knob of the calling thread: candidates per chunk (0 or > S3D_ORIENT_CHUNK restores the default; the scratch
 * size is unaffected). */
void s3d_k_set_orient_chunk(uint32_t n);
/* Stable compaction of kept candidates: for i with keep[i], writes x,y,z,o,s (int32 x5) and R.
 * *d_num_out receives the number kept.  d_scratch: >= num/256 + 2 uint32. */
int s3d_k_compact_keys(const s3d_pyramid_desc *pyr, const uint32_t *d_idx, const uint32_t *d_tag,
                       const float *d_R, const uint32_t *d_keep, uint32_t num, int32_t *d_xyzos,
                       float *d_R_out, uint32_t *d_num_out, uint32_t *d_scratch, s3d_stream stream);
/* Keypoint budget (extension, sift3d_amd_set_max_keypoints).  d_strength[i] = |D| of candidate i's own voxel, D the DoG voxel
 * as the reference stores it (build_dog, sift.c:1052-1071: one f32 subtraction of GSS levels s + 1 and s), i.e.
 * |d_level[o*L + k + 1][idx] - d_level[o*L + k][idx]| with tag = o<<8 | k, k = s - first_level as for s3d_k_orient: the voxel
 * sift3d_amd_download_pyramid(.., 1) returns, never stored on the device.  d_keep (may be NULL: every candidate): entries with
 * d_keep[i] == 0 are not written.  The caller vouches for idx < the level's voxels and k + 1 < num_levels. */
int s3d_k_key_strength(const s3d_pyramid_desc *pyr, const uint32_t *d_idx, const uint32_t *d_tag, const uint32_t *d_keep,
                       uint32_t num, float *d_strength, s3d_stream stream);
/* Clears d_keep[i] of every kept entry (d_keep[i] != 0) that is not among the `budget` (> 0) kept entries of largest
 * d_strength; equal strengths go to the lower i.  Exact and deterministic: a radix select over the bit patterns of the
 * non-negative strengths (the sign bit is ignored; no NaNs) with integer atomics only, then an ordered count over the entries
 * equal to the threshold.  No more kept entries than `budget`: d_keep is left untouched -- decided on the device, the host
 * need not know the number (budget >= num returns without a launch).  Entries with d_keep[i] == 0 are never read.  Eight
 * launches ordered by the stream, none waits for another workgroup.  d_scratch: s3d_k_select_scratch_bytes(num) bytes,
 * owned by the call until it has run. */
size_t s3d_k_select_scratch_bytes(uint32_t num);
int s3d_k_select_strongest(const float *d_strength, uint32_t *d_keep, uint32_t num, uint32_t budget, void *d_scratch,
                           s3d_stream stream);
/* Sub-voxel refinement (extension, sift3d_amd_set_subvoxel): offsets of the records d_xyzos[5i ..] = x, y, z, o, s (the layout
 * s3d_k_compact_keys writes; s a pyramid level index, first_level included) from a quadratic fit to the DoG around each, D
 * being the signed voxel s3d_k_key_strength takes the magnitude of, widened to f64:
 *   g_a = (D(a+1) - D(a-1)) / 2,  H_aa = D(a+1) + D(a-1) - 2 D0,  H_ab = (D(a+1,b+1) - D(a+1,b-1) - D(a-1,b+1) + D(a-1,b-1)) / 4
 * for a, b in x, y, z within DoG level s, and g_s, H_ss alike over the centre voxel of DoG levels s - 1, s + 1 (no space-scale
 * cross terms).  Space: the solution of H3 d = -g3 if H3 or -H3 is positive definite (Sylvester) and every |d_a| <= 0.5 (flag
 * bit 0); otherwise d_a = -g_a / H_aa per axis, clipped to [-0.5, 0.5], 0 where H_aa == 0 or the quotient is not finite (flag
 * bit 1).  Scale: d_s = -g_s / H_ss under the same clip and zero rule.  d_off[4i ..] = d_x, d_y, d_z (octave voxels), d_s (levels).
 * The number of records is read on the device: *d_num, at most max_num (the grid's bound), so a caller that has just compacted
 * need not fetch the count first.  d_counters[0], [1]: how many records took the 3-D fit / the fallback; zeroed by the call.
 * A record that cannot be refined -- a voxel outside 1 .. n - 2 of its octave, or a level without both DoG neighbours -- gets
 * zero offsets and flag bit 2 and counts in neither; nothing is read for it.  One thread per record, all arithmetic f64. */
int s3d_k_refine_keys(const s3d_pyramid_desc *pyr, const int32_t *d_xyzos, const uint32_t *d_num, uint32_t max_num,
                      double *d_off, uint32_t *d_flags, uint32_t *d_counters, s3d_stream stream);

/* One record per keypoint for the descriptor kernel; the scalar set-up mirrors
 * extract_descrip (sift.c:1845-1851) and is done on the host in the same float arithmetic. */
typedef struct {
    float cx, cy, cz;        /* (float) key->xd, yd, zd */
    float sigma;             /* (float)(sd * desc_sig_fctr) */
    float rad;               /* (float)(desc_rad_fctr * sigma) */
    float half;              /* (float)(rad / sqrt(2)) */
    float binf;              /* 1.0f / ((2.0f*half) / NHIST_PER_DIM) */
    int level;               /* index into s3d_pyramid_desc.d_level */
    int octave;
    float R[9];              /* key->R, row-major */
} s3d_desc_key;

/* extract_descrip (sift.c:1834-1928) incl. SIFT3D_desc_acc_interp (sift.c:1687-1791),
 * icos_hist_bin/cart2bary (sift.c:1646-1683, 335-394) and both normalisations (sift.c:1794-1821).
 * d_mesh: table from s3d_mesh_table().  Descriptor i is written to d_out[i*out_stride .. +768),
 * order 12*(cx+4cy+16cz)+vertex (out_stride = 776 lays records out like SIFT3D_Descriptor).
 * The level buffers in pyr must be readable for 16 bytes past their last voxel (wide gathers;
 * s3d_rt_malloc adds the slack itself).
 * d_work: one uint32 of device memory owned by the caller, not shared with a launch on another stream: the kernel runs
 * one persistent workgroup per CU and the workgroups draw their keypoints from this counter (zeroed by the call, in
 * stream order). */
int s3d_k_describe(const s3d_pyramid_desc *pyr, const s3d_desc_key *d_keys, uint32_t num,
                   const float *d_mesh, float *d_out, size_t out_stride /* floats, >= 768 */,
                   uint32_t *d_work, s3d_stream stream);

/* The descriptor kernel sets the grid of a keypoint's fixed-point histogram from a sampled estimate of the window's
 * gradient mass and proves afterwards that no 32-bit field wrapped; a keypoint whose proof fails is described again
 * with the grid of its measured mass.  *described / *redone: how many windows the current device has described / has
 * described twice since the counters were last reset (reset != 0 clears them). */
int s3d_k_describe_redo_stats(unsigned long long *described, unsigned long long *redone, int reset);

/* Test aids of the descriptor kernel's back end (S3D_TESTING builds only).  A window voxel's 24 histogram contributions are
 * f32 products while its scaled magnitude stays below 2^24 grid units and f64 fused multiply-adds otherwise; both give
 * the same integers.  s3d_k_set_describe_f32_limit multiplies that limit by s in [0, 1] (0: every voxel takes the f64
 * form); s3d_k_describe_path_stats reports how many voxels took each form since the last reset.  In the product library
 * both fail: its kernel has neither the hook nor the counters. */
int s3d_k_set_describe_f32_limit(float s);
int s3d_k_describe_path_stats(unsigned long long *fast_vox, unsigned long long *slow_vox, int reset);

/* Test / diagnostics aid: d_stats[2i] = number of voxels the descriptor window of keypoint i accepts, d_stats[2i+1] = a
 * checksum of their coordinates, produced by the descriptor kernel's own window enumeration. */
int s3d_k_describe_window_stats(const s3d_pyramid_desc *pyr, const s3d_desc_key *d_keys, uint32_t num,
                                uint32_t *d_stats, uint32_t *d_work, s3d_stream stream);

/* Self-test: d_out[i] = the kernels' window-weight exponential of d_in[i] (a restatement of glibc 2.35 expf,
 * which the reference reaches through expf() at sift.c:1401, 1890, 2333); |d_in[i]| < 80. */
int s3d_k_expf_selftest(const float *d_in, float *d_out, uint32_t n, s3d_stream stream);

/* Icosahedron table for the kernels (host computation in f32, mirrors init_geometry sift.c:215-326
 * incl. the v[0]<->v[1] swap quirk).  Layout per face (16 floats): e1[3] e2[3] t[3] q[3] e2q
 * idx0 idx1 idx2 (indices stored as float bit patterns of ints), followed by a 32-entry face lookup
 * (int bit patterns; key = sign bits of x,y,z | type<<3, see s3d_icos_bin_fast).  out: 20*16+32 floats. */
#define S3D_MESH_FLOATS (S3D_NFACES * 16 + 32)
void s3d_mesh_table(float *out);

/* ---- dense descriptors (SIFT3D_extract_dense_descriptors sift.c:2354-2496) ----------------------- */
/* Gradient -> icosahedron barycentric weights into a zeroed 12-channel image (sift.c:2460-2480). */
int s3d_k_dense_bary(const float *d_smooth, int nx, int ny, int nz, const float unitsf[3],
                     const float *d_mesh, float *d_out12, s3d_stream stream);
/* s3d_k_dense_bary followed by the 12-channel s3d_k_sep_fir, fused for unit tap spacing (the barycentric
 * image stays in LDS).  d_dst, d_tmp: nx*ny*nz*12 floats.  Returns 1 without doing anything when the
 * configuration is not eligible (run the two separate calls instead), 0 on success, -1 on error. */
int s3d_k_dense_bary_blur(const float *d_smooth, float *d_dst, float *d_tmp, int nx, int ny, int nz,
                          const float unitsf[3], const float uf[3], const float *d_mesh, const float *taps,
                          int width, const float *d_post_in, s3d_stream stream);
/* profiling runs: the marching passes of the above in `nchunks` chunks (0: the built-in choice); per calling thread */
void s3d_k_dense_set_chunks(int nchunks);
/* dense_rotate = 1 (sift.c:2521-2588, 2295-2343): per-voxel sphere histogram of gradients rotated by the
 * voxel's own orientation.  d_R / d_keep: output of s3d_k_orient run with one candidate per voxel
 * (d_idx = d_tag = d_center = NULL); rejected voxels use the identity.  sigma = sigma0*7.0711/4. */
int s3d_k_dense_rot_hist(const float *d_smooth, int nx, int ny, int nz, const float unitsf[3], double sigma,
                         const float *d_R, const uint32_t *d_keep, const float *d_mesh, float *d_out12,
                         s3d_stream stream);
/* postproc_Hist per voxel (sift.c:2267-2292, 2396-2412): normalise, clamp, normalise, times in(x,y,z) */
int s3d_k_dense_post(float *d_desc12, const float *d_in, size_t nvox, s3d_stream stream);

/* ---- inverse affine warp (s3d_resample.hip; im_inv_transform, imutil.c:2040-2175) --------------------- */
/* d_dst(x,y,z,c) = sample of d_src at A [x y z 1]^T; A: 3 x 4 row-major doubles; interp 0 = tri-linear
 * (bit-identical to the reference), 1 = Lanczos-2; zero outside the source. */
int s3d_k_inv_affine(const float *d_src, int snx, int sny, int snz, int nc, float *d_dst, int dnx, int dny, int dnz,
                     const double A[12], int interp, s3d_stream stream);

/* ---- inverse thin-plate-spline warp (s3d_resample.hip; im_inv_transform through apply_Tps_xyz, imutil.c:2676-2729) --------
 * d_dst(x,y,z,c) = sample of d_src at f(x,y,z) = sum_n U(r2_n) w_n + a_0 + a_x x + a_y y + a_z z in f64, U(r2) = r2 log r2 and
 * U(0) = 0, r2_n the squared distance to control point n.  d_ctrl: n_ctrl x 3 row major; d_params: 3 x (n_ctrl + 4) row major
 * (row r: the n_ctrl weights of output coordinate r, its constant, its x, y, z coefficients).  Control points are summed in
 * ascending order, then the constant, then the x, y, z terms, each its own separately rounded multiplication and addition, so
 * n_ctrl = 0 (d_ctrl may be NULL) is bit-identical to the reference; the kernel sum uses fused multiply-adds and the device's
 * log.  Sampling, the zero outside the source and the NaN rule are s3d_k_inv_affine's.  Any n_ctrl: the control points are
 * streamed through LDS S3D_TPS_TILE at a time. */
#define S3D_TPS_TILE 128                 /* control points per LDS tile */
int s3d_k_inv_tps(const float *d_src, int snx, int sny, int snz, int nc, float *d_dst, int dnx, int dny, int dnz,
                  const double *d_ctrl, const double *d_params, uint32_t n_ctrl, int interp, s3d_stream stream);

/* ---- RANSAC consensus counts (s3d_resample.hip; the scoring loop of find_tform_ransac, imutil.c:4527-4552, 4802-4815) ----
 * counts[m] = #{ i < npts : !(e(i,m) > thr2) },  e = |src_i - M_m [ref_i 1]^T|^2 in f64 with the host loop's operation order
 * (x' = A0*x + A1*y + A2*z + A3 left to right, no contraction), so a NaN e counts and e == thr2 counts.  d_src, d_ref: npts x 3
 * row major; d_models: nmodels x 12 (3 x 4 row major); d_counts: nmodels ints, zeroed by the call.  Integer atomics only: the
 * counts do not depend on the schedule.  npts, nmodels >= 1; nmodels <= 65535 * S3D_RANSAC_TILE (the grid's y extent). */
#define S3D_RANSAC_TILE 64               /* models a workgroup of 256 matches walks */
int s3d_k_ransac_count(const double *d_src, const double *d_ref, uint32_t npts, const double *d_models, uint32_t nmodels,
                       double thr2, int *d_counts, s3d_stream stream);

/* ---- similarity of a source under a transform against a reference (s3d_resample.hip; extension, sift3d_amd_im_similarity) ----
 * One pass over the reference volume d_ref (rnx x rny x rnz, one channel): voxel (x, y, z) goes through the transform exactly
 * as in s3d_k_inv_affine / s3d_k_inv_tps (the kernels share the coordinate and sampling functions), the one-channel source
 * d_src is sampled there, and the pair (a, b) = (reference voxel, the float the warp would have stored) is accumulated instead
 * of stored.  A voxel counts iff the warp would sample it (no coordinate outside [0, n - 1], none NaN) and a and b are finite.
 *   d_hist[ia * bins + ib] (u64, bins^2, zeroed by the call): ia = bin of a, t = ((double)a - ref_lo) * ref_scale in f64,
 *       ia = t < 0 ? 0 : t >= bins ? bins - 1 : (int)t; ib likewise from b, src_lo, src_scale.  Integer atomics: exact.
 *   d_sums[0 .. 7): sum a', sum b', sum a'^2, sum b'^2, sum a'b', sum (a - b)^2, sum |a - b| in f64, a' = a - c_ref,
 *       b' = b - c_src.  No floating-point atomics: per-workgroup partials in d_scratch, added by a second launch in a fixed
 *       order; which voxels a thread sums depends on the dimensions and bins only, so a call's bits repeat.
 * bins in 2 .. S3D_SIM_MAX_BINS; interp as for the warps.  d_scratch: s3d_k_similarity_scratch_bytes(..) bytes (0: bad
 * arguments), owned by the call until it has run.  Fails with a message for volumes whose rows (rny * rnz) exceed 2^31 - 1 or
 * whose share per workgroup would overflow a 32-bit counter. */
#define S3D_SIM_MAX_BINS 128
size_t s3d_k_similarity_scratch_bytes(int rnx, int rny, int rnz, int bins);
int s3d_k_similarity_affine(const float *d_src, int snx, int sny, int snz, const float *d_ref, int rnx, int rny, int rnz,
                            const double A[12], int interp, int bins, double ref_lo, double ref_scale, double src_lo,
                            double src_scale, double c_ref, double c_src, unsigned long long *d_hist, double *d_sums,
                            void *d_scratch, s3d_stream stream);
int s3d_k_similarity_tps(const float *d_src, int snx, int sny, int snz, const float *d_ref, int rnx, int rny, int rnz,
                         const double *d_ctrl, const double *d_params, uint32_t n_ctrl, int interp, int bins, double ref_lo,
                         double ref_scale, double src_lo, double src_scale, double c_ref, double c_src,
                         unsigned long long *d_hist, double *d_sums, void *d_scratch, s3d_stream stream);
/* Profiling knob of the calling thread: 1 -- lanes of a wave that share the first counted lane's histogram counter add their
 * number with one LDS atomic (volumes whose voxels crowd into one background bin); 0 -- every lane its own atomic; < 0 -- the
 * default (0: profiles/similarity_cost.txt).  The histogram and the sums are the same either way. */
void s3d_k_similarity_set_aggregate(int on);
int s3d_k_similarity_get_aggregate(void);
/* d_minmax[0], [1] = the minimum and maximum over the finite elements of d_v[0 .. n); both NaN when none is finite.
 * Integer maxima over an order-preserving encoding: the result does not depend on the schedule. */
int s3d_k_minmax_finite(const float *d_v, size_t n, float *d_minmax, s3d_stream stream);

/* ---- normal equations of an intensity-based affine fit (s3d_resample.hip; extension, sift3d_amd_refine_affine) --------------
 * One pass over the reference volume d_ref (rnx x rny x rnz) against the source d_src (snx x sny x snz), both one channel with
 * default strides: the sums of one Gauss-Newton step on the 12 entries of the affine map A (3 x 4 row major, reference voxel ->
 * source voxel coordinates), for the residual r = sb (b - mb) - sa (a - ma).  Raw SSD is (sa, ma, sb, mb) = (1, 0, 1, 0).
 * For every reference voxel (x, y, z), all in f64, every operation rounded on its own (no contraction), left to right:
 *   (tx, ty, tz) = A [x y z 1]^T as s3d_k_inv_affine computes it;   q = (qx, qy, qz, 1) = (x - c[0], y - c[1], z - c[2], 1);
 *   a = d_ref(x, y, z);   b = the float s3d_k_inv_affine (tri-linear) would store for this voxel;
 *   X0 = min(floor(tx), snx - 2), fx = tx - X0, ux = 1 - fx, likewise Y0, fy, uy, Z0, fz, uz;  cijk = d_src(X0 + i, Y0 + j, Z0 + k);
 *   gx = sb * (((c100 - c000) * uy + (c110 - c010) * fy) * uz + ((c101 - c001) * uy + (c111 - c011) * fy) * fz)
 *   gy = sb * (((c010 - c000) * ux + (c110 - c100) * fx) * uz + ((c011 - c001) * ux + (c111 - c101) * fx) * fz)
 *   gz = sb * (((c001 - c000) * ux + (c101 - c100) * fx) * uy + ((c011 - c010) * ux + (c111 - c110) * fx) * fy)
 *       -- the gradient of the tri-linear interpolant on the cell [X0, X0 + 1] x .., one-sided on a lattice point and on the
 *       last plane of an axis;
 *   r = sb * ((double)b - mb) - sa * ((double)a - ma).
 * The voxel counts iff s3d_k_inv_affine would sample it (no coordinate outside [0, n - 1], none NaN), a and b are finite floats
 * and gx, gy, gz are finite.  d_sums, S3D_NEQ_SUMS = 74 doubles, over the counted voxels:
 *   [P * 10 + Q], P < 6, Q < 10:  sum (g_i * g_j) * (q_k * q_l),  P the pair (i, j) of xx, xy, xz, yy, yz, zz and Q the pair
 *       (k, l) of 00, 01, 02, 03, 11, 12, 13, 22, 23, 33 (q_3 = 1, so (q_k * q_3) is q_k and (q_3 * q_3) is 1).  The Jacobian row
 *       of r in the entry (i, k) of [D | d] -- the step in centred coordinates, A <- A + D, t <- t + d - D c -- is g_i q_k, so
 *       H[(i, k), (j, l)] = d_sums[P(i, j) * 10 + Q(k, l)];
 *   [60 + i * 4 + k]:  sum (r * g_i) * q_k, the gradient's entry (i, k);      [72]: sum r * r;      [73]: n, the count.
 * No floating-point atomics: per-workgroup partials in d_scratch, added by a second launch in a fixed order; which voxels a
 * thread sums depends on the dimensions only, so a call's bits repeat on the same device and build.  n is exact.  d_scratch:
 * s3d_k_affine_normal_eq_scratch_bytes(..) bytes (0: bad dimensions), owned by the call until it has run.  Fails with a message,
 * the outputs untouched, for a dimension < 1, a source dimension < 2 (no gradient: H would be singular), more than 2^31 - 1 rows
 * (rny * rnz) and NULL pointers. */
#define S3D_NEQ_SUMS 74
size_t s3d_k_affine_normal_eq_scratch_bytes(int rnx, int rny, int rnz);
int s3d_k_affine_normal_eq(const float *d_src, int snx, int sny, int snz, const float *d_ref, int rnx, int rny, int rnz,
                           const double A[12], const double c[3], double sa, double ma, double sb, double mb, double *d_sums,
                           void *d_scratch, s3d_stream stream);

/* ---- deformable registration (s3d_resample.hip; extension, sift3d_amd_register_demons) --------------------------------------
 * A displacement field over a reference volume of N = rnx * rny * rnz voxels is PLANAR: component c (0 = x, 1 = y, 2 = z, in
 * source voxels) of reference voxel i = (z * rny + y) * rnx + x is d_u[c * N + i], 3 N floats.  (A wave then reads and writes 256
 * contiguous bytes per component, and a component is a one-channel volume to s3d_k_sep_fir's fused path.)
 *
 * s3d_k_demons_step: one update of Thirion's demons with the gradient of the moving (source) image.  For every reference voxel
 * (x, y, z), all in f64, every operation rounded on its own (no contraction), left to right:
 *   (tx, ty, tz) = (A [x y z 1]^T as s3d_k_inv_affine computes it) + ((double)u_x, (double)u_y, (double)u_z);
 *   a, b, X0, Y0, Z0, gx, gy, gz (scaled by sb) and r = sb (b - mb) - sa (a - ma) at (tx, ty, tz) exactly as
 *       s3d_k_affine_normal_eq defines them, and the voxel counts under its rule (the sample inside, a and b finite floats,
 *       the gradient finite);
 *   D = ((gx * gx + gy * gy) + gz * gz) + kstep * (r * r);
 *   if the voxel counts, D > 0 and D is finite:  m = (-r) / D,  d_c = m * g_c,  v_c = (float)((double)u_c + d_c);
 *   otherwise v_c = u_c, its bits copied, and d_c = 0.
 * |d| = |r| |g| / (|g|^2 + kstep r^2) <= 1 / (2 sqrt(kstep)) (the arithmetic-geometric mean inequality on the denominator), so
 * kstep = 1 / (4 max_step^2) bounds an update's length by max_step source voxels.
 *   d_sums[0] = sum r * r,  [1] = n (a sum of 1.0: exact),  [2] = sum ((d_x * d_x + d_y * d_y) + d_z * d_z), over the counted voxels.
 * No floating-point atomics: per-workgroup partials in d_scratch, added by a second launch in a fixed order; the grid depends on
 * the dimensions only, so a call's bits repeat.  d_v may be d_u (a voxel reads only its own entry).  d_scratch:
 * s3d_k_demons_step_scratch_bytes(..) bytes (0: bad dimensions).  Fails with a message, the outputs untouched, for a dimension
 * < 1, a source dimension < 2, more than 2^31 - 1 rows (rny * rnz) and NULL pointers. */
size_t s3d_k_demons_step_scratch_bytes(int rnx, int rny, int rnz);
int s3d_k_demons_step(const float *d_src, int snx, int sny, int snz, const float *d_ref, int rnx, int rny, int rnz,
                      const double A[12], const float *d_u, float *d_v, double sa, double ma, double sb, double mb, double kstep,
                      double *d_sums, void *d_scratch, s3d_stream stream);
/* d_dst(x, y, z, .) = the s3d_k_inv_affine sample of d_src at A [x y z 1]^T + u(x, y, z), d_u a planar field over the dnx x dny x
 * dnz output grid: zero outside the source, the NaN rule, both interpolations and any nc as there; bit-identical to
 * s3d_k_inv_affine where u is zero. */
int s3d_k_inv_field(const float *d_src, int snx, int sny, int snz, int nc, float *d_dst, int dnx, int dny, int dnz,
                    const double A[12], const float *d_u, int interp, s3d_stream stream);
/* A planar field one pyramid level up.  Requires c?? = f?? / 2 (integer division), each >= 1.  Every component of fine voxel
 * (x, y, z) is (float)(2.0 * (double)b), b the float the tri-linear s3d_k_inv_affine sample stores for the coarse component at
 * (min(x / 2.0, cnx - 1), min(y / 2.0, cny - 1), min(z / 2.0, cnz - 1)): a displacement in coarse voxels is twice as long in fine
 * voxels. */
int s3d_k_field_upsample2(const float *d_coarse, int cnx, int cny, int cnz, float *d_fine, int fnx, int fny, int fnz,
                          s3d_stream stream);
/* The lengths of a planar field's entries, m = sqrt((u_x * u_x + u_y * u_y) + u_z * u_z) in f64, entries whose m is not finite
 * left out: d_partials, S3D_FIELD_NORM_SLOTS x 3 doubles, receives per slot (sum m, the count, max m) of the voxels the slot's
 * workgroup walked (zeros in the slots not used); the caller adds them in slot order.  Which voxels a slot holds depends on nvox
 * only, so a call's bits repeat. */
#define S3D_FIELD_NORM_SLOTS 1024
int s3d_k_field_norm_slots(void);        /* S3D_FIELD_NORM_SLOTS, for callers that do not read this header */
int s3d_k_field_norm(const float *d_u, size_t nvox, double *d_partials, s3d_stream stream);

/* ---- the inverse of a field's map and its Jacobian determinant (s3d_resample.hip; sift3d_amd_invert_field, .._field_jacobian) --
 * The map of a field u over the reference grid is phi(x) = A [x 1]^T + u(x), reference voxel to source voxel coordinates.
 *
 * s3d_k_field_invert: the field w over the source grid snx x sny x snz (planar, 3 * snx * sny * snz floats at d_w) with
 * phi(B [y 1]^T + w(y)) = y, B the inverse of A as the caller computed it, so that (B, w) is itself a map of the kind above,
 * source voxel to reference voxel.  Per source voxel y = (x, y, z), all in f64, every operation rounded on its own, left to right:
 *   1. p0 = B [y 1]^T as s3d_k_inv_affine computes it;  w = (+0, +0, +0);  k = 0.
 *   2. p = p0 + w.  A component of p that is not finite: the voxel is INVALID.
 *   3. q_a = p_a < 0 ? 0 : p_a > rn_a - 1 ? rn_a - 1 : p_a: the field is continued constantly past its faces.
 *   4. s_c = the tri-linear s3d_k_inv_affine sample of component c of u at q, as the f64 it is before that kernel rounds it to
 *      float.  An s_c that is not finite: INVALID.
 *   5. r_i = ((A[4i] * w_x + A[4i+1] * w_y) + A[4i+2] * w_z) + s_i, which is phi(B y + w) - y in source voxels, and
 *      e2 = (r_x * r_x + r_y * r_y) + r_z * r_z.  If e2 <= tol * tol (the product rounded once): CONVERGED, w stays.
 *      Otherwise, if k == max_iter: NOT CONVERGED, w stays.
 *      Otherwise w_i = -((B[4i] * s_x + B[4i+1] * s_y) + B[4i+2] * s_z), k = k + 1, and again from step 2.
 *   6. d_w receives (float)w_c; an INVALID voxel the three words 0x7FC00000.
 *   7. d_status (one byte per source voxel, may be NULL) receives 0: converged and the final p == q, inside the reference grid on
 *      every axis; 1: converged on the continued field; 2: not converged; 3: invalid.
 * (The update is the fixed-point form of w = -B u(B y + w); it contracts where |B grad u| < 1, which is also where phi does not
 * fold.)  u is only read, so a voxel's iteration depends on no other voxel and one launch runs all of them to their end.
 * d_partials, S3D_FIELD_INV_SLOTS x S3D_FIELD_INV_STATS doubles, cleared by the call, receives per slot: [0 .. 3] the number of
 * voxels of status 0 .. 3 and [4] the sum of k over all of its voxels (sums of integers in f64: exact), [5] the sum and [6] the
 * maximum of sqrt(e2) over its voxels of status 0, 1 and 2 (a NaN never becomes the maximum).  The caller adds the slots in slot
 * order.  Which voxels a slot holds depends on the source dimensions only, and there are no floating-point atomics, so a call's
 * bits repeat.  A zero field gives all-zero bits and no update.  Fails with a message, the outputs untouched, for a dimension
 * < 1, NULL d_u, d_w, A, B or d_partials, max_iter < 0, tol negative or NaN, and sny or snz above 65535 (s3d_k_inv_affine's limit). */
#define S3D_FIELD_INV_SLOTS 2048
#define S3D_FIELD_INV_STATS 7
int s3d_k_field_invert_slots(void);      /* the two constants, for callers that do not read this header */
int s3d_k_field_invert_stats(void);
int s3d_k_field_invert(const float *d_u, int rnx, int rny, int rnz, const double A[12], const double B[12], float *d_w, int snx,
                       int sny, int snz, int max_iter, double tol, unsigned char *d_status, double *d_partials, s3d_stream stream);
/* s3d_k_field_jacobian: det(d phi / d x) per reference voxel.  g_ia, the derivative of component i of u along axis a, is
 * ((double)u[+1] - (double)u[-1]) * 0.5 away from the faces, (double)u[1] - (double)u[0] at index 0 and (double)u[n-1] -
 * (double)u[n-2] at index n - 1 of that axis;  J_ia = A[4i+a] + g_ia;
 *   det = (J00 * (J11 * J22 - J12 * J21) - J01 * (J10 * J22 - J12 * J20)) + J02 * (J10 * J21 - J11 * J20),
 * every operation a rounded f64 operation, stored as (float)det at d_det (rnx * rny * rnz floats; NULL: statistics only).  The
 * determinant is in voxel coordinates: the ratio of physical volumes is det times the ratio of the source's voxel volume to the
 * reference's, a positive factor, so the sign -- det <= 0: the map folds there -- is that of the physical map.
 * d_partials, S3D_FIELD_JAC_SLOTS x S3D_FIELD_JAC_STATS doubles, cleared by the call, receives per slot over the finite det of
 * its voxels: [0] their sum, [1] their number, [2] the number of those <= 0, [3] their minimum and [4] their maximum ([3] and [4]
 * mean something only in a slot whose [1] > 0).  A det that is not finite is stored as computed and left out of all five.  The
 * caller adds the slots in slot order; the bits repeat as above.  Fails with a message, the outputs untouched, for a dimension
 * < 2, NULL d_u, A or d_partials, and rny or rnz above 65535. */
#define S3D_FIELD_JAC_SLOTS 2048
#define S3D_FIELD_JAC_STATS 5
int s3d_k_field_jacobian_slots(void);
int s3d_k_field_jacobian_stats(void);
int s3d_k_field_jacobian(const float *d_u, int rnx, int rny, int rnz, const double A[12], float *d_det, double *d_partials,
                         s3d_stream stream);

/* ---- matcher (s3d_match.hip; replaces match_desc, sift.c:2892-2969) ------------------------------- */
/* For each of the `na` query rows (row r = d_a + (d_a_sel ? d_a_sel[r] : r) * a_stride, 768 floats) the
 * smallest and second-smallest f64 sum of squared differences over the nb rows of d_b and the index of
 * the smallest (lowest index on ties).  Strides in floats, multiples of 4; rows 16-byte aligned. */
int s3d_k_nn_best2(const float *d_a, size_t a_stride, const int *d_a_sel, uint32_t na, const float *d_b,
                   size_t b_stride, uint32_t nb, double *d_best, double *d_second, int *d_idx,
                   s3d_stream stream);
/* Same outputs (bit for bit) through an f32 screening pass + exact verification of the few columns that can be
 * the nearest or second-nearest neighbour (see s3d_match.hip).  Returns 1 when it declines (a row with more than
 * 64 candidates, nb < 2): run s3d_k_nn_best2 instead. */
int s3d_k_nn_best2_fast(const float *d_a, size_t a_stride, const int *d_a_sel, uint32_t na, const float *d_b,
                        size_t b_stride, uint32_t nb, double *d_best, double *d_second, int *d_idx,
                        s3d_stream stream);
/* Both directions of SIFT3D_nn_match from one f32 score matrix: best / second / index of every row of A over B
 * (d_f*) and of every row of B over A (d_b*), bit-identical to s3d_k_nn_best2 run each way.  Declines (returns 1)
 * when the padded na x nb score matrix would exceed 8 GiB, a side has fewer than two rows, or a row/column has
 * more than 64 candidates. */
int s3d_k_nn_match2_fast(const float *d_a, size_t a_stride, uint32_t na, const float *d_b, size_t b_stride, uint32_t nb,
                         double *d_fbest, double *d_fsecond, int *d_fidx, double *d_bbest, double *d_bsecond, int *d_bidx,
                         s3d_stream stream);
/* The screened matcher keeps its scratch (operand copies, score matrix, partial minima, candidate lists: about
 * 4.3 B per pair) per device between calls; this gives it back. */
void s3d_k_nn_release_scratch(void);

#ifdef __cplusplus
}
#endif
#endif
