/* sift3d_amd.h -- C ABI of libsift3d_amd.so, the MI355X-native drop-in for the hot path of
 * bbrister/SIFT3D v1.4.6 (libsift3D + the part of libimutil it stands on).
 *
 * The structs below are byte-for-byte layout compatible with the reference's imutil/imtypes.h
 * (x86-64 SysV; sizes/offsets are _Static_assert'ed at the bottom), because the reference's callers
 * allocate them on their own stack and read their fields directly.  The field names are therefore
 * the reference's; everything else in this header is written for this repo.  A program built
 * against the reference's headers can be relinked against libsift3d_amd.so unchanged for the
 * entry points listed here; see INTEGRATION.md.
 *
 * Device state:  the reference has no opaque pointer in any struct; its only extension slots are
 * the dummy OpenCL fields (int sized when OpenCL is compiled out, imtypes.h:49-68).  This library
 * stores a small integer HANDLE into a process-global registry of device contexts in
 * SIFT3D.kernels.downsample_2 (0 = none) -- never a pointer.  The Gaussian scale-space pyramid of the
 * last SIFT3D_detect_keypoints stays resident in HBM for SIFT3D_extract_descriptors; the host-side
 * `Pyramid` carries valid metadata (dims, units, scales) and level `data` pointers are NULL until
 * sift3d_amd_download_pyramid() is called.
 *
 * Every function returns SIFT3D_SUCCESS (0) or SIFT3D_FAILURE (-1) like the reference and reports
 * through stderr.  There is no CPU fallback: without a usable gfx950 device the compute entry
 * points fail.
 */
#ifndef SIFT3D_AMD_H
#define SIFT3D_AMD_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SIFT3D_SUCCESS 0
#define SIFT3D_FAILURE (-1)
#define SIFT3D_TRUE 1
#define SIFT3D_FALSE 0

#define IM_NDIMS 3
#define NHIST_PER_DIM 4
#define ICOS_NFACES 20
#define ICOS_NVERT 12
#define HIST_NUMEL ICOS_NVERT
#define DESC_NUM_TOTAL_HIST (NHIST_PER_DIM * NHIST_PER_DIM * NHIST_PER_DIM)
#define DESC_NUMEL (DESC_NUM_TOTAL_HIST * HIST_NUMEL)

/* Return codes of im_read / im_write (imutil.h:20-31) and parse_gnu (imtypes.h:23-24) */
#define SIFT3D_FILE_DOES_NOT_EXIST 1
#define SIFT3D_UNSUPPORTED_FILE_TYPE 2
#define SIFT3D_WRAPPER_NOT_COMPILED 3
#define SIFT3D_HELP 1
#define SIFT3D_VERSION 2

/* Image file formats (imtypes.h:101-108) */
typedef enum _im_format { ANALYZE, DICOM, DIRECTORY, NIFTI, UNKNOWN, FILE_ERROR } im_format;

typedef enum _Mat_rm_type { SIFT3D_DOUBLE, SIFT3D_FLOAT, SIFT3D_INT } Mat_rm_type;

/* Row-major dense matrix (imtypes.h:136-149). Only the 3x3 float `Keypoint.R` is used here. */
typedef struct _Mat_rm {
    union {
        double *data_double;
        float *data_float;
        int *data_int;
    } u;
    size_t size;
    int num_cols;
    int num_rows;
    int static_mem;
    Mat_rm_type type;
} Mat_rm;

/* Dense volume, x fastest, channels interleaved (imtypes.h:156-168).  Element (x,y,z,c) lives at
 * data[x*xs + y*ys + z*zs + c]; default strides xs = nc, ys = nc*nx, zs = nc*nx*ny. */
typedef struct _Image {
    float *data;
    int cl_image;     /* reference: dummy cl_mem.  Unused by this library. */
    double s;         /* scale-space location */
    size_t size;      /* number of floats */
    int nx, ny, nz;
    double ux, uy, uz;
    size_t xs, ys, zs;
    int nc;
    int cl_valid;     /* reference: dummy flag.  Unused by this library. */
} Image;

typedef struct _Sep_FIR_filter {
    int cl_apply_unrolled; /* reference: dummy cl_kernel */
    float *kernel;
    int dim;
    int width;
    int symmetric;
} Sep_FIR_filter;

typedef struct _Gauss_filter {
    double sigma;
    Sep_FIR_filter f;
} Gauss_filter;

typedef struct _GSS_filters {
    Gauss_filter first_gauss;
    Gauss_filter *gauss_octave;
    int num_filters;
    int first_level;
} GSS_filters;

typedef struct _SIFT_cl_kernels {
    int downsample_2; /* reference: dummy cl_kernel.  HERE: handle of the device context (0 = none). */
} SIFT_cl_kernels;

typedef struct _Pyramid {
    Image *levels;    /* [(o - first_octave) * num_levels + (s - first_level)] */
    double sigma_n;
    double sigma0;
    int num_kp_levels;
    int first_octave;
    int num_octaves;
    int first_level;
    int num_levels;
} Pyramid;

typedef struct _Cvec { float x, y, z; } Cvec;

typedef struct _Slab {
    void *buf;
    size_t num;
    size_t buf_size;
} Slab;

typedef struct _Keypoint {
    float r_data[IM_NDIMS * IM_NDIMS]; /* storage of R */
    Mat_rm R;                          /* 3x3 float rotation, R.u.data_float == r_data */
    double xd, yd, zd;                 /* integer voxel coordinates in octave o, stored as double */
    double sd;                         /* scale */
    int o, s;                          /* octave, level */
} Keypoint;

typedef struct _Keypoint_store {
    Keypoint *buf;
    Slab slab;
    int nx, ny, nz;
} Keypoint_store;

typedef struct _Hist { float bins[HIST_NUMEL]; } Hist;

typedef struct _Tri {
    Cvec v[3];
    int idx[3];
} Tri;

typedef struct _Mesh {
    Tri *tri;
    int num;
} Mesh;

typedef struct _SIFT3D_Descriptor {
    Hist hists[DESC_NUM_TOTAL_HIST]; /* element 12*(cx + 4*cy + 16*cz) + vertex */
    double xd, yd, zd, sd;
} SIFT3D_Descriptor;

typedef struct _SIFT3D_Descriptor_store {
    SIFT3D_Descriptor *buf;
    size_t num;
    int nx, ny, nz;
} SIFT3D_Descriptor_store;

typedef struct _SIFT3D {
    Mesh mesh;
    GSS_filters gss;
    SIFT_cl_kernels kernels;
    Pyramid gpyr;
    Pyramid dog;
    Image im;
    double peak_thresh;
    double corner_thresh;
    int dense_rotate;
} SIFT3D;

/* Indexing helpers (semantics of immacros.h:58-63, 157-159) */
#define SIFT3D_IM_GET_IDX(im, x, y, z, c) \
    ((size_t)(x) * (im)->xs + (size_t)(y) * (im)->ys + (size_t)(z) * (im)->zs + (size_t)(c))
#define SIFT3D_IM_GET_VOX(im, x, y, z, c) ((im)->data[SIFT3D_IM_GET_IDX((im), (x), (y), (z), (c))])
#define SIFT3D_PYR_IM_GET(pyr, o, s) \
    ((pyr)->levels + ((o) - (pyr)->first_octave) * (pyr)->num_levels + ((s) - (pyr)->first_level))

/* ======================= libimutil subset (replaces imutil/imutil.h entries) ======================= */
void init_im(Image *const im);                                          /* imutil.c:3634 */
int init_im_with_dims(Image *const im, const int nx, const int ny, const int nz, const int nc); /* imutil.c:1424 */
void im_free(Image *im);                                                /* imutil.c:1916 */
void im_default_stride(Image *const im);                                /* imutil.c:1453 */
int im_resize(Image *const im);                                         /* imutil.c:1527 */
int im_copy_dims(const Image *const src, Image *dst);                   /* imutil.c:1873 */
int im_copy_data(const Image *const src, Image *const dst);             /* imutil.c:1895 */
void im_zero(Image *im);                                                /* imutil.c:2020 */
void *SIFT3D_safe_realloc(void *ptr, size_t size);                      /* imutil.c:247 */

int init_Gauss_filter(Gauss_filter *const gauss, const double sigma, const int dim);   /* imutil.c:3657 */
int init_Gauss_incremental_filter(Gauss_filter *const gauss, const double s_cur,
                                  const double s_next, const int dim);                 /* imutil.c:3713 */
void cleanup_Gauss_filter(Gauss_filter *gauss);                                          /* imutil.c:3737 */
int init_Sep_FIR_filter(Sep_FIR_filter *const f, const int dim, const int width,
                        const float *const kernel, const int symmetric);               /* imutil.c:3552 */
void cleanup_Sep_FIR_filter(Sep_FIR_filter *const f);                                    /* imutil.c:3620 */
/* The north-star "im_Gauss_filter": x, y, z passes on the GPU.  Host images in, host image out. */
int apply_Sep_FIR_filter(const Image *const src, Image *const dst, Sep_FIR_filter *const f,
                         const double unit);                                             /* imutil.c:3459 */
/* The element-wise steps of the pyramid build as the reference exports them: host images in and out, the work on
 * the device (the kernels of rows a2, a7, a8).  im_max_abs returns NaN if the device call fails. */
float im_max_abs(const Image *const im);                                 /* imutil.c:1959 */
void im_scale(const Image *const im);                                    /* imutil.c:1977 */
int im_subtract(Image *src1, Image *src2, Image *dst);                   /* imutil.c:1997 */
int im_downsample_2x(const Image *const src, Image *const dst);          /* imutil.c:1742 */

void init_GSS_filters(GSS_filters *const gss);                          /* imutil.c:3744 */
int make_gss(GSS_filters *const gss, const Pyramid *const pyr);         /* imutil.c:3752 */
void cleanup_GSS_filters(GSS_filters *const gss);                       /* imutil.c:3806 */
void init_Pyramid(Pyramid *const pyr);                                  /* imutil.c:3832 */
int resize_Pyramid(const Image *const im, const int first_level, const unsigned int num_kp_levels,
                   const unsigned int num_levels, const int first_octave,
                   const unsigned int num_octaves, Pyramid *const pyr); /* imutil.c:3858 */
int set_scales_Pyramid(const double sigma0, const double sigma_n, Pyramid *const pyr); /* imutil.c:3957 */
void cleanup_Pyramid(Pyramid *const pyr);                               /* imutil.c:4051 */

/* ======================= libsift3D subset (replaces sift3d/sift.h entries) ========================= */
int init_SIFT3D(SIFT3D *sift3d);                                        /* sift.c:583 */
void cleanup_SIFT3D(SIFT3D *const sift3d);                              /* sift.c:659 */
/* Deep copy: parameters, image and pyramids (device to device into a context of dst's own). */
int copy_SIFT3D(const SIFT3D *const src, SIFT3D *const dst);          /* sift.c:629 */
int set_peak_thresh_SIFT3D(SIFT3D *const sift3d, const double peak_thresh);       /* sift.c:514 */
int set_corner_thresh_SIFT3D(SIFT3D *const sift3d, const double corner_thresh);   /* sift.c:527 */
int set_num_kp_levels_SIFT3D(SIFT3D *const sift3d, const unsigned int num_kp_levels); /* sift.c:542 */
int set_sigma_n_SIFT3D(SIFT3D *const sift3d, const double sigma_n);               /* sift.c:552 */
int set_sigma0_SIFT3D(SIFT3D *const sift3d, const double sigma0);                 /* sift.c:568 */

void init_Keypoint_store(Keypoint_store *const kp);                     /* sift.c:399 */
int init_Keypoint(Keypoint *const key);                                 /* sift.c:406 */
int resize_Keypoint_store(Keypoint_store *const kp, const size_t num);  /* sift.c:417 */
int copy_Keypoint(const Keypoint *const src, Keypoint *const dst);      /* sift.c:439 */
void cleanup_Keypoint_store(Keypoint_store *const kp);                  /* sift.c:455 */
void init_SIFT3D_Descriptor_store(SIFT3D_Descriptor_store *const desc);    /* sift.c:462 */
void cleanup_SIFT3D_Descriptor_store(SIFT3D_Descriptor_store *const desc); /* sift.c:468 */

/* THE BOUNDARY */
int SIFT3D_detect_keypoints(SIFT3D *const sift3d, const Image *const im,
                            Keypoint_store *const kp);                  /* sift.c:1609 */
int SIFT3D_have_gpyr(const SIFT3D *const sift3d);                       /* sift.c:1936 */
int SIFT3D_extract_descriptors(SIFT3D *const sift3d, const Keypoint_store *const kp,
                               SIFT3D_Descriptor_store *const desc);    /* sift.c:2025 */
int SIFT3D_extract_raw_descriptors(SIFT3D *const sift3d, const Image *const im,
                                   const Keypoint_store *const kp,
                                   SIFT3D_Descriptor_store *const desc); /* sift.c:2131 */
int SIFT3D_assign_orientations(const SIFT3D *const sift3d, const Image *const im,
                               Keypoint_store *const kp, double **const conf); /* sift.c:1534 */
int SIFT3D_extract_dense_descriptors(SIFT3D *const sift3d, const Image *const in,
                                     Image *const desc);                /* sift.c:2354 */

/* Matching: exhaustive search on the device, bit-identical decisions. */
int SIFT3D_nn_match(const SIFT3D_Descriptor_store *const d1, const SIFT3D_Descriptor_store *const d2,
                    const float nn_thresh, int **const matches);        /* sift.c:2840 */
int SIFT3D_matches_to_Mat_rm(SIFT3D_Descriptor_store *d1, SIFT3D_Descriptor_store *d2,
                             const int *const matches, Mat_rm *const match1,
                             Mat_rm *const match2);                      /* sift.c:2784 */
int init_Mat_rm(Mat_rm *const mat, const int num_rows, const int num_cols, const Mat_rm_type type,
                const int set_zero);                                     /* imutil.c:631 */
int resize_Mat_rm(Mat_rm *const mat);                                    /* imutil.c:844 */
int zero_Mat_rm(Mat_rm *const mat);                                      /* imutil.c:900 */
void cleanup_Mat_rm(Mat_rm *mat);                                        /* imutil.c:962 */

/* Formats and command-line surface either side of the path. */
im_format im_get_format(const char *path);                               /* imutil.c:1158 */
int im_read(const char *path, Image *const im);                          /* imutil.c:1215 (.nii, .nii.gz, .img/.hdr) */
int im_write(const char *path, const Image *const im);                   /* imutil.c:1262 (.nii, .nii.gz) */
int read_nii(const char *path, Image *const im);                         /* nifti.c:51 */
int write_nii(const char *path, const Image *const im);                  /* nifti.c:167 */
int write_Mat_rm(const char *path, const Mat_rm *const mat);             /* imutil.c:1343 */
int im_channel(const Image *const src, Image *const dst, const unsigned int chan); /* imutil.c:1893 */
int draw_points(const Mat_rm *const in, const int *const dims, int radius,
                Image *const out);                                       /* imutil.c:1012 */
int Keypoint_store_to_Mat_rm(const Keypoint_store *const kp, Mat_rm *const mat);          /* sift.c:2597 */
int SIFT3D_Descriptor_store_to_Mat_rm(const SIFT3D_Descriptor_store *const store,
                                      Mat_rm *const mat);                /* sift.c:2674 */
int Mat_rm_to_SIFT3D_Descriptor_store(const Mat_rm *const mat,
                                      SIFT3D_Descriptor_store *const store); /* sift.c:2721 */
int write_Keypoint_store(const char *path, const Keypoint_store *const kp);               /* sift.c:3143 */
int write_SIFT3D_Descriptor_store(const char *path,
                                  const SIFT3D_Descriptor_store *const desc);             /* sift.c:3206 */
void print_opts_SIFT3D(void);                                            /* sift.c:703 */
int parse_args_SIFT3D(SIFT3D *const sift3d, const int argc, char **argv,
                      const int check_err);                              /* sift.c:754 */
int parse_gnu(const int argc, char *const *argv);                        /* imutil.c:4891 */
void print_bug_msg(void);                                                /* imutil.c:4925 */

/* Registration tail: types of imutil/imtypes.h:337-391 and reg/reg.h. */
typedef enum _tform_type { AFFINE, TPS } tform_type;
typedef enum _interp_type { LINEAR, LANCZOS2 } interp_type;
typedef struct _Tform_vtable {
    int (*copy)(const void *const, void *const);
    void (*apply_xyz)(const void *const, const double, const double, const double, double *const, double *const,
                      double *const);
    int (*apply_Mat_rm)(const void *const, const Mat_rm *const, Mat_rm *const);
    size_t (*get_size)(void);
    int (*write)(const char *, const void *const);
    void (*cleanup)(void *const);
} Tform_vtable;
typedef struct _Tform {
    tform_type type;
    const Tform_vtable *vtable;
} Tform;
typedef struct _Affine {
    Tform tform;
    Mat_rm A;                          /* dim x (dim+1) doubles: x' = A [x 1]^T */
} Affine;
typedef struct _Tps {                  /* imtypes.h:380-385 */
    Tform tform;
    Mat_rm params;                     /* dim x (N + dim + 1) doubles: N kernel weights, the constant, the x, y, z coefficients */
    Mat_rm kp_src;                     /* N x dim doubles: the control points */
    int dim;
} Tps;
typedef struct _Ransac {
    double err_thresh;                 /* inlier threshold (its square bounds the squared error) */
    int num_iter;
} Ransac;
typedef struct _Reg_SIFT3D {
    double src_units[IM_NDIMS], ref_units[IM_NDIMS];
    SIFT3D sift3d;
    Ransac ran;
    SIFT3D_Descriptor_store desc_src, desc_ref;
    Mat_rm match_src, match_ref;
    double nn_thresh;
    int verbose;
} Reg_SIFT3D;
#define SIFT3D_SINGULAR 1              /* imutil.h:19 */

void init_Ransac(Ransac *const ran);                                     /* imutil.c:4238 */
int set_err_thresh_Ransac(Ransac *const ran, double err_thresh);         /* imutil.c:4245 */
int set_num_iter_Ransac(Ransac *const ran, int num_iter);                /* imutil.c:4260 */
int copy_Ransac(const Ransac *const src, Ransac *const dst);             /* imutil.c:4274 */
int init_Affine(Affine *const affine, const int dim);                    /* imutil.c:2560 */
int Affine_set_mat(const Mat_rm *const mat, Affine *const affine);       /* imutil.c:2620 */
int init_tform(void *const tform, const tform_type type);                /* imutil.c:2540 */
int init_Tps(Tps *tps, int dim, int terms);                              /* imutil.c:4213 (terms = N + dim + 1) */
int resize_Tps(Tps *tps, int num_pts, int dim);                          /* imutil.c:4727 */
extern const Tform_vtable Tps_vtable;                                    /* imutil.c:138; copy and write are functional here */
void cleanup_tform(void *const tform);
int copy_tform(const void *const src, void *const dst);
size_t tform_get_size(const void *const tform);
size_t tform_type_get_size(const tform_type type);
tform_type tform_get_type(const void *const tform);
void apply_tform_xyz(const void *const tform, const double x_in, const double y_in, const double z_in,
                     double *const x_out, double *const y_out, double *const z_out);
int write_tform(const char *path, const void *const tform);
int find_tform_ransac(const Ransac *const ran, const Mat_rm *const src, const Mat_rm *const ref,
                      void *const tform);                                /* imutil.c:4757 */
int im_inv_transform(const void *const tform, const Image *const src, const interp_type interp,
                     const int resize, Image *const dst);                /* imutil.c:2040 (resampling on the device) */
int im_resample(const Image *const src, const double *const units, const interp_type interp,
                Image *const dst);                                       /* imutil.c:2191 */
int copy_Mat_rm(const Mat_rm *const src, Mat_rm *const dst);             /* imutil.c:775 */
int concat_Mat_rm(const Mat_rm *const src1, const Mat_rm *const src2, Mat_rm *const dst, const int dim);
int init_Reg_SIFT3D(Reg_SIFT3D *const reg);                              /* reg.c:121 */
void cleanup_Reg_SIFT3D(Reg_SIFT3D *const reg);
int set_nn_thresh_Reg_SIFT3D(Reg_SIFT3D *const reg, const double nn_thresh);
int set_Ransac_Reg_SIFT3D(Reg_SIFT3D *const reg, const Ransac *const ran);
int set_SIFT3D_Reg_SIFT3D(Reg_SIFT3D *const reg, const SIFT3D *const sift3d);
int set_src_Reg_SIFT3D(Reg_SIFT3D *const reg, const Image *const src);
int set_ref_Reg_SIFT3D(Reg_SIFT3D *const reg, const Image *const ref);
int register_SIFT3D(Reg_SIFT3D *const reg, void *const tform);           /* reg.c:239 */
int register_SIFT3D_resample(Reg_SIFT3D *const reg, const Image *const src, const Image *const ref,
                             const interp_type interp, void *const tform); /* reg.c:366 */
int get_matches_Reg_SIFT3D(const Reg_SIFT3D *const reg, Mat_rm *const match_src, Mat_rm *const match_ref);
/* picture outputs of regSift3D (host only) */
int convert_Mat_rm(const Mat_rm *const in, Mat_rm *const out, const Mat_rm_type type);       /* imutil.c:567 */
int im_pad(const Image *const im, Image *const pad);                     /* imutil.c:1471 */
int im_concat(const Image *const src1, const Image *const src2, const int dim, Image *const dst); /* imutil.c:1613 */
int draw_lines(const Mat_rm *const points1, const Mat_rm *const points2, const int *const dims,
               Image *const out);                                        /* imutil.c:1063 */
int SIFT3D_Descriptor_coords_to_Mat_rm(const SIFT3D_Descriptor_store *const store, Mat_rm *const mat); /* sift.c:2628 */
int draw_matches(const Image *const left, const Image *const right, const Mat_rm *const keys_left,
                 const Mat_rm *const keys_right, const Mat_rm *const match_left, const Mat_rm *const match_right,
                 Image *const concat, Image *const keys, Image *const lines);               /* sift.c:2990 */

/* small host-side exports a relinked caller may reach */
void init_Mesh(Mesh *const mesh);                                        /* imutil.c:549 */
void cleanup_Mesh(Mesh *const mesh);                                     /* imutil.c:557 */
void init_Slab(Slab *const slab);                                        /* imutil.c:4071 */
void cleanup_Slab(Slab *const slab);                                     /* imutil.c:4078 */
int init_Mat_rm_p(Mat_rm *const mat, const void *const p, const int num_rows, const int num_cols,
                  const Mat_rm_type type, const int set_zero);           /* imutil.c:655 */
int eigen_Mat_rm(Mat_rm *A, Mat_rm *Q, Mat_rm *L);                       /* imutil.c:2992 (Jacobi instead of LAPACK dsyevd) */
int transpose_Mat_rm(const Mat_rm *const src, Mat_rm *const dst);        /* imutil.c:3338 */
/* the small public helpers beside the hot path (csrc/host/s3d_host_mat.c): host C, no LAPACK */
int identity_Mat_rm(const int n, Mat_rm *const mat);                                             /* imutil.c:934 */
int mul_Mat_rm(const Mat_rm *const mat_in1, const Mat_rm *const mat_in2, Mat_rm *const mat_out); /* imutil.c:2923 */
int solve_Mat_rm(const Mat_rm *const A, const Mat_rm *const B, const double limit, Mat_rm *const X);   /* imutil.c:3089 (LU; SIFT3D_SINGULAR below `limit`, < 0: 100 eps) */
int solve_Mat_rm_ls(const Mat_rm *const A, const Mat_rm *const B, Mat_rm *const X);              /* imutil.c:3207 (min-norm least squares, Jacobi SVD instead of dgelss) */
int det_symm_Mat_rm(Mat_rm *mat, void *det);                                                     /* imutil.c:3389 (the reference's value: the SUM of the eigenvalues) */
int apply_tform_Mat_rm(const void *const tform, const Mat_rm *const mat_in, Mat_rm *const mat_out);   /* imutil.c:2733 */
int im_permute(const Image *const src, const int dim1, const int dim2, Image *const dst);        /* imutil.c:2476 */
int im_upsample_2x(const Image *const src, Image *const dst);                                    /* imutil.c:1685 */
int im_restride(const Image *const src, const size_t *const strides, Image *const dst);          /* imutil.c:2537 */
int draw_grid(Image *grid, int nx, int ny, int nz, int spacing, int line_width);                 /* imutil.c:973 */
int trace_Mat_rm(Mat_rm *mat, void *trace);                                                      /* imutil.c:3301 */
int print_Mat_rm(const Mat_rm *const mat);                                                       /* imutil.c:803 */
void sprint_type_Mat_rm(const Mat_rm *const mat, char *const str);                               /* imutil.c:678 */
char *im_get_parent_dir(const char *path);                                                       /* imutil.c:1322; free() the result */
void err_exit(const char *str);                                                                  /* imutil.c:4112; does not return */
/* Defaults the reference exports as data (its regSift3D prints them: cli/regSift3D.c:83-84) */
extern const double SIFT3D_nn_thresh_default;                            /* reg.h:20, reg.c:24 */
extern const double SIFT3D_err_thresh_default;                           /* imutil.h:33, imutil.c:102 */
extern const int SIFT3D_num_iter_default;                                /* imutil.h:34, imutil.c:103 */
int copy_Pyramid(const Pyramid *const src, Pyramid *const dst);          /* imutil.c:3995 */
int write_pyramid(const char *path, Pyramid *pyr);                       /* imutil.c:4093 (after sift3d_amd_download_pyramid) */

/* ======================= extensions (not in the reference) ========================================= */
/* Device-resident variants: `d_vol` is a float32 volume already in HBM (x fastest, nx*ny*nz). */
int sift3d_amd_detect_keypoints_dev(SIFT3D *const sift3d, const float *d_vol, int nx, int ny, int nz,
                                    double ux, double uy, double uz, Keypoint_store *const kp);
/* Descriptors stay in HBM: *d_desc receives a device pointer to num records laid out like SIFT3D_Descriptor
 * (768 bins followed by xd, yd, zd, sd: 776 floats per record), owned by the library and valid until the next
 * call on this SIFT3D; pass the result of detect in kp. */
int sift3d_amd_extract_descriptors_dev(SIFT3D *const sift3d, const Keypoint_store *const kp,
                                       const float **d_desc);
/* Dense descriptors device to device: d_in nx*ny*nz floats, d_out nx*ny*nz*12 floats.
 * out_units = the units `desc` would carry on entry to the reference call (quirk C-17). */
int sift3d_amd_extract_dense_dev(SIFT3D *const sift3d, const float *d_in, int nx, int ny, int nz,
                                 double ux, double uy, double uz, const double out_units[3], float *d_out);
/* One Gaussian application device to device (d_tmp: scratch of equal size). */
int sift3d_amd_gauss_dev(const float *d_src, float *d_dst, float *d_tmp, int nx, int ny, int nz, int nc,
                         const double units[3], const float *taps, int width, double unit);
/* Copy GSS level data (and, if want_dog, materialise + copy the DoG levels) into the host Pyramids
 * of sift3d, allocating level->data.  Only needed by callers that read pyramid voxels. */
int sift3d_amd_download_pyramid(SIFT3D *const sift3d, int want_dog);
/* For callers that read sift3d->gpyr / sift3d->dog voxels after SIFT3D_detect_keypoints the way they would after the
 * reference's call (sift.c:989-1071 leaves both pyramids on the host): mode 1 copies the Gaussian levels into the host
 * Pyramid at the end of every SIFT3D_detect_keypoints on `sift3d`, mode 2 the DoG levels as well, 0 (default) neither.
 * Without a call the environment variable SIFT3D_HOST_PYRAMID (0 / 1 / 2) decides -- the knob of an LD_PRELOAD deployment.
 * Costs the PCIe transfer of the pyramid (512^3: 3.7 GB, ~0.15 s).  In the multi-GPU mode every rank copies the planes it
 * owns (sift3d_amd_download_pyramid likewise). */
int sift3d_amd_set_host_pyramid(SIFT3D *const sift3d, int mode);
/* Host-only: size the pyramid metadata and the Gaussian bank of `sift3d` for an nx x ny x nz volume as
 * SIFT3D_detect_keypoints would, without device work (used by the multi-GPU Z-slab driver). */
int sift3d_amd_plan(SIFT3D *const sift3d, int nx, int ny, int nz, double ux, double uy, double uz);
/* SIFT3D_nn_match on descriptors already in HBM (e.g. from sift3d_amd_extract_descriptors_dev): rows of
 * 768 floats `stride` floats apart (multiple of 4); matches: host array of na ints. */
int sift3d_amd_nn_match_dev(const float *d_a, size_t a_stride, long na, const float *d_b, size_t b_stride,
                            long nb, float nn_thresh, int *matches, void *hip_stream);
/* Diagnostics: for each keypoint of kp (detected on this SIFT3D) the number of voxels its descriptor window accepts
 * (stats[2i]) and a checksum of their coordinates (stats[2i+1]); stats: host array of 2 * kp->slab.num. */
int sift3d_amd_describe_window_stats(SIFT3D *const sift3d, const Keypoint_store *const kp, unsigned int *stats);
/* Number of extrema candidates before orientation rejection in the last single-GPU detect (diagnostics; a detect on several
 * GPUs does not update it); with a mask set (sift3d_amd_set_mask): after masking. */
long sift3d_amd_last_num_candidates(const SIFT3D *const sift3d);
/* Stream on which this SIFT3D's kernels run (opaque hipStream_t); set before the first detect. */
int sift3d_amd_set_stream(SIFT3D *const sift3d, void *hip_stream);
const char *sift3d_amd_last_error(void);

/* ---- volumes as stored: 8- and 16-bit integers without a float copy ------------------------------------------------------
 * CT, MR and microscopy volumes are stored as int16, uint16 or uint8.  read_nii widens them to float on the host; the entry
 * points below keep the stored elements, so the upload is 2 or 1 bytes per voxel instead of 4 and the caller holds no
 * float copy.  The element types carry their NIfTI-1 datatype codes, so a header's `datatype` can be passed through. */
enum { SIFT3D_AMD_U8 = 2, SIFT3D_AMD_I16 = 4, SIFT3D_AMD_F32 = 16, SIFT3D_AMD_I8 = 256, SIFT3D_AMD_U16 = 512 };
/* vol: nx*ny*nz elements of `dtype`, x fastest; on the host (on_device = 0) or in HBM (on_device = 1, read in place, aligned
 * to its element size).  The result is that of SIFT3D_detect_keypoints on the float image whose voxels are
 * (float)((double)raw * slope + inter) -- bit for bit: the device evaluates that expression as the host reader does, with
 * two separately rounded f64 operations, in the loads of the pyramid's first filter where the volume has unit voxels and
 * whole quads per row (nx % 4 == 0), in a conversion pass of its own otherwise.  slope == 0 counts as 1
 * (read_nii's rule); slope and inter must be finite.  SIFT3D_AMD_F32 forwards to SIFT3D_detect_keypoints /
 * sift3d_amd_detect_keypoints_dev (slope and inter must then be 1 and 0).  Afterwards the struct is in the state a float
 * detect leaves (SIFT3D_extract_descriptors, sift3d_amd_download_pyramid, copy_SIFT3D ...).
 * With several GPUs (SIFT3D_NGPU > 1 / sift3d_amd_set_num_gpus) the typed transport does not apply: the volume is converted
 * on the host and takes the float path -- correct, without the saving (and on_device = 1 is then refused). */
int sift3d_amd_detect_keypoints_typed(SIFT3D *const sift3d, const void *vol, int dtype, int on_device, int nx, int ny, int nz,
                                      double ux, double uy, double uz, double slope, double inter, Keypoint_store *const kp);
/* A NIfTI-1 volume (.nii, .nii.gz, .hdr/.img) with its elements as the file stores them: header handling as read_nii (byte
 * order, vox_offset, units, scl_slope == 0 -> 1).  Single-channel files of the four integer types keep their elements
 * (byte-swapped where the file is) with the header's slope / inter; every other supported datatype comes back as
 * SIFT3D_AMD_F32 with slope 1 / inter 0, converted as read_nii converts; files with more than one channel fail.  `data`
 * is released with sift3d_amd_free_volume. */
typedef struct { void *data; int dtype; int nx, ny, nz; double ux, uy, uz, slope, inter; } sift3d_amd_volume;
int sift3d_amd_read_nii_native(const char *path, sift3d_amd_volume *out);
void sift3d_amd_free_volume(sift3d_amd_volume *v);

/* ---- region of interest: keypoints inside a voxel mask only ------------------------------------------------------------------
 * mask: nx*ny*nz bytes, x fastest, of the volume's own dimensions; a voxel is inside the region iff its byte is non-zero (the
 * whole byte).  A keypoint of octave o at octave coordinates (x, y, z) is kept iff
 *     mask[(z << o) * ny * nx + (y << o) * nx + (x << o)] != 0
 * -- the voxel of the input it sits on (octave o is the input decimated o times at (2x, 2y, 2z), imutil.c:1742-1768; keypoints
 * map back with ldexp(1.0, o), sift.c:2616).  Nothing else changes: the pyramid, the DoG maxima and the peak thresholds are those
 * of the whole volume, so the masked detect returns exactly the unmasked keypoint list with the masked-out records deleted,
 * byte for byte and in the same order, and the descriptors of the survivors are those of the unmasked run.
 * Masked-out candidates are removed BEFORE orientation assignment (that, and the descriptors never computed, is the saving):
 *  - sift3d_amd_last_num_candidates reports the count after masking (single GPU; it is not updated by a multi-GPU detect,
 *    whose ranks do not mask: see below);
 *  - a NaN gradient in the orientation window of a masked-out candidate no longer fails the call (the reference fails at
 *    sift.c:1430): a masked background stops being fatal.
 * on_device: the mask lies in HBM and is read in place, else it is uploaded through a staging buffer that is released again.
 * Any address will do; a device mask that is 16-byte aligned (every allocation is; an offset view of one may not be) is read
 * 16 bytes per lane, any other a byte per lane -- the same bits, several times slower for that one pass over the mask.
 * The mask is packed to one bit per voxel of every octave once, here (about n/7 bytes stay with the struct; the caller's
 * buffer is not referenced after the call returns), and stays in force for every following SIFT3D_detect_keypoints,
 * sift3d_amd_detect_keypoints_dev and sift3d_amd_detect_keypoints_typed on the struct, the verbatim pass of non-finite volumes
 * included, until it is replaced or cleared (mask == NULL; the dimensions are then ignored).  A detect on a volume of other
 * dimensions fails with a message naming both; bad arguments fail and leave a mask already set in force.  copy_SIFT3D copies
 * the mask, cleanup_SIFT3D frees it.  sift3d_amd_plan, the descriptor entry points, the dense path and the matcher do not look
 * at it.  With several GPUs (SIFT3D_NGPU > 1 / sift3d_amd_set_num_gpus) the gathered keypoint list is filtered on the host
 * against the same bits: the same result, without the saving. */
int sift3d_amd_set_mask(SIFT3D *const sift3d, const unsigned char *mask, int on_device, int nx, int ny, int nz);
int sift3d_amd_have_mask(const SIFT3D *const sift3d);       /* 1: a mask is in force */

/* ---- keypoint budget: the n strongest keypoints only -----------------------------------------------------------------------------
 * The strength of a keypoint (x, y, z, o, s) is fabsf(D) as an f32, D the voxel (x, y, z) of DoG level (o, s) as the reference
 * stores it: the single-rounded f32 difference of the two Gaussian levels either side (build_dog, sift.c:1052-1071) -- the voxel
 * sift3d_amd_download_pyramid(sift3d, 1) returns in sift3d->dog.  (The DoG is not stored on the device; the kernel subtracts.)
 * With a budget n > 0 set, a detect returns exactly the list the same detect returns without one, with every record deleted
 * except the n of largest strength: equal strengths go to the record that comes earlier in that list, the survivors keep the
 * reference's order and are byte for byte the records of the unbudgeted run (R and sd included), and so are their descriptors.
 * A list of no more than n records comes back unchanged.  n = 0, the default, is no budget: nothing is launched for it.
 * Order of steps: a mask (sift3d_amd_set_mask) removes candidates first, orientation assignment then decides on all that remain
 * as it does without a budget, and the budget ranks the survivors of both.  So the budget never changes which calls fail (a NaN
 * orientation window still fails the call), sift3d_amd_last_num_candidates is unaffected, and the result is a pure function of
 * the unbudgeted list; what is saved is the describe of the deleted records (and whatever the caller does per keypoint
 * afterwards), not the orientation step.  The selection runs on the device between orientation and the compaction, exact and
 * deterministic, without a synchronisation of its own.
 * Applies to SIFT3D_detect_keypoints, sift3d_amd_detect_keypoints_dev and sift3d_amd_detect_keypoints_typed, the verbatim pass of
 * non-finite volumes included, until it is changed.  n < 0 fails and leaves the previous value.  copy_SIFT3D copies the budget;
 * init_SIFT3D and a fresh struct have none.  The descriptor entry points, the dense path and the matcher do not look at it.
 * With several GPUs (SIFT3D_NGPU > 1 / sift3d_amd_set_num_gpus) and a budget set a detect FAILS with a message that says so
 * (the Z-slab ranks' gather carries no strengths); with no budget the multi-GPU path is unchanged. */
int sift3d_amd_set_max_keypoints(SIFT3D *const sift3d, long n);
long sift3d_amd_get_max_keypoints(const SIFT3D *const sift3d);
/* out[i] = the strength of kp's record i, gathered on demand from the pyramid this struct holds in HBM (after a detect, with or
 * without a budget; an unbudgeted detect pays nothing for it): out is a host array of kp->slab.num floats.  Fails with a message
 * when the struct has no device pyramid, when a record lies outside its DoG level (or the store is empty: verify_keys), or when
 * the pyramid is spread over several GPUs. */
int sift3d_amd_keypoint_strengths(SIFT3D *const sift3d, const Keypoint_store *const kp, float *out);
/* Profiling: HIP events (hipEvent_t) that the single-GPU detects of the calling thread record on their stream in front of the
 * orientation step, behind it, and behind the budget's strength and selection kernels (which follow it directly; without a
 * budget the last two coincide).  NULLs, the default, record nothing. */
void sift3d_amd_set_orient_events(void *before_orient, void *after_orient, void *after_select);

/* ---- sub-voxel keypoints: position and scale refined by a quadratic fit to the DoG ---------------------------------------------
 * Off by default: keypoints then sit on integer voxels of their octave and on pyramid levels, as the reference's do
 * (detect_extrema, sift.c:1200-1205), and every output is what it was.  With refinement on, a detect returns exactly the list the
 * same detect returns with it off -- same count, same order, same o, s and R (orientation is still assigned at the integer voxel) --
 * in which xd, yd, zd have each moved by at most 0.5 octave voxels and sd has been multiplied by 2^(ds / num_kp_levels), |ds| <= 0.5.
 * The fit per keypoint (x, y, z, o, s), D the DoG voxel as the reference stores it (sift3d_amd_download_pyramid(.., 1)), in f64:
 *   gradient g_a = (D(a+1) - D(a-1)) / 2 and second differences H_aa, H_ab (the four diagonal neighbours / 4) over x, y, z within
 *   level s; g_s and H_ss over the centre voxel of levels s - 1, s + 1.  No space-scale cross terms: at the coarse level spacing
 *   they made positions worse.
 *   Space: the solution of H3 d = -g3 where H3 or -H3 is positive definite and every |d_a| <= 0.5; otherwise the per-axis
 *   parabolas d_a = -g_a / H_aa clipped to [-0.5, 0.5] (0 where H_aa == 0 or the quotient is not finite).
 *   Scale: ds = -g_s / H_ss with the same clip and zero rule.
 * xd = x + d_x (likewise yd, zd), sd = level scale * pow(2.0, ds / num_kp_levels).  Extrema lie in 1 .. n - 2 and keypoint levels
 * have both DoG neighbours, so every read is inside the pyramid and every refined position passes SIFT3D_extract_descriptors'
 * bounds check.  The kernel (s3d_k_refine_keys) runs behind the compaction on the compacted records, without a synchronisation of
 * its own; a mask and a budget compose unchanged (both act before it).  Descriptors of refined keypoints are those of the refined
 * doubles: the descriptor kernel takes centres off the grid.  sift3d_amd_keypoint_strengths truncates positions to a voxel: take
 * strengths from an unrefined store.
 * Applies to SIFT3D_detect_keypoints, sift3d_amd_detect_keypoints_dev and sift3d_amd_detect_keypoints_typed, the verbatim pass of
 * non-finite volumes included, until it is changed.  Without a call the environment variable SIFT3D_SUBVOXEL (non-zero: on)
 * decides, read once per struct at its first detect (for unchanged callers: register_SIFT3D, regSift3D); an explicit call
 * overrides it.  copy_SIFT3D copies the setting.  With several GPUs (SIFT3D_NGPU > 1 / sift3d_amd_set_num_gpus) and refinement
 * on a detect FAILS with a message that says so (the Z-slab ranks' gather carries integer records). */
int sift3d_amd_set_subvoxel(SIFT3D *const sift3d, int on);
int sift3d_amd_get_subvoxel(const SIFT3D *const sift3d);       /* 0 / 1: what the next detect on this struct will do */
/* out[0] / out[1]: how many keypoints of the struct's last single-GPU detect took the 3-D fit / the per-axis fallback (their sum
 * is the keypoint count; both 0 after an unrefined detect) */
int sift3d_amd_last_subvoxel_counts(const SIFT3D *const sift3d, long out[2]);
/* Profiling: HIP events the refining single-GPU detects of the calling thread record in front of and behind s3d_k_refine_keys
 * (its counter reset included).  NULLs, the default, record nothing. */
void sift3d_amd_set_subvoxel_events(void *before_refine, void *after_refine);

/* ---- RANSAC: the hypotheses of find_tform_ransac scored on the device --------------------------------------------------------
 * find_tform_ransac draws its num_iter four-point models exactly as before (the same rand() calls in the same order; scoring
 * consumes none) and counts every model's inliers either in the host loop or in one kernel launch per batch of models
 * (s3d_k_ransac_count).  A count is an integer computed with the same f64 operations either way, so both paths pick the same
 * winner (the lowest iteration holding the maximum count) and return the same transform, bit for bit, and the same failures.
 * The knob is process-wide (Ransac is 16 bytes by ABI and carries no field for it):
 *   AUTO (default)  the device path when a device is usable and npts * num_iter is large enough to pay for the transfers
 *                   (S3D_RANSAC_AUTO_MIN_WORK, s3d_host_reg.c); the host path otherwise, and silently, with the identical
 *                   result, when no device is found or a device call fails;
 *   HOST            always the host loop;
 *   DEVICE          always the device; a missing device or a failing device call is SIFT3D_FAILURE with sift3d_amd_last_error set.
 * Without a call to sift3d_amd_set_ransac_device the environment variable SIFT3D_RANSAC_DEVICE (-1 / 0 / 1) decides, read once
 * per process (for LD_PRELOAD deployments of unchanged callers).  register_SIFT3D, register_SIFT3D_resample and regSift3D go
 * through find_tform_ransac and need no change.  Device memory of a call (the matches, one batch of models and counts) is
 * freed before it returns. */
#define SIFT3D_AMD_RANSAC_AUTO (-1)
#define SIFT3D_AMD_RANSAC_HOST 0
#define SIFT3D_AMD_RANSAC_DEVICE 1
int sift3d_amd_set_ransac_device(int mode);   /* other values: SIFT3D_FAILURE, the mode is left as it was */
int sift3d_amd_get_ransac_device(void);
int sift3d_amd_ransac_last_path(void);        /* 0 host, 1 device: the scoring path of the calling thread's last find_tform_ransac */
/* Profiling: with on != 0 the device path brackets its transfers and kernels with HIP events, and
 * sift3d_amd_ransac_last_device_ms returns their sum for the calling thread's last find_tform_ransac (0 on the host path). */
void sift3d_amd_set_ransac_profile(int on);
double sift3d_amd_ransac_last_device_ms(void);

/* ---- thin-plate-spline registration: fit from matches, warp on the device ----------------------------------------------------
 * A Tps maps a point p of the reference volume to the source volume (the direction im_inv_transform needs):
 *     f(p) = sum_n U(|p - c_n|^2) w_n + a_0 + a_x p_x + a_y p_y + a_z p_z,     U(r2) = r2 log r2, U(0) = 0,
 * c_n the rows of kp_src, w_n and a_* the columns of params (Tps above).  apply_tform_xyz / apply_tform_Mat_rm evaluate it with
 * the reference's expression and summation order (bit-identical to its apply_Tps_*); copy_tform deep-copies; write_tform writes
 * one CSV of N + 4 rows x 6 columns: row n < N is [c_x c_y c_z w_x w_y w_z], the last four rows are [0 0 0 a_x a_y a_z] for the
 * constant and the x, y, z coefficients.  im_inv_transform warps through a 3-D Tps on the device (s3d_k_inv_tps).
 * init_tform(t, TPS) still fails as the reference's does: it has no point count to allocate with.  Use init_Tps(t, 3, 4).
 *
 * sift3d_amd_fit_tps: src, ref n x 3 doubles, one point per row (as find_tform_ransac takes them), f(ref_i) ~ src_i.  Solves
 *     [K + lambda I, P; P^T, 0] [w; a] = [src; 0],   K_ij = U(|ref_i - ref_j|^2),  P = [1 x y z]
 * in f64 by LU with partial pivoting; lambda = 0 interpolates, larger values trade fidelity for bending energy.  Rows whose ref
 * point equals an earlier row's exactly are dropped with their src point.  Works in the coordinates given: with voxel
 * coordinates of anisotropic volumes the bending energy is measured in voxels, not mm.  SIFT3D_FAILURE with
 * sift3d_amd_last_error set for fewer than 4 remaining points, a singular system (coplanar points), lambda < 0 or NaN, and
 * matrices of the wrong shape or type.  tps must have been initialised (init_Tps); it is resized. */
int sift3d_amd_fit_tps(const Mat_rm *const src, const Mat_rm *const ref, double lambda, Tps *const tps);
/* register_SIFT3D into `affine` (voxel space, as today), then a spline through the matches that agree with it:
 * control points are the matches whose residual under the affine, in physical units and by find_tform_ransac's rule
 * (!(e > thresh^2)), is within ctrl_thresh -- deliberately wider than the consensus threshold, which rejects exactly the matches
 * that carry the deformation.  More than max_points of them: every k-th in match order, k = ceil(count / max_points).  They go
 * to sift3d_amd_fit_tps in voxel coordinates.  opts NULL, or a field <= 0 (lambda < 0): the default of that field. */
typedef struct {
    double lambda;        /* default 1000 */
    double ctrl_thresh;   /* default 4 * reg->ran.err_thresh */
    int max_points;       /* default 512 */
} sift3d_amd_tps_opts;
#define SIFT3D_AMD_TPS_LAMBDA_DEFAULT 1000.0
#define SIFT3D_AMD_TPS_MAX_POINTS_DEFAULT 512
int sift3d_amd_register_tps(Reg_SIFT3D *const reg, const sift3d_amd_tps_opts *const opts, Affine *const affine, Tps *const tps);

/* ---- similarity of a registration: MSE, NCC and mutual information on the device ------------------------------------------
 * "How well does src under tform agree with ref?"  One fused pass over the reference volume (s3d_k_similarity_*): every voxel
 * (x, y, z) of ref goes through tform exactly as im_inv_transform pushes it (a 3-D Affine, a 3-D Tps, or NULL: the identity,
 * scored as the affine [I | 0]), src is sampled there (LINEAR or LANCZOS2), and the pair a = ref voxel, b = the float the warp
 * would have stored is accumulated; the warped volume is never written.  Single-channel volumes only.
 *   Overlap: the voxels the warp samples (no coordinate outside [0, n - 1] of src, none NaN) whose a and b are both finite.
 *       Everything below is over the overlap; n is its size, n_total the voxels of ref.
 *   Joint histogram: bins B in 2 .. 128 over [ref_range] x [src_range]; the bin of a is t = ((double)a - lo) * (B / (hi - lo))
 *       in f64, each operation rounded, index t < 0 ? 0 : t >= B ? B - 1 : (int)t (so a == hi lands in bin B - 1 and Lanczos
 *       overshoot clamps); an empty range (hi == lo) has scale 0: everything in bin 0.  joint[ia * B + ib], row = reference
 *       bin, 64-bit counts; n is their sum.  Exact whatever the schedule.
 *   Default ranges: the minimum and maximum over the finite voxels of each whole volume (src itself, not its warp), found on
 *       the device; a volume without a finite voxel fails.  A caller's range is used when its [1] > [0].
 *   Moments: seven f64 sums about the pivots c = 0.5 * (lo + hi) of the two ranges; from them, in f64,
 *       mean = c + S/n, var = S2/n - (S/n)^2, cov = Sab/n - (Sa/n)(Sb/n), ncc = cov / sqrt(var_ref * var_src) (NaN when a
 *       variance is <= 0), mse = sum (a - b)^2 / n, mae = sum |a - b| / n.  The sums are added in a fixed order: two calls on
 *       the same device and build return the same bits.
 *   Entropies in nats from the histogram's marginals and cells; mi = h_ref + h_src - h_joint; nmi = (h_ref + h_src) / h_joint
 *       (NaN when h_joint == 0).
 *   n == 0 is a success: n = 0 and every statistic NaN.
 * SIFT3D_FAILURE with sift3d_amd_last_error set, and out / joint untouched, for: bins outside 2 .. 128 (0: 64), an interp that
 * is neither LINEAR nor LANCZOS2, a tform that is neither NULL, a 3-D Affine nor a 3-D Tps, nc != 1, NULL data, a NaN in a
 * range, a volume without a finite voxel, and a device failure.  opts NULL: all defaults. */
typedef struct { long long n, n_total; double mean_ref, mean_src, var_ref, var_src, mse, mae, ncc,
                 h_ref, h_src, h_joint, mi, nmi; } sift3d_amd_similarity;
typedef struct { int bins;              /* 0: 64 */
                 interp_type interp;    /* LINEAR */
                 double ref_range[2], src_range[2];   /* used when [1] > [0], else the volume's finite min / max */
               } sift3d_amd_similarity_opts;
#define SIFT3D_AMD_SIMILARITY_BINS_DEFAULT 64
#define SIFT3D_AMD_SIMILARITY_BINS_MAX 128
/* Host volumes: non-default strides are gathered as im_inv_transform does, both volumes are uploaded, scored and freed. */
int sift3d_amd_im_similarity(const void *tform, const Image *src, const Image *ref,
                             const sift3d_amd_similarity_opts *opts, sift3d_amd_similarity *out,
                             unsigned long long *joint /* bins*bins, row = reference bin; may be NULL */);
/* Device-resident volumes (x fastest, default strides); the work is ordered on hip_stream and has completed on return. */
int sift3d_amd_similarity_dev(const void *tform, const float *d_src, int snx, int sny, int snz,
                              const float *d_ref, int rnx, int rny, int rnz,
                              const sift3d_amd_similarity_opts *opts, sift3d_amd_similarity *out,
                              unsigned long long *joint, void *hip_stream);

/* ---- intensity-based refinement of an affine registration on the device ----------------------------------------------------
 * Improves an affine map (reference voxel -> source voxel coordinates, what register_SIFT3D returns) on the voxel intensities:
 * Levenberg-Marquardt on its 12 entries for the cost sum r^2 / n over the overlap, r = sb (b - mb) - sa (a - ma), a the
 * reference voxel and b the tri-linear sample of the source (the pair sift3d_amd_im_similarity scores; the overlap is its
 * overlap, less the voxels whose intensity gradient is not finite).  Every evaluation is one fused pass on the device
 * (s3d_k_affine_normal_eq, include/s3d_device.h) that returns the cost and the normal equations together, so a rejected step
 * costs one pass; the 12 x 12 system (H + lambda diag H) delta = -grad is solved on the host in f64, in coordinates centred on
 * the reference volume.
 *   Step rule: lambda starts at 1e-3; a step is accepted when the cost decreases and n >= min_overlap * (n at the level's
 *       start; on level 0: n_before), then lambda / 10, else lambda * 10.  A level stops CONVERGED when an accepted step moves no
 *       corner of ref by more than tol level-0 voxels (or the gradient is exactly zero), MAX_ITER after max_iter accepted steps,
 *       STALLED when lambda exceeds 1e10.
 *   Pyramid: coarse to fine on the device; level l is l rounds of (Gaussian of sigma 1 voxel, every second voxel), level voxel
 *       i being level-0 voxel 2^l i in both volumes, so the linear part carries over and the translation scales by 2^-l.  A
 *       level at which a dimension of either volume would fall below 16 is skipped.  Level 0 starts from the coarse levels'
 *       result only if that is no worse there (cost and overlap) than the affine as given, else from the affine as given.
 *   normalize = 1: sa = 1 / std(a), ma = mean(a), sb = 1 / std(b), mb = mean(b) over the overlap at the level's starting
 *       transform (sift3d_amd_similarity_dev), frozen for the level; a variance that is not positive gives scale 1.  This makes
 *       the cost blind to a gain and an offset between the volumes at the price of a small bias from the frozen constants.
 *   Non-finite voxels are excluded per voxel as in the similarity overlap.  The Gaussian of the coarse levels spreads them over
 *       its support; nothing is done about that.
 * Returns SIFT3D_SUCCESS with *affine refined: its level-0 cost is <= the cost of the affine as given and its
 * n >= min_overlap * n_before.  Where no such map was found, *affine is returned bit for bit as given with status UNCHANGED.
 * info (may be NULL): status is the way level 0 ended unless UNCHANGED; iters counts the accepted steps behind the returned
 * map, passes every normal-equation pass; costs are sum r^2 / n at level 0 with level 0's constants.
 * SIFT3D_FAILURE with sift3d_amd_last_error set, *affine and *info untouched, for: no overlap at the start, nc != 1, NULL data, a
 * source dimension < 2, a transform that is not a 3-D Affine, a NaN or negative option, and a device failure.  opts NULL: all
 * defaults.  Device memory of a call is freed before it returns. */
typedef struct {
    int levels;          /* 0: 3.  pyramid levels, coarse to fine */
    int max_iter;        /* 0: 30 accepted steps per level */
    double tol;          /* 0: 1e-3 level-0 voxels */
    double min_overlap;  /* 0: 0.5 */
    int normalize;       /* 0: raw SSD.  1: z-scored */
} sift3d_amd_refine_opts;
#define SIFT3D_AMD_REFINE_CONVERGED 0
#define SIFT3D_AMD_REFINE_MAX_ITER 1
#define SIFT3D_AMD_REFINE_STALLED 2
#define SIFT3D_AMD_REFINE_UNCHANGED 3
typedef struct {
    int status;                        /* SIFT3D_AMD_REFINE_* */
    int levels_run, iters, passes;
    long long n_before, n_after;       /* level 0 */
    double cost_before, cost_after;    /* level 0 */
    double max_corner_shift;           /* level-0 voxels: the largest displacement of a corner of ref, start against result */
} sift3d_amd_refine_info;
#define SIFT3D_AMD_REFINE_LEVELS_DEFAULT 3
#define SIFT3D_AMD_REFINE_ITER_DEFAULT 30
/* Host volumes: non-default strides are gathered, both volumes are uploaded, the map is refined, everything is freed. */
int sift3d_amd_refine_affine(const Image *src, const Image *ref, const sift3d_amd_refine_opts *opts,
                             Affine *affine /* in: the start; out: refined */, sift3d_amd_refine_info *info);
/* Device-resident volumes (x fastest, default strides); the work is ordered on hip_stream and has completed on return. */
int sift3d_amd_refine_affine_dev(const float *d_src, int snx, int sny, int snz, const float *d_ref, int rnx, int rny, int rnz,
                                 const sift3d_amd_refine_opts *opts, Affine *affine, sift3d_amd_refine_info *info,
                                 void *hip_stream);

/* ---- deformable registration on the device: demons refinement of an affine map --------------------------------------------
 * What is left after the affine map -- local deformation -- as a dense displacement field u over the reference volume, from the
 * voxel intensities: the source is compared at T(x) + u(x), T the affine map as given (NULL: the identity), u in source voxels.
 * Thirion's demons with the gradient of the moving (source) image, diffusion-regularised: one iteration is one pass over the
 * reference volume (s3d_k_demons_step, include/s3d_device.h: the update, the cost and the count together) and one Gaussian of
 * sigma voxels over each component of the field (s3d_k_sep_fir, one channel, unit spacing).  The cost is that of
 * sift3d_amd_refine_affine, sum r^2 / n over the overlap, r = sb (b - mb) - sa (a - ma).
 *   Pyramid: the refinement's -- level l is l rounds of (Gaussian of sigma 1 voxel, every second voxel), dimensions n / 2, the
 *       linear part of T kept and its translation scaled by 2^-l; a level at which a dimension of either volume would fall
 *       below 16 is skipped, and so is one whose reference is too small for the field's Gaussian (a dimension below
 *       ceil(3 sigma) + 2).  The field of a level is in that level's voxels.
 *   Start of a level: the coarsest level starts from the zero field, every finer one from s3d_k_field_upsample2 of the level above.
 *   Iteration k = 0, 1, .. of a level: (1) s3d_k_demons_step from u into v with kstep = 1 / (4 max_step^2), so no voxel moves
 *       by more than max_step level voxels in one update; (2) the three sums S are read back, c_k = S[0] / S[1]; (3) each
 *       component of v is smoothed into u.  The taps are init_Gauss_filter's: half width ceil(3 sigma), tap i =
 *       (float)exp(-0.5 x^2), x = (i - half width) / (sigma + DBL_EPSILON), divided by their float sum.
 *   Stopping: a level stops CONVERGED at the first k >= 5 with c_k > (1 - tol) c_(k-5), before that pass's update is applied (u
 *       stays the field c_k was measured on); MAX_ITER after max_iter passes, each applied.  A level whose first pass counts no
 *       voxel (S[1] == 0) is left out: its field goes on to the next level as it came.
 *   normalize = 1: sa, ma, sb, mb as in sift3d_amd_refine_affine -- sift3d_amd_similarity_dev under the level's affine map alone,
 *       frozen for the level.
 *   Acceptance: cost_before and n_before are those of a level-0 pass with the zero field (no overlap there is a failure),
 *       cost_after and n_after those of one more level-0 pass on the final field, both with level 0's constants.  The field is
 *       returned only if cost_after <= cost_before and n_after >= min_overlap * n_before, and level 0 was not left out;
 *       otherwise it is returned all zero bits with status UNCHANGED.
 * field: ref's dimensions and units, nc = 3 (x, y, z displacement in source voxels, channel fastest), resized by the call;
 * d_field: planar, 3 N floats (include/s3d_device.h).  info (may be NULL): status is the way level 0 ended unless UNCHANGED;
 * levels_run counts the levels not left out, iters the updates applied and passes every s3d_k_demons_step of the call;
 * mean_disp and max_disp are the mean and the largest |u| over the returned field's finite entries.
 * SIFT3D_FAILURE with sift3d_amd_last_error set, *field (d_field) and *info untouched, for: no overlap at the start, nc != 1,
 * NULL data or field, a source dimension < 2, a reference dimension < ceil(3 sigma) + 2, a transform that is neither NULL nor a
 * 3-D Affine (a Tps is not supported as the base transform), negative levels or max_iter, a NaN or negative tol or min_overlap,
 * normalize other than 0 or 1, sigma outside 0.5 .. 8, a max_step that is not positive, and a device failure.  opts NULL: all
 * defaults.  Device memory of a call is freed before it returns. */
typedef struct {
    int levels;          /* 0: 3 */
    int max_iter;        /* 0: 50 passes per level */
    double sigma;        /* 0: 1.5 level voxels; allowed 0.5 .. 8 */
    double max_step;     /* 0: 1.0 level voxel */
    double tol;          /* 0: 1e-3 */
    double min_overlap;  /* 0: 0.5 */
    int normalize;       /* 0: raw SSD.  1: z-scored */
} sift3d_amd_demons_opts;
#define SIFT3D_AMD_DEMONS_CONVERGED 0
#define SIFT3D_AMD_DEMONS_MAX_ITER 1
#define SIFT3D_AMD_DEMONS_UNCHANGED 3
typedef struct {
    int status;                        /* SIFT3D_AMD_DEMONS_*, level 0 */
    int levels_run, iters, passes;
    long long n_before, n_after;       /* level 0 */
    double cost_before, cost_after;    /* level 0, sum r^2 / n */
    double mean_disp, max_disp;        /* |u| over the field, level-0 voxels */
} sift3d_amd_demons_info;
#define SIFT3D_AMD_DEMONS_LEVELS_DEFAULT 3
#define SIFT3D_AMD_DEMONS_ITER_DEFAULT 50
/* Host volumes: non-default strides are gathered, both volumes are uploaded, the field is downloaded and interleaved. */
int sift3d_amd_register_demons(const Image *src, const Image *ref, const void *tform /* NULL or a 3-D Affine */,
                               const sift3d_amd_demons_opts *opts, Image *field /* out: ref's dims and units, nc = 3 */,
                               sift3d_amd_demons_info *info);
/* Device-resident volumes (x fastest, default strides); the work is ordered on hip_stream and has completed on return. */
int sift3d_amd_register_demons_dev(const float *d_src, int snx, int sny, int snz, const float *d_ref, int rnx, int rny, int rnz,
                                   const void *tform, const sift3d_amd_demons_opts *opts, float *d_field /* planar, 3 * N */,
                                   sift3d_amd_demons_info *info, void *hip_stream);
/* im_inv_transform through tform (NULL or a 3-D Affine) plus a field: dst(x) = src sampled at T(x) + field(x).  dst takes the
 * field's dimensions and units and src's channels; the field (nc = 3) is de-interleaved on upload (s3d_k_inv_field). */
int sift3d_amd_im_warp_field(const void *tform, const Image *field, const Image *src, interp_type interp, Image *dst);

/* ---- the other direction of a field's map, whether it folds, and points through it ----------------------------------------------
 * (extension.)  A transform T (NULL: the identity, or a 3-D Affine) and a field u over the reference grid are the map
 * phi(x) = T(x) + u(x), reference voxel to source voxel coordinates: what sift3d_amd_register_demons returns and
 * sift3d_amd_im_warp_field takes.
 *
 * sift3d_amd_invert_field: psi = phi^-1 over the source grid snx x sny x snz, returned as a pair of the same kind,
 * psi(y) = inv_tform(y) + inv_field(y), source voxel to reference voxel coordinates.  So sift3d_amd_im_warp_field(&inv_tform,
 * &inv_field, ref, ..) pulls the reference (an atlas, a label volume) onto the source grid, and sift3d_amd_field_apply_points
 * with the pair carries source-side points into the reference.  inv_tform = T^-1, the 3 x 3 inverse by cofactors on the host;
 * inv_field by s3d_k_field_invert (include/s3d_device.h: the iteration, its operation order and the status values): per source
 * voxel the fixed-point iteration w <- -T^-1 u(T^-1 y + w) on the field continued constantly past its faces, at most max_iter
 * updates, ended when |phi(psi(y)) - y| <= tol source voxels.  It contracts where the map does not fold; where it does not end,
 * the voxel keeps its last w and is counted.  info: n = n_converged + n_outside + n_not_converged + n_invalid source voxels --
 * converged with psi(y) inside the reference grid; converged on the continued field (psi(y) outside it: an extrapolation);
 * not converged; invalid (a coordinate or a sample that is not finite: the voxel's entries are NaN) --, updates the updates made
 * over all voxels, mean_residual and max_residual |phi(psi(y)) - y| in source voxels over the voxels that are not invalid.
 * inv_field takes the source dimensions, src_units (NULL: 1, 1, 1) and nc = 3.
 * SIFT3D_FAILURE with sift3d_amd_last_error() set and every output untouched for: a transform that is neither NULL nor a 3-D
 * Affine (a Tps is not supported as the base transform), a linear part that is singular or not finite, a field whose nc != 3,
 * NULL data or outputs, an inv_tform that is not an initialised 3-D Affine, a dimension < 1, negative max_iter, negative or NaN
 * tol, units that are not positive, and a device failure.  opts NULL: all defaults.  Device memory of a call is freed before it
 * returns. */
typedef struct {
    int max_iter;        /* 0: 30 updates per voxel */
    double tol;          /* 0: 1e-3 source voxel */
} sift3d_amd_field_inverse_opts;
typedef struct {
    long long n, n_converged, n_outside, n_not_converged, n_invalid, updates;
    double mean_residual, max_residual;
} sift3d_amd_field_inverse_info;
#define SIFT3D_AMD_FIELD_INVERSE_ITER_DEFAULT 30
/* Host field (nc = 3, any strides): de-interleaved on upload, the inverse field downloaded and interleaved. */
int sift3d_amd_invert_field(const void *tform /* NULL or a 3-D Affine */, const Image *field, int snx, int sny, int snz,
                            const double src_units[3] /* NULL: 1, 1, 1 */, const sift3d_amd_field_inverse_opts *opts,
                            Affine *inv_tform /* out, initialised by the caller */, Image *inv_field /* out: nc = 3 */,
                            sift3d_amd_field_inverse_info *info /* may be NULL */);
/* Device-resident planar fields (3 * rnx * rny * rnz floats in, 3 * snx * sny * snz out); no field is copied to the host.  The
 * work is ordered on hip_stream and has completed on return.  inv_A: T^-1 as 3 x 4 row-major doubles. */
int sift3d_amd_invert_field_dev(const float *d_field, int rnx, int rny, int rnz, const void *tform, float *d_inv_field, int snx,
                                int sny, int snz, const sift3d_amd_field_inverse_opts *opts, double inv_A[12] /* out */,
                                sift3d_amd_field_inverse_info *info, void *hip_stream);

/* sift3d_amd_field_jacobian: the determinant of d phi / d x per reference voxel (s3d_k_field_jacobian: central differences of
 * the field, one-sided on the faces, plus T's linear part).  det (may be NULL: statistics only) takes the field's dimensions and
 * units and nc = 1.  info (may be NULL, not both): n voxels, n_finite of them with a finite determinant, n_folded of those with
 * det <= 0 -- the map is not invertible there --, and the minimum, maximum and mean over the finite ones (NaN when there is
 * none).  The determinant is in voxel coordinates: the ratio of physical volumes is det times the ratio of the source's voxel
 * volume to the reference's; the sign, and with it n_folded, is unaffected.  Fails as above, and for a dimension < 2. */
typedef struct {
    long long n, n_finite, n_folded;
    double min_det, max_det, mean_det;
} sift3d_amd_field_jacobian_info;
int sift3d_amd_field_jacobian(const void *tform, const Image *field, Image *det /* may be NULL: statistics only */,
                              sift3d_amd_field_jacobian_info *info /* may be NULL, not both */);
int sift3d_amd_field_jacobian_dev(const float *d_field, int rnx, int rny, int rnz, const void *tform, float *d_det,
                                  sift3d_amd_field_jacobian_info *info, void *hip_stream);

/* out(:, j) = T(in(:, j)) + the tri-linear sample of the field at in(:, j) clamped to the grid: in and out 3 x n doubles (out is
 * resized; it may be in).  On the host, in plain C: the f64 sample expression of s3d_k_field_invert, not rounded to float, so at
 * an integer point of the grid it is T(x) + (double)u(x) to the bit.  A point with a coordinate that is not finite gives NaN. */
int sift3d_amd_field_apply_points(const void *tform, const Image *field, const Mat_rm *in, Mat_rm *out);

/* ---- ABI checks (x86-64 SysV; values measured on the compiled reference) ----------- */
#if defined(__x86_64__) && !defined(SIFT3D_AMD_NO_ABI_ASSERT)
#define S3D_ABI_SIZE(T, n) _Static_assert(sizeof(T) == (n), "ABI size of " #T)
#define S3D_ABI_OFF(T, f, n) _Static_assert(offsetof(T, f) == (n), "ABI offset of " #T "." #f)
#ifndef __cplusplus
S3D_ABI_SIZE(Image, 104); S3D_ABI_OFF(Image, cl_image, 8); S3D_ABI_OFF(Image, s, 16);
S3D_ABI_OFF(Image, size, 24); S3D_ABI_OFF(Image, nx, 32); S3D_ABI_OFF(Image, ux, 48);
S3D_ABI_OFF(Image, xs, 72); S3D_ABI_OFF(Image, nc, 96); S3D_ABI_OFF(Image, cl_valid, 100);
S3D_ABI_SIZE(Reg_SIFT3D, 512); S3D_ABI_OFF(Reg_SIFT3D, sift3d, 48); S3D_ABI_OFF(Reg_SIFT3D, ran, 352);
S3D_ABI_OFF(Reg_SIFT3D, desc_src, 368); S3D_ABI_OFF(Reg_SIFT3D, match_src, 432); S3D_ABI_OFF(Reg_SIFT3D, nn_thresh, 496);
S3D_ABI_SIZE(Ransac, 16); S3D_ABI_SIZE(Tform, 16); S3D_ABI_SIZE(Affine, 48); S3D_ABI_OFF(Affine, A, 16); S3D_ABI_SIZE(Tform_vtable, 48);
S3D_ABI_SIZE(Tps, 88); S3D_ABI_OFF(Tps, params, 16); S3D_ABI_OFF(Tps, kp_src, 48); S3D_ABI_OFF(Tps, dim, 80);
S3D_ABI_SIZE(Mat_rm, 32); S3D_ABI_SIZE(Keypoint, 112); S3D_ABI_OFF(Keypoint, R, 40);
S3D_ABI_OFF(Keypoint, xd, 72); S3D_ABI_OFF(Keypoint, sd, 96); S3D_ABI_OFF(Keypoint, o, 104);
S3D_ABI_OFF(Keypoint, s, 108); S3D_ABI_SIZE(Slab, 24); S3D_ABI_SIZE(Keypoint_store, 48);
S3D_ABI_SIZE(Hist, 48); S3D_ABI_SIZE(SIFT3D_Descriptor, 3104); S3D_ABI_OFF(SIFT3D_Descriptor, xd, 3072);
S3D_ABI_SIZE(SIFT3D_Descriptor_store, 32); S3D_ABI_SIZE(Sep_FIR_filter, 32); S3D_ABI_SIZE(Gauss_filter, 40);
S3D_ABI_SIZE(GSS_filters, 56); S3D_ABI_SIZE(Pyramid, 48); S3D_ABI_SIZE(Tri, 48); S3D_ABI_SIZE(Mesh, 16);
S3D_ABI_SIZE(SIFT3D, 304); S3D_ABI_OFF(SIFT3D, gss, 16); S3D_ABI_OFF(SIFT3D, gpyr, 80);
S3D_ABI_OFF(SIFT3D, dog, 128); S3D_ABI_OFF(SIFT3D, im, 176); S3D_ABI_OFF(SIFT3D, peak_thresh, 280);
S3D_ABI_OFF(SIFT3D, dense_rotate, 296);
#endif
#endif

#ifdef __cplusplus
}
#endif
#endif
