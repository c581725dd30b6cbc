/* s3d_host_reg.c -- the registration tail: match -> RANSAC affine -> resample.
 *
 *   Ransac / Affine / Tform lifecycle         imutil.c:2563-2672, 2846-2860, 4238-4277
 *   find_tform_ransac + ransac                imutil.c:4611-4882 (n_choose_k on libc rand(), 4286-4325)
 *   solve: square systems (the 4-point sample) by LU with partial pivoting and a 1-norm condition test
 *          against 100 eps (solve_Mat_rm over dgetrf/dgecon/dgetrs, imutil.c:3089-3190); the least-squares
 *          refinement on the consensus set by SVD with the minimum-norm convention of dgelss
 *          (solve_Mat_rm_ls, imutil.c:3196-3300).  LAPACK is not available to the product, so both are
 *          written out here: one-sided Jacobi for the SVD, an explicit inverse for the condition number
 *          (the exact value where dgecon estimates it).  Solutions agree with LAPACK's to rounding.
 *   im_inv_transform / im_resample            imutil.c:2040-2244 -- the warp itself runs on the device
 *   Reg_SIFT3D                                reg/reg.c:121-441
 *
 * Host C; the device does detection, description, matching (SIFT3D_nn_match), the resampling and, where it pays, the
 * scoring of the RANSAC hypotheses (s3d_k_ransac_count).
 */
#include <float.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include "s3d_host.h"

/* ---- small dense helpers ------------------------------------------------------------------------ */
int copy_Mat_rm(const Mat_rm *const src, Mat_rm *const dst)
{
    dst->type = src->type;
    dst->num_rows = src->num_rows;
    dst->num_cols = src->num_cols;
    if (resize_Mat_rm(dst)) return SIFT3D_FAILURE;
    if (src->size) memcpy(dst->u.data_double, src->u.data_double, src->size);
    return SIFT3D_SUCCESS;
}

static size_t s3d_elem_size(Mat_rm_type t) { return t == SIFT3D_DOUBLE ? sizeof(double) : t == SIFT3D_FLOAT ? sizeof(float) : sizeof(int); }

/* dim 0: stack vertically, dim 1: side by side (imutil.c:702-770) */
int concat_Mat_rm(const Mat_rm *const src1, const Mat_rm *const src2, Mat_rm *const dst, const int dim)
{
    const int d1[2] = {src1->num_rows, src1->num_cols}, d2[2] = {src2->num_rows, src2->num_cols};
    if (dim < 0 || dim > 1) return SIFT3D_FAILURE;
    if (d1[1 - dim] != d2[1 - dim]) {
        S3D_MSG("concat_Mat_rm: incompatible dimensions: left: [%d x %d] right: [%d x %d] dim: %d \n", d1[0], d1[1], d2[0],
                d2[1], dim);
        return SIFT3D_FAILURE;
    }
    if (src1->type != src2->type) {
        S3D_MSG("concat_Mat_rm: incompatible types \n");
        return SIFT3D_FAILURE;
    }
    dst->type = src1->type;
    dst->num_rows = dim == 0 ? d1[0] + d2[0] : d1[0];
    dst->num_cols = dim == 1 ? d1[1] + d2[1] : d1[1];
    if (resize_Mat_rm(dst)) return SIFT3D_FAILURE;
    const size_t es = s3d_elem_size(dst->type);
    char *out = (char *)dst->u.data_double;
    const char *a = (const char *)src1->u.data_double, *b = (const char *)src2->u.data_double;
    if (dim == 0) {
        if (src1->size) memcpy(out, a, src1->size);
        if (src2->size) memcpy(out + src1->size, b, src2->size);
    } else {
        for (int i = 0; i < d1[0]; i++) {
            memcpy(out + (size_t)i * dst->num_cols * es, a + (size_t)i * d1[1] * es, (size_t)d1[1] * es);
            memcpy(out + ((size_t)i * dst->num_cols + d1[1]) * es, b + (size_t)i * d2[1] * es, (size_t)d2[1] * es);
        }
    }
    return SIFT3D_SUCCESS;
}

/* ---- exported defaults (data symbols of libimutil / libreg that callers link: cli/regSift3D.c:83-84) ---- */
const double SIFT3D_nn_thresh_default = 0.8;        /* reg.c:24 */
const double SIFT3D_err_thresh_default = 5.0;       /* imutil.c:102 */
const int SIFT3D_num_iter_default = 500;            /* imutil.c:103 */

/* ---- Ransac parameters ---------------------------------------------------------------------------- */
void init_Ransac(Ransac *const ran)
{
    ran->err_thresh = SIFT3D_err_thresh_default;
    ran->num_iter = SIFT3D_num_iter_default;
}

int set_err_thresh_Ransac(Ransac *const ran, double err_thresh)
{
    if (err_thresh < 0.0) {
        S3D_MSG("set_err_thresh_Ransac: invalid error threshold: %f \n", err_thresh);
        return SIFT3D_FAILURE;
    }
    ran->err_thresh = err_thresh;
    return SIFT3D_SUCCESS;
}

int set_num_iter_Ransac(Ransac *const ran, int num_iter)
{
    if (num_iter < 1) {
        S3D_MSG("set_num_iter_Ransac: invalid number of iterations: %d \n", num_iter);
        return SIFT3D_FAILURE;
    }
    ran->num_iter = num_iter;
    return SIFT3D_SUCCESS;
}

int copy_Ransac(const Ransac *const src, Ransac *const dst)
{
    return set_num_iter_Ransac(dst, src->num_iter) || set_err_thresh_Ransac(dst, src->err_thresh);
}

/* ---- transforms (only the affine type is functional in the reference as well) ----------------------- */
static int s3d_copy_Affine(const void *const src, void *const dst) { return Affine_set_mat(&((const Affine *)src)->A, (Affine *)dst); }

static void s3d_apply_Affine_xyz(const void *const affine, const double x, const double y, const double z,
                                 double *const xo, double *const yo, double *const zo)
{
    const double *A = ((const Affine *)affine)->A.u.data_double;    /* 3 x 4 */
    *xo = A[0] * x + A[1] * y + A[2] * z + A[3];
    *yo = A[4] * x + A[5] * y + A[6] * z + A[7];
    *zo = A[8] * x + A[9] * y + A[10] * z + A[11];
}

/* rows of mat_in are points; mat_out = (A [p 1]^T)^T per row */
static int s3d_apply_Affine_Mat_rm(const void *const affine, const Mat_rm *const in, Mat_rm *const out)
{
    const Affine *const aff = (const Affine *)affine;
    const int dim = aff->A.num_rows;
    if (in->type != SIFT3D_DOUBLE || in->num_cols != dim) return SIFT3D_FAILURE;
    out->type = SIFT3D_DOUBLE;
    out->num_rows = in->num_rows;
    out->num_cols = dim;
    if (resize_Mat_rm(out)) return SIFT3D_FAILURE;
    const double *A = aff->A.u.data_double;
    for (int i = 0; i < in->num_rows; i++)
        for (int r = 0; r < dim; r++) {
            double acc = A[r * (dim + 1) + dim];
            for (int c = 0; c < dim; c++) acc += A[r * (dim + 1) + c] * in->u.data_double[(size_t)i * dim + c];
            out->u.data_double[(size_t)i * dim + r] = acc;
        }
    return SIFT3D_SUCCESS;
}

static size_t s3d_Affine_get_size(void) { return sizeof(Affine); }
static int s3d_write_Affine(const char *path, const void *const tform) { return write_Mat_rm(path, &((const Affine *)tform)->A); }
static void s3d_cleanup_Affine(void *const affine) { cleanup_Mat_rm(&((Affine *)affine)->A); }

static const Tform_vtable s3d_Affine_vtable = {s3d_copy_Affine, s3d_apply_Affine_xyz, s3d_apply_Affine_Mat_rm,
                                               s3d_Affine_get_size, s3d_write_Affine, s3d_cleanup_Affine};

int init_Affine(Affine *const affine, const int dim)
{
    if (dim < 2) return SIFT3D_FAILURE;
    affine->tform.type = AFFINE;
    affine->tform.vtable = &s3d_Affine_vtable;
    return init_Mat_rm(&affine->A, dim, dim + 1, SIFT3D_DOUBLE, SIFT3D_TRUE) ? SIFT3D_FAILURE : SIFT3D_SUCCESS;
}

int Affine_set_mat(const Mat_rm *const mat, Affine *const affine)
{
    if (mat->num_cols != mat->num_rows + 1 || mat->num_rows < 2) return SIFT3D_FAILURE;
    Mat_rm *const A = &affine->A;
    A->type = SIFT3D_DOUBLE;
    A->num_rows = mat->num_rows;
    A->num_cols = mat->num_cols;
    if (resize_Mat_rm(A)) return SIFT3D_FAILURE;
    const size_t n = (size_t)mat->num_rows * mat->num_cols;
    for (size_t i = 0; i < n; i++)                          /* convert_Mat_rm(..., SIFT3D_DOUBLE) */
        A->u.data_double[i] = mat->type == SIFT3D_DOUBLE ? mat->u.data_double[i]
                            : mat->type == SIFT3D_FLOAT ? (double)mat->u.data_float[i] : (double)mat->u.data_int[i];
    return SIFT3D_SUCCESS;
}

int init_tform(void *const tform, const tform_type type)
{
    switch (type) {
    case TPS: puts("init_tform: TPS not yet implemented \n"); return SIFT3D_FAILURE;
    case AFFINE: return init_Affine((Affine *)tform, IM_NDIMS) ? SIFT3D_FAILURE : SIFT3D_SUCCESS;
    default: puts("init_tform: unrecognized type \n"); return SIFT3D_FAILURE;
    }
}

tform_type tform_get_type(const void *const tform) { return ((const Tform *)tform)->type; }
size_t tform_get_size(const void *const tform) { return ((const Tform *)tform)->vtable->get_size(); }
size_t tform_type_get_size(const tform_type type) { return type == AFFINE ? sizeof(Affine) : type == TPS ? sizeof(Tps) : 0; }
int copy_tform(const void *const src, void *const dst) { return ((const Tform *)src)->vtable->copy(src, dst); }
int write_tform(const char *path, const void *const tform) { return ((const Tform *)tform)->vtable->write(path, tform); }
void cleanup_tform(void *const tform)
{
    if (tform != NULL && ((Tform *)tform)->vtable != NULL) ((Tform *)tform)->vtable->cleanup(tform);
}
void apply_tform_xyz(const void *const tform, const double x_in, const double y_in, const double z_in, double *const x_out,
                     double *const y_out, double *const z_out)
{
    ((const Tform *)tform)->vtable->apply_xyz(tform, x_in, y_in, z_in, x_out, y_out, z_out);
}

/* ---- solvers -------------------------------------------------------------------------------------- */
/* In-place LU with partial pivoting of the n x n row-major matrix a (n <= 8); returns -1 if a pivot is 0 */
static int s3d_lu(double *a, int n, int *piv)
{
    for (int k = 0; k < n; k++) {
        int p = k;
        for (int i = k + 1; i < n; i++)
            if (fabs(a[i * n + k]) > fabs(a[p * n + k])) p = i;
        piv[k] = p;
        if (a[p * n + k] == 0.0) return -1;
        if (p != k)
            for (int j = 0; j < n; j++) { const double t = a[k * n + j]; a[k * n + j] = a[p * n + j]; a[p * n + j] = t; }
        for (int i = k + 1; i < n; i++) {
            a[i * n + k] /= a[k * n + k];
            for (int j = k + 1; j < n; j++) a[i * n + j] -= a[i * n + k] * a[k * n + j];
        }
    }
    return 0;
}

static void s3d_lu_solve(const double *lu, const int *piv, int n, double *b /* n x nrhs, row major */, int nrhs)
{
    for (int k = 0; k < n; k++)
        if (piv[k] != k)
            for (int j = 0; j < nrhs; j++) { const double t = b[k * nrhs + j]; b[k * nrhs + j] = b[piv[k] * nrhs + j]; b[piv[k] * nrhs + j] = t; }
    for (int i = 1; i < n; i++)
        for (int k = 0; k < i; k++)
            for (int j = 0; j < nrhs; j++) b[i * nrhs + j] -= lu[i * n + k] * b[k * nrhs + j];
    for (int i = n - 1; i >= 0; i--)
        for (int j = 0; j < nrhs; j++) {
            double acc = b[i * nrhs + j];
            for (int k = i + 1; k < n; k++) acc -= lu[i * n + k] * b[k * nrhs + j];
            b[i * nrhs + j] = acc / lu[i * n + i];
        }
}

static double s3d_norm1(const double *a, int n)
{
    double best = 0.0;
    for (int j = 0; j < n; j++) {
        double s = 0.0;
        for (int i = 0; i < n; i++) s += fabs(a[i * n + j]);
        if (s > best) best = s;
    }
    return best;
}

/* A X = B for square A (n <= 8).  SIFT3D_SINGULAR when 1 / (|A|_1 |A^-1|_1) < 100 eps, as solve_Mat_rm does
 * with limit < 0. */
static int s3d_solve_square(const double *A, int n, const double *B, int nrhs, double *X)
{
    double lu[64], inv[64];
    int piv[8];
    if (n > 8) return SIFT3D_FAILURE;
    memcpy(lu, A, sizeof(double) * n * n);
    const double anorm = s3d_norm1(A, n);
    if (s3d_lu(lu, n, piv)) return SIFT3D_SINGULAR;
    memset(inv, 0, sizeof(inv));
    for (int i = 0; i < n; i++) inv[i * n + i] = 1.0;
    s3d_lu_solve(lu, piv, n, inv, n);
    const double inorm = s3d_norm1(inv, n);
    const double rcond = (anorm == 0.0 || inorm == 0.0) ? 0.0 : (1.0 / anorm) / inorm;
    if (!(rcond >= 100.0 * DBL_EPSILON)) return SIFT3D_SINGULAR;
    memcpy(X, B, sizeof(double) * n * nrhs);
    s3d_lu_solve(lu, piv, n, X, nrhs);
    return SIFT3D_SUCCESS;
}

/* min-norm least squares X = argmin |A X - B| for A m x n (n <= 8, m >= 1) through a one-sided Jacobi SVD
 * A = U S V^T; singular values below eps * s_max are treated as zero (dgelss with rcond = -1). */
static int s3d_solve_ls(const double *A, int m, int n, const double *B, int nrhs, double *X)
{
    if (n > 8) return SIFT3D_FAILURE;
    double *U = (double *)malloc(sizeof(double) * (size_t)m * n);
    double V[64], s[8];
    if (U == NULL) return SIFT3D_FAILURE;
    memcpy(U, A, sizeof(double) * (size_t)m * n);
    memset(V, 0, sizeof(V));
    for (int i = 0; i < n; i++) V[i * n + i] = 1.0;
    for (int sweep = 0; sweep < 60; sweep++) {
        double off = 0.0;
        for (int p = 0; p < n - 1; p++)
            for (int q = p + 1; q < n; q++) {
                double alpha = 0.0, beta = 0.0, gamma = 0.0;
                for (int i = 0; i < m; i++) {
                    alpha += U[(size_t)i * n + p] * U[(size_t)i * n + p];
                    beta += U[(size_t)i * n + q] * U[(size_t)i * n + q];
                    gamma += U[(size_t)i * n + p] * U[(size_t)i * n + q];
                }
                if (gamma == 0.0) continue;
                const double rel = fabs(gamma) / sqrt(alpha * beta);
                if (rel > off) off = rel;
                if (rel < 1e-16) continue;
                const double zeta = (beta - alpha) / (2.0 * gamma);
                const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                const double c = 1.0 / sqrt(1.0 + t * t), sn = c * t;
                for (int i = 0; i < m; i++) {
                    const double up = U[(size_t)i * n + p], uq = U[(size_t)i * n + q];
                    U[(size_t)i * n + p] = c * up - sn * uq;
                    U[(size_t)i * n + q] = sn * up + c * uq;
                }
                for (int i = 0; i < n; i++) {
                    const double vp = V[i * n + p], vq = V[i * n + q];
                    V[i * n + p] = c * vp - sn * vq;
                    V[i * n + q] = sn * vp + c * vq;
                }
            }
        if (off < 1e-15) break;
    }
    double smax = 0.0;
    for (int j = 0; j < n; j++) {
        double ss = 0.0;
        for (int i = 0; i < m; i++) ss += U[(size_t)i * n + j] * U[(size_t)i * n + j];
        s[j] = sqrt(ss);
        if (s[j] > smax) smax = s[j];
    }
    /* X = V diag(1/s) (U/s)^T B */
    for (int r = 0; r < n; r++)
        for (int k = 0; k < nrhs; k++) X[r * nrhs + k] = 0.0;
    for (int j = 0; j < n; j++) {
        if (!(s[j] > DBL_EPSILON * smax)) continue;
        for (int k = 0; k < nrhs; k++) {
            double proj = 0.0;
            for (int i = 0; i < m; i++) proj += U[(size_t)i * n + j] * B[(size_t)i * nrhs + k];
            proj /= s[j] * s[j];
            for (int r = 0; r < n; r++) X[r * nrhs + k] += V[r * n + j] * proj;
        }
    }
    free(U);
    return SIFT3D_SUCCESS;
}

/* affine from correspondences: [ref 1] X = src, A = X^T (solve_system + make_affine_matrix, imutil.c:4413-4520) */
static int s3d_solve_affine(const double *src, const double *ref, int npts, int dim, Affine *aff)
{
    const int n = dim + 1;
    double X[8 * 8];
    double *sys = (double *)malloc(sizeof(double) * (size_t)npts * n);
    if (sys == NULL) return SIFT3D_FAILURE;
    for (int i = 0; i < npts; i++) {
        for (int j = 0; j < dim; j++) sys[(size_t)i * n + j] = ref[(size_t)i * dim + j];
        sys[(size_t)i * n + dim] = 1.0;
    }
    const int rc = npts == n ? s3d_solve_square(sys, n, src, dim, X) : s3d_solve_ls(sys, npts, n, src, dim, X);
    free(sys);
    if (rc != SIFT3D_SUCCESS) return rc;
    Mat_rm *const A = &aff->A;
    A->type = SIFT3D_DOUBLE; A->num_rows = dim; A->num_cols = n;
    if (resize_Mat_rm(A)) return SIFT3D_FAILURE;
    for (int r = 0; r < dim; r++)
        for (int c = 0; c < n; c++) A->u.data_double[r * n + c] = X[c * dim + r];
    return SIFT3D_SUCCESS;
}

/* ---- thin-plate spline (imtypes.h:380-385; imutil.c:2676-2805, 4213-4235, 4727-4744) ------------------------------------
 * The reference has the struct, its allocation and the two apply functions; copy, write and the fit are this library's. */
static int s3d_tps_is_3d(const Tps *const t)
{
    const int n = t->kp_src.num_rows;
    return t->dim == IM_NDIMS && n >= 0 && t->kp_src.type == SIFT3D_DOUBLE && t->params.type == SIFT3D_DOUBLE &&
           t->params.num_rows == IM_NDIMS && t->params.num_cols == n + IM_NDIMS + 1 && t->params.u.data_double != NULL &&
           (n == 0 || (t->kp_src.num_cols == IM_NDIMS && t->kp_src.u.data_double != NULL));
}

/* the reference's expression and summation order; this file is compiled without contraction */
static void s3d_apply_Tps_xyz(const void *const tps, const double x_in, const double y_in, const double z_in, double *const x_out,
                              double *const y_out, double *const z_out)
{
    const Tps *const t = (const Tps *)tps;
    const int n_ctrl = t->kp_src.num_rows;
    const double *const c = t->kp_src.u.data_double, *const px = t->params.u.data_double, *const py = px + t->params.num_cols,
                 *const pz = py + t->params.num_cols;
    double temp_x = 0.0, temp_y = 0.0, temp_z = 0.0;
    for (int n = 0; n < n_ctrl; n++) {
        const double x_c = c[(size_t)n * 3], y_c = c[(size_t)n * 3 + 1], z_c = c[(size_t)n * 3 + 2];
        const double r_sq = (x_in - x_c) * (x_in - x_c) + (y_in - y_c) * (y_in - y_c) + (z_in - z_c) * (z_in - z_c);
        const double U = r_sq == 0 ? 0.0 : r_sq * log(r_sq);
        temp_x += U * px[n];
        temp_y += U * py[n];
        temp_z += U * pz[n];
    }
    temp_x += px[n_ctrl]; temp_x += px[n_ctrl + 1] * x_in; temp_x += px[n_ctrl + 2] * y_in; temp_x += px[n_ctrl + 3] * z_in;
    temp_y += py[n_ctrl]; temp_y += py[n_ctrl + 1] * x_in; temp_y += py[n_ctrl + 2] * y_in; temp_y += py[n_ctrl + 3] * z_in;
    temp_z += pz[n_ctrl]; temp_z += pz[n_ctrl + 1] * x_in; temp_z += pz[n_ctrl + 2] * y_in; temp_z += pz[n_ctrl + 3] * z_in;
    *x_out = temp_x; *y_out = temp_y; *z_out = temp_z;
}

/* in: 3 x num_pts, one point per COLUMN (the reference's format for this call); out likewise, resized here */
static int s3d_apply_Tps_Mat_rm(const void *const tps, const Mat_rm *const in, Mat_rm *const out)
{
    const Tps *const t = (const Tps *)tps;
    if (!s3d_tps_is_3d(t) || in->type != SIFT3D_DOUBLE || in->num_rows < IM_NDIMS) return SIFT3D_FAILURE;
    const int num_pts = in->num_cols;
    out->type = SIFT3D_DOUBLE;
    out->num_rows = IM_NDIMS;
    out->num_cols = num_pts;
    if (resize_Mat_rm(out)) return SIFT3D_FAILURE;
    for (int q = 0; q < num_pts; q++)
        s3d_apply_Tps_xyz(tps, in->u.data_double[q], in->u.data_double[(size_t)num_pts + q],
                          in->u.data_double[2 * (size_t)num_pts + q], out->u.data_double + q,
                          out->u.data_double + (size_t)num_pts + q, out->u.data_double + 2 * (size_t)num_pts + q);
    return SIFT3D_SUCCESS;
}

static int s3d_copy_Tps(const void *const src, void *const dst)
{
    const Tps *const s = (const Tps *)src;
    Tps *const d = (Tps *)dst;
    if (copy_Mat_rm(&s->params, &d->params) || copy_Mat_rm(&s->kp_src, &d->kp_src)) return SIFT3D_FAILURE;
    d->dim = s->dim;
    return SIFT3D_SUCCESS;
}

static size_t s3d_Tps_get_size(void) { return sizeof(Tps); }

/* N + 4 rows x 6 columns: [c_x c_y c_z w_x w_y w_z] per control point, then [0 0 0 a_x a_y a_z] for the constant and the
 * x, y, z coefficients */
static int s3d_write_Tps(const char *path, const void *const tform)
{
    const Tps *const t = (const Tps *)tform;
    Mat_rm m;
    if (!s3d_tps_is_3d(t)) {
        S3D_MSG("write_Tps: only 3-D splines can be written \n");
        return SIFT3D_FAILURE;
    }
    const int n = t->kp_src.num_rows, cols = t->params.num_cols;
    if (init_Mat_rm(&m, n + 4, 6, SIFT3D_DOUBLE, SIFT3D_TRUE)) return SIFT3D_FAILURE;
    for (int i = 0; i < n + 4; i++)
        for (int k = 0; k < 3; k++) {
            if (i < n) m.u.data_double[(size_t)i * 6 + k] = t->kp_src.u.data_double[(size_t)i * 3 + k];
            m.u.data_double[(size_t)i * 6 + 3 + k] = t->params.u.data_double[(size_t)k * cols + i];
        }
    const int rc = write_Mat_rm(path, &m);
    cleanup_Mat_rm(&m);
    return rc;
}

static void s3d_cleanup_Tps(void *const tps)
{
    cleanup_Mat_rm(&((Tps *)tps)->params);
    cleanup_Mat_rm(&((Tps *)tps)->kp_src);
}

const Tform_vtable Tps_vtable = {s3d_copy_Tps, s3d_apply_Tps_xyz, s3d_apply_Tps_Mat_rm, s3d_Tps_get_size, s3d_write_Tps,
                                 s3d_cleanup_Tps};

int init_Tps(Tps *tps, int dim, int terms)
{
    if (dim < 2) return SIFT3D_FAILURE;
    tps->tform.type = TPS;
    tps->tform.vtable = &Tps_vtable;
    if (init_Mat_rm(&tps->params, dim, terms, SIFT3D_DOUBLE, SIFT3D_TRUE)) return SIFT3D_FAILURE;
    if (init_Mat_rm(&tps->kp_src, terms - dim - 1, dim, SIFT3D_DOUBLE, SIFT3D_TRUE)) return SIFT3D_FAILURE;
    tps->dim = dim;
    return SIFT3D_SUCCESS;
}

int resize_Tps(Tps *tps, int num_pts, int dim)
{
    tps->params.num_cols = num_pts + dim + 1;
    tps->params.num_rows = dim;
    tps->kp_src.num_rows = num_pts;
    tps->kp_src.num_cols = dim;
    if (resize_Mat_rm(&tps->params) || resize_Mat_rm(&tps->kp_src)) return SIFT3D_FAILURE;
    tps->dim = dim;
    return SIFT3D_SUCCESS;
}

/* 1 when the points (n x 3) span no volume: the 4 x 4 Gram matrix of [1 x y z], coordinates centred and scaled to [-1, 1],
 * fails solve_Mat_rm's condition test (reciprocal condition below 100 eps).  With distinct points this is the only way the
 * spline system is singular: r2 log r2 is conditionally positive definite of order 2. */
static int s3d_tps_points_flat(const double *p, int n)
{
    double lo[3], hi[3], G[16], I4[16], X[16], scale = 0.0;
    for (int k = 0; k < 3; k++) lo[k] = hi[k] = p[k];
    for (int i = 1; i < n; i++)
        for (int k = 0; k < 3; k++) {
            const double v = p[(size_t)i * 3 + k];
            if (v < lo[k]) lo[k] = v;
            if (v > hi[k]) hi[k] = v;
        }
    for (int k = 0; k < 3; k++)
        if (hi[k] - lo[k] > scale) scale = hi[k] - lo[k];
    if (!(scale > 0.0) || !(scale <= DBL_MAX)) return 1;
    memset(G, 0, sizeof(G));
    memset(I4, 0, sizeof(I4));
    for (int i = 0; i < n; i++) {
        double q[4] = {1.0, 0.0, 0.0, 0.0};
        for (int k = 0; k < 3; k++) q[k + 1] = (2.0 * p[(size_t)i * 3 + k] - (lo[k] + hi[k])) / scale;
        for (int a = 0; a < 4; a++)
            for (int b = 0; b < 4; b++) G[a * 4 + b] += q[a] * q[b];
    }
    for (int a = 0; a < 4; a++) I4[a * 4 + a] = 1.0;
    return s3d_solve_square(G, 4, I4, 4, X) != SIFT3D_SUCCESS;
}

int sift3d_amd_fit_tps(const Mat_rm *const src, const Mat_rm *const ref, double lambda, Tps *const tps)
{
    if (src == NULL || ref == NULL || tps == NULL) {
        s3d_api_set_error("sift3d_amd_fit_tps: NULL argument");
        return SIFT3D_FAILURE;
    }
    if (src->type != SIFT3D_DOUBLE || ref->type != SIFT3D_DOUBLE) {
        s3d_api_set_error("sift3d_amd_fit_tps: all matrices must have type double");
        return SIFT3D_FAILURE;
    }
    if (src->num_cols != IM_NDIMS || ref->num_cols != IM_NDIMS || src->num_rows != ref->num_rows || src->num_rows < 0) {
        s3d_api_set_error("sift3d_amd_fit_tps: src and ref must both be n x %d, one point per row. Provided: [%d x %d] and "
                          "[%d x %d]", IM_NDIMS, src->num_rows, src->num_cols, ref->num_rows, ref->num_cols);
        return SIFT3D_FAILURE;
    }
    if (!(lambda >= 0.0) || lambda > DBL_MAX) {
        s3d_api_set_error("sift3d_amd_fit_tps: lambda must be a finite number >= 0. Provided: %f", lambda);
        return SIFT3D_FAILURE;
    }
    const int nin = src->num_rows;
    int rc = SIFT3D_FAILURE, n = 0;
    double *R = (double *)malloc(sizeof(double) * 3 * (size_t)(nin + 1)), *S = (double *)malloc(sizeof(double) * 3 * (size_t)(nin + 1));
    double *M = NULL, *B = NULL;
    int *piv = NULL;
    if (R == NULL || S == NULL) goto nomem;
    for (int i = 0; i < nin; i++) {                        /* rows whose ref point equals an earlier row's are dropped */
        const double *r = ref->u.data_double + (size_t)i * 3;
        int dup = 0;
        for (int j = 0; j < n && !dup; j++) dup = R[(size_t)j * 3] == r[0] && R[(size_t)j * 3 + 1] == r[1] && R[(size_t)j * 3 + 2] == r[2];
        if (dup) continue;
        memcpy(R + (size_t)n * 3, r, sizeof(double) * 3);
        memcpy(S + (size_t)n * 3, src->u.data_double + (size_t)i * 3, sizeof(double) * 3);
        n++;
    }
    if (n < IM_NDIMS + 1) {
        s3d_api_set_error("sift3d_amd_fit_tps: a spline needs at least %d distinct points. Provided: %d (%d rows)", IM_NDIMS + 1, n, nin);
        goto done;
    }
    if (s3d_tps_points_flat(R, n)) {
        s3d_api_set_error("sift3d_amd_fit_tps: singular system: the %d reference points lie in one plane (or are not finite)", n);
        goto done;
    }
    const int m = n + 4;
    M = (double *)calloc((size_t)m * m, sizeof(double));
    B = (double *)calloc((size_t)m * 3, sizeof(double));
    piv = (int *)malloc(sizeof(int) * (size_t)m);
    if (M == NULL || B == NULL || piv == NULL) goto nomem;
    for (int i = 0; i < n; i++) {
        const double *ri = R + (size_t)i * 3;
        for (int j = 0; j < n; j++) {
            const double *rj = R + (size_t)j * 3;
            const double r_sq = (ri[0] - rj[0]) * (ri[0] - rj[0]) + (ri[1] - rj[1]) * (ri[1] - rj[1]) + (ri[2] - rj[2]) * (ri[2] - rj[2]);
            M[(size_t)i * m + j] = r_sq == 0 ? 0.0 : r_sq * log(r_sq);
        }
        M[(size_t)i * m + i] += lambda;
        M[(size_t)i * m + n] = M[(size_t)n * m + i] = 1.0;
        for (int k = 0; k < 3; k++) {
            M[(size_t)i * m + n + 1 + k] = M[(size_t)(n + 1 + k) * m + i] = ri[k];
            B[(size_t)i * 3 + k] = S[(size_t)i * 3 + k];
        }
    }
    int finite = s3d_lu(M, m, piv) == 0;
    if (finite) {
        s3d_lu_solve(M, piv, m, B, 3);
        for (size_t i = 0; i < (size_t)m * 3; i++) finite &= B[i] - B[i] == 0.0;
    }
    if (!finite) {
        s3d_api_set_error("sift3d_amd_fit_tps: singular system (%d points, lambda %g)", n, lambda);
        goto done;
    }
    if (resize_Tps(tps, n, IM_NDIMS)) goto nomem;
    tps->tform.type = TPS;
    tps->tform.vtable = &Tps_vtable;
    memcpy(tps->kp_src.u.data_double, R, sizeof(double) * 3 * (size_t)n);
    for (int k = 0; k < 3; k++)
        for (int j = 0; j < m; j++) tps->params.u.data_double[(size_t)k * m + j] = B[(size_t)j * 3 + k];
    rc = SIFT3D_SUCCESS;
    goto done;
nomem:
    s3d_api_set_error("sift3d_amd_fit_tps: out of memory (%d points)", nin);
done:
    free(R); free(S); free(M); free(B); free(piv);
    return rc;
}

/* ---- RANSAC --------------------------------------------------------------------------------------- */
/* k distinct integers of 0..n-1 by a partial Fisher-Yates shuffle on libc rand(), call for call the
 * reference's n_choose_k: same seed, same glibc => same samples.  scratch holds the identity on entry and again on
 * return: the reference refills it on every draw, here the k swaps are undone instead (an n-long fill per draw is the
 * largest host term once the scoring runs on the device); the picks are the same. */
static int s3d_n_choose_k(int n, int k, int *out /* k */, int *scratch /* n */)
{
    int js[8];
    if (n < k || k < 1 || k > 8) return SIFT3D_FAILURE;
    for (int i = 0; i < k; i++) {
        const int j = i + rand() % (n - i);
        const int t = scratch[i]; scratch[i] = scratch[j]; scratch[j] = t;
        js[i] = j;
    }
    memcpy(out, scratch, sizeof(int) * k);
    for (int i = k - 1; i >= 0; i--) {
        const int t = scratch[i]; scratch[i] = scratch[js[i]]; scratch[js[i]] = t;
    }
    return SIFT3D_SUCCESS;
}

/* -- where the hypotheses are scored (sift3d_amd.h: sift3d_amd_set_ransac_device) -- */
/* AUTO scores on the device from this many affine applications (npts * num_iter) on.  profiles/ransac_cost.txt, part 2, has
 * the measured grid this is taken from: the smallest product at which the device form beat the host form by more than the
 * host form's own min-max spread was 200 x 500 = 100 000 (0.236 against 0.304 ms), rounded up to a power of two.  Below it
 * (60 x 500) one allocation, upload, launch and download cost more than the host loop. */
#define S3D_RANSAC_AUTO_MIN_WORK (1L << 17)

#define S3D_RANSAC_MODE_UNSET (-2)
static int g_ransac_mode = S3D_RANSAC_MODE_UNSET;      /* process-wide */
static int g_ransac_profile;
static __thread int g_ransac_last_path;
static __thread double g_ransac_last_ms;

static int s3d_ransac_mode_ok(long m) { return m == SIFT3D_AMD_RANSAC_AUTO || m == SIFT3D_AMD_RANSAC_HOST || m == SIFT3D_AMD_RANSAC_DEVICE; }

int sift3d_amd_get_ransac_device(void)
{
    int m = __atomic_load_n(&g_ransac_mode, __ATOMIC_RELAXED);
    if (m == S3D_RANSAC_MODE_UNSET) {                      /* no call yet: SIFT3D_RANSAC_DEVICE of the environment, read once */
        const char *e = getenv("SIFT3D_RANSAC_DEVICE");
        char *end = NULL;
        const long v = e != NULL && *e ? strtol(e, &end, 10) : SIFT3D_AMD_RANSAC_AUTO;
        m = (end == NULL || *end == '\0') && s3d_ransac_mode_ok(v) ? (int)v : SIFT3D_AMD_RANSAC_AUTO;
        int unset = S3D_RANSAC_MODE_UNSET;
        if (!__atomic_compare_exchange_n(&g_ransac_mode, &unset, m, 0, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) m = unset;
    }
    return m;
}

int sift3d_amd_set_ransac_device(int mode)
{
    if (!s3d_ransac_mode_ok(mode)) {
        s3d_api_set_error("sift3d_amd_set_ransac_device: the mode must be -1 (auto), 0 (host) or 1 (device). Provided: %d", mode);
        return SIFT3D_FAILURE;
    }
    __atomic_store_n(&g_ransac_mode, mode, __ATOMIC_RELAXED);
    return SIFT3D_SUCCESS;
}

int sift3d_amd_ransac_last_path(void) { return g_ransac_last_path; }
void sift3d_amd_set_ransac_profile(int on) { __atomic_store_n(&g_ransac_profile, on != 0, __ATOMIC_RELAXED); }
double sift3d_amd_ransac_last_device_ms(void) { return g_ransac_last_ms; }

/* the consensus set of one model: tform_err_sq (imutil.c:4527-4552) over every match, s3d_apply_Affine_xyz's operation
 * order.  Returns its length; the members go to cset unless that is NULL.  (s3d_k_ransac_count computes the same length.) */
static int s3d_ransac_consensus(const double *src, const double *ref, int npts, const double *A, double thr2, int *cset)
{
    int len = 0;
    for (int i = 0; i < npts; i++) {
        const double *r = ref + (size_t)i * IM_NDIMS, *s = src + (size_t)i * IM_NDIMS;
        const double xo = A[0] * r[0] + A[1] * r[1] + A[2] * r[2] + A[3];
        const double yo = A[4] * r[0] + A[5] * r[1] + A[6] * r[2] + A[7];
        const double zo = A[8] * r[0] + A[9] * r[1] + A[10] * r[2] + A[11];
        const double e = (s[0] - xo) * (s[0] - xo) + (s[1] - yo) * (s[1] - yo) + (s[2] - zo) * (s[2] - zo);
        if (e > thr2) continue;
        if (cset != NULL) cset[len] = i;
        len++;
    }
    return len;
}

/* the device side of one find_tform_ransac call: one allocation holding the matches, a batch of models and their counts */
typedef struct {
    void *d_buf, *ev0, *ev1;
    double *d_src, *d_ref, *d_models;
    int *d_counts;
    double ms;
} s3d_ransac_dev;

static void s3d_ransac_dev_close(s3d_ransac_dev *d)
{
    if (d->ev0) s3d_rt_event_destroy(d->ev0);
    if (d->ev1) s3d_rt_event_destroy(d->ev1);
    s3d_rt_free(d->d_buf);
    memset(d, 0, sizeof(*d));
}

static int s3d_ransac_dev_lap(s3d_ransac_dev *d)          /* adds ev0 -> ev1 to the call's device time */
{
    float ms = 0.0f;
    if (d->ev0 == NULL) return 0;
    if (s3d_rt_event_elapsed_ms(d->ev0, d->ev1, &ms)) return -1;
    d->ms += ms;
    return 0;
}

static int s3d_ransac_dev_open(s3d_ransac_dev *d, const double *src, const double *ref, int npts)
{
    const size_t pts = sizeof(double) * IM_NDIMS * (size_t)npts, mod = sizeof(double) * 12 * S3D_RANSAC_BATCH;
    memset(d, 0, sizeof(*d));
    if (s3d_rt_malloc(&d->d_buf, 2 * pts + mod + sizeof(int) * S3D_RANSAC_BATCH)) return -1;
    d->d_src = (double *)d->d_buf;
    d->d_ref = (double *)((char *)d->d_buf + pts);
    d->d_models = (double *)((char *)d->d_buf + 2 * pts);
    d->d_counts = (int *)((char *)d->d_buf + 2 * pts + mod);
    if (__atomic_load_n(&g_ransac_profile, __ATOMIC_RELAXED) &&
        (s3d_rt_event_create(&d->ev0) || s3d_rt_event_create(&d->ev1) || s3d_rt_event_record(d->ev0, NULL)))
        return -1;
    if (s3d_rt_h2d(d->d_src, src, pts, NULL) || s3d_rt_h2d(d->d_ref, ref, pts, NULL)) return -1;
    if (d->ev1 && s3d_rt_event_record(d->ev1, NULL)) return -1;
    return s3d_ransac_dev_lap(d);
}

static int s3d_ransac_dev_score(s3d_ransac_dev *d, const double *models, int nb, int npts, double thr2, int *counts)
{
    if (d->ev0 && s3d_rt_event_record(d->ev0, NULL)) return -1;
    if (s3d_rt_h2d(d->d_models, models, sizeof(double) * 12 * (size_t)nb, NULL) ||
        s3d_k_ransac_count(d->d_src, d->d_ref, (uint32_t)npts, d->d_models, (uint32_t)nb, thr2, d->d_counts, NULL) ||
        s3d_rt_d2h(counts, d->d_counts, sizeof(int) * (size_t)nb, NULL))
        return -1;
    if (d->ev1 && s3d_rt_event_record(d->ev1, NULL)) return -1;
    if (s3d_rt_sync(NULL)) return -1;
    return s3d_ransac_dev_lap(d);
}

/* Three phases per batch of at most S3D_RANSAC_BATCH iterations: draw the batch's models (today's loop head: the same rand()
 * calls in the same order -- scoring consumes none), score them (host loop or s3d_k_ransac_count: the same integers), and keep
 * the first model holding the largest count so far (`>` is strict, as the reference's len > len_best).  The winner's consensus
 * set is then recomputed on the host for that single model, and the tail is the reference's. */
int find_tform_ransac(const Ransac *const ran, const Mat_rm *const src, const Mat_rm *const ref, void *const tform)
{
    g_ransac_last_path = 0;
    g_ransac_last_ms = 0.0;
    if (tform_get_type(tform) != AFFINE) {
        puts("find_tform_ransac: unsupported transformation type \n");
        return SIFT3D_FAILURE;
    }
    if (src->type != SIFT3D_DOUBLE || ref->type != SIFT3D_DOUBLE) {
        puts("ransac: all matrices must have type double \n");
        return SIFT3D_FAILURE;
    }
    if (src->num_rows != ref->num_rows || src->num_cols != ref->num_cols) {
        puts("ransac: src and ref must have the same dimensions \n");
        return SIFT3D_FAILURE;
    }
    const int dim = ((Affine *)tform)->A.num_rows, nterms = dim + 1, npts = src->num_rows;
    if (dim != IM_NDIMS || src->num_cols != IM_NDIMS) return SIFT3D_FAILURE;
    if (npts < nterms) {
        printf("Not enough matched points \n");
        return SIFT3D_FAILURE;
    }
    const double *const S = src->u.data_double, *const R = ref->u.data_double;
    const double thr2 = ran->err_thresh * ran->err_thresh;
    /* the scoring path */
    const int mode = sift3d_amd_get_ransac_device();
    int on_dev = 0, ndev = 0;
    if (mode == SIFT3D_AMD_RANSAC_DEVICE ||
        (mode == SIFT3D_AMD_RANSAC_AUTO && (double)npts * (double)ran->num_iter >= (double)S3D_RANSAC_AUTO_MIN_WORK)) {
        on_dev = s3d_rt_device_count(&ndev) == 0 && ndev > 0;
        if (!on_dev && mode == SIFT3D_AMD_RANSAC_DEVICE) {
            s3d_api_set_error("find_tform_ransac: scoring on the device was asked for (SIFT3D_AMD_RANSAC_DEVICE) but no device "
                              "is usable (%d found): %s", ndev, s3d_rt_last_error());
            return SIFT3D_FAILURE;
        }
    }
    int rc = SIFT3D_FAILURE, len_best = 0;
    Affine cur;
    s3d_ransac_dev dev;
    memset(&dev, 0, sizeof(dev));
    int *best = (int *)malloc(sizeof(int) * npts), *scratch = (int *)malloc(sizeof(int) * npts);
    int *counts = (int *)malloc(sizeof(int) * S3D_RANSAC_BATCH);
    double *models = (double *)malloc(sizeof(double) * 12 * S3D_RANSAC_BATCH);
    double *ps = NULL, *pr = NULL, best_model[12];
    if (init_Affine(&cur, dim)) {
        free(best); free(scratch); free(counts); free(models);
        return SIFT3D_FAILURE;
    }
    if (!best || !scratch || !counts || !models) goto done;
    for (int i = 0; i < npts; i++) scratch[i] = i;
    if (on_dev && s3d_ransac_dev_open(&dev, S, R, npts)) {
        s3d_ransac_dev_close(&dev);
        if (mode == SIFT3D_AMD_RANSAC_DEVICE) goto dev_failed;
        on_dev = 0;                                        /* AUTO: the host loop gives the identical result */
    }
    g_ransac_last_path = on_dev;
    for (int it0 = 0; it0 < ran->num_iter; it0 += S3D_RANSAC_BATCH) {
        int nb = ran->num_iter - it0 < S3D_RANSAC_BATCH ? ran->num_iter - it0 : S3D_RANSAC_BATCH, draw_failed = 0, improved = 0;
        for (int b = 0; b < nb; b++) {                     /* draw */
            int pick[8], ret;
            double s4[8 * IM_NDIMS], r4[8 * IM_NDIMS];
            do {                                           /* singular samples are redrawn (imutil.c:4797-4800) */
                if ((ret = s3d_n_choose_k(npts, nterms, pick, scratch)) != SIFT3D_SUCCESS) break;
                for (int i = 0; i < nterms; i++)
                    for (int j = 0; j < dim; j++) {
                        s4[i * dim + j] = S[(size_t)pick[i] * dim + j];
                        r4[i * dim + j] = R[(size_t)pick[i] * dim + j];
                    }
                ret = s3d_solve_affine(s4, r4, nterms, dim, &cur);
            } while (ret == SIFT3D_SINGULAR);
            if (ret != SIFT3D_SUCCESS) {                   /* a hard error: the iterations before this one still count, as */
                nb = b;                                    /* in the one-by-one loop, which had scored them by now */
                draw_failed = 1;
                break;
            }
            memcpy(models + (size_t)b * 12, cur.A.u.data_double, sizeof(double) * 12);
        }
        if (on_dev && nb > 0 && s3d_ransac_dev_score(&dev, models, nb, npts, thr2, counts)) {   /* score */
            s3d_ransac_dev_close(&dev);
            if (mode == SIFT3D_AMD_RANSAC_DEVICE) goto dev_failed;
            on_dev = g_ransac_last_path = 0;               /* AUTO: this batch and the rest on the host */
        }
        if (!on_dev)
            for (int b = 0; b < nb; b++) counts[b] = s3d_ransac_consensus(S, R, npts, models + (size_t)b * 12, thr2, NULL);
        for (int b = 0; b < nb; b++)                       /* select */
            if (counts[b] > len_best) {
                len_best = counts[b];
                memcpy(best_model, models + (size_t)b * 12, sizeof(best_model));
                improved = 1;
            }
        g_ransac_last_ms = dev.ms;
        if (improved) {                                    /* the best sample's model so far is left in tform, whatever follows */
            if (cur.A.u.data_double == NULL || cur.A.num_rows != dim || cur.A.num_cols != nterms) goto done;
            memcpy(cur.A.u.data_double, best_model, sizeof(best_model));
            if (copy_tform(&cur, tform)) goto done;
        }
        if (draw_failed) goto done;
    }
    if (len_best < 5) {                                    /* min_num_inliers, imutil.c:4783 */
        puts("find_tform_ransac: No good model was found! \n");
        goto done;
    }
    if (s3d_ransac_consensus(S, R, npts, best_model, thr2, best) != len_best) {
        /* the two scoring paths compute the same integers: this is a defect (of the device's counts), not an input's property */
        s3d_api_set_error("find_tform_ransac: the winner's consensus set, recomputed on the host, does not have the %d members it "
                          "was scored with (%s path)", len_best, g_ransac_last_path ? "device" : "host");
        goto done;
    }
    /* least-squares refinement on the consensus set (SIFT3D_RANSAC_REFINE, imutil.c:4840-4856) */
    ps = (double *)malloc(sizeof(double) * (size_t)len_best * dim);
    pr = (double *)malloc(sizeof(double) * (size_t)len_best * dim);
    if (!ps || !pr) goto done;
    for (int i = 0; i < len_best; i++)
        for (int j = 0; j < dim; j++) {
            ps[(size_t)i * dim + j] = S[(size_t)best[i] * dim + j];
            pr[(size_t)i * dim + j] = R[(size_t)best[i] * dim + j];
        }
    switch (s3d_solve_affine(ps, pr, len_best, dim, &cur)) {
    case SIFT3D_SUCCESS:
        if (copy_tform(&cur, tform)) goto done;
        break;
    case SIFT3D_SINGULAR: break;                           /* keep the sample's model */
    default: goto done;
    }
    rc = SIFT3D_SUCCESS;
    goto done;
dev_failed:
    s3d_api_set_error("find_tform_ransac: scoring on the device (SIFT3D_AMD_RANSAC_DEVICE) failed: %s", s3d_rt_last_error());
done:
    s3d_ransac_dev_close(&dev);
    free(best); free(scratch); free(counts); free(models); free(ps); free(pr);
    cleanup_tform(&cur);
    return rc;
}

/* ---- resampling (device) -------------------------------------------------------------------------- */
int im_inv_transform(const void *const tform, const Image *const src, const interp_type interp, const int resize,
                     Image *const dst)
{
    if (resize && im_copy_dims(src, dst)) return SIFT3D_FAILURE;
    if (interp != LINEAR && interp != LANCZOS2) {
        S3D_MSG("im_inv_transform: unrecognized interpolation type");
        return SIFT3D_FAILURE;
    }
    const int is_tps = tform_get_type(tform) == TPS && s3d_tps_is_3d((const Tps *)tform);
    if (!is_tps && (tform_get_type(tform) != AFFINE || ((const Affine *)tform)->A.num_rows != IM_NDIMS)) {
        S3D_MSG("im_inv_transform: only 3-D affine transforms are supported \n");
        return SIFT3D_FAILURE;
    }
    if (dst->nc != src->nc || dst->data == NULL || src->data == NULL) return SIFT3D_FAILURE;
    const size_t ns = (size_t)src->nx * src->ny * src->nz * src->nc, nd = (size_t)dst->nx * dst->ny * dst->nz * dst->nc;
    float *d_src = NULL, *d_dst = NULL, *packed = NULL;
    double *d_tps = NULL;                                   /* the spline: params (3 x (N + 4)), then kp_src (N x 3) */
    int rc = SIFT3D_FAILURE;
    /* the device works on default strides */
    const float *h_src = src->data;
    if (!s3d_im_is_default_stride(src)) {
        if ((packed = (float *)malloc(ns * sizeof(float))) == NULL) return SIFT3D_FAILURE;
        s3d_im_gather(src, packed);
        h_src = packed;
    }
    if (!s3d_im_is_default_stride(dst)) im_default_stride(dst);
    int dev_rc = s3d_rt_malloc((void **)&d_src, ns * sizeof(float)) || s3d_rt_malloc((void **)&d_dst, nd * sizeof(float)) ||
                 s3d_rt_h2d(d_src, h_src, ns * sizeof(float), NULL);
    if (!dev_rc && is_tps) {
        const Tps *const t = (const Tps *)tform;
        const size_t n = (size_t)t->kp_src.num_rows, np = 3 * (n + 4);
        dev_rc = s3d_rt_malloc((void **)&d_tps, (np + 3 * n) * sizeof(double)) ||
                 s3d_rt_h2d(d_tps, t->params.u.data_double, np * sizeof(double), NULL) ||
                 (n && s3d_rt_h2d(d_tps + np, t->kp_src.u.data_double, 3 * n * sizeof(double), NULL)) ||
                 s3d_k_inv_tps(d_src, src->nx, src->ny, src->nz, src->nc, d_dst, dst->nx, dst->ny, dst->nz, d_tps + np, d_tps,
                               (uint32_t)n, interp == LINEAR ? 0 : 1, NULL);
    } else if (!dev_rc) {
        dev_rc = s3d_k_inv_affine(d_src, src->nx, src->ny, src->nz, src->nc, d_dst, dst->nx, dst->ny, dst->nz,
                                  ((const Affine *)tform)->A.u.data_double, interp == LINEAR ? 0 : 1, NULL);
    }
    if (dev_rc || s3d_rt_d2h(dst->data, d_dst, nd * sizeof(float), NULL) || s3d_rt_sync(NULL))
        S3D_MSG("im_inv_transform: device failure: %s\n", s3d_rt_last_error());
    else
        rc = SIFT3D_SUCCESS;
    s3d_rt_free(d_src); s3d_rt_free(d_dst); s3d_rt_free(d_tps);
    free(packed);
    return rc;
}

int im_resample(const Image *const src, const double *const units, const interp_type interp, Image *const dst)
{
    Affine aff;
    double factors[IM_NDIMS];
    const double su[IM_NDIMS] = {src->ux, src->uy, src->uz};
    const int sd[IM_NDIMS] = {src->nx, src->ny, src->nz};
    int dd[IM_NDIMS];
    if (init_Affine(&aff, IM_NDIMS)) return SIFT3D_FAILURE;
    for (int i = 0; i < IM_NDIMS; i++) {
        factors[i] = su[i] / units[i];
        aff.A.u.data_double[i * (IM_NDIMS + 1) + i] = 1.0 / factors[i];
        dd[i] = (int)ceil((double)sd[i] * factors[i]);
    }
    dst->nc = src->nc;
    dst->nx = dd[0]; dst->ny = dd[1]; dst->nz = dd[2];
    im_default_stride(dst);
    int rc = im_resize(dst) || im_inv_transform(&aff, src, interp, SIFT3D_FALSE, dst);
    if (!rc) { dst->ux = units[0]; dst->uy = units[1]; dst->uz = units[2]; }
    cleanup_tform(&aff);
    return rc ? SIFT3D_FAILURE : SIFT3D_SUCCESS;
}

/* ---- Reg_SIFT3D ----------------------------------------------------------------------------------- */
int init_Reg_SIFT3D(Reg_SIFT3D *const reg)
{
    reg->nn_thresh = SIFT3D_nn_thresh_default;
    init_SIFT3D_Descriptor_store(&reg->desc_src);
    init_SIFT3D_Descriptor_store(&reg->desc_ref);
    init_Ransac(&reg->ran);
    if (init_SIFT3D(&reg->sift3d) || init_Mat_rm(&reg->match_src, 0, 0, SIFT3D_DOUBLE, SIFT3D_FALSE) ||
        init_Mat_rm(&reg->match_ref, 0, 0, SIFT3D_DOUBLE, SIFT3D_FALSE)) {
        S3D_MSG("register_SIFT3D: unexpected error \n");
        return SIFT3D_FAILURE;
    }
    return SIFT3D_SUCCESS;
}

void cleanup_Reg_SIFT3D(Reg_SIFT3D *const reg)
{
    cleanup_SIFT3D_Descriptor_store(&reg->desc_src);
    cleanup_SIFT3D_Descriptor_store(&reg->desc_ref);
    cleanup_SIFT3D(&reg->sift3d);
    cleanup_Mat_rm(&reg->match_src);
    cleanup_Mat_rm(&reg->match_ref);
}

int set_nn_thresh_Reg_SIFT3D(Reg_SIFT3D *const reg, const double nn_thresh)
{
    if (nn_thresh <= 0 || nn_thresh > 1) {
        S3D_MSG("set_nn_thresh_Reg_SIFT3D: invalid threshold: %f \n", nn_thresh);
        return SIFT3D_FAILURE;
    }
    reg->nn_thresh = nn_thresh;
    return SIFT3D_SUCCESS;
}

int set_Ransac_Reg_SIFT3D(Reg_SIFT3D *const reg, const Ransac *const ran) { return copy_Ransac(ran, &reg->ran); }

/* The reference deep-copies the whole detector (copy_SIFT3D, sift.c:590-640); what a fresh detector needs
 * from another one are its five parameters and the dense flag. */
int set_SIFT3D_Reg_SIFT3D(Reg_SIFT3D *const reg, const SIFT3D *const sift3d)
{
    SIFT3D *const d = &reg->sift3d;
    d->dense_rotate = sift3d->dense_rotate;
    return set_peak_thresh_SIFT3D(d, sift3d->peak_thresh) || set_corner_thresh_SIFT3D(d, sift3d->corner_thresh) ||
           set_num_kp_levels_SIFT3D(d, (unsigned int)sift3d->gpyr.num_kp_levels) ||
           set_sigma_n_SIFT3D(d, sift3d->gpyr.sigma_n) || set_sigma0_SIFT3D(d, sift3d->gpyr.sigma0);
}

static int s3d_set_im_Reg(Reg_SIFT3D *const reg, const Image *const im, double *const units,
                          SIFT3D_Descriptor_store *const desc, const char *which)
{
    Keypoint_store kp;
    int rc = SIFT3D_FAILURE;
    init_Keypoint_store(&kp);
    units[0] = im->ux; units[1] = im->uy; units[2] = im->uz;
    if (SIFT3D_detect_keypoints(&reg->sift3d, im, &kp))
        S3D_MSG("set_%s_Reg_SIFT3D: failed to detect keypoints\n", which);
    else if (SIFT3D_extract_descriptors(&reg->sift3d, &kp, desc))
        S3D_MSG("set_%s_Reg_SIFT3D: failed to extract descriptors \n", which);
    else
        rc = SIFT3D_SUCCESS;
    cleanup_Keypoint_store(&kp);
    return rc;
}

int set_src_Reg_SIFT3D(Reg_SIFT3D *const reg, const Image *const src) { return s3d_set_im_Reg(reg, src, reg->src_units, &reg->desc_src, "src"); }
int set_ref_Reg_SIFT3D(Reg_SIFT3D *const reg, const Image *const ref) { return s3d_set_im_Reg(reg, ref, reg->ref_units, &reg->desc_ref, "ref"); }

/* voxel coordinates -> physical units, column by column (im2mm, reg.c:43-74) */
static int s3d_im2mm(const Mat_rm *const im, const double *const units, Mat_rm *const mm)
{
    if (im->num_cols != IM_NDIMS) { S3D_MSG("im2mm: input must have IM_NDIMS columns. \n"); return SIFT3D_FAILURE; }
    if (im->type != SIFT3D_DOUBLE) { S3D_MSG("im2mm: input must have type double. \n"); return SIFT3D_FAILURE; }
    if (copy_Mat_rm(im, mm)) return SIFT3D_FAILURE;
    for (int i = 0; i < mm->num_rows; i++)
        for (int j = 0; j < IM_NDIMS; j++) mm->u.data_double[(size_t)i * IM_NDIMS + j] *= units[j];
    return SIFT3D_SUCCESS;
}

/* a transform between physical coordinates -> one between voxel coordinates (mm2im, reg.c:79-118) */
static int s3d_mm2im(const double *const src_units, const double *const ref_units, void *const tform)
{
    if (tform_get_type(tform) != AFFINE) { S3D_MSG("mm2im: unsupported transform type \n"); return SIFT3D_FAILURE; }
    Mat_rm *const A = &((Affine *)tform)->A;
    if (A->num_rows != IM_NDIMS) { S3D_MSG("mm2im: Invalid transform dimensionality: %d \n", A->num_rows); return SIFT3D_FAILURE; }
    for (int i = 0; i < A->num_rows; i++)
        for (int j = 0; j < A->num_cols; j++) {
            double *const a = A->u.data_double + (size_t)i * A->num_cols + j;
            *a *= j < IM_NDIMS ? ref_units[j] : 1.0;
            *a /= src_units[i];
        }
    return SIFT3D_SUCCESS;
}

int register_SIFT3D(Reg_SIFT3D *const reg, void *const tform)
{
    Mat_rm src_mm, ref_mm;
    int *matches = NULL, rc = SIFT3D_FAILURE;
    if (reg->desc_src.num <= 0) { S3D_MSG("register_SIFT3D: no source image descriptors are available \n"); return SIFT3D_FAILURE; }
    if (reg->desc_ref.num <= 0) { S3D_MSG("register_SIFT3D: no reference image descriptors are available \n"); return SIFT3D_FAILURE; }
    if (init_Mat_rm(&src_mm, 0, 0, SIFT3D_DOUBLE, SIFT3D_FALSE) || init_Mat_rm(&ref_mm, 0, 0, SIFT3D_DOUBLE, SIFT3D_FALSE)) {
        S3D_MSG("register_SIFT3D: failed initialization \n");
        return SIFT3D_FAILURE;
    }
    if (SIFT3D_nn_match(&reg->desc_src, &reg->desc_ref, (float)reg->nn_thresh, &matches))
        S3D_MSG("register_SIFT3D: failed to match descriptors \n");
    else if (SIFT3D_matches_to_Mat_rm(&reg->desc_src, &reg->desc_ref, matches, &reg->match_src, &reg->match_ref))
        S3D_MSG("register_SIFT3D: failed to extract coordinate matrices \n");
    else if (tform == NULL)
        rc = SIFT3D_SUCCESS;
    else if (s3d_im2mm(&reg->match_src, reg->src_units, &src_mm) == 0 && s3d_im2mm(&reg->match_ref, reg->ref_units, &ref_mm) == 0 &&
             find_tform_ransac(&reg->ran, &src_mm, &ref_mm, tform) == 0 && s3d_mm2im(reg->src_units, reg->ref_units, tform) == 0)
        rc = SIFT3D_SUCCESS;
    free(matches);
    cleanup_Mat_rm(&src_mm);
    cleanup_Mat_rm(&ref_mm);
    return rc;
}

static void s3d_scale_descriptors(const double *const f, SIFT3D_Descriptor_store *const d)
{
    const double scale = pow(f[0] * f[1] * f[2], -1.0 / (double)IM_NDIMS);
    for (size_t i = 0; i < d->num; i++) {
        d->buf[i].xd *= f[0]; d->buf[i].yd *= f[1]; d->buf[i].zd *= f[2];
        d->buf[i].sd *= scale;
    }
}

int register_SIFT3D_resample(Reg_SIFT3D *const reg, const Image *const src, const Image *const ref, const interp_type interp,
                             void *const tform)
{
    const double su[IM_NDIMS] = {src->ux, src->uy, src->uz}, ru[IM_NDIMS] = {ref->ux, ref->uy, ref->uz};
    if (!memcmp(su, ru, sizeof(su)))
        return set_src_Reg_SIFT3D(reg, src) || set_ref_Reg_SIFT3D(reg, ref) || register_SIFT3D(reg, tform) ? SIFT3D_FAILURE
                                                                                                            : SIFT3D_SUCCESS;
    double umin[IM_NDIMS], fs[IM_NDIMS], fr[IM_NDIMS];
    Image si, ri;
    init_im(&si);
    init_im(&ri);
    for (int i = 0; i < IM_NDIMS; i++) {
        umin[i] = su[i] < ru[i] ? su[i] : ru[i];
        fs[i] = umin[i] / su[i];
        fr[i] = umin[i] / ru[i];
    }
    int rc = im_resample(src, umin, interp, &si) || im_resample(ref, umin, interp, &ri) || set_src_Reg_SIFT3D(reg, &si) ||
             set_ref_Reg_SIFT3D(reg, &ri);
    if (!rc) {
        s3d_scale_descriptors(fs, &reg->desc_src);
        s3d_scale_descriptors(fr, &reg->desc_ref);
        rc = register_SIFT3D(reg, tform);
    }
    im_free(&si);
    im_free(&ri);
    return rc ? SIFT3D_FAILURE : SIFT3D_SUCCESS;
}

int get_matches_Reg_SIFT3D(const Reg_SIFT3D *const reg, Mat_rm *const match_src, Mat_rm *const match_ref)
{
    return copy_Mat_rm(&reg->match_src, match_src) || copy_Mat_rm(&reg->match_ref, match_ref);
}

/* ---- affine, then a spline through the matches that agree with it (sift3d_amd.h) ------------------------------------------- */
int sift3d_amd_register_tps(Reg_SIFT3D *const reg, const sift3d_amd_tps_opts *const opts, Affine *const affine, Tps *const tps)
{
    if (reg == NULL || affine == NULL || tps == NULL) {
        s3d_api_set_error("sift3d_amd_register_tps: NULL argument");
        return SIFT3D_FAILURE;
    }
    const double lambda = opts != NULL && opts->lambda >= 0.0 ? opts->lambda : SIFT3D_AMD_TPS_LAMBDA_DEFAULT;
    const double thresh = opts != NULL && opts->ctrl_thresh > 0.0 ? opts->ctrl_thresh : 4.0 * reg->ran.err_thresh;
    const int max_points = opts != NULL && opts->max_points > 0 ? opts->max_points : SIFT3D_AMD_TPS_MAX_POINTS_DEFAULT;
    if (opts != NULL && (opts->lambda != opts->lambda || opts->ctrl_thresh != opts->ctrl_thresh)) {
        s3d_api_set_error("sift3d_amd_register_tps: lambda and ctrl_thresh must be numbers");
        return SIFT3D_FAILURE;
    }
    if (tform_get_type(affine) != AFFINE || affine->A.num_rows != IM_NDIMS) {
        s3d_api_set_error("sift3d_amd_register_tps: `affine` must be an initialised 3-D Affine");
        return SIFT3D_FAILURE;
    }
    if (register_SIFT3D(reg, affine)) {
        s3d_api_set_error("sift3d_amd_register_tps: the affine registration failed");
        return SIFT3D_FAILURE;
    }
    /* the residual of a match in physical units: the voxel-space affine is the physical one with column j scaled by
     * ref_units[j] and row i divided by src_units[i] (mm2im), so row i of the voxel residual times src_units[i] */
    const int nm = reg->match_src.num_rows;
    const double *const S = reg->match_src.u.data_double, *const R = reg->match_ref.u.data_double, *const A = affine->A.u.data_double;
    const double thr2 = thresh * thresh;
    int *keep = (int *)malloc(sizeof(int) * (size_t)(nm + 1)), count = 0, rc = SIFT3D_FAILURE;
    Mat_rm ps, pr;
    if (keep == NULL || init_Mat_rm(&ps, 0, IM_NDIMS, SIFT3D_DOUBLE, SIFT3D_FALSE)) { free(keep); return SIFT3D_FAILURE; }
    if (init_Mat_rm(&pr, 0, IM_NDIMS, SIFT3D_DOUBLE, SIFT3D_FALSE)) { free(keep); cleanup_Mat_rm(&ps); return SIFT3D_FAILURE; }
    for (int i = 0; i < nm; i++) {
        const double *r = R + (size_t)i * IM_NDIMS, *s = S + (size_t)i * IM_NDIMS;
        double e = 0.0;
        for (int k = 0; k < IM_NDIMS; k++) {
            const double d = (s[k] - (A[4 * k] * r[0] + A[4 * k + 1] * r[1] + A[4 * k + 2] * r[2] + A[4 * k + 3])) * reg->src_units[k];
            e += d * d;
        }
        if (e > thr2) continue;
        keep[count++] = i;
    }
    const int step = (count + max_points - 1) / max_points > 1 ? (count + max_points - 1) / max_points : 1;
    const int n = (count + step - 1) / step;
    ps.num_rows = pr.num_rows = n;
    if (resize_Mat_rm(&ps) || resize_Mat_rm(&pr)) goto done;
    for (int j = 0; j < n; j++) {
        memcpy(ps.u.data_double + (size_t)j * IM_NDIMS, S + (size_t)keep[j * step] * IM_NDIMS, sizeof(double) * IM_NDIMS);
        memcpy(pr.u.data_double + (size_t)j * IM_NDIMS, R + (size_t)keep[j * step] * IM_NDIMS, sizeof(double) * IM_NDIMS);
    }
    rc = sift3d_amd_fit_tps(&ps, &pr, lambda, tps);
done:
    free(keep);
    cleanup_Mat_rm(&ps);
    cleanup_Mat_rm(&pr);
    return rc;
}

/* ---- similarity of a registration: MSE, NCC and mutual information (sift3d_amd.h) ------------------------------------------
 * The device accumulates the joint histogram and seven f64 sums (s3d_k_similarity_*); everything derived from them is here. */
static double s3d_entropy_nats(const double *const counts, const size_t num, const double n)
{
    double h = 0.0;
    for (size_t i = 0; i < num; i++)
        if (counts[i] > 0.0) {
            const double p = counts[i] / n;
            h -= p * log(p);
        }
    return h;
}

static void s3d_similarity_derive(const unsigned long long *const hist, const int bins, const double *const S,
                                  const double c_ref, const double c_src, const long long n_total, sift3d_amd_similarity *const out,
                                  double *const marg /* 2 * bins */)
{
    const size_t nb2 = (size_t)bins * bins;
    unsigned long long cnt = 0;
    for (size_t i = 0; i < nb2; i++) cnt += hist[i];
    out->n = (long long)cnt;
    out->n_total = n_total;
    if (cnt == 0) {
        out->mean_ref = out->mean_src = out->var_ref = out->var_src = out->mse = out->mae = out->ncc = out->h_ref = out->h_src =
            out->h_joint = out->mi = out->nmi = NAN;
        return;
    }
    const double n = (double)cnt, ma = S[0] / n, mb = S[1] / n;
    out->mean_ref = c_ref + ma;
    out->mean_src = c_src + mb;
    out->var_ref = S[2] / n - ma * ma;
    out->var_src = S[3] / n - mb * mb;
    const double cov = S[4] / n - ma * mb;
    out->ncc = out->var_ref > 0.0 && out->var_src > 0.0 ? cov / sqrt(out->var_ref * out->var_src) : NAN;
    out->mse = S[5] / n;
    out->mae = S[6] / n;
    double *const pa = marg, *const pb = marg + bins, hj = 0.0;
    for (int i = 0; i < 2 * bins; i++) marg[i] = 0.0;
    for (int i = 0; i < bins; i++)
        for (int j = 0; j < bins; j++) {
            const double c = (double)hist[(size_t)i * bins + j];
            if (c > 0.0) {
                const double p = c / n;
                hj -= p * log(p);
                pa[i] += c;                                /* integers below 2^53: exact */
                pb[j] += c;
            }
        }
    out->h_ref = s3d_entropy_nats(pa, (size_t)bins, n);
    out->h_src = s3d_entropy_nats(pb, (size_t)bins, n);
    out->h_joint = hj;
    out->mi = out->h_ref + out->h_src - hj;
    out->nmi = hj == 0.0 ? NAN : (out->h_ref + out->h_src) / hj;
}

#define S3D_SIM_FAIL(...) do { s3d_api_set_error("sift3d_amd_im_similarity: " __VA_ARGS__); return SIFT3D_FAILURE; } while (0)

/* what both entry points refuse before anything is allocated; *bins and *interp receive the effective values */
static int s3d_similarity_check(const void *const tform, const sift3d_amd_similarity_opts *const opts,
                                const sift3d_amd_similarity *const out, int *const bins, int *const interp, int *const is_tps)
{
    if (out == NULL) S3D_SIM_FAIL("NULL result");
    *bins = opts != NULL && opts->bins != 0 ? opts->bins : SIFT3D_AMD_SIMILARITY_BINS_DEFAULT;
    if (*bins < 2 || *bins > SIFT3D_AMD_SIMILARITY_BINS_MAX) S3D_SIM_FAIL("bins must be in 2 .. 128 (0: 64), not %d", *bins);
    *interp = opts != NULL ? (int)opts->interp : (int)LINEAR;
    if (*interp != (int)LINEAR && *interp != (int)LANCZOS2) S3D_SIM_FAIL("unrecognized interpolation type %d", *interp);
    *is_tps = 0;
    if (tform != NULL) {
        *is_tps = tform_get_type(tform) == TPS && s3d_tps_is_3d((const Tps *)tform);
        if (!*is_tps && (tform_get_type(tform) != AFFINE || ((const Affine *)tform)->A.num_rows != IM_NDIMS ||
                         ((const Affine *)tform)->A.num_cols != IM_NDIMS + 1 || ((const Affine *)tform)->A.type != SIFT3D_DOUBLE ||
                         ((const Affine *)tform)->A.u.data_double == NULL))
            S3D_SIM_FAIL("the transform must be NULL, a 3-D Affine or a 3-D Tps");
    }
    if (opts != NULL)
        for (int i = 0; i < 2; i++)
            if (opts->ref_range[i] != opts->ref_range[i] || opts->src_range[i] != opts->src_range[i])
                S3D_SIM_FAIL("a range holds a NaN");
    return SIFT3D_SUCCESS;
}

int sift3d_amd_similarity_dev(const void *tform, const float *d_src, int snx, int sny, int snz, const float *d_ref, int rnx, int rny,
                              int rnz, const sift3d_amd_similarity_opts *opts, sift3d_amd_similarity *out,
                              unsigned long long *joint, void *hip_stream)
{
    int bins, interp, is_tps;
    if (s3d_similarity_check(tform, opts, out, &bins, &interp, &is_tps)) return SIFT3D_FAILURE;
    if (d_src == NULL || d_ref == NULL) S3D_SIM_FAIL("NULL data");
    if (snx < 1 || sny < 1 || snz < 1 || rnx < 1 || rny < 1 || rnz < 1) S3D_SIM_FAIL("bad dimensions");
    const size_t nb2 = (size_t)bins * bins, scratch_bytes = s3d_k_similarity_scratch_bytes(rnx, rny, rnz, bins);
    const size_t ns = (size_t)snx * sny * snz, nr = (size_t)rnx * rny * rnz;
    /* one device block: the histogram, the sums, two min / max pairs, the partials, the spline */
    const Tps *const t = is_tps ? (const Tps *)tform : NULL;
    const size_t nctrl = t ? (size_t)t->kp_src.num_rows : 0, np = t ? 3 * (nctrl + 4) : 0;
    const size_t off_sums = nb2 * 8, off_mm = off_sums + 7 * 8, off_scr = off_mm + 16, off_tps = off_scr + scratch_bytes;
    unsigned char *d_blk = NULL;
    unsigned long long *h_hist = (unsigned long long *)malloc(nb2 * sizeof(*h_hist));
    double *marg = (double *)malloc(2 * (size_t)bins * sizeof(double));
    int rc = SIFT3D_FAILURE;
    if (h_hist == NULL || marg == NULL) { s3d_api_set_error("sift3d_amd_im_similarity: out of memory"); goto done; }
    if (s3d_rt_malloc((void **)&d_blk, off_tps + (np + 3 * nctrl) * sizeof(double))) goto dev_failed;
    /* the ranges: the caller's where [1] > [0], else the finite minimum and maximum of the whole volume */
    double rng[2][2];
    const int have_ref = opts != NULL && opts->ref_range[1] > opts->ref_range[0];
    const int have_src = opts != NULL && opts->src_range[1] > opts->src_range[0];
    if (have_ref) { rng[0][0] = opts->ref_range[0]; rng[0][1] = opts->ref_range[1]; }
    if (have_src) { rng[1][0] = opts->src_range[0]; rng[1][1] = opts->src_range[1]; }
    if (!have_ref || !have_src) {
        float mm[4];
        float *const d_mm = (float *)(d_blk + off_mm);
        if ((!have_ref && s3d_k_minmax_finite(d_ref, nr, d_mm, hip_stream)) ||
            (!have_src && s3d_k_minmax_finite(d_src, ns, d_mm + 2, hip_stream)) ||
            s3d_rt_d2h(mm, d_mm, sizeof(mm), hip_stream) || s3d_rt_sync(hip_stream))
            goto dev_failed;
        if (!have_ref) {
            if (mm[0] != mm[0]) { s3d_api_set_error("sift3d_amd_im_similarity: the reference volume has no finite voxel"); goto done; }
            rng[0][0] = mm[0]; rng[0][1] = mm[1];
        }
        if (!have_src) {
            if (mm[2] != mm[2]) { s3d_api_set_error("sift3d_amd_im_similarity: the source volume has no finite voxel"); goto done; }
            rng[1][0] = mm[2]; rng[1][1] = mm[3];
        }
    }
    double scale[2], piv[2];
    for (int k = 0; k < 2; k++) {
        scale[k] = rng[k][1] > rng[k][0] ? (double)bins / (rng[k][1] - rng[k][0]) : 0.0;
        piv[k] = 0.5 * (rng[k][0] + rng[k][1]);
        if (!(fabs(scale[k]) <= DBL_MAX) || !(fabs(piv[k]) <= DBL_MAX)) {
            s3d_api_set_error("sift3d_amd_im_similarity: a range is too narrow or too wide for %d bins", bins);
            goto done;
        }
    }
    unsigned long long *const d_hist = (unsigned long long *)d_blk;
    double *const d_sums = (double *)(d_blk + off_sums);
    void *const d_scr = d_blk + off_scr;
    int dev_rc;
    if (t != NULL) {
        double *const d_tps = (double *)(d_blk + off_tps);
        dev_rc = s3d_rt_h2d(d_tps, t->params.u.data_double, np * sizeof(double), hip_stream) ||
                 (nctrl && s3d_rt_h2d(d_tps + np, t->kp_src.u.data_double, 3 * nctrl * sizeof(double), hip_stream)) ||
                 s3d_k_similarity_tps(d_src, snx, sny, snz, d_ref, rnx, rny, rnz, d_tps + np, d_tps, (uint32_t)nctrl, interp == (int)LINEAR ? 0 : 1,
                                      bins, rng[0][0], scale[0], rng[1][0], scale[1], piv[0], piv[1], d_hist, d_sums, d_scr, hip_stream);
    } else {
        static const double identity[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
        const double *const A = tform != NULL ? ((const Affine *)tform)->A.u.data_double : identity;
        dev_rc = s3d_k_similarity_affine(d_src, snx, sny, snz, d_ref, rnx, rny, rnz, A, interp == (int)LINEAR ? 0 : 1, bins, rng[0][0],
                                         scale[0], rng[1][0], scale[1], piv[0], piv[1], d_hist, d_sums, d_scr, hip_stream);
    }
    double sums[7];
    if (dev_rc || s3d_rt_d2h(h_hist, d_hist, nb2 * sizeof(*h_hist), hip_stream) || s3d_rt_d2h(sums, d_sums, sizeof(sums), hip_stream) ||
        s3d_rt_sync(hip_stream))
        goto dev_failed;
    sift3d_amd_similarity res;
    s3d_similarity_derive(h_hist, bins, sums, piv[0], piv[1], (long long)nr, &res, marg);
    *out = res;
    if (joint != NULL) memcpy(joint, h_hist, nb2 * sizeof(*h_hist));
    rc = SIFT3D_SUCCESS;
    goto done;
dev_failed:
    s3d_api_set_error("sift3d_amd_im_similarity: device failure: %s", s3d_rt_last_error());
done:
    s3d_rt_free(d_blk);
    free(h_hist); free(marg);
    return rc;
}

int sift3d_amd_im_similarity(const void *tform, const Image *src, const Image *ref, const sift3d_amd_similarity_opts *opts,
                             sift3d_amd_similarity *out, unsigned long long *joint)
{
    int bins, interp, is_tps;
    if (s3d_similarity_check(tform, opts, out, &bins, &interp, &is_tps)) return SIFT3D_FAILURE;
    if (src == NULL || ref == NULL) S3D_SIM_FAIL("NULL image");
    if (src->nc != 1 || ref->nc != 1) S3D_SIM_FAIL("single-channel volumes only (nc = %d and %d)", src->nc, ref->nc);
    if (src->data == NULL || ref->data == NULL) S3D_SIM_FAIL("NULL data");
    if (src->nx < 1 || src->ny < 1 || src->nz < 1 || ref->nx < 1 || ref->ny < 1 || ref->nz < 1) S3D_SIM_FAIL("bad dimensions");
    const Image *const ims[2] = {src, ref};
    float *d_im[2] = {NULL, NULL};
    int rc = SIFT3D_FAILURE;
    for (int k = 0; k < 2; k++) {                           /* the device works on default strides */
        const size_t n = (size_t)ims[k]->nx * ims[k]->ny * ims[k]->nz;
        const float *h = ims[k]->data;
        float *packed = NULL;
        if (!s3d_im_is_default_stride(ims[k])) {
            if ((packed = (float *)malloc(n * sizeof(float))) == NULL) { s3d_api_set_error("sift3d_amd_im_similarity: out of memory"); goto done; }
            s3d_im_gather(ims[k], packed);
            h = packed;
        }
        const int dev_rc = s3d_rt_malloc((void **)&d_im[k], n * sizeof(float)) || s3d_rt_h2d(d_im[k], h, n * sizeof(float), NULL) ||
                           s3d_rt_sync(NULL);
        free(packed);
        if (dev_rc) { s3d_api_set_error("sift3d_amd_im_similarity: device failure: %s", s3d_rt_last_error()); goto done; }
    }
    rc = sift3d_amd_similarity_dev(tform, d_im[0], src->nx, src->ny, src->nz, d_im[1], ref->nx, ref->ny, ref->nz, opts, out, joint, NULL);
done:
    s3d_rt_free(d_im[0]); s3d_rt_free(d_im[1]);
    return rc;
}

/* ---- intensity-based refinement of an affine map (sift3d_amd.h) --------------------------------------------------------------
 * Levenberg-Marquardt on the 12 entries of the map.  The device returns the cost and the normal equations of a map in one pass
 * (s3d_k_affine_normal_eq); the 12 x 12 solve, the step rule and the pyramid schedule are here.  The map is kept in level-0
 * voxel coordinates throughout; a level sees it with the translation scaled by 2^-l. */
#define S3D_REF_FAIL(...) do { s3d_api_set_error("sift3d_amd_refine_affine: " __VA_ARGS__); return SIFT3D_FAILURE; } while (0)
#define S3D_REF_MAX_LEVELS 16
#define S3D_REF_MIN_DIM 16
#define S3D_REF_LAMBDA0 1e-3
#define S3D_REF_LAMBDA_MAX 1e10

typedef struct {
    const float *src, *ref;                                 /* device */
    int sd[3], rd[3];
} s3d_ref_level;

typedef struct {
    s3d_ref_level lv[S3D_REF_MAX_LEVELS];
    int nlv, passes;
    double *d_sums;
    void *d_scr, *stream;
} s3d_ref_ctx;

/* The coarse-to-fine pyramid, shared by the refinement and the demons driver.  s3d_ref_plan_pyramid fills in the levels that
 * exist -- at most `levels`, none with a source dimension below min_sdim or a reference dimension below min_rdim -- and returns the bytes of device memory
 * they take at the front of the caller's block: the coarse volumes, then (with more than one level) the two work volumes of
 * the Gaussian.  s3d_ref_build_pyramid fills them: level l is level l - 1 through init_Gauss_filter's taps at sigma = 1,
 * every second voxel. */
#define S3D_REF_VOX(d) ((size_t)(d)[0] * (d)[1] * (d)[2])
#define S3D_REF_ALIGN(b) (((b) + 255) & ~(size_t)255)
typedef struct { size_t off[S3D_REF_MAX_LEVELS][2], off_work, nwork; } s3d_ref_plan;

static size_t s3d_ref_plan_pyramid(s3d_ref_ctx *const c, s3d_ref_plan *const plan, const int levels, const int min_sdim, const int min_rdim,
                                   const float *d_src, int snx, int sny, int snz, const float *d_ref, int rnx, int rny, int rnz,
                                   void *const stream)
{
    size_t bytes = 0;
    memset(c, 0, sizeof(*c));
    c->stream = stream;
    c->lv[0] = (s3d_ref_level){d_src, d_ref, {snx, sny, snz}, {rnx, rny, rnz}};
    c->nlv = 1;
    while (c->nlv < levels) {
        const s3d_ref_level *const p = &c->lv[c->nlv - 1];
        s3d_ref_level *const n = &c->lv[c->nlv];
        int small = 0;
        for (int k = 0; k < 3; k++) {
            n->sd[k] = p->sd[k] / 2;
            n->rd[k] = p->rd[k] / 2;
            small = small || n->sd[k] < min_sdim || n->rd[k] < min_rdim;
        }
        if (small) break;                                   /* every coarser level would be smaller still */
        plan->off[c->nlv][0] = bytes; bytes += S3D_REF_ALIGN(S3D_REF_VOX(n->sd) * sizeof(float));
        plan->off[c->nlv][1] = bytes; bytes += S3D_REF_ALIGN(S3D_REF_VOX(n->rd) * sizeof(float));
        c->nlv++;
    }
    plan->nwork = S3D_REF_VOX(c->lv[0].sd) > S3D_REF_VOX(c->lv[0].rd) ? S3D_REF_VOX(c->lv[0].sd) : S3D_REF_VOX(c->lv[0].rd);
    plan->off_work = bytes;
    if (c->nlv > 1) bytes += 2 * S3D_REF_ALIGN(plan->nwork * sizeof(float));
    return bytes;
}

static int s3d_ref_build_pyramid(s3d_ref_ctx *const c, const s3d_ref_plan *const plan, unsigned char *const d_blk)
{
    if (c->nlv < 2) return 0;
    float taps[7], acc = 0;                                 /* init_Gauss_filter at sigma = 1 */
    for (int i = 0; i < 7; i++) {
        const double x = ((double)i - 3) / (1.0 + DBL_EPSILON);
        taps[i] = (float)exp(-0.5 * x * x);
        acc += taps[i];
    }
    for (int i = 0; i < 7; i++) taps[i] /= acc;
    static const float uf[3] = {1.0f, 1.0f, 1.0f};
    float *const blur = (float *)(d_blk + plan->off_work);
    float *const tmp = (float *)(d_blk + plan->off_work + S3D_REF_ALIGN(plan->nwork * sizeof(float)));
    for (int l = 1; l < c->nlv; l++) {
        const s3d_ref_level *const p = &c->lv[l - 1];
        float *const dst[2] = {(float *)(d_blk + plan->off[l][0]), (float *)(d_blk + plan->off[l][1])};
        if (s3d_k_sep_fir(p->src, blur, tmp, p->sd[0], p->sd[1], p->sd[2], 1, uf, taps, 7, c->stream) ||
            s3d_k_decimate2(blur, p->sd[0], p->sd[1], p->sd[2], dst[0], c->stream) ||
            s3d_k_sep_fir(p->ref, blur, tmp, p->rd[0], p->rd[1], p->rd[2], 1, uf, taps, 7, c->stream) ||
            s3d_k_decimate2(blur, p->rd[0], p->rd[1], p->rd[2], dst[1], c->stream))
            return -1;
        c->lv[l].src = dst[0];
        c->lv[l].ref = dst[1];
    }
    return 0;
}

/* the sums of the level-0 map A0 on level l with the constants K = (sa, ma, sb, mb); -1: device failure */
static int s3d_ref_pass(s3d_ref_ctx *const c, const int l, const double A0[12], const double K[4], double S[S3D_NEQ_SUMS])
{
    const s3d_ref_level *const v = &c->lv[l];
    const double scale = ldexp(1.0, l), ctr[3] = {0.5 * (v->rd[0] - 1), 0.5 * (v->rd[1] - 1), 0.5 * (v->rd[2] - 1)};
    double A[12];
    memcpy(A, A0, sizeof(A));
    for (int i = 0; i < 3; i++) A[i * 4 + 3] = A0[i * 4 + 3] / scale;
    if (s3d_k_affine_normal_eq(v->src, v->sd[0], v->sd[1], v->sd[2], v->ref, v->rd[0], v->rd[1], v->rd[2], A, ctr, K[0], K[1], K[2],
                               K[3], c->d_sums, c->d_scr, c->stream) ||
        s3d_rt_d2h(S, c->d_sums, S3D_NEQ_SUMS * sizeof(double), c->stream) || s3d_rt_sync(c->stream))
        return -1;
    c->passes++;
    return 0;
}

/* the largest displacement of a corner of the rd[0] x rd[1] x rd[2] volume between the maps A and B */
static double s3d_ref_corner_shift(const double A[12], const double B[12], const int rd[3])
{
    double best = 0.0;
    for (int k = 0; k < 8; k++) {
        const double p[4] = {(k & 1) ? rd[0] - 1.0 : 0.0, (k & 2) ? rd[1] - 1.0 : 0.0, (k & 4) ? rd[2] - 1.0 : 0.0, 1.0};
        double d2 = 0.0;
        for (int i = 0; i < 3; i++) {
            double d = 0.0;
            for (int j = 0; j < 4; j++) d += (A[i * 4 + j] - B[i * 4 + j]) * p[j];
            d2 += d * d;
        }
        if (!(d2 <= best * best)) best = sqrt(d2);          /* a NaN shift stays visible */
    }
    return best;
}

/* delta (12: entry (i, k) of [D | d] at [i * 4 + k]) from the sums S and the damping lambda; non-zero: no usable step */
static int s3d_ref_solve(const double S[S3D_NEQ_SUMS], const double lambda, double delta[12])
{
    static const int P[3][3] = {{0, 1, 2}, {1, 3, 4}, {2, 4, 5}}, Q[4][4] = {{0, 1, 2, 3}, {1, 4, 5, 6}, {2, 5, 7, 8}, {3, 6, 8, 9}};
    double M[144];
    int piv[12];
    for (int i = 0; i < 3; i++)
        for (int k = 0; k < 4; k++)
            for (int j = 0; j < 3; j++)
                for (int m = 0; m < 4; m++) M[(i * 4 + k) * 12 + j * 4 + m] = S[P[i][j] * 10 + Q[k][m]];
    for (int p = 0; p < 12; p++) {
        M[p * 12 + p] += lambda * M[p * 12 + p];
        delta[p] = -S[60 + p];
    }
    if (s3d_lu(M, 12, piv)) return 1;
    s3d_lu_solve(M, piv, 12, delta, 1);
    for (int p = 0; p < 12; p++)
        if (!(fabs(delta[p]) <= DBL_MAX)) return 1;
    return 0;
}

/* One level.  A (level 0 coordinates) and S, its sums on level l, are the start and become the result; n_floor: the smallest
 * count a step may have.  *iters grows by the accepted steps.  Returns the status the level ended with, or -1. */
static int s3d_ref_run_level(s3d_ref_ctx *const c, const int l, double A[12], const double K[4], double S[S3D_NEQ_SUMS],
                             const double n_floor, const int max_iter, const double tol, int *const iters)
{
    const s3d_ref_level *const v = &c->lv[l];
    const double scale = ldexp(1.0, l), ctr[3] = {0.5 * (v->rd[0] - 1), 0.5 * (v->rd[1] - 1), 0.5 * (v->rd[2] - 1)};
    double lambda = S3D_REF_LAMBDA0;
    int accepted = 0;
    for (;;) {
        int flat = 1;
        for (int p = 0; p < 12; p++) flat = flat && S[60 + p] == 0.0;
        if (flat) return SIFT3D_AMD_REFINE_CONVERGED;       /* a stationary point: every step would be zero */
        double delta[12], B[12], T[S3D_NEQ_SUMS];
        int ok = !s3d_ref_solve(S, lambda, delta);
        if (ok) {
            for (int i = 0; i < 3; i++) {
                const double *const D = delta + i * 4;
                for (int j = 0; j < 3; j++) B[i * 4 + j] = A[i * 4 + j] + D[j];
                B[i * 4 + 3] = A[i * 4 + 3] + scale * (D[3] - (D[0] * ctr[0] + D[1] * ctr[1] + D[2] * ctr[2]));
            }
            if (s3d_ref_pass(c, l, B, K, T)) return -1;
            ok = T[73] > 0.0 && T[73] >= n_floor && T[72] / T[73] < S[72] / S[73];
        }
        if (ok) {
            const double shift = s3d_ref_corner_shift(A, B, c->lv[0].rd);
            memcpy(A, B, sizeof(B));
            memcpy(S, T, sizeof(T));
            lambda /= 10.0;
            accepted++;
            (*iters)++;
            if (shift <= tol) return SIFT3D_AMD_REFINE_CONVERGED;
            if (accepted >= max_iter) return SIFT3D_AMD_REFINE_MAX_ITER;
        } else {
            lambda *= 10.0;
            if (lambda > S3D_REF_LAMBDA_MAX) return SIFT3D_AMD_REFINE_STALLED;
        }
    }
}

/* K = (sa, ma, sb, mb) of a level at the level-0 map A0: (1, 0, 1, 0), or the z-score of both sides over the overlap */
static int s3d_ref_constants(s3d_ref_ctx *const c, const int l, const Affine *const like, const double A0[12], const int normalize,
                             double K[4])
{
    K[0] = K[2] = 1.0;
    K[1] = K[3] = 0.0;
    if (!normalize) return 0;
    const s3d_ref_level *const v = &c->lv[l];
    double A[12];
    memcpy(A, A0, sizeof(A));
    for (int i = 0; i < 3; i++) A[i * 4 + 3] = A0[i * 4 + 3] / ldexp(1.0, l);
    Affine t = *like;
    t.A.u.data_double = A;
    sift3d_amd_similarity sim;
    if (sift3d_amd_similarity_dev(&t, v->src, v->sd[0], v->sd[1], v->sd[2], v->ref, v->rd[0], v->rd[1], v->rd[2], NULL, &sim, NULL,
                                  c->stream))
        return -1;
    if (sim.n > 0) {
        K[0] = sim.var_ref > 0.0 && sim.var_ref <= DBL_MAX ? 1.0 / sqrt(sim.var_ref) : 1.0;
        K[1] = fabs(sim.mean_ref) <= DBL_MAX ? sim.mean_ref : 0.0;
        K[2] = sim.var_src > 0.0 && sim.var_src <= DBL_MAX ? 1.0 / sqrt(sim.var_src) : 1.0;
        K[3] = fabs(sim.mean_src) <= DBL_MAX ? sim.mean_src : 0.0;
    }
    return 0;
}

static int s3d_refine_check(const sift3d_amd_refine_opts *const opts, const Affine *const affine)
{
    if (affine == NULL) S3D_REF_FAIL("NULL transform");
    if (tform_get_type(affine) != AFFINE || affine->A.num_rows != IM_NDIMS || affine->A.num_cols != IM_NDIMS + 1 ||
        affine->A.type != SIFT3D_DOUBLE || affine->A.u.data_double == NULL)
        S3D_REF_FAIL("the transform must be a 3-D Affine");
    if (opts != NULL) {
        if (opts->levels < 0 || opts->max_iter < 0) S3D_REF_FAIL("levels and max_iter must not be negative (%d, %d)", opts->levels, opts->max_iter);
        if (!(opts->tol >= 0.0) || !(opts->min_overlap >= 0.0)) S3D_REF_FAIL("tol and min_overlap must be numbers >= 0");
        if (opts->normalize != 0 && opts->normalize != 1) S3D_REF_FAIL("normalize must be 0 or 1, not %d", opts->normalize);
    }
    return SIFT3D_SUCCESS;
}

int sift3d_amd_refine_affine_dev(const float *d_src, int snx, int sny, int snz, const float *d_ref, int rnx, int rny, int rnz,
                                 const sift3d_amd_refine_opts *opts, Affine *affine, sift3d_amd_refine_info *info, void *hip_stream)
{
    if (s3d_refine_check(opts, affine)) return SIFT3D_FAILURE;
    if (d_src == NULL || d_ref == NULL) S3D_REF_FAIL("NULL data");
    if (snx < 1 || sny < 1 || snz < 1 || rnx < 1 || rny < 1 || rnz < 1) S3D_REF_FAIL("bad dimensions");
    if (snx < 2 || sny < 2 || snz < 2) S3D_REF_FAIL("a source dimension below 2 has no intensity gradient (%d x %d x %d)", snx, sny, snz);
    int levels = opts != NULL && opts->levels != 0 ? opts->levels : SIFT3D_AMD_REFINE_LEVELS_DEFAULT;
    if (levels > S3D_REF_MAX_LEVELS) levels = S3D_REF_MAX_LEVELS;
    const int max_iter = opts != NULL && opts->max_iter != 0 ? opts->max_iter : SIFT3D_AMD_REFINE_ITER_DEFAULT;
    const double tol = opts != NULL && opts->tol != 0.0 ? opts->tol : 1e-3;
    const double min_overlap = opts != NULL && opts->min_overlap != 0.0 ? opts->min_overlap : 0.5;
    const int normalize = opts != NULL ? opts->normalize : 0;

    /* the levels that exist, and one device block for them: the coarse volumes, the two work volumes of the Gaussian, the
     * sums and the partials */
    s3d_ref_ctx c;
    s3d_ref_plan plan;
    size_t bytes = s3d_ref_plan_pyramid(&c, &plan, levels, S3D_REF_MIN_DIM, S3D_REF_MIN_DIM, d_src, snx, sny, snz, d_ref, rnx, rny, rnz, hip_stream);
    const size_t off_sums = bytes;
    bytes += S3D_REF_ALIGN(S3D_NEQ_SUMS * sizeof(double));
    const size_t off_scr = bytes;
    bytes += s3d_k_affine_normal_eq_scratch_bytes(rnx, rny, rnz);   /* the finest level has the most workgroups */
    unsigned char *d_blk = NULL;
    int rc = SIFT3D_FAILURE;
    if (s3d_rt_malloc((void **)&d_blk, bytes)) goto dev_failed;
    c.d_sums = (double *)(d_blk + off_sums);
    c.d_scr = d_blk + off_scr;
    if (s3d_ref_build_pyramid(&c, &plan, d_blk)) goto dev_failed;

    double A_start[12], A[12], K[4], S_start[S3D_NEQ_SUMS], S[S3D_NEQ_SUMS];
    static const double raw[4] = {1.0, 0.0, 1.0, 0.0};
    memcpy(A_start, affine->A.u.data_double, sizeof(A_start));
    memcpy(A, A_start, sizeof(A));
    if (s3d_ref_pass(&c, 0, A_start, raw, S_start)) goto dev_failed;
    if (!(S_start[73] > 0.0)) {
        s3d_api_set_error("sift3d_amd_refine_affine: the volumes do not overlap under the transform as given");
        goto done;
    }
    int iters = 0, levels_run = 0;
    for (int l = c.nlv - 1; l >= 1; l--) {                  /* the coarse levels; one that has no overlap is left out */
        if (s3d_ref_constants(&c, l, affine, A, normalize, K)) goto done;
        if (s3d_ref_pass(&c, l, A, K, S)) goto dev_failed;
        if (!(S[73] > 0.0)) continue;
        if (s3d_ref_run_level(&c, l, A, K, S, min_overlap * S[73], max_iter, tol, &iters) < 0) goto dev_failed;
        levels_run++;
    }
    if (s3d_ref_constants(&c, 0, affine, A, normalize, K)) goto done;
    if (normalize && s3d_ref_pass(&c, 0, A_start, K, S_start)) goto dev_failed;
    const double n_before = S_start[73], cost_before = S_start[72] / S_start[73], n_floor = min_overlap * n_before;
    memcpy(S, S_start, sizeof(S));
    if (memcmp(A, A_start, sizeof(A)) != 0) {               /* keep the coarse levels' map only if it is no worse here */
        if (s3d_ref_pass(&c, 0, A, K, S)) goto dev_failed;
        if (!(S[73] > 0.0 && S[73] >= n_floor && S[72] / S[73] <= cost_before)) {
            memcpy(A, A_start, sizeof(A));
            memcpy(S, S_start, sizeof(S));
            iters = 0;
        }
    }
    int status = s3d_ref_run_level(&c, 0, A, K, S, n_floor, max_iter, tol, &iters);
    if (status < 0) goto dev_failed;
    levels_run++;
    if (!(S[73] >= n_floor && S[72] / S[73] <= cost_before) || memcmp(A, A_start, sizeof(A)) == 0) {
        memcpy(A, A_start, sizeof(A));
        memcpy(S, S_start, sizeof(S));
        status = SIFT3D_AMD_REFINE_UNCHANGED;
        iters = 0;
    }
    if (status != SIFT3D_AMD_REFINE_UNCHANGED) memcpy(affine->A.u.data_double, A, sizeof(A));
    if (info != NULL) {
        info->status = status;
        info->levels_run = levels_run;
        info->iters = iters;
        info->passes = c.passes;
        info->n_before = (long long)n_before;
        info->n_after = (long long)S[73];
        info->cost_before = cost_before;
        info->cost_after = S[72] / S[73];
        info->max_corner_shift = s3d_ref_corner_shift(A_start, A, c.lv[0].rd);
    }
    rc = SIFT3D_SUCCESS;
    goto done;
dev_failed:
    s3d_api_set_error("sift3d_amd_refine_affine: device failure: %s", s3d_rt_last_error());
done:
    s3d_rt_free(d_blk);
    return rc;
}

int sift3d_amd_refine_affine(const Image *src, const Image *ref, const sift3d_amd_refine_opts *opts, Affine *affine,
                             sift3d_amd_refine_info *info)
{
    if (s3d_refine_check(opts, affine)) return SIFT3D_FAILURE;
    if (src == NULL || ref == NULL) S3D_REF_FAIL("NULL image");
    if (src->nc != 1 || ref->nc != 1) S3D_REF_FAIL("single-channel volumes only (nc = %d and %d)", src->nc, ref->nc);
    if (src->data == NULL || ref->data == NULL) S3D_REF_FAIL("NULL data");
    if (src->nx < 1 || src->ny < 1 || src->nz < 1 || ref->nx < 1 || ref->ny < 1 || ref->nz < 1) S3D_REF_FAIL("bad dimensions");
    if (src->nx < 2 || src->ny < 2 || src->nz < 2)
        S3D_REF_FAIL("a source dimension below 2 has no intensity gradient (%d x %d x %d)", src->nx, src->ny, src->nz);
    const Image *const ims[2] = {src, ref};
    float *d_im[2] = {NULL, NULL};
    int rc = SIFT3D_FAILURE;
    for (int k = 0; k < 2; k++) {                           /* the device works on default strides */
        const size_t n = (size_t)ims[k]->nx * ims[k]->ny * ims[k]->nz;
        const float *h = ims[k]->data;
        float *packed = NULL;
        if (!s3d_im_is_default_stride(ims[k])) {
            if ((packed = (float *)malloc(n * sizeof(float))) == NULL) { s3d_api_set_error("sift3d_amd_refine_affine: out of memory"); goto done; }
            s3d_im_gather(ims[k], packed);
            h = packed;
        }
        const int dev_rc = s3d_rt_malloc((void **)&d_im[k], n * sizeof(float)) || s3d_rt_h2d(d_im[k], h, n * sizeof(float), NULL) ||
                           s3d_rt_sync(NULL);
        free(packed);
        if (dev_rc) { s3d_api_set_error("sift3d_amd_refine_affine: device failure: %s", s3d_rt_last_error()); goto done; }
    }
    rc = sift3d_amd_refine_affine_dev(d_im[0], src->nx, src->ny, src->nz, d_im[1], ref->nx, ref->ny, ref->nz, opts, affine, info, NULL);
done:
    s3d_rt_free(d_im[0]); s3d_rt_free(d_im[1]);
    return rc;
}

/* ---- deformable registration: demons refinement of an affine map (sift3d_amd.h) ------------------------------------------------
 * The device makes an update and scores the field it started from in one pass (s3d_k_demons_step) and smooths the result
 * (s3d_k_sep_fir per component); the schedule -- pyramid, stopping rule, acceptance -- is here.  The pyramid is the refinement's. */
#define S3D_DEM_FAIL(...) do { s3d_api_set_error("sift3d_amd_register_demons: " __VA_ARGS__); return SIFT3D_FAILURE; } while (0)
#define S3D_DEM_LAG 5

typedef struct { int levels, max_iter, hw, normalize; double sigma, max_step, tol, min_overlap; } s3d_dem_cfg;

/* what both entry points refuse before anything is allocated; *cfg receives the effective options */
static int s3d_demons_check(const void *const tform, const sift3d_amd_demons_opts *const o, s3d_dem_cfg *const cfg)
{
    if (tform != NULL) {
        const Affine *const a = (const Affine *)tform;
        if (tform_get_type(tform) != AFFINE || a->A.num_rows != IM_NDIMS || a->A.num_cols != IM_NDIMS + 1 ||
            a->A.type != SIFT3D_DOUBLE || a->A.u.data_double == NULL)
            S3D_DEM_FAIL("the transform must be NULL or a 3-D Affine (a Tps is not supported as the base transform)");
    }
    if (o != NULL) {
        if (o->levels < 0 || o->max_iter < 0) S3D_DEM_FAIL("levels and max_iter must not be negative (%d, %d)", o->levels, o->max_iter);
        if (!(o->tol >= 0.0) || !(o->min_overlap >= 0.0)) S3D_DEM_FAIL("tol and min_overlap must be numbers >= 0");
        if (o->normalize != 0 && o->normalize != 1) S3D_DEM_FAIL("normalize must be 0 or 1, not %d", o->normalize);
        if (o->sigma != 0.0 && !(o->sigma >= 0.5 && o->sigma <= 8.0)) S3D_DEM_FAIL("sigma must be in 0.5 .. 8 (0: 1.5), not %g", o->sigma);
        if (!(o->max_step >= 0.0) || !(o->max_step <= DBL_MAX)) S3D_DEM_FAIL("max_step must be a positive number (0: 1), not %g", o->max_step);
    }
    cfg->levels = o != NULL && o->levels != 0 ? o->levels : SIFT3D_AMD_DEMONS_LEVELS_DEFAULT;
    if (cfg->levels > S3D_REF_MAX_LEVELS) cfg->levels = S3D_REF_MAX_LEVELS;
    cfg->max_iter = o != NULL && o->max_iter != 0 ? o->max_iter : SIFT3D_AMD_DEMONS_ITER_DEFAULT;
    cfg->sigma = o != NULL && o->sigma != 0.0 ? o->sigma : 1.5;
    cfg->max_step = o != NULL && o->max_step != 0.0 ? o->max_step : 1.0;
    cfg->tol = o != NULL && o->tol != 0.0 ? o->tol : 1e-3;
    cfg->min_overlap = o != NULL && o->min_overlap != 0.0 ? o->min_overlap : 0.5;
    cfg->normalize = o != NULL ? o->normalize : 0;
    cfg->hw = (int)ceil(cfg->sigma * 3.0);
    return SIFT3D_SUCCESS;
}

static int s3d_demons_check_dims(const s3d_dem_cfg *const cfg, int snx, int sny, int snz, int rnx, int rny, int rnz)
{
    if (snx < 1 || sny < 1 || snz < 1 || rnx < 1 || rny < 1 || rnz < 1) S3D_DEM_FAIL("bad dimensions");
    if (snx < 2 || sny < 2 || snz < 2) S3D_DEM_FAIL("a source dimension below 2 has no intensity gradient (%d x %d x %d)", snx, sny, snz);
    if (rnx < cfg->hw + 2 || rny < cfg->hw + 2 || rnz < cfg->hw + 2)
        S3D_DEM_FAIL("the reference (%d x %d x %d) is too small for a Gaussian of sigma %g: every dimension must be at least %d", rnx,
                     rny, rnz, cfg->sigma, cfg->hw + 2);
    return SIFT3D_SUCCESS;
}

typedef struct {
    s3d_ref_ctx c;
    double kstep, *d_sums;
    void *d_scr;
    float *u, *v, *tmp;                                     /* device: the field, the updated field, the Gaussian's scratch */
    float taps[2 * 24 + 1];                                 /* sigma <= 8 */
    int width, passes;
} s3d_dem_ctx;

/* one s3d_k_demons_step on level l from d->u into d->v under the level-0 map A0 and the constants K; S: its three sums */
static int s3d_dem_pass(s3d_dem_ctx *const d, const int l, const double A0[12], const double K[4], double S[3])
{
    const s3d_ref_level *const v = &d->c.lv[l];
    double A[12];
    memcpy(A, A0, sizeof(A));
    for (int i = 0; i < 3; i++) A[i * 4 + 3] = A0[i * 4 + 3] / ldexp(1.0, l);
    if (s3d_k_demons_step(v->src, v->sd[0], v->sd[1], v->sd[2], v->ref, v->rd[0], v->rd[1], v->rd[2], A, d->u, d->v, K[0], K[1], K[2],
                          K[3], d->kstep, d->d_sums, d->d_scr, d->c.stream) ||
        s3d_rt_d2h(S, d->d_sums, 3 * sizeof(double), d->c.stream) || s3d_rt_sync(d->c.stream))
        return -1;
    d->passes++;
    return 0;
}

/* One level from the field in d->u, which becomes the result.  Returns the status the level ended with, -2 where its first
 * pass counts no voxel (the level is left out), -1 on a device failure.  *iters grows by the updates applied. */
static int s3d_dem_run_level(s3d_dem_ctx *const d, const int l, const double A0[12], const double K[4], const int max_iter,
                             const double tol, int *const iters)
{
    static const float uf[3] = {1.0f, 1.0f, 1.0f};
    const s3d_ref_level *const lv = &d->c.lv[l];
    const size_t n = S3D_REF_VOX(lv->rd);
    double hist[S3D_DEM_LAG], S[3];
    for (int k = 0; k < max_iter; k++) {
        if (s3d_dem_pass(d, l, A0, K, S)) return -1;
        if (k == 0 && !(S[1] > 0.0)) return -2;
        const double c = S[0] / S[1];
        if (k >= S3D_DEM_LAG && c > (1.0 - tol) * hist[k % S3D_DEM_LAG]) return SIFT3D_AMD_DEMONS_CONVERGED;
        hist[k % S3D_DEM_LAG] = c;
        for (int comp = 0; comp < 3; comp++)
            if (s3d_k_sep_fir(d->v + comp * n, d->u + comp * n, d->tmp, lv->rd[0], lv->rd[1], lv->rd[2], 1, uf, d->taps, d->width,
                              d->c.stream))
                return -1;
        (*iters)++;
    }
    return SIFT3D_AMD_DEMONS_MAX_ITER;
}

/* Both entry points behind their checks.  The field goes to d_field (device, planar) and h_field (host, planar), either of
 * which may be NULL. */
static int s3d_demons_run(const float *d_src, int snx, int sny, int snz, const float *d_ref, int rnx, int rny, int rnz,
                          const void *const tform, const s3d_dem_cfg *const cfg, float *const d_field, float *const h_field,
                          sift3d_amd_demons_info *const info, void *const hip_stream)
{
    s3d_dem_ctx d;
    s3d_ref_plan plan;
    memset(&d, 0, sizeof(d));
    /* the reference of a level must hold the field's Gaussian as well as the refinement's 16 voxels */
    const int min_rdim = cfg->hw + 2 > S3D_REF_MIN_DIM ? cfg->hw + 2 : S3D_REF_MIN_DIM;
    size_t bytes = s3d_ref_plan_pyramid(&d.c, &plan, cfg->levels, S3D_REF_MIN_DIM, min_rdim, d_src, snx, sny, snz, d_ref, rnx, rny, rnz, hip_stream);
    const size_t n0 = S3D_REF_VOX(d.c.lv[0].rd), field_bytes = 3 * n0 * sizeof(float);
    const size_t off_sums = bytes;
    bytes += S3D_REF_ALIGN(3 * sizeof(double));
    const size_t off_scr = bytes;
    bytes += S3D_REF_ALIGN(s3d_k_demons_step_scratch_bytes(rnx, rny, rnz));   /* the finest level has the most workgroups */
    const size_t off_u = bytes, off_v = off_u + S3D_REF_ALIGN(field_bytes), off_tmp = off_v + S3D_REF_ALIGN(field_bytes);
    const size_t off_norm = off_tmp + S3D_REF_ALIGN(n0 * sizeof(float)), norm_bytes = S3D_FIELD_NORM_SLOTS * 3 * sizeof(double);
    bytes = off_norm + norm_bytes;
    unsigned char *d_blk = NULL;
    double *h_norm = NULL;
    Affine ident;
    int rc = SIFT3D_FAILURE, have_ident = 0;
    if (tform == NULL) {                                    /* the identity, as a transform the similarity entry point takes */
        if (init_Affine(&ident, IM_NDIMS)) { s3d_api_set_error("sift3d_amd_register_demons: out of memory"); return SIFT3D_FAILURE; }
        have_ident = 1;
        for (int i = 0; i < 12; i++) ident.A.u.data_double[i] = i % 5 == 0 ? 1.0 : 0.0;
    }
    const Affine *const like = tform != NULL ? (const Affine *)tform : &ident;
    double A[12], K0[4], K[4], S_before[3], S[3];
    memcpy(A, like->A.u.data_double, sizeof(A));
    if (s3d_rt_malloc((void **)&d_blk, bytes)) goto dev_failed;
    d.d_sums = (double *)(d_blk + off_sums);
    d.d_scr = d_blk + off_scr;
    d.u = (float *)(d_blk + off_u);
    d.v = (float *)(d_blk + off_v);
    d.tmp = (float *)(d_blk + off_tmp);
    d.kstep = 1.0 / (4.0 * cfg->max_step * cfg->max_step);
    d.width = 2 * cfg->hw + 1;
    {
        float acc = 0;                                      /* init_Gauss_filter at sigma */
        for (int i = 0; i < d.width; i++) {
            double x = (double)i - cfg->hw;
            x /= cfg->sigma + DBL_EPSILON;
            d.taps[i] = (float)exp(-0.5 * x * x);
            acc += d.taps[i];
        }
        for (int i = 0; i < d.width; i++) d.taps[i] /= acc;
    }
    if (s3d_ref_build_pyramid(&d.c, &plan, d_blk)) goto dev_failed;

    /* the start: the zero field at level 0 */
    if (s3d_ref_constants(&d.c, 0, like, A, cfg->normalize, K0)) goto done;
    if (s3d_rt_memset(d.u, 0, field_bytes, hip_stream) || s3d_dem_pass(&d, 0, A, K0, S_before)) goto dev_failed;
    if (!(S_before[1] > 0.0)) {
        s3d_api_set_error("sift3d_amd_register_demons: the volumes do not overlap under the transform as given");
        goto done;
    }
    int iters = 0, levels_run = 0, status = SIFT3D_AMD_DEMONS_UNCHANGED;
    for (int l = d.c.nlv - 1; l >= 0; l--) {
        const s3d_ref_level *const lv = &d.c.lv[l];
        if (l < d.c.nlv - 1) {                              /* the field of the level above, in this level's voxels */
            const s3d_ref_level *const up = &d.c.lv[l + 1];
            if (s3d_k_field_upsample2(d.u, up->rd[0], up->rd[1], up->rd[2], d.v, lv->rd[0], lv->rd[1], lv->rd[2], hip_stream))
                goto dev_failed;
            float *const t = d.u;
            d.u = d.v;
            d.v = t;
        }
        if (l == 0) memcpy(K, K0, sizeof(K));
        else if (s3d_ref_constants(&d.c, l, like, A, cfg->normalize, K)) goto done;
        const int st = s3d_dem_run_level(&d, l, A, K, cfg->max_iter, cfg->tol, &iters);
        if (st == -1) goto dev_failed;
        if (st == -2) continue;
        levels_run++;
        if (l == 0) status = st;
    }
    if (s3d_dem_pass(&d, 0, A, K0, S)) goto dev_failed;
    const double cost_before = S_before[0] / S_before[1];
    /* (a level 0 that was left out has no status of its own: its field is not returned) */
    const int accepted = status != SIFT3D_AMD_DEMONS_UNCHANGED && S[1] > 0.0 && S[0] / S[1] <= cost_before && S[1] >= cfg->min_overlap * S_before[1];
    if (!accepted) {
        status = SIFT3D_AMD_DEMONS_UNCHANGED;
        iters = 0;
        memcpy(S, S_before, sizeof(S));
        if (s3d_rt_memset(d.u, 0, field_bytes, hip_stream)) goto dev_failed;
    }
    /* the returned field, and the lengths of its entries: per-workgroup partials from the device, added here in slot order */
    if ((h_norm = (double *)malloc(norm_bytes)) == NULL) { s3d_api_set_error("sift3d_amd_register_demons: out of memory"); goto done; }
    if (s3d_k_field_norm(d.u, n0, (double *)(d_blk + off_norm), hip_stream) ||
        s3d_rt_d2h(h_norm, d_blk + off_norm, norm_bytes, hip_stream) ||
        (h_field != NULL && s3d_rt_d2h(h_field, d.u, field_bytes, hip_stream)) ||
        (d_field != NULL && s3d_rt_d2d(d_field, d.u, field_bytes, hip_stream)) || s3d_rt_sync(hip_stream))
        goto dev_failed;
    if (info != NULL) {
        double sum = 0.0, cnt = 0.0, big = 0.0;
        for (int k = 0; k < S3D_FIELD_NORM_SLOTS; k++) {
            sum += h_norm[3 * k];
            cnt += h_norm[3 * k + 1];
            if (h_norm[3 * k + 2] > big) big = h_norm[3 * k + 2];
        }
        info->status = status;
        info->levels_run = levels_run;
        info->iters = iters;
        info->passes = d.passes;
        info->n_before = (long long)S_before[1];
        info->n_after = (long long)S[1];
        info->cost_before = cost_before;
        info->cost_after = S[0] / S[1];
        info->mean_disp = cnt > 0.0 ? sum / cnt : 0.0;
        info->max_disp = big;
    }
    rc = SIFT3D_SUCCESS;
    goto done;
dev_failed:
    s3d_api_set_error("sift3d_amd_register_demons: device failure: %s", s3d_rt_last_error());
done:
    s3d_rt_free(d_blk);
    free(h_norm);
    if (have_ident) cleanup_tform(&ident);
    return rc;
}

int sift3d_amd_register_demons_dev(const float *d_src, int snx, int sny, int snz, const float *d_ref, int rnx, int rny, int rnz,
                                   const void *tform, const sift3d_amd_demons_opts *opts, float *d_field,
                                   sift3d_amd_demons_info *info, void *hip_stream)
{
    s3d_dem_cfg cfg;
    if (s3d_demons_check(tform, opts, &cfg)) return SIFT3D_FAILURE;
    if (d_src == NULL || d_ref == NULL) S3D_DEM_FAIL("NULL data");
    if (d_field == NULL) S3D_DEM_FAIL("NULL field");
    if (s3d_demons_check_dims(&cfg, snx, sny, snz, rnx, rny, rnz)) return SIFT3D_FAILURE;
    return s3d_demons_run(d_src, snx, sny, snz, d_ref, rnx, rny, rnz, tform, &cfg, d_field, NULL, info, hip_stream);
}

/* the volumes of ims (one channel) on the device with default strides; `who` names the caller in a message */
static int s3d_upload_pair(const Image *const ims[2], float *d_im[2], const char *const who)
{
    for (int k = 0; k < 2; k++) {
        const size_t n = (size_t)ims[k]->nx * ims[k]->ny * ims[k]->nz * ims[k]->nc;
        const float *h = ims[k]->data;
        float *packed = NULL;
        if (!s3d_im_is_default_stride(ims[k])) {
            if ((packed = (float *)malloc(n * sizeof(float))) == NULL) { s3d_api_set_error("%s: out of memory", who); return -1; }
            s3d_im_gather(ims[k], packed);
            h = packed;
        }
        const int dev_rc = s3d_rt_malloc((void **)&d_im[k], n * sizeof(float)) || s3d_rt_h2d(d_im[k], h, n * sizeof(float), NULL) ||
                           s3d_rt_sync(NULL);
        free(packed);
        if (dev_rc) { s3d_api_set_error("%s: device failure: %s", who, s3d_rt_last_error()); return -1; }
    }
    return 0;
}

int sift3d_amd_register_demons(const Image *src, const Image *ref, const void *tform, const sift3d_amd_demons_opts *opts,
                               Image *field, sift3d_amd_demons_info *info)
{
    s3d_dem_cfg cfg;
    if (s3d_demons_check(tform, opts, &cfg)) return SIFT3D_FAILURE;
    if (src == NULL || ref == NULL) S3D_DEM_FAIL("NULL image");
    if (field == NULL) S3D_DEM_FAIL("NULL field");
    if (src->nc != 1 || ref->nc != 1) S3D_DEM_FAIL("single-channel volumes only (nc = %d and %d)", src->nc, ref->nc);
    if (src->data == NULL || ref->data == NULL) S3D_DEM_FAIL("NULL data");
    if (s3d_demons_check_dims(&cfg, src->nx, src->ny, src->nz, ref->nx, ref->ny, ref->nz)) return SIFT3D_FAILURE;
    const Image *const ims[2] = {src, ref};
    float *d_im[2] = {NULL, NULL};
    const size_t n = (size_t)ref->nx * ref->ny * ref->nz;
    float *planar = (float *)malloc(3 * n * sizeof(float)), *fresh = (float *)malloc(3 * n * sizeof(float));
    sift3d_amd_demons_info got;
    int rc = SIFT3D_FAILURE;
    if (planar == NULL || fresh == NULL) { s3d_api_set_error("sift3d_amd_register_demons: out of memory"); goto done; }
    if (s3d_upload_pair(ims, d_im, "sift3d_amd_register_demons")) goto done;
    if (s3d_demons_run(d_im[0], src->nx, src->ny, src->nz, d_im[1], ref->nx, ref->ny, ref->nz, tform, &cfg, NULL, planar, &got, NULL))
        goto done;
    for (size_t i = 0; i < n; i++)
        for (int c = 0; c < 3; c++) fresh[3 * i + c] = planar[c * n + i];
    free(field->data);                                      /* nothing can fail from here on: the field takes the new block */
    field->data = fresh;
    fresh = NULL;
    field->size = 3 * n;
    field->nx = ref->nx; field->ny = ref->ny; field->nz = ref->nz;
    field->nc = 3;
    field->ux = ref->ux; field->uy = ref->uy; field->uz = ref->uz;
    im_default_stride(field);
    if (info != NULL) *info = got;
    rc = SIFT3D_SUCCESS;
done:
    s3d_rt_free(d_im[0]); s3d_rt_free(d_im[1]);
    free(planar); free(fresh);
    return rc;
}

int sift3d_amd_im_warp_field(const void *tform, const Image *field, const Image *src, interp_type interp, Image *dst)
{
#define S3D_WF_FAIL(...) do { s3d_api_set_error("sift3d_amd_im_warp_field: " __VA_ARGS__); return SIFT3D_FAILURE; } while (0)
    static const double identity[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    if (tform != NULL) {
        const Affine *const a = (const Affine *)tform;
        if (tform_get_type(tform) != AFFINE || a->A.num_rows != IM_NDIMS || a->A.num_cols != IM_NDIMS + 1 ||
            a->A.type != SIFT3D_DOUBLE || a->A.u.data_double == NULL)
            S3D_WF_FAIL("the transform must be NULL or a 3-D Affine");
    }
    if (interp != LINEAR && interp != LANCZOS2) S3D_WF_FAIL("unrecognized interpolation type %d", (int)interp);
    if (field == NULL || src == NULL || dst == NULL) S3D_WF_FAIL("NULL image");
    if (field->data == NULL || src->data == NULL) S3D_WF_FAIL("NULL data");
    if (field->nc != 3) S3D_WF_FAIL("a field has three channels, not %d", field->nc);
    if (field->nx < 1 || field->ny < 1 || field->nz < 1 || src->nx < 1 || src->ny < 1 || src->nz < 1 || src->nc < 1)
        S3D_WF_FAIL("bad dimensions");
    const double *const A = tform != NULL ? ((const Affine *)tform)->A.u.data_double : identity;
    const size_t n = (size_t)field->nx * field->ny * field->nz, ns = (size_t)src->nx * src->ny * src->nz * src->nc;
    const size_t nd = n * (size_t)src->nc;
    float *planar = (float *)malloc(3 * n * sizeof(float)), *packed = NULL, *d_src = NULL, *d_dst = NULL, *d_u = NULL;
    int rc = SIFT3D_FAILURE;
    if (planar == NULL) { s3d_api_set_error("sift3d_amd_im_warp_field: out of memory"); goto done; }
    for (int z = 0; z < field->nz; z++)                     /* de-interleave (any strides) */
        for (int y = 0; y < field->ny; y++)
            for (int x = 0; x < field->nx; x++)
                for (int c = 0; c < 3; c++)
                    planar[c * n + ((size_t)z * field->ny + y) * field->nx + x] = SIFT3D_IM_GET_VOX(field, x, y, z, c);
    const float *h_src = src->data;
    if (!s3d_im_is_default_stride(src)) {
        if ((packed = (float *)malloc(ns * sizeof(float))) == NULL) { s3d_api_set_error("sift3d_amd_im_warp_field: out of memory"); goto done; }
        s3d_im_gather(src, packed);
        h_src = packed;
    }
    dst->nx = field->nx; dst->ny = field->ny; dst->nz = field->nz;
    dst->nc = src->nc;
    dst->ux = field->ux; dst->uy = field->uy; dst->uz = field->uz;
    im_default_stride(dst);
    if (im_resize(dst)) { s3d_api_set_error("sift3d_amd_im_warp_field: out of memory"); goto done; }
    if (s3d_rt_malloc((void **)&d_src, ns * sizeof(float)) || s3d_rt_malloc((void **)&d_dst, nd * sizeof(float)) ||
        s3d_rt_malloc((void **)&d_u, 3 * n * sizeof(float)) || s3d_rt_h2d(d_src, h_src, ns * sizeof(float), NULL) ||
        s3d_rt_h2d(d_u, planar, 3 * n * sizeof(float), NULL) ||
        s3d_k_inv_field(d_src, src->nx, src->ny, src->nz, src->nc, d_dst, dst->nx, dst->ny, dst->nz, A, d_u, interp == LINEAR ? 0 : 1,
                        NULL) ||
        s3d_rt_d2h(dst->data, d_dst, nd * sizeof(float), NULL) || s3d_rt_sync(NULL)) {
        s3d_api_set_error("sift3d_amd_im_warp_field: device failure: %s", s3d_rt_last_error());
        goto done;
    }
    rc = SIFT3D_SUCCESS;
done:
    s3d_rt_free(d_src); s3d_rt_free(d_dst); s3d_rt_free(d_u);
    free(planar); free(packed);
    return rc;
#undef S3D_WF_FAIL
}

/* ---- the inverse of a field's map, its Jacobian determinant and points through it (sift3d_amd.h) ------------------------------
 * The device inverts (s3d_k_field_invert) and differentiates (s3d_k_field_jacobian); here are the 3 x 3 inverse, the checks, the
 * sums of the per-workgroup partials in slot order and the layout of the host forms. */
static const double s3d_identity34[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};

/* NULL or a 3-D Affine with its matrix in place */
static int s3d_is_affine3_or_null(const void *const tform)
{
    if (tform == NULL) return 1;
    const Affine *const a = (const Affine *)tform;
    return tform_get_type(tform) == AFFINE && a->A.num_rows == IM_NDIMS && a->A.num_cols == IM_NDIMS + 1 &&
           a->A.type == SIFT3D_DOUBLE && a->A.u.data_double != NULL;
}

static const double *s3d_affine34(const void *const tform)
{
    return tform != NULL ? ((const Affine *)tform)->A.u.data_double : s3d_identity34;
}

/* B = A^-1 as a 3 x 4 map, by cofactors; -1 where A's linear part is singular or an entry of A or B is not finite */
static int s3d_invert_affine34(const double A[12], double B[12])
{
    for (int i = 0; i < 12; i++)
        if (!(fabs(A[i]) <= DBL_MAX)) return -1;
    const double c00 = A[5] * A[10] - A[6] * A[9], c01 = A[4] * A[10] - A[6] * A[8], c02 = A[4] * A[9] - A[5] * A[8];
    const double det = A[0] * c00 - A[1] * c01 + A[2] * c02;
    if (!(fabs(det) > 0.0) || !(fabs(det) <= DBL_MAX)) return -1;
    B[0] = c00 / det;
    B[1] = -(A[1] * A[10] - A[2] * A[9]) / det;
    B[2] = (A[1] * A[6] - A[2] * A[5]) / det;
    B[4] = -c01 / det;
    B[5] = (A[0] * A[10] - A[2] * A[8]) / det;
    B[6] = -(A[0] * A[6] - A[2] * A[4]) / det;
    B[8] = c02 / det;
    B[9] = -(A[0] * A[9] - A[1] * A[8]) / det;
    B[10] = (A[0] * A[5] - A[1] * A[4]) / det;
    for (int i = 0; i < 3; i++) B[4 * i + 3] = -((B[4 * i] * A[3] + B[4 * i + 1] * A[7]) + B[4 * i + 2] * A[11]);
    for (int i = 0; i < 12; i++)
        if (!(fabs(B[i]) <= DBL_MAX)) return -1;
    return 0;
}

/* the channels of a field image, any strides, as a planar field */
static void s3d_field_to_planar(const Image *const field, float *const planar)
{
    const size_t n = (size_t)field->nx * field->ny * field->nz;
    for (int z = 0; z < field->nz; z++)
        for (int y = 0; y < field->ny; y++)
            for (int x = 0; x < field->nx; x++)
                for (int c = 0; c < 3; c++)
                    planar[c * n + ((size_t)z * field->ny + y) * field->nx + x] = SIFT3D_IM_GET_VOX(field, x, y, z, c);
}

#define S3D_FI_FAIL(...) do { s3d_api_set_error("sift3d_amd_invert_field: " __VA_ARGS__); return SIFT3D_FAILURE; } while (0)

/* what both forms of the inversion refuse; max_iter, tol: the effective options; A, B: the map and its inverse */
static int s3d_invert_check(const void *const tform, const sift3d_amd_field_inverse_opts *const o, int rnx, int rny, int rnz, int snx,
                            int sny, int snz, int *const max_iter, double *const tol, const double **const A, double B[12])
{
    if (!s3d_is_affine3_or_null(tform))
        S3D_FI_FAIL("the transform must be NULL or a 3-D Affine (a Tps is not supported as the base transform)");
    if (o != NULL) {
        if (o->max_iter < 0) S3D_FI_FAIL("max_iter must not be negative (%d)", o->max_iter);
        if (!(o->tol >= 0.0)) S3D_FI_FAIL("tol must be a number >= 0");
    }
    if (rnx < 1 || rny < 1 || rnz < 1 || snx < 1 || sny < 1 || snz < 1)
        S3D_FI_FAIL("bad dimensions (field %d x %d x %d, source grid %d x %d x %d)", rnx, rny, rnz, snx, sny, snz);
    *max_iter = o != NULL && o->max_iter != 0 ? o->max_iter : SIFT3D_AMD_FIELD_INVERSE_ITER_DEFAULT;
    *tol = o != NULL && o->tol != 0.0 ? o->tol : 1e-3;
    *A = s3d_affine34(tform);
    if (s3d_invert_affine34(*A, B)) S3D_FI_FAIL("the transform's linear part is singular or not finite: the map has no inverse");
    return SIFT3D_SUCCESS;
}

/* the inversion behind its checks: the inverse field to d_w (device, planar), the statistics to *info */
static int s3d_invert_run(const float *d_u, int rnx, int rny, int rnz, const double A[12], const double B[12], float *d_w, int snx,
                          int sny, int snz, int max_iter, double tol, sift3d_amd_field_inverse_info *const info, void *const hip_stream)
{
    const size_t part_bytes = (size_t)S3D_FIELD_INV_SLOTS * S3D_FIELD_INV_STATS * sizeof(double);
    double *d_part = NULL, *h_part = (double *)malloc(part_bytes);
    int rc = SIFT3D_FAILURE;
    if (h_part == NULL) { s3d_api_set_error("sift3d_amd_invert_field: out of memory"); goto done; }
    if (s3d_rt_malloc((void **)&d_part, part_bytes) ||
        s3d_k_field_invert(d_u, rnx, rny, rnz, A, B, d_w, snx, sny, snz, max_iter, tol, NULL, d_part, hip_stream) ||
        s3d_rt_d2h(h_part, d_part, part_bytes, hip_stream) || s3d_rt_sync(hip_stream)) {
        s3d_api_set_error("sift3d_amd_invert_field: device failure: %s", s3d_rt_last_error());
        goto done;
    }
    if (info != NULL) {
        double s[S3D_FIELD_INV_STATS] = {0};
        for (int k = 0; k < S3D_FIELD_INV_SLOTS; k++) {
            const double *const p = h_part + (size_t)k * S3D_FIELD_INV_STATS;
            for (int j = 0; j < 6; j++) s[j] += p[j];
            if (p[6] > s[6]) s[6] = p[6];
        }
        info->n = (long long)snx * sny * snz;
        info->n_converged = (long long)s[0];
        info->n_outside = (long long)s[1];
        info->n_not_converged = (long long)s[2];
        info->n_invalid = (long long)s[3];
        info->updates = (long long)s[4];
        const double valid = (s[0] + s[1]) + s[2];
        info->mean_residual = valid > 0.0 ? s[5] / valid : 0.0;
        info->max_residual = s[6];
    }
    rc = SIFT3D_SUCCESS;
done:
    s3d_rt_free(d_part);
    free(h_part);
    return rc;
}

int sift3d_amd_invert_field_dev(const float *d_field, int rnx, int rny, int rnz, const void *tform, float *d_inv_field, int snx,
                                int sny, int snz, const sift3d_amd_field_inverse_opts *opts, double inv_A[12],
                                sift3d_amd_field_inverse_info *info, void *hip_stream)
{
    int max_iter;
    double tol, B[12];
    const double *A;
    if (d_field == NULL || d_inv_field == NULL) S3D_FI_FAIL("NULL data");
    if (inv_A == NULL) S3D_FI_FAIL("NULL inverse transform");
    if (s3d_invert_check(tform, opts, rnx, rny, rnz, snx, sny, snz, &max_iter, &tol, &A, B)) return SIFT3D_FAILURE;
    sift3d_amd_field_inverse_info got;
    if (s3d_invert_run(d_field, rnx, rny, rnz, A, B, d_inv_field, snx, sny, snz, max_iter, tol, &got, hip_stream)) return SIFT3D_FAILURE;
    memcpy(inv_A, B, sizeof(B));
    if (info != NULL) *info = got;
    return SIFT3D_SUCCESS;
}

int sift3d_amd_invert_field(const void *tform, const Image *field, int snx, int sny, int snz, const double src_units[3],
                            const sift3d_amd_field_inverse_opts *opts, Affine *inv_tform, Image *inv_field,
                            sift3d_amd_field_inverse_info *info)
{
    int max_iter;
    double tol, B[12];
    const double *A;
    if (field == NULL || inv_field == NULL) S3D_FI_FAIL("NULL image");
    if (inv_tform == NULL) S3D_FI_FAIL("NULL inverse transform");
    if (!s3d_is_affine3_or_null(inv_tform)) S3D_FI_FAIL("the inverse transform must be an initialised 3-D Affine");
    if (field->data == NULL) S3D_FI_FAIL("NULL data");
    if (field->nc != 3) S3D_FI_FAIL("a field has three channels, not %d", field->nc);
    if (src_units != NULL && !(src_units[0] > 0.0 && src_units[1] > 0.0 && src_units[2] > 0.0)) S3D_FI_FAIL("source units must be positive");
    if (s3d_invert_check(tform, opts, field->nx, field->ny, field->nz, snx, sny, snz, &max_iter, &tol, &A, B)) return SIFT3D_FAILURE;
    const size_t rn = (size_t)field->nx * field->ny * field->nz, sn = (size_t)snx * sny * snz;
    float *planar = (float *)malloc(3 * (rn > sn ? rn : sn) * sizeof(float)), *fresh = (float *)malloc(3 * sn * sizeof(float));
    float *d_u = NULL, *d_w = NULL;
    sift3d_amd_field_inverse_info got;
    int rc = SIFT3D_FAILURE;
    if (planar == NULL || fresh == NULL) { s3d_api_set_error("sift3d_amd_invert_field: out of memory"); goto done; }
    s3d_field_to_planar(field, planar);
    if (s3d_rt_malloc((void **)&d_u, 3 * rn * sizeof(float)) || s3d_rt_malloc((void **)&d_w, 3 * sn * sizeof(float)) ||
        s3d_rt_h2d(d_u, planar, 3 * rn * sizeof(float), NULL) || s3d_rt_sync(NULL)) {
        s3d_api_set_error("sift3d_amd_invert_field: device failure: %s", s3d_rt_last_error());
        goto done;
    }
    if (s3d_invert_run(d_u, field->nx, field->ny, field->nz, A, B, d_w, snx, sny, snz, max_iter, tol, &got, NULL)) goto done;
    if (s3d_rt_d2h(planar, d_w, 3 * sn * sizeof(float), NULL) || s3d_rt_sync(NULL)) {
        s3d_api_set_error("sift3d_amd_invert_field: device failure: %s", s3d_rt_last_error());
        goto done;
    }
    for (size_t i = 0; i < sn; i++)
        for (int c = 0; c < 3; c++) fresh[3 * i + c] = planar[c * sn + i];
    free(inv_field->data);                                  /* nothing can fail from here on */
    inv_field->data = fresh;
    fresh = NULL;
    inv_field->size = 3 * sn;
    inv_field->nx = snx; inv_field->ny = sny; inv_field->nz = snz;
    inv_field->nc = 3;
    inv_field->ux = src_units != NULL ? src_units[0] : 1.0;
    inv_field->uy = src_units != NULL ? src_units[1] : 1.0;
    inv_field->uz = src_units != NULL ? src_units[2] : 1.0;
    im_default_stride(inv_field);
    memcpy(inv_tform->A.u.data_double, B, sizeof(B));
    if (info != NULL) *info = got;
    rc = SIFT3D_SUCCESS;
done:
    s3d_rt_free(d_u); s3d_rt_free(d_w);
    free(planar); free(fresh);
    return rc;
}
#undef S3D_FI_FAIL

#define S3D_FJ_FAIL(...) do { s3d_api_set_error("sift3d_amd_field_jacobian: " __VA_ARGS__); return SIFT3D_FAILURE; } while (0)

/* the determinant behind its checks: the map to d_det (device, may be NULL), the statistics to *info */
static int s3d_jacobian_run(const float *d_u, int rnx, int rny, int rnz, const double A[12], float *d_det,
                            sift3d_amd_field_jacobian_info *const info, void *const hip_stream)
{
    const size_t part_bytes = (size_t)S3D_FIELD_JAC_SLOTS * S3D_FIELD_JAC_STATS * sizeof(double);
    double *d_part = NULL, *h_part = (double *)malloc(part_bytes);
    int rc = SIFT3D_FAILURE;
    if (h_part == NULL) { s3d_api_set_error("sift3d_amd_field_jacobian: out of memory"); goto done; }
    if (s3d_rt_malloc((void **)&d_part, part_bytes) || s3d_k_field_jacobian(d_u, rnx, rny, rnz, A, d_det, d_part, hip_stream) ||
        s3d_rt_d2h(h_part, d_part, part_bytes, hip_stream) || s3d_rt_sync(hip_stream)) {
        s3d_api_set_error("sift3d_amd_field_jacobian: device failure: %s", s3d_rt_last_error());
        goto done;
    }
    if (info != NULL) {
        double sum = 0.0, cnt = 0.0, fold = 0.0, lo = 0.0, hi = 0.0;
        for (int k = 0; k < S3D_FIELD_JAC_SLOTS; k++) {
            const double *const p = h_part + (size_t)k * S3D_FIELD_JAC_STATS;
            if (!(p[1] > 0.0)) continue;
            if (!(cnt > 0.0) || p[3] < lo) lo = p[3];
            if (!(cnt > 0.0) || p[4] > hi) hi = p[4];
            sum += p[0];
            cnt += p[1];
            fold += p[2];
        }
        info->n = (long long)rnx * rny * rnz;
        info->n_finite = (long long)cnt;
        info->n_folded = (long long)fold;
        info->min_det = cnt > 0.0 ? lo : NAN;
        info->max_det = cnt > 0.0 ? hi : NAN;
        info->mean_det = cnt > 0.0 ? sum / cnt : NAN;
    }
    rc = SIFT3D_SUCCESS;
done:
    s3d_rt_free(d_part);
    free(h_part);
    return rc;
}

static int s3d_jacobian_check(const void *const tform, int rnx, int rny, int rnz)
{
    if (!s3d_is_affine3_or_null(tform))
        S3D_FJ_FAIL("the transform must be NULL or a 3-D Affine (a Tps is not supported as the base transform)");
    if (rnx < 2 || rny < 2 || rnz < 2) S3D_FJ_FAIL("every dimension must be at least 2 (%d x %d x %d)", rnx, rny, rnz);
    return SIFT3D_SUCCESS;
}

int sift3d_amd_field_jacobian_dev(const float *d_field, int rnx, int rny, int rnz, const void *tform, float *d_det,
                                  sift3d_amd_field_jacobian_info *info, void *hip_stream)
{
    if (d_field == NULL) S3D_FJ_FAIL("NULL data");
    if (d_det == NULL && info == NULL) S3D_FJ_FAIL("neither a determinant map nor statistics asked for");
    if (s3d_jacobian_check(tform, rnx, rny, rnz)) return SIFT3D_FAILURE;
    sift3d_amd_field_jacobian_info got;
    if (s3d_jacobian_run(d_field, rnx, rny, rnz, s3d_affine34(tform), d_det, &got, hip_stream)) return SIFT3D_FAILURE;
    if (info != NULL) *info = got;
    return SIFT3D_SUCCESS;
}

int sift3d_amd_field_jacobian(const void *tform, const Image *field, Image *det, sift3d_amd_field_jacobian_info *info)
{
    if (field == NULL) S3D_FJ_FAIL("NULL image");
    if (det == NULL && info == NULL) S3D_FJ_FAIL("neither a determinant map nor statistics asked for");
    if (field->data == NULL) S3D_FJ_FAIL("NULL data");
    if (field->nc != 3) S3D_FJ_FAIL("a field has three channels, not %d", field->nc);
    if (s3d_jacobian_check(tform, field->nx, field->ny, field->nz)) return SIFT3D_FAILURE;
    const size_t n = (size_t)field->nx * field->ny * field->nz;
    float *planar = (float *)malloc(3 * n * sizeof(float)), *fresh = det != NULL ? (float *)malloc(n * sizeof(float)) : NULL;
    float *d_u = NULL, *d_det = NULL;
    sift3d_amd_field_jacobian_info got;
    int rc = SIFT3D_FAILURE;
    if (planar == NULL || (det != NULL && fresh == NULL)) { s3d_api_set_error("sift3d_amd_field_jacobian: out of memory"); goto done; }
    s3d_field_to_planar(field, planar);
    if (s3d_rt_malloc((void **)&d_u, 3 * n * sizeof(float)) || (det != NULL && s3d_rt_malloc((void **)&d_det, n * sizeof(float))) ||
        s3d_rt_h2d(d_u, planar, 3 * n * sizeof(float), NULL) || s3d_rt_sync(NULL)) {
        s3d_api_set_error("sift3d_amd_field_jacobian: device failure: %s", s3d_rt_last_error());
        goto done;
    }
    if (s3d_jacobian_run(d_u, field->nx, field->ny, field->nz, s3d_affine34(tform), d_det, &got, NULL)) goto done;
    if (det != NULL) {
        if (s3d_rt_d2h(fresh, d_det, n * sizeof(float), NULL) || s3d_rt_sync(NULL)) {
            s3d_api_set_error("sift3d_amd_field_jacobian: device failure: %s", s3d_rt_last_error());
            goto done;
        }
        free(det->data);                                    /* nothing can fail from here on */
        det->data = fresh;
        fresh = NULL;
        det->size = n;
        det->nx = field->nx; det->ny = field->ny; det->nz = field->nz;
        det->nc = 1;
        det->ux = field->ux; det->uy = field->uy; det->uz = field->uz;
        im_default_stride(det);
    }
    if (info != NULL) *info = got;
    rc = SIFT3D_SUCCESS;
done:
    s3d_rt_free(d_u); s3d_rt_free(d_det);
    free(planar); free(fresh);
    return rc;
}
#undef S3D_FJ_FAIL

/* s3d_k_field_invert's steps 3 and 4 on the host, for channel c of a field image: the same expression, the same order */
static double s3d_field_sample_clamped(const Image *const f, const int c, double tx, double ty, double tz)
{
    const double hx = (double)(f->nx - 1), hy = (double)(f->ny - 1), hz = (double)(f->nz - 1);
    tx = tx < 0.0 ? 0.0 : tx > hx ? hx : tx;
    ty = ty < 0.0 ? 0.0 : ty > hy ? hy : ty;
    tz = tz < 0.0 ? 0.0 : tz > hz ? hz : tz;
    const int fx = (int)floor(tx), fy = (int)floor(ty), fz = (int)floor(tz);
    const int cx = (int)ceil(tx), cy = (int)ceil(ty), cz = (int)ceil(tz);
    const double dx = tx - fx, dy = ty - fy, dz = tz - fz;
    const double c0 = SIFT3D_IM_GET_VOX(f, fx, fy, fz, c), c1 = SIFT3D_IM_GET_VOX(f, fx, cy, fz, c);
    const double c2 = SIFT3D_IM_GET_VOX(f, cx, fy, fz, c), c3 = SIFT3D_IM_GET_VOX(f, cx, cy, fz, c);
    const double c4 = SIFT3D_IM_GET_VOX(f, fx, fy, cz, c), c5 = SIFT3D_IM_GET_VOX(f, fx, cy, cz, c);
    const double c6 = SIFT3D_IM_GET_VOX(f, cx, fy, cz, c), c7 = SIFT3D_IM_GET_VOX(f, cx, cy, cz, c);
    return c0 * (1.0 - dx) * (1.0 - dy) * (1.0 - dz) + c1 * (1.0 - dx) * dy * (1.0 - dz) +
           c2 * dx * (1.0 - dy) * (1.0 - dz) + c3 * dx * dy * (1.0 - dz) +
           c4 * (1.0 - dx) * (1.0 - dy) * dz + c5 * (1.0 - dx) * dy * dz +
           c6 * dx * (1.0 - dy) * dz + c7 * dx * dy * dz;
}

int sift3d_amd_field_apply_points(const void *tform, const Image *field, const Mat_rm *in, Mat_rm *out)
{
#define S3D_FP_FAIL(...) do { s3d_api_set_error("sift3d_amd_field_apply_points: " __VA_ARGS__); return SIFT3D_FAILURE; } while (0)
    if (!s3d_is_affine3_or_null(tform))
        S3D_FP_FAIL("the transform must be NULL or a 3-D Affine (a Tps is not supported as the base transform)");
    if (field == NULL || in == NULL || out == NULL) S3D_FP_FAIL("NULL argument");
    if (field->data == NULL) S3D_FP_FAIL("NULL data");
    if (field->nc != 3) S3D_FP_FAIL("a field has three channels, not %d", field->nc);
    if (field->nx < 1 || field->ny < 1 || field->nz < 1) S3D_FP_FAIL("bad dimensions");
    if (in->type != SIFT3D_DOUBLE || in->num_rows != IM_NDIMS || in->num_cols < 0 || (in->num_cols > 0 && in->u.data_double == NULL))
        S3D_FP_FAIL("the points must be a 3 x n matrix of doubles");
    const double *const A = s3d_affine34(tform);
    const size_t n = (size_t)in->num_cols;
    double *res = NULL;
    if (n > 0 && (res = (double *)malloc(3 * n * sizeof(double))) == NULL) S3D_FP_FAIL("out of memory");
    for (size_t j = 0; j < n; j++) {
        const double x = in->u.data_double[j], y = in->u.data_double[n + j], z = in->u.data_double[2 * n + j];
        const int ok = fabs(x) <= DBL_MAX && fabs(y) <= DBL_MAX && fabs(z) <= DBL_MAX;     /* a NaN has no cell: NaN out */
        for (int i = 0; i < 3; i++) {
            const double t = A[4 * i] * x + A[4 * i + 1] * y + A[4 * i + 2] * z + A[4 * i + 3];
            res[i * n + j] = ok ? t + s3d_field_sample_clamped(field, i, x, y, z) : NAN;
        }
    }
    out->type = SIFT3D_DOUBLE;
    out->num_rows = IM_NDIMS;
    out->num_cols = in->num_cols;
    if (resize_Mat_rm(out)) { free(res); S3D_FP_FAIL("out of memory"); }
    if (n > 0) memcpy(out->u.data_double, res, 3 * n * sizeof(double));
    free(res);
    return SIFT3D_SUCCESS;
#undef S3D_FP_FAIL
}
#undef S3D_REF_VOX
#undef S3D_REF_ALIGN
