/* s3d_resample.hip -- the device unit of the registration tail: the inverse affine warp of a
 * volume, the inverse thin-plate-spline warp, the consensus counts of find_tform_ransac's hypotheses and, at the end of the
 * file, the similarity scores of a registration (the warp's pass that accumulates instead of storing).
 *
 * im_inv_transform (imutil/imutil.c:2040-2085): every output voxel (x, y, z) is pushed through the
 * transform, (tx, ty, tz) = A [x y z 1]^T in f64 (apply_Affine_xyz, imutil.c:2651-2672), and the source
 * is sampled there: tri-linear (resample_linear, imutil.c:2087-2127) or the 5^3 Lanczos-2 window
 * (resample_lanczos2, imutil.c:2129-2175), all in f64 with the reference's operation order and no
 * contraction, result cast to float; outside [0, n-1] the sample is 0.  One thread per output voxel;
 * x-consecutive lanes keep the gathers of a near-identity transform coalesced.  The tri-linear form is
 * bit-identical to the reference; Lanczos goes through device sin(), so it agrees to ~1e-15 relative. */
#include "s3d_common.h"
#include "../../include/s3d_device.h"

struct AffineD { double a[12]; };          /* 3 x 4, row major */

__device__ __forceinline__ double s3d_lanczos2(double x)
{
    const double pi_x = 3.14159265358979323846 * x;
    return 2.0 * sin(pi_x) * sin(pi_x / 2.0) / (pi_x * pi_x);
}

/* Whether s3d_sample_store samples at (tx, ty, tz): not outside [0, n - 1] on any axis and no NaN coordinate (NaN coordinates
 * fail every comparison in the reference and would index out of range there). */
__device__ __forceinline__ bool s3d_sample_inside(int snx, int sny, int snz, double tx, double ty, double tz)
{
    const bool outside = tx < 0 || tx > snx - 1 || ty < 0 || ty > sny - 1 || tz < 0 || tz > snz - 1;
    return !(outside || !(tx == tx) || !(ty == ty) || !(tz == tz));
}

/* resample_linear's expression at (tx, ty, tz), inside [0, n - 1] on every axis, in f64 before any rounding to float: p the
 * channel's first element, the strides in floats.  s3d_sample_store<0> stores its float; the field inversion iterates on it. */
__device__ __forceinline__ double s3d_trilinear_f64(const float *__restrict__ p, size_t sxs, size_t sys, size_t szs, double tx,
                                                    double ty, double tz)
{
    const int fx = (int)floor(tx), fy = (int)floor(ty), fz = (int)floor(tz);
    const int cx = (int)ceil(tx), cy = (int)ceil(ty), cz = (int)ceil(tz);
    const double dx = tx - fx, dy = ty - fy, dz = tz - fz;
    const double c0 = p[fx * sxs + fy * sys + fz * szs], c1 = p[fx * sxs + cy * sys + fz * szs];
    const double c2 = p[cx * sxs + fy * sys + fz * szs], c3 = p[cx * sxs + cy * sys + fz * szs];
    const double c4 = p[fx * sxs + fy * sys + cz * szs], c5 = p[fx * sxs + cy * sys + cz * szs];
    const double c6 = p[cx * sxs + fy * sys + cz * szs], c7 = p[cx * sxs + cy * sys + cz * szs];
    return c0 * (1.0 - dx) * (1.0 - dy) * (1.0 - dz) + c1 * (1.0 - dx) * dy * (1.0 - dz) +
           c2 * dx * (1.0 - dy) * (1.0 - dz) + c3 * dx * dy * (1.0 - dz) +
           c4 * (1.0 - dx) * (1.0 - dy) * dz + c5 * (1.0 - dx) * dy * dz +
           c6 * dx * (1.0 - dy) * dz + c7 * dx * dy * dz;
}

/* The sample of src at (tx, ty, tz), every channel, to out[0 .. nc): the reference's resample_linear / resample_lanczos2.
 * Shared by the affine and the spline warp and by the similarity kernels. */
template <int INTERP>
__device__ __forceinline__ void s3d_sample_store(const float *__restrict__ src, int snx, int sny, int snz, int nc,
                                                 float *__restrict__ out, double tx, double ty, double tz)
{
    const size_t sxs = (size_t)nc, sys = (size_t)nc * snx, szs = (size_t)nc * snx * sny;
    if (!s3d_sample_inside(snx, sny, snz, tx, ty, tz)) {
        for (int c = 0; c < nc; c++) out[c] = 0.0f;
        return;
    }
    if (INTERP == 0) {
        for (int c = 0; c < nc; c++) out[c] = (float)s3d_trilinear_f64(src + c, sxs, sys, szs, tx, ty, tz);
    } else {
        const double a = 2.0;
        const double flx = floor(tx), fly = floor(ty), flz = floor(tz);
        const int x0 = (int)(flx - a > 0.0 ? flx - a : 0.0), x1 = (int)(flx + a < snx - 1 ? flx + a : (double)(snx - 1));
        const int y0 = (int)(fly - a > 0.0 ? fly - a : 0.0), y1 = (int)(fly + a < sny - 1 ? fly + a : (double)(sny - 1));
        const int z0 = (int)(flz - a > 0.0 ? flz - a : 0.0), z1 = (int)(flz + a < snz - 1 ? flz + a : (double)(snz - 1));
        for (int c = 0; c < nc; c++) {
            double val = 0.0;
            for (int zs = z0; zs <= z1; zs++)
                for (int ys = y0; ys <= y1; ys++)
                    for (int xs = x0; xs <= x1; xs++) {
                        const double xw = fabs((double)xs - tx) + 2.220446049250313e-16;
                        const double yw = fabs((double)ys - ty) + 2.220446049250313e-16;
                        const double zw = fabs((double)zs - tz) + 2.220446049250313e-16;
                        const double k = s3d_lanczos2(xw) * s3d_lanczos2(yw) * s3d_lanczos2(zw);
                        val += k * (double)src[xs * sxs + ys * sys + zs * szs + c];
                    }
            out[c] = (float)val;
        }
    }
}

/* (tx, ty, tz) = A [x y z 1]^T, left to right, every operation rounded (apply_Affine_xyz); shared by the affine warp and the
 * affine similarity kernel, so both see the same bits */
__device__ __forceinline__ void s3d_affine_xyz(const AffineD &A, double xd, double yd, double zd, double &tx, double &ty, double &tz)
{
    tx = A.a[0] * xd + A.a[1] * yd + A.a[2] * zd + A.a[3];
    ty = A.a[4] * xd + A.a[5] * yd + A.a[6] * zd + A.a[7];
    tz = A.a[8] * xd + A.a[9] * yd + A.a[10] * zd + A.a[11];
}

template <int INTERP>
__global__ void __launch_bounds__(256)
k_inv_affine(const float *__restrict__ src, int snx, int sny, int snz, int nc, float *__restrict__ dst, int dnx, int dny,
             int dnz, AffineD A)
{
    const int x = blockIdx.x * 256 + threadIdx.x;
    const int y = blockIdx.y, z = blockIdx.z;
    if (x >= dnx) return;
    const double xd = (double)x, yd = (double)y, zd = (double)z;
    double tx, ty, tz;
    s3d_affine_xyz(A, xd, yd, zd, tx, ty, tz);
    float *out = dst + (((size_t)z * dny + y) * dnx + x) * nc;
    s3d_sample_store<INTERP>(src, snx, sny, snz, nc, out, tx, ty, tz);
}

/* d_src: snx x sny x snz x nc (channels interleaved), d_dst: dnx x dny x dnz x nc; A: 3 x 4 row-major
 * doubles mapping output voxel coordinates to source voxel coordinates; interp 0 = linear, 1 = Lanczos-2. */
extern "C" int s3d_k_inv_affine(const float *d_src, int snx, int sny, int snz, int nc, float *d_dst, int dnx, int dny,
                                int dnz, const double A[12], int interp, s3d_stream stream)
{
    if (snx < 1 || sny < 1 || snz < 1 || nc < 1 || dnx < 1 || dny < 1 || dnz < 1) S3D_FAIL("bad dimensions");
    if (dny > 65535 || dnz > 65535) S3D_FAIL("volume too large for the resampling grid");
    AffineD a;
    for (int i = 0; i < 12; i++) a.a[i] = A[i];
    const dim3 grid(s3d_div_up(dnx, 256), dny, dnz);
    if (interp == 0)
        hipLaunchKernelGGL((k_inv_affine<0>), grid, dim3(256), 0, (hipStream_t)stream, d_src, snx, sny, snz, nc, d_dst, dnx,
                           dny, dnz, a);
    else if (interp == 1)
        hipLaunchKernelGGL((k_inv_affine<1>), grid, dim3(256), 0, (hipStream_t)stream, d_src, snx, sny, snz, nc, d_dst, dnx,
                           dny, dnz, a);
    else
        S3D_FAIL("unrecognized interpolation type");
    S3D_CHECK_LAUNCH();
    return S3D_OK;
}

/* ---- inverse thin-plate-spline warp (im_inv_transform through apply_Tps_xyz, imutil.c:2676-2729) --------------------------
 * One thread per output voxel, x-consecutive lanes as above.  Every voxel sums U(r2) = r2 log r2 over all control points in
 * f64: the kernel is bound by the f64 log, not by memory.  A control point is six doubles (its coordinates and its three
 * weights) that every lane of the workgroup needs at the same time: the workgroup stages S3D_TPS_TILE of them in LDS
 * (6 KiB) and each lane reads them from there at one address (a broadcast, no bank conflict), so any n_ctrl streams through.
 * Control points ascend; the sum uses fused multiply-adds (fewer roundings than the reference's, 5 f64 instructions less per
 * point: 84 f64 VALU instructions per voxel and point in all, 73 of them the log; 104 VGPRs, no private segment; 256^3 x 512
 * points in 22.6 ms, 82 % of the f64 issue rate, profiles/tps_warp_cost.txt); r2 == 0 is tested explicitly, since control points sit on voxels of the output grid and 0 * log(0) is NaN.  The
 * tail -- the constant, then the x, y and z terms -- is the reference's expression, separately rounded (this file is compiled
 * without contraction), so n_ctrl = 0 gives the reference's bits.  No lane leaves before the last barrier. */
/* The spline's coordinates of voxel (xd, yd, zd) for every thread of a 256-thread workgroup: the control-point loop through
 * the LDS tile s_pt (S3D_TPS_TILE * 6 doubles), then the tail.  Collective: every thread of the workgroup calls it, the same
 * number of times (it holds barriers).  again: s_pt may still be read from an earlier call of this workgroup.  Shared by the
 * spline warp and the spline similarity kernel. */
__device__ __forceinline__ void s3d_tps_xyz(double *s_pt, const double *__restrict__ ctrl, const double *__restrict__ params,
                                            uint32_t n_ctrl, bool again, double xd, double yd, double zd, double &tx_out,
                                            double &ty_out, double &tz_out)
{
    const size_t row = (size_t)n_ctrl + 4;                  /* row length of params */
    double tx = 0.0, ty = 0.0, tz = 0.0;
    for (uint32_t n0 = 0; n0 < n_ctrl; n0 += S3D_TPS_TILE) {
        const uint32_t nt = n_ctrl - n0 < (uint32_t)S3D_TPS_TILE ? n_ctrl - n0 : (uint32_t)S3D_TPS_TILE;
        if (n0 || again) __syncthreads();                   /* the previous tile has been read by every lane */
        for (uint32_t e = threadIdx.x; e < nt * 6u; e += 256u) {
            const uint32_t j = e / 6u, k = e - j * 6u;
            s_pt[e] = k < 3u ? ctrl[(size_t)(n0 + j) * 3 + k] : params[(size_t)(k - 3u) * row + n0 + j];
        }
        __syncthreads();
        for (uint32_t j = 0; j < nt; j++) {
            const double *p = s_pt + j * 6u;
            const double dx = xd - p[0], dy = yd - p[1], dz = zd - p[2];
            const double r2 = fma(dz, dz, fma(dy, dy, dx * dx));
            const double u = r2 == 0.0 ? 0.0 : r2 * log(r2);
            tx = fma(u, p[3], tx);
            ty = fma(u, p[4], ty);
            tz = fma(u, p[5], tz);
        }
    }
    const double *ax = params + n_ctrl, *ay = ax + row, *az = ay + row;
    tx += ax[0]; tx += ax[1] * xd; tx += ax[2] * yd; tx += ax[3] * zd;
    ty += ay[0]; ty += ay[1] * xd; ty += ay[2] * yd; ty += ay[3] * zd;
    tz += az[0]; tz += az[1] * xd; tz += az[2] * yd; tz += az[3] * zd;
    tx_out = tx; ty_out = ty; tz_out = tz;
}

template <int INTERP>
__global__ void __launch_bounds__(256)
k_inv_tps(const float *__restrict__ src, int snx, int sny, int snz, int nc, float *__restrict__ dst, int dnx, int dny, int dnz,
          const double *__restrict__ ctrl, const double *__restrict__ params, uint32_t n_ctrl)
{
    __shared__ double s_pt[S3D_TPS_TILE * 6];               /* per point: x y z w_x w_y w_z */
    const int x = blockIdx.x * 256 + threadIdx.x;
    const int y = blockIdx.y, z = blockIdx.z;
    const double xd = (double)x, yd = (double)y, zd = (double)z;
    double tx, ty, tz;
    s3d_tps_xyz(s_pt, ctrl, params, n_ctrl, false, xd, yd, zd, tx, ty, tz);
    if (x >= dnx) return;
    float *out = dst + (((size_t)z * dny + y) * dnx + x) * nc;
    s3d_sample_store<INTERP>(src, snx, sny, snz, nc, out, tx, ty, tz);
}

/* d_ctrl: n_ctrl x 3, d_params: 3 x (n_ctrl + 4), row-major doubles (the Tps struct's kp_src and params); the rest as above. */
extern "C" int s3d_k_inv_tps(const float *d_src, int snx, int sny, int snz, int nc, float *d_dst, int dnx, int dny, int dnz,
                             const double *d_ctrl, const double *d_params, uint32_t n_ctrl, int interp, s3d_stream stream)
{
    if (snx < 1 || sny < 1 || snz < 1 || nc < 1 || dnx < 1 || dny < 1 || dnz < 1) S3D_FAIL("bad dimensions");
    if (dny > 65535 || dnz > 65535) S3D_FAIL("volume too large for the resampling grid");
    if (d_params == NULL || (n_ctrl > 0 && d_ctrl == NULL)) S3D_FAIL("missing spline parameters");
    const dim3 grid(s3d_div_up(dnx, 256), dny, dnz);
    if (interp == 0)
        hipLaunchKernelGGL((k_inv_tps<0>), grid, dim3(256), 0, (hipStream_t)stream, d_src, snx, sny, snz, nc, d_dst, dnx, dny,
                           dnz, d_ctrl, d_params, n_ctrl);
    else if (interp == 1)
        hipLaunchKernelGGL((k_inv_tps<1>), grid, dim3(256), 0, (hipStream_t)stream, d_src, snx, sny, snz, nc, d_dst, dnx, dny,
                           dnz, d_ctrl, d_params, n_ctrl);
    else
        S3D_FAIL("unrecognized interpolation type");
    S3D_CHECK_LAUNCH();
    return S3D_OK;
}

/* ---- RANSAC consensus counts (find_tform_ransac's scoring loop, imutil.c:4527-4552 + 4802-4815) ---------------------------
 * counts[m] = #{ i : !(e(i, m) > thr2) }, e the squared residual of match i under model m in f64, with the host loop's
 * operation order and no contraction, so a count is the integer the host loop finds.  One thread keeps one match (six doubles
 * in registers) and walks the S3D_RANSAC_TILE models of its workgroup; a model's address is wave-uniform, so its twelve
 * doubles arrive through the scalar cache and cost no vector or LDS bandwidth.  Per model one __ballot + popcount per wave,
 * the four waves' partial sums in LDS, and at the end one integer atomicAdd per model per workgroup: integer sums do not
 * depend on the order, so the counts are exact whatever the schedule.  No thread leaves early (the ballots are collective). */
__global__ void __launch_bounds__(256)
k_ransac_count(const double *__restrict__ src, const double *__restrict__ ref, uint32_t npts, const double *__restrict__ models,
               uint32_t nmodels, double thr2, int *__restrict__ counts)
{
    __shared__ int s_part[4][S3D_RANSAC_TILE];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t i = blockIdx.x * 256u + tid;
    const bool valid = i < npts;
    double x = 0.0, y = 0.0, z = 0.0, s0 = 0.0, s1 = 0.0, s2 = 0.0;
    if (valid) {
        const double *r = ref + (size_t)i * 3, *s = src + (size_t)i * 3;
        x = r[0]; y = r[1]; z = r[2];
        s0 = s[0]; s1 = s[1]; s2 = s[2];
    }
    const uint32_t m0 = blockIdx.y * (uint32_t)S3D_RANSAC_TILE;
    const uint32_t nm = nmodels - m0 < (uint32_t)S3D_RANSAC_TILE ? nmodels - m0 : (uint32_t)S3D_RANSAC_TILE;
    for (uint32_t j = 0; j < nm; j++) {
        const double *A = models + (size_t)(m0 + j) * 12;
        const double xo = A[0] * x + A[1] * y + A[2] * z + A[3];
        const double yo = A[4] * x + A[5] * y + A[6] * z + A[7];
        const double zo = A[8] * x + A[9] * y + A[10] * z + A[11];
        const double e = (s0 - xo) * (s0 - xo) + (s1 - yo) * (s1 - yo) + (s2 - zo) * (s2 - zo);
        const unsigned long long in = __ballot(valid && !(e > thr2));     /* the host's `if (e > thr2) continue;` */
        if (lane == 0) s_part[wave][j] = __popcll(in);
    }
    __syncthreads();
    if (tid < nm) {
        const int c = s_part[0][tid] + s_part[1][tid] + s_part[2][tid] + s_part[3][tid];
        if (c) atomicAdd(&counts[m0 + tid], c);
    }
}

/* d_src, d_ref: npts x 3 row-major doubles; d_models: nmodels x 12 (3 x 4 row major); d_counts: nmodels ints, zeroed here. */
extern "C" int s3d_k_ransac_count(const double *d_src, const double *d_ref, uint32_t npts, const double *d_models,
                                  uint32_t nmodels, double thr2, int *d_counts, s3d_stream stream)
{
    if (npts < 1 || nmodels < 1) S3D_FAIL("bad dimensions");
    if (npts > 0x7fffffffu) S3D_FAIL("too many matches for an int count");
    const unsigned gy = s3d_div_up(nmodels, S3D_RANSAC_TILE);
    if (gy > 65535u) S3D_FAIL("too many models for the scoring grid");
    S3D_HIP(hipMemsetAsync(d_counts, 0, (size_t)nmodels * sizeof(int), (hipStream_t)stream));
    hipLaunchKernelGGL(k_ransac_count, dim3(s3d_div_up(npts, 256), gy), dim3(256), 0, (hipStream_t)stream, d_src, d_ref, npts,
                       d_models, nmodels, thr2, d_counts);
    S3D_CHECK_LAUNCH();
    return S3D_OK;
}

/* ---- similarity of a source under a transform against a reference (sift3d_amd_im_similarity) -------------------------------
 * The warp's pass -- every reference voxel through the transform, the source sampled there -- that accumulates instead of
 * storing: the joint histogram of (reference voxel a, sample b) and seven f64 sums over the overlap, the voxels that
 * s3d_sample_store samples and whose two values are finite.  The warped volume is never written.  The coordinates come from
 * s3d_affine_xyz / s3d_tps_xyz and the sample from s3d_sample_store, the functions of the warp kernels, so a voxel's (a, b) is
 * what im_inv_transform would have stored beside the reference.
 *
 * Workgroups are persistent: workgroup g walks the reference rows g, g + G, g + 2G, .. (a row: rnx voxels at one y, z), 256
 * x-consecutive voxels at a time, G = s3d_sim_grid(rows, rnx, bins) -- a function of the dimensions and the bin count alone, so the
 * voxels of a thread, and with them every f64 sum, are the same in every call.  The joint histogram is private to the workgroup
 * in LDS, bins^2 32-bit counters (4 bins^2 bytes: 16 KiB at 64 bins, 64 KiB at 128; the launcher keeps the voxels of a
 * workgroup below 2^32), and is flushed once, non-zero counters only, with 64-bit integer atomicAdds: integer sums do not depend
 * on the order.  The seven sums have no atomics: a thread's registers, then the wave by shuffles, the four waves through LDS in
 * wave order, and the workgroup's seven partials to its own slot of the scratch; k_sim_finish adds the slots in a fixed order
 * (lane l takes slots l, l + 64, .., then the same shuffle tree).  The spline form stages the control points through LDS as
 * k_inv_tps does; there every thread of the workgroup stays in the loop (s3d_tps_xyz holds barriers).
 * AGG: one round of wave-level aggregation before the LDS atomic (s3d_k_similarity_set_aggregate).  Measured, it does not pay:
 * same-counter atomics of a wave cost nothing visible even with 98 % of the voxels in one bin (profiles/similarity_cost.txt). */
struct SimBins { double ref_lo, ref_scale, src_lo, src_scale, c_ref, c_src; };
#define S3D_SIM_NSUM 7
#define S3D_SIM_AGGREGATE_DEFAULT 0                         /* decided by profiles/similarity_cost.txt */
#define S3D_SIM_CUS 256                                     /* the MI355X's compute units: the grid is a constant of the build */

__device__ __forceinline__ bool s3d_finite_f(float v) { return fabsf(v) <= 3.4028234663852886e38f; }   /* false for NaN */

__device__ __forceinline__ int s3d_sim_bin(float v, double lo, double scale, int bins)
{
    const double t = ((double)v - lo) * scale;
    return t < 0 ? 0 : t >= bins ? bins - 1 : (int)t;
}

/* sum over the wave to lane 0, a fixed tree */
__device__ __forceinline__ double s3d_wave_sum_f64(double v)
{
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_down(v, d);
    return v;
}

/* workgroups of a similarity launch: as many as the LDS (160 KiB per CU; the histogram, the spline tile, the partials) and
 * the wave slots (8 workgroups of 4 waves) let be resident on S3D_SIM_CUS compute units, no more than there are rows, and no
 * more than give every workgroup S3D_SIM_MIN_VOX voxels (its histogram is cleared and flushed, its sums reduced, once) */
#define S3D_SIM_MIN_VOX 2048
static unsigned s3d_sim_grid(size_t rows, size_t rnx, int bins)
{
    const size_t lds = (size_t)4 * bins * bins + S3D_TPS_TILE * 6 * sizeof(double) + 4 * S3D_SIM_NSUM * sizeof(double);
    size_t per_cu = (size_t)160 * 1024 / lds;
    if (per_cu > 8) per_cu = 8;
    size_t g = (size_t)S3D_SIM_CUS * per_cu;
    const size_t by_work = (rows * rnx + S3D_SIM_MIN_VOX - 1) / S3D_SIM_MIN_VOX;
    if (g > by_work) g = by_work;
    return (unsigned)(rows < g ? rows : g);
}

template <int INTERP, bool TPS, bool AGG>
__global__ void __launch_bounds__(256)
k_similarity(const float *__restrict__ src, int snx, int sny, int snz, const float *__restrict__ ref, int rnx, int rny,
             uint32_t rows, AffineD A, const double *__restrict__ ctrl, const double *__restrict__ params, uint32_t n_ctrl,
             int bins, SimBins R, unsigned long long *__restrict__ hist, double *__restrict__ partials)
{
    S3D_DYN_LDS(uint32_t, s_hist);                          /* bins * bins counters, row = reference bin */
    __shared__ double s_pt[TPS ? S3D_TPS_TILE * 6 : 1];
    __shared__ double s_red[4][S3D_SIM_NSUM];
    const uint32_t tid = threadIdx.x, nb2 = (uint32_t)(bins * bins);
    for (uint32_t i = tid; i < nb2; i += 256u) s_hist[i] = 0u;
    __syncthreads();
    double sum[S3D_SIM_NSUM];
    for (int k = 0; k < S3D_SIM_NSUM; k++) sum[k] = 0.0;
    bool again = false;
    for (uint32_t row = blockIdx.x; row < rows; row += gridDim.x) {
        const uint32_t z = row / (uint32_t)rny, y = row - z * (uint32_t)rny;
        const double yd = (double)y, zd = (double)z;
        for (int x0 = 0; x0 < rnx; x0 += 256) {
            const int x = x0 + (int)tid;
            const double xd = (double)x;
            double tx, ty, tz;
            if (TPS) {
                s3d_tps_xyz(s_pt, ctrl, params, n_ctrl, again, xd, yd, zd, tx, ty, tz);
                again = true;
            } else {
                s3d_affine_xyz(A, xd, yd, zd, tx, ty, tz);
            }
            int cell = -1;                                  /* the voxel's counter; -1: not in the overlap */
            if (x < rnx && s3d_sample_inside(snx, sny, snz, tx, ty, tz)) {
                const float a = ref[(size_t)row * rnx + x];
                float b;
                s3d_sample_store<INTERP>(src, snx, sny, snz, 1, &b, tx, ty, tz);
                if (s3d_finite_f(a) && s3d_finite_f(b)) {
                    const int ia = s3d_sim_bin(a, R.ref_lo, R.ref_scale, bins), ib = s3d_sim_bin(b, R.src_lo, R.src_scale, bins);
                    cell = ia * bins + ib;
                    const double ap = (double)a - R.c_ref, bp = (double)b - R.c_src, d = (double)a - (double)b;
                    sum[0] += ap;
                    sum[1] += bp;
                    sum[2] += ap * ap;
                    sum[3] += bp * bp;
                    sum[4] += ap * bp;
                    sum[5] += d * d;
                    sum[6] += fabs(d);
                }
            }
            if (AGG) {
                /* one round of wave-level aggregation: the lanes that share the first counted lane's counter add their number
                 * with one atomic (the background bin of a medical volume), the others add one each */
                const unsigned long long counted = __ballot(cell >= 0);
                if (counted) {                              /* wave-uniform */
                    const int first = __ffsll(counted) - 1;
                    const int c0 = __shfl(cell, first);
                    const unsigned long long same = __ballot(cell == c0);
                    if (cell == c0) {
                        if ((int)(tid & 63u) == first) atomicAdd(&s_hist[c0], (uint32_t)__popcll(same));
                    } else if (cell >= 0) {
                        atomicAdd(&s_hist[cell], 1u);
                    }
                }
            } else if (cell >= 0) {
                atomicAdd(&s_hist[cell], 1u);
            }
        }
    }
    const uint32_t lane = tid & 63u, wave = tid >> 6;
    for (int k = 0; k < S3D_SIM_NSUM; k++) {
        const double v = s3d_wave_sum_f64(sum[k]);
        if (lane == 0) s_red[wave][k] = v;
    }
    __syncthreads();                                        /* the histogram is complete, the waves' sums are in LDS */
    if (tid < S3D_SIM_NSUM)
        partials[(size_t)blockIdx.x * S3D_SIM_NSUM + tid] = ((s_red[0][tid] + s_red[1][tid]) + s_red[2][tid]) + s_red[3][tid];
    for (uint32_t i = tid; i < nb2; i += 256u) {
        const uint32_t c = s_hist[i];
        if (c) atomicAdd(&hist[i], (unsigned long long)c);
    }
}

/* sums[k] = the slots' k-th partials, added in a fixed order: wave k of 7, lane l takes slots l, l + 64, .. */
__global__ void __launch_bounds__(64 * S3D_SIM_NSUM)
k_sim_finish(const double *__restrict__ partials, uint32_t nslots, double *__restrict__ sums)
{
    const uint32_t lane = threadIdx.x & 63u, k = threadIdx.x >> 6;
    double v = 0.0;
    for (uint32_t s = lane; s < nslots; s += 64u) v += partials[(size_t)s * S3D_SIM_NSUM + k];
    v = s3d_wave_sum_f64(v);
    if (lane == 0) sums[k] = v;
}

/* whether the calling thread's launches aggregate equal counters within a wave before the LDS atomic (profiling knob) */
static thread_local int g_sim_aggregate = S3D_SIM_AGGREGATE_DEFAULT;
extern "C" void s3d_k_similarity_set_aggregate(int on) { g_sim_aggregate = on < 0 ? S3D_SIM_AGGREGATE_DEFAULT : on != 0; }
extern "C" int s3d_k_similarity_get_aggregate(void) { return g_sim_aggregate; }

extern "C" size_t s3d_k_similarity_scratch_bytes(int rnx, int rny, int rnz, int bins)
{
    if (rnx < 1 || rny < 1 || rnz < 1 || bins < 2 || bins > S3D_SIM_MAX_BINS) return 0;
    return (size_t)s3d_sim_grid((size_t)rny * rnz, (size_t)rnx, bins) * S3D_SIM_NSUM * sizeof(double);
}

/* a histogram of 128 bins is 64 KiB of dynamic LDS beside the static tiles, above what a launch gets by default: raise the
 * limit of the four kernels once per device, as s3d_k_describe does for its kernel */
static int s3d_sim_prepare(void)
{
#if !defined(S3D_EMU)
    static unsigned char done[64];
    int dev = 0;
    S3D_HIP(hipGetDevice(&dev));
    if (dev < 0 || dev >= 64 || !done[dev]) {
        const int bytes = 4 * S3D_SIM_MAX_BINS * S3D_SIM_MAX_BINS;
#define S3D_SIM_RAISE(I, T, G) \
    S3D_HIP(hipFuncSetAttribute((const void *)k_similarity<I, T, G>, hipFuncAttributeMaxDynamicSharedMemorySize, bytes))
        S3D_SIM_RAISE(0, false, false); S3D_SIM_RAISE(1, false, false); S3D_SIM_RAISE(0, true, false); S3D_SIM_RAISE(1, true, false);
        S3D_SIM_RAISE(0, false, true); S3D_SIM_RAISE(1, false, true); S3D_SIM_RAISE(0, true, true); S3D_SIM_RAISE(1, true, true);
#undef S3D_SIM_RAISE
        if (dev >= 0 && dev < 64) done[dev] = 1;
    }
#endif
    return S3D_OK;
}

static int s3d_sim_launch(bool tps, const float *d_src, int snx, int sny, int snz, const float *d_ref, int rnx, int rny, int rnz,
                          const double A[12], const double *d_ctrl, const double *d_params, uint32_t n_ctrl, int interp, int bins,
                          double ref_lo, double ref_scale, double src_lo, double src_scale, double c_ref, double c_src,
                          unsigned long long *d_hist, double *d_sums, void *d_scratch, s3d_stream stream)
{
    if (snx < 1 || sny < 1 || snz < 1 || rnx < 1 || rny < 1 || rnz < 1) S3D_FAIL("bad dimensions");
    if (bins < 2 || bins > S3D_SIM_MAX_BINS) S3D_FAIL("bins outside 2 .. 128");
    if (interp != 0 && interp != 1) S3D_FAIL("unrecognized interpolation type");
    if (d_src == NULL || d_ref == NULL || d_hist == NULL || d_sums == NULL || d_scratch == NULL) S3D_FAIL("missing buffer");
    if (tps && (d_params == NULL || (n_ctrl > 0 && d_ctrl == NULL))) S3D_FAIL("missing spline parameters");
    const size_t rows = (size_t)rny * rnz;
    if (rows > 0x7fffffffu) S3D_FAIL("volume too large for the similarity grid");
    const unsigned grid = s3d_sim_grid(rows, (size_t)rnx, bins);
    /* a workgroup's 32-bit counters: its rows times the row length */
    if ((rows + grid - 1) / grid * (size_t)rnx > 0xffffffffu) S3D_FAIL("volume too large for the workgroups' 32-bit counters");
    if (s3d_sim_prepare()) return S3D_ERR;
    AffineD a;
    for (int i = 0; i < 12; i++) a.a[i] = A ? A[i] : 0.0;
    const SimBins R = {ref_lo, ref_scale, src_lo, src_scale, c_ref, c_src};
    const size_t lds = (size_t)4 * bins * bins;
    double *part = (double *)d_scratch;
    S3D_HIP(hipMemsetAsync(d_hist, 0, (size_t)bins * bins * sizeof(unsigned long long), (hipStream_t)stream));
#define S3D_SIM_GO(I, T, G)                                                                                                       \
    hipLaunchKernelGGL((k_similarity<I, T, G>), dim3(grid), dim3(256), lds, (hipStream_t)stream, d_src, snx, sny, snz, d_ref, rnx, \
                       rny, (uint32_t)rows, a, d_ctrl, d_params, n_ctrl, bins, R, d_hist, part)
#define S3D_SIM_GO2(I, T) do { if (g_sim_aggregate) S3D_SIM_GO(I, T, true); else S3D_SIM_GO(I, T, false); } while (0)
    if (tps) { if (interp == 0) S3D_SIM_GO2(0, true); else S3D_SIM_GO2(1, true); }
    else { if (interp == 0) S3D_SIM_GO2(0, false); else S3D_SIM_GO2(1, false); }
#undef S3D_SIM_GO2
#undef S3D_SIM_GO
    S3D_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_sim_finish, dim3(1), dim3(64 * S3D_SIM_NSUM), 0, (hipStream_t)stream, part, (uint32_t)grid, d_sums);
    S3D_CHECK_LAUNCH();
    return S3D_OK;
}

extern "C" int s3d_k_similarity_affine(const float *d_src, int snx, int sny, int snz, const float *d_ref, int rnx, int rny,
                                       int rnz, const double A[12], int interp, int bins, double ref_lo, double ref_scale,
                                       double src_lo, double src_scale, double c_ref, double c_src, unsigned long long *d_hist,
                                       double *d_sums, void *d_scratch, s3d_stream stream)
{
    if (A == NULL) S3D_FAIL("missing affine matrix");
    return s3d_sim_launch(false, d_src, snx, sny, snz, d_ref, rnx, rny, rnz, A, NULL, NULL, 0, interp, bins, ref_lo, ref_scale,
                          src_lo, src_scale, c_ref, c_src, d_hist, d_sums, d_scratch, stream);
}

extern "C" int s3d_k_similarity_tps(const float *d_src, int snx, int sny, int snz, const float *d_ref, int rnx, int rny, int rnz,
                                    const double *d_ctrl, const double *d_params, uint32_t n_ctrl, int interp, int bins,
                                    double ref_lo, double ref_scale, double src_lo, double src_scale, double c_ref, double c_src,
                                    unsigned long long *d_hist, double *d_sums, void *d_scratch, s3d_stream stream)
{
    return s3d_sim_launch(true, d_src, snx, sny, snz, d_ref, rnx, rny, rnz, NULL, d_ctrl, d_params, n_ctrl, interp, bins, ref_lo,
                          ref_scale, src_lo, src_scale, c_ref, c_src, d_hist, d_sums, d_scratch, stream);
}

/* ---- minimum and maximum over the finite voxels (the default ranges of the joint histogram) --------------------------------
 * Order-free: the bit pattern of a finite float under the usual order-preserving map to unsigned (negative: all bits flipped,
 * else the sign bit set) is reduced with integer maxima only -- the maximum over the map, the minimum as the maximum over its
 * complement -- so the result does not depend on the schedule.  Both encodings of a finite float are non-zero; a zero word
 * after the pass says that no voxel was finite and decodes to NaN.  d_minmax: two floats, used as two words in between. */
__device__ __forceinline__ uint32_t s3d_ord_f32(float v)
{
    const uint32_t u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__global__ void __launch_bounds__(256)
k_minmax_finite(const float *__restrict__ v, size_t n, uint32_t *__restrict__ enc /* [0]: ~min, [1]: max */)
{
    uint32_t emax = 0u, emin = 0u;
    for (size_t i = (size_t)blockIdx.x * 256u + threadIdx.x; i < n; i += (size_t)gridDim.x * 256u) {
        const float f = v[i];
        if (s3d_finite_f(f)) {
            const uint32_t e = s3d_ord_f32(f);
            emax = e > emax ? e : emax;
            emin = ~e > emin ? ~e : emin;
        }
    }
    for (int d = 32; d >= 1; d >>= 1) {
        const uint32_t omax = __shfl_down(emax, d), omin = __shfl_down(emin, d);
        emax = omax > emax ? omax : emax;
        emin = omin > emin ? omin : emin;
    }
    if ((threadIdx.x & 63u) == 0) {
        if (emin) atomicMax(&enc[0], emin);
        if (emax) atomicMax(&enc[1], emax);
    }
}

__global__ void k_minmax_decode(uint32_t *enc)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const uint32_t e[2] = {enc[0] ? ~enc[0] : 0u, enc[1]};
    for (int k = 0; k < 2; k++) {
        const uint32_t u = e[k] == 0u ? 0x7fc00000u : (e[k] & 0x80000000u) ? (e[k] & 0x7fffffffu) : ~e[k];
        enc[k] = u;
    }
}

extern "C" int s3d_k_minmax_finite(const float *d_v, size_t n, float *d_minmax, s3d_stream stream)
{
    if (n < 1 || d_v == NULL || d_minmax == NULL) S3D_FAIL("bad dimensions");
    size_t g = (n + 256 * 16 - 1) / (256 * 16);
    if (g > 2048) g = 2048;
    S3D_HIP(hipMemsetAsync(d_minmax, 0, 2 * sizeof(uint32_t), (hipStream_t)stream));
    hipLaunchKernelGGL(k_minmax_finite, dim3((unsigned)g), dim3(256), 0, (hipStream_t)stream, d_v, n, (uint32_t *)d_minmax);
    S3D_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_minmax_decode, dim3(1), dim3(64), 0, (hipStream_t)stream, (uint32_t *)d_minmax);
    S3D_CHECK_LAUNCH();
    return S3D_OK;
}

/* ---- normal equations of one Gauss-Newton step of an intensity-based affine fit (sift3d_amd_refine_affine) ------------------
 * The similarity pass once more -- every reference voxel through the affine map, the source sampled there -- accumulating the 74
 * sums of s3d_k_affine_normal_eq (include/s3d_device.h: the terms, their operation order and the index layout) instead of the
 * histogram.  The coordinates come from s3d_affine_xyz and the sample b from s3d_sample_store, so a voxel's (a, b) and its overlap
 * are the similarity pass's; the gradient of the tri-linear interpolant is taken on the cell [X0, X0 + 1] x [Y0, Y0 + 1] x
 * [Z0, Z0 + 1], X0 = min(floor(tx), snx - 2), which is the sampled cell except on the last plane of an axis, where it is the
 * cell below (a one-sided derivative; the launcher refuses a source dimension < 2).
 *
 * Workgroups are persistent as in k_similarity: workgroup g walks the rows g, g + G, .., 256 x-consecutive voxels at a time,
 * G = s3d_neq_grid(rows, rnx), a function of the dimensions alone.  A thread keeps the 74 sums in registers (148 VGPRs; the
 * kernel runs at the occupancy that leaves, no private segment: DESIGN.md), then the wave by shuffles, the four waves through
 * LDS in wave order, the workgroup's partials to its own slot of the scratch, and k_neq_finish adds the slots in a fixed order
 * (workgroup k of 74, lane l takes slots l, l + 64, .., then the same shuffle tree).  No floating-point atomics.  The count is
 * carried as a sum of 1.0: integer-valued doubles below 2^53 add exactly in any order.  Every product below is its own rounded
 * f64 operation (the file is compiled without contraction), so a term is the same f64 here and under the emulator. */
#define S3D_NEQ_NSUM S3D_NEQ_SUMS
#define S3D_NEQ_WG_PER_CU 2                                 /* resident workgroups per compute unit at the kernel's registers */
struct NeqConst { double cx, cy, cz, sa, ma, sb, mb; };

__device__ __forceinline__ bool s3d_finite_d(double v) { return fabs(v) <= 1.7976931348623157e308; }   /* false for NaN */

/* workgroups of a normal-equation launch: what is resident on S3D_SIM_CUS compute units, no more than there are rows and no
 * more than give every workgroup S3D_SIM_MIN_VOX voxels (its 74 sums are reduced once) */
static unsigned s3d_neq_grid(size_t rows, size_t rnx)
{
    size_t g = (size_t)S3D_SIM_CUS * S3D_NEQ_WG_PER_CU;
    const size_t by_work = (rows * rnx + S3D_SIM_MIN_VOX - 1) / S3D_SIM_MIN_VOX;
    if (g > by_work) g = by_work;
    return (unsigned)(rows < g ? rows : g);
}

__global__ void __launch_bounds__(256)
k_affine_normal_eq(const float *__restrict__ src, int snx, int sny, int snz, const float *__restrict__ ref, int rnx, int rny,
                   uint32_t rows, AffineD A, NeqConst K, double *__restrict__ partials)
{
    __shared__ double s_red[4][S3D_NEQ_NSUM];
    const uint32_t tid = threadIdx.x;
    const size_t sys = (size_t)snx, szs = (size_t)snx * sny;
    double sum[S3D_NEQ_NSUM];
#pragma unroll
    for (int k = 0; k < S3D_NEQ_NSUM; k++) sum[k] = 0.0;
    for (uint32_t row = blockIdx.x; row < rows; row += gridDim.x) {
        const uint32_t z = row / (uint32_t)rny, y = row - z * (uint32_t)rny;
        const double yd = (double)y, zd = (double)z;
        const double qy = yd - K.cy, qz = zd - K.cz;
        for (int x0 = 0; x0 < rnx; x0 += 256) {
            const int x = x0 + (int)tid;
            const double xd = (double)x;
            double tx, ty, tz;
            s3d_affine_xyz(A, xd, yd, zd, tx, ty, tz);
            if (!(x < rnx && s3d_sample_inside(snx, sny, snz, tx, ty, tz))) continue;
            const float a = ref[(size_t)row * rnx + x];
            float b;
            s3d_sample_store<0>(src, snx, sny, snz, 1, &b, tx, ty, tz);
            /* the gradient's cell and the position in it: fx, fy, fz in [0, 1], 1 only on the last plane */
            int X0 = (int)floor(tx), Y0 = (int)floor(ty), Z0 = (int)floor(tz);
            X0 = X0 < snx - 2 ? X0 : snx - 2;
            Y0 = Y0 < sny - 2 ? Y0 : sny - 2;
            Z0 = Z0 < snz - 2 ? Z0 : snz - 2;
            const double fx = tx - (double)X0, fy = ty - (double)Y0, fz = tz - (double)Z0;
            const double ux = 1.0 - fx, uy = 1.0 - fy, uz = 1.0 - fz;
            const float *p = src + ((size_t)X0 + (size_t)Y0 * sys + (size_t)Z0 * szs);
            const double c000 = p[0], c100 = p[1], c010 = p[sys], c110 = p[sys + 1];
            const double c001 = p[szs], c101 = p[szs + 1], c011 = p[szs + sys], c111 = p[szs + sys + 1];
            double gx = ((c100 - c000) * uy + (c110 - c010) * fy) * uz + ((c101 - c001) * uy + (c111 - c011) * fy) * fz;
            double gy = ((c010 - c000) * ux + (c110 - c100) * fx) * uz + ((c011 - c001) * ux + (c111 - c101) * fx) * fz;
            double gz = ((c001 - c000) * ux + (c101 - c100) * fx) * uy + ((c011 - c010) * ux + (c111 - c110) * fx) * fy;
            gx = K.sb * gx;
            gy = K.sb * gy;
            gz = K.sb * gz;
            if (!(s3d_finite_f(a) && s3d_finite_f(b) && s3d_finite_d(gx) && s3d_finite_d(gy) && s3d_finite_d(gz))) continue;
            const double r = K.sb * ((double)b - K.mb) - K.sa * ((double)a - K.ma);
            const double qx = xd - K.cx;
            const double gg[6] = {gx * gx, gx * gy, gx * gz, gy * gy, gy * gz, gz * gz};
            const double qq[10] = {qx * qx, qx * qy, qx * qz, qx, qy * qy, qy * qz, qy, qz * qz, qz, 1.0};
#pragma unroll
            for (int i = 0; i < 6; i++)
#pragma unroll
                for (int k = 0; k < 10; k++) sum[i * 10 + k] += gg[i] * qq[k];
            const double rg[3] = {r * gx, r * gy, r * gz};
#pragma unroll
            for (int i = 0; i < 3; i++) {
                sum[60 + i * 4 + 0] += rg[i] * qx;
                sum[60 + i * 4 + 1] += rg[i] * qy;
                sum[60 + i * 4 + 2] += rg[i] * qz;
                sum[60 + i * 4 + 3] += rg[i];
            }
            sum[72] += r * r;
            sum[73] += 1.0;
        }
    }
    const uint32_t lane = tid & 63u, wave = tid >> 6;
#pragma unroll
    for (int k = 0; k < S3D_NEQ_NSUM; k++) {
        const double v = s3d_wave_sum_f64(sum[k]);
        if (lane == 0) s_red[wave][k] = v;
    }
    __syncthreads();
    if (tid < S3D_NEQ_NSUM)
        partials[(size_t)blockIdx.x * S3D_NEQ_NSUM + tid] = ((s_red[0][tid] + s_red[1][tid]) + s_red[2][tid]) + s_red[3][tid];
}

/* sums[k] = the slots' k-th partials, added in a fixed order: workgroup k of 74 (one wave), lane l takes slots l, l + 64, .. */
__global__ void __launch_bounds__(64)
k_neq_finish(const double *__restrict__ partials, uint32_t nslots, double *__restrict__ sums)
{
    const uint32_t lane = threadIdx.x, k = blockIdx.x;
    double v = 0.0;
    for (uint32_t s = lane; s < nslots; s += 64u) v += partials[(size_t)s * S3D_NEQ_NSUM + k];
    v = s3d_wave_sum_f64(v);
    if (lane == 0) sums[k] = v;
}

extern "C" size_t s3d_k_affine_normal_eq_scratch_bytes(int rnx, int rny, int rnz)
{
    if (rnx < 1 || rny < 1 || rnz < 1) return 0;
    return (size_t)s3d_neq_grid((size_t)rny * rnz, (size_t)rnx) * S3D_NEQ_NSUM * sizeof(double);
}

extern "C" int s3d_k_affine_normal_eq(const float *d_src, int snx, int sny, int snz, const float *d_ref, int rnx, int rny, int rnz,
                                      const double A[12], const double c[3], double sa, double ma, double sb, double mb,
                                      double *d_sums, void *d_scratch, s3d_stream stream)
{
    if (snx < 1 || sny < 1 || snz < 1 || rnx < 1 || rny < 1 || rnz < 1) S3D_FAIL("bad dimensions");
    if (snx < 2 || sny < 2 || snz < 2) S3D_FAIL("a source dimension below 2 has no intensity gradient");
    if (d_src == NULL || d_ref == NULL || d_sums == NULL || d_scratch == NULL) S3D_FAIL("missing buffer");
    if (A == NULL || c == NULL) S3D_FAIL("missing affine matrix or centre");
    const size_t rows = (size_t)rny * rnz;
    if (rows > 0x7fffffffu) S3D_FAIL("volume too large for the normal-equation grid");
    const unsigned grid = s3d_neq_grid(rows, (size_t)rnx);
    AffineD a;
    for (int i = 0; i < 12; i++) a.a[i] = A[i];
    const NeqConst K = {c[0], c[1], c[2], sa, ma, sb, mb};
    double *part = (double *)d_scratch;
    hipLaunchKernelGGL(k_affine_normal_eq, dim3(grid), dim3(256), 0, (hipStream_t)stream, d_src, snx, sny, snz, d_ref, rnx, rny,
                       (uint32_t)rows, a, K, part);
    S3D_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_neq_finish, dim3(S3D_NEQ_NSUM), dim3(64), 0, (hipStream_t)stream, part, (uint32_t)grid, d_sums);
    S3D_CHECK_LAUNCH();
    return S3D_OK;
}

/* ---- deformable registration: the demons update, the warp through a displacement field, the field one level up -------------
 * (sift3d_amd_register_demons; include/s3d_device.h has the definitions).  A field is planar: component c of voxel i at
 * d_u[c * N + i], so a wave reads and writes 256 contiguous bytes per component and a component is a one-channel volume to
 * s3d_k_sep_fir.
 *
 * k_demons_step is k_affine_normal_eq with three sums for 74: the same persistent workgroups over rows, the same sample, cell and
 * gradient at the voxel's coordinates -- here the affine map plus the voxel's own displacement -- and the same reduction (thread,
 * wave by shuffles, four waves through LDS in wave order, one slot of partials per workgroup, k_demons_finish in a fixed order).
 * A voxel reads and writes only its own field entry, so the update may be made in place.  Three sums leave the registers to
 * the gathers (89 VGPRs, five waves per SIMD, no private segment: DESIGN.md); the grid is what is resident at that. */
#define S3D_DEM_NSUM 3
#define S3D_DEM_WG_PER_CU 5                                 /* resident workgroups per compute unit at the kernel's registers */
struct DemConst { double sa, ma, sb, mb, kstep; };

static unsigned s3d_dem_grid(size_t rows, size_t rnx)
{
    size_t g = (size_t)S3D_SIM_CUS * S3D_DEM_WG_PER_CU;
    const size_t by_work = (rows * rnx + S3D_SIM_MIN_VOX - 1) / S3D_SIM_MIN_VOX;
    if (g > by_work) g = by_work;
    return (unsigned)(rows < g ? rows : g);
}

__global__ void __launch_bounds__(256)
k_demons_step(const float *__restrict__ src, int snx, int sny, int snz, const float *__restrict__ ref, int rnx, int rny,
              uint32_t rows, AffineD A, DemConst K, const float *u, float *v, size_t nvox, double *__restrict__ partials)
{
    __shared__ double s_red[4][S3D_DEM_NSUM];
    const uint32_t tid = threadIdx.x;
    const size_t sys = (size_t)snx, szs = (size_t)snx * sny;
    double sum_rr = 0.0, sum_n = 0.0, sum_dd = 0.0;
    for (uint32_t row = blockIdx.x; row < rows; row += gridDim.x) {
        const uint32_t z = row / (uint32_t)rny, y = row - z * (uint32_t)rny;
        const double yd = (double)y, zd = (double)z;
        for (int x0 = 0; x0 < rnx; x0 += 256) {
            const int x = x0 + (int)tid;
            if (x >= rnx) continue;
            const size_t i = (size_t)row * rnx + x;
            const float u0 = u[i], u1 = u[nvox + i], u2 = u[2 * nvox + i];
            double tx, ty, tz;
            s3d_affine_xyz(A, (double)x, yd, zd, tx, ty, tz);
            tx = tx + (double)u0;
            ty = ty + (double)u1;
            tz = tz + (double)u2;
            bool moved = false;
            if (s3d_sample_inside(snx, sny, snz, tx, ty, tz)) {
                const float a = ref[i];
                float b;
                s3d_sample_store<0>(src, snx, sny, snz, 1, &b, tx, ty, tz);
                int X0 = (int)floor(tx), Y0 = (int)floor(ty), Z0 = (int)floor(tz);
                X0 = X0 < snx - 2 ? X0 : snx - 2;
                Y0 = Y0 < sny - 2 ? Y0 : sny - 2;
                Z0 = Z0 < snz - 2 ? Z0 : snz - 2;
                const double fx = tx - (double)X0, fy = ty - (double)Y0, fz = tz - (double)Z0;
                const double ux = 1.0 - fx, uy = 1.0 - fy, uz = 1.0 - fz;
                const float *p = src + ((size_t)X0 + (size_t)Y0 * sys + (size_t)Z0 * szs);
                const double c000 = p[0], c100 = p[1], c010 = p[sys], c110 = p[sys + 1];
                const double c001 = p[szs], c101 = p[szs + 1], c011 = p[szs + sys], c111 = p[szs + sys + 1];
                double gx = ((c100 - c000) * uy + (c110 - c010) * fy) * uz + ((c101 - c001) * uy + (c111 - c011) * fy) * fz;
                double gy = ((c010 - c000) * ux + (c110 - c100) * fx) * uz + ((c011 - c001) * ux + (c111 - c101) * fx) * fz;
                double gz = ((c001 - c000) * ux + (c101 - c100) * fx) * uy + ((c011 - c010) * ux + (c111 - c110) * fx) * fy;
                gx = K.sb * gx;
                gy = K.sb * gy;
                gz = K.sb * gz;
                if (s3d_finite_f(a) && s3d_finite_f(b) && s3d_finite_d(gx) && s3d_finite_d(gy) && s3d_finite_d(gz)) {
                    const double r = K.sb * ((double)b - K.mb) - K.sa * ((double)a - K.ma);
                    const double D = ((gx * gx + gy * gy) + gz * gz) + K.kstep * (r * r);
                    sum_rr += r * r;
                    sum_n += 1.0;
                    if (D > 0.0 && s3d_finite_d(D)) {
                        const double m = (-r) / D;
                        const double dx = m * gx, dy = m * gy, dz = m * gz;
                        v[i] = (float)((double)u0 + dx);
                        v[nvox + i] = (float)((double)u1 + dy);
                        v[2 * nvox + i] = (float)((double)u2 + dz);
                        sum_dd += (dx * dx + dy * dy) + dz * dz;
                        moved = true;
                    }
                }
            }
            if (!moved && v != u) {                         /* the entry as it is, bit for bit (a NaN keeps its payload) */
                const s3d_u32a *ub = (const s3d_u32a *)u;
                s3d_u32a *vb = (s3d_u32a *)v;
                vb[i] = ub[i];
                vb[nvox + i] = ub[nvox + i];
                vb[2 * nvox + i] = ub[2 * nvox + i];
            }
        }
    }
    const uint32_t lane = tid & 63u, wave = tid >> 6;
    const double w0 = s3d_wave_sum_f64(sum_rr), w1 = s3d_wave_sum_f64(sum_n), w2 = s3d_wave_sum_f64(sum_dd);
    if (lane == 0) {
        s_red[wave][0] = w0;
        s_red[wave][1] = w1;
        s_red[wave][2] = w2;
    }
    __syncthreads();
    if (tid < S3D_DEM_NSUM)
        partials[(size_t)blockIdx.x * S3D_DEM_NSUM + tid] = ((s_red[0][tid] + s_red[1][tid]) + s_red[2][tid]) + s_red[3][tid];
}

/* sums[k] = the slots' k-th partials, added in a fixed order: workgroup k of 3 (one wave), lane l takes slots l, l + 64, .. */
__global__ void __launch_bounds__(64)
k_demons_finish(const double *__restrict__ partials, uint32_t nslots, double *__restrict__ sums)
{
    const uint32_t lane = threadIdx.x, k = blockIdx.x;
    double v = 0.0;
    for (uint32_t s = lane; s < nslots; s += 64u) v += partials[(size_t)s * S3D_DEM_NSUM + k];
    v = s3d_wave_sum_f64(v);
    if (lane == 0) sums[k] = v;
}

extern "C" size_t s3d_k_demons_step_scratch_bytes(int rnx, int rny, int rnz)
{
    if (rnx < 1 || rny < 1 || rnz < 1) return 0;
    return (size_t)s3d_dem_grid((size_t)rny * rnz, (size_t)rnx) * S3D_DEM_NSUM * sizeof(double);
}

extern "C" int s3d_k_demons_step(const float *d_src, int snx, int sny, int snz, const float *d_ref, int rnx, int rny, int rnz,
                                 const double A[12], const float *d_u, float *d_v, double sa, double ma, double sb, double mb,
                                 double kstep, double *d_sums, void *d_scratch, s3d_stream stream)
{
    if (snx < 1 || sny < 1 || snz < 1 || rnx < 1 || rny < 1 || rnz < 1) S3D_FAIL("bad dimensions");
    if (snx < 2 || sny < 2 || snz < 2) S3D_FAIL("a source dimension below 2 has no intensity gradient");
    if (d_src == NULL || d_ref == NULL || d_u == NULL || d_v == NULL || d_sums == NULL || d_scratch == NULL) S3D_FAIL("missing buffer");
    if (A == NULL) S3D_FAIL("missing affine matrix");
    const size_t rows = (size_t)rny * rnz;
    if (rows > 0x7fffffffu) S3D_FAIL("volume too large for the demons grid");
    const unsigned grid = s3d_dem_grid(rows, (size_t)rnx);
    AffineD a;
    for (int i = 0; i < 12; i++) a.a[i] = A[i];
    const DemConst K = {sa, ma, sb, mb, kstep};
    double *part = (double *)d_scratch;
    hipLaunchKernelGGL(k_demons_step, dim3(grid), dim3(256), 0, (hipStream_t)stream, d_src, snx, sny, snz, d_ref, rnx, rny,
                       (uint32_t)rows, a, K, d_u, d_v, rows * (size_t)rnx, part);
    S3D_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_demons_finish, dim3(S3D_DEM_NSUM), dim3(64), 0, (hipStream_t)stream, part, (uint32_t)grid, d_sums);
    S3D_CHECK_LAUNCH();
    return S3D_OK;
}

/* k_inv_affine with the voxel's displacement added to its coordinates */
template <int INTERP>
__global__ void __launch_bounds__(256)
k_inv_field(const float *__restrict__ src, int snx, int sny, int snz, int nc, float *__restrict__ dst, int dnx, int dny, int dnz,
            AffineD A, const float *__restrict__ u)
{
    const int x = blockIdx.x * 256 + threadIdx.x;
    const int y = blockIdx.y, z = blockIdx.z;
    if (x >= dnx) return;
    const size_t nvox = (size_t)dnx * dny * dnz, i = ((size_t)z * dny + y) * dnx + x;
    double tx, ty, tz;
    s3d_affine_xyz(A, (double)x, (double)y, (double)z, tx, ty, tz);
    tx = tx + (double)u[i];
    ty = ty + (double)u[nvox + i];
    tz = tz + (double)u[2 * nvox + i];
    s3d_sample_store<INTERP>(src, snx, sny, snz, nc, dst + i * nc, tx, ty, tz);
}

extern "C" int s3d_k_inv_field(const float *d_src, int snx, int sny, int snz, int nc, float *d_dst, int dnx, int dny, int dnz,
                               const double A[12], const float *d_u, int interp, s3d_stream stream)
{
    if (snx < 1 || sny < 1 || snz < 1 || nc < 1 || dnx < 1 || dny < 1 || dnz < 1) S3D_FAIL("bad dimensions");
    if (dny > 65535 || dnz > 65535) S3D_FAIL("volume too large for the resampling grid");
    if (d_src == NULL || d_dst == NULL || d_u == NULL || A == NULL) S3D_FAIL("missing buffer");
    AffineD a;
    for (int i = 0; i < 12; i++) a.a[i] = A[i];
    const dim3 grid(s3d_div_up(dnx, 256), dny, dnz);
    if (interp == 0)
        hipLaunchKernelGGL((k_inv_field<0>), grid, dim3(256), 0, (hipStream_t)stream, d_src, snx, sny, snz, nc, d_dst, dnx, dny,
                           dnz, a, d_u);
    else if (interp == 1)
        hipLaunchKernelGGL((k_inv_field<1>), grid, dim3(256), 0, (hipStream_t)stream, d_src, snx, sny, snz, nc, d_dst, dnx, dny,
                           dnz, a, d_u);
    else
        S3D_FAIL("unrecognized interpolation type");
    S3D_CHECK_LAUNCH();
    return S3D_OK;
}

/* one thread per fine voxel, the three components in turn: the tri-linear sample of the coarse component at half the fine
 * coordinates (clamped to the last coarse sample, so every coordinate is inside), doubled */
__global__ void __launch_bounds__(256)
k_field_upsample2(const float *__restrict__ coarse, int cnx, int cny, int cnz, float *__restrict__ fine, int fnx, int fny, int fnz)
{
    const int x = blockIdx.x * 256 + threadIdx.x;
    const int y = blockIdx.y, z = blockIdx.z;
    if (x >= fnx) return;
    const size_t nc = (size_t)cnx * cny * cnz, nf = (size_t)fnx * fny * fnz, i = ((size_t)z * fny + y) * fnx + x;
    double tx = (double)x / 2.0, ty = (double)y / 2.0, tz = (double)z / 2.0;
    tx = tx < (double)(cnx - 1) ? tx : (double)(cnx - 1);
    ty = ty < (double)(cny - 1) ? ty : (double)(cny - 1);
    tz = tz < (double)(cnz - 1) ? tz : (double)(cnz - 1);
    for (int c = 0; c < 3; c++) {
        float b;
        s3d_sample_store<0>(coarse + c * nc, cnx, cny, cnz, 1, &b, tx, ty, tz);
        fine[c * nf + i] = (float)(2.0 * (double)b);
    }
}

extern "C" int s3d_k_field_upsample2(const float *d_coarse, int cnx, int cny, int cnz, float *d_fine, int fnx, int fny, int fnz,
                                     s3d_stream stream)
{
    if (cnx < 1 || cny < 1 || cnz < 1 || fnx < 1 || fny < 1 || fnz < 1) S3D_FAIL("bad dimensions");
    if (cnx != fnx / 2 || cny != fny / 2 || cnz != fnz / 2) S3D_FAIL("the coarse dimensions must be half the fine ones (integer division)");
    if (fny > 65535 || fnz > 65535) S3D_FAIL("volume too large for the resampling grid");
    if (d_coarse == NULL || d_fine == NULL) S3D_FAIL("missing buffer");
    hipLaunchKernelGGL(k_field_upsample2, dim3(s3d_div_up(fnx, 256), fny, fnz), dim3(256), 0, (hipStream_t)stream, d_coarse, cnx,
                       cny, cnz, d_fine, fnx, fny, fnz);
    S3D_CHECK_LAUNCH();
    return S3D_OK;
}

/* The length of every entry of a planar field in f64, m = sqrt((x * x + y * y) + z * z); entries whose m is not finite are left
 * out.  Workgroup g of the fixed grid walks the voxels g * 256 + t, + grid * 256, .. and leaves (sum m, the count, max m) in its
 * slot; the caller adds the S3D_FIELD_NORM_SLOTS slots (cleared by the call, so the unused ones hold zeros) in slot order.  Which
 * voxels a thread sees depends on nvox only, so the result repeats. */
__global__ void __launch_bounds__(256)
k_field_norm(const float *__restrict__ u, size_t nvox, double *__restrict__ partials)
{
    __shared__ double s_red[4][3];
    const uint32_t tid = threadIdx.x;
    double sum = 0.0, cnt = 0.0, big = 0.0;
    for (size_t i = (size_t)blockIdx.x * 256 + tid; i < nvox; i += (size_t)gridDim.x * 256) {
        const double x = u[i], y = u[nvox + i], z = u[2 * nvox + i];
        const double m = sqrt((x * x + y * y) + z * z);
        if (!s3d_finite_d(m)) continue;
        sum += m;
        cnt += 1.0;
        big = m > big ? m : big;
    }
    sum = s3d_wave_sum_f64(sum);
    cnt = s3d_wave_sum_f64(cnt);
    for (int d = 32; d >= 1; d >>= 1) {
        const double o = __shfl_down(big, d);
        big = o > big ? o : big;
    }
    const uint32_t lane = tid & 63u, wave = tid >> 6;
    if (lane == 0) {
        s_red[wave][0] = sum;
        s_red[wave][1] = cnt;
        s_red[wave][2] = big;
    }
    __syncthreads();
    if (tid == 0) {
        double *out = partials + (size_t)blockIdx.x * 3;
        out[0] = ((s_red[0][0] + s_red[1][0]) + s_red[2][0]) + s_red[3][0];
        out[1] = ((s_red[0][1] + s_red[1][1]) + s_red[2][1]) + s_red[3][1];
        double b = s_red[0][2];
        for (int w = 1; w < 4; w++) b = s_red[w][2] > b ? s_red[w][2] : b;
        out[2] = b;
    }
}

extern "C" int s3d_k_field_norm_slots(void) { return S3D_FIELD_NORM_SLOTS; }

extern "C" int s3d_k_field_norm(const float *d_u, size_t nvox, double *d_partials, s3d_stream stream)
{
    if (nvox < 1) S3D_FAIL("bad dimensions");
    if (d_u == NULL || d_partials == NULL) S3D_FAIL("missing buffer");
    const size_t blocks = (nvox + 255) / 256;
    const unsigned grid = (unsigned)(blocks < S3D_FIELD_NORM_SLOTS ? blocks : S3D_FIELD_NORM_SLOTS);
    S3D_HIP(hipMemsetAsync(d_partials, 0, (size_t)S3D_FIELD_NORM_SLOTS * 3 * sizeof(double), (hipStream_t)stream));
    hipLaunchKernelGGL(k_field_norm, dim3(grid), dim3(256), 0, (hipStream_t)stream, d_u, nvox, d_partials);
    S3D_CHECK_LAUNCH();
    return S3D_OK;
}

/* ---- the inverse of a displacement field and the Jacobian determinant of its map (include/s3d_device.h has the definitions) ---
 * Both walk a volume the way k_demons_step does: workgroup g of a grid that depends on the dimensions only takes the rows g,
 * g + G, .., 256 x-consecutive voxels at a time, keeps its statistics in registers, reduces them by shuffles and through LDS in
 * wave order and leaves them in its own slot of d_partials, which the call has cleared; the caller adds the slots in order.
 *
 * k_field_invert: per source voxel the fixed-point iteration w <- -B s(B y + w), s the tri-linear sample of the field continued
 * constantly past its faces.  The field is only read, so a voxel's iteration depends on no other voxel's and one launch runs all
 * of them to their end; a wave stays in the loop until its slowest lane is done.  Per update: 24 gathers (eight corners of three
 * components, of which a smooth field leaves most in the same cache lines as the neighbouring lanes') and some 130 f64
 * operations, none of them a division. */
struct InvStat { double n[4], k, sum, big; };

__device__ __forceinline__ double s3d_wave_max_f64(double v)
{
    for (int d = 32; d >= 1; d >>= 1) {
        const double o = __shfl_down(v, d);
        v = o > v ? o : v;
    }
    return v;
}

__device__ __forceinline__ double s3d_wave_min_f64(double v)
{
    for (int d = 32; d >= 1; d >>= 1) {
        const double o = __shfl_down(v, d);
        v = o < v ? o : v;
    }
    return v;
}

__device__ __forceinline__ double s3d_clamp_d(double v, double hi) { return v < 0.0 ? 0.0 : v > hi ? hi : v; }

__global__ void __launch_bounds__(256)
k_field_invert(const float *__restrict__ u, int rnx, int rny, int rnz, AffineD A, AffineD B, float *__restrict__ w_out, int snx,
               int sny, uint32_t rows, int max_iter, double tol2, unsigned char *__restrict__ status, double *__restrict__ partials)
{
    __shared__ double s_red[4][S3D_FIELD_INV_STATS];
    const uint32_t tid = threadIdx.x;
    const size_t rn = (size_t)rnx * rny * rnz, sn = (size_t)rows * snx;
    const size_t sys = (size_t)rnx, szs = (size_t)rnx * rny;
    const double hx = (double)(rnx - 1), hy = (double)(rny - 1), hz = (double)(rnz - 1);
    double n0 = 0.0, n1 = 0.0, n2 = 0.0, n3 = 0.0, sum_k = 0.0, sum_res = 0.0, max_res = 0.0;
    for (uint32_t row = blockIdx.x; row < rows; row += gridDim.x) {
        const uint32_t z = row / (uint32_t)sny, y = row - z * (uint32_t)sny;
        for (int x0 = 0; x0 < snx; x0 += 256) {
            const int x = x0 + (int)tid;
            if (x >= snx) continue;
            double p0x, p0y, p0z;
            s3d_affine_xyz(B, (double)x, (double)y, (double)z, p0x, p0y, p0z);
            double wx = 0.0, wy = 0.0, wz = 0.0, e2 = 0.0;
            int k = 0, st;
            for (;;) {
                const double px = p0x + wx, py = p0y + wy, pz = p0z + wz;
                if (!(s3d_finite_d(px) && s3d_finite_d(py) && s3d_finite_d(pz))) { st = 3; break; }
                const double qx = s3d_clamp_d(px, hx), qy = s3d_clamp_d(py, hy), qz = s3d_clamp_d(pz, hz);
                const double s0 = s3d_trilinear_f64(u, 1, sys, szs, qx, qy, qz);
                const double s1 = s3d_trilinear_f64(u + rn, 1, sys, szs, qx, qy, qz);
                const double s2 = s3d_trilinear_f64(u + 2 * rn, 1, sys, szs, qx, qy, qz);
                if (!(s3d_finite_d(s0) && s3d_finite_d(s1) && s3d_finite_d(s2))) { st = 3; break; }
                const double rx = ((A.a[0] * wx + A.a[1] * wy) + A.a[2] * wz) + s0;
                const double ry = ((A.a[4] * wx + A.a[5] * wy) + A.a[6] * wz) + s1;
                const double rz = ((A.a[8] * wx + A.a[9] * wy) + A.a[10] * wz) + s2;
                e2 = (rx * rx + ry * ry) + rz * rz;
                if (e2 <= tol2) { st = (qx == px && qy == py && qz == pz) ? 0 : 1; break; }
                if (k == max_iter) { st = 2; break; }
                wx = -((B.a[0] * s0 + B.a[1] * s1) + B.a[2] * s2);
                wy = -((B.a[4] * s0 + B.a[5] * s1) + B.a[6] * s2);
                wz = -((B.a[8] * s0 + B.a[9] * s1) + B.a[10] * s2);
                k++;
            }
            const size_t i = (size_t)row * snx + x;
            if (st == 3) {
                s3d_u32a *wb = (s3d_u32a *)w_out;
                wb[i] = 0x7FC00000u;
                wb[sn + i] = 0x7FC00000u;
                wb[2 * sn + i] = 0x7FC00000u;
                n3 += 1.0;
            } else {
                w_out[i] = (float)wx;
                w_out[sn + i] = (float)wy;
                w_out[2 * sn + i] = (float)wz;
                const double res = sqrt(e2);
                sum_res += res;
                max_res = res > max_res ? res : max_res;
                if (st == 0) n0 += 1.0;
                else if (st == 1) n1 += 1.0;
                else n2 += 1.0;
            }
            sum_k += (double)k;
            if (status != NULL) status[i] = (unsigned char)st;
        }
    }
    const uint32_t lane = tid & 63u, wave = tid >> 6;
    const double r0 = s3d_wave_sum_f64(n0), r1 = s3d_wave_sum_f64(n1), r2 = s3d_wave_sum_f64(n2), r3 = s3d_wave_sum_f64(n3);
    const double r4 = s3d_wave_sum_f64(sum_k), r5 = s3d_wave_sum_f64(sum_res), r6 = s3d_wave_max_f64(max_res);
    if (lane == 0) {
        s_red[wave][0] = r0; s_red[wave][1] = r1; s_red[wave][2] = r2; s_red[wave][3] = r3;
        s_red[wave][4] = r4; s_red[wave][5] = r5; s_red[wave][6] = r6;
    }
    __syncthreads();
    if (tid < S3D_FIELD_INV_STATS) {
        double v;
        if (tid == 6) {
            v = s_red[0][6];
            for (int w = 1; w < 4; w++) v = s_red[w][6] > v ? s_red[w][6] : v;
        } else {
            v = ((s_red[0][tid] + s_red[1][tid]) + s_red[2][tid]) + s_red[3][tid];
        }
        partials[(size_t)blockIdx.x * S3D_FIELD_INV_STATS + tid] = v;
    }
}

extern "C" int s3d_k_field_invert_slots(void) { return S3D_FIELD_INV_SLOTS; }
extern "C" int s3d_k_field_invert_stats(void) { return S3D_FIELD_INV_STATS; }

extern "C" int s3d_k_field_invert(const float *d_u, int rnx, int rny, int rnz, const double A[12], const double B[12], float *d_w,
                                  int snx, int sny, int snz, int max_iter, double tol, unsigned char *d_status, double *d_partials,
                                  s3d_stream stream)
{
    if (rnx < 1 || rny < 1 || rnz < 1 || snx < 1 || sny < 1 || snz < 1) S3D_FAIL("bad dimensions");
    if (d_u == NULL || d_w == NULL || A == NULL || B == NULL || d_partials == NULL) S3D_FAIL("missing buffer");
    if (max_iter < 0) S3D_FAIL("max_iter must not be negative");
    if (!(tol >= 0.0)) S3D_FAIL("tol must be a number >= 0");
    if (sny > 65535 || snz > 65535) S3D_FAIL("volume too large for the resampling grid");
    const size_t rows = (size_t)sny * snz;
    const unsigned grid = (unsigned)(rows < S3D_FIELD_INV_SLOTS ? rows : S3D_FIELD_INV_SLOTS);
    AffineD a, b;
    for (int i = 0; i < 12; i++) { a.a[i] = A[i]; b.a[i] = B[i]; }
    S3D_HIP(hipMemsetAsync(d_partials, 0, (size_t)S3D_FIELD_INV_SLOTS * S3D_FIELD_INV_STATS * sizeof(double), (hipStream_t)stream));
    hipLaunchKernelGGL(k_field_invert, dim3(grid), dim3(256), 0, (hipStream_t)stream, d_u, rnx, rny, rnz, a, b, d_w, snx, sny,
                       (uint32_t)rows, max_iter, tol * tol, d_status, d_partials);
    S3D_CHECK_LAUNCH();
    return S3D_OK;
}

/* the derivative of a component along one axis at index i of n >= 2 (p: the voxel's entry, stride in floats): central inside,
 * one-sided on the two faces */
__device__ __forceinline__ double s3d_field_diff(const float *__restrict__ p, ptrdiff_t stride, int i, int n)
{
    if (i == 0) return (double)p[stride] - (double)p[0];
    if (i == n - 1) return (double)p[0] - (double)p[-stride];
    return ((double)p[stride] - (double)p[-stride]) * 0.5;
}

/* k_field_jacobian: 18 loads per voxel (the x neighbours are the neighbouring lanes' own entries, the y and z neighbours full
 * rows read as such), nine differences and the 3 x 3 determinant of A + grad u. */
__global__ void __launch_bounds__(256)
k_field_jacobian(const float *__restrict__ u, int rnx, int rny, int rnz, uint32_t rows, AffineD A, float *__restrict__ det_out,
                 double *__restrict__ partials)
{
    __shared__ double s_red[4][S3D_FIELD_JAC_STATS];
    const uint32_t tid = threadIdx.x;
    const size_t rn = (size_t)rows * rnx;
    const ptrdiff_t sys = (ptrdiff_t)rnx, szs = (ptrdiff_t)rnx * rny;
    double sum = 0.0, cnt = 0.0, fold = 0.0, lo = __builtin_huge_val(), hi = -__builtin_huge_val();
    for (uint32_t row = blockIdx.x; row < rows; row += gridDim.x) {
        const int z = (int)(row / (uint32_t)rny), y = (int)(row - (uint32_t)z * (uint32_t)rny);
        for (int x0 = 0; x0 < rnx; x0 += 256) {
            const int x = x0 + (int)tid;
            if (x >= rnx) continue;
            const size_t i = (size_t)row * rnx + x;
            double J[9];
#pragma unroll
            for (int c = 0; c < 3; c++) {
                const float *p = u + c * rn + i;
                J[3 * c + 0] = A.a[4 * c + 0] + s3d_field_diff(p, 1, x, rnx);
                J[3 * c + 1] = A.a[4 * c + 1] + s3d_field_diff(p, sys, y, rny);
                J[3 * c + 2] = A.a[4 * c + 2] + s3d_field_diff(p, szs, z, rnz);
            }
            const double det = (J[0] * (J[4] * J[8] - J[5] * J[7]) - J[1] * (J[3] * J[8] - J[5] * J[6])) +
                               J[2] * (J[3] * J[7] - J[4] * J[6]);
            if (det_out != NULL) det_out[i] = (float)det;
            if (!s3d_finite_d(det)) continue;
            sum += det;
            cnt += 1.0;
            if (det <= 0.0) fold += 1.0;
            lo = det < lo ? det : lo;
            hi = det > hi ? det : hi;
        }
    }
    const uint32_t lane = tid & 63u, wave = tid >> 6;
    const double r0 = s3d_wave_sum_f64(sum), r1 = s3d_wave_sum_f64(cnt), r2 = s3d_wave_sum_f64(fold);
    const double r3 = s3d_wave_min_f64(lo), r4 = s3d_wave_max_f64(hi);
    if (lane == 0) {
        s_red[wave][0] = r0; s_red[wave][1] = r1; s_red[wave][2] = r2; s_red[wave][3] = r3; s_red[wave][4] = r4;
    }
    __syncthreads();
    if (tid == 0) {
        double *out = partials + (size_t)blockIdx.x * S3D_FIELD_JAC_STATS;
        for (int k = 0; k < 3; k++) out[k] = ((s_red[0][k] + s_red[1][k]) + s_red[2][k]) + s_red[3][k];
        double a = s_red[0][3], b = s_red[0][4];
        for (int w = 1; w < 4; w++) {
            a = s_red[w][3] < a ? s_red[w][3] : a;
            b = s_red[w][4] > b ? s_red[w][4] : b;
        }
        out[3] = a;
        out[4] = b;
    }
}

extern "C" int s3d_k_field_jacobian_slots(void) { return S3D_FIELD_JAC_SLOTS; }
extern "C" int s3d_k_field_jacobian_stats(void) { return S3D_FIELD_JAC_STATS; }

extern "C" int s3d_k_field_jacobian(const float *d_u, int rnx, int rny, int rnz, const double A[12], float *d_det,
                                    double *d_partials, s3d_stream stream)
{
    if (rnx < 2 || rny < 2 || rnz < 2) S3D_FAIL("every dimension must be at least 2 (a derivative needs two samples)");
    if (d_u == NULL || A == NULL || d_partials == NULL) S3D_FAIL("missing buffer");
    if (rny > 65535 || rnz > 65535) S3D_FAIL("volume too large for the resampling grid");
    const size_t rows = (size_t)rny * rnz;
    const unsigned grid = (unsigned)(rows < S3D_FIELD_JAC_SLOTS ? rows : S3D_FIELD_JAC_SLOTS);
    AffineD a;
    for (int i = 0; i < 12; i++) a.a[i] = A[i];
    S3D_HIP(hipMemsetAsync(d_partials, 0, (size_t)S3D_FIELD_JAC_SLOTS * S3D_FIELD_JAC_STATS * sizeof(double), (hipStream_t)stream));
    hipLaunchKernelGGL(k_field_jacobian, dim3(grid), dim3(256), 0, (hipStream_t)stream, d_u, rnx, rny, rnz, (uint32_t)rows, a,
                       d_det, d_partials);
    S3D_CHECK_LAUNCH();
    return S3D_OK;
}
