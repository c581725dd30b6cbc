/* s3d_resample.hip -- the device unit of the registration tail: the inverse affine warp of a
 * volume, the inverse thin-plate-spline warp and, at the end of the file, the consensus counts of find_tform_ransac's
 * hypotheses.
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

/* The sample of src at (tx, ty, tz), every channel, to out[0 .. nc): the reference's resample_linear / resample_lanczos2.
 * Shared by the affine and the spline warp. */
template <int INTERP>
__device__ __forceinline__ void s3d_sample_store(const float *__restrict__ src, int snx, int sny, int snz, int nc,
                                                 float *__restrict__ out, double tx, double ty, double tz)
{
    const bool outside = tx < 0 || tx > snx - 1 || ty < 0 || ty > sny - 1 || tz < 0 || tz > snz - 1;
    const size_t sxs = (size_t)nc, sys = (size_t)nc * snx, szs = (size_t)nc * snx * sny;
    if (outside || !(tx == tx) || !(ty == ty) || !(tz == tz)) {
        /* NaN coordinates fail every comparison in the reference and would index out of range there */
        for (int c = 0; c < nc; c++) out[c] = 0.0f;
        return;
    }
    if (INTERP == 0) {
        const int fx = (int)floor(tx), fy = (int)floor(ty), fz = (int)floor(tz);
        const int cx = (int)ceil(tx), cy = (int)ceil(ty), cz = (int)ceil(tz);
        const double dx = tx - fx, dy = ty - fy, dz = tz - fz;
        for (int c = 0; c < nc; c++) {
            const float *p = src + c;
            const double c0 = p[fx * sxs + fy * sys + fz * szs], c1 = p[fx * sxs + cy * sys + fz * szs];
            const double c2 = p[cx * sxs + fy * sys + fz * szs], c3 = p[cx * sxs + cy * sys + fz * szs];
            const double c4 = p[fx * sxs + fy * sys + cz * szs], c5 = p[fx * sxs + cy * sys + cz * szs];
            const double c6 = p[cx * sxs + fy * sys + cz * szs], c7 = p[cx * sxs + cy * sys + cz * szs];
            const double v = c0 * (1.0 - dx) * (1.0 - dy) * (1.0 - dz) + c1 * (1.0 - dx) * dy * (1.0 - dz) +
                             c2 * dx * (1.0 - dy) * (1.0 - dz) + c3 * dx * dy * (1.0 - dz) +
                             c4 * (1.0 - dx) * (1.0 - dy) * dz + c5 * (1.0 - dx) * dy * dz +
                             c6 * dx * (1.0 - dy) * dz + c7 * dx * dy * dz;
            out[c] = (float)v;
        }
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

template <int INTERP>
__global__ void __launch_bounds__(256)
k_inv_affine(const float *__restrict__ src, int snx, int sny, int snz, int nc, float *__restrict__ dst, int dnx, int dny,
             int dnz, AffineD A)
{
    const int x = blockIdx.x * 256 + threadIdx.x;
    const int y = blockIdx.y, z = blockIdx.z;
    if (x >= dnx) return;
    const double xd = (double)x, yd = (double)y, zd = (double)z;
    const double tx = A.a[0] * xd + A.a[1] * yd + A.a[2] * zd + A.a[3];
    const double ty = A.a[4] * xd + A.a[5] * yd + A.a[6] * zd + A.a[7];
    const double tz = A.a[8] * xd + A.a[9] * yd + A.a[10] * zd + A.a[11];
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
template <int INTERP>
__global__ void __launch_bounds__(256)
k_inv_tps(const float *__restrict__ src, int snx, int sny, int snz, int nc, float *__restrict__ dst, int dnx, int dny, int dnz,
          const double *__restrict__ ctrl, const double *__restrict__ params, uint32_t n_ctrl)
{
    __shared__ double s_pt[S3D_TPS_TILE * 6];               /* per point: x y z w_x w_y w_z */
    const int x = blockIdx.x * 256 + threadIdx.x;
    const int y = blockIdx.y, z = blockIdx.z;
    const double xd = (double)x, yd = (double)y, zd = (double)z;
    const size_t row = (size_t)n_ctrl + 4;                  /* row length of params */
    double tx = 0.0, ty = 0.0, tz = 0.0;
    for (uint32_t n0 = 0; n0 < n_ctrl; n0 += S3D_TPS_TILE) {
        const uint32_t nt = n_ctrl - n0 < (uint32_t)S3D_TPS_TILE ? n_ctrl - n0 : (uint32_t)S3D_TPS_TILE;
        if (n0) __syncthreads();                            /* the previous tile has been read by every lane */
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
    if (x >= dnx) return;
    const double *ax = params + n_ctrl, *ay = ax + row, *az = ay + row;
    tx += ax[0]; tx += ax[1] * xd; tx += ax[2] * yd; tx += ax[3] * zd;
    ty += ay[0]; ty += ay[1] * xd; ty += ay[2] * yd; ty += ay[3] * zd;
    tz += az[0]; tz += az[1] * xd; tz += az[2] * yd; tz += az[3] * zd;
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
