"""Kernels on either side of their 32-bit offset limits, against the oracle.

Every other parity test runs on levels of at most 2^30 voxels.  Many kernels address with 32-bit offsets or indices, each
kept in range by a host-side guard; the tests here run shapes just below and just above those guards and compare the
result with the plain-C restatement (oracle/) or a numpy restatement, bit for bit.

Patch tiling.  A large volume is exact zeros plus K identical copies of one patch: content with a zero border in x and y,
spanning the volume's whole z range.  The border is wider than the dependency cone of everything downstream, so every output
voxel of a copy equals the oracle's output on the patch alone, and the oracle never runs at full size:
  - sep_fir: output <- input within +-hw per axis; the border must also cover the edge rules of the patch-alone run (mirrored
    and blended samples of the first / last hw + 1 columns): 2 hw + 1 = 9 for the half-width-4 smoothing filter;
  - dense: smoothing (hw 4) + gradient (1) + the window blur (hw 9) = 14 from the content, plus the blur's own edge rule
    (hw + 1 = 10) -> 24; the zero voxels around content give zero outputs (the output is multiplied by the input voxel).
The copies sit where the pre-fix kernels' wrapped addresses land on different content: a wrapped 32-bit offset in a z pass
moves a column of the plane's tail back by 2^32 bytes, into the head of the same plane, so the copies go into the tail and
the head stays zero.  Device buffers are filled and read in row bands; no host array holds a whole volume.

Audit: every 32-bit offset or index held in a kernel, where it wraps, the host guard that keeps it out, and the test on each
side of the guard.  "Limit" is the first size that is refused or routed elsewhere.

| site | 32-bit quantity | wraps at | guard (limit) | tests |
|---|---|---|---|---|
| s3d_dense.hip k_dmarch z pass (POST) | loff = colid*16, colid < 3 nx ny | nx ny >= 89 478 486 | s3d_k_dense_bary_blur: 48 nx ny > 2^32-1 -> separate steps (was nx ny >= 0x7fffffff/3: the bug) | test_dense_plane_limit below / above |
| s3d_dense.hip k_dmarch epilogue | evox, pvox = nx ny | nx ny >= 2^32 | same guard (far tighter) | same |
| s3d_dense.hip k_dmarch y pass | loff over 3 nx columns | nx >= 89 478 486 | fast_mc_eligible: 12 nx <= 2^24 | below the limit only (nx <= 1.4 M) |
| s3d_gauss.hip k_gauss_zs (MAXOUT, raw smoothing) | loff = colid*16, colid < nx/4 ny | (nx/4) ny > 2^28 | s3d_k_sep_fir_max returns 1 and launch_fast refuses d_maxout when (nx/4) ny 16 >= 2^32-1 (was: no guard, the bug) | test_smooth_max_plane_limit below / above |
| s3d_gauss.hip k_gauss_zs (mode bit 7) | same | same | launch_fast: same condition -> k_gauss_z | mode bit 7 is an A/B knob: not tested |
| s3d_gauss.hip k_conv_x_dyadic_v4 | row, gid | nrows nedge >= 2^32 | launch_x_dyadic_v4: nrows nedge < 2^32-1 else generic pass | not reached by a test: the dyadic x pass serves pyramid levels, whose size the extrema guard bounds far below |
| s3d_gauss.hip k_conv_x_mc | q4 = nx nc / 4, q | nx nc >= 2^32 | fast_mc_eligible: nx nc <= 2^24 | dense tests (nx nc = 196 608) |
| s3d_extrema.hip k_extrema | idx, plane = nx ny | n >= 2^32 | s3d_k_extrema_slab: n >= 0xFFFFFF00 refused | test_extrema_index_limits: 3 * 2^30 voxels (above 2^31); the refusal is not run on a device (the host returns before any launch) |
| s3d_extrema.hip k_extrema_fused | idx, magic division of i * m in 64 bits | n >= 0x7FFFFF00 | extrema_fused_launch: returns 1 -> per-level k_extrema | test_extrema_index_limits: 0x7F000000 (taken), 2^31 (declined) |
| s3d_extrema.hip k_cb_emit | out index idx_base + 64 w + b | n >= 2^32 | the extrema guard | test_extrema_index_limits: indices >= 2^31 |
| s3d_keypoint.hip k_ck_emit, orient_one, describe | uint32 voxel index -> x, y, z; plane unsigned | n >= 2^32 | the extrema guard | test_extrema_index_limits (compacted indices >= 2^31); detect + describe end to end above 2^31 voxels is not tested yet |
| s3d_keypoint.hip orientation window table | e.off = dz * (int)plane + dy nx + dx (signed) | \\|off\\| >= 2^31 | none needed: a table is replayed only for a window inside the level (its box equals the table's), so \\|dz\\| <= (nz-1)/2, \\|dy\\| <= (ny-1)/2, \\|dx\\| <= (nx-1)/2 and \\|off\\| <= (nx ny nz - 1)/2 < 2^31 under the extrema guard | none: unreachable (the build of a never-replayed table may hold a wrapped value; it is not dereferenced) |
| s3d_dense.hip k_dense_rot_hist | vox = blockIdx.x, plane unsigned | n >= 2^31 | s3d_k_dense_rot_hist and the host: n >= 0x7FFFFFFF refused | not run at that size (dense_rotate of 2^31 voxels takes hours) |
"""
import ctypes as C
import os

import numpy as np
import pytest

from tests import parity
from tests.util import nbitdiff

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(os.environ.get("S3D_TEST_LARGE") == "0", reason="S3D_TEST_LARGE=0")]

GIB = 1 << 30
_vp = C.c_void_p
_f32p = C.POINTER(C.c_float)


def _dev(lib):
    dev = parity.dev_of(lib)
    L = dev.L
    L.s3d_k_sep_fir_max.argtypes = [_vp, _vp, _vp, C.c_int, C.c_int, C.c_int, _f32p, _f32p, C.c_int, _vp, _vp]
    L.s3d_k_sep_fir.argtypes = [_vp, _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, _f32p, _f32p, C.c_int, _vp]
    L.s3d_k_dense_bary_blur.argtypes = [_vp, _vp, _vp, C.c_int, C.c_int, C.c_int, _f32p, _f32p, _vp, _f32p, C.c_int,
                                        _vp, _vp]
    L.s3d_k_extrema.argtypes = [_vp] * 4 + [C.c_int] * 3 + [C.c_double, _vp, _vp, _vp]
    L.s3d_k_extrema_fused.argtypes = [_vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, _vp, _vp,
                                      _vp]
    L.s3d_k_compact_bits.argtypes = [_vp, C.c_size_t, _vp, _vp, C.c_uint32, C.c_uint32, _vp, _vp, _vp]
    return dev


_FREE0 = {}


def _need(dev, nbytes):
    free, _ = dev.mem_info()
    _FREE0.setdefault("v", free)
    if free < nbytes + 2 * GIB:
        pytest.skip(f"needs {nbytes / GIB:.0f} GiB of device memory, {free / GIB:.0f} GiB free")


class _Bufs:
    """device buffers freed together (also when an assertion fails)"""

    def __init__(self, dev):
        self.dev, self.ptrs = dev, []

    def alloc(self, nbytes):
        p = self.dev.malloc(nbytes)
        self.ptrs.append(p)
        return p

    def report(self, what):
        """device memory in use now against the module's start (the tests sample it at their peak)"""
        free, _ = self.dev.mem_info()
        print(f"\n{what}: {(_FREE0.get('v', free) - free) / GIB:.1f} GiB of device memory in use")

    def free(self):
        for p in self.ptrs:
            self.dev.free(p)
        self.ptrs = []


def _h2d(dev, d, off_bytes, a):
    a = np.ascontiguousarray(a)
    dev.check(dev.L.s3d_rt_h2d(_vp(d + off_bytes), _vp(a.ctypes.data), a.nbytes, None), "h2d")


def _d2h(dev, d, off_bytes, shape, dtype=np.float32):
    out = np.empty(shape, dtype)
    dev.check(dev.L.s3d_rt_d2h(_vp(out.ctypes.data), _vp(d + off_bytes), out.nbytes, None), "d2h")
    return out


def _put_copies(dev, d_vol, dims, patch, copies):
    """zeros (already there) plus `patch` [nz, py, px] at every (x0, y0) of `copies`, written band by band"""
    nx, ny, nz = dims
    py, px = patch.shape[1:]
    for y0 in sorted({y for _, y in copies}):
        band = np.zeros((nz, py, nx), np.float32)
        for x0, yc in copies:
            if yc == y0:
                band[:, :, x0:x0 + px] = patch
        for z in range(nz):
            _h2d(dev, d_vol, 4 * ((z * ny + y0) * nx), band[z])
    dev.sync()


def _check_bands(dev, d_out, dims, nc, want_patch, copies, extra_rows=()):
    """every voxel of the row bands that hold copies: the patch's expected output at the copies, +0.0 elsewhere; also the
    bands `extra_rows` (background only).  Returns the number of differing elements."""
    nx, ny, nz = dims
    py, px = want_patch.shape[1:3]
    tail = (nc,) if nc > 1 else ()
    bad = 0
    bands = sorted({y for _, y in copies}) + list(extra_rows)
    for y0 in bands:
        want = np.zeros((py, nx) + tail, np.float32)
        for z in range(nz):
            want[...] = 0.0
            for x0, yc in copies:
                if yc == y0:
                    want[:, x0:x0 + px] = want_patch[z]
            got = _d2h(dev, d_out, 4 * nc * ((z * ny + y0) * nx), (py, nx) + tail)
            bad += nbitdiff(got, want)
    dev.sync()
    return bad


def _patch(shape, border, seed):
    """content (smooth blobs, positive) with a zero border of `border` voxels in x and y"""
    nz, py, px = shape
    v = parity.dense_input((px, py, nz), seed)
    v[:, :border, :] = 0.0
    v[:, py - border:, :] = 0.0
    v[:, :, :border] = 0.0
    v[:, :, px - border:] = 0.0
    return v


# ---- T1: dense descriptors, fused z pass (k_dmarch) across its plane limit --------------------------------------------------
DENSE_NX, DENSE_NZ = 16384, 11                    # nz: the smallest the fused path takes with the window's half width 9
DENSE_LIMIT = (2**32 + 47) // 48                  # nx * ny from which loff = colid * 16 wraps: 89 478 486
DENSE_P, DENSE_B = 128, 32                        # patch side, zero border (cone 14 + the blur's edge rule 10, rounded up)


@pytest.mark.parametrize("ny, fused", [(5461, True), (5600, False)], ids=["below", "above"])
def test_dense_plane_limit(hip, oracle, ny, fused):
    """sift3d_amd_extract_dense_dev on 16384 x ny x 11: ny = 5461 is the last plane under the limit (the fused path),
    ny = 5600 puts 138 rows of every plane past it (the separate steps since the fix; before it, the fused z pass read those
    rows' columns from the plane's head).  Every voxel of the bands with copies -- head, middle, far end of the plane, every z
    plane -- against oracle.dense on the patch, bit for bit; background bands +0.0."""
    from sift3d_amd import abi
    assert (DENSE_NX * 5461 < DENSE_LIMIT) and (DENSE_NX * 5600 >= DENSE_LIMIT) and 48 * (DENSE_LIMIT - 1) < 2**32
    dev = _dev(hip)
    nx, nz = DENSE_NX, DENSE_NZ
    dims = (nx, ny, nz)
    n = nx * ny * nz
    _need(dev, 4 * n * (2 + 12 * 3))
    patch = _patch((nz, DENSE_P, DENSE_P), DENSE_B, seed=7)
    want = oracle.dense(patch)
    assert not np.any(want[:, :DENSE_B - 10].view(np.uint32)) and not np.any(want[:, :, :DENSE_B - 10].view(np.uint32))
    p0_row = DENSE_LIMIT // nx                    # the first row whose tail wraps (5461)
    if fused:
        copies = [(64, 64), (8192, 2688), (nx - DENSE_P - 64, ny - DENSE_P - 64), (nx - DENSE_P, 64)]
    else:                                         # the rows past the limit hold copies; the plane's head stays zero
        yt = p0_row + 2
        assert yt + DENSE_P <= ny
        copies = [(64, yt), (8192, yt), (nx - DENSE_P - 8, yt), (8192, 2688)]
    s = abi.SIFT3D()
    assert hip.sift.init_SIFT3D(C.byref(s)) == 0
    B = _Bufs(dev)
    try:
        d_in = B.alloc(4 * n)
        d_out = B.alloc(4 * 12 * n)
        dev.check(dev.L.s3d_rt_memset(_vp(d_in), 0, 4 * n, None), "memset")
        _put_copies(dev, d_in, dims, patch, copies)
        # the eligibility decision itself: 0 = fused launch, 1 = declined (nothing launched)
        taps = np.ascontiguousarray(oracle.gauss_taps(1.6 * 7.0710678118654755 / 4.0), np.float32)
        assert taps.size == 19
        one = np.ones(3, np.float32)
        mesh = np.ascontiguousarray(dev.mesh_table())
        d_mesh = B.alloc(mesh.nbytes)
        _h2d(dev, d_mesh, 0, mesh)
        d_tmp = B.alloc(4 * 12 * n)
        rc = dev.L.s3d_k_dense_bary_blur(_vp(d_in), _vp(d_out), _vp(d_tmp), nx, ny, nz,
                                         one.ctypes.data_as(_f32p), one.ctypes.data_as(_f32p), _vp(d_mesh),
                                         taps.ctypes.data_as(_f32p), taps.size, _vp(d_in), None)
        dev.sync()
        B.ptrs.remove(d_tmp)
        dev.free(d_tmp)
        ou = (C.c_double * 3)(1.0, 1.0, 1.0)
        assert hip.sift.sift3d_amd_extract_dense_dev(C.byref(s), _vp(d_in), nx, ny, nz, 1.0, 1.0, 1.0, ou, _vp(d_out)) == 0
        dev.sync()
        B.report(f"dense {nx}x{ny}x{nz}")
        bad = _check_bands(dev, d_out, dims, 12, want, copies, extra_rows=[ny // 3, 1000 if fused else 0])
        assert bad == 0, f"dense {nx}x{ny}x{nz}: {bad} elements differ from the oracle's patch output"
        assert rc == (0 if fused else 1), f"s3d_k_dense_bary_blur returned {rc} for nx*ny = {nx * ny}"
    finally:
        hip.sift.cleanup_SIFT3D(C.byref(s))
        B.free()


# ---- T2: raw-image smoothing with the maximum kept (k_gauss_zs) at 4 GiB planes ----------------------------------------------
SMOOTH_NX, SMOOTH_NZ = 32768, 6
SMOOTH_P, SMOOTH_B = 96, 16                       # patch side, zero border (>= 2 hw + 1 = 9)


@pytest.mark.parametrize("ny, fused", [(32764, True), (32928, False)], ids=["below", "above"])
def test_smooth_max_plane_limit(hip, oracle, ny, fused):
    """s3d_k_sep_fir_max (and s3d_k_sep_fir) with the half-width-4 filter of smooth_scale_raw on 32768 x ny x 6:
    (nx/4) ny 16 just under 2^32 (the maximum-keeping z pass) and 160 rows past it (since the fix: returns 1, the caller
    runs s3d_k_sep_fir + s3d_k_absmax; before it, the z pass read and wrote those rows through wrapped offsets).  Copies
    against oracle.sep_fir on the patch, bit for bit; the maximum against the patch's."""
    dev = _dev(hip)
    L = dev.L
    nx, nz = SMOOTH_NX, SMOOTH_NZ
    dims = (nx, ny, nz)
    n = nx * ny * nz
    _need(dev, 3 * 4 * n)
    taps = np.ascontiguousarray(oracle.gauss_taps(oracle.incremental_sigma(1.15, 1.6)), np.float32)
    assert taps.size == 9
    patch = _patch((nz, SMOOTH_P, SMOOTH_P), SMOOTH_B, seed=3)
    want = oracle.sep_fir(patch, taps)
    want_max = np.abs(want).max()
    p0_row = 2**30 // nx                          # plane offsets of the rows from here on are >= 2^32 bytes
    if fused:
        copies = [(64, 64), (16384, 16384), (nx - SMOOTH_P - 64, ny - SMOOTH_P - 64)]
    else:
        yt = p0_row + 16
        assert yt + SMOOTH_P <= ny
        copies = [(64, yt), (16384, yt), (nx - SMOOTH_P - 8, yt), (16384, 16384)]
    uf = np.ones(3, np.float32)
    B = _Bufs(dev)
    try:
        d_src, d_dst, d_tmp = B.alloc(4 * n), B.alloc(4 * n), B.alloc(4 * n)
        d_max = B.alloc(16)
        dev.check(L.s3d_rt_memset(_vp(d_src), 0, 4 * n, None), "memset")
        _put_copies(dev, d_src, dims, patch, copies)
        rc = L.s3d_k_sep_fir_max(_vp(d_src), _vp(d_dst), _vp(d_tmp), nx, ny, nz, uf.ctypes.data_as(_f32p),
                                 taps.ctypes.data_as(_f32p), taps.size, _vp(d_max), None)
        assert rc in (0, 1)
        if rc == 1:                               # what smooth_scale_raw_dev does then
            assert L.s3d_k_sep_fir(_vp(d_src), _vp(d_dst), _vp(d_tmp), nx, ny, nz, 1, uf.ctypes.data_as(_f32p),
                                   taps.ctypes.data_as(_f32p), taps.size, None) == 0
            assert L.s3d_k_absmax(_vp(d_dst), n, _vp(d_max), None) == 0
        dev.sync()
        B.report(f"smoothing {nx}x{ny}x{nz}")
        got_max = _d2h(dev, d_max, 0, (1,))
        bad = _check_bands(dev, d_dst, dims, 1, want, copies, extra_rows=[ny // 3])
        assert bad == 0, f"s3d_k_sep_fir_max {nx}x{ny}x{nz} (rc {rc}): {bad} elements differ from the oracle's patch output"
        assert nbitdiff(got_max, np.float32([want_max])) == 0, (got_max, want_max)
        # the plain filter at the same size (the fall-back itself)
        dev.check(L.s3d_rt_memset(_vp(d_dst), 0, 4 * n, None), "memset")
        assert L.s3d_k_sep_fir(_vp(d_src), _vp(d_dst), _vp(d_tmp), nx, ny, nz, 1, uf.ctypes.data_as(_f32p),
                               taps.ctypes.data_as(_f32p), taps.size, None) == 0
        dev.sync()
        bad = _check_bands(dev, d_dst, dims, 1, want, copies)
        assert bad == 0, f"s3d_k_sep_fir {nx}x{ny}x{nz}: {bad} elements differ"
        assert rc == (0 if fused else 1), f"s3d_k_sep_fir_max returned {rc} for (nx/4)*ny = {nx // 4 * ny}"
    finally:
        B.free()


# ---- T3: extrema bitmaps and candidate indices on both sides of 2^31 ------------------------------------------------------------
EXT_NX = EXT_NY = 4096
EXT_PERIOD = 5                                    # distinct random planes; a level repeats them along z
PEAK = 0.1


def _levels_host(nlev, seed):
    rng = np.random.default_rng(seed)
    base = rng.standard_normal((EXT_PERIOD, EXT_NY, EXT_NX), dtype=np.float32)
    return [np.ascontiguousarray(base * np.float32(1.0 - 0.13 * k) +
                                 rng.standard_normal(base.shape, dtype=np.float32) * np.float32(0.05 * (k + 1)))
            for k in range(nlev)]


def _fill_periodic(dev, d, slab, nz):
    """level[z] = slab[z % P] for z < nz: P planes uploaded, then doubled device to device"""
    plane = EXT_NX * EXT_NY
    _h2d(dev, d, 0, slab)
    have = EXT_PERIOD
    while have < nz:
        m = min(have, nz - have)
        dev.check(dev.L.s3d_rt_d2d(_vp(d + 4 * plane * have), _vp(d), 4 * plane * m, None), "d2d")
        have += m
    dev.sync()


def _want_bits(lv, nz, zs, dogmax):
    """the bitmap words of planes zs (consecutive) of the level made of lv[0..3] (periodic), numpy float32 restatement of
    k_extrema / detect_extrema: strict tests against the 6 face neighbours and the two scale neighbours, |v| > thr"""
    P = EXT_PERIOD
    thr = np.float32(PEAK * float(dogmax))
    out = []
    for z in zs:
        g = lambda k, dz: lv[k][(z + dz) % P]                                       # noqa: E731
        c1, c2 = g(1, 0), g(2, 0)
        v = c1 - c2
        pred = np.zeros((EXT_NY, EXT_NX), bool)
        if 1 <= z <= nz - 2:
            pv = g(0, 0) - c1
            nv = c2 - g(3, 0)
            zm = g(1, -1) - g(2, -1)
            zp = g(1, 1) - g(2, 1)
            s = (slice(1, EXT_NY - 1), slice(1, EXT_NX - 1))
            vc = v[s]
            xm, xp = v[1:-1, :-2], v[1:-1, 2:]
            ym, yp = v[:-2, 1:-1], v[2:, 1:-1]
            nb = [pv[s], xp, xm, yp, ym, zm[s], zp[s], nv[s]]
            is_max = np.logical_and.reduce([vc > b for b in nb])
            is_min = np.logical_and.reduce([vc < b for b in nb])
            pred[s] = ((vc > thr) | (vc < -thr)) & (is_max | is_min)
        out.append(np.packbits(pred.reshape(-1), bitorder="little").view(np.uint64))
    return np.concatenate(out)


def test_extrema_index_limits(hip):
    """s3d_k_extrema_fused on 4096^2 x 127 (0x7F000000 voxels: takes the level) and 4096^2 x 128 (2^31: returns 1 and
    launches nothing); s3d_k_extrema on 4096^2 x 192 (3 * 2^30).  Dense random levels (nearly every voxel tested): the
    bitmap words of planes at the start, the middle and, for the per-level kernel, above voxel index 2^31 against a numpy
    float32 restatement; s3d_k_compact_bits gives the same ascending indices at and above 2^31."""
    dev = _dev(hip)
    L = dev.L
    plane = EXT_NX * EXT_NY
    nz_big = 192
    n_big = plane * nz_big
    assert n_big == 3 * 2**30 and n_big < 0xFFFFFF00
    _need(dev, 4 * plane * (4 * nz_big + 2 * 127) + n_big // 2 + 8 * (n_big // 3))
    lv = _levels_host(6, seed=13)
    dogmax = [np.abs(lv[k + 1] - lv[k + 2]).max() for k in range(3)]                # the periodic level's own maxima
    B = _Bufs(dev)
    try:
        d_lv = [B.alloc(4 * plane * (nz_big if k < 4 else 127)) for k in range(6)]
        d_max = B.alloc(16)
        _h2d(dev, d_max, 0, np.float32(dogmax))
        # -- fused kernel: 127 planes (taken), 128 planes (declined) --
        nz = 127
        n = plane * nz
        assert n < 0x7FFFFF00 <= plane * 128
        for k in range(6):
            _fill_periodic(dev, d_lv[k], lv[k], nz)
        nw = (n + 63) // 64
        d_bits = [B.alloc(8 * nw) for _ in range(3)]
        P6 = (C.c_void_p * 6)(*d_lv)
        B3 = (C.c_void_p * 3)(*d_bits)
        assert L.s3d_k_extrema_fused(P6, 3, EXT_NX, EXT_NY, 128, 0, 128, PEAK, _vp(d_max), B3, None) == 1
        assert L.s3d_k_extrema_fused(P6, 3, EXT_NX, EXT_NY, nz, 0, nz, PEAK, _vp(d_max), B3, None) == 0
        dev.sync()
        wpp = plane // 64                                                            # bitmap words per plane
        total = 0
        for k in range(3):
            lk = lv[k:k + 4]
            for zs in ([0, 1, 2], [63, 64], [nz - 2, nz - 1]):
                got = _d2h(dev, d_bits[k], 8 * wpp * zs[0], (wpp * len(zs),), np.uint64)
                want = _want_bits(lk, nz, zs, dogmax[k])
                assert np.array_equal(got, want), f"fused level {k} planes {zs}: {int((got != want).sum())} words differ"
                total += int(np.bitwise_count(want).sum())
        assert total > 1000000
        for p in d_bits:
            B.ptrs.remove(p)
            dev.free(p)
        # -- per-level kernel: 192 planes, voxel indices up to 3 * 2^30 --
        for k in range(4):
            _fill_periodic(dev, d_lv[k], lv[k], nz_big)
        nw = n_big // 64
        d_b = B.alloc(8 * nw)
        assert L.s3d_k_extrema(d_lv[0], d_lv[1], d_lv[2], d_lv[3], EXT_NX, EXT_NY, nz_big, PEAK, _vp(d_max), _vp(d_b),
                               None) == 0
        cap = n_big // 3
        d_idx, d_tag = B.alloc(4 * cap), B.alloc(4 * cap)
        d_cnt = B.alloc(16)
        d_scr = B.alloc(4 * (nw // 1024 + 2))
        dev.check(L.s3d_rt_memset(_vp(d_cnt), 0, 16, None), "memset")
        assert L.s3d_k_compact_bits(_vp(d_b), nw, _vp(d_idx), _vp(d_tag), 0, cap, _vp(d_cnt), _vp(d_scr), None) == 0
        dev.sync()
        B.report("extrema")
        allbits = _d2h(dev, d_b, 0, (nw,), np.uint64)
        count = int(_d2h(dev, d_cnt, 0, (1,), np.uint32)[0])
        assert count == int(np.bitwise_count(allbits).sum()) and count <= cap
        z_hi = 2**31 // plane                                                        # 128: the first plane above 2^31
        for zs in ([1, 2], [96], [z_hi - 1, z_hi, z_hi + 1], [nz_big - 2, nz_big - 1]):
            w0 = wpp * zs[0]
            got = allbits[w0:w0 + wpp * len(zs)]
            want = _want_bits(lv[0:4], nz_big, zs, dogmax[0])
            assert np.array_equal(got, want), f"k_extrema planes {zs}: {int((got != want).sum())} words differ"
            # the compacted indices of these planes: ascending voxel indices, the same as the bitmap's
            before = int(np.bitwise_count(allbits[:w0]).sum())
            bits = np.unpackbits(want.view(np.uint8), bitorder="little")
            want_idx = (np.flatnonzero(bits) + 64 * w0).astype(np.uint64)
            got_idx = _d2h(dev, d_idx, 4 * before, (len(want_idx),), np.uint32).astype(np.uint64)
            assert np.array_equal(got_idx, want_idx), f"compacted indices of planes {zs} differ"
            if zs[0] >= z_hi:
                assert len(want_idx) > 0 and want_idx.min() >= 2**31
    finally:
        B.free()
