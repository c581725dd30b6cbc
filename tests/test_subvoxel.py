"""CPU: sub-voxel keypoints (sift3d_amd_set_subvoxel, s3d_k_refine_keys, SIFT3D_SUBVOXEL, kpSift3D --subvoxel).

The product's sources run on the SIMT emulator (tests/emu).  The contract every test here uses: a detect with refinement on
returns the list the same detect returns with it off -- same count, order, o, s and R -- with xd, yd, zd moved by the offsets of
a separable quadratic fit to the DoG (a 3-D fit in space where the Hessian is definite and the step stays within the voxel, per-axis
parabolas otherwise; an independent parabola over the levels) and sd multiplied by 2^(ds / num_kp_levels).  Expected values come
from the oracle (its candidate and keypoint lists, its DoG levels) and from the numpy restatement `restate` (np.linalg.solve in
f64), never from the library.  tests/test_gpu_subvoxel.py runs the same bodies on the device (`gpu=True`: buffers go through HBM)."""
import ctypes as C
import gzip
import os
import subprocess

import numpy as np
import pytest

from sift3d_amd import abi, synth
from sift3d_amd.device import DeviceLib, bind_extensions
from tests import parity
from tests import test_budget as B
from tests import test_mask as M
from tests import test_typed_input as T
from tests.test_host_io import nifti1_bytes

ROOT = M.ROOT
EMU_DIR = M.EMU_DIR
P = C.POINTER
UNIT = (1.0, 1.0, 1.0)
FIRST, NKP = -1, 3                      # first pyramid level and keypoint levels per octave of the default parameters
NGSS, NDOG = NKP + 3, NKP + 2
TOL = 1e-9                              # offsets are <= 0.5 and cond(H3) < 1e4: rounding ~1e-12; room for another operation order
SENTINEL = 0xA5A5A5A5
SMALL = (24, 20, 18, 80, 0.04)          # nx, ny, nz, blobs, peak threshold (seed 1): 4 keypoints, a detect in a fraction of a second


@pytest.fixture(scope="module")
def emu():
    subprocess.run(["sh", os.path.join(EMU_DIR, "build_emu.sh")], check=True, capture_output=True)
    L = C.CDLL(os.path.join(EMU_DIR, "libsift3d_emu.so"))
    lib = abi.Sift3dLib(L, None, "emulated")
    bind_extensions(L)
    return lib


# ---- the oracle's pass over a volume, kept --------------------------------------------------------------------------------------
def snapshot(oracle, vol, units, key=None, **params):
    """One oracle detect: its keypoints, its candidates and every GSS and DoG level, copied out (the oracle holds one pass)."""
    if params:
        oracle.set_params(**params)
    try:
        xyzos, sd, R = oracle.detect(vol, units)
        noct = oracle.num_octaves()
        st = dict(key=key, vol=vol, units=units, xyzos=xyzos, sd=sd, R=R, cands=oracle.candidates()[0], noct=noct, gss={}, dog={},
                  scale={}, units_o={}, dog64={})
        for o in range(noct):
            st["units_o"][o] = oracle.level("gss", o, FIRST)[1]
            for s in range(FIRST, FIRST + NGSS):
                st["gss"][(o, s)] = oracle.level("gss", o, s)[0]
            for s in range(FIRST, FIRST + NDOG):
                st["dog"][(o, s)], _, st["scale"][(o, s)] = oracle.level("dog", o, s)
                # the DoG the kernel forms from two GSS levels is the voxel the oracle stores
                assert st["dog"][(o, s)].tobytes() == (st["gss"][(o, s)] - st["gss"][(o, s + 1)]).tobytes()
    finally:
        if params:
            oracle.set_params()
    return st


_snap = {}


def volume_snapshot(oracle, i):
    if i not in _snap:
        dims, units, nblobs, seed, _ = T.VOLUMES[i]
        _snap[i] = snapshot(oracle, synth.blobs(*dims, nblobs, seed), units, key=("vol", i))
        assert (len(_snap[i]["xyzos"]), len(_snap[i]["cands"])) == B.COUNTS[i][:2], "the oracle's counts moved"
    return _snap[i]


# ---- the restatement --------------------------------------------------------------------------------------------------------------
def parabola(g, h):
    if h == 0.0:
        return 0.0
    with np.errstate(all="ignore"):
        v = -g / h
    return float(np.clip(v, -0.5, 0.5)) if np.isfinite(v) else 0.0


def restate(st, recs):
    """Offsets [n, 4] (dx, dy, dz, ds), flags [n] (1: the 3-D fit, 2: the per-axis fallback), cond(H3) [n] and the raw 3-D
    solution [n, 3] of the records x, y, z, o, s on the oracle's DoG levels, in f64."""
    recs = np.asarray(recs, np.int64).reshape(-1, 5)
    n = len(recs)
    off, flags, cond, raw = np.zeros((n, 4)), np.zeros(n, np.uint32), np.zeros(n), np.full((n, 3), np.nan)
    for i, (x, y, z, o, s) in enumerate(recs):
        for l in (s - 1, s, s + 1):
            if (o, l) not in st["dog64"]:
                st["dog64"][(o, l)] = st["dog"][(o, l)].astype(np.float64)
        D = st["dog64"][(o, s)]
        assert 1 <= x <= D.shape[2] - 2 and 1 <= y <= D.shape[1] - 2 and 1 <= z <= D.shape[0] - 2
        d0 = D[z, y, x]
        e = np.eye(3, dtype=np.int64)

        def at(v):
            return D[z + v[2], y + v[1], x + v[0]]
        g = np.array([0.5 * (at(e[a]) - at(-e[a])) for a in range(3)])
        H = np.zeros((3, 3))
        for a in range(3):
            H[a, a] = at(e[a]) + at(-e[a]) - 2.0 * d0
            for b in range(a + 1, 3):
                H[a, b] = H[b, a] = 0.25 * (at(e[a] + e[b]) - at(e[a] - e[b]) - at(-e[a] + e[b]) + at(-e[a] - e[b]))
        sm, sp = st["dog64"][(o, s - 1)][z, y, x], st["dog64"][(o, s + 1)][z, y, x]
        with np.errstate(all="ignore"):
            cond[i] = np.linalg.cond(H)
            try:
                raw[i] = np.linalg.solve(H, -g)
            except np.linalg.LinAlgError:
                pass
        definite = any(all(np.linalg.det(sg * H[:k, :k]) > 0.0 for k in (1, 2, 3)) for sg in (1.0, -1.0))   # Sylvester
        if definite and np.isfinite(raw[i]).all() and np.abs(raw[i]).max() <= 0.5:
            off[i, :3], flags[i] = raw[i], 1
        else:
            off[i, :3], flags[i] = [parabola(g[a], H[a, a]) for a in range(3)], 2
        off[i, 3] = parabola(0.5 * (sp - sm), sp + sm - 2.0 * d0)
    return off, flags, cond, raw


def usable(st, recs):
    """The condition on the inputs, checked on the restatement alone: cond(H3) < 1e4 and no 3-D offset within 1e-6 of 0.5 (where
    the two sides of the test could differ legitimately).  At most 2 % of a list may go."""
    _, _, cond, raw = restate(st, recs)
    with np.errstate(invalid="ignore"):
        ok = (cond < 1e4) & ~(np.abs(np.abs(raw) - 0.5) < 1e-6).any(axis=1)
    assert (~ok).sum() <= 0.02 * len(ok), f"{(~ok).sum()} of {len(ok)} records are ill-conditioned"
    return ok


# ---- the kernel on caller-built records -------------------------------------------------------------------------------------------
_pd = {}


def pyr_desc(lib, st, gpu):
    """s3d_pyramid_desc over the oracle's GSS levels (uploaded once per library and pass; the tests read them only)."""
    key = (lib.name, gpu, st["key"])
    if key not in _pd:
        dev = DeviceLib(lib.sift)
        pd = parity._PyrDesc()
        hold, d_ptrs = [], []
        for o in range(st["noct"]):
            for k in range(NGSS):
                a = np.ascontiguousarray(st["gss"][(o, k + FIRST)])
                if gpu:
                    d_ptrs.append(dev.upload(a))
                else:
                    hold.append(a)
                pd.d_level[o * NGSS + k] = d_ptrs[-1] if gpu else a.ctypes.data
            nz, ny, nx = st["gss"][(o, FIRST)].shape
            pd.dims[o][0], pd.dims[o][1], pd.dims[o][2] = nx, ny, nz
            for a_ in range(3):
                pd.unitsf[o][a_] = float(st["units_o"][o][a_])
        pd.num_octaves, pd.num_levels, pd.first_level = st["noct"], NGSS, FIRST
        _pd[key] = (pd, hold, d_ptrs)
    return _pd[key][0]


def release_pyr_desc(lib, st, gpu):
    for p in _pd.pop((lib.name, gpu, st["key"]), (None, [], []))[2]:
        DeviceLib(lib.sift).free(p)


def run_kernel(lib, st, recs, gpu, slack=37):
    """s3d_k_refine_keys on `recs` with a grid bound `slack` records above the count: (offsets, flags, counters).  The slots
    past the count hold records that must not be read (far outside every level) and outputs that must not be written."""
    dev = DeviceLib(lib.sift)
    recs = np.ascontiguousarray(recs, np.int32).reshape(-1, 5)
    n, cap = len(recs), len(recs) + slack
    xyzos = np.full((cap, 5), 0x3FFFFFFF, np.int32)
    xyzos[:n] = recs
    off = np.full((cap, 4), np.nan)
    flags = np.full(cap, SENTINEL, np.uint32)
    num = np.array([n], np.uint32)
    counters = np.full(4, SENTINEL, np.uint32)
    arrs = [xyzos, num, off, flags, counters]
    ptr = [dev.upload(a) for a in arrs] if gpu else [a.ctypes.data for a in arrs]
    dev.refine_keys(pyr_desc(lib, st, gpu), ptr[0], ptr[1], cap, ptr[2], ptr[3], ptr[4])
    dev.sync()
    if gpu:
        off, flags, counters = dev.download(ptr[2], off.shape, np.float64), dev.download(ptr[3], flags.shape, np.uint32), \
            dev.download(ptr[4], counters.shape, np.uint32)
        for p in ptr:
            dev.free(p)
    assert np.isnan(off[n:]).all() and (flags[n:] == SENTINEL).all(), "wrote past the count on the device"
    assert (counters[2:] == SENTINEL).all(), "the call owns two counters"
    return off[:n], flags[:n], counters[:2]


def assert_kernel_is_restatement(lib, st, recs, gpu, what=""):
    w_off, w_flags, _, _ = restate(st, recs)
    off, flags, counters = run_kernel(lib, st, recs, gpu)
    assert np.array_equal(flags, w_flags), f"{what}: flags differ at {np.flatnonzero(flags != w_flags)[:8]}"
    err = np.abs(off - w_off).max(initial=0.0)
    print(f"{what}: {len(recs)} records, {int((w_flags == 1).sum())} 3-D fits, max |offset - restatement| = {err:.3e}")
    assert err <= TOL, f"{what}: offsets differ from the restatement by {err}"
    assert np.abs(off).max(initial=0.0) <= 0.5
    assert tuple(counters) == (int((w_flags == 1).sum()), int((w_flags == 2).sum()))
    return off, flags


# ---- 1: the kernel against the restatement -----------------------------------------------------------------------------------------
LENGTHS = [1, 63, 64, 65, 256, 257]


def check_kernel(lib, oracle, i, length, gpu):
    st = volume_snapshot(oracle, i)
    cands = st["cands"][usable(st, st["cands"])]
    assert len(cands) >= 55 and len(np.unique(cands[:, 3])) == B.COUNTS[i][2] and len(np.unique(cands[:, 4])) == NKP
    recs = cands[np.arange(length) % len(cands)]                     # a prefix, or the list repeated
    _, flags = assert_kernel_is_restatement(lib, st, recs, gpu, f"{T.VOLUMES[i][0]} x {length}")
    if length >= 256:
        assert (flags == 1).any() and (flags == 2).any(), "both branches are taken"


@pytest.mark.parametrize("length", LENGTHS)
@pytest.mark.parametrize("i", range(5))
def test_kernel_against_the_restatement(emu, oracle, i, length):
    check_kernel(emu, oracle, i, length, gpu=False)


def check_unrefinable(lib, oracle, gpu):
    """Caller-built records the fit has no neighbours for -- a face voxel, a level without both DoG neighbours, an octave that
    does not exist -- get zero offsets and flag bit 2, count in neither counter, and are not read."""
    st = volume_snapshot(oracle, 1)
    nz, ny, nx = st["gss"][(0, 0)].shape
    good = st["cands"][usable(st, st["cands"])][:3]
    bad = np.array([[0, 5, 5, 0, 0], [5, ny - 1, 5, 0, 1], [5, 5, nz - 1, 0, 2], [5, 5, 5, 0, FIRST], [5, 5, 5, 0, FIRST + NDOG - 1],
                    [5, 5, 5, st["noct"], 0], [5, 5, 5, -1, 0], [nx, 5, 5, 0, 0], [-3, 5, 5, 0, 0]], np.int32)
    recs = np.concatenate([good[:1], bad[:4], good[1:2], bad[4:], good[2:]])
    isbad = np.array([0] + [1] * 4 + [0] + [1] * 5 + [0], bool)
    off, flags, counters = run_kernel(lib, st, recs, gpu)
    w_off, w_flags, _, _ = restate(st, recs[~isbad])
    assert (flags[isbad] == 4).all() and (off[isbad] == 0.0).all()
    assert np.array_equal(flags[~isbad], w_flags) and np.abs(off[~isbad] - w_off).max() <= TOL
    assert int(counters.sum()) == 3
    # no records at all: the counters are cleared, nothing else happens
    off, flags, counters = run_kernel(lib, st, np.zeros((0, 5), np.int32), gpu)
    assert len(off) == 0 and tuple(counters) == (0, 0)


def test_records_that_cannot_be_refined(emu, oracle):
    check_unrefinable(emu, oracle, gpu=False)


# ---- 2: accuracy on isolated blobs --------------------------------------------------------------------------------------------------
def check_isolated_blobs(lib, oracle, gpu):
    rng = np.random.default_rng(0)
    z, y, x = np.meshgrid(*[np.arange(48.0)] * 3, indexing="ij")
    total, worst = 0, 0.0
    for t in range(12):
        c = 24 + rng.uniform(-0.5, 0.5, 3)
        sigma = rng.uniform(2.0, 3.5)
        vol = np.exp(-((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2) / (2 * sigma ** 2)).astype(np.float32)
        st = snapshot(oracle, vol, UNIT, key=("blob", t))
        cands = st["cands"]
        near = cands[(cands[:, 3] == 0) & (np.linalg.norm(cands[:, :3] - c, axis=1) <= 2.0)]
        if len(near) == 0:
            continue
        near = near[usable(st, near)]
        off, flags, _, _ = restate(st, near)
        err = np.linalg.norm(near[:, :3] + off[:, :3] - c, axis=1)
        int_err = np.linalg.norm(near[:, :3] - c, axis=1)
        print(f"blob {t}: centre {c}, sigma {sigma:.3f}: {len(near)} candidates, integer error {int_err}, refined error {err}")
        assert (err <= 0.05).all(), f"blob {t}: the restated fit misses the centre by {err.max():.4f} voxel"
        assert_kernel_is_restatement(lib, st, near, gpu, f"blob {t}")
        total += len(near)
        worst = max(worst, float(err.max()))
        release_pyr_desc(lib, st, gpu)
    assert total >= 10, f"only {total} candidates at the blobs' centres"


def test_isolated_blobs(emu, oracle):
    check_isolated_blobs(emu, oracle, gpu=False)


# ---- runs through the public API ---------------------------------------------------------------------------------------------------
def run(lib, vol, units, subvoxel=None, n=0, mask=None, params=None, describe=False):
    """One detect on a fresh struct.  subvoxel: None leaves the struct alone (the environment decides), else set_subvoxel."""
    L = lib.sift
    s = T.new_sift(lib)
    for k, v in (params or {}).items():
        assert getattr(L, f"set_{k}_SIFT3D")(C.byref(s), v) == 0
    if mask is not None:
        assert M.set_mask(lib, s, mask) == 0, L.sift3d_amd_last_error()
    if n:
        B.set_budget(lib, s, n)
    if subvoxel is not None:
        assert abi.set_subvoxel(L, s, subvoxel) == 0 and abi.get_subvoxel(L, s) == bool(subvoxel)
    kp = T.float_detect(lib, s, vol, units)
    xyz, o, lev, sd, R = abi.refined_keypoints_to_numpy(kp)
    out = dict(rows=M.record_rows(kp), xyz=xyz, o=o, s=lev, sd=sd, R=R, counts=abi.last_subvoxel_counts(L, s),
               mode=abi.get_subvoxel(L, s), ncand=L.sift3d_amd_last_num_candidates(C.byref(s)))
    if describe:
        out["bins"], out["xyzs"] = M.descriptors(lib, s, kp)
    L.cleanup_Keypoint_store(C.byref(kp))
    L.cleanup_SIFT3D(C.byref(s))
    return out


def assert_integer_list(got, st, keep=None, what=""):
    """An unrefined result is the oracle's list: positions, o, s and sd equal, R within the detect contract's 1e-5."""
    keep = np.ones(len(st["xyzos"]), bool) if keep is None else keep
    w = st["xyzos"][keep]
    assert len(got["xyz"]) == len(w), what
    assert np.array_equal(got["xyz"], w[:, :3].astype(np.float64)) and np.array_equal(got["o"], w[:, 3]), what
    assert np.array_equal(got["s"], w[:, 4]) and np.array_equal(got["sd"], st["sd"][keep]), what
    assert np.abs(got["R"] - st["R"][keep]).max(initial=0) <= 1e-5, what
    assert got["counts"] == (0, 0) and got["mode"] is False, what


def assert_refined_list(got, base, st, keep=None, what=""):
    """`got` (refined run) against the restated offsets of the oracle's list on the oracle's DoG, and against `base` (the
    unrefined run of the same library with the same settings; None: not compared)."""
    keep = np.ones(len(st["xyzos"]), bool) if keep is None else keep
    w = st["xyzos"][keep]
    assert len(got["xyz"]) == len(w), f"{what}: {len(got['xyz'])} keypoints, {len(w)} expected"
    assert np.array_equal(got["o"], w[:, 3]) and np.array_equal(got["s"], w[:, 4]), what
    assert np.abs(got["R"] - st["R"][keep]).max(initial=0) <= 1e-5, what
    assert usable(st, w).all(), what
    off, flags, _, _ = restate(st, w)
    err = np.abs(got["xyz"] - (w[:, :3] + off[:, :3])).max(initial=0.0)
    w_sd = st["sd"][keep] * 2.0 ** (off[:, 3] / NKP)
    sd_err = np.abs(got["sd"] / w_sd - 1.0).max(initial=0.0)
    print(f"{what}: {len(w)} keypoints, {int((flags == 1).sum())} 3-D fits, max position error {err:.3e}, sd {sd_err:.3e}")
    assert err <= TOL and sd_err <= 1e-12, (what, err, sd_err)
    assert np.abs(got["xyz"] - w[:, :3]).max(initial=0.0) <= 0.5
    assert got["counts"] == (int((flags == 1).sum()), int((flags == 2).sum())) and got["mode"] is True, what
    if base is None:
        return off, flags
    # the records differ from the unrefined ones in xd, yd, zd and sd only: R is assigned at the integer voxel
    assert got["ncand"] == base["ncand"] and got["R"].tobytes() == base["R"].tobytes(), what
    a, b = got["rows"].copy(), base["rows"].copy()
    first = abi.Keypoint.r_data.size + abi.Keypoint.xd.offset - abi.Keypoint.R.offset - 8
    for r in (a, b):
        r[:, first:first + 32] = 0
    assert a.tobytes() == b.tobytes(), f"{what}: the records differ outside xd, yd, zd, sd"
    return off, flags


# ---- 3: the contract ----------------------------------------------------------------------------------------------------------------
_off_runs = {}


def unrefined(lib, st, i):
    if (lib.name, i) not in _off_runs:
        _off_runs[(lib.name, i)] = run(lib, st["vol"], st["units"], subvoxel=False)
    return _off_runs[(lib.name, i)]


def check_contract(lib, oracle, i):
    st = volume_snapshot(oracle, i)
    base = unrefined(lib, st, i)
    assert_integer_list(base, st, what=f"{T.VOLUMES[i][0]} off")
    got = run(lib, st["vol"], st["units"], subvoxel=True)
    off, flags = assert_refined_list(got, base, st, what=f"{T.VOLUMES[i][0]} on")
    assert (np.abs(off[:, :3]).max(axis=1) > 0.01).sum() > len(off) // 2, "the offsets are not trivial"


@pytest.mark.parametrize("i", range(5))
def test_refined_detect_is_the_integer_detect_moved(emu, oracle, i, monkeypatch):
    monkeypatch.delenv("SIFT3D_SUBVOXEL", raising=False)
    check_contract(emu, oracle, i)


def check_with_mask_and_budget(lib, oracle):
    """Volume 1: a mask, a budget, and both.  Expected list: oracle list -> mask -> top n; the offsets are those of the survivors."""
    i, n = 1, 3
    st = volume_snapshot(oracle, i)
    strength = B.oracle_strengths(oracle_of(st), st["xyzos"])
    mask = M.make_mask("ball", st["vol"].shape)
    inside = M.kept(st["xyzos"], mask)
    assert 0 < n < int(inside.sum()) < len(inside)
    both = np.zeros(len(inside), bool)
    both[np.flatnonzero(inside)[B.top_n(strength[inside], n)]] = True
    for what, kw, keep in (("mask", dict(mask=mask), inside), ("budget", dict(n=n), B.top_n(strength, n)),
                           ("mask + budget", dict(mask=mask, n=n), both)):
        base = None
        if what != "mask + budget":                                  # (the third case: against the oracle and the restatement alone)
            base = run(lib, st["vol"], st["units"], subvoxel=False, **kw)
            assert_integer_list(base, st, keep, what)
        got = run(lib, st["vol"], st["units"], subvoxel=True, **kw)
        assert_refined_list(got, base, st, keep, what)


class oracle_of:
    """B.oracle_strengths reads DoG levels through `.level`: serve it the snapshot's."""

    def __init__(self, st):
        self.st = st

    def level(self, which, o, s):
        assert which == "dog"
        return self.st["dog"][(o, s)], None, None


def test_mask_and_budget_compose(emu, oracle, monkeypatch):
    monkeypatch.delenv("SIFT3D_SUBVOXEL", raising=False)
    check_with_mask_and_budget(emu, oracle)


def check_lifecycle(lib, oracle, monkeypatch):
    """The getter, the counters, copy_SIFT3D and SIFT3D_SUBVOXEL."""
    L = lib.sift
    params = {"peak_thresh": SMALL[4]}
    st = snapshot(oracle, synth.blobs(*SMALL[:3], SMALL[3], 1), UNIT, key=("small",), peak=SMALL[4])
    assert len(st["xyzos"]) == 4
    monkeypatch.delenv("SIFT3D_SUBVOXEL", raising=False)
    base = run(lib, st["vol"], UNIT, subvoxel=False, params=params)
    plain = run(lib, st["vol"], UNIT, params=params)                     # no call, no variable: the integer list
    assert plain["rows"].tobytes() == base["rows"].tobytes() and plain["mode"] is False and plain["counts"] == (0, 0)
    assert_integer_list(plain, st, what="unset")
    on = run(lib, st["vol"], UNIT, subvoxel=True, params=params)
    assert_refined_list(on, base, st, what="on")
    assert on["rows"].tobytes() != base["rows"].tobytes()

    def new_sift():
        s = T.new_sift(lib)
        assert L.set_peak_thresh_SIFT3D(C.byref(s), SMALL[4]) == 0
        return s

    def detect(s):
        kp = T.float_detect(lib, s, st["vol"], UNIT)
        rows = M.record_rows(kp)
        L.cleanup_Keypoint_store(C.byref(kp))
        return rows

    # a struct switches back and forth; the counters follow
    s = new_sift()
    assert abi.get_subvoxel(L, s) is False and abi.last_subvoxel_counts(L, s) == (0, 0)
    assert abi.set_subvoxel(L, s, True) == 0 and abi.get_subvoxel(L, s) is True
    for _ in range(2):
        assert detect(s).tobytes() == on["rows"].tobytes() and abi.last_subvoxel_counts(L, s) == on["counts"]
    assert sum(on["counts"]) == len(on["rows"]) and on["counts"][0] > 0
    # copy_SIFT3D carries the setting, as a copy
    L.copy_SIFT3D.argtypes = [P(abi.SIFT3D), P(abi.SIFT3D)]
    s2 = new_sift()
    assert L.copy_SIFT3D(C.byref(s), C.byref(s2)) == 0 and abi.get_subvoxel(L, s2) is True
    assert detect(s2).tobytes() == on["rows"].tobytes()
    assert abi.set_subvoxel(L, s2, False) == 0 and abi.get_subvoxel(L, s) is True
    assert detect(s2).tobytes() == base["rows"].tobytes() and abi.last_subvoxel_counts(L, s2) == (0, 0)
    L.cleanup_SIFT3D(C.byref(s2))
    assert abi.set_subvoxel(L, s, False) == 0
    assert detect(s).tobytes() == base["rows"].tobytes() and abi.last_subvoxel_counts(L, s) == (0, 0)
    L.cleanup_SIFT3D(C.byref(s))
    # the environment switch: unchanged callers get refinement; read once per struct; an explicit call overrides it
    monkeypatch.setenv("SIFT3D_SUBVOXEL", "1")
    s = new_sift()
    assert abi.get_subvoxel(L, s) is True
    assert detect(s).tobytes() == on["rows"].tobytes()
    monkeypatch.setenv("SIFT3D_SUBVOXEL", "0")
    assert detect(s).tobytes() == on["rows"].tobytes(), "the variable is read once per struct"
    L.cleanup_SIFT3D(C.byref(s))
    s = new_sift()
    assert abi.get_subvoxel(L, s) is False
    assert detect(s).tobytes() == base["rows"].tobytes()
    L.cleanup_SIFT3D(C.byref(s))
    monkeypatch.setenv("SIFT3D_SUBVOXEL", "1")
    off = run(lib, st["vol"], UNIT, subvoxel=False, params=params)
    assert off["rows"].tobytes() == base["rows"].tobytes(), "an explicit 0 overrides the variable"
    monkeypatch.delenv("SIFT3D_SUBVOXEL")


def test_lifecycle(emu, oracle, monkeypatch):
    check_lifecycle(emu, oracle, monkeypatch)


def check_loopback_ranks(lib, ranks=2):
    """Two loop-back Z-slab ranks and refinement: the detect fails and says why; switched off, the same struct detects."""
    L = lib.sift
    L.sift3d_amd_set_num_gpus.argtypes = [P(abi.SIFT3D), C.c_int, C.c_int]
    dims, units, nblobs, seed, params = parity.NONFINITE_BASES["slab64"]
    vol = synth.blobs(*dims, nblobs, seed)
    base = run(lib, vol, units, subvoxel=False, params=params)
    assert len(base["rows"]) > 3
    s = T.new_sift(lib)
    for k, v in params.items():
        assert getattr(L, f"set_{k}_SIFT3D")(C.byref(s), v) == 0
    assert L.sift3d_amd_set_num_gpus(C.byref(s), ranks, 1) == 0                # 1 = SIFT3D_AMD_SLAB_LOOPBACK
    assert abi.set_subvoxel(L, s, True) == 0
    im = lib.image_from_numpy(vol, units)
    kp = T.new_kp(lib)
    assert L.SIFT3D_detect_keypoints(C.byref(s), C.byref(im), C.byref(kp)) == -1
    msg = L.sift3d_amd_last_error().decode()
    assert "sub-voxel" in msg and "several GPUs" in msg, msg
    assert abi.set_subvoxel(L, s, False) == 0
    assert L.SIFT3D_detect_keypoints(C.byref(s), C.byref(im), C.byref(kp)) == 0
    assert M.record_rows(kp).tobytes() == base["rows"].tobytes()
    lib.free_image(im)
    L.cleanup_Keypoint_store(C.byref(kp))
    L.cleanup_SIFT3D(C.byref(s))


def test_two_loopback_ranks_refuse_refinement(emu, monkeypatch):
    monkeypatch.delenv("SIFT3D_SUBVOXEL", raising=False)
    monkeypatch.setenv("S3D_EMU_DEVICES", "2")
    check_loopback_ranks(emu)


# ---- 4: describe at refined keys -----------------------------------------------------------------------------------------------------
def check_describe(lib, oracle, i):
    """SIFT3D_extract_descriptors on the refined store against the oracle's describe at the library's own refined doubles."""
    dims, units, nblobs, seed, _ = T.VOLUMES[i]
    vol = synth.blobs(*dims, nblobs, seed)
    got = run(lib, vol, units, subvoxel=True, describe=True)
    assert len(got["xyz"]) == B.COUNTS[i][0] and (got["xyz"] != np.rint(got["xyz"])).any(axis=1).sum() > len(got["xyz"]) // 2
    oracle.detect(vol, units)                                          # the oracle describes from its last pass
    wb, wx = oracle.describe(got["xyz"], np.stack([got["o"], got["s"]], axis=1), got["sd"], got["R"])
    f = np.ldexp(1.0, got["o"])[:, None]
    assert np.array_equal(got["xyzs"][:, :3], got["xyz"] * f) and np.array_equal(got["xyzs"][:, 3], got["sd"])
    assert np.array_equal(got["xyzs"], wx)
    ok = parity.rel_close(got["bins"], wb, rtol=1e-4, atol=1e-7)
    assert ok.all(), f"{(~ok).sum()} descriptor floats beyond 1e-4 relative, max abs {np.abs(got['bins'] - wb).max()}"


@pytest.mark.parametrize("i", [1, 3, 4])
def test_descriptors_at_refined_keys(emu, oracle, i, monkeypatch):
    monkeypatch.delenv("SIFT3D_SUBVOXEL", raising=False)
    check_describe(emu, oracle, i)


# ---- 5: shift recovery -----------------------------------------------------------------------------------------------------------------
SHIFT = np.array([0.3, 0.4, -0.2])


def shift_volume(shift, seed, n=56, nblobs=70):
    rng = np.random.default_rng(seed)
    z, y, x = np.meshgrid(*[np.arange(float(n))] * 3, indexing="ij")
    acc = np.zeros((n, n, n), np.float64)
    for _ in range(nblobs):
        c = rng.uniform(4, n - 4, 3) + shift
        s = rng.uniform(1.5, 4)
        a = rng.uniform(0.3, 1) * rng.choice([-1, 1])
        sx, sy, sz = s * rng.uniform(0.7, 1.4, 3)
        acc += a * np.exp(-((x - c[0]) ** 2 / (2 * sx ** 2) + (y - c[1]) ** 2 / (2 * sy ** 2) + (z - c[2]) ** 2 / (2 * sz ** 2)))
    return acc.astype(np.float32)


def check_shift_recovery(lib, oracle, seed):
    sts = [snapshot(oracle, shift_volume(sh, seed), UNIT, key=("shift", seed, k)) for k, sh in enumerate((np.zeros(3), SHIFT))]
    offs = []
    for st in sts:
        assert usable(st, st["xyzos"]).all()
        offs.append(restate(st, st["xyzos"])[0])
    A, Bk = sts[0]["xyzos"].astype(np.int64), sts[1]["xyzos"].astype(np.int64)
    pairs = []
    for ia, ra in enumerate(A):
        near = np.flatnonzero((Bk[:, 3] == ra[3]) & (Bk[:, 4] == ra[4]) & (np.abs(Bk[:, :3] - ra[:3]).max(axis=1) <= 1))
        if len(near):
            pairs.append((ia, near[np.argmin(np.abs(Bk[near, :3] - ra[:3]).sum(axis=1))]))
    ia, ib = np.array(pairs).T
    f = np.ldexp(1.0, A[ia, 3])[:, None]

    def residual(pa, pb):
        return np.linalg.norm(pb - pa - SHIFT / f, axis=1) * f[:, 0]
    r_int = residual(A[ia, :3].astype(np.float64), Bk[ib, :3].astype(np.float64))
    r_ref = residual(A[ia, :3] + offs[0][ia, :3], Bk[ib, :3] + offs[1][ib, :3])
    print(f"seed {seed}: {len(pairs)} pairs, median residual integer {np.median(r_int):.3f} refined {np.median(r_ref):.3f} "
          f"(ratio {np.median(r_ref) / np.median(r_int):.2f}), mean {r_int.mean():.3f} -> {r_ref.mean():.3f}")
    assert len(pairs) >= 8
    assert np.median(r_ref) <= 0.75 * np.median(r_int), "the restated fit does not recover the shift"
    for st in sts:                                                       # the library is the restatement
        assert_refined_list(run(lib, st["vol"], UNIT, subvoxel=True), None, st, what=f"seed {seed} on")


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_shift_recovery(emu, oracle, seed, monkeypatch):
    monkeypatch.delenv("SIFT3D_SUBVOXEL", raising=False)
    check_shift_recovery(emu, oracle, seed)


# ---- 6: kpSift3D --subvoxel ------------------------------------------------------------------------------------------------------------
def check_cli(lib, tmp_path, env, oracle, dims=SMALL[:3], nblobs=SMALL[3], seed=1, peak=SMALL[4]):
    prog = os.path.join(ROOT, "sift3d_amd", "bin", "kpSift3D")
    if not os.path.exists(prog):
        from sift3d_amd import build as _b
        _b.build()
    vol = synth.blobs(*dims, nblobs, seed)
    src = str(tmp_path / "vol.nii.gz")
    with gzip.open(src, "wb") as f:
        f.write(nifti1_bytes(np.ascontiguousarray(vol.transpose(2, 1, 0)), UNIT))
    e = dict(os.environ if env is None else dict(os.environ, **env))
    e.pop("SIFT3D_SUBVOXEL", None)

    def kp_run(*args):
        return subprocess.run([prog, "--peak_thresh", str(peak), *args, src], capture_output=True, text=True, timeout=600, env=e)

    def csv(r):
        rows = zip(r["xyz"], r["o"], r["sd"], r["R"])
        return [",".join("%f" % v for v in (*xyz, float(o), sd, *R.ravel().astype(np.float64))) for xyz, o, sd, R in rows]

    st = snapshot(oracle, vol, UNIT, key=("cli",), peak=peak)
    assert len(st["xyzos"]) >= 3, "the volume has keypoints"
    params = {"peak_thresh": peak}
    base = run(lib, vol, UNIT, subvoxel=False, params=params)
    assert_integer_list(base, st, what="cli off")
    want = run(lib, vol, UNIT, subvoxel=True, params=params)
    assert_refined_list(want, base, st, what="cli on")
    plain, fine = str(tmp_path / "k0.csv"), str(tmp_path / "k1.csv")
    r = kp_run("--keys", plain)
    assert r.returncode == 0, r.stderr
    r = kp_run("--subvoxel", "--keys", fine)
    assert r.returncode == 0, r.stderr
    assert open(plain).read().splitlines() == csv(base)
    assert open(fine).read().splitlines() == csv(want) != csv(base)
    r = subprocess.run([prog, "--help"], capture_output=True, text=True, timeout=60)
    assert r.stdout.startswith("Usage: kpSift3D [image.nii]") and " --subvoxel \n" in r.stdout


def test_kpSift3D_subvoxel_emulated(emu, oracle, tmp_path, monkeypatch):
    monkeypatch.delenv("SIFT3D_SUBVOXEL", raising=False)
    check_cli(emu, tmp_path, {"LD_PRELOAD": os.path.join(EMU_DIR, "libsift3d_emu.so")}, oracle)
