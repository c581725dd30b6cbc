"""CPU: a keypoint budget (sift3d_amd_set_max_keypoints, sift3d_amd_keypoint_strengths, s3d_k_key_strength,
s3d_k_select_strongest).

The product's sources run on the SIMT emulator (tests/emu).  The contract every test here uses: the strength of a keypoint
(x, y, z, o, s) is |D| of voxel (x, y, z) of DoG level (o, s) as the reference stores it, and a detect with a budget N returns
exactly the list the same detect returns without one, with every record deleted except the N of largest strength -- equal
strengths to the earlier record, survivors in the reference's order and byte for byte the unbudgeted run's.  Expected values
come from the oracle (its keypoint list, its DoG levels) and from the numpy restatement `top_n`, never from the library.
tests/test_gpu_budget.py runs the same bodies on the device (`gpu=True`: buffers go through HBM)."""
import ctypes as C
import gzip
import os
import subprocess

import numpy as np
import pytest

from sift3d_amd import abi, synth
from sift3d_amd.device import DeviceLib, bind_extensions
from tests import parity
from tests import test_mask as M
from tests import test_typed_input as T
from tests.test_host_io import nifti1_bytes

ROOT = M.ROOT
EMU_DIR = M.EMU_DIR
P = C.POINTER
UNIT = (1.0, 1.0, 1.0)

# The oracle's counts for the first four T.VOLUMES and the anisotropic fifth: keypoints, candidates, octaves that hold keypoints
COUNTS = [(21, 57, 3), (15, 56, 3), (41, 127, 3), (42, 167, 4), (47, 147, 3)]


@pytest.fixture(scope="module")
def emu():
    subprocess.run(["sh", os.path.join(EMU_DIR, "build_emu.sh")], check=True, capture_output=True)
    L = C.CDLL(os.path.join(EMU_DIR, "libsift3d_emu.so"))
    lib = abi.Sift3dLib(L, None, "emulated")
    bind_extensions(L)
    return lib


# ---- the restatement ----------------------------------------------------------------------------------------------------------
def top_n(strength, n):
    """Boolean selection of the n largest strengths, ties to the earlier entry, in list order."""
    strength = np.asarray(strength, np.float32)
    order = np.argsort(-strength, kind="stable")[:n]
    keep = np.zeros(len(strength), bool)
    keep[np.sort(order)] = True
    return keep


def oracle_strengths(oracle, xyzos):
    """|D| of each record's own voxel from the DoG levels the oracle's last detect left."""
    levels = {}
    out = np.zeros(len(xyzos), np.float32)
    for i, (x, y, z, o, s) in enumerate(np.asarray(xyzos, np.int64)):
        if (o, s) not in levels:
            levels[(o, s)] = oracle.level("dog", int(o), int(s))[0]
        out[i] = np.abs(levels[(o, s)][z, y, x])
    return out


# ---- 1: s3d_k_select_strongest against numpy ----------------------------------------------------------------------------------
SELECT_SIZES = [1, 63, 64, 65, 256, 257, 4099]        # (and 70001 on the device: minutes on the emulator)
PATTERNS = ["distinct", "three_values", "all_equal", "low_byte", "exponent", "zeros"]
KEEPS = ["ones", "rand30", "decoys"]


def make_strengths(pattern, num, rng):
    if pattern == "distinct":            # distinct random positives over 64 binades
        return (0x30000000 + rng.choice(1 << 29, num, replace=False).astype(np.uint32)).view(np.float32)
    if pattern == "three_values":
        return rng.choice(np.array([0.25, 0.5, 1.5], np.float32), num)
    if pattern == "all_equal":
        return np.full(num, 0.125, np.float32)
    if pattern == "low_byte":            # differ in the lowest mantissa byte only
        return (0x3DCC0000 | rng.integers(0, 256, num).astype(np.uint32)).view(np.float32)
    if pattern == "exponent":            # differ in the exponent only
        return (rng.integers(1, 255, num).astype(np.uint32) << 23).view(np.float32)
    if pattern == "zeros":               # +0.0 present, and tied
        v = rng.random(num).astype(np.float32)
        v[rng.random(num) < 0.3] = 0.0
        if num > 1:
            v[num // 2] = 0.0
        return v
    raise KeyError(pattern)


def make_keep(name, strength, rng):
    num = len(strength)
    if name == "ones":
        return np.ones(num, np.uint32), strength
    if name == "rand30":
        return (rng.random(num) < 0.3).astype(np.uint32), strength
    if name == "decoys":                 # the entries that are not kept hold the largest strengths: they must be ignored
        keep = (rng.random(num) < 0.75).astype(np.uint32)
        s = strength.copy()
        s[keep == 0] = np.float32(3.0e38)
        return keep, s
    raise KeyError(name)


def check_select(lib, num, pattern, gpu):
    dev = DeviceLib(lib.sift)
    rng = np.random.default_rng(num * 7 + PATTERNS.index(pattern))
    base = make_strengths(pattern, num, rng)
    assert base.dtype == np.float32 and (base >= 0).all() and np.isfinite(base).all()
    nbytes = dev.select_scratch_bytes(num)
    ran = 0
    for kname in KEEPS:
        keep, strength = make_keep(kname, base, rng)
        kidx = np.flatnonzero(keep)
        kept = len(kidx)
        budgets = sorted({b for b in (1, 2, kept // 2, kept - 1, kept, kept + 1, num + 5) if b >= 1})
        for budget in budgets:
            want = np.zeros(num, np.uint32)
            want[kidx[top_n(strength[kidx], budget)]] = 1
            assert int(want.sum()) == min(budget, kept)
            got = keep.copy()
            scratch = np.full(nbytes // 4 + 4, 0xA5A5A5A5, np.uint32)           # dirty: the call clears what it relies on
            arrs = [strength, got, scratch]
            ptr = [dev.upload(a) for a in arrs] if gpu else [a.ctypes.data for a in arrs]
            dev.select_strongest(ptr[0], ptr[1], num, budget, ptr[2])
            dev.sync()
            if gpu:
                got = dev.download(ptr[1], got.shape, np.uint32)
                tail = dev.download(ptr[2] + nbytes, (4,), np.uint32)
                for p in ptr:
                    dev.free(p)
            else:
                tail = scratch[nbytes // 4:]
            assert (tail == 0xA5A5A5A5).all(), "wrote past s3d_k_select_scratch_bytes"
            assert np.array_equal(got, want), (num, pattern, kname, budget, kept)
            ran += 1
    assert ran >= 3 * 3 if num > 2 else ran >= 3


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("num", SELECT_SIZES)
def test_select_strongest_against_numpy(emu, num, pattern):
    check_select(emu, num, pattern, gpu=False)


def check_select_arguments(lib):
    dev = DeviceLib(lib.sift)
    with pytest.raises(RuntimeError):
        dev.select_strongest(None, None, 5, 0, None)            # a budget is positive
    dev.select_strongest(None, None, 0, 3, None)                # nothing to select from: no launch, no access
    assert dev.select_scratch_bytes(0) > 0 and dev.select_scratch_bytes(70001) >= 4 * (1024 + 70001 // 256)


def test_select_strongest_arguments(emu):
    check_select_arguments(emu)


# ---- runs ---------------------------------------------------------------------------------------------------------------------
def set_budget(lib, s, n):
    rc = abi.set_max_keypoints(lib.sift, s, n)
    assert rc == 0, lib.sift.sift3d_amd_last_error()
    assert abi.get_max_keypoints(lib.sift, s) == n


def run(lib, vol, units, n=0, mask=None, params=None, describe=True, levels=True, typed=None):
    """One detect (+ describe) on a fresh struct with budget `n`: M.run's dict plus the library's strengths of the result.
    typed = (q, slope, inter): the typed entry point on `q` instead of the float one on `vol`."""
    s = T.new_sift(lib)
    for k, v in (params or {}).items():
        assert getattr(lib.sift, f"set_{k}_SIFT3D")(C.byref(s), v) == 0
    if mask is not None:
        assert M.set_mask(lib, s, mask) == 0, lib.sift.sift3d_amd_last_error()
    assert abi.get_max_keypoints(lib.sift, s) == 0, "a fresh struct has no budget"
    if n:
        set_budget(lib, s, n)
    kp = T.typed_detect(lib, s, typed[0], units, typed[1], typed[2]) if typed else T.float_detect(lib, s, vol, units)
    xyzos, sd, R = lib.keypoints_to_numpy(kp)
    out = dict(rows=M.record_rows(kp), xyzos=xyzos, sd=sd, R=R, ncand=lib.sift.sift3d_amd_last_num_candidates(C.byref(s)),
               dims=(kp.nx, kp.ny, kp.nz))
    out["strength"] = abi.keypoint_strengths(lib.sift, s, kp) if len(xyzos) else np.zeros(0, np.float32)
    if levels:
        out["gss"] = T.gss_bytes(lib, s)
    if describe:
        out["bins"], out["xyzs"] = M.descriptors(lib, s, kp) if len(xyzos) else (np.zeros((0, 768), np.float32), np.zeros((0, 4)))
    lib.sift.cleanup_Keypoint_store(C.byref(kp))
    lib.sift.cleanup_SIFT3D(C.byref(s))
    return out


def assert_is_filtered(got, base, keep, what=""):
    """`got` (budgeted run) against `base` (unbudgeted run of the same library) restricted to `keep`."""
    assert len(got["rows"]) == int(keep.sum()), f"{what}: {len(got['rows'])} keypoints, the filtered list has {int(keep.sum())}"
    assert got["rows"].tobytes() == base["rows"][keep].tobytes(), f"{what}: keypoint records differ"
    assert got["dims"] == base["dims"] and got["ncand"] == base["ncand"], f"{what}: the candidate count is unaffected"
    assert got["strength"].tobytes() == base["strength"][keep].tobytes(), what
    if "gss" in got and "gss" in base:
        assert got["gss"] == base["gss"], f"{what}: the pyramid differs from the unbudgeted run's"
    if "bins" in got and "bins" in base:
        assert got["bins"].tobytes() == base["bins"][keep].tobytes(), f"{what}: descriptors differ from the unbudgeted run's rows"
        assert np.array_equal(got["xyzs"], base["xyzs"][keep])


_base = {}


def unbudgeted(lib, oracle, i):
    """The unbudgeted run of T.VOLUMES[i] on `lib`, the oracle's list and its strengths (from its own DoG), once per library."""
    key = (lib.name, i)
    if key not in _base:
        dims, units, nblobs, seed, _ = T.VOLUMES[i]
        vol = synth.blobs(*dims, nblobs, seed)
        want = oracle.detect(vol, units)
        ncand = len(oracle.candidates()[0])
        w_strength = oracle_strengths(oracle, want[0])
        _base[key] = (vol, units, run(lib, vol, units), want, w_strength, ncand)
    return _base[key]


# ---- 2: the strength kernel -----------------------------------------------------------------------------------------------------
def check_strengths(lib, oracle, i):
    vol, units, base, (w_xyzos, w_sd, w_R), w_strength, ncand = unbudgeted(lib, oracle, i)
    K, C_, noct = COUNTS[i]
    assert (len(w_xyzos), ncand, len(np.unique(w_xyzos[:, 3]))) == (K, C_, noct), "the oracle's counts moved"
    assert np.array_equal(base["xyzos"], w_xyzos) and base["ncand"] == ncand
    assert base["strength"].dtype == np.float32
    assert base["strength"].tobytes() == w_strength.tobytes(), "strengths differ from |DoG| of the oracle"
    assert len(np.unique(w_strength)) == K and (w_strength > 0).all(), "all strengths are distinct"
    half = top_n(w_strength, K // 2)
    assert len(np.unique(w_xyzos[half, 3])) > 1, "the strongest half is spread over the octaves"
    assert not half[:K // 2].all(), "the strongest half is not a prefix of the list"


@pytest.mark.parametrize("i", range(5))
def test_strengths_are_the_oracles_dog(emu, oracle, i):
    check_strengths(emu, oracle, i)


# ---- 3: budgeted detect == filtered unbudgeted detect -----------------------------------------------------------------------------
def check_volume_budget(lib, oracle, i, which, orient_chunk=0):
    vol, units, base, (w_xyzos, w_sd, w_R), w_strength, ncand = unbudgeted(lib, oracle, i)
    K = COUNTS[i][0]
    assert len(w_xyzos) == K
    n = {"1": 1, "7": 7, "K-1": K - 1, "K": K, "K+5": K + 5}[which]
    if which in ("1", "7", "K-1"):
        assert 0 < n < K, "the case must cut"
    keep = top_n(w_strength, n)
    assert int(keep.sum()) == min(n, K)
    lib.sift.s3d_k_set_orient_chunk.argtypes = [C.c_uint32]
    lib.sift.s3d_k_set_orient_chunk.restype = None
    lib.sift.s3d_k_set_orient_chunk(orient_chunk)
    try:
        got = run(lib, vol, units, n)
    finally:
        lib.sift.s3d_k_set_orient_chunk(0)
    assert_is_filtered(got, base, keep, f"{T.VOLUMES[i][0]} budget {n}")
    assert np.array_equal(got["xyzos"], w_xyzos[keep]) and np.array_equal(got["sd"], w_sd[keep])
    assert np.abs(got["R"] - w_R[keep]).max(initial=0) <= 1e-5          # parity.check_detect_describe's bound
    assert got["strength"].tobytes() == w_strength[keep].tobytes()


BUDGETS = ["1", "7", "K-1", "K", "K+5"]


@pytest.mark.parametrize("which", BUDGETS)
@pytest.mark.parametrize("i", range(5))
def test_budgeted_detect_is_the_filtered_unbudgeted_detect(emu, oracle, i, which):
    check_volume_budget(emu, oracle, i, which)


def test_selection_spans_orientation_chunks(emu, oracle):
    """127 candidates in chunks of 16: the selection is global over all of them."""
    check_volume_budget(emu, oracle, 2, "7", orient_chunk=16)


# ---- 4: with a mask, with typed input -------------------------------------------------------------------------------------------------
def check_mask_plus_budget(lib, oracle, n=5):
    """`ball` on volume 2: the mask removes first, the budget ranks what is left.  Expected: oracle list -> mask -> top n."""
    i = 2
    vol, units, base, (w_xyzos, w_sd, w_R), w_strength, _ = unbudgeted(lib, oracle, i)
    mask = M.make_mask("ball", vol.shape)
    inside = M.kept(w_xyzos, mask)
    assert int(inside.sum()) == M.COUNTS[i][1 + M.MASK_NAMES.index("ball")] and 0 < n < int(inside.sum())
    keep = np.zeros(len(w_xyzos), bool)
    keep[np.flatnonzero(inside)[top_n(w_strength[inside], n)]] = True
    assert not np.array_equal(keep, top_n(w_strength, n)), "the mask must change which n survive"
    got = run(lib, vol, units, n, mask=mask)
    masked = run(lib, vol, units, 0, mask=mask, describe=False, levels=False)
    assert got["ncand"] == masked["ncand"] < base["ncand"]
    got_cmp = dict(got, ncand=base["ncand"])
    assert_is_filtered(got_cmp, base, keep, "ball + budget")
    assert np.array_equal(got["xyzos"], w_xyzos[keep]) and np.array_equal(got["sd"], w_sd[keep])
    assert np.abs(got["R"] - w_R[keep]).max(initial=0) <= 1e-5


def test_mask_then_budget(emu, oracle):
    check_mask_plus_budget(emu, oracle)


def check_typed_plus_budget(lib, n=9):
    """An int16 volume on the fused route: the budgeted typed detect is the budgeted float detect."""
    dims, units, nblobs, seed, fused = T.VOLUMES[2]
    q = T.quantise(synth.blobs(*dims, nblobs, seed), np.int16)
    slope, inter = 0.01171875, -7.25
    assert fused and T.route_is_fused(lib, q, units)
    vol = T.converted(q, slope, inter)
    base = run(lib, vol, units, describe=False)
    K = len(base["rows"])
    assert 0 < n < K
    want = run(lib, vol, units, n, describe=False)
    got = run(lib, vol, units, n, describe=False, typed=(q, slope, inter))
    assert len(want["rows"]) == n and got["rows"].tobytes() == want["rows"].tobytes()
    assert got["gss"] == want["gss"] == base["gss"]
    assert got["strength"].tobytes() == want["strength"].tobytes()


def test_typed_input_plus_budget(emu):
    check_typed_plus_budget(emu)


# ---- 5: non-finite volumes ------------------------------------------------------------------------------------------------------
NONFINITE = ("iso72", "nan_far_edge", 31, 10)


def check_nonfinite_budget(lib, oracle, base, name, total, n):
    """The verbatim pass: the budgeted result is the golden list filtered by the oracle's DoG of the same volume."""
    want, g = parity.nonfinite_golden()
    edits = next(e for b, nm, e in parity.NONFINITE_CASES if (b, nm) == (base, name))
    vol, units, params = parity.nonfinite_input_checked(g, base, name, edits)
    w = want[(base, name)]
    assert w is not None and len(w[0]) == total and 0 < n < total
    o = parity.oracle_detect_describe_or_fail(oracle, vol, units, params)
    assert o is not None and np.array_equal(o[0], w[0]), "the oracle's list is the golden list"
    w_strength = oracle_strengths(oracle, w[0])
    assert np.isfinite(w_strength).all() and len(np.unique(w_strength)) == total
    keep = top_n(w_strength, n)
    assert not keep[:n].all()
    s = T.new_sift(lib)
    for k, v in (params or {}).items():
        assert getattr(lib.sift, f"set_{k}_SIFT3D")(C.byref(s), v) == 0
    set_budget(lib, s, n)
    kp = T.float_detect(lib, s, vol, units)
    xyzos, sd, R = lib.keypoints_to_numpy(kp)
    bins = M.descriptors(lib, s, kp)[0].copy()
    strength = abi.keypoint_strengths(lib.sift, s, kp)
    lib.sift.cleanup_Keypoint_store(C.byref(kp))
    lib.sift.cleanup_SIFT3D(C.byref(s))
    assert parity.assert_same_nonfinite_result((xyzos, sd, R, bins), tuple(a[keep] for a in w), f"{base}/{name} budget {n}") == n
    assert strength.tobytes() == w_strength[keep].tobytes()


def test_nonfinite_volume_with_a_budget(emu, oracle):
    check_nonfinite_budget(emu, oracle, *NONFINITE)


# ---- 6: lifecycle ----------------------------------------------------------------------------------------------------------------
def check_lifecycle(lib):
    L = lib.sift
    vol = synth.blobs(48, 48, 48, 120, 0)
    base = run(lib, vol, UNIT, levels=False, describe=False)
    K = len(base["rows"])
    assert K > 8
    keep5 = top_n(base["strength"], 5)                    # (the library's own strengths: checked against the oracle above)

    def detect(s, v=vol):
        kp = T.float_detect(lib, s, v, UNIT)
        rows = M.record_rows(kp)
        return rows, kp

    s = T.new_sift(lib)
    assert abi.get_max_keypoints(L, s) == 0
    # strengths before any detect: a message, not a crash
    kp0 = T.new_kp(lib)
    with pytest.raises(RuntimeError, match="pyramid"):
        abi.keypoint_strengths(L, s, kp0)
    L.cleanup_Keypoint_store(C.byref(kp0))
    # 0 on a struct that has never had a budget
    assert abi.set_max_keypoints(L, s, 0) == 0 and abi.get_max_keypoints(L, s) == 0
    set_budget(lib, s, 5)
    # a negative budget fails and keeps the old value
    assert abi.set_max_keypoints(L, s, -1) != 0 and b"budget" in L.sift3d_amd_last_error()
    assert abi.get_max_keypoints(L, s) == 5
    for _ in range(2):                                    # it stays in force
        rows, kp = detect(s)
        assert rows.tobytes() == base["rows"][keep5].tobytes()
        L.cleanup_Keypoint_store(C.byref(kp))
    # copy_SIFT3D carries it, as a copy
    L.copy_SIFT3D.argtypes = [P(abi.SIFT3D), P(abi.SIFT3D)]
    s2 = T.new_sift(lib)
    assert L.copy_SIFT3D(C.byref(s), C.byref(s2)) == 0 and abi.get_max_keypoints(L, s2) == 5
    rows, kp = detect(s2)
    assert rows.tobytes() == base["rows"][keep5].tobytes()
    L.cleanup_Keypoint_store(C.byref(kp))
    assert abi.set_max_keypoints(L, s2, 0) == 0 and abi.get_max_keypoints(L, s) == 5
    L.cleanup_SIFT3D(C.byref(s2))
    # the struct is reused across dimensions, the budget grows and shrinks
    other = synth.blobs(40, 48, 48, 100, 1)
    obase = run(lib, other, UNIT, levels=False, describe=False)
    assert len(obase["rows"]) > 5
    rows, kp = detect(s, other)
    assert rows.tobytes() == obase["rows"][top_n(obase["strength"], 5)].tobytes()
    L.cleanup_Keypoint_store(C.byref(kp))
    set_budget(lib, s, 2)
    rows, kp = detect(s)
    assert rows.tobytes() == base["rows"][top_n(base["strength"], 2)].tobytes()
    # an out-of-range record: a message
    kp.buf[1].xd = 1.0e6
    with pytest.raises(RuntimeError, match="keypoint"):
        abi.keypoint_strengths(L, s, kp)
    kp.buf[1].xd, kp.buf[1].s = 3.0, s.gpyr.first_level + s.gpyr.num_levels - 1          # no DoG level there
    with pytest.raises(RuntimeError, match="outside its DoG level"):
        abi.keypoint_strengths(L, s, kp)
    L.cleanup_Keypoint_store(C.byref(kp))
    # 0 restores the full list on the same struct
    set_budget(lib, s, 0)
    rows, kp = detect(s)
    assert rows.tobytes() == base["rows"].tobytes()
    assert abi.keypoint_strengths(L, s, kp).tobytes() == base["strength"].tobytes()
    L.cleanup_Keypoint_store(C.byref(kp))
    # a budget no list reaches
    set_budget(lib, s, 1 << 40)
    rows, kp = detect(s)
    assert rows.tobytes() == base["rows"].tobytes()
    L.cleanup_Keypoint_store(C.byref(kp))
    L.cleanup_SIFT3D(C.byref(s))


def test_lifecycle(emu):
    check_lifecycle(emu)


# ---- 7: several ranks ------------------------------------------------------------------------------------------------------------
def check_loopback_ranks(lib, ranks=2):
    """Two loop-back Z-slab ranks and a budget: the detect fails and says why; without the budget the same struct detects."""
    L = lib.sift
    L.sift3d_amd_set_num_gpus.argtypes = [P(abi.SIFT3D), C.c_int, C.c_int]
    dims, units, nblobs, seed, params = parity.NONFINITE_BASES["slab64"]
    vol = synth.blobs(*dims, nblobs, seed)
    base = run(lib, vol, units, params=params, levels=False, describe=False)
    assert len(base["rows"]) > 3
    s = T.new_sift(lib)
    for k, v in params.items():
        assert getattr(L, f"set_{k}_SIFT3D")(C.byref(s), v) == 0
    assert L.sift3d_amd_set_num_gpus(C.byref(s), ranks, 1) == 0                # 1 = SIFT3D_AMD_SLAB_LOOPBACK
    set_budget(lib, s, 3)
    im = lib.image_from_numpy(vol, units)
    kp = T.new_kp(lib)
    assert L.SIFT3D_detect_keypoints(C.byref(s), C.byref(im), C.byref(kp)) == -1
    msg = L.sift3d_amd_last_error().decode()
    assert "budget" in msg and "several GPUs" in msg, msg
    set_budget(lib, s, 0)
    assert L.SIFT3D_detect_keypoints(C.byref(s), C.byref(im), C.byref(kp)) == 0
    assert M.record_rows(kp).tobytes() == base["rows"].tobytes()
    with pytest.raises(RuntimeError, match="several GPUs"):
        abi.keypoint_strengths(L, s, kp)
    lib.free_image(im)
    L.cleanup_Keypoint_store(C.byref(kp))
    L.cleanup_SIFT3D(C.byref(s))


def test_two_loopback_ranks_refuse_a_budget(emu, monkeypatch):
    monkeypatch.setenv("S3D_EMU_DEVICES", "2")
    check_loopback_ranks(emu)


# ---- 8: kpSift3D --max_keypoints ---------------------------------------------------------------------------------------------------
def check_cli(tmp_path, env, oracle, dims, nblobs, seed, n=9):
    prog = os.path.join(ROOT, "sift3d_amd", "bin", "kpSift3D")
    if not os.path.exists(prog):
        from sift3d_amd import build as _b
        _b.build()
    nx, ny, nz = dims
    vol = synth.blobs(nx, ny, nz, nblobs, seed)
    src = str(tmp_path / "vol.nii.gz")
    with gzip.open(src, "wb") as f:
        f.write(nifti1_bytes(np.ascontiguousarray(vol.transpose(2, 1, 0)), UNIT))
    e = None if env is None else dict(os.environ, **env)

    def kp_run(*args):
        return subprocess.run([prog, "--peak_thresh", "0.08", *args, src], capture_output=True, text=True, timeout=600, env=e)

    def rows(path):
        return [line.split(",") for line in open(path).read().splitlines()]

    oracle.set_params(peak=0.08)
    try:
        w_xyzos = oracle.detect(vol, UNIT)[0]
        w_strength = oracle_strengths(oracle, w_xyzos)
    finally:
        oracle.set_params()
    plain, cut = str(tmp_path / "k0.csv"), str(tmp_path / "k1.csv")
    r = kp_run("--keys", plain)
    assert r.returncode == 0, r.stderr
    r = kp_run("--max_keypoints", str(n), "--keys", cut)
    assert r.returncode == 0, r.stderr
    all_rows, got = rows(plain), rows(cut)
    xyzo = np.array([[float(v) for v in r_[:4]] for r_ in all_rows]).astype(np.int64)
    assert np.array_equal(xyzo, w_xyzos[:, :4]) and 0 < n < len(all_rows)
    keep = top_n(w_strength, n)
    assert len(got) == n and got == [r_ for r_, k in zip(all_rows, keep) if k]
    r = kp_run("--max_keypoints", "0", "--keys", cut)
    assert r.returncode == 0 and rows(cut) == all_rows
    for bad in ("x", "-3", "7x", ""):
        r = kp_run("--max_keypoints", bad, "--keys", cut)
        assert r.returncode == 1 and 'Use "kpSift3D --help" for more information.' in r.stderr, (bad, r.stderr)
    r = subprocess.run([prog, "--help"], capture_output=True, text=True, timeout=60)
    assert r.stdout.startswith("Usage: kpSift3D [image.nii]") and " --max_keypoints [N] " in r.stdout


def test_kpSift3D_max_keypoints_emulated(emu, oracle, tmp_path):
    check_cli(tmp_path, {"LD_PRELOAD": os.path.join(EMU_DIR, "libsift3d_emu.so")}, oracle, (40, 36, 32), 120, 3)      # 13 keypoints
