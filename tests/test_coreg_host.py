"""CPU: the host half of the co-registration of two intensity images (include/unet_coreg.h, unet-studio_amd/coreg.py) -- the ABI the
library exports, the integer logarithm against the real one, argument errors found before any device call, the restatements of
tests/coreg_ref.py on hand-written answers, and the quality of the definition: the numpy search on the phantom.  No device calls."""
import ctypes
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

import unet_studio_amd as U
from unet_studio_amd import coreg as CR

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import coreg_ref as ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDENTITY = ref.IDENTITY


def vol(v):
    return np.array(v).reshape(1, 1, -1)


def shift(tx, ty=0, tz=0):
    return [1, 0, 0, 0, 1, 0, 0, 0, 1, tx, ty, tz]


# ---- the ABI -------------------------------------------------------------------------------------------------------------------------
def test_unet_coreg_h_declares_exactly_the_exports_and_the_library_exports_exactly_them():
    hdr = open(os.path.join(ROOT, "include", "unet_coreg.h")).read()
    body = hdr[hdr.index("#ifndef UNET_COREG_H"):]
    declared = set(re.findall(r"\b(unet_[a-z0-9_]+)\s*\(", body))
    assert declared == set(CR.EXPORTS) == {"unet_coreg_scratch_bytes", "unet_coreg_code", "unet_coreg_hist", "unet_coreg_score",
                                           "unet_coreg_search"}
    assert len(CR.EXPORTS) == len(set(CR.EXPORTS))
    lib = ctypes.CDLL(U.engine.LIB_PATH)
    for name in sorted(declared):
        assert hasattr(lib, name), "libunet_hip.so does not export " + name
    # every name with the prefix that the library's file holds (its dynamic symbols, and its messages, which name them) is declared
    in_file = set(m.decode() for m in re.findall(rb"unet_coreg_[a-z0-9_]+", open(U.engine.LIB_PATH, "rb").read()))
    assert in_file == declared, in_file ^ declared
    enums = {k: int(v) for k, v in re.findall(r"UNET_COREG_([A-Z_]+) = (\d+)", hdr)}
    assert enums == {"IMPL_DEFAULT": CR.IMPL_DEFAULT, "IMPL_LDS": CR.IMPL_LDS, "IMPL_GLOBAL": CR.IMPL_GLOBAL}
    assert (CR.IMPL_DEFAULT, CR.IMPL_LDS, CR.IMPL_GLOBAL) == (0, 1, 2)
    limits = {k: int(v) for k, v in re.findall(r"#define UNET_COREG_MAX_([A-Z]+) (\d+)", hdr)}
    assert limits == {"BINS": CR.MAX_BINS, "MAPS": CR.MAX_MAPS, "STAGES": CR.MAX_STAGES, "LEVEL": CR.MAX_LEVEL,
                      "ITERATIONS": CR.MAX_ITERATIONS}
    assert CR.MAX_MAPS == 1 + 2 * 12 and CR.BINS == (8, 16, 32) and CR.MAX_BINS == max(CR.BINS)
    assert U.coreg is CR
    assert CR.DEFAULT_STEP == ref.PHANTOM_STEP and [tuple(s) for s in CR.DEFAULT_STAGES] == ref.PHANTOM_STAGES


def test_the_other_headers_do_not_mention_the_new_prefix_and_this_one_mentions_no_other():
    for h in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if h != "unet_coreg.h":
            assert "unet_coreg" not in open(os.path.join(ROOT, "include", h)).read().lower(), h
    mine = open(os.path.join(ROOT, "include", "unet_coreg.h")).read().lower()
    for p in ("reg", "stats", "space", "atlas", "components", "preproc", "conn", "calib", "recal", "inst", "tiles", "dist", "mirror", "table",
              "ens", "morph"):                                     # what the other host tests forbid
        assert "unet_%s_" % p not in mine, p


# ---- the integer logarithm -----------------------------------------------------------------------------------------------------------
def test_the_integer_log_is_a_truncated_fixed_point_log2():
    assert ref.ilog(0) == 0 and ref.ilog(1) == 0 and ref.ilog(2) == 65536 and ref.ilog(1 << 30) == 30 << 16
    assert ref.ilog(3) == 103872 and ref.ilog((1 << 31) - 1) == 2031615
    ns = list(range(1, 65536)) + [(1 << k) + d for k in range(16, 31) for d in (-1, 0, 1)]
    got = ref.ilog_np(np.array(ns))
    worst = 0.0
    for n, v in zip(ns, got.tolist()):
        err = 65536 * math.log2(n) - v
        worst = max(worst, abs(err))
        assert -0.01 <= err <= 1.01, (n, v, err)                  # truncated: never above the real value, within 1.01 below it
    print("largest |65536 log2(n) - L(n)| = %.6f over %d values" % (worst, len(ns)))
    # the vectorised form used by the search is the Python-integer form
    some = [0, 1, 2, 3, 5, 7, 255, 256, 65535, 65536, 65537, 123456789, (1 << 31) - 1, 1 << 31, (1 << 32) - 1]
    assert [ref.ilog(v) for v in some + ns[::97]] == ref.ilog_np(np.array(some + ns[::97], np.uint64)).tolist()
    assert all(ref.ilog(a) <= ref.ilog(a + 1) for a in range(1, 5000))


# ---- the restatements on hand-written answers ----------------------------------------------------------------------------------------
def test_code_ref_on_the_edges_of_the_range():
    inf, nan = float("inf"), float("nan")
    v = np.array([0.0, -0.0, 1.0, 0.999, -1e-6, 0.0625, 0.124, 0.125, 0.875, 0.874, 2.0, inf, -inf, nan, 0.5], np.float32)
    assert ref.code_ref(v, 0, 1, 8).tolist() == [0, 0, 7, 7, 0, 0, 0, 1, 7, 6, 7, 7, 0, 8, 4]
    assert ref.code_ref(v, 0, 1, 8).dtype == np.uint8
    # the last bin takes everything from t = bins - 1 on: hi itself and beyond
    assert ref.code_ref(np.array([3.0, 2.99, 1.0, 0.99, 2.0, 1.99], np.float32), 1, 3, 16).tolist() == [15, 15, 0, 0, 8, 7]
    assert ref.code_ref(np.array([nan, 5.0], np.float32), -1, 1, 32).tolist() == [32, 31]


def test_hist_ref_counts_outside_and_none_in_the_last_column_and_skips_a_fixed_none():
    fixed, moving = vol([1, 1, 1, 8, 2]), vol([3, 8, 5])
    h = ref.hist_ref(fixed, moving, 8, [IDENTITY])[0]
    assert h.shape == (8, 9) and h.dtype == np.uint32
    # x = 0 reads 3; x = 1 reads the moving none -> column 8; x = 2 reads 5; x = 3 is a fixed none: skipped; x = 4 is outside -> column 8
    want = np.zeros((8, 9), np.int64)
    want[1, 3] = want[1, 8] = want[1, 5] = want[2, 8] = 1
    assert h.tolist() == want.tolist() and int(h.sum()) == ref.counted_kept(fixed, 8, 1) == 4
    # a value above bins reads as none on both sides
    assert ref.hist_ref(vol([200, 1]), vol([0, 99]), 8, [IDENTITY])[0][1].tolist() == [0] * 8 + [1]
    # x -> x - 0.5: voxel 0 sits at -0.5 (q = 0, inside, index 0); x -> x + 2.5: everything outside; a NaN entry: everything outside
    assert ref.hist_ref(vol([1, 1]), vol([2, 4]), 8, [shift(-0.5)])[0][1].tolist() == [0, 0, 1, 0, 1, 0, 0, 0, 0]
    nan_map = list(IDENTITY)
    nan_map[1] = float("nan")
    both = ref.hist_ref(vol([1, 1]), vol([2, 4]), 8, [shift(2.5), nan_map])
    assert both.shape == (2, 8, 9) and both[0][1].tolist() == both[1][1].tolist() == [0] * 8 + [2]
    # the stride rule: every histogram of one call has the same total
    f = np.arange(4 * 5 * 6).reshape(4, 5, 6) % 9
    totals = ref.hist_ref(f, f, 8, [IDENTITY, shift(3, 1, 1), nan_map], 2).sum((1, 2)).tolist()
    assert totals == [ref.counted_kept(f, 8, 2)] * 3 and totals[0] < 2 * 3 * 3 + 1


def test_score_ref_on_hand_worked_tables():
    def table(bins, cells):
        h = np.zeros((bins, bins + 1), np.int64)
        for (a, b), n in cells.items():
            h[a, b] = n
        return h
    # one cell: n (L(n) + L(n) - L(n) - L(n)) = 0; an empty table: 0
    assert ref.score_py(table(8, {(2, 3): 1000})) == 0 and ref.score_py(table(8, {})) == 0
    # a diagonal of four cells of 4: N = 16, each term 4 (L(4) + L(16) - L(4) - L(4)) = 4 * 2 * 65536: 16 voxels x 2 bits
    diag = table(8, {(i, i): 4 for i in range(4)})
    assert ref.score_py(diag) == 16 * 2 * 65536
    # independent: a uniform table has no information
    assert ref.score_py(np.concatenate([np.full((8, 8), 2), np.zeros((8, 1), np.int64)], 1)) == 0
    # everything outside: N and the rows count it, no term
    assert ref.score_py(table(8, {(i, 8): 5 for i in range(8)})) == 0
    # half outside: the outside column lowers the score of what stays (4 (L(4) + L(32) - L(8) - L(4)) per cell, 2 bits each)
    half = table(8, {(i, i): 4 for i in range(4)})
    half[:4, 8] = 4
    assert ref.score_py(half) == 16 * 2 * 65536 < ref.score_py(2 * diag) == 32 * 2 * 65536
    # the vectorised form is the Python-integer form
    rng = np.random.default_rng(3)
    for bins in (8, 16, 32):
        for _ in range(3):
            h = rng.integers(0, 50, (bins, bins + 1))
            assert ref.score_py(h) == ref.score_ref(h)
    assert ref.score_ref(table(8, {(0, 0): (1 << 31) - 1})) == 0


def test_search_ref_follows_the_state_machine_of_the_header():
    fixed, moving = vol([1, 1, 2, 2, 3, 3]), vol([0, 1, 1, 2, 2, 3, 3, 0])
    x_only = [0] * 9 + [1, 0, 0]
    m, trace, info = ref.search_ref(fixed, moving, 8, IDENTITY, x_only, [(1, 0, 1)], 10)
    # at 0 the pairs straddle: six cells of one voxel.  +1 lines them up: three cells of two, 2 (L(2) + L(6) - L(2) - L(2)) each; -1
    # sends a voxel outside.  At 1 nothing is better at level 0; at level 1, -0.5 samples the same voxels: a tie, candidate 0 stays
    best = 6 * (ref.ilog(6) - ref.ilog(2))
    assert trace[:3].tolist() == [[0, 0, 1, best], [0, 0, 0, best], [0, 1, 0, best]] and m.tolist() == shift(1)
    assert info.tolist() == [3, 1, best, 0] and best == ref.score_py(ref.hist_ref(fixed, moving, 8, [shift(1)])[0])
    assert ref.score_py(ref.hist_ref(fixed, moving, 8, [shift(1), shift(0.5)])[1]) == best
    n = int(info[0])
    assert (trace[n:] == -1).all() and trace.dtype == np.int64 and m.dtype == np.float32
    # the last stage finished on the last iteration allowed: converged; one fewer: not, and the untouched rows hold -1
    assert ref.search_ref(fixed, moving, 8, IDENTITY, x_only, [(1, 0, 1)], n)[2].tolist()[:2] == [n, 1]
    cut = ref.search_ref(fixed, moving, 8, IDENTITY, x_only, [(1, 0, 1)], n - 1)
    assert cut[2].tolist()[:2] == [n - 1, 0]
    one = ref.search_ref(fixed, moving, 8, IDENTITY, x_only, [(1, 0, 1)], 1)
    assert one[2].tolist()[:2] == [1, 0] and one[0].tolist() == shift(1) and one[1].shape == (1, 4)
    # a frozen parameter produces no candidates: K = 1 + 2 P
    c = ref.state_of(IDENTITY, (np.float32(1), np.float32(2), np.float32(3)))
    assert len(ref.candidates_ref(c, ref.PHANTOM_STEP, 0)) == 25 and len(ref.candidates_ref(c, x_only, 0)) == 3
    assert len(ref.candidates_ref(c, [0] * 9 + [4] * 3, 2)) == 7
    assert c[9:].tolist() == [1, 2, 3] and ref.map_of(c, (np.float32(1), np.float32(2), np.float32(3))).tolist() == IDENTITY


# ---- the quality of the definition ----------------------------------------------------------------------------------------------------------
def test_the_numpy_search_aligns_the_phantom():
    """Measured on the restatement at 32^3: 16 bins, the 1 % and 99 % quantiles as the range, step [0.08] * 9 + [4] * 3, stages
    [(2, 0, 3), (1, 1, 6)], from the identity.  The search must converge within 400 iterations, the largest displacement error over
    the eight grid corners must be at most 1.0 voxel, and the score at the map found at least that at the identity.  Measured: 68
    iterations, 0.30 voxel against 3.98 at the identity."""
    n = 32
    fixed, moving = ref.phantom_codes(n, 16)
    assert fixed.shape == moving.shape == (n, n, n) and fixed.dtype == np.uint8 and int(fixed.max()) == 15 and int(moving.max()) == 15
    m, trace, info = ref.phantom_search(n, 16)
    truth = ref.true_map(n)
    err, err0 = ref.corner_error(m, truth, (n, n, n)), ref.corner_error(IDENTITY, truth, (n, n, n))
    h = ref.hist_ref(fixed, moving, 16, [m, IDENTITY])
    found, start = ref.score_ref(h[0]), ref.score_ref(h[1])
    print("phantom: %d iterations, converged %d, corner error %.3f voxel (identity %.3f), score %d (identity %d)"
          % (info[0], info[1], err, err0, found, start))
    assert info[1] == 1 and info[0] <= 400 and info[3] == 1
    assert err <= 1.0
    assert found >= start and found == int(info[2])
    assert err0 > 3.0                                              # the phantom is misaligned to begin with
    assert int(h[0].sum()) == int(h[1].sum()) == n ** 3           # every candidate counts the same voxels


# ---- argument errors, before any device call -------------------------------------------------------------------------------------
def test_scratch_bytes_is_monotone_and_checks_its_arguments():
    by_bins = [CR.coreg_scratch_bytes(1000, b, 10) for b in (8, 16, 32)]
    assert by_bins[0] < by_bins[1] < by_bins[2] and by_bins[2] >= 25 * 32 * 33 * 4              # the counters of 25 candidates
    assert len({CR.coreg_scratch_bytes(v, 16, n) for v in (1, 10 ** 6, (1 << 31) - 1) for n in (1, 400, 1024)}) == 1
    for v, b, n, msg in ((0, 16, 1, "fixed_voxels"), (1 << 31, 16, 1, "fixed_voxels"), (10, 4, 1, "bins"), (10, 64, 1, "bins"),
                         (10, 12, 1, "bins must be 8, 16 or 32, got 12"), (10, 16, 0, "max_iterations"), (10, 16, 1025, "max_iterations")):
        with pytest.raises(U.UNetError, match=msg):
            CR.coreg_scratch_bytes(v, b, n)
    rc = U.engine.lib.unet_coreg_scratch_bytes(10, 16, 1, None)
    assert rc != 0 and "null output" in U.engine.lib.unet_last_error().decode()


P = [ctypes.c_void_p(0x1000 * (i + 1)) for i in range(8)]          # never dereferenced
F12 = (ctypes.c_float * 12)(*IDENTITY)


def grids_errors(call):
    assert "null fixed" in call(fixed=None) and "null moving" in call(moving=None)
    assert "fixed dimensions" in call(f=(0, 4, 4)) and "fixed dimensions" in call(f=(4, 4, -1))
    assert "moving dimensions" in call(m=(4, 0, 4))
    assert "fixed grid" in call(f=(2048, 1024, 1024)) and "moving grid" in call(m=(2048, 1024, 1024))
    assert "bins must be 8, 16 or 32, got 15" in call(bins=15) and "bins" in call(bins=0) and "bins" in call(bins=64)


def test_code_argument_errors_need_no_device():
    lib = U.engine.lib

    def call(image=P[0], voxels=64, lo=0.0, hi=1.0, bins=16, codes=P[1]):
        rc = lib.unet_coreg_code(image, voxels, lo, hi, bins, codes, None)
        assert rc != 0
        return lib.unet_last_error().decode()

    assert "null image" in call(image=None) and "image must be 4-byte aligned" in call(image=ctypes.c_void_p(0x1002))
    assert "null codes" in call(codes=None)
    assert "voxels" in call(voxels=0) and "voxels" in call(voxels=1 << 31)
    assert "lo and hi must be finite" in call(lo=float("nan")) and "finite" in call(hi=float("inf")) and "finite" in call(lo=float("-inf"))
    assert "lo must be below hi" in call(lo=1.0, hi=1.0) and "lo must be below hi" in call(lo=2.0, hi=1.0)
    assert "scale" in call(lo=-3e38, hi=3e38) and "scale" in call(lo=0.0, hi=1e-44)
    assert "bins must be 8, 16 or 32, got 7" in call(bins=7)


def test_hist_argument_errors_need_no_device():
    lib = U.engine.lib
    maps = (ctypes.c_float * 300)()

    def call(fixed=P[0], f=(4, 4, 4), moving=P[1], m=(4, 4, 4), bins=16, maps=maps, K=25, stride=1, hist=P[2], impl=0):
        rc = lib.unet_coreg_hist(fixed, *f, moving, *m, bins, maps, K, stride, hist, impl, None, 0, None)
        assert rc != 0
        return lib.unet_last_error().decode()

    grids_errors(call)
    assert "null maps" in call(maps=None) and "null hist" in call(hist=None)
    assert "K must be in [1, 25], got 0" in call(K=0) and "K must be" in call(K=26)
    assert "stride must be 1, 2, 4 or 8, got 3" in call(stride=3) and "stride" in call(stride=0) and "stride" in call(stride=16)
    assert "hist must be 4-byte aligned" in call(hist=ctypes.c_void_p(0x3002))
    assert "unknown impl 3" in call(impl=3) and "unknown impl -1" in call(impl=-1)


def test_score_argument_errors_need_no_device():
    lib = U.engine.lib

    def call(hist=P[0], K=25, bins=16, scores=P[1]):
        rc = lib.unet_coreg_score(hist, K, bins, scores, None)
        assert rc != 0
        return lib.unet_last_error().decode()

    assert "null hist" in call(hist=None) and "null scores" in call(scores=None)
    assert "hist must be 4-byte aligned" in call(hist=ctypes.c_void_p(0x3002))
    assert "scores must be 8-byte aligned" in call(scores=ctypes.c_void_p(0x3004))
    assert "K must be in [1, 25], got 0" in call(K=0) and "K must be" in call(K=26)
    assert "bins must be 8, 16 or 32, got 9" in call(bins=9)


def test_search_argument_errors_need_no_device():
    lib = U.engine.lib
    step = (ctypes.c_float * 12)(*ref.PHANTOM_STEP)
    stages = (ctypes.c_int * 9)(4, 0, 2, 2, 1, 4, 1, 2, 6)

    def floats(v):
        return (ctypes.c_float * 12)(*v)

    def ints(v):
        return (ctypes.c_int * len(v))(*v)

    def call(fixed=P[0], f=(4, 4, 4), moving=P[1], m=(4, 4, 4), bins=16, init=F12, step=step, stages=stages, n_stages=3, n_it=10,
             map_out=P[2], trace=P[3], info=P[4], impl=0, scratch=P[5], scratch_bytes=1 << 40):
        rc = lib.unet_coreg_search(fixed, *f, moving, *m, bins, init, step, stages, n_stages, n_it, map_out, trace, info, impl, scratch,
                                   scratch_bytes, None)
        assert rc != 0
        return lib.unet_last_error().decode()

    grids_errors(call)
    assert "null init" in call(init=None) and "null step" in call(step=None) and "null stages" in call(stages=None)
    assert "step[3] must be finite and >= 0" in call(step=floats([1, 1, 1, -1] + [0] * 8))
    assert "step[11]" in call(step=floats([0] * 11 + [float("inf")])) and "step[0]" in call(step=floats([float("nan")] + [0] * 11))
    assert "at least one step" in call(step=floats([0] * 12))
    assert "n_stages must be in [1, 4], got 0" in call(n_stages=0) and "n_stages" in call(n_stages=5)
    assert "stage 1: stride must be 1, 2, 4 or 8, got 3" in call(stages=ints([4, 0, 2, 3, 1, 4, 1, 2, 6]))
    assert "stage 0: levels" in call(stages=ints([4, -1, 2]), n_stages=1) and "stage 0: levels" in call(stages=ints([4, 3, 2]), n_stages=1)
    assert "stage 2: levels" in call(stages=ints([4, 0, 2, 2, 1, 4, 1, 2, 21]))
    assert "max_iterations" in call(n_it=0) and "max_iterations" in call(n_it=1025)
    assert "null map_out" in call(map_out=None) and "null info" in call(info=None)
    assert "map_out must be 4-byte aligned" in call(map_out=ctypes.c_void_p(0x3001))
    assert "trace must be 8-byte aligned" in call(trace=ctypes.c_void_p(0x4004)) and "info must be 8-byte aligned" in call(info=ctypes.c_void_p(0x5004))
    assert "unknown impl 3" in call(impl=3)
    assert "null scratch" in call(scratch=None)
    assert "scratch too small" in call(scratch_bytes=CR.coreg_scratch_bytes(64, 16, 10) - 1)
    assert "scratch too small" in call(bins=32, scratch_bytes=CR.coreg_scratch_bytes(64, 16, 10))


def test_wrapper_errors_need_no_device():
    c8, f32 = torch.zeros((2, 2, 2), dtype=torch.uint8), torch.zeros((2, 2, 2), dtype=torch.float32)
    h = torch.zeros((1, 8, 9), dtype=torch.int32)
    with pytest.raises(U.UNetError, match="device tensor"):
        CR.code(f32, 0, 1)
    with pytest.raises(U.UNetError, match="device tensor"):
        CR.joint_hist(c8, c8, 16, [IDENTITY])
    with pytest.raises(U.UNetError, match="device tensor"):
        CR.scores(h)
    with pytest.raises(U.UNetError, match="device tensor"):
        CR.search(c8, c8, 16, IDENTITY)
    with pytest.raises(U.UNetError, match="device tensor"):
        CR.align(f32, (1, 1, 1), f32, (1, 1, 1))
    with pytest.raises(U.UNetError):
        CR.robust_range(f32)
    with pytest.raises(U.UNetError, match="permille"):
        CR.robust_range(f32, permille=(10,))
