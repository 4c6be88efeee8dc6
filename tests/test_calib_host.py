"""CPU: the host half of the calibration tables (include/unet_calib.h, unet-studio_amd/calib.py) -- this file's own restatement of the
header's definitions (`code`, `bin_of`, `key`, `calib_ref`: plain numpy, integer-only once the three codings are applied to float32
values, importing nothing of the package's kernels) checked on hand-written answers, every host formula on hand-written tables, the
bracket of the negative log-likelihood on random probabilities, the ABI the library exports, argument errors found before any
device call and the refusals of qc.calibration_qc.  No device calls."""
import ctypes
import math
import os
import re
import types

import numpy as np
import pytest
import torch

import unet_studio_amd as U
from unet_studio_amd import calib as CB
from unet_studio_amd import qc as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
NAN, INF = float("nan"), float("inf")


# ---- the restatement -------------------------------------------------------------------------------------------------------------
def code(p):
    """int64 codes of fp32 probabilities that are not NaN: u = p * 65536 in fp32 (exact), 0 below 0, 65535 from 65535.0 on,
    otherwise truncated"""
    p = np.asarray(p, F)
    assert not np.isnan(p).any()
    with np.errstate(over="ignore"):
        u = p * F(65536.0)
    assert u.dtype == F
    inside = (u >= F(0)) & (u < F(65535.0))
    return np.where(u < F(0), 0, np.where(inside, np.where(inside, u, F(0)).astype(np.int64), 65535)).astype(np.int64)


def bin_of(q):
    return (np.asarray(q, np.int64) * 20) >> 16


def key(p):
    """int64: 0 for p <= 0, 4064 for p >= 1, otherwise the float's bits >> 18"""
    p = np.ascontiguousarray(np.asarray(p, F))
    bits = p.view(np.uint32).astype(np.int64)
    return np.where(p <= F(0), 0, np.where(p >= F(1), 4064, bits >> 18)).astype(np.int64)


def table_len(C):
    return 4 + 20 * 3 + C * 20 * 5 + 4065


def calib_ref(planes, label, mask=None, bad=None):
    """-> (int64 table {table_len(C)}, uint8 wrong {S}) of fp32 probability planes {C, S}, an fp32 label {S} and an optional uint8
    mask {S}.  bad: further voxels without probabilities (the logits' rule), beside those with a NaN plane."""
    planes = np.asarray(planes, F)
    C, S = planes.shape
    label = np.asarray(label, F).reshape(-1)
    assert label.size == S
    counted = np.ones(S, bool) if mask is None else np.asarray(mask).reshape(-1) != 0
    with np.errstate(invalid="ignore"):
        lab_ok = (label > F(-1.0)) & (label < F(C))
    t = np.where(lab_ok, np.trunc(np.where(lab_ok, label, F(0))), -1).astype(np.int64)
    is_bad = np.isnan(planes).any(axis=0) | (np.zeros(S, bool) if bad is None else np.asarray(bad, bool))
    skipped = ~counted
    invalid = counted & ~lab_ok
    bad_v = counted & lab_ok & is_bad
    valid = counted & lab_ok & ~is_bad
    head = np.asarray([valid.sum(), bad_v.sum(), invalid.sum(), skipped.sum()], np.int64)
    p = planes[:, valid]
    tv = t[valid]
    n = p.shape[1]
    pred = np.argmax(p, axis=0) if n else np.zeros(0, np.int64)          # the first index wins a tie
    conf = p[pred, np.arange(n)]
    qc = code(conf)
    correct = (pred == tv).astype(np.int64)
    top = np.stack([_sum_by(bin_of(qc), val, 20) for val in (np.ones(n, np.int64), correct, qc)], axis=1)
    cls = np.zeros((C, 20, 5), np.int64)
    for c in range(C):
        q = code(p[c])
        pos = (tv == c).astype(np.int64)
        for col, val in enumerate((np.ones(n, np.int64), pos, q, q * pos, q * q)):
            cls[c, :, col] = _sum_by(bin_of(q), val, 20)
    logh = np.bincount(key(p[tv, np.arange(n)]), minlength=4065).astype(np.int64)
    wrong = np.zeros(S, np.uint8)
    wrong[valid] = np.where(correct == 1, 1, 2)
    table = np.concatenate([head, top.reshape(-1), cls.reshape(-1), logh])
    assert table.size == table_len(C) and table.dtype == np.int64
    return table, wrong


def _sum_by(rows, values, n):
    """exact integer sums per row of values below 2^32: np.bincount sums its weights in float64, so the upper and the lower 16 bits
    are summed apart (each sum stays below 2^16 * 2^31 < 2^53) and put together as integers"""
    values = np.asarray(values, np.int64)
    assert values.size == 0 or (values.min() >= 0 and values.max() < 1 << 32)
    hi = np.bincount(rows, weights=(values >> 16).astype(np.float64), minlength=n).astype(np.int64)
    lo = np.bincount(rows, weights=(values & 0xFFFF).astype(np.float64), minlength=n).astype(np.int64)
    return (hi << 16) + lo


def softmax_exact(logits):
    """fp32 probabilities of logits in {0, -200, -inf}: 1 / k for the k channels at 0 (expf(-200) is 0 in fp32 beside a 0, and a
    voxel whose maximum is -200 has k channels at the maximum), 0 elsewhere; -> (planes, bad) with bad the voxels whose channels
    are all -inf"""
    x = np.asarray(logits, F)
    assert np.isin(x, [0.0, -200.0, -INF]).all()
    m = x.max(axis=0)
    bad = np.isneginf(m)
    top = x == m[None]
    k = top.sum(axis=0).astype(F)
    return np.where(top & ~bad[None], F(1) / k[None], F(0)).astype(F), bad


# ---- the restatement on hand-written answers ---------------------------------------------------------------------------------------
def test_the_codings_on_hand_worked_values():
    p = [0.0, -0.0, 1.0, 0.75, 0.5, 0.25, 2.0, -1.0, INF, 1.0 / 65536, 0.99999, np.nextafter(F(1), F(0))]
    assert code(p).tolist() == [0, 0, 65535, 49152, 32768, 16384, 65535, 0, 65535, 1, 65535, 65535]
    assert bin_of([0, 3276, 3277, 32767, 32768, 49152, 62259, 62260, 65535]).tolist() == [0, 0, 1, 9, 10, 15, 18, 19, 19]
    assert (bin_of(np.arange(65536)) == np.arange(65536) * 20 // 65536).all() and np.bincount(bin_of(np.arange(65536))).min() >= 3276
    assert key([0.0, -0.0, -3.0, 1.0, 1.5, INF, 0.5, 0.75, 0.25, np.nextafter(F(1), F(0))]).tolist() == [0, 0, 0, 4064, 4064, 4064, 4032, 4048, 4000, 4063]
    # 32 keys per octave, ordered as the values
    v = np.sort(np.random.default_rng(0).uniform(1e-6, 1, 1000).astype(F))
    assert (np.diff(key(v)) >= 0).all() and key([0.5])[0] - key([0.25])[0] == 32
    lo, hi = CB.key_edges(key(v))
    assert (lo <= v).all() and (v < hi).all() and (hi / lo <= 1 + 1 / 32 + 1e-12).all()


def test_calib_ref_on_a_hand_worked_volume():
    planes = np.asarray([[0.75, 0.5, 0.0, NAN, NAN], [0.25, 0.5, 1.0, NAN, 0.5]], F)
    label = np.asarray([0.0, 1.0, 1.0, 2.0, 0.0], F)
    table, wrong = calib_ref(planes, label)
    head, top, cls, logh = CB.split(table, 2)
    assert head.tolist() == [3, 1, 1, 0]                              # voxel 3: the label 2.0 is invalid; voxel 4: a NaN plane
    want_top = np.zeros((20, 3), np.int64)
    want_top[15] = [1, 1, 49152]                                      # (0.75, 0.25), truth 0: right at 0.75
    want_top[10] = [1, 0, 32768]                                      # the tie: pred 0, truth 1
    want_top[19] = [1, 1, 65535]                                      # (0, 1), truth 1
    assert (top == want_top).all()
    want = np.zeros((2, 20, 5), np.int64)
    want[0, 15] = [1, 1, 49152, 49152, 49152 ** 2]
    want[0, 10] = [1, 0, 32768, 0, 32768 ** 2]
    want[0, 0] = [1, 0, 0, 0, 0]
    want[1, 5] = [1, 0, 16384, 0, 16384 ** 2]
    want[1, 10] = [1, 1, 32768, 32768, 32768 ** 2]
    want[1, 19] = [1, 1, 65535, 65535, 65535 ** 2]
    assert (cls == want).all()
    assert logh.sum() == 3 and logh[4048] == 1 and logh[4032] == 1 and logh[4064] == 1
    assert wrong.tolist() == [1, 2, 1, 0, 0]
    # the mask comes first, then the label, then the probabilities; -0.5 truncates to class 0, C - 0.5 to C - 1, NaN is invalid
    table, wrong = calib_ref(planes, np.asarray([-0.5, 1.5, NAN, 0.0, -1.0], F), mask=np.asarray([1, 255, 1, 0, 7], np.uint8))
    head, top, cls, logh = CB.split(table, 2)
    assert head.tolist() == [2, 0, 2, 1] and wrong.tolist() == [1, 2, 0, 0, 0]
    assert top[15].tolist() == [1, 1, 49152] and top[10].tolist() == [1, 0, 32768] and cls[:, :, 0].sum() == 4
    # the logits' rule marks further voxels bad
    assert calib_ref(planes[:, :3], label[:3], bad=[False, True, False])[0][:4].tolist() == [2, 1, 0, 0]


def test_softmax_exact_is_one_over_k_or_zero():
    x = np.asarray([[0, 0, -200, -INF, -200, -INF], [0, -200, -200, -INF, -INF, 0], [-INF, 0, -200, -INF, -INF, -200]], F)
    p, bad = softmax_exact(x)
    assert bad.tolist() == [False, False, False, True, False, False]
    assert p[:, 0].tolist() == [0.5, 0.5, 0] and p[:, 1].tolist() == [0.5, 0, 0.5] and (p[:, 2] == F(1) / F(3)).all()
    assert p[:, 4].tolist() == [1, 0, 0] and p[:, 5].tolist() == [0, 1, 0] and not np.isnan(p).any()
    assert float(F(math.exp(-200))) == 0.0


def test_the_tables_of_random_volumes_are_consistent():
    rng = np.random.default_rng(1)
    for C in (2, 5):
        S = 500
        x = rng.standard_normal((C, S)) * 3
        p = (np.exp(x) / np.exp(x).sum(0)).astype(F)
        p[:, rng.random(S) < 0.05] = NAN
        label = rng.integers(-1, C + 1, S).astype(F)
        mask = (rng.random(S) < 0.8).astype(np.uint8)
        table, wrong = calib_ref(p, label, mask)
        head, top, cls, logh = CB.split(table, C)
        assert head.sum() == S and top[:, 0].sum() == head[0] == logh.sum() == (wrong > 0).sum()
        assert (cls[:, :, 0].sum(axis=1) == head[0]).all() and cls[:, :, 1].sum() == head[0]
        assert top[:, 1].sum() == (wrong == 1).sum() and (cls[:, :, 3] <= cls[:, :, 2]).all()
        assert CB.accuracy(top) == (wrong == 1).sum() / head[0]


# ---- every host formula on hand-written tables -------------------------------------------------------------------------------------
def test_split_and_merge_bins():
    t = np.arange(table_len(3), dtype=np.int64)
    head, top, cls, logh = CB.split(torch.from_numpy(t), 3)
    assert head.tolist() == [0, 1, 2, 3] and top.shape == (20, 3) and top[0, 0] == 4 and cls.shape == (3, 20, 5) and cls[0, 0, 0] == 64
    assert logh.shape == (4065,) and logh[0] == 364 and logh[-1] == t[-1]
    assert CB.merge_bins(top, 20).tolist() == top.tolist() and CB.merge_bins(top, 1).tolist() == [top.sum(0).tolist()]
    assert CB.merge_bins(top, 10)[3].tolist() == (top[6] + top[7]).tolist() and CB.merge_bins(cls, 5).shape == (3, 5, 5)
    assert CB.merge_bins(cls, 4)[2, 1].tolist() == cls[2, 5:10].sum(0).tolist()
    for bad in (3, 0, 40, 7):
        with pytest.raises(U.UNetError, match="bins"):
            CB.merge_bins(top, bad)
    with pytest.raises(U.UNetError, match="entries"):
        CB.split(t, 4)
    with pytest.raises(U.UNetError, match="integers"):
        CB.split(t.astype(np.float64), 3)


def test_ece_of_a_perfectly_calibrated_table_is_zero_and_of_an_all_wrong_one_is_one():
    top = np.zeros((20, 3), np.int64)
    top[15] = [4, 3, 196606]                                          # mean code 49151.5: confidence 0.75 exactly, 3 of 4 right
    top[10] = [2, 1, 65535]                                           # confidence 0.5 exactly, 1 of 2 right
    conf, acc, n = CB.reliability(top, 10)
    assert conf[7] == 0.75 and acc[7] == 0.75 and n[7] == 4 and conf[5] == 0.5 and acc[5] == 0.5 and np.isnan(conf[0]) and n[0] == 0
    assert CB.ece(top, 10) == 0.0 and CB.mce(top, 10) == 0.0 and CB.ece(top, 20) == 0.0 and CB.accuracy(top) == 4 / 6
    # merged into one bin the two are still calibrated together: confidence (196606 + 65535) / 6 -> 2/3
    assert abs(CB.ece(top, 1)) < 1e-15
    wrong = np.zeros((20, 3), np.int64)
    wrong[19] = [1000, 0, 65535 * 1000]
    assert CB.ece(wrong) == CB.mce(wrong) == 65535.5 / 65536 and CB.accuracy(wrong) == 0.0
    # two bins: the ECE weighs by the count, the MCE takes the worst
    top[19] = [6, 0, 6 * 65535]
    assert CB.ece(top, 10) == pytest.approx(0.5 * 65535.5 / 65536, abs=1e-15) and CB.mce(top, 10) == 65535.5 / 65536
    empty = np.zeros((20, 3), np.int64)
    assert math.isnan(CB.ece(empty)) and math.isnan(CB.mce(empty)) and math.isnan(CB.accuracy(empty))


def test_classwise_ece_and_brier_on_hand_written_rows():
    # certain and right: p = (1, 0), truth 0, n voxels.  The value of a code is its centre, so the Brier score of a class is
    # (0.5 / 65536)^2 = 5.8207660913467407e-11, not 0
    n = 1000
    cls = np.zeros((2, 20, 5), np.int64)
    cls[0, 19] = [n, n, 65535 * n, 65535 * n, 65535 ** 2 * n]
    cls[1, 0] = [n, 0, 0, 0, 0]
    per, total = CB.brier(cls)
    assert per.tolist() == [(0.5 / 65536) ** 2] * 2 == [5.8207660913467407e-11] * 2 and total == 2 * (0.5 / 65536) ** 2
    assert CB.classwise_ece(cls).tolist() == [0.5 / 65536, 0.5 / 65536]
    # certain and wrong: (65535.5 / 65536)^2 per class
    cls[0, 19, 1], cls[0, 19, 3], cls[1, 0, 1] = 0, 0, n
    per, total = CB.brier(cls)
    assert per.tolist() == [(65535.5 / 65536) ** 2] * 2
    # one voxel at (0.75, 0.25), truth 1: (49152.5 / 65536)^2 and (16384.5 / 65536 - 1)^2
    one = np.zeros((2, 20, 5), np.int64)
    one[0, 15] = [1, 0, 49152, 0, 49152 ** 2]
    one[1, 5] = [1, 1, 16384, 16384, 16384 ** 2]
    per, total = CB.brier(one)
    assert per.tolist() == [(49152.5 / 65536) ** 2, (16384.5 / 65536 - 1) ** 2] and total == per[0] + per[1]
    assert CB.classwise_ece(one, 10).tolist() == [49152.5 / 65536, 1 - 16384.5 / 65536]
    # the largest sums a volume can reach stay exact: 2^31 - 1 voxels at code 65535
    big = np.zeros((2, 20, 5), np.int64)
    m = (1 << 31) - 1
    big[:, 19] = [m, m, 65535 * m, 65535 * m, 65535 ** 2 * m]
    assert CB.brier(big)[0].tolist() == [(0.5 / 65536) ** 2] * 2
    assert np.isnan(CB.brier(np.zeros((2, 20, 5), np.int64))[0]).all()


def test_nll_bounds_are_ordered_and_honour_the_floor():
    logh = np.zeros(4065, np.int64)
    logh[4064] = 10
    assert CB.nll_bounds(logh) == (0.0, 0.0, 0.0)                     # p_t = 1
    logh[:] = 0
    logh[4032] = 4                                                    # p_t in [0.5, 0.515625)
    lo, mid, hi = CB.nll_bounds(logh)
    assert lo == -math.log(0.515625) and hi == math.log(2) and lo < mid < hi and mid == pytest.approx(-math.log(math.sqrt(0.5 * 0.515625)), abs=1e-15)
    logh[0] = 4                                                       # p_t <= 0 (or tiny): the floor
    lo2, mid2, hi2 = CB.nll_bounds(logh, floor=1e-12)
    assert lo2 == pytest.approx(0.5 * lo - 0.5 * math.log(1e-12), abs=1e-12) and hi2 == pytest.approx(0.5 * hi - 0.5 * math.log(1e-12), abs=1e-12)
    assert lo2 <= mid2 <= hi2
    # a key whose upper edge is at or below the floor counts -ln floor in all three
    only = np.zeros(4065, np.int64)
    only[int(key([1e-5])[0])] = 3
    assert CB.nll_bounds(only, floor=1e-3) == (-math.log(1e-3),) * 3
    a, b, c = CB.nll_bounds(only, floor=1e-12)
    assert a < b < c and a <= -math.log(1e-5) <= c
    assert all(math.isnan(v) for v in CB.nll_bounds(np.zeros(4065, np.int64)))
    for bad in (0.0, 1.0, -1.0):
        with pytest.raises(U.UNetError, match="floor"):
            CB.nll_bounds(only, floor=bad)
    with pytest.raises(U.UNetError, match="logh"):
        CB.nll_bounds(only[:-1])


def test_the_bracket_holds_the_clipped_nll_of_random_probabilities():
    rng = np.random.default_rng(2)
    for floor in (1e-12, 1e-4):
        p = np.concatenate([rng.uniform(0, 1, 6000), 10.0 ** rng.uniform(-30, 0, 3900), [0.0, 1.0] * 50]).astype(F)
        assert p.size == 10 ** 4 and not ((p > 0) & (p < F(1.2e-38))).any()                  # no subnormals
        logh = np.bincount(key(p), minlength=4065)
        lo, mid, hi = CB.nll_bounds(logh, floor=floor)
        mean = float(np.mean(-np.log(np.maximum(p.astype(np.float64), floor))))
        assert lo <= mean <= hi and lo <= mid <= hi, (lo, mean, hi)
        assert hi - lo <= math.log(1 + 1 / 32) + 1e-12                # a key is at most 1/32 of its value wide


def test_auroc_and_risk_coverage():
    z = np.zeros(256, np.int64)
    low, high = z.copy(), z.copy()
    low[10], low[20], high[200], high[250] = 5, 5, 3, 7
    assert CB.auroc(low, high) == 1.0 and CB.auroc(high, low) == 0.0 and CB.auroc(low, low) == 0.5 and CB.auroc(high, high) == 0.5
    # 2 correct at bin 1, 1 correct and 1 wrong at bin 2: the wrong one beats 2, ties with 1 -> (2 + 0.5) / 3
    a, b = z.copy(), z.copy()
    a[1], a[2], b[2] = 2, 1, 1
    assert CB.auroc(a, b) == 2.5 / 3
    assert math.isnan(CB.auroc(z, high)) and math.isnan(CB.auroc(low, z))
    with pytest.raises(U.UNetError, match="histograms"):
        CB.auroc(z, z[:-1])
    # separated: the risk stays 0 until the wrong voxels come in
    cov, risk, aurc = CB.risk_coverage(low, high)
    assert cov[-1] == 1.0 and cov[20] == 0.5 and risk[20] == 0.0 and risk[-1] == 0.5 and np.isnan(risk[0]) and cov[0] == 0.0
    # trapezoids: 0 up to coverage 0.5, then (0 + 3/13) / 2 over 0.15 and (3/13 + 0.5) / 2 over 0.35
    assert aurc == pytest.approx(0.15 * 0.5 * (3 / 13) + 0.35 * 0.5 * (3 / 13 + 0.5), abs=1e-15)
    # reversed: the wrong ones come first, the risk starts at 1
    cov, risk, worse = CB.risk_coverage(high, low)
    assert risk[20] == 1.0 and risk[200] == 10 / 13 and worse > aurc
    assert worse == pytest.approx(0.5 * 1.0 + 0.15 * 0.5 * (1 + 10 / 13) + 0.35 * 0.5 * (10 / 13 + 0.5), abs=1e-15)
    assert math.isnan(CB.risk_coverage(z, z)[2])


# ---- the ABI -------------------------------------------------------------------------------------------------------------------------
OTHERS = ("unet_stats_", "unet_ens_", "unet_table_", "unet_reg_", "unet_atlas_", "unet_components_", "unet_preproc_", "unet_dist_", "unet_inst_",
          "unet_morph_", "unet_conn_", "unet_mirror_", "unet_tiles_", "unet_space_", "unet_postproc_", "unet_qc_", "unet_feed_", "unet_augment_")


def test_unet_calib_h_declares_exactly_the_exports_and_the_library_has_them():
    lib = ctypes.CDLL(U.engine.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "unet_calib.h")).read()
    declared = set(re.findall(r"\b(unet_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(CB.EXPORTS) == {"unet_calib_table_len", "unet_calib_scratch_bytes", "unet_calib_tables"}
    for name in sorted(declared):
        assert hasattr(lib, name), "libunet_hip.so does not export " + name
    enums = {k: int(v) for k, v in re.findall(r"UNET_CALIB_([A-Z_]+) = (\d+)", hdr)}
    assert enums == {"SRC_LOGITS": CB.SRC_LOGITS, "SRC_PROBS": CB.SRC_PROBS, "IMPL_DEFAULT": CB.IMPL_DEFAULT, "IMPL_LDS": CB.IMPL_LDS,
                     "IMPL_GLOBAL": CB.IMPL_GLOBAL}
    assert (CB.SRC_LOGITS, CB.SRC_PROBS, CB.IMPL_DEFAULT, CB.IMPL_LDS, CB.IMPL_GLOBAL) == (0, 1, 0, 1, 2)
    defines = {k: int(v) for k, v in re.findall(r"#define UNET_CALIB_([A-Z_]+) (\d+)", hdr)}
    assert defines == {"MAX_CLASSES": CB.MAX_CLASSES, "BINS": CB.BINS, "LOG_BINS": CB.LOG_BINS, "CODES": CB.CODES, "LDS_CLASSES": CB.LDS_CLASSES,
                       "LDS_LOG_BINS": CB.LDS_LOG_BINS, "CACHE": CB.CACHE, "UNIT": CB.UNIT, "BLOCK_UNITS": CB.BLOCK_UNITS, "GRID_UNITS": CB.GRID_UNITS}
    assert (CB.MAX_CLASSES, CB.BINS, CB.LOG_BINS, CB.CODES) == (256, 20, 4065, 65536)
    # the static LDS of a block: head, top, the held classes' rows and the held keys, 64-bit entries
    assert (4 + 20 * 3 + CB.LDS_CLASSES * 20 * 5 + CB.LDS_LOG_BINS) * 8 <= 64 * 1024 and CB.LDS_LOG_BINS <= CB.LOG_BINS
    assert CB.GRID_UNITS % CB.BLOCK_UNITS == 0 and CB.BLOCK_UNITS % 64 == 0 and CB.GRID_UNITS * CB.UNIT < 1 << 25
    assert "this project's" in hdr and "NOT pinned" in hdr
    assert U.calib is CB


def test_the_prefixes_stay_apart_in_both_directions():
    for h in sorted(os.listdir(os.path.join(ROOT, "include"))):
        text = open(os.path.join(ROOT, "include", h)).read().lower()
        if h != "unet_calib.h":
            assert "unet_calib_" not in text, h
        else:
            for other in OTHERS:
                assert other not in text, other


# ---- argument errors, before any device call -------------------------------------------------------------------------------------
def test_table_len_and_scratch_bytes_are_monotone_and_check_their_arguments():
    lens = [CB.table_len(c) for c in range(2, 257)]
    assert lens == [table_len(c) for c in range(2, 257)] and all(a < b for a, b in zip(lens, lens[1:]))
    by_c = [CB.scratch_bytes(c, 1000) for c in (2, 3, 6, 16, 17, 255, 256)]
    assert all(a <= b for a, b in zip(by_c, by_c[1:])) and by_c[0] >= table_len(2) * 8 and by_c[-1] >= table_len(256) * 8
    assert len({CB.scratch_bytes(6, v) for v in (1, 64, 10 ** 6, 256 ** 3, (1 << 31) - 1)}) == 1      # nothing per voxel
    for c in (1, 0, -1, 257):
        with pytest.raises(U.UNetError, match=r"unet_calib_table_len: out_c must be in \[2, 256\], got %d" % c):
            CB.table_len(c)
        with pytest.raises(U.UNetError, match=r"unet_calib_scratch_bytes: out_c must be in \[2, 256\], got %d" % c):
            CB.scratch_bytes(c, 10)
    for v in (0, -5, 1 << 31):
        with pytest.raises(U.UNetError, match=r"unet_calib_scratch_bytes: voxels must be in \[1, 2\^31\), got %d" % v):
            CB.scratch_bytes(6, v)
    lib = U.engine.lib
    assert lib.unet_calib_table_len(6, None) != 0 and lib.unet_last_error().decode() == "unet_calib_table_len: null count"
    assert lib.unet_calib_scratch_bytes(6, 10, None) != 0 and lib.unet_last_error().decode() == "unet_calib_scratch_bytes: null bytes"


P = [ctypes.c_void_p(0x1000 * (i + 1)) for i in range(8)]          # never dereferenced
BIG = 1 << 40


def test_tables_argument_errors_need_no_device():
    lib = U.engine.lib

    def call(src=P[0], kind=0, C=6, voxels=64, label=P[1], mask=None, acc=0, tables=P[2], wrong=None, impl=0, scratch=P[3], scratch_bytes=BIG):
        rc = lib.unet_calib_tables(src, kind, C, voxels, label, mask, acc, tables, wrong, impl, scratch, scratch_bytes, None)
        assert rc != 0
        msg = lib.unet_last_error().decode()
        assert msg.startswith("unet_calib_tables: ")
        return msg

    assert "null src" in call(src=None) and "src must be 4-byte aligned" in call(src=ctypes.c_void_p(0x2002))
    assert "unknown src_kind 2" in call(kind=2) and "unknown src_kind -1" in call(kind=-1)
    assert "out_c must be in [2, 256], got 1" in call(C=1) and "out_c must be in [2, 256], got 257" in call(C=257)
    assert "voxels must be in [1, 2^31), got 0" in call(voxels=0) and "voxels" in call(voxels=-3) and "voxels" in call(voxels=1 << 31)
    assert "null label" in call(label=None) and "label must be 4-byte aligned" in call(label=ctypes.c_void_p(0x2001))
    assert "null tables" in call(tables=None) and "tables must be 8-byte aligned" in call(tables=ctypes.c_void_p(0x3004))
    assert "unknown impl 3" in call(impl=3) and "unknown impl -1" in call(impl=-1)
    assert "null scratch" in call(scratch=None)
    assert "scratch too small" in call(scratch_bytes=CB.scratch_bytes(6, 64) - 1)
    assert "scratch too small" in call(C=7, scratch_bytes=CB.scratch_bytes(6, 64))
    # both kinds and both flags of accumulate reach the same checks
    assert "null tables" in call(kind=1, acc=1, tables=None, mask=P[4], wrong=P[5])


def test_wrapper_errors_need_no_device():
    x, lab = torch.zeros(2, 8, dtype=torch.float32), torch.zeros(8, dtype=torch.float32)
    with pytest.raises(U.UNetError, match="logits must be"):
        CB.tables(x, lab)
    with pytest.raises(U.UNetError, match="planes must be"):
        CB.tables_from_probs(x, 2, 8, lab)
    with pytest.raises(U.UNetError, match="planes must be"):
        CB.tables_from_probs(None, 2, 8, lab)


# ---- the refusals of qc.calibration_qc --------------------------------------------------------------------------------------------------
def test_calibration_qc_refusals_need_no_device():
    m = types.SimpleNamespace(in_count=1, out_count=4, dim=(16, 16, 16), voxel_size=(1.0, 1.0, 1.0))
    case = [("a.nii.gz", "b.nii.gz", np.zeros((1, 16, 16, 16), F), np.zeros((16, 16, 16), F), True)]
    path = "/nowhere/model.nz"
    assert Q.calibration_qc(m, path, []) == (1, "no image/label pairs found")
    assert Q.calibration_qc(types.SimpleNamespace(in_count=1, out_count=1, dim=(16, 16, 16)), path, case) == (1, "QC requires a categorical model")
    assert Q.calibration_qc(m, path, case, mask="brain") == (1, "calibration_qc: mask must be one of all, foreground, got 'brain'")
    for bins in (3, 0, 40, 2.0, True):
        assert Q.calibration_qc(m, path, case, bins=bins) == (1, "calibration_qc: bins must divide 20, got %r" % (bins,))
    assert Q.calibration_qc(m, path, case, ensemble_weights=[1.0]) == (1, "ensemble_weights needs ensemble")
    assert Q.calibration_qc(m, path, case, ensemble=m)[1].startswith("ensemble must be a list of further models")
    other = types.SimpleNamespace(in_count=1, out_count=5, dim=(16, 16, 16))
    assert Q.calibration_qc(m, path, case, ensemble=[other]) == (1, "ensemble: member 1 has out_count 5, member 0 has 4")
    assert Q.calibration_qc(m, path, case, ensemble=[types.SimpleNamespace(in_count=1)]) == (1, "ensemble: member 1 is not a model (it has no out_count)")
    assert Q.calibration_report_path("/x/y/model.nz") == "/x/y/model.calibration_report.tsv"


def test_format_calibration_report():
    s = {"voxels": 10, "accuracy": 0.5, "ece": 0.25, "mce": 0.5, "brier": 0.125, "nll": 1.5, "cw_ece": np.asarray([0.1, 0.2]),
         "brier_c": np.asarray([0.0625, 0.0625]), "auroc_entropy": 0.75, "aurc_entropy": 0.2}
    text = Q.format_calibration_report(2, [("/d/a_T1w.nii.gz", "/d/a_seg.nii.gz", s), ("/d/b.nii.gz", "/d/b_seg.nii.gz", None), ("total", "", s)])
    lines = text.split("\n")
    assert lines[0] == "image\tground_truth\tvoxels\taccuracy\tece\tmce\tbrier\tnll\tcw_ece0\tcw_ece1\tbrier0\tbrier1" and lines[-1] == ""
    assert lines[1] == "a_T1w.nii.gz\ta_seg.nii.gz\t10\t0.5\t0.25\t0.5\t0.125\t1.5\t0.1\t0.2\t0.0625\t0.0625"
    assert lines[2] == "b.nii.gz\tb_seg.nii.gz" + "\tN/A" * 10 and lines[3].startswith("total\t\t10\t")
    with_e = Q.format_calibration_report(2, [("a", "b", s)], with_entropy=True).split("\n")
    assert with_e[0].endswith("\tbrier1\tauroc_entropy\taurc_entropy") and with_e[1].endswith("\t0.75\t0.2")
