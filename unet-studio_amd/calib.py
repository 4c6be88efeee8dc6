"""Calibration tables on the device (include/unet_calib.h): whether the probabilities of a segmentation mean anything.

  tables, tables_from_probs   one fused pass over the probabilities of a volume (formed from level-0 logits on the fly, or read from
               planes such as an ensemble state's), the truth label and an optional mask -> one int64 table: the head counts, the
               top-label reliability rows, the class-wise rows with their first and second moments, a log-spaced histogram of p_t
  uncertainty_hists   an uncertainty map histogrammed over the correct and over the wrong voxels (stats.hist on the `wrong` map)
  split, merge_bins, accuracy, reliability, ece, mce, classwise_ece, brier, nll_bounds, auroc, risk_coverage
               the host arithmetic on those tables: Python ints and float64

A probability p has the code q = (int)(p * 65536) clamped to [0, 65535], whose value is (q + 0.5) / 65536; 20 bins over the codes,
which merge into 10, 5, 4, 2 or 1; p_t also has the key float_bits(p) >> 18 (32 log-spaced bins per octave).  The reference has no
counterpart, so these are this project's definitions (parity NOT pinned).  Every entry of a table is an integer: the
device is pinned to the numpy restatement of tests/test_calib_host.py bit for bit.  IMPL_LDS gathers a block's updates in LDS,
IMPL_GLOBAL updates global memory only (the baseline and a second witness of the bits)."""
import ctypes as C
import math

import numpy as np
import torch

from . import engine as E
from .engine import UNetError

E._sig("unet_calib_table_len", C.c_int, C.c_int, C.POINTER(C.c_size_t))
E._sig("unet_calib_scratch_bytes", C.c_int, C.c_int, C.c_int64, C.POINTER(C.c_size_t))
E._sig("unet_calib_tables", C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
       C.c_int, C.c_void_p, C.c_size_t, C.c_void_p)
# every symbol include/unet_calib.h declares
EXPORTS = ["unet_calib_table_len", "unet_calib_scratch_bytes", "unet_calib_tables"]

SRC_LOGITS, SRC_PROBS = 0, 1
IMPL_DEFAULT, IMPL_LDS, IMPL_GLOBAL = 0, 1, 2
MAX_CLASSES, BINS, LOG_BINS, CODES = 256, 20, 4065, 65536
LDS_CLASSES, LDS_LOG_BINS, CACHE = 16, 1024, 8
UNIT, BLOCK_UNITS, GRID_UNITS = 8, 256, 131072
# head
VALID, BAD, INVALID_LABEL, SKIPPED = range(4)
# the columns of a top row and of a cls row
TOP_N, TOP_CORRECT, TOP_SUM_Q = range(3)
CLS_N, CLS_POS, CLS_SUM_Q, CLS_SUM_Q_POS, CLS_SUM_QQ = range(5)


# ---- the device calls ------------------------------------------------------------------------------------------------------------
def table_len(out_c):
    """int64 elements of the table of out_c classes: 4 + 20 * 3 + out_c * 20 * 5 + 4065; the library's refusal of out_c raises"""
    return E.size_query(E.lib.unet_calib_table_len, int(out_c))


def scratch_bytes(out_c, voxels):
    """bytes of the scratch of a tables call: the running table, nothing per voxel"""
    return E.size_query(E.lib.unet_calib_scratch_bytes, int(out_c), int(voxels))


def _dev(a, dtype, name, device=None):
    if not (torch.is_tensor(a) and a.is_cuda and a.dtype == dtype and a.is_contiguous()):
        raise UNetError("calib: %s must be a contiguous %s device tensor" % (name, str(dtype).replace("torch.", "")))
    if device is not None and a.device != device:
        raise UNetError("calib: %s is on %s, the planes on %s" % (name, a.device, device))
    return a


def _run(planes, kind, out_c, voxels, label, mask, out, accumulate, wrong, impl, scratch):
    dev = planes.device
    out_c, voxels = int(out_c), int(voxels)
    need = scratch_bytes(out_c, voxels)                 # the class / size checks first
    n = table_len(out_c)
    _dev(label, torch.float32, "label", dev)
    if label.numel() != voxels:
        raise UNetError("calib: label holds %d voxels, the planes %d" % (label.numel(), voxels))
    for t, name in ((mask, "mask"), (wrong, "wrong")):
        if t is not None:
            _dev(t, torch.uint8, name, dev)
            if t.numel() != voxels:
                raise UNetError("calib: %s holds %d voxels, the planes %d" % (name, t.numel(), voxels))
    if out is None:
        if accumulate:
            raise UNetError("calib: accumulate needs the table to add to (out)")
        out = torch.empty(n, dtype=torch.int64, device=dev)
    else:
        _dev(out, torch.int64, "out", dev)
        if out.numel() != n:
            raise UNetError("calib: out must hold %d entries for %d classes, got %d" % (n, out_c, out.numel()))
    scratch = E.scratch(scratch, need, dev)
    E.check(E.lib.unet_calib_tables(planes.data_ptr(), int(kind), out_c, voxels, label.data_ptr(), mask.data_ptr() if mask is not None else None,
                                    int(bool(accumulate)), out.data_ptr(), wrong.data_ptr() if wrong is not None else None, int(impl),
                                    scratch.data_ptr(), scratch.nbytes, E.stream(planes)))
    return out


def tables(logits, label, mask=None, out=None, accumulate=False, wrong=None, impl=IMPL_DEFAULT, scratch=None):
    """unet_calib_tables over level-0 logits on the current stream.  logits: {C, d, h, w} or {1, C, d, h, w} (any {C, ...}), a
    contiguous fp32 device tensor; label: fp32, one value per voxel; mask: uint8 per voxel or None (0: the voxel is skipped); out: the
    int64 table to write (or, with accumulate, to add to); wrong: a uint8 tensor per voxel that receives 0 / 1 / 2 (not counted /
    correct / wrong).  Returns the int64 device table of table_len(C) entries (split reads it).  No host synchronisation."""
    _dev(logits, torch.float32, "logits")
    if logits.dim() == 5 and logits.shape[0] == 1:
        logits = logits[0]
    if logits.dim() < 2:
        raise UNetError("calib: logits must be {C, ...}, got %s" % (tuple(logits.shape),))
    out_c = int(logits.shape[0])
    return _run(logits, SRC_LOGITS, out_c, logits.numel() // max(out_c, 1), label, mask, out, accumulate, wrong, impl, scratch)


def tables_from_probs(planes, out_c, voxels, label, mask=None, out=None, accumulate=False, wrong=None, impl=IMPL_DEFAULT, scratch=None):
    """unet_calib_tables over probabilities on the current stream.  planes: a contiguous device tensor that starts with out_c fp32
    planes of `voxels` values each -- a float32 tensor, or the uint8 state tensor of ensemble.new_state / ensemble.accumulate as it
    is (its first out_c planes are the mean probabilities).  The other arguments as for tables."""
    if not (torch.is_tensor(planes) and planes.is_cuda and planes.is_contiguous() and planes.dtype in (torch.float32, torch.uint8)):
        raise UNetError("calib: planes must be a contiguous float32 device tensor or an ensemble state")
    out_c, voxels = int(out_c), int(voxels)
    scratch_bytes(out_c, voxels)
    if planes.nbytes < out_c * voxels * 4:
        raise UNetError("calib: planes hold %d bytes, %d classes at %d voxels need %d" % (planes.nbytes, out_c, voxels, out_c * voxels * 4))
    return _run(planes, SRC_PROBS, out_c, voxels, label, mask, out, accumulate, wrong, impl, scratch)


def uncertainty_hists(wrong, umap, lo, hi):
    """An uncertainty map (entropy, mutual_info, 1 - confidence: fp32, one value per voxel) histogrammed over the voxels a tables call
    marked correct and over those it marked wrong: stats.hist with `wrong` as the label map -> (h_correct, h_wrong), int64 {256}
    device tensors over the codes of [lo, hi] (NaNs are not counted)."""
    from . import stats as ST
    rows = ST.hist(wrong.view(-1), umap.view(-1), 2, lo, hi)
    return rows[1], rows[2]


# ---- host arithmetic on the tables: Python ints and float64 --------------------------------------------------------------------------
def _host(t):
    if torch.is_tensor(t):
        t = t.cpu().numpy()
    t = np.asarray(t)
    if t.dtype.kind not in "iu":
        raise UNetError("calib: a table holds integers, got %s" % t.dtype)
    return t.astype(np.int64)


def split(tables, out_c):
    """-> (head {4}, top {20, 3}, cls {out_c, 20, 5}, logh {4065}): int64 numpy views of one table"""
    t = _host(tables).reshape(-1)
    out_c = int(out_c)
    n = 4 + BINS * 3 + out_c * BINS * 5 + LOG_BINS
    if out_c < 2 or t.size != n:
        raise UNetError("calib.split: a table of %d classes holds %d entries, got %d" % (out_c, n, t.size))
    a, b = 4 + BINS * 3, 4 + BINS * 3 + out_c * BINS * 5
    return t[:4], t[4:a].reshape(BINS, 3), t[a:b].reshape(out_c, BINS, 5), t[b:]


def merge_bins(t, bins):
    """the rows of top {20, k} or cls {C, 20, k} summed into `bins` equal bins (a divisor of 20)"""
    t = _host(t)
    bins = int(bins)
    if bins < 1 or BINS % bins or t.ndim < 2 or t.shape[-2] != BINS:
        raise UNetError("calib.merge_bins: bins must divide %d and the table have %d rows, got %d bins for %s" % (BINS, BINS, bins, t.shape))
    return t.reshape(t.shape[:-2] + (bins, BINS // bins, t.shape[-1])).sum(axis=-2)


def code_value(sum_q, n):
    """float64: the mean value of n codes whose sum is sum_q, (sum_q / n + 0.5) / 65536; NaN for n == 0"""
    sum_q, n = np.asarray(sum_q, np.float64), np.asarray(n, np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(n > 0, (sum_q / n + 0.5) / CODES, np.nan)


def accuracy(top):
    """correct / n over the top rows; NaN without voxels"""
    top = _host(top)
    n = int(top[:, TOP_N].sum())
    return int(top[:, TOP_CORRECT].sum()) / n if n else float("nan")


def reliability(top, bins=10):
    """-> (mean confidence, accuracy, count) per bin, float64 {bins}: the reliability diagram; an empty bin reads NaN, NaN, 0"""
    t = merge_bins(top, bins)
    n = t[:, TOP_N].astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        acc = np.where(n > 0, t[:, TOP_CORRECT] / n, np.nan)
    return code_value(t[:, TOP_SUM_Q], t[:, TOP_N]), acc, n


def _gaps(conf, acc, n):
    some = n > 0
    return np.abs(conf[some] - acc[some]), n[some]


def ece(top, bins=10):
    """the expected calibration error: sum over the bins of n_b / n * |accuracy_b - confidence_b|; NaN without voxels"""
    gap, n = _gaps(*reliability(top, bins))
    return float((gap * n).sum() / n.sum()) if n.size else float("nan")


def mce(top, bins=10):
    """the maximum calibration error: the largest |accuracy_b - confidence_b| over the bins that hold voxels"""
    gap, n = _gaps(*reliability(top, bins))
    return float(gap.max()) if n.size else float("nan")


def classwise_ece(cls, bins=10):
    """per class c, the ECE of p_c against the indicator t == c -> float64 {C}"""
    t = merge_bins(cls, bins)
    out = np.full(t.shape[0], np.nan)
    for c in range(t.shape[0]):
        n = t[c, :, CLS_N].astype(np.float64)
        if n.sum() > 0:
            with np.errstate(invalid="ignore", divide="ignore"):
                freq = np.where(n > 0, t[c, :, CLS_POS] / n, np.nan)
            gap, m = _gaps(code_value(t[c, :, CLS_SUM_Q], t[c, :, CLS_N]), freq, n)
            out[c] = (gap * m).sum() / m.sum()
    return out


def brier(cls):
    """-> (per class float64 {C}, their sum): the mean over the valid voxels of (v - y)^2 with v the value of the code of p_c and y the
    indicator t == c, from exact integers: sum (v - y)^2 = (sum q^2 + sum q + n / 4) / 2^32 - 2 (sum_pos q + pos / 2) / 2^16 + pos"""
    t = _host(cls)
    per = np.full(t.shape[0], np.nan)
    for c in range(t.shape[0]):
        n, pos, sq, sqp, sqq = (int(v) for v in t[c].sum(axis=0))
        if n:
            # times 2^34, an integer: 4 sum q^2 + 4 sum q + n - 2^19 sum_pos q - 2^18 pos + 2^34 pos
            num = 4 * sqq + 4 * sq + n - (sqp << 19) - (pos << 18) + (pos << 34)
            per[c] = num / (n << 34)                   # Python ints: one rounding
    return per, float(per.sum())


def key_edges(key):
    """float64 (lower, upper) edges of the p_t values of a key: key 0 is p <= 0 and what rounds below the first key, key 4064 is
    p >= 1 (both edges 1)"""
    k = np.asarray(key, np.int64)
    lo = (k.astype(np.uint32) << np.uint32(18)).view(np.float32).astype(np.float64)
    hi = ((np.minimum(k + 1, LOG_BINS - 1)).astype(np.uint32) << np.uint32(18)).view(np.float32).astype(np.float64)
    return lo, hi


def nll_bounds(logh, floor=1e-12):
    """-> (lo, mid, hi): the mean over the valid voxels of -ln max(p_t, floor), bracketed rigorously from each key's two edges (lo from
    the upper edge, hi from the lower) and estimated from their geometric mean.  A key whose upper edge is at or below `floor` counts
    -ln floor in all three; a lower edge below the floor is clipped to it, and a p_t above 1 counts as 1.  NaN without voxels."""
    h = _host(logh).reshape(-1)
    if h.size != LOG_BINS:
        raise UNetError("calib.nll_bounds: logh holds %d entries, got %d" % (LOG_BINS, h.size))
    floor = float(floor)
    if not 0.0 < floor < 1.0:
        raise UNetError("calib.nll_bounds: floor must be in (0, 1), got %r" % floor)
    n = int(h.sum())
    if not n:
        return float("nan"), float("nan"), float("nan")
    e_lo, e_hi = key_edges(np.arange(LOG_BINS))
    e_lo, e_hi = np.maximum(e_lo, floor), np.maximum(e_hi, floor)      # the upper edge at or below the floor: both become the floor
    w = h.astype(np.float64)
    lo, hi = -np.log(e_hi), -np.log(e_lo)
    mid = 0.5 * (lo + hi)                                              # -ln of the geometric mean of the edges
    return tuple(float(math.fsum(w * x) / n) + 0.0 for x in (lo, mid, hi))


def _hists(h_correct, h_wrong):
    a, b = _host(h_correct).reshape(-1), _host(h_wrong).reshape(-1)
    if a.size != b.size or not a.size:
        raise UNetError("calib: the two histograms must have the same bins")
    return a, b


def auroc(h_correct, h_wrong):
    """The probability that a wrong voxel is more uncertain than a correct one, ties within a bin counting a half, from the two
    histograms of uncertainty_hists (Python ints: exact before the last division); NaN when either is empty."""
    a, b = _hists(h_correct, h_wrong)
    na, nb = int(a.sum()), int(b.sum())
    if not na or not nb:
        return float("nan")
    below, twice = 0, 0
    for x, y in zip(a.tolist(), b.tolist()):
        twice += y * (2 * below + x)                   # the correct voxels in lower bins, and half of those in this one
        below += x
    return twice / (2 * na * nb)


def risk_coverage(h_correct, h_wrong):
    """-> (coverage {bins}, risk {bins}, aurc): keep the voxels of the k + 1 least uncertain bins; coverage is their share of all
    voxels, risk the share of wrong ones among them (NaN while nothing is kept).  aurc is the area under risk over coverage by
    trapezoids between the bins' ends, the first one starting at its own risk; NaN without voxels."""
    a, b = _hists(h_correct, h_wrong)
    n = int(a.sum()) + int(b.sum())
    if not n:
        return np.zeros(a.size), np.full(a.size, np.nan), float("nan")
    kept = np.cumsum(a + b).astype(np.float64)
    bad = np.cumsum(b).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        risk = np.where(kept > 0, bad / kept, np.nan)
    cov = kept / n
    area, k0, w0 = 0.0, 0.0, 0.0                       # trapezoids in coverage between the bins' ends; the first starts at its own risk
    for k, w in zip(kept.tolist(), bad.tolist()):
        if k > k0:
            r1 = w / k
            r0 = w0 / k0 if k0 else r1
            area += (k - k0) / n * 0.5 * (r0 + r1)
        k0, w0 = k, w
    return cov, risk, area
