"""The per-region intensity statistics on the device (include/unet_stats.h): what is in the regions of a parcellation.

  moments      per label: n, NaNs, below, above, the sums of q and q * q, min and max q, min and max key -- one pass over a label
               map and a float32 volume
  hist         per label: 256 bins over the codes' upper eight bits -- one pass
  quantiles    per label: up to eight quantiles (permille) as codes, by a two-level radix select -- two passes, no sort
  code_value, decode_key, summary   the host arithmetic on those rows, float64
  volume_range the exact (min, max) of a volume, from one moments call without a label map

A voxel's code q is (int)((v - lo) * scale) clamped to [0, 65535], scale = 65536 / (hi - lo), all in fp32; its key is the
order-preserving image of the float's bits.  With labels=None the whole volume is one region (n_labels 0, the single row 0).  The
reference has no counterpart, so these are this project's definitions (parity NOT pinned).  Every result is an integer: the device
is pinned to the numpy restatements of tests/test_stats_host.py bit for bit.  IMPL_LDS gathers a block's updates in LDS, IMPL_GLOBAL
updates global memory only (the measured baseline and a second witness of the bits)."""
import ctypes as C

import numpy as np
import torch

from . import engine as E
from .engine import UNetError

_common = (C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_int, C.c_float, C.c_float)
E._sig("unet_stats_scratch_bytes", C.c_int, C.c_int64, C.c_int, C.c_int, C.POINTER(C.c_size_t))
E._sig("unet_stats_moments", C.c_int, *_common, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p)
E._sig("unet_stats_hist", C.c_int, *_common, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p)
E._sig("unet_stats_quantiles", C.c_int, *_common, C.POINTER(C.c_int), C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p)
# every symbol include/unet_stats.h declares
EXPORTS = ["unet_stats_scratch_bytes", "unet_stats_moments", "unet_stats_hist", "unet_stats_quantiles"]

IMPL_DEFAULT, IMPL_LDS, IMPL_GLOBAL = 0, 1, 2
MAX_LABELS = 65535            # UNET_STATS_MAX_LABELS
MAX_QUANTILE_LABELS = 4095    # UNET_STATS_MAX_QUANTILE_LABELS
MAX_QUANTILES = 8             # UNET_STATS_MAX_QUANTILES
MOMENT_COLUMNS, HIST_BINS, CODES = 10, 256, 65536
LDS_ROWS, LDS_SLOTS, SLOT_BINS, LDS_PROBES = 1024, 512, 16, 8
UNIT, WAVE_UNITS, GRID_UNITS = 8, 512, 2097152
# the columns of a moments row
N, NAN, BELOW, ABOVE, SUM_Q, SUM_QQ, MIN_Q, MAX_Q, MIN_KEY, MAX_KEY = range(10)


def stats_scratch_bytes(voxels, n_labels, n_quantiles=0):
    """One size for the three calls (n_quantiles 0 for moments and hist): the running tables, nothing per voxel."""
    return E.size_query(E.lib.unet_stats_scratch_bytes, int(voxels), int(n_labels), int(n_quantiles))


def _inputs(labels, image, n_labels, who):
    """-> (labels pointer or None, label_bytes, voxels, L)"""
    if not (torch.is_tensor(image) and image.is_cuda and image.dtype == torch.float32 and image.is_contiguous() and image.numel() > 0):
        raise UNetError("stats.%s: image must be a contiguous float32 device tensor" % who)
    L = int(n_labels)
    if labels is None:
        if L != 0:
            raise UNetError("stats.%s: n_labels must be 0 without labels, got %d" % (who, L))
        return None, 1, image.numel(), 0
    if not (torch.is_tensor(labels) and labels.is_cuda and labels.dtype in (torch.uint8, torch.uint16) and labels.is_contiguous()
            and labels.device == image.device):
        raise UNetError("stats.%s: labels must be None or a contiguous uint8 or uint16 device tensor on image's device" % who)
    if labels.numel() != image.numel():
        raise UNetError("stats.%s: labels holds %d voxels, image %d" % (who, labels.numel(), image.numel()))
    return labels.data_ptr(), labels.element_size(), image.numel(), L


def _out(out, n, dtype, dev, who):
    if out is None:
        return torch.empty(n, dtype=dtype, device=dev)
    if not (torch.is_tensor(out) and out.is_cuda and out.device == dev and out.is_contiguous() and out.dtype == dtype and out.numel() == n):
        raise UNetError("stats.%s: out must be a contiguous %s device tensor of %d entries" % (who, str(dtype).replace("torch.", ""), n))
    return out


def moments(labels, image, n_labels, lo, hi, impl=IMPL_DEFAULT, out=None, scratch=None, stream=None):
    """unet_stats_moments on the current stream (or the raw `stream`).  labels: a uint8 or uint16 device tensor of image's element
    count, or None (one region, n_labels 0); a value above n_labels reads as 0.  image: float32.  Returns int64 {n_labels + 1, 10} on
    the device (written into `out` when given): n, NaNs, below, above, sum q, sum q * q, min q, max q, min key, max key; an empty
    row holds 0, its NaNs, 0, 0, 0, 0, 65536, -1, 0xFFFFFFFF, -1.  No host synchronisation."""
    ptr, nbytes, voxels, L = _inputs(labels, image, n_labels, "moments")
    need = stats_scratch_bytes(voxels, L)                          # the range checks, before any device work
    rows = _out(out, (L + 1) * MOMENT_COLUMNS, torch.int64, image.device, "moments")
    scratch = E.scratch(scratch, need, image.device)
    E.check(E.lib.unet_stats_moments(ptr, nbytes, image.data_ptr(), voxels, L, float(lo), float(hi), rows.data_ptr(), int(impl),
                                     scratch.data_ptr(), scratch.nbytes, E.stream(image, stream)))
    return rows.view(L + 1, MOMENT_COLUMNS)


def hist(labels, image, n_labels, lo, hi, impl=IMPL_DEFAULT, out=None, scratch=None, stream=None):
    """unet_stats_hist on the current stream (or the raw `stream`); arguments as for moments, n_labels <= 4095.  Returns int64
    {n_labels + 1, 256} on the device: the coded voxels of a row whose q >> 8 is the column.  No host synchronisation."""
    ptr, nbytes, voxels, L = _inputs(labels, image, n_labels, "hist")
    if L > MAX_QUANTILE_LABELS:
        raise UNetError("stats.hist: n_labels must be at most %d, got %d" % (MAX_QUANTILE_LABELS, L))
    need = stats_scratch_bytes(voxels, L)
    rows = _out(out, (L + 1) * HIST_BINS, torch.int64, image.device, "hist")
    scratch = E.scratch(scratch, need, image.device)
    E.check(E.lib.unet_stats_hist(ptr, nbytes, image.data_ptr(), voxels, L, float(lo), float(hi), rows.data_ptr(), int(impl),
                                  scratch.data_ptr(), scratch.nbytes, E.stream(image, stream)))
    return rows.view(L + 1, HIST_BINS)


def _permille(permille, who):
    try:
        p = [int(v) for v in permille]
        exact = all(float(v) == float(q) for v, q in zip(permille, p))
    except (TypeError, ValueError):
        p, exact = [], False
    if not exact or not 1 <= len(p) <= MAX_QUANTILES or any(v < 0 or v > 1000 for v in p):
        raise UNetError("stats.%s: permille must be 1 to %d integers in [0, 1000]" % (who, MAX_QUANTILES))
    return p


def quantiles(labels, image, n_labels, lo, hi, permille=(500,), impl=IMPL_DEFAULT, out=None, scratch=None, stream=None):
    """unet_stats_quantiles on the current stream (or the raw `stream`); arguments as for moments, n_labels <= 4095.  permille: 1 to 8
    integers in [0, 1000] (500 the median; duplicates allowed).  Returns int32 {n_labels + 1, len(permille)} on the device: the
    code of rank p * (n - 1) // 1000 among the row's n coded voxels, -1 for an empty row (code_value turns a code into image units).
    No host synchronisation."""
    ptr, nbytes, voxels, L = _inputs(labels, image, n_labels, "quantiles")
    p = _permille(permille, "quantiles")
    Q = len(p)
    need = stats_scratch_bytes(voxels, L, Q)
    res = _out(out, (L + 1) * Q, torch.int32, image.device, "quantiles")
    scratch = E.scratch(scratch, need, image.device)
    E.check(E.lib.unet_stats_quantiles(ptr, nbytes, image.data_ptr(), voxels, L, float(lo), float(hi), (C.c_int * Q)(*p), Q, res.data_ptr(),
                                       int(impl), scratch.data_ptr(), scratch.nbytes, E.stream(image, stream)))
    return res.view(L + 1, Q)


def volume_range(image):
    """The exact (min, max) of a float32 device volume over its non-NaN voxels, as Python floats; (nan, nan) when every voxel is
    NaN.  One moments call without a label map on the current stream; only the keys are read, so lo and hi do not matter.
    SYNCHRONISES with the host once: the row is copied back."""
    row = moments(None, image, 0, 0.0, 1.0).cpu().numpy()[0]
    if row[N] == 0:
        return float("nan"), float("nan")
    return float(decode_key(row[MIN_KEY])), float(decode_key(row[MAX_KEY]))


# ---- host arithmetic on the rows, float64 ----------------------------------------------------------------------------------------
def _scale(lo, hi):
    lo, hi = np.float32(lo), np.float32(hi)
    with np.errstate(all="ignore"):
        scale = np.float32(65536.0) / np.float32(hi - lo)
    if not (np.isfinite(lo) and np.isfinite(hi) and lo < hi and np.isfinite(scale) and scale > 0):
        raise UNetError("stats: lo and hi must be finite with lo < hi and a finite scale 65536 / (hi - lo)")
    return np.float64(lo), np.float64(scale)


def code_value(q, lo, hi):
    """float64: the centre of code q in image units, lo + (q + 0.5) / scale with the fp32 scale the device used"""
    lo64, scale = _scale(lo, hi)
    return lo64 + (np.asarray(q, np.float64) + 0.5) / scale


def decode_key(key):
    """float32: the value whose order-preserving key this is (the inverse of b ^ (b >> 31 ? 0xFFFFFFFF : 0x80000000))"""
    k = np.asarray(key).astype(np.int64)
    if ((k < 0) | (k > 0xFFFFFFFF)).any():
        raise UNetError("stats.decode_key: a key is an unsigned 32-bit value")
    k = k.astype(np.uint32)
    bits = np.where(k >> np.uint32(31), k ^ np.uint32(0x80000000), k ^ np.uint32(0xFFFFFFFF)).astype(np.uint32)
    return bits.view(np.float32)


def summary(rows, lo, hi, quantile_codes=None):
    """The table a parcellation is consumed as, from a moments table (and the codes quantiles returned): a dict of float64 arrays
    {labels + 1} -- n, nan, below, above, mean, std (population, from the sums of q and q * q, in image units), min, max (exact,
    from the keys) -- and `quantiles` {labels + 1, Q} in image units when quantile_codes is given.  An empty row yields NaN for
    mean, std, min, max and its quantiles."""
    if torch.is_tensor(rows):
        rows = rows.cpu().numpy()
    rows = np.asarray(rows)
    if rows.ndim != 2 or rows.shape[1] != MOMENT_COLUMNS or rows.dtype.kind not in "iu":
        raise UNetError("stats.summary: rows must be integers {labels + 1, %d}" % MOMENT_COLUMNS)
    rows = rows.astype(np.int64)
    lo64, scale = _scale(lo, hi)
    n = rows[:, N].astype(np.float64)
    some = rows[:, N] > 0
    with np.errstate(invalid="ignore", divide="ignore"):
        mq = rows[:, SUM_Q].astype(np.float64) / n
        # the variance from exact integers: n * sum q^2 - (sum q)^2 fits Python's integers, not int64
        var = np.asarray([(int(r[N]) * int(r[SUM_QQ]) - int(r[SUM_Q]) ** 2) / (int(r[N]) ** 2) if r[N] > 0 else np.nan for r in rows],
                         np.float64)
        out = {"n": n, "nan": rows[:, NAN].astype(np.float64), "below": rows[:, BELOW].astype(np.float64),
               "above": rows[:, ABOVE].astype(np.float64),
               "mean": np.where(some, lo64 + (mq + 0.5) / scale, np.nan), "std": np.where(some, np.sqrt(var) / scale, np.nan)}
    keys = np.where(some[:, None], rows[:, MIN_KEY:MAX_KEY + 1], 0x80000000)
    ext = decode_key(keys).astype(np.float64)
    out["min"], out["max"] = np.where(some, ext[:, 0], np.nan), np.where(some, ext[:, 1], np.nan)
    if quantile_codes is not None:
        if torch.is_tensor(quantile_codes):
            quantile_codes = quantile_codes.cpu().numpy()
        qc = np.asarray(quantile_codes)
        if qc.ndim != 2 or qc.shape[0] != rows.shape[0] or qc.dtype.kind not in "iu":
            raise UNetError("stats.summary: quantile_codes must be integers {labels + 1, Q}")
        out["quantiles"] = np.where(qc >= 0, code_value(np.maximum(qc, 0), lo, hi), np.nan)
    return out
