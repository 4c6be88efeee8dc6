"""The tables of a label map on the device (include/unet_table.h): what a parcellation is consumed as.

  regions      per label: the number of voxels, the sums of x, y and z, the bounding box -- from one pass over a region map
  overlap      per label: the voxels where a reads it, where b reads it, where both do -- from one pass over two maps
  volumes_mm3, centroids, dice   the host arithmetic on those rows, float64

The reference stops before using the atlas it loads (evaluate.cpp:488-496), so these are this project's definitions (parity NOT
pinned).  Every column is an integer count or extreme: the device is pinned to the numpy restatements of tests/test_table_host.py
bit for bit.  IMPL_LDS gathers the rows below LDS_ROWS in a block's LDS table, IMPL_GLOBAL updates global memory only (the
measured baseline and a second witness of the bits)."""
import ctypes as C

import numpy as np
import torch

from . import engine as E
from .engine import UNetError

E._sig("unet_table_scratch_bytes", C.c_int, C.c_int64, C.c_int, C.POINTER(C.c_size_t))
E._sig("unet_table_regions", C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t,
       C.c_void_p)
E._sig("unet_table_overlap", C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
       C.c_size_t, C.c_void_p)
# every symbol include/unet_table.h declares
EXPORTS = ["unet_table_scratch_bytes", "unet_table_regions", "unet_table_overlap"]

IMPL_DEFAULT, IMPL_LDS, IMPL_GLOBAL = 0, 1, 2
LDS_ROWS = 1024      # UNET_TABLE_LDS_ROWS
MAX_LABELS = 65535   # UNET_TABLE_MAX_LABELS
REGION_COLUMNS, OVERLAP_COLUMNS = 10, 3
# the columns of a regions row
COUNT, SUM_X, SUM_Y, SUM_Z, MIN_X, MIN_Y, MIN_Z, MAX_X, MAX_Y, MAX_Z = range(10)


def table_scratch_bytes(voxels, n_labels):
    """One size for both calls: the running table, nothing per voxel."""
    return E.size_query(E.lib.unet_table_scratch_bytes, int(voxels), int(n_labels))


def _map(t, name, who, dev=None):
    if not (torch.is_tensor(t) and t.is_cuda and t.dtype in (torch.uint8, torch.uint16) and t.is_contiguous() and t.numel() > 0
            and (dev is None or t.device == dev)):
        raise UNetError("table.%s: %s must be a contiguous uint8 or uint16 device tensor%s"
                        % (who, name, "" if dev is None else " on a's device"))
    return t.data_ptr(), t.element_size()


def _rows(out, n, dev, who):
    if out is None:
        return torch.empty(n, dtype=torch.int64, device=dev)
    if not (torch.is_tensor(out) and out.is_cuda and out.device == dev and out.is_contiguous() and out.dtype == torch.int64 and out.numel() == n):
        raise UNetError("table.%s: out must be a contiguous int64 device tensor of %d entries" % (who, n))
    return out


def regions(labels, n_labels, impl=IMPL_DEFAULT, out=None, scratch=None, stream=None):
    """unet_table_regions on the current stream (or the raw `stream`).  labels: a (D, H, W) uint8 or uint16 device tensor; a value
    above n_labels reads as 0.  Returns int64 {n_labels + 1, 10} on the device (written into `out` when given): per label the
    count, the sums of x, y, z, the minima and the maxima of x, y, z; an empty row holds 0, 0, 0, 0, (W, H, D), -1, -1, -1.  No host
    synchronisation."""
    ptr, nbytes = _map(labels, "labels", "regions")
    if labels.dim() != 3:
        raise UNetError("table.regions: labels must be a (D, H, W) tensor")
    d, h, w = (int(v) for v in labels.shape)
    L = int(n_labels)
    need = table_scratch_bytes(labels.numel(), L)                  # the range checks, before any device work
    rows = _rows(out, (L + 1) * REGION_COLUMNS, labels.device, "regions")
    scratch = E.scratch(scratch, need, labels.device)
    E.check(E.lib.unet_table_regions(ptr, nbytes, w, h, d, L, rows.data_ptr(), int(impl), scratch.data_ptr(), scratch.nbytes, E.stream(labels, stream)))
    return rows.view(L + 1, REGION_COLUMNS)


def overlap(a, b, n_labels, impl=IMPL_DEFAULT, out=None, scratch=None, stream=None):
    """unet_table_overlap on the current stream (or the raw `stream`).  a, b: two label maps of the same element count, uint8 or
    uint16 independently.  Returns int64 {n_labels + 1, 3} on the device: per label |a reads it|, |b reads it|, |both do|.  No host
    synchronisation."""
    pa, ab = _map(a, "a", "overlap")
    pb, bb = _map(b, "b", "overlap", a.device)
    if a.numel() != b.numel():
        raise UNetError("table.overlap: a holds %d voxels, b %d" % (a.numel(), b.numel()))
    L = int(n_labels)
    need = table_scratch_bytes(a.numel(), L)
    rows = _rows(out, (L + 1) * OVERLAP_COLUMNS, a.device, "overlap")
    scratch = E.scratch(scratch, need, a.device)
    E.check(E.lib.unet_table_overlap(pa, ab, pb, bb, a.numel(), L, rows.data_ptr(), int(impl), scratch.data_ptr(), scratch.nbytes, E.stream(a, stream)))
    return rows.view(L + 1, OVERLAP_COLUMNS)


# ---- host arithmetic on the rows, float64 ----------------------------------------------------------------------------------------
def _host_rows(rows, columns, who):
    if torch.is_tensor(rows):
        rows = rows.cpu().numpy()
    rows = np.asarray(rows)
    if rows.ndim != 2 or rows.shape[1] != columns or rows.dtype.kind not in "iu":
        raise UNetError("table.%s: rows must be integers {labels + 1, %d}" % (who, columns))
    return rows.astype(np.int64)


def volumes_mm3(rows, voxel_size):
    """count * (vx * vy * vz) per row of a regions table"""
    rows = _host_rows(rows, REGION_COLUMNS, "volumes_mm3")
    try:
        vs = np.asarray([float(v) for v in voxel_size], np.float64)
    except (TypeError, ValueError):
        raise UNetError("table.volumes_mm3: voxel_size must be three positive finite numbers")
    if vs.shape != (3,) or not (np.all(np.isfinite(vs)) and np.all(vs > 0)):
        raise UNetError("table.volumes_mm3: voxel_size must be three positive finite numbers")
    return rows[:, COUNT].astype(np.float64) * (vs[0] * vs[1] * vs[2])


def centroids(rows):
    """float64 {labels + 1, 3}: (sum x, sum y, sum z) / count in voxel units, NaN for an empty row"""
    rows = _host_rows(rows, REGION_COLUMNS, "centroids")
    n = rows[:, COUNT].astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(n[:, None] > 0, rows[:, SUM_X:SUM_Z + 1].astype(np.float64) / n[:, None], np.nan)


def dice(rows3):
    """float64 {labels + 1}: 2 * both / (|a| + |b|) per row of an overlap table, NaN where neither map holds the label"""
    rows = _host_rows(rows3, OVERLAP_COLUMNS, "dice")
    den = (rows[:, 0] + rows[:, 1]).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(den > 0, 2.0 * rows[:, 2].astype(np.float64) / den, np.nan)
