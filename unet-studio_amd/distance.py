"""Boundary distances of label maps on the device (include/unet_distance.h): how far apart two segmentations' surfaces are.

  metric             a voxel size in mm -> three integer weights and the mm^2 that one unit of the integer squared distance stands for
  transform          the exact squared Euclidean distance transform of one label's surface (or of the label itself), int32
  surface_distances  per label, the two directed lists of surface-to-surface squared distances, sorted, and the surface sizes
  hd, hd95, assd, summary   the host arithmetic on that result, float64, in mm

The reference measures no boundary distance, so these are this project's definitions (parity NOT pinned).  Everything the device
decides is an integer: it is pinned bit for bit to the numpy restatements of tests/test_distance_host.py, with scipy's
distance_transform_edt as a second witness.  The rounding of the weights in `metric` is the module's only approximation, and the
weights used are returned, so every check is exact with respect to them.  IMPL_LDS keeps feature masks and line slabs in LDS,
IMPL_GLOBAL runs the same passes from global memory (the measured baseline and a second witness of the bits)."""
import ctypes as C
import math

import numpy as np
import torch

from . import engine as E
from .engine import UNetError

E._sig("unet_dist_scratch_bytes", C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_size_t))
E._sig("unet_dist_transform", C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
       C.c_int, C.c_void_p, C.c_size_t, C.c_void_p)
E._sig("unet_dist_surface_counts", C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p)
E._sig("unet_dist_gather", C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
       C.c_void_p)
# every symbol include/unet_distance.h declares
EXPORTS = ["unet_dist_scratch_bytes", "unet_dist_transform", "unet_dist_surface_counts", "unet_dist_gather"]

IMPL_DEFAULT, IMPL_LDS, IMPL_GLOBAL = 0, 1, 2
OF_SURFACE, OF_LABEL = 0, 1
INF = 2 ** 31 - 1        # UNET_DIST_INF: the feature set is empty
MAX_LABEL = 65535        # UNET_DIST_MAX_LABEL
LDS_ROWS = 1024          # UNET_DIST_LDS_ROWS
SLAB_MAX_X = 32          # UNET_DIST_SLAB_MAX_X
LDS_MAX_LINE = 2048      # UNET_DIST_LDS_MAX_LINE
MAX_K = 1 << 16          # the finest the weights of `metric` resolve the ratio of two squared voxel sizes
_OF = {"surface": OF_SURFACE, "label": OF_LABEL}


# ---- the metric (host only) ------------------------------------------------------------------------------------------------------
def metric_bound(weights, dims):
    """wx (W-1)^2 + wy (H-1)^2 + wz (D-1)^2 for dims = (W, H, D): a call is refused unless it is below INF"""
    return sum(int(w) * (int(n) - 1) ** 2 for w, n in zip(weights, dims))


def metric(voxel_size, dims):
    """(weights, unit_mm2) for a voxel size (vx, vy, vz) in mm on a grid dims = (W, H, D): the squared distance between two voxels is
    wx dx^2 + wy dy^2 + wz dz^2 units of unit_mm2 mm^2.  Equal sizes: (1, 1, 1) and vs^2.  Otherwise w_a = round(K (vs_a / vs_min)^2)
    and unit_mm2 = vs_min^2 / K, K the largest power of two <= 2^16 for which the largest distance of the grid stays below INF."""
    try:
        vs = [float(v) for v in voxel_size]
        dm = [int(v) for v in dims]
    except (TypeError, ValueError):
        raise UNetError("distance.metric: voxel_size must be three positive finite numbers and dims three positive integers")
    if len(vs) != 3 or not all(math.isfinite(v) and v > 0 for v in vs):
        raise UNetError("distance.metric: voxel_size must be three positive finite numbers")
    if len(dm) != 3 or not all(n > 0 for n in dm):
        raise UNetError("distance.metric: dims must be three positive integers")
    vmin = min(vs)
    if vs[0] == vs[1] == vs[2]:
        if metric_bound((1, 1, 1), dm) >= INF:
            raise UNetError("distance.metric: the grid %s is too large for int32 squared distances" % (tuple(dm),))
        return (1, 1, 1), vmin * vmin
    K = MAX_K
    while K >= 1:
        weights = tuple(max(1, int(round(K * (v / vmin) ** 2))) for v in vs)
        if metric_bound(weights, dm) < INF:
            return weights, vmin * vmin / K
        K //= 2
    raise UNetError("distance.metric: the grid %s is too large for int32 squared distances at voxel size %s" % (tuple(dm), tuple(vs)))


# ---- the device half -------------------------------------------------------------------------------------------------------------
def distance_scratch_bytes(dims):
    """dims = (W, H, D): one int32 per voxel between the passes"""
    w, h, d = (int(v) for v in dims)
    return E.size_query(E.lib.unet_dist_scratch_bytes, w, h, d)


def _map(t, name, who, like=None):
    if not (torch.is_tensor(t) and t.is_cuda and t.dtype in (torch.uint8, torch.uint16) and t.is_contiguous() and t.dim() == 3
            and t.numel() > 0):
        raise UNetError("distance.%s: %s must be a contiguous (D, H, W) uint8 or uint16 device tensor" % (who, name))
    if like is not None and (t.device != like.device or t.shape != like.shape):
        raise UNetError("distance.%s: %s must have a's shape and device" % (who, name))
    return t.data_ptr(), t.element_size()


def _weights(weights, who):
    try:
        w = tuple(int(v) for v in weights)
        ok = len(w) == 3 and all(float(a) == b for a, b in zip(weights, w))
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise UNetError("distance.%s: weights must be three positive integers" % who)
    return w


def transform(labels, label, weights, of="surface", impl=IMPL_DEFAULT, out=None, scratch=None, stream=None):
    """unet_dist_transform on the current stream (or the raw `stream`).  labels: a (D, H, W) uint8 or uint16 device tensor.  Returns the
    int32 (D, H, W) device tensor (written into `out` when given) of the least squared distance, under weights = (wx, wy, wz), to the
    surface of `label` (of="surface") or to any voxel that reads it (of="label"): 0 at a feature voxel, INF everywhere when there is
    none.  No host synchronisation."""
    ptr, nbytes = _map(labels, "labels", "transform")
    if of not in _OF:
        raise UNetError("distance.transform: of must be 'surface' or 'label', got %r" % (of,))
    wx, wy, wz = _weights(weights, "transform")
    d, h, w = (int(v) for v in labels.shape)
    if min(wx, wy, wz) <= 0 or metric_bound((wx, wy, wz), (w, h, d)) >= INF:      # the library's refusal, before anything is allocated
        raise UNetError("distance.transform: weights %s: positive, and wx (W-1)^2 + wy (H-1)^2 + wz (D-1)^2 below 2^31 - 1" % ((wx, wy, wz),))
    need = distance_scratch_bytes((w, h, d))
    if out is None:
        out = torch.empty((d, h, w), dtype=torch.int32, device=labels.device)
    elif not (torch.is_tensor(out) and out.is_cuda and out.device == labels.device and out.is_contiguous() and out.dtype == torch.int32
              and out.numel() == labels.numel()):
        raise UNetError("distance.transform: out must be a contiguous int32 device tensor of %d entries" % labels.numel())
    scratch = E.scratch(scratch, need, labels.device)
    E.check(E.lib.unet_dist_transform(ptr, nbytes, w, h, d, int(label), _OF[of], wx, wy, wz, out.data_ptr(), int(impl), scratch.data_ptr(),
                                      scratch.nbytes, E.stream(labels, stream)))
    return out.view(d, h, w)


def surface_counts(a, b, n_labels, out=None, stream=None):
    """unet_dist_surface_counts: int64 {n_labels + 1, 2} on the device, row l = |S(a, l)|, |S(b, l)|.  No host synchronisation."""
    pa, ab = _map(a, "a", "surface_counts")
    pb, bb = _map(b, "b", "surface_counts", a)
    d, h, w = (int(v) for v in a.shape)
    L = int(n_labels)
    if not 1 <= L <= MAX_LABEL:
        raise UNetError("distance.surface_counts: n_labels must be in [1, 65535], got %d" % L)
    if out is None:
        out = torch.empty((L + 1) * 2, dtype=torch.int64, device=a.device)
    E.check(E.lib.unet_dist_surface_counts(pa, ab, pb, bb, w, h, d, L, out.data_ptr(), E.stream(a, stream)))
    return out.view(L + 1, 2)


def surface_distances(a, b, n_labels, weights, labels=None, impl=IMPL_DEFAULT, scratch=None):
    """The surface-to-surface squared distances of two label maps of one shape, on the current stream.  Per label l of `labels`
    (None: 1..n_labels, refused above 255 labels) whose surface is empty in neither map: the transform to S(b, l) read at S(a, l), and
    the reverse, both sorted ascending.  Returns {"counts": int64 {n_labels + 1, 2} (|S(a, l)|, |S(b, l)|, every row),
    "values": {l: (a_to_b, b_to_a)}} with int64 numpy arrays; a label with an empty surface has no entry in "values".
    Two host synchronisations, however many labels: the counts, and the sorted keys."""
    _map(a, "a", "surface_distances")
    _map(b, "b", "surface_distances", a)
    wts = _weights(weights, "surface_distances")
    L = int(n_labels)
    if not 1 <= L <= MAX_LABEL:
        raise UNetError("distance.surface_distances: n_labels must be in [1, 65535], got %d" % L)
    if labels is None:
        if L > 255:
            raise UNetError("distance.surface_distances: n_labels = %d: pass an explicit list of labels (at most 255 by default)" % L)
        labels = range(1, L + 1)
    labels = [int(l) for l in labels]
    if len(set(labels)) != len(labels) or not all(1 <= l <= L for l in labels):
        raise UNetError("distance.surface_distances: labels must be distinct and in [1, n_labels]")
    d, h, w = (int(v) for v in a.shape)
    dev = a.device
    stream = E.stream(dev)
    scratch = E.scratch(scratch, distance_scratch_bytes((w, h, d)), dev)
    counts = surface_counts(a, b, L).cpu().numpy()                                   # the first synchronisation
    todo = sorted(l for l in labels if counts[l, 0] > 0 and counts[l, 1] > 0)
    result = {"counts": counts, "values": {}}
    # the lists, one after the other: (label, direction) -> [start, start + n); direction 0 is a -> b
    spans, total = [], 0
    for l in todo:
        for direction in (0, 1):
            spans.append((l, direction, total, int(counts[l, direction])))
            total += int(counts[l, direction])
    if not total:
        return result
    values = torch.empty(total, dtype=torch.int32, device=dev)
    cursors = torch.zeros(len(spans), dtype=torch.int64, device=dev)
    dist = torch.empty((d, h, w), dtype=torch.int32, device=dev)
    for k, (l, direction, start, n) in enumerate(spans):
        at, to = (a, b) if direction == 0 else (b, a)
        transform(to, l, wts, "surface", impl, out=dist, scratch=scratch, stream=stream)
        E.check(E.lib.unet_dist_gather(at.data_ptr(), at.element_size(), w, h, d, l, dist.data_ptr(), values.data_ptr() + 4 * start, n,
                                       cursors.data_ptr() + 8 * k, stream))
    # key = (2 l + direction) << 32 | value: one sort orders every list
    ids = torch.tensor([2 * l + direction for l, direction, _, _ in spans], dtype=torch.int64).to(dev, non_blocking=True)
    lens = torch.tensor([n for _, _, _, n in spans], dtype=torch.int64).to(dev, non_blocking=True)
    keys = (torch.repeat_interleave(ids, lens, output_size=total) << 32) | values.to(torch.int64)
    keys = torch.sort(keys).values.cpu().numpy()                                     # the second synchronisation
    lists = {}
    for l, direction, start, n in spans:                                            # spans ascend in key: the sort keeps their places
        part = keys[start:start + n]
        if n and (int(part[0]) >> 32 != 2 * l + direction or int(part[-1]) >> 32 != 2 * l + direction):
            raise UNetError("distance.surface_distances: the gathered lists do not match the counted surfaces")
        lists[(l, direction)] = part & 0xFFFFFFFF
    for l in todo:
        result["values"][l] = (lists[(l, 0)], lists[(l, 1)])
    return result


# ---- host arithmetic on a surface_distances result, float64, mm -------------------------------------------------------------------
def _per_label(result, unit_mm2, who, both):
    try:
        counts = np.asarray(result["counts"])
        values = result["values"]
        unit = float(unit_mm2)
    except (TypeError, KeyError, ValueError):
        raise UNetError("distance.%s: expected a surface_distances result and unit_mm2" % who)
    if counts.ndim != 2 or counts.shape[1] != 2 or counts.dtype.kind not in "iu" or not (math.isfinite(unit) and unit > 0):
        raise UNetError("distance.%s: expected a surface_distances result and a positive finite unit_mm2" % who)
    out = np.full(counts.shape[0], np.nan, np.float64)
    for l in range(1, counts.shape[0]):
        na, nb = int(counts[l, 0]), int(counts[l, 1])
        if l in values:
            ab, ba = (np.sqrt(np.asarray(v, np.int64).astype(np.float64) * unit) for v in values[l])
            out[l] = both(ab, ba)
        elif (na == 0) != (nb == 0):
            out[l] = np.inf                             # exactly one surface is empty
    return out                                          # NaN: both empty, or a label that was not asked for


def hd(result, unit_mm2):
    """float64 {n_labels + 1}: the Hausdorff distance in mm, the larger of the two lists' maxima"""
    return _per_label(result, unit_mm2, "hd", lambda ab, ba: max(ab.max(), ba.max()))


def hd95(result, unit_mm2, percentile=95):
    """float64 {n_labels + 1}: numpy.percentile (linear interpolation) of the two lists concatenated, in mm"""
    q = float(percentile)
    if not 0 <= q <= 100:
        raise UNetError("distance.hd95: percentile must be in [0, 100]")
    return _per_label(result, unit_mm2, "hd95", lambda ab, ba: np.percentile(np.concatenate([ab, ba]), q))


def assd(result, unit_mm2):
    """float64 {n_labels + 1}: the average symmetric surface distance in mm, the mean of the two lists' means"""
    return _per_label(result, unit_mm2, "assd", lambda ab, ba: (ab.mean() + ba.mean()) / 2.0)


def summary(result, unit_mm2):
    """float64 {n_labels + 1, 3}: hd, hd95, assd per label.  NaN where both surfaces are empty (and for row 0 and labels not asked
    for), +inf where exactly one is."""
    return np.stack([hd(result, unit_mm2), hd95(result, unit_mm2), assd(result, unit_mm2)], axis=1)
