"""The instances of a label map on the device (include/unet_instances.h): a class seen as a set of objects.

  label          every 6-connected component of the listed classes gets a dense id (in the order of its smallest linear index) and a
                 row: class, voxels, coordinate sums, bounding box, smallest linear index
  match          the overlap in voxels of every pair (instance of a, instance of b) that shares a voxel
  remove_small   the instances below a size become 0 in the label map
  detection, lesion_scores   lesion-wise scores per class, host arithmetic in float64 on those tables

The reference stops at voxel counts (evaluate.cpp, qc.cpp), so these are this project's definitions (parity NOT pinned).  Every
device value is an integer: the device is pinned to the numpy restatements of tests/test_instances_host.py bit for bit.
label is the one body of the labelling: with connectivity 18 or 26 (lesion_scores(connectivity=...) too), and for
connectivity.label, it runs unet_conn_label (include/unet_connectivity.h).  Out of
scope: an optimal one-to-one assignment between instances, and wiring either call into EvaluateUNet or the post-processing chain."""
import ctypes as C

import numpy as np
import torch

from . import engine as E
from .components import check_connectivity
from .engine import UNetError

E._sig("unet_inst_scratch_bytes", C.c_int, C.c_int64, C.c_int, C.c_int64, C.POINTER(C.c_size_t))
E._sig("unet_inst_label", C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_uint32), C.c_int, C.c_void_p, C.c_void_p,
       C.c_int64, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p)
E._sig("unet_inst_match_scratch_bytes", C.c_int, C.c_int64, C.POINTER(C.c_size_t))
E._sig("unet_inst_match", C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_void_p,
       C.c_size_t, C.c_void_p)
E._sig("unet_inst_remove_small", C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int, C.c_void_p)
E._sig("unet_conn_label_scratch_bytes", C.c_int, C.c_int64, C.c_int, C.c_int64, C.POINTER(C.c_size_t))
E._sig("unet_conn_label", C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_uint32), C.c_int, C.c_void_p, C.c_void_p,
       C.c_int64, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p)
# every symbol include/unet_instances.h declares
EXPORTS = ["unet_inst_scratch_bytes", "unet_inst_label", "unet_inst_match_scratch_bytes", "unet_inst_match", "unet_inst_remove_small"]

LABEL_DEFAULT, LABEL_TILED, LABEL_GLOBAL = 0, 1, 2   # UNET_INST_LABEL_*: the labelling stage
IMPL_DEFAULT, IMPL_LDS, IMPL_GLOBAL = 0, 1, 2        # UNET_INST_IMPL_*: the pair table
COLUMNS = 12                                         # UNET_INST_COLUMNS
LDS_ROWS, LDS_SLOTS = 1024, 2048                     # UNET_INST_LDS_ROWS, UNET_INST_LDS_SLOTS
MAX_INSTANCES, MAX_PAIRS = 2147483646, 1 << 30       # UNET_INST_MAX_INSTANCES, UNET_INST_MAX_PAIRS
# the columns of a row
CLASS, COUNT, SUM_X, SUM_Y, SUM_Z, MIN_X, MIN_Y, MIN_Z, MAX_X, MAX_Y, MAX_Z, FIRST = range(12)
DEFAULT_MAX_INSTANCES = 65535
DEFAULT_MAX_PAIRS = 65536
KEY_UNUSED = (1 << 63) - 1                           # above every pair (ia < 2^31): the unwritten keys sort behind the written ones


def inst_scratch_bytes(voxels, n_classes, max_instances):
    return E.size_query(E.lib.unet_inst_scratch_bytes, int(voxels), int(n_classes), int(max_instances))


def conn_label_scratch_bytes(voxels, n_classes, max_instances):
    """unet_conn_label_scratch_bytes (connectivity.label_scratch_bytes): the same size under the newer header's name"""
    return E.size_query(E.lib.unet_conn_label_scratch_bytes, int(voxels), int(n_classes), int(max_instances))


def match_scratch_bytes(max_pairs):
    return E.size_query(E.lib.unet_inst_match_scratch_bytes, int(max_pairs))


def _out(t, n, dtype, dev, who, name):
    if t is None:
        return torch.empty(n, dtype=dtype, device=dev)
    if not (torch.is_tensor(t) and t.is_cuda and t.device == dev and t.is_contiguous() and t.dtype == dtype and t.numel() == n):
        raise UNetError("instances.%s: %s must be a contiguous %s device tensor of %d entries" % (who, name, str(dtype).split(".")[1], n))
    return t


def _label_map(labels, who):
    if not (torch.is_tensor(labels) and labels.is_cuda and labels.dtype in (torch.uint8, torch.uint16) and labels.is_contiguous()
            and labels.dim() == 3 and labels.numel() > 0):
        raise UNetError("instances.%s: labels must be a contiguous uint8 or uint16 (D, H, W) device tensor" % who)
    return labels if labels.dtype == torch.uint16 else labels.to(torch.int32).to(torch.uint16)


def label(labels, n_classes, classes=None, max_instances=DEFAULT_MAX_INSTANCES, impl=LABEL_DEFAULT, scratch=None, out=None, stream=None,
          connectivity=6, _who=None):
    """unet_inst_label on the current stream (or the raw `stream`).  labels: a (D, H, W) uint16 device tensor (uint8 is cast).
    classes: the listed classes, None for 1..n_classes-1.  Returns (inst, rows, info) on the device: inst int32 (D, H, W), 0 or the
    dense id of the voxel's 6-connected component; rows int64 {max_instances + 1, 12}: class, voxels, sums of x, y, z, minima, maxima,
    smallest linear index (row 0 and the rows above N are empty: 0, 0, 0, 0, 0, (W, H, D), -1, -1, -1, -1); info int64[2] = (N,
    min(N, max_instances)).  out: (inst, rows, info) to write into.  No host synchronisation.  connectivity: 6 (this header's
    call), 18 or 26 (unet_conn_label: the same outputs, scratch size and impl values).  _who: connectivity.label's message prefix;
    with it unet_conn_label runs at 6 too."""
    c = check_connectivity(connectivity, _who or "instances.label")
    conn = _who is not None or c != 6                             # which header's calls, and whose name the listed classes' message carries
    lab = _label_map(labels, "label")
    D, H, W = (int(v) for v in lab.shape)
    nc, M = int(n_classes), int(max_instances)
    need = (conn_label_scratch_bytes if conn else inst_scratch_bytes)(D * H * W, nc, M)   # the range checks, before any device work
    classes = E.listed_classes("connectivity.label" if conn else "instances.label", classes, nc)
    dev = lab.device
    o = out if out is not None else (None, None, None)
    inst = _out(o[0], D * H * W, torch.int32, dev, "label", "inst")
    rows = _out(o[1], (M + 1) * COLUMNS, torch.int64, dev, "label", "rows")
    info = _out(o[2], 2, torch.int64, dev, "label", "info")
    scratch = E.scratch(scratch, need, dev)
    head = (W, H, D, lab.data_ptr(), nc, E.u32_array(classes), len(classes), inst.data_ptr(), rows.data_ptr(), M, info.data_ptr())
    tail = (int(impl), scratch.data_ptr(), scratch.nbytes, E.stream(lab, stream))
    E.check(E.lib.unet_conn_label(*head, c, *tail) if conn else E.lib.unet_inst_label(*head, *tail))
    return inst.view(D, H, W), rows.view(M + 1, COLUMNS), info


def _inst_map(t, name, who, dev=None):
    if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.int32 and t.is_contiguous() and t.numel() > 0
            and (dev is None or t.device == dev)):
        raise UNetError("instances.%s: %s must be a contiguous int32 device tensor%s" % (who, name, "" if dev is None else " on ia's device"))
    return t


def match_raw(ia, ib, max_pairs, impl=IMPL_DEFAULT, scratch=None, out=None, stream=None):
    """unet_inst_match as it is: (keys int64 [max_pairs], counts int64 [max_pairs], info int64[2]) on the device, the pairs
    (ia << 32) | ib in no particular order, info = (pairs written, overflow).  No host synchronisation."""
    _inst_map(ia, "ia", "match")
    _inst_map(ib, "ib", "match", ia.device)
    if ia.numel() != ib.numel():
        raise UNetError("instances.match: ia holds %d voxels, ib %d" % (ia.numel(), ib.numel()))
    P = int(max_pairs)
    need = match_scratch_bytes(P)
    dev = ia.device
    o = out if out is not None else (None, None, None)
    keys = _out(o[0], P, torch.int64, dev, "match", "keys")
    counts = _out(o[1], P, torch.int64, dev, "match", "counts")
    info = _out(o[2], 2, torch.int64, dev, "match", "info")
    scratch = E.scratch(scratch, need, dev)
    E.check(E.lib.unet_inst_match(ia.data_ptr(), ib.data_ptr(), ia.numel(), keys.data_ptr() if P else None, counts.data_ptr() if P else None, P,
                                  info.data_ptr(), int(impl), scratch.data_ptr(), scratch.nbytes, E.stream(ia, stream)))
    return keys, counts, info


def match(ia, ib, max_pairs=DEFAULT_MAX_PAIRS, impl=IMPL_DEFAULT):
    """The overlap pairs of two instance maps: an int64 array {P, 3} of (i, j, voxels) sorted by (i, j), on the host.  The keys are
    sorted on the device with the counts carried along; reading info back is the one synchronisation.  When more than max_pairs
    distinct pairs exist the call is repeated with twice as many."""
    P = max(1, int(max_pairs))
    while True:
        keys = torch.full((P,), KEY_UNUSED, dtype=torch.int64, device=ia.device)
        keys, counts, info = match_raw(ia, ib, P, impl=impl, out=(keys, None, None))
        keys, order = torch.sort(keys)
        counts = counts[order]
        n, overflow = (int(v) for v in info.cpu())
        if not overflow:
            break
        if P >= MAX_PAIRS:
            raise UNetError("instances.match: more than %d distinct pairs" % MAX_PAIRS)
        P = min(2 * P, MAX_PAIRS)
    k, c = keys[:n].cpu().numpy(), counts[:n].cpu().numpy()
    return np.stack([k >> 32, k & 0xFFFFFFFF, c], axis=1).astype(np.int64).reshape(n, 3)


def remove_small(labels, inst, rows, min_voxels, removed=None, n_classes=0, stream=None):
    """unet_inst_remove_small in place on labels, a uint16 device tensor, with the inst and rows `label` returned for it: a voxel
    whose instance has a row counting fewer than min_voxels voxels becomes 0; an id above the rows' capacity is left alone.
    removed: a uint32 / int32 device tensor of n_classes entries that receives the voxels zeroed per class.  Returns labels."""
    if not (torch.is_tensor(labels) and labels.is_cuda and labels.dtype == torch.uint16 and labels.is_contiguous() and labels.numel() > 0):
        raise UNetError("instances.remove_small: labels must be a contiguous uint16 device tensor")
    _inst_map(inst, "inst", "remove_small", labels.device)
    if inst.numel() != labels.numel():
        raise UNetError("instances.remove_small: labels holds %d voxels, inst %d" % (labels.numel(), inst.numel()))
    if not (torch.is_tensor(rows) and rows.is_cuda and rows.device == labels.device and rows.dtype == torch.int64 and rows.is_contiguous()
            and rows.numel() >= COLUMNS and rows.numel() % COLUMNS == 0):
        raise UNetError("instances.remove_small: rows must be a contiguous int64 device tensor {max_instances + 1, %d}" % COLUMNS)
    if removed is not None and not (torch.is_tensor(removed) and removed.is_cuda and removed.device == labels.device
                                    and removed.dtype in (torch.uint32, torch.int32) and removed.is_contiguous()
                                    and removed.numel() == int(n_classes)):
        raise UNetError("instances.remove_small: removed must be a contiguous uint32 device tensor of n_classes entries on labels' device")
    E.check(E.lib.unet_inst_remove_small(labels.data_ptr(), inst.data_ptr(), labels.numel(), rows.data_ptr(), rows.numel() // COLUMNS - 1,
                                         int(min_voxels), removed.data_ptr() if removed is not None else None, int(n_classes),
                                         E.stream(labels, stream)))
    return labels


# ---- host arithmetic on the tables, float64 --------------------------------------------------------------------------------------
def _host(a, columns, who, name):
    if torch.is_tensor(a):
        a = a.cpu().numpy()
    a = np.asarray(a)
    if a.ndim != 2 or a.shape[1] != columns or a.dtype.kind not in "iu":
        raise UNetError("instances.%s: %s must be integers {n, %d}" % (who, name, columns))
    return a.astype(np.int64)


def detection(rows_ref, rows_pred, pairs, n_classes, rule="any", threshold=0.0, min_voxels=1):
    """Lesion-wise scores from the rows of a reference and of a predicted instance map and their overlap pairs (i, j, voxels), i a
    reference id and j a predicted one.

      eligible   an instance with at least min_voxels voxels (and at least one); a pair of two eligible instances of the same class
      a match    rule "any": every eligible pair; rule "iou": those with voxels / (|i| + |j| - voxels) >= threshold
      per class  (arrays of n_classes entries) n_ref, n_pred: the eligible instances; detected: the reference instances with a match,
                 missed = n_ref - detected; true_pred: the predicted instances with a match, false_pos = n_pred - true_pred;
                 sensitivity = detected / n_ref, precision = true_pred / n_pred (nan on a zero denominator);
                 f1 = 2 S P / (S + P): nan when either is nan, 0 when both are 0
      "instances"  per reference instance 1..n (every row that counts a voxel) int64 {n, 5}: id, class, voxels, the matched
                 prediction with the largest overlap (the smaller id among equal overlaps; 0 without a match), that overlap; and
                 "instance_dice" float64 {n}: 2 overlap / (|i| + |j|) of that pair, 0 without a match

    No one-to-one assignment is made: one prediction covering two references detects both."""
    who = "detection"
    rr, rp = _host(rows_ref, COLUMNS, who, "rows_ref"), _host(rows_pred, COLUMNS, who, "rows_pred")
    if not torch.is_tensor(pairs) and np.asarray(pairs).size == 0:
        pairs = np.zeros((0, 3), np.int64)
    pairs = _host(pairs, 3, who, "pairs")
    nc, mv = int(n_classes), max(1, int(min_voxels))
    if nc < 1:
        raise UNetError("instances.detection: n_classes must be positive")
    if rule not in ("any", "iou"):
        raise UNetError('instances.detection: rule must be "any" or "iou", got %r' % (rule,))
    thr = float(threshold)
    if rule == "iou" and not 0.0 <= thr <= 1.0:
        raise UNetError("instances.detection: threshold must be in [0, 1], got %r" % (threshold,))
    for rows, name in ((rr, "rows_ref"), (rp, "rows_pred")):
        if rows.shape[0] < 1 or (rows[:, CLASS] < 0).any() or (rows[:, CLASS] >= nc).any():
            raise UNetError("instances.detection: %s holds a class outside [0, %d]" % (name, nc - 1))
    i, j, both = pairs[:, 0], pairs[:, 1], pairs[:, 2]
    if pairs.shape[0] and (i.min() < 1 or i.max() >= rr.shape[0] or j.min() < 1 or j.max() >= rp.shape[0]):
        raise UNetError("instances.detection: pairs names an instance without a row")
    el_r, el_p = rr[:, COUNT] >= mv, rp[:, COUNT] >= mv
    si, sj = rr[i, COUNT], rp[j, COUNT]
    ok = el_r[i] & el_p[j] & (rr[i, CLASS] == rp[j, CLASS])
    if rule == "iou":
        with np.errstate(invalid="ignore", divide="ignore"):
            ok &= both.astype(np.float64) / (si + sj - both).astype(np.float64) >= thr
    i, j, both, si, sj = i[ok], j[ok], both[ok], si[ok], sj[ok]
    hit_r, hit_p = np.zeros(rr.shape[0], bool), np.zeros(rp.shape[0], bool)
    hit_r[i] = True
    hit_p[j] = True

    def per_class(rows, mask):
        return np.bincount(rows[mask, CLASS], minlength=nc).astype(np.int64)

    n_ref, n_pred = per_class(rr, el_r), per_class(rp, el_p)
    detected, true_pred = per_class(rr, hit_r), per_class(rp, hit_p)
    with np.errstate(invalid="ignore", divide="ignore"):
        sens = np.where(n_ref > 0, detected / n_ref.astype(np.float64), np.nan)
        prec = np.where(n_pred > 0, true_pred / n_pred.astype(np.float64), np.nan)
        f1 = np.where(sens + prec > 0, 2.0 * sens * prec / (sens + prec), sens + prec)     # nan stays nan, 0 + 0 stays 0
    # per reference instance the matched prediction with the largest overlap, the smaller id on a tie
    ids = np.flatnonzero(rr[:, COUNT] > 0)
    ids = ids[ids > 0]
    best_j, best_n = np.zeros(rr.shape[0], np.int64), np.zeros(rr.shape[0], np.int64)
    order = np.lexsort((j, -both, i))                               # by i, then the largest overlap, then the smaller j
    first = order[np.concatenate([[True], i[order][1:] != i[order][:-1]])] if order.size else order
    best_j[i[first]], best_n[i[first]] = j[first], both[first]
    inst = np.stack([ids, rr[ids, CLASS], rr[ids, COUNT], best_j[ids], best_n[ids]], axis=1).astype(np.int64).reshape(-1, 5)
    den = (rr[ids, COUNT] + rp[best_j[ids], COUNT]).astype(np.float64)
    dice = np.where(best_j[ids] > 0, 2.0 * best_n[ids] / den, 0.0)
    return {"n_ref": n_ref, "n_pred": n_pred, "detected": detected, "missed": n_ref - detected, "true_pred": true_pred,
            "false_pos": n_pred - true_pred, "sensitivity": sens, "precision": prec, "f1": f1, "instances": inst, "instance_dice": dice}


def _label_all(labels, n_classes, classes, max_instances, impl, scratch, connectivity=6):
    """label with rows for every instance: called again with N rows when N exceeds max_instances (reads info back)"""
    inst, rows, info = label(labels, n_classes, classes, max_instances, impl=impl, scratch=scratch, connectivity=connectivity)
    n = int(info[0].item())
    if n > int(max_instances):
        inst, rows, info = label(labels, n_classes, classes, n, impl=impl, scratch=None, connectivity=connectivity)
    return inst, rows[:n + 1]


def lesion_scores(pred, ref, n_classes, classes=None, rule="any", threshold=0.0, min_voxels=1, max_instances=DEFAULT_MAX_INSTANCES,
                  max_pairs=DEFAULT_MAX_PAIRS, impl=LABEL_DEFAULT, match_impl=IMPL_DEFAULT, scratch=None, connectivity=6):
    """`detection` of a predicted label map against a reference one, both (D, H, W) uint8 / uint16 device tensors of one shape: two
    `label` calls, one `match`, then the host arithmetic.  Returns detection's dict.  connectivity: 6, 18 or 26, what joins the
    voxels of one lesion in both maps (26 is what lesion-wise scores in the literature count)."""
    check_connectivity(connectivity, "instances.lesion_scores")
    if not (torch.is_tensor(pred) and torch.is_tensor(ref) and tuple(pred.shape) == tuple(ref.shape)):
        raise UNetError("instances.lesion_scores: pred and ref must be device tensors of one shape")
    inst_r, rows_r = _label_all(ref, n_classes, classes, max_instances, impl, scratch, connectivity)
    inst_p, rows_p = _label_all(pred, n_classes, classes, max_instances, impl, scratch, connectivity)
    pairs = match(inst_r.view(-1), inst_p.view(-1), max_pairs, impl=match_impl)
    return detection(rows_r, rows_p, pairs, n_classes, rule=rule, threshold=threshold, min_voxels=min_voxels)
