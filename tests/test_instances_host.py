"""CPU: the host half of the instances of a label map (include/unet_instances.h, unet-studio_amd/instances.py) -- this file's own
restatements of the header's definitions (`label_ref`, `rows_ref`, `match_ref`, `remove_small_ref`: plain numpy on integers, importing
nothing of the package's kernels) checked on hand-written answers and against scipy.ndimage.label as a second witness, `detection`
on hand-worked cases, the ABI the library exports, argument errors found before any device call, and the text of the lesion report.
No device calls."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
from scipy import ndimage

import unet_studio_amd as U
from unet_studio_amd import instances as IN
from unet_studio_amd import qc as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMPTY = [0, 0, 0, 0, 0]


# ---- the restatements ------------------------------------------------------------------------------------------------------------
def label_ref(labels, n_classes, classes=None):
    """(inst int32 (D, H, W), N): the 6-connected components of equal listed values, numbered 1..N in the order of their smallest
    linear index, 0 elsewhere.  A forest over linear indices: every round jumps all pointers to their roots, then every edge between
    two trees hooks the larger root under the smallest root it touches, until no edge joins two trees."""
    lab = np.asarray(labels).astype(np.int64)
    listed = np.zeros(max(int(n_classes), 1), bool)
    listed[list(range(1, n_classes)) if classes is None else [int(c) for c in classes]] = True
    member = (lab < n_classes) & listed[np.minimum(lab, n_classes - 1)]
    idx = np.arange(lab.size, dtype=np.int64).reshape(lab.shape)
    ea, eb = [], []
    for axis in range(3):
        hi, lo = [slice(None)] * 3, [slice(None)] * 3
        hi[axis], lo[axis] = slice(1, None), slice(0, -1)
        hi, lo = tuple(hi), tuple(lo)
        joined = member[hi] & member[lo] & (lab[hi] == lab[lo])
        ea.append(idx[hi][joined])
        eb.append(idx[lo][joined])
    ea, eb = np.concatenate(ea), np.concatenate(eb)
    parent = idx.reshape(-1).copy()
    while True:
        while True:
            up = parent[parent]
            if (up == parent).all():
                break
            parent = up
        ra, rb = parent[ea], parent[eb]
        apart = ra != rb
        if not apart.any():
            break
        np.minimum.at(parent, np.maximum(ra, rb)[apart], np.minimum(ra, rb)[apart])
    m = member.reshape(-1)
    roots = np.unique(parent[m])                                   # ascending: a root is its component's smallest linear index
    inst = np.zeros(lab.size, np.int32)
    inst[m] = np.searchsorted(roots, parent[m]) + 1
    return inst.reshape(lab.shape), int(roots.size)


def rows_ref(inst, labels, max_instances):
    """int64 {max_instances + 1, 12}: class, voxels, sums of x, y, z, minima, maxima, smallest linear index of the ids 1..max_instances
    of a (D, H, W) instance map; row 0 and every row without an instance hold 0, 0, 0, 0, 0, (W, H, D), -1, -1, -1, -1"""
    inst, labels = np.asarray(inst), np.asarray(labels)
    D, H, W = inst.shape
    M = int(max_instances)
    rows = np.zeros((M + 1, 12), np.int64)
    rows[:, 5:8] = (W, H, D)
    rows[:, 8:12] = -1
    flat = inst.reshape(-1).astype(np.int64)
    lin = np.flatnonzero((flat >= 1) & (flat <= M))
    if lin.size == 0:
        return rows
    order = lin[np.argsort(flat[lin], kind="stable")]               # the voxels grouped by id, ascending linear index inside a group
    present, starts = np.unique(flat[order], return_index=True)
    rows[present, 0] = labels.reshape(-1)[order[starts]]
    rows[present, 1] = np.diff(np.append(starts, order.size))
    for c, v in enumerate((order % W, (order // W) % H, order // (W * H))):
        rows[present, 2 + c] = np.add.reduceat(v, starts)
        rows[present, 5 + c] = np.minimum.reduceat(v, starts)
        rows[present, 8 + c] = np.maximum.reduceat(v, starts)
    rows[present, 11] = order[starts]
    return rows


def match_ref(ia, ib):
    """int64 {P, 3}: (i, j, voxels) of every pair with ia == i > 0 and ib == j > 0 somewhere, sorted by (i, j)"""
    a, b = np.asarray(ia).reshape(-1).astype(np.int64), np.asarray(ib).reshape(-1).astype(np.int64)
    assert a.size == b.size
    both = (a > 0) & (b > 0)
    keys, counts = np.unique((a[both] << 32) | b[both], return_counts=True)
    return np.stack([keys >> 32, keys & 0xFFFFFFFF, counts], axis=1).astype(np.int64).reshape(-1, 3)


def remove_small_ref(labels, inst, rows, min_voxels, n_classes):
    """(labels with the small instances zeroed, removed int64 [n_classes]); an id without a row is left alone"""
    labels, inst = np.asarray(labels), np.asarray(inst).astype(np.int64)
    M = rows.shape[0] - 1
    has_row = (inst >= 1) & (inst <= M)
    small = has_row & (rows[np.where(has_row, inst, 0), 1] < min_voxels)
    gone = labels[small].astype(np.int64)
    return np.where(small, 0, labels).astype(labels.dtype), np.bincount(gone[gone < n_classes], minlength=n_classes).astype(np.int64)


# ---- the restatements on hand-written answers --------------------------------------------------------------------------------------
def test_label_two_classes_touching_stay_two_and_ids_follow_the_first_voxel():
    lab = np.array([[[2, 2, 1, 1],
                     [0, 2, 1, 0],
                     [1, 0, 0, 2]]], np.uint16)                    # (D, H, W) = (1, 3, 4)
    inst, n = label_ref(lab, 3)
    assert n == 4 and inst.dtype == np.int32
    assert inst.tolist() == [[[1, 1, 2, 2], [0, 1, 2, 0], [3, 0, 0, 4]]]
    rows = rows_ref(inst, lab, 5)
    assert rows[0].tolist() == rows[5].tolist() == EMPTY + [4, 3, 1, -1, -1, -1, -1]
    assert rows[1].tolist() == [2, 3, 0 + 1 + 1, 0 + 0 + 1, 0, 0, 0, 0, 1, 1, 0, 0]
    assert rows[2].tolist() == [1, 3, 2 + 3 + 2, 1, 0, 2, 0, 0, 3, 1, 0, 2]
    assert rows[3].tolist() == [1, 1, 0, 2, 0, 0, 2, 0, 0, 2, 0, 8]
    assert rows[4].tolist() == [2, 1, 3, 2, 0, 3, 2, 0, 3, 2, 0, 11]
    # only class 2 listed: class 1 is background, and it splits nothing that was joined
    inst2, n2 = label_ref(lab, 3, [2])
    assert n2 == 2 and inst2.tolist() == [[[1, 1, 0, 0], [0, 1, 0, 0], [0, 0, 0, 2]]]
    # a capacity below N: the rows up to it are those of the full table
    assert rows_ref(inst, lab, 2).tolist() == rows[:3].tolist()
    # values at and above n_classes are no members
    assert label_ref(np.array([[[1, 5, 1]]]), 2)[0].tolist() == [[[1, 0, 2]]]
    assert label_ref(lab, 3, [])[1] == 0


def test_label_a_listed_class_split_by_an_unlisted_one_and_diagonals_do_not_join():
    lab = np.array([[[1, 1, 2, 1, 1]]])
    assert label_ref(lab, 3, [1])[0].tolist() == [[[1, 1, 0, 2, 2]]]
    diag = np.array([[[1, 0], [0, 1]], [[0, 1], [1, 0]]])
    inst, n = label_ref(diag, 2)
    assert n == 4 and inst.reshape(-1).tolist() == [1, 0, 0, 2, 0, 3, 4, 0]
    # a U: the two arms meet late, the id is that of the smallest index
    u = np.array([[[1, 0, 1], [1, 0, 1], [1, 1, 1]]])
    assert label_ref(u, 2)[1] == 1 and label_ref(u, 2)[0].tolist() == u.tolist()


@pytest.mark.parametrize("shape", [(3, 5, 7), (9, 9, 33), (12, 14, 13)])
@pytest.mark.parametrize("density", [0.2, 0.5, 0.8])
def test_label_ref_against_scipy_per_class(shape, density):
    """the same partition, and the same relative order within a class: the rank of an id among its class's ids is scipy's label"""
    rng = np.random.default_rng(int(density * 10) + shape[2])
    lab = np.where(rng.random(shape) < density, rng.integers(1, 4, shape), 0)
    inst, n = label_ref(lab, 4)
    assert n == sum(ndimage.label(lab == c)[1] for c in (1, 2, 3)) and set(np.unique(inst)) == set(range(0, n + 1)) | {0}
    assert ((inst > 0) == (lab > 0)).all()
    for c in (1, 2, 3):
        want, k = ndimage.label(lab == c)
        ids = np.unique(inst[lab == c])
        assert ids.size == k
        assert (np.searchsorted(ids, inst[lab == c]) + 1 == want[lab == c]).all()
    # one binary mask: scipy's numbering itself
    mask = lab > 0
    assert (label_ref(mask.astype(np.int64), 2)[0] == ndimage.label(mask)[0]).all()
    rows = rows_ref(inst, lab, n + 2)
    assert rows[1:n + 1, 1].sum() == mask.sum() and (np.diff(rows[1:n + 1, 11]) > 0).all()
    assert (rows[1:n + 1, 1] == np.bincount(inst.reshape(-1))[1:]).all()
    assert rows[n + 1].tolist() == EMPTY + list(shape[::-1]) + [-1] * 4


def test_match_and_remove_small_on_hand_written_maps():
    ia = np.array([1, 1, 0, 2, 2, 2, 0, 3])
    ib = np.array([1, 2, 2, 2, 2, 0, 0, 0])
    assert match_ref(ia, ib).tolist() == [[1, 1, 1], [1, 2, 1], [2, 2, 2]]
    assert match_ref(ia, np.zeros(8, np.int64)).shape == (0, 3)
    big = match_ref(np.array([2 ** 31 - 1]), np.array([2 ** 31 - 1]))
    assert big.tolist() == [[2 ** 31 - 1, 2 ** 31 - 1, 1]]
    lab = np.array([[[1, 1, 0, 2, 2, 2, 0, 1]]], np.uint16)
    inst, n = label_ref(lab, 3)
    assert n == 3 and inst.reshape(-1).tolist() == ia.tolist()
    out, removed = remove_small_ref(lab, inst, rows_ref(inst, lab, 3), 3, 3)
    assert out.tolist() == [[[0, 0, 0, 2, 2, 2, 0, 0]]] and removed.tolist() == [0, 3, 0] and out.dtype == np.uint16
    # the id above the capacity has no row: left alone
    out, removed = remove_small_ref(lab, inst, rows_ref(inst, lab, 2), 3, 3)
    assert out.tolist() == [[[0, 0, 0, 2, 2, 2, 0, 1]]] and removed.tolist() == [0, 2, 0]
    assert remove_small_ref(lab, inst, rows_ref(inst, lab, 3), 1, 3)[0].tolist() == lab.tolist()


# ---- detection on hand-worked cases ------------------------------------------------------------------------------------------------
def table(*instances):
    """rows {n + 1, 12} from (class, voxels) per instance; the other columns are not read"""
    rows = np.zeros((len(instances) + 1, 12), np.int64)
    for k, (c, n) in enumerate(instances):
        rows[k + 1, :2] = (c, n)
    return rows


def nan_equal(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return got.shape == want.shape and bool(((got == want) | (np.isnan(got) & np.isnan(want))).all())


NAN = float("nan")


def test_detection_an_empty_reference_and_an_empty_prediction():
    d = IN.detection(table(), table((1, 5), (1, 7)), [], 3)
    assert d["n_ref"].tolist() == [0, 0, 0] and d["n_pred"].tolist() == [0, 2, 0] and d["false_pos"].tolist() == [0, 2, 0]
    assert d["detected"].tolist() == d["missed"].tolist() == d["true_pred"].tolist() == [0, 0, 0]
    assert nan_equal(d["sensitivity"], [NAN] * 3) and nan_equal(d["precision"], [NAN, 0.0, NAN]) and nan_equal(d["f1"], [NAN] * 3)
    assert d["instances"].shape == (0, 5) and d["instance_dice"].shape == (0,)
    assert all(d[k].dtype == np.int64 for k in ("n_ref", "n_pred", "detected", "missed", "true_pred", "false_pos", "instances"))
    assert all(d[k].dtype == np.float64 for k in ("sensitivity", "precision", "f1", "instance_dice"))
    d = IN.detection(table((2, 5), (2, 1), (1, 9)), table(), np.zeros((0, 3), np.int64), 3)
    assert d["n_ref"].tolist() == [0, 1, 2] and d["missed"].tolist() == [0, 1, 2] and d["n_pred"].tolist() == [0, 0, 0]
    assert nan_equal(d["sensitivity"], [NAN, 0.0, 0.0]) and nan_equal(d["precision"], [NAN] * 3) and nan_equal(d["f1"], [NAN] * 3)
    assert d["instances"].tolist() == [[1, 2, 5, 0, 0], [2, 2, 1, 0, 0], [3, 1, 9, 0, 0]] and d["instance_dice"].tolist() == [0.0, 0.0, 0.0]


def test_detection_one_prediction_covering_two_references_detects_both():
    d = IN.detection(table((1, 4), (1, 6), (1, 3)), table((1, 20), (1, 2)), [[1, 1, 4], [2, 1, 6]], 2)
    assert d["n_ref"].tolist() == [0, 3] and d["detected"].tolist() == [0, 2] and d["missed"].tolist() == [0, 1]
    assert d["n_pred"].tolist() == [0, 2] and d["true_pred"].tolist() == [0, 1] and d["false_pos"].tolist() == [0, 1]
    s, p = 2 / 3, 1 / 2
    assert d["sensitivity"][1] == s and d["precision"][1] == p and d["f1"][1] == 2.0 * s * p / (s + p)
    assert d["instances"].tolist() == [[1, 1, 4, 1, 4], [2, 1, 6, 1, 6], [3, 1, 3, 0, 0]]
    assert d["instance_dice"].tolist() == [2.0 * 4 / 24, 2.0 * 6 / 26, 0.0]


def test_detection_a_cross_class_overlap_does_not_match_and_f1_is_0_when_both_are_0():
    d = IN.detection(table((1, 5)), table((2, 5)), [[1, 1, 5]], 3)
    assert d["n_ref"].tolist() == [0, 1, 0] and d["n_pred"].tolist() == [0, 0, 1]
    assert d["detected"].tolist() == [0, 0, 0] and d["false_pos"].tolist() == [0, 0, 1]
    assert nan_equal(d["sensitivity"], [NAN, 0.0, NAN]) and nan_equal(d["precision"], [NAN, NAN, 0.0]) and nan_equal(d["f1"], [NAN] * 3)
    assert d["instances"].tolist() == [[1, 1, 5, 0, 0]]
    # one of each in one class, not touching: S = P = 0 and f1 = 0
    d = IN.detection(table((1, 5)), table((1, 5)), [], 2)
    assert d["sensitivity"][1] == 0.0 and d["precision"][1] == 0.0 and d["f1"][1] == 0.0 and np.isnan(d["f1"][0])
    d = IN.detection(table((1, 5)), table((1, 5)), [[1, 1, 1]], 2)
    assert d["f1"][1] == 1.0


def test_detection_min_voxels_removes_one_side_of_a_pair():
    ref, pred, pairs = table((1, 2), (1, 8)), table((1, 10)), [[1, 1, 2]]
    d = IN.detection(ref, pred, pairs, 2, min_voxels=3)
    assert d["n_ref"].tolist() == [0, 1] and d["detected"].tolist() == [0, 0] and d["n_pred"].tolist() == [0, 1]
    assert d["true_pred"].tolist() == [0, 0] and d["false_pos"].tolist() == [0, 1]
    assert d["instances"].tolist() == [[1, 1, 2, 0, 0], [2, 1, 8, 0, 0]]          # every reference instance is listed, the small one unmatched
    d = IN.detection(ref, pred, pairs, 2, min_voxels=2)
    assert d["n_ref"].tolist() == [0, 2] and d["detected"].tolist() == [0, 1] and d["true_pred"].tolist() == [0, 1]
    d = IN.detection(ref, pred, pairs, 2, min_voxels=11)
    assert d["n_ref"].tolist() == d["n_pred"].tolist() == [0, 0] and nan_equal(d["f1"], [NAN, NAN])


def test_detection_iou_exactly_at_the_threshold_and_the_tie_goes_to_the_smaller_id():
    ref, pred = table((1, 2)), table((1, 1))
    pairs = [[1, 1, 1]]                                            # 1 / (2 + 1 - 1) = 0.5
    assert IN.detection(ref, pred, pairs, 2, rule="iou", threshold=0.5)["detected"].tolist() == [0, 1]
    assert IN.detection(ref, pred, pairs, 2, rule="iou", threshold=np.nextafter(0.5, 1.0))["detected"].tolist() == [0, 0]
    assert IN.detection(ref, pred, pairs, 2, rule="any", threshold=0.9)["detected"].tolist() == [0, 1]
    # three predictions on one reference: equal overlaps -> the smaller id; a larger overlap wins over a smaller id
    ref, pred = table((1, 10)), table((1, 3), (1, 3), (1, 4))
    d = IN.detection(ref, pred, [[1, 2, 3], [1, 1, 3], [1, 3, 2]], 2)
    assert d["instances"].tolist() == [[1, 1, 10, 1, 3]] and d["true_pred"].tolist() == [0, 3]
    d = IN.detection(ref, pred, [[1, 1, 2], [1, 2, 3], [1, 3, 3]], 2)
    assert d["instances"].tolist() == [[1, 1, 10, 2, 3]] and d["instance_dice"].tolist() == [2.0 * 3 / 13]
    # under "iou" the best is taken among the matches only: 3 / 10 and 2 / 12 against 0.25
    d = IN.detection(ref, pred, [[1, 1, 3], [1, 3, 2]], 2, rule="iou", threshold=0.25)
    assert d["instances"].tolist() == [[1, 1, 10, 1, 3]] and d["true_pred"].tolist() == [0, 1] and d["false_pos"].tolist() == [0, 2]


def test_detection_argument_errors():
    ref = table((1, 2))
    for kw, msg in ((dict(rule="dice"), "rule"), (dict(rule="iou", threshold=1.5), "threshold"), (dict(n_classes=0), "n_classes")):
        args = dict(rows_ref=ref, rows_pred=ref, pairs=[], n_classes=2)
        args.update(kw)
        with pytest.raises(U.UNetError, match=msg):
            IN.detection(**args)
    with pytest.raises(U.UNetError, match="rows_ref"):
        IN.detection(ref[:, :10], ref, [], 2)
    with pytest.raises(U.UNetError, match="class outside"):
        IN.detection(table((2, 2)), ref, [], 2)
    with pytest.raises(U.UNetError, match="without a row"):
        IN.detection(ref, ref, [[1, 2, 1]], 2)
    with pytest.raises(U.UNetError, match="pairs"):
        IN.detection(ref, ref, np.zeros((1, 2), np.int64), 2)


# ---- the ABI -------------------------------------------------------------------------------------------------------------------------
def test_unet_instances_h_declares_exactly_the_exports_and_the_library_has_them():
    lib = ctypes.CDLL(U.engine.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "unet_instances.h")).read()
    declared = set(re.findall(r"\b(unet_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(IN.EXPORTS) == {"unet_inst_scratch_bytes", "unet_inst_label", "unet_inst_match", "unet_inst_match_scratch_bytes",
                                           "unet_inst_remove_small"}
    for name in sorted(declared):
        assert hasattr(lib, name), "libunet_hip.so does not export " + name
    enums = {k: int(v) for k, v in re.findall(r"UNET_INST_([A-Z_]+) = (\d+)", hdr)}
    assert enums == {"LABEL_DEFAULT": IN.LABEL_DEFAULT, "LABEL_TILED": IN.LABEL_TILED, "LABEL_GLOBAL": IN.LABEL_GLOBAL,
                     "IMPL_DEFAULT": IN.IMPL_DEFAULT, "IMPL_LDS": IN.IMPL_LDS, "IMPL_GLOBAL": IN.IMPL_GLOBAL}
    assert (IN.LABEL_DEFAULT, IN.LABEL_TILED, IN.LABEL_GLOBAL) == (IN.IMPL_DEFAULT, IN.IMPL_LDS, IN.IMPL_GLOBAL) == (0, 1, 2)
    # the labelling impls are those of single_component_label, value for value
    assert (IN.LABEL_DEFAULT, IN.LABEL_TILED, IN.LABEL_GLOBAL) == (U.components.IMPL_DEFAULT, U.components.IMPL_TILED, U.components.IMPL_GLOBAL)
    defines = {k: int(v) for k, v in re.findall(r"#define UNET_INST_([A-Z_]+) (\d+)", hdr)}
    assert defines == {"COLUMNS": IN.COLUMNS, "LDS_ROWS": IN.LDS_ROWS, "LDS_SLOTS": IN.LDS_SLOTS, "MAX_INSTANCES": IN.MAX_INSTANCES,
                       "MAX_PAIRS": IN.MAX_PAIRS}
    assert IN.COLUMNS == 12 and IN.MAX_INSTANCES == 2 ** 31 - 2 and IN.MAX_PAIRS == 2 ** 30
    assert IN.LDS_ROWS * (3 * 8 + 6 * 4) <= 64 * 1024 and IN.LDS_SLOTS * 12 <= 64 * 1024
    assert "this project's" in hdr and "NOT pinned" in hdr
    assert U.instances is IN


def test_the_new_prefix_stays_in_its_header():
    for h in sorted(os.listdir(os.path.join(ROOT, "include"))):
        text = open(os.path.join(ROOT, "include", h)).read().lower()
        if h != "unet_instances.h":
            assert "unet_inst_" not in text, h
        else:                                                      # what the other host tests forbid
            for other in ("unet_dist_", "unet_table_", "unet_reg_", "unet_atlas_", "unet_components_", "unet_preproc_", "unet_tiles_",
                          "unet_space_", "unet_postproc_", "unet_qc_", "unet_feed_"):
                assert other not in text, other


# ---- argument errors, before any device call -------------------------------------------------------------------------------------
def test_scratch_bytes_grow_and_check_their_arguments():
    def mono(sizes):
        return all(a <= b for a, b in zip(sizes, sizes[1:]))
    by_v = [IN.inst_scratch_bytes(v, 4, 100) for v in (1, 4096, 4097, 10 ** 6, 256 ** 3, (1 << 31) - 1)]
    assert mono(by_v) and by_v[-1] >= 8 * ((1 << 31) - 1)          # parent and count per voxel
    by_m = [IN.inst_scratch_bytes(1000, 4, m) for m in (0, 1, 1023, 1024, 65535, 10 ** 6)]
    assert mono(by_m) and by_m[-1] - by_m[0] >= 10 ** 6 * (4 + 24 + 24)
    assert IN.inst_scratch_bytes(1000, 4, 0) >= U.components.components_scratch_bytes(1000, 4)
    by_p = [IN.match_scratch_bytes(p) for p in (0, 1, 32, 33, 65536, 10 ** 6)]
    assert mono(by_p) and by_p[0] >= 64 * 16 and by_p[-1] >= 2 * 10 ** 6 * 16
    for v, c, m, msg in ((0, 4, 1, "voxels"), (1 << 31, 4, 1, "voxels"), (10, 0, 1, "n_classes"), (10, 65537, 1, "n_classes"),
                         (10, 4, -1, "max_instances"), (10, 4, 1 << 31, "max_instances")):
        with pytest.raises(U.UNetError, match=msg):
            IN.inst_scratch_bytes(v, c, m)
    for p in (-1, (1 << 30) + 1):
        with pytest.raises(U.UNetError, match="max_pairs"):
            IN.match_scratch_bytes(p)
    lib = U.engine.lib
    assert lib.unet_inst_scratch_bytes(10, 4, 1, None) != 0 and "null bytes" in lib.unet_last_error().decode()
    assert lib.unet_inst_match_scratch_bytes(10, None) != 0 and "null bytes" in lib.unet_last_error().decode()


P = [ctypes.c_void_p(0x1000 * (i + 1)) for i in range(8)]          # never dereferenced
BIG = 1 << 40


def test_label_argument_errors_need_no_device():
    lib = U.engine.lib

    def call(dims=(4, 4, 4), label=P[0], nc=3, listed=(1, 2), n_listed=None, inst=P[1], rows=P[2], M=5, info=P[3], impl=0, scratch=P[4],
             scratch_bytes=BIG):
        arr = (ctypes.c_uint32 * max(1, len(listed)))(*listed) if listed is not None else None
        rc = lib.unet_inst_label(*dims, label, nc, arr, len(listed) if n_listed is None else n_listed, inst, rows, M, info, impl, scratch,
                                 scratch_bytes, None)
        assert rc != 0
        return lib.unet_last_error().decode()

    assert "dimensions (w, h, d) must be positive" in call(dims=(0, 4, 4)) and "dimensions" in call(dims=(4, -1, 4)) and "dimensions" in call(dims=(4, 4, 0))
    assert "voxels must be in [1, 2^31)" in call(dims=(2048, 1024, 1024))
    assert "n_classes must be in [1, 65536], got 0" in call(nc=0) and "n_classes must be in [1, 65536], got 65537" in call(nc=65537)
    assert "max_instances must be in [0, 2147483646], got -1" in call(M=-1) and "max_instances" in call(M=1 << 31)
    assert "null label" in call(label=None)
    assert "n_listed must not be negative, got -1" in call(n_listed=-1) and "null listed" in call(listed=None, n_listed=2)
    assert "null inst" in call(inst=None) and "inst must be 4-byte aligned" in call(inst=ctypes.c_void_p(0x2002))
    assert "null rows" in call(rows=None) and "rows must be 8-byte aligned" in call(rows=ctypes.c_void_p(0x3004))
    assert "null info" in call(info=None) and "info must be 8-byte aligned" in call(info=ctypes.c_void_p(0x4004))
    assert "unknown impl 3" in call(impl=3) and "unknown impl -1" in call(impl=-1)
    assert "null scratch" in call(scratch=None)
    assert "scratch too small" in call(scratch_bytes=IN.inst_scratch_bytes(64, 3, 5) - 1)
    assert "scratch too small" in call(M=10 ** 6, scratch_bytes=IN.inst_scratch_bytes(64, 3, 5))
    assert "listed class 0 is not in [1, 2]" in call(listed=(1, 0)) and "listed class 3 is not in [1, 2]" in call(listed=(3,))
    assert "listed class 1 is not in [1, 0]" in call(nc=1, listed=(1,))


def test_match_argument_errors_need_no_device():
    lib = U.engine.lib

    def call(ia=P[0], ib=P[1], voxels=64, keys=P[2], counts=P[3], max_pairs=10, info=P[4], impl=0, scratch=P[5], scratch_bytes=BIG):
        rc = lib.unet_inst_match(ia, ib, voxels, keys, counts, max_pairs, info, impl, scratch, scratch_bytes, None)
        assert rc != 0
        return lib.unet_last_error().decode()

    assert "null ia" in call(ia=None) and "null ib" in call(ib=None) and "ib must be 4-byte aligned" in call(ib=ctypes.c_void_p(0x2002))
    assert "voxels must be in [1, 2^31), got 0" in call(voxels=0) and "voxels must be in [1, 2^31)" in call(voxels=1 << 31)
    assert "max_pairs must be in [0, 2^30], got -1" in call(max_pairs=-1) and "max_pairs" in call(max_pairs=(1 << 30) + 1)
    assert "null keys" in call(keys=None) and "keys must be 8-byte aligned" in call(keys=ctypes.c_void_p(0x3004))
    assert "null counts" in call(counts=None) and "counts must be 8-byte aligned" in call(counts=ctypes.c_void_p(0x3004))
    assert "null info" in call(info=None) and "info must be 8-byte aligned" in call(info=ctypes.c_void_p(0x4004))
    assert "unknown impl 3" in call(impl=3) and "unknown impl -1" in call(impl=-1)
    assert "null scratch" in call(scratch=None)
    assert "scratch too small" in call(scratch_bytes=IN.match_scratch_bytes(10) - 1)
    assert "scratch too small" in call(max_pairs=10 ** 6, scratch_bytes=IN.match_scratch_bytes(10))
    # with no room for a pair the two arrays may be absent: the next check is the one that fails
    assert "null info" in call(keys=None, counts=None, max_pairs=0, info=None)


def test_remove_small_argument_errors_need_no_device():
    lib = U.engine.lib

    def call(label=P[0], inst=P[1], voxels=64, rows=P[2], M=5, min_voxels=3, removed=P[3], nc=3):
        rc = lib.unet_inst_remove_small(label, inst, voxels, rows, M, min_voxels, removed, nc, None)
        assert rc != 0
        return lib.unet_last_error().decode()

    assert "null label" in call(label=None) and "label must be 2-byte aligned" in call(label=ctypes.c_void_p(0x1001))
    assert "null inst" in call(inst=None) and "null rows" in call(rows=None) and "rows must be 8-byte aligned" in call(rows=ctypes.c_void_p(0x3004))
    assert "voxels must be in [1, 2^31), got 0" in call(voxels=0) and "voxels" in call(voxels=1 << 31)
    assert "max_instances must be in [0, 2147483646], got -1" in call(M=-1)
    assert "removed must be 4-byte aligned" in call(removed=ctypes.c_void_p(0x4002))
    assert "n_classes must be in [1, 65536], got 0" in call(nc=0) and "n_classes" in call(nc=65537)


def test_wrapper_errors_need_no_device():
    t16, t32 = torch.zeros((2, 2, 2), dtype=torch.uint16), torch.zeros((2, 2, 2), dtype=torch.int32)
    with pytest.raises(U.UNetError, match="device tensor"):
        IN.label(t16, 3)
    with pytest.raises(U.UNetError, match="device tensor"):
        IN.match(t32, t32)
    with pytest.raises(U.UNetError, match="device tensor"):
        IN.remove_small(t16, t32, torch.zeros((1, 12), dtype=torch.int64), 2)
    with pytest.raises(U.UNetError, match="one shape"):
        IN.lesion_scores(t16, torch.zeros((2, 2, 3), dtype=torch.uint16), 3)


# ---- the report ----------------------------------------------------------------------------------------------------------------------
def test_the_lesion_report_text():
    assert Q.lesion_report_path("/models/net.v2.nz") == "/models/net.v2.lesion_report.tsv"
    scores = IN.detection(table((1, 4), (1, 6), (1, 3), (2, 5)), table((1, 20), (1, 2)), [[1, 1, 4], [2, 1, 6]], 3)
    text = Q.format_lesion_report(3, [("/data/a_T1w.nii.gz", "/data/a_label.nii.gz", scores), ("/data/b.nii.gz", "/data/b_seg.nii.gz", None)])
    lines = text.split("\n")
    assert text.endswith("\n") and len(lines) == 4 and lines[3] == ""
    names = ["n_ref", "n_pred", "detected", "false_pos", "sensitivity", "precision", "f1"]
    assert Q.LESION_COLUMNS == tuple(names)
    assert lines[0].split("\t") == ["image", "ground_truth"] + [k + "1" for k in names] + [k + "2" for k in names]
    assert lines[1].split("\t") == ["a_T1w.nii.gz", "a_label.nii.gz", "3", "2", "2", "1", "%.9g" % (2 / 3), "0.5", "%.9g" % (4 / 7),
                                    "1", "0", "0", "0", "0", "nan", "nan"]
    assert lines[2].split("\t") == ["b.nii.gz", "b_seg.nii.gz"] + ["N/A"] * 14
