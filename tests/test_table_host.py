"""CPU: the host half of the tables of a label map (include/unet_table.h, unet-studio_amd/table.py) -- the ABI the library exports,
argument errors found before any device call, the scratch size, this file's own restatements of the header's definitions
(`regions_ref`, `overlap_ref`, plain numpy on integers, importing nothing of the package's kernels) checked on hand-written answers,
the host arithmetic on the rows, register.Atlas's argument errors and EvaluateUNet's refusals around the atlas stage.  No device
calls."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import unet_studio_amd as U
from unet_studio_amd import register as R
from unet_studio_amd import table as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")


# ---- the restatements ------------------------------------------------------------------------------------------------------------
def read_labels(labels, L):
    """a value above L reads as 0"""
    v = np.asarray(labels).astype(np.int64)
    return np.where(v > L, 0, v)


def regions_ref(labels, L):
    """int64 {L + 1, 10}: count, sum x, sum y, sum z, min x, y, z, max x, y, z per label of a (D, H, W) map; an empty row holds
    0, 0, 0, 0, (W, H, D), -1, -1, -1"""
    labels = np.asarray(labels)
    D, H, W = labels.shape
    lab = read_labels(labels, L).reshape(-1)
    z, y, x = (v.reshape(-1).astype(np.int64) for v in np.indices((D, H, W)))
    rows = np.zeros((L + 1, 10), np.int64)
    rows[:, 4:7] = (W, H, D)
    rows[:, 7:10] = -1
    order = np.argsort(lab, kind="stable")                         # the voxels grouped by label: integer reductions per group
    present, starts = np.unique(lab[order], return_index=True)
    rows[present, 0] = np.diff(np.append(starts, lab.size))
    for c, v in enumerate((x, y, z)):
        rows[present, 1 + c] = np.add.reduceat(v[order], starts)
        rows[present, 4 + c] = np.minimum.reduceat(v[order], starts)
        rows[present, 7 + c] = np.maximum.reduceat(v[order], starts)
    return rows


def overlap_ref(a, b, L):
    """int64 {L + 1, 3}: |a reads l|, |b reads l|, |both read l|"""
    la, lb = read_labels(a, L).reshape(-1), read_labels(b, L).reshape(-1)
    assert la.size == lb.size
    return np.stack([np.bincount(v, minlength=L + 1) for v in (la, lb, la[la == lb])], axis=1).astype(np.int64)


# ---- the restatements on hand-written answers ------------------------------------------------------------------------------------------
def test_regions_of_a_single_voxel():
    assert regions_ref(np.array([[[1]]]), 2).tolist() == [[0, 0, 0, 0, 1, 1, 1, -1, -1, -1], [1, 0, 0, 0, 0, 0, 0, 0, 0, 0],
                                                          [0, 0, 0, 0, 1, 1, 1, -1, -1, -1]]
    assert regions_ref(np.array([[[0]]]), 1).tolist() == [[1, 0, 0, 0, 0, 0, 0, 0, 0, 0], [0, 0, 0, 0, 1, 1, 1, -1, -1, -1]]


def test_regions_an_empty_row_holds_the_dims_and_minus_one_and_the_background_is_a_row():
    labels = np.zeros((2, 3, 4), np.uint8)                         # (D, H, W)
    labels[1, 2, 1:4] = 2
    labels[0, 0, 3] = 2
    rows = regions_ref(labels, 3)
    assert rows.dtype == np.int64 and rows.shape == (4, 10)
    assert rows[1].tolist() == rows[3].tolist() == [0, 0, 0, 0, 4, 3, 2, -1, -1, -1]
    # label 2: (3, 0, 0), (1, 2, 1), (2, 2, 1), (3, 2, 1)
    assert rows[2].tolist() == [4, 9, 6, 3, 1, 0, 0, 3, 2, 1]
    assert rows[0].tolist() == [20, 6 * 6 - 9, 6 * 4 - 6, 12 - 3, 0, 0, 0, 3, 2, 1]
    assert rows[:, 0].sum() == labels.size


def test_regions_a_value_above_n_labels_lands_in_row_0():
    labels = np.array([[[1, 7, 2, 65535]]], np.uint16)
    rows = regions_ref(labels, 2)
    assert rows[0].tolist() == [2, 1 + 3, 0, 0, 1, 0, 0, 3, 0, 0]
    assert rows[1, 0] == 1 and rows[2].tolist() == [1, 2, 0, 0, 2, 0, 0, 2, 0, 0]
    assert regions_ref(labels, 7)[7].tolist() == [1, 1, 0, 0, 1, 0, 0, 1, 0, 0]


def test_regions_the_sum_of_x_passes_2_to_the_32():
    rows = regions_ref(np.ones((2, 3, 70000), np.uint8), 1)
    assert rows[1, 1] == 6 * (70000 * 69999 // 2) > 2 ** 32 and rows[1, 0] == 420000 and rows[1, 7] == 69999


def test_overlap_a_label_in_a_only_and_values_above_n_labels():
    a = np.array([1, 1, 2, 3, 9, 0])
    b = np.array([1, 2, 2, 0, 0, 9])
    rows = overlap_ref(a, b, 3)
    assert rows.tolist() == [[2, 3, 2], [2, 1, 1], [1, 2, 1], [1, 0, 0]]       # 3 is in a only; the 9s read 0 and agree with 0
    assert rows[:, 0].sum() == rows[:, 1].sum() == 6
    assert overlap_ref(a, a, 3)[:, 2].tolist() == overlap_ref(a, a, 3)[:, 0].tolist()


# ---- the host arithmetic ---------------------------------------------------------------------------------------------------------------
def test_volumes_centroids_and_dice_on_hand_worked_rows():
    rows = np.array([[20, 27, 18, 9, 0, 0, 0, 3, 2, 1], [0, 0, 0, 0, 4, 3, 2, -1, -1, -1], [4, 9, 6, 3, 1, 0, 0, 3, 2, 1]], np.int64)
    vol = T.volumes_mm3(rows, (0.5, 2, 1.5))
    assert vol.dtype == np.float64 and vol.tolist() == [30.0, 0.0, 6.0]
    c = T.centroids(rows)
    assert c.dtype == np.float64 and c.shape == (3, 3)
    assert c[0].tolist() == [1.35, 0.9, 0.45] and np.isnan(c[1]).all() and c[2].tolist() == [2.25, 1.5, 0.75]
    d = T.dice(np.array([[2, 3, 2], [2, 1, 1], [0, 0, 0], [1, 0, 0]], np.int64))
    assert d.dtype == np.float64 and d[:2].tolist() == [0.8, 2 / 3] and np.isnan(d[2]) and d[3] == 0.0
    assert T.volumes_mm3(torch.from_numpy(rows), (1, 1, 1)).tolist() == [20.0, 0.0, 4.0]
    for bad in ((1, 1), (1, 0, 1), (1, NAN, 1), "abc", (1, -1, 1)):
        with pytest.raises(U.UNetError, match="voxel_size"):
            T.volumes_mm3(rows, bad)
    with pytest.raises(U.UNetError, match="rows"):
        T.centroids(rows[:, :3])
    with pytest.raises(U.UNetError, match="rows"):
        T.dice(rows)
    with pytest.raises(U.UNetError, match="rows"):
        T.volumes_mm3(rows.astype(np.float64), (1, 1, 1))


# ---- the ABI -------------------------------------------------------------------------------------------------------------------------
def test_unet_table_h_declares_exactly_the_exports_and_the_library_has_them():
    lib = ctypes.CDLL(U.engine.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "unet_table.h")).read()
    declared = set(re.findall(r"\b(unet_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(T.EXPORTS) == {"unet_table_scratch_bytes", "unet_table_regions", "unet_table_overlap"}
    for name in sorted(declared):
        assert hasattr(lib, name), "libunet_hip.so does not export " + name
    enums = {k: int(v) for k, v in re.findall(r"UNET_TABLE_([A-Z_]+) = (\d+)", hdr)}
    assert enums == {"IMPL_DEFAULT": T.IMPL_DEFAULT, "IMPL_LDS": T.IMPL_LDS, "IMPL_GLOBAL": T.IMPL_GLOBAL}
    assert (T.IMPL_DEFAULT, T.IMPL_LDS, T.IMPL_GLOBAL) == (0, 1, 2)
    defines = {k: int(v) for k, v in re.findall(r"#define UNET_TABLE_([A-Z_]+) (\d+)", hdr)}
    assert defines == {"MAX_LABELS": T.MAX_LABELS, "LDS_ROWS": T.LDS_ROWS, "REGION_COLUMNS": 10, "OVERLAP_COLUMNS": 3}
    assert T.MAX_LABELS == 65535
    # a row of the LDS table: four 64-bit sums and six 32-bit extremes
    assert T.LDS_ROWS * (4 * 8 + 6 * 4) <= 64 * 1024 and T.LDS_ROWS * 3 * 4 <= 64 * 1024
    assert U.table is T


def test_the_prefixes_stay_apart():
    for h in sorted(os.listdir(os.path.join(ROOT, "include"))):
        text = open(os.path.join(ROOT, "include", h)).read().lower()
        if h != "unet_table.h":
            assert "unet_table_" not in text, h
        else:
            for other in ("unet_reg_", "unet_atlas_", "unet_components_", "unet_preproc_", "unet_tiles_", "unet_space_", "unet_postproc_",
                          "unet_qc_", "unet_feed_"):
                assert other not in text, other


# ---- argument errors, before any device call -------------------------------------------------------------------------------------
def test_scratch_bytes_is_monotone_and_checks_its_arguments():
    def mono(sizes):
        return all(a <= b for a, b in zip(sizes, sizes[1:]))
    by_l = [T.table_scratch_bytes(1000, n) for n in (1, 2, 255, T.LDS_ROWS - 1, T.LDS_ROWS, T.LDS_ROWS + 1, 2035, 65535)]
    assert mono(by_l) and by_l[0] < by_l[-1] and by_l[-1] >= 65536 * (4 * 8 + 6 * 4)
    assert mono([T.table_scratch_bytes(v, 400) for v in (1, 64, 1000, 10 ** 6, 256 ** 3, (1 << 31) - 1)])
    for v, n, msg in ((0, 5, "voxels"), (1 << 31, 5, "voxels"), (10, 0, "n_labels"), (10, 65536, "n_labels"), (10, -1, "n_labels")):
        with pytest.raises(U.UNetError, match=msg):
            T.table_scratch_bytes(v, n)
    rc = U.engine.lib.unet_table_scratch_bytes(10, 5, None)
    assert rc != 0 and "null output" in U.engine.lib.unet_last_error().decode()


P = [ctypes.c_void_p(0x1000 * (i + 1)) for i in range(8)]          # never dereferenced
BIG = 1 << 40


def common_errors(call):
    assert "n_labels must be in [1, 65535], got 0" in call(L=0) and "n_labels must be in [1, 65535], got 65536" in call(L=65536)
    assert "null rows" in call(rows=None) and "rows must be 8-byte aligned" in call(rows=ctypes.c_void_p(0x3004))
    assert "unknown impl 3" in call(impl=3) and "unknown impl -1" in call(impl=-1)
    assert "null scratch" in call(scratch=None)
    assert "scratch too small" in call(scratch_bytes=T.table_scratch_bytes(64, 5) - 1)
    assert "scratch too small" in call(L=65535, scratch_bytes=T.table_scratch_bytes(64, 65000))     # sizes are rounded to 256 B


def test_regions_argument_errors_need_no_device():
    lib = U.engine.lib

    def call(labels=P[0], nbytes=1, dims=(4, 4, 4), L=5, rows=P[1], impl=0, scratch=P[2], scratch_bytes=BIG, ok=False):
        rc = lib.unet_table_regions(labels, nbytes, *dims, L, rows, impl, scratch, scratch_bytes, None)
        assert rc != 0
        return lib.unet_last_error().decode()

    common_errors(call)
    assert "null labels" in call(labels=None)
    assert "label_bytes must be 1 or 2, got 4" in call(nbytes=4) and "label_bytes must be 1 or 2, got 0" in call(nbytes=0)
    assert "dimensions must be positive" in call(dims=(0, 4, 4)) and "dimensions" in call(dims=(4, -1, 4)) and "dimensions" in call(dims=(4, 4, 0))
    assert "below 2^31 voxels" in call(dims=(2048, 1024, 1024))
    # more labels than a uint8 map can hold is allowed: the next check is the one that fails
    assert "null rows" in call(nbytes=1, L=65535, rows=None)


def test_overlap_argument_errors_need_no_device():
    lib = U.engine.lib

    def call(a=P[0], a_bytes=1, b=P[3], b_bytes=2, voxels=64, L=5, rows=P[1], impl=0, scratch=P[2], scratch_bytes=BIG):
        rc = lib.unet_table_overlap(a, a_bytes, b, b_bytes, voxels, L, rows, impl, scratch, scratch_bytes, None)
        assert rc != 0
        return lib.unet_last_error().decode()

    common_errors(call)
    assert "null a" in call(a=None) and "null b" in call(b=None)
    assert "a_bytes must be 1 or 2, got 3" in call(a_bytes=3) and "b_bytes must be 1 or 2, got 4" in call(b_bytes=4)
    assert "voxels must be positive" in call(voxels=0) and "voxels must be positive" in call(voxels=-5)
    assert "below 2^31 voxels" in call(voxels=1 << 31)
    assert "null rows" in call(a_bytes=1, b_bytes=1, L=300, rows=None)


def test_wrapper_errors_need_no_device():
    t8 = torch.zeros((2, 2, 2), dtype=torch.uint8)
    with pytest.raises(U.UNetError, match="device tensor"):
        T.regions(t8, 5)
    with pytest.raises(U.UNetError, match="device tensor"):
        T.overlap(t8, t8, 5)


def test_atlas_record_argument_errors_need_no_device():
    t8, a16 = torch.zeros((2, 2, 2), dtype=torch.uint8), torch.zeros((2, 2, 2), dtype=torch.uint16)
    with pytest.raises(U.UNetError, match="template must be"):
        R.Atlas(t8, (1, 1, 1), a16)
    with pytest.raises(U.UNetError, match="template must be"):
        R.Atlas(None, (1, 1, 1), a16)


# ---- EvaluateUNet's refusals around the atlas stage ------------------------------------------------------------------------------------
class FakeModel:
    """what EvaluateUNet reads of a model before the first upload"""
    in_count, out_count = 1, 3
    dim, voxel_size = (16, 16, 16), (1.0, 1.0, 1.0)
    postproc, preproc, orientation, fov_strategy = "softmax+create_mask+argmax", "", "", "align_top"
    single_component_label = []

    def device(self):
        return "cpu"

    def prepare_for_inference(self, device):
        pass

    def forward(self, x, packs_current=False):
        raise AssertionError("the forward was reached")


def test_evaluate_refuses_before_any_forward(monkeypatch):
    monkeypatch.setattr(torch.cuda, "Stream", lambda *a, **k: None)     # start() makes its copy stream first
    m = FakeModel()
    marker = np.zeros((16, 16, 16), np.float32)
    atlas = R.Atlas.__new__(R.Atlas)                                   # never read: every refusal comes before

    def start(**kw):
        ev = U.EvaluateUNet(m, device="cpu", **kw)
        out = ev.start([[marker]])
        assert ev.aborted and not ev.running and out[0][0] is marker
        return ev.error_msg

    assert start(postproc="model", outputs=("label", "atlas")) == "output atlas needs an atlas"
    assert start(postproc="model", outputs=("regions",)) == "output regions needs an atlas"
    assert "needs a postproc chain" in start(outputs=("atlas",), atlas=atlas)
    assert "needs a postproc chain" in start(postproc="", outputs=("regions",), atlas=atlas)
    assert "output label is not produced by the chain" in start(postproc="softmax+create_mask", outputs=("regions",), atlas=atlas)
    assert "output label is not produced by the chain" in start(postproc="softmax", outputs=("label_prob", "atlas"), atlas=atlas)
    assert "must be a register.Atlas" in start(postproc="model", outputs=("atlas",), atlas=object())
    # without an atlas the names are unknown outputs of a chain's, as before
    ev = U.EvaluateUNet(m, device="cpu", postproc="model", outputs=("label",))
    assert ev.atlas is None and ev.atlas_options is None


@pytest.mark.parametrize("kw,wins", [
    (dict(mirror_axes="q", outputs=("atlas",)), "mirror_axes: unknown axis 'q'"),
    (dict(mirror_swap=("x", [(1, 2)]), outputs=("atlas",)), "mirror_swap needs mirror_axes"),
    (dict(outputs=("label", "agreement"), fov_strategy="spiral"), "output agreement needs mirror_axes"),
    (dict(outputs=("atlas",), postproc="bogusA"), "output atlas needs an atlas"),
    (dict(postproc="bogusA", fov_strategy="spiral"), "unknown command bogusA"),
    (dict(postproc="model", preproc="bogusB", single_component_connectivity=7), "unknown command bogusB"),
    (dict(postproc="model", orientation="bogusC", single_component=[9]), "unknown command bogusC"),
    (dict(postproc="model", single_component=[9], single_component_connectivity=7), "single_component: class 9 is not in [1, 2]"),
    (dict(postproc="model", single_component_connectivity=7, fov_strategy="spiral"),
     "single_component: connectivity must be 6, 18 or 26, got 7"),
    (dict(postproc="model", fov_strategy="spiral", morphology=[("bogus",)]), "unknown fov_strategy spiral"),
    (dict(postproc="model", fov_strategy="tiles", tile_overlap=0.7, morphology=[("bogus",)]),
     "tiles: tile_overlap must be in [0, 0.5), got 0.7"),
    (dict(postproc="model", fov_strategy="tiles", mirror_axes="x", outputs=("label", "agreement"), tile_overlap=0.7),
     "output agreement is not available with fov_strategy tiles"),
])
def test_evaluate_refusal_precedence(monkeypatch, kw, wins):
    """two wrong arguments at once: the refusal that comes first in start()'s order of checks is the one reported"""
    monkeypatch.setattr(torch.cuda, "Stream", lambda *a, **k: None)     # start() makes its copy stream first
    marker = np.zeros((16, 16, 16), np.float32)
    ev = U.EvaluateUNet(FakeModel(), device="cpu", **kw)
    out = ev.start([[marker]])
    assert ev.aborted and not ev.running and out[0][0] is marker
    assert ev.error_msg.startswith(wins), ev.error_msg
