"""CPU: the host half of the boundary distances of label maps (include/unet_distance.h, unet-studio_amd/distance.py) -- the ABI the
library exports, argument errors found before any device call (the metric bound at its edge), `metric`, this file's own restatements
of the header's definitions (`surface_ref`, `transform_ref`, `surface_distances_ref`: plain numpy on integers, importing nothing of the
package's kernels) checked against scipy.ndimage as an independent witness, and the host arithmetic (hd, hd95, assd) against the
scipy formulation MedPy's metric.binary uses with connectivity 1.  No device calls."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
from scipy import ndimage

import unet_studio_amd as U
from unet_studio_amd import distance as DS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = 2 ** 31 - 1
BIG = 1 << 62                                                      # stands for INF inside the restatement's int64 sums


# ---- the restatements ------------------------------------------------------------------------------------------------------------
def read_labels(labels, L=None):
    """a value above L reads as 0"""
    v = np.asarray(labels).astype(np.int64)
    return v if L is None else np.where(v > L, 0, v)


def surface_ref(mask):
    """the voxels of a (D, H, W) mask with a 6-neighbour outside it, or on a face of the volume"""
    mask = np.asarray(mask, bool)
    p = np.pad(mask, 1, constant_values=False)
    inner = (p[:-2, 1:-1, 1:-1] & p[2:, 1:-1, 1:-1] & p[1:-1, :-2, 1:-1] & p[1:-1, 2:, 1:-1] & p[1:-1, 1:-1, :-2] & p[1:-1, 1:-1, 2:])
    return mask & ~inner


def features_ref(labels, label, of):
    mask = read_labels(labels) == label
    assert of in ("surface", "label")
    return surface_ref(mask) if of == "surface" else mask


def _axis_pass(g, w, axis):
    """min_i (w (p - i)^2 + g[i]) along an axis, a brute minimum in int64; BIG entries stay out of every sum that matters"""
    g = np.moveaxis(g, axis, -1)
    n = g.shape[-1]
    i = np.arange(n, dtype=np.int64)
    cost = w * (i[:, None] - i[None, :]) ** 2                      # [p, i]
    out = np.empty_like(g)
    for p in range(n):                                             # a row at a time: the memory of one volume
        out[..., p] = np.min(np.where(g >= BIG, BIG, g + cost[p]), axis=-1)
    return np.moveaxis(out, -1, axis)


def transform_of_features_ref(features, weights):
    """int32 (D, H, W): per voxel the least wx dx^2 + wy dy^2 + wz dz^2 to a voxel of `features`; INF everywhere when there is none"""
    wx, wy, wz = (int(v) for v in weights)
    g = np.where(np.asarray(features, bool), np.int64(0), np.int64(BIG))
    for w, axis in ((wx, 2), (wy, 1), (wz, 0)):
        g = _axis_pass(g, w, axis)
    assert ((g < INF) | (g >= BIG)).all()
    return np.where(g >= BIG, INF, g).astype(np.int32)


def transform_ref(labels, label, weights, of="surface"):
    return transform_of_features_ref(features_ref(labels, label, of), weights)


def surface_distances_ref(a, b, L, weights, labels=None):
    """{"counts": int64 {L + 1, 2}, "values": {l: (a_to_b, b_to_a)}}: the definitions of include/unet_distance.h restated"""
    ra, rb = read_labels(a, L), read_labels(b, L)
    counts = np.zeros((L + 1, 2), np.int64)
    for l in range(L + 1):
        if (ra == l).any() or (rb == l).any():
            counts[l] = int(surface_ref(ra == l).sum()), int(surface_ref(rb == l).sum())
    values = {}
    for l in (range(1, L + 1) if labels is None else labels):
        if counts[l, 0] and counts[l, 1]:
            sa, sb = surface_ref(ra == l), surface_ref(rb == l)
            values[l] = (np.sort(transform_of_features_ref(sb, weights)[sa].astype(np.int64)),
                         np.sort(transform_of_features_ref(sa, weights)[sb].astype(np.int64)))
    return {"counts": counts, "values": values}


# ---- the scipy witnesses -----------------------------------------------------------------------------------------------------------
def scipy_transform(features, weights):
    wx, wy, wz = weights
    return np.rint(ndimage.distance_transform_edt(~features, sampling=np.sqrt([wz, wy, wx])) ** 2)


def scipy_surface(mask):
    return mask & ~ndimage.binary_erosion(mask, ndimage.generate_binary_structure(3, 1), border_value=0)


def scipy_metrics(ma, mb, vs_zyx):
    """(hd, hd95, assd) as MedPy's metric.binary forms them with connectivity 1"""
    sa, sb = scipy_surface(ma), scipy_surface(mb)
    if not sa.any() and not sb.any():
        return (np.nan,) * 3
    if not sa.any() or not sb.any():
        return (np.inf,) * 3
    ab = ndimage.distance_transform_edt(~sb, sampling=vs_zyx)[sa]
    ba = ndimage.distance_transform_edt(~sa, sampling=vs_zyx)[sb]
    return max(ab.max(), ba.max()), np.percentile(np.hstack([ab, ba]), 95), (ab.mean() + ba.mean()) / 2


def blobs(rng, shape, p=0.45):
    """a smooth random mask: runs and holes at every scale the small shapes have"""
    return ndimage.uniform_filter(rng.random(shape), 3, mode="nearest") > p


def ball(shape, centre, radius):
    z, y, x = np.indices(shape)
    return (x - centre[0]) ** 2 + (y - centre[1]) ** 2 + (z - centre[2]) ** 2 <= radius ** 2


# ---- the restatements against scipy ------------------------------------------------------------------------------------------------
def test_surface_ref_is_mask_minus_its_6_connected_erosion():
    rng = np.random.default_rng(0)
    for shape in ((1, 1, 1), (1, 1, 9), (3, 5, 7), (9, 11, 13)):
        for p in (0.0, 0.3, 0.5, 2.0):
            mask = blobs(rng, shape, p)
            assert (surface_ref(mask) == scipy_surface(mask)).all()
    solid = np.ones((4, 5, 6), bool)
    assert surface_ref(solid).sum() == 4 * 5 * 6 - 2 * 3 * 4          # the faces of the volume are surface
    assert surface_ref(solid)[0].all() and not surface_ref(solid)[1:3, 1:4, 1:5].any()


@pytest.mark.parametrize("shape,weights", [((9, 11, 13), (1, 1, 1)), ((7, 20, 33), (4, 9, 25)), ((5, 6, 7), (1024, 1531, 9216))])
def test_transform_ref_equals_scipy_edt_squared(shape, weights):
    rng = np.random.default_rng(shape[2])
    labels = np.where(blobs(rng, shape), 2, rng.integers(0, 2, shape) * 3)
    one = np.zeros(shape, np.int64)
    one[shape[0] - 1, 0, shape[2] - 1] = 2
    for lab in (labels, one):
        for of in ("surface", "label"):
            features = features_ref(lab, 2, of)
            assert features.any()
            got = transform_ref(lab, 2, weights, of)
            assert got.dtype == np.int32 and (got == scipy_transform(features, weights)).all()
            assert (got[features] == 0).all() and (got[~features] > 0).all()
    assert DS.metric_bound(weights, shape[::-1]) < INF


def test_transform_ref_of_an_empty_feature_set_is_inf_everywhere():
    labels = np.ones((3, 4, 5), np.int64)
    for of in ("surface", "label"):
        got = transform_ref(labels, 2, (4, 9, 25), of)
        assert got.dtype == np.int32 and (got == INF).all()
    # a solid label: its surface is the faces of the volume
    assert transform_ref(labels, 1, (1, 1, 1), "label").max() == 0 and transform_ref(labels, 1, (1, 1, 1), "surface")[1, 1:3, 2].tolist() == [1, 1]


# ---- metric --------------------------------------------------------------------------------------------------------------------------
def test_metric_equal_sizes_and_the_power_of_two_rule():
    assert DS.metric((2, 2, 2), (16, 16, 16)) == ((1, 1, 1), 4.0)
    assert DS.metric((0.7, 0.7, 0.7), (192, 224, 192)) == ((1, 1, 1), 0.7 * 0.7)
    dims = (512, 512, 300)
    for vs in ((1, 1, 3), (0.8, 0.8, 2.2)):
        weights, unit = DS.metric(vs, dims)
        vmin = min(vs)
        K = weights[0]                                              # the smallest size gets exactly K
        assert K & (K - 1) == 0 and 1 <= K <= DS.MAX_K and unit == vmin * vmin / K
        assert weights == tuple(int(round(K * (v / vmin) ** 2)) for v in vs)
        assert DS.metric_bound(weights, dims) < INF
        # the next power of two does not fit (or is past the finest allowed)
        assert K == DS.MAX_K or DS.metric_bound(tuple(int(round(2 * K * (v / vmin) ** 2)) for v in vs), dims) >= INF
    assert DS.metric((1, 1, 3), dims) == ((1024, 1024, 9216), 1.0 / 1024)
    assert DS.metric((0.8, 0.8, 2.2), dims)[0] == (1024, 1024, 7744)
    assert DS.metric((1, 1, 3), (24, 22, 20)) == ((65536, 65536, 589824), 1.0 / 65536)       # K stops at 2^16
    assert DS.metric((3, 1, 2), (10, 10, 10))[0] == (589824, 65536, 262144)


def test_metric_refusals():
    for bad in ((1, 1), (1, 0, 1), (1, float("nan"), 1), (1, float("inf"), 1), "abc", (1, -1, 1), None):
        with pytest.raises(U.UNetError, match="voxel_size"):
            DS.metric(bad, (8, 8, 8))
    for bad in ((8, 8), (8, 0, 8), (8, -1, 8)):
        with pytest.raises(U.UNetError, match="dims"):
            DS.metric((1, 1, 1), bad)
    with pytest.raises(U.UNetError, match="too large"):
        DS.metric((1, 1, 1), (40000, 40000, 2))
    with pytest.raises(U.UNetError, match="too large"):
        DS.metric((1, 1, 1.5), (33000, 33000, 2))
    assert DS.metric((1, 1, 1.5), (20000, 20000, 2))[0] == (2, 2, 4)           # K = 2: 1.5^2 * 2 = 4.5 rounds to 4


# ---- surface_distances_ref and the host metrics against the scipy formulation ----------------------------------------------------------
def two_maps():
    """label 1: two overlapping balls; 2: in a only; 3: in b only; 4: in neither; 5: a single voxel in each"""
    shape = (20, 22, 24)
    a, b = np.zeros(shape, np.int64), np.zeros(shape, np.int64)
    a[ball(shape, (9, 10, 9), 6)] = 1
    b[ball(shape, (12, 11, 10), 7)] = 1
    a[1:4, 1:3, 18:23] = 2
    b[15:19, 17:21, 1:4] = 3
    a[18, 1, 1] = 5
    b[1, 20, 22] = 5
    return a, b


@pytest.mark.parametrize("vs", [(1.0, 1.0, 1.0), (1.0, 1.0, 3.0), (0.5, 0.5, 0.5)])
def test_host_metrics_equal_the_scipy_formulation(vs):
    a, b = two_maps()
    L = 5
    weights, unit = DS.metric(vs, a.shape[::-1])
    res = surface_distances_ref(a, b, L, weights)
    assert sorted(res["values"]) == [1, 5] and res["counts"].dtype == np.int64 and res["counts"].shape == (L + 1, 2)
    assert res["counts"][2].tolist() == [30, 0] and res["counts"][3, 0] == 0 and res["counts"][3, 1] == 4 * 4 * 3 - 2 * 2
    assert res["counts"][4].tolist() == [0, 0] and res["counts"][5].tolist() == [1, 1]
    for l, (ab, ba) in res["values"].items():
        assert ab.dtype == ba.dtype == np.int64 and (np.diff(ab) >= 0).all() and (np.diff(ba) >= 0).all()
        assert ab.size == res["counts"][l, 0] and ba.size == res["counts"][l, 1]
    table = DS.summary(res, unit)
    assert table.dtype == np.float64 and table.shape == (L + 1, 3)
    assert np.isnan(table[0]).all() and np.isnan(table[4]).all() and np.isinf(table[2]).all() and np.isinf(table[3]).all()
    for l in range(1, L + 1):
        want = scipy_metrics(a == l, b == l, vs[::-1])
        # float64 on both sides: sqrt(integer * unit) against scipy's sqrt of a sum of squares, a few roundings apart
        np.testing.assert_allclose(table[l], want, rtol=1e-12, atol=0, equal_nan=True)
    assert np.array_equal(table[:, 0], DS.hd(res, unit), equal_nan=True) and np.array_equal(table[:, 2], DS.assd(res, unit), equal_nan=True)
    assert np.array_equal(table[:, 1], DS.hd95(res, unit), equal_nan=True)
    assert table[1, 2] < table[1, 1] <= table[1, 0] and table[5, 0] == table[5, 1] == table[5, 2]
    # labels not asked for read NaN, whatever their counts
    part = surface_distances_ref(a, b, L, weights, labels=[5])
    assert sorted(part["values"]) == [5] and (part["counts"] == res["counts"]).all()
    assert np.isnan(DS.summary(part, unit)[1]).all() and (DS.summary(part, unit)[5] == table[5]).all()


def test_percentile_of_one_element_nan_and_inf_rules():
    one = {"counts": np.array([[0, 0], [1, 1], [0, 0], [3, 0], [0, 2]], np.int64),
           "values": {1: (np.array([9], np.int64), np.array([9], np.int64))}}
    for f in (DS.hd, DS.hd95, DS.assd):
        got = f(one, 0.25)
        assert got.dtype == np.float64 and got[1] == 1.5 and np.isnan(got[0]) and np.isnan(got[2]) and got[3] == got[4] == np.inf
    lone = {"counts": np.array([[0, 0], [1, 2]], np.int64), "values": {1: (np.array([16], np.int64), np.array([0, 4], np.int64))}}
    assert DS.hd(lone, 1.0)[1] == 4.0 and DS.assd(lone, 1.0)[1] == (4.0 + 1.0) / 2
    assert DS.hd95(lone, 1.0)[1] == np.percentile([4.0, 0.0, 2.0], 95) and DS.hd95(lone, 1.0, 50)[1] == 2.0 and DS.hd95(lone, 1.0, 100)[1] == 4.0
    assert DS.hd95({"counts": lone["counts"], "values": {1: (np.array([16], np.int64), np.array([], np.int64))}}, 1.0)[1] == 4.0
    with pytest.raises(U.UNetError, match="percentile"):
        DS.hd95(lone, 1.0, 101)
    for bad_unit in (0, -1, float("nan")):
        with pytest.raises(U.UNetError, match="unit_mm2"):
            DS.hd(lone, bad_unit)
    with pytest.raises(U.UNetError, match="surface_distances result"):
        DS.summary({"counts": np.zeros((3, 3), np.int64), "values": {}}, 1.0)


# ---- the ABI -------------------------------------------------------------------------------------------------------------------------
def test_unet_distance_h_declares_exactly_the_exports_and_the_library_has_them():
    lib = ctypes.CDLL(U.engine.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "unet_distance.h")).read()
    declared = set(re.findall(r"\b(unet_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(DS.EXPORTS) == {"unet_dist_scratch_bytes", "unet_dist_transform", "unet_dist_surface_counts", "unet_dist_gather"}
    for name in sorted(declared):
        assert hasattr(lib, name), "libunet_hip.so does not export " + name
    enums = {k: int(v) for k, v in re.findall(r"UNET_DIST_([A-Z_]+) = (\d+)", hdr)}
    assert enums == {"IMPL_DEFAULT": DS.IMPL_DEFAULT, "IMPL_LDS": DS.IMPL_LDS, "IMPL_GLOBAL": DS.IMPL_GLOBAL, "OF_SURFACE": DS.OF_SURFACE,
                     "OF_LABEL": DS.OF_LABEL}
    assert (DS.IMPL_DEFAULT, DS.IMPL_LDS, DS.IMPL_GLOBAL) == (0, 1, 2) and (DS.OF_SURFACE, DS.OF_LABEL) == (0, 1)
    defines = {k: int(v) for k, v in re.findall(r"#define UNET_DIST_([A-Z_]+) (\d+)", hdr)}
    assert defines == {"INF": DS.INF, "MAX_LABEL": DS.MAX_LABEL, "LDS_ROWS": DS.LDS_ROWS, "SLAB_MAX_X": DS.SLAB_MAX_X,
                       "LDS_MAX_LINE": DS.LDS_MAX_LINE}
    assert DS.INF == INF and DS.MAX_LABEL == 65535
    assert DS.LDS_MAX_LINE * 8 * 4 <= 64 * 1024 and DS.LDS_ROWS * 2 * 4 <= 64 * 1024 and DS.SLAB_MAX_X >= 8
    assert U.distance is DS


def test_the_new_prefix_stays_in_its_header():
    for h in sorted(os.listdir(os.path.join(ROOT, "include"))):
        text = open(os.path.join(ROOT, "include", h)).read().lower()
        if h != "unet_distance.h":
            assert "unet_dist_" not in text, h
        else:                                                      # what the other host tests forbid
            for other in ("unet_table_", "unet_reg_", "unet_atlas_", "unet_components_", "unet_preproc_", "unet_tiles_", "unet_space_",
                          "unet_postproc_", "unet_qc_", "unet_feed_"):
                assert other not in text, other


# ---- argument errors, before any device call -------------------------------------------------------------------------------------
P = [ctypes.c_void_p(0x1000 * (i + 1)) for i in range(8)]          # never dereferenced
HUGE = 1 << 40


def test_scratch_bytes_holds_a_volume_and_checks_its_arguments():
    sizes = [DS.distance_scratch_bytes(dims) for dims in ((1, 1, 1), (7, 5, 3), (64, 64, 64), (192, 224, 192), (2047, 1024, 1024))]
    assert all(a < b for a, b in zip(sizes, sizes[1:])) and sizes[3] >= 4 * 192 * 224 * 192 and sizes[0] <= 1024
    for dims, msg in (((0, 4, 4), "dimensions"), ((4, -1, 4), "dimensions"), ((4, 4, 0), "dimensions"), ((2048, 1024, 1024), "2\\^31 voxels")):
        with pytest.raises(U.UNetError, match=msg):
            DS.distance_scratch_bytes(dims)
    rc = U.engine.lib.unet_dist_scratch_bytes(4, 4, 4, None)
    assert rc != 0 and "null bytes" in U.engine.lib.unet_last_error().decode()


def test_transform_argument_errors_need_no_device():
    lib = U.engine.lib

    def call(labels=P[0], nbytes=1, dims=(4, 4, 4), label=1, of=0, weights=(1, 1, 1), out=P[1], impl=0, scratch=P[2], scratch_bytes=HUGE):
        rc = lib.unet_dist_transform(labels, nbytes, *dims, label, of, *weights, out, impl, scratch, scratch_bytes, None)
        assert rc != 0
        return lib.unet_last_error().decode()

    assert "null labels" in call(labels=None) and "null out" in call(out=None) and "null scratch" in call(scratch=None)
    assert "label_bytes must be 1 or 2, got 4" in call(nbytes=4) and "label_bytes must be 1 or 2, got 0" in call(nbytes=0)
    assert "dimensions" in call(dims=(0, 4, 4)) and "dimensions" in call(dims=(4, -1, 4)) and "dimensions" in call(dims=(4, 4, 0))
    assert "below 2^31 voxels" in call(dims=(2048, 1024, 1024))
    assert "label must be in [1, 65535], got 0" in call(label=0) and "label must be in [1, 65535], got 65536" in call(label=65536)
    assert "unknown of 2" in call(of=2) and "unknown of -1" in call(of=-1)
    for bad in ((0, 1, 1), (1, -2, 1), (1, 1, 0)):
        assert "weights (wx, wy, wz) must be positive" in call(weights=bad)
    assert "out must be 4-byte aligned" in call(out=ctypes.c_void_p(0x3002))
    assert "unknown impl 3" in call(impl=3) and "unknown impl -1" in call(impl=-1)
    assert "scratch too small" in call(scratch_bytes=DS.distance_scratch_bytes((4, 4, 4)) - 1)
    assert "scratch too small" in call(dims=(5, 4, 4), scratch_bytes=DS.distance_scratch_bytes((4, 4, 4)))
    # the metric bound at its edge: the largest weights that pass reach the next check, one more does not
    bound = "must stay below 2^31 - 1"
    assert "null out" in call(dims=(1001, 1, 1), weights=(2147, 1, 1), out=None)                     # 2147 * 10^6 < 2^31 - 1
    assert bound in call(dims=(1001, 1, 1), weights=(2148, 1, 1), out=None)
    assert "null out" in call(dims=(1001, 1, 1), weights=(2147, INF, INF), out=None)                # a line of one voxel adds nothing
    assert "null out" in call(dims=(2, 2, 2), weights=(INF - 3, 1, 1), out=None) and bound in call(dims=(2, 2, 2), weights=(INF - 2, 1, 1), out=None)
    assert bound in call(dims=(2, 2, 2), weights=(INF, INF, INF), out=None)
    assert (INF - 1 - 160) // 36 == 59652319
    assert "null out" in call(dims=(3, 5, 7), weights=(4, 9, 59652319), out=None)                   # 16 + 144 + 36 wz < 2^31 - 1
    assert bound in call(dims=(3, 5, 7), weights=(4, 9, 59652320), out=None)
    assert 46340 ** 2 < INF <= 46341 ** 2
    assert "null out" in call(dims=(46341, 1, 1), weights=(1, 1, 1), out=None) and bound in call(dims=(1, 46342, 1), weights=(1, 1, 1), out=None)


def test_surface_counts_and_gather_argument_errors_need_no_device():
    lib = U.engine.lib

    def counts(a=P[0], a_bytes=1, b=P[3], b_bytes=2, dims=(4, 4, 4), L=5, rows=P[1]):
        rc = lib.unet_dist_surface_counts(a, a_bytes, b, b_bytes, *dims, L, rows, None)
        assert rc != 0
        return lib.unet_last_error().decode()

    assert "null a" in counts(a=None) and "null b" in counts(b=None) and "null rows" in counts(rows=None)
    assert "a_bytes must be 1 or 2, got 3" in counts(a_bytes=3) and "b_bytes must be 1 or 2, got 4" in counts(b_bytes=4)
    assert "dimensions" in counts(dims=(4, 0, 4)) and "below 2^31 voxels" in counts(dims=(2048, 1024, 1024))
    assert "n_labels must be in [1, 65535], got 0" in counts(L=0) and "n_labels must be in [1, 65535], got 65536" in counts(L=65536)
    assert "rows must be 8-byte aligned" in counts(rows=ctypes.c_void_p(0x3004))
    assert "null rows" in counts(a_bytes=1, b_bytes=1, L=300, rows=None)        # more labels than a uint8 map can hold is allowed

    def gather(at=P[0], at_bytes=2, dims=(4, 4, 4), label=1, dist=P[1], values=P[2], capacity=10, cursor=P[3]):
        rc = lib.unet_dist_gather(at, at_bytes, *dims, label, dist, values, capacity, cursor, None)
        assert rc != 0
        return lib.unet_last_error().decode()

    assert "null at" in gather(at=None) and "null dist" in gather(dist=None) and "null values" in gather(values=None)
    assert "null cursor" in gather(cursor=None) and "at_bytes must be 1 or 2, got 0" in gather(at_bytes=0)
    assert "dimensions" in gather(dims=(-4, 4, 4)) and "below 2^31 voxels" in gather(dims=(2048, 1024, 1024))
    assert "label must be in [1, 65535], got 0" in gather(label=0) and "label must be in [1, 65535], got 70000" in gather(label=70000)
    assert "capacity must not be negative, got -1" in gather(capacity=-1)
    assert "dist must be 4-byte aligned" in gather(dist=ctypes.c_void_p(0x3002)) and "values must be 4-byte aligned" in gather(values=ctypes.c_void_p(0x3001))
    assert "cursor must be 8-byte aligned" in gather(cursor=ctypes.c_void_p(0x3004))


def test_wrapper_errors_need_no_device():
    t8 = torch.zeros((2, 2, 2), dtype=torch.uint8)
    with pytest.raises(U.UNetError, match="device tensor"):
        DS.transform(t8, 1, (1, 1, 1))
    with pytest.raises(U.UNetError, match="device tensor"):
        DS.surface_counts(t8, t8, 5)
    with pytest.raises(U.UNetError, match="device tensor"):
        DS.surface_distances(t8, t8, 5, (1, 1, 1))


def test_the_surface_report_text():
    from unet_studio_amd import qc as Q
    table = np.array([[np.nan] * 3, [1.5, 1.25, 1 / 3], [np.inf] * 3, [np.nan] * 3])
    text = Q.format_surface_report(4, [("/x/img1.nii.gz", "/y/lab1.nii.gz", table), ("img2", "lab2", None)])
    assert text == ("image\tground_truth\thd1\thd951\tassd1\thd2\thd952\tassd2\thd3\thd953\tassd3\n"
                    "img1.nii.gz\tlab1.nii.gz\t1.5\t1.25\t0.333333333\tinf\tinf\tinf\tnan\tnan\tnan\n"
                    "img2\tlab2" + "\tN/A" * 9 + "\n")
    assert Q.surface_report_path("/m/model.net.nz") == "/m/model.net.surface_report.tsv"
    assert Q.surface_qc(None, "/m/model.nz", []) == (1, "no image/label pairs found")
