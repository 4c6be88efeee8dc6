"""CPU: the host half of the per-region intensity statistics (include/unet_stats.h, unet-studio_amd/stats.py) -- this file's own
restatements of the header's definitions (`codes`, `keys`, `moments_ref`, `hist_ref`, `quantiles_ref`: plain numpy, fp32 where the
header says fp32, integers everywhere else, importing nothing of the package's kernels) checked on hand-written answers and against
two second witnesses, the host arithmetic on the rows, the ABI the library exports, argument errors found before any device call
and the scratch size.  No device calls."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import unet_studio_amd as U
from unet_studio_amd import stats as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
NAN, INF = float("nan"), float("inf")
EMPTY = [0, 0, 0, 0, 0, 0, 65536, -1, 0xFFFFFFFF, -1]


# ---- the restatements ------------------------------------------------------------------------------------------------------------
def scale_of(lo, hi):
    """65536.0f / (hi - lo): one fp32 subtraction, one fp32 division"""
    return F(65536.0) / (F(hi) - F(lo))


def codes(v, lo, hi):
    """int64 codes of fp32 values that are not NaN: t = (v - lo) * scale in fp32, each operation rounded once; 0 below 0, 65535 from
    65535.0 on, otherwise truncated"""
    v = np.asarray(v, F)
    with np.errstate(over="ignore", invalid="ignore"):
        d = v - F(lo)
        t = d * scale_of(lo, hi)
    assert d.dtype == F and t.dtype == F and not np.isnan(t).any()
    inside = (t >= F(0)) & (t < F(65535.0))
    return np.where(t < F(0), 0, np.where(inside, np.where(inside, t, F(0)).astype(np.int64), 65535)).astype(np.int64)


def keys(v):
    """int64: the order-preserving image of the floats' bits as unsigned 32-bit values"""
    b = np.ascontiguousarray(np.asarray(v, F)).view(np.uint32).astype(np.int64)
    return np.where(b >> 31, b ^ 0xFFFFFFFF, b ^ 0x80000000)


def read_labels(labels, voxels, L):
    """a value above L reads as 0; no map: one region"""
    if labels is None:
        assert L == 0
        return np.zeros(voxels, np.int64)
    v = np.asarray(labels).astype(np.int64).reshape(-1)
    assert v.size == voxels
    return np.where(v > L, 0, v)


class Groups:
    """the voxels grouped by label: an integer reduction per row"""

    def __init__(self, lab, R):
        self.lab, self.R = lab, R
        if R > 8:
            self.order = np.argsort(lab, kind="stable")
            self.present, self.starts = np.unique(lab[self.order], return_index=True)
        else:
            self.masks = [lab == l for l in range(R)]

    def reduce(self, col, ufunc, empty):
        out = np.full(self.R, empty, np.int64)
        if self.R > 8:
            if self.present.size:
                out[self.present] = ufunc.reduceat(col[self.order], self.starts)
        else:
            for l, m in enumerate(self.masks):                      # `empty` is the identity of the reduction as well
                out[l] = ufunc.reduce(col, where=m, initial=empty)
        return out


def moments_ref(labels, image, L, lo, hi):
    """int64 {L + 1, 10}: n, NaNs, below, above, sum q, sum q * q, min q, max q, min key, max key; an empty row holds
    0, its NaNs, 0, 0, 0, 0, 65536, -1, 0xFFFFFFFF, -1"""
    v = np.asarray(image, F).reshape(-1)
    lab = read_labels(labels, v.size, L)
    nan = np.isnan(v)
    ok = ~nan
    q = np.where(ok, codes(np.where(ok, v, F(0)), lo, hi), 0)
    k = keys(v)
    with np.errstate(invalid="ignore"):
        below, above = ok & (v < F(lo)), ok & (v > F(hi))
    g = Groups(lab, L + 1)
    cols = [g.reduce(c.astype(np.int64), np.add, 0) for c in (ok, nan, below, above, q, q * q)]
    cols += [g.reduce(np.where(ok, q, 65536), np.minimum, 65536), g.reduce(np.where(ok, q, -1), np.maximum, -1),
             g.reduce(np.where(ok, k, 0xFFFFFFFF), np.minimum, 0xFFFFFFFF), g.reduce(np.where(ok, k, -1), np.maximum, -1)]
    return np.stack(cols, axis=1)


def hist_ref(labels, image, L, lo, hi):
    """int64 {L + 1, 256}: the coded voxels of a row whose q >> 8 is the column"""
    v = np.asarray(image, F).reshape(-1)
    lab = read_labels(labels, v.size, L)
    ok = ~np.isnan(v)
    q = codes(v[ok], lo, hi)
    return np.bincount(lab[ok] * 256 + (q >> 8), minlength=(L + 1) * 256).reshape(L + 1, 256).astype(np.int64)


def rows_of(lab, R):
    """-> per present label the indices of its voxels"""
    order = np.argsort(lab, kind="stable")
    present, starts = np.unique(lab[order], return_index=True)
    ends = np.append(starts[1:], lab.size)
    return [(int(l), order[s:e]) for l, s, e in zip(present, starts, ends)]


def quantiles_ref(labels, image, L, lo, hi, permille):
    """int32 {L + 1, Q}: np.sort(the codes of the row)[p * (n - 1) // 1000], -1 for a row without coded voxels"""
    v = np.asarray(image, F).reshape(-1)
    lab = read_labels(labels, v.size, L)
    out = np.full((L + 1, len(permille)), -1, np.int32)
    for l, idx in rows_of(lab, L + 1):
        vals = v[idx]
        vals = vals[~np.isnan(vals)]
        if vals.size:
            s = np.sort(codes(vals, lo, hi).astype(np.uint16))      # 16 bits hold a code, and sort faster
            out[l] = [int(s[int(p) * (s.size - 1) // 1000]) for p in permille]
    return out


def quantiles_by_value(labels, image, L, lo, hi, permille):
    """the second witness: coding is monotone, so the code of the r-th smallest VALUE is the r-th smallest code"""
    v = np.asarray(image, F).reshape(-1)
    lab = read_labels(labels, v.size, L)
    out = np.full((L + 1, len(permille)), -1, np.int32)
    for l, idx in rows_of(lab, L + 1):
        vals = v[idx]
        vals = np.sort(vals[~np.isnan(vals)])
        if vals.size:
            out[l] = codes(np.asarray([vals[int(p) * (vals.size - 1) // 1000] for p in permille], F), lo, hi)
    return out


# ---- the restatements on hand-written answers ------------------------------------------------------------------------------------
def test_codes_on_hand_worked_values():
    # lo 0, hi 2: scale 32768, a code is 1 / 32768 wide
    v = [0.0, -0.0, 1.0, 2.0, 1.99999, 3.0, -1.0, INF, -INF, 1.0 / 32768, 255.5 / 32768, 256.0 / 32768]
    assert scale_of(0, 2) == 32768.0
    assert codes(v, 0, 2).tolist() == [0, 0, 32768, 65535, 65535, 65535, 0, 65535, 0, 1, 255, 256]
    # hi itself and the value just below it: both in the last code; the value just above lo: code 0
    assert codes([np.nextafter(F(2), F(0)), np.nextafter(F(0), F(1), dtype=F) + F(1e-6)], 0, 2).tolist() == [65535, 0]
    # lo -1000, hi 3000: scale 16.384 in fp32
    assert scale_of(-1000, 3000) == F(65536.0) / F(4000.0)
    assert codes([-1000.0, 0.0, 3000.0], -1000, 3000).tolist() == [0, int(F(1000.0) * scale_of(-1000, 3000)), 65535]


def test_keys_are_ordered_as_the_floats_and_decode_key_inverts_them():
    v = np.asarray([-INF, -3.5, -1e-30, -0.0, 0.0, 1e-30, 1.0, 2.5, 3e38, INF], F)
    k = keys(v)
    assert (np.diff(k) > 0).all() and k.min() > 0 and k.max() < 0xFFFFFFFF
    assert k[3] == 0x7FFFFFFF and k[4] == 0x80000000 and k[0] == 0x007FFFFF and k[-1] == 0xFF800000
    back = S.decode_key(k)
    assert back.dtype == F and back.tobytes() == v.tobytes()           # -0.0 comes back as -0.0
    assert S.decode_key(np.int64(0xBF800000)) == F(1.0)
    rng = np.random.default_rng(0)
    r = rng.standard_normal(1000).astype(F) * F(1e3)
    assert S.decode_key(keys(r)).tobytes() == r.tobytes()
    assert (np.argsort(keys(r), kind="stable") == np.argsort(r, kind="stable")).all()
    for bad in (-1, 1 << 32):
        with pytest.raises(U.UNetError, match="key"):
            S.decode_key(bad)


def test_moments_of_a_hand_worked_map():
    labels = np.asarray([1, 1, 2, 2, 2, 0, 9, 1], np.uint8)
    image = np.asarray([0.5, NAN, 2.0, -1.0, 3.0, 1.0, INF, 0.0], F)
    rows = moments_ref(labels, image, 3, 0, 2)
    assert rows.dtype == np.int64 and rows.shape == (4, 10)
    # row 0: 1.0 and +inf (the 9 reads 0)
    assert rows[0].tolist() == [2, 0, 0, 1, 32768 + 65535, 32768 ** 2 + 65535 ** 2, 32768, 65535, 0xBF800000, 0xFF800000]
    # row 1: 0.5, NaN, 0.0
    assert rows[1].tolist() == [2, 1, 0, 0, 16384, 16384 ** 2, 0, 16384, 0x80000000, 0xBF000000]
    # row 2: 2.0 (== hi: neither below nor above), -1.0 (below), 3.0 (above)
    assert rows[2].tolist() == [3, 0, 1, 1, 2 * 65535, 2 * 65535 ** 2, 0, 65535, int(keys([-1.0])[0]), int(keys([3.0])[0])]
    assert rows[3].tolist() == EMPTY
    # no map: one region
    one = moments_ref(None, image, 0, 0, 2)
    assert one.shape == (1, 10) and one[0, :4].tolist() == [7, 1, 1, 2] and one[0, 8:].tolist() == [int(keys([-1.0])[0]), 0xFF800000]
    # a row of NaNs only is empty but for its NaNs
    assert moments_ref(np.asarray([1, 1]), np.asarray([NAN, NAN], F), 1, 0, 1)[1].tolist() == [0, 2] + EMPTY[2:]


def test_hist_and_quantiles_of_a_hand_worked_map():
    labels = np.asarray([1, 1, 1, 1, 2, 2, 0, 1], np.uint16)
    image = np.asarray([0.0, 1.0, 2.0, 0.5, NAN, 1.5, 1.0, NAN], F)
    h = hist_ref(labels, image, 3, 0, 2)
    assert h.shape == (4, 256) and h.sum() == 6 and h[1, 0] == 1 and h[1, 64] == 1 and h[1, 128] == 1 and h[1, 255] == 1
    assert h[2].sum() == 1 and h[2, 192] == 1 and h[0, 128] == 1 and h[3].sum() == 0
    q = quantiles_ref(labels, image, 3, 0, 2, [0, 500, 1000, 500, 999, 1])
    assert q.dtype == np.int32 and q.shape == (4, 6)
    # row 1: codes 0, 16384, 32768, 65535; n = 4: ranks 0, 1, 3, 1, 2, 0
    assert q[1].tolist() == [0, 16384, 65535, 16384, 32768, 0]
    assert q[2].tolist() == [49152] * 6 and q[0].tolist() == [32768] * 6 and q[3].tolist() == [-1] * 6
    # n = 2: the median is the lower one
    assert quantiles_ref(None, np.asarray([1.0, 0.0], F), 0, 0, 2, [500, 1000]).tolist() == [[0, 32768]]


# ---- the second witnesses ----------------------------------------------------------------------------------------------------------
def random_case(rng, n=None, L=None):
    n = int(rng.integers(1, 400)) if n is None else n
    L = int(rng.integers(1, 12)) if L is None else L
    lo = float(F(rng.uniform(-50, 50)))
    hi = float(F(lo + rng.uniform(0.5, 200)))
    v = rng.uniform(lo - 0.2 * (hi - lo), hi + 0.2 * (hi - lo), n).astype(F)
    v[rng.random(n) < 0.05] = F(lo)                                 # planted: v == lo, v == hi, their neighbours, NaN, the infinities
    v[rng.random(n) < 0.05] = F(hi)
    v[rng.random(n) < 0.02] = np.nextafter(F(hi), F(-INF))
    v[rng.random(n) < 0.02] = np.nextafter(F(lo), F(INF))
    v[rng.random(n) < 0.03] = NAN
    v[rng.random(n) < 0.01] = INF
    v[rng.random(n) < 0.01] = -INF
    labels = rng.integers(0, L + 3, n).astype(np.uint16)            # some above L
    return labels, v, L, lo, hi


def test_the_code_of_the_sorted_value_is_the_sorted_code_and_the_histogram_sums_to_n():
    rng = np.random.default_rng(5)
    for i in range(200):
        labels, v, L, lo, hi = random_case(rng)
        pm = [0, 500, 1000] + [int(p) for p in rng.integers(0, 1001, 3)]
        want = quantiles_ref(labels, v, L, lo, hi, pm)
        assert (quantiles_by_value(labels, v, L, lo, hi, pm) == want).all(), i
        m, h = moments_ref(labels, v, L, lo, hi), hist_ref(labels, v, L, lo, hi)
        assert (h.sum(1) == m[:, 0]).all() and int(m[:, :2].sum()) == v.size
        assert ((want >= 0) == (m[:, :1] > 0)).all()
        some = m[:, 0] > 0
        # the extremes of the codes are the codes of the extremes, and the quantiles 0 and 1000 are the extremes of the codes
        assert (want[some, 0] == m[some, 6]).all() and (want[some, 2] == m[some, 7]).all()
        assert (codes(S.decode_key(m[some, 8]), lo, hi) == m[some, 6]).all() and (codes(S.decode_key(m[some, 9]), lo, hi) == m[some, 7]).all()


def test_the_two_group_reductions_of_the_restatement_agree():
    rng = np.random.default_rng(6)
    labels, v, _, lo, hi = random_case(rng, n=3000, L=5)
    few = moments_ref(labels, v, 5, lo, hi)                         # at most 8 rows: masks
    many = moments_ref(labels, v, 40, lo, hi)                       # sorted groups; the labels 6 and 7 now have rows of their own
    assert (few[1:6] == many[1:6]).all() and (many[8:] == np.asarray(EMPTY)).all()
    assert few[0, 0] == many[0, 0] + many[6, 0] + many[7, 0]


# ---- the host arithmetic ---------------------------------------------------------------------------------------------------------------
def test_code_value_is_the_centre_of_the_code():
    assert S.code_value(0, 0, 2) == 0.5 / 32768 and S.code_value(65535, 0, 2) == 2 - 0.5 / 32768
    cv = S.code_value(np.arange(4), -1000, 3000)
    assert cv.dtype == np.float64 and np.allclose(np.diff(cv), 4000 / 65536, rtol=1e-6, atol=0)
    for lo, hi in ((1, 1), (2, 1), (NAN, 1), (0, INF), (-3e38, 3e38)):
        with pytest.raises(U.UNetError, match="lo and hi"):
            S.code_value(0, lo, hi)


def test_summary_mean_within_one_code_width_and_exact_extremes():
    """Coding moves a voxel by at most half a code width plus the fp32 rounding of (v - lo) * scale (0.51 widths at worst as
    measured), so the mean of the code centres lies within one width of the float64 mean of the in-range voxels."""
    rng = np.random.default_rng(7)
    for lo, hi in ((0.0, 1.0), (-1000.0, 3000.0), (-3.25, 17.5)):
        n, L = 20000, 6
        width = (hi - lo) / 65536
        v = rng.uniform(lo, hi, n).astype(F)
        v = np.clip(v, F(lo), F(hi))
        v[:3] = [lo, hi, (lo + hi) / 2]
        labels = rng.integers(0, L, n).astype(np.uint8)             # row L stays empty
        v[labels == 2] = F(0.25 * lo + 0.75 * hi)                   # a constant row: std 0
        rows = moments_ref(labels, v, L, lo, hi)
        pm = [0, 500, 1000]
        s = S.summary(rows, lo, hi, quantiles_ref(labels, v, L, lo, hi, pm))
        assert sorted(s) == ["above", "below", "max", "mean", "min", "n", "nan", "quantiles", "std"]
        assert s["quantiles"].shape == (L + 1, 3) and all(s[k].dtype == np.float64 and s[k].shape == (L + 1,) for k in s if k != "quantiles")
        for l in range(L):
            x = v[labels == l].astype(np.float64)
            assert s["n"][l] == x.size and s["nan"][l] == s["below"][l] == s["above"][l] == 0
            assert abs(s["mean"][l] - x.mean()) <= width, (l, s["mean"][l], x.mean())
            assert abs(s["std"][l] - x.std()) <= 2 * width
            assert s["min"][l] == x.min() and s["max"][l] == x.max()
            assert abs(s["quantiles"][l, 1] - np.sort(x)[(x.size - 1) // 2]) <= width
            assert abs(s["quantiles"][l, 0] - x.min()) <= width and abs(s["quantiles"][l, 2] - x.max()) <= width
        assert s["std"][2] == 0.0
        for k in ("mean", "std", "min", "max"):
            assert np.isnan(s[k][L])
        assert np.isnan(s["quantiles"][L]).all() and s["n"][L] == 0


def test_summary_counts_nan_below_and_above_and_checks_its_arguments():
    v = np.asarray([NAN, -5.0, 0.25, 7.0, INF, NAN], F)
    rows = moments_ref(None, v, 0, 0, 1)
    s = S.summary(torch.from_numpy(rows), 0, 1)
    assert "quantiles" not in s and (s["n"][0], s["nan"][0], s["below"][0], s["above"][0]) == (4, 2, 1, 2)
    assert s["min"][0] == -5.0 and s["max"][0] == INF
    with pytest.raises(U.UNetError, match="rows"):
        S.summary(rows[:, :9], 0, 1)
    with pytest.raises(U.UNetError, match="rows"):
        S.summary(rows.astype(np.float64), 0, 1)
    with pytest.raises(U.UNetError, match="quantile_codes"):
        S.summary(rows, 0, 1, np.zeros((2, 3), np.int32))
    with pytest.raises(U.UNetError, match="lo and hi"):
        S.summary(rows, 1, 1)


# ---- the ABI -------------------------------------------------------------------------------------------------------------------------
OTHERS = ("unet_table_", "unet_reg_", "unet_atlas_", "unet_components_", "unet_preproc_", "unet_dist_", "unet_inst_", "unet_morph_",
          "unet_conn_", "unet_mirror_", "unet_tiles_", "unet_space_", "unet_postproc_", "unet_qc_", "unet_feed_", "unet_augment_")


def test_unet_stats_h_declares_exactly_the_exports_and_the_library_has_them():
    lib = ctypes.CDLL(U.engine.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "unet_stats.h")).read()
    declared = set(re.findall(r"\b(unet_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(S.EXPORTS) == {"unet_stats_scratch_bytes", "unet_stats_moments", "unet_stats_hist", "unet_stats_quantiles"}
    for name in sorted(declared):
        assert hasattr(lib, name), "libunet_hip.so does not export " + name
    enums = {k: int(v) for k, v in re.findall(r"UNET_STATS_([A-Z_]+) = (\d+)", hdr)}
    assert enums == {"IMPL_DEFAULT": S.IMPL_DEFAULT, "IMPL_LDS": S.IMPL_LDS, "IMPL_GLOBAL": S.IMPL_GLOBAL}
    assert (S.IMPL_DEFAULT, S.IMPL_LDS, S.IMPL_GLOBAL) == (0, 1, 2)
    defines = {k: int(v) for k, v in re.findall(r"#define UNET_STATS_([A-Z_]+) (\d+)", hdr)}
    assert defines == {"MAX_LABELS": S.MAX_LABELS, "MAX_QUANTILE_LABELS": S.MAX_QUANTILE_LABELS, "MAX_QUANTILES": S.MAX_QUANTILES,
                       "MOMENT_COLUMNS": S.MOMENT_COLUMNS, "HIST_BINS": S.HIST_BINS, "CODES": S.CODES, "LDS_ROWS": S.LDS_ROWS,
                       "LDS_SLOTS": S.LDS_SLOTS, "SLOT_BINS": S.SLOT_BINS, "LDS_PROBES": S.LDS_PROBES, "UNIT": S.UNIT, "WAVE_UNITS": S.WAVE_UNITS,
                       "GRID_UNITS": S.GRID_UNITS}
    assert (S.MAX_LABELS, S.MAX_QUANTILE_LABELS, S.MAX_QUANTILES, S.MOMENT_COLUMNS, S.HIST_BINS, S.CODES) == (65535, 4095, 8, 10, 256, 65536)
    # the static LDS of a block: a moments row is six 64-bit sums and two 32-bit keys, a slot SLOT_BINS 32-bit counters and its key
    assert S.LDS_ROWS * (6 * 8 + 2 * 4) <= 64 * 1024 and S.LDS_SLOTS * (S.SLOT_BINS * 4 + 4) <= 64 * 1024 and S.HIST_BINS % S.SLOT_BINS == 0
    assert S.WAVE_UNITS % 64 == 0 and S.GRID_UNITS % S.WAVE_UNITS == 0 and S.GRID_UNITS * S.UNIT < 1 << 25
    assert U.stats is S


def test_the_prefixes_stay_apart_in_both_directions():
    for h in sorted(os.listdir(os.path.join(ROOT, "include"))):
        text = open(os.path.join(ROOT, "include", h)).read().lower()
        if h != "unet_stats.h":
            assert "unet_stats_" not in text, h
        else:
            for other in OTHERS:
                assert other not in text, other


# ---- argument errors, before any device call -------------------------------------------------------------------------------------
def test_scratch_bytes_is_monotone_and_checks_its_arguments():
    def mono(sizes):
        return all(a <= b for a, b in zip(sizes, sizes[1:]))
    by_l = [S.stats_scratch_bytes(1000, n) for n in (0, 1, 2, 255, S.LDS_ROWS - 1, S.LDS_ROWS, 2035, 4095, 4096, 65535)]
    assert mono(by_l) and by_l[0] < by_l[-1] and by_l[-1] >= 65536 * (6 * 8 + 2 * 4) and by_l[7] >= 4096 * 1024
    for L in (0, 1, 400, 4095):
        by_q = [S.stats_scratch_bytes(1000, L, q) for q in range(9)]
        assert mono(by_q) and by_q[0] < by_q[1] < by_q[8] and by_q[8] >= (L + 1) * 9 * 1024
        assert by_q[8] - by_q[7] >= (L + 1) * 1024                  # 1 KiB per row and per quantile
    for q in (0, 1, 8):
        assert mono([S.stats_scratch_bytes(1000, n, q) for n in (0, 1, 2, 255, 1024, 2035, 4095)])
    # nothing per voxel
    assert len({S.stats_scratch_bytes(v, 400, 3) for v in (1, 64, 1000, 10 ** 6, 256 ** 3, (1 << 31) - 1)}) == 1
    for v, n, q, msg in ((0, 5, 0, "voxels"), (1 << 31, 5, 0, "voxels"), (10, -1, 0, "n_labels"), (10, 65536, 0, "n_labels"),
                         (10, 4096, 1, "n_labels"), (10, 5, -1, "n_quantiles"), (10, 5, 9, "n_quantiles")):
        with pytest.raises(U.UNetError, match=msg):
            S.stats_scratch_bytes(v, n, q)
    rc = U.engine.lib.unet_stats_scratch_bytes(10, 5, 0, None)
    assert rc != 0 and "null output" in U.engine.lib.unet_last_error().decode()


P = [ctypes.c_void_p(0x1000 * (i + 1)) for i in range(8)]          # never dereferenced
BIG = 1 << 40


def common_errors(call, max_labels, out_name, out_align, n_quantiles):
    assert "null image" in call(image=None) and "image must be 4-byte aligned" in call(image=ctypes.c_void_p(0x2002))
    assert "n_labels must be 0 when labels is null, got 5" in call(labels=None)
    assert "when labels is given, got 0" in call(L=0) and "got -1" in call(L=-1)
    assert "n_labels must be in [1, %d] when labels is given, got %d" % (max_labels, max_labels + 1) in call(L=max_labels + 1)
    assert "label_bytes must be 1 or 2, got 4" in call(nbytes=4) and "label_bytes must be 1 or 2, got 0" in call(nbytes=0)
    assert "voxels must be in [1, 2^31)" in call(voxels=0) and "voxels" in call(voxels=-3) and "voxels" in call(voxels=1 << 31)
    for lo, hi in ((NAN, 1.0), (0.0, NAN), (-INF, 1.0), (0.0, INF)):
        assert "lo and hi must be finite" in call(lo=lo, hi=hi)
    assert "lo must be below hi" in call(lo=1.0, hi=1.0) and "lo must be below hi" in call(lo=2.0, hi=1.0)
    assert "scale" in call(lo=-3e38, hi=3e38) and "scale" in call(lo=0.0, hi=1e-42)
    assert "null " + out_name in call(out=None)
    assert "%s must be %d-byte aligned" % (out_name, out_align) in call(out=ctypes.c_void_p(0x3000 + out_align // 2))
    assert "unknown impl 3" in call(impl=3) and "unknown impl -1" in call(impl=-1)
    assert "null scratch" in call(scratch=None)
    assert "scratch too small" in call(scratch_bytes=S.stats_scratch_bytes(64, 5, n_quantiles) - 1)
    assert "scratch too small" in call(L=400, scratch_bytes=S.stats_scratch_bytes(64, 399, n_quantiles))
    # with no map the label_bytes are ignored: the next check is the one that fails
    assert "null " + out_name in call(labels=None, L=0, nbytes=7, out=None)
    # more labels than a uint8 map can hold is allowed
    assert "null " + out_name in call(nbytes=1, L=max_labels, out=None)


@pytest.mark.parametrize("name", ["unet_stats_moments", "unet_stats_hist"])
def test_moments_and_hist_argument_errors_need_no_device(name):
    lib = U.engine.lib

    def call(labels=P[0], nbytes=2, image=P[1], voxels=64, L=5, lo=0.0, hi=1.0, out=P[2], impl=0, scratch=P[3], scratch_bytes=BIG):
        rc = getattr(lib, name)(labels, nbytes, image, voxels, L, lo, hi, out, impl, scratch, scratch_bytes, None)
        assert rc != 0
        msg = lib.unet_last_error().decode()
        assert msg.startswith(name + ": ")
        return msg

    common_errors(call, 65535 if name.endswith("moments") else 4095, "rows", 8, 0)


def test_quantiles_argument_errors_need_no_device():
    lib = U.engine.lib

    def call(labels=P[0], nbytes=2, image=P[1], voxels=64, L=5, lo=0.0, hi=1.0, permille=(0, 500, 1000), Q=None, out=P[2], impl=0,
             scratch=P[3], scratch_bytes=BIG):
        pm = None if permille is None else (ctypes.c_int * max(1, len(permille)))(*permille)
        rc = lib.unet_stats_quantiles(labels, nbytes, image, voxels, L, lo, hi, pm, len(permille or ()) if Q is None else Q, out, impl,
                                      scratch, scratch_bytes, None)
        assert rc != 0
        msg = lib.unet_last_error().decode()
        assert msg.startswith("unet_stats_quantiles: ")
        return msg

    common_errors(call, 4095, "out", 4, 3)
    assert "null permille" in call(permille=None, Q=1)
    assert "n_quantiles must be in [1, 8], got 0" in call(Q=0) and "n_quantiles must be in [1, 8], got 9" in call(permille=(1,) * 9)
    assert "permille[1] must be in [0, 1000], got 1001" in call(permille=(0, 1001)) and "permille[0] must be in [0, 1000], got -1" in call(permille=(-1,))
    assert "scratch too small" in call(scratch_bytes=S.stats_scratch_bytes(64, 5, 2))      # three quantiles asked


def test_wrapper_errors_need_no_device():
    img, lab = torch.zeros(8, dtype=torch.float32), torch.zeros(8, dtype=torch.uint8)
    for fn in (S.moments, S.hist, S.quantiles):
        with pytest.raises(U.UNetError, match="image must be"):
            fn(lab, img, 5, 0, 1)
        with pytest.raises(U.UNetError, match="image must be"):
            fn(None, img.to(torch.float64), 0, 0, 1)
    with pytest.raises(U.UNetError, match="image must be"):
        S.volume_range(img)
    for bad in ((), (1,) * 9, (1001,), (-1,), (0.5,), "abc", 5):
        with pytest.raises(U.UNetError, match="permille"):
            S._permille(bad, "quantiles")
    assert S._permille((0, 500.0, np.int64(1000), 500), "quantiles") == [0, 500, 1000, 500]
