"""CPU: the host half of the non-linear refinement of a co-registration (include/unet_cowarp.h, unet-studio_amd/cowarp.py) -- the ABI
the library exports, argument errors found before any device call, the scratch size, and the restatements of tests/cowarp_ref.py
checked on hand-written answers.  The quality of the definition (does a lattice warp scored by point-wise mutual information bring a
smoothly warped image of another contrast back onto its partner) is measured here, on the restatement, not on the device.  No device
calls."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

import unet_studio_amd as U
from unet_studio_amd import cowarp as CW
from unet_studio_amd import warp as W

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import coreg_ref as cr  # noqa: E402
import cowarp_ref as ref  # noqa: E402
import warp_ref as wr  # noqa: E402
from test_register_host import IDENTITY, TRUE_MAP, ellipsoid_case, shift  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIG = 1 << 20                                                      # a limit that forbids nothing
L = cr.ilog


def table(bins, cells):
    h = np.zeros((bins, bins + 1), np.uint32)
    for (a, b), n in cells.items():
        h[a, b] = n
    return h


# ---- weights_ref on hand-worked tables ------------------------------------------------------------------------------------------------
def test_weights_of_a_diagonal_histogram():
    # two codes of 4 and 12 voxels, each always met by itself: N = 16, r = c = (4, 12)
    w = ref.weights_ref(table(8, {(0, 0): 4, (1, 1): 12}))
    assert w.dtype == np.int16 and w.shape == (8, 9)
    # L(4) + L(16) - L(4) - L(4) = log2(4) = 2 bit -> 2 * 65536 >> 8 = 512; L(12) + L(16) - 2 L(12) = L(16) - L(12)
    assert w[0, 0] == 512 and w[1, 1] == (L(16) - L(12)) >> 8 == 106
    # an empty cell of two used codes: 0 + L(16) - L(4) - L(12) = 4 - 2 - log2(12) bit: negative, shifted arithmetically
    assert w[0, 1] == w[1, 0] == (L(16) - L(4) - L(12)) >> 8 == -406 and (L(16) - L(4) - L(12)) % 256 != 0
    # a moving code never seen (c = 0): L(16) - L(r) >= 0; the outside column: the row's minimum, at most 0
    assert w[0, 2] == (L(16) - L(4)) >> 8 == 512 and w[1, 2] == 106 and w[0, 8] == w[1, 8] == -406
    # an empty row (r = 0, n = 0): L(N) - L(c_b) >= 0 everywhere, so its outside column is 0
    assert w[2, 0] == 512 and w[2, 1] == 106 and w[2, 2] == (L(16)) >> 8 == 1024 and w[2, 8] == 0 and (w[2:] >= 0).all()


def test_weights_of_a_uniform_histogram_are_within_one_unit_below_zero():
    for bins, n in ((8, 5), (16, 1000), (32, 3), (8, 1 << 20)):
        h = np.zeros((bins, bins + 1), np.uint32)
        h[:, :bins] = n                                            # independent codes: no information anywhere
        w = ref.weights_ref(h)
        assert (w <= 0).all() and (w >= -1).all(), (bins, n, w.min(), w.max())
    # counts in the outside column raise r_a and N alike and cost every inside cell of the row
    h[:, bins] = 7 << 20
    assert (ref.weights_ref(h)[:, :bins] == ref.weights_ref(h)[0, 0]).all() and ref.weights_ref(h)[0, 0] <= 0


def test_weights_the_outside_column_is_the_rows_minimum_and_never_positive():
    rng = np.random.default_rng(1)
    h = rng.integers(0, 50, (16, 17)).astype(np.uint32)
    h[3, :16] = 0                                                  # an empty row but for the outside column
    h[5] = 0
    wide = ref.weights_wide(h)
    assert (wide[:, 16] == np.minimum(0, wide[:, :16].min(1))).all() and (wide[:, 16] <= 0).all()
    assert wide[5, 16] == 0 and (wide[5, :16] >= 0).all()
    # against Python integers, cell by cell
    r, c, n = h.sum(1), h[:, :16].sum(0), int(h.sum())
    for a in range(16):
        for b in range(16):
            assert wide[a, b] == (L(h[a, b]) + L(n) - L(r[a]) - L(c[b])) >> 8, (a, b)
    assert ref.weights_ref(h).tolist() == wide.tolist()


def test_weights_stay_within_2_to_the_13_and_local_sums_within_int32():
    rng = np.random.default_rng(2)
    worst = 0
    for bins in (8, 16, 32):
        for total in (1, 7, 1000, 1 << 20, (1 << 31) - 1):
            for _ in range(4):
                p = rng.dirichlet(np.full(bins * (bins + 1), rng.choice([0.02, 0.3, 5.0])))
                h = np.floor(p * total).astype(np.int64)
                h.flat[rng.integers(h.size)] += total - int(h.sum())   # the total is exact
                h = h.reshape(bins, bins + 1)
                assert int(h.sum()) == total and h.min() >= 0
                wide = ref.weights_wide(h)
                worst = max(worst, int(np.abs(wide).max()))
                assert ref.weights_ref(h).tolist() == wide.tolist()    # int16 holds it
    # one voxel in one cell of a full table: the extreme of L(n) - L(r)
    h = np.zeros((8, 9), np.int64)
    h[0, 0], h[0, 1], h[1, 0] = 1, (1 << 30) - 1, (1 << 30) - 1
    worst = max(worst, int(np.abs(ref.weights_wide(h)).max()))
    assert 0 < worst <= CW.MAX_WEIGHT == 1 << 13
    assert max(L(n) for n in (1, 3, (1 << 31) - 1)) < 1 << 21 and L((1 << 31) - 1) == 2031615
    # the header's bound: a support of at most 31^3 voxels, seven int32 sums
    assert CW.MAX_SUPPORT == ref.MAX_SUPPORT == 31 ** 3 == (2 * 16 - 1) ** 3 and CW.MAX_SUPPORT * CW.MAX_WEIGHT < 1 << 29
    assert (2 * 32 - 1) ** 3 * CW.MAX_WEIGHT >= 1 << 29             # why g = 32 is refused


# ---- hist_ref ----------------------------------------------------------------------------------------------------------------------------
def test_a_zero_field_gives_the_histogram_of_the_affine_map_alone():
    rng = np.random.default_rng(3)
    shear = [1.05, 0.1, 0, -0.08, 0.97, 0.04, 0.02, 0, 1.1, -1.25, 0.75, -0.5]
    fixed, moving = ref.warped_codes()
    small_f, small_m = rng.integers(0, 20, (3, 5, 7)).astype(np.uint8), rng.integers(0, 20, (3, 7, 5)).astype(np.uint8)   # codes above 16 too
    for f, m, m12 in ((fixed, moving, TRUE_MAP), (small_f, small_m, IDENTITY), (small_f, small_m, shear), (small_f, small_m, shift(0.5, -0.5, 0.5))):
        for g in (4, 8, 16):
            got = ref.hist_ref(f, m, 16, m12, wr.zero_field(f.shape, g), g)
            assert got.dtype == np.uint32 and got.shape == (16, 17) and got.tobytes() == cr.hist_ref(f, m, 16, [m12], 1)[0].tobytes()
    assert int(got.sum()) == int((small_f < 16).sum()) < small_f.size


def test_the_histogram_follows_the_field_and_skips_fixed_voxels_without_a_code():
    fixed = np.array([1, 1, 1, 8, 1], np.uint8).reshape(1, 1, 5)   # 8 = bins: "none"
    moving = np.array([1, 1, 1, 1, 1, 2], np.uint8).reshape(1, 1, 6)
    D = wr.zero_field(fixed.shape, 4)
    assert ref.hist_ref(fixed, moving, 8, IDENTITY, D, 4)[1].tolist() == [0, 4, 0, 0, 0, 0, 0, 0, 0]
    D[0, 0, 1, 0] = 256                                            # x = 4 goes to 5 and reads 2
    assert ref.hist_ref(fixed, moving, 8, IDENTITY, D, 4)[1].tolist() == [0, 3, 1, 0, 0, 0, 0, 0, 0]
    D[0, 0, 1, 0] = 512                                            # x = 4 goes to 6: outside, the last column
    assert ref.hist_ref(fixed, moving, 8, IDENTITY, D, 4)[1].tolist() == [0, 3, 0, 0, 0, 0, 0, 0, 1]
    moving[0, 0, 2] = 200                                          # a moving code above bins reads as "none": the last column too
    assert ref.hist_ref(fixed, moving, 8, IDENTITY, D, 4)[1].tolist() == [0, 2, 0, 0, 0, 0, 0, 0, 2]


# ---- sweep_ref on hand-written answers ---------------------------------------------------------------------------------------------------
def test_sweep_a_score_tie_stays_on_candidate_0():
    fixed, moving = np.ones((1, 1, 5), np.uint8), np.ones((9, 9, 12), np.uint8)
    D0 = wr.zero_field(fixed.shape, 4)
    seen = []
    D, info = ref.sweep_ref(fixed, moving, 8, shift(4, 4, 4), D0, 4, 256, BIG, scores_out=seen)
    # one cell in use: W[1][1] = 0, every candidate of both nodes sees code 1 everywhere and scores 0
    assert D.tolist() == D0.tolist() and D.dtype == np.int32 and info.tolist() == [0, 2]
    assert [n.tolist() for n, _, _ in seen] == [[0], [1], [], [], [], [], [], []]
    assert seen[0][1].reshape(-1).tolist() == [0] * 7 and seen[0][2].all()
    # with weights that are not zero: codes 1 and 2 in two halves, aligned; every move can only lose or tie
    fixed = np.array([1, 1, 1, 2, 2, 2, 2, 2], np.uint8).reshape(1, 1, 8)
    moving = np.array([3, 3, 3, 3, 5, 5, 5, 5, 5, 5], np.uint8).reshape(1, 1, 10)
    seen = []
    D, info = ref.sweep_ref(fixed, moving, 8, shift(1), wr.zero_field(fixed.shape, 4), 4, 256, BIG, scores_out=seen)
    assert not D.any() and info.tolist() == [0, 3]
    for nodes, local, adm in seen:
        assert (local[0] >= local[1:]).all() and (local[0] > 0).all()


def test_sweep_a_fixed_voxel_without_a_code_adds_nothing_and_visits_nothing():
    fixed = np.array([1, 1, 1, 2, 2, 2, 2, 2], np.uint8).reshape(1, 1, 8)
    moving = np.array([3, 3, 3, 3, 3, 5, 5, 5, 5, 5], np.uint8).reshape(1, 1, 10)      # the edge sits one voxel to the right
    seen = []
    D, info = ref.sweep_ref(fixed, moving, 8, shift(1), wr.zero_field(fixed.shape, 4), 4, 256, BIG, scores_out=seen)
    assert info[0] > 0 and info[1] == 3 and D[0, 0, 1, 0] == 256    # the node at x = 4 pushes its voxels over the edge
    # the same with every voxel of the node at x = 8 (support 5..7) and one voxel of the two other nodes turned into "none"
    holes = fixed.copy()
    holes[0, 0, 5:] = 8
    holes[0, 0, 2] = 255
    seen2 = []
    D2, info2 = ref.sweep_ref(holes, moving, 8, shift(1), wr.zero_field(fixed.shape, 4), 4, 256, 0, scores_out=seen2)   # limit 0: nothing moves
    assert [n.tolist() for n, _, _ in seen2] == [[0], [1], [], [], [], [], [], []] and info2.tolist() == [0, 2] and not D2.any()
    # candidate 0 by hand from W: node 0 holds x = 0, 1, 3 (2 is a hole), which read moving 1, 2, 4: codes 3, 3, 3; node 1 holds
    # x = 1, 3, 4, which read moving 2, 4, 5: codes 3, 3, 5
    Wt = ref.weights_ref(ref.hist_ref(holes, moving, 8, shift(1), wr.zero_field(fixed.shape, 4), 4)).astype(np.int64)
    assert seen2[0][1][0, 0] == 2 * Wt[1, 3] + Wt[2, 3] and seen2[1][1][0, 0] == Wt[1, 3] + Wt[2, 3] + Wt[2, 5]
    # candidate 1 (+x by a whole voxel at the node, less away from it): node 1's x = 3 (weight 3/4: 4.75 + 0.5 -> 5) now reads code 5
    assert seen2[1][1][1, 0] == Wt[1, 3] + Wt[2, 5] + Wt[2, 5]
    # an image that is all "none": an empty histogram, zero weights, nothing visited, nothing moved
    none = np.full((3, 5, 9), 8, np.uint8)
    h = ref.hist_ref(none, moving, 8, IDENTITY, wr.zero_field(none.shape, 4), 4)
    assert not h.any() and not ref.weights_ref(h).any()
    D3, info3 = ref.sweep_ref(none, moving, 8, IDENTITY, wr.zero_field(none.shape, 4), 4, 256, BIG)
    assert not D3.any() and info3.tolist() == [0, 0]


def test_sweep_the_frozen_total_never_decreases_across_a_pass_and_the_true_score_is_reported():
    rng = np.random.default_rng(5)
    fixed, moving = rng.integers(0, 9, (6, 9, 11)).astype(np.uint8), rng.integers(0, 9, (7, 9, 12)).astype(np.uint8)
    m = [1.05, 0.1, 0, -0.08, 0.97, 0.04, 0.02, 0, 1.1, 0.25, 0.75, -0.5]
    for g in (4, 8):
        D = (rng.integers(-300, 301, wr.lattice_ref(fixed.shape, g) + (3,))).astype(np.int32)
        for step in (256, 64, 1):
            Wt = ref.weights_ref(ref.hist_ref(fixed, moving, 8, m, D, g))
            totals = [ref.total_ref(ref.hist_ref(fixed, moving, 8, m, D, g), Wt)]
            D, info = ref.sweep_ref(fixed, moving, 8, m, D, g, step, 700,
                                    after_pass=lambda d: totals.append(ref.total_ref(ref.hist_ref(fixed, moving, 8, m, d, g), Wt)))
            assert len(totals) == 9 and all(b >= a for a, b in zip(totals, totals[1:])), totals
            assert step == 1 or totals[-1] > totals[0]
        assert info[1] > 0


# ---- resample_ref ------------------------------------------------------------------------------------------------------------------------
def test_resample_follows_the_field_linearly():
    moving = np.arange(12, dtype=np.float32).reshape(1, 1, 12) ** 2
    D = wr.zero_field((1, 1, 9), 4)
    assert ref.resample_ref(moving, (1, 1, 9), IDENTITY, D, 4).reshape(-1).tolist() == [float(x * x) for x in range(9)]
    D[0, 0, 1, 0] = 128                                            # the node at x = 4 moved by half a moving voxel
    got = ref.resample_ref(moving, (1, 1, 9), IDENTITY, D, 4).reshape(-1)
    assert got.dtype == np.float32 and got[4] == (16 + 25) / 2 and got[2] == 4 + 0.25 * 5 and got[0] == 0 and got[8] == 64
    D[0, 0, 1, 0] = -5 * 256                                       # x = 4 goes to -1: outside reads 0; x = 3 goes to -0.75 too
    got = ref.resample_ref(moving, (1, 1, 9), IDENTITY, D, 4).reshape(-1)
    assert got[4] == 0 and got[3] == 0 and got[5] == 1.25 ** 2 + 0.25 * 0.75   # 1.25 between 1 and 4: 1 + 0.25 * 3
    D[0, 0, 1] = (0, 1, 0)                                         # the smallest step off the one-row volume along y: outside
    assert ref.resample_ref(moving, (1, 1, 9), IDENTITY, D, 4).reshape(-1)[4] == 0


# ---- the quality of the definition -------------------------------------------------------------------------------------------------------
def test_the_fit_brings_the_warped_contrast_pair_back_together():
    """Measured on the restatement: warp_ref.warped_case() (the ellipsoid template sampled through TRUE_MAP plus a smooth warp of
    about 2 voxels) rendered in two contrasts with noise, 16 bins.  Under TRUE_MAP alone N * MI is 2 691 835 403 (0.614 bit per
    voxel) and the Dice of the hidden tissue maps 0.7434; fit_ref from TRUE_MAP with the defaults reaches 4 211 003 941 (0.961 bit,
    x 1.56) and 0.9324, N * MI rising in each of the 8 rows; the largest displacement of the final field is 1200 (4.7 moving
    voxels).  The floors asserted are the issue's: Dice below 0.80 before and at least 0.90 after, N * MI at least 1.4 times the
    affine one."""
    subject, template = wr.warped_case()
    fixed, moving = ref.warped_codes()
    assert fixed.shape == subject.shape == (38, 44, 40) and moving.shape == template.shape and fixed.dtype == np.uint8
    assert int(fixed.max()) < 16 and int(moving.max()) < 16
    levels = wr.levels_ref(TRUE_MAP)
    assert W.levels_of(W.DEFAULT_LEVELS, None, TRUE_MAP).tolist() == [list(lv) for lv in levels] and all(lv[0] in CW.SPACINGS for lv in levels)
    zero = wr.zero_field(fixed.shape, 16)
    affine = cr.score_ref(ref.hist_ref(fixed, moving, 16, TRUE_MAP, zero, 16))
    D, report = ref.warped_fit(check_total=True)                   # the frozen-W total is asserted across all 384 passes
    rows = report[report[:, 0] >= 0]
    before = wr.dice_ref(wr.hist_ref(subject, template, 5, TRUE_MAP, zero, 16))
    after = wr.dice_ref(wr.hist_ref(subject, template, 5, TRUE_MAP, D, 4))
    n = int((fixed < 16).sum())
    print("contrast pair: N*MI %d (%.3f bit) -> %d (%.3f bit), x %.3f; hidden Dice %.4f -> %.4f; max |D| %d" % (
        affine, affine / n / 65536, rows[-1, 4], rows[-1, 4] / n / 65536, rows[-1, 4] / affine, before, after, int(np.abs(D).max())))
    print(rows)
    assert before < 0.80 and after >= 0.90
    assert rows[-1, 4] >= 1.4 * affine
    assert D.shape == wr.lattice_ref(fixed.shape, 4) + (3,) and D.dtype == np.int32 and report.shape == (32, 5)
    assert rows[:, 0].tolist() == [16, 16, 16, 8, 8, 8, 4, 4] and rows[:, 1].tolist() == [512, 256, 128, 256, 128, 64, 128, 64]
    assert (report[len(rows):] == -1).all() and ((rows[:, 2] >= 1) & (rows[:, 2] <= 6)).all()
    assert rows[-1, 4] == cr.score_ref(ref.hist_ref(fixed, moving, 16, TRUE_MAP, D, 4)) == CW.score(ref.hist_ref(fixed, moving, 16, TRUE_MAP, D, 4))
    assert (rows[rows[:, 2] < 6, 3] == 0).all() and int(np.abs(D).max()) <= 32767
    assert affine == CW.score(ref.hist_ref(fixed, moving, 16, TRUE_MAP, zero, 16)) == cr.score_py(ref.hist_ref(fixed, moving, 16, TRUE_MAP, zero, 16))


def test_the_control_without_a_warp_does_not_fall_below_the_affine_score():
    """The same two contrasts with the subject sampled through TRUE_MAP alone (test_register_host's ellipsoid case): there is nothing
    to find.  Measured on the restatement: N * MI is 4 398 209 317 under TRUE_MAP; the fit still moves 1451 of the 1452 nodes, by up
    to 1024 (4 moving voxels), chasing the noise: the first coarse row LOSES score (3 564 257 690: the frozen table rewards what the
    true mutual information does not), the rows after it win it back and the fit ends at 4 415 206 499.  Asserted is only what the
    issue asks: the final N * MI is not below the affine one."""
    subject, template = ellipsoid_case()
    fixed, moving = ref.contrast_pair(subject, template)
    affine = cr.score_ref(ref.hist_ref(fixed, moving, 16, TRUE_MAP, wr.zero_field(fixed.shape, 16), 16))
    D, report = ref.fit_ref(fixed, moving, 16, TRUE_MAP, check_total=False)
    rows = report[report[:, 0] >= 0]
    print("control: N*MI %d -> %d; max |D| %d, %d of %d nodes moved" % (affine, rows[-1, 4], int(np.abs(D).max()), int((D != 0).any(-1).sum()),
                                                                        D[..., 0].size))
    print(rows)
    assert rows[-1, 4] >= affine


# ---- the ABI -------------------------------------------------------------------------------------------------------------------------
def test_unet_cowarp_h_declares_exactly_the_exports_and_names_no_other_prefix():
    lib = ctypes.CDLL(U.engine.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "unet_cowarp.h")).read()
    declared = set(re.findall(r"\b(unet_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(CW.EXPORTS) == {"unet_cowarp_scratch_bytes", "unet_cowarp_hist", "unet_cowarp_weights", "unet_cowarp_sweep",
                                           "unet_cowarp_fit", "unet_cowarp_resample"}
    for name in sorted(declared):
        assert hasattr(lib, name), "libunet_hip.so does not export " + name
    enums = {k: int(v) for k, v in re.findall(r"UNET_COWARP_(IMPL_[A-Z]+) = (\d+)", hdr)}
    assert enums == {"IMPL_DEFAULT": CW.IMPL_DEFAULT, "IMPL_NODE": CW.IMPL_NODE, "IMPL_VOXEL": CW.IMPL_VOXEL}
    assert (CW.IMPL_DEFAULT, CW.IMPL_NODE, CW.IMPL_VOXEL) == (0, 1, 2)
    limits = {k: int(v) for k, v in re.findall(r"#define UNET_COWARP_MAX_([A-Z]+) (\d+)", hdr)}
    assert limits == {"BINS": CW.MAX_BINS, "DISP": CW.MAX_DISP, "STEP": CW.MAX_STEP, "LEVELS": CW.MAX_LEVELS, "SWEEPS": CW.MAX_SWEEPS,
                      "ROWS": CW.MAX_ROWS, "SUPPORT": CW.MAX_SUPPORT, "WEIGHT": CW.MAX_WEIGHT}
    # the schedule and the field are the tissue warp's, so that its refine and its defaults serve both
    assert (CW.MAX_DISP, CW.MAX_STEP, CW.MAX_SWEEPS, CW.MAX_ROWS) == (W.MAX_DISP, W.MAX_STEP, W.MAX_SWEEPS, W.MAX_ROWS) and CW.MAX_ROWS == ref.MAX_ROWS
    assert CW.MAX_BINS == U.coreg.MAX_BINS and CW.SPACINGS == ref.SPACINGS == (4, 8, 16)
    assert U.cowarp is CW and CW.Plan() == (None, None, CW.IMPL_DEFAULT) and CW.Plan(limit=9).limit == 9
    # the header speaks of the two it builds on by name only (and of the co-registration header, which tests/test_coreg_host.py lets
    # no other header spell, as "the coreg header")
    low = hdr.lower()
    assert "unet_warp_" not in low and "unet_coreg" not in low and "unet_warp.h" in low and "the coreg header" in low
    for h in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if h != "unet_cowarp.h":
            assert "unet_cowarp_" not in open(os.path.join(ROOT, "include", h)).read().lower(), h


# ---- argument errors, before any device call -------------------------------------------------------------------------------------
P = [ctypes.c_void_p(0x1000 * (i + 1)) for i in range(8)]          # never dereferenced
F12 = (ctypes.c_float * 12)(*IDENTITY)


def ints(v):
    return (ctypes.c_int * len(v))(*v)


LEVELS = ints([16, 512, 128, 6, 974, 8, 256, 64, 6, 487, 4, 128, 64, 6, 243])


def levels_errors(call):
    """what every call that takes a schedule refuses"""
    assert "n_levels must be in [1, 3], got 0" in call(n_levels=0) and "n_levels" in call(n_levels=4) and "null levels" in call(levels=None)
    assert "level 0: g must be 4, 8 or 16, got 32" in call(levels=ints([32, 1, 1, 1, 0]), n_levels=1)
    assert "level 0: g must be 4, 8 or 16, got 12" in call(levels=ints([12, 1, 1, 1, 0]), n_levels=1)
    assert "level 0: g must be" in call(levels=ints([2, 1, 1, 1, 0]), n_levels=1)
    assert "level 1: g must be 4, 8 or 16, got 2" in call(levels=ints([4, 4, 2, 1, 0, 2, 4, 2, 1, 0]), n_levels=2)
    assert "level 1: g must be half the level before's, got 4" in call(levels=ints([16, 4, 2, 1, 0, 4, 4, 2, 1, 0]), n_levels=2)
    assert "level 1: g must be half" in call(levels=ints([8, 4, 2, 1, 0, 16, 4, 2, 1, 0]), n_levels=2)
    assert "level 0: first_step must be a power of two in [1, 16384], got 384" in call(levels=ints([8, 384, 128, 1, 0]), n_levels=1)
    assert "level 0: last_step must be a power of two" in call(levels=ints([8, 512, 96, 1, 0]), n_levels=1)
    assert "first_step must be a power of two" in call(levels=ints([8, 0, 0, 1, 0]), n_levels=1)
    assert "first_step must be a power of two" in call(levels=ints([8, 32768, 1, 1, 0]), n_levels=1)
    assert "level 2: first_step must not be below last_step" in call(levels=ints([16, 4, 2, 1, 0, 8, 4, 2, 1, 0, 4, 2, 4, 1, 0]))
    assert "level 0: max_sweeps must be in [1, 16], got 0" in call(levels=ints([8, 4, 2, 0, 0]), n_levels=1)
    assert "max_sweeps must be in [1, 16], got 17" in call(levels=ints([8, 4, 2, 17, 0]), n_levels=1)
    assert "level 0: limit must not be negative, got -1" in call(levels=ints([8, 4, 2, 1, -1]), n_levels=1)
    assert "33 (level, step) pairs" in call(levels=ints([16, 16384, 1, 1, 0, 8, 16384, 1, 1, 0, 4, 4, 1, 1, 0]), n_levels=3)


def grids_errors(call):
    assert "null fixed" in call(fixed=None) and "null moving" in call(moving=None)
    assert "fixed dimensions" in call(f=(0, 4, 4)) and "fixed dimensions" in call(f=(4, 4, -1)) and "moving dimensions" in call(m=(4, 0, 4))
    assert "fixed grid" in call(f=(2048, 1024, 1024)) and "moving grid" in call(m=(2048, 1024, 1024))
    assert "bins must be 8, 16 or 32, got 12" in call(bins=12) and "bins must be" in call(bins=0) and "bins must be" in call(bins=64)


def test_scratch_bytes_is_monotone_and_checks_its_arguments():
    lib = U.engine.lib

    def call(f=(40, 44, 38), bins=16, levels=LEVELS, n_levels=3, out=True):
        n = ctypes.c_size_t()
        rc = lib.unet_cowarp_scratch_bytes(*f, bins, levels, n_levels, ctypes.byref(n) if out else None)
        assert rc != 0
        return lib.unet_last_error().decode()

    levels_errors(call)
    assert "fixed dimensions" in call(f=(0, 4, 4)) and "fixed grid" in call(f=(2048, 1024, 1024))
    assert "bins must be 8, 16 or 32, got 9" in call(bins=9) and "null output" in call(out=False)
    assert call(bins=9).startswith("unet_cowarp_scratch_bytes: ")
    full = [list(lv) for lv in wr.levels_ref(TRUE_MAP)]
    sizes = [CW.scratch_bytes(s, 16, full) for s in ((1, 1, 1), (38, 44, 40), (64, 64, 64), (256, 256, 256))]
    assert all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[0] < sizes[-1]
    # the 8 counters per node of the finest lattice and the two coarser fields
    assert sizes[-1] >= 65 ** 3 * 8 * 4 + (17 ** 3 + 33 ** 3) * 3 * 4
    one = [CW.scratch_bytes((64, 64, 64), 32, [(g, 1, 1, 1, 0)]) for g in (16, 8, 4)]
    assert all(a <= b for a, b in zip(one, one[1:])) and one[-1] >= 17 ** 3 * 8 * 4 and one[-1] <= CW.scratch_bytes((64, 64, 64), 32, full)
    with pytest.raises(U.UNetError, match="g must be 4, 8 or 16, got 32"):
        CW.scratch_bytes((64, 64, 64), 16, [(32, 1, 1, 1, 0)])


def test_hist_weights_and_resample_argument_errors_need_no_device():
    lib = U.engine.lib

    def hist(fixed=P[0], f=(4, 4, 4), moving=P[1], m=(4, 4, 4), bins=16, map=F12, D=P[2], g=4, hist=P[3]):
        rc = lib.unet_cowarp_hist(fixed, *f, moving, *m, bins, map, D, g, hist, None)
        assert rc != 0
        return lib.unet_last_error().decode()

    grids_errors(hist)
    assert "null map" in hist(map=None) and "null D" in hist(D=None) and "null hist" in hist(hist=None)
    assert "D must be 4-byte aligned" in hist(D=ctypes.c_void_p(0x3002)) and "hist must be 4-byte aligned" in hist(hist=ctypes.c_void_p(0x3001))
    assert "g must be 4, 8 or 16, got 32" in hist(g=32) and "g must be" in hist(g=0) and "g must be" in hist(g=6)
    assert hist(g=3).startswith("unet_cowarp_hist: ")

    def weights(hist=P[0], bins=16, w=P[1]):
        rc = lib.unet_cowarp_weights(hist, bins, w, None)
        assert rc != 0
        return lib.unet_last_error().decode()

    assert "null hist" in weights(hist=None) and "null weights" in weights(w=None) and "bins must be 8, 16 or 32, got 4" in weights(bins=4)
    assert "hist must be 4-byte aligned" in weights(hist=ctypes.c_void_p(0x3002)) and "weights must be 2-byte aligned" in weights(w=ctypes.c_void_p(0x3001))

    def resample(moving=P[0], m=(4, 4, 4), f=(4, 4, 4), map=F12, D=P[1], g=8, out=P[2]):
        rc = lib.unet_cowarp_resample(moving, *m, *f, map, D, g, out, None)
        assert rc != 0
        return lib.unet_last_error().decode()

    assert "null moving" in resample(moving=None) and "null map" in resample(map=None) and "null D" in resample(D=None) and "null out" in resample(out=None)
    assert "moving must be 4-byte aligned" in resample(moving=ctypes.c_void_p(0x3002)) and "out must be 4-byte aligned" in resample(out=ctypes.c_void_p(0x3001))
    assert "D must be 4-byte aligned" in resample(D=ctypes.c_void_p(0x3003)) and "g must be 4, 8 or 16, got 32" in resample(g=32)
    assert "moving dimensions" in resample(m=(4, 0, 4)) and "fixed dimensions" in resample(f=(-1, 4, 4))
    assert "moving grid" in resample(m=(2048, 1024, 1024)) and "fixed grid" in resample(f=(2048, 1024, 1024))


def test_sweep_and_fit_argument_errors_need_no_device():
    lib = U.engine.lib

    def sweep(fixed=P[0], f=(4, 4, 4), moving=P[1], m=(4, 4, 4), bins=16, map=F12, D=P[2], g=4, step=256, limit=100, info=P[3], impl=0,
              scratch=P[4], scratch_bytes=1 << 40):
        rc = lib.unet_cowarp_sweep(fixed, *f, moving, *m, bins, map, D, g, step, limit, info, impl, scratch, scratch_bytes, None)
        assert rc != 0
        return lib.unet_last_error().decode()

    grids_errors(sweep)
    assert "null map" in sweep(map=None) and "null D" in sweep(D=None) and "null info" in sweep(info=None) and "null scratch" in sweep(scratch=None)
    assert "g must be 4, 8 or 16, got 32" in sweep(g=32) and "g must be 4, 8 or 16, got 5" in sweep(g=5)
    assert "step must be in [1, 32767], got 0" in sweep(step=0) and "step must be" in sweep(step=32768) and "step must be" in sweep(step=-4)
    assert "limit must not be negative, got -1" in sweep(limit=-1)
    assert "info must be 8-byte aligned" in sweep(info=ctypes.c_void_p(0x5004)) and "D must be 4-byte aligned" in sweep(D=ctypes.c_void_p(0x5001))
    assert "unknown impl 3" in sweep(impl=3) and "unknown impl -1" in sweep(impl=-1)
    need = CW.scratch_bytes((4, 4, 4), 16, [(4, 1, 1, 1, 0)])
    assert "scratch too small" in sweep(scratch_bytes=need - 1) and "scratch too small" in sweep(f=(64, 64, 64), scratch_bytes=need)

    def fit(fixed=P[0], f=(4, 4, 4), moving=P[1], m=(4, 4, 4), bins=16, map=F12, levels=LEVELS, n_levels=3, D=P[2], report=P[3], impl=0,
            scratch=P[4], scratch_bytes=1 << 40):
        rc = lib.unet_cowarp_fit(fixed, *f, moving, *m, bins, map, levels, n_levels, D, report, impl, scratch, scratch_bytes, None)
        assert rc != 0
        return lib.unet_last_error().decode()

    grids_errors(fit)
    levels_errors(fit)
    assert "null map" in fit(map=None) and "null D_out" in fit(D=None) and "null report" in fit(report=None) and "null scratch" in fit(scratch=None)
    assert "report must be 8-byte aligned" in fit(report=ctypes.c_void_p(0x5004)) and "D_out must be 4-byte aligned" in fit(D=ctypes.c_void_p(0x5002))
    assert "unknown impl 3" in fit(impl=3) and "unknown impl -1" in fit(impl=-1)
    need = CW.scratch_bytes((4, 4, 4), 16, np.asarray(list(LEVELS)).reshape(3, 5))
    assert "scratch too small" in fit(scratch_bytes=need - 1) and "scratch too small" in fit(f=(64, 64, 64), scratch_bytes=need)


def test_wrapper_errors_need_no_device():
    c8, f32 = torch.zeros((2, 2, 2), dtype=torch.uint8), torch.zeros((2, 2, 2), dtype=torch.float32)
    d = torch.zeros((2, 2, 2, 3), dtype=torch.int32)
    h = torch.zeros((16, 17), dtype=torch.int32)
    for call in (lambda: CW.hist(c8, c8, 16, IDENTITY, d, 4), lambda: CW.sweep(c8, c8, 16, IDENTITY, d, 4, 256, 100), lambda: CW.fit(c8, c8, 16, IDENTITY),
                 lambda: CW.resample(f32, (2, 2, 2), IDENTITY, d, 4), lambda: CW.weights(h),
                 lambda: U.coreg.align(f32, (1, 1, 1), f32, (1, 1, 1), warp=CW.Plan())):
        with pytest.raises(U.UNetError, match="device tensor"):
            call()
    with pytest.raises(U.UNetError, match="warp must be a cowarp.Plan"):
        U.coreg.align(f32, (1, 1, 1), f32, (1, 1, 1), warp=7)
    with pytest.raises(U.UNetError, match="warp.limit"):
        U.coreg.align(f32, (1, 1, 1), f32, (1, 1, 1), warp=CW.Plan(limit=-1))
    with pytest.raises(U.UNetError, match="levels must be rows"):
        U.coreg.align(f32, (1, 1, 1), f32, (1, 1, 1), warp=CW.Plan(levels=[(4, 1, 1)]))
    # score: Python integers on a histogram, the restatement's
    rng = np.random.default_rng(4)
    for bins in (8, 16, 32):
        hist = rng.integers(0, 1000, (bins, bins + 1)).astype(np.uint32)
        assert CW.score(hist) == cr.score_py(hist) == cr.score_ref(hist)
    assert CW.score(np.zeros((8, 9), np.uint32)) == 0
    with pytest.raises(U.UNetError, match="bins, bins"):
        CW.score(np.zeros((8, 8)))
