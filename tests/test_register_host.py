"""CPU: the host half of the parcellation of a subject (include/unet_register.h, unet-studio_amd/register.py) -- the ABI the library
exports, argument errors found before any device call, the scratch size, centre_init, and this file's own restatements of the
header's definitions, checked on hand-written answers: `hist_ref`, `search_ref` and `carry_ref`.  They never import the package's
kernels; all position arithmetic is in np.float32, one rounding per operation.  The quality of the definition (does the pattern
search find a known affine map) is measured here, on the restatement, not on the device.  No device calls."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import torch

import unet_studio_amd as U
from unet_studio_amd import register as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
DEFAULT_STEP = [0.125] * 9 + [4, 4, 4]           # written out: the restatements do not read the module's values
DEFAULT_STAGES = [(4, 0, 2), (2, 1, 4), (1, 2, 6)]
IDENTITY = [1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0]


# ---- the restatements ------------------------------------------------------------------------------------------------------------
def read_tissue(tissue, T):
    """a value >= T reads as 0"""
    t = np.asarray(tissue).astype(np.int64)
    return np.where(t >= T, 0, t)


def locate(map12, x, y, z):
    """q = map(x, y, z) + 0.5 per axis: fp32, left to right, every product and every sum rounded"""
    m = np.asarray(map12, F).reshape(12)
    x, y, z = (np.asarray(v).astype(F) for v in (x, y, z))
    with np.errstate(all="ignore"):
        return [(((m[3 * r] * x + m[3 * r + 1] * y) + m[3 * r + 2] * z) + m[9 + r]) + F(0.5) for r in range(3)]


def nearest(q, tshape):
    """-> (inside, ix, iy, iz): inside when 0 <= q < float(dim) on every axis (a NaN is not); the index floor(q), read as -2 when it is
    below -2, above dim + 1 or NaN (no voxel of the 3x3x3 cube around it is inside there)"""
    td, th, tw = tshape
    inside = np.ones(np.shape(q[0]), bool)
    idx = []
    with np.errstate(all="ignore"):
        for v, dim in zip(q, (tw, th, td)):
            inside &= (v >= F(0)) & (v < F(dim))
            f = np.floor(v)
            ok = (f >= F(-2)) & (f <= F(dim + 1))
            idx.append(np.where(ok, f, F(-2)).astype(np.int64))
    return inside, idx[0], idx[1], idx[2]


def counted(sshape, stride):
    """the coordinates of the counted voxels, {n} each, x fastest"""
    sd, sh, sw = sshape
    z, y, x = np.meshgrid(np.arange(0, sd, stride), np.arange(0, sh, stride), np.arange(0, sw, stride), indexing="ij")
    return x.reshape(-1), y.reshape(-1), z.reshape(-1)


def hist_ref(subject, template, T, maps, stride=1):
    """uint32 {K, T, T}: hist[k][a][b] = the counted subject voxels with tissue a whose nearest template sample under map k reads b"""
    subject, template = np.asarray(subject), np.asarray(template)
    s, t = read_tissue(subject, T), read_tissue(template, T)
    x, y, z = counted(subject.shape, stride)
    a = s[z, y, x]
    out = []
    for m in np.asarray(maps, F).reshape(-1, 12):
        inside, ix, iy, iz = nearest(locate(m, x, y, z), template.shape)
        b = np.where(inside, t[np.where(inside, iz, 0), np.where(inside, iy, 0), np.where(inside, ix, 0)], 0)
        out.append(np.bincount(a * T + b, minlength=T * T).reshape(T, T))
    return np.stack(out).astype(np.uint32)


def score_ref(hist):
    """int: agree - disagree of one {T, T} histogram"""
    h = np.asarray(hist).astype(np.int64)
    diag = int(np.trace(h))
    return (diag - int(h[0, 0])) - (int(h.sum()) - diag)


def centre_of(sshape):
    sd, sh, sw = sshape
    return F(sw // 2), F(sh // 2), F(sd // 2)


def state_of(init, centre):
    """the 12 parameters of a map: its matrix, then the template position of the subject's centre voxel"""
    m = np.asarray(init, F).reshape(12)
    cx, cy, cz = centre
    return np.array(list(m[:9]) + [((m[3 * r] * cx + m[3 * r + 1] * cy) + m[3 * r + 2] * cz) + m[9 + r] for r in range(3)], F)


def map_of(c, centre):
    cx, cy, cz = centre
    return np.array(list(c[:9]) + [c[9 + r] - ((c[3 * r] * cx + c[3 * r + 1] * cy) + c[3 * r + 2] * cz) for r in range(3)], F)


def candidates_ref(c, step, level):
    """the states of one iteration: the state itself, then + and - for every parameter with step > 0, in ascending order"""
    out = [np.array(c, F)]
    for i in range(12):
        if F(step[i]) > 0:
            d = np.ldexp(F(step[i]), -level)
            assert d.dtype == F
            for moved in (c[i] + d, c[i] - d):
                n = np.array(c, F)
                n[i] = moved
                out.append(n)
    return out


def search_ref(subject, template, T, init, step=DEFAULT_STEP, stages=DEFAULT_STAGES, max_iterations=400):
    """-> (map float32 {12}, trace int64 {max_iterations, 4}, info int64 {4})"""
    subject = np.asarray(subject)
    centre = centre_of(subject.shape)
    c = state_of(init, centre)
    trace = np.full((max_iterations, 4), -1, np.int64)
    g, level = 0, stages[0][1]
    it, converged, last = 0, 0, (0, 0)
    while it < max_iterations and not converged:
        cands = candidates_ref(c, step, level)
        hists = hist_ref(subject, template, T, [map_of(k, centre) for k in cands], stages[g][0])
        scores = [score_ref(h) for h in hists]
        best = int(np.argmax(scores))                              # the first maximum: the lowest index among equal scores
        trace[it] = (g, level, best, scores[best])
        last = (scores[best], g)
        it += 1
        if best == 0:
            level += 1
            if level > stages[g][2]:
                g += 1
                if g == len(stages):
                    converged = 1
                else:
                    level = stages[g][1]
        else:
            c = cands[best]
    return map_of(c, centre), trace, np.array([it, converged, last[0], last[1]], np.int64)


def mode_ref(rows):
    """rows {k, N}: per column the most frequent non-zero entry, the smallest among equal counts (0 for none)"""
    count = (rows[:, None, :] == rows[None, :, :]).sum(1)
    count = np.where(rows != 0, count, 0)
    key = count * 65536 + (65535 - rows)
    j = np.argmax(key, axis=0)
    cols = np.arange(rows.shape[1])
    return np.where(count[j, cols] > 0, rows[j, cols], 0)


def carry_ref(subject, template, atlas, T, map12):
    """-> (regions uint16 of the subject's shape, counts uint32 {3, T}: direct, rescued, left per tissue)"""
    subject, template = np.asarray(subject), np.asarray(template)
    td, th, tw = template.shape
    s, t = read_tissue(subject, T), read_tissue(template, T)
    lab = np.asarray(atlas).astype(np.int64).reshape(template.shape)
    x, y, z = counted(subject.shape, 1)
    a = s[z, y, x]
    inside, ix, iy, iz = nearest(locate(map12, x, y, z), template.shape)
    cz_, cy_, cx_ = np.where(inside, iz, 0), np.where(inside, iy, 0), np.where(inside, ix, 0)
    direct = (a > 0) & inside & (t[cz_, cy_, cx_] == a) & (lab[cz_, cy_, cx_] != 0)
    out = np.where(direct, lab[cz_, cy_, cx_], 0)
    todo = np.flatnonzero((a > 0) & ~direct)
    rows = []
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                xx, yy, zz = ix[todo] + dx, iy[todo] + dy, iz[todo] + dz
                ok = (xx >= 0) & (xx < tw) & (yy >= 0) & (yy < th) & (zz >= 0) & (zz < td)
                xx, yy, zz = np.where(ok, xx, 0), np.where(ok, yy, 0), np.where(ok, zz, 0)
                rows.append(np.where(ok & (t[zz, yy, xx] == a[todo]), lab[zz, yy, xx], 0))
    got = mode_ref(np.stack(rows)) if todo.size else np.zeros(0, np.int64)
    out[todo] = got
    rescued = np.zeros(a.size, bool)
    rescued[todo] = got != 0
    left = (a > 0) & ~direct & ~rescued
    counts = np.stack([np.bincount(a[k], minlength=T) for k in (direct, rescued, left)]).astype(np.uint32)
    return out.astype(np.uint16).reshape(subject.shape), counts


def dice_ref(subject, template, T, map12):
    h = hist_ref(subject, template, T, [map12], 1)[0].astype(np.int64)
    agree = int(np.trace(h)) - int(h[0, 0])
    return 2.0 * agree / (int(h[1:].sum()) + int(h[:, 1:].sum())), agree


# ---- the ellipsoid case (shared with tests/test_gpu_register.py) -------------------------------------------------------------------------
TRUE_MAP = [1.1, .05, 0, -.04, .95, .03, 0, .02, 1.05, -3, 2.5, -1.5]


@functools.lru_cache(maxsize=None)
def ellipsoid_case():
    """-> (subject uint8 (38, 44, 40), template uint8 (36, 48, 40)): nested ellipsoids, the subject sampled through TRUE_MAP"""
    D, H, W = 36, 48, 40
    z, y, x = np.meshgrid(np.arange(D), np.arange(H), np.arange(W), indexing="ij")
    d = ((x - 19.5) / 15) ** 2 + ((y - 23.5) / 19) ** 2 + ((z - 17.5) / 14) ** 2
    template = np.zeros((D, H, W), np.uint8)
    template[d < 1] = 2
    template[d < 0.6] = 1
    template[d < 0.15] = 4
    template[(d < 1) & (z < 17.5 - 0.55 * 14)] = 3
    sshape = (38, 44, 40)
    sx, sy, sz = counted(sshape, 1)
    inside, ix, iy, iz = nearest(locate(TRUE_MAP, sx, sy, sz), template.shape)
    subject = np.where(inside, template[np.where(inside, iz, 0), np.where(inside, iy, 0), np.where(inside, ix, 0)], 0).astype(np.uint8)
    subject, template = subject.reshape(sshape), template
    subject.setflags(write=False)
    template.setflags(write=False)
    return subject, template


@functools.lru_cache(maxsize=None)
def ellipsoid_search():
    """search_ref on the ellipsoid case from centre_init with the defaults, computed once"""
    subject, template = ellipsoid_case()
    m, t = R.centre_init(subject.shape, (1, 1, 1), template.shape, (1, 1, 1))
    out = search_ref(subject, template, 5, list(m) + list(t))
    for a in out:
        a.setflags(write=False)
    return out


def vol(v):
    return np.array(v).reshape(1, 1, -1)


def shift(tx, ty=0, tz=0):
    return [1, 0, 0, 0, 1, 0, 0, 0, 1, tx, ty, tz]


# ---- hist_ref on hand-written answers --------------------------------------------------------------------------------------------------
def test_hist_a_position_at_minus_a_half_is_inside_and_one_at_dim_minus_a_half_is_outside():
    subject, template = vol([1, 1, 1]), vol([1, 2])
    # x -> x - 0.5: voxel 0 sits at -0.5 (q = 0, inside, index 0), voxel 1 at 0.5 (index 1), voxel 2 at 1.5 = dim - 0.5 (q = 2: outside)
    h = hist_ref(subject, template, 3, [shift(-0.5)])[0]
    assert h.tolist() == [[0, 0, 0], [1, 1, 1], [0, 0, 0]]
    # x -> x + 0.5: positions 0.5, 1.5, 2.5 -> template 2, outside, outside
    assert hist_ref(subject, template, 3, [shift(0.5)])[0][1].tolist() == [2, 0, 1]
    assert hist_ref(subject, template, 3, [IDENTITY])[0][1].tolist() == [1, 1, 1]
    assert h.dtype == np.uint32


def test_hist_a_nan_entry_sends_everything_outside_and_a_value_of_t_or_more_reads_0():
    subject, template = vol([1, 2, 7, 0]), vol([1, 2, 2, 9])
    nan_map = list(IDENTITY)
    nan_map[1] = float("nan")                                      # NaN * 0 is NaN: every position
    assert hist_ref(subject, template, 3, [nan_map])[0].tolist() == [[2, 0, 0], [1, 0, 0], [1, 0, 0]]
    # the 7 reads 0 on the subject side, the 9 reads 0 on the template side
    assert hist_ref(subject, template, 3, [IDENTITY])[0].tolist() == [[1, 0, 1], [0, 1, 0], [0, 0, 1]]
    both = hist_ref(subject, template, 3, [IDENTITY, nan_map])
    assert both.shape == (2, 3, 3) and both[1].tolist() == [[2, 0, 0], [1, 0, 0], [1, 0, 0]]


def test_hist_a_stride_larger_than_the_grid_counts_voxel_0_only():
    subject = np.arange(1, 7).reshape(1, 2, 3) % 3
    assert hist_ref(subject, subject, 3, [IDENTITY], 8)[0].tolist() == [[0, 0, 0], [0, 1, 0], [0, 0, 0]]
    assert hist_ref(subject, subject, 3, [IDENTITY], 2)[0].tolist() == [[1, 0, 0], [0, 1, 0], [0, 0, 0]]      # x = 0 and x = 2 of row 0
    assert int(hist_ref(subject, subject, 3, [IDENTITY], 1).sum()) == 6


def test_score_is_agree_minus_disagree_and_background_agreement_counts_nothing():
    assert score_ref([[100, 2, 0], [3, 10, 1], [0, 0, 5]]) == 15 - 6
    assert score_ref([[7, 0], [0, 0]]) == 0


# ---- search_ref on hand-written answers ------------------------------------------------------------------------------------------------
X_ONLY = [0] * 9 + [1, 0, 0]


def test_search_equal_scores_stay_on_candidate_0_and_levels_hand_over_to_the_next_stage():
    subject, template = vol([1, 1]), np.ones((9, 9, 9), np.int64)
    m, trace, info = search_ref(subject, template, 2, shift(4, 4, 4), DEFAULT_STEP, [(1, 0, 1), (2, 2, 3)], 10)
    # every candidate sees tissue 1 everywhere: a tie, candidate 0 at every level, levels 0, 1 of stage 0 then 2, 3 of stage 1
    assert trace[:4].tolist() == [[0, 0, 0, 2], [0, 1, 0, 2], [1, 2, 0, 1], [1, 3, 0, 1]] and (trace[4:] == -1).all()
    assert info.tolist() == [4, 1, 1, 1] and m.tolist() == shift(4, 4, 4) and m.dtype == np.float32
    # the last stage finished on the last iteration allowed: converged; one fewer: not
    assert search_ref(subject, template, 2, shift(4, 4, 4), DEFAULT_STEP, [(1, 0, 1), (2, 2, 3)], 4)[2].tolist() == [4, 1, 1, 1]
    assert search_ref(subject, template, 2, shift(4, 4, 4), DEFAULT_STEP, [(1, 0, 1), (2, 2, 3)], 3)[2].tolist() == [3, 0, 1, 1]


def test_search_a_tie_between_plus_and_minus_goes_to_plus():
    subject, template = vol([1]), vol([0, 1, 0, 1, 0])
    m, trace, info = search_ref(subject, template, 2, shift(2), X_ONLY, [(1, 0, 0)], 10)
    # at 2 the sample reads 0 (score -1); +1 and -1 both read 1 (score 1): candidate 1, the +; there nothing is better
    assert trace[:2].tolist() == [[0, 0, 1, 1], [0, 0, 0, 1]] and info.tolist() == [2, 1, 1, 0] and m.tolist() == shift(3)


def test_search_a_frozen_parameter_produces_no_candidates():
    c = state_of(IDENTITY, (F(1), F(2), F(3)))
    assert len(candidates_ref(c, DEFAULT_STEP, 0)) == 25 and len(candidates_ref(c, X_ONLY, 0)) == 3
    only = candidates_ref(c, [0, 0.5, 0, 0, 0, 0, 0, 0, 0, 0, 0, 3], 2)
    assert len(only) == 5 and [float(k[1]) for k in only] == [0, 0.125, -0.125, 0, 0] and [float(k[11]) for k in only] == [3, 3, 3, 3.75, 2.25]
    assert all(k.dtype == np.float32 for k in only)
    # the centred form: the state holds the template position of the centre voxel, the map gives it back
    assert c[9:].tolist() == [1, 2, 3] and map_of(c, (F(1), F(2), F(3))).tolist() == IDENTITY
    moved = map_of(only[1], (F(1), F(2), F(3)))                    # m1 + 0.125 turns about the centre: t0 = 1 - (1 + 0.125 * 2)
    assert moved[1] == 0.125 and moved[9:].tolist() == [-0.25, 0, 0]


def test_search_the_budget_cuts_it_short():
    subject, template = vol([1]), vol([0, 0, 0, 0, 0, 0, 1])
    full = search_ref(subject, template, 2, shift(3), X_ONLY, [(1, 0, 0)], 10)
    # at 3 every candidate reads 0: candidate 0, level 0 was the last: converged without ever moving
    assert full[2].tolist() == [1, 1, -1, 0]
    subject, template = vol([1]), vol([0, 1, 2, 2, 2, 2, 1, 0])
    walk = search_ref(subject, template, 3, shift(3), [0] * 9 + [4, 0, 0], [(1, 0, 2)], 2)
    # level 0 (+-4): outside either way, a tie at -1: candidate 0; level 1 (+-2): 5 reads 2, 1 reads 1: candidate 2, the budget ends
    assert walk[1].tolist() == [[0, 0, 0, -1], [0, 1, 2, 1]] and walk[2].tolist() == [2, 0, 1, 0] and walk[0].tolist() == shift(1)
    more = search_ref(subject, template, 3, shift(3), [0] * 9 + [4, 0, 0], [(1, 0, 2)], 3)
    assert more[1][2].tolist() == [0, 1, 0, 1] and more[2].tolist() == [3, 0, 1, 0]


# ---- carry_ref on hand-written answers -------------------------------------------------------------------------------------------------
def test_carry_direct_rescued_and_left():
    template, atlas = vol([1, 1, 2, 2, 0]), vol([7, 0, 9, 9, 5])
    subject = vol([1, 1, 2, 1, 2, 0])
    out, counts = carry_ref(subject, template, atlas, 3, IDENTITY)
    # 0: direct 7.  1: centre 0 in the atlas, the cube holds 7 in tissue 1: rescued.  2: direct 9.  3: centre in tissue 2, the cube
    # (2, 3, 4) holds no tissue 1: left.  4: centre tissue 0, the cube holds 9 in tissue 2: rescued.  5: tissue 0
    assert out.reshape(-1).tolist() == [7, 7, 9, 0, 9, 0] and out.dtype == np.uint16 and out.shape == subject.shape
    assert counts.tolist() == [[0, 1, 1], [0, 1, 1], [0, 1, 0]] and counts.dtype == np.uint32
    # a subject value >= T reads as 0: nothing, and it is in no count
    out, counts = carry_ref(vol([5]), template, atlas, 3, IDENTITY)
    assert out.reshape(-1).tolist() == [0] and int(counts.sum()) == 0


def test_carry_the_smallest_label_wins_among_equal_counts_and_the_more_frequent_wins():
    template = np.ones((1, 3, 3), np.int64)
    atlas = np.array([[[8, 3, 8], [3, 0, 0], [0, 0, 0]]])
    assert carry_ref(vol([1]), template, atlas, 2, shift(1, 1))[0].reshape(-1).tolist() == [3]       # two 8, two 3
    atlas = np.array([[[8, 3, 8], [3, 0, 8], [0, 0, 0]]])
    assert carry_ref(vol([1]), template, atlas, 2, shift(1, 1))[0].reshape(-1).tolist() == [8]       # three 8, two 3
    template = np.array([[[1, 1, 1], [1, 1, 2], [1, 1, 1]]])                                          # the third 8 is in another tissue
    assert carry_ref(vol([1]), template, atlas, 2 + 1, shift(1, 1))[0].reshape(-1).tolist() == [3]


def test_carry_an_index_outside_the_template_whose_cube_reaches_inside():
    template, atlas = vol([1, 1, 1]), vol([4, 0, 6])
    # x -> x - 1: voxel 0 sits at -1, outside, nearest index -1; its cube holds index 0.  x -> x + 3: index 3 = dim, cube holds 2
    out, counts = carry_ref(vol([1]), template, atlas, 2, shift(-1))
    assert out.reshape(-1).tolist() == [4] and counts.tolist() == [[0, 0], [0, 1], [0, 0]]
    assert carry_ref(vol([1]), template, atlas, 2, shift(3))[0].reshape(-1).tolist() == [6]
    # one further out, a NaN, an infinity: nothing in reach
    for far in (shift(-2), shift(4), shift(float("nan")), shift(float("inf")), shift(-3e38)):
        out, counts = carry_ref(vol([1]), template, atlas, 2, far)
        assert out.reshape(-1).tolist() == [0] and counts.tolist() == [[0, 0], [0, 0], [0, 1]]
    # the cube is clipped on every axis: y and z have one voxel
    assert carry_ref(vol([1]), template, atlas, 2, shift(1, 0.4, -0.4))[0].reshape(-1).tolist() == [4]


# ---- centre_init ----------------------------------------------------------------------------------------------------------------------
def test_centre_init_on_hand_worked_cases():
    m, t = R.centre_init((38, 44, 40), (1, 1, 1), (36, 48, 40), (1, 1, 1))
    assert m.tolist() == [1, 0, 0, 0, 1, 0, 0, 0, 1] and t.tolist() == [0, 2, -1] and m.dtype == t.dtype == np.float32
    # 2 mm subject voxels on a 1 mm template: the subject centre (5, 4, 3) goes to the template centre (10, 10, 8)
    m, t = R.centre_init((7, 8, 10), (2, 2, 2), (16, 20, 20), (1, 1, 1))
    assert m.tolist() == [2, 0, 0, 0, 2, 0, 0, 0, 2] and t.tolist() == [0, 2, 2]
    m, t = R.centre_init((4, 4, 4), (1, 1.5, 3), (9, 9, 9), (2, 1, 1))
    assert m.tolist() == [0.5, 0, 0, 0, 1.5, 0, 0, 0, 3] and t.tolist() == [3, 1, -2]
    c = state_of(list(m) + list(t), centre_of((4, 4, 4)))
    assert c[9:].tolist() == [4, 4, 4]                             # the centre voxels coincide
    for bad in (((4, 4), (1, 1, 1), (4, 4, 4), (1, 1, 1)), ((4, 4, 4), (1, 0, 1), (4, 4, 4), (1, 1, 1)),
                ((4, 4, 4), (1, 1, 1), (4, 0, 4), (1, 1, 1)), ((4, 4, 4), (1, 1, 1), (4, 4, 4), (1, float("nan"), 1))):
        with pytest.raises(U.UNetError):
            R.centre_init(*bad)
    assert R.DEFAULT_STEP == DEFAULT_STEP and [tuple(s) for s in R.DEFAULT_STAGES] == DEFAULT_STAGES


# ---- the quality of the definition ----------------------------------------------------------------------------------------------------------
def test_the_search_finds_the_map_of_the_ellipsoid_case():
    """Measured on the restatement: from centre_init at equal voxel sizes with the defaults the search must reach a Dice of at least
    0.99 at stride 1.  The pattern search is local: on m = [.9,0,.08, .06,1.1,0, -.05,0,.92], t = [4,-2,3] it stalls near 0.89
    (DESIGN.md §20); that case is not asserted on."""
    subject, template = ellipsoid_case()
    assert subject.shape == (38, 44, 40) and template.shape == (36, 48, 40)
    assert int((subject > 0).sum()) == 15248
    assert score_ref(hist_ref(subject, template, 5, [TRUE_MAP])[0]) == 15248
    m, trace, info = ellipsoid_search()
    dice, agree = dice_ref(subject, template, 5, m)
    print("ellipsoid case: %d iterations, converged %d, score %d, Dice %.4f (agree %d)" % (info[0], info[1], info[2], dice, agree))
    assert info[1] == 1 and info[3] == 2
    assert dice >= 0.99
    assert (trace[:info[0], 3][trace[:info[0], 0] == 2] <= 15248).all()


# ---- the ABI -------------------------------------------------------------------------------------------------------------------------
def test_unet_register_h_declares_exactly_the_exports_and_the_library_has_them():
    lib = ctypes.CDLL(U.engine.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "unet_register.h")).read()
    declared = set(re.findall(r"\b(unet_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(R.EXPORTS) == {"unet_reg_scratch_bytes", "unet_reg_hist", "unet_reg_search", "unet_reg_carry"}
    for name in sorted(declared):
        assert hasattr(lib, name), "libunet_hip.so does not export " + name
    enums = {k: int(v) for k, v in re.findall(r"UNET_REG_([A-Z_]+) = (\d+)", hdr)}
    assert enums == {"IMPL_DEFAULT": R.IMPL_DEFAULT, "IMPL_LDS": R.IMPL_LDS, "IMPL_GLOBAL": R.IMPL_GLOBAL}
    assert (R.IMPL_DEFAULT, R.IMPL_LDS, R.IMPL_GLOBAL) == (0, 1, 2)
    limits = {k: int(v) for k, v in re.findall(r"#define UNET_REG_MAX_([A-Z]+) (\d+)", hdr)}
    assert limits == {"TISSUES": R.MAX_TISSUES, "MAPS": R.MAX_MAPS, "STAGES": R.MAX_STAGES, "LEVEL": R.MAX_LEVEL,
                      "ITERATIONS": R.MAX_ITERATIONS}
    assert R.MAX_MAPS == 1 + 2 * 12 and R.MAX_MAPS * R.MAX_TISSUES ** 2 * 4 <= 64 * 1024           # a table a block can hold
    assert U.register is R


def test_the_other_headers_do_not_mention_the_new_prefix():
    for h in sorted(os.listdir(os.path.join(ROOT, "include"))):
        text = open(os.path.join(ROOT, "include", h)).read().lower()
        if h != "unet_register.h":
            assert "unet_reg_" not in text, h
        else:                                                      # what the other host tests forbid
            assert "unet_atlas_" not in text and "unet_components_" not in text and "unet_preproc_" not in text


# ---- argument errors, before any device call -------------------------------------------------------------------------------------
def test_scratch_bytes_is_monotone_and_checks_its_arguments():
    def mono(sizes):
        return all(a <= b for a, b in zip(sizes, sizes[1:]))
    by_t = [R.reg_scratch_bytes(1000, t, 10) for t in range(2, 17)]
    assert mono(by_t) and by_t[0] < by_t[-1] and by_t[-1] >= 25 * 16 * 16 * 4                       # the counters of 25 candidates
    assert mono([R.reg_scratch_bytes(v, 5, 10) for v in (1, 64, 1000, 10 ** 6, 256 ** 3, (1 << 31) - 1)])
    assert mono([R.reg_scratch_bytes(1000, 5, n) for n in (1, 2, 400, 1024)])
    for v, t, n, msg in ((0, 5, 1, "subject_voxels"), (1 << 31, 5, 1, "subject_voxels"), (10, 1, 1, "n_tissues"), (10, 17, 1, "n_tissues"),
                         (10, 5, 0, "max_iterations"), (10, 5, 1025, "max_iterations")):
        with pytest.raises(U.UNetError, match=msg):
            R.reg_scratch_bytes(v, t, n)
    rc = U.engine.lib.unet_reg_scratch_bytes(10, 5, 1, None)
    assert rc != 0 and "null output" in U.engine.lib.unet_last_error().decode()


P = [ctypes.c_void_p(0x1000 * (i + 1)) for i in range(8)]          # never dereferenced
F12 = (ctypes.c_float * 12)(*IDENTITY)


def grids_errors(call):
    assert "null subject" in call(subject=None) and "null template" in call(template=None)
    assert "sbytes must be 1 or 2, got 4" in call(sbytes=4) and "tbytes must be 1 or 2, got 0" in call(tbytes=0)
    assert "subject dimensions" in call(s=(0, 4, 4)) and "subject dimensions" in call(s=(4, 4, -1))
    assert "template dimensions" in call(t=(4, 0, 4))
    assert "subject grid" in call(s=(2048, 1024, 1024)) and "template grid" in call(t=(2048, 1024, 1024))
    assert "n_tissues must be in [2, 16], got 1" in call(T=1) and "n_tissues" in call(T=17)


def test_hist_argument_errors_need_no_device():
    lib = U.engine.lib
    maps = (ctypes.c_float * 300)()

    def call(subject=P[0], sbytes=1, s=(4, 4, 4), template=P[1], tbytes=2, t=(4, 4, 4), T=5, maps=maps, K=25, stride=1, hist=P[2], impl=0):
        rc = lib.unet_reg_hist(subject, sbytes, *s, template, tbytes, *t, T, maps, K, stride, hist, impl, None, 0, None)
        assert rc != 0
        return lib.unet_last_error().decode()

    grids_errors(call)
    assert "null maps" in call(maps=None) and "null hist" in call(hist=None)
    assert "K must be in [1, 25], got 0" in call(K=0) and "K must be" in call(K=26)
    assert "stride must be 1, 2, 4 or 8, got 3" in call(stride=3) and "stride" in call(stride=0) and "stride" in call(stride=16)
    assert "hist must be 4-byte aligned" in call(hist=ctypes.c_void_p(0x3002))
    assert "unknown impl 3" in call(impl=3) and "unknown impl -1" in call(impl=-1)


def test_search_argument_errors_need_no_device():
    lib = U.engine.lib
    step = (ctypes.c_float * 12)(*DEFAULT_STEP)
    stages = (ctypes.c_int * 9)(4, 0, 2, 2, 1, 4, 1, 2, 6)

    def floats(v):
        return (ctypes.c_float * 12)(*v)

    def ints(v):
        return (ctypes.c_int * len(v))(*v)

    def call(subject=P[0], sbytes=1, s=(4, 4, 4), template=P[1], tbytes=2, t=(4, 4, 4), T=5, init=F12, step=step, stages=stages, n_stages=3,
             n_it=10, map_out=P[2], trace=P[3], info=P[4], impl=0, scratch=P[5], scratch_bytes=1 << 40):
        rc = lib.unet_reg_search(subject, sbytes, *s, template, tbytes, *t, T, init, step, stages, n_stages, n_it, map_out, trace, info, impl,
                                 scratch, scratch_bytes, None)
        assert rc != 0
        return lib.unet_last_error().decode()

    grids_errors(call)
    assert "null init" in call(init=None) and "null step" in call(step=None) and "null stages" in call(stages=None)
    assert "step[3] must be finite and >= 0" in call(step=floats([1, 1, 1, -1] + [0] * 8))
    assert "step[11]" in call(step=floats([0] * 11 + [float("inf")])) and "step[0]" in call(step=floats([float("nan")] + [0] * 11))
    assert "at least one step" in call(step=floats([0] * 12))
    assert "n_stages must be in [1, 4], got 0" in call(n_stages=0) and "n_stages" in call(n_stages=5)
    assert "stage 1: stride must be 1, 2, 4 or 8, got 3" in call(stages=ints([4, 0, 2, 3, 1, 4, 1, 2, 6]))
    assert "stage 0: levels" in call(stages=ints([4, -1, 2]), n_stages=1) and "stage 0: levels" in call(stages=ints([4, 3, 2]), n_stages=1)
    assert "stage 2: levels" in call(stages=ints([4, 0, 2, 2, 1, 4, 1, 2, 21]))
    assert "max_iterations" in call(n_it=0) and "max_iterations" in call(n_it=1025)
    assert "null map_out" in call(map_out=None) and "null info" in call(info=None)
    assert "map_out must be 4-byte aligned" in call(map_out=ctypes.c_void_p(0x3001))
    assert "trace must be 8-byte aligned" in call(trace=ctypes.c_void_p(0x4004)) and "info must be 8-byte aligned" in call(info=ctypes.c_void_p(0x5004))
    assert "unknown impl 3" in call(impl=3)
    assert "null scratch" in call(scratch=None)
    assert "scratch too small" in call(scratch_bytes=R.reg_scratch_bytes(64, 5, 10) - 1)
    assert "scratch too small" in call(T=16, scratch_bytes=R.reg_scratch_bytes(64, 5, 10))


def test_carry_argument_errors_need_no_device():
    lib = U.engine.lib

    def call(subject=P[0], sbytes=2, s=(4, 4, 4), template=P[1], tbytes=1, t=(4, 4, 4), atlas=P[2], T=5, map=F12, out=P[3], counts=P[4]):
        rc = lib.unet_reg_carry(subject, sbytes, *s, template, tbytes, *t, atlas, T, map, out, counts, None)
        assert rc != 0
        return lib.unet_last_error().decode()

    grids_errors(call)
    assert "null atlas" in call(atlas=None) and "null map" in call(map=None) and "null out" in call(out=None)
    assert "atlas must be 2-byte aligned" in call(atlas=ctypes.c_void_p(0x3001)) and "out must be 2-byte aligned" in call(out=ctypes.c_void_p(0x4001))
    assert "counts must be 4-byte aligned" in call(counts=ctypes.c_void_p(0x5002))


def test_wrapper_errors_need_no_device():
    t8, a16 = torch.zeros((2, 2, 2), dtype=torch.uint8), torch.zeros((2, 2, 2), dtype=torch.uint16)
    with pytest.raises(U.UNetError, match="device tensor"):
        R.joint_hist(t8, t8, 5, [IDENTITY])
    with pytest.raises(U.UNetError, match="device tensor"):
        R.search(t8, t8, 5, IDENTITY)
    with pytest.raises(U.UNetError, match="device tensor"):
        R.carry(t8, t8, a16, 5, IDENTITY)
    with pytest.raises(U.UNetError, match="device tensor"):
        R.parcellate(t8, (1, 1, 1), t8, (1, 1, 1), a16)
