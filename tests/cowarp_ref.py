"""The numpy restatements of include/unet_cowarp.h, shared by tests/test_cowarp_host.py (which checks them on hand-written answers)
and tests/test_gpu_cowarp.py (which pins the device to them bit for bit): `hist_ref`, `weights_ref`, `sweep_ref`, `fit_ref`,
`resample_ref`.  numpy only: nothing here calls the package's kernels.  The positions, the owner of a voxel, admissibility and refine
are tests/warp_ref.py's; the integer logarithm, the score and the codes are tests/coreg_ref.py's; the trilinear rule is
oracle/augment_ref.py's (what tests/test_gpu_space.py pins unet_space_resample to).  All counting is in int64."""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import coreg_ref as cr  # noqa: E402
import warp_ref as wr  # noqa: E402
from oracle import augment_ref as ar  # noqa: E402
from test_register_host import TRUE_MAP  # noqa: E402

F = np.float32
MAX_ROWS, MAX_SUPPORT = 32, 29791                                  # written out: the restatements do not read the module's values
SPACINGS = (4, 8, 16)


def sample(m, bins, q):
    """the nearest moving code at positions q, `bins` outside; m: the codes as read"""
    inside, ix, iy, iz = cr.nearest(q, m.shape)
    return np.where(inside, m[iz, iy, ix], bins)


def hist_ref(fixed, moving, bins, map12, D, g):
    """uint32 {bins, bins + 1}: every fixed voxel whose code is < bins, under its warped nearest position"""
    fixed, moving = np.asarray(fixed), np.asarray(moving)
    f, m = cr.read_code(fixed, bins), cr.read_code(moving, bins)
    x, y, z = cr.counted(fixed.shape, 1)
    a = f[z, y, x]
    keep = a < bins
    x, y, z, a = x[keep], y[keep], z[keep], a[keep]
    b = sample(m, bins, wr.warped(wr.affine_ref(map12, x, y, z), wr.corner_sums(D, g, x, y, z), g))
    return np.bincount(a * (bins + 1) + b, minlength=bins * (bins + 1)).reshape(bins, bins + 1).astype(np.uint32)


def weights_wide(hist):
    """int64 {bins, bins + 1}: the table before it is stored as int16"""
    h = np.asarray(hist).astype(np.int64)
    bins = h.shape[0]
    assert h.shape == (bins, bins + 1)
    r = h.sum(1) & 0xFFFFFFFF
    c = h[:, :bins].sum(0) & 0xFFFFFFFF
    ln = cr.ilog_np(np.array([int(h.sum()) & 0xFFFFFFFF]))[0]
    inner = (cr.ilog_np(h[:, :bins]) + ln - cr.ilog_np(r)[:, None] - cr.ilog_np(c)[None, :]) >> 8    # arithmetic
    return np.concatenate([inner, np.minimum(0, inner.min(1))[:, None]], axis=1)


def weights_ref(hist):
    """int16 {bins, bins + 1}"""
    return weights_wide(hist).astype(np.int16)


def total_ref(hist, W):
    """the frozen-W total of a histogram"""
    return int((np.asarray(hist).astype(np.int64) * np.asarray(W).astype(np.int64)).sum())


def sweep_ref(fixed, moving, bins, map12, D, g, step, limit, scores_out=None, after_pass=None, check_total=True):
    """-> (the field after one sweep, int32 like D; info int64 {2} = nodes changed, nodes visited).  scores_out: a list that receives
    per colour (nodes visited, their int64 {7, n} local scores, their admissibility); after_pass: called with the field after every
    colour pass; check_total: assert that the frozen-W total never decreases across a pass"""
    fixed, moving = np.asarray(fixed), np.asarray(moving)
    assert g in SPACINGS
    D = np.array(D, np.int64)
    nz, ny, nx = D.shape[:3]
    assert (nz, ny, nx) == wr.lattice_ref(fixed.shape, g)
    W = weights_ref(hist_ref(fixed, moving, bins, map12, D, g)).astype(np.int64)
    f, m = cr.read_code(fixed, bins), cr.read_code(moving, bins)
    x, y, z = cr.counted(fixed.shape, 1)
    a_all = f[z, y, x]
    keep = a_all < bins                                            # a fixed "none" voxel is in no support
    x, y, z, a_all = x[keep], y[keep], z[keep], a_all[keep]
    p_all = wr.affine_ref(map12, x, y, z)
    total = total_ref(hist_ref(fixed, moving, bins, map12, D, g), W) if check_total else 0
    changed = visited = 0
    for c in range(8):
        i, j, k = wr.owner(x, g, c & 1), wr.owner(y, g, (c >> 1) & 1), wr.owner(z, g, c >> 2)
        act = (i >= 0) & (j >= 0) & (k >= 0)
        xa, ya, za, ia, ja, ka, a = x[act], y[act], z[act], i[act], j[act], k[act], a_all[act]
        p = [v[act] for v in p_all]
        node = (ka * ny + ja) * nx + ia
        n = wr.corner_sums(D, g, xa, ya, za)
        ws = (g - np.abs(xa - ia * g)) * (g - np.abs(ya - ja * g)) * (g - np.abs(za - ka * g)) * step
        scores = np.zeros((7, nz * ny * nx), np.int64)
        for cand in range(7):
            nn = n.copy()
            if cand:
                nn[:, (cand - 1) // 2] += ws if cand & 1 else -ws
            b = sample(m, bins, wr.warped(p, nn, g))
            scores[cand] = np.bincount(node, weights=W[a, b], minlength=nz * ny * nx).astype(np.int64)
        count = np.bincount(node, minlength=nz * ny * nx)
        assert count.max(initial=0) <= MAX_SUPPORT and np.abs(scores).max(initial=0) < 1 << 29
        nodes = np.flatnonzero(count)                              # the colour's nodes whose support holds a voxel with a code
        adm = wr.admissible_ref(D, step, limit).reshape(7, -1)[:, nodes]
        local = scores[:, nodes]
        best = np.argmax(np.where(adm, local, np.iinfo(np.int64).min), axis=0)   # the first maximum: the lowest index among equals
        if scores_out is not None:
            scores_out.append((nodes, local, adm))
        flat = D.reshape(-1, 3)
        moved = best > 0
        flat[nodes[moved], (best[moved] - 1) // 2] += np.where(best[moved] & 1, step, -step)
        changed += int(moved.sum())
        visited += nodes.size
        if check_total:
            now = total_ref(hist_ref(fixed, moving, bins, map12, D, g), W)
            assert now >= total, (c, total, now)
            total = now
        if after_pass is not None:
            after_pass(D.astype(np.int32))
    return D.astype(np.int32), np.array([changed, visited], np.int64)


def fit_ref(fixed, moving, bins, map12, levels=None, check_total=True):
    """levels: rows of (g, first_step, last_step, max_sweeps, limit).  -> (D int32 on the last level's lattice, report int64
    {MAX_ROWS, 5}: g, step, sweeps run, nodes changed in the last sweep run, N * MI after it; -1 past the schedule)"""
    fixed = np.asarray(fixed)
    levels = wr.levels_ref(map12) if levels is None else levels
    report = np.full((MAX_ROWS, 5), -1, np.int64)
    D, row = wr.zero_field(fixed.shape, levels[0][0]), 0
    for l, (g, first, last, max_sweeps, limit) in enumerate(levels):
        step = first
        while step >= last:
            ran = 0
            for _ in range(max_sweeps):
                D, info = sweep_ref(fixed, moving, bins, map12, D, g, step, limit, check_total=check_total)
                ran += 1
                if info[0] == 0:
                    break
            report[row] = (g, step, ran, info[0], cr.score_ref(hist_ref(fixed, moving, bins, map12, D, g)))
            row += 1
            step //= 2
        if l + 1 < len(levels):
            D = wr.refine_ref(D, fixed.shape, g)
    return D, report


def resample_ref(moving, fshape, map12, D, g):
    """float32 {fd, fh, fw}: the moving volume at p' = p + ldexp(float32(n), -(8 + 3 lg)) under the LINEAR rule, 0 outside"""
    moving = np.asarray(moving, F)
    md, mh, mw = moving.shape
    x, y, z = cr.counted(fshape, 1)
    p, n = wr.affine_ref(map12, x, y, z), wr.corner_sums(D, g, x, y, z)
    with np.errstate(all="ignore"):
        q = [p[r] + np.ldexp(n[:, r].astype(F), -(8 + 3 * wr.LG[g])) for r in range(3)]
        assert all(v.dtype == F for v in q)
        return ar._trilinear(moving, ar._locate(q[0], q[1], q[2], mw, mh, md)).reshape(fshape)


# ---- the shared case: two contrasts of the warped ellipsoid -----------------------------------------------------------------------------
FIXED_LEVEL, MOVING_LEVEL = [0.05, 0.55, 0.85, 0.30, 0.70], [0.05, 0.80, 0.35, 0.60, 0.15]


def contrast_pair(subject, template, seed=5, bins=16):
    """two code images of one anatomy: each tissue gets a grey level per image, plus N(0, 0.04) noise from one generator (the fixed
    image first)"""
    rng = np.random.default_rng(seed)
    out = []
    for levels, lab in ((FIXED_LEVEL, subject), (MOVING_LEVEL, template)):
        lab = np.asarray(lab)
        c = cr.code_ref(np.asarray(levels)[lab] + rng.normal(0, 0.04, lab.shape), 0, 1, bins)
        c.setflags(write=False)
        out.append(c)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def warped_codes():
    """-> (fixed uint8 (38, 44, 40), moving uint8 (36, 48, 40)), 16 bins: warp_ref.warped_case() in two contrasts"""
    return contrast_pair(*wr.warped_case())


@functools.lru_cache(maxsize=None)
def warped_fit(check_total=False):
    """fit_ref on warped_codes() from TRUE_MAP with the defaults, computed once (check_total doubles its time: the host test asks
    for it, the device tests do not)"""
    fixed, moving = warped_codes()
    out = fit_ref(fixed, moving, 16, TRUE_MAP, check_total=check_total)
    for a in out:
        a.setflags(write=False)
    return out
