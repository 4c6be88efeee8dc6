"""The numpy restatements of include/unet_warp.h, shared by tests/test_warp_host.py (which checks them on hand-written answers) and
tests/test_gpu_warp.py (which pins the device to them bit for bit): `positions_ref`, `hist_ref`, `sweep_ref`, `refine_ref`,
`fit_ref`, `carry_ref`.  numpy only: nothing here calls the package's kernels; all position arithmetic is in np.float32, one rounding
per operation, all counting in int64.  A colour pass is vectorised over the whole volume: a voxel belongs to at most one support of
the colour, so the per-node sums of a candidate are one np.bincount."""
import functools
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_register_host import TRUE_MAP, counted, ellipsoid_case, mode_ref, nearest, read_tissue  # noqa: E402

F = np.float32
MAX_DISP, MAX_ROWS = 32767, 32                                     # written out: the restatements do not read the module's values
DEFAULT_LEVELS = [(16, 512, 128, 6), (8, 256, 64, 6), (4, 128, 64, 6)]
LG = {4: 2, 8: 3, 16: 4, 32: 5}


def lattice_ref(sshape, g):
    """(nz, ny, nx) of the lattice of spacing g over a (D, H, W) grid"""
    return tuple((int(d) + g - 1) // g + 1 for d in sshape)


def zero_field(sshape, g):
    return np.zeros(lattice_ref(sshape, g) + (3,), np.int32)


def corner_sums(D, g, x, y, z):
    """n {N, 3} int64: the 8 corners of each voxel's cell, weighted by the products of {g - f, f}"""
    D = np.asarray(D).astype(np.int64)
    lg = LG[g]
    cx, cy, cz, fx, fy, fz = x >> lg, y >> lg, z >> lg, x & (g - 1), y & (g - 1), z & (g - 1)
    n = np.zeros((x.size, 3), np.int64)
    for c in range(8):
        dx, dy, dz = c & 1, (c >> 1) & 1, c >> 2
        w = (fx if dx else g - fx) * (fy if dy else g - fy) * (fz if dz else g - fz)
        n += w[:, None] * D[cz + dz, cy + dy, cx + dx]
    return n


def affine_ref(map12, x, y, z):
    """p per axis: fp32, left to right, every product and every sum rounded"""
    m = np.asarray(map12, F).reshape(12)
    x, y, z = (np.asarray(v).astype(F) for v in (x, y, z))
    with np.errstate(all="ignore"):
        return [((m[3 * r] * x + m[3 * r + 1] * y) + m[3 * r + 2] * z) + m[9 + r] for r in range(3)]


def warped(p, n, g):
    """q = (p + ldexp(float32(n), -(8 + 3 lg))) + 0.5 per axis"""
    with np.errstate(all="ignore"):
        out = []
        for r in range(3):
            d = np.ldexp(n[:, r].astype(F), -(8 + 3 * LG[g]))
            assert d.dtype == F
            out.append((p[r] + d) + F(0.5))
        return out


def positions_ref(map12, D, g, sshape):
    """q {3 x N} float32 of every voxel of a (D, H, W) grid, x fastest"""
    x, y, z = counted(sshape, 1)
    return warped(affine_ref(map12, x, y, z), corner_sums(D, g, x, y, z), g)


def sample(t, q):
    """the nearest template tissue at positions q, 0 outside"""
    inside, ix, iy, iz = nearest(q, t.shape)
    return np.where(inside, t[np.where(inside, iz, 0), np.where(inside, iy, 0), np.where(inside, ix, 0)], 0)


def hist_ref(subject, template, T, map12, D, g):
    """uint32 {T, T}"""
    subject, template = np.asarray(subject), np.asarray(template)
    x, y, z = counted(subject.shape, 1)
    a = read_tissue(subject, T)[z, y, x]
    b = sample(read_tissue(template, T), positions_ref(map12, D, g, subject.shape))
    return np.bincount(a * T + b, minlength=T * T).reshape(T, T).astype(np.uint32)


def score_ref(hist):
    h = np.asarray(hist).astype(np.int64)
    diag = int(np.trace(h))
    return (diag - int(h[0, 0])) - (int(h.sum()) - diag)


def dice_ref(hist):
    h = np.asarray(hist).astype(np.int64)
    return 2.0 * (int(np.trace(h)) - int(h[0, 0])) / (int(h[1:].sum()) + int(h[:, 1:].sum()))


def owner(x, g, parity):
    """the node of `parity` along one axis whose open support (i-1)g < x < (i+1)g holds x, -1 for none"""
    cell, f = x >> LG[g], x & (g - 1)
    return np.where((cell & 1) == parity, cell, np.where(f == 0, -1, cell + 1))


def admissible_ref(D, step, limit):
    """bool {7, nz, ny, nx}: candidate 0 always; a moved one when its moved component stays within +-MAX_DISP and every component
    stays within `limit` of each lattice neighbour that exists"""
    D = np.asarray(D).astype(np.int64)
    adm = np.ones((7,) + D.shape[:3], bool)
    idx = np.indices(D.shape[:3])
    for c in range(1, 7):
        axis = (c - 1) // 2
        cand = D.copy()
        cand[..., axis] += step if c & 1 else -step
        ok = np.abs(cand[..., axis]) <= MAX_DISP
        for arr_axis in range(3):
            for s in (-1, 1):
                exists = (idx[arr_axis] + s >= 0) & (idx[arr_axis] + s < D.shape[arr_axis])
                nb = np.roll(D, -s, axis=arr_axis)
                ok &= (np.abs(cand - nb) <= limit).all(-1) | ~exists
        adm[c] = ok
    return adm


def sweep_ref(subject, template, T, map12, D, g, step, limit, scores_out=None, after_pass=None):
    """-> (the field after one sweep, int32 like D; info int64 {2} = nodes changed, nodes visited).  scores_out: a list that receives
    per colour (nodes visited, their int64 {7, n} local scores, their admissibility) for the hand-written tests; after_pass: called
    with the field after every colour pass"""
    subject, template = np.asarray(subject), np.asarray(template)
    D = np.array(D, np.int64)
    nz, ny, nx = D.shape[:3]
    assert (nz, ny, nx) == lattice_ref(subject.shape, g)
    x, y, z = counted(subject.shape, 1)
    a_all, t = read_tissue(subject, T)[z, y, x], read_tissue(template, T)
    p_all = affine_ref(map12, x, y, z)
    changed = visited = 0
    for c in range(8):
        i, j, k = owner(x, g, c & 1), owner(y, g, (c >> 1) & 1), owner(z, g, c >> 2)
        act = (i >= 0) & (j >= 0) & (k >= 0)
        xa, ya, za, ia, ja, ka, a = x[act], y[act], z[act], i[act], j[act], k[act], a_all[act]
        p = [v[act] for v in p_all]
        node = (ka * ny + ja) * nx + ia
        n = corner_sums(D, g, xa, ya, za)
        ws = (g - np.abs(xa - ia * g)) * (g - np.abs(ya - ja * g)) * (g - np.abs(za - ka * g)) * step
        scores = np.zeros((7, nz * ny * nx), np.int64)
        for cand in range(7):
            nn = n.copy()
            if cand:
                nn[:, (cand - 1) // 2] += ws if cand & 1 else -ws
            b = sample(t, warped(p, nn, g))
            vote = np.where(a == b, (a > 0).astype(np.int64), -1)
            scores[cand] = np.bincount(node, weights=vote, minlength=nz * ny * nx).astype(np.int64)
        nodes = np.flatnonzero(np.bincount(node, minlength=nz * ny * nx))      # the colour's nodes whose support is not empty
        adm = admissible_ref(D, step, limit).reshape(7, -1)[:, nodes]
        local = scores[:, nodes]
        best = np.argmax(np.where(adm, local, np.iinfo(np.int64).min), axis=0)   # the first maximum: the lowest index among equals
        if scores_out is not None:
            scores_out.append((nodes, local, adm))
        flat = D.reshape(-1, 3)
        moved = best > 0
        flat[nodes[moved], (best[moved] - 1) // 2] += np.where(best[moved] & 1, step, -step)
        changed += int(moved.sum())
        visited += nodes.size
        if after_pass is not None:
            after_pass(D.astype(np.int32))
    return D.astype(np.int32), np.array([changed, visited], np.int64)


def refine_ref(D, sshape, g):
    """the field on the lattice of g // 2: fine node = (the sum of the 8 combinations of coarse indices + 4) >> 3"""
    D = np.asarray(D).astype(np.int64)
    assert D.shape[:3] == lattice_ref(sshape, g)
    fine = lattice_ref(sshape, g // 2)
    pairs = []
    for n_f, n_c in zip(fine, D.shape[:3]):
        i = np.arange(n_f)
        pairs.append((i >> 1, np.minimum((i >> 1) + (i & 1), n_c - 1)))
    total = np.zeros(fine + (3,), np.int64)
    for kz in pairs[0]:
        for jy in pairs[1]:
            for ix in pairs[2]:
                total += D[kz[:, None, None], jy[None, :, None], ix[None, None, :]]
    return ((total + 4) >> 3).astype(np.int32)


def default_limit_ref(map12, g):
    m = np.asarray(map12, F).reshape(12)[:9].astype(np.float64).reshape(3, 3)
    return int(math.floor(64.0 * g * max(float(np.sqrt((m * m).sum(0)).min()), 0.25)))


def levels_ref(map12, levels=DEFAULT_LEVELS, limit=None):
    return [tuple(lv) + ((default_limit_ref(map12, lv[0]) if limit is None else limit,) if len(lv) == 4 else ()) for lv in levels]


def fit_ref(subject, template, T, map12, levels=None):
    """levels: rows of (g, first_step, last_step, max_sweeps, limit).  -> (D int32 on the last level's lattice, report int64
    {MAX_ROWS, 5}: g, step, sweeps run, nodes changed in the last sweep run, the score after it; -1 past the schedule)"""
    subject = np.asarray(subject)
    levels = levels_ref(map12) if levels is None else levels
    report = np.full((MAX_ROWS, 5), -1, np.int64)
    D, row = zero_field(subject.shape, levels[0][0]), 0
    for l, (g, first, last, max_sweeps, limit) in enumerate(levels):
        step = first
        while step >= last:
            ran = 0
            for _ in range(max_sweeps):
                D, info = sweep_ref(subject, template, T, map12, D, g, step, limit)
                ran += 1
                if info[0] == 0:
                    break
            report[row] = (g, step, ran, info[0], score_ref(hist_ref(subject, template, T, map12, D, g)))
            row += 1
            step //= 2
        if l + 1 < len(levels):
            D = refine_ref(D, subject.shape, g)
    return D, report


def carry_ref(subject, template, atlas, T, map12, D, g):
    """test_register_host.carry_ref's rules at the warped positions -> (regions uint16, counts uint32 {3, T})"""
    subject, template = np.asarray(subject), np.asarray(template)
    td, th, tw = template.shape
    s, t = read_tissue(subject, T), read_tissue(template, T)
    lab = np.asarray(atlas).astype(np.int64).reshape(template.shape)
    x, y, z = counted(subject.shape, 1)
    a = s[z, y, x]
    inside, ix, iy, iz = nearest(positions_ref(map12, D, g, subject.shape), template.shape)
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


# ---- the warped ellipsoid case (shared by the host and the GPU tests) -----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def warped_case():
    """-> (subject uint8 (38, 44, 40), template uint8 (36, 48, 40)): test_register_host's ellipsoid template sampled at TRUE_MAP's
    positions plus a smooth warp of about 2 voxels: 2 sin(y / 7), 2 cos(z / 6), 1.5 sin(x / 8 + 1) per component (float64 -> fp32)"""
    _, template = ellipsoid_case()
    sshape = (38, 44, 40)
    x, y, z = counted(sshape, 1)
    p = affine_ref(TRUE_MAP, x, y, z)
    d = [(2 * np.sin(y / 7.0)).astype(F), (2 * np.cos(z / 6.0)).astype(F), (1.5 * np.sin(x / 8.0 + 1)).astype(F)]
    subject = sample(np.asarray(template), [(p[r] + d[r]) + F(0.5) for r in range(3)]).astype(np.uint8).reshape(sshape)
    subject.setflags(write=False)
    return subject, template


@functools.lru_cache(maxsize=None)
def warped_fit():
    """fit_ref on the warped ellipsoid case from TRUE_MAP with the defaults, computed once"""
    subject, template = warped_case()
    out = fit_ref(subject, template, 5, TRUE_MAP)
    for a in out:
        a.setflags(write=False)
    return out
