"""The numpy restatements of include/unet_coreg.h and the phantom its tests share (tests/test_coreg_host.py on the CPU,
tests/test_gpu_coreg.py against the device).  Nothing here imports the package: `code_ref`, `hist_ref`, `ilog`, `score_ref` and
`search_ref` restate the header from its text.  All position arithmetic is in np.float32, one rounding per operation; every score is
made of integers."""
import functools

import numpy as np

F = np.float32
IDENTITY = [1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0]
PHANTOM_STEP = [0.08] * 9 + [4] * 3
PHANTOM_STAGES = [(2, 0, 3), (1, 1, 6)]


# ---- codes -----------------------------------------------------------------------------------------------------------------------
def code_ref(image, lo, hi, bins):
    """uint8 of image's shape: 0 for t < 0, bins - 1 for t >= bins - 1, otherwise int(t), t = (v - lo) * scale in fp32 with
    scale = float32(bins) / (hi - lo); a NaN becomes `bins`"""
    v = np.asarray(image, F)
    lo, hi = F(lo), F(hi)
    scale = F(bins) / F(hi - lo)
    assert scale.dtype == F
    with np.errstate(all="ignore"):
        t = (v - lo) * scale
    assert t.dtype == F
    nan = np.isnan(t)
    whole = np.clip(np.where(nan, F(0), t), F(0), F(bins - 1)).astype(np.int64)   # t < 0 -> 0, t >= bins - 1 -> bins - 1, else trunc
    return np.where(nan, bins, whole).astype(np.uint8)


def read_code(codes, bins):
    """a value above bins reads as `bins`"""
    c = np.asarray(codes).astype(np.int64)
    return np.where(c > bins, bins, c)


# ---- positions (the text of unet_register.h, restated) -------------------------------------------------------------------------------
def locate(map12, x, y, z):
    """q = map(x, y, z) + 0.5 per axis: fp32, left to right, every product and every sum rounded"""
    m = np.asarray(map12, F).reshape(12)
    x, y, z = (np.asarray(v).astype(F) for v in (x, y, z))
    with np.errstate(all="ignore"):
        return [(((m[3 * r] * x + m[3 * r + 1] * y) + m[3 * r + 2] * z) + m[9 + r]) + F(0.5) for r in range(3)]


def nearest(q, mshape):
    """-> (inside, ix, iy, iz): inside when 0 <= q < float(dim) on every axis (a NaN is not); the indices are 0 where outside"""
    md, mh, mw = mshape
    inside = np.ones(np.shape(q[0]), bool)
    with np.errstate(all="ignore"):
        for v, dim in zip(q, (mw, mh, md)):
            inside &= (v >= F(0)) & (v < F(dim))
        idx = [np.where(inside, np.floor(v), F(0)).astype(np.int64) for v in q]
    return inside, idx[0], idx[1], idx[2]


def counted(fshape, stride):
    """the coordinates of the counted voxels, {n} each, x fastest"""
    fd, fh, fw = fshape
    z, y, x = np.meshgrid(np.arange(0, fd, stride), np.arange(0, fh, stride), np.arange(0, fw, stride), indexing="ij")
    return x.reshape(-1), y.reshape(-1), z.reshape(-1)


# ---- joint histograms ------------------------------------------------------------------------------------------------------------
def hist_ref(fixed, moving, bins, maps, stride=1):
    """uint32 {K, bins, bins + 1}: hist[k][a][b] = the counted fixed voxels with code a < bins whose nearest moving voxel under map k
    has the code b; b = bins outside or for a moving code `bins`"""
    fixed, moving = np.asarray(fixed), np.asarray(moving)
    f, m = read_code(fixed, bins), read_code(moving, bins)
    x, y, z = counted(fixed.shape, stride)
    a = f[z, y, x]
    keep = a < bins
    x, y, z, a = x[keep], y[keep], z[keep], a[keep]
    out = []
    for m12 in np.asarray(maps, F).reshape(-1, 12):
        inside, ix, iy, iz = nearest(locate(m12, x, y, z), moving.shape)
        b = np.where(inside, m[iz, iy, ix], bins)
        out.append(np.bincount(a * (bins + 1) + b, minlength=bins * (bins + 1)).reshape(bins, bins + 1))
    return np.stack(out).astype(np.uint32)


def counted_kept(fixed, bins, stride):
    """the number of counted fixed voxels whose code is not `none`: every histogram's total"""
    f = read_code(fixed, bins)
    return int((f[::stride, ::stride, ::stride] < bins).sum())


# ---- the integer logarithm and the score -------------------------------------------------------------------------------------------
def ilog(n):
    """L(n) in Python integers, from the header's text"""
    n = int(n)
    if n == 0:
        return 0
    e = n.bit_length() - 1                                         # 31 - clz(n)
    x = (n << (31 - e)) & 0xFFFFFFFF
    f = 0
    for _ in range(16):
        y = (x * x) >> 31
        if y >= 1 << 32:
            f = 2 * f + 1
            x = y >> 1
        else:
            f = 2 * f
            x = y
    return (e << 16) | f


def ilog_np(n):
    """ilog on an array of values below 2^32 (uint64 arithmetic: x * x stays below 2^64); checked against ilog by the host test"""
    n = np.asarray(n).astype(np.uint64)
    some = n > 0
    safe = np.where(some, n, 1)
    e = np.zeros(n.shape, np.uint64)
    for k in (16, 8, 4, 2, 1):                                     # floor(log2(n)) by halving
        up = (safe >> (e + np.uint64(k))) > 0
        e = np.where(up, e + np.uint64(k), e)
    x = (safe << (np.uint64(31) - e)) & np.uint64(0xFFFFFFFF)
    f = np.zeros(n.shape, np.uint64)
    for _ in range(16):
        y = (x * x) >> np.uint64(31)
        big = y >= np.uint64(1 << 32)
        f = f * np.uint64(2) + big.astype(np.uint64)
        x = np.where(big, y >> np.uint64(1), y)
    return np.where(some, (e << np.uint64(16)) | f, 0).astype(np.int64)


def score_py(hist):
    """int: the score of one {bins, bins + 1} histogram, in Python integers only"""
    h = [[int(v) for v in row] for row in np.asarray(hist)]
    bins = len(h)
    assert all(len(row) == bins + 1 for row in h)
    r = [sum(row) & 0xFFFFFFFF for row in h]
    c = [sum(h[a][b] for a in range(bins)) & 0xFFFFFFFF for b in range(bins)]
    ln = ilog(sum(sum(row) for row in h) & 0xFFFFFFFF)
    return sum(h[a][b] * (ilog(h[a][b]) + ln - ilog(r[a]) - ilog(c[b])) for a in range(bins) for b in range(bins))


def score_ref(hist):
    """int: score_py, vectorised (int64 holds every term: the magnitude stays below 2^54)"""
    h = np.asarray(hist).astype(np.int64)
    bins = h.shape[0]
    r = h.sum(1) & 0xFFFFFFFF
    c = h[:, :bins].sum(0) & 0xFFFFFFFF
    ln = ilog_np(np.array([int(h.sum()) & 0xFFFFFFFF]))[0]
    inner = h[:, :bins]
    return int((inner * (ilog_np(inner) + ln - ilog_np(r)[:, None] - ilog_np(c)[None, :])).sum())


# ---- the search (the state machine of unet_register.h, restated) ----------------------------------------------------------------------
def centre_of(fshape):
    fd, fh, fw = fshape
    return F(fw // 2), F(fh // 2), F(fd // 2)


def state_of(init, centre):
    """the 12 parameters of a map: its matrix, then the moving position of the fixed grid's centre voxel"""
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


def search_ref(fixed, moving, bins, init, step=PHANTOM_STEP, stages=PHANTOM_STAGES, max_iterations=400):
    """-> (map float32 {12}, trace int64 {max_iterations, 4}, info int64 {4})"""
    fixed = np.asarray(fixed)
    centre = centre_of(fixed.shape)
    c = state_of(init, centre)
    trace = np.full((max_iterations, 4), -1, np.int64)
    g, level = 0, stages[0][1]
    it, converged, last = 0, 0, (0, 0)
    while it < max_iterations and not converged:
        cands = candidates_ref(c, step, level)
        hists = hist_ref(fixed, moving, bins, [map_of(k, centre) for k in cands], stages[g][0])
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


# ---- the phantom -----------------------------------------------------------------------------------------------------------------------
def blob_volume(seed, n):
    """twelve Gaussian blobs from default_rng(seed) on an n^3 grid; per blob, in this order: the centre (x, y, z) uniform in
    [0.2 n, 0.8 n], sigma uniform in [0.08 n, 0.2 n], the amplitude uniform in [0.3, 1]"""
    rng = np.random.default_rng(seed)
    z, y, x = np.indices((n, n, n)).astype(np.float64)
    v = np.zeros((n, n, n))
    for _ in range(12):
        cx, cy, cz = rng.uniform(0.2 * n, 0.8 * n, 3)
        sigma = rng.uniform(0.08 * n, 0.2 * n)
        amp = rng.uniform(0.3, 1.0)
        v += amp * np.exp(-((x - cx) ** 2 + (y - cy) ** 2 + (z - cz) ** 2) / (2 * sigma ** 2))
    return v


def moving_to_fixed(n):
    """(matrix {3, 3}, translation {3}) float64: a moving voxel -> its fixed position.  A 5 degree rotation about z with the rows
    scaled by 1.04, 0.97 and 1, and a translation of (2, -1.5, 1), about the grid's centre voxel n // 2"""
    a = np.deg2rad(5.0)
    rot = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    m = np.diag([1.04, 0.97, 1.0]) @ rot
    c = np.full(3, float(n // 2))
    return m, c + np.array([2.0, -1.5, 1.0]) - m @ c


def true_map(n):
    """(matrix, translation) float64: a fixed voxel -> its moving position, the inverse of moving_to_fixed"""
    m, t = moving_to_fixed(n)
    inv = np.linalg.inv(m)
    return inv, -inv @ t


def sample_linear(vol, m, t, shape):
    """vol seen through (m, t) on a (D, H, W) grid: trilinear in float64, positions clamped to the grid (the border repeats)"""
    z, y, x = np.indices(shape).astype(np.float64)
    p = [np.clip(m[r, 0] * x + m[r, 1] * y + m[r, 2] * z + t[r], 0, dim - 1) for r, dim in zip(range(3), vol.shape[::-1])]
    i0 = [np.minimum(np.floor(v).astype(np.int64), dim - 2) for v, dim in zip(p, vol.shape[::-1])]
    w = [v - i for v, i in zip(p, i0)]
    out = np.zeros(shape)
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                wt = (w[0] if dx else 1 - w[0]) * (w[1] if dy else 1 - w[1]) * (w[2] if dz else 1 - w[2])
                out += wt * vol[i0[2] + dz, i0[1] + dy, i0[0] + dx]
    return out


@functools.lru_cache(maxsize=None)
def phantom(n=32):
    """-> (fixed, moving) float32 {n, n, n}, read only.
    fixed   the seed-1 blob volume over its maximum, cut at 0.15, 0.35 and 0.6, the class index over 3; plus 0.15 times the seed-2
            blob volume over its maximum; plus 0.02 N(0, 1) from default_rng(5).
    moving  1 - sqrt(fixed / max(fixed)) (negative noise read as 0) seen through moving_to_fixed, sampled linearly, plus 0.02 N(0, 1)
            from default_rng(0): another contrast of the same anatomy on a rotated, scaled and shifted grid."""
    b1, b2 = blob_volume(1, n), blob_volume(2, n)
    classes = np.digitize(b1 / b1.max(), [0.15, 0.35, 0.6]) / 3.0
    fixed = classes + 0.15 * b2 / b2.max() + 0.02 * np.random.default_rng(5).standard_normal((n, n, n))
    other = 1.0 - np.sqrt(np.clip(fixed / fixed.max(), 0, None))
    m, t = moving_to_fixed(n)
    moving = sample_linear(other, m, t, (n, n, n)) + 0.02 * np.random.default_rng(0).standard_normal((n, n, n))
    fixed, moving = fixed.astype(F), moving.astype(F)
    fixed.setflags(write=False)
    moving.setflags(write=False)
    return fixed, moving


def quantile_range(image):
    """(lo, hi) float32: the 1 % and 99 % quantiles of the image"""
    lo, hi = np.quantile(np.asarray(image, np.float64), [0.01, 0.99])
    return F(lo), F(hi)


@functools.lru_cache(maxsize=None)
def phantom_codes(n=32, bins=16):
    """-> (fixed codes, moving codes) uint8 {n, n, n}, read only: code_ref over each image's quantile_range"""
    out = []
    for img in phantom(n):
        c = code_ref(img, *quantile_range(img), bins)
        c.setflags(write=False)
        out.append(c)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def phantom_search(n=32, bins=16):
    """search_ref on the phantom's codes from the identity with PHANTOM_STEP and PHANTOM_STAGES, computed once"""
    fixed, moving = phantom_codes(n, bins)
    out = search_ref(fixed, moving, bins, IDENTITY)
    for a in out:
        a.setflags(write=False)
    return out


def corner_error(map12, truth, shape):
    """the largest distance, in voxels, between map12 and the (matrix, translation) truth over the eight corners of a (D, H, W) grid"""
    m12 = np.asarray(map12, np.float64).reshape(12)
    m, t = m12[:9].reshape(3, 3), m12[9:]
    tm, tt = truth
    d, h, w = shape
    worst = 0.0
    for x in (0, w - 1):
        for y in (0, h - 1):
            for z in (0, d - 1):
                p = np.array([x, y, z], np.float64)
                worst = max(worst, float(np.linalg.norm((m @ p + t) - (tm @ p + tt))))
    return worst
