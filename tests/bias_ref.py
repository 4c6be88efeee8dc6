"""The numpy restatements of include/unet_bias.h, shared by tests/test_bias_host.py (which checks them on hand-written answers) and
tests/test_gpu_bias.py (which pins the device to them bit for bit): `logcode_ref`, `levels_ref`, `residual_ref`, `sweep_ref`,
`refine_ref`, `cost_ref`, `fit_ref`, `apply_ref`, `correct_ref`, and the exact `energy` in Python integers.  numpy only: nothing here
calls the package's kernels.  All sums are int64 (the header says why they fit; `worst_case_bounds` restates it in Python integers);
a colour pass is vectorised over the whole volume: a voxel belongs to at most one support of the colour, so a node's sums are one
np.add.at (exact in int64, unlike np.bincount's float64 weights)."""
import functools

import numpy as np

F = np.float32
NONE, SKIP, MAX = -2 ** 31, -2 ** 15, 8192                          # written out: the restatements do not read the module's values
MAX_CLASSES, MAX_LAM, MAX_ROWS = 16, 4096, 32
LG = {4: 2, 8: 3, 16: 4, 32: 5}
DEFAULT_LEVELS = [(32, 4, 1), (16, 4, 1), (8, 4, 1)]
DEFAULT_OUTER, DEFAULT_CLIP = 2, 2048
TABLE = np.exp2(np.arange(4096, dtype=np.float64) / 4096.0).astype(F)   # T[j]: float64 exp2 rounded once to float32


def lattice_ref(shape, g):
    """(nz, ny, nx) of the lattice of spacing g over a (D, H, W) grid"""
    return tuple((int(d) + g - 1) // g + 1 for d in shape)


def zero_field(shape, g):
    return np.zeros(lattice_ref(shape, g), np.int32)


def coords(shape):
    """x, y, z of every voxel of a (D, H, W) grid, x fastest"""
    d, h, w = shape
    i = np.arange(d * h * w, dtype=np.int64)
    return i % w, (i // w) % h, i // (w * h)


def logcode_ref(v):
    """int32 like v: 4096 * log2 v truncated, by the exponent and 16 squarings of the mantissa; NONE for what has no logarithm"""
    v = np.ascontiguousarray(v, F)
    b = v.view(np.uint32).astype(np.int64)
    ex, man = (b >> 23) & 0xFF, b & 0x7FFFFF
    ok = ((b >> 31) == 0) & (ex != 0) & (ex != 255)
    x = ((man | (1 << 23)) << 8).astype(np.uint64)
    f = np.zeros(v.shape, np.int64)
    for _ in range(16):
        y = (x * x) >> np.uint64(31)                                # x < 2^32: the square fits uint64
        bit = (y >> np.uint64(32)) != 0
        f = 2 * f + bit
        x = np.where(bit, y >> np.uint64(1), y)
    q = ((ex - 127) * 65536 + f) >> 4
    return np.where(ok, q, NONE).astype(np.int32)


def corner_sum(B, g, x, y, z):
    """n int64 {N}: the 8 corners of each voxel's cell, weighted by the products of {g - f, f}"""
    B = np.asarray(B).astype(np.int64)
    lg = LG[g]
    cx, cy, cz, fx, fy, fz = x >> lg, y >> lg, z >> lg, x & (g - 1), y & (g - 1), z & (g - 1)
    n = np.zeros(x.size, np.int64)
    for c in range(8):
        dx, dy, dz = c & 1, (c >> 1) & 1, c >> 2
        n += (fx if dx else g - fx) * (fy if dy else g - fy) * (fz if dz else g - fz) * B[cz + dz, cy + dy, cx + dx]
    return n


def class_of(labels, classes):
    """int64 like labels: the index of each label in classes, -1 for none"""
    labels = np.asarray(labels).astype(np.int64)
    t = np.full(labels.shape, -1, np.int64)
    for k, c in enumerate(classes):
        t[labels == int(c)] = k
    return t


def levels_ref(q, labels, classes, B, g):
    """int64 {16, 3}: row t = (m_t, count, sum) over the voxels of class t with a valid q, of q - (n >> 3 lg); (NONE, 0, 0) without"""
    q = np.asarray(q).astype(np.int64)
    d = q.reshape(-1) - (corner_sum(B, g, *coords(q.shape)) >> (3 * LG[g]))
    t = class_of(labels, classes).reshape(-1)
    lev = np.zeros((MAX_CLASSES, 3), np.int64)
    lev[:, 0] = NONE
    for k in range(len(classes)):
        sel = (t == k) & (q.reshape(-1) != NONE)
        if sel.any():
            s, n = int(d[sel].sum()), int(sel.sum())
            lev[k] = (s // n, n, s)                                 # Python's // floors
    return lev


def residual_ref(q, labels, classes, lev, clip):
    """int16 like q"""
    q = np.asarray(q).astype(np.int64)
    t = class_of(labels, classes)
    m = np.where(t >= 0, np.asarray(lev)[:, 0][np.maximum(t, 0)], NONE)
    d = q - m
    ok = (t >= 0) & (m != NONE) & (q != NONE) & (np.abs(d) <= clip)
    return np.where(ok, d, SKIP).astype(np.int16)


def owner(x, g, parity):
    """the node of `parity` along one axis whose open support (i-1)g < x < (i+1)g holds x, -1 for none"""
    cell, f = x >> LG[g], x & (g - 1)
    return np.where((cell & 1) == parity, cell, np.where(f == 0, -1, cell + 1))


def links(B):
    """(the sum over each node's existing lattice neighbours of B_nbr - B_node, their number), int64 like B"""
    B = np.asarray(B).astype(np.int64)
    dsum, nbrs = np.zeros(B.shape, np.int64), np.zeros(B.shape, np.int64)
    for axis in range(3):
        for s in (-1, 1):
            idx = np.arange(B.shape[axis]) + s
            ok = (idx >= 0) & (idx < B.shape[axis])
            shape = [1, 1, 1]
            shape[axis] = -1
            okb = ok.reshape(shape)
            nb = np.take(B, np.clip(idx, 0, B.shape[axis] - 1), axis=axis)
            dsum += np.where(okb, nb - B, 0)
            nbrs += np.where(okb, 1, 0) + np.zeros(B.shape, np.int64)
    return dsum, nbrs


def sweep_ref(r, B, g, lam, after_node_pass=None, colours=range(8)):
    """-> (the field after one sweep, int32 like B; info int64 {2} = nodes changed, nodes visited).  after_node_pass: called with
    (colour, field before the pass, field after it); colours: the passes to run (a sweep is all 8, in order)"""
    r = np.asarray(r)
    B = np.array(B, np.int64)
    nz, ny, nx = B.shape
    assert (nz, ny, nx) == lattice_ref(r.shape, g) and 0 <= lam <= MAX_LAM
    x, y, z = coords(r.shape)
    rr = r.reshape(-1).astype(np.int64)
    Lam = lam * g ** 6
    kk, jj, ii = np.indices(B.shape)
    changed = visited = 0
    for c in colours:
        i, j, k = owner(x, g, c & 1), owner(y, g, (c >> 1) & 1), owner(z, g, c >> 2)
        act = (i >= 0) & (j >= 0) & (k >= 0) & (rr != SKIP)
        xa, ya, za, ia, ja, ka = x[act], y[act], z[act], i[act], j[act], k[act]
        W = (g - np.abs(xa - ia * g)) * (g - np.abs(ya - ja * g)) * (g - np.abs(za - ka * g))
        e = rr[act] * g ** 3 - corner_sum(B, g, xa, ya, za)
        S1, S2 = np.zeros(B.size, np.int64), np.zeros(B.size, np.int64)
        node = (ka * ny + ja) * nx + ia
        np.add.at(S1, node, W * e)
        np.add.at(S2, node, W * W)
        dsum, nbrs = links(B)
        num, den = S1.reshape(B.shape) + Lam * dsum, S2.reshape(B.shape) + Lam * nbrs
        delta = np.where(den > 0, (2 * num + den) // np.maximum(2 * den, 1), 0)   # numpy's // floors
        mine = ((ii & 1) == (c & 1)) & ((jj & 1) == ((c >> 1) & 1)) & ((kk & 1) == (c >> 2))
        new = np.where(mine, np.clip(B + delta, -MAX, MAX), B)
        changed += int((new != B).sum())
        visited += int((mine & (den > 0)).sum())
        if after_node_pass is not None:
            after_node_pass(c, B.astype(np.int32), new.astype(np.int32))
        B = new
    return B.astype(np.int32), np.array([changed, visited], np.int64)


def energy(r, B, g, lam):
    """the exact energy as a Python integer: the sum of (r g^3 - n)^2 over the voxels that count + lam g^6 * the sum over the
    lattice's links of (B_i - B_j)^2"""
    r = np.asarray(r)
    rr = r.reshape(-1).astype(np.int64)
    e = (rr * g ** 3 - corner_sum(B, g, *coords(r.shape)))[rr != SKIP]
    total = sum(int(v) * int(v) for v in e)
    Bo = np.asarray(B).astype(np.int64)
    link = 0
    for axis in range(3):
        d = np.diff(Bo, axis=axis).reshape(-1)
        link += sum(int(v) * int(v) for v in d)
    return total + lam * g ** 6 * link


def worst_case_bounds(g, lam=MAX_LAM):
    """dict of the largest magnitudes a node's sums can take at spacing g, in Python integers: every voxel of a full support at
    r = +-8192 against a field at -+8192 everywhere, every neighbour 2 * 8192 away"""
    w1 = [g - abs(d) for d in range(-(g - 1), g)]                   # the node's weights along one axis of a full support
    sum_w, sum_w2 = sum(w1) ** 3, sum(v * v for v in w1) ** 3
    e = MAX * g ** 3 + g ** 3 * MAX                                 # |r g^3| + |n|
    S1, S2, Lam = sum_w * e, sum_w2, lam * g ** 6
    num, den = S1 + Lam * 6 * 2 * MAX, S2 + Lam * 6
    return dict(sum_w=sum_w, e=e, S1=S1, S2=S2, Lam=Lam, num=num, den=den, top=2 * num + den)


def refine_ref(B, shape, g):
    """the field on the lattice of g // 2: (the sum of the 8 coarse combinations + 4) >> 3"""
    B = np.asarray(B).astype(np.int64)
    cz, cy, cx = B.shape
    assert B.shape == lattice_ref(shape, g)
    fz, fy, fx = lattice_ref(shape, g // 2)
    k, j, i = np.indices((fz, fy, fx))
    ia = [i >> 1, np.minimum((i >> 1) + (i & 1), cx - 1)]
    ja = [j >> 1, np.minimum((j >> 1) + (j & 1), cy - 1)]
    ka = [k >> 1, np.minimum((k >> 1) + (k & 1), cz - 1)]
    s = sum(B[ka[c >> 2], ja[(c >> 1) & 1], ia[c & 1]] for c in range(8))
    return ((s + 4) >> 3).astype(np.int32)


def cost_ref(r, B, g):
    """int64 {2}: the sum of (r - (n >> 3 lg))^2 over the voxels that count, their number"""
    r = np.asarray(r)
    rr = r.reshape(-1).astype(np.int64)
    d = (rr - (corner_sum(B, g, *coords(r.shape)) >> (3 * LG[g])))[rr != SKIP]
    return np.array([int((d * d).sum()), d.size], np.int64)


def fit_ref(q, labels, classes, clip=DEFAULT_CLIP, levels=DEFAULT_LEVELS, outer=DEFAULT_OUTER, early=True, watch=None):
    """-> (B int32 on the last level's lattice, report int64 {32, 6}).  early=False runs every sweep of the schedule (the field must
    not differ).  watch(r, B_before, B_after, g, lam) is called around every sweep"""
    shape = np.asarray(q).shape
    report = np.full((MAX_ROWS, 6), -1, np.int64)
    B = zero_field(shape, levels[0][0])
    row = 0
    for l, (g, sweeps, lam) in enumerate(levels):
        assert l == 0 or 2 * g == levels[l - 1][0]
        for o in range(outer):
            r = residual_ref(q, labels, classes, levels_ref(q, labels, classes, B, g), clip)
            changed = []
            for s in range(sweeps):
                before = B
                B, info = sweep_ref(r, B, g, lam)
                if watch is not None:
                    watch(r, before, B, g, lam)
                changed.append(int(info[0]))
                if early and info[0] == 0:
                    break
            ran = 1                                                 # the device's report: sweep s ran when s - 1 changed a node
            while ran < sweeps and changed[ran - 1]:
                ran += 1
            report[row] = (g, o, ran, changed[ran - 1], *cost_ref(r, B, g))
            row += 1
        if l + 1 < len(levels):
            B = refine_ref(B, shape, g)
    return B, report


def apply_ref(v, B, g):
    """-> (out, gain) float32 like v: ldexp(v * T[j], k), the bits of v where c = 0, a NaN result as 0x7FC00000"""
    v = np.ascontiguousarray(v, F)
    lg3 = 3 * LG[g]
    c = ((-corner_sum(B, g, *coords(v.shape)) + (1 << (lg3 - 1))) >> lg3).reshape(v.shape)
    k, t = (c >> 12).astype(np.int32), TABLE[c & 4095]
    with np.errstate(all="ignore"):
        p = v * t
        assert p.dtype == F
        o = np.ldexp(p, k).astype(F)
        o = np.where(np.isnan(o), np.array([0x7FC00000], np.uint32).view(F)[0], o)
        out = np.where(c == 0, v.view(np.uint32), o.view(np.uint32)).astype(np.uint32).view(F)
        gain = np.ldexp(t, k).astype(F)
    return out, gain


def correct_ref(volume, labels, classes, clip=DEFAULT_CLIP, levels=DEFAULT_LEVELS, outer=DEFAULT_OUTER):
    """-> (corrected, B, g, report)"""
    B, report = fit_ref(logcode_ref(volume), labels, classes, clip, levels, outer)
    return apply_ref(volume, B, levels[-1][0])[0], B, levels[-1][0], report


def cv_ref(volume, labels, cls):
    v = np.asarray(volume, np.float64)[np.asarray(labels) == cls]
    return float(v.std() / v.mean())


@functools.lru_cache(maxsize=None)
def phantom(shape=(36, 40, 48), seed=0):
    """-> (volume float32, labels uint8, the true gain float64): two nested ellipsoids, class 1 (level 100) around class 2 (level 60), on a
    background at 10 (class 0), times the gain 2^(a x' + b (y'^2 - 1/2) + c z') with x', y', z' in [-1, 1] (0.77 .. 1.30), times
    3 % Gaussian noise.  Read only: shared between tests"""
    d, h, w = shape
    z, y, x = np.indices(shape).astype(np.float64)
    xs, ys, zs = 2 * x / (w - 1) - 1, 2 * y / (h - 1) - 1, 2 * z / (d - 1) - 1
    rad = np.sqrt((xs / 0.9) ** 2 + (ys / 0.85) ** 2 + (zs / 0.8) ** 2)
    labels = np.where(rad < 0.55, 2, np.where(rad < 1.0, 1, 0)).astype(np.uint8)
    gain = np.exp2(0.2 * xs + 0.15 * (ys * ys - 0.5) - 0.1 * zs)
    rng = np.random.default_rng(seed)
    level = np.choose(labels, [10.0, 100.0, 60.0])
    volume = (level * gain * (1 + 0.03 * rng.standard_normal(shape))).astype(F)
    for a in (volume, labels, gain):
        a.setflags(write=False)
    return volume, labels, gain


@functools.lru_cache(maxsize=None)
def phantom_fit(classes=(1, 2)):
    """correct_ref of the phantom under the default plan; read only"""
    volume, labels, _ = phantom()
    out = correct_ref(volume, labels, list(classes))
    for a in (out[0], out[1], out[3]):
        a.setflags(write=False)
    return out
