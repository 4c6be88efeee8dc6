"""The patch feed's definitions (include/unet_patches.h) restated in numpy and Python integers, for test_patches_host.py and
test_gpu_patches.py.  Nothing here calls the library."""
import numpy as np

M64 = (1 << 64) - 1
G = 0x9E3779B97F4A7C15
SEG = 1024


def mix(z):
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9 & M64
    z = (z ^ (z >> 27)) * 0x94D049BB133111EB & M64
    return z ^ (z >> 31)


def draw(seed, index, k):
    return mix((mix(mix((seed + G) & M64) ^ (index & M64)) + (k + 1) * G) & M64) >> 32


def decide(seed, index, fg_classes, num=1, den=3):
    """(cls, u_rank, u_x, u_y, u_z): forced foreground when (u0 * den) >> 32 < num, the class (u1 * m) >> 32 of the m listed"""
    u = [draw(seed, index, k) for k in range(6)]
    m = len(fg_classes)
    forced = (u[0] * den) >> 32 < num
    cls = fg_classes[(u[1] * m) >> 32] if forced and m else -1
    return (cls,) + tuple(u[2:6])


def class_map(label, classes):
    """int64 class per voxel, -1 for none"""
    l = np.asarray(label, dtype=np.float32).reshape(-1)
    if classes == 0:
        return (l > 0).astype(np.int64)
    with np.errstate(invalid="ignore"):
        t = np.trunc(l.astype(np.float64))
        ok = (t >= 0) & (t < classes)          # NaN fails both
    return np.where(ok, t, -1.0).astype(np.int64)


def index_ref(label, classes):
    """(totals int64[K], prefix int64[K, S]) from np.bincount per segment"""
    cm = class_map(label, classes)
    K = classes or 2
    S = (cm.size + SEG - 1) // SEG
    key = (np.arange(cm.size) // SEG) * K + cm                  # (segment, class) in one bincount
    counts = np.bincount(key[cm >= 0], minlength=S * K).reshape(S, K).T
    return counts.sum(axis=1), np.cumsum(counts, axis=1) - counts


def origin_class(centre, u, T, C):
    return min(max(centre - ((u * T) >> 32), 0), C - T)


def origin_uniform(u, T, C):
    return (u * (C - T + 1)) >> 32


def u_for(r, n):
    """the smallest draw u with (u * n) >> 32 == r"""
    return -((-r << 32) // n)


def pick_ref(cm, dims, window, pk):
    """(x, y, z, flag) of one pick; cm: class_map of the canvas, dims (W, H, D), window (tw, th, td)"""
    cls, u_rank, ux, uy, uz = pk
    hits = np.flatnonzero(cm == cls) if cls >= 0 else np.zeros(0, np.int64)
    if hits.size == 0:
        return tuple(origin_uniform(u, t, c) for u, t, c in zip((ux, uy, uz), window, dims)) + (0,)
    centre = int(hits[(u_rank * hits.size) >> 32])
    W, H, _ = dims
    c3 = (centre % W, centre // W % H, centre // (W * H))
    return tuple(origin_class(c, u, t, cc) for c, u, t, cc in zip(c3, (ux, uy, uz), window, dims)) + (1,)
