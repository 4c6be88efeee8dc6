"""The shapes and the input generators of the layer-kernel op tests (csrc/kernels_elem.hip), each shape named for the branch it is there
for.  tests/test_layer_ref_host.py asserts the generators' conditions for every case without a GPU; tests/test_gpu_layer_ops.py holds
the claims about the forms against the engine (unet_op_norm_choice) and runs the cases.

Forms of the five steps of a norm layer, in the order unet_op_norm_choice (include/unet_hip.h) numbers them."""
import functools
import types
import zlib

import numpy as np

import layer_ref as R

FWD_FINALIZE = ("fused", "sep64", "sep256")                    # k_norm_finalize_apply8 | k_norm_finalize at 64 | at 256 threads
COPY = ("fused", "view8g", "view8", "materialize")             # in that fused launch | k_apply_view8g | k_apply_view8 | k_materialize
BWD_STATS = ("stats8_shfl", "stats8_lds", "generic")           # k_norm_bwd_stats8 shuffle | LDS reduction | k_stats_partial<T, 1>
BWD_FINALIZE = ("fused", "sep64", "sep256")                    # k_norm_bwd_finalize_apply8 | k_norm_bwd_finalize at 64 | at 256 threads
BWD_APPLY = ("fused", "apply8", "generic")                     # in that fused launch | k_norm_bwd_apply8 | k_norm_bwd_apply
STEPS = (FWD_FINALIZE, COPY, BWD_STATS, BWD_FINALIZE, BWD_APPLY)


def _n(dt, C, S, forms, why):
    forms = tuple(forms)
    assert len(forms) == 5 and all(f in STEPS[i] for i, f in enumerate(forms)), forms
    return (dt, C, S), forms, why


def _fused(bstats):
    return ("fused", "fused", bstats, "fused", "fused")


# (dtype, C, S) -> the form of each step, and the branch the shape is there for.  rows = stats_blocks(S) = ceil(S / max(32, ceil(S / 1024)))
_NORM = [
    _n("bf16", 8, 1, _fused("stats8_shfl"), "one voxel, one row (instance norm only)"),
    _n("bf16", 8, 33, _fused("stats8_shfl"), "two rows, the second one voxel; prologue row groups RG = 64"),
    _n("bf16", 16, 100, _fused("stats8_shfl"), "ragged last row"),
    _n("bf16", 64, 4096, _fused("stats8_shfl"), "exactly 128 rows: the fused forms' last"),
    _n("bf16", 16, 4097, ("sep256", "view8", "stats8_shfl", "sep256", "apply8"), "129 rows: separate finalize at 256 threads"),
    _n("bf16", 256, 130, _fused("stats8_shfl"), "G8 = 32: the shuffle reduction's last"),
    _n("bf16", 512, 96, _fused("stats8_lds"), "G8 = 64: the LDS reduction's first; the fused forms' largest C, RG = 1"),
    _n("bf16", 1024, 70, ("sep64", "view8", "stats8_lds", "sep64", "apply8"), "C > 512 with few rows: separate finalize at 64 threads"),
    _n("bf16", 2048, 40, ("sep64", "view8", "stats8_lds", "sep64", "apply8"), "G8 = 256: one voxel lane per block"),
    _n("bf16", 2048, 130, ("sep64", "view8g", "stats8_lds", "sep64", "apply8"), "8g copy with one voxel lane"),
    _n("bf16", 16, 16389, ("sep256", "view8g", "stats8_shfl", "sep256", "apply8"), "8g copy with a ragged tail"),
    _n("bf16", 64, 4133, ("sep256", "view8g", "stats8_shfl", "sep256", "apply8"), "8g copy with a ragged tail"),
    _n("bf16", 32, 40000, ("sep256", "view8g", "stats8_shfl", "sep256", "apply8"), "40 voxels per row (vpb > 32), not a multiple of the 8 lanes' trips"),
    _n("bf16", 24, 300, ("sep64", "view8", "generic", "sep64", "generic"), "C / 8 = 3 is no power of two"),
    _n("bf16", 40, 4100, ("sep256", "view8", "generic", "sep256", "generic"), "C / 8 = 5 is no power of two, 129 rows"),
    _n("bf16", 1, 513, ("sep64", "materialize", "generic", "sep64", "generic"), "generic everything, one channel"),
    _n("bf16", 5, 77, ("sep64", "materialize", "generic", "sep64", "generic"), "generic everything, pow2_ge(C) = 8 lane tail"),
    _n("bf16", 7, 4100, ("sep256", "materialize", "generic", "sep256", "generic"), "generic everything, 129 rows"),
    _n("bf16", 264, 50, ("sep64", "view8", "generic", "sep64", "generic"), "generic channel loop (C > 256) with a tail of 8"),
    _n("bf16", 520, 40, ("sep64", "view8", "generic", "sep64", "generic"), "generic channel loop, three trips"),
    _n("fp32", 1, 513, ("sep64", "materialize", "generic", "sep64", "generic"), "fp64 rows, one channel"),
    _n("fp32", 5, 77, ("sep64", "materialize", "generic", "sep64", "generic"), "fp64 rows, lane tail"),
    _n("fp32", 16, 4097, ("sep256", "materialize", "generic", "sep256", "generic"), "fp64 rows, 129 of them"),
    _n("fp32", 48, 1000, ("sep64", "materialize", "generic", "sep64", "generic"), "fp64 rows, pow2_ge(C) = 64"),
    _n("fp32", 320, 64, ("sep64", "materialize", "generic", "sep64", "generic"), "fp64 rows, channel loop with a tail"),
    _n("fp32", 16, 40000, ("sep256", "materialize", "generic", "sep256", "generic"), "fp64 rows, 1000 of 40 voxels"),
]
NORM_CASES = [c for c, _, _ in _NORM]
NORM_FORMS = {c: f for c, f, _ in _NORM}
NORM_WHY = {c: w for c, _, w in _NORM}
NORM_KINDS = ("in", "bn")
# eval-mode BatchNorm (k_norm_eval, then the copy alone): one case per copy form and element type
EVAL_CASES = [("bf16", 16, 100), ("bf16", 2048, 130), ("bf16", 24, 300), ("bf16", 5, 77), ("fp32", 5, 77), ("fp32", 48, 1000)]

# (C, (D, H, W)): pool, upsample, views, export / import.  One channel and one window; odd extents in every axis; 8-channel vectors;
# C / 8 = 3; several blocks; an extent of 2 next to an odd one
VOLUME_CASES = [(1, (2, 2, 2)), (5, (5, 6, 7)), (16, (4, 4, 4)), (24, (3, 9, 8)), (64, (2, 3, 33)), (7, (9, 2, 5))]
ALL_EQUAL_CASE, NAN_CASE = (16, (4, 4, 4)), (5, (5, 6, 7))
CONCAT_CASES = [(5, 7), (16, 8), (32, 32)]
CONCAT_S = 77
DTYPES = ("bf16", "fp32")


def stats_vpb(S):
    """voxels per statistics row (kernels_elem.hip stats_vpb)"""
    return max(32, (S + 1023) // 1024)


def stats_rows(S):
    return (S + stats_vpb(S) - 1) // stats_vpb(S)


def bf16_round(x):
    """round to bf16 (nearest even) -> float64"""
    b = np.ascontiguousarray(np.asarray(x, np.float32)).view(np.uint32).astype(np.uint64)
    r = ((b + 0x7FFF + ((b >> 16) & 1)) & 0xFFFF0000).astype(np.uint32)
    return r.view(np.float32).astype(np.float64)


def quant(x, dt):
    """the values of x as the element type stores them, in float64"""
    return bf16_round(x) if dt == "bf16" else np.asarray(x, np.float32).astype(np.float64)


def f32(x):
    return np.asarray(x, np.float32).astype(np.float64)


def rng_of(*key):
    return np.random.default_rng([zlib.crc32(repr(key).encode())])


def frozen(**arrays):
    for a in arrays.values():
        if isinstance(a, np.ndarray):
            a.flags.writeable = False
    return types.SimpleNamespace(**arrays)


KINK_MARGIN = 2.0 ** -7


def kink_clear(u, scale, shift):
    """|u scale + shift| >= 2^-7 (|u scale| + |shift|) at every voxel: no fp32 evaluation of the pre-activation, fused or not, can land
    on the other side of an activation's kink than the float64 one"""
    a, b = u * scale, np.broadcast_to(shift, u.shape)
    return np.abs(a + b) >= KINK_MARGIN * (np.abs(a) + np.abs(b))


def stat_row(f):
    """the fp32 stat row [4][C] a forward leaves, from the float64 reference"""
    return f32(np.stack([f["mean"], f["rstd"], f["scale"], f["shift"]]))


FAR_MEAN = 22.0


def heavy_voxels(S):
    """the voxels whose gradient norm_inputs draws 16 times larger: 32..63 and the last statistics row (none below 64 voxels)"""
    m = np.zeros(S, bool)
    if S >= 64:
        m[32:64] = True
        m[(stats_rows(S) - 1) * stats_vpb(S):] = True
    return m


@functools.lru_cache(maxsize=None)
def norm_inputs(dt, C, S, kind):
    """the inputs of a norm case, shared read-only by every activation: u, the older gradient g = dL/d(view), gamma, beta, rm, rv, the
    float64 forward reference f of the stored u and its fp32 stat row.
    Every fourth channel is drawn with its mean 32 standard deviations out.  Voxels whose pre-activation would lie within the kink margin
    are then moved out to twice the margin, until none is left; for those channels the margin is 2^-6 |mean scale|, half a gamma wide, so
    the move widens their spread: as stored, |mean| rstd is at least FAR_MEAN = 22 there (the host test asserts it for every case).
    g is 16 times larger on the voxels of heavy_voxels(S) -- 32..63 and the last statistics row -- so that a lost row shows in sums of
    40000 terms."""
    rng = rng_of("norm", dt, C, S, kind)
    sigma = 0.5 + rng.random(C)
    mu = np.where(np.arange(C) % 4 == 1, 32.0, rng.standard_normal(C) * 0.5) * sigma
    gamma = f32(1.0 + 0.2 * rng.standard_normal(C))
    beta = f32(np.where(rng.random(C) < 0.5, -1.0, 1.0) * (0.25 + 0.25 * rng.random(C)))
    rm = f32(mu + 0.1 * rng.standard_normal(C))
    rv = f32(sigma ** 2 * (0.8 + 0.4 * rng.random(C)))
    if S == 1:      # xhat = 0 and the pre-activation is beta: only a small u keeps |u scale| = 316 |u gamma| inside the margin
        u = quant(np.clip(rng.standard_normal((S, C)), -3, 3) * 2.0 ** -7, dt)
    else:
        u = rng.standard_normal((S, C)) * sigma + mu
        u[S - 1, 0] = mu[0] + 1.5 * sigma[0] * np.sign(gamma[0])     # the last voxel of channel 0 on an activation's slope-1 side:
        u = quant(u, dt)                                             # with one channel and a last row of one voxel it is all that row holds
    ev = kind == "bn_eval"

    def fwd(u):
        return R.norm_fwd(u, gamma, beta, R.EPS[kind], rm if kind != "in" else None, rv if kind != "in" else None, use_running=ev)
    for _ in range(40):
        st = stat_row(fwd(u))
        bad = ~kink_clear(u, st[2], st[3])
        if not bad.any() or S == 1:
            break
        sc, sh = np.broadcast_to(st[2], u.shape)[bad], np.broadcast_to(st[3], u.shape)[bad]
        z = u[bad] * sc + sh
        want = np.where(z < 0, -1.0, 1.0) * 2 * KINK_MARGIN * (np.abs(u[bad] * sc) + np.abs(sh))
        u[bad] = (want - sh) / sc
        u = quant(u, dt)
    f = fwd(u)
    w = np.where(heavy_voxels(S), 16.0, 1.0)[:, None]
    g = rng.standard_normal((S, C)) * w
    g[S - 1, 0] = w[S - 1, 0]
    g = quant(g, dt)
    return frozen(u=u, g=g, gamma=gamma, beta=beta, rm=rm, rv=rv, f={k: v for k, v in f.items()}, stat=stat_row(f))


def grid(rng, shape, lim=8, step=0.125):
    return rng.integers(-lim, lim + 1, shape).astype(np.float64) * step


@functools.lru_cache(maxsize=None)
def volume_inputs(C, dims):
    """exact data of a pool / upsample / copy case: x, the gradients of the coarse (gc), same-size (gs) and fine (gf) outputs and the older
    gradient, all k / 8 with |k| <= 8 -- bf16 holds every value and every sum of up to nine of them, so fp32 sums are exact in any order.
    Window (0, 0, 0) of channel 0 has its maximum 9/8 twice (elements 3 and 5) and its minimum -9/8 twice (elements 2 and 6: the tie
    under a view with a negative scale), and its gradient is 1; ALL_EQUAL_CASE has window (1, 1, 1) constant in every
    channel; NAN_CASE (xn) has NaN at elements 2 and 6 of window (1, 1, 1) of channel 2."""
    D, H, W = dims
    rng = rng_of("volume", C, dims)
    x = grid(rng, (D, H, W, C))
    x[0, 1, 1, 0] = x[1, 0, 1, 0] = 9 / 8
    x[0, 1, 0, 0] = x[1, 1, 0, 0] = -9 / 8
    gc = grid(rng, (D // 2, H // 2, W // 2, C))
    gc[0, 0, 0, 0] = 1.0
    if (C, dims) == ALL_EQUAL_CASE:
        x[2:4, 2:4, 2:4, :] = 0.25
    xn = None
    if (C, dims) == NAN_CASE:
        xn = x.copy()
        xn[2, 3, 2, 2] = xn[3, 3, 2, 2] = np.nan
    return frozen(x=x, xn=xn, gc=gc, gs=grid(rng, (D, H, W, C)), gf=grid(rng, (2 * D, 2 * H, 2 * W, C)),
                  old=grid(rng, (D, H, W, C)), old_fine=grid(rng, (2 * D, 2 * H, 2 * W, C)))


@functools.lru_cache(maxsize=None)
def exact_view(C, tag=0):
    """relu(x scale + shift) that stays on the grid: scale in {-1, 1, 2}, shift in {-1, 0, 1} / 8 (post-affine zeros occur)"""
    rng = rng_of("exact view", C, tag)
    return frozen(scale=rng.choice([-1.0, 1.0, 2.0], C), shift=rng.integers(-1, 2, C) / 8.0, act=1)


@functools.lru_cache(maxsize=None)
def norm_view(C, act, tag=0):
    """a norm + activation view of grid data: fp32 scale and shift as a stat row holds them, redrawn per channel until every grid level
    clears the kink margin"""
    rng = rng_of("norm view", C, act, tag)
    scale = f32((1.0 + 0.3 * rng.standard_normal(C)) * np.where(rng.random(C) < 0.3, -1.0, 1.0))
    shift = f32(0.3 * rng.standard_normal(C))
    levels = np.arange(-9, 10)[:, None] / 8.0
    for _ in range(100):
        bad = ~kink_clear(np.broadcast_to(levels, (19, C)), scale, shift).all(0)
        if not bad.any():
            break
        shift = np.where(bad, f32(0.3 * rng.standard_normal(C)), shift)
    assert kink_clear(np.broadcast_to(levels, (19, C)), scale, shift).all(), "no shift clear of the kink margin was drawn"
    return frozen(scale=scale, shift=shift, act=act)


@functools.lru_cache(maxsize=None)
def concat_inputs(c0, c1):
    """grid data of a concat case: the two sources, the gradient of the concatenation and the older gradients of the sources, and the
    two pairs of views the sources are read through: (plain, exact relu view) and two different norm + activation views"""
    S, rng = CONCAT_S, rng_of("concat", c0, c1)
    return frozen(x0=grid(rng, (S, c0)), x1=grid(rng, (S, c1)), gout=grid(rng, (S, c0 + c1)), o0=grid(rng, (S, c0)), o1=grid(rng, (S, c1)),
                  views=(("exact", None, exact_view(c1, 1)), ("norm", norm_view(c0, 2, 1), norm_view(c1, 3, 2))))


def tied_windows(x):
    """how many (window, channel) pairs hold their maximum more than once"""
    w = R._windows(np.asarray(x, np.float64))
    with np.errstate(invalid="ignore"):
        return int(((w == np.nanmax(w, 3, keepdims=True)).sum(3) > 1).sum())


# ---- voxels on the kink, built on purpose (fp32 stat rows; bf16 holds every u of the first kind) ----
def kink_inputs(dt, C=8, dims=(2, 2, 4)):
    """even channels: the pre-activation is exactly 0 at a quarter of the voxels (u = 1, scale = 2, shift = -2; others -1, 1, 2).
    odd channels, fp32: u = scale = 1 + 2^-12, shift = -(1 + 2^-11): the exact pre-activation is 2^-24 > 0 and one fused multiply-add
    gives it, but the product rounded first (a tie, to even) gives 0; the other voxels are about -0.5, 1 and 2.  Odd
    channels, bf16: scale = -1, shift = 1 with the same u as the even ones."""
    D, H, W = dims
    rng = rng_of("kink", dt, C, dims)
    scale, shift = np.empty(C), np.empty(C)
    u = np.empty((D, H, W, C))
    for c in range(C):
        if c % 2 == 0 or dt == "bf16":
            scale[c], shift[c] = (2.0, -2.0) if c % 2 == 0 else (-1.0, 1.0)
            lv = np.array([1.0, 0.5, 1.5, 2.0])
        else:
            scale[c], shift[c] = 1 + 2.0 ** -12, -(1 + 2.0 ** -11)
            lv = np.array([1 + 2.0 ** -12, 0.5, 2 + 2.0 ** -11, 3.0])
        u[..., c] = lv[(rng.permutation(D * H * W) % 4).reshape(D, H, W)]
    assert np.array_equal(quant(u, dt), u) and np.array_equal(f32(scale), scale) and np.array_equal(f32(shift), shift)
    z = u * scale + shift
    special = (z == 0) | (z == 2.0 ** -24)
    return frozen(u=u, scale=scale, shift=shift, z=z, special=special)


def kink_pool_inputs(dt, C=8, dims=(2, 2, 4)):
    """kink_inputs for the pool: every window of every channel holds ONE voxel on the kink (never its element 0) and seven whose
    pre-activation is negative (-0.5 .. -2), so the window's maximum is the voxel on the kink: 2^-24 in the odd fp32 channels, where
    the product rounded before the add gives 0 -- the forward value then differs, and under relu the backward sends the gradient to
    element 0 of an all-zero window instead.  (At a pre-activation of exactly 0 every activation gives 0 on either side: there only
    the derivative tells the sides apart.)  wrong: the pre-activations with 2^-24 replaced by that 0."""
    D, H, W = dims
    scale, shift = np.empty(C), np.empty(C)
    uw = np.empty((D // 2, H // 2, W // 2, 8, C))
    for c in range(C):
        if c % 2 == 0:
            scale[c], shift[c], kink, lv = 2.0, -2.0, 1.0, np.array([0.5, 0.25, 0.0])
        elif dt == "bf16":
            scale[c], shift[c], kink, lv = -1.0, 1.0, 1.0, np.array([1.5, 2.0, 3.0])
        else:
            scale[c], shift[c], kink, lv = 1 + 2.0 ** -12, -(1 + 2.0 ** -11), 1 + 2.0 ** -12, np.array([0.5, 0.25, 0.75])
        for w in range(uw.shape[2]):
            uw[0, 0, w, :, c] = lv[(np.arange(8) + c + w) % 3]
            uw[0, 0, w, 1 + (c + w) % 7, c] = kink
    u = uw.reshape(D // 2, H // 2, W // 2, 2, 2, 2, C).transpose(0, 3, 1, 4, 2, 5, 6).reshape(D, H, W, C)
    assert D == H == 2 and np.array_equal(R._windows(u), uw)
    assert np.array_equal(quant(u, dt), u) and np.array_equal(f32(scale), scale) and np.array_equal(f32(shift), shift)
    z = u * scale + shift
    special = (z == 0) | (z == 2.0 ** -24)
    return frozen(u=u, scale=scale, shift=shift, z=z, special=special, wrong=np.where(z == 2.0 ** -24, 0.0, z))
