"""Exact-arithmetic data, poisoned and guarded device buffers, and a bitwise comparison for the conv / conv_trans op tests.

Exact data.  Activations and output gradients are uniform in {-1, 0, 1}, filters are in {-1, 0, 1} and nonzero with probability
pw = min(1, 2400 / K) (K: the longer contraction of the forward and the dgrad), biases are integers in [-3, 3] and the weight / bias
gradients start from integers in [-4, 4].  Every product is then an integer, every partial sum of a contraction stays far below
2^24 and is exact in fp32 IN ANY ORDER -- split-K atomics, slab reduces and sliding-window accumulation included -- and bf16
holds every operand exactly.  With max|y| and max|dx| <= 256 the bf16 results are exactly representable too (the engine stores with
round-to-nearest-even, which leaves a representable value alone), so a kernel is right if and only if its output equals the C oracle's
bit for bit: a dropped, doubled or misplaced (tap, channel) product changes at least one output integer.  The preconditions are
asserted on the reference alone (check_preconditions), before any device result is looked at; a case that misses the bf16 bound gets a
smaller pw through PW_FACTOR -- the bounds themselves never move.

Poisoned, guarded buffers.  Every device output is a view into a larger allocation with GUARD_BYTES of a fixed byte pattern on each
side (a multiple of 256 bytes, so the view keeps the allocator's alignment).  The interior starts as NaN (weight / bias gradients:
their integer start values), scratch as 0xFF bytes (NaN in bf16 and in fp32).  After a call the guards must be untouched and the
interior finite: a voxel the kernel never wrote, stale scratch read as data and a write past either end all show."""
import ctypes as C
import functools
import types
import zlib

import numpy as np
import torch

from oracle import oracle as O

DEV = "cuda:0"
TDT = {"fp32": torch.float32, "bf16": torch.bfloat16}
GUARD_BYTES = 4096
GUARD_BYTE = 0xA5
BF16_EXACT = 256          # integers of magnitude <= 2^8 are bf16 values
F32_EXACT = 1 << 24       # ... below 2^24, fp32 values

# case -> factor on pw, for the cases whose reference misses the bf16 bound with the plain recipe (halve until it holds; none needed so far)
PW_FACTOR = {}


def is_convt(case):
    return len(case) == 3


def out_dims(case):
    dims = case[2]
    if is_convt(case):
        return tuple(2 * s for s in dims)
    ks, st = case[3], case[4]
    pad = (ks - 1) // 2
    return tuple((s + 2 * pad - ks) // st + 1 for s in dims)


def filter_density(case):
    cin, cout = case[:2]
    K = max(cin, 8 * cout) if is_convt(case) else case[3] ** 3 * max(cin, cout)
    return min(1.0, 2400.0 / K) * PW_FACTOR.get(case, 1.0)


def _rng(case, seed):
    return np.random.default_rng([zlib.crc32(repr(tuple(case)).encode()), seed])


def _ternary(rng, shape):
    return rng.integers(-1, 2, shape).astype(np.float32)


def _filter(rng, shape, pw):
    return ((rng.integers(0, 2, shape) * 2 - 1) * (rng.random(shape) < pw)).astype(np.float32)


def _frozen(**arrays):
    for a in arrays.values():
        if isinstance(a, np.ndarray):
            a.flags.writeable = False
    return types.SimpleNamespace(**arrays)


def exact_data(case, seed=0):
    """x [Cin,D,H,W], w (torch layout), b, dy [Cout,Do,Ho,Wo] and the start values dw0 / db0 of the gradients, all integers in fp32"""
    cin, cout, dims = case[:3]
    wshape = (cin, cout, 2, 2, 2) if is_convt(case) else (cout, cin) + (case[3],) * 3
    rng = _rng(case, seed)
    return dict(x=_ternary(rng, (cin, *dims)), w=_filter(rng, wshape, filter_density(case)),
                b=rng.integers(-3, 4, (cout,)).astype(np.float32), dy=_ternary(rng, (cout, *out_dims(case))),
                dw0=rng.integers(-4, 5, wshape).astype(np.float32), db0=rng.integers(-4, 5, (cout,)).astype(np.float32))


def oracle_forward(case, x, w, b):
    cin, cout, (D, H, W) = case[:3]
    y = np.empty((cout, *out_dims(case)), np.float32)
    if is_convt(case):
        O.lib().orc_convt_fwd(O._f(x), O._f(w), O._f(b), O._f(y), cin, cout, D, H, W)
    else:
        O.lib().orc_conv3d_fwd(O._f(x), O._f(w), O._f(b), O._f(y), cin, cout, D, H, W, case[3], case[4])
    return y


def oracle_dgrad(case, dy, w):
    cin, cout, (D, H, W) = case[:3]
    dx = np.empty((cin, D, H, W), np.float32)
    if is_convt(case):
        O.lib().orc_convt_bwd_data(O._f(dy), O._f(w), O._f(dx), cin, cout, D, H, W)
    else:
        O.lib().orc_conv3d_bwd_data(O._f(dy), O._f(w), O._f(dx), cin, cout, D, H, W, case[3], case[4])
    return dx


def oracle_wgrad(case, x, dy, dw0, db0):
    """dw0 + dL/dw, db0 + dL/db (the oracle sums in double and adds the rounded sum, as the += of .grad does)"""
    cin, cout, (D, H, W) = case[:3]
    dw, db = dw0.copy(), db0.copy()
    if is_convt(case):
        O.lib().orc_convt_bwd_weight(O._f(x), O._f(dy), O._f(dw), O._f(db), cin, cout, D, H, W)
    else:
        O.lib().orc_conv3d_bwd_weight(O._f(x), O._f(dy), O._f(dw), O._f(db), cin, cout, D, H, W, case[3], case[4])
    return dw, db


@functools.lru_cache(maxsize=None)
def reference(case, seed=0, directions=("fwd", "dgrad", "wgrad")):
    """the exact data of a case and the oracle's results on it, computed once and shared read-only: y, dx, dw, db (None where the
    direction was not asked for)"""
    d = exact_data(case, seed)
    y = oracle_forward(case, d["x"], d["w"], d["b"]) if "fwd" in directions else None
    dx = oracle_dgrad(case, d["dy"], d["w"]) if "dgrad" in directions else None
    dw, db = oracle_wgrad(case, d["x"], d["dy"], d["dw0"], d["db0"]) if "wgrad" in directions else (None, None)
    return _frozen(y=y, dx=dx, dw=dw, db=db, **d)


@functools.lru_cache(maxsize=None)
def fused_reference(case, seed=0):
    """exact data for the read-side fusion: the consumer sees relu(x * scale + shift) with scale in {-1, 1} and shift in {-1, 0, 1}, a
    small non-negative integer (xa); y = conv(xa) + b by the oracle.  case: (cin, cout, dims, ks, stride)"""
    cin, cout = case[:2]
    d = exact_data(case, seed)
    rng = _rng(case, seed + 1000)
    scale = (rng.integers(0, 2, (cin,)) * 2 - 1).astype(np.float32)
    shift = rng.integers(-1, 2, (cin,)).astype(np.float32)
    xa = np.maximum(d["x"] * scale[:, None, None, None] + shift[:, None, None, None], 0.0).astype(np.float32)
    return _frozen(x=d["x"], w=d["w"], b=d["b"], scale=scale, shift=shift, xa=xa, y=oracle_forward(case, xa, d["w"], d["b"]))


def merged(case2):
    """(c0, c1, cout, dims, ks, stride) -> the case of c0 + c1 input channels the oracle computes: the concatenation of two ternary
    tensors is a ternary tensor, so its results are the two-source layer's and the test only splits them"""
    c0, c1, cout, dims, ks, st = case2
    return (c0 + c1, cout, dims, ks, st)


@functools.lru_cache(maxsize=None)
def old_gradient(case, seed=0):
    """what an accumulating dgrad adds to: integers in [-2, 2], [Cin, D, H, W]"""
    a = _rng(case, seed + 2000).integers(-2, 3, (case[0], *case[2])).astype(np.float32)
    a.flags.writeable = False
    return a


def check_accumulate_precondition(ref, old, dt, what=""):
    """on the reference alone: dx + old is integral and, for the bf16 engine, within the bf16 bound"""
    a = np.asarray(ref.dx, np.float64) + np.asarray(old, np.float64)
    bound = BF16_EXACT if dt == "bf16" else F32_EXACT - 1
    assert np.all(a == np.rint(a)), "%s dx + old: not integral" % what
    assert np.abs(a).max() <= bound, "%s dx + old: max %g exceeds %g (halve pw for this case in PW_FACTOR)" % (what, np.abs(a).max(), bound)


@functools.lru_cache(maxsize=None)
def head_reference(cin, cout, S, seed=0, plain=False):
    """exact data for a head: the 1x1x1 conv reads xa = relu(x * scale + shift) (scale in {-1, 1}, shift in {-1, 0, 1}: xa in {0, 1, 2});
    y, dx = dL/d(view), dw0 + dL/dw and db0 + dL/db by the oracle's 1x1x1 conv on xa; old: what an accumulating dx starts from.
    plain: the source is read as it is (scale and shift None, xa = x).  Arrays are [C, S, 1, 1]"""
    case = (cin, cout, (S, 1, 1), 1, 1)
    d = exact_data(case, seed)
    rng = _rng(case, seed + 1000)
    scale = (rng.integers(0, 2, (cin,)) * 2 - 1).astype(np.float32)
    shift = rng.integers(-1, 2, (cin,)).astype(np.float32)
    xa = np.maximum(d["x"] * scale[:, None, None, None] + shift[:, None, None, None], 0.0).astype(np.float32)
    if plain:
        scale, shift, xa = None, None, d["x"]
    dw, db = oracle_wgrad(case, xa, d["dy"], d["dw0"], d["db0"])
    return _frozen(scale=scale, shift=shift, xa=xa, y=oracle_forward(case, xa, d["w"], d["b"]), dx=oracle_dgrad(case, d["dy"], d["w"]),
                   dw=dw, db=db, old=old_gradient(case, seed), **d)


def check_preconditions(ref, dt, what=""):
    """on the reference alone: every value an integer; bf16 engine: max|y|, max|dx| <= 256; fp32 engine: below 2^24; dw / db (fp32
    in both engines): below 2^24"""
    act_bound = BF16_EXACT if dt == "bf16" else F32_EXACT - 1
    for name, bound in (("y", act_bound), ("dx", act_bound), ("dw", F32_EXACT - 1), ("db", F32_EXACT - 1)):
        a = getattr(ref, name, None)
        if a is None:
            continue
        a = np.asarray(a, np.float64)
        assert np.all(a == np.rint(a)), "%s %s: the reference is not integral" % (what, name)
        assert np.abs(a).max() <= bound, "%s %s: max |reference| %g exceeds %g (halve pw for this case in PW_FACTOR)" % (
            what, name, np.abs(a).max(), bound)


def exact_stat_channels(y_ref):
    """channels whose statistics row {sum y, sum y^2} is exact in fp32 whatever the order of summation: sum|y| < 2^24 and
    sum y^2 < 2^24, judged on the reference alone -> (sum exact, sum of squares exact, the float64 sums [C][2])"""
    yy = np.asarray(y_ref, np.float64).reshape(y_ref.shape[0], -1)
    sums = np.stack([yy.sum(1), (yy * yy).sum(1)], 1)
    return np.abs(yy).sum(1) < F32_EXACT, sums[:, 1] < F32_EXACT, sums


def assert_exact_stats(stats, y_ref, what, need_all_exact):
    """the rows of the exact channels equal the float64 sums; -> masks of the channels left to the caller's tolerance"""
    ok0, ok1, sums = exact_stat_channels(y_ref)
    if need_all_exact:
        assert ok0.all() and ok1.all(), "%s: a case of <= 4096 output voxels must have exact statistics on every channel" % what
    got = np.asarray(stats, np.float64)
    for k, ok in ((0, ok0), (1, ok1)):
        bad = np.flatnonzero(ok & (got[:, k] != sums[:, k]))
        assert bad.size == 0, "%s: statistics column %d differs on channels %s: got %s, want %s" % (
            what, k, bad[:8].tolist(), got[bad[:8], k].tolist(), sums[bad[:8], k].tolist())
    return ~ok0, ~ok1, sums


def _bits(t):
    # + 0.0 folds -0.0 into +0.0 (a sum that cancels is +0 either way, a product of -1 and 0 is not); NaNs stay NaNs
    t = (t + 0.0).contiguous()
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32).numpy()


def assert_exact(got, ref, what="output"):
    """got (a tensor or an array in the logical layout of ref, e.g. [C,D,H,W]) equals ref cast to got's type, bit for bit.  A failure
    names the count, the first indices and the extents, so that it points at the tile edge"""
    g = got.detach().cpu() if isinstance(got, torch.Tensor) else torch.from_numpy(np.array(got))
    r = torch.from_numpy(np.array(ref)).to(g.dtype)
    assert tuple(g.shape) == tuple(r.shape), "%s: shape %s, reference %s" % (what, tuple(g.shape), tuple(r.shape))
    bad = _bits(g) != _bits(r)
    if bad.any():
        idx = np.argwhere(bad)
        gf, rf = g.float().numpy(), r.float().numpy()
        first = ", ".join("%s: got %g want %g" % (tuple(int(v) for v in i), gf[tuple(i)], rf[tuple(i)]) for i in idx[:8])
        raise AssertionError("%s: %d of %d elements differ bitwise (extents %s; mismatches within %s .. %s); first: %s" % (
            what, idx.shape[0], bad.size, tuple(g.shape), tuple(int(v) for v in idx.min(0)), tuple(int(v) for v in idx.max(0)), first))


# ---- device side ----
class Guarded:
    """a device tensor of `shape` inside a larger allocation, with GUARD_BYTES of GUARD_BYTE in front and (rounded up to 256) behind.
    fill: a number (NaN by default; for uint8 a byte) or an array / tensor of start values"""

    def __init__(self, shape, dtype, fill=float("nan")):
        shape = tuple(int(s) for s in shape)
        self.nbytes = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
        body = (self.nbytes + 255) // 256 * 256
        self.raw = torch.full((2 * GUARD_BYTES + body,), GUARD_BYTE, dtype=torch.uint8, device=DEV)
        self.t = self.raw[GUARD_BYTES:GUARD_BYTES + self.nbytes].view(dtype).view(shape)
        assert self.t.data_ptr() % 256 == 0
        if isinstance(fill, (np.ndarray, torch.Tensor)):
            self.t.copy_(torch.tensor(np.array(fill) if isinstance(fill, np.ndarray) else fill).reshape(shape).to(dtype))
        else:
            self.t.fill_(fill)

    def data_ptr(self):
        return self.t.data_ptr()

    def check(self, what, finite=True):
        lo, hi = self.raw[:GUARD_BYTES], self.raw[GUARD_BYTES + self.nbytes:]
        for name, band in (("in front of", lo), ("behind", hi)):
            hit = torch.nonzero(band != GUARD_BYTE).flatten()
            assert hit.numel() == 0, "%s: %d guard bytes %s the buffer were overwritten (first at byte %d of the band)" % (
                what, hit.numel(), name, int(hit[0]))
        if finite:
            nf = torch.nonzero(~torch.isfinite(self.t.float()).flatten()).flatten()
            assert nf.numel() == 0, "%s: %d of %d elements were left NaN / not finite (first at flat index %d, shape %s)" % (
                what, nf.numel(), self.t.numel(), int(nf[0]), tuple(self.t.shape))


class Fenced:
    """a read-only source inside a larger allocation whose other elements are NaN (`pad` elements on each side, a multiple of 128 so that
    the view keeps 256-byte alignment): a kernel that reads past either end of the source poisons its result"""

    def __init__(self, t, pad=2048):
        assert pad % 128 == 0
        self.raw = torch.full((t.numel() + 2 * pad,), float("nan"), dtype=t.dtype, device=DEV)
        self.t = self.raw[pad:pad + t.numel()].view(t.shape)
        self.t.copy_(t)
        assert self.t.data_ptr() % 256 == 0

    def data_ptr(self):
        return self.t.data_ptr()


def adjacent(t0, t1):
    """t0 and t1 in ONE allocation, t1 at the next 256-byte boundary behind t0 (as a workspace lays two tensors out) -> the two views"""
    es = t0.element_size()
    off = (t0.numel() * es + 255) // 256 * 256 // es
    raw = torch.zeros((off + t1.numel(),), dtype=t0.dtype, device=DEV)
    a, b = raw[:t0.numel()].view(t0.shape), raw[off:off + t1.numel()].view(t1.shape)
    a.copy_(t0)
    b.copy_(t1)
    return a, b


def poisoned_scratch(cin, cout, D=1, H=1, W=1):
    """unet_op_scratch_bytes() bytes of 0xFF, guarded"""
    import unet_studio_amd as U
    b = C.c_size_t()
    U.engine.check(U.engine.lib.unet_op_scratch_bytes(cin, cout, D, H, W, C.byref(b)))
    return Guarded((b.value,), torch.uint8, 0xFF)


def check_all(what, *named):
    """guards (and finiteness, except for scratch) of every buffer of a call: pairs (name, Guarded)"""
    for name, gb in named:
        gb.check("%s %s" % (what, name), finite=gb.t.dtype != torch.uint8)


def to_cl(x, dt):  # numpy [C,D,H,W] -> device channels-last [D,H,W,C]
    return torch.from_numpy(np.array(np.transpose(x, (1, 2, 3, 0)), order="C")).to(DEV).to(TDT[dt]).contiguous()


def cf(t):  # device [D,H,W,C] -> the same tensor seen as [C,D,H,W]
    return t.permute(3, 0, 1, 2)
