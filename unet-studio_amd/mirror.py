"""Test-time mirroring: a volume is run through the network under every combination of axis flips, and the members' logits are
flipped back, their lateralised channels swapped back, and averaged before softmax / argmax (include/unet_mirror.h).

The reference has no counterpart (its flips are the orientation's only).  The members, the swap, the combine and the agreement are
this project's definitions, written down in the header: parity with TIPL is NOT pinned.

`parse_axes`, `check_swap`, `stack_bytes` and `_combine_reference` are host only.  `flip_input` and `forward_members` make the stack
(one forward per member), `combine` and `postproc_mirror` run the two kernels on the current stream.  Masks are ascending ints, bit 0
= x, bit 1 = y, bit 2 = z; a swap is (axis, [(a, b), ...]) with the axis a letter or 0, 1, 2.  Shapes are torch's (d, h, w).

The member stack costs K * out_c * voxels * 4 bytes on the device (8 members of 6 x 128^3: 403 MB), and K forwards."""
import ctypes as C

import numpy as np
import torch

from . import engine as E
from . import space as SP
from .engine import UNetError

MAX_PAIRS = 64      # UNET_MIRROR_MAX_PAIRS
MAX_MEMBERS = 8     # UNET_MIRROR_MAX_MEMBERS

_ip = C.POINTER(C.c_int)
E._sig("unet_mirror_combine", C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _ip, C.c_int, _ip, C.c_int, C.c_void_p,
       C.c_void_p, C.c_void_p)
E._sig("unet_mirror_postproc", C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _ip, C.c_int, _ip, C.c_int, C.c_float,
       C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p)
# every symbol include/unet_mirror.h declares
EXPORTS = ["unet_mirror_combine", "unet_mirror_postproc"]

OUTPUTS = SP.OUTPUTS + ("agreement",)
_AXIS = {"x": 0, "y": 1, "z": 2}
_FLIPS = ("flip_x", "flip_y", "flip_z")


# ---- the members and the swap (host only) ----------------------------------------------------------------------------------------
def parse_axes(text):
    """'xz' -> [0, 1, 4, 5]: the masks of all subsets of the axes, ascending (include/unet_mirror.h, MEMBERS).  None / '' -> [0]."""
    if text is None:
        text = ""
    if not isinstance(text, str):
        raise UNetError("mirror_axes must be a string of the letters x, y, z, got %r" % (text,))
    bits = 0
    for ch in text:
        if ch not in _AXIS:
            raise UNetError("mirror_axes: unknown axis %r in %r (letters x, y, z)" % (ch, text))
        if bits >> _AXIS[ch] & 1:
            raise UNetError("mirror_axes: axis %s is repeated in %r" % (ch, text))
        bits |= 1 << _AXIS[ch]
    return [m for m in range(8) if m & ~bits == 0]


def _masks(masks):
    try:
        ms = [int(m) for m in masks]
    except (TypeError, ValueError):
        raise UNetError("mirror: masks must be a list of ints (parse_axes)")
    if len(ms) not in (1, 2, 4, 8):
        raise UNetError("mirror: masks must hold 1, 2, 4 or 8 members, got %d" % len(ms))
    if ms[0] != 0 or any(b <= a for a, b in zip(ms, ms[1:])) or ms[-1] > 7:
        raise UNetError("mirror: masks must start at 0, strictly ascend and stay in [0, 7], got %s" % (ms,))
    return ms


def check_swap(swap_axis, pairs, out_c, masks):
    """The SWAP of include/unet_mirror.h: returns (axis as -1, 0, 1, 2, [(a, b), ...]); raises UNetError.  swap_axis: a letter, 0, 1, 2,
    or None / -1 for none."""
    ms = _masks(masks)
    if swap_axis is None or swap_axis == -1:
        axis = -1
    elif swap_axis in _AXIS:
        axis = _AXIS[swap_axis]
    elif swap_axis in (0, 1, 2) and not isinstance(swap_axis, bool):
        axis = int(swap_axis)
    else:
        raise UNetError("mirror_swap: the axis must be x, y or z (or 0, 1, 2), got %r" % (swap_axis,))
    try:
        ps = [(int(a), int(b)) for a, b in (pairs or [])]
    except (TypeError, ValueError):
        raise UNetError("mirror_swap: pairs must be a list of (a, b) channel pairs")
    if len(ps) > MAX_PAIRS:
        raise UNetError("mirror_swap: at most %d pairs, got %d" % (MAX_PAIRS, len(ps)))
    if ps and axis < 0:
        raise UNetError("mirror_swap: pairs given without a swap axis")
    if axis >= 0 and not any(m >> axis & 1 for m in ms):
        raise UNetError("mirror_swap: axis %s is not among the mirrored axes" % "xyz"[axis])
    seen = set()
    for a, b in ps:
        if a == b:
            raise UNetError("mirror_swap: a pair swaps two different classes, got (%d, %d)" % (a, b))
        for v in (a, b):
            if not 0 <= v < int(out_c):
                raise UNetError("mirror_swap: class %d is not in [0, %d)" % (v, int(out_c)))
            if v in seen:
                raise UNetError("mirror_swap: class %d is in more than one pair" % v)
            seen.add(v)
    return axis, ps


def _swap(swap, out_c, masks):
    if swap is None:
        return -1, []
    try:
        axis, pairs = swap
    except (TypeError, ValueError):
        raise UNetError("mirror_swap must be (axis, [(a, b), ...]) or None, got %r" % (swap,))
    return check_swap(axis, pairs, out_c, masks)


def stack_bytes(masks, out_c, voxels):
    """bytes of the member stack {K, out_c, voxels} fp32"""
    return len(_masks(masks)) * int(out_c) * int(voxels) * 4


def _combine_reference(stack_np, masks, swap=None):
    """The numpy restatement of COMBINE and AGREEMENT (include/unet_mirror.h): stack {K, C, D, H, W} float32 -> (mean {C, D, H, W}
    float32, agreement {D, H, W} uint8).  Host only; the tests on both sides pin this text."""
    stack = np.asarray(stack_np, dtype=np.float32)
    ms = _masks(masks)
    if stack.ndim != 5 or stack.shape[0] != len(ms):
        raise UNetError("mirror: the stack must be {%d members, out_c, d, h, w}, got %s" % (len(ms), stack.shape))
    Cn = stack.shape[1]
    axis, pairs = _swap(swap, Cn, ms)
    sigma = np.arange(Cn)
    for a, b in pairs:
        sigma[a], sigma[b] = b, a
    back = []                                                    # member m brought back: stack[m][sigma_m(c)][FLIP_m(v)]
    for k, m in enumerate(ms):
        v = stack[k]
        if m & 1:
            v = v[:, :, :, ::-1]
        if m & 2:
            v = v[:, :, ::-1, :]
        if m & 4:
            v = v[:, ::-1, :, :]
        if axis >= 0 and m >> axis & 1:
            v = v.take(sigma, axis=0)
        back.append(np.ascontiguousarray(v))
    with np.errstate(invalid="ignore", over="ignore"):
        mean = back[0].copy()
        for v in back[1:]:
            mean = (mean + v).astype(np.float32)                 # fp32 adds in member order
        if len(ms) > 1:
            mean = (mean * np.float32(1.0 / len(ms))).astype(np.float32)

        def amax(x):                                             # best = 0; a later channel wins only when greater
            best = np.zeros(x.shape[1:], dtype=np.int64)
            bv = x[0].copy()
            for c in range(1, Cn):
                win = x[c] > bv                                  # a comparison with NaN is false
                best[win] = c
                bv[win] = x[c][win]
            return best

        top = amax(mean)
        agreement = np.zeros(mean.shape[1:], dtype=np.uint8)
        for v in back:
            agreement += (amax(v) == top).astype(np.uint8)
    return mean, agreement


# ---- the members' forwards -------------------------------------------------------------------------------------------------------
def flip_input(x, mask):
    """x {C_in, d, h, w}, a contiguous fp32 device tensor -> its FLIP_mask copy through the exact permute of preproc.py, one call
    per set bit; mask 0 returns x itself."""
    from . import preproc as PRE
    mask = int(mask)
    if not 0 <= mask <= 7:
        raise UNetError("mirror: a mask must be in [0, 7], got %d" % mask)
    for bit in range(3):
        if mask >> bit & 1:
            x = PRE.apply(_FLIPS[bit], x)
    return x


def forward_members(model, x, masks, packed_sizes=None, out=None):
    """x {C_in, d, h, w} on the device -> the stack {K, out_count, d, h, w} of level-0 logits, one forward per member on the flipped
    input, written straight into its slot.  packed_sizes: the set of volume sizes whose filter packs are current (the weights are
    frozen); it is updated.  out: a contiguous fp32 device tensor of at least that many values to reuse."""
    ms = _masks(masks)
    x = SP._f32(x, "x")
    if x.dim() != 4:
        raise UNetError("mirror: x must be {C_in, d, h, w}, got %s" % (tuple(x.shape),))
    size = tuple(int(v) for v in x.shape[1:])
    shape = (len(ms), int(model.out_count)) + size
    n = int(np.prod(shape))
    if out is None:
        stack = torch.empty(shape, dtype=torch.float32, device=x.device)
    elif SP._f32(out, "out").numel() < n or out.device != x.device:
        raise UNetError("mirror: out must hold %d values on x's device" % n)
    else:
        stack = out.view(-1)[:n].view(shape)
    packed = packed_sizes if packed_sizes is not None else set()
    for k, m in enumerate(ms):
        y = model.forward(flip_input(x, m).unsqueeze(0), packs_current=size in packed)[0]
        packed.add(size)
        stack[k].copy_(y.view(shape[1:]))
    return stack


# ---- the device calls ------------------------------------------------------------------------------------------------------------
def _stack(stack, ms):
    if not (torch.is_tensor(stack) and stack.is_cuda and stack.dtype == torch.float32 and stack.is_contiguous()):
        raise UNetError("mirror: the stack must be a contiguous float32 device tensor")
    if stack.dim() != 5 or stack.shape[0] != len(ms):
        raise UNetError("mirror: the stack must be {%d members, out_c, d, h, w}, got %s" % (len(ms), tuple(stack.shape)))
    return tuple(int(v) for v in stack.shape[1:])


def _host_args(ms, axis, pairs):
    flat = [v for p in pairs for v in p]
    return (C.c_int * len(ms))(*ms), axis, ((C.c_int * len(flat))(*flat) if flat else None), len(pairs)


def _take(out, name, shape, dt, dev):
    t = (out or {}).get(name)
    if t is None:
        return torch.empty(shape, dtype=dt, device=dev)
    if not (torch.is_tensor(t) and t.is_cuda and t.dtype == dt and t.is_contiguous() and t.numel() == int(np.prod(shape))
            and t.device == dev):
        raise UNetError("mirror: out[%s] must be a contiguous %s tensor of %d values on the stack's device" % (name, dt, int(np.prod(shape))))
    return t


def combine(stack, masks, swap=None, want_mean=True, want_agreement=False, out=None):
    """unet_mirror_combine on the current stream.  stack: {K, out_c, d, h, w}, a contiguous fp32 device tensor; masks: parse_axes';
    swap: (axis, pairs) or None.  Returns (mean {out_c, d, h, w} fp32 or None, agreement {d, h, w} uint8 or None).  out: {"mean": ...,
    "agreement": ...} tensors to write into instead of new ones."""
    ms = _masks(masks)
    out_c, D, H, W = _stack(stack, ms)
    axis, pairs = _swap(swap, out_c, ms)
    if not (want_mean or want_agreement):
        raise UNetError("mirror: no output wanted")
    dev = stack.device
    mean = _take(out, "mean", (out_c, D, H, W), torch.float32, dev) if want_mean else None
    agr = _take(out, "agreement", (D, H, W), torch.uint8, dev) if want_agreement else None
    cm, ax, cp, npairs = _host_args(ms, axis, pairs)
    E.check(E.lib.unet_mirror_combine(stack.data_ptr(), out_c, W, H, D, len(ms), cm, ax, cp, npairs,
                                      mean.data_ptr() if mean is not None else None, agr.data_ptr() if agr is not None else None,
                                      E.stream(stack)))
    return mean, agr


def postproc_mirror(stack, masks, swap=None, threshold=0.5, outputs=SP.OUTPUTS, out=None):
    """unet_mirror_postproc on the current stream: softmax / create_mask / argmax of the combined logits, which are never stored.
    Arguments as combine's.  Returns {name: tensor} for the wanted outputs: label_prob {out_c-1, d, h, w} fp32, fg_prob {d, h, w}
    fp32, label {d, h, w} uint16, agreement {d, h, w} uint8.  out: {name: tensor} to write into instead of new ones."""
    outputs = tuple(outputs)
    for o in outputs:
        if o not in OUTPUTS:
            raise UNetError("unknown output %s (one of %s)" % (o, ", ".join(OUTPUTS)))
    if not outputs:
        raise UNetError("mirror: no output wanted")
    ms = _masks(masks)
    out_c, D, H, W = _stack(stack, ms)
    axis, pairs = _swap(swap, out_c, ms)
    dev = stack.device
    shapes = {"label_prob": ((out_c - 1, D, H, W), torch.float32), "fg_prob": ((D, H, W), torch.float32),
              "label": ((D, H, W), torch.uint16), "agreement": ((D, H, W), torch.uint8)}
    res = {o: _take(out, o, shapes[o][0], shapes[o][1], dev) for o in outputs}
    ptr = lambda o: res[o].data_ptr() if o in res else None
    cm, ax, cp, npairs = _host_args(ms, axis, pairs)
    E.check(E.lib.unet_mirror_postproc(stack.data_ptr(), out_c, W, H, D, len(ms), cm, ax, cp, npairs, float(threshold),
                                       ptr("label_prob"), ptr("fg_prob"), ptr("label"), ptr("agreement"), E.stream(stack)))
    return res
