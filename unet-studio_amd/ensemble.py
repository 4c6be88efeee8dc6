"""A model ensemble: the level-0 logits of several models (folds, seeds) for one volume become softmax probabilities one member at a
time and are folded, weighted, into a running state {C + 2, voxels} that does not grow with the number of members; a closing pass
reads the state into the label map, the mean probabilities and two voxel-wise uncertainty maps (include/unet_ensemble.h).

The reference has no counterpart (it evaluates one network per run).  The members, the state, the entropy and the mutual
information are this project's definitions, written down in the header: parity with TIPL is NOT pinned.

`normalize_weights`, `normalized_entropy` and `state_bytes` are host only.  `accumulate` and `finalize` run the two kernels on the
current stream; `combine` is the convenience over a list of members.  `entropy` is the entropy of the mean prediction in nats
(high when the members disagree OR when every member is unsure), `mutual_info` is that entropy minus the members' mean entropy
(high only when they disagree).  Shapes are torch's (d, h, w).

The state costs (C + 2) * voxels * 4 bytes on the device (6 classes at 128^3: 67 MB), whatever the number of members."""
import ctypes as C
import math

import numpy as np
import torch

from . import engine as E
from . import space as SP
from .engine import UNetError

E._sig("unet_ens_state_bytes", C.c_int, C.c_int, C.c_int64, C.POINTER(C.c_size_t))
E._sig("unet_ens_accumulate", C.c_int, C.c_void_p, C.c_int, C.c_int64, C.c_float, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p)
E._sig("unet_ens_finalize", C.c_int, C.c_void_p, C.c_size_t, C.c_int, C.c_int64, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
       C.c_void_p, C.c_void_p)
# every symbol include/unet_ensemble.h declares
EXPORTS = ["unet_ens_state_bytes", "unet_ens_accumulate", "unet_ens_finalize"]

UNCERTAINTY = ("entropy", "mutual_info")
OUTPUTS = SP.OUTPUTS + UNCERTAINTY


# ---- host only -------------------------------------------------------------------------------------------------------------------
def state_bytes(out_c, voxels):
    """bytes of the state {out_c + 2, voxels} fp32; the library's refusal of the arguments raises"""
    return E.size_query(E.lib.unet_ens_state_bytes, int(out_c), int(voxels))


def normalize_weights(weights, n):
    """The members' weights as n Python floats that sum to 1 (in double; each is handed to the kernel as fp32).  None: equal
    weights 1/n.  Raises UNetError for a wrong length and for an entry that is not finite or not positive."""
    n = int(n)
    if n < 1:
        raise UNetError("ensemble: at least one member, got %d" % n)
    if weights is None:
        return [1.0 / n] * n
    try:
        ws = [float(w) for w in weights]
    except (TypeError, ValueError):
        raise UNetError("ensemble_weights must be a list of numbers, got %r" % (weights,))
    if len(ws) != n:
        raise UNetError("ensemble_weights: %d weights for %d members" % (len(ws), n))
    for w in ws:
        if not math.isfinite(w) or w <= 0.0:
            raise UNetError("ensemble_weights: a weight must be finite and positive, got %r" % (w,))
    try:
        total = math.fsum(ws)
    except OverflowError:
        total = math.inf
    if not math.isfinite(total):
        raise UNetError("ensemble_weights: the weights' sum is not finite")
    return [w / total for w in ws] if n > 1 else [1.0]


def normalized_entropy(h, out_c):
    """h / ln(out_c): an entropy in nats (a number, a numpy array or a tensor) as a fraction of the largest one out_c classes allow"""
    out_c = int(out_c)
    if out_c < 2:
        raise UNetError("normalized_entropy: out_c must be at least 2, got %d" % out_c)
    return h / math.log(out_c)


# ---- the device calls ------------------------------------------------------------------------------------------------------------
def _f32(a, name):
    if not (torch.is_tensor(a) and a.is_cuda and a.dtype == torch.float32 and a.is_contiguous()):
        raise UNetError("ensemble: %s must be a contiguous float32 device tensor" % name)
    return a


def _state(state, out_c, voxels):
    need = state_bytes(out_c, voxels)                  # the class / size checks first
    if not (torch.is_tensor(state) and state.is_cuda and state.is_contiguous()):
        raise UNetError("ensemble: the state must be a contiguous device tensor (state_bytes)")
    if state.nbytes < need:
        raise UNetError("ensemble: the state holds %d bytes, %d classes at %d voxels need %d" % (state.nbytes, out_c, voxels, need))
    return state


def new_state(out_c, voxels, device):
    """an uninitialised state for out_c classes at `voxels` voxels (the first member overwrites it)"""
    return torch.empty(state_bytes(out_c, voxels), dtype=torch.uint8, device=device)


def accumulate(logits, state, weight, first):
    """unet_ens_accumulate on the current stream.  logits: one member's {C, d, h, w} (or {1, C, d, h, w}), a contiguous fp32 device
    tensor; state: a device tensor of at least state_bytes(C, d*h*w) bytes; weight: this member's normalised weight, in (0, 1];
    first: True for member 0, which overwrites the state without reading it."""
    logits = _f32(logits, "logits")
    if logits.dim() == 5 and logits.shape[0] == 1:
        logits = logits[0]
    if logits.dim() != 4:
        raise UNetError("ensemble: a member's logits must be {C, d, h, w}, got %s" % (tuple(logits.shape),))
    out_c, voxels = int(logits.shape[0]), int(logits[0].numel())
    _state(state, out_c, voxels)
    if state.device != logits.device:
        raise UNetError("ensemble: the state and the logits are on different devices")
    E.check(E.lib.unet_ens_accumulate(logits.data_ptr(), out_c, voxels, float(weight), int(bool(first)), state.data_ptr(), state.nbytes,
                                      E.stream(logits)))
    return state


def _take(out, name, shape, dt, dev):
    t = (out or {}).get(name)
    if t is None:
        return torch.empty(shape, dtype=dt, device=dev)
    if not (torch.is_tensor(t) and t.is_cuda and t.dtype == dt and t.is_contiguous() and t.numel() == int(np.prod(shape))
            and t.device == dev):
        raise UNetError("ensemble: out[%s] must be a contiguous %s tensor of %d values on the state's device" % (name, dt, int(np.prod(shape))))
    return t


def finalize(state, out_c, shape, threshold=0.5, outputs=("label",), out=None):
    """unet_ens_finalize on the current stream.  state: what accumulate filled; shape: (d, h, w).  Returns {name: tensor} for the
    wanted outputs: label_prob {out_c-1, d, h, w} fp32, fg_prob {d, h, w} fp32, label {d, h, w} uint16, entropy and mutual_info
    {d, h, w} fp32.  out: {name: tensor} to write into instead of new ones."""
    outputs = tuple(outputs)
    for o in outputs:
        if o not in OUTPUTS:
            raise UNetError("unknown output %s (one of %s)" % (o, ", ".join(OUTPUTS)))
    if not outputs:
        raise UNetError("ensemble: no output wanted")
    out_c = int(out_c)
    D, H, W = SP._shape3(shape, "shape")
    _state(state, out_c, D * H * W)
    dev = state.device
    shapes = {"label_prob": ((out_c - 1, D, H, W), torch.float32), "fg_prob": ((D, H, W), torch.float32),
              "label": ((D, H, W), torch.uint16), "entropy": ((D, H, W), torch.float32), "mutual_info": ((D, H, W), torch.float32)}
    res = {o: _take(out, o, shapes[o][0], shapes[o][1], dev) for o in outputs}
    ptr = lambda o: res[o].data_ptr() if o in res else None
    E.check(E.lib.unet_ens_finalize(state.data_ptr(), state.nbytes, out_c, D * H * W, float(threshold), ptr("label_prob"), ptr("fg_prob"),
                                    ptr("label"), ptr("entropy"), ptr("mutual_info"), E.stream(state)))
    return res


def combine(members, weights=None, threshold=0.5, outputs=("label",), state=None):
    """The ensemble of a list of members' logits, each {C, d, h, w} (a contiguous fp32 device tensor, all of one shape): accumulate
    in list order, then finalize.  weights: one per member (normalize_weights), None for equal ones; state: a device tensor to
    reuse.  Returns {output: tensor}."""
    members = list(members)
    ws = normalize_weights(weights, len(members))
    first = _f32(members[0], "members[0]")
    if first.dim() == 5 and first.shape[0] == 1:
        first = first[0]
    if first.dim() != 4:
        raise UNetError("ensemble: a member's logits must be {C, d, h, w}, got %s" % (tuple(first.shape),))
    shape = tuple(first.shape)
    for k, mem in enumerate(members):
        if not torch.is_tensor(mem) or tuple(mem.shape[-4:]) != shape:
            raise UNetError("ensemble: member %d is %s, member 0 is %s" % (k, tuple(getattr(mem, "shape", ())), shape))
    out_c, voxels = int(shape[0]), int(np.prod(shape[1:]))
    if state is None:
        state = new_state(out_c, voxels, first.device)
    for k, (mem, w) in enumerate(zip(members, ws)):
        accumulate(mem, state, w, k == 0)
    return finalize(state, out_c, shape[1:], threshold, outputs)
