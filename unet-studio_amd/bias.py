"""The intensity-inhomogeneity correction on the device (include/unet_bias.h): the smooth multiplicative shading of an MR scan, fitted as
a field on a lattice over the voxels whose tissue a label map (the network's, or an atlas's) says is uniform, and removed.

  logcode          q = 4096 * log2 v truncated, exact integer arithmetic; NONE for what has no logarithm
  levels           per listed class the floored mean of q minus the field: the tissue's own level
  residual         r = q - its class's level as int16, SKIP for a voxel that does not count (no class, no q, outside the clip)
  sweep            one sweep: 8 colour passes, every node of a colour moves to the rounded minimiser of its quadratic
  refine           a field on the lattice of spacing g brought onto that of g / 2
  cost             the sum of (r - field)^2 over the voxels that count, and their number
  fit              the whole schedule, enqueued at once: levels of (g, sweeps, lam), `outer` rounds of levels + residual + sweeps each
  apply            v * 2^-field: one rounded multiply by a table entry and one scaling; optionally the gain itself
  correct          logcode, fit, apply
  gain             the gain map of a field alone
  Plan             the classes, the schedule, the clip and the impl of `correct`
  summary, cv      host arithmetic: fit's report decoded; a class's coefficient of variation

The field is int32 {nz, ny, nx} in 1/4096 of a log2 unit on `lattice(shape, g)`, g in (4, 8, 16, 32).  These are this project's
definitions (parity with outside tools NOT pinned).  Everything but apply's one multiply is integer arithmetic: the results are pinned
to the numpy restatement of tests/bias_ref.py bit for bit.  IMPL_NODE runs a block per lattice node, IMPL_VOXEL a thread per voxel
with two 64-bit atomic counters per node (the measured baseline and a second witness of the bits)."""
import collections
import ctypes as C
import math

import numpy as np
import torch

from . import engine as E
from . import register as R
from .engine import UNetError

_ip = C.POINTER(C.c_int)
_vol = (C.c_int, C.c_int, C.c_int)                                  # w, h, d
_lab = (C.c_void_p, C.c_void_p, C.c_int, *_vol, _ip, C.c_int)       # q, labels, lbytes, w, h, d, classes, K
E._sig("unet_bias_lattice", C.c_int, *_vol, C.c_int, _ip, _ip, _ip)
E._sig("unet_bias_scratch_bytes", C.c_int, *_vol, _ip, C.c_int, C.POINTER(C.c_size_t))
E._sig("unet_bias_logcode", C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p)
E._sig("unet_bias_levels", C.c_int, *_lab, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p)
E._sig("unet_bias_residual", C.c_int, *_lab, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p)
E._sig("unet_bias_sweep", C.c_int, C.c_void_p, *_vol, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p)
E._sig("unet_bias_refine", C.c_int, C.c_void_p, *_vol, C.c_int, C.c_void_p, C.c_void_p)
E._sig("unet_bias_cost", C.c_int, C.c_void_p, *_vol, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p)
E._sig("unet_bias_fit", C.c_int, *_lab, C.c_int, _ip, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p)
E._sig("unet_bias_apply", C.c_int, C.c_void_p, *_vol, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p)
# every symbol include/unet_bias.h declares
EXPORTS = ["unet_bias_lattice", "unet_bias_scratch_bytes", "unet_bias_logcode", "unet_bias_levels", "unet_bias_residual", "unet_bias_sweep",
           "unet_bias_refine", "unet_bias_cost", "unet_bias_fit", "unet_bias_apply"]

IMPL_DEFAULT, IMPL_NODE, IMPL_VOXEL = 0, 1, 2
NONE, SKIP, MAX = -2 ** 31, -2 ** 15, 8192
MAX_CLASSES, MAX_LAM, MAX_LEVELS, MAX_SWEEPS, MAX_OUTER, MAX_ROWS = 16, 4096, 4, 16, 8, 32
SPACINGS = (4, 8, 16, 32)
DEFAULT_LEVELS = [(32, 4, 1), (16, 4, 1), (8, 4, 1)]                # (g, sweeps, lam); chosen on the phantom of DESIGN.md §37
DEFAULT_OUTER = 2
DEFAULT_CLIP = 2048                                                 # half a log2 unit around a class's level

Plan = collections.namedtuple("Plan", ("classes", "levels", "outer", "clip", "impl"),
                              defaults=(DEFAULT_LEVELS, DEFAULT_OUTER, DEFAULT_CLIP, IMPL_DEFAULT))
Plan.__doc__ = ("How a scan's inhomogeneity is fitted: the label values whose tissue is taken to be uniform, the levels (g, sweeps, lam) "
                "and outer rounds of bias.fit, the clip (Q12) beyond which a voxel is left out, and the impl.")


def _dims(shape, who):
    try:
        d, h, w = (int(v) for v in shape)
    except (TypeError, ValueError):
        raise UNetError("bias.%s: a shape is (D, H, W)" % who)
    return w, h, d


def lattice(shape, g):
    """(nz, ny, nx), the nodes of the lattice of spacing g over a grid (D, H, W): (dim + g - 1) // g + 1 per axis."""
    n = [C.c_int() for _ in range(3)]
    E.check(E.lib.unet_bias_lattice(*_dims(shape, "lattice"), int(g), *(C.byref(v) for v in n)))
    return n[2].value, n[1].value, n[0].value


def levels_of(levels, who="bias.fit"):
    """int32 {n, 3}: rows of (g, sweeps, lam)"""
    try:
        rows = [[int(v) for v in lv] for lv in levels]
        if not rows or any(len(lv) != 3 for lv in rows):
            raise ValueError
    except (TypeError, ValueError):
        raise UNetError("%s: levels must be rows of (g, sweeps, lam) integers" % who)
    return np.ascontiguousarray(np.asarray(rows, np.int32).reshape(-1, 3))


def scratch_bytes(shape, levels):
    """The scratch of a fit of `levels` (rows of (g, sweeps, lam)); a sweep takes `sweep_scratch_bytes`."""
    lv = levels_of(levels, "bias.scratch_bytes")
    return E.size_query(E.lib.unet_bias_scratch_bytes, *_dims(shape, "scratch_bytes"), lv.ctypes.data_as(_ip), int(lv.shape[0]))


def sweep_scratch_bytes(shape, g):
    """The scratch of one sweep at g: the two 64-bit counters per node behind an aligned base, 256 + 16 B per node rounded up to 256."""
    return 256 + (16 * int(np.prod(lattice(shape, g))) + 255) // 256 * 256


def _classes(classes, who):
    try:
        cls = [int(v) for v in classes]
    except (TypeError, ValueError):
        raise UNetError("bias.%s: classes must be label values" % who)
    return (C.c_int * max(1, len(cls)))(*cls), len(cls)


def _volume(t, dtypes, name, who, like=None):
    ok = torch.is_tensor(t) and t.is_cuda and t.dtype in dtypes and t.is_contiguous() and t.dim() == 3 and t.numel() > 0
    if not ok or (like is not None and (t.device != like.device or t.shape != like.shape)):
        raise UNetError("bias.%s: %s must be a contiguous (D, H, W) %s device tensor%s"
                        % (who, name, " or ".join(str(d).replace("torch.", "") for d in dtypes), "" if like is None else " like the first"))
    return t


def _labelled(q, labels, classes, who):
    _volume(q, (torch.int32,), "q", who)
    _volume(labels, (torch.uint8, torch.uint16), "labels", who, q)
    d, h, w = (int(v) for v in q.shape)
    cls, K = _classes(classes, who)
    return (q.data_ptr(), labels.data_ptr(), labels.element_size(), w, h, d, cls, K)


def _field(B, shape, g, dev, who):
    want = lattice(tuple(shape), g)
    if not (torch.is_tensor(B) and B.is_cuda and (dev is None or B.device == dev) and B.dtype == torch.int32 and B.is_contiguous()
            and tuple(B.shape) == want):
        raise UNetError("bias.%s: B must be a contiguous int32 %s device tensor" % (who, list(want)))
    return B


def logcode(volume, out=None, stream=None):
    """unet_bias_logcode on the current stream (or the raw `stream`): int32 q like the float32 `volume`.  No host synchronisation."""
    _volume(volume, (torch.float32,), "volume", "logcode")
    q = R._out(out, volume.numel(), torch.int32, volume.device, "out", "logcode", "bias")
    E.check(E.lib.unet_bias_logcode(volume.data_ptr(), volume.numel(), q.data_ptr(), E.stream(volume, stream)))
    return q.view(volume.shape)


def levels(q, labels, classes, B, g, out=None, stream=None):
    """unet_bias_levels on the current stream (or the raw `stream`): int64 {MAX_CLASSES, 3} on the device, row t = (m_t, count, sum)
    of class t under the field B; (NONE, 0, 0) for a class without a voxel and past the classes.  No host synchronisation."""
    a = _labelled(q, labels, classes, "levels")
    _field(B, q.shape, g, q.device, "levels")
    lev = R._out(out, MAX_CLASSES * 3, torch.int64, q.device, "out", "levels", "bias")
    E.check(E.lib.unet_bias_levels(*a, B.data_ptr(), int(g), lev.data_ptr(), E.stream(q, stream)))
    return lev.view(MAX_CLASSES, 3)


def residual(q, labels, classes, lev, clip=DEFAULT_CLIP, out=None, stream=None):
    """unet_bias_residual on the current stream (or the raw `stream`): int16 r like q from the table of `levels`.  `out` must be
    16-byte aligned.  No host synchronisation."""
    a = _labelled(q, labels, classes, "residual")
    if not (torch.is_tensor(lev) and lev.is_cuda and lev.device == q.device and lev.dtype == torch.int64 and lev.is_contiguous()
            and lev.numel() == MAX_CLASSES * 3):
        raise UNetError("bias.residual: lev must be the int64 {%d, 3} device tensor of bias.levels" % MAX_CLASSES)
    r = R._out(out, q.numel(), torch.int16, q.device, "out", "residual", "bias")
    E.check(E.lib.unet_bias_residual(*a, lev.data_ptr(), int(clip), r.data_ptr(), E.stream(q, stream)))
    return r.view(q.shape)


def sweep(r, B, g, lam, impl=IMPL_DEFAULT, scratch=None, stream=None):
    """unet_bias_sweep on the current stream (or the raw `stream`): one sweep over B IN PLACE.  Returns info int64 {2} on the device:
    nodes changed, nodes visited.  No host synchronisation."""
    _volume(r, (torch.int16,), "r", "sweep")
    _field(B, r.shape, g, r.device, "sweep")
    d, h, w = (int(v) for v in r.shape)
    scratch = E.scratch(scratch, sweep_scratch_bytes(tuple(r.shape), g), r.device)
    info = torch.empty(2, dtype=torch.int64, device=r.device)
    E.check(E.lib.unet_bias_sweep(r.data_ptr(), w, h, d, B.data_ptr(), int(g), int(lam), info.data_ptr(), int(impl), scratch.data_ptr(),
                                  scratch.nbytes, E.stream(r, stream)))
    return info


def refine(B, shape, g, out=None, stream=None):
    """unet_bias_refine on the current stream (or the raw `stream`): B on the lattice of spacing g over the grid (D, H, W) -> the field
    on the lattice of g // 2, each fine node the rounded mean of the coarse nodes around it.  No host synchronisation."""
    w, h, d = _dims(shape, "refine")
    if isinstance(g, bool) or g not in (8, 16, 32):
        raise UNetError("bias.refine: g must be 8, 16 or 32, got %r" % (g,))
    _field(B, (d, h, w), g, None, "refine")
    fine = lattice((d, h, w), g // 2)
    out = R._out(out, int(np.prod(fine)), torch.int32, B.device, "out", "refine", "bias")
    E.check(E.lib.unet_bias_refine(B.data_ptr(), w, h, d, int(g), out.data_ptr(), E.stream(B, stream)))
    return out.view(fine)


def cost(r, B, g, out=None, stream=None):
    """unet_bias_cost on the current stream (or the raw `stream`): int64 {2} on the device = the sum of (r - field)^2 over the voxels
    that count (Q12 squared), and their number.  No host synchronisation."""
    _volume(r, (torch.int16,), "r", "cost")
    _field(B, r.shape, g, r.device, "cost")
    d, h, w = (int(v) for v in r.shape)
    c = R._out(out, 2, torch.int64, r.device, "out", "cost", "bias")
    E.check(E.lib.unet_bias_cost(r.data_ptr(), w, h, d, B.data_ptr(), int(g), c.data_ptr(), E.stream(r, stream)))
    return c


def fit(q, labels, classes, levels=DEFAULT_LEVELS, outer=DEFAULT_OUTER, clip=DEFAULT_CLIP, impl=IMPL_DEFAULT, scratch=None, stream=None):
    """unet_bias_fit on the current stream (or the raw `stream`): the field from zero through every level.  Returns device tensors: B
    int32 {nz, ny, nx} on the LAST level's lattice and report int64 {MAX_ROWS, 6}: per (level, outer round) g, round, sweeps run,
    nodes changed in the last sweep run, cost, count; -1 past the schedule.  Every launch is enqueued here; no host synchronisation."""
    a = _labelled(q, labels, classes, "fit")
    lv = levels_of(levels)
    need = scratch_bytes(tuple(q.shape), lv)                        # the range checks, before any device work
    scratch = E.scratch(scratch, need, q.device)
    B = torch.empty(lattice(tuple(q.shape), int(lv[-1, 0])), dtype=torch.int32, device=q.device)
    report = torch.empty((MAX_ROWS, 6), dtype=torch.int64, device=q.device)
    E.check(E.lib.unet_bias_fit(*a, int(clip), lv.ctypes.data_as(_ip), int(lv.shape[0]), int(outer), B.data_ptr(), report.data_ptr(),
                                int(impl), scratch.data_ptr(), scratch.nbytes, E.stream(q, stream)))
    return B, report


def apply(volume, B, g, gain=False, out=None, stream=None):
    """unet_bias_apply on the current stream (or the raw `stream`): volume * 2^-field, float32 like `volume` (written into `out` when
    given).  gain: True or a tensor to write into: also the gain map; then (corrected, gain) is returned.  No host synchronisation."""
    _volume(volume, (torch.float32,), "volume", "apply")
    _field(B, volume.shape, g, volume.device, "apply")
    d, h, w = (int(v) for v in volume.shape)
    res = R._out(out, volume.numel(), torch.float32, volume.device, "out", "apply", "bias")
    gn = None
    if gain is not False and gain is not None:
        gn = R._out(None if gain is True else gain, volume.numel(), torch.float32, volume.device, "gain", "apply", "bias")
    E.check(E.lib.unet_bias_apply(volume.data_ptr(), w, h, d, B.data_ptr(), int(g), res.data_ptr(), gn.data_ptr() if gn is not None else None,
                                  E.stream(volume, stream)))
    return res.view(volume.shape) if gn is None else (res.view(volume.shape), gn.view(volume.shape))


def gain(B, g, shape, out=None, stream=None):
    """The gain map 2^-field of B on lattice(shape, g): float32 (D, H, W) on B's device.  No host synchronisation."""
    w, h, d = _dims(shape, "gain")
    _field(B, (d, h, w), g, None, "gain")
    gn = R._out(out, w * h * d, torch.float32, B.device, "out", "gain", "bias")
    E.check(E.lib.unet_bias_apply(None, w, h, d, B.data_ptr(), int(g), None, gn.data_ptr(), E.stream(B, stream)))
    return gn.view(d, h, w)


def _plan(plan, who):
    try:
        classes, lv, outer, clip, impl = list(plan.classes), list(plan.levels), plan.outer, plan.clip, plan.impl
    except (AttributeError, TypeError):
        raise UNetError("%s: plan must be a bias.Plan(classes, levels, outer, clip, impl)" % who)
    for name, v in (("outer", outer), ("clip", clip), ("impl", impl)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise UNetError("%s: bias.%s must be an integer, got %r" % (who, name, v))
    return classes, levels_of(lv, who), int(outer), int(clip), int(impl)


def correct(volume, labels, plan, scratch=None, stream=None):
    """logcode, fit, apply on the current stream (or the raw `stream`).  volume: (D, H, W) float32, labels: uint8 or uint16 like it,
    plan: a bias.Plan.  Returns (corrected, B, g, report): the corrected volume, the field and its spacing, fit's report.  No host
    synchronisation."""
    classes, lv, outer, clip, impl = _plan(plan, "bias.correct")
    q = logcode(volume, stream=stream)
    B, report = fit(q, labels, classes, lv, outer, clip, impl, scratch=scratch, stream=stream)
    g = int(lv[-1, 0])
    return apply(volume, B, g, stream=stream), B, g, report


# ---- host arithmetic ---------------------------------------------------------------------------------------------------------------
def summary(report):
    """fit's report decoded: a list of dict(g, round, sweeps, changed, cost, count, rms) per (level, outer round) that ran; rms is the
    root mean square of r - field in log2 units (nan when no voxel counts).  report: a host array, or a device tensor: then this
    SYNCHRONISES."""
    if torch.is_tensor(report):
        report = report.cpu().numpy()
    rows = []
    for g, rnd, ran, changed, cst, n in np.asarray(report).reshape(-1, 6).tolist():
        if g < 0:
            break
        rows.append(dict(g=g, round=rnd, sweeps=ran, changed=changed, cost=cst, count=n,
                         rms=math.sqrt(cst / n) / 4096.0 if n else float("nan")))
    return rows


def cv(volume, labels, cls):
    """The coefficient of variation (standard deviation / mean, float64) of the voxels of `volume` whose label is `cls`; nan when there
    are none.  Host arrays, or device tensors: then this SYNCHRONISES."""
    if torch.is_tensor(volume):
        volume = volume.cpu().numpy()
    if torch.is_tensor(labels):
        labels = (labels.view(torch.int16) if labels.dtype == torch.uint16 else labels).cpu().numpy()
        labels = labels.view(np.uint16) if labels.dtype == np.int16 else labels
    v = np.asarray(volume, np.float64)[np.asarray(labels) == int(cls)]
    return float(v.std() / v.mean()) if v.size else float("nan")
