"""The non-linear refinement of a co-registration on the device (include/unet_cowarp.h): after `coreg.search` has found the affine
map, a displacement field on a lattice over the fixed grid is moved node by node towards a larger mutual information of the two code
images, coarse to fine, and the moving image is resampled through map + field.  It is to `coreg` what `warp` is to `register`.

  hist             the joint code histogram {bins, bins + 1} under the warped positions
  weights          a histogram's point-wise mutual-information terms as an int16 table W {bins, bins + 1}
  sweep            one sweep: hist, weights, then 8 colour passes in which every node of a colour tries its six unit moves of `step`
                   and keeps the one with the largest sum of W over its support
  fit              the whole schedule, enqueued at once: levels of (g, first_step, last_step, max_sweeps[, limit])
  resample         a float32 moving volume on the fixed grid through map + field, trilinear
  Plan             what `coreg.align(warp=...)` takes
  score            host arithmetic on a histogram: N times the mutual information in units of 2^-16 bit

The field is int32 {nz, ny, nx, 3} in 1/256 of a MOVING voxel on `warp.lattice(fixed.shape, g)`, g in (4, 8, 16); it is a valid
argument of `warp.refine` and `warp.displacement_mm`.  These are this project's definitions (parity with TIPL's non-linear stage NOT
pinned).  Every choice is made on integers: the results are pinned to the numpy restatement of tests/cowarp_ref.py bit for bit.
IMPL_NODE runs a block per lattice node, IMPL_VOXEL a thread per voxel with atomic counters per node (the measured baseline and a
second witness of the bits)."""
import collections
import ctypes as C

import numpy as np
import torch

from . import coreg as CR
from . import engine as E
from . import register as R
from . import warp as W
from .engine import UNetError

_grid = (C.c_void_p, C.c_int, C.c_int, C.c_int)   # codes, w, h, d
_fp = C.POINTER(C.c_float)
_ip = C.POINTER(C.c_int)
E._sig("unet_cowarp_scratch_bytes", C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _ip, C.c_int, C.POINTER(C.c_size_t))
E._sig("unet_cowarp_hist", C.c_int, *_grid, *_grid, C.c_int, _fp, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p)
E._sig("unet_cowarp_weights", C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p)
E._sig("unet_cowarp_sweep", C.c_int, *_grid, *_grid, C.c_int, _fp, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
       C.c_size_t, C.c_void_p)
E._sig("unet_cowarp_fit", C.c_int, *_grid, *_grid, C.c_int, _fp, _ip, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t,
       C.c_void_p)
E._sig("unet_cowarp_resample", C.c_int, *_grid, C.c_int, C.c_int, C.c_int, _fp, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p)
# every symbol include/unet_cowarp.h declares
EXPORTS = ["unet_cowarp_scratch_bytes", "unet_cowarp_hist", "unet_cowarp_weights", "unet_cowarp_sweep", "unet_cowarp_fit",
           "unet_cowarp_resample"]

IMPL_DEFAULT, IMPL_NODE, IMPL_VOXEL = 0, 1, 2
MAX_BINS, MAX_DISP, MAX_STEP, MAX_LEVELS, MAX_SWEEPS, MAX_ROWS, MAX_SUPPORT, MAX_WEIGHT = 32, 32767, 16384, 3, 16, 32, 29791, 8192
SPACINGS = (4, 8, 16)

Plan = collections.namedtuple("Plan", ("levels", "limit", "impl"), defaults=(None, None, IMPL_DEFAULT))
Plan.__doc__ = ("How a co-registration is refined: the levels (g, first_step, last_step, max_sweeps[, limit]) of cowarp.fit (None: "
                "warp.DEFAULT_LEVELS), the limit on the difference of neighbouring nodes (Q8; None: warp.default_limit per level) and "
                "the impl.")


def _plan(plan, who):
    try:
        levels, limit, impl = plan.levels, plan.limit, plan.impl
        levels = list(W.DEFAULT_LEVELS if levels is None else levels)
    except (AttributeError, TypeError):
        raise UNetError("%s: warp must be a cowarp.Plan(levels, limit, impl)" % who)
    return W._plan_rows(levels, limit, who) + (int(impl),)


def _codes(t, name, who, dev=None):
    if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous() and t.dim() == 3 and t.numel() > 0
            and (dev is None or t.device == dev)):
        raise UNetError("cowarp.%s: %s must be a contiguous (D, H, W) uint8 device tensor of codes%s"
                        % (who, name, "" if dev is None else " on the fixed image's device"))
    d, h, w = (int(v) for v in t.shape)
    return (t.data_ptr(), w, h, d)


def _bins(bins, who):
    if isinstance(bins, bool) or bins not in CR.BINS:
        raise UNetError("cowarp.%s: bins must be 8, 16 or 32, got %r" % (who, bins))
    return int(bins)


def _field(D, fixed_shape, g, dev, who):
    """D on warp.lattice(fixed_shape, g), g one of SPACINGS, on `dev`"""
    return W._lattice_field(D, fixed_shape, W._g(g, SPACINGS, who), dev, who, "tensor on the fixed image's device")


def scratch_bytes(fixed_shape, bins, levels):
    """The scratch of a fit of `levels` (int {n, 5}); a sweep at g takes that of [(g, 1, 1, 1, 0)]."""
    lv = np.ascontiguousarray(np.asarray(levels, np.int32).reshape(-1, 5))
    return E.size_query(E.lib.unet_cowarp_scratch_bytes, *W._dims(fixed_shape, "scratch_bytes"), int(bins), lv.ctypes.data_as(_ip),
                        int(lv.shape[0]))


def hist(fixed, moving, bins, map, D, g, out=None, stream=None):
    """unet_cowarp_hist on the current stream (or the raw `stream`).  fixed, moving: (D, H, W) uint8 device tensors of codes.  Returns
    uint32 {bins, bins + 1} on the device (written into `out` when given): every fixed voxel with a code, counted at its warped
    position; the last column counts the samples outside the moving grid or without a code.  No host synchronisation."""
    fg = _codes(fixed, "fixed", "hist")
    mg = _codes(moving, "moving", "hist", fixed.device)
    b = _bins(bins, "hist")
    m = R._map12(map, "cowarp.hist")
    _field(D, fixed.shape, g, fixed.device, "cowarp.hist")
    h = R._out(out, b * (b + 1), torch.uint32, fixed.device, "out", "hist", "cowarp")
    E.check(E.lib.unet_cowarp_hist(*fg, *mg, b, R._floats(m), D.data_ptr(), int(g), h.data_ptr(), E.stream(fixed, stream)))
    return h.view(b, b + 1)


def weights(hist, out=None, stream=None):
    """unet_cowarp_weights on the current stream (or the raw `stream`).  hist: uint32 {bins, bins + 1} on the device.  Returns int16
    {bins, bins + 1} on the device (written into `out` when given): (L(n_ab) + L(N) - L(r_a) - L(c_b)) >> 8 inside, the row's
    minimum (at most 0) in the last column.  No host synchronisation."""
    if not (torch.is_tensor(hist) and hist.is_cuda and hist.dtype == torch.uint32 and hist.is_contiguous() and hist.dim() == 2
            and hist.shape[0] in CR.BINS and hist.shape[1] == hist.shape[0] + 1):
        raise UNetError("cowarp.weights: hist must be a contiguous uint32 {bins, bins + 1} device tensor")
    b = int(hist.shape[0])
    w = R._out(out, b * (b + 1), torch.int16, hist.device, "out", "weights", "cowarp")
    E.check(E.lib.unet_cowarp_weights(hist.data_ptr(), b, w.data_ptr(), E.stream(hist, stream)))
    return w.view(b, b + 1)


def sweep(fixed, moving, bins, map, D, g, step, limit, impl=IMPL_DEFAULT, scratch=None, stream=None):
    """unet_cowarp_sweep on the current stream (or the raw `stream`): one sweep over D IN PLACE.  Returns info int64 {2} on the
    device: nodes changed, nodes visited.  No host synchronisation."""
    fg = _codes(fixed, "fixed", "sweep")
    mg = _codes(moving, "moving", "sweep", fixed.device)
    b = _bins(bins, "sweep")
    m = R._map12(map, "cowarp.sweep")
    _field(D, fixed.shape, g, fixed.device, "cowarp.sweep")
    need = scratch_bytes(tuple(fixed.shape), b, [(int(g), 1, 1, 1, 0)])
    scratch = E.scratch(scratch, need, fixed.device)
    info = torch.empty(2, dtype=torch.int64, device=fixed.device)
    E.check(E.lib.unet_cowarp_sweep(*fg, *mg, b, R._floats(m), D.data_ptr(), int(g), int(step), int(limit), info.data_ptr(), int(impl),
                                    scratch.data_ptr(), scratch.nbytes, E.stream(fixed, stream)))
    return info


def fit(fixed, moving, bins, map, levels=None, limit=None, impl=IMPL_DEFAULT, scratch=None, stream=None):
    """unet_cowarp_fit on the current stream (or the raw `stream`): the field from zero through every level (None:
    warp.DEFAULT_LEVELS; a row without a limit gets `limit`, or warp.default_limit of its g).  Returns device tensors: D int32
    {nz, ny, nx, 3} on the LAST level's lattice and report int64 {MAX_ROWS, 5}: per (level, step) g, step, sweeps run, nodes changed
    in the last sweep run, N * MI after it; -1 past the schedule.  Every launch is enqueued here; no host synchronisation."""
    fg = _codes(fixed, "fixed", "fit")
    mg = _codes(moving, "moving", "fit", fixed.device)
    b = _bins(bins, "fit")
    m = R._map12(map, "cowarp.fit")
    lv = W.levels_of(W.DEFAULT_LEVELS if levels is None else levels, limit, m, "cowarp.fit")
    need = scratch_bytes(tuple(fixed.shape), b, lv)                 # the range checks, before any device work
    scratch = E.scratch(scratch, need, fixed.device)
    D = torch.empty(W.lattice(tuple(fixed.shape), int(lv[-1, 0])) + (3,), dtype=torch.int32, device=fixed.device)
    report = torch.empty((MAX_ROWS, 5), dtype=torch.int64, device=fixed.device)
    E.check(E.lib.unet_cowarp_fit(*fg, *mg, b, R._floats(m), lv.ctypes.data_as(_ip), int(lv.shape[0]), D.data_ptr(), report.data_ptr(),
                                  int(impl), scratch.data_ptr(), scratch.nbytes, E.stream(fixed, stream)))
    return D, report


def resample(moving, fixed_shape, map, D, g, out=None, stream=None):
    """unet_cowarp_resample on the current stream (or the raw `stream`).  moving: a (D, H, W) float32 device tensor; returns float32
    of `fixed_shape` on the device (written into `out` when given): the moving volume at map + field, trilinear, 0 outside.  With a
    zero field it is space.resample(mode="linear") bit for bit.  No host synchronisation."""
    if not (torch.is_tensor(moving) and moving.is_cuda and moving.dtype == torch.float32 and moving.is_contiguous() and moving.dim() == 3
            and moving.numel() > 0):
        raise UNetError("cowarp.resample: moving must be a contiguous (D, H, W) float32 device tensor")
    fw, fh, fd = W._dims(fixed_shape, "resample")
    m = R._map12(map, "cowarp.resample")
    _field(D, (fd, fh, fw), g, moving.device, "cowarp.resample")
    md, mh, mw = (int(v) for v in moving.shape)
    res = R._out(out, fw * fh * fd, torch.float32, moving.device, "out", "resample", "cowarp")
    E.check(E.lib.unet_cowarp_resample(moving.data_ptr(), mw, mh, md, fw, fh, fd, R._floats(m), D.data_ptr(), int(g), res.data_ptr(),
                                       E.stream(moving, stream)))
    return res.view(fd, fh, fw)


# ---- host arithmetic ---------------------------------------------------------------------------------------------------------------
def _ilog(n):
    """L(n) of include/unet_coreg.h in Python integers"""
    n = int(n)
    if n == 0:
        return 0
    e = n.bit_length() - 1
    x, f = (n << (31 - e)) & 0xFFFFFFFF, 0
    for _ in range(16):
        y = (x * x) >> 31
        f, x = (2 * f + 1, y >> 1) if y >> 32 else (2 * f, y)
    return (e << 16) | f


def score(hist):
    """N * MI of a {bins, bins + 1} joint histogram in units of 2^-16 bit (the Score of include/unet_coreg.h), a Python int; hist: a
    host array, or a device tensor: then this SYNCHRONISES."""
    if torch.is_tensor(hist):
        hist = hist.cpu().numpy()
    h = [[int(v) for v in row] for row in np.asarray(hist)]
    bins = len(h)
    if any(len(row) != bins + 1 for row in h):
        raise UNetError("cowarp.score: hist must be {bins, bins + 1}")
    r = [sum(row) & 0xFFFFFFFF for row in h]
    c = [sum(h[a][b] for a in range(bins)) & 0xFFFFFFFF for b in range(bins)]
    ln = _ilog(sum(r) & 0xFFFFFFFF)
    return sum(h[a][b] * (_ilog(h[a][b]) + ln - _ilog(r[a]) - _ilog(c[b])) for a in range(bins) for b in range(bins) if h[a][b])
