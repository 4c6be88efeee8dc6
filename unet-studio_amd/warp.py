"""The non-linear refinement of a parcellation on the device (include/unet_warp.h): after `register.search` has found the affine map,
a displacement field on a lattice over the subject grid is moved node by node towards a better agreement of the two tissue maps,
coarse to fine, and the atlas is carried through the warped map.

  lattice          the nodes of a lattice of spacing g over a subject grid
  hist             the joint tissue histogram under the warped positions
  sweep            one sweep: 8 colour passes, every node of a colour tries its six unit moves of `step` and keeps the best
  refine           a field on the lattice of spacing g brought onto that of g / 2
  fit              the whole schedule, enqueued at once: levels of (g, first_step, last_step, max_sweeps[, limit])
  carry            register.carry at the warped positions
  Plan             what `register.parcellate(warp=...)` and `EvaluateUNet(atlas_warp=...)` take
  score, dice, displacement_mm    host arithmetic on a histogram and on a field

The field is int32 {nz, ny, nx, 3} in 1/256 of a TEMPLATE voxel.  These are this project's definitions (parity with TIPL's
non-linear stage NOT pinned).  Every choice is made on integer counts: the results are pinned to the numpy restatement of
tests/warp_ref.py bit for bit.  IMPL_NODE runs a block per lattice node, IMPL_VOXEL a thread per voxel with atomic counters per node
(the measured baseline and a second witness of the bits)."""
import collections
import ctypes as C
import math

import numpy as np
import torch

from . import engine as E
from . import register as R
from .engine import UNetError

_grid = (C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int)   # tissue, bytes, w, h, d
_fp = C.POINTER(C.c_float)
_ip = C.POINTER(C.c_int)
E._sig("unet_warp_lattice", C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _ip, _ip, _ip)
E._sig("unet_warp_scratch_bytes", C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _ip, C.c_int, C.POINTER(C.c_size_t))
E._sig("unet_warp_hist", C.c_int, *_grid, *_grid, C.c_int, _fp, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p)
E._sig("unet_warp_sweep", C.c_int, *_grid, *_grid, C.c_int, _fp, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
       C.c_size_t, C.c_void_p)
E._sig("unet_warp_refine", C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p)
E._sig("unet_warp_fit", C.c_int, *_grid, *_grid, C.c_int, _fp, _ip, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t,
       C.c_void_p)
E._sig("unet_warp_carry", C.c_int, *_grid, *_grid, C.c_void_p, C.c_int, _fp, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p)
# every symbol include/unet_warp.h declares
EXPORTS = ["unet_warp_lattice", "unet_warp_scratch_bytes", "unet_warp_hist", "unet_warp_sweep", "unet_warp_refine", "unet_warp_fit",
           "unet_warp_carry"]

IMPL_DEFAULT, IMPL_NODE, IMPL_VOXEL = 0, 1, 2
MAX_TISSUES, MAX_DISP, MAX_STEP, MAX_LEVELS, MAX_SWEEPS, MAX_ROWS = 16, 32767, 16384, 4, 16, 32
DEFAULT_LEVELS = [(16, 512, 128, 6), (8, 256, 64, 6), (4, 128, 64, 6)]     # (g, first_step, last_step, max_sweeps)

Plan = collections.namedtuple("Plan", ("levels", "limit"), defaults=(DEFAULT_LEVELS, None))
Plan.__doc__ = ("How a parcellation is refined: the levels (g, first_step, last_step, max_sweeps[, limit]) of warp.fit and the limit "
                "on the difference of neighbouring nodes (Q8; None: a quarter of the node spacing as the affine map sees it).")


def _dims(shape, who):
    try:
        d, h, w = (int(v) for v in shape)
    except (TypeError, ValueError):
        raise UNetError("warp.%s: a subject shape is (D, H, W)" % who)
    return w, h, d


def lattice(subject_shape, g):
    """(nz, ny, nx), the nodes of the lattice of spacing g over a subject grid (D, H, W): (dim + g - 1) // g + 1 per axis."""
    n = [C.c_int() for _ in range(3)]
    E.check(E.lib.unet_warp_lattice(*_dims(subject_shape, "lattice"), int(g), *(C.byref(v) for v in n)))
    return n[2].value, n[1].value, n[0].value


def default_limit(map, g):
    """floor(64 * g * s), s the smallest column norm of the map's matrix (float64), floored at 1 / 4: a quarter of the node spacing
    in template voxels, in Q8."""
    m = R._map12(map, "default_limit")[:9].astype(np.float64).reshape(3, 3)
    s = float(np.sqrt((m * m).sum(0)).min())
    if not math.isfinite(s):
        raise UNetError("warp.default_limit: the map's matrix must be finite")
    return int(math.floor(64.0 * int(g) * max(s, 0.25)))


def levels_of(levels, limit, map, who="warp.fit"):
    """int32 {n, 5}: rows of (g, first_step, last_step, max_sweeps) get `limit` (default_limit per level when None) appended."""
    rows = []
    try:
        for lv in levels:
            lv = [int(v) for v in lv]
            if len(lv) == 4:
                lv.append(default_limit(map, lv[0]) if limit is None else int(limit))
            if len(lv) != 5:
                raise ValueError
            rows.append(lv)
    except (TypeError, ValueError):
        raise UNetError("%s: levels must be rows of (g, first_step, last_step, max_sweeps[, limit]) integers" % who)
    if not rows:
        raise UNetError("%s: levels must not be empty" % who)
    return np.ascontiguousarray(np.asarray(rows, np.int32).reshape(-1, 5))


def _plan_rows(levels, limit, who):
    """(levels, limit) of a warp.Plan or a cowarp.Plan, checked"""
    if limit is not None and (isinstance(limit, bool) or int(limit) != limit or limit < 0):
        raise UNetError("%s: warp.limit must be a non-negative integer or None, got %r" % (who, limit))
    levels_of(levels, 0, None, who)                                 # the rows' form; the ranges are the library's to check
    return levels, limit


def _plan(plan, who):
    try:
        levels, limit = list(plan.levels), plan.limit
    except (AttributeError, TypeError):
        raise UNetError("%s: warp must be a warp.Plan(levels, limit)" % who)
    return _plan_rows(levels, limit, who)


def scratch_bytes(subject_shape, n_tissues, levels):
    """The scratch of a fit of `levels` (int {n, 5}); a sweep at g takes that of [(g, 1, 1, 1, 0)]."""
    lv = np.ascontiguousarray(np.asarray(levels, np.int32).reshape(-1, 5))
    return E.size_query(E.lib.unet_warp_scratch_bytes, *_dims(subject_shape, "scratch_bytes"), int(n_tissues), lv.ctypes.data_as(_ip),
                        int(lv.shape[0]))


def _g(g, spacings, who):
    """a lattice spacing of cowarp or deform (`who`: "module.function"); warp's own is the library's to check"""
    if isinstance(g, bool) or g not in spacings:
        raise UNetError("%s: g must be %s or %d, got %r" % (who, ", ".join(str(v) for v in spacings[:-1]), spacings[-1], g))
    return int(g)


def _lattice_field(D, shape, g, dev, who, where):
    """D on lattice(shape, g), and on `dev` unless None; `where`: the words of the message behind the shape"""
    want = lattice(tuple(shape), g) + (3,)
    if not (torch.is_tensor(D) and D.is_cuda and (dev is None or D.device == dev) and D.dtype == torch.int32 and D.is_contiguous()
            and tuple(D.shape) == want):
        raise UNetError("%s: D must be a contiguous int32 %s %s" % (who, list(want), where))
    return D


def _field(D, subject, g, who):
    try:
        lattice(tuple(subject.shape), g)
    except UNetError as e:
        raise UNetError("warp.%s: %s" % (who, e))
    return _lattice_field(D, subject.shape, g, subject.device, "warp." + who, "tensor on the subject's device")


def _tissues(subject, template, n_tissues, who):
    sg = R._tissue(subject, "subject", who)
    tg = R._tissue(template, "template", who, subject.device)
    T = int(n_tissues)
    if not 2 <= T <= MAX_TISSUES:
        raise UNetError("warp.%s: n_tissues must be in [2, %d], got %d" % (who, MAX_TISSUES, T))
    return sg, tg, T


def hist(subject, template, n_tissues, map, D, g, out=None, stream=None):
    """unet_warp_hist on the current stream (or the raw `stream`): uint32 {T, T} on the device (written into `out` when given), every
    subject voxel counted at its warped position.  No host synchronisation."""
    sg, tg, T = _tissues(subject, template, n_tissues, "hist")
    m = R._map12(map, "hist")
    _field(D, subject, g, "hist")
    h = R._out(out, T * T, torch.uint32, subject.device, "out", "hist")
    E.check(E.lib.unet_warp_hist(*sg, *tg, T, R._floats(m), D.data_ptr(), int(g), h.data_ptr(), E.stream(subject, stream)))
    return h.view(T, T)


def sweep(subject, template, n_tissues, map, D, g, step, limit, impl=IMPL_DEFAULT, scratch=None, stream=None):
    """unet_warp_sweep on the current stream (or the raw `stream`): one sweep over D IN PLACE.  Returns info int64 {2} on the device:
    nodes changed, nodes visited.  No host synchronisation."""
    sg, tg, T = _tissues(subject, template, n_tissues, "sweep")
    m = R._map12(map, "sweep")
    _field(D, subject, g, "sweep")
    need = scratch_bytes(tuple(subject.shape), T, [(int(g), 1, 1, 1, 0)])
    scratch = E.scratch(scratch, need, subject.device)
    info = torch.empty(2, dtype=torch.int64, device=subject.device)
    E.check(E.lib.unet_warp_sweep(*sg, *tg, T, R._floats(m), D.data_ptr(), int(g), int(step), int(limit), info.data_ptr(), int(impl),
                                  scratch.data_ptr(), scratch.nbytes, E.stream(subject, stream)))
    return info


def refine(D, subject_shape, g, out=None, stream=None):
    """unet_warp_refine on the current stream (or the raw `stream`): D on the lattice of spacing g over the subject grid (D, H, W) ->
    the field on the lattice of g // 2, each fine node the rounded mean of the coarse nodes around it.  No host synchronisation."""
    w, h, d = _dims(subject_shape, "refine")
    if g not in (8, 16, 32):
        raise UNetError("warp.refine: g must be 8, 16 or 32, got %r" % (g,))
    coarse, fine = lattice((d, h, w), g) + (3,), lattice((d, h, w), g // 2) + (3,)
    if not (torch.is_tensor(D) and D.is_cuda and D.dtype == torch.int32 and D.is_contiguous() and tuple(D.shape) == coarse):
        raise UNetError("warp.refine: D must be a contiguous int32 %s device tensor" % list(coarse))
    out = R._out(out, int(np.prod(fine)), torch.int32, D.device, "out", "refine")
    E.check(E.lib.unet_warp_refine(D.data_ptr(), w, h, d, int(g), out.data_ptr(), E.stream(D, stream)))
    return out.view(fine)


def fit(subject, template, n_tissues, map, levels=DEFAULT_LEVELS, limit=None, impl=IMPL_DEFAULT, scratch=None, stream=None):
    """unet_warp_fit on the current stream (or the raw `stream`): the field from zero through every level.  Returns device tensors: D
    int32 {nz, ny, nx, 3} on the LAST level's lattice and report int64 {MAX_ROWS, 5}: per (level, step) g, step, sweeps run, nodes
    changed in the last sweep run, score after it; -1 past the schedule.  Every launch is enqueued here; no host synchronisation."""
    sg, tg, T = _tissues(subject, template, n_tissues, "fit")
    m = R._map12(map, "fit")
    lv = levels_of(levels, limit, m)
    need = scratch_bytes(tuple(subject.shape), T, lv)                # the range checks, before any device work
    scratch = E.scratch(scratch, need, subject.device)
    D = torch.empty(lattice(tuple(subject.shape), int(lv[-1, 0])) + (3,), dtype=torch.int32, device=subject.device)
    report = torch.empty((MAX_ROWS, 5), dtype=torch.int64, device=subject.device)
    E.check(E.lib.unet_warp_fit(*sg, *tg, T, R._floats(m), lv.ctypes.data_as(_ip), int(lv.shape[0]), D.data_ptr(), report.data_ptr(),
                                int(impl), scratch.data_ptr(), scratch.nbytes, E.stream(subject, stream)))
    return D, report


def carry(subject, template, atlas, n_tissues, map, D, g, counts=True, out=None, stream=None):
    """unet_warp_carry on the current stream (or the raw `stream`): register.carry's rules at the warped positions.  Returns (regions
    uint16 on the subject grid, counts uint32 {3, n_tissues} = direct, rescued, left per tissue, or None).  No host synchronisation."""
    sg, tg, T = _tissues(subject, template, n_tissues, "carry")
    if not (torch.is_tensor(atlas) and atlas.is_cuda and atlas.device == subject.device and atlas.dtype == torch.uint16 and atlas.is_contiguous()
            and atlas.numel() == template.numel()):
        raise UNetError("warp.carry: atlas must be a contiguous uint16 device tensor on the template grid")
    m = R._map12(map, "carry")
    _field(D, subject, g, "carry")
    regions = R._out(out, subject.numel(), torch.uint16, subject.device, "out", "carry")
    cnt = torch.empty(3 * T, dtype=torch.uint32, device=subject.device) if counts else None
    E.check(E.lib.unet_warp_carry(*sg, *tg, atlas.data_ptr(), T, R._floats(m), D.data_ptr(), int(g), regions.data_ptr(),
                                  cnt.data_ptr() if counts else None, E.stream(subject, stream)))
    return regions.view(subject.shape), (cnt.view(3, T) if counts else None)


# ---- host arithmetic ---------------------------------------------------------------------------------------------------------------
def score(hist):
    """agree - disagree of a {T, T} joint histogram: agree = the diagonal without [0][0], disagree = the rest."""
    h = np.asarray(hist).astype(np.int64)
    diag = int(np.trace(h))
    return (diag - int(h[0, 0])) - (int(h.sum()) - diag)


def dice(hist):
    """2 * agree / (subject foreground + sampled template foreground) of a {T, T} joint histogram; nan when both are empty."""
    h = np.asarray(hist).astype(np.int64)
    both = int(h[1:].sum()) + int(h[:, 1:].sum())
    return 2.0 * (int(np.trace(h)) - int(h[0, 0])) / both if both else float("nan")


def displacement_mm(D, template_vs):
    """(maximum, mean) length in mm of the nodes' displacements: D {nz, ny, nx, 3} in Q8 template voxels (a host array, or a device
    tensor: then this SYNCHRONISES), template_vs the template's voxel size (x, y, z)."""
    if torch.is_tensor(D):
        D = D.cpu().numpy()
    vs = np.asarray([float(v) for v in template_vs], np.float64).reshape(3)
    mm = np.sqrt(((np.asarray(D).astype(np.float64).reshape(-1, 3) / 256.0 * vs) ** 2).sum(1))
    return float(mm.max()), float(mm.mean())
