"""The geometry of a fitted lattice warp on the device (include/unet_deform.h): what `warp.fit` and `cowarp.fit` find pulls template
things onto the subject grid; this is the way back, and the report of what the field did to volume.

  jacobian         the determinant of the derivative of map + field at every subject voxel, with the count of folded voxels
                   (det <= 0, or NaN) and the exact extremes
  pull             a subject-grid volume (float32: trilinear; uint8 / uint16 labels: nearest) on the template grid through the inverse
                   of map + field, a fixed-point iteration of `iters` rounds per template voxel; optionally the dense inverse itself
  inverse_map      host arithmetic: the inverse of a 12-float map in float64, rounded once
  relative         host arithmetic: det / det(M) in float64, the local volume change of the field alone
  summary          host arithmetic: jacobian's info decoded
  Plan             what `register.parcellate(geometry=...)` and `coreg.align(geometry=...)` take

The mean volume change of a region needs no kernel of its own: `stats.moments(regions, det, n_labels, lo, hi)` and `stats.summary` of the
det map over a parcellation's regions gives count, mean and extremes per region; divide by det(M) (`relative`) for the field's share.

The field is either warp's: int32 {nz, ny, nx, 3} in 1/256 of a template voxel on `warp.lattice(subject_shape, g)`, g in (4, 8, 16,
32).  These are this project's definitions (parity with TIPL NOT pinned).  All arithmetic is fp32 with every operation rounded: the
results are pinned to the numpy restatement of tests/deform_ref.py bit for bit.  IMPL_GLOBAL gathers every lattice node from global
memory, IMPL_TILE stages a brick's lattice window in LDS; both give the same bits."""
import collections
import ctypes as C

import numpy as np
import torch

from . import engine as E
from . import register as R
from . import warp as W
from .engine import UNetError

_fp = C.POINTER(C.c_float)
E._sig("unet_deform_jacobian", C.c_int, C.c_int, C.c_int, C.c_int, _fp, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p)
E._sig("unet_deform_pull", C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _fp, _fp, C.c_void_p, C.c_int,
       C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p)
# every symbol include/unet_deform.h declares
EXPORTS = ["unet_deform_jacobian", "unet_deform_pull"]

IMPL_DEFAULT, IMPL_GLOBAL, IMPL_TILE = 0, 1, 2
KIND_F32, KIND_U8, KIND_U16 = 0, 1, 2
MAX_DISP, MAX_ITERS, MAX_WINDOW = 32767, 32, 1536
SPACINGS = (4, 8, 16, 32)
_KINDS = {torch.float32: KIND_F32, torch.uint8: KIND_U8, torch.uint16: KIND_U16}

Plan = collections.namedtuple("Plan", ("jacobian", "iters", "impl"), defaults=(True, 8, IMPL_DEFAULT))
Plan.__doc__ = ("The geometry of a fitted warp: whether the determinant map is formed after the fit, and the rounds and the impl that "
                "register.to_template pulls with.")


def _plan(plan, who):
    try:
        jac, iters, impl = bool(plan.jacobian), plan.iters, plan.impl
    except (AttributeError, TypeError):
        raise UNetError("%s: geometry must be a deform.Plan(jacobian, iters, impl)" % who)
    _iters(iters, who)
    return jac, int(iters), int(impl)


def _iters(iters, who):
    if isinstance(iters, bool) or not isinstance(iters, (int, np.integer)) or not 0 <= iters <= MAX_ITERS:
        raise UNetError("%s: iters must be an integer in [0, %d], got %r" % (who, MAX_ITERS, iters))


def _field(D, subject_shape, g, dev, who):
    """D on warp.lattice(subject_shape, g), g one of SPACINGS, and on `dev` unless None"""
    return W._lattice_field(D, subject_shape, W._g(g, SPACINGS, who), dev, who,
                            "device tensor" + ("" if dev is None else " on the volume's device"))


def jacobian(subject_shape, map, D, g, det=True, stream=None):
    """unet_deform_jacobian on the current stream (or the raw `stream`).  D: the field of warp.fit or cowarp.fit on
    warp.lattice(subject_shape, g).  Returns (det, info): det float32 of `subject_shape` on the device (written into `det` when a
    tensor is given, None when det is False), info int64 {4} on the device = voxels, folded voxels (det <= 0, or NaN), and the keys
    of the smallest and the largest det (`summary` decodes them).  No host synchronisation."""
    sw, sh, sd = W._dims(subject_shape, "jacobian")
    m = R._map12(map, "deform.jacobian")
    _field(D, (sd, sh, sw), g, None, "deform.jacobian")
    out = None
    if det is not False and det is not None:
        out = R._out(None if det is True else det, sw * sh * sd, torch.float32, D.device, "det", "jacobian", "deform")
    info = torch.empty(4, dtype=torch.int64, device=D.device)
    E.check(E.lib.unet_deform_jacobian(sw, sh, sd, R._floats(m), D.data_ptr(), int(g), out.data_ptr() if out is not None else None,
                                       info.data_ptr(), E.stream(D, stream)))
    return (out.view(sd, sh, sw) if out is not None else None), info


def pull(volume, template_shape, map, D, g, inv=None, iters=8, pos=False, impl=IMPL_DEFAULT, out=None, stream=None):
    """unet_deform_pull on the current stream (or the raw `stream`).  volume: a (D, H, W) device tensor on the subject grid, float32
    (sampled trilinearly, 0 outside) or uint8 / uint16 (the nearest voxel, 0 outside); D: the field on warp.lattice(volume.shape, g),
    or None for the affine inverse alone; inv: the inverse of `map` (inverse_map(map) when None; it is NOT checked against map).
    Returns (out, pos, info): out of `template_shape` in the volume's type, pos float32 {3, D, H, W} (the subject position of every
    template voxel; None unless `pos` is True or a tensor to write into), info int64 {2} on the device = template voxels whose
    position is inside the subject grid, and of those the ones not converged to 1/16 of a template voxel.  No host synchronisation."""
    if not (torch.is_tensor(volume) and volume.is_cuda and volume.dtype in _KINDS and volume.is_contiguous() and volume.dim() == 3
            and volume.numel() > 0):
        raise UNetError("deform.pull: volume must be a contiguous (D, H, W) float32, uint8 or uint16 device tensor")
    tw, th, td = W._dims(template_shape, "pull")
    m = R._map12(map, "deform.pull")
    iv = inverse_map(m) if inv is None else R._map12(inv, "deform.pull")
    _iters(iters, "deform.pull")
    sd, sh, sw = (int(v) for v in volume.shape)
    if D is not None:
        _field(D, volume.shape, g, volume.device, "deform.pull")
    res = R._out(out, tw * th * td, volume.dtype, volume.device, "out", "pull", "deform")
    p = None
    if pos is not False and pos is not None:
        p = R._out(None if pos is True else pos, 3 * tw * th * td, torch.float32, volume.device, "pos", "pull", "deform")
    info = torch.empty(2, dtype=torch.int64, device=volume.device)
    E.check(E.lib.unet_deform_pull(volume.data_ptr(), _KINDS[volume.dtype], sw, sh, sd, tw, th, td, R._floats(m), R._floats(iv),
                                   D.data_ptr() if D is not None else None, int(g), int(iters), res.data_ptr(),
                                   p.data_ptr() if p is not None else None, info.data_ptr(), int(impl), E.stream(volume, stream)))
    return res.view(td, th, tw), (p.view(3, td, th, tw) if p is not None else None), info


# ---- host arithmetic ---------------------------------------------------------------------------------------------------------------
def inverse_map(map):
    """float32 {12}: the inverse of a map (m[9], t[3]) or 12 numbers, computed in float64 and rounded once; a singular map raises."""
    m = R._map12(map, "deform.inverse_map").astype(np.float64)
    try:
        with np.errstate(all="ignore"):
            a = np.linalg.inv(m[:9].reshape(3, 3))
    except np.linalg.LinAlgError:
        raise UNetError("deform.inverse_map: the map is singular")
    if not np.isfinite(a).all():
        raise UNetError("deform.inverse_map: the map is singular or not finite")
    return np.ascontiguousarray(np.concatenate([a.reshape(9), -(a @ m[9:])]).astype(np.float32))


def relative(det, map):
    """det / det(M) in float64: the volume change of the field alone (1 where the field is locally a translation).  det: a host
    array, or a device tensor: then this SYNCHRONISES."""
    if torch.is_tensor(det):
        det = det.cpu().numpy()
    m = R._map12(map, "deform.relative").astype(np.float64)
    return np.asarray(det, np.float64) / float(np.linalg.det(m[:9].reshape(3, 3)))


def _unkey(k):
    k = int(k) & 0xFFFFFFFF
    b = k ^ (0x80000000 if k >> 31 else 0xFFFFFFFF)
    return float(np.array([b], np.uint32).view(np.float32)[0])


def summary(info):
    """jacobian's info decoded: dict(voxels, folded, det_min, det_max); the extremes are NaN when no det entered them.  info: a host
    array, or a device tensor: then this SYNCHRONISES."""
    if torch.is_tensor(info):
        info = info.cpu().numpy()
    v = [int(x) for x in np.asarray(info).reshape(4)]
    none = v[2] == 0xFFFFFFFF and v[3] == 0
    return dict(voxels=v[0], folded=v[1], det_min=float("nan") if none else _unkey(v[2]), det_max=float("nan") if none else _unkey(v[3]))
