"""Connected components with a chosen connectivity on the device (include/unet_connectivity.h): the keep-largest call of
components.py, the instance labelling of instances.py and the hole filling of morph.py with `connectivity` 6, 18 or 26 (face; face
and edge; face, edge and corner neighbours).

  keep_largest   every listed class keeps its largest c-connected component
  label          every c-connected component of the listed classes gets a dense id and a row
  fill_holes     the c-connected components of the complement that touch no face of the volume are set: `connectivity` is the
                 background's, 26 the strict one (scipy.ndimage.binary_fill_holes with generate_binary_structure(3, 3))

With connectivity 6 each call writes exactly the bytes of its sibling.  The public callers (components.keep_largest,
instances.label / lesion_scores, qc.lesion_qc, morph.fill_holes / fill_holes_label / run, postproc.run_postproc, EvaluateUNet) take
a keyword that defaults to 6 and come here for 18 and 26.  These are this project's definitions (parity NOT pinned); every device
value is an integer, pinned bit for bit to scipy.ndimage.label with a structure (tests/test_connectivity_host.py).  No function
here synchronises with the host.  Out of scope: the defragment command of the post-processing chain, the surface definition of
distance.py, the C++ host."""
import ctypes as C

import torch

from . import engine as E
from .engine import UNetError

_I, _P = C.c_int, C.c_void_p
E._sig("unet_conn_scratch_bytes", _I, C.c_int64, _I, C.POINTER(C.c_size_t))
E._sig("unet_conn_keep_largest", _I, _I, _I, _I, _P, _I, C.POINTER(C.c_uint32), _I, _P, _I, _I, _P, C.c_size_t, _P)
E._sig("unet_conn_label_scratch_bytes", _I, C.c_int64, _I, C.c_int64, C.POINTER(C.c_size_t))
E._sig("unet_conn_label", _I, _I, _I, _I, _P, _I, C.POINTER(C.c_uint32), _I, _P, _P, C.c_int64, _P, _I, _I, _P, C.c_size_t, _P)
E._sig("unet_conn_holes_scratch_bytes", _I, _I, _I, _I, C.POINTER(C.c_size_t))
E._sig("unet_conn_holes", _I, _I, _I, _I, _P, _P, _P, _I, _I, _P, C.c_size_t, _P)
# every symbol include/unet_connectivity.h declares
EXPORTS = ["unet_conn_scratch_bytes", "unet_conn_keep_largest", "unet_conn_label_scratch_bytes", "unet_conn_label",
           "unet_conn_holes_scratch_bytes", "unet_conn_holes"]

IMPL_DEFAULT, IMPL_TILED, IMPL_GLOBAL = 0, 1, 2      # UNET_CONN_IMPL_*
CONN_6, CONN_18, CONN_26 = 6, 18, 26                 # UNET_CONN_6 / _18 / _26
CONNECTIVITIES = (CONN_6, CONN_18, CONN_26)
COLUMNS = 12                                         # the columns of a row of `label`, as in instances.py
DEFAULT_MAX_INSTANCES = 65535


def check(connectivity, who="connectivity"):
    """6, 18 or 26 as an int; anything else raises UNetError naming the value.  Host only."""
    if isinstance(connectivity, bool) or not isinstance(connectivity, int) or connectivity not in CONNECTIVITIES:
        raise UNetError("%s: connectivity must be 6, 18 or 26, got %r" % (who, connectivity))
    return int(connectivity)


def backward_offsets(connectivity):
    """N-(c): the (dx, dy, dz) of the neighbourhood whose neighbour has the smaller linear index, 3, 9 or 13 of them: what a voxel
    hooks to in the kernels (cc_for_backward in csrc/cc_union_find.h)"""
    reach = {6: 1, 18: 2, 26: 3}[check(connectivity)]
    return [(dx, dy, dz) for dz in (-1, 0) for dy in (-1, 0, 1) for dx in (-1, 0, 1)
            if 1 <= abs(dx) + abs(dy) + abs(dz) <= reach and (dz, dy, dx) < (0, 0, 0)]


def keep_largest_scratch_bytes(voxels, n_classes):
    n = C.c_size_t()
    E.check(E.lib.unet_conn_scratch_bytes(int(voxels), int(n_classes), C.byref(n)))
    return n.value


def label_scratch_bytes(voxels, n_classes, max_instances):
    n = C.c_size_t()
    E.check(E.lib.unet_conn_label_scratch_bytes(int(voxels), int(n_classes), int(max_instances), C.byref(n)))
    return n.value


def holes_scratch_bytes(shape):
    """unet_conn_holes_scratch_bytes for a (D, H, W) grid"""
    D, H, W = (int(v) for v in shape)
    n = C.c_size_t()
    E.check(E.lib.unet_conn_holes_scratch_bytes(W, H, D, C.byref(n)))
    return n.value


def keep_largest_args(who, label, classes, n_classes, removed, scratch_bytes):
    """keep_largest's argument checks, here and in components.py, under the message prefix `who`: ((D, H, W), classes, the scratch
    bytes needed)"""
    if not (torch.is_tensor(label) and label.is_cuda and label.dtype == torch.uint16 and label.is_contiguous() and label.dim() == 3):
        raise UNetError("%s: label must be a contiguous uint16 (D, H, W) device tensor" % who)
    D, H, W = (int(v) for v in label.shape)
    if removed is not None and not (torch.is_tensor(removed) and removed.is_cuda and removed.device == label.device
                                    and removed.dtype in (torch.uint32, torch.int32) and removed.is_contiguous()
                                    and removed.numel() == int(n_classes)):
        raise UNetError("%s: removed must be a contiguous uint32 device tensor of n_classes entries on label's device" % who)
    classes = [int(v) for v in classes]
    need = scratch_bytes(D * H * W, n_classes)                   # the size checks, before any device work
    for v in classes:
        if not 0 <= v < 1 << 32:
            raise UNetError("%s: listed class %d is not in [1, %d]" % (who, v, int(n_classes) - 1))
    return (D, H, W), classes, need


def keep_largest(label, classes, n_classes, connectivity=6, removed=None, scratch=None, impl=IMPL_DEFAULT, stream=None):
    """unet_conn_keep_largest in place on label, a (D, H, W) uint16 device tensor, on the current stream (or the raw `stream`);
    returns label.  Arguments as components.keep_largest: every listed class keeps its largest `connectivity`-connected component,
    the one holding the smallest linear index among equal counts."""
    c = check(connectivity, "connectivity.keep_largest")
    (D, H, W), classes, need = keep_largest_args("connectivity.keep_largest", label, classes, n_classes, removed, keep_largest_scratch_bytes)
    scratch = E.scratch(scratch, need, label.device)
    arr = (C.c_uint32 * max(1, len(classes)))(*classes)
    E.check(E.lib.unet_conn_keep_largest(W, H, D, label.data_ptr(), int(n_classes), arr, len(classes),
                                         removed.data_ptr() if removed is not None else None, c, int(impl), scratch.data_ptr(), scratch.nbytes,
                                         E.stream(label, stream)))
    return label


def label(labels, n_classes, classes=None, connectivity=6, max_instances=DEFAULT_MAX_INSTANCES, impl=IMPL_DEFAULT, scratch=None, out=None,
          stream=None):
    """unet_conn_label on the current stream (or the raw `stream`): (inst, rows, info) on the device exactly as instances.label
    returns them, for the `connectivity`-connected components of the listed classes.  No host synchronisation."""
    from . import instances as INS                      # its checks of the arguments; instances imports this module
    c = check(connectivity, "connectivity.label")
    lab = INS._label_map(labels, "label")
    D, H, W = (int(v) for v in lab.shape)
    nc, M = int(n_classes), int(max_instances)
    need = label_scratch_bytes(D * H * W, nc, M)                    # the range checks, before any device work
    classes = list(range(1, nc)) if classes is None else [int(v) for v in classes]
    for v in classes:
        if not 0 <= v < 1 << 32:
            raise UNetError("connectivity.label: listed class %d is not in [1, %d]" % (v, nc - 1))
    dev = lab.device
    o = out if out is not None else (None, None, None)
    inst = INS._out(o[0], D * H * W, torch.int32, dev, "label", "inst")
    rows = INS._out(o[1], (M + 1) * COLUMNS, torch.int64, dev, "label", "rows")
    info = INS._out(o[2], 2, torch.int64, dev, "label", "info")
    scratch = E.scratch(scratch, need, dev)
    arr = (C.c_uint32 * max(1, len(classes)))(*classes)
    E.check(E.lib.unet_conn_label(W, H, D, lab.data_ptr(), nc, arr, len(classes), inst.data_ptr(), rows.data_ptr(), M, info.data_ptr(), c,
                                  int(impl), scratch.data_ptr(), scratch.nbytes, E.stream(lab, stream)))
    return inst.view(D, H, W), rows.view(M + 1, COLUMNS), info


def fill_holes(m, connectivity=6, impl=IMPL_DEFAULT, scratch=None, out=None):
    """unet_conn_holes on a morph.Mask: (Mask, info); info a device int64[2] tensor: the voxels filled, the holes.  connectivity is
    the background's.  out may be m"""
    from . import morph as MO                            # the Mask; morph imports this module
    c = check(connectivity, "connectivity.fill_holes")
    D, H, W = MO._mask(m, "fill_holes").shape
    out = MO._out_mask(out, m, "fill_holes")
    scratch = E.scratch(scratch, holes_scratch_bytes(m.shape), m.bits.device)
    info = torch.empty(2, dtype=torch.int64, device=m.bits.device)
    E.check(E.lib.unet_conn_holes(W, H, D, m.bits.data_ptr(), out.bits.data_ptr(), info.data_ptr(), c, int(impl), scratch.data_ptr(), scratch.nbytes,
                                  E.stream(m.bits)))
    return out, info
