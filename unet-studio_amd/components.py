"""A model's single_component_label (unet.hpp:23; main.cpp:186 loads it, evaluate.cpp:199 hands it to every evaluation set) on the
device (include/unet_components.h): every listed class of a label map keeps its largest 6-connected component, the one holding the
smallest linear index among equal counts, and every other voxel of that class becomes 0.  Unlisted values are never touched.

The definition is this project's; parity with TIPL's evalution_set is not pinned.  All listed classes are labelled
in one pass over the uint16 label map: IMPL_TILED builds each TILE's union-find in LDS and hooks the tiles together across their
faces, IMPL_GLOBAL hooks every voxel in global memory (the measured baseline and a second witness of the bits).
keep_largest is the one body of the operation: with connectivity 18 or 26, and for connectivity.keep_largest, it runs
unet_conn_keep_largest (include/unet_connectivity.h).  What instances.py, morph.py and connectivity.py share about a connectivity
(the three values, check_connectivity, backward_offsets) lives here, below all of them."""
import ctypes as C

import torch

from . import engine as E
from .engine import UNetError

_I, _P = C.c_int, C.c_void_p
E._sig("unet_components_scratch_bytes", _I, C.c_int64, _I, C.POINTER(C.c_size_t))
E._sig("unet_components_keep_largest", _I, _I, _I, _I, _P, _I, C.POINTER(C.c_uint32), _I, _P, _I, _P, C.c_size_t, _P)
E._sig("unet_conn_scratch_bytes", _I, C.c_int64, _I, C.POINTER(C.c_size_t))
E._sig("unet_conn_keep_largest", _I, _I, _I, _I, _P, _I, C.POINTER(C.c_uint32), _I, _P, _I, _I, _P, C.c_size_t, _P)
# every symbol include/unet_components.h declares
EXPORTS = ["unet_components_scratch_bytes", "unet_components_keep_largest"]

IMPL_DEFAULT, IMPL_TILED, IMPL_GLOBAL = 0, 1, 2
TILE = (32, 8, 8)   # (TX, TY, TZ) of IMPL_TILED: UNET_COMPONENTS_TILE_X / _Y / _Z
CONN_6, CONN_18, CONN_26 = 6, 18, 26                 # UNET_CONN_6 / _18 / _26
CONNECTIVITIES = (CONN_6, CONN_18, CONN_26)


def check_connectivity(connectivity, who="connectivity"):
    """6, 18 or 26 as an int; anything else raises UNetError naming the value.  Host only."""
    if isinstance(connectivity, bool) or not isinstance(connectivity, int) or connectivity not in CONNECTIVITIES:
        raise UNetError("%s: connectivity must be 6, 18 or 26, got %r" % (who, connectivity))
    return int(connectivity)


def backward_offsets(connectivity):
    """N-(c): the (dx, dy, dz) of the neighbourhood whose neighbour has the smaller linear index, 3, 9 or 13 of them: what a voxel
    hooks to in the kernels (cc_for_backward in csrc/cc_union_find.h)"""
    reach = {6: 1, 18: 2, 26: 3}[check_connectivity(connectivity)]
    return [(dx, dy, dz) for dz in (-1, 0) for dy in (-1, 0, 1) for dx in (-1, 0, 1)
            if 1 <= abs(dx) + abs(dy) + abs(dz) <= reach and (dz, dy, dx) < (0, 0, 0)]


def resolve(spec, model):
    """The caller's choice -> a sorted list of distinct classes.  None and () give []; "model" gives model.single_component_label;
    an iterable of ints gives its entries.  An entry that is 0 or >= model.out_count raises UNetError naming it.  Host only."""
    if spec is None:
        return []
    if isinstance(spec, str):
        if spec != "model":
            raise UNetError('single_component: "model" or a list of classes, got %r' % (spec,))
        spec = model.single_component_label
    out = set()
    for v in spec:
        if isinstance(v, bool) or int(v) != v:
            raise UNetError("single_component: class %r is not an integer" % (v,))
        v = int(v)
        if v <= 0 or v >= model.out_count:
            raise UNetError("single_component: class %d is not in [1, %d]" % (v, model.out_count - 1))
        out.add(v)
    return sorted(out)


def components_scratch_bytes(voxels, n_classes):
    return E.size_query(E.lib.unet_components_scratch_bytes, int(voxels), int(n_classes))


def conn_scratch_bytes(voxels, n_classes):
    """unet_conn_scratch_bytes (connectivity.keep_largest_scratch_bytes): the same size under the newer header's name"""
    return E.size_query(E.lib.unet_conn_scratch_bytes, int(voxels), int(n_classes))


def keep_largest(label, classes, n_classes, removed=None, scratch=None, impl=IMPL_DEFAULT, stream=None, connectivity=6, _who=None):
    """In place on label, a (D, H, W) uint16 device tensor, on the current stream (or the raw `stream`); returns label.
    classes: the listed classes (an empty list changes nothing).  removed: a uint32 / int32 device tensor of n_classes entries that
    receives the voxels zeroed per class.  scratch: a uint8 device tensor of components_scratch_bytes(D*H*W, n_classes) bytes to
    reuse (one is made when needed).  connectivity: 6 (this header's call), 18 or 26 (unet_conn_keep_largest: the same scratch
    size and impl values serve it).  _who: connectivity.keep_largest's message prefix; with it unet_conn_keep_largest runs at 6 too."""
    c = check_connectivity(connectivity, _who or "components.keep_largest")
    conn = _who is not None or c != 6                             # which header's calls, and whose name the messages carry
    who = (_who or "connectivity.keep_largest") if conn else "components"
    if not (torch.is_tensor(label) and label.is_cuda and label.dtype == torch.uint16 and label.is_contiguous() and label.dim() == 3):
        raise UNetError("%s: label must be a contiguous uint16 (D, H, W) device tensor" % who)
    D, H, W = (int(v) for v in label.shape)
    if removed is not None and not (torch.is_tensor(removed) and removed.is_cuda and removed.device == label.device
                                    and removed.dtype in (torch.uint32, torch.int32) and removed.is_contiguous()
                                    and removed.numel() == int(n_classes)):
        raise UNetError("%s: removed must be a contiguous uint32 device tensor of n_classes entries on label's device" % who)
    classes = [int(v) for v in classes]                          # a list is required here: None does not mean every class
    need = (conn_scratch_bytes if conn else components_scratch_bytes)(D * H * W, n_classes)   # the size checks, before any device work
    classes = E.listed_classes(who, classes, n_classes)
    scratch = E.scratch(scratch, need, label.device)
    head = (W, H, D, label.data_ptr(), int(n_classes), E.u32_array(classes), len(classes), removed.data_ptr() if removed is not None else None)
    tail = (int(impl), scratch.data_ptr(), scratch.nbytes, E.stream(label, stream))
    E.check(E.lib.unet_conn_keep_largest(*head, c, *tail) if conn else E.lib.unet_components_keep_largest(*head, *tail))
    return label
