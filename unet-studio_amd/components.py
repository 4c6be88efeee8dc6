"""A model's single_component_label (unet.hpp:23; main.cpp:186 loads it, evaluate.cpp:199 hands it to every evaluation set) on the
device (include/unet_components.h): every listed class of a label map keeps its largest 6-connected component, the one holding the
smallest linear index among equal counts, and every other voxel of that class becomes 0.  Unlisted values are never touched.

The definition is this project's; parity with TIPL's evalution_set is not pinned.  All listed classes are labelled
in one pass over the uint16 label map: IMPL_TILED builds each TILE's union-find in LDS and hooks the tiles together across their
faces, IMPL_GLOBAL hooks every voxel in global memory (the measured baseline and a second witness of the bits).
keep_largest(connectivity=18 | 26) goes through connectivity.py (include/unet_connectivity.h)."""
import ctypes as C


from . import connectivity as CN
from . import engine as E
from .engine import UNetError

E._sig("unet_components_scratch_bytes", C.c_int, C.c_int64, C.c_int, C.POINTER(C.c_size_t))
E._sig("unet_components_keep_largest", C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_uint32), C.c_int,
       C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p)
# every symbol include/unet_components.h declares
EXPORTS = ["unet_components_scratch_bytes", "unet_components_keep_largest"]

IMPL_DEFAULT, IMPL_TILED, IMPL_GLOBAL = 0, 1, 2
TILE = (32, 8, 8)   # (TX, TY, TZ) of IMPL_TILED: UNET_COMPONENTS_TILE_X / _Y / _Z


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
    n = C.c_size_t()
    E.check(E.lib.unet_components_scratch_bytes(int(voxels), int(n_classes), C.byref(n)))
    return n.value


def keep_largest(label, classes, n_classes, removed=None, scratch=None, impl=IMPL_DEFAULT, stream=None, connectivity=6):
    """In place on label, a (D, H, W) uint16 device tensor, on the current stream (or the raw `stream`); returns label.
    classes: the listed classes (an empty list changes nothing).  removed: a uint32 / int32 device tensor of n_classes entries that
    receives the voxels zeroed per class.  scratch: a uint8 device tensor of components_scratch_bytes(D*H*W, n_classes) bytes to
    reuse (one is made when needed).  connectivity: 6 (this header's call), 18 or 26 (connectivity.keep_largest: the same scratch
    size and impl values serve it)."""
    if CN.check(connectivity, "components.keep_largest") != 6:
        return CN.keep_largest(label, classes, n_classes, connectivity, removed=removed, scratch=scratch, impl=impl, stream=stream)
    (D, H, W), classes, need = CN.keep_largest_args("components", label, classes, n_classes, removed, components_scratch_bytes)
    scratch = E.scratch(scratch, need, label.device)
    arr = (C.c_uint32 * max(1, len(classes)))(*classes)
    E.check(E.lib.unet_components_keep_largest(W, H, D, label.data_ptr(), int(n_classes), arr, len(classes),
                                               removed.data_ptr() if removed is not None else None, int(impl), scratch.data_ptr(),
                                               scratch.nbytes, E.stream(label, stream)))
    return label
