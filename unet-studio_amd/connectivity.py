"""Connected components with a chosen connectivity on the device (include/unet_connectivity.h): the keep-largest call of
components.py, the instance labelling of instances.py and the hole filling of morph.py with `connectivity` 6, 18 or 26 (face; face
and edge; face, edge and corner neighbours).

  keep_largest   every listed class keeps its largest c-connected component
  label          every c-connected component of the listed classes gets a dense id and a row
  fill_holes     the c-connected components of the complement that touch no face of the volume are set: `connectivity` is the
                 background's, 26 the strict one (scipy.ndimage.binary_fill_holes with generate_binary_structure(3, 3))

With connectivity 6 each call writes exactly the bytes of its sibling.  Each operation has one body, in the module that owns it
(components.keep_largest, instances.label, morph.fill_holes): it calls the older header's symbol at 6 and this header's at 18 and
26, and the three functions here are that body under this module's name, with this header's symbol at 6 too.  The public callers
(instances.lesion_scores, qc.lesion_qc, morph.fill_holes_label / run, postproc.run_postproc, EvaluateUNet) take a keyword that
defaults to 6.  These are this project's definitions (parity NOT pinned); every device value is an integer, pinned bit for bit to
scipy.ndimage.label with a structure (tests/test_connectivity_host.py).  No function here synchronises with the host.  Out of
scope: the defragment command of the post-processing chain, the surface definition of distance.py, the C++ host."""
from . import components as CMP
from . import instances as INS
from . import morph as MO
from .components import CONN_6, CONN_18, CONN_26, CONNECTIVITIES, backward_offsets  # noqa: F401
from .instances import COLUMNS, DEFAULT_MAX_INSTANCES  # noqa: F401  (the columns of a row of `label`)

# what the three modules below this one own, under this header's names
check = CMP.check_connectivity
keep_largest_scratch_bytes, label_scratch_bytes, holes_scratch_bytes = CMP.conn_scratch_bytes, INS.conn_label_scratch_bytes, MO.conn_holes_scratch_bytes

# every symbol include/unet_connectivity.h declares (each is bound by the module that calls it)
EXPORTS = ["unet_conn_scratch_bytes", "unet_conn_keep_largest", "unet_conn_label_scratch_bytes", "unet_conn_label",
           "unet_conn_holes_scratch_bytes", "unet_conn_holes"]

IMPL_DEFAULT, IMPL_TILED, IMPL_GLOBAL = 0, 1, 2      # UNET_CONN_IMPL_*


def keep_largest(label, classes, n_classes, connectivity=6, removed=None, scratch=None, impl=IMPL_DEFAULT, stream=None):
    """unet_conn_keep_largest in place on label, a (D, H, W) uint16 device tensor, on the current stream (or the raw `stream`);
    returns label.  Arguments as components.keep_largest: every listed class keeps its largest `connectivity`-connected component,
    the one holding the smallest linear index among equal counts."""
    return CMP.keep_largest(label, classes, n_classes, removed, scratch, impl, stream, connectivity, _who="connectivity.keep_largest")


def label(labels, n_classes, classes=None, connectivity=6, max_instances=DEFAULT_MAX_INSTANCES, impl=IMPL_DEFAULT, scratch=None, out=None,
          stream=None):
    """unet_conn_label on the current stream (or the raw `stream`): (inst, rows, info) on the device exactly as instances.label
    returns them, for the `connectivity`-connected components of the listed classes.  No host synchronisation."""
    return INS.label(labels, n_classes, classes, max_instances, impl, scratch, out, stream, connectivity, _who="connectivity.label")


def fill_holes(m, connectivity=6, impl=IMPL_DEFAULT, scratch=None, out=None):
    """unet_conn_holes on a morph.Mask: (Mask, info); info a device int64[2] tensor: the voxels filled, the holes.  connectivity is
    the background's.  out may be m"""
    check(connectivity, "connectivity.fill_holes")               # refused before m is looked at, which the body does first
    return MO.fill_holes(m, impl, scratch, out, connectivity, _who="connectivity.fill_holes")
