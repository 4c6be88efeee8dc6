"""Binary morphology on bit-packed masks on the device (include/unet_morph.h): the repair of a label map.

  pack, unpack, count        a label map -> a mask of one bit a voxel (uint64 words along x), back to bytes, its set bits
  dilate, erode              n steps with a 6-, 18- or 26-neighbourhood; an erosion's outside reads `border`
  open, close                host chains: open = dilate n of (erode n, border 1), close = erode n, border 1, of (dilate n); with
                             border 1 a closing never removes a voxel and an opening never adds one
  fill_holes                 the 6-connected components of the complement that touch no face of the volume are set
                             (scipy.ndimage.binary_fill_holes with its default structure), through the exact labelling of components.py;
                             connectivity=18 | 26 chooses the background's connectivity (unet_conn_holes of
                             include/unet_connectivity.h, from the same body; connectivity.fill_holes is that body too)
  dilate_label, erode_label, open_label, close_label, fill_holes_label     the same on one value of a uint16 label map, in place
  run                        a list of such ops on a label map; postproc.run_postproc(morphology=...) and EvaluateUNet(morphology=...)
                             run it on the `label` output after single_component

The reference leaves this to TIPL (defragment_smoothing, fill_and_smooth_labels), so these are this project's definitions (parity NOT
pinned).  Every device value is a bit or an integer count: the device is pinned to the numpy restatements of
tests/test_morph_host.py bit for bit.  No function here synchronises with the host.  Out of scope: grey-scale morphology, structuring
elements other than the three, geodesic reconstruction, acting on fg_prob / label_prob, and the C++ host."""
import ctypes as C

import torch

from . import engine as E
from .components import check_connectivity
from .engine import UNetError

_I, _P = C.c_int, C.c_void_p
E._sig("unet_morph_scratch_bytes", _I, _I, _I, _I, C.POINTER(C.c_size_t))
E._sig("unet_morph_pack", _I, _I, _I, _I, _P, _I, _I, C.POINTER(C.c_uint32), _I, _P, _P, C.c_size_t, _P)
E._sig("unet_morph_unpack", _I, _I, _I, _I, _P, _P, _P)
E._sig("unet_morph_count", _I, _I, _I, _I, _P, _P, _P)
E._sig("unet_morph_step", _I, _I, _I, _I, _P, _P, _I, _I, _I, _I, _I, _P, C.c_size_t, _P)
E._sig("unet_morph_holes", _I, _I, _I, _I, _P, _P, _P, _I, _P, C.c_size_t, _P)
E._sig("unet_morph_apply", _I, _I, _I, _I, _P, _P, _I, _I, _P, _P)
E._sig("unet_conn_holes_scratch_bytes", _I, _I, _I, _I, C.POINTER(C.c_size_t))
E._sig("unet_conn_holes", _I, _I, _I, _I, _P, _P, _P, _I, _I, _P, C.c_size_t, _P)
# every symbol include/unet_morph.h declares
EXPORTS = ["unet_morph_scratch_bytes", "unet_morph_pack", "unet_morph_unpack", "unet_morph_count", "unet_morph_step", "unet_morph_holes",
           "unet_morph_apply"]

IMPL_DEFAULT, IMPL_LDS, IMPL_GLOBAL = 0, 1, 2        # UNET_MORPH_IMPL_*
DILATE, ERODE = 0, 1                                 # UNET_MORPH_DILATE, UNET_MORPH_ERODE
SET, KEEP = 0, 1                                     # UNET_MORPH_SET, UNET_MORPH_KEEP
FUSE_MAX = 4                                         # UNET_MORPH_FUSE_MAX
BRICK_XW, BRICK_Y, BRICK_Z = 2, 16, 16               # UNET_MORPH_BRICK_*
MAX_ITERATIONS = 255                                 # UNET_MORPH_MAX_ITERATIONS
CONNECTIVITIES = (6, 18, 26)
STEP_OPS = ("dilate", "erode", "open", "close")


class Mask:
    """bits: an int64 device tensor (D, H, WPL), WPL = ceil(W / 64), voxel x of a line in bit (x & 63) of word (x >> 6);
    shape: (D, H, W)"""

    def __init__(self, bits, shape):
        D, H, W = (int(v) for v in shape)
        if not (torch.is_tensor(bits) and bits.is_cuda and bits.dtype == torch.int64 and bits.is_contiguous()
                and tuple(bits.shape) == (D, H, (W + 63) // 64) and bits.numel() > 0):
            raise UNetError("morph.Mask: bits must be a contiguous int64 device tensor (D, H, ceil(W / 64)) for shape %s" % ((D, H, W),))
        self.bits, self.shape = bits, (D, H, W)

    def new(self):
        return Mask(torch.empty_like(self.bits), self.shape)


def morph_scratch_bytes(shape):
    """unet_morph_scratch_bytes for a (D, H, W) grid: one size serves every call"""
    D, H, W = (int(v) for v in shape)
    return E.size_query(E.lib.unet_morph_scratch_bytes, W, H, D)


def conn_holes_scratch_bytes(shape):
    """unet_conn_holes_scratch_bytes for a (D, H, W) grid (connectivity.holes_scratch_bytes): the same size under the newer header's name"""
    D, H, W = (int(v) for v in shape)
    return E.size_query(E.lib.unet_conn_holes_scratch_bytes, W, H, D)


def _scratch(scratch, shape, dev):
    need = morph_scratch_bytes(shape)                    # the size checks, before any device work
    return E.scratch(scratch, need, dev)


def _mask(m, who, name="m"):
    if not isinstance(m, Mask):
        raise UNetError("morph.%s: %s must be a morph.Mask" % (who, name))
    return m


def _out_mask(out, m, who):
    if out is None:
        return m.new()
    _mask(out, who, "out")
    if out.shape != m.shape or out.bits.device != m.bits.device:
        raise UNetError("morph.%s: out must be a Mask of shape %s on m's device" % (who, m.shape))
    return out


def _label_map(labels, who, dtypes=(torch.uint8, torch.uint16)):
    if not (torch.is_tensor(labels) and labels.is_cuda and labels.dtype in dtypes and labels.is_contiguous() and labels.dim() == 3
            and labels.numel() > 0):
        raise UNetError("morph.%s: labels must be a contiguous %s (D, H, W) device tensor"
                        % (who, " or ".join(str(t).split(".")[1] for t in dtypes)))
    return labels


def _connectivity(c, who):
    if c not in CONNECTIVITIES:
        raise UNetError("morph.%s: connectivity must be 6, 18 or 26, got %r" % (who, c))
    return int(c)


def _iterations(n, who):
    if not (isinstance(n, int) and 0 <= n <= MAX_ITERATIONS):
        raise UNetError("morph.%s: iterations must be an integer in [0, %d], got %r" % (who, MAX_ITERATIONS, n))
    return n


def pack(labels, n_classes, classes=None, scratch=None, out=None):
    """unet_morph_pack: the Mask of the voxels of a uint8 / uint16 (D, H, W) device tensor that hold a listed class; classes None
    lists 1..n_classes-1, an empty list gives the empty mask"""
    lab = _label_map(labels, "pack")
    D, H, W = (int(v) for v in lab.shape)
    nc = int(n_classes)
    classes = E.listed_classes("morph.pack", classes, nc)
    dev = lab.device
    scratch = _scratch(scratch, (D, H, W), dev)
    m = out if out is not None else Mask(torch.empty((D, H, (W + 63) // 64), dtype=torch.int64, device=dev), (D, H, W))
    if _mask(m, "pack", "out").shape != (D, H, W) or m.bits.device != dev:
        raise UNetError("morph.pack: out must be a Mask of shape %s on labels' device" % ((D, H, W),))
    E.check(E.lib.unet_morph_pack(W, H, D, lab.data_ptr(), lab.element_size(), nc, E.u32_array(classes), len(classes), m.bits.data_ptr(),
                                  scratch.data_ptr(), scratch.nbytes, E.stream(lab)))
    return m


def unpack(m):
    """unet_morph_unpack: a uint8 (D, H, W) device tensor, 1 where the bit is set"""
    D, H, W = _mask(m, "unpack").shape
    out = torch.empty((D, H, W), dtype=torch.uint8, device=m.bits.device)
    E.check(E.lib.unet_morph_unpack(W, H, D, m.bits.data_ptr(), out.data_ptr(), E.stream(out)))
    return out


def count(m):
    """unet_morph_count: a device int64[1] tensor, the set bits"""
    D, H, W = _mask(m, "count").shape
    out = torch.empty(1, dtype=torch.int64, device=m.bits.device)
    E.check(E.lib.unet_morph_count(W, H, D, m.bits.data_ptr(), out.data_ptr(), E.stream(out)))
    return out


def _step(m, op, connectivity, iterations, border, impl, scratch, out, who):
    D, H, W = _mask(m, who).shape
    c, n = _connectivity(connectivity, who), _iterations(iterations, who)
    out = _out_mask(out, m, who)
    scratch = _scratch(scratch, m.shape, m.bits.device)
    E.check(E.lib.unet_morph_step(W, H, D, m.bits.data_ptr(), out.bits.data_ptr(), op, c, n, int(border), int(impl), scratch.data_ptr(),
                                  scratch.nbytes, E.stream(m.bits)))
    return out


def dilate(m, connectivity=6, iterations=1, impl=IMPL_DEFAULT, scratch=None, out=None):
    """unet_morph_step, UNET_MORPH_DILATE: a new Mask (or `out`, which must not be m)"""
    return _step(m, DILATE, connectivity, iterations, 0, impl, scratch, out, "dilate")


def erode(m, connectivity=6, iterations=1, impl=IMPL_DEFAULT, scratch=None, out=None, border=0):
    """unet_morph_step, UNET_MORPH_ERODE: a neighbour outside the grid reads `border` (0: scipy.ndimage's default; 1: a face of
    the volume is not an edge of the object)"""
    return _step(m, ERODE, connectivity, iterations, border, impl, scratch, out, "erode")


def open(m, connectivity=6, iterations=1, impl=IMPL_DEFAULT, scratch=None):   # noqa: A001  (the operation's name)
    """dilate n of (erode n, border 1): never adds a voxel"""
    return dilate(erode(m, connectivity, iterations, impl, scratch, border=1), connectivity, iterations, impl, scratch)


def close(m, connectivity=6, iterations=1, impl=IMPL_DEFAULT, scratch=None):
    """erode n, border 1, of (dilate n): never removes a voxel"""
    return erode(dilate(m, connectivity, iterations, impl, scratch), connectivity, iterations, impl, scratch, border=1)


def fill_holes(m, impl=IMPL_DEFAULT, scratch=None, out=None, connectivity=6, _who=None):
    """unet_morph_holes: (Mask, info); info a device int64[2] tensor: the voxels filled, the holes.  out may be m.  connectivity: the
    background's, 6 (this header's call), 18 or 26 (unet_conn_holes: the same scratch size and impl values).  _who:
    connectivity.fill_holes' message prefix; with it unet_conn_holes runs at 6 too."""
    D, H, W = _mask(m, "fill_holes").shape
    c = check_connectivity(connectivity, _who or "morph.fill_holes")
    conn = _who is not None or c != 6                             # which header's calls
    out = _out_mask(out, m, "fill_holes")
    scratch = E.scratch(scratch, (conn_holes_scratch_bytes if conn else morph_scratch_bytes)(m.shape), m.bits.device)
    info = torch.empty(2, dtype=torch.int64, device=m.bits.device)
    head = (W, H, D, m.bits.data_ptr(), out.bits.data_ptr(), info.data_ptr())
    tail = (int(impl), scratch.data_ptr(), scratch.nbytes, E.stream(m.bits))
    E.check(E.lib.unet_conn_holes(*head, c, *tail) if conn else E.lib.unet_morph_holes(*head, *tail))
    return out, info


def apply(labels, m, value, mode, changed=None):
    """unet_morph_apply in place on a uint16 (D, H, W) device tensor.  SET: a voxel whose bit is 1 and whose label is 0 becomes value;
    KEEP: a voxel whose label is value and whose bit is 0 becomes 0.  Returns the device int64[1] tensor of the voxels written
    (`changed` when given: one int64 entry)"""
    lab = _label_map(labels, "apply", (torch.uint16,))
    if _mask(m, "apply").shape != tuple(int(v) for v in lab.shape) or m.bits.device != lab.device:
        raise UNetError("morph.apply: the mask's shape %s is not the labels' %s" % (m.shape, tuple(lab.shape)))
    if changed is None:
        changed = torch.empty(1, dtype=torch.int64, device=lab.device)
    elif not (torch.is_tensor(changed) and changed.is_cuda and changed.device == lab.device and changed.dtype == torch.int64
              and changed.numel() == 1):
        raise UNetError("morph.apply: changed must be a device int64 tensor of one entry on labels' device")
    D, H, W = m.shape
    E.check(E.lib.unet_morph_apply(W, H, D, lab.data_ptr(), m.bits.data_ptr(), int(value), int(mode), changed.data_ptr(), E.stream(lab)))
    return changed


# ---- on a uint16 label map, in place -------------------------------------------------------------------------------------------------
def _value(value, who):
    if not (isinstance(value, int) and 1 <= value <= 65535):
        raise UNetError("morph.%s: value must be an integer in [1, 65535], got %r" % (who, value))
    return value


def _label_op(name, labels, value, connectivity, iterations, border, impl, scratch, changed):
    lab = _label_map(labels, name + "_label", (torch.uint16,))
    v = _value(value, name + "_label")
    _connectivity(connectivity, name + "_label")
    _iterations(iterations, name + "_label")
    scratch = _scratch(scratch, lab.shape, lab.device)
    m = pack(lab, v + 1, [v], scratch=scratch)             # the voxels equal to value: everything above it is no member
    if name == "dilate":
        m = dilate(m, connectivity, iterations, impl, scratch)
    elif name == "erode":
        m = erode(m, connectivity, iterations, impl, scratch, border=border)
    elif name == "open":
        m = open(m, connectivity, iterations, impl, scratch)
    else:
        m = close(m, connectivity, iterations, impl, scratch)
    return apply(lab, m, v, SET if name in ("dilate", "close") else KEEP, changed)


def dilate_label(labels, value, connectivity=6, iterations=1, impl=IMPL_DEFAULT, scratch=None, changed=None):
    """the voxels equal to value grow: a grown voxel that reads 0 becomes value.  Returns the device count of the voxels written"""
    return _label_op("dilate", labels, value, connectivity, iterations, 0, impl, scratch, changed)


def close_label(labels, value, connectivity=6, iterations=1, impl=IMPL_DEFAULT, scratch=None, changed=None):
    """a voxel the closing of the voxels equal to value adds, and that reads 0, becomes value"""
    return _label_op("close", labels, value, connectivity, iterations, 0, impl, scratch, changed)


def erode_label(labels, value, connectivity=6, iterations=1, impl=IMPL_DEFAULT, scratch=None, changed=None, border=0):
    """a voxel the erosion of the voxels equal to value removes becomes 0"""
    return _label_op("erode", labels, value, connectivity, iterations, border, impl, scratch, changed)


def open_label(labels, value, connectivity=6, iterations=1, impl=IMPL_DEFAULT, scratch=None, changed=None):
    """a voxel the opening of the voxels equal to value removes becomes 0"""
    return _label_op("open", labels, value, connectivity, iterations, 0, impl, scratch, changed)


def fill_holes_label(labels, classes, value, n_classes, impl=IMPL_DEFAULT, scratch=None, changed=None, connectivity=6):
    """the holes of the voxels of the listed classes: a hole voxel that reads 0 becomes value; one that holds an unlisted class is
    left alone.  connectivity: the background's, 6, 18 or 26"""
    check_connectivity(connectivity, "morph.fill_holes_label")
    lab = _label_map(labels, "fill_holes_label", (torch.uint16,))
    v = _value(value, "fill_holes_label")
    scratch = _scratch(scratch, lab.shape, lab.device)
    m = pack(lab, n_classes, classes, scratch=scratch)
    fill_holes(m, impl, scratch, out=m, connectivity=connectivity)
    return apply(lab, m, v, SET, changed)


def check_ops(ops, n_classes):
    """The ops of `run`, validated on the host: ("dilate" | "erode" | "open" | "close", value, connectivity, iterations) and
    ("fill_holes", classes, value) or ("fill_holes", classes, value, connectivity), the background's connectivity (6 without it).
    Returns them as a list of tuples, a fill_holes op with as many elements as it came with; a bad op raises UNetError naming it."""
    nc = int(n_classes)
    if nc < 2 or nc > 65536:
        raise UNetError("morphology: n_classes must be in [2, 65536], got %d" % nc)
    if isinstance(ops, (str, bytes)) or not hasattr(ops, "__iter__"):
        raise UNetError("morphology: ops must be a list of tuples, got %r" % (ops,))
    checked = []
    for i, op in enumerate(ops):
        def bad(why):
            return UNetError("morphology: op %d %r: %s" % (i, op, why))

        def integer(v):
            return isinstance(v, int) and not isinstance(v, bool)

        if not isinstance(op, (tuple, list)) or not op or not isinstance(op[0], str):
            raise bad("an op is a tuple that starts with its name")
        name = op[0]
        if name in STEP_OPS:
            if len(op) != 4:
                raise bad("%s takes (value, connectivity, iterations)" % name)
            value, c, n = op[1:]
            if not integer(value) or not 1 <= value < nc:
                raise bad("value must be an integer in [1, %d]" % (nc - 1))
            if not integer(c) or c not in CONNECTIVITIES:
                raise bad("connectivity must be 6, 18 or 26")
            if not integer(n) or not 0 <= n <= MAX_ITERATIONS:
                raise bad("iterations must be an integer in [0, %d]" % MAX_ITERATIONS)
            checked.append((name, value, c, n))
        elif name == "fill_holes":
            if len(op) not in (3, 4):
                raise bad("fill_holes takes (classes, value) or (classes, value, connectivity)")
            classes, value = op[1:3]
            if isinstance(classes, (str, bytes)) or not hasattr(classes, "__iter__"):
                raise bad("classes must be a list")
            classes = list(classes)
            for v in classes:
                if not integer(v) or not 1 <= v < nc:
                    raise bad("class %r is not an integer in [1, %d]" % (v, nc - 1))
            if not integer(value) or not 1 <= value < nc:
                raise bad("value must be an integer in [1, %d]" % (nc - 1))
            if len(op) == 4 and (not integer(op[3]) or op[3] not in CONNECTIVITIES):
                raise bad("connectivity must be 6, 18 or 26")
            checked.append((name, classes, value) + tuple(op[3:]))
        else:
            raise bad("unknown op (one of %s, fill_holes)" % ", ".join(STEP_OPS))
    return checked


def run(labels, ops, n_classes, scratch=None):
    """Applies the ops in order, in place on a uint16 (D, H, W) device tensor.  Returns a device int64 tensor: the voxels each op
    changed.  Every op is validated before any device work (check_ops)."""
    ops = check_ops(ops, n_classes)
    lab = _label_map(labels, "run", (torch.uint16,))
    changed = torch.zeros(len(ops), dtype=torch.int64, device=lab.device)
    if ops:
        scratch = _scratch(scratch, lab.shape, lab.device)
    for i, op in enumerate(ops):
        if op[0] == "fill_holes":
            fill_holes_label(lab, op[1], op[2], n_classes, scratch=scratch, changed=changed[i:i + 1],
                             connectivity=op[3] if len(op) == 4 else 6)
        else:
            _label_op(op[0], lab, op[1], op[2], op[3], 0, IMPL_DEFAULT, scratch, changed[i:i + 1])
    return changed
