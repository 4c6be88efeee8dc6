"""The pre-processing chain and the orientation a model carries (preproc / orientation; run_preproc and handle_orientation,
evaluate.cpp:201-204, the command names evaluate.cpp:5-17), on the device (include/unet_preproc.h).

A chain is commands separated by '+', run left to right on the scan's own grid before it is brought to the model's:
none, gaussian_filter, smoothing_filter, normalize, upsampling, downsampling, flip_x|y|z, swap_xy|yz|xz.  An orientation is a
chain of the six flip / swap names.  The definitions are in include/unet_preproc.h; they are this project's, and parity with
TIPL's run_preproc / handle_orientation is not pinned.

The geometry commands move voxels, so the chain also yields a map: `geometry` returns the grid after the chain and the map from
its voxels back to positions on the original grid.  An orientation never runs as a pass: `orientation_map` turns it into the map
from a model voxel to the grid the model -> image map is computed on, and EvaluateUNet folds both into the two resampling maps
it already uses.  Maps are space.py's (m[9], t[3]) float32, composed in float64 and rounded once; dims are (w, h, d), shapes
torch's (d, h, w)."""
import ctypes as C

import numpy as np
import torch

from . import engine as E
from . import space as SP
from .engine import UNetError

E._sig("unet_preproc_filter", C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p)
E._sig("unet_preproc_downsample", C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p)
E._sig("unet_preproc_upsample", C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p)
E._sig("unet_preproc_permute", C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p)
E._sig("unet_preproc_scratch_bytes", C.c_int, C.c_int64, C.POINTER(C.c_size_t))
E._sig("unet_preproc_normalize", C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_size_t, C.c_void_p)
# every symbol include/unet_preproc.h declares
EXPORTS = ["unet_preproc_filter", "unet_preproc_downsample", "unet_preproc_upsample", "unet_preproc_permute",
           "unet_preproc_scratch_bytes", "unet_preproc_normalize"]

FILTER_GAUSSIAN, FILTER_MEAN = 0, 1
IMPL_DEFAULT, IMPL_LDS, IMPL_VOXEL = 0, 1, 2
FILTERS = {"gaussian_filter": FILTER_GAUSSIAN, "smoothing_filter": FILTER_MEAN}
PERMUTES = {"flip_x": 0, "flip_y": 1, "flip_z": 2, "swap_xy": 3, "swap_yz": 4, "swap_xz": 5}
# evaluate.cpp:5-17
COMMANDS = ("none", "gaussian_filter", "smoothing_filter", "normalize", "upsampling", "downsampling") + tuple(PERMUTES)
_SWAP_AXES = {"swap_xy": (0, 1), "swap_yz": (1, 2), "swap_xz": (0, 2)}


# ---- parsing (host only) ---------------------------------------------------------------------------------------------------------
def _parse(text, allowed):
    steps = []
    for name in (s.strip() for s in (text or "").split("+")):
        if not name:
            continue
        if name not in allowed:
            raise UNetError("unknown command " + name)
        steps.append(name)
    return steps


def parse_chain(text):
    """'gaussian_filter+downsampling' -> ['gaussian_filter', 'downsampling'].  Raises UNetError("unknown command <name>")."""
    return _parse(text, COMMANDS)


def parse_orientation(text):
    """the same syntax; only the six flip / swap names"""
    return _parse(text, PERMUTES)


def _steps(steps, parse):
    if steps is None or isinstance(steps, str):
        return parse(steps)
    steps = list(steps)
    for name in steps:
        if name not in (COMMANDS if parse is parse_chain else PERMUTES):
            raise UNetError("unknown command %s" % (name,))
    return steps


def active(steps):
    """the commands that do something: a chain of only `none` is an empty chain"""
    return [s for s in steps if s != "none"]


def needs_scratch(steps):
    return "normalize" in steps


# ---- maps (host only) ------------------------------------------------------------------------------------------------------------
def _result_grid(name, dims, vs):
    """one command: (dims', vs', m {3,3}, t {3}) float64, the map taking a voxel of the result to a position of the source"""
    dims, vs = list(dims), list(vs)
    m, t = np.eye(3), np.zeros(3)
    if name in _SWAP_AXES:
        a, b = _SWAP_AXES[name]
        m[[a, b]] = m[[b, a]]
        dims[a], dims[b] = dims[b], dims[a]
        vs[a], vs[b] = vs[b], vs[a]
    elif name in PERMUTES:                       # flip: x -> dim-1-x
        a = "xyz".index(name[-1])
        m[a, a], t[a] = -1.0, dims[a] - 1
    elif name == "downsampling":                 # the centre of the 2x2x2 cell
        m, t = m * 2.0, t + 0.5
        dims, vs = [(v + 1) // 2 for v in dims], [v * 2.0 for v in vs]
    elif name == "upsampling":
        m, t = m * 0.5, t - 0.25
        dims, vs = [v * 2 for v in dims], [v * 0.5 for v in vs]
    return tuple(dims), tuple(vs), m, t


def geometry(steps, dims, vs):
    """The grid after the chain and the way back: (dims', vs', G), G taking a voxel of the preprocessed grid to a position on the
    original dims grid (float64 composition of every command's map, rounded once).  Filters, normalize and none are identities."""
    steps = _steps(steps, parse_chain)
    dims, vs = SP._dims(dims, "dims"), SP._triple(vs, "voxel size")
    m, t = np.eye(3), np.zeros(3)
    for name in steps:
        dims, vs, ms, ts = _result_grid(name, dims, vs)
        m, t = m @ ms, m @ ts + t                # original <- ... <- this command's source <- its result
        if dims[0] * dims[1] * dims[2] >= 1 << 31:
            raise UNetError("preproc: %s makes a grid of 2^31 voxels or more" % name)
    return dims, vs, SP._f32_map(m, t)


def orientation_map(steps, model_dim, model_vs):
    """(D0, vs0, M): the orientation commands applied in order to a grid D0 at vs0 yield exactly the model's grid, so D0 and vs0
    are model_dim and model_vs run through the swaps in reverse order; M takes a model voxel to a D0 voxel."""
    steps = _steps(steps, parse_orientation)
    d0, vs0 = SP._dims(model_dim, "model_dim"), SP._triple(model_vs, "model_vs")
    for name in reversed(steps):
        if name in _SWAP_AXES:
            d0, vs0 = _result_grid(name, d0, vs0)[:2]
    _, _, M = geometry(steps, d0, vs0)
    return d0, vs0, M


# ---- the device calls ------------------------------------------------------------------------------------------------------------
def preproc_scratch_bytes(values):
    return E.size_query(E.lib.unet_preproc_scratch_bytes, int(values))


def _vol(a, name):
    if not (torch.is_tensor(a) and a.is_cuda and a.dtype == torch.float32 and a.is_contiguous() and a.dim() == 4):
        raise UNetError("preproc: %s must be a contiguous float32 {C, d, h, w} device tensor" % name)
    return a


def _out(src, out, shape):
    if out is None:
        return torch.empty(shape, dtype=torch.float32, device=src.device)
    if not (torch.is_tensor(out) and out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.device == src.device
            and out.numel() == int(np.prod(shape))):
        raise UNetError("preproc: out must be a contiguous float32 tensor of %d values on the source's device" % int(np.prod(shape)))
    return out.view(shape)


def result_shape(name, shape):
    """{C, d, h, w} after one command"""
    c, d, h, w = (int(v) for v in shape)
    (w, h, d) = _result_grid(name, (w, h, d), (1.0, 1.0, 1.0))[0]
    return (c, d, h, w)


def apply(name, src, out=None, impl=IMPL_DEFAULT):
    """One out-of-place command (a filter, downsampling, upsampling, a flip or a swap) on the current stream: src {C, d, h, w}
    -> a new {C, d', h', w'} tensor (or out, of that many values)."""
    c, d, h, w = (int(v) for v in _vol(src, "src").shape)
    if name not in COMMANDS or name in ("none", "normalize"):
        raise UNetError("preproc: %s is not an out-of-place command" % (name,))
    out = _out(src, out, result_shape(name, src.shape))
    st = E.stream(src)
    if name in FILTERS:
        E.check(E.lib.unet_preproc_filter(src.data_ptr(), out.data_ptr(), w, h, d, c, FILTERS[name], int(impl), st))
    elif name == "downsampling":
        E.check(E.lib.unet_preproc_downsample(src.data_ptr(), out.data_ptr(), w, h, d, c, st))
    elif name == "upsampling":
        E.check(E.lib.unet_preproc_upsample(src.data_ptr(), out.data_ptr(), w, h, d, c, st))
    else:
        E.check(E.lib.unet_preproc_permute(src.data_ptr(), out.data_ptr(), w, h, d, c, PERMUTES[name], st))
    return out


def normalize_(buf, scratch=None):
    """In place on the current stream: the whole buffer divided by its maximum when that is > 0 (NaN skipped)."""
    if not (torch.is_tensor(buf) and buf.is_cuda and buf.dtype == torch.float32 and buf.is_contiguous()):
        raise UNetError("preproc: normalize needs a contiguous float32 device tensor")
    need = preproc_scratch_bytes(buf.numel())
    scratch = E.scratch(scratch, need, buf.device)
    E.check(E.lib.unet_preproc_normalize(buf.data_ptr(), buf.numel(), scratch.data_ptr(), scratch.nbytes,
                                         E.stream(buf)))
    return buf


def run_preproc(x, steps, scratch=None):
    """Runs the chain (a string or parsed steps) on x {C, d, h, w}, a contiguous fp32 device tensor, on the current stream and
    returns the preprocessed {C, d', h', w'} tensor.  The out-of-place commands ping-pong between two buffers sized for the
    largest grid of the chain; x is never written (a chain that does nothing returns x itself).  scratch: a uint8 device tensor
    of preproc_scratch_bytes(values) bytes for normalize to reuse."""
    steps = active(_steps(steps, parse_chain))
    _vol(x, "x")
    shapes, shape = [], tuple(int(v) for v in x.shape)
    for name in steps:                                   # every size check before any device work
        if name != "normalize":
            shape = result_shape(name, shape)
            if shape[1] * shape[2] * shape[3] >= 1 << 31:
                raise UNetError("preproc: %s makes a grid of 2^31 voxels or more" % name)
        shapes.append(shape)
    if not steps:
        return x
    cap = max(int(np.prod(s)) for s in shapes)
    bufs = [None, None]
    cur, at = x, -1                                      # at: the buffer cur lives in (-1: the caller's tensor)
    for name, shape in zip(steps, shapes):
        if name == "normalize" and at >= 0:
            normalize_(cur, scratch)
            continue
        to = 1 - at if at >= 0 else 0
        if bufs[to] is None:
            bufs[to] = torch.empty(cap, dtype=torch.float32, device=x.device)
        dst = bufs[to][:int(np.prod(shape))].view(shape)
        if name == "normalize":                          # on the caller's tensor: on a copy
            dst.copy_(cur)
            normalize_(dst, scratch)
        else:
            apply(name, cur, out=dst)
        cur, at = dst, to
    return cur
