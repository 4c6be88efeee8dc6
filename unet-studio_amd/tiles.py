"""A scan larger than the model's field of view, evaluated in overlapping tiles whose logits are blended (include/unet_tiles.h).

The reference loops over several model_io chunks per file (evaluate.cpp:223-230); what makes more than one chunk is TIPL's
handle_fov_pre / handle_fov_post, which is not in the reference tree.  The canvas, the plan, the weight and the blend are this
project's definitions, written down in the header: parity with TIPL is NOT pinned.

`canvas_dims`, `plan_axis`, `plan_tiles` and `weights` are host only.  `blend` and `postproc_tiles` run the two kernels on the
current stream.  A plan is three lists of integer tile origins, (x, y, z); the tile index is (iz*ny + iy)*nx + ix.  Shapes are
torch's (d, h, w); dims, as model.dim, are (w, h, d).

The stack of tile logits costs tiles * out_c * tile_voxels * 4 bytes on the device: 27 tiles of 6 x 128^3 are 1.36 GB."""
import ctypes as C
import math

import numpy as np
import torch

from . import engine as E
from . import space as SP
from .engine import UNetError

TILES_MAX_AXIS = 16     # UNET_TILES_MAX_AXIS
TILES_MAX_DIM = 512     # UNET_TILES_MAX_DIM


class UnetTilePlan(C.Structure):
    _fields_ = [("n", C.c_int * 3), ("origin", (C.c_int * TILES_MAX_AXIS) * 3)]


E._sig("unet_tiles_blend", C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(UnetTilePlan), C.c_int, C.c_int, C.c_int,
       C.c_void_p, C.c_void_p)
E._sig("unet_tiles_postproc", C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(UnetTilePlan), C.c_int, C.c_int,
       C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p)
# every symbol include/unet_tiles.h declares
EXPORTS = ["unet_tiles_blend", "unet_tiles_postproc"]

OUTPUTS = SP.OUTPUTS


# ---- the canvas and the plan (host only) -----------------------------------------------------------------------------------------
def check_overlap(overlap):
    try:
        ov = float(overlap)
    except (TypeError, ValueError):
        ov = float("nan")
    if not 0.0 <= ov < 0.5:
        raise UNetError("tiles: tile_overlap must be in [0, 0.5), got %r" % (overlap,))
    return ov


def _extent(image_dim, image_vs, model_vs):
    """ceil(image_dim * image_vs / model_vs) in float64; a ratio within 1e-6 of an integer is that integer"""
    r = float(image_dim) * float(image_vs) / float(model_vs)
    n = round(r)
    return int(n) if abs(r - n) <= 1e-6 else int(math.ceil(r))


def canvas_dims(model_dim, model_vs, image_dim, image_vs, orientation=None):
    """The canvas of a scan, (w, h, d) in the model's frame: per axis max(model_dim, extent of the scan in model voxels).
    orientation (a flip / swap chain or parsed steps): the extents are taken in the frame preproc.orientation_map calls D0 / vs0,
    the one the model -> image map is computed in, and the canvas is brought back to the model's frame through the swaps."""
    from . import preproc as PRE
    md, mv = SP._dims(model_dim, "model_dim"), SP._triple(model_vs, "model_vs")
    idim, iv = SP._dims(image_dim, "image_dim"), SP._triple(image_vs, "image_vs")
    steps = PRE._steps(orientation, PRE.parse_orientation)
    d0, vs0 = PRE.orientation_map(steps, md, mv)[:2] if steps else (md, mv)
    c = tuple(max(d0[a], _extent(idim[a], iv[a], vs0[a])) for a in range(3))
    for name in steps:
        if name in PRE._SWAP_AXES:
            c = PRE._result_grid(name, c, (1.0, 1.0, 1.0))[0]
    return tuple(int(v) for v in c)


def plan_axis(canvas, tile, overlap=0.25):
    """the integer tile origins of one axis (include/unet_tiles.h, PLAN)"""
    Cn, T, ov = int(canvas), int(tile), check_overlap(overlap)
    if T < 1 or Cn < T:
        raise UNetError("tiles: a canvas of %d does not hold a tile of %d" % (Cn, T))
    if Cn == T:
        return [0]
    S = T - int(math.ceil(ov * T))
    if S < 1:
        raise UNetError("tiles: an overlap of %r leaves no step for a tile of %d" % (overlap, T))
    n = 1 + -((T - Cn) // S)
    if n > TILES_MAX_AXIS:
        raise UNetError("tiles: %d tiles along one axis (canvas %d, tile %d), at most %d" % (n, Cn, T, TILES_MAX_AXIS))
    return [(i * (Cn - T) + (n - 1) // 2) // (n - 1) for i in range(n)]


def plan_tiles(canvas_dim, tile_dim, overlap=0.25):
    """the plan of a canvas (w, h, d) in tiles of tile_dim (w, h, d): (x origins, y origins, z origins)"""
    cd, td = SP._dims(canvas_dim, "canvas_dim"), SP._dims(tile_dim, "tile_dim")
    if max(td) > TILES_MAX_DIM:
        raise UNetError("tiles: a tile dimension above %d (the weights must stay exact in fp32), got %s" % (TILES_MAX_DIM, td))
    return tuple(plan_axis(cd[a], td[a], overlap) for a in range(3))


def tile_origins(plan):
    """[(ox, oy, oz), ...] in tile-index order"""
    px, py, pz = plan
    return [(ox, oy, oz) for oz in pz for oy in py for ox in px]


def weights(T):
    """w(p) = min(p, T-1-p) + 1 for p in 0..T-1, float32"""
    p = np.arange(int(T))
    return (np.minimum(p, int(T) - 1 - p) + 1).astype(np.float32)


def _plan_struct(plan):
    try:
        axes = [[int(v) for v in a] for a in plan]
    except (TypeError, ValueError):
        raise UNetError("tiles: a plan is three lists of origins (x, y, z)")
    if len(axes) != 3:
        raise UNetError("tiles: a plan is three lists of origins (x, y, z)")
    s = UnetTilePlan()
    for a, o in enumerate(axes):
        if not 1 <= len(o) <= TILES_MAX_AXIS:
            raise UNetError("tiles: axis %s: n must be in [1, %d], got %d" % ("xyz"[a], TILES_MAX_AXIS, len(o)))
        s.n[a] = len(o)
        for i, v in enumerate(o):
            s.origin[a][i] = v
    return s


# ---- the device calls ------------------------------------------------------------------------------------------------------------
def _stack(tiles, ps):
    if not (torch.is_tensor(tiles) and tiles.is_cuda and tiles.dtype == torch.float32 and tiles.is_contiguous()):
        raise UNetError("tiles: the stack must be a contiguous float32 device tensor")
    n = ps.n[0] * ps.n[1] * ps.n[2]
    if tiles.dim() != 5 or tiles.shape[0] != n:
        raise UNetError("tiles: the stack must be {%d tiles, out_c, td, th, tw}, got %s" % (n, tuple(tiles.shape)))
    return tuple(int(v) for v in tiles.shape[1:])


def blend(tiles, plan, canvas_shape, out=None):
    """unet_tiles_blend on the current stream.  tiles: the stack {n tiles, out_c, td, th, tw} of level-0 logits, a contiguous fp32
    device tensor (tiles * out_c * tile_voxels * 4 bytes: 27 tiles of 6 x 128^3 are 1.36 GB); plan: (x, y, z) origins;
    canvas_shape: (D, H, W).  Returns the canvas logits {out_c, D, H, W}."""
    ps = _plan_struct(plan)
    D, H, W = SP._shape3(canvas_shape, "canvas_shape")
    out_c, td, th, tw = _stack(tiles, ps)
    if out is None:
        out = torch.empty((out_c, D, H, W), dtype=torch.float32, device=tiles.device)
    elif SP._f32(out, "out").numel() != out_c * D * H * W or out.device != tiles.device:
        raise UNetError("tiles: out must hold %d values on the stack's device" % (out_c * D * H * W))
    E.check(E.lib.unet_tiles_blend(tiles.data_ptr(), out_c, tw, th, td, C.byref(ps), W, H, D, out.data_ptr(), E.stream(tiles)))
    return out.view(out_c, D, H, W)


def postproc_tiles(tiles, plan, canvas_shape, threshold=0.5, outputs=OUTPUTS, out=None):
    """unet_tiles_postproc on the current stream: softmax / create_mask / argmax of the blended logits, which are never stored.
    Arguments as blend's.  Returns {name: tensor} for the wanted outputs: label_prob {out_c-1, D, H, W} fp32, fg_prob {D, H, W}
    fp32, label {D, H, W} uint16.  out: {name: tensor} to write into instead of new ones."""
    outputs = tuple(outputs)
    for o in outputs:
        if o not in OUTPUTS:
            raise UNetError("unknown output %s (one of %s)" % (o, ", ".join(OUTPUTS)))
    if not outputs:
        raise UNetError("tiles: no output wanted")
    ps = _plan_struct(plan)
    D, H, W = SP._shape3(canvas_shape, "canvas_shape")
    out_c, td, th, tw = _stack(tiles, ps)
    dev = tiles.device
    shapes = {"label_prob": ((out_c - 1, D, H, W), torch.float32), "fg_prob": ((D, H, W), torch.float32), "label": ((D, H, W), torch.uint16)}
    res = {}
    for o in outputs:
        shape, dt = shapes[o]
        t = (out or {}).get(o)
        if t is None:
            t = torch.empty(shape, dtype=dt, device=dev)
        elif not (torch.is_tensor(t) and t.is_cuda and t.dtype == dt and t.is_contiguous() and t.numel() == int(np.prod(shape))
                  and t.device == dev):
            raise UNetError("tiles: out[%s] must be a contiguous %s tensor of %d values on the stack's device" % (o, dt, int(np.prod(shape))))
        res[o] = t
    ptr = lambda o: res[o].data_ptr() if o in res else None
    E.check(E.lib.unet_tiles_postproc(tiles.data_ptr(), out_c, tw, th, td, C.byref(ps), W, H, D, float(threshold), ptr("label_prob"),
                                      ptr("fg_prob"), ptr("label"), E.stream(tiles)))
    return res
