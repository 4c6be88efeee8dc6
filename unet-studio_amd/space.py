"""Between a scan's own grid and the model's grid, on the device (include/unet_space.h).

The way in is `read_image_and_label` after the file read (train.cpp:13-40, called for every training, test and QC case): a map from
model voxels to image voxels whose only free parameter is translocation[2] (train.cpp:27), the image sampled tipl::linear and then
tipl::normalize'd, the label sampled tipl::majority -- `to_model_space`.  Its results are valid `image` / `label` entries of the
cases `TrainingFeed` and `qc` take.  The way back is handle_fov_post before run_postproc (evaluate.cpp:274): the logits go to the
native grid and softmax / create_mask / argmax run there -- `postproc_native`, which interpolates the logits inside the fused pass
and never stores them.

`model_to_image_map` is this project's stand-in for tipl::transformation_matrix(arg, model_dim, model_vs, image_dim, image_vs)
(TIPL, not in the reference tree), with the convention augment.affine_matrix uses (centre = dim / 2).  The sampling rules are the
augmentation's (oracle/augment_ref.py restates them).  Parity with TIPL is NOT pinned for either.  These
maps are the model's default fov_strategy "align_top" (unet.cpp:110): one window of model.dim, whatever lies outside it cropped.
A scan larger than that window is tiles.py's (EvaluateUNet(fov_strategy="tiles")); reading files stays out of scope.  A model's preproc
chain and orientation are preproc.py's: EvaluateUNet(preproc=, orientation=) folds them into these maps with `invert_map` /
`compose_map`, which also let a caller fold a NIfTI transform into the map.

A map is (m[9] row-major, t[3]) float32: p_src = m * (x, y, z)_dst + t in voxel units, x fastest.  Shapes are torch's (d, h, w);
dims, as model.dim, are (w, h, d)."""
import ctypes as C
import math

import numpy as np
import torch

from . import engine as E
from .engine import UNetError


class UnetSpaceMap(C.Structure):
    _fields_ = [("m", C.c_float * 9), ("t", C.c_float * 3)]


E._sig("unet_space_scratch_bytes", C.c_int, C.c_int64, C.c_int, C.POINTER(C.c_size_t))
E._sig("unet_space_resample", C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
       C.POINTER(UnetSpaceMap), C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p)
E._sig("unet_space_postproc", C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(UnetSpaceMap), C.c_int, C.c_int,
       C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p)
# every symbol include/unet_space.h declares
EXPORTS = ["unet_space_scratch_bytes", "unet_space_resample", "unet_space_postproc"]

SPACE_LINEAR, SPACE_MAJORITY = 0, 1
MODES = {"linear": SPACE_LINEAR, "majority": SPACE_MAJORITY, SPACE_LINEAR: SPACE_LINEAR, SPACE_MAJORITY: SPACE_MAJORITY}
OUTPUTS = ("label_prob", "fg_prob", "label")


# ---- maps (host only) ------------------------------------------------------------------------------------------------------------
def _triple(v, name, positive=True):
    try:
        out = tuple(float(x) for x in v)
    except (TypeError, ValueError):
        raise UNetError("space: %s must be three numbers, got %r" % (name, v))
    if len(out) != 3 or not all(math.isfinite(x) and (x > 0 or not positive) for x in out):
        raise UNetError("space: %s must be three %s numbers, got %r" % (name, "positive finite" if positive else "finite", v))
    return out


def _dims(v, name):
    out = _triple(v, name)
    if any(x != int(x) for x in out):
        raise UNetError("space: %s must be whole numbers, got %r" % (name, v))
    return tuple(int(x) for x in out)


def _as_map(map):
    """(m, t) in any array form -> (float64 {3,3}, float64 {3})"""
    try:
        m, t = map
        m = np.asarray(m, dtype=np.float64).reshape(3, 3)
        t = np.asarray(t, dtype=np.float64).reshape(3)
    except (TypeError, ValueError):
        raise UNetError("space: a map is (m[9], t[3])")
    if not (np.isfinite(m).all() and np.isfinite(t).all()):
        raise UNetError("space: a map must be finite")
    return m, t


def _f32_map(m, t):
    return m.astype(np.float32).reshape(9), t.astype(np.float32)


def model_to_image_map(model_dim, model_vs, image_dim, image_vs):
    """The model -> image map of read_image_and_label (train.cpp:26-28) as (m[9], t[3]) float32; dims are (w, h, d), voxel sizes
    (x, y, z).  Per axis  p_image = (p_model - model_dim/2) * model_vs/image_vs + image_dim/2 + translocation/image_vs  with
    translocation = (0, 0, 0.5*((image_dim[2]-1)*image_vs[2] - (model_dim[2]-1)*model_vs[2])), in float64, rounded once.
    With equal voxel sizes it puts the model's last z-slice on the image's last z-slice and centres x and y: the model's default
    fov_strategy "align_top".  A stand-in for tipl::transformation_matrix: parity with TIPL is not pinned."""
    md, id_ = _dims(model_dim, "model_dim"), _dims(image_dim, "image_dim")
    mv, iv = _triple(model_vs, "model_vs"), _triple(image_vs, "image_vs")
    tl = (0.0, 0.0, 0.5 * ((id_[2] - 1) * iv[2] - (md[2] - 1) * mv[2]))
    m, t = np.zeros((3, 3)), np.zeros(3)
    for a in range(3):
        s = mv[a] / iv[a]
        m[a, a] = s
        t[a] = id_[a] / 2.0 - s * (md[a] / 2.0) + tl[a] / iv[a]
    return _f32_map(m, t)


def invert_map(map):
    """the inverse map (float64, rounded once); a singular matrix is refused"""
    m, t = _as_map(map)
    det = np.linalg.det(m)
    if not math.isfinite(det) or abs(det) <= 1e-12 * max(1.0, float(np.abs(m).max())) ** 3:
        raise UNetError("space: the map is singular")
    inv = np.linalg.inv(m)
    return _f32_map(inv, -inv @ t)


def compose_map(a, b):
    """the map p -> a(b(p)) (float64, rounded once): b takes the destination to a middle grid, a takes that to the source"""
    ma, ta = _as_map(a)
    mb, tb = _as_map(b)
    return _f32_map(ma @ mb, ma @ tb + ta)


def _map_struct(map):
    m, t = _as_map(map)
    s = UnetSpaceMap()
    s.m[:] = [float(v) for v in m.astype(np.float32).reshape(9)]
    s.t[:] = [float(v) for v in t.astype(np.float32)]
    return s


# ---- the device calls ------------------------------------------------------------------------------------------------------------
def space_scratch_bytes(dst_voxels, channels):
    return E.size_query(E.lib.unet_space_scratch_bytes, int(dst_voxels), int(channels))


def _f32(a, name):
    if not (torch.is_tensor(a) and a.is_cuda and a.dtype == torch.float32 and a.is_contiguous()):
        raise UNetError("space: %s must be a contiguous float32 device tensor" % name)
    return a


def _shape3(v, name):
    d, h, w = _dims(v, name)
    return d, h, w


def resample(src, dst_shape, map, mode="linear", normalize=False, out=None, scratch=None):
    """unet_space_resample on the current stream.  src: {C, d, h, w} (or {d, h, w}) contiguous fp32 device tensor; dst_shape:
    (D, H, W); map: destination voxel -> source position.  Returns {C, D, H, W} (or {D, H, W}).  normalize (linear only) divides
    the whole result by its maximum when that is > 0."""
    if mode not in MODES:
        raise UNetError("space: unknown mode %r (linear or majority)" % (mode,))
    mode = MODES[mode]
    if normalize and mode != SPACE_LINEAR:
        raise UNetError("space: normalize goes with linear only")
    ms = _map_struct(map)
    D, H, W = _shape3(dst_shape, "dst_shape")
    if _f32(src, "src").dim() not in (3, 4):
        raise UNetError("space: src must be a {C, d, h, w} or {d, h, w} tensor")
    ch = int(src.shape[0]) if src.dim() == 4 else 1
    sd, sh, sw = (int(v) for v in src.shape[-3:])
    shape = (ch, D, H, W) if src.dim() == 4 else (D, H, W)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=src.device)
    elif _f32(out, "out").numel() != ch * D * H * W or out.device != src.device:
        raise UNetError("space: out must hold %d values on the source's device" % (ch * D * H * W))
    sc_ptr, sc_bytes = None, 0
    if normalize:
        need = space_scratch_bytes(D * H * W, ch)
        scratch = E.scratch(scratch, need, src.device)
        sc_ptr, sc_bytes = scratch.data_ptr(), scratch.nbytes
    E.check(E.lib.unet_space_resample(src.data_ptr(), sw, sh, sd, out.data_ptr(), W, H, D, ch, C.byref(ms), mode, int(bool(normalize)),
                                      sc_ptr, sc_bytes, E.stream(src)))
    return out.view(shape)


def postproc_native(logits, map, native_shape, threshold=0.5, outputs=OUTPUTS, out=None):
    """unet_space_postproc on the current stream: softmax / create_mask / argmax of the model-grid logits ({C, D, H, W} or
    {1, C, D, H, W}, contiguous fp32 device tensor) evaluated on the native grid native_shape = (d, h, w); map: native voxel ->
    model position (invert_map of the model -> image map).  Returns {name: tensor} for the wanted outputs: label_prob {C-1, d, h, w}
    fp32, fg_prob {d, h, w} fp32, label {d, h, w} uint16.  out: {name: tensor} to write into instead of new ones."""
    outputs = tuple(outputs)
    for o in outputs:
        if o not in OUTPUTS:
            raise UNetError("unknown output %s (one of %s)" % (o, ", ".join(OUTPUTS)))
    if not outputs:
        raise UNetError("space: no output wanted")
    ms = _map_struct(map)
    d, h, w = _shape3(native_shape, "native_shape")
    if _f32(logits, "logits").dim() not in (4, 5) or (logits.dim() == 5 and logits.shape[0] != 1):
        raise UNetError("space: logits must be {C, D, H, W} of one volume")
    out_c, D, H, W = (int(v) for v in logits.shape[-4:])
    dev = logits.device
    shapes = {"label_prob": ((out_c - 1, d, h, w), torch.float32), "fg_prob": ((d, h, w), torch.float32), "label": ((d, h, w), torch.uint16)}
    res = {}
    for o in outputs:
        shape, dt = shapes[o]
        t = (out or {}).get(o)
        if t is None:
            t = torch.empty(shape, dtype=dt, device=dev)
        elif not (torch.is_tensor(t) and t.is_cuda and t.dtype == dt and t.is_contiguous() and t.numel() == int(np.prod(shape))
                  and t.device == dev):
            raise UNetError("space: out[%s] must be a contiguous %s tensor of %d values on the logits' device" % (o, dt, int(np.prod(shape))))
        res[o] = t
    ptr = lambda o: res[o].data_ptr() if o in res else None
    E.check(E.lib.unet_space_postproc(logits.data_ptr(), out_c, W, H, D, C.byref(ms), w, h, d, float(threshold), ptr("label_prob"),
                                      ptr("fg_prob"), ptr("label"), E.stream(logits)))
    return res


# ---- read_image_and_label after the file read --------------------------------------------------------------------------------------
def _check_image(model, image, label):
    """-> (d, h, w) of an {in_count, d, h, w} image (numpy or tensor) and its optional {d, h, w} label; host only"""
    shape = tuple(int(v) for v in getattr(image, "shape", ()))
    if len(shape) != 4 or shape[0] != model.in_count or min(shape) < 1:
        raise UNetError("space: image must be {in_count = %d, d, h, w}, got %s" % (model.in_count, shape))
    if label is not None and tuple(int(v) for v in getattr(label, "shape", ())) != shape[1:]:
        raise UNetError("space: label must be {d, h, w} = %s, got %s" % (shape[1:], tuple(getattr(label, "shape", ()))))
    return shape[1:]


def _to_device(a, device):
    if torch.is_tensor(a):
        return a.to(device=device, dtype=torch.float32).contiguous()
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(device)


def to_model_space(model, image, image_vs, label=None, map=None, scratch=None):
    """read_image_and_label (train.cpp:13-40) after the file read, on the model's device and the current stream.
    image: {in_count, d, h, w} at any size, numpy or device array, voxel size image_vs = (x, y, z); label: {d, h, w} or None.
    Returns (image' {in_count, D, H, W}, label' {D, H, W} or None) at model.dim: the image sampled linear and divided by its
    maximum (tipl::normalize of the whole buffer), the label sampled majority.  map overrides model_to_image_map(model.dim,
    model.voxel_size, (w, h, d), image_vs).  The caller's arrays are not written."""
    d, h, w = _check_image(model, image, label)
    vs = _triple(image_vs, "image_vs")
    W, H, D = _dims(model.dim, "model.dim")
    if map is None:
        map = model_to_image_map((W, H, D), model.voxel_size, (w, h, d), vs)
    else:
        map = _f32_map(*_as_map(map))
    dev = model.device()
    with torch.cuda.device(dev):
        img = resample(_to_device(image, dev), (D, H, W), map, "linear", normalize=True, scratch=scratch)
        lab = resample(_to_device(label, dev), (D, H, W), map, "majority") if label is not None else None
    return img, lab


class NativeVolume:
    """A `model_io` entry of EvaluateUNet on the scan's own grid: data, a float32 host buffer (in_count*d, h, w) (the input
    channels stacked along z, as the plain entries), with its voxel size (x, y, z).  map overrides the model -> image map."""

    def __init__(self, data, voxel_size, map=None):
        self.data = data
        self.voxel_size = voxel_size
        self.map = map
        self.check()

    def check(self):
        """host only; raises UNetError"""
        shape = tuple(int(v) for v in getattr(self.data, "shape", ()))
        if len(shape) != 3 or min(shape) < 1:
            raise UNetError("NativeVolume: data must be (in_count*d, h, w), got %s" % (shape,))
        _triple(self.voxel_size, "voxel_size")
        if self.map is not None:
            _as_map(self.map)
        return shape
