"""Training on windows of scans larger than the model's field of view: a patch feed (include/unet_patches.h).

EvaluateUNet(fov_strategy="tiles") covers such a scan with windows of model.dim (tiles.py); `WindowFeed` is the training-time
counterpart of that.  A case is kept on the device as a canvas (`to_canvas`: the scan at the model's voxel size, tiles.canvas_dims).
Per sample a window of model.dim is chosen, forced onto a voxel of a foreground class for a fraction of the samples, cut out on the
device, and handed to the tail of `feed.TrainingFeed` (simulate_modality, augmentation, target), which runs at model.dim as before.
The host decides the class from integer tables read once per case; where the window lies is decided on the device and never read
back.  The reference has no such code: the definitions (class, index, pick, draws) are this project's, written down in the header.

`draws`, `decide` and `test_windows` are host only.  `index`, `pick` and `crop` run the kernels on the current stream.  Shapes are
torch's (d, h, w); dims, as model.dim, are (w, h, d)."""
import ctypes as C

import numpy as np
import torch

from . import augment as G
from . import engine as E
from . import feed as FD
from . import qc as Q
from . import space as SP
from . import tiles as T
from .engine import UNetError

SEGMENT = 1024       # UNET_PATCHES_SEGMENT
MAX_CLASSES = 256    # UNET_PATCHES_MAX_CLASSES
MAX_PICKS = 32       # UNET_PATCHES_MAX_PICKS
# which draw of a sample (k of unet_patches_draws) decides what
DRAW_FOREGROUND, DRAW_CLASS, DRAW_RANK, DRAW_X, DRAW_Y, DRAW_Z = range(6)


class UnetPatchPick(C.Structure):
    _fields_ = [("cls", C.c_int32), ("u_rank", C.c_uint32), ("u_x", C.c_uint32), ("u_y", C.c_uint32), ("u_z", C.c_uint32)]


E._sig("unet_patches_index_bytes", C.c_int, C.c_int64, C.c_int, C.POINTER(C.c_size_t))
E._sig("unet_patches_index", C.c_int, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p)
E._sig("unet_patches_pick", C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
       C.POINTER(UnetPatchPick), C.c_int, C.c_void_p, C.c_void_p)
E._sig("unet_patches_crop", C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
       C.c_void_p, C.c_void_p, C.c_void_p)
E._sig("unet_patches_draws", C.c_int, C.c_uint64, C.c_uint64, C.c_uint32, C.c_int, C.POINTER(C.c_uint32))
# every symbol include/unet_patches.h declares
EXPORTS = ["unet_patches_index_bytes", "unet_patches_index", "unet_patches_pick", "unet_patches_crop", "unet_patches_draws"]

_U64 = 0xFFFFFFFFFFFFFFFF


# ---- the host rules --------------------------------------------------------------------------------------------------------------
def draws(seed, index, first_k, count):
    """unet_patches_draws -> uint32[count]: draw(seed, index, first_k + i), a pure function of its arguments"""
    if index < 0:
        raise UNetError("patches: sample index must not be negative")
    out = np.zeros(max(0, int(count)), dtype=np.uint32)
    E.check(E.lib.unet_patches_draws(int(seed) & _U64, int(index) & _U64, int(first_k), int(count),
                                     out.ctypes.data_as(C.POINTER(C.c_uint32))))
    return out


def check_foreground(foreground):
    try:
        num, den = (int(v) for v in foreground)
    except (TypeError, ValueError):
        raise UNetError("patches: foreground is a fraction (num, den) of whole numbers, got %r" % (foreground,))
    if den < 1 or not 0 <= num <= den or den >= 1 << 31:
        raise UNetError("patches: foreground (num, den) needs 0 <= num <= den, den >= 1, got %r" % (foreground,))
    return num, den


def decide(seed, index, fg_classes, foreground=(1, 3)):
    """The pick of sample `index`, in integers only -> (cls, u_rank, u_x, u_y, u_z).  The sample is forced onto the foreground when
    (u0 * den) >> 32 < num; its class is then fg_classes[(u1 * m) >> 32] of the case's m foreground classes (classes >= 1 with a
    voxel, ascending).  Otherwise, and always when m = 0, cls = -1: the window is drawn uniformly."""
    num, den = check_foreground(foreground)
    u = [int(v) for v in draws(seed, index, 0, 6)]
    m = len(fg_classes)
    forced = (u[DRAW_FOREGROUND] * den) >> 32 < num
    cls = int(fg_classes[(u[DRAW_CLASS] * m) >> 32]) if forced and m else -1
    return cls, u[DRAW_RANK], u[DRAW_X], u[DRAW_Y], u[DRAW_Z]


def test_windows(canvas_dim, model_dim):
    """[(ox, oy, oz), ...]: the windows of model_dim that cover a canvas without more overlap than its size asks for
    (tiles.plan_tiles, overlap 0), in tile-index order"""
    return T.tile_origins(T.plan_tiles(canvas_dim, model_dim, overlap=0))


# ---- the device calls ------------------------------------------------------------------------------------------------------------
def _f32(a, name):
    if not (torch.is_tensor(a) and a.is_cuda and a.dtype == torch.float32 and a.is_contiguous()):
        raise UNetError("patches: %s must be a contiguous float32 device tensor" % name)
    return a


def _i32(a, name, count):
    if not (torch.is_tensor(a) and a.is_cuda and a.dtype == torch.int32 and a.is_contiguous() and a.numel() >= count):
        raise UNetError("patches: %s must be a contiguous int32 device tensor of at least %d values" % (name, count))
    return a


def index_layout(voxels, classes):
    """(K, S): the classes and segments of an index; it holds K totals, then K rows of S exclusive prefixes"""
    nbytes = E.size_query(E.lib.unet_patches_index_bytes, int(voxels), int(classes))
    K = int(classes) if classes else 2
    return K, nbytes // (4 * K) - 1


def index(label, classes, out=None):
    """unet_patches_index on the current stream -> int32 device tensor {K + K*S} (include/unet_patches.h INDEX); classes: K >= 1
    for class labels, 0 for continuous labels (class 1 where l > 0)"""
    K, S = index_layout(_f32(label, "label").numel(), classes)
    if out is None:
        out = torch.empty(K + K * S, dtype=torch.int32, device=label.device)
    elif _i32(out, "out", K + K * S).device != label.device:
        raise UNetError("patches: out must live on the label's device")
    E.check(E.lib.unet_patches_index(label.data_ptr(), label.numel(), int(classes), out.data_ptr(), out.numel() * 4, E.stream(label)))
    return out


def _canvas(label, window):
    if _f32(label, "label").dim() != 3:
        raise UNetError("patches: label must be {d, h, w}, got %s" % (tuple(label.shape),))
    return tuple(int(v) for v in label.shape), SP._shape3(window, "window")


def pick(label, index, classes, picks, window, out=None):
    """unet_patches_pick on the current stream.  label {d, h, w} and its index; picks: up to 32 (cls, u_rank, u_x, u_y, u_z); window
    (td, th, tw).  Returns int32 device tensor {n, 4}: origin x, y, z and the flag (1: the class rule, 0: the uniform rule)."""
    (D, H, W), (td, th, tw) = _canvas(label, window)
    picks = list(picks)
    if not 1 <= len(picks) <= MAX_PICKS:
        raise UNetError("patches: 1 to %d picks per call, got %d" % (MAX_PICKS, len(picks)))
    arr = (UnetPatchPick * len(picks))(*[UnetPatchPick(*(int(v) for v in p)) for p in picks])
    if out is None:
        out = torch.empty((len(picks), 4), dtype=torch.int32, device=label.device)
    elif _i32(out, "out", 4 * len(picks)).device != label.device:
        raise UNetError("patches: out must live on the label's device")
    K, S = index_layout(label.numel(), classes)
    _i32(index, "index", K + K * S)
    E.check(E.lib.unet_patches_pick(label.data_ptr(), index.data_ptr(), int(classes), W, H, D, tw, th, td, arr, len(picks), out.data_ptr(),
                                    E.stream(label)))
    return out


def crop(image, label, origin, window, out=None):
    """unet_patches_crop on the current stream.  image {c, d, h, w}, label {d, h, w} or None; origin: int32 device tensor whose
    first three words are x, y, z (a row of pick's result; the kernel clamps it into the canvas); window (td, th, tw).  Returns
    (x {c, td, th, tw}, lab {td, th, tw} or None), fresh or the pair `out`."""
    if _f32(image, "image").dim() != 4:
        raise UNetError("patches: image must be {c, d, h, w}, got %s" % (tuple(image.shape),))
    ch, D, H, W = (int(v) for v in image.shape)
    td, th, tw = SP._shape3(window, "window")
    if label is not None and (tuple(_f32(label, "label").shape) != (D, H, W) or label.device != image.device):
        raise UNetError("patches: label must be {d, h, w} = %s on the image's device" % ((D, H, W),))
    _i32(origin, "origin", 3)
    x, lab = out if out is not None else (None, None)
    if x is None:
        x = torch.empty((ch, td, th, tw), dtype=torch.float32, device=image.device)
    elif _f32(x, "out x").numel() != ch * td * th * tw or x.device != image.device:
        raise UNetError("patches: out x must hold %d values on the image's device" % (ch * td * th * tw))
    if label is not None:
        if lab is None:
            lab = torch.empty((td, th, tw), dtype=torch.float32, device=image.device)
        elif _f32(lab, "out lab").numel() != td * th * tw or lab.device != image.device:
            raise UNetError("patches: out lab must hold %d values on the image's device" % (td * th * tw))
    E.check(E.lib.unet_patches_crop(image.data_ptr(), ch, label.data_ptr() if label is not None else None, W, H, D, tw, th, td,
                                    origin.data_ptr(), x.data_ptr(), lab.data_ptr() if label is not None else None, E.stream(image)))
    return x.view(ch, td, th, tw), (lab.view(td, th, tw) if label is not None else None)


# ---- a scan as a canvas case -------------------------------------------------------------------------------------------------------
def to_canvas(model, image, image_vs, label=None, scratch=None):
    """A scan of any size as a canvas case, on the model's device: image {in_count, d, h, w} (numpy or device array, voxel size
    image_vs) -> (image' {in_count, Dc, Hc, Wc}, label' {Dc, Hc, Wc} or None) on tiles.canvas_dims(model.dim, model.voxel_size, ...),
    the image sampled linear and divided by its maximum over the whole canvas, the label sampled majority.  A scan that fits
    model.dim gives space.to_model_space's result."""
    d, h, w = SP._check_image(model, image, label)
    vs = SP._triple(image_vs, "image_vs")
    Wc, Hc, Dc = T.canvas_dims(model.dim, model.voxel_size, (w, h, d), vs)
    if Wc * Hc * Dc >= 1 << 31:
        raise UNetError("patches: a canvas of %d x %d x %d has 2^31 voxels or more" % (Wc, Hc, Dc))
    m = SP.model_to_image_map((Wc, Hc, Dc), model.voxel_size, (w, h, d), vs)
    dev = model.device()
    with torch.cuda.device(dev):
        img = SP.resample(SP._to_device(image, dev), (Dc, Hc, Wc), m, "linear", normalize=True, scratch=scratch)
        lab = SP.resample(SP._to_device(label, dev), (Dc, Hc, Wc), m, "majority") if label is not None else None
    return img, lab


# ---- the feed ----------------------------------------------------------------------------------------------------------------------
class WindowFeed(FD.TrainingFeed):
    """`TrainingFeed` over canvas cases: `feed(i)` -> (x fp32 {1,in,D,H,W}, t int64 {1,D,H,W}), a window of model.dim of the case
    that the schedule gives sample i, a pure function of i.

    cases: TrainingFeed's tuples (image_name, label_name, image {in_count, Dc, Hc, Wc}, label {Dc, Hc, Wc}, is_template), each at
    least model.dim on every axis (to_canvas makes them).  foreground = (num, den): the fraction of the samples whose window is put
    on a voxel of a foreground class (decide).  Per case the label is prepared once on the whole canvas (normalize, subject shift:
    elementwise, so a window holds the values TrainingFeed forms per sample) and indexed as read; the label maxima and the class
    totals of all cases are read in one host read at construction, the only one of the feed."""

    def __init__(self, model, cases, param, options=None, is_label=True, foreground=(1, 3)):
        self.model, self.param, self.options, self.is_label = model, param, options, bool(is_label)
        self.foreground = check_foreground(foreground)
        cases = list(cases)
        if not cases:
            raise UNetError("no image/label pairs found")
        W, H, D = (int(v) for v in model.dim)
        self.size, self.voxels = (D, H, W), D * H * W
        dev = model.device()
        self.device = dev
        self.cases = cases
        self.classes = int(model.out_count) if self.is_label else 0
        if self.classes > MAX_CLASSES:
            raise UNetError("patches: at most %d classes, out_count is %d" % (MAX_CLASSES, model.out_count))
        K = self.classes or 2
        images, labels = [], []
        for case in cases:
            ishape, lshape = (tuple(int(v) for v in getattr(a, "shape", ())) for a in (case[2], case[3]))
            if len(ishape) != 4 or ishape[0] != model.in_count or lshape != ishape[1:]:
                raise UNetError("patches: a case is image {in_count = %d, d, h, w} and label {d, h, w}, got %s and %s: %s"
                                % (model.in_count, ishape, lshape, case[0]))
            if any(c < t for c, t in zip(lshape, (D, H, W))):
                raise UNetError("patches: a canvas of %s is smaller than the model's %s (no padding): %s" % (lshape, (D, H, W), case[0]))
            if int(np.prod(lshape)) >= 1 << 31:
                raise UNetError("patches: a canvas of %s has 2^31 voxels or more: %s" % (lshape, case[0]))
            images.append(Q._to_device(case[2], dev))
            labels.append(Q._to_device(case[3], dev))
        self.templates = [i for i, c in enumerate(cases) if c[4]]
        self.subjects = [i for i, c in enumerate(cases) if not c[4]]
        self.has_subject_data = bool(self.subjects)
        if self.templates and model.out_count >= G.SIM_MAX_LABELS:
            raise UNetError("feed: simulate_modality takes labels up to %d; out_count is %d" % (G.SIM_MAX_LABELS - 1, model.out_count))
        self._sc = {}

        with torch.cuda.device(dev):
            first = {}
            for i, case in enumerate(cases):
                first.setdefault(case[1], i)
            # per case: [label max, K class totals], one buffer, one host read
            info = torch.empty((len(cases), 1 + K), dtype=torch.int32, device=dev)
            self._index = []
            for i, lab in enumerate(labels):
                FD.label_max(lab, out=info[i, :1], scratch=self._scratch("feed", FD.feed_scratch_bytes(lab.numel())))
                self._index.append(index(lab, self.classes))
                info[i, 1:].copy_(self._index[i][:K])
            host = info.cpu().tolist()   # the one host read
            by_name = {case[1]: host[first[case[1]]][0] for case in cases}
            plan_cases = [(c[0], c[1], None, c[1], c[4]) for c in cases]
            self.max_template_label, self.shifted = Q.label_plan(plan_cases, model.out_count, max_of=by_name.__getitem__)
            self.totals = [row[1:] for row in host]
            self.fg_classes = [[c for c in range(1, K) if row[c] > 0] for row in self.totals]
            # the label every window is cut from: normalized (!is_label) and shifted (a shifted subject) once, on the whole canvas
            self._prep = []
            for i, lab in enumerate(labels):
                shift = self.max_template_label if (not cases[i][4] and self.shifted[i]) else 0
                if shift or not self.is_label:
                    lab = FD.prepare(lab.clone(), images[i].view(-1), normalize=not self.is_label, shift_by=shift,
                                     scratch=self._scratch("feed", FD.feed_scratch_bytes(lab.numel())))
                self._prep.append(lab)
        self._images, self._labels = images, labels
        self._test = FD.choose_test_cases(cases)
        self._sched_case = np.zeros(0, np.int32)
        self._sched_tpl = np.zeros(0, bool)

    def pick_of(self, index):
        """(case position, the pick (cls, u_rank, u_x, u_y, u_z)) of sample `index`; host only"""
        i, _ = self._case_of(index)
        return i, decide(self.param.seed, index, self.fg_classes[i], self.foreground)

    def window(self, index):
        """(origin int32 {4} on the device: x, y, z, flag; x {1,in,D,H,W}; lab {D,H,W}): where sample `index`'s window lies and the
        raw crop, before the tail"""
        i, pk = self.pick_of(index)
        with torch.cuda.device(self.device):
            origin = pick(self._labels[i], self._index[i], self.classes, [pk], self.size)[0]
            x, lab = crop(self._images[i], self._prep[i], origin, self.size)
        return origin, x.view((1, self.model.in_count) + self.size), lab

    def __call__(self, index):
        _, is_template = self._case_of(index)
        _, x, lab = self.window(index)
        return self._finish(index, is_template, x, lab)

    def test_set(self):
        """(test_in, test_out) for Trainer.validate: every window of test_windows(canvas, model.dim) of the up to 2 test cases
        choose_test_cases picks, cut at integer origins, unaugmented; the target as TrainingFeed.test_set makes it (the label
        normalized by its maximum over the canvas when out_count == 1, cast to int64)"""
        D, H, W = self.size
        test_in, test_out = [], []
        with torch.cuda.device(self.device):
            for i in self._test:
                lab = self._labels[i]
                Dc, Hc, Wc = (int(v) for v in lab.shape)
                sc = self._scratch("feed", FD.feed_scratch_bytes(max(lab.numel(), self.voxels)))
                if self.model.out_count == 1:
                    lab = FD.prepare(lab.clone(), normalize=True, scratch=sc)
                for o in test_windows((Wc, Hc, Dc), (W, H, D)):
                    origin = torch.tensor(o, dtype=torch.int32, device=self.device)
                    x, l = crop(self._images[i], lab, origin, self.size)
                    test_in.append(x.view((1, self.model.in_count) + self.size))
                    test_out.append(FD.target(l, scratch=sc).view(1, D, H, W))
        return test_in, test_out
