"""The co-registration of two intensity images on the device (include/unet_coreg.h): what puts a second image of one subject (a
T2 / FLAIR beside a T1, an FA or SUV map beside the scan) on the scan's grid, for a model with in_count > 1 and for `stats`.

  code          a float32 volume as uint8 codes in [0, bins) over a range (lo, hi); a NaN becomes the code `bins`, "none"
  joint_hist    K joint code histograms (fixed code x nearest moving code, with a column for "outside or none"), one per map, from
                one pass over the fixed image
  scores        the integer mutual-information score of each histogram: N * MI in units of 2^-16 bit
  search        the centred pattern search of `register` over the 12 parameters of an affine map, entirely on the device: every
                iteration scores its up to 25 candidates from one pass, the host enqueues the launches and reads nothing back
  robust_range  the (lo, hi) two quantiles of an image span (the only host read of an alignment)
  align         range, codes, search from register.centre_init, and the moving image resampled onto the fixed grid; with `warp`, a
                lattice field fitted after the search (cowarp.fit) and the image resampled through map + field

In place of the reference's linear_cuda (evaluate.cpp:19-26, TIPL's affine registration; TIPL is not in the reference tree, so
these are this project's definitions and parity is NOT pinned).  Every choice is made on integers, the score included: the results
are pinned to the numpy restatements of tests/coreg_ref.py bit for bit.  IMPL_LDS gathers the counters in a block's LDS table,
IMPL_GLOBAL adds in global memory (the measured baseline and a second witness of the bits)."""
import ctypes as C

import numpy as np
import torch

from . import engine as E
from . import register as R
from . import space as SP
from . import start as STA
from . import stats as ST
from .engine import UNetError

_grid = (C.c_void_p, C.c_int, C.c_int, C.c_int)   # codes, w, h, d
_fp = C.POINTER(C.c_float)
E._sig("unet_coreg_scratch_bytes", C.c_int, C.c_int64, C.c_int, C.c_int, C.POINTER(C.c_size_t))
E._sig("unet_coreg_code", C.c_int, C.c_void_p, C.c_int64, C.c_float, C.c_float, C.c_int, C.c_void_p, C.c_void_p)
E._sig("unet_coreg_hist", C.c_int, *_grid, *_grid, C.c_int, _fp, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p)
E._sig("unet_coreg_score", C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p)
E._sig("unet_coreg_search", C.c_int, *_grid, *_grid, C.c_int, _fp, _fp, C.POINTER(C.c_int), C.c_int, C.c_int, C.c_void_p, C.c_void_p,
       C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p)
# every symbol include/unet_coreg.h declares
EXPORTS = ["unet_coreg_scratch_bytes", "unet_coreg_code", "unet_coreg_hist", "unet_coreg_score", "unet_coreg_search"]

IMPL_DEFAULT, IMPL_LDS, IMPL_GLOBAL = 0, 1, 2
MAX_BINS, MAX_MAPS, MAX_STAGES, MAX_LEVEL, MAX_ITERATIONS = 32, 25, 4, 20, 1024
BINS = (8, 16, 32)
DEFAULT_STEP = [0.08] * 9 + [4, 4, 4]
DEFAULT_STAGES = [(2, 0, 3), (1, 1, 6)]


def coreg_scratch_bytes(fixed_voxels, bins, max_iterations=1):
    return E.size_query(E.lib.unet_coreg_scratch_bytes, int(fixed_voxels), int(bins), int(max_iterations))


def _floats(a):
    return a.ctypes.data_as(_fp)


def _bins(bins, who):
    if isinstance(bins, bool) or bins not in BINS:
        raise UNetError("coreg.%s: bins must be 8, 16 or 32, got %r" % (who, bins))
    return int(bins)


def _image(t, name, who, dev=None):
    if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.dim() == 3 and t.numel() > 0
            and (dev is None or t.device == dev)):
        raise UNetError("coreg.%s: %s must be a contiguous (D, H, W) float32 device tensor%s"
                        % (who, name, "" if dev is None else " on the fixed image's device"))
    return t


def _codes(t, name, who, dev=None):
    if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous() and t.dim() == 3 and t.numel() > 0
            and (dev is None or t.device == dev)):
        raise UNetError("coreg.%s: %s must be a contiguous (D, H, W) uint8 device tensor of codes%s"
                        % (who, name, "" if dev is None else " on the fixed image's device"))
    d, h, w = (int(v) for v in t.shape)
    return (t.data_ptr(), w, h, d)


def code(image, lo, hi, bins=16, out=None, stream=None):
    """unet_coreg_code on the current stream (or the raw `stream`).  image: a contiguous float32 device tensor; returns uint8 of its
    shape on the device (written into `out` when given): 0 below lo, bins - 1 from the last bin on, `bins` for a NaN.  No host
    synchronisation."""
    if not (torch.is_tensor(image) and image.is_cuda and image.dtype == torch.float32 and image.is_contiguous() and image.numel() > 0):
        raise UNetError("coreg.code: image must be a contiguous float32 device tensor")
    b = _bins(bins, "code")
    codes = R._out(out, image.numel(), torch.uint8, image.device, "out", "code", "coreg")
    E.check(E.lib.unet_coreg_code(image.data_ptr(), image.numel(), float(lo), float(hi), b, codes.data_ptr(), E.stream(image, stream)))
    return codes.view(image.shape)


def joint_hist(fixed, moving, bins, maps, stride=1, impl=IMPL_DEFAULT, out=None, stream=None):
    """unet_coreg_hist on the current stream (or the raw `stream`).  fixed, moving: (D, H, W) uint8 device tensors of codes; maps:
    K maps, {K, 12} numbers (m[9] then t[3]), fixed voxel -> moving position.  Returns uint32 {K, bins, bins + 1} on the device
    (written into `out` when given); the last column counts the samples outside the moving grid or without a code.  No host
    synchronisation."""
    fg = _codes(fixed, "fixed", "joint_hist")
    mg = _codes(moving, "moving", "joint_hist", fixed.device)
    b = _bins(bins, "joint_hist")
    try:
        flat = np.ascontiguousarray(np.asarray(maps, np.float32).reshape(-1, 12))
    except (TypeError, ValueError):
        raise UNetError("coreg.joint_hist: maps must be {K, 12} numbers")
    K = int(flat.shape[0])
    if not 1 <= K <= MAX_MAPS:
        raise UNetError("coreg.joint_hist: K must be in [1, %d], got %d" % (MAX_MAPS, K))
    hist = R._out(out, K * b * (b + 1), torch.uint32, fixed.device, "out", "joint_hist", "coreg")
    E.check(E.lib.unet_coreg_hist(*fg, *mg, b, _floats(flat), K, int(stride), hist.data_ptr(), int(impl), None, 0, E.stream(fixed, stream)))
    return hist.view(K, b, b + 1)


def scores(hist, out=None, stream=None):
    """unet_coreg_score on the current stream (or the raw `stream`).  hist: uint32 {K, bins, bins + 1} on the device.  Returns int64
    {K} on the device: N times the mutual information of each table, in units of 2^-16 bit.  No host synchronisation."""
    if not (torch.is_tensor(hist) and hist.is_cuda and hist.dtype == torch.uint32 and hist.is_contiguous() and hist.dim() == 3
            and hist.shape[1] in BINS and hist.shape[2] == hist.shape[1] + 1 and 1 <= hist.shape[0] <= MAX_MAPS):
        raise UNetError("coreg.scores: hist must be a contiguous uint32 {K, bins, bins + 1} device tensor, K in [1, %d]" % MAX_MAPS)
    K, b = int(hist.shape[0]), int(hist.shape[1])
    res = R._out(out, K, torch.int64, hist.device, "out", "scores", "coreg")
    E.check(E.lib.unet_coreg_score(hist.data_ptr(), K, b, res.data_ptr(), E.stream(hist, stream)))
    return res


def search(fixed, moving, bins, init, step=DEFAULT_STEP, stages=DEFAULT_STAGES, max_iterations=400, impl=IMPL_DEFAULT, trace=True,
           scratch=None, stream=None):
    """unet_coreg_search on the current stream (or the raw `stream`).  fixed, moving: codes; init: the map to start from; step: 12
    numbers (0 freezes a parameter); stages: (stride, first_level, last_level) triples.  Returns device tensors: map float32 {12},
    trace int64 {max_iterations, 4} (None with trace=False), info int64 {4} = (iterations, converged, score, stage of the last
    iteration).  No host synchronisation."""
    fg = _codes(fixed, "fixed", "search")
    mg = _codes(moving, "moving", "search", fixed.device)
    b = _bins(bins, "search")
    m0 = R._map12(init, "search")
    try:
        st = np.ascontiguousarray(np.asarray(step, np.float32).reshape(12))
        sl = np.ascontiguousarray(np.asarray(stages, np.int32).reshape(-1, 3))
    except (TypeError, ValueError):
        raise UNetError("coreg.search: step must be 12 numbers and stages (stride, first_level, last_level) triples")
    n_it, dev = int(max_iterations), fixed.device
    need = coreg_scratch_bytes(fixed.numel(), b, n_it)               # the range checks, before any device work
    scratch = E.scratch(scratch, need, dev)
    map_out = torch.empty(12, dtype=torch.float32, device=dev)
    tr = torch.empty((n_it, 4), dtype=torch.int64, device=dev) if trace else None
    info = torch.empty(4, dtype=torch.int64, device=dev)
    E.check(E.lib.unet_coreg_search(*fg, *mg, b, _floats(m0), _floats(st), sl.ctypes.data_as(C.POINTER(C.c_int)), int(sl.shape[0]), n_it,
                                    map_out.data_ptr(), tr.data_ptr() if trace else None, info.data_ptr(), int(impl), scratch.data_ptr(),
                                    scratch.nbytes, E.stream(fixed, stream)))
    return map_out, tr, info


def robust_range(image, permille=(10, 990)):
    """(lo, hi) as Python floats, in image units: the two quantiles of a float32 device volume, taken as 16-bit codes over its exact
    range (stats.volume_range, stats.quantiles without a label map) and read as the centres of those codes.  SYNCHRONISES with the
    host twice (the range, then the two codes): the only host reads of an alignment."""
    try:
        p = tuple(permille)
    except TypeError:
        p = ()
    if len(p) != 2:
        raise UNetError("coreg.robust_range: permille must be two integers in [0, 1000], the lower first")
    vmin, vmax = ST.volume_range(image)
    if not (np.isfinite(vmin) and np.isfinite(vmax) and vmin < vmax):
        raise UNetError("coreg.robust_range: the image must hold two different finite values (its range is %r .. %r)" % (vmin, vmax))
    q = ST.quantiles(None, image, 0, vmin, vmax, permille=p).cpu().numpy()[0]
    lo, hi = (float(v) for v in ST.code_value(q, vmin, vmax))
    if not lo < hi:
        raise UNetError("coreg.robust_range: the quantiles %r of the image coincide at %r" % (p, lo))
    return lo, hi


def align(moving, moving_vs, fixed, fixed_vs, bins=16, init=None, step=DEFAULT_STEP, stages=DEFAULT_STAGES, max_iterations=400,
          impl=IMPL_DEFAULT, starts=None, warp=None, geometry=None):
    """The moving image on the fixed image's grid.  moving, fixed: (D, H, W) float32 device tensors of one subject, voxel sizes
    (x, y, z).  In order: robust_range and code of both images; the start, register.centre_init(fixed.shape, fixed_vs, moving.shape,
    moving_vs) unless `init` (a map, fixed voxel -> moving position) is given; search; the moving image resampled through the map
    found, linearly.

    starts: a start.Plan(degrees, n, rank_stride).  The moments of the two code images (codes 1..bins-1) give start.candidates
    (the start above is only their fallback); one coreg.joint_hist per 25 of them at rank_stride and coreg.scores rank them; the n
    best (the unrotated one always among them) are read back once, n searches run one after another on the stream, and the best
    final state by start.best_of's key is taken from one readback of the n infos.  None: the single search, unchanged.

    warp: a cowarp.Plan(levels, limit, impl) refines the map non-linearly: after the search and the readback of the
    map, cowarp.fit runs on the two code images and cowarp.resample takes space.resample's place.  A fourth element is returned,
    dict(field int32 {nz, ny, nx, 3} on the last level's lattice, g its spacing, report int64 {cowarp.MAX_ROWS, 5}, score_affine
    and score_warped int64 {1} (N * MI before and after), max_disp_q8 int32 {}), all device tensors, not read here.  None: the
    3-tuple, from the same calls as before the keyword existed.

    geometry: a deform.Plan(jacobian, iters, impl), only with `warp`: deform.jacobian runs on the fitted field and
    the fourth element gains det (float32 on the fixed grid, None when the plan's jacobian is False), folded, det_min, det_max (int64
    {1} each, the extremes as deform.summary's keys), device tensors, not read here.  None: nothing of this runs.

    Returns (map float32 {12} on the device, info int64 {4} on the device = (iterations, converged, score, stage of the last
    iteration), moved float32 of fixed's shape).  The host reads the two ranges before the search and the 12 floats of the map
    after it (the resampling takes its map in the launch arguments)."""
    if warp is not None:
        from . import cowarp as CW
        from . import warp as W
        warp_levels, warp_limit, warp_impl = CW._plan(warp, "coreg.align")
    if geometry is not None:
        from . import deform as DF
        if warp is None:
            raise UNetError("coreg.align: geometry needs warp: there is no field without a fit")
        geo_det = DF._plan(geometry, "coreg.align")[0]
    _image(fixed, "fixed", "align")
    _image(moving, "moving", "align", fixed.device)
    b = _bins(bins, "align")
    if init is None:
        init = R.centre_init(tuple(fixed.shape), fixed_vs, tuple(moving.shape), moving_vs)
    m0 = R._map12(init, "align")
    fc = code(fixed, *robust_range(fixed), b)
    mc = code(moving, *robust_range(moving), b)
    if starts is None:
        map_dev, _, info = search(fc, mc, b, m0, step=step, stages=stages, max_iterations=max_iterations, impl=impl, trace=False)
    else:
        degrees, n, rank_stride = STA._plan(starts, "coreg.align")
        mom = torch.stack([STA.moments(fc, 1, b - 1), STA.moments(mc, 1, b - 1)]).cpu().numpy()
        maps = STA.candidates(mom[0], mom[1], degrees, fallback=m0)
        S = int(maps.shape[0])
        ranked = torch.cat([scores(joint_hist(fc, mc, b, maps[k:k + MAX_MAPS], stride=rank_stride, impl=impl))
                            for k in range(0, S, MAX_MAPS)]).cpu().numpy()
        order = sorted(range(S), key=lambda k: (-int(ranked[k]), k))[:min(n, S)]
        always = STA.ALWAYS if S > STA.ALWAYS else 0
        if always not in order:
            order[-1] = always
        runs = [search(fc, mc, b, maps[k], step=step, stages=stages, max_iterations=max_iterations, impl=impl, trace=False) for k in order]
        best = STA.best_of(torch.stack([r[2] for r in runs]).cpu().numpy())
        map_dev, info = runs[best][0], runs[best][2]
    m = map_dev.cpu().numpy()
    if warp is None:
        moved = SP.resample(moving, tuple(fixed.shape), (m[:9], m[9:]), mode="linear")
        return map_dev, info, moved
    levels = W.levels_of(warp_levels, warp_limit, m, "coreg.align")
    g0, g = int(levels[0, 0]), int(levels[-1, 0])
    zero = torch.zeros(W.lattice(tuple(fixed.shape), g0) + (3,), dtype=torch.int32, device=fixed.device)
    score_affine = scores(CW.hist(fc, mc, b, m, zero, g0).view(1, b, b + 1))
    field, report = CW.fit(fc, mc, b, m, levels=levels, impl=warp_impl)
    score_warped = scores(CW.hist(fc, mc, b, m, field, g).view(1, b, b + 1))
    moved = CW.resample(moving, tuple(fixed.shape), m, field, g)
    extra = dict(field=field, g=g, report=report, score_affine=score_affine, score_warped=score_warped, max_disp_q8=field.abs().max())
    if geometry is not None:
        det, det_info = DF.jacobian(tuple(fixed.shape), m, field, g, det=geo_det)
        extra.update(det=det, folded=det_info[1:2], det_min=det_info[2:3], det_max=det_info[3:4])
    return map_dev, info, moved, extra
