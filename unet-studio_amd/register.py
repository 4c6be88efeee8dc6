"""The parcellation of a subject on the device (include/unet_register.h), what `--template ... --atlas ...` exists for: the atlas's
regions on the subject's own grid.

  joint_hist   K joint tissue histograms (subject tissue x nearest template tissue), one per map, from one pass over the subject
  search       a centred pattern search over the 12 parameters of an affine map, entirely on the device: every iteration scores its
               up to 25 candidates from one pass, the host enqueues the launches and reads nothing back
  carry        the atlas brought onto the subject grid through a map: the nearest template voxel when its tissue agrees, else the
               mode of the agreeing voxels of the 3x3x3 cube around it
  parcellate   search from centre_init (or, with `starts`, the best of several searches from ranked starts: start.find), carry
               (with `warp`, through the lattice field warp.fit finds after the search), then atlas.grow on the subject grid for
               what carry left

In place of the reference's linear_cuda (evaluate.cpp:19-26, TIPL's affine registration; TIPL is not in the reference tree, so
these are this project's definitions and parity is NOT pinned).  Every choice is made on integer counts: the results are pinned to
the numpy restatements of tests/test_register_host.py bit for bit.  IMPL_LDS gathers the counters in a block's LDS table,
IMPL_GLOBAL adds in global memory (the measured baseline and a second witness of the bits)."""
import ctypes as C

import numpy as np
import torch

from . import engine as E
from .engine import UNetError

_grid = (C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int)   # tissue, bytes, w, h, d
_fp = C.POINTER(C.c_float)
E._sig("unet_reg_scratch_bytes", C.c_int, C.c_int64, C.c_int, C.c_int, C.POINTER(C.c_size_t))
E._sig("unet_reg_hist", C.c_int, *_grid, *_grid, C.c_int, _fp, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p)
E._sig("unet_reg_search", C.c_int, *_grid, *_grid, C.c_int, _fp, _fp, C.POINTER(C.c_int), C.c_int, C.c_int, C.c_void_p, C.c_void_p,
       C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p)
E._sig("unet_reg_carry", C.c_int, *_grid, *_grid, C.c_void_p, C.c_int, _fp, C.c_void_p, C.c_void_p, C.c_void_p)
# every symbol include/unet_register.h declares
EXPORTS = ["unet_reg_scratch_bytes", "unet_reg_hist", "unet_reg_search", "unet_reg_carry"]

IMPL_DEFAULT, IMPL_LDS, IMPL_GLOBAL = 0, 1, 2
MAX_TISSUES, MAX_MAPS, MAX_STAGES, MAX_LEVEL, MAX_ITERATIONS = 16, 25, 4, 20, 1024
DEFAULT_STEP = [0.125] * 9 + [4, 4, 4]
DEFAULT_STAGES = [(4, 0, 2), (2, 1, 4), (1, 2, 6)]


def reg_scratch_bytes(subject_voxels, n_tissues, max_iterations=1):
    return E.size_query(E.lib.unet_reg_scratch_bytes, int(subject_voxels), int(n_tissues), int(max_iterations))


def centre_init(subject_shape, subject_vs, template_shape, template_vs):
    """The map a search starts from, as (m[9], t[3]) float32: the matrix diag(subject_vs / template_vs), the translation that puts
    the subject's centre voxel (w // 2, h // 2, d // 2) on the template's.  Shapes are (D, H, W), voxel sizes (x, y, z); float32
    arithmetic, one rounding per operation."""
    try:
        sd, sh, sw = (int(v) for v in subject_shape)
        td, th, tw = (int(v) for v in template_shape)
        svs = np.asarray([float(v) for v in subject_vs], np.float32)
        tvs = np.asarray([float(v) for v in template_vs], np.float32)
    except (TypeError, ValueError):
        raise UNetError("register.centre_init: shapes must be (D, H, W) and voxel sizes (x, y, z)")
    if svs.shape != (3,) or tvs.shape != (3,) or not (np.all(np.isfinite(svs)) and np.all(np.isfinite(tvs)) and np.all(svs > 0) and np.all(tvs > 0)):
        raise UNetError("register.centre_init: voxel sizes must be three positive finite numbers")
    if min(sd, sh, sw, td, th, tw) < 1:
        raise UNetError("register.centre_init: shapes must be positive")
    scale = svs / tvs
    sc = np.asarray([sw // 2, sh // 2, sd // 2], np.float32)
    tc = np.asarray([tw // 2, th // 2, td // 2], np.float32)
    return np.diag(scale).astype(np.float32).reshape(9), (tc - scale * sc).astype(np.float32)


def _map12(map, who):
    """(m, t) or 12 numbers -> float32 {12}"""
    try:
        if len(map) == 2:
            flat = np.concatenate([np.asarray(map[0], np.float32).reshape(9), np.asarray(map[1], np.float32).reshape(3)])
        else:
            flat = np.asarray(map, np.float32).reshape(12)
    except (TypeError, ValueError):
        raise UNetError("register.%s: a map is (m[9], t[3]) or 12 numbers" % who)
    return np.ascontiguousarray(flat)


def _floats(a):
    return a.ctypes.data_as(_fp)


def _tissue(t, name, who, dev=None):
    if not (torch.is_tensor(t) and t.is_cuda and t.dtype in (torch.uint8, torch.uint16) and t.is_contiguous() and t.dim() == 3 and t.numel() > 0
            and (dev is None or t.device == dev)):
        raise UNetError("register.%s: %s must be a contiguous (D, H, W) uint8 or uint16 device tensor%s"
                        % (who, name, "" if dev is None else " on the subject's device"))
    d, h, w = (int(v) for v in t.shape)
    return (t.data_ptr(), t.element_size(), w, h, d)


def _out(out, n, dtype, dev, name, who, mod="register"):
    """the output tensor of `mod`.`who` (coreg, cowarp and deform name themselves): a new one, or the caller's `name`, checked"""
    if out is None:
        return torch.empty(n, dtype=dtype, device=dev)
    if not (torch.is_tensor(out) and out.is_cuda and out.device == dev and out.is_contiguous() and out.dtype == dtype and out.numel() == n):
        raise UNetError("%s.%s: %s must be a contiguous %s device tensor of %d entries" % (mod, who, name, dtype, n))
    return out


def joint_hist(subject, template, n_tissues, maps, stride=1, impl=IMPL_DEFAULT, out=None, stream=None):
    """unet_reg_hist on the current stream (or the raw `stream`).  subject, template: (D, H, W) uint8 or uint16 device tensors;
    maps: K maps, {K, 12} numbers (m[9] then t[3]).  Returns uint32 {K, n_tissues, n_tissues} on the device (written into `out`
    when given).  No host synchronisation."""
    sg = _tissue(subject, "subject", "joint_hist")
    tg = _tissue(template, "template", "joint_hist", subject.device)
    try:
        flat = np.ascontiguousarray(np.asarray(maps, np.float32).reshape(-1, 12))
    except (TypeError, ValueError):
        raise UNetError("register.joint_hist: maps must be {K, 12} numbers")
    K, T = int(flat.shape[0]), int(n_tissues)
    if not (1 <= K <= MAX_MAPS and 2 <= T <= MAX_TISSUES):
        raise UNetError("register.joint_hist: K must be in [1, %d] and n_tissues in [2, %d], got %d and %d" % (MAX_MAPS, MAX_TISSUES, K, T))
    hist = _out(out, K * T * T, torch.uint32, subject.device, "out", "joint_hist")
    E.check(E.lib.unet_reg_hist(*sg, *tg, T, _floats(flat), K, int(stride), hist.data_ptr(), int(impl), None, 0, E.stream(subject, stream)))
    return hist.view(K, T, T)


def search(subject, template, n_tissues, init, step=DEFAULT_STEP, stages=DEFAULT_STAGES, max_iterations=400, impl=IMPL_DEFAULT,
           trace=True, scratch=None, stream=None):
    """unet_reg_search on the current stream (or the raw `stream`).  init: the map to start from; step: 12 numbers (0 freezes a
    parameter); stages: (stride, first_level, last_level) triples.  Returns device tensors: map float32 {12}, trace int64
    {max_iterations, 4} (None with trace=False), info int64 {4} = (iterations, converged, score, stage of the last iteration).  No
    host synchronisation."""
    sg = _tissue(subject, "subject", "search")
    tg = _tissue(template, "template", "search", subject.device)
    m0 = _map12(init, "search")
    try:
        st = np.ascontiguousarray(np.asarray(step, np.float32).reshape(12))
        sl = np.ascontiguousarray(np.asarray(stages, np.int32).reshape(-1, 3))
    except (TypeError, ValueError):
        raise UNetError("register.search: step must be 12 numbers and stages (stride, first_level, last_level) triples")
    T, n_it, dev = int(n_tissues), int(max_iterations), subject.device
    need = reg_scratch_bytes(subject.numel(), T, n_it)               # the range checks, before any device work
    scratch = E.scratch(scratch, need, dev)
    map_out = torch.empty(12, dtype=torch.float32, device=dev)
    tr = torch.empty((n_it, 4), dtype=torch.int64, device=dev) if trace else None
    info = torch.empty(4, dtype=torch.int64, device=dev)
    E.check(E.lib.unet_reg_search(*sg, *tg, T, _floats(m0), _floats(st), sl.ctypes.data_as(C.POINTER(C.c_int)), int(sl.shape[0]), n_it,
                                  map_out.data_ptr(), tr.data_ptr() if trace else None, info.data_ptr(), int(impl), scratch.data_ptr(),
                                  scratch.nbytes, E.stream(subject, stream)))
    return map_out, tr, info


def carry(subject, template, atlas, n_tissues, map, counts=True, out=None, stream=None):
    """unet_reg_carry on the current stream (or the raw `stream`).  atlas: a contiguous uint16 device tensor on the template grid.
    Returns (regions uint16 on the subject grid, counts uint32 {3, n_tissues} = direct, rescued, left per tissue, or None).  No host
    synchronisation."""
    sg = _tissue(subject, "subject", "carry")
    tg = _tissue(template, "template", "carry", subject.device)
    if not (torch.is_tensor(atlas) and atlas.is_cuda and atlas.device == subject.device and atlas.dtype == torch.uint16 and atlas.is_contiguous()
            and atlas.numel() == template.numel()):
        raise UNetError("register.carry: atlas must be a contiguous uint16 device tensor on the template grid")
    T = int(n_tissues)
    if not 2 <= T <= MAX_TISSUES:
        raise UNetError("register.carry: n_tissues must be in [2, %d], got %d" % (MAX_TISSUES, T))
    m = _map12(map, "carry")
    regions = _out(out, subject.numel(), torch.uint16, subject.device, "out", "carry")
    cnt = torch.empty(3 * T, dtype=torch.uint32, device=subject.device) if counts else None
    E.check(E.lib.unet_reg_carry(*sg, *tg, atlas.data_ptr(), T, _floats(m), regions.data_ptr(), cnt.data_ptr() if counts else None,
                                 E.stream(subject, stream)))
    return regions.view(subject.shape), (cnt.view(3, T) if counts else None)


class Atlas:
    """What atlas.prepare_atlas leaves for an evaluation (EvaluateUNet's `atlas`): the template's tissue map and the corrected atlas
    on its grid, as device tensors, and the template's voxel size (x, y, z).  n_regions: the atlas's largest id; None reads it from
    the atlas once, here (a host synchronisation)."""

    def __init__(self, template, template_vs, regions, n_tissues=5, n_regions=None):
        if not (torch.is_tensor(template) and template.is_cuda and template.dtype in (torch.uint8, torch.uint16) and template.dim() == 3
                and template.is_contiguous() and template.numel() > 0):
            raise UNetError("register.Atlas: template must be a contiguous (D, H, W) uint8 or uint16 device tensor")
        if not (torch.is_tensor(regions) and regions.is_cuda and regions.device == template.device and regions.dtype == torch.uint16
                and regions.is_contiguous() and tuple(regions.shape) == tuple(template.shape)):
            raise UNetError("register.Atlas: regions must be a contiguous uint16 device tensor of the template's shape, on its device")
        try:
            vs = tuple(float(v) for v in template_vs)
        except (TypeError, ValueError):
            vs = ()
        if len(vs) != 3 or not all(np.isfinite(v) and v > 0 for v in vs):
            raise UNetError("register.Atlas: template_vs must be three positive finite numbers")
        if isinstance(n_tissues, bool) or int(n_tissues) != n_tissues or not 2 <= int(n_tissues) <= MAX_TISSUES:
            raise UNetError("register.Atlas: n_tissues must be in [2, %d], got %r" % (MAX_TISSUES, n_tissues))
        if n_regions is None:
            n_regions = max(int(regions.to(torch.int32).max().item()), 1)
        if isinstance(n_regions, bool) or int(n_regions) != n_regions or not 1 <= int(n_regions) <= 65535:
            raise UNetError("register.Atlas: n_regions must be in [1, 65535], got %r" % (n_regions,))
        self.template, self.template_vs, self.regions = template, vs, regions
        self.n_tissues, self.n_regions = int(n_tissues), int(n_regions)
        self._moments = None

    def moments(self):
        """The template's foreground moments (start.moments over tissues 1..n_tissues-1) as 10 host integers: a constant of the
        atlas, read from the device once (a host synchronisation) and kept."""
        if self._moments is None:
            from . import start as ST
            self._moments = ST.moments(self.template, 1, self.n_tissues - 1).cpu().numpy()
        return self._moments


def parcellate(subject_tissue, subject_vs, template, template_vs, atlas, n_tissues=5, init=None, step=DEFAULT_STEP, stages=DEFAULT_STAGES,
               max_iterations=400, max_rounds=None, smooth_rounds=1, impl=IMPL_DEFAULT, starts=None, template_moments=None, warp=None, geometry=None):
    """The atlas's regions on the subject's grid.  subject_tissue: the subject's tissue map (an evaluation's label output), template:
    the template's, atlas: the corrected atlas on the template grid (atlas.prepare_atlas); (D, H, W) device tensors, voxel sizes
    (x, y, z).  search from `init` (centre_init when None), carry, then atlas.grow on the subject grid with the subject tissue as
    the tissue map, tissues 1..n_tissues-1 flagged, CLAMP | PRESERVE: the regions grow into what carry left.

    starts: a start.Plan(degrees, n, rank_stride) replaces the single search with start.find (the best of n searches from starts
    ranked among the moments-and-rotations candidates; `init`, when given, is only the fallback for moments that say nothing);
    template_moments: the template's start.moments when the caller has them (Atlas.moments()).  None: the single search, unchanged.

    warp: a warp.Plan(levels, limit) refines the map non-linearly: warp.fit runs after the search on the map read
    back at synchronisation 1, and warp.carry takes carry's place.  The report gains warp = dict(levels int32 {n, 5}, report (the
    rows of the schedule), score_affine, score_warped, max_disp_q8).  None: today's calls, unchanged.

    geometry: a deform.Plan(jacobian, iters, impl), only with `warp`: deform.jacobian runs on the fitted field and
    the report gains geometry = dict(field int32 {nz, ny, nx, 3} and det float32 on the subject grid (device tensors; det is None
    when the plan's jacobian is False), g the field's spacing, folded, det_min, det_max, iters, impl): what `to_template` pulls
    with.  Its info travels in the final readback: no further host synchronisation.  None: nothing of this runs.

    Returns (regions uint16 on the subject grid, report) with report = dict(map (m[9], t[3]) float32, iterations, converged, score,
    direct, rescued, left, filled (uint32 {n_tissues} each), rounds, grow_converged); with `starts` also starts = start.report's
    dict, and iterations, converged and score are the best state's.  With `starts` the host also waits once for the subject's
    moments before the searches.

    Two host synchronisations: the 12 floats of the map after the search (carry's map travels in its launch arguments), and the
    reports, read back once at the end."""
    from . import atlas as A
    T = int(n_tissues)
    if warp is not None:
        from . import warp as W
        warp_levels, warp_limit = W._plan(warp, "register.parcellate")
    if geometry is not None:
        from . import deform as DF
        if warp is None:
            raise UNetError("register.parcellate: geometry needs warp: there is no field without a fit")
        geo_det, geo_iters, geo_impl = DF._plan(geometry, "register.parcellate")
    if init is None:
        if not (torch.is_tensor(subject_tissue) and torch.is_tensor(template)):
            raise UNetError("register.parcellate: subject_tissue and template must be device tensors")
        init = centre_init(tuple(subject_tissue.shape), subject_vs, tuple(template.shape), template_vs)
    pending = None
    if starts is not None:
        from . import start as ST
        degrees, n, rank_stride = ST._plan(starts, "register.parcellate")
        map_dev, pending = ST.find(subject_tissue, template, T, template_moments=template_moments, degrees=degrees, n=n,
                                   rank_stride=rank_stride, step=step, stages=stages, max_iterations=max_iterations, fallback=init)
    else:
        map_dev, _, info = search(subject_tissue, template, T, init, step=step, stages=stages, max_iterations=max_iterations, impl=impl,
                                  trace=False)
    m = map_dev.cpu().numpy()                                         # host synchronisation 1
    if warp is None:
        regions, counts = carry(subject_tissue, template, atlas, T, m)
    else:
        levels = W.levels_of(warp_levels, warp_limit, m, "register.parcellate")
        field, rows = W.fit(subject_tissue, template, T, m, levels=levels)
        regions, counts = W.carry(subject_tissue, template, atlas, T, m, field, int(levels[-1, 0]))
        affine_hist, max_disp = joint_hist(subject_tissue, template, T, [m]), field.abs().amax()
        if geometry is not None:
            det, det_info = DF.jacobian(tuple(subject_tissue.shape), m, field, int(levels[-1, 0]), det=geo_det)
    g = A.grow(subject_tissue, regions, T, list(range(1, T)), flags=A.CLAMP | A.PRESERVE, max_rounds=max_rounds, smooth_rounds=smooth_rounds)

    def u32(t):
        return t.view(torch.int32).cpu().numpy().view(np.uint32)

    found = None
    if pending is not None:
        found = ST.report(pending)
        info_h = found["info"][found["best"]]
    else:
        info_h = info.cpu().numpy()
    counts_h, filled, ginfo = u32(counts), u32(g["filled"]), u32(g["info"])                                   # 2
    report = dict(map=(m[:9].copy(), m[9:].copy()), iterations=int(info_h[0]), converged=bool(info_h[1]), score=int(info_h[2]),
                  direct=counts_h[0], rescued=counts_h[1], left=counts_h[2], filled=filled, rounds=int(ginfo[0]),
                  grow_converged=bool(ginfo[1]))
    if found is not None:
        report["starts"] = found
    if warp is not None:
        rows_h = rows.cpu().numpy()
        rows_h = rows_h[rows_h[:, 0] >= 0]
        report["warp"] = dict(levels=levels, report=rows_h, score_affine=W.score(u32(affine_hist)[0]), score_warped=int(rows_h[-1, 4]),
                              max_disp_q8=int(max_disp.cpu()))
    if geometry is not None:
        d = DF.summary(det_info)
        report["geometry"] = dict(field=field, g=int(levels[-1, 0]), det=det, folded=d["folded"], det_min=d["det_min"], det_max=d["det_max"],
                                  iters=geo_iters, impl=geo_impl)
    return regions, report


def to_template(volume, report, template_shape, kind=None, iters=None, pos=False):
    """A subject-grid volume on the template grid, through the inverse of what `parcellate(warp=, geometry=)` found: deform.pull with
    report["map"] and report["geometry"]'s field.  volume: a (D, H, W) device tensor of the subject's shape, float32 (trilinear) or
    uint8 / uint16 (labels, tissue maps, regions: nearest); kind: None takes it from the dtype, otherwise deform.KIND_F32 / _U8 /
    _U16, which the dtype must match; iters: None takes the plan's.  Returns deform.pull's (out, pos, info); no host
    synchronisation."""
    from . import deform as DF
    try:
        geo, m = report["geometry"], report["map"]
        field, g = geo["field"], geo["g"]
        iters = geo["iters"] if iters is None else iters
        impl = geo["impl"]
    except (KeyError, TypeError):
        raise UNetError("register.to_template: report must be parcellate's with warp= and geometry=")
    if kind is not None and (not torch.is_tensor(volume) or DF._KINDS.get(volume.dtype) != kind):
        raise UNetError("register.to_template: kind %r does not match the volume's dtype" % (kind,))
    return DF.pull(volume, template_shape, m, field, g, iters=iters, pos=pos, impl=impl)
