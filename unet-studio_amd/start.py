"""The starts of a registration on the device (include/unet_start.h): where `register.search` (and, through `coreg.align`, the
search over intensity codes) begins.  That search is local; from `register.centre_init` it stalls on a subject rotated by more than a
few degrees or off the middle of its field of view.

  moments      the ten raw moments of a volume's foreground, from one pass
  candidates   host arithmetic: the 27 starts of two moment sets, centroids and per-axis scales with a 3 x 3 x 3 grid of rotations
  rank         the joint histograms of S starts at a coarse stride (register.joint_hist in passes of 25)
  pick         their scores and the n starts to search from: the n best, the unrotated start always among them
  search       n <= 4 searches over the same two tissue maps advancing in lock-step inside the same launches (IMPL_BATCHED), or one
               after another through register's own entry point (IMPL_SEQUENTIAL: the yardstick and the second witness); the best
               FINAL state and its map
  find         moments -> candidates -> rank -> pick -> search
  Plan         what `register.parcellate(starts=...)`, `EvaluateUNet(atlas_starts=...)` and `coreg.align(starts=...)` take

All device work is integer counting or fp32 with every operation rounded: pinned to the numpy restatements of tests/start_ref.py bit
for bit."""
import collections
import ctypes as C
import itertools
import math

import numpy as np
import torch

from . import engine as E
from . import register as R
from .engine import UNetError

_grid = (C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int)   # tissue, bytes, w, h, d
_fp = C.POINTER(C.c_float)
E._sig("unet_start_scratch_bytes", C.c_int, C.c_int, C.c_int, C.POINTER(C.c_size_t))
E._sig("unet_start_moments", C.c_int, *_grid, C.c_int, C.c_int, C.c_void_p, C.c_void_p)
E._sig("unet_start_pick", C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p)
E._sig("unet_start_search", C.c_int, *_grid, *_grid, C.c_int, C.c_void_p, C.c_int, _fp, C.POINTER(C.c_int), C.c_int, C.c_int, C.c_void_p,
       C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p)
# every symbol include/unet_start.h declares
EXPORTS = ["unet_start_scratch_bytes", "unet_start_moments", "unet_start_pick", "unet_start_search"]

IMPL_DEFAULT, IMPL_BATCHED, IMPL_SEQUENTIAL = 0, 1, 2
MAX_STATES, MAX_STARTS, MAX_DIM = 4, 125, 65535
ALWAYS = 13                                                 # the unrotated start of candidates()

Plan = collections.namedtuple("Plan", ("degrees", "n", "rank_stride"), defaults=(12.0, 4, 2))
Plan.__doc__ = "How a registration finds its start: the rotation grid's angle in degrees, the searches run, the stride of the ranking."


def start_scratch_bytes(n_tissues, n=MAX_STATES):
    return E.size_query(E.lib.unet_start_scratch_bytes, int(n_tissues), int(n))


def _plan(plan, who):
    try:
        degrees, n, stride = float(plan.degrees), int(plan.n), int(plan.rank_stride)
    except (AttributeError, TypeError, ValueError):
        raise UNetError("%s: starts must be a start.Plan(degrees, n, rank_stride)" % who)
    if not (math.isfinite(degrees) and 0 < degrees < 90):
        raise UNetError("%s: starts.degrees must be in (0, 90), got %r" % (who, plan.degrees))
    if not 1 <= n <= MAX_STATES:
        raise UNetError("%s: starts.n must be in [1, %d], got %r" % (who, MAX_STATES, plan.n))
    if stride not in (1, 2, 4, 8):
        raise UNetError("%s: starts.rank_stride must be 1, 2, 4 or 8, got %r" % (who, plan.rank_stride))
    return degrees, n, stride


def moments(volume, lo, hi, out=None, stream=None):
    """unet_start_moments on the current stream (or the raw `stream`).  volume: a contiguous (D, H, W) uint8 or uint16 device
    tensor; a voxel is foreground when lo <= v <= hi.  Returns int64 {10} on the device (written into `out` when given): n, Sx, Sy,
    Sz, Sxx, Syy, Szz, Sxy, Sxz, Syz.  No host synchronisation."""
    if not (torch.is_tensor(volume) and volume.is_cuda and volume.dtype in (torch.uint8, torch.uint16) and volume.is_contiguous()
            and volume.dim() == 3 and volume.numel() > 0):
        raise UNetError("start.moments: volume must be a contiguous (D, H, W) uint8 or uint16 device tensor")
    d, h, w = (int(v) for v in volume.shape)
    if out is None:
        out = torch.empty(10, dtype=torch.int64, device=volume.device)
    elif not (torch.is_tensor(out) and out.is_cuda and out.device == volume.device and out.is_contiguous() and out.dtype == torch.int64
              and out.numel() == 10):
        raise UNetError("start.moments: out must be a contiguous int64 device tensor of 10 entries")
    E.check(E.lib.unet_start_moments(volume.data_ptr(), volume.element_size(), w, h, d, int(lo), int(hi), out.data_ptr(),
                                     E.stream(volume, stream)))
    return out


def _rot(axis, degrees):
    p, q = ((1, 2), (0, 2), (0, 1))[axis]
    a = math.radians(degrees)
    r = np.eye(3)
    r[p, p] = r[q, q] = math.cos(a)
    r[p, q] = -math.sin(a)
    r[q, p] = math.sin(a)
    return r


def _centroid_variance(m, who, name):
    try:
        s = [int(v) for v in np.asarray(m).reshape(10)]
    except (TypeError, ValueError):
        raise UNetError("start.%s: %s must be the 10 sums of start.moments" % (who, name))
    if s[0] < 0:
        raise UNetError("start.%s: %s holds a negative count" % (who, name))
    if s[0] == 0:
        return None, None
    n = float(s[0])
    c = np.array([s[1] / n, s[2] / n, s[3] / n])
    v = np.array([s[4] / n, s[5] / n, s[6] / n]) - c * c
    return c, v


def candidates(subject_moments, template_moments, degrees=12.0, fallback=None):
    """The starts of a search, float32 {27, 12} (row-major M then t, subject voxel -> template position): from each moment set the
    centroid c and the per-axis variance v = Saa / n - c^2; sc_r = sqrt(v_template_r / v_subject_r); for (i, j, k) in
    itertools.product((-degrees, 0, +degrees), repeat=3), M = rot(0, i) rot(1, j) rot(2, k) diag(sc), t = c_template - M c_subject.
    Index 13 is the unrotated start.  float64 arithmetic, rounded to float32 once at the end.

    When a foreground is empty or a variance is not positive the moments say nothing: the result is `fallback` (a map, e.g.
    register.centre_init's) alone, float32 {1, 12}; without a fallback that raises."""
    if not (isinstance(degrees, (int, float)) and not isinstance(degrees, bool) and math.isfinite(degrees) and 0 < degrees < 90):
        raise UNetError("start.candidates: degrees must be in (0, 90), got %r" % (degrees,))
    cs, vs = _centroid_variance(subject_moments, "candidates", "subject_moments")
    ct, vt = _centroid_variance(template_moments, "candidates", "template_moments")
    if cs is None or ct is None or not (np.all(vs > 0) and np.all(vt > 0)):
        if fallback is None:
            raise UNetError("start.candidates: an empty foreground or a zero variance, and no fallback map was given")
        return R._map12(fallback, "candidates").reshape(1, 12).copy()
    sc = np.sqrt(vt / vs)
    out = []
    for i, j, k in itertools.product((-degrees, 0.0, degrees), repeat=3):
        m = _rot(0, i) @ _rot(1, j) @ _rot(2, k) @ np.diag(sc)
        out.append(np.concatenate([m.reshape(9), ct - m @ cs]))
    return np.asarray(out, np.float64).astype(np.float32)


def rank(subject, template, n_tissues, maps, stride=2, stream=None):
    """The joint histograms of S starts, uint32 {S, T, T} on the device: register.joint_hist at `stride` in passes of at most 25
    maps.  maps: host, {S, 12}.  No host synchronisation."""
    try:
        flat = np.ascontiguousarray(np.asarray(maps, np.float32).reshape(-1, 12))
    except (TypeError, ValueError):
        raise UNetError("start.rank: maps must be {S, 12} numbers")
    S, T = int(flat.shape[0]), int(n_tissues)
    if not 1 <= S <= MAX_STARTS:
        raise UNetError("start.rank: S must be in [1, %d], got %d" % (MAX_STARTS, S))
    if not 2 <= T <= R.MAX_TISSUES:
        raise UNetError("start.rank: n_tissues must be in [2, %d], got %d" % (R.MAX_TISSUES, T))
    if not (torch.is_tensor(subject) and subject.is_cuda):
        raise UNetError("start.rank: subject must be a contiguous (D, H, W) uint8 or uint16 device tensor")
    hist = torch.empty(S * T * T, dtype=torch.uint32, device=subject.device)
    for k0 in range(0, S, R.MAX_MAPS):
        k1 = min(S, k0 + R.MAX_MAPS)
        R.joint_hist(subject, template, T, flat[k0:k1], stride=stride, out=hist[k0 * T * T:k1 * T * T], stream=stream)
    return hist.view(S, T, T)


def pick(hist, maps, n=MAX_STATES, always=ALWAYS, stream=None):
    """unet_start_pick on the current stream (or the raw `stream`).  hist: uint32 {S, T, T} on the device; maps: float32 {S, 12} on
    the device.  Returns device tensors: scores int64 {S}, inits float32 {n, 12}, picked int32 {n}: the n best scores in descending
    order, the lowest index first among equal scores, `always` (-1: nothing) in the last place when it is not among them.  No host
    synchronisation."""
    if not (torch.is_tensor(hist) and hist.is_cuda and hist.dtype == torch.uint32 and hist.is_contiguous() and hist.dim() == 3
            and hist.shape[1] == hist.shape[2]):
        raise UNetError("start.pick: hist must be a contiguous uint32 {S, T, T} device tensor")
    S, T = int(hist.shape[0]), int(hist.shape[1])
    if not (torch.is_tensor(maps) and maps.is_cuda and maps.device == hist.device and maps.dtype == torch.float32 and maps.is_contiguous()
            and maps.numel() == S * 12):
        raise UNetError("start.pick: maps must be a contiguous float32 {S, 12} tensor on hist's device")
    n, always = int(n), int(always)
    if not 1 <= n <= min(S, MAX_STATES):
        raise UNetError("start.pick: n must be in [1, min(S, %d)], got %d for S = %d" % (MAX_STATES, n, S))
    dev = hist.device
    scores = torch.empty(S, dtype=torch.int64, device=dev)
    inits = torch.empty((n, 12), dtype=torch.float32, device=dev)
    picked = torch.empty(n, dtype=torch.int32, device=dev)
    E.check(E.lib.unet_start_pick(hist.data_ptr(), S, T, maps.data_ptr(), n, always, scores.data_ptr(), inits.data_ptr(), picked.data_ptr(),
                                  E.stream(hist, stream)))
    return scores, inits, picked


def search(subject, template, n_tissues, inits, step=R.DEFAULT_STEP, stages=R.DEFAULT_STAGES, max_iterations=400, impl=IMPL_DEFAULT,
           trace=True, scratch=None, stream=None):
    """unet_start_search on the current stream (or the raw `stream`).  inits: float32 {n, 12} ON THE DEVICE, n <= 4.  Returns device
    tensors: maps float32 {n, 12}, trace int64 {n, max_iterations, 4} (None with trace=False), info int64 {n, 4}, best int32 {1},
    best_map float32 {12}; state s is what register.search gives from inits[s].  No host synchronisation under IMPL_BATCHED; one
    under IMPL_SEQUENTIAL."""
    sg = R._tissue(subject, "subject", "search")
    tg = R._tissue(template, "template", "search", subject.device)
    dev = subject.device
    if not (torch.is_tensor(inits) and inits.is_cuda and inits.device == dev and inits.dtype == torch.float32 and inits.is_contiguous()
            and inits.dim() == 2 and inits.shape[1] == 12 and 1 <= inits.shape[0] <= MAX_STATES):
        raise UNetError("start.search: inits must be a contiguous float32 {n, 12} tensor on the subject's device, n in [1, %d]" % MAX_STATES)
    try:
        st = np.ascontiguousarray(np.asarray(step, np.float32).reshape(12))
        sl = np.ascontiguousarray(np.asarray(stages, np.int32).reshape(-1, 3))
    except (TypeError, ValueError):
        raise UNetError("start.search: step must be 12 numbers and stages (stride, first_level, last_level) triples")
    T, n_it, n = int(n_tissues), int(max_iterations), int(inits.shape[0])
    if not 1 <= n_it <= R.MAX_ITERATIONS:
        raise UNetError("start.search: max_iterations must be in [1, %d], got %d" % (R.MAX_ITERATIONS, n_it))
    need = start_scratch_bytes(T, n)                                 # the range checks, before any device work
    scratch = E.scratch(scratch, need, dev)
    maps = torch.empty((n, 12), dtype=torch.float32, device=dev)
    tr = torch.empty((n, n_it, 4), dtype=torch.int64, device=dev) if trace else None
    info = torch.empty((n, 4), dtype=torch.int64, device=dev)
    best = torch.empty(1, dtype=torch.int32, device=dev)
    best_map = torch.empty(12, dtype=torch.float32, device=dev)
    E.check(E.lib.unet_start_search(*sg, *tg, T, inits.data_ptr(), n, st.ctypes.data_as(_fp), sl.ctypes.data_as(C.POINTER(C.c_int)),
                                    int(sl.shape[0]), n_it, maps.data_ptr(), tr.data_ptr() if trace else None, info.data_ptr(),
                                    best.data_ptr(), best_map.data_ptr(), int(impl), scratch.data_ptr(), scratch.nbytes,
                                    E.stream(subject, stream)))
    return maps, tr, info, best, best_map


def _host_moments(m, who, name):
    if torch.is_tensor(m):
        m = m.cpu().numpy()                                          # a host synchronisation
    try:
        return np.asarray(m).astype(np.int64).reshape(10)
    except (TypeError, ValueError):
        raise UNetError("start.%s: %s must be the 10 sums of start.moments" % (who, name))


def find(subject, template, n_tissues, subject_moments=None, template_moments=None, degrees=12.0, n=MAX_STATES, rank_stride=2,
         step=R.DEFAULT_STEP, stages=R.DEFAULT_STAGES, max_iterations=400, impl=IMPL_DEFAULT, fallback=None, scratch=None):
    """The map of the best of n searches from ranked starts: moments (of the voxels with tissue 1..T-1; either set may be given, as
    10 host numbers or a device tensor) -> candidates -> rank at `rank_stride` -> pick (the unrotated start always among the n) ->
    search.  fallback: the start when the moments say nothing (register.centre_init at equal voxel sizes when None).

    Returns (best_map float32 {12} on the device, pending): `pending` holds the device tensors of the report, read by
    `start.report(pending)` wherever the caller reads its own.  One host synchronisation: the subject's 80 bytes of moments (and the
    template's, when they are not given)."""
    R._tissue(subject, "subject", "find")
    R._tissue(template, "template", "find", subject.device)
    T = int(n_tissues)
    if not 2 <= T <= R.MAX_TISSUES:
        raise UNetError("start.find: n_tissues must be in [2, %d], got %d" % (R.MAX_TISSUES, T))
    degrees, n, rank_stride = _plan(Plan(degrees, n, rank_stride), "start.find")
    if template_moments is None:
        template_moments = moments(template, 1, T - 1)
    if subject_moments is None:
        subject_moments = moments(subject, 1, T - 1)
    tm = _host_moments(template_moments, "find", "template_moments")
    sm = _host_moments(subject_moments, "find", "subject_moments")
    if fallback is None:
        fallback = R.centre_init(tuple(subject.shape), (1, 1, 1), tuple(template.shape), (1, 1, 1))
    maps = candidates(sm, tm, degrees, fallback=fallback)
    S = int(maps.shape[0])
    maps_dev = torch.from_numpy(maps).to(subject.device)
    hist = rank(subject, template, T, maps, stride=rank_stride)
    scores, inits, picked = pick(hist, maps_dev, n=min(n, S), always=ALWAYS if S > ALWAYS else 0)
    maps_out, _, info, best, best_map = search(subject, template, T, inits, step=step, stages=stages, max_iterations=max_iterations,
                                               impl=impl, trace=False, scratch=scratch)
    pending = dict(candidates=maps, degenerate=S == 1, subject_moments=sm, template_moments=tm, scores=scores, picked=picked, maps=maps_out,
                   info=info, best=best)
    return best_map, pending


def report(pending):
    """The host report of a `find`: candidates float32 {S, 12}, degenerate (the moments said nothing: the fallback alone), the two
    moment sets, scores int64 {S}, picked int32 {n}, maps float32 {n, 12}, info int64 {n, 4} (iterations, converged, score, stage per
    state) and best.  SYNCHRONISES with the host."""
    out = dict(pending)
    for k in ("scores", "picked", "maps", "info"):
        out[k] = pending[k].cpu().numpy()
    out["best"] = int(pending["best"].cpu().numpy()[0])
    return out


def best_of(infos):
    """The index of the state with the greatest (converged, stage of the last iteration, score), the lowest among equal keys: the
    closing kernel's choice, on the host, for a caller that ran its searches itself.  infos: {n, 4} integers."""
    rows = np.asarray(infos).astype(np.int64).reshape(-1, 4)
    keys = [(int(r[1]), int(r[3]), int(r[2])) for r in rows]
    return max(range(len(keys)), key=lambda s: (keys[s], -s))
