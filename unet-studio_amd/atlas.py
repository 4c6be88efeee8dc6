"""The atlas preparation of evaluate_unet::load_atlas (evaluate.cpp:112-179) and reclassify_labels_by_template (evaluate.cpp:60-110)
on the device (include/unet_atlas.h), the path of `--template ... --atlas ...` (evaluate.cpp:488-496):

  reclassify      tissue votes per region, the per-region majority tissue, the erase of every region's voxels that lie in another
                  tissue, the tissue totals and the covered counts -- evaluate.cpp:63-94,136-152 literally, integer-only: PINNED
  grow            the regions grown back into the unlabelled voxels of the flagged tissues and smoothed -- this project's definition
                  in place of tipl::morphology::fill_and_smooth_labels (TIPL, not in the reference tree: parity NOT pinned)
  prepare_atlas   load_atlas end to end: majority resampling onto the template grid, CLAMP | PRESERVE, coverage, reclassify, grow

IMPL_LDS gathers the votes in a block's LDS table and flushes it once, IMPL_GLOBAL adds in global memory (the measured baseline and a
second witness of the bits)."""
import ctypes as C

import numpy as np
import torch

from . import engine as E
from .engine import UNetError

E._sig("unet_atlas_scratch_bytes", C.c_int, C.c_int64, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_size_t))
E._sig("unet_atlas_reclassify", C.c_int, C.c_int64, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
       C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p)
E._sig("unet_atlas_grow", C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_uint8),
       C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p)
# every symbol include/unet_atlas.h declares
EXPORTS = ["unet_atlas_scratch_bytes", "unet_atlas_reclassify", "unet_atlas_grow"]

IMPL_DEFAULT, IMPL_LDS, IMPL_GLOBAL = 0, 1, 2
CLAMP, PRESERVE, COUNT_ONLY = 1, 2, 4
LDS_ENTRIES = 8192   # UNET_ATLAS_LDS_ENTRIES
MAX_TISSUES, MAX_REGIONS, MAX_ROUNDS, MAX_SMOOTH = 256, 65535, 65534, 16


def atlas_scratch_bytes(voxels, n_regions, n_tissues, max_rounds=0):
    """One size for both calls; reclassify alone needs only atlas_scratch_bytes(1, n_regions, n_tissues, 0): it has no per-voxel
    scratch."""
    return E.size_query(E.lib.unet_atlas_scratch_bytes, int(voxels), int(n_regions), int(n_tissues), int(max_rounds))


def _maps(tissue, atlas, who):
    if not (torch.is_tensor(atlas) and atlas.is_cuda and atlas.dtype == torch.uint16 and atlas.is_contiguous()):
        raise UNetError("atlas.%s: atlas must be a contiguous uint16 device tensor" % who)
    if not (torch.is_tensor(tissue) and tissue.is_cuda and tissue.dtype in (torch.uint8, torch.uint16) and tissue.is_contiguous()
            and tissue.device == atlas.device):
        raise UNetError("atlas.%s: tissue must be a contiguous uint8 or uint16 tensor on the atlas's device" % who)
    if tissue.numel() != atlas.numel() or atlas.numel() == 0:
        raise UNetError("atlas.%s: tissue holds %d voxels, atlas %d" % (who, tissue.numel(), atlas.numel()))
    return tissue.element_size()


def _reports(out, spec, dev, who):
    """the report tensors: the caller's (`out`, a dict that must hold every one, of the right size) or new ones"""
    if out is None:
        return {k: torch.empty(shape, dtype=dt, device=dev) for k, (shape, dt) in spec.items()}
    for k, (shape, dt) in spec.items():
        t = out.get(k)
        if not (torch.is_tensor(t) and t.is_cuda and t.device == dev and t.is_contiguous() and t.element_size() == torch.empty(0, dtype=dt).element_size()
                and t.numel() == int(np.prod(shape))):
            raise UNetError("atlas.%s: out[%r] must be a contiguous %s device tensor of %d entries" % (who, k, dt, int(np.prod(shape))))
    return out


def reclassify(tissue, atlas, n_regions, n_tissues, flags=0, count_only=False, impl=IMPL_DEFAULT, scratch=None, stream=None, out=None):
    """evaluate.cpp:63-94,136-152 on the current stream (or the raw `stream`).  atlas: a contiguous uint16 device tensor, changed in
    place (not with count_only); tissue: uint8 or uint16 of the same element count.  Returns the five reports as device tensors:
    votes uint32 {n_regions + 1, n_tissues}, tissue_total and covered uint32 {n_tissues}, majority uint8 {n_regions + 1}, erased
    uint32 {n_regions + 1} (written into `out`'s tensors when that dict is given).  No host synchronisation."""
    tb = _maps(tissue, atlas, "reclassify")
    R, T = int(n_regions), int(n_tissues)
    need = atlas_scratch_bytes(1, R, T, 0)                       # the range checks, before any device work
    flags = int(flags) | (COUNT_ONLY if count_only else 0)
    dev = atlas.device
    out = _reports(out, dict(votes=((R + 1, T), torch.uint32), tissue_total=((T,), torch.uint32), covered=((T,), torch.uint32),
                             majority=((R + 1,), torch.uint8), erased=((R + 1,), torch.uint32)), dev, "reclassify")
    scratch = E.scratch(scratch, need, dev)
    E.check(E.lib.unet_atlas_reclassify(atlas.numel(), tissue.data_ptr(), tb, atlas.data_ptr(), R, T, flags, out["votes"].data_ptr(),
                                        out["tissue_total"].data_ptr(), out["covered"].data_ptr(), out["majority"].data_ptr(),
                                        out["erased"].data_ptr(), int(impl), scratch.data_ptr(), scratch.nbytes, E.stream(atlas, stream)))
    return out


def grow(tissue, atlas, n_tissues, grow_tissues, flags=0, max_rounds=None, smooth_rounds=1, scratch=None, stream=None, out=None):
    """The fill and the smoothing of include/unet_atlas.h on the current stream (or the raw `stream`), in place on atlas.  tissue: a
    (D, H, W) uint8 or uint16 device tensor; atlas: uint16 of the same element count.  grow_tissues: the tissues to work on.
    max_rounds=None means W + H + D; the caller sees whether that was enough in info[1].  Returns the reports as device tensors:
    filled and relabelled uint32 {n_tissues}, info uint32 {2} = (fill rounds that filled something, converged), written into
    `out`'s tensors when that dict is given.  No host synchronisation."""
    tb = _maps(tissue, atlas, "grow")
    if tissue.dim() != 3:
        raise UNetError("atlas.grow: tissue must be a (D, H, W) tensor")
    D, H, W = (int(v) for v in tissue.shape)
    T = int(n_tissues)
    if max_rounds is None:
        max_rounds = min(W + H + D, MAX_ROUNDS)
    flagged = np.zeros(MAX_TISSUES, np.uint8)
    for t in grow_tissues:
        if isinstance(t, bool) or int(t) != t or not 0 <= int(t) < min(max(T, 0), MAX_TISSUES):
            raise UNetError("atlas.grow: tissue %r is not in [0, %d]" % (t, T - 1))
        flagged[int(t)] = 1
    need = atlas_scratch_bytes(W * H * D, 0, T, int(max_rounds))
    dev = atlas.device
    out = _reports(out, dict(filled=((T,), torch.uint32), relabelled=((T,), torch.uint32), info=((2,), torch.uint32)), dev, "grow")
    scratch = E.scratch(scratch, need, dev)
    arr = (C.c_uint8 * MAX_TISSUES)(*flagged.tolist())
    E.check(E.lib.unet_atlas_grow(W, H, D, tissue.data_ptr(), tb, atlas.data_ptr(), T, int(flags), arr, int(max_rounds), int(smooth_rounds),
                                  out["filled"].data_ptr(), out["relabelled"].data_ptr(), out["info"].data_ptr(), scratch.data_ptr(),
                                  scratch.nbytes, E.stream(atlas, stream)))
    return out


# ---- load_atlas's host arithmetic (evaluate.cpp:141-152,166-169) -----------------------------------------------------------------
def tissue_coverage(covered, tissue_total):
    """float32(covered) / float32(tissue_total) for the tissues >= 1 with a non-zero total, 0 elsewhere (evaluate.cpp:141-152)"""
    covered, total = np.asarray(covered, np.uint32), np.asarray(tissue_total, np.uint32)
    cov = np.zeros(total.size, np.float32)
    for t in range(1, total.size):
        if total[t]:
            cov[t] = np.float32(covered[t]) / np.float32(total[t])
    return cov


def tissues_to_grow(coverage, threshold=0.75):
    """the tissues >= 1 whose coverage is > threshold in float32 (evaluate.cpp:166-169: `<= 0.75f` is skipped)"""
    coverage = np.asarray(coverage, np.float32)
    return [t for t in range(1, coverage.size) if coverage[t] > np.float32(threshold)]


def prepare_atlas(template, atlas, n_tissues=5, map=None, coverage=0.75, max_rounds=None, smooth_rounds=1, impl=IMPL_DEFAULT):
    """evaluate_unet::load_atlas (evaluate.cpp:112-179) without the file reads and the corrected-atlas cache.  template: the tissue
    map, a (D, H, W) uint8 or uint16 device tensor (values >= n_tissues read as 0, evaluate.hpp:38).  atlas: a region map, an integer
    device tensor; with `map` (template voxel -> atlas position, space.py's convention) it lives on its own grid and is brought onto
    the template's with space.resample(mode="majority") (:126), otherwise it has the template's shape.  The input is not changed.

    Returns (corrected uint16 atlas of the template's shape, report) with report = dict(n_regions, coverage float32 {n_tissues},
    tissue_total, covered, majority, erased (every region), erased_reported (the regions with a non-zero majority, :99-105), grown
    (the tissues worked on), filled, relabelled, rounds, converged).

    Two host synchronisations: the atlas's maximum (:131) and the 2 * n_tissues counters the coverage needs (:148-152), and one more
    at the end to read the reports; acceptable in a once-per-atlas preparation."""
    from . import space as SP
    if not (torch.is_tensor(template) and template.is_cuda and template.dim() == 3):
        raise UNetError("atlas.prepare_atlas: template must be a (D, H, W) device tensor")
    if not (torch.is_tensor(atlas) and atlas.is_cuda and atlas.device == template.device):
        raise UNetError("atlas.prepare_atlas: atlas must be a tensor on the template's device")
    T = int(n_tissues)
    if map is not None:
        src = atlas.to(torch.int32).to(torch.float32).contiguous()      # region ids are exact in fp32
        if src.dim() != 3:
            raise UNetError("atlas.prepare_atlas: atlas must be a (d, h, w) tensor")
        on_grid = SP.resample(src, tuple(template.shape), map, mode="majority")
        work = on_grid.to(torch.int32).to(torch.uint16)
    else:
        if atlas.numel() != template.numel():
            raise UNetError("atlas.prepare_atlas: without a map the atlas must have the template's shape")
        work = atlas.to(torch.int32).to(torch.uint16).reshape(template.shape).clone()
    work = work.contiguous()
    template = template.contiguous()
    R = int(work.to(torch.int32).max().item())                           # host synchronisation 1 (:131)
    flags = CLAMP | PRESERVE
    rep = reclassify(template, work, R, T, flags=flags, impl=impl)
    counters = torch.stack([rep["covered"].view(torch.int32), rep["tissue_total"].view(torch.int32)]).cpu().numpy()   # 2 (:148-152)
    cov = tissue_coverage(counters[0].view(np.uint32), counters[1].view(np.uint32))
    todo = tissues_to_grow(cov, coverage)
    g = grow(template, work, T, todo, flags=flags, max_rounds=max_rounds, smooth_rounds=smooth_rounds)

    def host(t):
        return t.cpu().numpy() if t.dtype == torch.uint8 else t.view(torch.int32).cpu().numpy().view(np.uint32)

    majority, erased, info = host(rep["majority"]), host(rep["erased"]), host(g["info"])
    report = dict(n_regions=R, coverage=cov, tissue_total=counters[1].view(np.uint32), covered=counters[0].view(np.uint32),
                  majority=majority, erased=erased, erased_reported=[int(erased[a]) for a in range(1, R + 1) if majority[a] > 0],
                  grown=todo, filled=host(g["filled"]), relabelled=host(g["relabelled"]), rounds=int(info[0]), converged=bool(info[1]))
    return work, report
