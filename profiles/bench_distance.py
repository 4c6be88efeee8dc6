#!/usr/bin/env python3
"""Boundary distances on the device (include/unet_distance.h) at 192 x 224 x 192, under the weights (1, 1, 1) and (4, 4, 9):
  transform          of the surface of a ball and of a cortex-like thin sheet, UNET_DIST_IMPL_LDS and UNET_DIST_IMPL_GLOBAL alternating in
                     one process, compared for equal bits before anything is timed
  surface_distances  for 5 labels (nested shells against the same shells shifted and perturbed), end to end: the counts, ten
                     transforms and gathers, one sort, two copies to the host; a host clock around the call, which ends synchronised
  scipy              scipy.ndimage.distance_transform_edt of the same mask on the host, once, as context (skipped with --no-scipy)
HIP events around `reps` transforms (default 20 = the median's sample; one event pair per call) after a warm-up.  The maps rotate
over more than 256 MB together with the outputs, so nothing sits in the Infinity Cache between calls.  Every transform row carries
its algorithmic bytes -- the x pass reads the map (1 B a voxel) and writes int32, the y and z passes read and write int32: 21 B a
voxel -- and the fraction of the 8 TB/s floor they amount to.  One JSON line per row, printed and APPENDED to --out (default
profiles/distance_bench.jsonl) with the run's tag."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import unet_studio_amd as U  # noqa: E402,F401
from unet_studio_amd import distance as DS  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "distance_bench.jsonl"))
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--dims", type=int, nargs=3, default=[192, 224, 192], metavar=("W", "H", "D"))
ap.add_argument("--tag", default="run")
ap.add_argument("--no-scipy", action="store_true")
args = ap.parse_args()

DEV = "cuda:0"
HBM = 8.0e12   # MI355X peak HBM bytes/s
CACHE = 256e6  # Infinity Cache
W, H, D = args.dims
S = W * H * D
device = torch.cuda.get_device_name(0)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
z, y, x = torch.meshgrid(torch.arange(D, device=DEV), torch.arange(H, device=DEV), torch.arange(W, device=DEV), indexing="ij")


def radius2(shift):
    """the squared distance from a centre `shift` voxels off the middle, normalised so that 1 is the inscribed ellipsoid"""
    return (((x - W / 2 - shift) / (W / 2)) ** 2 + ((y - H / 2 - shift) / (H / 2)) ** 2 + ((z - D / 2 - shift) / (D / 2)) ** 2)


def ball_map(shift):
    return (radius2(shift) < 0.5).to(torch.uint8)


def sheet_map(shift):
    """a folded sheet two to three voxels thick: a wavy shell, features near every voxel as in a cortical ribbon"""
    r = torch.sqrt(radius2(shift)) + 0.06 * torch.sin(x / 5.0) * torch.sin(y / 6.0) * torch.cos(z / 5.5)
    return ((r > 0.70) & (r < 0.70 + 5.0 / min(W, H, D))).to(torch.uint8)


def shells_map(shift, seed):
    """labels 1..5 in nested shells, the boundaries perturbed by a smooth wave that depends on the seed"""
    r = torch.sqrt(radius2(shift)) + 0.03 * torch.sin((x + 11 * seed) / 7.0) * torch.sin((y + 5 * seed) / 6.0)
    return torch.clamp(6 - torch.ceil(r * 6), 0, 5).to(torch.uint8)


def event_times(fn, reps):
    """us per call, one event pair per call"""
    out = []
    for _ in range(reps):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        fn()
        ev[1].record()
        torch.cuda.synchronize()
        out.append(ev[0].elapsed_time(ev[1]) * 1e3)
    return out


def emit(row):
    print(json.dumps(row), flush=True)
    with open(args.out, "a") as f:
        f.write(json.dumps(row) + "\n")


nbuf = int(CACHE // (5 * S)) + 2                                 # > 256 MB of maps and outputs in rotation
outs = [torch.empty((D, H, W), dtype=torch.int32, device=DEV) for _ in range(nbuf)]
scratch = torch.empty(DS.distance_scratch_bytes((W, H, D)), dtype=torch.uint8, device=DEV)
ALGO_BYTES = S * (1 + 4 + 8 + 8)
for weights in ((1, 1, 1), (4, 4, 9)):
    for kind, make in (("ball", ball_map), ("sheet", sheet_map)):
        maps = [make(i) for i in range(nbuf)]
        k = [0]

        def call(impl):
            k[0] = (k[0] + 1) % nbuf
            return DS.transform(maps[k[0]], 1, weights, "surface", impl, out=outs[k[0]], scratch=scratch)

        cands = {"lds": DS.IMPL_LDS, "global": DS.IMPL_GLOBAL}
        res = {}
        for name, impl in cands.items():                        # equal bits first, on the same map
            k[0] = nbuf - 1
            res[name] = call(impl).clone()
        assert torch.equal(res["lds"], res["global"]), "IMPL_LDS and IMPL_GLOBAL differ"
        features = int((res["lds"] == 0).sum())
        far = float(res["lds"].max()) ** 0.5
        del res
        for impl in cands.values():
            for _ in range(3):
                call(impl)
        torch.cuda.synchronize()
        times = {name: [] for name in cands}
        for _ in range(4):                                       # alternate the candidates, reps / 4 calls at a time
            for name, impl in cands.items():
                times[name] += event_times(lambda: call(impl), max(1, args.reps // 4))
        med = {name: statistics.median(t) for name, t in times.items()}
        host_ms = None
        if not args.no_scipy:
            from scipy import ndimage
            mask = maps[0].cpu().numpy().astype(bool)
            surface = mask & ~ndimage.binary_erosion(mask, ndimage.generate_binary_structure(3, 1), border_value=0)
            t0 = time.perf_counter()
            ndimage.distance_transform_edt(~surface, sampling=np.sqrt(weights[::-1]))
            host_ms = round((time.perf_counter() - t0) * 1e3, 1)
        for name, t in times.items():
            emit(dict(tag=args.tag, name="transform %s w=%s %s" % (kind, "x".join(map(str, weights)), name), call="transform", map=kind,
                      weights=list(weights), candidate=name, dims=[W, H, D], us=round(med[name], 1), us_min=round(min(t), 1),
                      us_max=round(max(t), 1), global_over_lds=round(med["global"] / med["lds"], 3), surface_voxels=features,
                      farthest_voxels=round(far, 1), algorithmic_bytes=ALGO_BYTES, floor_us=round(ALGO_BYTES / HBM * 1e6, 2),
                      hbm_fraction=round(ALGO_BYTES / (med[name] * 1e-6) / HBM, 5), bitwise_equal_to_lds=True, reps=len(t),
                      scipy_edt_host_ms=host_ms, buffers_rotated=nbuf, device=device))
        del maps
    # surface_distances, 5 labels, end to end (the call ends with a copy to the host: a host clock)
    a, b = shells_map(0, 0), shells_map(2, 1)
    for impl_name, impl in (("lds", DS.IMPL_LDS), ("global", DS.IMPL_GLOBAL)):
        for _ in range(2):
            res = DS.surface_distances(a, b, 5, weights, impl=impl, scratch=scratch)
        ms = []
        for _ in range(max(3, args.reps // 4)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = DS.surface_distances(a, b, 5, weights, impl=impl, scratch=scratch)
            ms.append((time.perf_counter() - t0) * 1e3)
        table = DS.summary(res, 1.0)
        emit(dict(tag=args.tag, name="surface_distances 5 labels w=%s %s" % ("x".join(map(str, weights)), impl_name), call="surface_distances",
                  weights=list(weights), candidate=impl_name, dims=[W, H, D], ms=round(statistics.median(ms), 3), ms_min=round(min(ms), 3),
                  ms_max=round(max(ms), 3), labels_measured=len(res["values"]), surface_voxels=int(res["counts"][1:].sum()),
                  hd_units=[round(float(v), 3) for v in table[1:, 0]], reps=len(ms), device=device))
