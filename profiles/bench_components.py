#!/usr/bin/env python3
"""A model's single_component_label on the device (include/unet_components.h) at 192x224x192: three candidates alternating in one
process --
  tiled     UNET_COMPONENTS_IMPL_TILED: the tile's union-find in LDS, the tiles hooked together across their faces
  global    UNET_COMPONENTS_IMPL_GLOBAL: every voxel hooks in global memory
  parent    the only route before this kernel: per listed class a float mask plane built with torch (label == v), then
            unet_postproc_defragment with size_ratio = 1 on it, then the zeroed voxels taken over into the label map.  It keeps
            EVERY component of the largest count, so it differs on ties: it is timed on the solid map only and not bit-compared.
on two label maps --
  solid     nested shells of 5 classes around a ball, plus small scattered fragments of each class
  random    130 classes, uniform
with K = 1, 5 and 129 listed classes (solid holds 5 classes: the entries above 5 list classes that do not occur).
HIP events around `reps` calls (default 50) after a warm-up, repeated in `rounds` alternating rounds (default 5; the median and the
spread over rounds are reported); the label maps rotate over more than 256 MB so they cannot sit in the Infinity Cache, and every
timed call works on a fresh copy of its source (the call is in place), whose cost is measured as `copy` and subtracted.  Every row
carries its algorithmic bytes (2 B read per voxel plus 2 B per removed voxel) and the fraction of the 8 TB/s floor they amount to.
tiled and global are compared bitwise first.  One JSON line per row, printed and APPENDED to --out (default
profiles/components_bench.jsonl) with the run's tag, so repeating the whole command gives the run-to-run spread."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import unet_studio_amd as U  # noqa: E402,F401
from unet_studio_amd import components as CMP  # noqa: E402
from unet_studio_amd import postproc as P  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "components_bench.jsonl"))
ap.add_argument("--reps", type=int, default=50)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--tag", default="run")
args = ap.parse_args()

DEV = "cuda:0"
HBM = 8.0e12   # MI355X peak HBM bytes/s
CACHE = 256e6  # Infinity Cache
W, H, D = 192, 224, 192
S = W * H * D
N_CLASSES = 130
device = torch.cuda.get_device_name(0)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)


def solid_map(seed):
    """nested shells of classes 1..5 around a ball (class 5 innermost), and 0.2 % of the voxels turned into a random class 1..5"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    z, y, x = torch.meshgrid(torch.arange(D, device=DEV), torch.arange(H, device=DEV), torch.arange(W, device=DEV), indexing="ij")
    r = torch.sqrt(((x - W / 2) / (W / 2)) ** 2 + ((y - H / 2) / (H / 2)) ** 2 + ((z - D / 2) / (D / 2)) ** 2)
    lab = (5 - torch.floor(r / 0.18)).clamp(0, 5).to(torch.int32)
    frag = torch.rand((D, H, W), device=DEV, generator=g) < 0.002
    vals = torch.randint(1, 6, (D, H, W), device=DEV, generator=g, dtype=torch.int32)
    return torch.where(frag, vals, lab).to(torch.uint16)


def random_map(seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randint(0, N_CLASSES, (D, H, W), device=DEV, generator=g, dtype=torch.int32).to(torch.uint16)


def time_it(fn, reps):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(reps):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / reps * 1e3   # us


nbuf = int(CACHE // (2 * S)) + 2                             # > 256 MB of label maps in rotation
scratch = torch.empty(CMP.components_scratch_bytes(S, N_CLASSES), dtype=torch.uint8, device=DEV)
pp_scratch = torch.empty(P.postproc_scratch_bytes(2, S), dtype=torch.uint8, device=DEV)
work = torch.empty((D, H, W), dtype=torch.uint16, device=DEV)
plane = torch.empty((D, H, W), dtype=torch.float32, device=DEV)
rows = []
for kind, make in (("solid", solid_map), ("random", random_map)):
    srcs = [make(100 + i) for i in range(nbuf)]
    k = [0]

    def nxt():
        k[0] = (k[0] + 1) % nbuf
        return srcs[k[0]]

    for K in (1, 5, 129):
        listed = list(range(1, K + 1))

        def run(impl):
            work.copy_(nxt())
            CMP.keep_largest(work, listed, N_CLASSES, scratch=scratch, impl=impl)

        def parent_route():
            work.copy_(nxt())
            w16 = work.view(torch.int16)                     # torch's comparisons take int16; the values are below 130
            for v in listed:
                torch.eq(w16, v, out=mask_b)
                plane.copy_(mask_b)
                P.defragment_call((W, H, D), False, 0.5, 1.0, plane, None, 0, None, pp_scratch)
                w16.masked_fill_(mask_b & (plane == 0), 0)

        mask_b = torch.empty((D, H, W), dtype=torch.bool, device=DEV)
        cands = {"tiled": lambda: run(CMP.IMPL_TILED), "global": lambda: run(CMP.IMPL_GLOBAL)}
        if kind == "solid":
            cands["parent"] = parent_route
        cands["copy"] = lambda: work.copy_(nxt())            # every candidate's fresh copy, subtracted from its row
        # tiled and global compute the same bits; the removed voxels give the algorithmic bytes
        a, b = srcs[0].clone(), srcs[0].clone()
        removed = torch.zeros(N_CLASSES, dtype=torch.int32, device=DEV)
        CMP.keep_largest(a, listed, N_CLASSES, removed=removed, scratch=scratch, impl=CMP.IMPL_TILED)
        CMP.keep_largest(b, listed, N_CLASSES, scratch=scratch, impl=CMP.IMPL_GLOBAL)
        same = bool(torch.equal(a.view(torch.int16), b.view(torch.int16)))
        n_removed = int(removed.sum().item())
        assert n_removed == int((a.view(torch.int16) != srcs[0].view(torch.int16)).sum().item())
        del a, b
        reps = args.reps if "parent" not in cands or K < 129 else max(2, args.reps // 10)   # 129 labellings per call
        for name, fn in cands.items():                       # warm-up: every candidate
            for _ in range(1 if name == "parent" and K == 129 else 3):
                fn()
        torch.cuda.synchronize()
        times = {name: [] for name in cands}
        for _ in range(args.rounds):                         # alternate the candidates
            for name, fn in cands.items():
                times[name].append(time_it(fn, reps if name == "parent" else args.reps))
        copy_us = statistics.median(times["copy"])
        nbytes = 2 * S + 2 * n_removed
        for name in cands:
            if name == "copy":
                continue
            t = [v - copy_us for v in times[name]]
            us = statistics.median(t)
            rows.append(dict(tag=args.tag, name="%s K=%d %s" % (kind, K, name), map=kind, listed=K, candidate=name, dims=[W, H, D],
                             us=round(us, 1), us_min=round(min(t), 1), us_max=round(max(t), 1), copy_us=round(copy_us, 1),
                             removed_voxels=n_removed, algorithmic_bytes=nbytes, floor_us=round(nbytes / HBM * 1e6, 2),
                             hbm_fraction=round(nbytes / (us * 1e-6) / HBM, 5), bitwise_equal=same,
                             reps=reps if name == "parent" else args.reps, rounds=args.rounds, buffers_rotated=nbuf, device=device))
            print(json.dumps(rows[-1]), flush=True)
            with open(args.out, "a") as f:
                f.write(json.dumps(rows[-1]) + "\n")
    del srcs
