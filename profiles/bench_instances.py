#!/usr/bin/env python3
"""The instances of a label map on the device (include/unet_instances.h) at 128^3 and 256^3: for `label` and for `match` the two
implementations alternating in one process --
  label   tiled    UNET_INST_LABEL_TILED: the tile's union-find in LDS, the tiles hooked across their faces, the table in a block's LDS
          global   UNET_INST_LABEL_GLOBAL: every voxel hooks in global memory, the table in global memory
          scipy    for context, the only route without these kernels: the map copied to the host, scipy.ndimage.label per listed
                   class, the instance map copied back (a host clock around it, one call; it gives no table)
  match   lds      UNET_INST_IMPL_LDS: a block gathers its runs in an LDS table and flushes one update per touched pair
          global   UNET_INST_IMPL_GLOBAL: every run goes to the global table
on two uint16 maps --
  solid    5 x 5 x 4 blocks, one class per block, all 100 listed: what a parcellation looks like (100 instances)
  sparse   a few hundred balls of radius 2..4 of one class in an empty volume: what a lesion map looks like
`match` pairs the instance map with that of the same map shifted by (1, 2, 3) voxels.  Both implementations are compared for equal
bits (match: after a sort) before anything is timed; the row records the outcome.  HIP events around `reps` calls (default 20) after
a warm-up, repeated in `rounds` alternating rounds (default 5; the median and the spread over rounds are reported); the maps rotate
over more than 256 MB (at most 10 buffers) so that they do not sit in the Infinity Cache.  Every row carries its algorithmic bytes
(label: 2 B read and 4 B written per voxel; match: 8 B read per voxel) and the fraction of the 8 TB/s floor they amount to.  One JSON
line per row, printed and APPENDED to --out (default profiles/instances_bench.jsonl) with the run's tag."""
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
from unet_studio_amd import instances as IN  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "instances_bench.jsonl"))
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--sizes", type=int, nargs="+", default=[128, 256])
ap.add_argument("--no-scipy", action="store_true")
ap.add_argument("--tag", default="run")
args = ap.parse_args()

DEV = "cuda:0"
HBM = 8.0e12   # MI355X peak HBM bytes/s
CACHE = 256e6  # Infinity Cache
MAX_BUFFERS = 10
MAX_INSTANCES, MAX_PAIRS = 4095, 16384
device = torch.cuda.get_device_name(0)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)


def time_it(fn, reps):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(reps):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / reps * 1e3   # us


def emit(row):
    print(json.dumps(row), flush=True)
    with open(args.out, "a") as f:
        f.write(json.dumps(row) + "\n")


for size in args.sizes:
    W = H = D = size
    S = W * H * D
    z, y, x = torch.meshgrid(torch.arange(D, device=DEV), torch.arange(H, device=DEV), torch.arange(W, device=DEV), indexing="ij")

    def solid_map(seed):
        """5 x 5 x 4 blocks shifted by the seed, classes 1..100"""
        xs, ys, zs = (x + 3 * seed) % W, (y + 5 * seed) % H, (z + 7 * seed) % D
        return (1 + xs * 5 // W + 5 * (ys * 5 // H + 5 * (zs * 4 // D))).to(torch.int32).to(torch.uint16)

    def sparse_map(seed):
        """300 balls of radius 2..4 of class 1 at random centres"""
        g = torch.Generator().manual_seed(seed)
        lab = torch.zeros((D, H, W), dtype=torch.bool, device=DEV)
        c = torch.randint(5, size - 5, (300, 3), generator=g)
        r = torch.randint(2, 5, (300,), generator=g)
        for (cz, cy, cx), rr in zip(c.tolist(), r.tolist()):
            sub = (slice(cz - rr, cz + rr + 1), slice(cy - rr, cy + rr + 1), slice(cx - rr, cx + rr + 1))
            lab[sub] |= ((z[sub] - cz) ** 2 + (y[sub] - cy) ** 2 + (x[sub] - cx) ** 2) <= rr * rr
        return lab.to(torch.int32).to(torch.uint16)

    nbuf = min(MAX_BUFFERS, int(CACHE // (2 * S)) + 2)
    for kind, make, n_classes in (("solid", solid_map, 101), ("sparse", sparse_map, 2)):
        maps = [make(i) for i in range(nbuf)]
        scratch = torch.empty(IN.inst_scratch_bytes(S, n_classes, MAX_INSTANCES), dtype=torch.uint8, device=DEV)
        out = (torch.empty(S, dtype=torch.int32, device=DEV), torch.empty((MAX_INSTANCES + 1) * 12, dtype=torch.int64, device=DEV),
               torch.empty(2, dtype=torch.int64, device=DEV))
        k = [0]

        def nxt():
            k[0] = (k[0] + 1) % nbuf
            return k[0]

        # ---- label ----
        cands = {"tiled": lambda: IN.label(maps[nxt()], n_classes, None, MAX_INSTANCES, impl=IN.LABEL_TILED, scratch=scratch, out=out),
                 "global": lambda: IN.label(maps[nxt()], n_classes, None, MAX_INSTANCES, impl=IN.LABEL_GLOBAL, scratch=scratch, out=out)}
        res = {}
        for name, fn in cands.items():                           # equal bits first, on the same map
            k[0] = nbuf - 1
            res[name] = [t.clone() for t in fn()]
        same = all(torch.equal(a, b) for a, b in zip(res["tiled"], res["global"]))
        assert same, "LABEL_TILED and LABEL_GLOBAL differ"
        n_inst = int(res["tiled"][2][0])
        assert n_inst <= MAX_INSTANCES
        del res
        for fn in cands.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        times = {name: [] for name in cands}
        for _ in range(args.rounds):
            for name, fn in cands.items():
                times[name].append(time_it(fn, args.reps))
        scipy_us = None
        if not args.no_scipy:
            from scipy import ndimage
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            host = maps[0].view(torch.int16).cpu().numpy()
            inst, n = np.zeros(host.shape, np.int32), 0
            for c in range(1, n_classes):
                got, m = ndimage.label(host == c)
                inst[got > 0] = got[got > 0] + n
                n += m
            back = torch.from_numpy(inst).to(DEV)
            torch.cuda.synchronize()
            scipy_us = (time.perf_counter() - t0) * 1e6
            assert n == n_inst
            del back
        nbytes = 6 * S
        med = {name: statistics.median(t) for name, t in times.items()}
        for name, t in times.items():
            emit(dict(tag=args.tag, name="label %s %d^3 %s" % (kind, size, name), call="label", map=kind, candidate=name, dims=[W, H, D],
                      instances=n_inst, us=round(med[name], 1), us_min=round(min(t), 1), us_max=round(max(t), 1),
                      global_over_tiled=round(med["global"] / med["tiled"], 3),
                      scipy_per_class_with_copies_us=None if scipy_us is None else round(scipy_us, 0), algorithmic_bytes=nbytes,
                      floor_us=round(nbytes / HBM * 1e6, 2), hbm_fraction=round(nbytes / (med[name] * 1e-6) / HBM, 5), bitwise_equal=same,
                      reps=args.reps, rounds=args.rounds, buffers_rotated=nbuf, device=device))

        # ---- match: every map's instances against those of the map shifted by (1, 2, 3) ----
        ias = [IN.label(m, n_classes, None, MAX_INSTANCES, scratch=scratch)[0].view(-1).clone() for m in maps]
        ibs = [IN.label(torch.roll(m.view(torch.int16), (3, 2, 1), (0, 1, 2)).view(torch.uint16).contiguous(), n_classes, None, MAX_INSTANCES,
                        scratch=scratch)[0].view(-1).clone() for m in maps]
        mscratch = torch.empty(IN.match_scratch_bytes(MAX_PAIRS), dtype=torch.uint8, device=DEV)
        mout = (torch.empty(MAX_PAIRS, dtype=torch.int64, device=DEV), torch.empty(MAX_PAIRS, dtype=torch.int64, device=DEV),
                torch.empty(2, dtype=torch.int64, device=DEV))

        def run_match(impl):
            i = nxt()
            return IN.match_raw(ias[i], ibs[i], MAX_PAIRS, impl=impl, scratch=mscratch, out=mout)

        cands = {"lds": lambda: run_match(IN.IMPL_LDS), "global": lambda: run_match(IN.IMPL_GLOBAL)}
        res = {}
        for name, fn in cands.items():
            k[0] = nbuf - 1
            keys, counts, info = fn()
            n, overflow = (int(v) for v in info.cpu())
            assert not overflow
            keys, order = torch.sort(keys[:n])
            res[name] = (keys.clone(), counts[:n][order].clone())
        same = all(torch.equal(a, b) for a, b in zip(res["lds"], res["global"]))
        assert same, "IMPL_LDS and IMPL_GLOBAL differ"
        n_pairs = int(res["lds"][0].numel())
        del res
        for fn in cands.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        times = {name: [] for name in cands}
        for _ in range(args.rounds):
            for name, fn in cands.items():
                times[name].append(time_it(fn, args.reps))
        nbytes = 8 * S
        med = {name: statistics.median(t) for name, t in times.items()}
        for name, t in times.items():
            emit(dict(tag=args.tag, name="match %s %d^3 %s" % (kind, size, name), call="match", map=kind, candidate=name, dims=[W, H, D],
                      pairs=n_pairs, max_pairs=MAX_PAIRS, us=round(med[name], 1), us_min=round(min(t), 1), us_max=round(max(t), 1),
                      global_over_lds=round(med["global"] / med["lds"], 3), algorithmic_bytes=nbytes, floor_us=round(nbytes / HBM * 1e6, 2),
                      hbm_fraction=round(nbytes / (med[name] * 1e-6) / HBM, 5), bitwise_equal_after_sort=same, reps=args.reps,
                      rounds=args.rounds, buffers_rotated=nbuf, device=device))
        del maps, ias, ibs, scratch, out, mscratch, mout
