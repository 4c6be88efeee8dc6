#!/usr/bin/env python3
"""Connected components with a chosen connectivity on the device (include/unet_connectivity.h) at 128^3 and 256^3, the candidates
alternating in one process --
  keep_largest   connectivity.keep_largest on a fresh copy of the map (the call is in place; the copy is timed in a row of its own,
                 `restore`, and subtracted)
  label          connectivity.label with room for 65535 instances
with connectivity 6, 18 and 26 under UNET_CONN_IMPL_TILED (a tile's union-find in LDS, the tiles hooked across their boundaries) and
UNET_CONN_IMPL_GLOBAL (every voxel hooked in global memory), on two uint16 maps --
  solid    a ball of class 1 of half the volume with 20 cavities of radius 2..4 inside it
  sparse   300 balls of radius 2..4 of class 1 in an empty volume: what a lesion map looks like
(the maps of profiles/bench_morph.py).  The two impls of a connectivity are compared for equal bits before anything is timed; the row
records the outcome and the instances found.  HIP events around `reps` calls (default 20) after a warm-up, repeated in `rounds`
alternating rounds (default 5; the median and the spread over rounds are reported); several maps rotate.  The connectivity-6 row of
the same call, map, size and impl in the same run is the yardstick: `over_c6` is the row's median over that row's.  `global_over_tiled`
is what UNET_CONN_IMPL_DEFAULT rests on.  One JSON line per row, printed and APPENDED to --out (default
profiles/connectivity_bench.jsonl) with the run's tag."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import unet_studio_amd as U  # noqa: E402,F401
from unet_studio_amd import connectivity as CN  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "connectivity_bench.jsonl"))
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--sizes", type=int, nargs="+", default=[128, 256])
ap.add_argument("--tag", default="run")
args = ap.parse_args()

DEV = "cuda:0"
NBUF = 4
M = 65535
IMPLS = {"tiled": CN.IMPL_TILED, "global": CN.IMPL_GLOBAL}
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


def measure(cands):
    """{name: fn} -> {name: [us per round]}: a warm-up, then alternating rounds"""
    for fn in cands.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in cands}
    for _ in range(args.rounds):
        for name, fn in cands.items():
            times[name].append(time_it(fn, args.reps))
    return times


for size in args.sizes:
    W = H = D = size
    S = W * H * D
    shape = (D, H, W)
    z, y, x = torch.meshgrid(torch.arange(D, device=DEV), torch.arange(H, device=DEV), torch.arange(W, device=DEV), indexing="ij")

    def balls(lab, n, seed, value, lo, hi):
        g = torch.Generator().manual_seed(seed)
        c = torch.randint(lo, hi, (n, 3), generator=g)
        r = torch.randint(2, 5, (n,), generator=g)
        for (cz, cy, cx), rr in zip(c.tolist(), r.tolist()):
            sub = (slice(cz - rr, cz + rr + 1), slice(cy - rr, cy + rr + 1), slice(cx - rr, cx + rr + 1))
            lab[sub] = torch.where(((z[sub] - cz) ** 2 + (y[sub] - cy) ** 2 + (x[sub] - cx) ** 2) <= rr * rr, value, lab[sub])
        return lab

    def solid_map(seed):
        """a ball of half the volume, its centre shifted by the seed, with 20 cavities well inside it"""
        r = (3.0 / (8.0 * np.pi)) ** (1.0 / 3.0) * size
        c = size / 2 - 0.5 + 0.25 * seed
        lab = (((z - c) ** 2 + (y - c) ** 2 + (x - c) ** 2) <= r * r).to(torch.int32)
        return balls(lab, 20, seed, 0, size // 3, 2 * size // 3).to(torch.uint16)

    def sparse_map(seed):
        return balls(torch.zeros(shape, dtype=torch.int32, device=DEV), 300, seed, 1, 5, size - 5).to(torch.uint16)

    for kind, make in (("solid", solid_map), ("sparse", sparse_map)):
        maps = [make(i) for i in range(NBUF)]
        scratch = torch.empty(max(CN.keep_largest_scratch_bytes(S, 2), CN.label_scratch_bytes(S, 2, M)), dtype=torch.uint8, device=DEV)
        work = torch.empty_like(maps[0])
        outs = (torch.empty(S, dtype=torch.int32, device=DEV), torch.empty((M + 1) * 12, dtype=torch.int64, device=DEV),
                torch.empty(2, dtype=torch.int64, device=DEV))
        k = [0]

        def nxt():
            k[0] = (k[0] + 1) % NBUF
            return maps[k[0]]

        def restore():
            work.view(torch.int16).copy_(nxt().view(torch.int16))

        def keep(c, impl):
            restore()
            CN.keep_largest(work, [1], 2, c, scratch=scratch, impl=impl)

        def label(c, impl):
            CN.label(nxt(), 2, [1], c, max_instances=M, impl=impl, scratch=scratch, out=outs)

        # the two impls compute the same bits
        same, found = {}, {}
        for c in CN.CONNECTIVITIES:
            res = {}
            for name, impl in IMPLS.items():
                inst, rows, info = CN.label(maps[0], 2, [1], c, max_instances=M, impl=impl, scratch=scratch)
                kept = maps[0].clone()
                CN.keep_largest(kept, [1], 2, c, scratch=scratch, impl=impl)
                res[name] = (inst, rows, info, kept.view(torch.int16))
            same[c] = all(torch.equal(a, b) for a, b in zip(res["tiled"], res["global"]))
            assert same[c], "IMPL_TILED and IMPL_GLOBAL differ at connectivity %d" % c
            found[c] = int(res["tiled"][2][0].item())
        cands = {"restore": restore}
        for c in CN.CONNECTIVITIES:
            for name, impl in IMPLS.items():
                cands["keep_largest c%d %s" % (c, name)] = lambda c=c, impl=impl: keep(c, impl)
                cands["label c%d %s" % (c, name)] = lambda c=c, impl=impl: label(c, impl)
        t = measure(cands)
        restore_us = statistics.median(t["restore"])
        emit(dict(tag=args.tag, name="restore %s %d^3" % (kind, size), call="restore", map=kind, dims=[W, H, D], us=round(restore_us, 1),
                  us_min=round(min(t["restore"]), 1), us_max=round(max(t["restore"]), 1), reps=args.reps, rounds=args.rounds, device=device))
        med = {}
        for call in ("keep_largest", "label"):
            for c in CN.CONNECTIVITIES:
                for name in IMPLS:
                    v = t["%s c%d %s" % (call, c, name)]
                    if call == "keep_largest":
                        v = [u - restore_us for u in v]
                    med[(call, c, name)] = (statistics.median(v), min(v), max(v))
        for call in ("keep_largest", "label"):
            for c in CN.CONNECTIVITIES:
                for name in IMPLS:
                    us, lo, hi = med[(call, c, name)]
                    emit(dict(tag=args.tag, name="%s c%d %s %d^3 %s" % (call, c, kind, size, name), call=call, connectivity=c, map=kind,
                              candidate=name, dims=[W, H, D], us=round(us, 1), us_min=round(lo, 1), us_max=round(hi, 1),
                              over_c6=round(us / med[(call, 6, name)][0], 3),
                              global_over_tiled=round(med[(call, c, "global")][0] / med[(call, c, "tiled")][0], 3),
                              instances=found[c], bitwise_equal=same[c], restore_us_subtracted=round(restore_us, 1) if call == "keep_largest" else 0,
                              reps=args.reps, rounds=args.rounds, buffers_rotated=NBUF, device=device))
        del maps
