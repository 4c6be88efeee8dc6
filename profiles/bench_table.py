#!/usr/bin/env python3
"""The tables of a label map on the device (include/unet_table.h) at 256^3: for `regions` and for `overlap` three candidates
alternating in one process --
  lds       UNET_TABLE_IMPL_LDS: the rows below UNET_TABLE_LDS_ROWS gathered in a block's LDS table, one global update per touched row
  global    UNET_TABLE_IMPL_GLOBAL: the same run merging, every update a global atomic
  torch     the only route without these kernels: one pass per column -- bincount for the counts, scatter_add_ for the three sums,
            scatter_reduce_ amin / amax for the six extremes (regions); three bincounts (overlap)
on two uint16 maps --
  solid 400      8 x 10 x 5 blocks, one label per block: what a parcellation looks like, a unit of 8 voxels is one run
  random 65535   uniform random labels over all rows: no run merges, nearly every update misses the LDS table
All three are compared for equal bits before anything is timed; the row records the outcome.  HIP events around `reps` calls
(default 20; the torch route a fifth of that) after a warm-up, repeated in `rounds` alternating rounds (default 5; the median and the
spread over rounds are reported); the maps rotate over more than 256 MB so they cannot sit in the Infinity Cache.  Every row carries
its algorithmic bytes (2 B per voxel and map read once) and the fraction of the 8 TB/s floor they amount to.  One JSON line per
row, printed and APPENDED to --out (default profiles/table_bench.jsonl) with the run's tag."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import unet_studio_amd as U  # noqa: E402,F401
from unet_studio_amd import table as T  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "table_bench.jsonl"))
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--size", type=int, default=256)
ap.add_argument("--tag", default="run")
args = ap.parse_args()

DEV = "cuda:0"
HBM = 8.0e12   # MI355X peak HBM bytes/s
CACHE = 256e6  # Infinity Cache
W = H = D = args.size
S = W * H * D
device = torch.cuda.get_device_name(0)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
z, y, x = (v.contiguous().view(-1) for v in torch.meshgrid(torch.arange(D, device=DEV), torch.arange(H, device=DEV),
                                                            torch.arange(W, device=DEV), indexing="ij"))


def solid_map(seed):
    """8 x 10 x 5 blocks shifted by the seed, labels 1..400"""
    xs, ys, zs = (x + 3 * seed) % W, (y + 5 * seed) % H, (z + 7 * seed) % D
    return (1 + xs * 8 // W + 8 * (ys * 10 // H + 10 * (zs * 5 // D))).to(torch.int32).to(torch.uint16).view(D, H, W)


def random_map(L, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randint(0, L + 1, (D, H, W), device=DEV, generator=g, dtype=torch.int32).to(torch.uint16)


def read(lab, L):
    v = lab.view(-1).to(torch.int64)
    return torch.where(v > L, torch.zeros_like(v), v)


def torch_regions(lab, L):
    l = read(lab, L)
    cols = [torch.bincount(l, minlength=L + 1)]
    cols += [torch.zeros(L + 1, dtype=torch.int64, device=DEV).scatter_add_(0, l, c) for c in (x, y, z)]
    cols += [torch.full((L + 1,), dim, dtype=torch.int64, device=DEV).scatter_reduce_(0, l, c, "amin") for c, dim in ((x, W), (y, H), (z, D))]
    cols += [torch.full((L + 1,), -1, dtype=torch.int64, device=DEV).scatter_reduce_(0, l, c, "amax") for c in (x, y, z)]
    return torch.stack(cols, 1)


def torch_overlap(a, b, L):
    la, lb = read(a, L), read(b, L)
    both = torch.where(la == lb, la, torch.full_like(la, L + 1))
    return torch.stack([torch.bincount(la, minlength=L + 1), torch.bincount(lb, minlength=L + 1),
                        torch.bincount(both, minlength=L + 2)[:L + 1]], 1)


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


nbuf = int(CACHE // (2 * S)) + 2                             # > 256 MB of maps in rotation
for kind, L in (("solid", 400), ("random", 65535)):
    maps = [solid_map(i) if kind == "solid" else random_map(L, 300 + i) for i in range(nbuf)]
    # overlap's second map: the first with a tenth of its voxels redrawn
    others = []
    for i, m in enumerate(maps):
        g = torch.Generator(device=DEV).manual_seed(900 + i)
        redraw = torch.rand((D, H, W), device=DEV, generator=g) < 0.1
        others.append(torch.where(redraw, random_map(L, 600 + i).to(torch.int32), m.to(torch.int32)).to(torch.uint16))
    scratch = torch.empty(T.table_scratch_bytes(S, L), dtype=torch.uint8, device=DEV)
    rows10 = torch.empty((L + 1) * 10, dtype=torch.int64, device=DEV)
    rows3 = torch.empty((L + 1) * 3, dtype=torch.int64, device=DEV)
    k = [0]

    def nxt():
        k[0] = (k[0] + 1) % nbuf
        return k[0]

    calls = {
        "regions": {"lds": lambda: T.regions(maps[nxt()], L, impl=T.IMPL_LDS, out=rows10, scratch=scratch),
                    "global": lambda: T.regions(maps[nxt()], L, impl=T.IMPL_GLOBAL, out=rows10, scratch=scratch),
                    "torch": lambda: torch_regions(maps[nxt()], L)},
        "overlap": {"lds": lambda: T.overlap(maps[nxt()], others[k[0]], L, impl=T.IMPL_LDS, out=rows3, scratch=scratch),
                    "global": lambda: T.overlap(maps[nxt()], others[k[0]], L, impl=T.IMPL_GLOBAL, out=rows3, scratch=scratch),
                    "torch": lambda: torch_overlap(maps[nxt()], others[k[0]], L)},
    }
    for call, cands in calls.items():
        # equal bits first, on the same map
        res = {}
        for name, fn in cands.items():
            k[0] = nbuf - 1                                  # nxt() -> 0
            res[name] = fn().clone().view(L + 1, -1)
        same = {name: bool(torch.equal(res[name], res["lds"])) for name in res}
        assert same["global"], "IMPL_LDS and IMPL_GLOBAL differ"
        del res
        for fn in cands.values():                            # warm-up: every candidate
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        times = {name: [] for name in cands}
        for _ in range(args.rounds):                         # alternate the candidates
            for name, fn in cands.items():
                times[name].append(time_it(fn, max(2, args.reps // 5) if name == "torch" else args.reps))
        nbytes = 2 * S * (1 if call == "regions" else 2)
        med = {name: statistics.median(t) for name, t in times.items()}
        for name, t in times.items():
            emit(dict(tag=args.tag, name="%s %s L=%d %s" % (call, kind, L, name), call=call, map=kind, n_labels=L, candidate=name,
                      dims=[W, H, D], us=round(med[name], 1), us_min=round(min(t), 1), us_max=round(max(t), 1),
                      torch_over_this=round(med["torch"] / med[name], 2), global_over_lds=round(med["global"] / med["lds"], 3),
                      algorithmic_bytes=nbytes, floor_us=round(nbytes / HBM * 1e6, 2), hbm_fraction=round(nbytes / (med[name] * 1e-6) / HBM, 5),
                      bitwise_equal_to_lds=same[name], reps=max(2, args.reps // 5) if name == "torch" else args.reps, rounds=args.rounds,
                      buffers_rotated=nbuf, device=device))
    del maps, others, scratch
