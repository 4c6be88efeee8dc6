#!/usr/bin/env python3
"""The atlas preparation on the device (include/unet_atlas.h) at 192x224x192: for `reclassify` three candidates alternating in one
process --
  lds       UNET_ATLAS_IMPL_LDS: the votes gathered in a block's LDS table, flushed once
  global    UNET_ATLAS_IMPL_GLOBAL: the same run merging, every add global
  parent    the only route before these kernels: torch.bincount over atlas * T + tissue, argmax, torch.where, a second bincount
on three atlases over a tissue map of nested shells (tissues 0..4, uint8) --
  solid R=130, solid R=1000   every tissue's shell cut into blocks, one region per block, 2 % of the voxels given a random region
                              (wrong-tissue voxels the erase pass removes)
  random R=130                uniform random regions over uniform random tissues
All three are compared for equal bits (atlas, votes, majority, erased) before anything is timed; the row records the outcome.
HIP events around `reps` calls (default 50) after a warm-up, repeated in `rounds` alternating rounds (default 5; the median and the
spread over rounds are reported); the (tissue, atlas) pairs rotate over more than 256 MB so they cannot sit in the Infinity Cache,
and every timed call works on a fresh copy of its atlas (the call is in place), whose cost is measured as `copy` and subtracted.
Every row carries its algorithmic bytes -- the votes pass reads 2 B + tissue_bytes per voxel, the erase pass reads the same and
writes 2 B per erased voxel -- and the fraction of the 8 TB/s floor they amount to.
For `grow`: the solid R=130 atlas after reclassify with 10 % of each tissue's labels removed; the time with max_rounds = 100 and
with max_rounds = 600 (both far beyond convergence), the rounds that filled something, and the cost of one early-exited round
(the difference over 500).
One JSON line per row, printed and APPENDED to --out (default profiles/atlas_bench.jsonl) with the run's tag, so repeating the whole
command gives the run-to-run spread."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import unet_studio_amd as U  # noqa: E402,F401
from unet_studio_amd import atlas as A  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "atlas_bench.jsonl"))
ap.add_argument("--reps", type=int, default=50)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--tag", default="run")
args = ap.parse_args()

DEV = "cuda:0"
HBM = 8.0e12   # MI355X peak HBM bytes/s
CACHE = 256e6  # Infinity Cache
W, H, D = 192, 224, 192
S = W * H * D
T = 5
device = torch.cuda.get_device_name(0)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
z, y, x = torch.meshgrid(torch.arange(D, device=DEV), torch.arange(H, device=DEV), torch.arange(W, device=DEV), indexing="ij")


def tissue_map():
    """nested shells: tissue 4 innermost, 0 outside"""
    r = torch.sqrt(((x - W / 2) / (W / 2)) ** 2 + ((y - H / 2) / (H / 2)) ** 2 + ((z - D / 2) / (D / 2)) ** 2)
    return (4 - torch.floor(r / 0.22)).clamp(0, 4).to(torch.int32)


def solid_atlas(tis, R, seed):
    """every shell cut into R // 4 blocks, one region per (tissue, block); 2 % of the voxels get a random region 1..R"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    per = R // 4
    bx = 5
    bz = max(1, per // 25)
    by = max(1, per // (bx * bz))
    block = ((x * bx // W) + bx * ((y * by // H) + by * (z * bz // D))).to(torch.int32) % per
    a = torch.where(tis > 0, (tis - 1) * per + 1 + block, torch.zeros_like(tis))
    wrong = torch.rand((D, H, W), device=DEV, generator=g) < 0.02
    vals = torch.randint(1, R + 1, (D, H, W), device=DEV, generator=g, dtype=torch.int32)
    return torch.where(wrong, vals, a).to(torch.uint16)


def random_pair(R, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return (torch.randint(0, T, (D, H, W), device=DEV, generator=g, dtype=torch.int32).to(torch.uint8),
            torch.randint(0, R + 1, (D, H, W), device=DEV, generator=g, dtype=torch.int32).to(torch.uint16))


def time_it(fn, reps):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(reps):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / reps * 1e3   # us


def parent_route(tis, work, R):
    """torch only: what a caller had before these kernels.  Returns (votes, majority, erased); work is changed in place"""
    a = work.to(torch.int64)
    t = tis.to(torch.int64)
    votes = torch.bincount((a * T + t).view(-1), minlength=(R + 1) * T).view(R + 1, T)
    votes[0] = 0
    majority = votes.argmax(1)
    gone = (a > 0) & (t != majority[a])
    work.copy_(torch.where(gone, torch.zeros_like(a), a).to(torch.int32).to(torch.uint16))
    erased = torch.bincount(torch.where(gone, a, torch.zeros_like(a)).view(-1), minlength=R + 1)
    erased[0] = 0
    return votes, majority, erased


def u32(t):
    return t.view(torch.int32).to(torch.int64) & 0xFFFFFFFF


def emit(row):
    print(json.dumps(row), flush=True)
    with open(args.out, "a") as f:
        f.write(json.dumps(row) + "\n")


nbuf = int(CACHE // (3 * S)) + 2                             # > 256 MB of (tissue, atlas) pairs in rotation
tis_i32 = tissue_map()
tis_u8 = tis_i32.to(torch.uint8)
work = torch.empty((D, H, W), dtype=torch.uint16, device=DEV)
for kind, R in (("solid", 130), ("solid", 1000), ("random", 130)):
    if kind == "solid":
        pairs = [(tis_u8.clone(), solid_atlas(tis_i32, R, 100 + i)) for i in range(nbuf)]
    else:
        pairs = [random_pair(R, 200 + i) for i in range(nbuf)]
    scratch = torch.empty(A.atlas_scratch_bytes(S, R, T, 600), dtype=torch.uint8, device=DEV)
    k = [0]

    def nxt():
        k[0] = (k[0] + 1) % nbuf
        return pairs[k[0]]

    def run(impl):
        tis, src = nxt()
        work.copy_(src)
        A.reclassify(tis, work, R, T, impl=impl, scratch=scratch)

    def run_parent():
        tis, src = nxt()
        work.copy_(src)
        parent_route(tis, work, R)

    def run_copy():
        work.copy_(nxt()[1])

    # equal bits first
    tis, src = pairs[0]
    res = {}
    for name, impl in (("lds", A.IMPL_LDS), ("global", A.IMPL_GLOBAL)):
        w = src.clone()
        rep = A.reclassify(tis, w, R, T, impl=impl, scratch=scratch)
        res[name] = (w.view(torch.int16), u32(rep["votes"]), rep["majority"].to(torch.int64), u32(rep["erased"]))
    w = src.clone()
    pv, pm, pe = parent_route(tis, w, R)
    res["parent"] = (w.view(torch.int16), pv, pm, pe)
    same = {name: all(bool(torch.equal(p, q)) for p, q in zip(res[name], res["lds"])) for name in res}
    assert same["global"], "IMPL_LDS and IMPL_GLOBAL differ"
    n_erased = int(res["lds"][3].sum().item())
    del res, w, pv, pm, pe
    cands = {"lds": lambda: run(A.IMPL_LDS), "global": lambda: run(A.IMPL_GLOBAL), "parent": run_parent, "copy": run_copy}
    for name, fn in cands.items():                           # warm-up: every candidate
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in cands}
    for _ in range(args.rounds):                             # alternate the candidates
        for name, fn in cands.items():
            times[name].append(time_it(fn, max(2, args.reps // 5) if name == "parent" else args.reps))
    copy_us = statistics.median(times["copy"])
    nbytes = 2 * (2 + 1) * S + 2 * n_erased
    for name in ("lds", "global", "parent"):
        t = [v - copy_us for v in times[name]]
        us = statistics.median(t)
        emit(dict(tag=args.tag, name="reclassify %s R=%d %s" % (kind, R, name), call="reclassify", atlas=kind, n_regions=R, n_tissues=T,
                  candidate=name, dims=[W, H, D], us=round(us, 1), us_min=round(min(t), 1), us_max=round(max(t), 1),
                  copy_us=round(copy_us, 1), erased_voxels=n_erased, algorithmic_bytes=nbytes, floor_us=round(nbytes / HBM * 1e6, 2),
                  hbm_fraction=round(nbytes / (us * 1e-6) / HBM, 5), bitwise_equal_to_lds=same[name],
                  reps=max(2, args.reps // 5) if name == "parent" else args.reps, rounds=args.rounds, buffers_rotated=nbuf, device=device))

    if kind == "solid" and R == 130:
        # grow: the reclassified atlas with 10 % of each tissue's labels removed
        g = torch.Generator(device=DEV).manual_seed(7)
        srcs = []
        for i in range(nbuf):
            w = pairs[i][1].clone()
            A.reclassify(tis_u8, w, R, T, scratch=scratch)
            drop = torch.rand((D, H, W), device=DEV, generator=g) < 0.1
            srcs.append(torch.where(drop, torch.zeros_like(tis_i32), w.to(torch.int32)).to(torch.uint16))
        j = [0]
        info = {}

        def run_grow(max_rounds):
            j[0] = (j[0] + 1) % nbuf
            work.copy_(srcs[j[0]])
            info[max_rounds] = A.grow(tis_u8, work, T, [1, 2, 3, 4], max_rounds=max_rounds, smooth_rounds=1, scratch=scratch)

        def run_grow_copy():
            j[0] = (j[0] + 1) % nbuf
            work.copy_(srcs[j[0]])

        gc = {"grow100": lambda: run_grow(100), "grow600": lambda: run_grow(600), "copy": run_grow_copy}
        for fn in gc.values():
            fn()
        torch.cuda.synchronize()
        gt = {name: [] for name in gc}
        greps = max(2, args.reps // 5)
        for _ in range(args.rounds):
            for name, fn in gc.items():
                gt[name].append(time_it(fn, greps))
        gcopy = statistics.median(gt["copy"])
        med = {name: statistics.median([v - gcopy for v in gt[name]]) for name in ("grow100", "grow600")}
        for name, mr in (("grow100", 100), ("grow600", 600)):
            t = [v - gcopy for v in gt[name]]
            rep = u32(info[mr]["info"]).tolist()
            emit(dict(tag=args.tag, name="grow solid R=130 max_rounds=%d" % mr, call="grow", atlas=kind, n_regions=R, n_tissues=T,
                      max_rounds=mr, smooth_rounds=1, dims=[W, H, D], us=round(med[name], 1), us_min=round(min(t), 1),
                      us_max=round(max(t), 1), copy_us=round(gcopy, 1), fill_rounds=rep[0], converged=rep[1],
                      filled_voxels=int(u32(info[mr]["filled"]).sum().item()),
                      early_exit_round_us=round((med["grow600"] - med["grow100"]) / 500, 3), reps=greps, rounds=args.rounds,
                      buffers_rotated=nbuf, device=device))
        del srcs
    del pairs, scratch
