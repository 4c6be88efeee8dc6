#!/usr/bin/env python3
"""The 3x3x3 binomial filter of the pre-processing chain (include/unet_preproc.h, gaussian_filter) at 256x256x180, C = 1 and C = 2:
three candidates alternating in one process --
  lds        k_preproc_filter_lds: a block marches along z, planes staged in LDS, the 27 taps in registers
  voxel      k_preproc_filter_voxel: one thread per voxel, 27 loads through the vector L1 (binomial3)
  plane_op   the only path with the same arithmetic before this kernel: postproc's gaussian_smoothing plane op on the same planes.
             It works in place, so it makes an EXTRA copy pass (planes -> scratch, then the filter back): it moves 16 B per voxel
             where the two above move 8.
HIP events around `reps` calls (default 50) after a warm-up, repeated in `rounds` alternating rounds (default 5; the median and the
spread over rounds are reported); the sources rotate over more than 256 MB so they cannot sit in the Infinity Cache.  Every row
carries its algorithmic bytes (8 B per voxel: one read, one write) and the fraction of the 8 TB/s floor they amount to.  The three
results are compared bitwise first.  One JSON line per row, printed and APPENDED to --out (default profiles/preproc_bench.jsonl)
with the run's tag, so repeating the whole command gives the run-to-run spread."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import unet_studio_amd as U  # noqa: E402,F401
from unet_studio_amd import postproc as P  # noqa: E402
from unet_studio_amd import preproc as PRE  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "preproc_bench.jsonl"))
ap.add_argument("--reps", type=int, default=50)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--tag", default="run")
args = ap.parse_args()

DEV = "cuda:0"
HBM = 8.0e12   # MI355X peak HBM bytes/s
CACHE = 256e6  # Infinity Cache
W, H, D = 256, 256, 180
S = W * H * D
device = torch.cuda.get_device_name(0)


def time_it(fn, reps):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(reps):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / reps * 1e3   # us


rows = []
for C in (1, 2):
    nbuf = int(CACHE // (4 * C * S)) + 2                     # > 256 MB of sources in rotation
    srcs = [torch.rand((C, D, H, W), device=DEV) for _ in range(nbuf)]
    dst = torch.empty((C, D, H, W), device=DEV)
    work = torch.empty((C, D, H, W), device=DEV)
    scratch = torch.empty(P.postproc_scratch_bytes(C + 1, S), dtype=torch.uint8, device=DEV)
    k = [0]

    def nxt():
        k[0] = (k[0] + 1) % nbuf
        return srcs[k[0]]

    def plane_op():                                          # in place on the planes themselves: sources stay intact on a copy
        work.copy_(nxt())
        P.plane_op_call(P.PP_SMOOTH, 0.0, (W, H, D), work, C, scratch)

    cands = {
        "lds": lambda: PRE.apply("gaussian_filter", nxt(), out=dst, impl=PRE.IMPL_LDS),
        "voxel": lambda: PRE.apply("gaussian_filter", nxt(), out=dst, impl=PRE.IMPL_VOXEL),
        "plane_op": plane_op,
        "copy": lambda: work.copy_(nxt()),                   # plane_op's source-preserving copy, subtracted from its row
    }
    # the three compute the same bits
    a = PRE.apply("gaussian_filter", srcs[0], impl=PRE.IMPL_LDS)
    b = PRE.apply("gaussian_filter", srcs[0], impl=PRE.IMPL_VOXEL)
    work.copy_(srcs[0])
    P.plane_op_call(P.PP_SMOOTH, 0.0, (W, H, D), work, C, scratch)
    same = bool(torch.equal(a, b) and torch.equal(a, work))
    del a, b
    for fn in cands.values():                                # warm-up: every candidate, every shape
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in cands}
    for _ in range(args.rounds):                             # alternate the candidates
        for name, fn in cands.items():
            times[name].append(time_it(fn, args.reps))
    copy_us = statistics.median(times["copy"])
    for name in ("lds", "voxel", "plane_op"):
        t = [v - copy_us for v in times[name]] if name == "plane_op" else times[name]
        us = statistics.median(t)
        nbytes = 8 * C * S
        rows.append(dict(tag=args.tag, name="gaussian_filter " + name, channels=C, dims=[W, H, D], us=round(us, 1),
                         us_min=round(min(t), 1), us_max=round(max(t), 1), algorithmic_bytes=nbytes,
                         hbm_fraction=round(nbytes / (us * 1e-6) / HBM, 4), bitwise_equal=same, reps=args.reps, rounds=args.rounds,
                         buffers_rotated=nbuf, device=device,
                         note="extra in-place copy pass inside (16 B/voxel moved); the bench's own source copy (%.1f us) subtracted"
                         % copy_us if name == "plane_op" else ""))
        print(json.dumps(rows[-1]), flush=True)
    del srcs, dst, work, scratch

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "a") as f:
    for r in rows:
        f.write(json.dumps(r) + "\n")
