#!/usr/bin/env python3
"""The blend of overlapping tiles (include/unet_tiles.h): unet_tiles_blend and unet_tiles_postproc for 27 tiles of 6 x 128^3 on a
228 x 228 x 320 canvas (3 x 3 x 3 tiles at overlap 0.25), HIP events, warm caches, the median of 20 runs -- next to a torch
device-to-device copy that moves the same number of bytes (it copies half the blend's algorithmic bytes: each is read and written),
timed in the same run.  Then the whole tiled evaluation of that volume (EvaluateUNet(fov_strategy="tiles") on a plain array, the
default architecture in bf16, the model's chain, `label` only) next to 27 bare forwards of 128^3, wall clock with a device
synchronisation, the median of 3.  Appends one JSON line to --out (default profiles/tiles_bench.jsonl)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import unet_studio_amd as U  # noqa: E402
from unet_studio_amd import tiles as TL  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "tiles_bench.jsonl"))
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--no-evaluate", action="store_true", help="the two kernels and the copy only")
args = ap.parse_args()

DEV = "cuda:0"
C, T, CANVAS, OV = 6, 128, (228, 228, 320), 0.25          # canvas (w, h, d)
plan = TL.plan_tiles(CANVAS, (T, T, T), OV)
assert plan == ([0, 50, 100], [0, 50, 100], [0, 96, 192])
cshape = CANVAS[::-1]
S, n = CANVAS[0] * CANVAS[1] * CANVAS[2], 27


def median_us(fn, reps):
    fn()
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3)
    return statistics.median(out)


stack = torch.randn((n, C, T, T, T), device=DEV) * 3
canvas = torch.empty((C,) + cshape, device=DEV)
lab = torch.empty(cshape, dtype=torch.uint16, device=DEV)
fg = torch.empty(cshape, device=DEV)
lp = torch.empty((C - 1,) + cshape, device=DEV)
read = 4 * C * n * T ** 3
res = dict(device=torch.cuda.get_device_name(0), out_c=C, tile=T, canvas=CANVAS, tiles=n, reps=args.reps)

b_blend = read + 4 * C * S
t = median_us(lambda: TL.blend(stack, plan, cshape, out=canvas), args.reps)
res.update(blend_us=round(t, 1), blend_bytes=b_blend, blend_gbps=round(b_blend / t / 1e3, 1))
src = torch.empty(b_blend // 8, device=DEV)
dst = torch.empty_like(src)
tc = median_us(lambda: dst.copy_(src), args.reps)
res.update(copy_us=round(tc, 1), copy_bytes_moved=8 * src.numel(), copy_gbps=round(8 * src.numel() / tc / 1e3, 1))
res["blend_fraction_of_copy_bandwidth"] = round(res["blend_gbps"] / res["copy_gbps"], 3)
del src, dst
for what, outs, wbytes in (("label", {"label": lab}, 2 * S), ("all", {"label_prob": lp, "fg_prob": fg, "label": lab}, (4 * C + 2) * S)):
    rbytes = read if what == "label" else read + 4 * (C - 1) * n * T ** 3          # label_prob reads the foreground planes again
    t = median_us(lambda: TL.postproc_tiles(stack, plan, cshape, 0.5, tuple(outs), out=outs), args.reps)
    res["postproc_%s_us" % what] = round(t, 1)
    res["postproc_%s_bytes" % what] = rbytes + wbytes
    res["postproc_%s_fraction_of_copy_bandwidth" % what] = round((rbytes + wbytes) / t / 1e3 / res["copy_gbps"], 3)
del stack, canvas, lp

if not args.no_evaluate:
    m = U.UNet3d(1, C, U.default_feature(C), device=DEV, dtype="bf16", seed=0)
    m.dim, m.voxel_size = (T, T, T), (1.0, 1.0, 1.0)
    io = np.random.RandomState(0).rand(*cshape).astype(np.float32)
    ev = U.EvaluateUNet(m, postproc="model", outputs=("label",), fov_strategy="tiles", tile_overlap=OV)

    def evaluate():
        out = ev.start([[io]])
        assert not ev.aborted, ev.error_msg
        return out

    x = torch.rand((1, 1, T, T, T), device=DEV)

    def forwards():
        with torch.no_grad():
            for i in range(n):
                m.forward(x, packs_current=i > 0)

    def wall_ms(fn, reps=3):
        fn()
        out = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            out.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(out)

    te, tf = wall_ms(evaluate), wall_ms(forwards)
    res.update(evaluate_tiles_ms=round(te, 1), forwards_27_ms=round(tf, 1), share_outside_forwards=round(1 - tf / te, 3))

print(json.dumps(res), flush=True)
with open(args.out, "a") as f:
    f.write(json.dumps(res) + "\n")
