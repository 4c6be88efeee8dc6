#!/usr/bin/env python3
"""Times the patch feed (patches.py, include/unet_patches.h) with HIP events on the launch stream, warm, as the median of 20 runs:
the index and one pick on a 228 x 228 x 320 canvas with 8 classes; the crop of a 128^3 window (one input channel and the label)
next to a torch device-to-device copy of the same number of bytes; and a whole WindowFeed sample next to a TrainingFeed sample at
the same model.dim = 128^3 (host decisions and recipe draws included).  The kernels and the copy are timed behind a spinning kernel,
so their intervals hold device time only; the two samples are timed as a stream sees one call.  Appends one JSON line to
profiles/patches_bench.jsonl.
  python profiles/bench_patches.py [--runs 20]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import unet_studio_amd as U  # noqa: E402
from unet_studio_amd import patches as P  # noqa: E402

DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))


def median_us(fn, runs, ahead=True):
    """ahead: a spinning kernel (no memory traffic) goes first, so the host has queued the events and the call before the device
    reaches them and the interval holds device time only; without it the interval is what a stream sees of one call, host included"""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        if ahead:
            torch.cuda._sleep(400000)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) * 1000.0)
    return round(statistics.median(out), 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    a = ap.parse_args()
    W, H, D, K, n = 228, 228, 320, 8, 128
    g = torch.Generator(device=DEV).manual_seed(0)
    # a canvas that is mostly background, with blocks of the classes 1..7
    lab = torch.zeros((D, H, W), device=DEV)
    for k in range(1, K):
        lab[30 * k:30 * k + 40, 20 * k:20 * k + 60, 60:160] = float(k)
    img = torch.rand((1, D, H, W), generator=g, device=DEV)
    idx = P.index(lab, K)
    origins = torch.empty((1, 4), dtype=torch.int32, device=DEV)
    pk = [(3, 0x80000000, 0x40000000, 0x40000000, 0x40000000)]
    x = torch.empty((1, n, n, n), device=DEV)
    l = torch.empty((n, n, n), device=DEV)
    src, dst = torch.rand(2 * n ** 3, generator=g, device=DEV), torch.empty(2 * n ** 3, device=DEV)
    row = {"canvas": [W, H, D], "classes": K, "window": [n, n, n], "runs": a.runs, "device": torch.cuda.get_device_name(0)}
    row["index_us"] = median_us(lambda: P.index(lab, K, out=idx), a.runs)
    row["pick_us"] = median_us(lambda: P.pick(lab, idx, K, pk, (n, n, n), out=origins), a.runs)
    row["crop_us"] = median_us(lambda: P.crop(img, lab, origins[0], (n, n, n), out=(x, l)), a.runs)
    row["crop_bytes"] = 2 * 2 * 4 * n ** 3                    # the window of the image and of the label, read and written
    row["torch_copy_us"] = median_us(lambda: dst.copy_(src), a.runs)
    row["crop_over_copy"] = round(row["crop_us"] / row["torch_copy_us"], 3)

    m = U.UNet3d(1, 8, U.default_feature(8), device=DEV, dtype="bf16", seed=0)
    m.dim = (n, n, n)
    param = U.TrainingParam(batch_size=2, seed=0)
    wf = U.WindowFeed(m, [("t", "tl", img, lab, True)], param)
    x0, l0 = P.crop(img, lab, origins[0], (n, n, n))
    tf = U.TrainingFeed(m, [("t", "tl", x0, l0, True)], param)
    row["window_feed_sample_us"] = median_us(lambda: wf(1), a.runs, ahead=False)
    row["training_feed_sample_us"] = median_us(lambda: tf(1), a.runs, ahead=False)
    row["window_over_training_feed"] = round(row["window_feed_sample_us"] / row["training_feed_sample_us"], 3)
    print(json.dumps(row), flush=True)
    with open(os.path.join(HERE, "patches_bench.jsonl"), "a") as f:
        f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
