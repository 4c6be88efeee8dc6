#!/usr/bin/env python3
"""Times the per-sample work of the template/subject feed (feed.TrainingFeed, include/unet_feed.h) at 128^3 with HIP events on the
launch stream after a warm-up: unet_feed_prepare (subject shift; normalize + shift), simulate_modality (with and without labels),
the augmentation (default options, a label volume) and unet_feed_target, then one whole TrainingFeed sample of a template and of a
shifted subject (host recipe draws included).  Prints one JSON line per step: microseconds per call, and for the feed kernels the
algorithmic bytes and the fraction of 8 TB/s.  The prepare rows restore the label before every call: the time of that copy alone is
subtracted.
  python profiles/bench_feed.py [--iters 50]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import unet_studio_amd as U  # noqa: E402
from unet_studio_amd import augment as G  # noqa: E402
from unet_studio_amd import feed as FD  # noqa: E402

HBM_PEAK = 8.0e12
DEV = "cuda:0"


def time_us(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1000.0 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    a = ap.parse_args()
    n = 128
    S = n ** 3
    g = torch.Generator(device=DEV).manual_seed(0)
    img = torch.rand(S, generator=g, device=DEV)
    lab0 = torch.randint(0, 4, (S,), generator=g, device=DEV).to(torch.float32)
    lab = lab0.clone()
    sc = torch.empty(FD.feed_scratch_bytes(S), dtype=torch.uint8, device=DEV)
    tgt = torch.empty(S, dtype=torch.int64, device=DEV)
    rows = []

    def row(step, us, nbytes=None):
        r = {"dims": [n, n, n], "step": step, "us": round(us, 2)}
        if nbytes:
            r.update(bytes=nbytes, hbm_floor_us=round(nbytes / HBM_PEAK * 1e6, 2), frac_of_8TBps=round(nbytes / HBM_PEAK * 1e6 / us, 3))
        rows.append(r)
        print(json.dumps(r), flush=True)

    def prep_shift():
        lab.copy_(lab0)
        FD.prepare(lab, img, shift_by=3, scratch=sc)
    copy_us = time_us(lambda: lab.copy_(lab0), a.iters)
    row("prepare_shift", time_us(prep_shift, a.iters) - copy_us, 12 * S)            # label read + write, image0 read

    def prep_norm_shift():
        lab.copy_(lab0)
        FD.prepare(lab, img, normalize=True, shift_by=3, scratch=sc)
    row("prepare_normalize_shift", time_us(prep_norm_shift, a.iters) - copy_us, 16 * S)   # + the max pass
    row("label_max", time_us(lambda: FD.label_max(lab0, scratch=sc), a.iters), 4 * S)
    row("target", time_us(lambda: FD.target(lab0, out=tgt, scratch=sc), a.iters), 12 * S)
    row("target_normalize", time_us(lambda: FD.target(lab0, normalize=True, out=tgt, scratch=sc), a.iters), 16 * S)

    t1w = img.clone()
    rl = G.sim_to_struct(G.make_simulate_recipe((n, n, n), 8, 1))
    rn = G.sim_to_struct(G.make_simulate_recipe((n, n, n), None, 1))
    ssc = G.simulate(rl, t1w, lab0)
    row("simulate_with_labels", time_us(lambda: G.simulate(rl, t1w, lab0, ssc), a.iters))
    row("simulate_without_labels", time_us(lambda: G.simulate(rn, t1w, None, ssc), a.iters))
    ra = G.to_struct(G.make_recipe(None, (n, n, n), 1, True, 7, label_depth=n))
    x, l2 = img.clone(), lab0.clone()
    asc = G.augment(ra, x, l2)
    row("augment", time_us(lambda: G.augment(ra, x, l2, asc), a.iters))

    m = U.UNet3d(1, 8, U.default_feature(8), device=DEV, dtype="bf16", seed=0)
    m.dim = (n, n, n)
    lab_s = (lab0 > 2).to(torch.float32)                     # max label 1 < 3: a shifted subject
    cases = [("t", "tl", img.view(1, n, n, n), lab0.view(n, n, n), True), ("s", "sl", img.view(1, n, n, n), lab_s.view(n, n, n), False)]
    feed = U.TrainingFeed(m, cases, U.TrainingParam(batch_size=2, seed=0))
    assert feed.sample_info(0) == (True, False) and feed.sample_info(1) == (False, True)
    row("feed_sample_template", time_us(lambda: feed(0), a.iters))
    row("feed_sample_shifted_subject", time_us(lambda: feed(1), a.iters))


if __name__ == "__main__":
    main()
