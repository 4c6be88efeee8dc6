#!/usr/bin/env python3
"""Times unet_qc_counts (include/unet_qc.h) with HIP events on the launch stream after a warm-up, at the model's default size
(192 x 224 x 192) with out_c = 6 (without and with the subject-label shift) and out_c = 130, and the reference's ATen sequence of
qc.cpp:86-135 (logsumexp / cat / argmax / ne / bincount) on the same device tensors for comparison.  Prints one JSON line per
configuration: microseconds per call, the algorithmic bytes -- 4 S (out_c + 1) for logits and label, + 4 S for input channel 0 with
the shift -- and the achieved fraction of 8 TB/s.  The two results are also checked equal.
  python profiles/bench_qc.py [--iters 50]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import unet_studio_amd as U  # noqa: E402,F401
from unet_studio_amd import qc as Q  # noqa: E402

HBM_PEAK = 8.0e12


def aten_counts(logits, label, k, image0, shift):
    """qc.cpp:86-135 (+ train.cpp:248-256) as the reference runs it, on the device"""
    if shift:
        label = torch.where(label != 0, label + float(shift), (image0 > 0).to(torch.float32))
    C = logits.shape[0]
    t = label.to(torch.int64)
    valid = t.ge(0).logical_and(t.lt(C))
    lg = logits.unsqueeze(0)
    cp = C
    if k:
        lg = torch.cat([torch.logsumexp(lg[:, :k], 1, True), lg[:, k:]], 1)
        t = torch.clamp_min(t - k + 1, 0)
        cp = C - k + 1
    bins = torch.where(valid, t.clamp(0, cp - 1), torch.full_like(t, cp))
    wrong = lg.argmax(1)[0].ne(t).logical_and(valid).to(torch.float32)
    return torch.stack([bins.bincount(None, cp + 1).to(torch.float64), bins.bincount(wrong, cp + 1).to(torch.float64)])


def time_us(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--dims", type=int, nargs=3, default=[192, 224, 192])
    a = ap.parse_args()
    dev = "cuda:0"
    S = a.dims[0] * a.dims[1] * a.dims[2]
    g = torch.Generator(device=dev).manual_seed(0)
    for C, k, shift in ((6, 0, 0), (6, 3, 2), (130, 0, 0)):
        logits = torch.randn(C, S, device=dev, generator=g)
        label = torch.randint(0, C, (S,), device=dev, generator=g).to(torch.float32)
        label[torch.rand(S, device=dev, generator=g) < 0.7] = 0.0          # mostly background
        image0 = torch.randn(S, device=dev, generator=g)
        scratch = torch.empty(Q.qc_scratch_bytes(C, S, k), dtype=torch.uint8, device=dev)
        run = lambda: Q.qc_counts(logits, label, k, image0 if shift else None, shift, scratch)
        got = run().cpu().to(torch.float64).view(2, -1)
        ref = aten_counts(logits, label, k, image0, shift).cpu()
        cp = got.shape[1]
        same = torch.equal(got, ref[:, :cp])
        us = time_us(run, a.iters)
        us_aten = time_us(lambda: aten_counts(logits, label, k, image0, shift), max(5, a.iters // 5))
        nbytes = 4 * S * (C + 1) + (4 * S if shift else 0)
        print(json.dumps({"dims": a.dims, "out_c": C, "collapse_before": k, "shift_by": shift, "voxels": S, "bytes": nbytes,
                          "qc_us": round(us, 2), "hbm_floor_us": round(nbytes / HBM_PEAK * 1e6, 2),
                          "frac_of_8TBps": round(nbytes / HBM_PEAK / (us * 1e-6), 3), "aten_us": round(us_aten, 1),
                          "speedup_vs_aten": round(us_aten / us, 1), "counts_equal_aten": same}), flush=True)
        del logits, label, image0, scratch


if __name__ == "__main__":
    main()
