#!/usr/bin/env python3
"""Test-time mirroring (include/unet_mirror.h): unet_mirror_combine, the fused unet_mirror_postproc (label only; label + agreement;
the three postproc outputs; all four) and the unfused pair combine + unet_postproc_softmax with the same outputs, for K = 2, 4, 8
members at 128^3 and 192x224x192 with 6 classes, one row on the scalar path (the stack one float off 16-byte alignment), each
against the HBM floor of its algorithmic bytes; and profiles/bench_evaluate.py's 16 x 128^3 inference loop with the model chain and
`label` only, mirrored over xyz against not mirrored.  HIP events around 20 calls; the calls rotate over enough stacks that the data
cannot sit in the 256 MB Infinity Cache.  One JSON line per row, to the file named on the command line (default
profiles/mirror_bench.jsonl) and to stdout."""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import unet_studio_amd as U  # noqa: E402
from unet_studio_amd import mirror as MR  # noqa: E402
from unet_studio_amd import postproc as P  # noqa: E402

DEV = "cuda:0"
HBM = 8.0e12   # MI355X peak HBM bytes/s
C = 6
SP3 = ("label_prob", "fg_prob", "label")
path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "mirror_bench.jsonl")
rows = []


def emit(row):
    rows.append(row)
    print(json.dumps(row), flush=True)


def time_it(fn, reps=20):
    fn()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(reps):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / reps * 1e3   # us


def row(name, dims, K, nbuf, nbytes, us, **extra):
    emit(dict(row=name, dims=list(dims), out_c=C, members=K, stacks_rotated=nbuf, algorithmic_bytes=nbytes,
              floor_us_at_8TBs=nbytes / HBM * 1e6, us=us, hbm_fraction=nbytes / (us * 1e-6) / HBM, **extra))


device = torch.cuda.get_device_name(0)
for dims in ((128, 128, 128), (192, 224, 192)):
    W, H, D = dims
    S = W * H * D
    mean = torch.empty((C, D, H, W), device=DEV)
    lp = torch.empty((C - 1, D, H, W), device=DEV)
    fg = torch.empty((D, H, W), device=DEV)
    lab = torch.empty((D, H, W), dtype=torch.uint16, device=DEV)
    agr = torch.empty((D, H, W), dtype=torch.uint8, device=DEV)
    for axes in ("x", "xy", "xyz"):
        ms = MR.parse_axes(axes)
        K = len(ms)
        swap = ("x", [(0, 1), (2, 5)])
        sbytes = 4 * K * C * S
        nbuf = max(2, -(-800_000_000 // sbytes)) if sbytes < 800_000_000 else 1     # one stack above 800 MB evicts itself
        flat = [torch.randn(K * C * S + 4, device=DEV) * 3 for _ in range(nbuf)]
        k = [0]

        def stack(off=0):
            k[0] = (k[0] + 1) % nbuf
            return flat[k[0]][off:off + K * C * S].view(K, C, D, H, W)

        b_mean, b_lab = sbytes + 4 * C * S, sbytes + 2 * S
        b_all = sbytes + 4 * (C - 1) * S + 4 * S + 2 * S + S
        all_out = {"label_prob": lp, "fg_prob": fg, "label": lab, "agreement": agr}

        def unfused(outs):
            MR.combine(stack(), ms, swap, out={"mean": mean})
            P.softmax_call(mean, C, S, 0.5, *outs)

        row("combine", dims, K, nbuf, b_mean, time_it(lambda: MR.combine(stack(), ms, swap, out={"mean": mean})))
        row("combine+agreement", dims, K, nbuf, b_mean + S,
            time_it(lambda: MR.combine(stack(), ms, swap, True, True, out={"mean": mean, "agreement": agr})))
        t_f = time_it(lambda: MR.postproc_mirror(stack(), ms, swap, 0.5, ("label",), out={"label": lab}))
        row("postproc label", dims, K, nbuf, b_lab, t_f)
        t_u = time_it(lambda: unfused((None, None, lab)))
        # the pair also writes and re-reads the mean: its own algorithmic bytes
        row("combine + softmax label", dims, K, nbuf, b_mean + 4 * C * S + 2 * S, t_u, fused_over_unfused=t_f / t_u)
        t_f = time_it(lambda: MR.postproc_mirror(stack(), ms, swap, 0.5, ("label", "agreement"), out=all_out))
        row("postproc label + agreement", dims, K, nbuf, b_lab + S, t_f)

        def unfused_la():
            MR.combine(stack(), ms, swap, True, True, out={"mean": mean, "agreement": agr})
            P.softmax_call(mean, C, S, 0.5, None, None, lab)

        t_u = time_it(unfused_la)
        row("combine + softmax label + agreement", dims, K, nbuf, b_mean + S + 4 * C * S + 2 * S, t_u, fused_over_unfused=t_f / t_u)
        t_f = time_it(lambda: MR.postproc_mirror(stack(), ms, swap, 0.5, SP3, out=all_out))
        row("postproc label_prob fg_prob label", dims, K, nbuf, b_all - S, t_f)
        t_u = time_it(lambda: unfused((lp, fg, lab)))
        row("combine + softmax label_prob fg_prob label", dims, K, nbuf, b_mean + 4 * C * S + 4 * (C - 1) * S + 4 * S + 2 * S, t_u,
            fused_over_unfused=t_f / t_u)
        t_f = time_it(lambda: MR.postproc_mirror(stack(), ms, swap, 0.5, MR.OUTPUTS, out=all_out))
        row("postproc all outputs", dims, K, nbuf, b_all, t_f)

        def unfused_all():
            MR.combine(stack(), ms, swap, True, True, out={"mean": mean, "agreement": agr})
            P.softmax_call(mean, C, S, 0.5, lp, fg, lab)

        t_u = time_it(unfused_all)
        row("combine + softmax all outputs", dims, K, nbuf, b_mean + S + 4 * C * S + 4 * (C - 1) * S + 4 * S + 2 * S, t_u,
            fused_over_unfused=t_f / t_u)
        if K == 8:
            row("combine, scalar path", dims, K, nbuf, b_mean, time_it(lambda: MR.combine(stack(1), ms, swap, out={"mean": mean})))
            row("postproc label, scalar path", dims, K, nbuf, b_lab,
                time_it(lambda: MR.postproc_mirror(stack(1), ms, swap, 0.5, ("label",), out={"label": lab})))
        del flat
    del mean, lp, fg, lab, agr

n, nvol = 128, 16
rs = np.random.RandomState(0)
ios = [[rs.rand(n, n, n).astype(np.float32)] for _ in range(nvol)]
for dt in ("bf16", "fp32"):
    m = U.UNet3d(1, 6, U.default_feature(6), device=DEV, dtype=dt, seed=0)
    res = {}
    for name, kw in (("label", {}), ("label_mirror_xyz", {"mirror_axes": "xyz"}),
                     ("label_mirror_xyz_swap", {"mirror_axes": "xyz", "mirror_swap": ("x", [(1, 2), (3, 4)])})):
        ev = U.EvaluateUNet(m, postproc="model", outputs=("label",), **kw)
        ev.start(ios[:2])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ev.start(ios)
        res[name + "_ms_per_volume"] = (time.perf_counter() - t0) / nvol * 1e3
        assert not ev.aborted, ev.error_msg
    emit(dict(row="evaluate 16 x 128^3, out 6, model chain, label only", dtype=dt, device=device, **res))

with open(path, "w") as f:
    for r in rows:
        f.write(json.dumps(r) + "\n")
