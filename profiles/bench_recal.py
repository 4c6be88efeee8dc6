#!/usr/bin/env python3
"""The recalibration pass on the device (include/unet_recal.h) at 6 x 128^3 with 1, 2, 4 and 8 candidates, beside the two passes that
read the same planes -- the fused softmax pass of include/unet_postproc.h and the calibration tables of include/unet_calib.h -- on
the same buffers, the candidates alternating in one process.  Logits 4 * randn with a truth that is right most of the time.
HIP events around `reps` calls (default 20) after a warm-up, repeated in `rounds` alternating rounds (default 7; the median and the
spread over rounds are reported).  The inputs rotate over NBUF buffers, more than 256 MiB, so that no call finds its data in the
Infinity Cache.  Every row carries its algorithmic bytes, 4 * S * (C + 1) (plus the mask where it takes part), the ratio of its time
to the two yardsticks', and what a round of qc.recalibration_qc buys per unit of time at that candidate count,
log2(K + 1) / (forward + pass), with the forward it re-runs at --forward-us (0.86 ms).  One JSON line per row,
printed and APPENDED to --out (default profiles/recal_bench.jsonl) with the run's tag."""
import argparse
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import unet_studio_amd as U  # noqa: E402,F401
from unet_studio_amd import calib as CB  # noqa: E402
from unet_studio_amd import postproc as P  # noqa: E402
from unet_studio_amd import recal as RC  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "recal_bench.jsonl"))
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--size", type=int, default=128)
ap.add_argument("--classes", type=int, default=6)
ap.add_argument("--forward-us", type=float, default=860.0)
ap.add_argument("--tag", default="run")
args = ap.parse_args()

DEV = "cuda:0"
HBM = 8.0e12   # MI355X peak HBM bytes/s
NBUF = 6
device = torch.cuda.get_device_name(0)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)

C, D = args.classes, args.size
shape = (D, D, D)
S = D ** 3
g = torch.Generator(device=DEV).manual_seed(0)


def make():
    x = 4.0 * torch.randn((C,) + shape, generator=g, device=DEV)
    truth = torch.argmax(x + 2.0 * torch.randn((C,) + shape, generator=g, device=DEV), dim=0)     # right most of the time
    return x.contiguous(), truth.to(torch.float32).contiguous()


bufs = [make() for _ in range(NBUF)]
mask = (torch.rand(S, generator=g, device=DEV) < 0.9).to(torch.uint8)
table = torch.empty(RC.TABLE_LEN, dtype=torch.int64, device=DEV)
scratch = torch.empty(RC.scratch_bytes(C, S), dtype=torch.uint8, device=DEV)
cb_table = torch.empty(CB.table_len(C), dtype=torch.int64, device=DEV)
cb_scratch = torch.empty(CB.scratch_bytes(C, S), dtype=torch.uint8, device=DEV)
outs = dict(label_prob=torch.empty((C - 1,) + shape, device=DEV), fg_prob=torch.empty(shape, device=DEV),
            label=torch.empty(shape, dtype=torch.uint16, device=DEV))
BETAS = [float(b) for b in RC.Solver().betas()]                     # round 1 of the default search
k = [0]


def nxt():
    k[0] = (k[0] + 1) % NBUF
    return k[0]


def time_it(fn, reps):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(reps):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / reps * 1e3   # us


def recal_call(K, with_mask=False):
    betas = BETAS[:K] if K > 1 else [1.0]

    def fn():
        x, t = bufs[nxt()]
        RC.eval_betas(x, t.view(-1), betas, mask=mask if with_mask else None, out=table, scratch=scratch)
    return fn


def softmax():
    P.softmax_call(bufs[nxt()][0], C, S, 0.5, outs["label_prob"], outs["fg_prob"], outs["label"])


def calib_tables():
    x, t = bufs[nxt()]
    CB.tables(x, t.view(-1), out=cb_table, scratch=cb_scratch)


plain = 4 * S * (C + 1)
cands = {"softmax": (softmax, 4 * S * (C + C - 1 + 1) + 2 * S, 0), "calib_tables": (calib_tables, plain, 0)}
for K in (1, 2, 4, 8):
    cands["recal_k%d" % K] = (recal_call(K), plain, K)
cands["recal_k8_mask"] = (recal_call(8, True), plain + S, 8)

for fn, _, _ in cands.values():
    for _ in range(3):
        fn()
torch.cuda.synchronize()
times = {name: [] for name in cands}
for _ in range(args.rounds):
    for name, (fn, _, _) in cands.items():
        times[name].append(time_it(fn, args.reps))
med = {name: statistics.median(t) for name, t in times.items()}
for name, (_, nbytes, K) in cands.items():
    t = times[name]
    row = dict(tag=args.tag, name="%s %d x %d^3" % (name, C, D), call=name, candidates=K, classes=C, dims=[D, D, D],
               us=round(med[name], 1), us_min=round(min(t), 1), us_max=round(max(t), 1), algorithmic_bytes=nbytes,
               gb_per_s=round(nbytes / (med[name] * 1e-6) / 1e9, 1), hbm_fraction=round(nbytes / (med[name] * 1e-6) / HBM, 4),
               us_over_softmax=round(med[name] / med["softmax"], 3), us_over_calib_tables=round(med[name] / med["calib_tables"], 3),
               reps=args.reps, rounds=args.rounds, buffers_rotated=NBUF, device=device)
    if K:
        row["forward_us"] = args.forward_us
        row["bits_per_ms"] = round(math.log2(K + 1) / ((args.forward_us + med[name]) * 1e-3), 4)
    print(json.dumps(row), flush=True)
    with open(args.out, "a") as f:
        f.write(json.dumps(row) + "\n")
