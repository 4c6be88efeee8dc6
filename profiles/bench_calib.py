#!/usr/bin/env python3
"""The calibration tables' fused pass on the device (include/unet_calib.h) at 6 x 128^3, beside the two passes that read the same
planes -- the QC counts of include/unet_qc.h and the fused softmax pass of include/unet_postproc.h -- on the same buffers, the
candidates alternating in one process.  Two inputs:
  random      logits 4 * randn: every bin of every class is hit, runs of equal updates are short
  saturated   99 % background at p = 1 with a sprinkled structure: the workload's own case, where without run merging every voxel
              would update the same three addresses
and per input
  softmax, qc_counts            the yardsticks
  logits_lds, logits_global     unet_calib_tables over the logits under both impls
  probs_lds, probs_global       the same over probability planes (an ensemble state of one member)
  logits_lds_wrong              with the mask read and the correct / wrong byte map written
HIP events around `reps` calls (default 20) after a warm-up, repeated in `rounds` alternating rounds (default 7; the median and the
spread over rounds are reported).  The inputs rotate over NBUF buffers per kind, more than 256 MiB each way, so that no call finds
its data in the Infinity Cache.  Every row carries its algorithmic bytes, 4 * S * (C + 1) plus the mask and the byte map where they
take part, and the ratio of its time to the two yardsticks'.  One JSON line per row, printed and APPENDED to --out (default
profiles/calib_bench.jsonl) with the run's tag."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import unet_studio_amd as U  # noqa: E402,F401
from unet_studio_amd import calib as CB  # noqa: E402
from unet_studio_amd import ensemble as EN  # noqa: E402
from unet_studio_amd import postproc as P  # noqa: E402
from unet_studio_amd import qc as Q  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "calib_bench.jsonl"))
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--size", type=int, default=128)
ap.add_argument("--classes", type=int, default=6)
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


def make(kind):
    """-> (logits, label) of one buffer"""
    x = 4.0 * torch.randn((C,) + shape, generator=g, device=DEV)
    truth = torch.argmax(x + 2.0 * torch.randn((C,) + shape, generator=g, device=DEV), dim=0)     # right most of the time
    if kind == "saturated":
        bg = torch.rand(shape, generator=g, device=DEV) >= 0.01
        x[0][bg] = 30.0                                             # expf(-30) vanishes beside 1: p = (1, 0, ...) exactly
        for c in range(1, C):
            x[c][bg] = 0.0
        truth[bg] = 0
    return x.contiguous(), truth.to(torch.float32).contiguous()


inputs = {}
for kind in ("random", "saturated"):
    bufs = [make(kind) for _ in range(NBUF)]
    states = []
    for x, _ in bufs:
        st = EN.new_state(C, S, DEV)
        EN.accumulate(x, st, 1.0, True)
        states.append(st)
    inputs[kind] = (bufs, states)
mask = (torch.rand(S, generator=g, device=DEV) < 0.9).to(torch.uint8)
wrong = torch.empty(S, dtype=torch.uint8, device=DEV)
table = torch.empty(CB.table_len(C), dtype=torch.int64, device=DEV)
scratch = torch.empty(CB.scratch_bytes(C, S), dtype=torch.uint8, device=DEV)
qc_scratch = torch.empty(Q.qc_scratch_bytes(C, S), dtype=torch.uint8, device=DEV)
outs = dict(label_prob=torch.empty((C - 1,) + shape, device=DEV), fg_prob=torch.empty(shape, device=DEV),
            label=torch.empty(shape, dtype=torch.uint16, device=DEV))
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


def candidates(kind):
    bufs, states = inputs[kind]

    def logits_call(impl, with_wrong=False):
        def fn():
            x, t = bufs[nxt()]
            CB.tables(x, t.view(-1), mask=mask if with_wrong else None, out=table, wrong=wrong if with_wrong else None, impl=impl, scratch=scratch)
        return fn

    def probs_call(impl):
        def fn():
            i = nxt()
            CB.tables_from_probs(states[i], C, S, bufs[i][1].view(-1), out=table, impl=impl, scratch=scratch)
        return fn

    def softmax():
        P.softmax_call(bufs[nxt()][0], C, S, 0.5, outs["label_prob"], outs["fg_prob"], outs["label"])

    def qc_counts():
        x, t = bufs[nxt()]
        Q.qc_counts(x, t.view(-1), scratch=qc_scratch)

    plain = 4 * S * (C + 1)
    return {"softmax": (softmax, 4 * S * (C + C - 1 + 1) + 2 * S), "qc_counts": (qc_counts, plain),
            "logits_lds": (logits_call(CB.IMPL_LDS), plain), "logits_global": (logits_call(CB.IMPL_GLOBAL), plain),
            "probs_lds": (probs_call(CB.IMPL_LDS), plain), "probs_global": (probs_call(CB.IMPL_GLOBAL), plain),
            "logits_lds_wrong": (logits_call(CB.IMPL_LDS, True), plain + 2 * S)}


for kind in ("random", "saturated"):
    cands = candidates(kind)
    for fn, _ in cands.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in cands}
    for _ in range(args.rounds):
        for name, (fn, _) in cands.items():
            times[name].append(time_it(fn, args.reps))
    med = {name: statistics.median(t) for name, t in times.items()}
    for name, (_, nbytes) in cands.items():
        t = times[name]
        row = dict(tag=args.tag, name="%s %s %d x %d^3" % (name, kind, C, D), call=name, input=kind, classes=C, dims=[D, D, D],
                   us=round(med[name], 1), us_min=round(min(t), 1), us_max=round(max(t), 1), algorithmic_bytes=nbytes,
                   gb_per_s=round(nbytes / (med[name] * 1e-6) / 1e9, 1), hbm_fraction=round(nbytes / (med[name] * 1e-6) / HBM, 4),
                   us_over_softmax=round(med[name] / med["softmax"], 3), us_over_qc_counts=round(med[name] / med["qc_counts"], 3),
                   reps=args.reps, rounds=args.rounds, buffers_rotated=NBUF, device=device)
        print(json.dumps(row), flush=True)
        with open(args.out, "a") as f:
            f.write(json.dumps(row) + "\n")
