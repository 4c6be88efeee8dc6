#!/usr/bin/env python3
"""The model ensemble's two passes on the device (include/unet_ensemble.h) at 6 x 128^3, beside the fused softmax pass of
include/unet_postproc.h on the same logits, the candidates alternating in one process --
  softmax            k_pp_softmax with label_prob, fg_prob and label wanted: the yardstick, the streaming pass this one is shaped on
  accumulate_first   the first member: the logits read, the C + 2 state planes written
  accumulate_next    a later member: the logits read, the state read and written
  finalize           every output wanted: the state read, label_prob / fg_prob / entropy / mutual_info and the label written
  finalize_label     the label alone
HIP events around `reps` calls (default 20) after a warm-up, repeated in `rounds` alternating rounds (default 7; the median and the
spread over rounds are reported).  The logits rotate over NBUF buffers and the states over NSTATE, 570 MB together, so that no call
finds its data in the 256 MiB Infinity Cache.  Every row carries its algorithmic bytes -- every plane a pass reads counted once,
although both the softmax pass (for label_prob) and a state of more than 8 channels read logits twice, the second time from cache
-- and the bytes per second they amount to.  One JSON line per row, printed and APPENDED to --out (default
profiles/ensemble_bench.jsonl) with the run's tag."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import unet_studio_amd as U  # noqa: E402,F401
from unet_studio_amd import ensemble as EN  # noqa: E402
from unet_studio_amd import postproc as P  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "ensemble_bench.jsonl"))
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--size", type=int, default=128)
ap.add_argument("--classes", type=int, default=6)
ap.add_argument("--tag", default="run")
args = ap.parse_args()

DEV = "cuda:0"
HBM = 8.0e12   # MI355X peak HBM bytes/s
NBUF, NSTATE = 6, 4
device = torch.cuda.get_device_name(0)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)

C, D = args.classes, args.size
shape = (D, D, D)
S = D ** 3
g = torch.Generator(device=DEV).manual_seed(0)
logits = [4.0 * torch.randn((C,) + shape, generator=g, device=DEV) for _ in range(NBUF)]
states = [EN.new_state(C, S, DEV) for _ in range(NSTATE)]
for k, st in enumerate(states):
    EN.accumulate(logits[k], st, 0.25, True)
outs = dict(label_prob=torch.empty((C - 1,) + shape, device=DEV), fg_prob=torch.empty(shape, device=DEV),
            label=torch.empty(shape, dtype=torch.uint16, device=DEV), entropy=torch.empty(shape, device=DEV),
            mutual_info=torch.empty(shape, device=DEV))
ALL = tuple(outs)
k = [0, 0]


def nxt(i, n):
    k[i] = (k[i] + 1) % n
    return k[i]


def time_it(fn, reps):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(reps):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / reps * 1e3   # us


cands = {
    "softmax": (lambda: P.softmax_call(logits[nxt(0, NBUF)], C, S, 0.5, outs["label_prob"], outs["fg_prob"], outs["label"]),
                4 * S * (C + C - 1 + 1) + 2 * S),
    "accumulate_first": (lambda: EN.accumulate(logits[nxt(0, NBUF)], states[nxt(1, NSTATE)], 0.25, True), 4 * S * (C + C + 2)),
    "accumulate_next": (lambda: EN.accumulate(logits[nxt(0, NBUF)], states[nxt(1, NSTATE)], 0.25, False), 4 * S * (C + 2 * (C + 2))),
    "finalize": (lambda: EN.finalize(states[nxt(1, NSTATE)], C, shape, 0.5, ALL, out=outs), 4 * S * (C + 2 + C - 1 + 3) + 2 * S),
    "finalize_label": (lambda: EN.finalize(states[nxt(1, NSTATE)], C, shape, 0.5, ("label",), out=outs), 4 * S * C + 2 * S),
}
for fn, _ in cands.values():
    for _ in range(3):
        fn()
torch.cuda.synchronize()
times = {name: [] for name in cands}
for _ in range(args.rounds):
    for name, (fn, _) in cands.items():
        times[name].append(time_it(fn, args.reps))
base = None
for name, (_, nbytes) in cands.items():
    t = times[name]
    med = statistics.median(t)
    gbs = [nbytes / (v * 1e-6) / 1e9 for v in t]
    row = dict(tag=args.tag, name="%s %d x %d^3" % (name, C, D), call=name, classes=C, dims=[D, D, D], us=round(med, 1),
               us_min=round(min(t), 1), us_max=round(max(t), 1), algorithmic_bytes=nbytes, gb_per_s=round(nbytes / (med * 1e-6) / 1e9, 1),
               gb_per_s_min=round(min(gbs), 1), gb_per_s_max=round(max(gbs), 1), hbm_fraction=round(nbytes / (med * 1e-6) / HBM, 4),
               reps=args.reps, rounds=args.rounds, buffers_rotated=[NBUF, NSTATE], device=device)
    if name == "softmax":
        base = row["gb_per_s"]
    else:
        row["gb_per_s_over_softmax"] = round(row["gb_per_s"] / base, 3)
    print(json.dumps(row), flush=True)
    with open(args.out, "a") as f:
        f.write(json.dumps(row) + "\n")
