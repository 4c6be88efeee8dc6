#!/usr/bin/env python3
"""The starts of a registration on the device (include/unet_start.h), measured at 128^3 against 128^3, T = 5, n = 4:
  search_batched     unet_start_search under UNET_START_IMPL_BATCHED: four searches in lock-step inside the same launches
  search_sequential  the same four searches under UNET_START_IMPL_SEQUENTIAL: one after another through register's entry point
  reg_search         the yardstick: ONE plain register.search from centre_init on the same grids, in the same run
  find               one whole start.find (moments, candidates, rank, pick, search under the default implementation), from a host
                     clock around the call, ended by a device synchronise; reg_search_host: the plain search under the same clock
The template is tests/test_register_host.py's nested ellipsoids scaled to 128^3; the subject is the template seen through a
rotation of 15 degrees about z and -12 about x with an off-centre pivot (tests/start_ref.py's rot15, scaled).  The four starts are
those start.pick chooses; both implementations are compared for equal bits before anything is timed.  HIP events around `reps`
calls (default 2), warm, `runs` times per candidate (default 20) with the candidates alternating; the median, the minimum and the
maximum over the runs are recorded.  One JSON line, printed and APPENDED to --out (default profiles/start_bench.jsonl) with the
run's tag."""
import argparse
import json
import math
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import unet_studio_amd as U  # noqa: E402,F401
from unet_studio_amd import register as R  # noqa: E402
from unet_studio_amd import start as ST  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "start_bench.jsonl"))
ap.add_argument("--n", type=int, default=128)
ap.add_argument("--reps", type=int, default=2)
ap.add_argument("--runs", type=int, default=20)
ap.add_argument("--find-runs", type=int, default=10)
ap.add_argument("--tag", default="run")
args = ap.parse_args()

assert torch.cuda.is_available(), "bench_start.py measures on the GPU only"
DEV = "cuda:0"
N, T, NS = args.n, 5, 4
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)


def time_it(fn, reps):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(reps):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / reps * 1e3   # us


def rot(axis, degrees):
    p, q = ((1, 2), (0, 2), (0, 1))[axis]
    a = math.radians(degrees)
    r = np.eye(3)
    r[p, p] = r[q, q] = math.cos(a)
    r[p, q] = -math.sin(a)
    r[q, p] = math.sin(a)
    return r


k = N / 48.0
z, y, x = np.meshgrid(*(np.arange(N, dtype=np.float32),) * 3, indexing="ij")
c_t = np.array([19.5, 23.5, 17.5]) * k + (N - 40 * k) / 2
d = ((x - c_t[0]) / (15 * k)) ** 2 + ((y - c_t[1]) / (19 * k)) ** 2 + ((z - c_t[2]) / (14 * k)) ** 2
template = np.zeros((N, N, N), np.uint8)
template[d < 1] = 2
template[d < 0.6] = 1
template[d < 0.15] = 4
template[(d < 1) & (z < c_t[2] - 0.55 * 14 * k)] = 3
m = rot(2, 15) @ rot(0, -12)
true = np.concatenate([m.reshape(9), c_t - m @ (np.array([26, 21, 23]) * k + (N - 46 * k) / 2)]).astype(np.float32)
q = [np.floor(true[3 * r] * x + true[3 * r + 1] * y + true[3 * r + 2] * z + true[9 + r] + 0.5) for r in range(3)]
inside = (q[0] >= 0) & (q[0] < N) & (q[1] >= 0) & (q[1] < N) & (q[2] >= 0) & (q[2] < N)
idx = [np.where(inside, v, 0).astype(np.int64) for v in q]
subject = np.where(inside, template[idx[2], idx[1], idx[0]], 0).astype(np.uint8)
s_dev, t_dev = torch.from_numpy(subject).to(DEV), torch.from_numpy(template).to(DEV)
del x, y, z, d, q, idx, inside

# the four starts start.pick chooses, as find does
sm, tm = ST.moments(s_dev, 1, T - 1).cpu().numpy(), ST.moments(t_dev, 1, T - 1).cpu().numpy()
maps = ST.candidates(sm, tm)
scores, inits, picked = ST.pick(ST.rank(s_dev, t_dev, T, maps, stride=2), torch.from_numpy(maps).to(DEV), n=NS)
centre = np.concatenate(R.centre_init((N, N, N), (1, 1, 1), (N, N, N), (1, 1, 1)))
scratch = torch.empty(ST.start_scratch_bytes(T, NS), dtype=torch.uint8, device=DEV)
reg_scratch = torch.empty(R.reg_scratch_bytes(N ** 3, T, 400), dtype=torch.uint8, device=DEV)

row = dict(tag=args.tag, device=torch.cuda.get_device_name(0), subject=[N, N, N], template=[N, N, N], T=T, n=NS, reps=args.reps, runs=args.runs,
           picked=picked.cpu().tolist())
res = {impl: ST.search(s_dev, t_dev, T, inits, impl=impl, scratch=scratch) for impl in (ST.IMPL_BATCHED, ST.IMPL_SEQUENTIAL)}
for a, b in zip(res[ST.IMPL_BATCHED], res[ST.IMPL_SEQUENTIAL]):
    assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b), \
        "IMPL_BATCHED and IMPL_SEQUENTIAL differ"
info = res[ST.IMPL_BATCHED][2].cpu().numpy()
row["iterations"], row["converged"], row["best"] = info[:, 0].tolist(), info[:, 1].tolist(), int(res[ST.IMPL_BATCHED][3].cpu()[0])
plain = R.search(s_dev, t_dev, T, centre, trace=False, scratch=reg_scratch)
row["reg_search_iterations"] = int(plain[2].cpu()[0])


def dice(map12):
    h = R.joint_hist(s_dev, t_dev, T, [map12]).view(torch.int32).cpu().numpy()[0].astype(np.int64)
    agree = int(np.trace(h)) - int(h[0, 0])
    return round(2.0 * agree / (int(h[1:].sum()) + int(h[:, 1:].sum())), 4)


row["dice_best_of_4"], row["dice_from_centre_init"] = dice(res[ST.IMPL_BATCHED][4].cpu().numpy()), dice(plain[0].cpu().numpy())

cands = {
    "search_batched": lambda: ST.search(s_dev, t_dev, T, inits, impl=ST.IMPL_BATCHED, trace=False, scratch=scratch),
    "search_sequential": lambda: ST.search(s_dev, t_dev, T, inits, impl=ST.IMPL_SEQUENTIAL, trace=False, scratch=scratch),
    "reg_search": lambda: R.search(s_dev, t_dev, T, centre, trace=False, scratch=reg_scratch),
}
for fn in cands.values():                                           # warm
    for _ in range(2):
        fn()
torch.cuda.synchronize()
times = {name: [] for name in cands}
for _ in range(args.runs):                                          # alternating
    for name, fn in cands.items():
        times[name].append(time_it(fn, args.reps))
for name, v in times.items():
    row[name + "_us"] = round(statistics.median(v), 1)
    row[name + "_us_min_max"] = [round(min(v), 1), round(max(v), 1)]
row["batched_over_reg_search"] = round(row["search_batched_us"] / row["reg_search_us"], 3)
row["sequential_over_reg_search"] = round(row["search_sequential_us"] / row["reg_search_us"], 3)
row["search_faster"] = "batched" if row["search_batched_us"] <= row["search_sequential_us"] else "sequential"

# one whole find against one plain search, under a host clock ended by a device synchronise
hosted = {
    "find": lambda: ST.find(s_dev, t_dev, T, template_moments=tm, scratch=scratch),
    "reg_search_host": lambda: R.search(s_dev, t_dev, T, centre, trace=False, scratch=reg_scratch),
}
for name, fn in hosted.items():
    fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(args.find_runs):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        t.append((time.perf_counter() - t0) * 1e3)
    row[name + "_ms"] = round(statistics.median(t), 3)
    row[name + "_ms_min_max"] = [round(min(t), 3), round(max(t), 3)]
row["find_over_reg_search_host"] = round(row["find_ms"] / row["reg_search_host_ms"], 3)
print(json.dumps(row), flush=True)
with open(args.out, "a") as f:
    f.write(json.dumps(row) + "\n")
