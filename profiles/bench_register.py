#!/usr/bin/env python3
"""The parcellation of a subject on the device (include/unet_register.h): `joint_hist` at K = 25 maps, T = 5 tissues, subject 256^3,
template 157x189x136 (uint8 both), at strides 1, 2 and 4 -- three candidates alternating in one process --
  lds       UNET_REG_IMPL_LDS: the K*T*T counters gathered in a block's LDS table, flushed once
  global    UNET_REG_IMPL_GLOBAL: the same run merging, every add global
  torch     the only route before these kernels, per candidate: the positions in fp32 (one rounding per operation, as the header
            orders them), the inside test, a gather of the template and torch.bincount over a * T + b; 25 times
The template is nested ellipsoids (tissues 0..4), the subject is the template seen through an affine map, and the 25 maps are the
candidates of the search's first iteration from centre_init.  All three are compared for equal bits before anything is timed; the
row records the outcome.  HIP events around `reps` calls (default 20) after a warm-up, repeated in `rounds` alternating rounds
(default 5; the median and the spread over rounds are reported); the subjects rotate over more than 256 MB so they cannot sit in
the Infinity Cache (the template, a few MB, is meant to stay resident).  Every row carries the voxel-samples per second (counted
voxels x 25) and the subject bytes read.
Then a whole `search` with the defaults (max_iterations = 400: 800 launches enqueued, the ones after convergence return at once)
under both implementations: the time of the call from enqueue to completion, the iterations it ran, its score.
One JSON line per row, printed and APPENDED to --out (default profiles/register_bench.jsonl) with the run's tag."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import unet_studio_amd as U  # noqa: E402,F401
from unet_studio_amd import register as R  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "register_bench.jsonl"))
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--tag", default="run")
args = ap.parse_args()

DEV = "cuda:0"
CACHE = 256e6  # Infinity Cache
T, K = 5, 25
SW = SH = SD = 256
TW, TH, TD = 157, 189, 136
S = SW * SH * SD
F = np.float32
device = torch.cuda.get_device_name(0)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)


def emit(row):
    print(json.dumps(row), flush=True)
    with open(args.out, "a") as f:
        f.write(json.dumps(row) + "\n")


def time_it(fn, reps):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(reps):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / reps * 1e3   # us


def template_map():
    """nested ellipsoids: tissue 2 inside d < 1, 1 inside 0.6, 4 inside 0.15, 3 the lower cap"""
    z, y, x = torch.meshgrid(torch.arange(TD, device=DEV), torch.arange(TH, device=DEV), torch.arange(TW, device=DEV), indexing="ij")
    d = ((x - TW / 2) / (0.42 * TW)) ** 2 + ((y - TH / 2) / (0.42 * TH)) ** 2 + ((z - TD / 2) / (0.42 * TD)) ** 2
    t = torch.zeros((TD, TH, TW), dtype=torch.int32, device=DEV)
    t[d < 1] = 2
    t[d < 0.6] = 1
    t[d < 0.15] = 4
    t[(d < 1) & (z < TD / 2 - 0.55 * 0.42 * TD)] = 3
    return t.to(torch.uint8)


def sample(template, m, stride):
    """the torch route's gather: the template's tissue at the nearest voxel of map(counted subject voxel), 0 outside; fp32, every
    product and every sum its own kernel, so rounded as the header orders them.  Returns (b, the counted subject index)"""
    z, y, x = torch.meshgrid(torch.arange(0, SD, stride, device=DEV), torch.arange(0, SH, stride, device=DEV),
                             torch.arange(0, SW, stride, device=DEV), indexing="ij")
    xf, yf, zf = x.to(torch.float32), y.to(torch.float32), z.to(torch.float32)
    inside = None
    idx = []
    for r, dim in ((0, TW), (1, TH), (2, TD)):
        q = (((float(m[3 * r]) * xf + float(m[3 * r + 1]) * yf) + float(m[3 * r + 2]) * zf) + float(m[9 + r])) + 0.5
        ok = (q >= 0) & (q < float(dim))
        inside = ok if inside is None else inside & ok
        idx.append(torch.where(ok, torch.floor(q), torch.zeros_like(q)).to(torch.int64))
    b = template.view(-1)[(idx[2] * TH + idx[1]) * TW + idx[0]].to(torch.int64)
    return torch.where(inside, b, torch.zeros_like(b)), (z * SH + y) * SW + x


def torch_hist(subject, template, maps, stride):
    out = []
    for m in maps:
        b, at = sample(template, m, stride)
        a = subject.view(-1)[at.view(-1)].to(torch.int64)
        out.append(torch.bincount(a * T + b.view(-1), minlength=T * T))
    return torch.stack(out).view(K, T, T)


def first_candidates(init):
    """the 25 maps of the search's first iteration (level 0) from `init`, in float32 as the header orders the operations"""
    c = np.array(init, F)
    cx, cy, cz = F(SW // 2), F(SH // 2), F(SD // 2)
    for r in range(3):
        c[9 + r] = ((c[3 * r] * cx + c[3 * r + 1] * cy) + c[3 * r + 2] * cz) + c[9 + r]
    states = [c.copy()]
    for i in range(12):
        for sign in (1, -1):
            n = c.copy()
            n[i] = c[i] + F(R.DEFAULT_STEP[i]) if sign > 0 else c[i] - F(R.DEFAULT_STEP[i])
            states.append(n)
    maps = []
    for n in states:
        maps.append(list(n[:9]) + [n[9 + r] - ((n[3 * r] * cx + n[3 * r + 1] * cy) + n[3 * r + 2] * cz) for r in range(3)])
    return np.array(maps, F)


template = template_map()
true_map = [0.62, 0.03, 0, -0.025, 0.72, 0.02, 0, 0.015, 0.55, -2.0, 1.5, -1.0]      # subject voxel -> template position
subject0 = sample(template, true_map, 1)[0].to(torch.uint8).view(SD, SH, SW)
nbuf = int(CACHE // S) + 2
subjects = [subject0.clone() for _ in range(nbuf)]
m0, t0 = R.centre_init((SD, SH, SW), (1, 1, 1), (TD, TH, TW), (SW / TW, SH / TH, SD / TD))
init = list(m0) + list(t0)
maps = first_candidates(init)
hist = torch.empty(K * T * T, dtype=torch.uint32, device=DEV)
k = [0]


def nxt():
    k[0] = (k[0] + 1) % nbuf
    return subjects[k[0]]


for stride in (1, 2, 4):
    counted = len(range(0, SW, stride)) * len(range(0, SH, stride)) * len(range(0, SD, stride))
    res = {name: R.joint_hist(subject0, template, T, maps, stride=stride, impl=impl).view(torch.int32).to(torch.int64).clone()
           for name, impl in (("lds", R.IMPL_LDS), ("global", R.IMPL_GLOBAL))}
    res["torch"] = torch_hist(subject0, template, maps, stride)
    same = {name: bool(torch.equal(res[name], res["lds"])) for name in res}
    assert same["global"], "IMPL_LDS and IMPL_GLOBAL differ"
    assert int(res["lds"].sum().item()) == K * counted
    cands = {"lds": lambda: R.joint_hist(nxt(), template, T, maps, stride=stride, impl=R.IMPL_LDS, out=hist),
             "global": lambda: R.joint_hist(nxt(), template, T, maps, stride=stride, impl=R.IMPL_GLOBAL, out=hist),
             "torch": lambda: torch_hist(nxt(), template, maps, stride)}
    for fn in cands.values():
        fn()
    torch.cuda.synchronize()
    times = {name: [] for name in cands}
    for _ in range(args.rounds):
        for name, fn in cands.items():
            times[name].append(time_it(fn, 2 if name == "torch" else args.reps))
    med = {name: statistics.median(v) for name, v in times.items()}
    for name in cands:
        emit(dict(tag=args.tag, name="joint_hist stride=%d %s" % (stride, name), call="joint_hist", candidate=name, stride=stride, K=K,
                  n_tissues=T, subject=[SW, SH, SD], template=[TW, TH, TD], us=round(med[name], 1), us_min=round(min(times[name]), 1),
                  us_max=round(max(times[name]), 1), counted_voxels=counted, samples_per_us=round(K * counted / med[name], 1),
                  subject_bytes=counted, speedup_over_global=round(med["global"] / med[name], 3),
                  speedup_over_torch=round(med["torch"] / med[name], 2), bitwise_equal_to_lds=same[name],
                  reps=2 if name == "torch" else args.reps, rounds=args.rounds, buffers_rotated=nbuf, device=device))

# a whole search with the defaults
scratch = torch.empty(R.reg_scratch_bytes(S, T, 400), dtype=torch.uint8, device=DEV)
for name, impl in (("lds", R.IMPL_LDS), ("global", R.IMPL_GLOBAL)):
    out = {}

    def run():
        out["r"] = R.search(nxt(), template, T, init, max_iterations=400, impl=impl, scratch=scratch)

    run()
    torch.cuda.synchronize()
    t = [time_it(run, 2) for _ in range(args.rounds)]
    info = out["r"][2].cpu().tolist()
    emit(dict(tag=args.tag, name="search defaults %s" % name, call="search", candidate=name, K=K, n_tissues=T, subject=[SW, SH, SD],
              template=[TW, TH, TD], max_iterations=400, us=round(statistics.median(t), 1), us_min=round(min(t), 1), us_max=round(max(t), 1),
              iterations=info[0], converged=info[1], score=info[2], subject_nonzero=int((subject0 > 0).sum().item()),
              map=[round(float(v), 5) for v in out["r"][0].cpu().tolist()], reps=2, rounds=args.rounds, device=device))
