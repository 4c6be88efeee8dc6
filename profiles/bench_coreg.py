#!/usr/bin/env python3
"""The co-registration of two intensity images on the device (include/unet_coreg.h), measured at 128^3 against 128^3:
  joint_hist   K = 25 maps (the candidates of a search's first iteration from the identity), stride 1, at 16 and 32 bins, under
               UNET_COREG_IMPL_LDS and UNET_COREG_IMPL_GLOBAL
  reg_hist     the yardstick from before this module: register.joint_hist (unet_register.h) on tissue maps of the same two grids
               (T = 5, the phantom's classes), the same 25 maps, both implementations, in the same run
  align        one whole alignment with the defaults: ranges, codes, the search (max_iterations = 400) and the resampling, from a
               host clock around the call, ended by a device synchronise
The fixed image is a smooth four-class phantom with texture and noise; the moving image is another contrast of it seen through a
5 degree rotation, a scaling and a shift.  The images are a few MB and stay in the caches between calls, as they do between the
iterations of a search: that is the case a user runs.  The implementations are compared for equal bits before anything is timed.
HIP events around `reps` calls (default 10), warm, `runs` times per candidate (default 20) with the candidates alternating; the
median, the minimum and the maximum over the runs are recorded.  One JSON line, printed and APPENDED to --out (default
profiles/coreg_bench.jsonl) with the run's tag."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import unet_studio_amd as U  # noqa: E402,F401
from unet_studio_amd import coreg as CR  # noqa: E402
from unet_studio_amd import register as R  # noqa: E402
from unet_studio_amd import space as SP  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "coreg_bench.jsonl"))
ap.add_argument("--n", type=int, default=128)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--runs", type=int, default=20)
ap.add_argument("--align-runs", type=int, default=5)
ap.add_argument("--tag", default="run")
args = ap.parse_args()

assert torch.cuda.is_available(), "bench_coreg.py measures on the GPU only"
DEV = "cuda:0"
N, K = args.n, 25
F = np.float32
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)


def time_it(fn, reps):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(reps):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / reps * 1e3   # us


def blobs(seed):
    g = torch.Generator().manual_seed(seed)
    z, y, x = torch.meshgrid(*(torch.arange(N, device=DEV, dtype=torch.float32),) * 3, indexing="ij")
    v = torch.zeros((N, N, N), device=DEV)
    for _ in range(12):
        c = (0.2 + 0.6 * torch.rand(3, generator=g)) * N
        sigma = float(0.08 + 0.12 * torch.rand(1, generator=g)) * N
        amp = float(0.3 + 0.7 * torch.rand(1, generator=g))
        v += amp * torch.exp(-((x - float(c[0])) ** 2 + (y - float(c[1])) ** 2 + (z - float(c[2])) ** 2) / (2 * sigma ** 2))
    return v / v.max()


def first_candidates(step):
    """the 25 maps of a search's first iteration (level 0) from the identity, in float32 as the header orders the operations"""
    c = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], F)
    cx = cy = cz = F(N // 2)
    for r in range(3):
        c[9 + r] = ((c[3 * r] * cx + c[3 * r + 1] * cy) + c[3 * r + 2] * cz) + c[9 + r]
    states = [c.copy()]
    for i in range(12):
        for sign in (1, -1):
            n = c.copy()
            n[i] = c[i] + F(step[i]) if sign > 0 else c[i] - F(step[i])
            states.append(n)
    return np.array([list(n[:9]) + [n[9 + r] - ((n[3 * r] * cx + n[3 * r + 1] * cy) + n[3 * r + 2] * cz) for r in range(3)] for n in states], F)


g = torch.Generator(device=DEV).manual_seed(5)
b1 = blobs(1)
classes = (b1 > 0.15).to(torch.float32) + (b1 > 0.35) + (b1 > 0.6)
fixed = (classes / 3 + 0.15 * blobs(2) + 0.02 * torch.randn((N, N, N), device=DEV, generator=g)).contiguous()
other = (1 - torch.sqrt(torch.clamp(fixed / fixed.max(), min=0))).contiguous()
a = np.deg2rad(5.0)
m2f = np.diag([1.04, 0.97, 1.0]) @ np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
centre = np.full(3, N / 2.0)
t2f = centre + np.array([2.0, -1.5, 1.0]) * N / 32 - m2f @ centre
moving = (SP.resample(other, (N, N, N), (m2f.reshape(9), t2f), mode="linear") + 0.02 * torch.randn((N, N, N), device=DEV, generator=g)).contiguous()
fixed_tissue = classes.to(torch.uint8).contiguous()
moving_tissue = torch.round(SP.resample(classes.contiguous(), (N, N, N), (m2f.reshape(9), t2f), mode="linear")).to(torch.uint8).contiguous()
maps = first_candidates(CR.DEFAULT_STEP)
assert maps.shape == (K, 12)

row = dict(tag=args.tag, device=torch.cuda.get_device_name(0), fixed=[N, N, N], moving=[N, N, N], K=K, stride=1, reps=args.reps, runs=args.runs)
cands, codes = {}, {}
for bins in (16, 32):
    fc = CR.code(fixed, *CR.robust_range(fixed), bins)
    mc = CR.code(moving, *CR.robust_range(moving), bins)
    codes[bins] = (fc, mc)
    ref = CR.joint_hist(fc, mc, bins, maps, impl=CR.IMPL_LDS).view(torch.int32).clone()
    assert torch.equal(ref, CR.joint_hist(fc, mc, bins, maps, impl=CR.IMPL_GLOBAL).view(torch.int32)), "IMPL_LDS and IMPL_GLOBAL differ"
    assert int(ref.to(torch.int64).sum().item()) == K * N ** 3
    out = torch.empty(K * bins * (bins + 1), dtype=torch.uint32, device=DEV)
    for name, impl in (("lds", CR.IMPL_LDS), ("global", CR.IMPL_GLOBAL)):
        cands["coreg_hist_%d_%s" % (bins, name)] = (lambda fc=fc, mc=mc, bins=bins, impl=impl, out=out:
                                                     CR.joint_hist(fc, mc, bins, maps, impl=impl, out=out))
T = 5
reg_out = torch.empty(K * T * T, dtype=torch.uint32, device=DEV)
ref = R.joint_hist(fixed_tissue, moving_tissue, T, maps, impl=R.IMPL_LDS).view(torch.int32).clone()
assert torch.equal(ref, R.joint_hist(fixed_tissue, moving_tissue, T, maps, impl=R.IMPL_GLOBAL).view(torch.int32))
for name, impl in (("lds", R.IMPL_LDS), ("global", R.IMPL_GLOBAL)):
    cands["reg_hist_%s" % name] = lambda impl=impl: R.joint_hist(fixed_tissue, moving_tissue, T, maps, impl=impl, out=reg_out)

for fn in cands.values():                                           # warm: every shape the timed window uses
    for _ in range(3):
        fn()
torch.cuda.synchronize()
times = {name: [] for name in cands}
for _ in range(args.runs):                                          # alternating
    for name, fn in cands.items():
        times[name].append(time_it(fn, args.reps))
for name, v in times.items():
    row[name + "_us"] = round(statistics.median(v), 1)
    row[name + "_us_min_max"] = [round(min(v), 1), round(max(v), 1)]
yard = min(row["reg_hist_lds_us"], row["reg_hist_global_us"])
for bins in (16, 32):
    best = min(row["coreg_hist_%d_lds_us" % bins], row["coreg_hist_%d_global_us" % bins])
    row["coreg_hist_%d_faster" % bins] = "lds" if row["coreg_hist_%d_lds_us" % bins] <= row["coreg_hist_%d_global_us" % bins] else "global"
    row["coreg_hist_%d_over_reg_hist" % bins] = round(best / yard, 3)
    row["coreg_hist_%d_samples_per_us" % bins] = round(K * N ** 3 / best, 1)

# one whole alignment with the defaults, under both implementations
for name, impl in (("lds", CR.IMPL_LDS), ("global", CR.IMPL_GLOBAL)):
    res = CR.align(moving, (1, 1, 1), fixed, (1, 1, 1), impl=impl)  # warm
    torch.cuda.synchronize()
    t = []
    for _ in range(args.align_runs):
        t0 = time.perf_counter()
        res = CR.align(moving, (1, 1, 1), fixed, (1, 1, 1), impl=impl)
        torch.cuda.synchronize()
        t.append((time.perf_counter() - t0) * 1e3)
    info = res[1].cpu().tolist()
    row["align_%s_ms" % name] = round(statistics.median(t), 2)
    row["align_%s_ms_min_max" % name] = [round(min(t), 2), round(max(t), 2)]
    row["align_iterations"], row["align_converged"], row["align_score"] = info[0], info[1], info[2]
    row["align_map"] = [round(float(v), 5) for v in res[0].cpu().tolist()]
inv = np.linalg.inv(m2f)
truth = np.concatenate([inv.reshape(9), -inv @ t2f])
row["true_map"] = [round(float(v), 5) for v in truth]
print(json.dumps(row), flush=True)
with open(args.out, "a") as f:
    f.write(json.dumps(row) + "\n")
