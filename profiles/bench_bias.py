#!/usr/bin/env python3
"""The intensity-inhomogeneity correction on the device (include/unet_bias.h) at 128^3 and 256 x 256 x 192, on a shaded phantom (two
nested ellipsoids at 100 and 60 on a background, a gain of about +-30 %, 3 % noise) --
  sweep     one sweep at each g in (32, 16, 8, 4), lam 1, under UNET_BIAS_IMPL_NODE and UNET_BIAS_IMPL_VOXEL alternating in one
            process, beside the bytes a sweep must move: the int16 residual once per colour pass (8 x 2 B per voxel)
  fit       the default plan (bias.DEFAULT_LEVELS, DEFAULT_OUTER) under both
  apply     4 B read and 4 B written per voxel; with the gain output 4 B more
  logcode   4 B read and 4 B written per voxel
node and voxel are compared for equal bits before anything is timed.  HIP events around `reps` calls (default 5) after a warm-up,
repeated in `rounds` alternating rounds (default 5; the median and the spread over rounds are reported).  The volumes of apply and
logcode rotate over more than 256 MB so they cannot sit in the Infinity Cache; a sweep's residual (4 MB at 128^3, 25 MB at the large
size) is read 8 times in a row and is meant to stay resident, as it does inside a fit.  One JSON line per row, printed and APPENDED
to --out (default profiles/bias_bench.jsonl) with the run's tag."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import unet_studio_amd as U  # noqa: E402,F401
from unet_studio_amd import bias as BS  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "bias_bench.jsonl"))
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--sizes", default="128x128x128,256x256x192", help="W x H x D, comma separated")
ap.add_argument("--tag", default="run")
args = ap.parse_args()

DEV = "cuda:0"
CACHE = 256e6  # Infinity Cache
device = torch.cuda.get_device_name(0)
f32 = torch.float32
IMPLS = {"node": BS.IMPL_NODE, "voxel": BS.IMPL_VOXEL}


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


def phantom(w, h, d):
    z, y, x = torch.meshgrid(torch.arange(d, device=DEV), torch.arange(h, device=DEV), torch.arange(w, device=DEV), indexing="ij")
    xs, ys, zs = 2 * x / (w - 1) - 1, 2 * y / (h - 1) - 1, 2 * z / (d - 1) - 1
    rad = torch.sqrt((xs / 0.9) ** 2 + (ys / 0.85) ** 2 + (zs / 0.8) ** 2)
    labels = torch.where(rad < 0.55, 2, torch.where(rad < 1.0, 1, 0)).to(torch.uint8)
    gain = torch.exp2(0.2 * xs + 0.15 * (ys * ys - 0.5) - 0.1 * zs)
    gen = torch.Generator(device=DEV).manual_seed(0)
    level = torch.tensor([10.0, 100.0, 60.0], device=DEV)[labels.long()]
    return (level * gain * (1 + 0.03 * torch.randn(labels.shape, generator=gen, device=DEV))).to(f32).contiguous(), labels.contiguous()


def rounds_of(cands):
    """-> (times per candidate over the alternating rounds, the reps each used).  A candidate whose single call takes long (the
    voxel baseline at a large g: millions of 64-bit atomics on the two counters of a few hundred nodes) gets fewer reps, so that
    a round of it stays near 0.1 s; every candidate is still timed in every round"""
    reps = {}
    for name, fn in cands.items():
        fn()
        torch.cuda.synchronize()
        reps[name] = max(1, min(args.reps, int(1e5 / max(time_it(fn, 1), 1.0))))
    times = {name: [] for name in cands}
    for _ in range(args.rounds):
        for name, fn in cands.items():
            times[name].append(time_it(fn, reps[name]))
    return times, reps


for size in args.sizes.split(","):
    W, H, D = (int(v) for v in size.split("x"))
    S, shape = W * H * D, (D, H, W)
    volume, labels = phantom(W, H, D)
    q = BS.logcode(volume)
    classes = [1, 2]
    common = dict(tag=args.tag, size=[W, H, D], rounds=args.rounds, device=device)

    # ---- a sweep at each g, from the field and the residual a fit reaches there --------------------------------------------------------
    for g in (32, 16, 8, 4):
        B0 = torch.zeros(BS.lattice(shape, g), dtype=torch.int32, device=DEV)
        r = BS.residual(q, labels, classes, BS.levels(q, labels, classes, B0, g), BS.DEFAULT_CLIP)
        scratch = torch.empty(BS.sweep_scratch_bytes(shape, g), dtype=torch.uint8, device=DEV)
        fields = {}
        for name, impl in IMPLS.items():
            fields[name] = B0.clone()
            info = BS.sweep(r, fields[name], g, 1, impl=impl, scratch=scratch)
        assert torch.equal(fields["node"], fields["voxel"]), "IMPL_NODE and IMPL_VOXEL differ"
        work = {name: B0.clone() for name in IMPLS}
        cands = {name: (lambda name=name, impl=impl: BS.sweep(r, work[name], g, 1, impl=impl, scratch=scratch)) for name, impl in IMPLS.items()}
        times, used = rounds_of(cands)
        med = {name: statistics.median(v) for name, v in times.items()}
        for name in IMPLS:
            emit(dict(common, name="sweep g=%d %s" % (g, name), call="sweep", candidate=name, reps=used[name], g=g, lattice=list(B0.shape), us=round(med[name], 1),
                      us_min=round(min(times[name]), 1), us_max=round(max(times[name]), 1), bytes_read=16 * S,
                      gb_per_s=round(16 * S / med[name] / 1e3, 1), counted=int((r != BS.SKIP).sum().item()), visited=int(info[1].item()),
                      node_over_voxel=round(med["voxel"] / med["node"], 2)))

    # ---- the default fit ------------------------------------------------------------------------------------------------------------------
    scratch = torch.empty(BS.scratch_bytes(shape, BS.DEFAULT_LEVELS), dtype=torch.uint8, device=DEV)
    fits = {name: BS.fit(q, labels, classes, impl=impl, scratch=scratch) for name, impl in IMPLS.items()}
    assert torch.equal(fits["node"][0], fits["voxel"][0]) and torch.equal(fits["node"][1], fits["voxel"][1]), "the fits differ"
    rows = BS.summary(fits["node"][1])
    cands = {name: (lambda impl=impl: BS.fit(q, labels, classes, impl=impl, scratch=scratch)) for name, impl in IMPLS.items()}
    cands["default"] = lambda: BS.fit(q, labels, classes, scratch=scratch)
    times, used = rounds_of(cands)
    for name in cands:
        m = statistics.median(times[name])
        emit(dict(common, name="fit %s" % name, call="fit", candidate=name, reps=used[name], levels=BS.DEFAULT_LEVELS, outer=BS.DEFAULT_OUTER, us=round(m, 1),
                  us_min=round(min(times[name]), 1), us_max=round(max(times[name]), 1), sweeps=[r["sweeps"] for r in rows],
                  rms=[round(r["rms"], 4) for r in rows]))
    B, g = fits["node"][0], BS.DEFAULT_LEVELS[-1][0]
    emit(dict(common, name="quality", call="quality", cv_before=round(BS.cv(volume, labels, 1), 4),
              cv_after=round(BS.cv(BS.apply(volume, B, g), labels, 1), 4)))

    # ---- apply and logcode, over rotating buffers --------------------------------------------------------------------------------------------
    nbuf = int(CACHE // (4 * S)) + 2
    vols = [volume.clone() for _ in range(nbuf)]
    outs = [torch.empty(S, dtype=f32, device=DEV) for _ in range(nbuf)]
    gains = [torch.empty(S, dtype=f32, device=DEV) for _ in range(2)]
    codes = [torch.empty(S, dtype=torch.int32, device=DEV) for _ in range(nbuf)]
    k = [0]

    def nxt():
        k[0] += 1
        return k[0] % nbuf

    cands = {"apply": lambda: BS.apply(vols[nxt()], B, g, out=outs[nxt()]),
             "apply+gain": lambda: BS.apply(vols[nxt()], B, g, gain=gains[k[0] % 2], out=outs[nxt()]),
             "logcode": lambda: BS.logcode(vols[nxt()], out=codes[nxt()])}
    moved = {"apply": 8 * S, "apply+gain": 12 * S, "logcode": 8 * S}
    times, used = rounds_of(cands)
    for name in cands:
        m = statistics.median(times[name])
        emit(dict(common, name=name, call=name, reps=used[name], g=g, us=round(m, 1), us_min=round(min(times[name]), 1), us_max=round(max(times[name]), 1),
                  bytes_moved=moved[name], gb_per_s=round(moved[name] / m / 1e3, 1), buffers_rotated=nbuf))
    del vols, outs, gains, codes
