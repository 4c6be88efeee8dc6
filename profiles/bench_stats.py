#!/usr/bin/env python3
"""The per-region intensity statistics on the device (include/unet_stats.h) at 256^3: for `moments`, `hist` and `quantiles` three
candidates alternating in one process --
  lds       UNET_STATS_IMPL_LDS: a block gathers its updates in LDS (moments: the rows below UNET_STATS_LDS_ROWS; histograms:
            UNET_STATS_LDS_SLOTS slots of UNET_STATS_SLOT_BINS counters behind a (row, bin) -> slot cache), one global update per
            touched entry
  global    UNET_STATS_IMPL_GLOBAL: the same run merging, every update a global atomic
  torch     the only route without these kernels: moments -- the codes in fp32, bincount for the four counts, scatter_add_ for the
            two sums, scatter_reduce_ amin / amax for the four extremes; hist -- one bincount of label * 256 + (q >> 8); quantiles --
            torch.sort of (label << 16) | code over the whole volume, a bincount for the row sizes and a gather at the ranks
on a uint16 map --
  solid 400      8 x 10 x 5 blocks, one label per block: what a parcellation looks like
  random 4095    uniform random labels over all rows: no run merges, nearly every histogram update misses the slot cache
and a float32 image --
  noise          smooth noise in [0, 1]: a 3 x 3 x 3 box filter over uniform noise, neighbouring voxels rarely share a code
  mask           a 0 / 1 mask in solid blocks: long runs of one (label, code) pair
All three are compared for equal bits before anything is timed; the row records the outcome.  HIP events around `reps` calls
(default 20; the torch route a fifth of that) after a warm-up, repeated in `rounds` alternating rounds (default 5; the median and the
spread over rounds are reported); the inputs rotate over more than 256 MB so they cannot sit in the Infinity Cache.  Every row carries
its algorithmic bytes (6 B per voxel and pass: 2 of the map, 4 of the image; one pass for moments and for hist, two for quantiles)
and the fraction of the 8 TB/s floor they amount to.  One JSON line per row, printed and APPENDED to --out (default
profiles/stats_bench.jsonl) with the run's tag."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import unet_studio_amd as U  # noqa: E402,F401
from unet_studio_amd import stats as S  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "stats_bench.jsonl"))
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--size", type=int, default=256)
ap.add_argument("--tag", default="run")
args = ap.parse_args()

DEV = "cuda:0"
HBM = 8.0e12   # MI355X peak HBM bytes/s
CACHE = 256e6  # Infinity Cache
W = H = D = args.size
V = W * H * D
LO, HI = 0.0, 1.0
PM = (50, 500, 950)
device = torch.cuda.get_device_name(0)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
z, y, x = (v.contiguous().view(-1) for v in torch.meshgrid(torch.arange(D, device=DEV), torch.arange(H, device=DEV),
                                                            torch.arange(W, device=DEV), indexing="ij"))


def solid_map(seed):
    """8 x 10 x 5 blocks shifted by the seed, labels 1..400"""
    xs, ys, zs = (x + 3 * seed) % W, (y + 5 * seed) % H, (z + 7 * seed) % D
    return (1 + xs * 8 // W + 8 * (ys * 10 // H + 10 * (zs * 5 // D))).to(torch.int32).to(torch.uint16).view(D, H, W)


def random_map(L, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randint(0, L + 1, (D, H, W), device=DEV, generator=g, dtype=torch.int32).to(torch.uint16)


def noise_image(seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    v = torch.rand((1, 1, D, H, W), device=DEV, generator=g)
    return torch.nn.functional.avg_pool3d(v, 3, stride=1, padding=1, count_include_pad=False).view(D, H, W).contiguous()


def mask_image(seed):
    xs, ys, zs = (x + 11 * seed) % W, (y + 3 * seed) % H, (z + 5 * seed) % D
    return ((xs * 5 // W + ys * 3 // H + zs * 4 // D) % 2).to(torch.float32).view(D, H, W)


def read(lab, L):
    v = lab.view(-1).to(torch.int64)
    return torch.where(v > L, torch.zeros_like(v), v)


def torch_codes(img):
    t = (img.view(-1) - LO) * (65536.0 / (HI - LO))                # fp32, one rounding each
    return torch.where(t < 0, 0, torch.where(t >= 65535.0, 65535, t.to(torch.int64)))


def torch_keys(img):
    b = img.view(-1).view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    return torch.where(b >> 31 != 0, b ^ 0xFFFFFFFF, b ^ 0x80000000)


def torch_moments(lab, img, L):
    """the images here hold no NaN, so every voxel has a code; the NaN column is counted all the same"""
    l, q, k, v = read(lab, L), torch_codes(img), torch_keys(img), img.view(-1)
    cols = [torch.bincount(l, minlength=L + 1)]
    cols += [torch.bincount(l[m], minlength=L + 1) for m in (v != v, v < LO, v > HI)]
    cols += [torch.zeros(L + 1, dtype=torch.int64, device=DEV).scatter_add_(0, l, c) for c in (q, q * q)]
    cols += [torch.full((L + 1,), 65536, dtype=torch.int64, device=DEV).scatter_reduce_(0, l, q, "amin"),
             torch.full((L + 1,), -1, dtype=torch.int64, device=DEV).scatter_reduce_(0, l, q, "amax"),
             torch.full((L + 1,), 0xFFFFFFFF, dtype=torch.int64, device=DEV).scatter_reduce_(0, l, k, "amin"),
             torch.full((L + 1,), -1, dtype=torch.int64, device=DEV).scatter_reduce_(0, l, k, "amax")]
    return torch.stack(cols, 1)


def torch_hist(lab, img, L):
    return torch.bincount(read(lab, L) * 256 + (torch_codes(img) >> 8), minlength=(L + 1) * 256).view(L + 1, 256)


def torch_quantiles(lab, img, L):
    l = read(lab, L)
    s = torch.sort((l << 16) | torch_codes(img)).values
    n = torch.bincount(l, minlength=L + 1)
    start = torch.cumsum(n, 0) - n
    pm = torch.tensor(PM, dtype=torch.int64, device=DEV)
    r = pm[None, :] * (n[:, None] - 1).clamp(min=0) // 1000
    got = s[(start[:, None] + r).clamp(max=V - 1)] & 0xFFFF
    return torch.where(n[:, None] > 0, got, -1).to(torch.int32)


def time_it(fn, reps):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(reps):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / reps * 1e3   # us


def emit(row):
    print(json.dumps(row), flush=True)
    with open(args.out, "a") as f:
        f.write(json.dumps(row) + "\n")


nbuf = int(CACHE // (6 * V)) + 2                             # > 256 MB of maps and images in rotation
for kind, L in (("solid", 400), ("random", 4095)):
    maps = [solid_map(i) if kind == "solid" else random_map(L, 300 + i) for i in range(nbuf)]
    for image in ("noise", "mask"):
        imgs = [noise_image(700 + i) if image == "noise" else mask_image(i) for i in range(nbuf)]
        scratch = torch.empty(S.stats_scratch_bytes(V, L, len(PM)), dtype=torch.uint8, device=DEV)
        rows10 = torch.empty((L + 1) * 10, dtype=torch.int64, device=DEV)
        rows256 = torch.empty((L + 1) * 256, dtype=torch.int64, device=DEV)
        rowsq = torch.empty((L + 1) * len(PM), dtype=torch.int32, device=DEV)
        k = [0]

        def nxt():
            k[0] = (k[0] + 1) % nbuf
            return k[0]

        def ours(call, impl, out):
            if call == "quantiles":
                return lambda: S.quantiles(maps[nxt()], imgs[k[0]], L, LO, HI, PM, impl=impl, out=out, scratch=scratch)
            return lambda: getattr(S, call)(maps[nxt()], imgs[k[0]], L, LO, HI, impl=impl, out=out, scratch=scratch)

        calls = {
            "moments": {"lds": ours("moments", S.IMPL_LDS, rows10), "global": ours("moments", S.IMPL_GLOBAL, rows10),
                        "torch": lambda: torch_moments(maps[nxt()], imgs[k[0]], L)},
            "hist": {"lds": ours("hist", S.IMPL_LDS, rows256), "global": ours("hist", S.IMPL_GLOBAL, rows256),
                     "torch": lambda: torch_hist(maps[nxt()], imgs[k[0]], L)},
            "quantiles": {"lds": ours("quantiles", S.IMPL_LDS, rowsq), "global": ours("quantiles", S.IMPL_GLOBAL, rowsq),
                          "torch": lambda: torch_quantiles(maps[nxt()], imgs[k[0]], L)},
        }
        for call, cands in calls.items():
            # equal bits first, on the same inputs
            res = {}
            for name, fn in cands.items():
                k[0] = nbuf - 1                              # nxt() -> 0
                res[name] = fn().clone().view(L + 1, -1)
            same = {name: bool(torch.equal(res[name], res["lds"])) for name in res}
            assert same["global"], "IMPL_LDS and IMPL_GLOBAL differ"
            del res
            for fn in cands.values():                        # warm-up: every candidate
                for _ in range(3):
                    fn()
            torch.cuda.synchronize()
            times = {name: [] for name in cands}
            for _ in range(args.rounds):                     # alternate the candidates
                for name, fn in cands.items():
                    times[name].append(time_it(fn, max(2, args.reps // 5) if name == "torch" else args.reps))
            nbytes = 6 * V * (2 if call == "quantiles" else 1)
            med = {name: statistics.median(t) for name, t in times.items()}
            for name, t in times.items():
                emit(dict(tag=args.tag, name="%s %s L=%d %s %s" % (call, kind, L, image, name), call=call, map=kind, image=image, n_labels=L,
                          candidate=name, dims=[W, H, D], us=round(med[name], 1), us_min=round(min(t), 1), us_max=round(max(t), 1),
                          torch_over_this=round(med["torch"] / med[name], 2), global_over_lds=round(med["global"] / med["lds"], 3),
                          algorithmic_bytes=nbytes, floor_us=round(nbytes / HBM * 1e6, 2),
                          hbm_fraction=round(nbytes / (med[name] * 1e-6) / HBM, 5), bitwise_equal_to_lds=same[name],
                          reps=max(2, args.reps // 5) if name == "torch" else args.reps, rounds=args.rounds, buffers_rotated=nbuf,
                          device=device))
        del imgs, scratch
    del maps
