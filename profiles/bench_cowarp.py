#!/usr/bin/env python3
"""The non-linear refinement of a co-registration on the device (include/unet_cowarp.h): one `sweep` per lattice spacing g in 16, 8,
4 at 16 and 32 bins, fixed 256^3, moving 157x189x136 (uint8 codes both) -- three candidates alternating in one process --
  node      UNET_COWARP_IMPL_NODE: a block (a wave at g = 4) per node of the active colour, W and the node's neighbourhood in LDS
  voxel     UNET_COWARP_IMPL_VOXEL: a thread per voxel, integer atomic adds into 8 counters per node, then a pick kernel
  tissue    warp.sweep (include/unet_warp.h) at the same shapes on the tissue maps the code images were rendered from: the yardstick,
            the same sweep with +1 / -1 in place of the table and without the histogram and the weights in front
The moving image is nested ellipsoids in one contrast plus noise; the fixed image is the same anatomy in another contrast, seen through
an affine map plus a smooth warp of a few voxels, so that a sweep from the zero field at step 128 moves nodes.  node and voxel are
compared for equal bits (the field after the sweep and its two counts) before anything is timed.  Every call starts from a copy of
the same field (the copy is inside the timed region of all three).  HIP events around `reps` calls (default 5) after a warm-up,
repeated in `rounds` alternating rounds (default 5; the median and the spread over rounds are reported); the fixed images rotate over
more than 256 MB so they cannot sit in the Infinity Cache (the moving image, a few MB, is meant to stay resident).
Then a whole `fit` with the defaults under both implementations (the call from enqueue to completion, and its report), and
`resample` beside space.resample (linear) through the same map.
One JSON line per row, printed and APPENDED to --out (default profiles/cowarp_bench.jsonl) with the run's tag."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import unet_studio_amd as U  # noqa: E402,F401
from unet_studio_amd import coreg as CR  # noqa: E402
from unet_studio_amd import cowarp as CW  # noqa: E402
from unet_studio_amd import space as SP  # noqa: E402
from unet_studio_amd import warp as W  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "cowarp_bench.jsonl"))
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--size", type=int, default=256, help="the fixed image's edge (256; smaller for a quick look)")
ap.add_argument("--tag", default="run")
args = ap.parse_args()

DEV = "cuda:0"
CACHE = 256e6  # Infinity Cache
T = 5
FW = FH = FD = args.size
MW, MH, MD = 157, 189, 136
S = FW * FH * FD
STEP = 128
device = torch.cuda.get_device_name(0)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
i64, f32 = torch.int64, torch.float32


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
    z, y, x = torch.meshgrid(torch.arange(MD, device=DEV), torch.arange(MH, device=DEV), torch.arange(MW, device=DEV), indexing="ij")
    d = ((x - MW / 2) / (0.42 * MW)) ** 2 + ((y - MH / 2) / (0.42 * MH)) ** 2 + ((z - MD / 2) / (0.42 * MD)) ** 2
    t = torch.zeros((MD, MH, MW), dtype=torch.int32, device=DEV)
    t[d < 1] = 2
    t[d < 0.6] = 1
    t[d < 0.15] = 4
    t[(d < 1) & (z < MD / 2 - 0.55 * 0.42 * MD)] = 3
    return t.to(torch.uint8)


def affine(m, x, y, z):
    xf, yf, zf = x.to(f32), y.to(f32), z.to(f32)
    return [((float(m[3 * r]) * xf + float(m[3 * r + 1]) * yf) + float(m[3 * r + 2]) * zf) + float(m[9 + r]) for r in range(3)]


def gather(template, q):
    """the template's tissue at the nearest voxel of the positions q (+ 0.5 already added), 0 outside"""
    inside, idx = None, []
    for v, dim in zip(q, (MW, MH, MD)):
        ok = (v >= 0) & (v < float(dim))
        inside = ok if inside is None else inside & ok
        idx.append(torch.where(ok, torch.floor(v), torch.zeros_like(v)).to(i64))
    b = template.view(-1)[(idx[2] * MH + idx[1]) * MW + idx[0]].to(i64)
    return torch.where(inside, b, torch.zeros_like(b))


def contrast(tissue, levels, seed):
    """a float32 image: a grey level per tissue plus N(0, 0.04) noise"""
    gen = torch.Generator(device=DEV).manual_seed(seed)
    return torch.tensor(levels, dtype=f32, device=DEV)[tissue.to(i64)] + 0.04 * torch.randn(tissue.shape, generator=gen, device=DEV)


template = template_map()
true_map = [0.62, 0.03, 0, -0.025, 0.72, 0.02, 0, 0.015, 0.55, -2.0, 1.5, -1.0]      # fixed voxel -> moving position
true_map = [v * 256.0 / args.size if e < 9 else v for e, v in enumerate(true_map)]
z, y, x = (v.reshape(-1) for v in torch.meshgrid(torch.arange(FD, device=DEV), torch.arange(FH, device=DEV), torch.arange(FW, device=DEV),
                                                 indexing="ij"))
p = affine(true_map, x, y, z)
smooth = [3 * torch.sin(y / 40.0), 3 * torch.cos(z / 35.0), 2.5 * torch.sin(x / 45.0 + 1)]
subject0 = gather(template, [(p[r] + smooth[r].to(f32)) + 0.5 for r in range(3)]).to(torch.uint8).view(FD, FH, FW)
del p, smooth, x, y, z
fixed_image = contrast(subject0, [0.05, 0.55, 0.85, 0.30, 0.70], 5)
moving_image = contrast(template, [0.05, 0.80, 0.35, 0.60, 0.15], 6)
nbuf = int(CACHE // S) + 2
subjects = [subject0.clone() for _ in range(nbuf)]
k = [0]


def nxt():
    k[0] = (k[0] + 1) % nbuf
    return k[0]


for bins in (16, 32):
    fixed0, moving = CR.code(fixed_image, 0.0, 1.0, bins), CR.code(moving_image, 0.0, 1.0, bins)
    fixeds = [fixed0.clone() for _ in range(nbuf)]
    for g in (16, 8, 4):
        limit = W.default_limit(true_map, g)
        shape = W.lattice((FD, FH, FW), g) + (3,)
        D0 = torch.zeros(shape, dtype=torch.int32, device=DEV)
        scratch = torch.empty(CW.scratch_bytes((FD, FH, FW), bins, [(g, 1, 1, 1, 0)]), dtype=torch.uint8, device=DEV)
        tscratch = torch.empty(W.scratch_bytes((FD, FH, FW), T, [(g, 1, 1, 1, 0)]), dtype=torch.uint8, device=DEV)
        D = {name: D0.clone() for name in ("node", "voxel", "tissue")}

        def run(name, b):
            D[name].copy_(D0)
            if name == "tissue":
                return W.sweep(subjects[b], template, T, true_map, D[name], g, STEP, limit, scratch=tscratch)
            return CW.sweep(fixeds[b], moving, bins, true_map, D[name], g, STEP, limit, impl=CW.IMPL_NODE if name == "node" else CW.IMPL_VOXEL,
                            scratch=scratch)

        info = {name: run(name, 0).cpu().tolist() for name in D}
        assert torch.equal(D["voxel"], D["node"]) and info["voxel"] == info["node"], "IMPL_NODE and IMPL_VOXEL differ"
        assert info["node"][0] > 0, "the sweep moved nothing: the timing would be that of an idle field"
        cands = {name: (lambda name=name: run(name, nxt())) for name in D}
        torch.cuda.synchronize()
        times = {name: [] for name in cands}
        for _ in range(args.rounds):
            for name, fn in cands.items():
                times[name].append(time_it(fn, args.reps))
        med = {name: statistics.median(v) for name, v in times.items()}
        for name in cands:
            emit(dict(tag=args.tag, name="sweep bins=%d g=%d %s" % (bins, g, name), call="sweep", candidate=name, bins=bins, g=g, step=STEP,
                      limit=limit, fixed=[FW, FH, FD], moving=[MW, MH, MD], lattice=list(shape[:3]), us=round(med[name], 1),
                      us_min=round(min(times[name]), 1), us_max=round(max(times[name]), 1), nodes_changed=info[name][0],
                      nodes_visited=info[name][1], voxel_candidates_per_us=round(7 * S / med[name], 1),
                      speedup_over_voxel=round(med["voxel"] / med[name], 3), time_over_tissue=round(med[name] / med["tissue"], 3),
                      bitwise_equal_to_node=None if name == "tissue" else True, reps=args.reps, rounds=args.rounds, buffers_rotated=nbuf,
                      device=device))

    if bins == 16:   # a whole fit with the defaults
        levels = W.levels_of(W.DEFAULT_LEVELS, None, true_map)
        scratch = torch.empty(CW.scratch_bytes((FD, FH, FW), bins, levels), dtype=torch.uint8, device=DEV)
        fields = {}
        for name, impl in (("node", CW.IMPL_NODE), ("voxel", CW.IMPL_VOXEL)):
            out = {}

            def fit():
                out["r"] = CW.fit(fixeds[nxt()], moving, bins, true_map, levels=levels, impl=impl, scratch=scratch)

            fit()
            torch.cuda.synchronize()
            t = [time_it(fit, 1) for _ in range(args.rounds)]
            fields[name] = out["r"][0].clone()
            rows = out["r"][1].cpu().numpy()
            rows = rows[rows[:, 0] >= 0]
            zero = torch.zeros(W.lattice((FD, FH, FW), 16) + (3,), dtype=torch.int32, device=DEV)
            emit(dict(tag=args.tag, name="fit defaults %s" % name, call="fit", candidate=name, bins=bins, fixed=[FW, FH, FD], moving=[MW, MH, MD],
                      levels=levels.tolist(), us=round(statistics.median(t), 1), us_min=round(min(t), 1), us_max=round(max(t), 1),
                      report=rows.tolist(), score_affine=CW.score(CW.hist(fixed0, moving, bins, true_map, zero, 16)),
                      max_disp_q8=int(fields[name].abs().max().item()), bitwise_equal_to_node=bool(torch.equal(fields[name], fields["node"])),
                      reps=1, rounds=args.rounds, device=device))

        # resample through map + field beside space.resample through the map alone
        images = [moving_image.clone() for _ in range(int(CACHE // (4 * moving_image.numel())) + 2)]
        outs = [torch.empty((FD, FH, FW), dtype=f32, device=DEV) for _ in range(int(CACHE // (4 * S)) + 2)]
        j = [0]

        def bufs():
            j[0] += 1
            return images[j[0] % len(images)], outs[j[0] % len(outs)]

        m = (true_map[:9], true_map[9:])
        cands = {"cowarp": lambda: CW.resample(bufs()[0], (FD, FH, FW), true_map, fields["node"], 4, out=bufs()[1].view(-1)),
                 "space": lambda: SP.resample(bufs()[0], (FD, FH, FW), m, mode="linear", out=bufs()[1])}
        zero4 = torch.zeros_like(fields["node"])
        assert torch.equal(CW.resample(moving_image, (FD, FH, FW), true_map, zero4, 4), SP.resample(moving_image, (FD, FH, FW), m, mode="linear"))
        for fn in cands.values():
            fn()
        torch.cuda.synchronize()
        times = {name: [] for name in cands}
        for _ in range(args.rounds):
            for name, fn in cands.items():
                times[name].append(time_it(fn, args.reps))
        for name in cands:
            med = statistics.median(times[name])
            emit(dict(tag=args.tag, name="resample %s" % name, call="resample", candidate=name, fixed=[FW, FH, FD], moving=[MW, MH, MD], g=4,
                      us=round(med, 1), us_min=round(min(times[name]), 1), us_max=round(max(times[name]), 1),
                      gb_per_s_written=round(4 * S / med / 1e3, 1), zero_field_bitwise_equal_to_space=True, reps=args.reps, rounds=args.rounds,
                      device=device))
        del images, outs
