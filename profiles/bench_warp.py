#!/usr/bin/env python3
"""The non-linear refinement of a parcellation on the device (include/unet_warp.h): one `sweep` per lattice spacing g in 32, 16, 8, 4
at T = 5 tissues, subject 256^3, template 157x189x136 (uint8 both) -- three candidates alternating in one process --
  node      UNET_WARP_IMPL_NODE: a block (a wave at g = 4) per node of the active colour, seven sums in registers
  voxel     UNET_WARP_IMPL_VOXEL: a thread per voxel, integer atomic adds into 7 counters per node, then a pick kernel
  torch     the only route before these kernels, per colour: the owning node of every voxel, the corner sums in int64, the positions
            in fp32 (one rounding per operation, as the header orders them), a gather of the template, the vote, and one index_add_
            per candidate into the nodes' scores; then the admissibility, the choice and the update of the field
The template is nested ellipsoids (tissues 0..4); the subject is the template seen through an affine map plus a smooth warp of a few
voxels, so that a sweep from the zero field at step 128 moves nodes.  All three are compared for equal bits (the field after the
sweep and its two counts) before anything is timed; the row records the outcome.  Every call starts from a copy of the same field
(the copy is inside the timed region of all three).  HIP events around `reps` calls (default 5; the torch route 1) after a warm-up,
repeated in `rounds` alternating rounds (default 5; the median and the spread over rounds are reported); the subjects rotate over
more than 256 MB so they cannot sit in the Infinity Cache (the template, a few MB, is meant to stay resident).
Then a whole `fit` with the defaults under both implementations: the time of the call from enqueue to completion and its report.
One JSON line per row, printed and APPENDED to --out (default profiles/warp_bench.jsonl) with the run's tag."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import unet_studio_amd as U  # noqa: E402,F401
from unet_studio_amd import warp as W  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "warp_bench.jsonl"))
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--size", type=int, default=256, help="the subject's edge (256; smaller for a quick look)")
ap.add_argument("--tag", default="run")
args = ap.parse_args()

DEV = "cuda:0"
CACHE = 256e6  # Infinity Cache
T = 5
SW = SH = SD = args.size
TW, TH, TD = 157, 189, 136
S = SW * SH * SD
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
    z, y, x = torch.meshgrid(torch.arange(TD, device=DEV), torch.arange(TH, device=DEV), torch.arange(TW, device=DEV), indexing="ij")
    d = ((x - TW / 2) / (0.42 * TW)) ** 2 + ((y - TH / 2) / (0.42 * TH)) ** 2 + ((z - TD / 2) / (0.42 * TD)) ** 2
    t = torch.zeros((TD, TH, TW), dtype=torch.int32, device=DEV)
    t[d < 1] = 2
    t[d < 0.6] = 1
    t[d < 0.15] = 4
    t[(d < 1) & (z < TD / 2 - 0.55 * 0.42 * TD)] = 3
    return t.to(torch.uint8)


def affine(m, x, y, z):
    """p per axis in fp32: every product and every sum its own kernel, so rounded as the header orders them"""
    xf, yf, zf = x.to(f32), y.to(f32), z.to(f32)
    return [((float(m[3 * r]) * xf + float(m[3 * r + 1]) * yf) + float(m[3 * r + 2]) * zf) + float(m[9 + r]) for r in range(3)]


def gather(template, q):
    """the template's tissue at the nearest voxel of the positions q (+ 0.5 already added), 0 outside"""
    inside, idx = None, []
    for v, dim in zip(q, (TW, TH, TD)):
        ok = (v >= 0) & (v < float(dim))
        inside = ok if inside is None else inside & ok
        idx.append(torch.where(ok, torch.floor(v), torch.zeros_like(v)).to(i64))
    b = template.view(-1)[(idx[2] * TH + idx[1]) * TW + idx[0]].to(i64)
    return torch.where(inside, b, torch.zeros_like(b))


def owner(x, g, lg, parity):
    cell, f = x >> lg, x & (g - 1)
    return torch.where((cell & 1) == parity, cell, torch.where(f == 0, torch.full_like(cell, -1), cell + 1))


def torch_sweep(subject, template, m, D, g, step, limit):
    """one sweep of the header's definition in torch ops; D int32 {nz, ny, nx, 3} in place; returns (changed, visited) tensors"""
    lg = {4: 2, 8: 3, 16: 4, 32: 5}[g]
    nz, ny, nx = D.shape[:3]
    nodes = nz * ny * nx
    z, y, x = (v.reshape(-1) for v in torch.meshgrid(torch.arange(SD, device=DEV), torch.arange(SH, device=DEV), torch.arange(SW, device=DEV),
                                                     indexing="ij"))
    a_all, p_all = subject.view(-1).to(i64), affine(m, x, y, z)
    changed, visited = torch.zeros((), dtype=i64, device=DEV), torch.zeros((), dtype=i64, device=DEV)
    idx = torch.meshgrid(torch.arange(nz, device=DEV), torch.arange(ny, device=DEV), torch.arange(nx, device=DEV), indexing="ij")
    for c in range(8):
        i, j, k = owner(x, g, lg, c & 1), owner(y, g, lg, (c >> 1) & 1), owner(z, g, lg, c >> 2)
        act = torch.nonzero((i >= 0) & (j >= 0) & (k >= 0)).view(-1)
        xa, ya, za, ia, ja, ka, a = x[act], y[act], z[act], i[act], j[act], k[act], a_all[act]
        p = [v[act] for v in p_all]
        node = (ka * ny + ja) * nx + ia
        D64 = D.to(i64)
        fx, fy, fz = xa & (g - 1), ya & (g - 1), za & (g - 1)
        n = torch.zeros((act.numel(), 3), dtype=i64, device=DEV)
        for corner in range(8):
            dx, dy, dz = corner & 1, (corner >> 1) & 1, corner >> 2
            w = (fx if dx else g - fx) * (fy if dy else g - fy) * (fz if dz else g - fz)
            n += w[:, None] * D64[(za >> lg) + dz, (ya >> lg) + dy, (xa >> lg) + dx]
        ws = (g - (xa - ia * g).abs()) * (g - (ya - ja * g).abs()) * (g - (za - ka * g).abs()) * step
        scores = torch.zeros((7, nodes), dtype=i64, device=DEV)
        for cand in range(7):
            nn = n.clone()
            if cand:
                nn[:, (cand - 1) // 2] += ws if cand & 1 else -ws
            q = [(p[r] + nn[:, r].to(f32) * 2.0 ** -(8 + 3 * lg)) + 0.5 for r in range(3)]
            b = gather(template, q)
            vote = torch.where(a == b, (a > 0).to(i64), torch.full_like(a, -1))
            scores[cand].index_add_(0, node, vote)
        has = torch.zeros(nodes, dtype=i64, device=DEV).index_add_(0, node, torch.ones_like(node)) > 0
        adm = torch.ones((7, nz, ny, nx), dtype=torch.bool, device=DEV)
        for cand in range(1, 7):
            axis = (cand - 1) // 2
            moved = D64.clone()
            moved[..., axis] += step if cand & 1 else -step
            ok = moved[..., axis].abs() <= W.MAX_DISP
            for arr_axis in range(3):
                for s in (-1, 1):
                    exists = (idx[arr_axis] + s >= 0) & (idx[arr_axis] + s < D.shape[arr_axis])
                    ok &= ((moved - torch.roll(D64, -s, dims=arr_axis)).abs() <= limit).all(-1) | ~exists
            adm[cand] = ok
        masked = torch.where(adm.view(7, -1), scores, torch.full_like(scores, -(1 << 62)))
        top, best = masked[0].clone(), torch.zeros(nodes, dtype=i64, device=DEV)
        for cand in range(1, 7):                                    # strictly larger: the lowest index stays among equal scores
            better = masked[cand] > top
            best, top = torch.where(better, torch.full_like(best, cand), best), torch.where(better, masked[cand], top)
        best = torch.where(has, best, torch.zeros_like(best))
        flat = D.view(-1, 3)
        for cand in range(1, 7):
            flat[:, (cand - 1) // 2] += torch.where(best == cand, step if cand & 1 else -step, 0).to(torch.int32)
        changed += (best > 0).sum()
        visited += has.sum()
    return torch.stack([changed, visited])


template = template_map()
true_map = [0.62, 0.03, 0, -0.025, 0.72, 0.02, 0, 0.015, 0.55, -2.0, 1.5, -1.0]      # subject voxel -> template position
true_map = [v * 256.0 / args.size if e < 9 else v for e, v in enumerate(true_map)]
z, y, x = (v.reshape(-1) for v in torch.meshgrid(torch.arange(SD, device=DEV), torch.arange(SH, device=DEV), torch.arange(SW, device=DEV),
                                                 indexing="ij"))
p = affine(true_map, x, y, z)
smooth = [3 * torch.sin(y / 40.0), 3 * torch.cos(z / 35.0), 2.5 * torch.sin(x / 45.0 + 1)]
subject0 = gather(template, [(p[r] + smooth[r].to(f32)) + 0.5 for r in range(3)]).to(torch.uint8).view(SD, SH, SW)
del p, smooth, x, y, z
nbuf = int(CACHE // S) + 2
subjects = [subject0.clone() for _ in range(nbuf)]
k = [0]


def nxt():
    k[0] = (k[0] + 1) % nbuf
    return subjects[k[0]]


for g in (32, 16, 8, 4):
    limit = W.default_limit(true_map, g)
    shape = W.lattice((SD, SH, SW), g) + (3,)
    D0 = torch.zeros(shape, dtype=torch.int32, device=DEV)
    scratch = torch.empty(W.scratch_bytes((SD, SH, SW), T, [(g, 1, 1, 1, 0)]), dtype=torch.uint8, device=DEV)
    D = {name: D0.clone() for name in ("node", "voxel", "torch")}

    def run(name, subject):
        D[name].copy_(D0)
        if name == "torch":
            return torch_sweep(subject, template, true_map, D[name], g, STEP, limit)
        return W.sweep(subject, template, T, true_map, D[name], g, STEP, limit, impl=W.IMPL_NODE if name == "node" else W.IMPL_VOXEL,
                       scratch=scratch)

    info = {name: run(name, subject0).cpu().tolist() for name in D}
    same = {name: bool(torch.equal(D[name], D["node"])) and info[name] == info["node"] for name in D}
    assert same["voxel"], "IMPL_NODE and IMPL_VOXEL differ"
    assert info["node"][0] > 0, "the sweep moved nothing: the timing would be that of an idle field"
    cands = {name: (lambda name=name: run(name, nxt())) for name in D}
    torch.cuda.synchronize()
    times = {name: [] for name in cands}
    for _ in range(args.rounds):
        for name, fn in cands.items():
            times[name].append(time_it(fn, 1 if name == "torch" else args.reps))
    med = {name: statistics.median(v) for name, v in times.items()}
    for name in cands:
        emit(dict(tag=args.tag, name="sweep g=%d %s" % (g, name), call="sweep", candidate=name, g=g, step=STEP, limit=limit, n_tissues=T,
                  subject=[SW, SH, SD], template=[TW, TH, TD], lattice=list(shape[:3]), us=round(med[name], 1), us_min=round(min(times[name]), 1),
                  us_max=round(max(times[name]), 1), nodes_changed=info[name][0], nodes_visited=info[name][1],
                  voxel_candidates_per_us=round(7 * S / med[name], 1), speedup_over_voxel=round(med["voxel"] / med[name], 3),
                  speedup_over_torch=round(med["torch"] / med[name], 2), bitwise_equal_to_node=same[name],
                  reps=1 if name == "torch" else args.reps, rounds=args.rounds, buffers_rotated=nbuf, device=device))

# a whole fit with the defaults
levels = W.levels_of(W.DEFAULT_LEVELS, None, true_map)
scratch = torch.empty(W.scratch_bytes((SD, SH, SW), T, levels), dtype=torch.uint8, device=DEV)
fields = {}
for name, impl in (("node", W.IMPL_NODE), ("voxel", W.IMPL_VOXEL)):
    out = {}

    def fit():
        out["r"] = W.fit(nxt(), template, T, true_map, levels=levels, impl=impl, scratch=scratch)

    fit()
    torch.cuda.synchronize()
    t = [time_it(fit, 1) for _ in range(args.rounds)]
    fields[name] = out["r"][0].clone()
    rows = out["r"][1].cpu().numpy()
    rows = rows[rows[:, 0] >= 0]
    emit(dict(tag=args.tag, name="fit defaults %s" % name, call="fit", candidate=name, n_tissues=T, subject=[SW, SH, SD], template=[TW, TH, TD],
              levels=levels.tolist(), us=round(statistics.median(t), 1), us_min=round(min(t), 1), us_max=round(max(t), 1),
              report=rows.tolist(), max_disp_q8=int(fields[name].abs().max().item()), subject_nonzero=int((subject0 > 0).sum().item()),
              bitwise_equal_to_node=bool(torch.equal(fields[name], fields["node"])), reps=1, rounds=args.rounds, device=device))
