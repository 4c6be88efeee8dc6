#!/usr/bin/env python3
"""The geometry of a fitted lattice warp on the device (include/unet_deform.h): subject 256^3, template 157x189x136, the fields
cowarp.fit finds on bench_cowarp.py's image pair, cut after its first, second and third level (g = 16, 8, 4) --
  pull      a float32 subject volume onto the template grid, 8 rounds, three candidates alternating in one process:
              global    UNET_DEFORM_IMPL_GLOBAL: every lattice node of every round gathered from global memory
              tile      UNET_DEFORM_IMPL_TILE: the brick's lattice window staged in LDS
              torch     a chain of torch ops that computes the same positions (the header's arithmetic, one op per rounding) and
                        samples with the same trilinear rule: the baseline the default must beat; its bits are compared and reported
  jacobian  with and without the det output, beside its write traffic (4 B per voxel)
global and tile are compared for equal bits before anything is timed.  HIP events around `reps` calls (default 5) after a warm-up,
repeated in `rounds` alternating rounds (default 5; the median and the spread over rounds are reported); the subject volumes and the
outputs rotate over more than 256 MB so they cannot sit in the Infinity Cache (the field, 3.3 MB at g = 4, is meant to stay resident).
One JSON line per row, printed and APPENDED to --out (default profiles/deform_bench.jsonl) with the run's tag."""
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
from unet_studio_amd import deform as DF  # noqa: E402
from unet_studio_amd import warp as W  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "deform_bench.jsonl"))
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--size", type=int, default=256, help="the subject's edge (256; smaller for a quick look)")
ap.add_argument("--tag", default="run")
args = ap.parse_args()

DEV = "cuda:0"
CACHE = 256e6  # Infinity Cache
SW = SH = SD = args.size
TW, TH, TD = 157, 189, 136
S, N = SW * SH * SD, TW * TH * TD
ITERS = 8
device = torch.cuda.get_device_name(0)
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


# ---- bench_cowarp.py's image pair ------------------------------------------------------------------------------------------------------
def template_map():
    z, y, x = torch.meshgrid(torch.arange(TD, device=DEV), torch.arange(TH, device=DEV), torch.arange(TW, device=DEV), indexing="ij")
    d = ((x - TW / 2) / (0.42 * TW)) ** 2 + ((y - TH / 2) / (0.42 * TH)) ** 2 + ((z - TD / 2) / (0.42 * TD)) ** 2
    t = torch.zeros((TD, TH, TW), dtype=torch.int32, device=DEV)
    t[d < 1] = 2
    t[d < 0.6] = 1
    t[d < 0.15] = 4
    t[(d < 1) & (z < TD / 2 - 0.55 * 0.42 * TD)] = 3
    return t.to(torch.uint8)


def affine(m, x, y, z):
    return [((float(m[3 * r]) * x + float(m[3 * r + 1]) * y) + float(m[3 * r + 2]) * z) + float(m[9 + r]) for r in range(3)]


def contrast(tissue, levels, seed):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    return torch.tensor(levels, dtype=f32, device=DEV)[tissue.to(i64)] + 0.04 * torch.randn(tissue.shape, generator=gen, device=DEV)


template = template_map()
true_map = [0.62, 0.03, 0, -0.025, 0.72, 0.02, 0, 0.015, 0.55, -2.0, 1.5, -1.0]      # subject voxel -> template position
true_map = [v * 256.0 / args.size if e < 9 else v for e, v in enumerate(true_map)]
z, y, x = (v.reshape(-1).to(f32) for v in torch.meshgrid(torch.arange(SD, device=DEV), torch.arange(SH, device=DEV),
                                                         torch.arange(SW, device=DEV), indexing="ij"))
p = affine(true_map, x, y, z)
smooth = [3 * torch.sin(y / 40.0), 3 * torch.cos(z / 35.0), 2.5 * torch.sin(x / 45.0 + 1)]
q = [(p[r] + smooth[r]) + 0.5 for r in range(3)]
inside = (q[0] >= 0) & (q[0] < TW) & (q[1] >= 0) & (q[1] < TH) & (q[2] >= 0) & (q[2] < TD)
idx = [torch.where(inside, torch.floor(v), torch.zeros_like(v)).to(i64) for v in q]
subject0 = torch.where(inside, template.view(-1)[(idx[2] * TH + idx[1]) * TW + idx[0]], torch.zeros((), dtype=torch.uint8, device=DEV))
subject0 = subject0.view(SD, SH, SW)
del p, smooth, q, inside, idx, x, y, z
fixed_image = contrast(subject0, [0.05, 0.55, 0.85, 0.30, 0.70], 5)
moving_image = contrast(template, [0.05, 0.80, 0.35, 0.60, 0.15], 6)
fixed, moving = CR.code(fixed_image, 0.0, 1.0, 16), CR.code(moving_image, 0.0, 1.0, 16)
levels = W.levels_of(W.DEFAULT_LEVELS, None, true_map)
inv = DF.inverse_map(true_map)

nvol, nout = int(CACHE // (4 * S)) + 2, int(CACHE // (4 * N)) + 2
volumes = [fixed_image.clone() for _ in range(nvol)]
outs = [torch.empty(N, dtype=f32, device=DEV) for _ in range(nout)]
dets = [torch.empty(S, dtype=f32, device=DEV) for _ in range(nvol)]
k = [0]


def nxt():
    k[0] += 1
    return k[0]


def torch_pull(volume, D, g, out):
    """the header's arithmetic in torch ops, one op per rounding"""
    nz, ny, nx = D.shape[:3]
    uz, uy, ux = (v.reshape(-1).to(f32) for v in torch.meshgrid(torch.arange(TD, device=DEV), torch.arange(TH, device=DEV),
                                                               torch.arange(TW, device=DEV), indexing="ij"))
    s0 = affine(inv, ux, uy, uz)
    s = list(s0)
    Df = D.reshape(-1, 3)

    def cell(v, n):
        t = v * (1.0 / g)
        t = torch.where(t > 0, t, torch.zeros_like(t))
        t = torch.where(t < float(n - 1), t, torch.full_like(t, float(n - 1)))
        c = torch.clamp(torch.floor(t).to(i64), max=n - 2)
        return c, t - c.to(f32)

    def lerp(t, a, b):
        return a + t * (b - a)

    for _ in range(ITERS):
        (cx, fx), (cy, fy), (cz, fz) = cell(s[0], nx), cell(s[1], ny), cell(s[2], nz)
        base = (cz * ny + cy) * nx + cx
        v = [Df[base + (dz * ny + dy) * nx + dx].to(f32) for dz in (0, 1) for dy in (0, 1) for dx in (0, 1)]   # {N, 3} each
        fx3, fy3, fz3 = fx[:, None], fy[:, None], fz[:, None]
        e = lerp(fz3, lerp(fy3, lerp(fx3, v[0], v[1]), lerp(fx3, v[2], v[3])), lerp(fy3, lerp(fx3, v[4], v[5]), lerp(fx3, v[6], v[7])))
        e = e * (1.0 / 256)
        s = [s0[r] - ((float(inv[3 * r]) * e[:, 0] + float(inv[3 * r + 1]) * e[:, 1]) + float(inv[3 * r + 2]) * e[:, 2]) for r in range(3)]
    ok = (s[0] >= 0) & (s[1] >= 0) & (s[2] >= 0) & (s[0] <= SW - 1) & (s[1] <= SH - 1) & (s[2] <= SD - 1)
    s = [torch.where(ok, v, torch.zeros_like(v)) for v in s]
    fl = [torch.floor(v) for v in s]
    t = [a - b for a, b in zip(s, fl)]
    i0 = [v.to(i64) for v in fl]
    i1 = [torch.clamp(a + 1, max=d - 1) for a, d in zip(i0, (SW, SH, SD))]
    vol = volume.view(-1)
    at = lambda xx, yy, zz: vol[(zz * SH + yy) * SW + xx]  # noqa: E731
    c00, c10 = lerp(t[0], at(i0[0], i0[1], i0[2]), at(i1[0], i0[1], i0[2])), lerp(t[0], at(i0[0], i1[1], i0[2]), at(i1[0], i1[1], i0[2]))
    c01, c11 = lerp(t[0], at(i0[0], i0[1], i1[2]), at(i1[0], i0[1], i1[2])), lerp(t[0], at(i0[0], i1[1], i1[2]), at(i1[0], i1[1], i1[2]))
    out.copy_(torch.where(ok, lerp(t[2], lerp(t[1], c00, c10), lerp(t[1], c01, c11)), torch.zeros_like(c00)))
    return out, torch.stack(s)


for n_levels, g in ((1, 16), (2, 8), (3, 4)):
    D, _ = CW.fit(fixed, moving, 16, true_map, levels=levels[:n_levels])
    assert tuple(D.shape) == W.lattice((SD, SH, SW), g) + (3,)

    def pull(impl):
        return DF.pull(volumes[nxt() % nvol], (TD, TH, TW), true_map, D, g, inv=inv, iters=ITERS, impl=impl, out=outs[nxt() % nout])

    a, pa, ia = DF.pull(volumes[0], (TD, TH, TW), true_map, D, g, inv=inv, iters=ITERS, pos=True, impl=DF.IMPL_GLOBAL)
    b, pb, ib = DF.pull(volumes[0], (TD, TH, TW), true_map, D, g, inv=inv, iters=ITERS, pos=True, impl=DF.IMPL_TILE)
    assert torch.equal(a, b) and torch.equal(pa, pb) and torch.equal(ia, ib), "IMPL_GLOBAL and IMPL_TILE differ"
    c, pc = torch_pull(volumes[0], D, g, torch.empty(N, dtype=f32, device=DEV))
    ok = (pa.reshape(3, -1)[0] >= 0) & (pa.reshape(3, -1)[1] >= 0) & (pa.reshape(3, -1)[2] >= 0) & (pa.reshape(3, -1)[0] <= SW - 1) & (
        pa.reshape(3, -1)[1] <= SH - 1) & (pa.reshape(3, -1)[2] <= SD - 1)
    torch_equal = bool(torch.equal(a.reshape(-1), c)) and bool(torch.equal(pa.reshape(3, -1)[:, ok], pc[:, ok]))
    info = ia.cpu().tolist()
    del a, b, c, pa, pb, pc, ok
    cands = {"global": lambda: pull(DF.IMPL_GLOBAL), "tile": lambda: pull(DF.IMPL_TILE),
             "torch": lambda: torch_pull(volumes[nxt() % nvol], D, g, outs[nxt() % nout])}
    for fn in cands.values():
        fn()
    torch.cuda.synchronize()
    times = {name: [] for name in cands}
    for _ in range(args.rounds):
        for name, fn in cands.items():
            times[name].append(time_it(fn, args.reps if name != "torch" else 1))
    med = {name: statistics.median(v) for name, v in times.items()}
    for name in cands:
        emit(dict(tag=args.tag, name="pull g=%d %s" % (g, name), call="pull", candidate=name, g=g, iters=ITERS, subject=[SW, SH, SD],
                  template=[TW, TH, TD], lattice=list(D.shape[:3]), us=round(med[name], 1), us_min=round(min(times[name]), 1),
                  us_max=round(max(times[name]), 1), inside=info[0], not_converged=info[1], max_disp_q8=int(D.abs().max().item()),
                  corner_gathers_per_us=round(N * (ITERS + 1) * 8 / med[name], 1), speedup_over_torch=round(med["torch"] / med[name], 2),
                  bitwise_equal_to_global=torch_equal if name == "torch" else True, reps=args.reps if name != "torch" else 1,
                  rounds=args.rounds, buffers_rotated=[nvol, nout], device=device))

    def jac(with_det):
        return DF.jacobian((SD, SH, SW), true_map, D, g, det=dets[nxt() % nvol] if with_det else False)

    cands = {"det": lambda: jac(True), "info only": lambda: jac(False)}
    summary = DF.summary(jac(True)[1])
    torch.cuda.synchronize()
    times = {name: [] for name in cands}
    for _ in range(args.rounds):
        for name, fn in cands.items():
            times[name].append(time_it(fn, args.reps))
    for name in cands:
        m = statistics.median(times[name])
        emit(dict(tag=args.tag, name="jacobian g=%d %s" % (g, name), call="jacobian", candidate=name, g=g, subject=[SW, SH, SD],
                  us=round(m, 1), us_min=round(min(times[name]), 1), us_max=round(max(times[name]), 1),
                  gb_per_s_written=round(4 * S / m / 1e3, 1) if name == "det" else None, folded=summary["folded"],
                  det_min=summary["det_min"], det_max=summary["det_max"], reps=args.reps, rounds=args.rounds, device=device))
