#!/usr/bin/env python3
"""Binary morphology on bit-packed masks on the device (include/unet_morph.h) at 128^3 and 256^3, the candidates alternating in one
process --
  pack              the mask of class 1 of a uint16 map
  step              dilate, connectivity 6 and 26, 1 / 2 / 4 iterations: UNET_MORPH_IMPL_LDS (a brick in LDS, up to 4 iterations a
                    launch) against UNET_MORPH_IMPL_GLOBAL (one thread per word, one launch per iteration)
  close             connectivity 26, 2 iterations, both impls
  fill_holes        impl LDS (the tiled labelling) against GLOBAL (the global labelling)
  close_label, fill_holes_label   end to end on the label map with the default impls; the map is restored from a pristine copy
                    before every call, and that copy is timed in a row of its own (`restore`)
  scipy             for context, the only route without these kernels: the map copied to the host, scipy.ndimage, the result
                    copied back (a host clock around it, one call)
on two uint16 maps --
  solid    a ball of class 1 of half the volume with 20 cavities of radius 2..4 inside it
  sparse   300 balls of radius 2..4 of class 1 in an empty volume: what a lesion map looks like
The two impls of a row are compared for equal bits before anything is timed; the row records the outcome.  HIP events around `reps`
calls (default 20) after a warm-up, repeated in `rounds` alternating rounds (default 5; the median and the spread over rounds are
reported); several maps rotate.  A mask of 256^3 is 2 MiB, so the masks sit in cache on purpose: that is how they are used.  Every
row carries its algorithmic bytes (pack: 2 B read and 1/8 B written per voxel; step and close: 2 x S / 8 per call; fill_holes: the
mask in and out, the uint16 background map written and read, parent and count written and read; the label calls: the map read by
pack and by apply) and the fraction of the 8 TB/s floor they amount to.  One JSON line per row, printed and APPENDED to --out
(default profiles/morph_bench.jsonl) with the run's tag."""
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
from unet_studio_amd import morph as MO  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "morph_bench.jsonl"))
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--sizes", type=int, nargs="+", default=[128, 256])
ap.add_argument("--no-scipy", action="store_true")
ap.add_argument("--tag", default="run")
args = ap.parse_args()

DEV = "cuda:0"
HBM = 8.0e12   # MI355X peak HBM bytes/s
NBUF = 4
IMPLS = {"lds": MO.IMPL_LDS, "global": MO.IMPL_GLOBAL}
device = torch.cuda.get_device_name(0)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)


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


def measure(cands):
    """{name: fn} -> {name: [us per round]}: a warm-up, then alternating rounds"""
    for fn in cands.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in cands}
    for _ in range(args.rounds):
        for name, fn in cands.items():
            times[name].append(time_it(fn, args.reps))
    return times


for size in args.sizes:
    W = H = D = size
    S = W * H * D
    shape = (D, H, W)
    z, y, x = torch.meshgrid(torch.arange(D, device=DEV), torch.arange(H, device=DEV), torch.arange(W, device=DEV), indexing="ij")

    def balls(lab, n, seed, value, lo, hi):
        g = torch.Generator().manual_seed(seed)
        c = torch.randint(lo, hi, (n, 3), generator=g)
        r = torch.randint(2, 5, (n,), generator=g)
        for (cz, cy, cx), rr in zip(c.tolist(), r.tolist()):
            sub = (slice(cz - rr, cz + rr + 1), slice(cy - rr, cy + rr + 1), slice(cx - rr, cx + rr + 1))
            lab[sub] = torch.where(((z[sub] - cz) ** 2 + (y[sub] - cy) ** 2 + (x[sub] - cx) ** 2) <= rr * rr, value, lab[sub])
        return lab

    def solid_map(seed):
        """a ball of half the volume, its centre shifted by the seed, with 20 cavities well inside it"""
        r = (3.0 / (8.0 * np.pi)) ** (1.0 / 3.0) * size
        c = size / 2 - 0.5 + 0.25 * seed
        lab = (((z - c) ** 2 + (y - c) ** 2 + (x - c) ** 2) <= r * r).to(torch.int32)
        return balls(lab, 20, seed, 0, size // 3, 2 * size // 3).to(torch.uint16)

    def sparse_map(seed):
        return balls(torch.zeros(shape, dtype=torch.int32, device=DEV), 300, seed, 1, 5, size - 5).to(torch.uint16)

    for kind, make in (("solid", solid_map), ("sparse", sparse_map)):
        maps = [make(i) for i in range(NBUF)]
        scratch = torch.empty(MO.morph_scratch_bytes(shape), dtype=torch.uint8, device=DEV)
        masks = [MO.pack(m, 2, [1], scratch=scratch) for m in maps]
        out, tmp = masks[0].new(), masks[0].new()
        work = torch.empty_like(maps[0])
        k = [0]

        def nxt():
            k[0] = (k[0] + 1) % NBUF
            return k[0]

        def row(call, cand, t, nbytes, **extra):
            med = statistics.median(t)
            emit(dict(tag=args.tag, name="%s %s %d^3 %s" % (call, kind, size, cand), call=call, map=kind, candidate=cand, dims=[W, H, D],
                      us=round(med, 1), us_min=round(min(t), 1), us_max=round(max(t), 1), algorithmic_bytes=nbytes,
                      floor_us=round(nbytes / HBM * 1e6, 3), hbm_fraction=round(nbytes / (med * 1e-6) / HBM, 5), reps=args.reps,
                      rounds=args.rounds, buffers_rotated=NBUF, device=device, **extra))

        # ---- pack ----
        t = measure({"pack": lambda: MO.pack(maps[nxt()], 2, [1], scratch=scratch, out=out)})
        row("pack", "wave_ballot", t["pack"], 2 * S + S // 8, voxels_set=int(MO.count(masks[0])))

        # ---- step: dilate, and close ----
        def step_cands(f):
            return {name: (lambda impl=impl: f(masks[nxt()], impl)) for name, impl in IMPLS.items()}

        for c in (6, 26):
            for n in (1, 2, 4):
                res = {name: MO.dilate(masks[0], c, n, impl=impl, scratch=scratch).bits for name, impl in IMPLS.items()}
                same = torch.equal(res["lds"], res["global"])
                assert same, "IMPL_LDS and IMPL_GLOBAL differ"
                t = measure(step_cands(lambda m, impl: MO.dilate(m, c, n, impl=impl, scratch=scratch, out=out)))
                ratio = round(statistics.median(t["global"]) / statistics.median(t["lds"]), 3)
                for name in IMPLS:
                    row("dilate c%d n%d" % (c, n), name, t[name], 2 * (S // 8), global_over_lds=ratio, bitwise_equal=same)

        def close2(m, impl):
            MO.dilate(m, 26, 2, impl=impl, scratch=scratch, out=tmp)
            return MO.erode(tmp, 26, 2, impl=impl, scratch=scratch, out=out, border=1)

        res = {name: close2(masks[0], impl).bits.clone() for name, impl in IMPLS.items()}
        same = torch.equal(res["lds"], res["global"])
        assert same, "IMPL_LDS and IMPL_GLOBAL differ"
        t = measure(step_cands(close2))
        ratio = round(statistics.median(t["global"]) / statistics.median(t["lds"]), 3)
        for name in IMPLS:
            row("close c26 n2", name, t[name], 4 * (S // 8), global_over_lds=ratio, bitwise_equal=same)

        # ---- fill_holes ----
        res = {}
        for name, impl in IMPLS.items():
            got, info = MO.fill_holes(masks[0], impl=impl, scratch=scratch)
            res[name] = (got.bits, info)
        same = all(torch.equal(a, b) for a, b in zip(res["lds"], res["global"]))
        assert same, "the two labellings differ"
        filled, holes = (int(v) for v in res["lds"][1].cpu())
        t = measure(step_cands(lambda m, impl: MO.fill_holes(m, impl=impl, scratch=scratch, out=out)))
        ratio = round(statistics.median(t["global"]) / statistics.median(t["lds"]), 3)
        for name in IMPLS:
            row("fill_holes", name, t[name], 2 * (S // 8) + 4 * S + 16 * S, global_over_tiled=ratio, bitwise_equal=same,
                voxels_filled=filled, holes=holes)

        # ---- on the label map, end to end (the default impls); the map is restored before every call ----
        def restore():
            work.view(torch.int16).copy_(maps[nxt()].view(torch.int16))

        def close_label():
            restore()
            MO.close_label(work, 1, 26, 2, scratch=scratch)

        def fill_label():
            restore()
            MO.fill_holes_label(work, [1], 1, 2, scratch=scratch)

        t = measure({"restore": restore, "close_label": close_label, "fill_holes_label": fill_label})
        row("restore", "copy", t["restore"], 4 * S)
        row("close_label c26 n2", "default", t["close_label"], 4 * S + 2 * S + 6 * (S // 8), includes="restore")
        row("fill_holes_label", "default", t["fill_holes_label"], 4 * S + 2 * S + 4 * (S // 8) + 20 * S, includes="restore")

        # ---- for context: the host route, one call each under a host clock ----
        if not args.no_scipy:
            from scipy import ndimage
            s26 = ndimage.generate_binary_structure(3, 3)
            for call, f in (("close_label c26 n2", lambda m: ndimage.binary_erosion(ndimage.binary_dilation(m, s26, iterations=2), s26,
                                                                                    iterations=2, border_value=1)),
                            ("fill_holes_label", ndimage.binary_fill_holes)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                host = maps[0].view(torch.int16).cpu().numpy()
                got = np.where(f(host == 1) & (host == 0), 1, host).astype(np.int16)
                back = torch.from_numpy(got).to(DEV)
                torch.cuda.synchronize()
                us = (time.perf_counter() - t0) * 1e6
                work.view(torch.int16).copy_(maps[0].view(torch.int16))
                (MO.close_label(work, 1, 26, 2, scratch=scratch) if call.startswith("close") else MO.fill_holes_label(work, [1], 1, 2, scratch=scratch))
                same = torch.equal(back, work.view(torch.int16))
                assert same, "the device and scipy.ndimage differ"
                emit(dict(tag=args.tag, name="%s %s %d^3 scipy" % (call, kind, size), call=call, map=kind, candidate="scipy_with_copies",
                          dims=[W, H, D], us=round(us, 0), clock="host, one call", bitwise_equal_to_device=same, device=device))
                del back
        del maps, masks, out, tmp, work, scratch
