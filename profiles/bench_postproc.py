#!/usr/bin/env python3
"""The post-processing chain (include/unet_postproc.h): the fused softmax / create_mask / argmax pass at 192x224x192 with 6 and 130
classes (label only, all three outputs, and label only on the scalar path) against the HBM floor of its algorithmic bytes;
defragment on a near-percolation random mask (density 0.31) and on one large blob; and profiles/bench_evaluate.py's 16 x 128^3 inference loop end to end with the model
chain and `label` only, against logits.  One JSON line."""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import unet_studio_amd as U  # noqa: E402
from unet_studio_amd import postproc as P  # noqa: E402

DEV = "cuda:0"
HBM = 8.0e12   # MI355X peak HBM bytes/s


def time_it(fn, reps=20):
    fn()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(reps):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / reps * 1e3   # us


out = {"device": torch.cuda.get_device_name(0)}
W, H, D = 192, 224, 192
S = W * H * D
fusedres = {}
for C in (6, 130):
    # C = 6: the 199 MB of logits would fit the 256 MB Infinity Cache, so the calls rotate over 4 volumes (796 MB) that do not
    nbuf = 4 if C == 6 else 1
    lgs = [torch.randn(C * S + 1, device=DEV) * 3 for _ in range(nbuf)]
    lab = torch.empty(S, dtype=torch.uint16, device=DEV)
    fg = torch.empty(S, device=DEV)
    lp = torch.empty((C - 1) * S, device=DEV)
    k = [0]

    def call(outs, off=0):
        k[0] = (k[0] + 1) % nbuf
        P.softmax_call(lgs[k[0]][off:], C, S, 0.5, *outs)

    t_lab = time_it(lambda: call((None, None, lab)))
    t_all = time_it(lambda: call((lp, fg, lab)))
    t_lab_scalar = time_it(lambda: call((None, None, lab), 1))    # logits one float off 16 B: the scalar kernel
    b_lab = 4 * C * S + 2 * S
    b_all = 4 * C * S + 4 * (C - 1) * S + 4 * S + 2 * S
    fusedres["C%d" % C] = {"label_us": t_lab, "label_hbm_fraction": b_lab / (t_lab * 1e-6) / HBM,
                           "all_us": t_all, "all_hbm_fraction_algorithmic": b_all / (t_all * 1e-6) / HBM,
                           "label_scalar_path_us": t_lab_scalar, "label_scalar_path_hbm_fraction": b_lab / (t_lab_scalar * 1e-6) / HBM,
                           "buffers_rotated": nbuf}
    del lgs, lp
out["fused_192x224x192"] = fusedres

rs = np.random.RandomState(0)
scratch = torch.empty(P.postproc_scratch_bytes(2, S), dtype=torch.uint8, device=DEV)
perc = torch.from_numpy((rs.rand(D, H, W) < 0.31).astype(np.float32)).to(DEV)
z, y, x = np.meshgrid(np.arange(D), np.arange(H), np.arange(W), indexing="ij")
blob = ((z - D / 2) ** 2 + (y - H / 2) ** 2 + (x - W / 2) ** 2 < (0.45 * min(D, H, W)) ** 2).astype(np.float32)
blob[: D // 8, : H // 8, : W // 8] = 1.0      # a second, smaller component
blob = torch.from_numpy(blob).to(DEV)
defrag = {}
for name, m in (("percolation_0.31", perc), ("blob", blob)):
    work = m.clone()

    def run():
        work.copy_(m)
        P.defragment_call((W, H, D), False, 0.5, 0.05, work, None, 0, None, scratch)

    copy_us = time_it(lambda: work.copy_(m))
    defrag[name] = {"us": time_it(run, 10) - copy_us, "mask_voxels": int(m.sum().item())}
    run()
    a = work.clone()
    run()
    defrag[name]["bitwise_reproducible"] = bool(torch.equal(a, work))
out["defragment_192x224x192"] = defrag
del perc, blob, scratch

n, nvol = 128, 16
ios = [[rs.rand(n, n, n).astype(np.float32)] for _ in range(nvol)]
ev_res = {}
for dt in ("bf16", "fp32"):
    m = U.UNet3d(1, 6, U.default_feature(6), device=DEV, dtype=dt, seed=0)
    row = {}
    for name, kw in (("logits", {}), ("label", {"postproc": "model", "outputs": ("label",)})):
        ev = U.EvaluateUNet(m, **kw)
        ev.start(ios[:2])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = ev.start(ios)
        dtm = (time.perf_counter() - t0) / nvol
        assert not ev.aborted, ev.error_msg
        row[name + "_ms_per_volume"] = dtm * 1e3
    ev_res[dt] = row
out["evaluate_16x128^3_out6"] = ev_res
print(json.dumps(out))
