"""GPU (-m gpu): a conv and the norm layer next to it, per layer, against a float64 reference of the same layer.

unet_op_conv3d_fwd_norm and unet_op_conv3d_bwd_data_norm (and its sibling with a stride, _strided; include/unet_hip.h) launch the conv through the functions the executor
launches it through (conv_fwd, conv_dgrad in csrc/engine.cpp) and the norm's own launches through norm_fwd_passes / norm_bwd_passes: on the
deep levels one split-K launch of kernels_mfma_deep.hip with the norm in the epilogue of the block that draws the last ticket
(DEEP_FWD_NORM: conv, statistics, running statistics, activated copy; DEEP_BWD_NORM: dgrad, the norm's backward sums, coef,
dgamma / dbeta, dL/d(raw)), elsewhere the MFMA conv and the norm's separate launches (k_norm_finalize_apply8, k_norm_bwd_*).  The
last test reruns every case with UNET_NO_DEEP_KERNELS=1, so both paths meet the same bounds.

Inputs.  The conv operands lie on a coarse grid (activations k / 8, filters k / 16, |k| <= 8; the older gradient k / 128): every
product is a multiple of 2^-7 and every partial sum stays below 2^17, so the fp32 contraction is EXACT in any order and the only
rounding before the norm is the one to bf16.  That makes a lost or doubled K range visible at full size, and lets the backward
reference model the kernel's one rounding before dv, dL/d(view) = bf16(dgrad + old), without ambiguity.  The raw norm tensor u and
the affine parameters are ordinary random values.

Bounds, derived from the rounding points (eps32 = 2^-24, the fp32 unit roundoff):
  * bf16-stored tensors (raw conv output y, dL/d(raw)): half a bf16 ulp, <= 2^-8 |ref|, plus 1e-3 max|ref| for the fp32 work in front
    of the rounding (bias add; the fp32 evaluation of dL/d(raw) = A dv + B u + D, whose cancellation is bounded separately by
    2^-20 |c0| (|dv| + |m1| + |m2| rstd (|u| + |mean|)): three fp32 roundings of each of those terms, with margin);
  * the activated copy, from the kernel's own stored y and stat row: act(fma(y, scale, shift)) rounds the fma to fp32 (2^-23 (|y scale|
    + |shift|), |act'| <= 1), then to bf16: one bf16 ulp of the reference;
  * statistics: the kernel sums y and y^2 in fp32 per thread / per tile and combines in fp64; 1e-5 of A = sum|y| / V bounds the mean,
    dvar = 1e-5 (B + 2 |mean| A) (B = sum y^2 / V) the variance E[y^2] - mean^2, 0.5 dvar / (var + eps) + 1e-6 the relative error of
    rstd and scale; shift = beta - mean scale adds the two; running statistics scale these by the momentum (plus 1e-6 of the value for
    the fp32 results); eval mode takes rm / rv as they are: 1e-6 relative;
  * coef = {gamma rstd (1e-6 relative), mean(dv), mean(dv xhat)}, dgamma, dbeta: 1e-4 of the sum of |terms| of each sum (fp32 dv and
    xhat, fp32 partial sums), plus 2^-23 |1 + sum| for the += onto the starting value 1.0.

Teeth: for each case three wrong references are built in numpy -- one 32-channel chunk of the centre tap left out of the
contraction (a lost K range), the statistics of channel c taken from channel c + 16 (the wrong 16-channel row tile), and for volumes
over 64 voxels the statistics without one 64-voxel group -- and each must miss the bounds by at least 10x, so the bounds cannot
drift loose enough to pass those bugs.

Determinism: every output is filled with NaN before each call, and each case runs twice (the second call reuses the arrival
counters the first left behind); the two results must be bit-identical.

Not covered: BatchNorm at one voxel (eps is 0 there and the variance 0: rstd is infinite; the reference refuses it in training)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import unet_studio_amd as U  # noqa: E402

E = U.engine
DEV = "cuda:0"
EPS = {"in": 1e-5, "bn": 0.0}         # graph.cpp: InstanceNorm 1e-5, BatchNorm 0
MOMENTUM = 0.1


def stream():
    return torch.cuda.current_stream(DEV).cuda_stream


def bf(x):
    """round to bf16 (nearest even) and back to float64"""
    return torch.from_numpy(np.asarray(x, np.float32)).to(torch.bfloat16).double().numpy()


def grid(shape, seed, step, lim=8):
    return np.random.default_rng(seed).integers(-lim, lim + 1, shape).astype(np.float64) * step


def rnd(shape, seed, scale=1.0, offset=0.0):
    return np.random.default_rng(seed).standard_normal(shape) * scale + offset


def act64(z, a):
    if a == 1:
        return np.maximum(z, 0.0)
    if a == 2:
        return np.where(z > 0, z, 0.01 * z)
    if a == 3:
        return np.where(z > 0, z, np.expm1(np.minimum(z, 0.0)))
    return z


def act_t(z, a):
    if a == 1:
        return torch.relu(z)
    if a == 2:
        return torch.nn.functional.leaky_relu(z, 0.01)
    if a == 3:
        return torch.nn.functional.elu(z)
    return z


def bf16_ulp(x):
    _, e = np.frexp(np.abs(x))
    return np.ldexp(1.0, e - 8)


def dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(DEV)


def nan_like(t):
    return t.fill_(float("nan"))


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32).numpy().copy()


def scratch(cin, cout, D, H, W):
    b = ctypes.c_size_t()
    E.check(E.lib.unet_op_scratch_bytes(cin, cout, D, H, W, ctypes.byref(b)))
    return torch.empty(b.value, dtype=torch.uint8, device=DEV)


def miss(wrong, ref, bound):
    """by how many times a wrong reference misses the bound at its worst element"""
    return float(np.max(np.abs(np.asarray(wrong, np.float64) - ref) / bound))


def teeth(bug, r):
    assert r >= 10, "%s misses the bounds by only %.1fx" % (bug, r)


def check(name, got, ref, bound):
    err = np.abs(np.asarray(got, np.float64) - ref)
    assert np.all(np.isfinite(got)), name + ": not finite"
    worst = float(np.max(err / bound))
    assert worst <= 1.0, "%s: error %.3g of the bound (max abs err %.3g)" % (name, worst, float(err.max()))
    return worst


# ---------------------------------------------------------------------------------------------------------------------------------
# forward: conv k3 (+ bias) -> norm -> activation
# (cin0, cin1, cout, (D, H, W), stride, act, norm, eval)
FWD_CASES = [
    # <1,3,1> DEEP_FWD_NORM: <= 64 output voxels
    (32, 0, 16, (3, 4, 5), 1, 2, "in", False),
    (64, 0, 48, (4, 4, 4), 1, 1, "bn", False),        # exactly 64 voxels, 3 row tiles
    (512, 0, 256, (2, 3, 3), 1, 3, "in", False),      # K split 16
    (512, 0, 16, (1, 2, 3), 1, 3, "bn", False),       # K split 32
    (32, 32, 48, (3, 4, 5), 1, 0, "bn", True),        # two sources, eval
    (64, 128, 16, (2, 3, 3), 1, 2, "in", False),      # two sources
    (32, 0, 16, (1, 1, 1), 1, 2, "in", False),        # one voxel: xhat = 0, output act(beta)
    (128, 0, 256, (4, 4, 4), 1, 1, "bn", True),
    # <2,3,1> DEEP_FWD_NORM: stride 2 from odd extents, Wo <= 8
    (32, 0, 48, (7, 5, 3), 2, 2, "in", False),
    (256, 0, 64, (8, 8, 8), 2, 1, "bn", False),
    (64, 64, 32, (5, 7, 7), 2, 3, "bn", True),
    # > 64 output voxels: MFMA conv with statistics rows, then k_norm_finalize(_apply8) / k_norm_eval + the activated copy
    (32, 0, 32, (8, 8, 8), 1, 2, "in", False),
    (64, 0, 64, (16, 16, 16), 1, 1, "bn", False),
    (32, 32, 32, (8, 8, 8), 1, 0, "bn", True),
    (32, 0, 64, (16, 16, 16), 2, 3, "in", False),
]


def fwd_inputs(case):
    cin0, cin1, cout, (D, H, W), st, a, norm, ev = case
    cin = cin0 + cin1
    seed = cin * 7 + cout * 13 + D * 17 + H * 19 + W * 23 + st
    x0 = grid((D, H, W, cin0), seed + 1, 1 / 8)
    x1 = grid((D, H, W, cin1), seed + 2, 1 / 8) if cin1 else None
    w = grid((cout, cin, 3, 3, 3), seed + 3, 1 / 16)
    b = rnd((cout,), seed + 4).astype(np.float32).astype(np.float64)
    gamma = rnd((cout,), seed + 5, 0.2, 1.0).astype(np.float32).astype(np.float64)
    sgn = np.where(np.random.default_rng(seed + 6).random(cout) < 0.5, -1.0, 1.0)
    beta = (sgn * (0.1 + 0.4 * np.random.default_rng(seed + 7).random(cout))).astype(np.float32).astype(np.float64)
    rm = rnd((cout,), seed + 8, 0.5).astype(np.float32).astype(np.float64)
    rv = (0.5 + np.random.default_rng(seed + 9).random(cout)).astype(np.float32).astype(np.float64)
    return x0, x1, w, b, gamma, beta, rm, rv


def conv64(x, w, b, st):
    y = torch.nn.functional.conv3d(torch.from_numpy(x).permute(3, 0, 1, 2)[None], torch.from_numpy(w), torch.from_numpy(b),
                                   stride=st, padding=1)
    return y[0].permute(1, 2, 3, 0).numpy()


def run_fwd(case, x0, x1, w, b, gamma, beta, rm, rv):
    cin0, cin1, cout, (D, H, W), st, a, norm, ev = case
    od = [(s - 1) // st + 1 for s in (D, H, W)]
    xd0 = dev(x0, torch.bfloat16)
    xd1 = dev(x1, torch.bfloat16) if cin1 else None
    wd, bd = dev(w, torch.float32), dev(b, torch.float32)
    gd, btd = dev(gamma, torch.float32), dev(beta, torch.float32)
    bn = norm == "bn"
    sc = scratch(cin0 + cin1, cout, D, H, W)
    outs = []
    for _ in range(2):
        rmd = dev(rm, torch.float32) if bn else None
        rvd = dev(rv, torch.float32) if bn else None
        y = nan_like(torch.empty((*od, cout), dtype=torch.bfloat16, device=DEV))
        ya = nan_like(torch.empty((*od, cout), dtype=torch.bfloat16, device=DEV))
        stat = nan_like(torch.empty((4 * cout,), dtype=torch.float32, device=DEV))
        E.check(E.lib.unet_op_conv3d_fwd_norm(xd0.data_ptr(), xd1.data_ptr() if cin1 else None, cin0, cin1, wd.data_ptr(), bd.data_ptr(),
                                              gd.data_ptr(), btd.data_ptr(), EPS[norm], rmd.data_ptr() if bn else None,
                                              rvd.data_ptr() if bn else None, MOMENTUM, 1 if ev else 0, a, y.data_ptr(), ya.data_ptr(),
                                              stat.data_ptr(), cout, D, H, W, st, sc.data_ptr(), stream()))
        torch.cuda.synchronize()
        outs.append({"y": y, "ya": ya, "stat": stat, "rm": rmd, "rv": rvd})
    for k in outs[0]:
        if outs[0][k] is not None:
            assert np.array_equal(bits(outs[0][k]), bits(outs[1][k])), "%s differs between two identical calls" % k
    return {k: (v.float().cpu().numpy().astype(np.float64) if v is not None else None) for k, v in outs[0].items()}


def stat_ref(y, gamma, beta, eps, groups_lost=False):
    """fp64 statistics of the stored values y [V, C] and their bounds (module docstring)"""
    V = y.shape[0]
    if groups_lost:
        y = y[64:]
    mean = y.sum(0) / V
    Ey2 = (y * y).sum(0) / V
    var = np.maximum(Ey2 - mean * mean, 0.0) if groups_lost else ((y - y.mean(0)) ** 2).mean(0)
    return mean, var, Ey2


def fwd_expect(y, gamma, beta, eps, rm, rv, ev):
    """{name: (ref, bound)} of the statistics, running statistics (bnorm training) and the stat row, from the stored raw output"""
    V = y.shape[0]
    A, B = np.abs(y).sum(0) / V, (y * y).sum(0) / V
    if ev:
        mean, var = rm, rv
        rstd = 1.0 / np.sqrt(var + eps)
        r_rel = 1e-6 + 0 * rstd
        dmean = 1e-6 * np.abs(mean)
    else:
        mean, var, _ = stat_ref(y, gamma, beta, eps)
        rstd = 1.0 / np.sqrt(var + eps)
        dvar = 1e-5 * (B + 2 * np.abs(mean) * A)
        r_rel = 0.5 * dvar / (var + eps) + 1e-6
        dmean = 1e-5 * A
    scale = gamma * rstd
    shift = beta - mean * scale
    exp = {"mean": (mean, dmean + 1e-30), "rstd": (rstd, r_rel * rstd), "scale": (scale, r_rel * np.abs(scale) + 1e-30),
           "shift": (shift, dmean * np.abs(scale) + np.abs(mean) * r_rel * np.abs(scale) + 1e-6 * (np.abs(beta) + np.abs(mean * scale)))}
    if not ev and rm is not None:
        ub = V / (V - 1.0)
        exp["rm"] = ((1 - MOMENTUM) * rm + MOMENTUM * mean, MOMENTUM * dmean + 1e-6 * ((1 - MOMENTUM) * np.abs(rm) + MOMENTUM * A))
        exp["rv"] = ((1 - MOMENTUM) * rv + MOMENTUM * var * ub, MOMENTUM * ub * dvar + 1e-6 * ((1 - MOMENTUM) * rv + MOMENTUM * B * ub))
    return exp


def fwd_wrong_stats(y, gamma, beta, eps, rm, rv, ev, cout, lost_group):
    """the stat row (and running statistics) of the two statistics bugs"""
    out = []
    if cout > 16:           # channel c's statistics from channel c + 16: the wrong row tile
        p = (np.arange(cout) + 16) % cout
        if ev:
            mean, var = rm[p], rv[p]
        else:
            mean, var, _ = stat_ref(y[:, p], gamma, beta, eps)
        out.append(("row tile", mean, var))
    if lost_group and not ev:
        mean, var, _ = stat_ref(y, gamma, beta, eps, groups_lost=True)
        out.append(("64-voxel group", mean, var))
    res = []
    for name, mean, var in out:
        rstd = 1.0 / np.sqrt(var + eps)
        scale = gamma * rstd
        d = {"mean": mean, "rstd": rstd, "scale": scale, "shift": beta - mean * scale}
        if not ev and rm is not None:
            V = y.shape[0]
            d["rm"] = (1 - MOMENTUM) * rm + MOMENTUM * mean
            d["rv"] = (1 - MOMENTUM) * rv + MOMENTUM * var * V / (V - 1.0)
        res.append((name, d))
    return res


@pytest.mark.parametrize("case", FWD_CASES, ids=lambda c: "%d+%dx%d_%dx%dx%d_s%d_act%d_%s%s" % (c[0], c[1], c[2], *c[3], c[4], c[5], c[6],
                                                                                             "_eval" if c[7] else ""))
def test_conv_norm_forward_against_fp64(case):
    cin0, cin1, cout, (D, H, W), st, a, norm, ev = case
    if norm == "bn" and not ev:
        assert (D - 1) // st + 1 > 1 or (H - 1) // st + 1 > 1 or (W - 1) // st + 1 > 1, "BatchNorm training at one voxel is not defined"
    x0, x1, w, b, gamma, beta, rm, rv = fwd_inputs(case)
    x = np.concatenate([x0, x1], axis=3) if cin1 else x0
    eps = EPS[norm]
    bn = norm == "bn"
    got = run_fwd(case, x0, x1, w, b, gamma, beta, rm, rv)
    ref = conv64(x, w, b, st)
    V = ref.shape[0] * ref.shape[1] * ref.shape[2]
    ref = ref.reshape(V, cout)
    yk = got["y"].reshape(V, cout)
    # the raw output
    by = 2.0 ** -8 * np.abs(ref) + 1e-3 * np.abs(ref).max()
    check("y", yk, ref, by)
    # the statistics of the values as stored
    exp = fwd_expect(yk, gamma, beta, eps, rm if bn else None, rv if bn else None, ev)
    st4 = got["stat"].reshape(4, cout)
    for i, k in enumerate(("mean", "rstd", "scale", "shift")):
        check(k, st4[i], *exp[k])
    if bn and ev:
        assert np.array_equal(got["rm"], rm) and np.array_equal(got["rv"], rv), "eval mode changed the running statistics"
    elif bn:
        check("running mean", got["rm"], *exp["rm"])
        check("running var", got["rv"], *exp["rv"])
    # the activated copy from the kernel's own stored y and stat row
    t = yk * st4[2] + st4[3]
    ra = act64(t, a)
    ba = bf16_ulp(ra) + 2.0 ** -23 * (np.abs(yk * st4[2]) + np.abs(st4[3])) + 1e-30
    check("activated copy", got["ya"].reshape(V, cout), ra, ba)
    if V == 1 and norm == "in":     # xhat = 0: the output is act(beta)
        check("act(beta) at one voxel", got["ya"].reshape(cout), act64(beta, a), bf16_ulp(act64(beta, a)) + 2.0 ** -20 * np.abs(yk[0] * st4[2]))

    # teeth
    wl = w.copy()
    wl[:, 0:32, 1, 1, 1] = 0.0
    teeth("a lost K range", miss(conv64(x, wl, b, st).reshape(V, cout), ref, by))
    for name, d in fwd_wrong_stats(yk, gamma, beta, eps, rm if bn else None, rv if bn else None, ev, cout, V > 64):
        teeth("statistics without the right " + name, max(miss(d[k], *exp[k]) for k in d))


# ---------------------------------------------------------------------------------------------------------------------------------
# backward: dgrad into the view of a norm layer's tensor u, then that norm's backward
# (kind: 0 conv k3 s1, 1 conv_trans k2 s2, 2 conv k3 s2; cin = channels of u / dx, cout = channels of dy, (D, H, W) of u, act, accumulate, norm)
BWD_CASES = [
    # <1,3,1> DEEP_BWD_NORM: conv k3 s1, <= 64 voxels
    (0, 16, 32, (3, 4, 5), 2, 0, "in"),
    (0, 48, 64, (4, 4, 4), 1, 1, "bn"),
    (0, 256, 512, (2, 3, 3), 3, 0, "in"),
    (0, 32, 512, (1, 2, 3), 0, 1, "bn"),
    (0, 32, 64, (1, 1, 1), 2, 0, "in"),                # one voxel: dL/d(raw) = 0
    (0, 64, 32, (2, 2, 2), 3, 1, "in"),
    # <2,2,0> DEEP_BWD_NORM: conv_trans k2 s2, coarse grids <= 512 voxels, W <= 8
    (1, 64, 32, (7, 8, 8), 2, 0, "in"),                # K split 1
    (1, 96, 64, (5, 7, 8), 1, 1, "bn"),                # ragged last 64-voxel group
    (1, 256, 128, (4, 4, 4), 3, 1, "in"),
    (1, 512, 32, (8, 8, 8), 0, 0, "bn"),               # two row tiles per block
    # larger: the dgrad (with its statistics epilogue where it has one) and k_norm_bwd_partial / k_norm_bwd_finalize(_apply8)
    (0, 32, 32, (8, 8, 8), 2, 0, "in"),
    (0, 64, 64, (16, 16, 16), 1, 1, "bn"),
    (1, 32, 32, (8, 8, 16), 3, 0, "in"),
    # conv k3 s2 (unet_op_conv3d_bwd_data_norm_strided), the dgrad that writes a skip tensor's gradient last.  k_s2_scatter with the
    # statistics rows (coarse grid >= 16 wide, >= 4 deep, 32 or 64 dy channels), written <0,KS,false,true> and accumulated
    # <0,KS,true,true>: KS 2 on the smallest coarse grid it serves, (4, 4, 16) -- 256 voxels, which mfma_dgrad gives to the split-K
    # scatter kind first: k_s2_scatter runs these two in the UNET_NO_DEEP_KERNELS rerun -- and on (5, 6, 18); KS 1 from odd fine extents
    (2, 32, 64, (8, 8, 32), 2, 0, "in"),
    (2, 32, 64, (8, 8, 32), 1, 1, "bn"),
    (2, 32, 64, (10, 12, 36), 2, 1, "in"),
    (2, 16, 32, (9, 13, 35), 3, 0, "bn"),
    (2, 16, 32, (9, 13, 35), 2, 1, "in"),
    # coarse grid (9, 10, 11): too narrow for k_s2_scatter, above the split-K kernel's 512 voxels -> the halo-tile scatter kind
    # (k_mfma_conv_p<1,2,0,..,true>) and the norm's separate launches
    (2, 16, 32, (17, 19, 21), 2, 1, "in"),
    # coarse grid (4, 5, 6): the split-K scatter kind k_deep_conv<1,2,0,true,DEEP_PLAIN> (a scattering kind has no norm epilogue:
    # deep_dgrad_outcome), then the norm's separate launches.  (<2,2,0,false,DEEP_BWD_NORM> is the conv_trans kind: the cases above)
    (2, 16, 32, (7, 9, 11), 1, 0, "bn"),
]


def bwd_inputs(case):
    tr, cin, cout, (D, H, W), a, acc, norm = case
    seed = 1000 + cin * 7 + cout * 13 + D * 17 + H * 19 + W * 23 + tr
    fine = {0: (D, H, W), 1: (2 * D, 2 * H, 2 * W), 2: ((D - 1) // 2 + 1, (H - 1) // 2 + 1, (W - 1) // 2 + 1)}[tr]   # the grid of dy
    dy = grid((*fine, cout), seed + 1, 1 / 8)
    w = grid((cin, cout, 2, 2, 2) if tr == 1 else (cout, cin, 3, 3, 3), seed + 2, 1 / 16)
    u = bf(rnd((D, H, W, cin), seed + 3, 1.0, 0.3))
    old = grid((D, H, W, cin), seed + 4, 1 / 128, 256) if acc else np.zeros((D, H, W, cin))
    gamma = rnd((cin,), seed + 5, 0.2, 1.0).astype(np.float32).astype(np.float64)
    sgn = np.where(np.random.default_rng(seed + 6).random(cin) < 0.5, -1.0, 1.0)
    beta = (sgn * (0.1 + 0.4 * np.random.default_rng(seed + 7).random(cin))).astype(np.float32).astype(np.float64)
    return dy, w, u, old, gamma, beta


def dgrad64(tr, dy, w, dims=None):
    d = torch.from_numpy(dy).permute(3, 0, 1, 2)[None]
    if tr == 1:
        g = torch.nn.functional.conv3d(d, torch.from_numpy(w), stride=2)
    elif tr == 2:   # onto the fine grid `dims`: an even extent has one more voxel than 2 * coarse - 1
        g = torch.nn.functional.conv_transpose3d(d, torch.from_numpy(w), stride=2, padding=1, output_padding=[1 - s % 2 for s in dims])
    else:
        g = torch.nn.functional.conv_transpose3d(d, torch.from_numpy(w), padding=1)
    return g[0].permute(1, 2, 3, 0).numpy()


def norm_bwd64(gview, u, gamma, beta, eps, a):
    """fp64 autograd through act(gamma (u - mean) rstd + beta), the statistics of u: dL/d(raw), coef, dgamma, dbeta and the sums' scales"""
    V, C = u.shape
    ut = torch.from_numpy(u).requires_grad_(True)
    gt, bt = torch.from_numpy(gamma).requires_grad_(True), torch.from_numpy(beta).requires_grad_(True)
    mean = ut.mean(0)
    rstd = 1.0 / torch.sqrt(((ut - mean) ** 2).mean(0) + eps)
    xhat = (ut - mean) * rstd
    z = gt * xhat + bt
    (act_t(z, a) * torch.from_numpy(gview)).sum().backward()
    xh, zz, rs, mn = xhat.detach().numpy(), z.detach().numpy(), rstd.detach().numpy(), mean.detach().numpy()
    ad = (zz > 0) + (zz <= 0) * {0: 1.0, 1: 0.0, 2: 0.01, 3: np.exp(np.minimum(zz, 0.0))}[a]
    dv = gview * ad
    return {"ad": ad, "du": ut.grad.numpy(), "dgamma": gt.grad.numpy(), "dbeta": bt.grad.numpy(), "c0": gamma * rs, "m1": dv.mean(0), "m2": (dv * xh).mean(0),
            "dv": dv, "xhat": xh, "z": zz, "rstd": rs, "mean": mn}


def bwd_closed(dv, xhat, c0, V, keep=None):
    """dL/d(raw) and the sums from dv (the norm backward's closed form; keep: the voxels the sums see)"""
    s = slice(None) if keep is None else keep
    m1, m2 = dv[s].sum(0) / V, (dv[s] * xhat[s]).sum(0) / V
    return {"du": c0 * (dv - m1 - xhat * m2), "m1": m1, "m2": m2, "dgamma": (dv[s] * xhat[s]).sum(0), "dbeta": dv[s].sum(0)}


def run_bwd(case, dy, w, u, old, stat, gamma):
    tr, cin, cout, (D, H, W), a, acc, norm = case
    dyd, wd, ud = dev(dy, torch.bfloat16), dev(w, torch.float32), dev(u, torch.bfloat16)
    sd, gd = dev(stat, torch.float32), dev(gamma, torch.float32)
    sc = scratch(cout, cin, D, H, W)
    outs = []
    for _ in range(2):
        dx = dev(old, torch.bfloat16) if acc else nan_like(torch.empty((D, H, W, cin), dtype=torch.bfloat16, device=DEV))
        coef = nan_like(torch.empty((3 * cin,), dtype=torch.float32, device=DEV))
        dgam = torch.ones((cin,), dtype=torch.float32, device=DEV)
        dbet = torch.ones((cin,), dtype=torch.float32, device=DEV)
        if tr == 2:
            E.check(E.lib.unet_op_conv3d_bwd_data_norm_strided(0, 2, dyd.data_ptr(), wd.data_ptr(), dx.data_ptr(), acc, ud.data_ptr(),
                                                               sd.data_ptr(), gd.data_ptr(), a, coef.data_ptr(), dgam.data_ptr(),
                                                               dbet.data_ptr(), cin, cout, D, H, W, sc.data_ptr(), stream()))
        else:
            E.check(E.lib.unet_op_conv3d_bwd_data_norm(tr, dyd.data_ptr(), wd.data_ptr(), dx.data_ptr(), acc, ud.data_ptr(), sd.data_ptr(),
                                                       gd.data_ptr(), a, coef.data_ptr(), dgam.data_ptr(), dbet.data_ptr(), cin, cout, D, H, W,
                                                       sc.data_ptr(), stream()))
        torch.cuda.synchronize()
        outs.append({"dx": dx, "coef": coef, "dgamma": dgam, "dbeta": dbet})
    for k in outs[0]:
        assert np.array_equal(bits(outs[0][k]), bits(outs[1][k])), "%s differs between two identical calls" % k
    return {k: v.float().cpu().numpy().astype(np.float64) for k, v in outs[0].items()}


@pytest.mark.parametrize("case", BWD_CASES, ids=lambda c: "%s_%dx%d_%dx%dx%d_act%d_acc%d_%s" % (("conv", "convt", "convs2")[c[0]], c[1], c[2], *c[3],
                                                                                             c[4], c[5], c[6]))
def test_dgrad_norm_backward_against_fp64(case):
    tr, cin, cout, (D, H, W), a, acc, norm = case
    V = D * H * W
    eps = EPS[norm]
    assert V > 1 or norm == "in", "BatchNorm training at one voxel is not defined"
    dy, w, u, old, gamma, beta = bwd_inputs(case)
    uf = u.reshape(V, cin)
    mean = uf.mean(0)
    rstd = 1.0 / np.sqrt(((uf - mean) ** 2).mean(0) + eps)
    scale = gamma * rstd
    stat = np.concatenate([mean, rstd, scale, beta - mean * scale]).astype(np.float32).astype(np.float64)
    got = run_bwd(case, dy, w, u, old, stat, gamma)

    gview = bf(dgrad64(tr, dy, w, (D, H, W)) + old).reshape(V, cin)       # the one rounding before dv: dL/d(view) = bf16(dgrad + old)
    R = norm_bwd64(gview, uf, gamma, beta, eps, a)
    if a in (1, 2):      # no pre-activation so close to the kink that the kernel's fp32 fma could take the other side of it
        st4 = stat.reshape(4, cin)
        assert np.all(np.abs(R["z"]) > 2.0 ** -20 * (np.abs(uf * st4[2]) + np.abs(st4[3]))), "test data too close to the activation's kink"
    dv, xh = R["dv"], R["xhat"]
    assert np.allclose(bwd_closed(dv, xh, R["c0"], V)["du"], R["du"], rtol=1e-9, atol=1e-12 * np.abs(R["du"]).max() + 1e-300)
    m2abs = np.abs(dv * xh).sum(0) / V
    bounds = {
        "du": 2.0 ** -8 * np.abs(R["du"]) + 1e-3 * np.abs(R["du"]).max()
              + 2.0 ** -20 * np.abs(R["c0"]) * (np.abs(dv) + np.abs(R["m1"]) + np.abs(R["m2"]) * R["rstd"] * (np.abs(uf) + np.abs(R["mean"]))),
        "c0": 1e-6 * np.abs(R["c0"]),
        "m1": 1e-4 * np.abs(dv).sum(0) / V + 1e-30,
        "m2": 1e-4 * m2abs + 1e-30,
        "dgamma": 1e-4 * np.abs(dv * xh).sum(0) + 2.0 ** -23 * np.abs(1 + R["dgamma"]),
        "dbeta": 1e-4 * np.abs(dv).sum(0) + 2.0 ** -23 * np.abs(1 + R["dbeta"]),
    }
    coef = got["coef"].reshape(3, cin)
    # dgamma / dbeta started at 1.0 (+= semantics); the subtraction is exact in fp64
    gotq = {"du": got["dx"].reshape(V, cin), "c0": coef[0], "m1": coef[1], "m2": coef[2], "dgamma": got["dgamma"] - 1.0, "dbeta": got["dbeta"] - 1.0}
    refq = {k: R[k] for k in ("du", "c0", "m1", "m2", "dgamma", "dbeta")}
    if V == 1:
        assert np.all(refq["du"] == 0)       # xhat = 0 and dv = mean(dv): no gradient reaches the raw tensor
    for k in refq:
        check(k, gotq[k], refq[k], bounds[k])

    # teeth
    def ratio(wr):
        return max(miss(wr[k], refq[k], bounds[k]) for k in ("du", "m1", "m2", "dgamma", "dbeta"))
    wl = w.copy()
    if tr == 1:
        wl[:, 0:32, 0, 0, 0] = 0.0
    else:
        wl[0:32, :, 1, 1, 1] = 0.0
    gl = bf(dgrad64(tr, dy, wl, (D, H, W)) + old).reshape(V, cin)
    teeth("a lost K range", ratio(bwd_closed(gl * R["ad"], xh, R["c0"], V)))
    if cin > 16:
        p = (np.arange(cin) + 16) % cin
        wr = bwd_closed(dv, xh, R["c0"], V)
        wr = {"m1": wr["m1"][p], "m2": wr["m2"][p], "dgamma": wr["dgamma"][p], "dbeta": wr["dbeta"][p]}
        wr["du"] = R["c0"] * (dv - wr["m1"] - xh * wr["m2"])
        teeth("statistics without the right row tile", ratio(wr))
    if V > 64:
        teeth("statistics without the right 64-voxel group", ratio(bwd_closed(dv, xh, R["c0"], V, keep=slice(64, None))))


def test_separate_launches_meet_the_same_bounds():
    """UNET_NO_DEEP_KERNELS=1 (read once per process): every case of this file on the MFMA conv / dgrad and the norm's separate
    launches, in a child process."""
    env = dict(os.environ, UNET_NO_DEEP_KERNELS="1")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-m", "gpu", "-p", "no:cacheprovider",
                          "-k", "not separate_launches"], capture_output=True, text=True, timeout=1200, env=env, cwd=root)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]
    assert " passed" in out.stdout and " failed" not in out.stdout
