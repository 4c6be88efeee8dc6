"""GPU: the recalibration pass on the device (include/unet_recal.h) -- unet_recal_eval against recal_ref (the fp64 restatement of
test_recal_host.py) inside its a-priori round-off bounds, every call twice into garbage-filled tables with guard words on both sides;
device against device bit for bit across load widths, candidate counts and splits of a volume; the special voxels; the cross-check
with the calibration tables' independent kernel; the fit end to end against an fp64 bisection; the fold; and qc.recalibration_qc
against the same composition written out by hand.  The voxel counts come from the kernel's own constants."""
import math
import os
import sys

import numpy as np
import pytest
import torch

import unet_studio_amd as U
from unet_studio_amd import calib as CB
from unet_studio_amd import postproc as P
from unet_studio_amd import qc as Q
from unet_studio_amd import recal as RC

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_recal_host import recal_ref, table_of  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F = np.float32
NAN, INF = float("nan"), float("inf")
ONE = 1 << RC.SCALE_BITS
G = 64                                                             # guard words on each side of a table
GUARD = -0x5A3C5A3C
N = RC.TABLE_LEN
BLOCK = RC.UNIT * RC.BLOCK_UNITS                                   # the voxels a block takes at once
STRIDE = RC.UNIT * RC.GRID_UNITS                                   # the voxels the capped grid takes per stride
BETAS = [0.0625, 0.3, 0.7, 1.0, 1.5, 2.5, 6.0, 16.0]
SHARE = {}                                                         # the largest share of a bound the device used, printed per check


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def offset(t, by):
    """a copy of the tensor t that starts `by` bytes after a 256-byte boundary"""
    n = by // t.element_size()
    assert n * t.element_size() == by
    buf = torch.empty(t.numel() + n, dtype=t.dtype, device=t.device)
    assert buf.data_ptr() % 256 == 0
    view = buf[n:].view(t.shape)
    view.copy_(t)
    return view


def run(logits, label, mask, betas, rep=0, accumulate=False, start=None):
    """one call into a guarded table (garbage-filled, or holding `start` for accumulate) -> the table as numpy"""
    buf = torch.full((N + 2 * G,), GUARD, dtype=torch.int64, device=DEV)
    out = buf[G:G + N]
    out[:] = 0x7B7B7B7B7B7B if rep == 0 else -3
    if start is not None:
        out.copy_(dev(start))
    got = RC.eval_betas(logits, label, betas, mask=mask, out=out, accumulate=accumulate)
    assert got.data_ptr() == out.data_ptr()
    b = buf.cpu().numpy()
    assert (b[:G] == GUARD).all() and (b[G + N:] == GUARD).all()
    return b[G:G + N].copy()


def check(x, label, mask, betas):
    """the device twice against recal_ref: the head exactly, every sum inside its bound -> (the restatement, the device's table)"""
    x = np.ascontiguousarray(x, F)
    ref = recal_ref(x, label, mask, betas)
    d_x, d_l, d_m = dev(x), dev(np.asarray(label, F)), None if mask is None else dev(np.asarray(mask, np.uint8))
    K = len(betas)
    for rep in range(2):
        t = run(d_x, d_l, d_m, betas, rep)
        assert t[:6].tolist() == ref["head"], (rep, t[:6].tolist(), ref["head"])
        assert (t[6 + 2 * K:] == 0).all()                           # the unused candidates read 0
        for k in range(K):
            for name, at in (("nll", 6 + 2 * k), ("g", 7 + 2 * k)):
                err, bound = abs(int(t[at]) - ref[name][k]) / ONE, ref[name + "_bound"][k]
                assert err <= bound, (name, k, betas[k], int(t[at]) / ONE, ref[name][k] / ONE, err, bound)
                # a sum of few voxels can differ by one step of 2^-20 and then uses much of its bound; the volumes say more
                key = (name, "volumes" if ref["head"][0] >= BLOCK // 2 else "a few voxels")
                if bound > 0 and err / bound > SHARE.get(key, (0.0,))[0]:
                    SHARE[key] = (err / bound, "C %d S %d beta %g: %d steps of 2^-20" % (x.shape[0], x.shape[1], betas[k], round(err * ONE)))
    assert sum(ref["head"][:5]) == x.shape[1]
    print("share of the bound used so far: " + "; ".join("%s, %s: %.4f (%s)" % (k + v) for k, v in sorted(SHARE.items())))
    return ref, t


# ---- inputs --------------------------------------------------------------------------------------------------------------------------
def volume(rng, C, S, scale=3.0, special=True, with_mask=True):
    x = (rng.standard_normal((C, S)) * scale).astype(F)
    label = rng.integers(0, C, S).astype(F)
    mask = None
    if special:
        for v, share in ((NAN, 0.02), (INF, 0.01), (-INF, 0.05)):
            at = np.flatnonzero(rng.random(S) < share)
            x[rng.integers(0, C, at.size), at] = v
        x[:, rng.random(S) < 0.01] = -INF                           # all channels -inf
        at = np.flatnonzero(rng.random(S) < 0.02)                   # the truth's channel alone: impossible
        x[label[at].astype(int), at] = -INF
        for i, v in enumerate([NAN, INF, -INF]):
            if i < S:
                x[i % C, i] = v
        for v, share in ((-0.5, 0.01), (C - 0.5, 0.01), (float(C), 0.01), (NAN, 0.01), (-1.0, 0.01)):
            label[rng.random(S) < share] = v
    if with_mask:
        mask = rng.choice(np.asarray([0, 1, 255], np.uint8), S, p=[0.2, 0.5, 0.3])
    return x, label, mask


# ---- 1. against the reference --------------------------------------------------------------------------------------------------------
COUNTS = [1, RC.UNIT - 1, RC.UNIT, BLOCK + 3 * RC.UNIT, BLOCK + 3 * RC.UNIT + 3]   # the last: a tail that is no whole unit


@pytest.mark.parametrize("C", [2, 6, 9, 17, 256])
@pytest.mark.parametrize("S", COUNTS)
def test_against_the_reference_around_a_unit_and_a_block(C, S):
    rng = np.random.default_rng(1000 * C + S)
    for K in (1, 2, 8):
        x, label, mask = volume(rng, C, S, scale=(1.0, 3.0, 10.0)[K % 3], special=S > RC.UNIT, with_mask=K != 2)
        ref, _ = check(x, label, mask, BETAS[:K] if K > 1 else [0.7])
        if S > BLOCK and K == 8:
            assert min(ref["head"][:5]) > 0                         # every kind of voxel took part


@pytest.mark.parametrize("C,K", [(6, 8), (9, 1)])
def test_the_capped_grid_strides_twice(C, K):
    S = 2 * STRIDE + 3
    rng = np.random.default_rng(C)
    x, label, mask = volume(rng, C, S)
    check(x, label, mask, BETAS[:K])
    check(x[:, :2 * STRIDE], label[:2 * STRIDE], None, BETAS[:K])   # 16-byte loads


# ---- 2. bits, device against device --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [6, 9])
def test_the_bits_do_not_depend_on_alignment_candidate_count_or_split(C):
    rng = np.random.default_rng(77 + C)
    for S in (BLOCK * 3 + 8, BLOCK * 3 + 7):
        x, label, mask = volume(rng, C, S)
        d_x, d_l, d_m = dev(x), dev(label), dev(mask)
        assert d_x.data_ptr() % 16 == 0 and d_l.data_ptr() % 16 == 0
        want = run(d_x, d_l, d_m, BETAS)
        assert want[0] > 0 and want[6] != 0 and want[7] != 0
        assert (run(d_x, d_l, d_m, BETAS, rep=1) == want).all()                               # a repeat
        o_x, o_l, o_m = offset(d_x, 4), offset(d_l, 4), offset(d_m, 1)
        assert o_x.data_ptr() % 16 == 4 and o_l.data_ptr() % 16 == 4
        assert run(o_x, o_l, o_m, BETAS).tobytes() == want.tobytes()                         # scalar loads
        assert run(o_x, d_l, d_m, BETAS).tobytes() == want.tobytes() and run(d_x, o_l, o_m, BETAS).tobytes() == want.tobytes()
        assert run(d_x, d_l, None, BETAS).tobytes() == run(o_x, o_l, None, BETAS, rep=1).tobytes()
        for k, b in enumerate(BETAS):                                                         # column k of K = 8 is the K = 1 call
            single = run(d_x, d_l, d_m, [b], rep=k & 1)
            assert single[:5].tobytes() == want[:5].tobytes()
            assert single[6:8].tobytes() == want[6 + 2 * k:8 + 2 * k].tobytes(), (k, b)
        for K in (2, 3, 4, 5):
            part = run(d_x, d_l, d_m, BETAS[:K])
            assert part[6:6 + 2 * K].tobytes() == want[6:6 + 2 * K].tobytes() and (part[6 + 2 * K:] == 0).all()
        cut = int(rng.integers(1, S - 1))                                                     # two arbitrary halves add up to the whole
        first = run(d_x[:, :cut].contiguous(), d_l[:cut].contiguous(), d_m[:cut].contiguous(), BETAS)
        both = run(d_x[:, cut:].contiguous(), d_l[cut:].contiguous(), d_m[cut:].contiguous(), BETAS, rep=1, accumulate=True, start=first)
        assert both.tobytes() == want.tobytes(), cut


# ---- 3. the special voxels -----------------------------------------------------------------------------------------------------------
def test_special_voxels_clamped_terms_and_accumulate():
    C = 3
    cols = [([0.0, 0.0, -INF], 0, 1), ([0.0, -INF, -INF], 0, 1), ([0.0, -INF, -INF], 1, 1), ([NAN, 0.0, 0.0], 1, 1), ([0.0, INF, 0.0], 0, 255),
            ([-INF, -INF, -INF], 0, 1), ([0.5, -1.0, 2.0], -0.5, 1), ([0.5, -1.0, 2.0], C - 0.5, 1), ([0.5, -1.0, 2.0], float(C), 1),
            ([0.5, -1.0, 2.0], NAN, 1), ([NAN, 0.0, 0.0], NAN, 0), ([NAN, 0.0, 0.0], NAN, 1), ([NAN, -INF, 0.0], 1, 1),
            ([5000.0, -5000.0, -INF], 1, 1), ([5000.0, -5000.0, -5000.0], 0, 1), ([-5000.0, 5000.0, 0.0], 0, 7), ([1.0, 2.0, 3.0], 2, 0)]
    x = np.asarray([c[0] for c in cols], F).T
    label, mask = np.asarray([c[1] for c in cols], F), np.asarray([c[2] for c in cols], np.uint8)
    betas = [16.0, 1.0, 0.0625]
    ref, t = check(x, label, mask, betas)
    assert ref["head"] == [7, 4, 3, 2, 1, 2]
    # the two clamped voxels enter with the clamped values: nll 160000 and g 10000 at beta 16 both read 4096
    only = recal_ref(x[:, 13:14], label[13:14], None, betas)
    assert only["head"] == [1, 0, 0, 0, 0, 1] and only["nll"] == [4096 * ONE, 4096 * ONE, 625 * ONE] and only["g"] == [4096 * ONE] * 3
    got = run(dev(x[:, 13:14]), dev(label[13:14]), None, betas)
    assert (got == table_of(only)).all()                           # exact: every term is a clamp or an integer
    hand = run(dev(np.asarray([[0.0], [0.0]], F)), dev(np.zeros(1, F)), None, [0.5, 1.0, 3.0])
    assert hand[:6].tolist() == [1, 0, 0, 0, 0, 0] and [int(v) for v in hand[7:12:2]] == [0, 0, 0]
    assert all(abs(int(v) / ONE - math.log(2.0)) < 2.0 ** -19 for v in hand[6:12:2])
    # accumulate into a non-zero table adds, entry by entry, the unused candidates included
    start = np.arange(1, N + 1, dtype=np.int64) * 1000003 - 7
    d_x, d_l, d_m = dev(x), dev(label), dev(mask)
    once = run(d_x, d_l, d_m, betas)
    assert (run(d_x, d_l, d_m, betas, rep=1, accumulate=True, start=start) == start + once).all()
    assert (once == t).all()
    with pytest.raises(U.UNetError, match="accumulate needs the table"):
        RC.eval_betas(d_x, d_l, betas, accumulate=True)
    with pytest.raises(U.UNetError, match=r"betas\[1\] must be finite and positive"):
        RC.eval_betas(d_x, d_l, [1.0, 0.0])
    with pytest.raises(U.UNetError, match="n_betas must be in"):
        RC.eval_betas(d_x, d_l, [1.0] * 9)
    with pytest.raises(U.UNetError, match="label holds 3 voxels"):
        RC.eval_betas(d_x, d_l[:3].contiguous(), [1.0])


# ---- 4. the cross-check with an independent kernel -------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [4, 11])
def test_head_and_nll_agree_with_the_calibration_tables(C):
    S = BLOCK * 2 + 5
    rng = np.random.default_rng(40 + C)
    x, label, mask = volume(rng, C, S, scale=1.5, special=False)
    x[rng.integers(0, C, 40), rng.integers(0, S, 40)] = NAN         # bad voxels, invalid labels and the mask, but no single -inf:
    x[:, rng.integers(0, S, 20)] = -INF                             # no voxel is impossible
    label[rng.integers(0, S, 30)] = float(C)
    ref = recal_ref(x, label, mask, [1.0])
    assert ref["head"][4] == 0 and ref["head"][5] == 0 and min(ref["head"][:4]) > 0
    d_x, d_l, d_m = dev(x), dev(label), dev(mask)
    t = run(d_x, d_l, d_m, [1.0])
    head, _, _, logh = CB.split(CB.tables(d_x, d_l, mask=d_m), C)
    assert t[:4].tolist() == head.tolist() == ref["head"][:4]
    lo, _, hi = CB.nll_bounds(logh)                                 # p_t > 1e-12, the floor: logits of scale 1.5
    valid = int(t[0])
    mean, slack = int(t[6]) / ONE / valid, ref["nll_bound"][0] / valid
    print("nll %.9g in [%.9g, %.9g]" % (mean, lo, hi))
    assert lo - slack <= mean <= hi + slack


# ---- 5. the fit, end to end ------------------------------------------------------------------------------------------------------------
def g_total(x, t, beta):
    """fp64: the slope of the summed nll at beta, unquantised"""
    d = x - x.max(axis=0)
    e = np.exp(beta * d)
    return float(((e * d).sum(axis=0) / e.sum(axis=0) - d[t, np.arange(t.size)]).sum())


def bisect(x, t, lo=2.0 ** -6, hi=2.0 ** 6):
    assert g_total(x, t, lo) < 0.0 < g_total(x, t, hi)
    while hi - lo > 1e-12:
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if g_total(x, t, mid) < 0.0 else (lo, mid)
    return 0.5 * (lo + hi)


def draw(rng, x, beta):
    """labels drawn from softmax(beta * x)"""
    p = np.exp(beta * (x - x.max(axis=0)))
    cdf = np.cumsum(p / p.sum(axis=0), axis=0)
    return np.minimum((rng.random(x.shape[1]) > cdf).sum(axis=0), x.shape[0] - 1)


def inside(bracket, value):
    return bracket[0] * (1.0 - 2.0 ** -12) <= value <= bracket[1] * (1.0 + 2.0 ** -12)


def test_the_fit_end_to_end():
    C, S = 6, 16 ** 3
    rng = np.random.default_rng(2024)
    x = (3.0 * rng.standard_normal((C, S))).astype(F)
    x64 = x.astype(np.float64)
    t = draw(rng, x64, 0.7)
    star = bisect(x64, t)
    assert 0.6 < star < 0.8
    d_x = dev(x).view(C, 16, 16, 16)
    calls = []

    def batches(label):
        def gen():
            calls.append(1)
            yield d_x, dev(label.astype(F))
        return gen

    r = RC.fit(batches(t))
    print("beta* %.12g, fitted %.12g, bracket %r" % (star, r["beta"], r["bracket"]))
    assert r["at_bound"] == 0 and r["rounds"] == 3 and len(calls) == 3 and r["valid"] == S      # one pass over the cases per round
    assert inside(r["bracket"], star) and abs(math.log2(r["bracket"][1] / r["bracket"][0]) - RC.Solver().width()) < 1e-6
    assert r["bracket"][0] <= r["beta"] <= r["bracket"][1] and abs(r["beta"] / star - 1.0) < 1e-4 and r["temperature"] == 1.0 / r["beta"]
    # two cases that accumulate, the second with its own mask, against one call over both
    m = (rng.random(S) < 0.5).astype(np.uint8)
    both = RC.fit(lambda: iter([(d_x, dev(t.astype(F))), (d_x, dev(t.astype(F)), dev(m))]))
    keep = np.concatenate([np.ones(S, bool), m > 0])
    star2 = bisect(np.concatenate([x64, x64], axis=1)[:, keep], np.concatenate([t, t])[keep])
    assert inside(both["bracket"], star2) and both["valid"] == int(keep.sum())
    # certain and right: sharper is better without end; certain and wrong: flatter is
    sharp = dev((50.0 * x).astype(F))
    r = RC.fit(lambda: iter([(sharp, dev(x.argmax(axis=0).astype(F)))]))
    assert r["at_bound"] == 1 and r["beta"] == 16.0 and r["bracket"] == (16.0, 16.0) and r["rounds"] == 1
    r = RC.fit(lambda: iter([(d_x, dev(x.argmin(axis=0).astype(F)))]))
    assert r["at_bound"] == -1 and r["beta"] == 0.0625 and r["rounds"] == 1


# ---- 6. the fold -----------------------------------------------------------------------------------------------------------------------
SMALL_ARCH = ("conv8,ks3,stride1+norm,leaky_relu+conv8,ks3,stride1+norm,leaky_relu\n"
              "conv16,ks3,stride2+norm,leaky_relu+conv16,ks3,stride1+norm,leaky_relu+conv_trans8,ks2,stride2\n"
              "conv8,ks3,stride1+norm,leaky_relu+conv8,ks3,stride1+norm,leaky_relu+%s")
DEEP_ARCH = ("conv8,ks3,stride1+norm,leaky_relu\n"
             "conv16,ks3,stride2+norm,leaky_relu\n"
             "conv16,ks3,stride2+norm,leaky_relu+conv_trans16,ks2,stride2\n"
             "conv16,ks3,stride1+norm,leaky_relu+%s+conv_trans8,ks2,stride2\n"
             "conv8,ks3,stride1+norm,leaky_relu+%s")


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


HEAD5 = "conv5,ks1,stride1"
CHAIN = "softmax+create_mask+argmax"


@pytest.mark.parametrize("arch,n,dtype,levels", [(SMALL_ARCH % HEAD5, 16, "fp32", 1), (SMALL_ARCH % HEAD5, 16, "bf16", 1),
                                                 (DEEP_ARCH % (HEAD5, HEAD5), 16, "fp32", 2), (DEEP_ARCH % (HEAD5, HEAD5), 16, "bf16", 2),
                                                 (None, 32, "bf16", 5)],
                         ids=["three-lines-fp32", "three-lines-bf16", "coarse-head-fp32", "coarse-head-bf16", "default-32-bf16"])
def test_fold_scales_the_level0_logits_and_nothing_else(arch, n, dtype, levels):
    C = 5
    arch = U.default_feature(C) if arch is None else arch
    g = torch.Generator().manual_seed(n)
    x = torch.randn(1, 1, n, n, n, generator=g).to(DEV)
    for beta in (0.5, 2.0):
        m = U.UNet3d(1, C, arch, device=DEV, dtype=dtype, seed=11)
        m.prepare_for_inference()
        before = [o.clone() for o in m.forward(x)]
        assert len(before) == levels and all(o is not None for o in before)
        # the label map at threshold 0: the largest foreground class wherever the foreground has any probability, which no positive
        # scale changes.  (At the default threshold 0.5 the fold moves the foreground probability across it: that is its purpose.)
        label = P.run_postproc(before[0], CHAIN, {"argmax": 0.0}, outputs=("label",))["label"].clone()
        assert int(label.to(torch.int32).min()) > 0
        params = [p.clone() for p in m.parameters()]
        version = m._params_version
        assert RC.fold(m, beta) == beta and m._params_version == version + 1
        names = m._probe.param_names
        for nm, p, q in zip(names, params, m.parameters()):
            assert same(q, p * beta if nm.startswith("output0.") else p), nm
        after = m.forward(x)
        assert same(after[0], before[0] * beta)                     # a power of two scales exactly
        assert before[0].abs().max() > 0
        for a, b in zip(after[1:], before[1:]):
            assert same(a, b)                                       # the coarse heads are not touched
        assert same(P.run_postproc(after[0], CHAIN, {"argmax": 0.0}, outputs=("label",))["label"], label)
        assert same(torch.argmax(after[0], dim=1), torch.argmax(before[0], dim=1))
        assert same(m._forward_level0(x), before[0] * beta)


def test_fold_refuses_a_head_with_an_activation_and_a_refit_finds_one():
    C, n = 5, 16
    m = U.UNet3d(1, C, SMALL_ARCH % "conv5,ks1,stride1,leaky_relu", device=DEV, dtype="fp32", seed=3)
    params = [p.clone() for p in m.parameters()]
    with pytest.raises(U.UNetError, match="the level-0 head 'conv5,ks1,stride1,leaky_relu' is not a bare conv"):
        RC.fold(m, 2.0)
    assert all(same(p, q) for p, q in zip(params, m.parameters()))
    m = U.UNet3d(1, C, SMALL_ARCH % "conv5,ks1,stride1", device=DEV, dtype="fp32", seed=3)
    m.prepare_for_inference()
    RC.fold(m, 8.0)                                                 # a fresh head's logits are small: give them a spread
    g = torch.Generator().manual_seed(5)
    x = torch.randn(1, 1, n, n, n, generator=g).to(DEV)
    logits = m._forward_level0(x)[0].view(C, -1).cpu().numpy().astype(np.float64)
    t = dev(draw(np.random.default_rng(8), logits, 0.7).astype(F))

    def batches():
        yield m._forward_level0(x)[0], t

    first = RC.fit(batches)
    assert first["at_bound"] == 0 and 0.2 < first["beta"] < 2.0
    RC.fold(m, first["beta"])
    second = RC.fit(batches)
    print("first %r, second %r" % (first, second))
    assert second["at_bound"] == 0 and inside(second["bracket"], 1.0)


# ---- 7. recalibration_qc ----------------------------------------------------------------------------------------------------------------
def test_recalibration_qc_report_equals_the_composition_by_hand(tmp_path):
    dim, C = (16, 16, 16), 4
    W, H, D = dim
    S = W * H * D
    m = U.UNet3d(1, C, SMALL_ARCH % "conv4,ks1,stride1", device=DEV, dtype="fp32", seed=9)
    m.dim, m.voxel_size = dim, (1.0, 1.0, 1.0)
    m.prepare_for_inference()
    RC.fold(m, 8.0)
    g = torch.Generator().manual_seed(3)

    def vol(max_label):
        lab = torch.randint(0, max_label + 1, (D, H, W), generator=g).to(torch.float32)
        lab[torch.rand(D, H, W, generator=g) < 0.4] = 0.0
        lab.view(-1)[0] = max_label
        return torch.randn(1, D, H, W, generator=g).numpy(), lab.numpy()

    cases = [("/data/tpl/t0_T1w.nii.gz", "/data/tpl/t0_label.nii.gz") + vol(2) + (True,),
             ("/data/sub-01/anat/sub-01_T1w.nii.gz", "/data/sub-01/anat/sub-01_dseg.nii.gz") + vol(1) + (False,),     # 1 < 2, 1 + 2 < 4: shifted
             ("/data/tpl/t1_T1w.nii.gz", "/data/tpl/t1_label.nii.gz") + vol(2) + (True,)]
    # labels the model half agrees with, so that the fit has something to find
    for k in (0, 2):
        x = torch.from_numpy(cases[k][2]).view(1, 1, D, H, W).to(DEV)
        pred = m._forward_level0(x)[0].view(C, S).argmax(dim=0).to(torch.float32).cpu().numpy().reshape(D, H, W)
        lab = np.where(np.random.default_rng(k).random((D, H, W)) < 0.5, np.minimum(pred, 2.0), cases[k][3]).astype(F)
        lab.reshape(-1)[0] = 2.0
        cases[k] = cases[k][:3] + (lab, True)
    assert Q.label_plan(cases, C)[1] == [False, True, False]
    path = str(tmp_path / "qc_model.nz")
    report = str(tmp_path / "qc_model.recalibration_report.tsv")
    for kw in (dict(), dict(mask="foreground", u_range=(-3.0, 3.0), rounds=2)):
        assert Q.recalibration_qc(m, path, cases, **kw) == (0, report)
        got = open(report, "rb").read()
        assert sorted(os.listdir(tmp_path)) == ["qc_model.recalibration_report.tsv"]      # no .tmp left behind
        # by hand through the public functions on further forwards of the same model: the engine's fp32 forward is deterministic
        def batches():
            for case in (cases[0], cases[2]):
                x = torch.from_numpy(case[2]).view(1, 1, D, H, W).to(DEV)
                t = torch.from_numpy(case[3]).view(-1).to(DEV)
                logits = m._forward_level0(x)[0]
                region = None
                if kw.get("mask") == "foreground":
                    region = ((torch.trunc(t) != 0) | (torch.argmax(logits.view(C, S), dim=0) != 0)).to(torch.uint8)
                yield logits, t, region

        fitted = RC.fit(batches, solver=RC.Solver(*kw.get("u_range", (-4.0, 4.0)), rounds=kw.get("rounds", 3)))
        total = torch.zeros(N, dtype=torch.int64, device=DEV)
        tables, bound = [], [0.0, 0.0]
        for logits, t, region in batches():
            table = RC.eval_betas(logits, t, (1.0, fitted["beta"]), mask=region)
            total += table
            tables.append(table.cpu())
            ref = recal_ref(logits.view(C, S).cpu().numpy(), t.cpu().numpy(), None if region is None else region.cpu().numpy(), (1.0, fitted["beta"]))
            bound = [bound[0] + ref["nll_bound"][0], bound[1] + ref["nll_bound"][1]]
        fitted["table"] = total.cpu()
        rows = [(cases[0][0], cases[0][1], tables[0]), (cases[1][0], cases[1][1], None), (cases[2][0], cases[2][1], tables[1])]
        assert RC.format_report(rows, fitted).encode() == got
        lines = [l.split("\t") for l in got.decode().splitlines()]
        assert len(lines) == 5 and lines[0][:5] == ["image", "ground_truth", "voxels", "nll_before", "nll_after"] and len(lines[0]) == 12
        assert lines[2] == ["sub-01_T1w.nii.gz", "sub-01_dseg.nii.gz", "N/A", "N/A", "N/A"] + [""] * 7
        assert lines[4][:2] == ["total", ""] and int(lines[4][2]) == int(lines[1][2]) + int(lines[3][2])
        assert (0 < int(lines[1][2]) <= S) if "mask" in kw else int(lines[1][2]) == S
        valid = int(lines[4][2])
        before, after = float(lines[4][3]), float(lines[4][4])
        print("total: nll %.9g -> %.9g at beta %s (at_bound %s)" % (before, after, lines[4][5], lines[4][9]))
        assert after <= before + (bound[0] + bound[1]) / valid
        assert float(lines[4][5]) == pytest.approx(fitted["beta"], rel=1e-8) and int(lines[4][9]) == fitted["at_bound"]
    # apply: the folded model is an ordinary model, and the calibration tables see the new probabilities
    params = [p.clone() for p in m.parameters()]
    assert Q.recalibration_qc(m, path, cases, apply=True) == (0, report)
    line = open(report).read().splitlines()[4].split("\t")
    beta, after = float(np.float32(float(line[5]))), float(line[4])
    names = m._probe.param_names
    changed = [nm for nm, p, q in zip(names, params, m.parameters()) if not same(p, q)]
    assert changed == ["output0.0.weight", "output0.0.bias"] or beta == 1.0
    total = torch.zeros(CB.table_len(C), dtype=torch.int64, device=DEV)
    for case in (cases[0], cases[2]):
        x = torch.from_numpy(case[2]).view(1, 1, D, H, W).to(DEV)
        total += CB.tables(m._forward_level0(x)[0], torch.from_numpy(case[3]).view(-1).to(DEV))
    lo, _, hi = CB.nll_bounds(CB.split(total, C)[3])
    print("folded: nll_after %.9g in [%.9g, %.9g]" % (after, lo, hi))
    assert lo <= after <= hi
    bad = [cases[0][:2] + (cases[0][2][:, :8], cases[0][3], True)]
    assert Q.recalibration_qc(m, path, bad) == (1, "/data/tpl/t0_T1w.nii.gz: training data dimension mismatch")
    refused = U.UNet3d(1, C, SMALL_ARCH % "conv4,ks1,stride1,leaky_relu", device=DEV, dtype="fp32", seed=9)
    refused.dim = dim
    assert Q.recalibration_qc(refused, path, cases, apply=True)[0] == 1
