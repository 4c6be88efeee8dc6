"""GPU: the post-processing chain (include/unet_postproc.h) on the device.  The fused softmax / create_mask / argmax pass against
fp64 torch on the CPU; defragment against the numpy union-find restatement of tests/test_postproc_host.py (kept sets equal, and the
same call twice bitwise identical); the per-plane ops against numpy and oracle.augment_ref._smooth; and EvaluateUNet with
postproc="model" against the restatement applied to the logits of a run without post-processing."""
import os
import sys
import threading

import numpy as np
import pytest
import torch

import unet_studio_amd as U
from unet_studio_amd import postproc as P
from oracle import augment_ref as R

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_postproc_host import kept_mask  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GAP = 1e-5   # the tie rule: labels are compared where the top two foreground probabilities, and fg_prob and the threshold, lie apart

SMOKE_ARCH = ("conv8,ks3,stride1+norm,leaky_relu+conv8,ks3,stride1+norm,leaky_relu\n"
              "conv16,ks3,stride2+norm,leaky_relu+conv16,ks3,stride1+norm,leaky_relu+conv_trans8,ks2,stride2\n"
              "conv8,ks3,stride1+norm,leaky_relu+conv8,ks3,stride1+norm,leaky_relu+conv%d,ks1,stride1")
MIX_ARCH = ("conv8,ks3,stride1+norm,elu+conv8,ks3,stride1+norm,leaky_relu\n"
            "conv16,ks3,stride2+norm,elu+conv16,ks3,stride1+norm,leaky_relu\n"
            "max_pool+conv16,ks3,stride1+norm,relu+upsample\n"
            "conv16,ks3,stride1+norm,leaky_relu+conv%d,ks1,stride1+conv_trans8,ks2,stride2\n"
            "conv8,ks3,stride1+norm,leaky_relu+conv%d,ks1,stride1")


# ---- the restatement ---------------------------------------------------------------------------------------------------------
def ref_softmax(lg, thr=0.5):
    """lg {C, S} -> (label_prob {C-1, S} fp64, fg_prob {S} fp64, label {S} int64, comparable {S} bool) by torch on the CPU in fp64"""
    p = torch.softmax(lg.double().cpu(), 0)
    fg = p[1:].sum(0)
    top = p[1:].topk(min(2, p.shape[0] - 1), 0).values
    am = p[1:].argmax(0) + 1
    lab = torch.where(fg > thr, am, torch.zeros_like(am))
    ok = (fg - thr).abs() >= GAP
    if top.shape[0] == 2:
        ok &= ((top[0] - top[1]) >= GAP) | (top[0] == top[1])   # equal logits give equal p: the first index wins
    ok |= torch.isnan(fg)
    return p[1:], fg, lab, ok


def assert_probs(got, exp):
    got = got.cpu().double()
    assert torch.equal(torch.isnan(got), torch.isnan(exp))
    fin = ~torch.isnan(exp)
    if fin.any():
        assert (got[fin] - exp[fin]).abs().max().item() <= 2e-6


def assert_labels(got, exp, ok):
    got = got.cpu().to(torch.int64).reshape(-1)
    assert torch.equal(got[ok], exp[ok]), int((got[ok] != exp[ok]).sum())


def make_logits(C, S, seed, special=False):
    g = torch.Generator().manual_seed(seed)
    lg = torch.randn(C, S, generator=g) * 4
    if C > 2 and S > 4:
        idx = torch.randperm(S, generator=g)[: max(1, S // 8)]
        lg[2, idx] = lg[1, idx]                          # exact ties between foreground channels: the first index wins
    if special and S >= 8:
        inf = float("inf")
        lg[0, 0] = float("nan")
        lg[C - 1, 1] = inf
        lg[:, 2] = -inf
        lg[1:, 3] = -inf                                 # background only: fg 0
        lg[0, 4] = -inf
        lg[1, 5], lg[C - 1, 5] = inf, inf
        lg[C - 1, 6] = -inf
    return lg


def fused(lg, thr=0.5, want=("label_prob", "fg_prob", "label"), offset=0):
    """unet_postproc_softmax on a device copy of lg; offset > 0 shifts every array by that many elements (unaligned pointers)"""
    C, S = lg.shape
    buf = torch.full((C * S + offset,), 7.0, device=DEV)
    d = buf[offset:].view(C, S)
    d.copy_(lg)
    lpb = torch.full(((C - 1) * S + offset,), 7.0, device=DEV)
    fgb = torch.full((S + offset,), 7.0, device=DEV)
    lbb = torch.full((S + offset,), 7, dtype=torch.uint16, device=DEV)
    lp, fg, lab = lpb[offset:].view(C - 1, S), fgb[offset:], lbb[offset:]
    P.softmax_call(d, C, S, thr, lp if "label_prob" in want else None, fg if "fg_prob" in want else None,
                   lab if "label" in want else None)
    torch.cuda.synchronize()
    return lp, fg, lab


@pytest.mark.parametrize("C", [2, 3, 6, 33, 130])
@pytest.mark.parametrize("S", [1, 7, 4099, 64 ** 3])
def test_fused_pass_against_fp64(C, S):
    lg = make_logits(C, S, 10 * C + S % 97, special=True)
    lp, fg, lab = fused(lg)
    elp, efg, elab, ok = ref_softmax(lg)
    assert_probs(lp, elp)
    assert_probs(fg, efg)
    assert_labels(lab, elab, ok)


def test_fused_pass_nan_and_inf_follow_torch():
    lg = make_logits(5, 16, 3, special=True)
    lp, fg, lab = fused(lg)
    fg = fg.cpu()
    for v in (0, 1, 2, 5):          # NaN, +inf, all -inf, two +inf: every probability NaN, label 0
        assert torch.isnan(fg[v]) and torch.isnan(lp[:, v].cpu()).all() and int(lab[v]) == 0
    assert float(fg[3]) == 0.0 and int(lab[3]) == 0 and (lp[:, 3].cpu() == 0).all()
    assert float(fg[4]) == pytest.approx(1.0, abs=1e-6)   # background -inf: all mass in the foreground
    assert float(lp[3, 6].cpu()) == 0.0


@pytest.mark.parametrize("mask", range(1, 8))
def test_every_subset_of_outputs_and_untouched_ones(mask):
    want = tuple(n for i, n in enumerate(("label_prob", "fg_prob", "label")) if mask >> i & 1)
    lg = make_logits(6, 4099, 5)
    lp, fg, lab = fused(lg, 0.3, want)
    elp, efg, elab, ok = ref_softmax(lg, 0.3)
    if "label_prob" in want:
        assert_probs(lp, elp)
    else:
        assert (lp.cpu() == 7.0).all()
    if "fg_prob" in want:
        assert_probs(fg, efg)
    else:
        assert (fg.cpu() == 7.0).all()
    if "label" in want:
        assert_labels(lab, elab, ok)
    else:
        assert (lab.cpu().to(torch.int64) == 7).all()


@pytest.mark.parametrize("offset", [1, 2, 3])
@pytest.mark.parametrize("S", [4096, 4099])
def test_unaligned_pointers(offset, S):
    lg = make_logits(6, S, offset)
    lp, fg, lab = fused(lg, 0.5, offset=offset)
    elp, efg, elab, ok = ref_softmax(lg)
    assert_probs(lp, elp)
    assert_probs(fg, efg)
    assert_labels(lab, elab, ok)


def test_two_threads_on_two_streams():
    cases = [make_logits(33, 64 ** 3, 1), make_logits(6, 64 ** 3 + 3, 2)]
    got, errs = [None, None], []

    def work(i):
        try:
            s = torch.cuda.Stream(DEV)
            with torch.cuda.stream(s):
                for _ in range(3):
                    lg = cases[i].to(DEV)
                    got[i] = P.run_postproc(lg.view(lg.shape[0], 1, 1, -1), "softmax+create_mask+argmax",
                                            outputs=("label_prob", "fg_prob", "label"))
            s.synchronize()
        except Exception as e:   # noqa: BLE001
            errs.append(e)

    th = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errs, errs
    for i in range(2):
        elp, efg, elab, ok = ref_softmax(cases[i])
        assert_probs(got[i]["label_prob"].view(elp.shape), elp)
        assert_probs(got[i]["fg_prob"].view(-1), efg)
        assert_labels(got[i]["label"], elab, ok)


# ---- defragment --------------------------------------------------------------------------------------------------------------
def snake(D, H, W):
    m = np.zeros((D, H, W), bool)
    for z in range(0, D, 2):
        for y in range(H):
            if y % 2 == 0:
                m[z, y] = True
            else:
                m[z, y, W - 1 if (y // 2) % 2 == 0 else 0] = True
    for z in range(1, D, 2):
        if z % 4 == 1:
            m[z, 0, 0] = True
        else:
            m[z, H - 1, W - 1] = True
        m[z, 1, W // 2] = True            # an isolated voxel
    return m


def spiral(n, D=3):
    m = np.zeros((D, n, n), bool)
    y, x, dy, dx = 0, 0, 0, 1
    lengths = [n - 1, n - 1, n - 1]
    k = n - 3
    while k > 0:
        lengths += [k, k]
        k -= 2
    m[1, 0, 0] = True
    for L in lengths:
        for _ in range(L):
            y, x = y + dy, x + dx
            m[1, y, x] = True
        dy, dx = dx, -dy
    m[0, n // 2, 0] = True
    return m


def masks():
    rs = np.random.RandomState(7)
    yield "empty", np.zeros((4, 5, 6), bool)
    yield "full", np.ones((5, 6, 7), bool)
    one = np.zeros((3, 4, 5), bool)
    one[1, 2, 3] = True
    yield "one", one
    yield "1x1xN", rs.rand(1, 1, 1000) < 0.6
    yield "odd", rs.rand(5, 7, 9) < 0.45
    yield "snake", snake(9, 17, 33)
    yield "spiral", spiral(41)
    yield "perc48", rs.rand(48, 40, 56) < 0.31
    yield "perc_large", rs.rand(192, 224, 192) < 0.31


def defrag_case(mask, ratio, seed):
    """fg_prob: above 0.5 exactly in the mask; label_prob 3 planes and label derived from it"""
    rs = np.random.RandomState(seed)
    fg = np.where(mask, 0.5 + 0.5 * rs.rand(*mask.shape).astype(np.float32) + 1e-3, 0.5 * rs.rand(*mask.shape)).astype(np.float32)
    fg = np.minimum(fg, 1.0).astype(np.float32)
    lp = rs.rand(3, *mask.shape).astype(np.float32)
    lab = rs.randint(0, 4, mask.shape).astype(np.uint16)
    return fg, lp, lab


def run_defrag(fg, lp, lab, ratio, each=False):
    D, H, W = fg.shape
    dfg, dlp = torch.from_numpy(fg).to(DEV), torch.from_numpy(lp).to(DEV)
    dlab = torch.from_numpy(lab.astype(np.int32)).to(DEV).to(torch.uint16)
    scratch = torch.empty(P.postproc_scratch_bytes(lp.shape[0] + 1, fg.size) + 3, dtype=torch.uint8, device=DEV)[3:]   # unaligned
    if each:
        P.defragment_call((W, H, D), True, 0.5, ratio, None, dlp, lp.shape[0], None, scratch)
    else:
        P.defragment_call((W, H, D), False, 0.5, ratio, dfg, dlp, lp.shape[0], dlab, scratch)
    torch.cuda.synchronize()
    return dfg.cpu().numpy(), dlp.cpu().numpy(), dlab.cpu().to(torch.int32).numpy().astype(np.uint16)


@pytest.mark.parametrize("name", [n for n, _ in masks()])
def test_defragment_against_the_restatement(name):
    mask = dict(masks())[name]
    for ratio in (0.05, 0.5):
        fg, lp, lab = defrag_case(mask, ratio, 1)
        gfg, glp, glab = run_defrag(fg, lp, lab, ratio)
        drop = mask & ~kept_mask(mask, ratio)
        assert np.array_equal(gfg, np.where(drop, 0, fg))
        assert np.array_equal(glp, np.where(drop[None], 0, lp))
        assert np.array_equal(glab, np.where(drop, 0, lab))
        again = run_defrag(fg, lp, lab, ratio)
        assert all(np.array_equal(a, b) for a, b in zip(again, (gfg, glp, glab)))   # bitwise the same run to run
        if name == "snake":
            assert drop.sum() == (mask.shape[0] // 2) and not drop[0].any()          # the isolated voxels go, the chain stays


def test_defragment_size_ratio_boundary_is_inclusive():
    mask = np.zeros((1, 3, 25), bool)
    mask[0, 0, :20] = True          # 20 voxels
    mask[0, 2, :10] = True          # 10 = 0.5 * 20: kept
    mask[0, 2, 24] = True           # 1 < 0.5 * 20: dropped
    fg, lp, lab = defrag_case(mask, 0.5, 2)
    gfg, _, _ = run_defrag(fg, lp, lab, 0.5)
    assert (gfg[0, 0, :20] > 0.5).all() and (gfg[0, 2, :10] > 0.5).all() and gfg[0, 2, 24] == 0
    gfg, _, _ = run_defrag(fg, lp, lab, 0.5000001)
    assert (gfg[0, 2, :10] == 0).all() and (gfg[0, 0, :20] > 0.5).all()


def test_defragment_each_per_plane():
    rs = np.random.RandomState(3)
    lp = rs.rand(5, 13, 11, 17).astype(np.float32)        # 5 planes: one chunk of 4 and one of 1
    lp[1] = np.where(snake(13, 11, 17), 0.9, 0.1)
    fg, lab = np.zeros(lp.shape[1:], np.float32), np.zeros(lp.shape[1:], np.uint16)
    for ratio in (0.05, 0.3):
        _, glp, _ = run_defrag(fg, lp, lab, ratio, each=True)
        for p in range(lp.shape[0]):
            m = lp[p] > 0.5
            drop = m & ~kept_mask(m, ratio)
            assert np.array_equal(glp[p], np.where(drop, 0, lp[p])), p


# ---- per-plane ops -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(7, 9, 11), (1, 1, 5), (16, 16, 16)])
def test_plane_ops_against_numpy(shape):
    rs = np.random.RandomState(4)
    lp = (rs.rand(6, *shape).astype(np.float32) * 1.5 - 0.25).astype(np.float32)
    lp[5] = -np.abs(lp[5])                      # a plane whose max is not positive: normalize leaves it
    D, H, W = shape
    f32 = np.float32
    exp = {
        P.PP_UPPER_THRESHOLD: lambda x, t: np.where(x > t, f32(t), x),
        P.PP_LOWER_THRESHOLD: lambda x, t: np.where(x < t, f32(t), x),
        P.PP_MINUS: lambda x, t: (x - f32(t)).astype(f32),
        P.PP_BINARIZE: lambda x, t: np.where(x > t, f32(1), f32(0)),
        P.PP_NORMALIZE: lambda x, t: (x / x.max()).astype(f32) if x.max() > 0 else x,
        P.PP_SMOOTH: lambda x, t: R._smooth(x),
    }
    for op, fn in exp.items():
        for t in (0.5, 0.25):
            d = torch.from_numpy(lp).to(DEV)
            scratch = torch.empty(P.postproc_scratch_bytes(7, lp[0].size), dtype=torch.uint8, device=DEV)
            P.plane_op_call(op, t, (W, H, D), d, 6, scratch)
            got = d.cpu().numpy()
            for p in range(6):
                assert np.array_equal(got[p], fn(lp[p], t)), (op, t, p)


# ---- end to end through EvaluateUNet -----------------------------------------------------------------------------------------
def restate(logits, chain="softmax+create_mask+argmax"):
    """the chain on one result's logits {C, D, H, W} (numpy fp32) by the restatement; returns the outputs and the comparable voxels"""
    C = logits.shape[0]
    elp, efg, elab, ok = ref_softmax(torch.from_numpy(logits).reshape(C, -1))
    return {"label_prob": elp, "fg_prob": efg, "label": elab}, ok


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("arch", ["smoke", "mix"])
@pytest.mark.parametrize("outputs", [("label",), ("fg_prob",), ("label_prob",), ("label", "fg_prob", "label_prob")])
def test_evaluate_with_the_model_chain(arch, dt, outputs):
    out_c = 5
    a = SMOKE_ARCH % out_c if arch == "smoke" else MIX_ARCH % (out_c, out_c)
    m = U.UNet3d(1, out_c, a, device=DEV, dtype=dt, seed=2)
    assert m.postproc == "softmax+create_mask+argmax"
    rs = np.random.RandomState(5)
    ios = [[rs.rand(32, 32, 32).astype(np.float32)], [rs.rand(16, 24, 32).astype(np.float32), rs.rand(32, 32, 32).astype(np.float32)]]
    raw = U.EvaluateUNet(m).start(ios)
    ev = U.EvaluateUNet(m, postproc="model", outputs=outputs)
    got = ev.start(ios)
    assert not ev.aborted and ev.error_msg == "" and ev.cur_prog == 2
    for rf, gf in zip(raw, got):
        for r, g in zip(rf, gf):
            d = r.shape[0] // out_c
            exp, ok = restate(r.reshape(out_c, d, r.shape[1], r.shape[2]))
            assert sorted(g) == sorted(outputs)
            if "label" in g:
                assert g["label"].dtype == np.uint16 and g["label"].shape == (d,) + r.shape[1:]
                assert_labels(torch.from_numpy(g["label"].astype(np.int32)), exp["label"], ok)
            if "fg_prob" in g:
                assert g["fg_prob"].dtype == np.float32 and g["fg_prob"].shape == (d,) + r.shape[1:]
                assert_probs(torch.from_numpy(g["fg_prob"]).reshape(-1), exp["fg_prob"])
            if "label_prob" in g:
                assert g["label_prob"].shape == ((out_c - 1) * d,) + r.shape[1:]
                assert_probs(torch.from_numpy(g["label_prob"]).reshape(out_c - 1, -1), exp["label_prob"])


def test_evaluate_chain_errors_and_empty_chain():
    m = U.UNet3d(1, 3, SMOKE_ARCH % 3, device=DEV, dtype="fp32", seed=1)
    ios = [[np.random.RandomState(0).rand(16, 16, 16).astype(np.float32)]]
    ev = U.EvaluateUNet(m, postproc="softmax+frobnicate")
    ev.start(ios)
    assert ev.aborted and ev.error_msg == "unknown command frobnicate" and ev.cur_prog == 0
    m.postproc = ""
    ev = U.EvaluateUNet(m, postproc="model")
    out = ev.start(ios)
    assert not ev.aborted and out[0][0].shape == (3 * 16, 16, 16) and out[0][0].dtype == np.float32
    # an output the chain does not produce ends the run the same way
    ev = U.EvaluateUNet(m, postproc="softmax+create_mask", outputs=("label",))
    ev.start(ios)
    assert ev.aborted and ev.error_msg == "output label is not produced by the chain (it needs argmax)"
    ev = U.EvaluateUNet(m, postproc="softmax+minus+argmax")
    ev.start(ios)
    assert ev.aborted and ev.error_msg == "argmax after minus needs create_mask before it"


# ---- longer chains: the restatement applied to the fused pass's own outputs ----------------------------------------------------
F32 = np.float32
PLANE_REF = {
    "upper_threshold": lambda x, t: np.where(x > t, F32(t), x),
    "lower_threshold": lambda x, t: np.where(x < t, F32(t), x),
    "minus": lambda x, t: (x - F32(t)).astype(F32),
    "binarize": lambda x, t: np.where(x > t, F32(1), F32(0)),
    "normalize_each": lambda x, t: (x / x.max()).astype(F32) if x.max() > 0 else x,
    "gaussian_smoothing": lambda x, t: R._smooth(x),
}


def restate_chain(logits, chain, params):
    """the leading softmax / create_mask / argmax group by the fused kernel (tested above against fp64), every later command by
    numpy.  Returns ({output: array}, number of voxels some defragment zeroed)"""
    steps = P.parse_chain(chain, params)
    k = 0
    while k < len(steps) and steps[k][0] in ("softmax", "create_mask", "argmax"):
        k += 1
    lead = dict(steps[:k])
    first = P.run_postproc(logits, "+".join(n for n, _ in steps[:k]), {"argmax": lead["argmax"]["threshold"]} if "argmax" in lead else None,
                           outputs=tuple(o for o, c in P.PRODUCER.items() if c in lead))
    st = {o: v.cpu().numpy() if v.dtype != torch.uint16 else v.cpu().to(torch.int32).numpy().astype(np.uint16) for o, v in first.items()}
    dropped = 0
    for name, p in steps[k:]:
        lp = st["label_prob"]
        if name == "defragment":
            m = st["fg_prob"] > p["threshold"]
            drop = m & ~kept_mask(m, p["size_ratio"])
            dropped += int(drop.sum())
            st["fg_prob"] = np.where(drop, F32(0), st["fg_prob"])
            st["label_prob"] = np.where(drop[None], F32(0), lp)
            if "label" in st:
                st["label"] = np.where(drop, np.uint16(0), st["label"])
        elif name == "defragment_each":
            for c in range(lp.shape[0]):
                m = lp[c] > p["threshold"]
                drop = m & ~kept_mask(m, p["size_ratio"])
                dropped += int(drop.sum())
                lp[c] = np.where(drop, F32(0), lp[c])
        elif name == "argmax":
            st["label"] = np.where(st["fg_prob"] > F32(p["threshold"]), 1 + np.argmax(lp, 0), 0).astype(np.uint16)
        else:
            t = next(iter(p.values())) if p else 0.0
            st["label_prob"] = np.stack([PLANE_REF[name](lp[c], t) for c in range(lp.shape[0])])
    return st, dropped


@pytest.mark.parametrize("chain,params", [
    ("softmax+create_mask+defragment+argmax", {"defragment": (0.8, 0.3), "argmax": 0.4}),
    ("softmax+create_mask+argmax+defragment", {"defragment": (0.8, 0.3)}),
    ("softmax+create_mask+upper_threshold+defragment_each+minus+normalize_each+gaussian_smoothing+lower_threshold+argmax",
     {"upper_threshold": 0.8, "defragment_each": (0.5, 0.3), "minus": 0.1, "lower_threshold": 0.05, "argmax": 0.3}),
    ("softmax+create_mask+binarize+defragment+argmax", {"binarize": 0.3, "defragment": (0.7, 0.5), "argmax": 0.5}),
])
def test_longer_chains_against_the_restatement(chain, params):
    g = torch.Generator().manual_seed(9)
    logits = (torch.randn(4, 12, 10, 14, generator=g) * 2).to(DEV)
    exp, dropped = restate_chain(logits, chain, params)
    assert dropped > 0                                   # the defragment commands did remove something
    got = P.run_postproc(logits, chain, params, outputs=("label_prob", "fg_prob", "label"))
    assert sorted(got) == sorted(exp)
    for o, v in got.items():
        g_ = v.cpu().to(torch.int32).numpy().astype(np.uint16) if v.dtype == torch.uint16 else v.cpu().numpy()
        assert np.array_equal(g_, exp[o]), o
    # label alone: the state argmax reads is still formed (label_prob / fg_prob made for it, not returned)
    only = P.run_postproc(logits, chain, params, outputs=("label",))
    assert sorted(only) == ["label"] and np.array_equal(only["label"].cpu().to(torch.int32).numpy(), exp["label"].astype(np.int32))


def test_evaluate_with_a_longer_chain_and_params():
    m = U.UNet3d(1, 4, SMOKE_ARCH % 4, device=DEV, dtype="fp32", seed=4)
    ios = [[np.random.RandomState(1).rand(16, 24, 32).astype(np.float32)]]
    raw = U.EvaluateUNet(m).start(ios)[0][0]
    chain, params = "softmax+create_mask+defragment+argmax", {"defragment": (0.55, 0.5), "argmax": 0.5}
    ev = U.EvaluateUNet(m, postproc=chain, params=params, outputs=("label", "fg_prob", "label_prob"))
    got = ev.start(ios)[0][0]
    assert not ev.aborted, ev.error_msg
    exp, _ = restate_chain(torch.from_numpy(raw).view(4, 16, 24, 32).to(DEV), chain, params)
    assert np.array_equal(got["label"], exp["label"]) and np.array_equal(got["fg_prob"], exp["fg_prob"])
    assert np.array_equal(got["label_prob"], exp["label_prob"].reshape(3 * 16, 24, 32))


def test_evaluate_state_carried_across_volumes():
    """One start() over entries of different sizes (a plain array, a NativeVolume on a smaller and one on a larger grid, the
    first array again) with a chain that needs scratch, single_component, morphology and mirroring: the scratch buffers, the
    filter-pack bookkeeping, the member stack and the result in flight carry nothing from one entry into the next, so every
    output equals, bit for bit, that of a fresh EvaluateUNet run on the entry alone."""
    m = U.UNet3d(1, 4, SMOKE_ARCH % 4, device=DEV, dtype="fp32", seed=2)
    m.dim, m.voxel_size = (16, 16, 16), (1.0, 1.0, 1.0)
    rs = np.random.RandomState(11)
    plain = rs.rand(16, 16, 16).astype(np.float32)
    small = U.NativeVolume(rs.rand(10, 14, 12).astype(np.float32), (1.3, 1.1, 1.4))
    large = U.NativeVolume(rs.rand(20, 18, 22).astype(np.float32), (0.8, 0.9, 0.75))
    kw = dict(postproc="softmax+create_mask+defragment+argmax", params={"defragment": (0.55, 0.5), "argmax": 0.0},
              outputs=("label", "fg_prob", "label_prob"), single_component=[1, 2], single_component_connectivity=18,
              morphology=[("close", 2, 26, 1)], mirror_axes="x")
    ev = U.EvaluateUNet(m, **kw)
    got = ev.start([[plain, small], [large, plain.copy()]])
    assert not ev.aborted and ev.error_msg == "" and ev.cur_prog == 2
    got = got[0] + got[1]
    for g, io in zip(got, (plain, small, large, plain)):
        alone = U.EvaluateUNet(m, **kw)
        exp = alone.start([[io]])[0][0]
        assert not alone.aborted, alone.error_msg
        shape = io.data.shape if isinstance(io, U.NativeVolume) else io.shape
        assert sorted(g) == sorted(exp) == sorted(kw["outputs"]) and g["label"].shape == shape
        for k in exp:
            assert g[k].dtype == exp[k].dtype and np.array_equal(g[k], exp[k]), k
    assert all(np.array_equal(got[3][k], got[0][k]) for k in got[0])
