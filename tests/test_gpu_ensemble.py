"""GPU: the model ensemble (include/unet_ensemble.h) on gfx950.

unet_ens_accumulate + unet_ens_finalize against the fp64 restatement of test_ensemble_host.py on the smallest shapes at which each
code path can go wrong (the scalar path, the vector path, unequal weights, more channels than the register cache holds); device
against device bit for bit where the definitions promise it (an ensemble of one and the fused softmax pass, the scalar and the
vector path, two runs, a state the first member must not read, outputs that are not wanted); special values; and
EvaluateUNet(ensemble=...) against the same composition written out by hand through the public functions, bit for bit.
Shapes are (C, D, H, W, M) in the tables and (D, H, W) in the arrays."""
import os
import sys

import numpy as np
import pytest
import torch

import unet_studio_amd as U
from unet_studio_amd import components as CMP
from unet_studio_amd import ensemble as EN
from unet_studio_amd import postproc as P

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_ensemble_host import ens_ref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F = np.float32
INF = float("inf")
GAP = 1e-5            # the tie rule of test_gpu_postproc.py
ALL = ("label_prob", "fg_prob", "label", "entropy", "mutual_info")
FLOATS = ("label_prob", "fg_prob", "entropy", "mutual_info")

# (C, D, H, W, M), the logits' scale, the weights
CASES = [((2, 5, 6, 7, 2), 3.0, None),                       # S % 4 != 0: the scalar path
         ((5, 12, 20, 36, 3), 4.0, None),                    # the vector path, more than one block
         ((6, 9, 10, 68, 5), 5.0, (1.0, 2.0, 0.5, 3.0, 1.5)),   # unequal weights
         ((300, 3, 4, 8, 2), 6.0, None)]                     # more channels than any register cache
IDS = ["scalar", "vector", "weights", "channels"]


def prob_tol(M):
    """the project's bound for one softmax (test_gpu_postproc.py: 2e-6) carried through a convex combination, plus one rounding
    per add"""
    return 2e-6 + M * 2.0 ** -24


# entropy and mutual_info against fp64: four times the largest error measured on the four CASES, rounded up to one digit (the
# margin is for other seeds).  Measured: 2.18e-6 and 2.29e-6, both on the 300-channel case, whose 300 terms are
# summed one after the other in fp32 as the definition says; the three cases of up to 6 channels stay at or below 3.3e-7 and 3.6e-7
ENT_TOL = 9e-6
MI_TOL = 1e-5

_cache = {}


def case(i):
    """the members, the fp64 reference and the device's outputs of CASES[i], made once"""
    if i not in _cache:
        (C, D, H, W, M), scale, weights = CASES[i]
        rs = np.random.RandomState(100 + i)
        members = [(scale * rs.randn(C, D, H, W)).astype(F) for _ in range(M)]
        ref = ens_ref(members, weights)
        got = np_of(EN.combine([dev(x) for x in members], weights, outputs=ALL))
        _cache[i] = (members, weights, ref, got)
    return _cache[i]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def np_of(res):
    return {k: v.cpu().numpy() for k, v in res.items()}


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def offset(t):
    """a copy of t that starts one float (4 bytes) after a 16-byte boundary: forces the scalar path"""
    flat = t.reshape(-1)
    buf = torch.empty(flat.numel() + 1, dtype=t.dtype, device=t.device)
    assert buf.data_ptr() % 16 == 0
    view = buf[1:]
    view.copy_(flat)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    return view.view(t.shape)


# ---- 1: against the fp64 restatement ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_against_the_fp64_restatement(i):
    members, weights, ref, got = case(i)
    (C, D, H, W, M), _, _ = CASES[i]
    assert got["label_prob"].shape == (C - 1, D, H, W) and got["label"].dtype == np.uint16 and got["label"].shape == (D, H, W)
    errs = {k: float(np.abs(got[k].astype(np.float64) - ref[k]).max()) for k in FLOATS}
    print("ensemble %s: max |device - fp64| %s" % (IDS[i], ", ".join("%s %.3g" % kv for kv in errs.items())))
    assert not any(np.isnan(got[k]).any() for k in FLOATS)
    assert errs["label_prob"] <= prob_tol(M) and errs["fg_prob"] <= prob_tol(M)
    assert errs["entropy"] <= ENT_TOL
    assert errs["mutual_info"] <= MI_TOL
    assert float(got["entropy"].min()) >= 0 and float(got["entropy"].max()) <= np.log(C) + ENT_TOL and float(got["mutual_info"].min()) >= 0
    # the label where the fp64 answer is not a near tie
    fg = ref["label_prob"]
    ok = np.abs(ref["fg_prob"] - 0.5) >= GAP
    if C > 2:
        top = np.sort(fg, axis=0)[-2:]
        ok &= ((top[1] - top[0]) >= GAP) | (top[1] == top[0])
    assert ok.mean() >= 0.999
    assert np.array_equal(got["label"][ok].astype(np.int64), ref["label"][ok])
    assert got["label"].max() <= C - 1


# ---- 2: bit for bit, device against device ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_an_ensemble_of_one_equals_the_fused_softmax_pass(i):
    x = dev(case(i)[0][0])
    C, D, H, W = x.shape
    lp = torch.empty((C - 1, D, H, W), dtype=torch.float32, device=DEV)
    fg = torch.empty((D, H, W), dtype=torch.float32, device=DEV)
    P.softmax_call(x, C, D * H * W, 0.5, lp, fg, None)
    got = EN.combine([x], outputs=ALL)
    assert same(got["label_prob"].cpu().numpy(), lp.cpu().numpy()) and same(got["fg_prob"].cpu().numpy(), fg.cpu().numpy())
    assert float(got["mutual_info"].max()) <= MI_TOL               # entropy - H_0: two roads to one number
    x2 = offset(x)                                                 # ... and on the scalar path
    P.softmax_call(x2, C, D * H * W, 0.5, lp, fg, None)
    got2 = EN.combine([x2], outputs=("label_prob", "fg_prob"))
    assert same(got2["label_prob"].cpu().numpy(), lp.cpu().numpy()) and same(got2["fg_prob"].cpu().numpy(), fg.cpu().numpy())


def run(members, weights, state, outputs=ALL, out=None):
    ws = EN.normalize_weights(weights, len(members))
    for k, (x, w) in enumerate(zip(members, ws)):
        EN.accumulate(x, state, w, k == 0)
    C, D, H, W = members[0].shape
    return np_of(EN.finalize(state, C, (D, H, W), 0.5, outputs, out=out))


@pytest.mark.parametrize("i", [1, 2, 3], ids=IDS[1:])
def test_scalar_and_vector_paths_two_runs_and_a_dirty_state_give_the_same_bits(i):
    members, weights, _, got = case(i)
    C, D, H, W = members[0].shape
    assert (D * H * W) % 4 == 0
    xs = [dev(x) for x in members]
    nbytes = EN.state_bytes(C, D * H * W)
    zero = torch.zeros(nbytes, dtype=torch.uint8, device=DEV)
    again = run(xs, weights, zero)                                 # a second run, on a zeroed state
    dirty = torch.full((nbytes // 4,), float("nan"), dtype=torch.float32, device=DEV)
    nan = run(xs, weights, dirty)                                  # the first member never reads the state
    scalar_state = offset(torch.full((nbytes // 4,), float("nan"), dtype=torch.float32, device=DEV))
    scalar = run([offset(x) for x in xs], weights, scalar_state)   # every pointer 4 bytes past a 16-byte boundary
    for k in ALL:
        assert same(again[k], got[k]), k
        assert same(nan[k], got[k]), k
        assert same(scalar[k], got[k]), k


def test_an_output_that_is_not_wanted_is_not_written():
    members, weights, _, got = case(1)
    C, D, H, W = members[0].shape
    S = D * H * W
    state = EN.new_state(C, S, DEV)
    xs = [dev(x) for x in members]
    guard = 64
    sizes = {"label_prob": (C - 1) * S, "fg_prob": S, "entropy": S, "mutual_info": S}
    for wanted in [(k,) for k in ALL] + [("label", "entropy"), ("fg_prob", "mutual_info"), ALL]:
        arena = torch.full((sum(sizes.values()) + 5 * guard,), 7.0, dtype=torch.float32, device=DEV)
        lab = torch.full((S + 2 * guard,), 7, dtype=torch.int16, device=DEV)      # handed in as uint16, looked at as int16
        views, at = {}, guard
        for k, n in sizes.items():
            views[k] = arena[at:at + n]
            at += n + guard
        views["label"] = lab[guard:guard + S]
        out = {k: views[k].view(torch.uint16) if k == "label" else views[k] for k in wanted}
        res = run(xs, weights, state, wanted, out=out)
        assert sorted(res) == sorted(wanted)
        for k in wanted:
            assert same(res[k].reshape(got[k].shape), got[k]), (wanted, k)
        for k in ALL:                                              # the rest, and every guard, still hold the sentinel
            if k not in wanted:
                assert bool((views[k] == 7).all()), (wanted, k)
            views[k].fill_(7)
        assert bool((arena == 7).all()) and bool((lab == 7).all()), wanted


# ---- 3: special values -----------------------------------------------------------------------------------------------------------
def test_special_values():
    rs = np.random.RandomState(9)
    members = [(4 * rs.randn(3, 2, 3, 8)).astype(F) for _ in range(3)]
    members[1][1, 0, 0, 1] = np.nan                                # a NaN logit in one member of three
    members[0][2, 0, 1, 2] = -INF                                  # a -inf channel
    members[2][0, 1, 0, 3] = -INF
    members[2][:, 1, 2, 5] = -INF                                  # every channel -inf
    members[0][1, 1, 1, 6] = INF                                   # +inf
    members[1][:, 0, 2, 4] = 2.5                                   # a tie over all channels in one member
    ref = ens_ref(members)
    for xs in ([dev(x) for x in members], [offset(dev(x)) for x in members]):
        got = np_of(EN.combine(xs, outputs=ALL))
        for at in ((0, 0, 1), (1, 2, 5), (1, 1, 6)):
            for k in ("fg_prob", "entropy", "mutual_info"):
                assert np.isnan(got[k][at]), (k, at)
            assert np.isnan(got["label_prob"][(slice(None),) + at]).all() and got["label"][at] == 0
        for at in ((0, 1, 2), (1, 0, 3), (0, 2, 4)):
            assert np.isfinite(got["entropy"][at]) and np.isfinite(got["mutual_info"][at]) and np.isfinite(got["label_prob"][(slice(None),) + at]).all()
        for k in FLOATS:
            assert np.array_equal(np.isnan(got[k]), np.isnan(ref[k])), k
            fin = ~np.isnan(ref[k])
            assert np.abs(got[k][fin] - ref[k][fin]).max() <= {"entropy": ENT_TOL, "mutual_info": MI_TOL}.get(k, prob_tol(3)), k
        assert int(np.isnan(ref["entropy"]).sum()) == 3
    # one member with a -inf channel: p = (1/2, 0, 1/2) exactly, entropy ln 2, mutual information 0
    one = np.zeros((3, 1, 1, 4), F)
    one[1] = -INF
    got = np_of(EN.combine([dev(one)], outputs=ALL))
    assert np.array_equal(got["label_prob"][:, 0, 0, 0], (0.0, 0.5)) and abs(float(got["entropy"][0, 0, 0]) - np.log(2)) <= ENT_TOL
    assert (got["label"] == 0).all() and float(got["mutual_info"].max()) <= MI_TOL   # fg_prob is exactly the threshold


@pytest.mark.parametrize("M", [2, 3, 5])
def test_copies_of_one_member_change_nothing_and_share_no_information(M):
    x = dev(case(2)[0][0])
    one = np_of(EN.combine([x], outputs=ALL))
    many = np_of(EN.combine([x] * M, outputs=ALL))
    assert np.abs(many["label_prob"].astype(np.float64) - one["label_prob"]).max() <= M * 2.0 ** -24
    assert np.abs(many["fg_prob"].astype(np.float64) - one["fg_prob"]).max() <= M * 2.0 ** -24
    assert float(many["mutual_info"].max()) <= MI_TOL and float(many["mutual_info"].min()) >= 0


# ---- 4: EvaluateUNet -------------------------------------------------------------------------------------------------------------
SMOKE_ARCH = ("conv8,ks3,stride1+norm,leaky_relu+conv8,ks3,stride1+norm,leaky_relu\n"
              "conv16,ks3,stride2+norm,leaky_relu+conv16,ks3,stride1+norm,leaky_relu+conv_trans8,ks2,stride2\n"
              "conv8,ks3,stride1+norm,leaky_relu+conv8,ks3,stride1+norm,leaky_relu+conv3,ks1,stride1")
OUT_C = 3
CHAIN = "softmax+create_mask+argmax"
WANTED = ("label", "label_prob", "entropy", "mutual_info")
_models = []


def models():
    """the three-line 16^3 network of smoke() with 3 classes, seeds 0, 1, 2"""
    if not _models:
        for seed in (0, 1, 2):
            m = U.UNet3d(1, OUT_C, SMOKE_ARCH, device=DEV, dtype="fp32", seed=seed)
            m.dim, m.voxel_size = (16, 16, 16), (1.0, 1.0, 1.0)
            _models.append(m)
    return _models


def started(ev, ios):
    got = ev.start([ios])[0]
    assert not ev.aborted and ev.error_msg == "", ev.error_msg
    return got


def shape_of(io):
    return tuple((io.data if isinstance(io, U.NativeVolume) else io).shape)


def by_hand(io, weights=None, outputs=WANTED, chain=CHAIN, ms=None, **kw):
    """forward each model (a plain one-model run without a chain: the logits on the entry's own grid), accumulate, then run_postproc
    on the state; also returns finalize's own outputs"""
    ms = ms or models()
    shape = shape_of(io)
    ws = EN.normalize_weights(weights, len(ms))
    state = EN.new_state(OUT_C, int(np.prod(shape)), DEV)
    run_kw = {k: kw.pop(k) for k in ("single_component",) if k in kw}
    for k, (m, w) in enumerate(zip(ms, ws)):
        logits = started(U.EvaluateUNet(m, **kw), [io])[0]
        assert logits.shape == (OUT_C * shape[0],) + shape[1:]
        EN.accumulate(dev(logits.reshape((OUT_C,) + shape)), state, w, k == 0)
    fin = np_of(EN.finalize(state, OUT_C, shape, 0.5, outputs))
    return np_of(P.run_postproc(None, chain, outputs=outputs, ensemble=(state, OUT_C, shape), **run_kw)), fin


def check_equal(got, exp, shape):
    assert sorted(got) == sorted(exp)
    for k in exp:
        assert got[k].tobytes() == exp[k].tobytes(), k
    assert got["label"].dtype == np.uint16 and got["label"].shape == shape
    assert got["label_prob"].shape == ((OUT_C - 1) * shape[0],) + shape[1:]
    for k in ("entropy", "mutual_info"):
        assert got[k].dtype == F and got[k].shape == shape and np.isfinite(got[k]).all() and got[k].min() >= 0
    assert got["entropy"].max() <= np.log(OUT_C) + ENT_TOL and got["mutual_info"].max() > 0


def test_a_plain_array_equals_the_composition_by_hand():
    ms = models()
    vols = [np.random.RandomState(5 + i).rand(16, 16, 16).astype(F) for i in range(2)]
    ev = U.EvaluateUNet(ms[0], postproc=CHAIN, outputs=WANTED, ensemble=ms[1:])
    got = started(ev, vols)                                        # the state is reused across volumes
    for vol, g in zip(vols, got):
        exp, fin = by_hand(vol)
        check_equal(g, exp, (16, 16, 16))
        for k in WANTED:
            assert fin[k].tobytes() == exp[k].tobytes(), k         # the chain's leading group IS finalize
    # weights, and a chain that goes on after the leading group and ends in an argmax of the changed planes
    w = (2.0, 1.0, 0.5)
    for chain in (CHAIN, "softmax+create_mask+defragment+argmax", CHAIN + "+defragment_each+argmax"):
        ev = U.EvaluateUNet(ms[0], postproc=chain, outputs=WANTED, ensemble=ms[1:], ensemble_weights=w)
        check_equal(started(ev, [vols[0]])[0], by_hand(vols[0], weights=w, chain=chain)[0], (16, 16, 16))
    assert not same(started(ev, [vols[0]])[0]["label_prob"], got[0]["label_prob"])      # the weights matter


def test_a_native_volume_equals_the_composition_by_hand():
    ms = models()
    data = np.random.RandomState(7).rand(14, 13, 18).astype(F)
    nv = U.NativeVolume(data, (0.9, 1.2, 1.1))
    got = started(U.EvaluateUNet(ms[0], postproc=CHAIN, outputs=WANTED, ensemble=ms[1:]), [nv])[0]
    check_equal(got, by_hand(nv)[0], data.shape)


def test_tiles_equal_the_composition_by_hand():
    ms = models()
    io = np.random.RandomState(8).rand(24, 24, 24).astype(F)
    got = started(U.EvaluateUNet(ms[0], postproc=CHAIN, outputs=WANTED, ensemble=ms[1:], fov_strategy="tiles"), [io])[0]
    check_equal(got, by_hand(io, fov_strategy="tiles")[0], (24, 24, 24))


def test_mirroring_equals_the_composition_by_hand():
    ms = models()
    vol = np.random.RandomState(9).rand(16, 16, 16).astype(F)
    got = started(U.EvaluateUNet(ms[0], postproc=CHAIN, outputs=WANTED, ensemble=ms[1:], mirror_axes="x"), [vol])[0]
    check_equal(got, by_hand(vol, mirror_axes="x")[0], (16, 16, 16))
    plain = started(U.EvaluateUNet(ms[0], postproc=CHAIN, outputs=WANTED, ensemble=ms[1:]), [vol])[0]
    assert not same(plain["label_prob"], got["label_prob"])


def test_entropy_alone_runs_one_member_and_keeps_todays_probabilities():
    m = models()[0]
    vol = np.random.RandomState(10).rand(16, 16, 16).astype(F)
    today = started(U.EvaluateUNet(m, postproc=CHAIN, outputs=("label", "label_prob", "fg_prob")), [vol])[0]
    for kw in (dict(ensemble=[]), dict()):
        got = started(U.EvaluateUNet(m, postproc=CHAIN, outputs=("label", "label_prob", "fg_prob", "entropy"), **kw), [vol])[0]
        assert sorted(got) == ["entropy", "fg_prob", "label", "label_prob"]
        assert same(got["label_prob"], today["label_prob"]) and same(got["fg_prob"], today["fg_prob"])
        assert got["entropy"].shape == (16, 16, 16) and got["entropy"].min() >= 0 and got["entropy"].max() <= np.log(3) + ENT_TOL
    only = started(U.EvaluateUNet(m, postproc=CHAIN, outputs=("entropy",)), [vol])[0]
    assert sorted(only) == ["entropy"] and same(only["entropy"], got["entropy"])


def test_single_component_still_acts_on_the_ensembles_label():
    ms = models()
    vol = np.random.RandomState(11).rand(16, 16, 16).astype(F)
    plain = started(U.EvaluateUNet(ms[0], postproc=CHAIN, outputs=WANTED, ensemble=ms[1:]), [vol])[0]
    ms[0].single_component_label = [1, 2]
    try:
        got = started(U.EvaluateUNet(ms[0], postproc=CHAIN, outputs=WANTED, ensemble=ms[1:], single_component="model"), [vol])[0]
    finally:
        ms[0].single_component_label = []
    exp = by_hand(vol, single_component=[1, 2])[0]
    check_equal(got, exp, (16, 16, 16))
    kept = dev(plain["label"].copy())
    CMP.keep_largest(kept, [1, 2], OUT_C)
    assert same(got["label"], kept.cpu().numpy())
    for k in ("label_prob", "entropy", "mutual_info"):
        assert same(got[k], plain[k]), k                           # it acts on the label alone
    assert ((got["label"] == plain["label"]) | (got["label"] == 0)).all()


def test_refusals_end_the_run_without_a_forward(monkeypatch):
    ms = models()
    vol = np.random.RandomState(12).rand(16, 16, 16).astype(F)
    other = U.UNet3d(1, 4, SMOKE_ARCH.replace("conv3,ks1", "conv4,ks1"), device=DEV, dtype="fp32", seed=3)
    other.dim, other.voxel_size = (16, 16, 16), (1.0, 1.0, 1.0)

    def refuse(*a, **k):
        raise AssertionError("a forward after a refusal")
    for m in ms + [other]:
        monkeypatch.setattr(m, "forward", refuse)
    for kw, word in ((dict(ensemble=[ms[1], other], postproc=CHAIN), "ensemble: member 2 has out_count 4, member 0 has 3"),
                     (dict(ensemble=ms[1:], postproc=CHAIN, ensemble_weights=(1, 2)), "2 weights for 3 members"),
                     (dict(postproc=CHAIN, outputs=("mutual_info",)), "mutual_info needs more than one member"),
                     (dict(ensemble=ms[1:], postproc=CHAIN, outputs=("label", "agreement"), mirror_axes="x"), "agreement is not available with ensemble"),
                     (dict(ensemble=ms[1:], outputs=("entropy",)), "output entropy needs a postproc chain"),
                     (dict(ensemble=ms[1:], postproc=CHAIN + "+defragment+softmax", outputs=("label_prob",)), "softmax may not recur after defragment")):
        ev = U.EvaluateUNet(ms[0], **kw)
        out = ev.start([[vol]])
        assert ev.aborted and word in ev.error_msg and not ev.running and ev.cur_prog == 0, (kw, ev.error_msg)
        assert out[0][0] is vol
