"""CPU: the host half of the model ensemble (include/unet_ensemble.h, unet-studio_amd/ensemble.py) -- a plain-numpy fp64
restatement of the header's definitions (`ens_ref`, which imports nothing of the package and which the GPU tests compare the kernels
with) checked on hand-written answers, the weights' and the normalised entropy's arithmetic, the ABI the library exports, argument
errors found before any device call, and the new refusals of run_postproc and EvaluateUNet.  No device calls.  Shapes are (D, H, W)."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import unet_studio_amd as U
from unet_studio_amd import ensemble as EN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
INF = float("inf")
LN = math.log
FORBIDDEN = ("unet_inst_", "unet_dist_", "unet_table_", "unet_reg_", "unet_atlas_", "unet_components_", "unet_preproc_", "unet_tiles_",
             "unet_space_", "unet_postproc_", "unet_qc_", "unet_feed_", "unet_morph_", "unet_conn_", "unet_mirror_", "unet_stats_")


# ---- the fp64 restatement --------------------------------------------------------------------------------------------------------
def ens_ref(members, weights=None, threshold=0.5):
    """include/unet_ensemble.h in float64 numpy.  members: a list of M arrays {C, ...}; weights: M positive numbers or None.  The
    weights are normalised in double and rounded to fp32, as the host passes them.  Returns a dict of float64 arrays: q {C + 2, ...}
    (the state), label_prob, fg_prob, entropy, mutual_info, and label int64."""
    M = len(members)
    ws = np.full(M, 1.0 / M) if weights is None else np.asarray(weights, np.float64) / math.fsum(float(w) for w in weights)
    ws = ws.astype(np.float32).astype(np.float64)
    state = None
    with np.errstate(all="ignore"):
        for x, w in zip(members, ws):
            x = np.asarray(x, np.float64)
            bad = np.isnan(x).any(0) | (x == INF).any(0) | (x == -INF).all(0)
            m = np.where(bad, 0.0, x.max(0))
            d = x - m
            e = np.exp(d)
            s = e.sum(0)
            sf = e[1:].sum(0)
            p = e / s
            fg = sf / s
            ed = np.where(x == -INF, 0.0, e * d).sum(0)              # such a channel contributes 0
            h = np.log(s) - ed / s
            planes = np.concatenate([p, fg[None], h[None]])
            planes[:, bad] = np.nan
            state = w * planes if state is None else state + w * planes
        C = members[0].shape[0]
        q = state[:C]
        fg = state[C]
        best = np.zeros(q.shape[1:], np.int64)
        bv = q[1].copy()
        for c in range(2, C):                                        # the first index wins a tie; NaN compares false
            win = q[c] > bv
            best[win] = c - 1
            bv[win] = q[c][win]
        label = np.where(fg > threshold, best + 1, 0)
        terms = np.where(q == 0, 0.0, q * np.log(q))
        entropy = -terms.sum(0)
        t = entropy - state[C + 1]
        mi = np.where(t < 0, 0.0, t)
    return dict(q=state, label_prob=q[1:], fg_prob=fg, label=label, entropy=entropy, mutual_info=mi)


def col(*v):
    """one voxel's logits {C, 1}"""
    return np.array(v, np.float64).reshape(-1, 1)


def test_restatement_two_members_by_hand():
    r = ens_ref([col(0, 0), col(LN(3), 0)])
    assert np.allclose(r["q"][:2, 0], (0.625, 0.375), rtol=0, atol=1e-15)
    ent = -(0.625 * LN(0.625) + 0.375 * LN(0.375))
    h1, h2 = LN(2), -(0.75 * LN(0.75) + 0.25 * LN(0.25))
    assert abs(r["entropy"][0] - ent) < 1e-15 and abs(r["q"][3, 0] - (h1 + h2) / 2) < 1e-15
    assert abs(r["mutual_info"][0] - (ent - (h1 + h2) / 2)) < 1e-15 and r["mutual_info"][0] > 0.03
    assert abs(r["fg_prob"][0] - 0.375) < 1e-15 and abs(r["label_prob"][0, 0] - 0.375) < 1e-15
    assert r["label"][0] == 0 and ens_ref([col(0, 0), col(LN(3), 0)], threshold=0.3)["label"][0] == 1
    # weights 3 : 1 (0.75 and 0.25 are exact in fp32)
    r = ens_ref([col(0, 0), col(LN(3), 0)], weights=(3, 1))
    assert abs(r["q"][0, 0] - (0.75 * 0.5 + 0.25 * 0.75)) < 1e-15 and abs(r["q"][3, 0] - (0.75 * h1 + 0.25 * h2)) < 1e-15


def test_restatement_identical_members_have_no_mutual_information():
    x = np.random.RandomState(0).randn(4, 50) * 4
    one = ens_ref([x])
    many = ens_ref([x, x, x, x])                                     # weights 1/4: exact
    assert np.abs(many["mutual_info"]).max() < 1e-14 and np.abs(one["mutual_info"]).max() < 1e-14
    assert np.abs(many["q"] - one["q"]).max() < 1e-15
    p = np.exp(x - x.max(0)) / np.exp(x - x.max(0)).sum(0)
    assert np.abs(one["entropy"] + (p * np.log(p)).sum(0)).max() < 1e-13          # H_m is -sum p ln p
    assert (one["label"][one["fg_prob"] > 0.5] == 1 + x[1:].argmax(0)[one["fg_prob"] > 0.5]).all()
    # members that disagree completely: MI = ln 2, the members' own entropy ~ 0
    r = ens_ref([col(40, 0), col(0, 40)])
    assert abs(r["entropy"][0] - LN(2)) < 1e-12 and abs(r["mutual_info"][0] - LN(2)) < 1e-12
    # members that are each unsure, and agree: entropy ln 2, MI 0
    r = ens_ref([col(1, 1), col(-2, -2)])
    assert abs(r["entropy"][0] - LN(2)) < 1e-15 and r["mutual_info"][0] < 1e-15


def test_restatement_special_values():
    r = ens_ref([col(0, -INF, 0)])                                   # a -inf channel contributes 0: p = (1/2, 0, 1/2)
    assert np.array_equal(r["q"][:3, 0], (0.5, 0.0, 0.5)) and abs(r["entropy"][0] - LN(2)) < 1e-15 and r["mutual_info"][0] == 0
    assert abs(r["q"][4, 0] - LN(2)) < 1e-15
    for bad in (col(0, np.nan, 1), col(0, INF, 1), col(-INF, -INF, -INF)):
        r = ens_ref([col(1, 2, 3), bad, col(0, 0, 0)])              # one bad member of three: NaN everywhere, label 0
        for k in ("label_prob", "fg_prob", "entropy", "mutual_info", "q"):
            assert np.isnan(r[k]).all(), k
        assert r["label"][0] == 0
    r = ens_ref([col(0, 5, 5)])                                      # a tie: the first foreground class
    assert r["label"][0] == 1


# ---- host arithmetic -------------------------------------------------------------------------------------------------------------
def test_normalize_weights():
    assert EN.normalize_weights(None, 1) == [1.0] and EN.normalize_weights(None, 4) == [0.25] * 4
    assert EN.normalize_weights(None, 3) == [1.0 / 3] * 3
    assert EN.normalize_weights([7.5], 1) == [1.0]                   # M = 1 gives exactly 1
    assert EN.normalize_weights((3, 1), 2) == [0.75, 0.25]
    ws = EN.normalize_weights([0.1, 0.2, 0.3, 0.7], 4)
    assert abs(sum(ws) - 1.0) < 1e-15 and ws == [w / math.fsum([0.1, 0.2, 0.3, 0.7]) for w in (0.1, 0.2, 0.3, 0.7)]
    assert all(0 < np.float32(w) <= 1 for w in ws)
    for bad, n, word in (([1, 2], 3, "2 weights for 3 members"), ([1, 2, 3], 2, "3 weights for 2 members"),
                         ([1, 0], 2, "finite and positive"), ([1, -1], 2, "finite and positive"),
                         ([1, float("nan")], 2, "finite and positive"), ([1, INF], 2, "finite and positive"),
                         ([1e308, 1e308], 2, "sum is not finite"), ("ab", 2, "list of numbers"), (5, 1, "list of numbers"),
                         (None, 0, "at least one member")):
        with pytest.raises(U.UNetError, match=word):
            EN.normalize_weights(bad, n)


def test_normalized_entropy():
    assert EN.normalized_entropy(LN(6), 6) == 1.0 and EN.normalized_entropy(0.0, 2) == 0.0
    h = np.array([0.0, LN(2), LN(3)], F)
    assert np.allclose(EN.normalized_entropy(h, 3), h / LN(3), rtol=0, atol=0)
    with pytest.raises(U.UNetError, match="at least 2"):
        EN.normalized_entropy(h, 1)


# ---- the ABI ---------------------------------------------------------------------------------------------------------------------
def test_unet_ensemble_h_declares_exactly_the_exports_and_the_library_has_them():
    lib = ctypes.CDLL(U.engine.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "unet_ensemble.h")).read()
    declared = set(re.findall(r"\b(unet_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(EN.EXPORTS) == {"unet_ens_state_bytes", "unet_ens_accumulate", "unet_ens_finalize"}
    for name in sorted(declared):
        assert hasattr(lib, name), "libunet_hip.so does not export " + name
    assert "this project's" in hdr and "NOT pinned" in hdr
    assert U.ensemble is EN and EN.OUTPUTS == ("label_prob", "fg_prob", "label", "entropy", "mutual_info")


def test_the_new_prefix_stays_in_its_header():
    for h in sorted(os.listdir(os.path.join(ROOT, "include"))):
        text = open(os.path.join(ROOT, "include", h)).read().lower()
        if h != "unet_ensemble.h":
            assert "unet_ens_" not in text, h
        else:                                                      # what the other host tests forbid
            for other in FORBIDDEN:
                assert other not in text, other


# ---- argument errors, before any device call -------------------------------------------------------------------------------------
P = [ctypes.c_void_p(0x1000 * (i + 1)) for i in range(7)]          # never dereferenced
BIG = 1 << 40


def failing(f, *args):
    assert f(*args) != 0
    return U.engine.lib.unet_last_error().decode()


def acc_args(logits=P[0], c=3, voxels=100, weight=0.5, first=1, state=P[1], nbytes=BIG):
    return (logits, c, voxels, weight, first, state, nbytes, None)


def fin_args(state=P[1], nbytes=BIG, c=3, voxels=100, outs=(P[2], P[3], P[4], P[5], P[6])):
    return (state, nbytes, c, voxels, 0.5) + tuple(outs) + (None,)


SIZES = [(dict(c=1), "out_c must be at least 2"), (dict(c=0), "out_c must be at least 2"), (dict(c=65537), "65535 foreground classes"),
         (dict(voxels=0), "voxels must be positive"), (dict(voxels=-5), "voxels must be positive"),
         (dict(voxels=1 << 31), "below 2^31 voxels")]


@pytest.mark.parametrize("kw,msg", SIZES)
def test_abi_size_errors_come_before_any_device_call(kw, msg):
    lib = U.engine.lib
    n = ctypes.c_size_t()
    m = failing(lib.unet_ens_state_bytes, kw.get("c", 3), kw.get("voxels", 100), ctypes.byref(n))
    assert msg in m and m.startswith("unet_ens_state_bytes: ")
    m = failing(lib.unet_ens_accumulate, *acc_args(**kw))
    assert msg in m and m.startswith("unet_ens_accumulate: ")
    m = failing(lib.unet_ens_finalize, *fin_args(**kw))
    assert msg in m and m.startswith("unet_ens_finalize: ")


def test_abi_pointer_weight_state_and_output_errors():
    lib = U.engine.lib
    assert "null output" in failing(lib.unet_ens_state_bytes, 3, 100, None)
    assert "null logits" in failing(lib.unet_ens_accumulate, *acc_args(logits=None))
    assert "null state" in failing(lib.unet_ens_accumulate, *acc_args(state=None))
    assert "null state" in failing(lib.unet_ens_finalize, *fin_args(state=None))
    for w in (0.0, -0.25, 1.0000001, 2.0, float("nan"), INF, -INF):
        assert "weight must be finite and in (0, 1]" in failing(lib.unet_ens_accumulate, *acc_args(weight=w)), w
    need = EN.state_bytes(3, 100)
    assert need == 5 * 100 * 4
    assert "state too small" in failing(lib.unet_ens_accumulate, *acc_args(nbytes=need - 1))
    assert "state too small" in failing(lib.unet_ens_finalize, *fin_args(nbytes=need - 1))
    assert "no output wanted" in failing(lib.unet_ens_finalize, *fin_args(outs=(None,) * 5))
    assert "4-byte aligned" in failing(lib.unet_ens_accumulate, *acc_args(logits=ctypes.c_void_p(0x1002)))
    with pytest.raises(U.UNetError, match="out_c must be at least 2"):
        EN.state_bytes(1, 10)


def test_state_bytes_is_monotone_in_both_arguments():
    assert EN.state_bytes(2, 1) == 16 and EN.state_bytes(6, 128 ** 3) == 8 * 128 ** 3 * 4 == 67108864
    assert EN.state_bytes(65536, (1 << 31) - 1) == 65538 * ((1 << 31) - 1) * 4        # no 32-bit overflow
    cs, vs = (2, 3, 6, 300, 65536), (1, 7, 210, 8640, 128 ** 3, (1 << 31) - 1)
    for v in vs:
        row = [EN.state_bytes(c, v) for c in cs]
        assert all(a < b for a, b in zip(row, row[1:]))
    for c in cs:
        row = [EN.state_bytes(c, v) for v in vs]
        assert all(a < b for a, b in zip(row, row[1:]))


def test_python_calls_name_the_bad_argument_before_any_device_work():
    host = np.zeros((3, 2, 2, 2), F)
    with pytest.raises(U.UNetError, match="logits must be a contiguous float32 device tensor"):
        EN.accumulate(host, None, 0.5, True)
    with pytest.raises(U.UNetError, match="state must be a contiguous device tensor"):
        EN.finalize(host, 3, (2, 2, 2))
    with pytest.raises(U.UNetError, match="unknown output"):
        EN.finalize(None, 3, (2, 2, 2), outputs=("agreement",))
    with pytest.raises(U.UNetError, match="no output wanted"):
        EN.finalize(None, 3, (2, 2, 2), outputs=())
    with pytest.raises(U.UNetError, match="2 weights for 1 members"):
        EN.combine([host], weights=[1, 2])


# ---- run_postproc's refusals -----------------------------------------------------------------------------------------------------
def test_run_postproc_refusals():
    import torch
    CH = "softmax+create_mask+argmax"
    host = torch.zeros(5 * 8, dtype=torch.float32)                   # not a device tensor: refused last, after everything else
    ens = (host, 3, (2, 2, 2))
    for out in ("entropy", "mutual_info"):
        with pytest.raises(U.UNetError, match="output %s needs ensemble" % out):
            U.run_postproc(None, CH, outputs=("label", out))
    with pytest.raises(U.UNetError, match="agreement is not available with ensemble"):
        U.run_postproc(None, CH, outputs=("label", "agreement"), ensemble=ens)
    with pytest.raises(U.UNetError, match="agreement needs mirror"):  # as before
        U.run_postproc(None, CH, outputs=("label", "agreement"))
    for kw in (dict(native=(None, (2, 2, 2))), dict(tiles=(host, None, (2, 2, 2))), dict(mirror=(host, [0], None))):
        with pytest.raises(U.UNetError, match="ensemble comes in place of logits and does not combine with native, tiles or mirror"):
            U.run_postproc(None, CH, ensemble=ens, **kw)
    with pytest.raises(U.UNetError, match="ensemble comes in place of logits"):
        U.run_postproc(host, CH, ensemble=ens)
    with pytest.raises(U.UNetError, match=r"ensemble must be \(state, out_c, \(d, h, w\)\)"):
        U.run_postproc(None, CH, ensemble=host)
    # the logits themselves: softmax after a command that changed the state; an empty chain
    for chain, after in (("softmax+create_mask+argmax+defragment+softmax", "defragment"), ("softmax+create_mask+minus+softmax+argmax", "minus"),
                         ("softmax+create_mask+defragment_each+softmax+argmax", "defragment_each")):
        with pytest.raises(U.UNetError, match="softmax may not recur after %s" % after):
            U.run_postproc(None, chain, outputs=("label_prob",), ensemble=ens)
    with pytest.raises(U.UNetError, match="must start with its softmax / create_mask / argmax group"):
        U.run_postproc(None, "", outputs=(), ensemble=ens)
    with pytest.raises(U.UNetError, match="needs softmax before it"):  # check_chain's own rule comes first
        U.run_postproc(None, "minus+softmax", outputs=("label_prob",), ensemble=ens)
    # a later lone argmax is fine for the chain rules: the call only stops at the state, which is no device tensor here
    for chain in (CH, "softmax+create_mask+defragment+argmax", "softmax+create_mask+argmax+defragment_each+argmax"):
        with pytest.raises(U.UNetError, match="state must be a contiguous device tensor"):
            U.run_postproc(None, chain, outputs=("label", "entropy"), ensemble=ens)
    with pytest.raises(U.UNetError, match="out_c must be at least 2"):
        U.run_postproc(None, CH, ensemble=(host, 1, (2, 2, 2)))


# ---- EvaluateUNet's refusals -----------------------------------------------------------------------------------------------------
class FakeModel:
    """what EvaluateUNet reads of a model before the first upload"""
    in_count, out_count = 1, 3
    dim, voxel_size = (16, 16, 16), (1.0, 1.0, 1.0)
    postproc, preproc, orientation, fov_strategy = "softmax+create_mask+argmax", "", "", "align_top"
    single_component_label = []

    def __init__(self, **kw):
        self.prepared = 0
        self.__dict__.update(kw)

    def device(self):
        return "cpu"

    def prepare_for_inference(self, device):
        self.prepared += 1

    def forward(self, x, packs_current=False):
        raise AssertionError("the forward was reached")


def test_evaluate_refusals_need_no_device(monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, "Stream", lambda *a, **k: None)     # start() makes its copy stream first
    m = FakeModel()
    marker = np.zeros((16, 16, 16), F)
    CH = "softmax+create_mask+argmax"
    cases = [
        (dict(ensemble=[FakeModel(out_count=4)], postproc=CH), "ensemble: member 1 has out_count 4, member 0 has 3"),
        (dict(ensemble=[FakeModel(), FakeModel(in_count=2, out_count=4)], postproc=CH), "ensemble: member 2 has in_count 2, member 0 has 1"),
        (dict(ensemble=[FakeModel(dim=(16, 16, 32))], postproc=CH), "ensemble: member 1 has dim (16, 16, 32), member 0 has (16, 16, 16)"),
        (dict(ensemble=[FakeModel(voxel_size=(1.0, 1.0, 2.0))], postproc=CH), "ensemble: member 1 has voxel_size (1.0, 1.0, 2.0)"),
        (dict(ensemble=[object()], postproc=CH), "ensemble: member 1 is not a model"),
        (dict(ensemble=FakeModel(), postproc=CH), "ensemble must be a list of further models"),
        (dict(ensemble=[FakeModel()], ensemble_weights=[1, 2, 3], postproc=CH), "ensemble_weights: 3 weights for 2 members"),
        (dict(ensemble=[FakeModel()], ensemble_weights=[1, 0], postproc=CH), "a weight must be finite and positive"),
        (dict(ensemble_weights=[1], postproc=CH), "ensemble_weights needs ensemble"),
        (dict(postproc=CH, outputs=("label", "mutual_info")), "output mutual_info needs more than one member"),
        (dict(ensemble=[], postproc=CH, outputs=("label", "mutual_info")), "output mutual_info needs more than one member"),
        (dict(ensemble=[FakeModel()], postproc=CH, outputs=("label", "agreement"), mirror_axes="x"), "agreement is not available with ensemble"),
        (dict(postproc=CH, outputs=("entropy", "agreement"), mirror_axes="x"), "agreement is not available with ensemble"),
        (dict(outputs=("entropy",)), "output entropy needs a postproc chain"),
        (dict(ensemble=[FakeModel()], outputs=("mutual_info",)), "output mutual_info needs a postproc chain"),
        (dict(ensemble=[FakeModel()], outputs=()), "ensemble needs a postproc chain"),
        (dict(ensemble=[FakeModel()], postproc="softmax+create_mask+minus+softmax+argmax", outputs=("label_prob",)), "softmax may not recur after minus"),
        (dict(ensemble=[FakeModel()], postproc=CH, outputs=("label", "variance")), "unknown output variance"),
    ]
    for kw, word in cases:
        further = kw.get("ensemble") if isinstance(kw.get("ensemble"), list) else []
        ev = U.EvaluateUNet(m, device="cpu", **kw)
        out = ev.start([[marker]])
        assert ev.aborted and word in ev.error_msg and not ev.running and ev.cur_prog == 0, (kw, ev.error_msg)
        assert out[0][0] is marker
        assert all(getattr(f, "prepared", 0) == 0 for f in further)    # a refused run prepares no further member
