"""No device: the recalibration pass (include/unet_recal.h, unet_studio_amd/recal.py) -- the fp64 numpy restatement recal_ref of the
header's definitions on hand-worked voxels (tests/test_gpu_recal.py holds the device to it), Solver against synthetic convex problems
fed as hand-made integer tables, head_is_bare_conv, the ABI's exports and constants, every argument error of both entry points, the
wrapper errors, the refusals of qc.recalibration_qc and the report's formatting."""
import ctypes
import math
import os
import re
import types

import numpy as np
import pytest
import torch

import unet_studio_amd as U
from unet_studio_amd import qc as Q
from unet_studio_amd import recal as RC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
NAN, INF = float("nan"), float("inf")
ONE = 1 << RC.SCALE_BITS


# ---- the restatement -------------------------------------------------------------------------------------------------------------------
def classify(x, label, mask):
    """-> (kind {S}: 0 valid, 1 bad, 2 invalid_label, 3 skipped, 4 impossible; t {S}; M {S}): the header's order, mask before label
    before logits"""
    C, S = x.shape
    lab = np.asarray(label, F).reshape(S)
    with np.errstate(invalid="ignore"):
        lab_ok = (lab > F(-1.0)) & (lab < F(C))                   # false for a NaN
        t = np.where(lab_ok, np.trunc(np.where(lab_ok, lab, 0)), 0).astype(np.int64)
        M = np.fmax.reduce(x, axis=0)                             # a NaN is dropped; all NaN stays NaN
        bad = np.isnan(x).any(axis=0) | ~np.isfinite(M)           # a NaN, a +inf, or all channels -inf
    xt = x[t, np.arange(S)]
    skipped = np.zeros(S, bool) if mask is None else np.asarray(mask, np.uint8).reshape(S) == 0
    kind = np.where(skipped, 3, np.where(~lab_ok, 2, np.where(bad, 1, np.where(xt == -INF, 4, 0))))
    return kind, t, M


def recal_ref(logits, label, mask, betas):
    """The header's definitions in fp64 -> dict: head (6 ints), nll and g (per candidate, the integer sums of the quantised terms as
    Python ints), nll_bound and g_bound (per candidate, in the terms' unit: the a-priori round-off bounds of an fp32 evaluation,
    quantisation plus about 2 ulp per operation with no cancellation assumed)."""
    x = np.ascontiguousarray(logits, F).astype(np.float64)
    C, S = x.shape
    kind, t, M = classify(x, label, mask)
    v = np.flatnonzero(kind == 0)
    head = [int((kind == k).sum()) for k in range(5)] + [0]
    out = {"head": head, "nll": [], "g": [], "nll_bound": [], "g_bound": []}
    xv = x[:, v]
    d = xv - M[v]                                                 # -inf for a -inf channel, 0 at the max
    dt = d[t[v], np.arange(v.size)]
    fin = d != -INF
    d0 = np.where(fin, d, 0.0)
    sat = np.zeros(v.size, bool)
    for b in betas:
        b = float(F(b))
        with np.errstate(over="ignore", under="ignore"):
            e = np.exp(b * d)                                     # 0 for a -inf channel
        s = e.sum(axis=0)
        a = (e * d0).sum(axis=0)
        terms = (np.log(s) - b * dt, a / s - dt)
        for name, u in zip(("nll", "g"), terms):
            sat |= np.abs(u) > RC.CLAMP
            q = np.rint(np.clip(u, -RC.CLAMP, RC.CLAMP) * ONE).astype(np.int64)      # ties to even, as llrintf
            out[name].append(int(q.sum()))
        reach = np.where(b * d > -88.0, np.abs(d0), 0.0).max(axis=0) if v.size else np.zeros(0)
        out["nll_bound"].append(v.size * 2.0 ** -21 + 2.0 ** -20 * float((1.0 + np.abs(np.log(s)) + b * np.abs(dt)).sum()))
        out["g_bound"].append(v.size * 2.0 ** -21 + C * 2.0 ** -20 * float((1.0 + np.abs(dt) + reach).sum()))
    head[5] = int(sat.sum())
    return out


def table_of(ref):
    """the restatement as the int64 table the device would write (22 entries; the unused candidates 0)"""
    t = np.zeros(RC.TABLE_LEN, np.int64)
    t[:6] = ref["head"]
    for k, (n, g) in enumerate(zip(ref["nll"], ref["g"])):
        t[6 + 2 * k], t[7 + 2 * k] = n, g
    return t


def one(x, label, betas=(0.5, 1.0, 3.0), mask=None):
    return recal_ref(np.asarray(x, F).reshape(-1, 1), [label], None if mask is None else [mask], betas)


def test_recal_ref_on_hand_worked_voxels():
    r = one([0.0, 0.0], 0)                                        # C = 2, logits (0, 0): nll = ln 2 and g = 0 at every beta
    assert r["head"] == [1, 0, 0, 0, 0, 0] and r["g"] == [0, 0, 0]
    assert r["nll"] == [int(np.rint(math.log(2.0) * ONE))] * 3
    r = one([0.0, -INF], 0)                                       # one-hot with the right label: nll 0 and g 0
    assert r["head"] == [1, 0, 0, 0, 0, 0] and r["nll"] == [0, 0, 0] and r["g"] == [0, 0, 0]
    r = one([0.0, -INF], 1)                                       # the wrong label: the likelihood is 0 at every beta
    assert r["head"] == [0, 0, 0, 0, 1, 0] and r["nll"] == [0, 0, 0] and r["g"] == [0, 0, 0]
    for x in ([NAN, 0.0], [0.0, NAN], [INF, 0.0], [-INF, -INF], [NAN, INF]):
        assert one(x, 0)["head"] == [0, 1, 0, 0, 0, 0], x
    # a worked two-class voxel: x = (0, -ln 3), label 1, beta 1: p = (3/4, 1/4), nll = ln 4, g = sum p d - dt = -ln 3 / 4 + ln 3
    r = one([0.0, -math.log(3.0)], 1, betas=(1.0,))
    x1 = float(F(-math.log(3.0)))
    s = 1.0 + math.exp(x1)
    assert r["nll"] == [int(np.rint((math.log(s) - x1) * ONE))] and abs(r["nll"][0] / ONE - math.log(4.0)) < 1e-6
    assert abs(r["g"][0] / ONE - 0.75 * math.log(3.0)) < 1e-6
    assert r["nll_bound"][0] == pytest.approx(2.0 ** -21 + 2.0 ** -20 * (1.0 + math.log(s) - x1), rel=1e-12)
    assert r["g_bound"][0] == pytest.approx(2.0 ** -21 + 2 * 2.0 ** -20 * (1.0 - x1 - x1), rel=1e-12)


def test_labels_masks_and_the_order_of_the_rules():
    C = 3
    x = [0.5, -1.0, 2.0]
    assert one(x, -0.5)["head"][0] == 1 and one(x, C - 0.5)["head"][0] == 1                     # t = 0 and t = C - 1
    assert one(x, -0.5)["nll"] == one(x, 0.0)["nll"] and one(x, C - 0.5)["g"] == one(x, 2.0)["g"]
    for lab in (float(C), NAN, -1.0, INF, -INF):
        assert one(x, lab)["head"] == [0, 0, 1, 0, 0, 0], lab
    for m, want in ((0, [0, 0, 0, 1, 0, 0]), (1, [1, 0, 0, 0, 0, 0]), (255, [1, 0, 0, 0, 0, 0])):
        assert one(x, 1, mask=m)["head"] == want
    # mask before label before logits
    assert one([NAN, 0.0, 0.0], NAN, mask=0)["head"] == [0, 0, 0, 1, 0, 0]
    assert one([NAN, 0.0, 0.0], NAN, mask=1)["head"] == [0, 0, 1, 0, 0, 0]
    assert one([NAN, 0.0, 0.0], 1, mask=1)["head"] == [0, 1, 0, 0, 0, 0]
    assert one([0.0, -INF, 0.0], 1, mask=1)["head"] == [0, 0, 0, 0, 1, 0]
    assert one([NAN, -INF, 0.0], 1, mask=1)["head"] == [0, 1, 0, 0, 0, 0]                       # bad before impossible


def test_clamped_terms_count_once_and_enter_clamped():
    r = one([5000.0, -5000.0], 1, betas=(16.0, 1.0 / 16))
    # beta 16: nll = 160000 and g = 10000 are clamped to 4096; beta 1/16: nll = 625 is not, g = 10000 is
    assert r["head"] == [1, 0, 0, 0, 0, 1] and r["nll"] == [4096 * ONE, 625 * ONE] and r["g"] == [4096 * ONE, 4096 * ONE]
    r = one([5000.0, -5000.0], 0, betas=(16.0,))
    assert r["head"] == [1, 0, 0, 0, 0, 0] and r["nll"] == [0] and r["g"] == [0]
    assert 4096 * ONE == 1 << 32 and RC.CLAMP * ONE * ((1 << 31) - 1) < 1 << 63                 # every sum stays inside int64


def test_a_random_volume_is_consistent():
    rng = np.random.default_rng(5)
    C, S = 6, 500
    x = (rng.standard_normal((C, S)) * 3).astype(F)
    lab = rng.integers(0, C, S).astype(F)
    betas = (0.25, 1.0, 4.0)
    r = recal_ref(x, lab, None, betas)
    assert r["head"] == [S, 0, 0, 0, 0, 0]
    p = np.exp(x.astype(np.float64) - x.max(axis=0))
    p /= p.sum(axis=0)
    nll = -np.log(p[lab.astype(int), np.arange(S)]).sum()
    assert abs(r["nll"][1] / ONE - nll) < r["nll_bound"][1]
    assert r["g"][0] < r["g"][1] < r["g"][2]                      # g increases in beta: the nll is convex
    # g is the slope of nll
    h = 2.0 ** -10
    lo, hi = recal_ref(x, lab, None, (1.0 - h, 1.0 + h))["nll"]
    assert abs((hi - lo) / ONE / (2 * h) - r["g"][1] / ONE) < 1e-3 * S
    # two halves add up to the whole
    a, b = recal_ref(x[:, :123], lab[:123], None, betas), recal_ref(x[:, 123:], lab[123:], None, betas)
    assert (table_of(a) + table_of(b) == table_of(r)).all()


# ---- Solver --------------------------------------------------------------------------------------------------------------------------
def fed(betas, G, valid=1000):
    """a hand-made table: the candidates' G in the g entries"""
    t = np.zeros(RC.TABLE_LEN, np.int64)
    t[0] = valid
    for k, b in enumerate(betas):
        t[7 + 2 * k] = int(np.rint(G(float(b)) * ONE))
    return t


def test_sums_are_exact():
    t = np.arange(100, 122, dtype=np.int64)
    t[6], t[7] = -3, (1 << 62) + 1
    head, nll, g = RC.sums(t, 2)
    assert head == [100, 101, 102, 103, 104, 105] and nll[0] * ONE == -3 and g[0] * ONE == (1 << 62) + 1 and nll[1] * ONE == 108
    assert RC.sums(torch.from_numpy(t), 8)[2][7] * ONE == 121
    for n in (0, 9):
        with pytest.raises(U.UNetError, match="n_betas must be in"):
            RC.sums(t, n)
    with pytest.raises(U.UNetError, match="a table holds 22 integers"):
        RC.sums(t[:21], 1)
    with pytest.raises(U.UNetError, match="a table holds 22 integers"):
        RC.sums(t.astype(np.float64), 1)


@pytest.mark.parametrize("star", [0.0625 * 1.0001, 0.7, 1.0, 2.9, 15.99])
def test_solver_brackets_the_zero_after_every_round(star):
    s = RC.Solver()
    first = s.betas()
    assert len(first) == 8 and all(isinstance(b, np.float32) for b in first)
    assert [float(b) for b in first] == [float(F(2.0 ** (-4.0 + 8.0 * k / 7.0))) for k in range(8)] and first[0] == 0.0625 and first[7] == 16.0
    assert not s.done and s.width() == 8.0 / 7.0 / 81.0 and abs(s.width() - 0.0141) < 5e-5 and s.width(1) == 8.0 / 7.0
    for r in range(1, 4):
        sent = s.betas()
        s.update(fed(sent, lambda b: 100.0 * (math.log(b) - math.log(star))))
        res = s.result()
        lo, hi = res["bracket"]
        assert res["rounds"] == r and res["at_bound"] == 0 and lo < star <= hi and lo <= res["beta"] <= hi
        assert abs(math.log2(hi / lo) - s.width(r)) < 1e-6         # the candidates are float32
        if r > 1:
            assert all(plo < float(b) < phi for b in sent) and plo <= lo and hi <= phi    # 8 interior points of the last bracket
        plo, phi = lo, hi
        assert s.done == (r == 3)
    assert res["temperature"] == 1.0 / res["beta"] and abs(res["beta"] / star - 1.0) < 1e-4
    with pytest.raises(U.UNetError, match="the rounds are over"):
        s.betas()


def test_solver_at_both_bounds_and_on_a_candidate():
    s = RC.Solver()
    s.update(fed(s.betas(), lambda b: b))                          # G > 0 everywhere: the minimiser is below the range
    assert s.done and s.result() == {"beta": 0.0625, "temperature": 16.0, "bracket": (0.0625, 0.0625), "at_bound": -1, "rounds": 1}
    s = RC.Solver()
    s.update(fed(s.betas(), lambda b: 0.0 if b == 0.0625 else 1.0))   # G = 0 at u_lo counts as the bound
    assert s.result()["at_bound"] == -1
    s = RC.Solver()
    s.update(fed(s.betas(), lambda b: -1.0 / b))                   # G < 0 everywhere: above the range
    assert s.done and s.result() == {"beta": 16.0, "temperature": 0.0625, "bracket": (16.0, 16.0), "at_bound": 1, "rounds": 1}
    # a zero that falls exactly on a candidate: that candidate is the bracket's upper end, and the secant lands on it
    s = RC.Solver(rounds=2)
    sent = s.betas()
    s.update(fed(sent, lambda b: b - float(sent[3])))
    assert s.result()["bracket"] == (float(sent[2]), float(sent[3])) and s.result()["beta"] == float(sent[3]) and not s.done
    s.update(fed(s.betas(), lambda b: b - float(sent[3])))
    assert s.result()["bracket"][1] == float(sent[3]) and s.result()["beta"] == float(sent[3]) and s.done
    # another range and round count; the secant between the ends
    s = RC.Solver(-1.0, 1.0, rounds=1)
    assert [float(b) for b in s.betas()][::7] == [0.5, 2.0] and s.width() == 2.0 / 7.0
    s.update(fed(s.betas(), lambda b: b - 1.0))
    lo, hi = s.result()["bracket"]
    assert lo < 1.0 < hi and abs(s.result()["beta"] - 1.0) < 2e-6   # G is linear in beta: the secant is exact up to the quantisation
    with pytest.raises(U.UNetError, match="no valid voxel"):
        RC.Solver().update(fed(RC.Solver().betas(), lambda b: b, valid=0))
    with pytest.raises(U.UNetError, match="no round has run"):
        RC.Solver().result()
    for bad in ((1.0, 1.0), (2.0, 1.0), (NAN, 1.0), (-200.0, 0.0)):
        with pytest.raises(U.UNetError, match="u_lo < u_hi"):
            RC.Solver(*bad)
    for bad in (0, -1, 2.0, True):
        with pytest.raises(U.UNetError, match="rounds must be a positive integer"):
            RC.Solver(rounds=bad)


# ---- the head ------------------------------------------------------------------------------------------------------------------------
def test_head_is_bare_conv():
    assert RC.head_token(U.default_feature(6)) == "conv6,ks1,stride1" and RC.head_is_bare_conv(U.default_feature(6))
    body = "conv8,ks3,stride1+norm,leaky_relu\nconv8,ks3,stride1\nconv8,ks3,stride1+"
    for token, want in (("conv4,ks1,stride1", True), ("conv4", True), ("conv4,ks1", True), ("conv4,ks3,stride1", True),
                        ("conv4,ks1,stride1,relu", False), ("conv4,ks1,stride1,leaky_relu", False), ("conv4,elu", False),
                        ("norm", False), ("norm,leaky_relu", False), ("conv4,ks1,norm", False), ("conv_trans4,ks2,stride2", False),
                        ("conv,ks1", False), ("conv4,ks1,ks1", False), ("bnorm", False), ("upsample", False)):
        assert RC.head_is_bare_conv(body + token) is want, token
    assert RC.head_token("a\r\nb\r\n\r\nc+d \n") == "d"
    with pytest.raises(U.UNetError, match="empty"):
        RC.head_token("\n\n")


def test_fold_refuses_before_it_touches_anything():
    touched = []
    m = types.SimpleNamespace(architecture="conv8,ks3\nconv8,ks3\nconv8,ks3+conv4,ks1,stride1,relu", _params=touched, _params_version=7,
                              _probe=types.SimpleNamespace(param_names=["output0.0.weight", "output0.0.bias"]))
    with pytest.raises(U.UNetError, match=r"the level-0 head 'conv4,ks1,stride1,relu' is not a bare conv"):
        RC.fold(m, 2.0)
    m.architecture = "conv8,ks3\nconv8,ks3\nconv8,ks3+conv4,ks1,stride1"
    m._probe.param_names = ["decode0.0.weight", "decode0.0.bias", "output0.0.weight", "output0.0.bias", "output0.1.weight", "output0.1.bias"]
    with pytest.raises(U.UNetError, match=r"the level-0 head 'conv4,ks1,stride1' must own exactly output0.0.weight and output0.0.bias"):
        RC.fold(m, 2.0)
    m._probe.param_names = m._probe.param_names[:4]
    for beta in (0.0, -1.0, NAN, INF, 1e-60):
        with pytest.raises(U.UNetError, match="beta must be finite and positive"):
            RC.fold(m, beta)
    assert m._params_version == 7 and touched == []


# ---- the ABI -------------------------------------------------------------------------------------------------------------------------
OTHERS = ("unet_calib_", "unet_stats_", "unet_ens_", "unet_table_", "unet_reg_", "unet_atlas_", "unet_components_", "unet_preproc_",
          "unet_dist_", "unet_inst_", "unet_morph_", "unet_conn_", "unet_mirror_", "unet_tiles_", "unet_space_", "unet_postproc_",
          "unet_qc_", "unet_feed_", "unet_augment_")


def test_unet_recal_h_declares_exactly_the_exports_and_the_library_has_them():
    lib = ctypes.CDLL(U.engine.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "unet_recal.h")).read()
    declared = set(re.findall(r"\b(unet_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(RC.EXPORTS) == {"unet_recal_scratch_bytes", "unet_recal_eval"}
    for name in sorted(declared):
        assert hasattr(lib, name), "libunet_hip.so does not export " + name
    defines = {k: int(v) for k, v in re.findall(r"#define UNET_RECAL_([A-Z_]+) (\d+)", hdr)}
    assert defines == {"MAX_CLASSES": RC.MAX_CLASSES, "MAX_BETAS": RC.MAX_BETAS, "HEAD": RC.HEAD, "TABLE_LEN": RC.TABLE_LEN,
                       "SCALE_BITS": RC.SCALE_BITS, "CLAMP": RC.CLAMP, "CACHE": RC.CACHE, "UNIT": RC.UNIT, "BLOCK_UNITS": RC.BLOCK_UNITS,
                       "GRID_UNITS": RC.GRID_UNITS}
    assert (RC.MAX_CLASSES, RC.MAX_BETAS, RC.HEAD, RC.TABLE_LEN, RC.SCALE_BITS, RC.CLAMP) == (256, 8, 6, 22, 20, 4096)
    assert RC.TABLE_LEN == RC.HEAD + 2 * RC.MAX_BETAS
    assert RC.GRID_UNITS % RC.BLOCK_UNITS == 0 and RC.BLOCK_UNITS % 64 == 0 and RC.GRID_UNITS * RC.UNIT < 1 << 25
    assert "this project's" in hdr and "NOT pinned" in hdr
    assert U.recal is RC
    for other in OTHERS:                                           # the prefixes stay apart
        assert other not in hdr.lower(), other
    for h in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if h != "unet_recal.h":
            assert "unet_recal_" not in open(os.path.join(ROOT, "include", h)).read().lower(), h


# ---- argument errors, before any device call -------------------------------------------------------------------------------------
P = [ctypes.c_void_p(0x1000 * (i + 1)) for i in range(8)]          # never dereferenced
BIG = 1 << 40


def floats(*v):
    return (ctypes.c_float * len(v))(*v)


def test_scratch_bytes_checks_its_arguments():
    assert len({RC.scratch_bytes(c, v) for c in (2, 6, 256) for v in (1, 64, 10 ** 6, (1 << 31) - 1)}) == 1     # nothing per voxel or class
    assert RC.scratch_bytes(6, 10) >= RC.TABLE_LEN * 8
    for c in (1, 0, -1, 257):
        with pytest.raises(U.UNetError, match=r"unet_recal_scratch_bytes: out_c must be in \[2, 256\], got %d" % c):
            RC.scratch_bytes(c, 10)
    for v in (0, -5, 1 << 31):
        with pytest.raises(U.UNetError, match=r"unet_recal_scratch_bytes: voxels must be in \[1, 2\^31\), got %d" % v):
            RC.scratch_bytes(6, v)
    lib = U.engine.lib
    assert lib.unet_recal_scratch_bytes(6, 10, None) != 0 and lib.unet_last_error().decode() == "unet_recal_scratch_bytes: null bytes"


def test_eval_argument_errors_need_no_device():
    lib = U.engine.lib
    good = floats(0.5, 1.0, 2.0)

    def call(logits=P[0], C=6, voxels=64, label=P[1], mask=None, betas=good, n=3, acc=0, tables=P[2], scratch=P[3], scratch_bytes=BIG):
        rc = lib.unet_recal_eval(logits, C, voxels, label, mask, betas, n, acc, tables, scratch, scratch_bytes, None)
        assert rc != 0
        msg = lib.unet_last_error().decode()
        assert msg.startswith("unet_recal_eval: ")
        return msg

    assert "null logits" in call(logits=None) and "logits must be 4-byte aligned" in call(logits=ctypes.c_void_p(0x2002))
    assert "out_c must be in [2, 256], got 1" in call(C=1) and "out_c must be in [2, 256], got 257" in call(C=257)
    assert "voxels must be in [1, 2^31), got 0" in call(voxels=0) and "voxels" in call(voxels=-3) and "voxels" in call(voxels=1 << 31)
    assert "null label" in call(label=None) and "label must be 4-byte aligned" in call(label=ctypes.c_void_p(0x2001))
    assert "null betas" in call(betas=None)
    assert "n_betas must be in [1, 8], got 0" in call(n=0) and "n_betas must be in [1, 8], got 9" in call(n=9) and "n_betas" in call(n=-1)
    for k, v in ((0, 0.0), (1, -1.0), (2, NAN), (0, INF), (1, -INF), (2, -0.0)):
        b = [0.5, 1.0, 2.0]
        b[k] = v
        assert "betas[%d] must be finite and positive" % k in call(betas=floats(*b)), (k, v)
    assert "null tables" in call(betas=floats(0.5, NAN), n=1, tables=None)          # a value behind n_betas is not read
    assert "null tables" in call(tables=None) and "tables must be 8-byte aligned" in call(tables=ctypes.c_void_p(0x3004))
    assert "null scratch" in call(scratch=None)
    assert "scratch too small" in call(scratch_bytes=RC.scratch_bytes(6, 64) - 1)
    assert "null tables" in call(acc=1, tables=None, mask=P[4])                      # both flags of accumulate reach the same checks


def test_wrapper_errors_need_no_device():
    x, lab = torch.zeros(2, 8, dtype=torch.float32), torch.zeros(8, dtype=torch.float32)
    with pytest.raises(U.UNetError, match="logits must be a contiguous float32 device tensor"):
        RC.eval_betas(x, lab, (1.0,))
    with pytest.raises(U.UNetError, match="logits must be"):
        RC.eval_betas(None, lab, (1.0,))
    with pytest.raises(U.UNetError, match="batches yielded no case"):
        RC.fit(lambda: iter(()))
    with pytest.raises(U.UNetError, match="logits must be"):
        RC.fit(lambda: iter([(x, lab)]))


# ---- the refusals of qc.recalibration_qc ------------------------------------------------------------------------------------------------
def test_recalibration_qc_refusals_need_no_device():
    m = types.SimpleNamespace(in_count=1, out_count=4, dim=(16, 16, 16), voxel_size=(1.0, 1.0, 1.0),
                              architecture="conv8,ks3\nconv8,ks3\nconv8,ks3+conv4,ks1,stride1,leaky_relu")
    case = [("a.nii.gz", "b.nii.gz", np.zeros((1, 16, 16, 16), F), np.zeros((16, 16, 16), F), True)]
    path = "/nowhere/model.nz"
    assert Q.recalibration_qc(m, path, []) == (1, "no image/label pairs found")
    assert Q.recalibration_qc(types.SimpleNamespace(in_count=1, out_count=1, dim=(16, 16, 16)), path, case) == (1, "QC requires a categorical model")
    assert Q.recalibration_qc(m, path, case, mask="brain") == (1, "recalibration_qc: mask must be one of all, foreground, got 'brain'")
    for u in ((1.0, 1.0), (3.0, -3.0), (NAN, 1.0)):
        assert Q.recalibration_qc(m, path, case, u_range=u)[1].startswith("recalibration_qc: recal.Solver: u_lo < u_hi")
    for u in ((1.0,), 3.0, (1.0, 2.0, 3.0), ("a", "b")):
        assert Q.recalibration_qc(m, path, case, u_range=u) == (1, "recalibration_qc: u_range must be (u_lo, u_hi), got %r" % (u,))
    for r in (0, 2.5, True):
        assert Q.recalibration_qc(m, path, case, rounds=r) == (1, "recalibration_qc: recal.Solver: rounds must be a positive integer, got %r" % (r,))
    assert Q.recalibration_qc(m, path, case, apply=True) == (
        1, "recalibration_qc: the level-0 head 'conv4,ks1,stride1,leaky_relu' is not a bare conv: beta cannot be folded in")
    assert RC.report_path("/x/y/model.nz") == "/x/y/model.recalibration_report.tsv"


def test_format_report():
    def tab(valid, before, after, impossible=0, saturated=0):
        t = np.zeros(RC.TABLE_LEN, np.int64)
        t[0], t[4], t[5], t[6], t[8] = valid, impossible, saturated, int(before * valid * ONE), int(after * valid * ONE)
        return t

    fitted = {"beta": 0.75, "temperature": 1.0 / 0.75, "bracket": (0.7421875, 0.7578125), "at_bound": 0, "rounds": 3, "table": tab(30, 1.5, 1.25, 2, 1)}
    text = RC.format_report([("/d/a_T1w.nii.gz", "/d/a_seg.nii.gz", tab(10, 1.5, 1.25)), ("/d/b.nii.gz", "/d/b_seg.nii.gz", None),
                             ("/d/c.nii.gz", "/d/c_seg.nii.gz", tab(0, 0.0, 0.0))], fitted)
    lines = text.split("\n")
    assert lines[0] == "image\tground_truth\tvoxels\tnll_before\tnll_after\tbeta\ttemperature\tbeta_lo\tbeta_hi\tat_bound\timpossible\tsaturated"
    assert lines[1] == "a_T1w.nii.gz\ta_seg.nii.gz\t10\t1.5\t1.25" + "\t" * 7
    assert lines[2] == "b.nii.gz\tb_seg.nii.gz\tN/A\tN/A\tN/A" + "\t" * 7
    assert lines[3] == "c.nii.gz\tc_seg.nii.gz\t0\tnan\tnan" + "\t" * 7
    assert lines[4] == "total\t\t30\t1.5\t1.25\t0.75\t1.33333333\t0.7421875\t0.7578125\t0\t2\t1" and lines[5] == "" and len(lines) == 6
    none = RC.format_report([("a", "b", None)], None).split("\n")
    assert none[1] == "a\tb\tN/A\tN/A\tN/A" + "\t" * 7 and none[2] == "total\t" + "\tN/A" * 10
    assert RC.mean_nll(tab(4, 2.0, 1.0)) == (4, [2.0, 1.0])
