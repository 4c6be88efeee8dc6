"""GPU: the calibration tables on the device (include/unet_calib.h) -- unet_calib_tables under IMPL_LDS, IMPL_GLOBAL and the default
against calib_ref (the restatement of test_calib_host.py), every case twice into garbage-filled outputs with guard words on both
sides; LOGITS against PROBS on an ensemble state of one member, device against device; LOGITS on exact data against calib_ref;
accumulate, the byte map through uncertainty_hists, and qc.calibration_qc against the same composition written out by hand.  Every
comparison is exact equality of bytes.  The voxel counts come from the kernel's own constants."""
import os
import sys

import numpy as np
import pytest
import torch

import unet_studio_amd as U
from unet_studio_amd import calib as CB
from unet_studio_amd import ensemble as EN
from unet_studio_amd import qc as Q

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_calib_host import calib_ref, softmax_exact  # noqa: E402
from test_stats_host import hist_ref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F = np.float32
NAN, INF = float("nan"), float("inf")
IMPLS = (CB.IMPL_LDS, CB.IMPL_GLOBAL, CB.IMPL_DEFAULT)
G = 64                                                             # guard words on each side of an output
GUARD = -0x5A3C5A3C
GUARD8 = 0xA5
BLOCK = CB.UNIT * CB.BLOCK_UNITS                                   # the voxels a block takes at once


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def same(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()


def offset(t, by):
    """a copy of the flat tensor t that starts `by` bytes after a 256-byte boundary"""
    n = by // t.element_size()
    assert n * t.element_size() == by
    buf = torch.empty(t.numel() + n, dtype=t.dtype, device=t.device)
    assert buf.data_ptr() % 256 == 0
    view = buf[n:]
    view.copy_(t.reshape(-1))
    return view


def guarded_table(n, rep):
    buf = torch.full((n + 2 * G,), GUARD, dtype=torch.int64, device=DEV)
    buf[G:G + n] = 0x7B7B7B7B7B7B if rep == 0 else -3
    return buf, buf[G:G + n]


def guarded_bytes(n, rep, shift=0):
    buf = torch.full((n + 2 * G + shift,), GUARD8, dtype=torch.uint8, device=DEV)
    buf[G + shift:G + shift + n] = 0x7B if rep == 0 else 0xFD
    return buf, buf[G + shift:G + shift + n]


def guards_intact(buf, n, guard, shift=0):
    b = buf.cpu().numpy()
    return (b[:G + shift] == guard).all() and (b[G + shift + n:] == guard).all()


def run(src, kind, C, S, label, mask, impl, rep, want_wrong=True, shift=0):
    """one call into guarded, garbage-filled outputs -> (table, wrong) as numpy"""
    n = CB.table_len(C)
    tb, out = guarded_table(n, rep)
    wb, wrong = guarded_bytes(S, rep, shift) if want_wrong else (None, None)
    if kind == CB.SRC_LOGITS:
        got = CB.tables(src.view(C, S), label, mask=mask, out=out, wrong=wrong, impl=impl)
    else:
        got = CB.tables_from_probs(src, C, S, label, mask=mask, out=out, wrong=wrong, impl=impl)
    assert got.data_ptr() == out.data_ptr()
    t = got.cpu().numpy()
    assert guards_intact(tb, n, GUARD)
    if not want_wrong:
        return t, None
    assert guards_intact(wb, S, GUARD8, shift)
    return t, wrong.cpu().numpy()


def check_probs(planes, label, mask=None):
    """PROBS under every impl, twice each, against calib_ref -> the restatement's (table, wrong)"""
    planes = np.ascontiguousarray(planes, F)
    C, S = planes.shape
    want_t, want_w = calib_ref(planes, label, mask)
    d_p, d_l, d_m = dev(planes), dev(np.asarray(label, F)), None if mask is None else dev(np.asarray(mask, np.uint8))
    for impl in IMPLS:
        for rep in range(2):
            t, w = run(d_p, CB.SRC_PROBS, C, S, d_l, d_m, impl, rep)
            assert same(t, want_t), (impl, rep, np.argwhere(t != want_t)[:8].tolist())
            assert same(w, want_w), (impl, rep, np.argwhere(w != want_w)[:8].tolist())
    assert int(want_t[:4].sum()) == S
    return want_t, want_w


# ---- inputs --------------------------------------------------------------------------------------------------------------------------
def probs(rng, C, S, scale=3.0):
    """a softmax computed in numpy: arbitrary float32 values the device only reads"""
    x = rng.standard_normal((C, S)) * scale
    e = np.exp(x - x.max(axis=0))
    return (e / e.sum(axis=0)).astype(F)


def labels(rng, C, S):
    return rng.integers(0, C, S).astype(F)


def plant(rng, p, label, mask):
    """the special voxels at chosen places (the first ones of the volume, and its last), the rest at random"""
    C, S = p.shape
    vals = [NAN, 0.0, 1.0, -0.25, 1.5, -0.0]
    for i, v in enumerate(vals):
        if i < S:
            p[i % C, i] = v
    p[C - 1, S - 1] = 1.0
    for v, share in ((NAN, 0.02), (0.0, 0.03), (1.0, 0.03), (-0.5, 0.01), (2.0, 0.01), (-0.0, 0.01)):
        at = np.flatnonzero(rng.random(S) < share)
        p[rng.integers(0, C, at.size), at] = v
    for i, v in enumerate([-0.5, C - 0.5, float(C), NAN, -1.0, 0.5]):
        if 6 + i < S:
            label[6 + i] = v
    for v, share in ((-0.5, 0.01), (C - 0.5, 0.01), (float(C), 0.01), (NAN, 0.01)):
        label[rng.random(S) < share] = v
    if mask is not None:
        mask[:] = rng.choice(np.asarray([0, 1, 255], np.uint8), S, p=[0.2, 0.5, 0.3])
        mask[:3] = [0, 1, 255][:min(3, S)]


# ---- PROBS against calib_ref -----------------------------------------------------------------------------------------------------------
COUNTS = [1, CB.UNIT - 1, CB.UNIT, BLOCK + 3 * CB.UNIT + 5, BLOCK + 3 * CB.UNIT + 4]   # the last: 16-byte loads, half a unit at the end


@pytest.mark.parametrize("C", [2, 6, 9])
@pytest.mark.parametrize("S", COUNTS)
def test_probs_around_a_unit_and_a_block(C, S):
    rng = np.random.default_rng(100 * C + S)
    p, label, mask = probs(rng, C, S), labels(rng, C, S), np.ones(S, np.uint8)
    plant(rng, p, label, mask)
    t, w = check_probs(p, label, mask)
    check_probs(p, label, None)
    if S > BLOCK:
        assert (t[:4] > 0).all() and (w == 1).any() and (w == 2).any()


@pytest.mark.parametrize("C", [CB.LDS_CLASSES + 1, CB.MAX_CLASSES])
def test_probs_with_more_classes_than_the_lds_table_holds(C):
    S = BLOCK + 2 * CB.UNIT + (4 if C == CB.MAX_CLASSES else 3)
    rng = np.random.default_rng(C)
    p, label, mask = probs(rng, C, S, 6.0), labels(rng, C, S), np.ones(S, np.uint8)
    plant(rng, p, label, mask)
    t, _ = check_probs(p, label, mask)
    cls = CB.split(t, C)[2]
    assert cls[CB.LDS_CLASSES:, :, 0].sum() > 0 and cls[C - 1, :, 1].sum() > 0       # rows above the held range were updated


def test_the_capped_grid_strides_twice():
    S = 2 * CB.GRID_UNITS * CB.UNIT + 3 * CB.UNIT + 5
    rng = np.random.default_rng(7)
    p = np.empty((2, S), F)
    p[0] = (rng.integers(0, 4097, S) / F(4096)).astype(F)           # ties and exact ends everywhere
    p[1] = F(1) - p[0]
    label = (rng.random(S) < 0.3).astype(F)
    p[:, -3:] = [[0.25, NAN, 1.0], [0.75, 0.5, 0.0]]                 # the third stride's voxels count
    label[-3:] = [1.0, 0.0, 1.0]
    t, w = check_probs(p, label)
    assert t[1] == 1 and w[-3:].tolist() == [1, 0, 2]


def test_a_saturated_volume():
    C, S = 6, 40 * BLOCK + 12
    rng = np.random.default_rng(8)
    p = np.zeros((C, S), F)
    p[0] = 1.0
    label = np.zeros(S, F)
    where = np.flatnonzero(rng.random(S) < 0.01)                     # a sprinkled structure
    p[:, where] = probs(rng, C, where.size, 4.0)
    label[where] = rng.integers(0, C, where.size)
    t, _ = check_probs(p, label)
    head, top, cls, logh = CB.split(t, C)
    assert head[0] == S and top[19, 0] > 0.98 * S and logh[4064] > 0.98 * S and cls[1, 0, 0] > 0.98 * S


# ---- LOGITS against PROBS, device against device ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,scale,special", [(6, 3.0, False), (6, 6.0, True), (9, 6.0, True)])
def test_logits_equal_probs_of_an_ensemble_state_of_one_member(C, scale, special):
    S = BLOCK + 5 * CB.UNIT + 4
    rng = np.random.default_rng(int(C * scale))
    x = (rng.standard_normal((C, S)) * scale).astype(F)
    label, mask = labels(rng, C, S), np.ones(S, np.uint8)
    plant(rng, probs(rng, C, S), label, mask)                        # the labels and the mask only
    if special:
        at = np.flatnonzero(rng.random(S) < 0.2)
        x[rng.integers(0, C, at.size), at] = -INF
        x[0, 5], x[1, 13], x[:, 21], x[C - 1, 40] = NAN, INF, -INF, NAN
        label[[5, 13, 21, 40]], mask[[5, 13, 21, 40]] = 0.0, 1
    results = []
    for by in (0, 4):                                                # aligned pointers, and every pointer 4 bytes past a 16-byte boundary
        d_x, d_l = offset(dev(x), by), offset(dev(label), by)
        d_m = offset(dev(mask), by // 4)
        state = offset(EN.new_state(C, S, DEV).view(torch.float32), by)
        assert d_x.data_ptr() % 16 == by and d_l.data_ptr() % 16 == by and state.data_ptr() % 16 == by
        EN.accumulate(d_x.view(C, 1, 1, S), state, 1.0, True)
        for impl in IMPLS:
            for rep in range(2):
                a_t, a_w = run(d_x, CB.SRC_LOGITS, C, S, d_l, d_m, impl, rep, shift=by // 4)
                b_t, b_w = run(state, CB.SRC_PROBS, C, S, d_l, d_m, impl, rep, shift=by // 4)
                assert same(a_t, b_t), (by, impl, rep, np.argwhere(a_t != b_t)[:8].tolist())
                assert same(a_w, b_w), (by, impl, rep)
                results.append((a_t, a_w))
    assert all(same(t, results[0][0]) and same(w, results[0][1]) for t, w in results)      # both load widths, every impl
    head = results[0][0][:4]
    assert head.sum() == S and head[0] > 0 and (head[1] >= 4 if special else head[1] == 0)
    # and the state's planes through the restatement
    planes = state[:C * S].cpu().numpy().reshape(C, S)
    want_t, want_w = calib_ref(planes, label, mask)
    assert same(results[0][0], want_t) and same(results[0][1], want_w)


# ---- LOGITS on exact data against calib_ref -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [3, 6, 11])
def test_logits_on_exact_data(C):
    S = BLOCK + 4 * CB.UNIT + 3
    rng = np.random.default_rng(50 + C)
    x = rng.choice(np.asarray([0.0, -200.0, -INF], F), (C, S), p=[0.4, 0.3, 0.3])
    x[:, 9] = -INF                                                   # a bad voxel for certain
    label, mask = labels(rng, C, S), (rng.random(S) < 0.9).astype(np.uint8)
    label[9], mask[9] = 1.0, 1
    planes, bad = softmax_exact(x)
    assert bad[9] and not ((planes > 0) & (planes < F(1.2e-38))).any()          # no subnormals anywhere
    want_t, want_w = calib_ref(planes, label, mask, bad)
    d_x, d_l, d_m = dev(x), dev(label), dev(mask)
    for impl in IMPLS:
        for rep in range(2):
            t, w = run(d_x, CB.SRC_LOGITS, C, S, d_l, d_m, impl, rep)
            assert same(t, want_t), (impl, rep, np.argwhere(t != want_t)[:8].tolist())
            assert same(w, want_w), (impl, rep)
    assert want_t[1] >= 1 and want_t[0] > S // 2


# ---- further checks --------------------------------------------------------------------------------------------------------------------
def test_accumulate_adds_and_a_null_wrong_writes_nothing():
    C, S = 6, BLOCK + 11
    rng = np.random.default_rng(9)
    inputs = []
    for k in range(2):
        p, label = probs(rng, C, S), labels(rng, C, S)
        plant(rng, p, label, None)
        inputs.append((dev(p), dev(label), calib_ref(p, label)[0]))
    for impl in IMPLS:
        tb, out = guarded_table(CB.table_len(C), 0)
        out.zero_()
        for d_p, d_l, _ in inputs:
            CB.tables_from_probs(d_p, C, S, d_l, out=out, accumulate=True, impl=impl)
        assert same(out.cpu().numpy(), inputs[0][2] + inputs[1][2]) and guards_intact(tb, CB.table_len(C), GUARD)
        # without the byte map the table is the same
        t, w = run(inputs[0][0], CB.SRC_PROBS, C, S, inputs[0][1], None, impl, 1, want_wrong=False)
        assert w is None and same(t, inputs[0][2])
    with pytest.raises(U.UNetError, match="accumulate needs"):
        CB.tables_from_probs(inputs[0][0], C, S, inputs[0][1], accumulate=True)
    with pytest.raises(U.UNetError, match="out must hold"):
        CB.tables_from_probs(inputs[0][0], C, S, inputs[0][1], out=torch.empty(5, dtype=torch.int64, device=DEV))
    with pytest.raises(U.UNetError, match="label holds"):
        CB.tables_from_probs(inputs[0][0], C, S, inputs[0][1][:-1])


def test_the_byte_map_through_uncertainty_hists_equals_hist_ref():
    C, S = 4, BLOCK + 77
    rng = np.random.default_rng(10)
    p, label = probs(rng, C, S, 1.5), labels(rng, C, S)
    plant(rng, p, label, None)
    wrong = torch.empty(S, dtype=torch.uint8, device=DEV)
    CB.tables_from_probs(dev(p), C, S, dev(label), wrong=wrong)
    w = wrong.cpu().numpy()
    assert same(w, calib_ref(p, label)[1]) and (w == 1).any() and (w == 2).any() and (w == 0).any()
    with np.errstate(invalid="ignore", divide="ignore"):
        q = np.where(p > 0, p, F(1))
        umap = -(q * np.log(q)).sum(axis=0).astype(F)                # any float32 map will do; this one has NaNs where p has
    hi = float(np.log(C))
    hc, hw = CB.uncertainty_hists(wrong, dev(umap), 0.0, hi)
    want = hist_ref(w, umap, 2, 0.0, hi)
    assert same(hc.cpu().numpy(), want[1]) and same(hw.cpu().numpy(), want[2])
    assert 0.0 <= CB.auroc(hc, hw) <= 1.0


SMOKE_ARCH = ("conv8,ks3,stride1+norm,leaky_relu+conv8,ks3,stride1+norm,leaky_relu\n"
              "conv16,ks3,stride2+norm,leaky_relu+conv16,ks3,stride1+norm,leaky_relu+conv_trans8,ks2,stride2\n"
              "conv8,ks3,stride1+norm,leaky_relu+conv8,ks3,stride1+norm,leaky_relu+conv%d,ks1,stride1")


def test_calibration_qc_report_equals_the_composition_by_hand(tmp_path):
    dim, C = (16, 16, 16), 4
    W, H, D = dim
    S = W * H * D
    models = []
    for seed in (9, 10):
        m = U.UNet3d(1, C, SMOKE_ARCH % C, device=DEV, dtype="fp32", seed=seed)
        m.dim, m.voxel_size = dim, (1.0, 1.0, 1.0)
        m.prepare_for_inference()
        models.append(m)
    m, m2 = models
    g = torch.Generator().manual_seed(3)

    def vol(max_label):
        lab = torch.randint(0, max_label + 1, (D, H, W), generator=g).to(torch.float32)
        lab[torch.rand(D, H, W, generator=g) < 0.4] = 0.0
        lab.view(-1)[0] = max_label
        return torch.randn(1, D, H, W, generator=g).numpy(), lab.numpy()

    cases = [("/data/tpl/t0_T1w.nii.gz", "/data/tpl/t0_label.nii.gz") + vol(2) + (True,),
             ("/data/tpl/t1_T1w.nii.gz", "/data/tpl/t1_label.nii.gz") + vol(2) + (True,),
             ("/data/sub-01/anat/sub-01_T1w.nii.gz", "/data/sub-01/anat/sub-01_dseg.nii.gz") + vol(1) + (False,)]     # 1 < 2, 1 + 2 < 4: shifted
    assert Q.label_plan(cases, C)[1] == [False, False, True]
    path = str(tmp_path / "qc_model.nz")
    report = str(tmp_path / "qc_model.calibration_report.tsv")
    ln_c = float(np.log(C))
    for kw in (dict(), dict(bins=5, mask="foreground"), dict(ensemble=[m2]), dict(ensemble=[m2], ensemble_weights=[3.0, 1.0], mask="foreground", bins=20)):
        assert Q.calibration_qc(m, path, cases, **kw) == (0, report)
        got = open(report, "rb").read()
        assert sorted(os.listdir(tmp_path)) == ["qc_model.calibration_report.tsv"]      # no .tmp left behind
        # by hand through the public functions on second forwards of the same models: the engine's fp32 forward is deterministic
        bins, ens = kw.get("bins", 10), "ensemble" in kw
        total = torch.zeros(CB.table_len(C), dtype=torch.int64, device=DEV)
        hists = [torch.zeros(256, dtype=torch.int64, device=DEV) for _ in range(2)]
        rows = []
        for case in cases[:2]:
            x = torch.from_numpy(case[2]).view(1, 1, D, H, W).to(DEV)
            t = torch.from_numpy(case[3]).view(-1).to(DEV)
            if ens:
                ws = EN.normalize_weights(kw.get("ensemble_weights"), 2)
                state = EN.new_state(C, S, DEV)
                for k, member in enumerate(models):
                    EN.accumulate(member._forward_level0(x), state, ws[k], k == 0)
                planes = state[:C * S * 4].view(torch.float32).view(C, S)
            else:
                logits = m._forward_level0(x)
                planes = logits[0].view(C, S)
            mask = None
            if kw.get("mask") == "foreground":
                mask = ((torch.trunc(t) != 0) | (torch.argmax(planes, dim=0) != 0)).to(torch.uint8)
            if ens:
                wrong = torch.empty(S, dtype=torch.uint8, device=DEV)
                table = CB.tables_from_probs(state, C, S, t, mask=mask, wrong=wrong)
                entropy = EN.finalize(state, C, (D, H, W), outputs=("entropy",))["entropy"]
                h = CB.uncertainty_hists(wrong, entropy, 0.0, ln_c)
                hists[0] += h[0]
                hists[1] += h[1]
            else:
                table, h = CB.tables(planes, t, mask=mask), None
            total += table
            rows.append((case[0], case[1], Q.calibration_scores(table, C, bins, h)))
        rows.append((cases[2][0], cases[2][1], None))
        rows.append(("total", "", Q.calibration_scores(total, C, bins, tuple(hists) if ens else None)))
        assert Q.format_calibration_report(C, rows, ens).encode() == got
        lines = got.decode().splitlines()
        width = 6 + 2 * C + (2 if ens else 0)
        assert len(lines) == 5 and lines[0].split("\t")[:4] == ["image", "ground_truth", "voxels", "accuracy"]
        assert lines[3].split("\t") == ["sub-01_T1w.nii.gz", "sub-01_dseg.nii.gz"] + ["N/A"] * width
        assert "N/A" not in lines[1] + lines[2] + lines[4] and lines[4].startswith("total\t\t")
        voxels = [int(l.split("\t")[2]) for l in (lines[1], lines[2], lines[4])]
        assert voxels[2] == voxels[0] + voxels[1] and (0 < voxels[0] <= S if "mask" in kw else voxels[0] == S)
        assert lines[0].endswith("aurc_entropy") == ens
    bad = [cases[0][:2] + (cases[0][2][:, :8], cases[0][3], True)]
    assert Q.calibration_qc(m, path, bad) == (1, "/data/tpl/t0_T1w.nii.gz: training data dimension mismatch")
    assert Q.calibration_qc(m, path, cases, ensemble=[m2], ensemble_weights=[1.0]) == (1, "ensemble_weights: 1 weights for 2 members")
