"""GPU: quality control (qc.cpp) on the engine.  The counting kernel (include/unet_qc.h) against a torch-CPU restatement of
qc.cpp:86-135 and shift_subject_label (train.cpp:248-256) -- integer counts, demanded equal -- then calculate_qc end to end, and
qc() over a saved model with several worker threads."""
import math
import os
import threading

import pytest
import torch

import unet_studio_amd as U
from unet_studio_amd import qc as Q
from oracle import aten_ref as A

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

SMOKE_ARCH = ("conv8,ks3,stride1+norm,leaky_relu+conv8,ks3,stride1+norm,leaky_relu\n"
              "conv16,ks3,stride2+norm,leaky_relu+conv16,ks3,stride1+norm,leaky_relu+conv_trans8,ks2,stride2\n"
              "conv8,ks3,stride1+norm,leaky_relu+conv8,ks3,stride1+norm,leaky_relu+conv%d,ks1,stride1")


def ref_counts(logits, label, k=0, image0=None, shift_by=0):
    """qc.cpp:86-135 (+ train.cpp:248-256 when shift_by > 0) in torch on the CPU: logits {C, S}, label {S} -> [voxels[C'], wrong[C']]"""
    logits, label = logits.cpu(), label.cpu().reshape(-1)
    C, S = logits.shape[0], label.numel()
    if shift_by > 0:
        label = torch.where(label != 0, label + float(shift_by), (image0.cpu().reshape(-1)[:S] > 0).to(torch.float32))
    t = label.to(torch.int64)
    valid = t.ge(0).logical_and(t.lt(C))
    lg = logits.reshape(1, C, S)
    cp = C
    if k:
        lg = torch.cat([torch.logsumexp(lg[:, :k], 1, True), lg[:, k:]], 1)
        t = torch.clamp_min(t - k + 1, 0)
        cp = C - k + 1
    bins = torch.where(valid, t.clamp(0, cp - 1), torch.full_like(t, cp))
    wrong = lg.argmax(1)[0].ne(t).logical_and(valid)
    return torch.cat([torch.bincount(bins, minlength=cp + 1)[:cp], torch.bincount(bins[wrong], minlength=cp + 1)[:cp]]).tolist()


def near_ties(logits, k, gap):
    """voxels whose merged candidate lse(l_0..l_{k-1}) lies within `gap` of the largest other candidate"""
    if not k or k == logits.shape[0]:
        return torch.zeros(logits.shape[1], dtype=torch.bool)
    lse = torch.logsumexp(logits[:k].double(), 0)
    rest = logits[k:].double().max(0).values
    return (lse - rest).abs() < gap


def make_case(C, S, k, shift, seed):
    g = torch.Generator().manual_seed(seed)
    lg = torch.randn(C, S, generator=g) * 3
    if C > 1 and S > 1:
        # exact ties between channels, and NaNs
        idx = torch.randperm(S, generator=g)[: max(1, S // 8)]
        a, b = torch.randint(0, C, (2,), generator=g).tolist()
        lg[b, idx] = lg[a, idx]
        lg[C - 1, idx[::3]] = lg[0, idx[::3]]
        nan = torch.randperm(S, generator=g)[: max(1, S // 50)]
        lg[torch.randint(0, C, (nan.numel(),), generator=g), nan] = float("nan")
    # collapse: keep voxels off the lse / other-logit rounding boundary
    for _ in range(100):
        bad = near_ties(lg, k, 1e-3)
        if not bad.any():
            break
        lg[:, bad] = torch.randn(C, int(bad.sum()), generator=g) * 3
    assert not near_ties(lg, k, 1e-3).any()
    lab = torch.randint(-2, C + 3, (S,), generator=g).to(torch.float32)
    frac = torch.rand(S, generator=g) < 0.15
    lab[frac] = torch.rand(int(frac.sum()), generator=g) * (C + 3) - 1.5    # non-integers, in [-1.5, C + 1.5)
    lab[: min(S, 2)] = torch.tensor([2.7, -0.5])[: min(S, 2)]
    if shift:
        lab[torch.rand(S, generator=g) < 0.3] = 0.0
    img = torch.randn(S, generator=g)
    return lg, lab, img


def _unaligned(t):
    """a copy of t at a base address 4 bytes past a 16-B boundary"""
    buf = torch.empty(t.numel() + 4, dtype=t.dtype, device=DEV)
    assert buf.data_ptr() % 16 == 0
    out = buf[1:1 + t.numel()].view(t.shape)
    out.copy_(t)
    assert out.data_ptr() % 16 == 4
    return out


CASES = [(C, k) for C in (1, 2, 6, 33, 130) for k in sorted({0, 1, 2, C - 1}) if 0 <= k < C]


@pytest.mark.parametrize("S", [1, 7, 4099, 64 ** 3])
@pytest.mark.parametrize("C,k", CASES)
def test_counts_equal_the_torch_restatement(C, k, S):
    for shift in (0, 5):
        lg, lab, img = make_case(C, S, k, shift, seed=C * 1000 + k * 10 + shift + S)
        exp = ref_counts(lg, lab, k, img, shift)
        d_lg, d_lab, d_img = lg.to(DEV), lab.to(DEV), img.to(DEV)
        got = Q.qc_counts(d_lg, d_lab, k, d_img if shift else None, shift)
        assert got.dtype == torch.uint64 and got.cpu().tolist() == exp, (C, k, S, shift)
        assert sum(exp[: len(exp) // 2]) > 0 or S < 8
        if S % 4 == 0 or S == 4099:   # every base pointer unaligned (the scalar path where the aligned run took the 16-B one)
            got = Q.qc_counts(_unaligned(d_lg), _unaligned(d_lab), k, _unaligned(d_img) if shift else None, shift)
            assert got.cpu().tolist() == exp, ("unaligned", C, k, S, shift)


@pytest.mark.parametrize("k", [0, 1])
def test_counts_with_more_classes_than_the_lds_histogram(k):
    """C' > 4096: the per-block histogram lives in the block's own scratch column"""
    C, S = 5000, 4099
    lg, lab, _ = make_case(C, S, k, 0, seed=77 + k)
    lab = torch.where(torch.rand(S) < 0.5, torch.zeros(S), lab)
    assert Q.qc_counts(lg.to(DEV), lab.to(DEV), k).cpu().tolist() == ref_counts(lg, lab, k)


def test_counts_are_written_not_accumulated_and_abi_errors():
    C, S, k = 6, 4096, 2
    lg, lab, img = make_case(C, S, k, 5, seed=5)
    exp = ref_counts(lg, lab, k, img, 5)
    d_lg, d_lab, d_img = lg.to(DEV), lab.to(DEV), img.to(DEV)
    need = Q.qc_scratch_bytes(C, S, k)
    scratch = torch.full((need,), 0xAB, dtype=torch.uint8, device=DEV)
    counts = torch.full((len(exp),), -1, dtype=torch.int64, device=DEV)   # every bit set
    st = torch.cuda.current_stream().cuda_stream
    lib = U.engine.lib

    def call(collapse=k, image0=d_img.data_ptr(), shift=5, nbytes=need):
        return lib.unet_qc_counts(d_lg.data_ptr(), d_lab.data_ptr(), image0, C, S, collapse, shift, counts.data_ptr(),
                                  scratch.data_ptr(), nbytes, st)
    for _ in range(2):
        assert call() == 0
        assert counts.cpu().tolist() == exp
    err = lambda: lib.unet_last_error().decode()
    assert call(collapse=C) != 0 and err() == "invalid collapse_before"
    assert call(collapse=-1) != 0 and err() == "invalid collapse_before"
    assert call(image0=None) != 0 and "image0" in err()
    assert call(nbytes=need - 1) != 0 and "scratch too small" in err()
    assert lib.unet_qc_counts(d_lg.data_ptr(), d_lab.data_ptr(), None, C, 0, 0, 0, counts.data_ptr(), scratch.data_ptr(), need, st) != 0
    assert "voxels" in err()
    with pytest.raises(U.UNetError, match="^invalid collapse_before$"):
        Q.qc_counts(d_lg, d_lab, C)
    assert counts.cpu().tolist() == exp        # failed calls launch nothing


def test_two_threads_on_two_streams_match_the_sequential_results():
    probs = [make_case(33, 64 ** 3, 2, 5, seed=11), make_case(6, 96 ** 3, 0, 0, seed=12)]
    args = [(lg.to(DEV), lab.to(DEV), 2 if i == 0 else 0, img.to(DEV), 5 if i == 0 else 0) for i, (lg, lab, img) in enumerate(probs)]
    seq = [Q.qc_counts(a[0], a[1], a[2], a[3], a[4]).cpu().tolist() for a in args]
    assert seq[0] == ref_counts(probs[0][0], probs[0][1], 2, probs[0][2], 5)
    torch.cuda.synchronize()
    out, errs = [None, None], []

    def run(i):
        try:
            s = torch.cuda.Stream(DEV)
            scratch = torch.empty(Q.qc_scratch_bytes(args[i][0].shape[0], args[i][1].numel()), dtype=torch.uint8, device=DEV)
            with torch.cuda.stream(s):
                res = [Q.qc_counts(*args[i], scratch=scratch) for _ in range(8)]
                out[i] = [r.cpu().tolist() for r in res]
        except Exception as e:   # reported by the main thread
            errs.append(e)
    th = [threading.Thread(target=run, args=(i,)) for i in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errs, errs
    for i in range(2):
        assert all(r == seq[i] for r in out[i])


# ---- calculate_qc end to end ----------------------------------------------------------------------------------------------
def _model(which, dt, dim):
    if which == "smoke":
        m = U.UNet3d(1, 6, SMOKE_ARCH % 6, device=DEV, dtype=dt, seed=4)
    else:
        m = U.UNet3d(1, 6, U.default_feature(6), device=DEV, dtype=dt, seed=4)
    m.dim = dim
    m.prepare_for_inference()
    return m


def _volume(m, seed):
    W, H, D = m.dim
    g = torch.Generator().manual_seed(seed)
    img = torch.randn(m.in_count, D, H, W, generator=g)
    lab = torch.randint(-1, m.out_count + 2, (D, H, W), generator=g).to(torch.float32)
    lab[torch.rand(D, H, W, generator=g) < 0.1] = 2.7
    lab[torch.rand(D, H, W, generator=g) < 0.3] = 0.0
    return img, lab


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("which,dim", [("smoke", (32, 32, 32)), ("smoke", (20, 12, 28)), ("default", (32, 32, 32)),
                                       ("default", (32, 64, 96))])
def test_calculate_qc_end_to_end(which, dim, dt):
    m = _model(which, dt, dim)
    W, H, D = dim
    img, lab = _volume(m, seed=sum(dim))
    x = img.view(1, 1, D, H, W).to(DEV)
    full = m.forward(x)[0]
    lvl0 = m._forward_level0(x)
    assert torch.equal(lvl0, full), "level-0-only forward differs from forward()[0]"
    lg = full[0].reshape(6, -1).cpu()
    for k, shift in ((0, 0), (0, 2), (3, 2), (1, 0)):
        ties = int(near_ties(lg, k, 1e-4 * float(lg.abs().max())).sum())
        stats, overall = U.calculate_qc(m, img.numpy() if k % 2 == 0 else img.to(DEV), lab.numpy(), k, shift)
        exp_stats, exp_overall = Q.stats_from_counts(ref_counts(lg, lab, k, img[0], shift), 6, k)
        if not ties:
            assert stats == exp_stats and overall == exp_overall, (k, shift)
        else:   # an argmax may flip only where lse and another logit differ by rounding
            assert [s.voxels for s in stats] == [s.voxels for s in exp_stats]
            assert sum(abs(a.wrong - b.wrong) for a, b in zip(stats, exp_stats)) <= ties
    # torch's InstanceNorm3d refuses a one-voxel level, which the default architecture reaches at 32^3 (the engine does not)
    if dt == "fp32" and math.prod(d >> (5 if which == "default" else 1) for d in dim) > 1:
        # against the ATen executor in float64: the label bins are equal; a wrong count may move only by the voxels whose two largest
        # fp64 logits lie within 1e-4 of the largest logit magnitude (fp32 engine vs fp64: < 1e-5 relative, test_gpu_parity)
        ref = A.UNet3dRef(1, 6, m.architecture)
        with torch.no_grad():
            for p, q in zip(ref.parameters(), m.parameters()):
                p.copy_(q.cpu())
        ref = ref.double()
        ref.prepare_for_inference()
        with torch.no_grad():
            r = ref(img.view(1, 1, D, H, W).double())[0][0].reshape(6, -1)
        top2 = r.topk(2, 0).values
        slack = int(((top2[0] - top2[1]).abs() < 1e-4 * float(r.abs().max())).sum())
        exp_stats, _ = Q.stats_from_counts(ref_counts(r, lab), 6)
        stats, _ = U.calculate_qc(m, img.numpy(), lab.numpy())
        assert [s.voxels for s in stats] == [s.voxels for s in exp_stats]
        assert sum(abs(a.wrong - b.wrong) for a, b in zip(stats, exp_stats)) <= slack, slack


def test_calculate_qc_errors():
    m = _model("smoke", "fp32", (16, 16, 16))
    img, lab = _volume(m, 1)
    with pytest.raises(U.UNetError, match="^training data dimension mismatch$"):
        U.calculate_qc(m, img.numpy()[:, :8], lab.numpy())
    with pytest.raises(U.UNetError, match="^training data dimension mismatch$"):
        U.calculate_qc(m, img.numpy(), lab.numpy()[:8])
    with pytest.raises(U.UNetError, match="^invalid collapse_before$"):
        U.calculate_qc(m, img.numpy(), lab.numpy(), 6)


# ---- qc() over a saved model ------------------------------------------------------------------------------------------------
def _qc_cases(dim, seed):
    W, H, D = dim
    g = torch.Generator().manual_seed(seed)

    def vol(max_label, p_zero=0.4):
        lab = torch.randint(0, max_label + 1, (D, H, W), generator=g).to(torch.float32)
        lab[torch.rand(D, H, W, generator=g) < p_zero] = 0.0
        lab.view(-1)[0] = max_label
        return torch.randn(1, D, H, W, generator=g).numpy(), lab.numpy()
    cases = []
    for i in range(3):                                  # templates: max_template_label = 2
        im, lb = vol(2)
        cases.append(("/data/tpl/t%d_T1w.nii.gz" % i, "/data/tpl/t%d_label.nii.gz" % i, im, lb, True))
    im, lb = vol(1)                                     # 1 < 2, 1 + 2 < 6: shifted (collapse_before 3, shift_by 2)
    cases.append(("/data/sub-01/anat/sub-01_T1w.nii.gz", "/data/sub-01/anat/sub-01_dseg.nii.gz", im, lb, False))
    im, lb = vol(4)                                     # 4 is not below 2: not shifted
    cases.append(("/data/sub-02/anat/sub-02_T1w.nii.gz", "/data/sub-02/anat/sub-02_dseg.nii.gz", im, lb, False))
    return cases


def test_qc_report_from_threads_equals_one_thread_and_per_case_rows(tmp_path):
    dim = (24, 16, 20)
    m = U.UNet3d(1, 6, SMOKE_ARCH % 6, device=DEV, dtype="bf16", seed=9)
    m.dim = dim
    path = str(tmp_path / "qc_model.nz")
    assert U.save_to_file(m, path)
    cases = _qc_cases(dim, 3)
    mtl, shift = Q.label_plan(cases, 6)
    assert mtl == 2 and shift == [False, False, False, True, False]
    report = str(tmp_path / "qc_model.error_report.tsv")
    assert Q.qc(path, cases, device=DEV, thread_count=4) == (0, report)
    four = open(report, "rb").read()
    assert Q.qc(path, cases, device=DEV, thread_count=1) == (0, report)
    one = open(report, "rb").read()
    assert four == one
    assert sorted(os.listdir(tmp_path)) == ["qc_model.error_report.tsv", "qc_model.nz"]     # no .tmp left behind
    # the same rows from per-case calculate_qc on the same loaded, prepared model
    r = U.load_from_file(path, device=DEV, dtype="bf16")
    r.prepare_for_inference()
    rows = []
    for c, sh in zip(cases, shift):
        collapse, shift_by = Q.case_settings(sh, mtl)
        stats, overall = U.calculate_qc(r, c[2], c[3], collapse, shift_by)
        rows.append((c[0], c[1], stats, overall, collapse))
    assert Q.format_report(6, rows).encode() == four
    lines = four.decode().splitlines()
    assert len(lines) == 6 and lines[4].split("\t")[:2] == ["sub-01_T1w.nii.gz", "sub-01_dseg.nii.gz"]
    assert lines[4].split("\t")[3:6] == ["N/A"] * 3 and "N/A" not in lines[5]


def test_qc_failure_names_the_image_and_writes_no_report(tmp_path):
    dim = (16, 16, 16)
    m = U.UNet3d(1, 6, SMOKE_ARCH % 6, device=DEV, dtype="fp32", seed=9)
    m.dim = dim
    path = str(tmp_path / "m.nz")
    assert U.save_to_file(m, path)
    cases = _qc_cases(dim, 4)
    name, lname, im, lb, tpl = cases[3]
    cases[3] = (name, lname, im[:, :8], lb, tpl)          # the wrong size
    rc, msg = Q.qc(path, cases, device=DEV, thread_count=4)
    assert rc == 1 and msg == "/data/sub-01/anat/sub-01_T1w.nii.gz: training data dimension mismatch"
    assert sorted(os.listdir(tmp_path)) == ["m.nz"]
    # a model with one output class is refused
    m1 = U.UNet3d(1, 1, SMOKE_ARCH % 1, device=DEV, dtype="fp32", seed=9)
    p1 = str(tmp_path / "m1.nz")
    assert U.save_to_file(m1, p1)
    assert Q.qc(p1, cases, device=DEV) == (1, "QC requires a categorical model")
