"""GPU: the template/subject training feed (train.cpp:229-486,612-752) -- the three feed kernels (include/unet_feed.h) against a torch
restatement of read_label_info / tipl::normalize / shift_subject_label / .to(kLong), TrainingFeed against the manual composition of
its parts, and one mixed template/subject step of Trainer against a hand-written sequence and the ATen restatement."""
import numpy as np
import pytest
import torch

import unet_studio_amd as U
from oracle import aten_ref as A
from unet_studio_amd import augment as G
from unet_studio_amd import feed as FD

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# sizes below / at / above the 4-wide vector, a ragged tail, more voxels than one block, more blocks than the grid cap
SIZES = [1, 3, 4, 5, 1023, 4099, 16 * 16 * 16, 1024 * 1024 + 7]


def _labels(n, kind, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    if kind == "int":
        return torch.randint(0, 7, (n,), generator=g).to(torch.float32)
    if kind == "frac":       # negative and fractional values, both signs of truncation
        return (torch.rand(n, generator=g) * 15 - 5).to(torch.float32)
    if kind == "zero":
        return torch.zeros(n)
    return -torch.rand(n, generator=g) * 3 - 0.25     # "neg": every value negative (max < 0, normalize does nothing)


def _at(t, offset):
    """a device copy of t that starts `offset` floats into its allocation (16-B aligned for offset 0 only)"""
    buf = torch.empty(t.numel() + offset + 4, device=DEV)
    v = buf[offset:offset + t.numel()]
    v.copy_(t.to(DEV))
    return v


def ref_max(l):            # read_label_info: tipl::image<3,int> (toward zero), tipl::max_value
    return int(torch.trunc(l).max())


def ref_normalize(l):      # tipl::normalize: l / max(l) when max > 0
    m = l.max()
    return l / m if float(m) > 0 else l.clone()


def ref_shift(l, img, shift):   # shift_subject_label (train.cpp:248-257), in float
    return torch.where(l != 0, l + float(shift), (img > 0).to(torch.float32))


@pytest.mark.parametrize("offset", [0, 1, 3])
@pytest.mark.parametrize("kind", ["int", "frac", "zero", "neg"])
def test_label_max_equals_read_label_info(kind, offset):
    for n in SIZES:
        l = _at(_labels(n, kind, n), offset)
        got = FD.label_max(l)
        assert got.dtype == torch.int32 and got.is_cuda
        assert int(got.cpu()) == ref_max(l.cpu()), (n, kind, offset)


@pytest.mark.parametrize("offset", [0, 1, 2])
@pytest.mark.parametrize("normalize,shift", [(0, 0), (1, 0), (0, 3), (1, 3)])
@pytest.mark.parametrize("kind", ["int", "frac", "zero", "neg"])
def test_prepare_equals_normalize_then_shift(kind, normalize, shift, offset):
    for n in SIZES:
        l0 = _labels(n, kind, n + 1)
        img = torch.rand(n, generator=torch.Generator().manual_seed(n)) - 0.3     # some voxels <= 0
        l, im = _at(l0, offset), _at(img, (offset + 1) % 4)
        mx = torch.full((1,), -7, dtype=torch.int32, device=DEV)
        FD.prepare(l, im if shift else None, normalize=normalize, shift_by=shift, label_max_out=mx)
        want = ref_normalize(l0) if normalize else l0.clone()
        if shift:
            want = ref_shift(want, img, shift)
        assert torch.equal(l.cpu(), want), (n, kind)
        assert int(mx.cpu()) == ref_max(l0)
        assert torch.equal(im.cpu(), img)   # image0 is only read


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("normalize", [0, 1])
@pytest.mark.parametrize("kind", ["int", "frac", "zero", "neg"])
def test_target_equals_to_klong(kind, normalize, offset):
    for n in SIZES:
        l0 = _labels(n, kind, n + 2)
        l = _at(l0, offset)
        out = torch.empty(n + 1, dtype=torch.int64, device=DEV)[offset:offset + n]    # 8-B aligned, 16-B only at offset 0
        FD.target(l, normalize=normalize, out=out)
        want = (ref_normalize(l0) if normalize else l0).to(torch.int64)
        assert torch.equal(out.cpu(), want), (n, kind)
        assert torch.equal(l.cpu(), l0)


def test_two_streams_with_separate_scratch_run_at_once():
    n = 2 * 1024 * 1024 + 5
    ls = [_labels(n, "frac", s) for s in (1, 2)]
    img = torch.rand(n) - 0.5
    streams = [torch.cuda.Stream(DEV) for _ in range(2)]
    scratch = [torch.empty(FD.feed_scratch_bytes(n), dtype=torch.uint8, device=DEV) for _ in range(2)]
    dl = [l.to(DEV) for l in ls]
    di = img.to(DEV)
    tg, mx = [None, None], [None, None]
    torch.cuda.synchronize()
    for rep in range(3):       # the two streams' launches interleave
        for k in range(2):
            with torch.cuda.stream(streams[k]):
                if rep == 0:
                    mx[k] = FD.label_max(dl[k], scratch=scratch[k])
                elif rep == 1:
                    FD.prepare(dl[k], di, normalize=True, shift_by=2 + k, scratch=scratch[k])
                else:
                    tg[k] = FD.target(dl[k], normalize=True, scratch=scratch[k])
    torch.cuda.synchronize()
    for k in range(2):
        want = ref_shift(ref_normalize(ls[k]), img, 2 + k)
        assert int(mx[k].cpu()) == ref_max(ls[k])
        assert torch.equal(dl[k].cpu(), want)
        assert torch.equal(tg[k].cpu(), ref_normalize(want).to(torch.int64))


def test_argument_errors():
    l = torch.zeros(16, device=DEV)
    with pytest.raises(U.UNetError, match="needs input channel 0"):
        FD.prepare(l, None, shift_by=2)
    lib, st = U.engine.lib, torch.cuda.current_stream(DEV).cuda_stream
    mx = torch.empty(1, dtype=torch.int32, device=DEV)
    sc = torch.empty(FD.feed_scratch_bytes(16), dtype=torch.uint8, device=DEV)
    assert lib.unet_feed_label_max(l.data_ptr(), 16, mx.data_ptr(), sc.data_ptr(), 8, st) != 0       # the wrappers grow scratch
    assert b"scratch too small" in lib.unet_last_error()
    assert lib.unet_feed_prepare(None, l.data_ptr(), 16, 0, -1, None, sc.data_ptr(), sc.numel(), st) != 0
    assert b"shift_by must not be negative" in lib.unet_last_error()
    assert lib.unet_feed_target(l.data_ptr(), 0, 0, mx.data_ptr(), sc.data_ptr(), sc.numel(), st) != 0
    assert b"voxels must be positive" in lib.unet_last_error()
    with pytest.raises(U.UNetError, match="float32 device tensor"):
        FD.label_max(l.double())


# ---- TrainingFeed ---------------------------------------------------------------------------------------------------------------
ARCH = ("conv8,ks3,stride1+norm,leaky_relu+conv8,ks3,stride1+norm,leaky_relu\n"
        "conv16,ks3,stride2+norm,leaky_relu+conv16,ks3,stride1+norm,leaky_relu+conv_trans8,ks2,stride2\n"
        "conv8,ks3,stride1+norm,leaky_relu+conv8,ks3,stride1+norm,leaky_relu+conv8,ks1,stride1")
N = 16
OPTS = dict(G.DEFAULT_OPTIONS, rubber_stamping=4, perlin_texture=4, distortion=4, zero_background=0)


def _sphere_label(max_label, seed, n=N):
    """blobs of labels 1..max_label on a background of 0, and the image that goes with them"""
    g = torch.Generator().manual_seed(seed)
    z, y, x = torch.meshgrid(*(torch.arange(n, dtype=torch.float32),) * 3, indexing="ij")
    lab = torch.zeros(n, n, n)
    for k in range(1, max_label + 1):
        c = torch.rand(3, generator=g) * (n - 6) + 3
        lab[((z - c[0]) ** 2 + (y - c[1]) ** 2 + (x - c[2]) ** 2) < 9 + k] = float(k)
    img = (torch.rand(1, n, n, n, generator=g) * 0.5 + lab / (max_label + 1)).clamp(0, 1) * (lab > 0).float()
    img = img + 0.05 * torch.rand(1, n, n, n, generator=g)
    return img, lab


def _cases(on_device):
    """two templates with max label 3, two shifted subjects (max 1 and 2 < 3, + 3 < 8) and one unshifted subject (max 3)"""
    spec = [("t0", 3, True), ("s0", 1, False), ("t1", 2, True), ("s1", 2, False), ("s2", 3, False)]
    out = []
    for i, (name, ml, tpl) in enumerate(spec):
        img, lab = _sphere_label(ml, 10 + i, N + (2 if name == "t1" else 0))
        img, lab = img[:, :N, :N, :N].contiguous(), lab[:N, :N, :N].contiguous()
        if on_device:
            img, lab = img.to(DEV), lab.to(DEV)
        else:
            img, lab = img.numpy(), lab.numpy()
        out.append((name + ".nii.gz", name + "_label.nii.gz", img, lab, tpl))
    return out


def _model(dt="fp32"):
    m = U.UNet3d(1, 8, ARCH, device=DEV, dtype=dt, seed=0)
    m.dim = (N, N, N)
    return m


def _manual(feed, m, cases, index):
    """prepare -> simulate -> augment -> target, composed by hand from the public pieces"""
    i = feed.case_index(index)
    _, _, img, lab, is_template = cases[i]
    x = torch.as_tensor(img).to(DEV, torch.float32).clone().view(1, 1, N, N, N)
    l = torch.as_tensor(lab).to(DEV, torch.float32).clone()
    if not is_template and feed.shifted[i]:
        FD.prepare(l, x.view(-1), shift_by=feed.max_template_label)
    G.simulate(G.make_simulate_recipe((N, N, N), m.out_count if is_template else None, index), x.view(-1),
               l.view(-1) if is_template else None)
    G.augment(G.make_recipe(OPTS, (N, N, N), 1, True, index, label_depth=N), x.view(-1), l.view(-1))
    return x, FD.target(l).view(1, N, N, N)


@pytest.mark.parametrize("on_device", [True, False])
def test_feed_equals_the_manual_composition_and_leaves_the_inputs_alone(on_device):
    m = _model()
    cases = _cases(on_device)
    keep = [(np.array(torch.as_tensor(c[2]).cpu()), np.array(torch.as_tensor(c[3]).cpu())) for c in cases]
    param = U.TrainingParam(batch_size=4, seed=3)
    feed = U.TrainingFeed(m, cases, param, OPTS)
    assert feed.max_template_label == 3 and feed.has_subject_data
    assert feed.shifted == [False, True, False, True, False]
    seen = set()
    for index in range(24):
        is_template, is_shifted = feed.sample_info(index)
        assert is_template == (index % 4 < 2)                       # seed_id % batch_size < n_template
        seen.add(feed.case_index(index))
        x, t = feed(index)
        xm, tm = _manual(feed, m, cases, index)
        assert x.shape == (1, 1, N, N, N) and t.shape == (1, N, N, N) and t.dtype == torch.int64
        assert torch.equal(x, xm) and torch.equal(t, tm), index
    assert {0, 2} <= seen and len(seen) >= 4                      # both templates and subjects were drawn
    torch.cuda.synchronize()
    for c, (img, lab) in zip(cases, keep):
        assert np.array_equal(np.array(torch.as_tensor(c[2]).cpu()), img) and np.array_equal(np.array(torch.as_tensor(c[3]).cpu()), lab)
    # the test set: the two largest templates (equal bytes here: descending index), as read, int64
    test_in, test_out = feed.test_set()
    assert len(test_in) == 2
    for x, t, i in zip(test_in, test_out, (2, 0)):
        assert torch.equal(x.cpu().view(-1), torch.as_tensor(keep[i][0]).view(-1))
        assert torch.equal(t.cpu().view(-1), torch.as_tensor(keep[i][1]).view(-1).to(torch.int64))


def test_feed_resumed_at_an_epoch_and_prefetched_equal_a_fresh_feed():
    m = _model()
    cases = _cases(True)
    param = U.TrainingParam(batch_size=4, seed=11)
    a = U.TrainingFeed(m, cases, param, OPTS)
    ref = [a(i) for i in range(12)]
    b = U.TrainingFeed(m, cases, param, OPTS)                       # resumed at cur_epoch 2: the first request is seed_id 8
    for i in range(8, 12):
        x, t = b(i)
        assert torch.equal(x, ref[i][0]) and torch.equal(t, ref[i][1])
    p = U.PrefetchedVolumes(U.TrainingFeed(m, cases, param, OPTS))
    assert p.sample_info(5) == a.sample_info(5) and p.max_template_label == 3 and p.has_subject_data
    for i in range(12):
        x, t = p(i)
        assert torch.equal(x, ref[i][0]) and torch.equal(t, ref[i][1])
    torch.cuda.synchronize()


def test_feed_normalizes_image_labels_and_refuses_too_many_labels():
    m = _model()
    cases = _cases(True)
    feed = U.TrainingFeed(m, cases, U.TrainingParam(batch_size=4, seed=0), OPTS, is_label=False)
    for i in (0, 2):                                                # templates: prepared once, l / max(l) (train.cpp:415-416)
        assert torch.equal(feed._tpl_label[i], cases[i][3] / cases[i][3].max())
    x, t = feed(0)
    assert int(t.max()) <= 1 and int(t.min()) >= 0

    class Stand:   # what the feed reads of a model: 256 classes do not fit simulate_modality's label table
        in_count, out_count, dim = 1, 256, (N, N, N)

        def device(self):
            return torch.device(DEV)
    with pytest.raises(U.UNetError, match="simulate_modality"):
        U.TrainingFeed(Stand(), cases, U.TrainingParam(batch_size=4), OPTS)


# ---- the mixed step ---------------------------------------------------------------------------------------------------------------
def _mixed_trainer(dt="fp32", batch=6):
    m = _model(dt)
    param = U.TrainingParam(batch_size=batch, epoch=100, learning_rate=0.05, seed=5)
    feed = U.TrainingFeed(m, _cases(True), param, OPTS)
    return m, feed, U.Trainer(m, param, feed)


def test_mixed_step_equals_the_hand_written_sequence_and_counts_subjects_only(monkeypatch):
    monkeypatch.delenv("UNET_MICRO_IN_FLIGHT", raising=False)
    ma, feed, ta = _mixed_trainer()
    mb = _model()
    mb.create_optimizer(0.05)
    infos = [feed.sample_info(b) for b in range(6)]
    assert any(s for _, s in infos) and any(t for t, _ in infos) and any(not t and not s for t, s in infos)
    sa = ta.step().clone()
    # by hand: forward_backward per sample with collapse_before = 4 for shifted subjects, then the optimizer step of train.cpp:759-766
    for g in mb.optimizer.param_groups:
        g["lr"] = ta.lr_at(0)
    stats = torch.zeros(4, device=DEV)
    n_subj = 0
    for b in range(6):
        x, t = feed(b)
        is_template, is_shifted = infos[b]
        l = mb.forward_backward(x, t, collapse_before=4 if is_shifted else 0)
        if not is_template:
            stats += l
            n_subj += 1
    mb.optimizer.step(grad_scale=1.0 / 6, clip_norm=12.0)
    torch.cuda.synchronize()
    assert torch.equal(ma.flat_params, mb.flat_params)
    assert torch.equal(sa, stats)
    e = ta.record_errors()
    want = (stats.cpu()[1:4] / float(n_subj)).tolist()
    assert e == want and ma.training_errors == want
    # the same step with every shifted sample trained WITHOUT the collapse differs: the collapse is not vacuous
    mc = _model()
    mc.create_optimizer(0.05)
    for g in mc.optimizer.param_groups:
        g["lr"] = ta.lr_at(0)
    for b in range(6):
        mc.forward_backward(*feed(b))
    mc.optimizer.step(grad_scale=1.0 / 6, clip_norm=12.0)
    torch.cuda.synchronize()
    assert not torch.equal(mc.flat_params, mb.flat_params)


def test_mixed_step_with_two_micro_steps_in_flight_equals_the_sequential_one(monkeypatch):
    ma, _, ta = _mixed_trainer()
    mb, _, tb = _mixed_trainer()
    ta.in_flight, tb.in_flight = 2, 1
    for _ in range(2):
        sa, sb = ta.step().clone(), tb.step().clone()
        assert torch.allclose(sa, sb, rtol=1e-6, atol=1e-7)
        assert ta.record_errors() == pytest.approx(tb.record_errors(), rel=1e-6)
    torch.cuda.synchronize()
    assert ta._lanes is not None and tb._lanes is None
    assert torch.equal(ma.flat_params, mb.flat_params)


def test_templates_only_count_every_sample_and_no_counted_sample_appends_nothing():
    m = _model()
    cases = [c for c in _cases(True) if c[4]]
    param = U.TrainingParam(batch_size=3, epoch=100, learning_rate=0.05, seed=1)
    feed = U.TrainingFeed(m, cases, param, OPTS)
    assert not feed.has_subject_data
    tr = U.Trainer(m, param, feed)
    s = tr.step().clone()
    assert len(tr.record_errors()) == 3
    assert m.training_errors == pytest.approx((s.cpu()[1:4] / 3).tolist(), rel=1e-6)
    # a step whose samples are all templates while subject data exist: nothing counted, nothing appended (train.cpp:729-752)
    m2, feed2, tr2 = _mixed_trainer(batch=2)        # batch 2 = n_template: every seed_id is a template sample
    assert all(feed2.sample_info(b)[0] for b in range(2))
    tr2.step()
    assert tr2.record_errors() == [] and m2.training_errors == []


def test_mixed_fp32_step_against_the_aten_restatement():
    """the parameter change of one mixed step (per-sample collapse_before) against UNet3dRef in float64 + train_step_epilogue, within the
    fp32 small-net gradient bound of test_noncubic_network_against_live_aten (leaky_relu kinks: 1e-2 of the largest)"""
    m, feed, tr = _mixed_trainer()
    torch.manual_seed(0)
    ref = A.UNet3dRef(1, 8, ARCH)
    m.load_parameters([p.detach().numpy() for p in ref.parameters()])
    ref = ref.double()
    ref.train()
    p0 = m.flat_params.clone()
    samples = [(feed(b), feed.sample_info(b)) for b in range(6)]
    tr.step()
    opt = ref.create_optimizer(0.05)
    for (x, t), (is_template, is_shifted) in samples:
        outs = ref(x.cpu().double())
        loss, _ = A.deep_supervision_loss(outs, t.cpu(), 8, collapse_before=4 if is_shifted else 0)
        loss.backward()
    A.train_step_epilogue(ref, opt, 6, lr=tr.lr_at(0))
    want = torch.cat([p.detach().flatten() for p in ref.parameters()]).numpy() - p0.cpu().double().numpy()
    got = (m.flat_params - p0).cpu().double().numpy()
    e = np.abs(got - want).max() / np.abs(want).max()
    print("mixed fp32 step against ATen fp64: parameter change %.3g of the largest" % e)
    assert e < 1e-2
