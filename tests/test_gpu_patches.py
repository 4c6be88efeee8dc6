"""GPU: the patch feed (include/unet_patches.h) -- the index and the pick against the numpy restatement of
tests/patches_ref.py, bit for bit; the crop against the numpy slice as int32 views, inside poisoned buffers; WindowFeed against
TrainingFeed on cases that fit, against the tail applied by hand to the predicted numpy slice on larger canvases, and under Trainer."""
import numpy as np
import pytest
import torch

import patches_ref as R
import unet_studio_amd as U
from gpu_exact import Guarded
from unet_studio_amd import augment as G
from unet_studio_amd import feed as FD
from unet_studio_amd import patches as P

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# one voxel, a segment less one / exactly / plus one, several segments with a ragged tail, more segments than one round of the prefix
SIZES = [1, 1023, 1024, 1025, 4099, 1024 * 1024 + 7]
CLASSES = [0, 1, 2, 8, 256]


def _at(a, offset):
    """a device copy of the float32 array that starts `offset` floats into its allocation (16-B aligned for offset 0 only)"""
    a = torch.as_tensor(np.asarray(a, dtype=np.float32))
    buf = torch.empty(a.numel() + offset + 4, device=DEV)
    v = buf[offset:offset + a.numel()]
    v.copy_(a.reshape(-1).to(DEV))
    return v.view(a.shape)


def _labels(n, K, kind, seed):
    g = np.random.RandomState(seed)
    top = K if K else 3
    if kind == "int":
        return g.randint(0, top, n).astype(np.float32)
    if kind == "mixed":      # fractional and negative values, NaN, infinities and values >= K
        l = (g.rand(n) * (top + 6) - 3).astype(np.float32)
        l[g.rand(n) < 0.1] = np.nan
        l[g.rand(n) < 0.05] = 1e30
        l[g.rand(n) < 0.05] = -np.inf
        return l
    if kind == "ends":       # a class present only at the first voxel, and one present only at the last
        l = np.zeros(n, np.float32)
        l[0] = 1.0
        l[-1] = float(max(top - 1, 1)) if n > 1 else l[0]
        return l
    l = g.randint(0, top, n).astype(np.float32)      # "absent": a class with no voxel at all
    l[l == float(min(3, top - 1))] = 0.0
    return l


# ---- the index -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", [0, 1, 3])
@pytest.mark.parametrize("kind", ["int", "mixed", "ends", "absent"])
def test_index_equals_bincount_per_segment(kind, offset):
    for n in SIZES:
        for K in CLASSES:
            l0 = _labels(n, K, kind, n + K)
            lab = _at(l0, offset)
            idx = P.index(lab, K)
            Kn, S = P.index_layout(n, K)
            assert idx.dtype == torch.int32 and idx.numel() == Kn + Kn * S and S == (n + 1023) // 1024
            tot, pre = R.index_ref(l0, K)
            got = idx.cpu().numpy().astype(np.int64)
            assert np.array_equal(got[:Kn], tot), (n, K, kind)
            assert np.array_equal(got[Kn:].reshape(Kn, S), pre), (n, K, kind)
            assert np.array_equal(lab.cpu().numpy().view(np.int32), l0.view(np.int32))      # the label is only read


def test_index_into_a_poisoned_buffer_and_argument_errors():
    n, K = 4099, 8
    lab = _at(_labels(n, K, "mixed", 1), 1)
    Kn, S = P.index_layout(n, K)
    out = Guarded((Kn + Kn * S,), torch.int32, 0)
    out.t.fill_(-77)
    P.index(lab, K, out=out.t)
    out.check("index", finite=False)
    tot, pre = R.index_ref(lab.cpu().numpy(), K)
    assert np.array_equal(out.t.cpu().numpy(), np.concatenate([tot, pre.reshape(-1)]))
    with pytest.raises(U.UNetError, match="at least"):
        P.index(lab, K, out=out.t[:-1])
    with pytest.raises(U.UNetError, match="float32 device tensor"):
        P.index(lab.double(), K)
    with pytest.raises(U.UNetError, match="classes must be in"):
        P.index(lab, 300)


# ---- the pick --------------------------------------------------------------------------------------------------------------------
CANVASES = [(13, 11, 9), (33, 17, 19)]      # (W, H, D): 2 and 11 segments, the last one short


def _canvas_label(dims, K, seed, absent=None):
    W, H, D = dims
    g = np.random.RandomState(seed)
    l = g.randint(0, K, W * H * D).astype(np.float32)
    l[g.rand(l.size) < 0.05] = np.nan
    l[g.rand(l.size) < 0.05] = float(K + 1)
    l[g.rand(l.size) < 0.05] = -2.5
    if absent is not None:
        l[l == float(absent)] = 0.0
    return l.reshape(D, H, W)


def _pick_all(lab, idx, K, picks, window):
    rows = [P.pick(lab, idx, K, picks[i:i + 32], window) for i in range(0, len(picks), 32)]
    return torch.cat(rows).cpu().numpy().astype(np.int64)


@pytest.mark.parametrize("dims", CANVASES)
def test_every_rank_of_every_class_finds_its_voxel(dims):
    W, H, D = dims
    K = 4
    l0 = _canvas_label(dims, K, 5)
    lab = _at(l0, 1)
    idx = P.index(lab, K)
    cm = R.class_map(l0, K)
    lowest, highest, want = [], [], []
    for c in range(K):
        hits = np.flatnonzero(cm == c)
        n = hits.size
        assert n > 0
        for r in range(n):
            lo, hi = R.u_for(r, n), R.u_for(r + 1, n) - 1       # the smallest and the largest draw that reach rank r
            assert (lo * n) >> 32 == r == (hi * n) >> 32 and hi < 2 ** 32
            lowest.append((c, lo, 0, 0, 0))
            highest.append((c, hi, 0, 0, 0))
            want.append(int(hits[r]))
    want = np.array(want)
    # a window of one voxel: the origin is the centre itself
    got = _pick_all(lab, idx, K, lowest, (1, 1, 1))
    assert (got[:, 3] == 1).all()
    assert np.array_equal((got[:, 2] * H + got[:, 1]) * W + got[:, 0], want)
    sub = list(range(0, len(want), 7)) + [len(want) - 1]
    got = _pick_all(lab, idx, K, [highest[i] for i in sub], (1, 1, 1))
    assert np.array_equal((got[:, 2] * H + got[:, 1]) * W + got[:, 0], want[sub])


@pytest.mark.parametrize("dims", CANVASES)
def test_origins_equal_the_restated_rules(dims):
    W, H, D = dims
    K = 5
    l0 = _canvas_label(dims, K, 9, absent=4)
    lab = _at(l0, 3)
    idx = P.index(lab, K)
    cm = R.class_map(l0, K)
    g = np.random.RandomState(3)
    edge = [0, 2 ** 32 - 1]
    # a general window, one equal to the canvas on one axis, one equal to it on all axes, and a window of one voxel
    for window in [(3, 4, 5), (3, 4, W), (3, H, 5), (D, 4, 5), (D, H, W), (1, 1, 1)]:
        td, th, tw = window
        picks = []
        for cls in [-1, 0, 1, 2, 3, 4, 7, -5]:                 # 4: absent; 7 and -5: no class of this index -> the uniform rule
            for _ in range(6):
                picks.append((cls, int(g.randint(0, 2 ** 32, dtype=np.uint64)),) + tuple(int(g.randint(0, 2 ** 32, dtype=np.uint64)) for _ in range(3)))
            for ux in edge:
                for uy in edge:
                    for uz in edge:
                        picks.append((cls, edge[(ux ^ uy) & 1], ux, uy, uz))
        got = _pick_all(lab, idx, K, picks, window)
        for pk, row in zip(picks, got):
            cls = pk[0] if 0 <= pk[0] < K else -1
            assert tuple(row) == R.pick_ref(cm, dims, (tw, th, td), (cls,) + pk[1:]), (window, pk)
            assert 0 <= row[0] <= W - tw and 0 <= row[1] <= H - th and 0 <= row[2] <= D - td
        flags = {p[0]: int(r[3]) for p, r in zip(picks, got)}
        assert flags == {-1: 0, 0: 1, 1: 1, 2: 1, 3: 1, 4: 0, 7: 0, -5: 0}
        # one pick per launch gives the rows of 32 per launch
        for i in (0, 13, len(picks) - 1):
            assert np.array_equal(P.pick(lab, idx, K, [picks[i]], window).cpu().numpy()[0], got[i])


def test_continuous_labels_and_a_stale_index():
    dims = (13, 11, 9)
    W, H, D = dims
    g = np.random.RandomState(2)
    l0 = (g.rand(D, H, W).astype(np.float32) - 0.7)          # class 1 where l > 0
    l0[0, 0, 0] = np.nan
    lab = _at(l0, 0)
    idx = P.index(lab, 0)
    cm = R.class_map(l0, 0)
    picks = [(c, int(g.randint(0, 2 ** 32, dtype=np.uint64)), 0, 2 ** 31, 2 ** 32 - 1) for c in (0, 1, -1, 2) for _ in range(8)]
    got = _pick_all(lab, idx, 0, picks, (3, 4, 5))
    for pk, row in zip(picks, got):
        assert tuple(row) == R.pick_ref(cm, dims, (5, 4, 3), ((pk[0] if pk[0] < 2 else -1),) + pk[1:])
    # an index of another label: class 1 is gone from the volume the pick reads; the centre is the first voxel of the segment the
    # index points to, flag 0, and the call returns
    ones = _at(np.ones((D, H, W), np.float32), 0)
    stale = P.index(ones, 2)
    zeros = _at(np.zeros((D, H, W), np.float32), 0)
    n = W * H * D
    got = _pick_all(zeros, stale, 2, [(1, R.u_for(5, n), 0, 0, 0), (1, R.u_for(1030, n), 0, 0, 0)], (1, 1, 1))
    assert got.tolist() == [[0, 0, 0, 0], [1024 % W, 1024 // W % H, 1024 // (W * H), 0]]


# ---- the crop --------------------------------------------------------------------------------------------------------------------
def _bits(shape, seed):
    """random bit patterns as float32: NaN payloads, infinities and denormals included"""
    return np.random.RandomState(seed).randint(-2 ** 31, 2 ** 31, size=shape, dtype=np.int64).astype(np.int32).view(np.float32)


def _origin(*words):
    return torch.tensor(words, dtype=torch.int32, device=DEV)


@pytest.mark.parametrize("with_lab", [True, False])
@pytest.mark.parametrize("tw", [5, 16, 17])
@pytest.mark.parametrize("in_count", [1, 2])
def test_crop_equals_the_numpy_slice_bit_for_bit(in_count, tw, with_lab):
    W, H, D = 23, 9, 7
    th, td = 4, 3
    img0, lab0 = _bits((in_count, D, H, W), 1), _bits((D, H, W), 2)
    for src_off in (0, 1):
        img, lab = _at(img0, src_off), _at(lab0, (src_off + 2) % 4)
        for ox, oy, oz in [(0, 0, 0), (1, 5, 4), (2, 3, 1), (3, 1, 2), (W - tw, H - th, D - td)]:     # every residue of x mod 4
            x = Guarded((in_count, td, th, tw), torch.float32)
            l = Guarded((td, th, tw), torch.float32)
            gx, gl = P.crop(img, lab if with_lab else None, _origin(ox, oy, oz), (td, th, tw), out=(x.t, l.t if with_lab else None))
            x.check("crop x", finite=False)
            l.check("crop lab", finite=False)
            assert gx.data_ptr() == x.t.data_ptr() and (gl is None) == (not with_lab)
            want = img0[:, oz:oz + td, oy:oy + th, ox:ox + tw]
            assert np.array_equal(x.t.cpu().numpy().view(np.int32), want.view(np.int32)), (ox, oy, oz)
            if with_lab:
                assert np.array_equal(l.t.cpu().numpy().view(np.int32), lab0[oz:oz + td, oy:oy + th, ox:ox + tw].view(np.int32))
            else:
                assert torch.isnan(l.t).all()            # untouched
    assert np.array_equal(img.cpu().numpy().view(np.int32), img0.view(np.int32))


def test_crop_into_a_destination_that_is_not_16_byte_aligned():
    W, H, D, tw, th, td = 23, 9, 7, 16, 4, 3
    img0, lab0 = _bits((1, D, H, W), 3), _bits((D, H, W), 4)
    img, lab = _at(img0, 0), _at(lab0, 0)
    n = td * th * tw
    buf = torch.full((2 * n + 64,), -3.0, device=DEV)
    x, l = buf[1:1 + n], buf[n + 7:2 * n + 7]
    P.crop(img, lab, _origin(3, 2, 1), (td, th, tw), out=(x, l))
    assert np.array_equal(x.cpu().numpy().view(np.int32), img0[0, 1:1 + td, 2:2 + th, 3:3 + tw].reshape(-1).view(np.int32))
    assert np.array_equal(l.cpu().numpy().view(np.int32), lab0[1:1 + td, 2:2 + th, 3:3 + tw].reshape(-1).view(np.int32))
    rest = torch.cat([buf[:1], buf[1 + n:n + 7], buf[2 * n + 7:]])
    assert (rest == -3.0).all()


@pytest.mark.parametrize("tw", [16, 5])
def test_crop_clamps_whatever_the_origin_words_hold(tw):
    W, H, D, th, td = 23, 9, 7, 4, 3
    V = W * H * D
    img0, lab0 = _bits((2, D, H, W), 5), _bits((D, H, W), 6)
    # the canvas inside a larger allocation filled with a sentinel: a missing clamp on x or y reads other values
    big = torch.full((3 * V + 4096,), 12345.0, device=DEV)
    img = big[2048:2048 + 2 * V].view(2, D, H, W)
    lab = big[2048 + 2 * V:2048 + 3 * V].view(D, H, W)
    img.copy_(torch.as_tensor(img0))
    lab.copy_(torch.as_tensor(lab0))
    x, l = P.crop(img, lab, _origin(-5, H, 2 ** 30), (td, th, tw))
    ox, oy, oz = 0, H - th, D - td
    assert np.array_equal(x.cpu().numpy().view(np.int32), img0[:, oz:oz + td, oy:oy + th, ox:ox + tw].view(np.int32))
    assert np.array_equal(l.cpu().numpy().view(np.int32), lab0[oz:oz + td, oy:oy + th, ox:ox + tw].view(np.int32))
    x, _ = P.crop(img, None, _origin(2 ** 31 - 1, -2 ** 31, -1), (td, th, tw))
    assert np.array_equal(x.cpu().numpy().view(np.int32), img0[:, 0:td, 0:th, W - tw:W].view(np.int32))
    with pytest.raises(U.UNetError, match="must fit the canvas"):
        P.crop(img, lab, _origin(0, 0, 0), (td, th, W + 1))
    with pytest.raises(U.UNetError, match="int32 device tensor"):
        P.crop(img, lab, torch.zeros(3, device=DEV), (td, th, tw))


# ---- WindowFeed --------------------------------------------------------------------------------------------------------------------
ARCH = ("conv8,ks3,stride1+norm,leaky_relu+conv8,ks3,stride1+norm,leaky_relu\n"
        "conv16,ks3,stride2+norm,leaky_relu+conv16,ks3,stride1+norm,leaky_relu+conv_trans8,ks2,stride2\n"
        "conv8,ks3,stride1+norm,leaky_relu+conv8,ks3,stride1+norm,leaky_relu+conv8,ks1,stride1")
N = 16
OPTS = dict(G.DEFAULT_OPTIONS, rubber_stamping=4, perlin_texture=4, distortion=4, zero_background=0)


def _model():
    m = U.UNet3d(1, 8, ARCH, device=DEV, dtype="fp32", seed=0)
    m.dim = (N, N, N)
    return m


def _blobs(max_label, seed, shape):
    """blobs of labels 1..max_label on a background of 0 in a {d, h, w} volume, and the image that goes with them"""
    g = torch.Generator().manual_seed(seed)
    d, h, w = shape
    z, y, x = torch.meshgrid(torch.arange(d, dtype=torch.float32), torch.arange(h, dtype=torch.float32),
                             torch.arange(w, dtype=torch.float32), indexing="ij")
    lab = torch.zeros(shape)
    for k in range(1, max_label + 1):
        c = torch.rand(3, generator=g) * (torch.tensor([d, h, w]) - 6) + 3
        lab[((z - c[0]) ** 2 + (y - c[1]) ** 2 + (x - c[2]) ** 2) < 9 + k] = float(k)
    img = (torch.rand((1,) + tuple(shape), generator=g) * 0.5 + lab / (max_label + 1)).clamp(0, 1) * (lab > 0).float()
    return (img + 0.05 * torch.rand((1,) + tuple(shape), generator=g)).contiguous(), lab.contiguous()


def _cases(spec):
    """spec: (name, max label, is_template, shape {d, h, w}); with max template label 3 and 8 classes a subject of max 1 or 2 is shifted"""
    out = []
    for i, (name, ml, tpl, shape) in enumerate(spec):
        img, lab = _blobs(ml, 10 + i, shape)
        out.append((name + ".nii.gz", name + "_label.nii.gz", img.to(DEV), lab.to(DEV), tpl))
    return out


FIT = [("t0", 3, True, (N, N, N)), ("s0", 1, False, (N, N, N)), ("t1", 2, True, (N, N, N)), ("s1", 2, False, (N, N, N)),
       ("s2", 3, False, (N, N, N))]
LARGE = [("t0", 3, True, (16, 24, 40)), ("s0", 1, False, (48, 16, 16)), ("t1", 2, True, (48, 16, 16)), ("s1", 3, False, (16, 24, 40))]


def test_cases_that_fit_give_the_samples_of_training_feed():
    m = _model()
    cases = _cases(FIT)
    param = U.TrainingParam(batch_size=4, seed=3)
    a = U.TrainingFeed(m, cases, param, OPTS)
    b = U.WindowFeed(m, cases, param, OPTS)
    assert b.max_template_label == a.max_template_label == 3 and b.has_subject_data and b.shifted == a.shifted == [False, True, False, True, False]
    kinds = set()
    for i in range(8):
        assert b.sample_info(i) == a.sample_info(i) and b.case_index(i) == a.case_index(i)
        kinds.add(a.sample_info(i))
        (xa, ta), (xb, tb) = a(i), b(i)
        assert xb.shape == (1, 1, N, N, N) and tb.shape == (1, N, N, N) and tb.dtype == torch.int64
        assert torch.equal(xa, xb) and torch.equal(ta, tb), i
        assert b.window(i)[0].cpu().tolist()[:3] == [0, 0, 0]
    assert (True, False) in kinds and (False, True) in kinds           # templates and a shifted subject were drawn
    for (xa, ta), (xb, tb) in zip(zip(*a.test_set()), zip(*b.test_set())):
        assert torch.equal(xa, xb) and torch.equal(ta, tb)
    with pytest.raises(U.UNetError, match="smaller than the model"):
        U.WindowFeed(m, _cases([("t", 2, True, (N, N, N - 1))]), param, OPTS)


@pytest.fixture(scope="module")
def large():
    """a feed over canvases of 40 x 24 x 16 and 16 x 16 x 48, and per case what numpy says of it"""
    m = _model()
    cases = _cases(LARGE)
    param = U.TrainingParam(batch_size=4, seed=21)
    feed = U.WindowFeed(m, cases, param, OPTS)
    assert feed.max_template_label == 3 and feed.shifted == [False, True, False, False]
    ref = []
    for i, c in enumerate(cases):
        img, lab = c[2].cpu().numpy(), c[3].cpu().numpy()
        cm = R.class_map(lab, 8)
        prep = np.where(lab != 0, lab + np.float32(3), (img[0] > 0).astype(np.float32)) if feed.shifted[i] else lab
        ref.append(dict(img=img, lab=lab, cm=cm, prep=prep.astype(np.float32), fg=[k for k in range(1, 8) if (cm == k).any()],
                        dims=lab.shape[::-1]))
        assert feed.fg_classes[i] == ref[i]["fg"] and feed.totals[i] == np.bincount(cm, minlength=8).tolist()
    return m, cases, param, feed, ref


def _predict(feed, ref, param, index):
    r = ref[feed.case_index(index)]
    pk = R.decide(param.seed, index, r["fg"])
    return r, pk, R.pick_ref(r["cm"], r["dims"], (N, N, N), pk)


def test_windows_and_samples_equal_the_restatement_on_large_canvases(large):
    m, cases, param, feed, ref = large
    seen = set()
    for index in range(16):
        r, pk, (ox, oy, oz, flag) = _predict(feed, ref, param, index)
        is_template, _ = feed.sample_info(index)
        seen.add((feed.case_index(index), flag))
        origin, xr, lr = feed.window(index)
        assert origin.is_cuda and origin.cpu().tolist() == [ox, oy, oz, flag], index
        sl = (slice(oz, oz + N), slice(oy, oy + N), slice(ox, ox + N))
        assert np.array_equal(xr.cpu().numpy()[0], r["img"][(slice(None),) + sl]) and np.array_equal(lr.cpu().numpy(), r["prep"][sl])
        if flag:      # a forced sample: the chosen voxel lies in the window, where the restatement says, and holds the chosen class
            hits = np.flatnonzero(r["cm"] == pk[0])
            c = int(hits[(pk[1] * hits.size) >> 32])
            W, H, _ = r["dims"]
            px, py, pz = c % W - ox, c // W % H - oy, c // (W * H) - oz
            assert 0 <= px < N and 0 <= py < N and 0 <= pz < N
            shift = 3 if feed.shifted[feed.case_index(index)] else 0
            assert float(lr[pz, py, px]) == float(pk[0] + shift)
        # the tail by hand on the numpy slice
        x = torch.from_numpy(np.ascontiguousarray(r["img"][(slice(None),) + sl])).to(DEV).view(1, 1, N, N, N)
        l = torch.from_numpy(np.ascontiguousarray(r["prep"][sl])).to(DEV)
        G.simulate(G.make_simulate_recipe((N, N, N), m.out_count if is_template else None, index), x.view(-1),
                   l.view(-1) if is_template else None)
        G.augment(G.make_recipe(OPTS, (N, N, N), 1, True, index, label_depth=N), x.view(-1), l.view(-1))
        xf, tf = feed(index)
        assert torch.equal(xf, x) and torch.equal(tf, FD.target(l).view(1, N, N, N)), index
    assert len({c for c, _ in seen}) == 4 and {f for _, f in seen} == {0, 1}      # every case, forced and uniform windows
    for c, r in zip(cases, ref):                                                  # the caller's arrays are never written
        assert np.array_equal(c[2].cpu().numpy(), r["img"]) and np.array_equal(c[3].cpu().numpy(), r["lab"])


def test_a_sample_is_a_function_of_its_index_on_any_stream(large):
    m, cases, param, feed, _ = large
    ref = [feed(i) for i in range(6)]
    fresh = U.WindowFeed(m, cases, param, OPTS)
    side = torch.cuda.Stream(DEV)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        x, t = fresh(5)                       # the first request of a fresh feed, on a second stream
    side.synchronize()
    assert torch.equal(x, ref[5][0]) and torch.equal(t, ref[5][1])
    x, t = feed(5)
    assert torch.equal(x, ref[5][0]) and torch.equal(t, ref[5][1])


def test_test_set_is_every_window_of_the_overlap_free_plan(large):
    m, cases, param, feed, ref = large
    test_in, test_out = feed.test_set()
    k = 0
    for i in FD.choose_test_cases(cases):
        r = ref[i]
        for ox, oy, oz in P.test_windows(r["dims"], (N, N, N)):
            sl = (slice(oz, oz + N), slice(oy, oy + N), slice(ox, ox + N))
            assert np.array_equal(test_in[k].cpu().numpy()[0], r["img"][(slice(None),) + sl])
            assert np.array_equal(test_out[k].cpu().numpy()[0], r["lab"][sl].astype(np.int64))
            k += 1
    assert k == len(test_in) == len(test_out) == 6 + 3          # 3 x 2 x 1 windows of 40 x 24 x 16, 1 x 1 x 3 of 16 x 16 x 48


def test_to_canvas_equals_to_model_space_when_the_scan_fits_and_covers_a_larger_one():
    m = _model()
    g = torch.Generator().manual_seed(4)
    img, lab = torch.rand(1, 12, 14, 10, generator=g), torch.randint(0, 4, (12, 14, 10), generator=g).float()
    ia, la = U.to_model_space(m, img.numpy(), (1.0, 1.0, 1.0), lab.numpy())
    ib, lb = U.to_canvas(m, img.numpy(), (1.0, 1.0, 1.0), lab.numpy())
    assert torch.equal(ia, ib) and torch.equal(la, lb) and tuple(lb.shape) == (N, N, N)
    img, lab = torch.rand(1, 20, 12, 30, generator=g), torch.randint(0, 4, (20, 12, 30), generator=g).float()
    ic, lc = U.to_canvas(m, img.numpy(), (1.0, 1.5, 1.0), lab.numpy())
    assert tuple(lc.shape) == U.canvas_dims(m.dim, m.voxel_size, (30, 12, 20), (1.0, 1.5, 1.0))[::-1] == (20, 18, 30)
    assert tuple(ic.shape) == (1, 20, 18, 30) and float(ic.max()) == 1.0
    assert set(lc.unique().cpu().tolist()) <= {0.0, 1.0, 2.0, 3.0}
    U.WindowFeed(m, [("a", "b", ic, lc, True)], U.TrainingParam(batch_size=2, seed=0), OPTS)(0)


class _Listed:
    """a source that returns tensors made earlier, with what Trainer asks a feed"""

    def __init__(self, feed, n):
        self.samples = [feed(i) for i in range(n)]
        self.infos = [feed.sample_info(i) for i in range(n)]
        self.max_template_label, self.has_subject_data = feed.max_template_label, feed.has_subject_data

    def __call__(self, index):
        return self.samples[index]

    def sample_info(self, index):
        return self.infos[index]


def test_a_trainer_step_over_the_feed_equals_one_over_the_same_tensors(monkeypatch):
    monkeypatch.delenv("UNET_MICRO_IN_FLIGHT", raising=False)
    param = U.TrainingParam(batch_size=6, epoch=100, learning_rate=0.05, seed=21)
    cases = _cases(LARGE)
    ma, mb = _model(), _model()
    fa = U.WindowFeed(ma, cases, param, OPTS)
    ta = U.Trainer(ma, param, fa)
    tb = U.Trainer(mb, param, _Listed(U.WindowFeed(mb, cases, param, OPTS), 6))
    infos = [fa.sample_info(i) for i in range(6)]
    assert any(s for _, s in infos) and any(t for t, _ in infos)          # a shifted subject (collapsed classes) and a template
    sa, sb = ta.step().clone(), tb.step().clone()
    torch.cuda.synchronize()
    assert torch.equal(sa, sb) and torch.equal(ma.flat_params, mb.flat_params)
    assert ta.record_errors() == tb.record_errors() and len(ma.training_errors) == 3
