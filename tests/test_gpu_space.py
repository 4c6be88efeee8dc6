"""GPU: the step between a scan's grid and the model's (include/unet_space.h, unet-studio_amd/space.py).

unet_space_resample against oracle.augment_ref (_affine, _locate, _trilinear, _majority, _norm: the definitions the augmentation's
sampler already shares with its restatement): LINEAR within 5e-6 of values in [0, 1] (the bound tests/test_gpu_augment.py uses for
the same sampler), MAJORITY labels equal -- the position arithmetic is the restatement's operation for operation, so there is no
tie allowance.  unet_space_postproc against an fp64 restatement (the fp32 logits interpolated in fp64 in the same a + t*(b - a)
form, then torch.softmax): the probability bound is measured in the test, 4 x the distance of a plain fp32 CPU evaluation of the
same formula from the fp64 one, never less than the 2e-6 tests/test_gpu_postproc.py grants the softmax alone.  Measured on an
MI355X (each test prints its figures): the fp32 CPU evaluation is 2.1e-7, 2.6e-7, 3.6e-7, 5.4e-7, 1.0e-6 from fp64 for C = 2, 3, 6, 33,
130 (bounds 2e-6, 2e-6, 2e-6, 2.15e-6, 4.1e-6), the kernel 2.1e-7, 2.8e-7, 4.1e-7, 4.4e-7, 7.8e-7; 0 to 20 of the 61600 inside voxels
lie within 1e-5 of a tie; the resampling sweep differs from the restatement by exactly 0.  Then fused = unfused bit for bit inside the model's field of view,
EvaluateUNet with NativeVolume entries against the manual sequence, and to_model_space's results as qc / feed cases."""
import threading

import numpy as np
import pytest
import torch

import unet_studio_amd as U
from unet_studio_amd import postproc as P
from unet_studio_amd import space as SP
from oracle import augment_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F = np.float32
GAP = 1e-5      # the tie rule of tests/test_gpu_postproc.py
LINEAR_TOL = 5e-6

SMOKE_ARCH = ("conv8,ks3,stride1+norm,leaky_relu+conv8,ks3,stride1+norm,leaky_relu\n"
              "conv16,ks3,stride2+norm,leaky_relu+conv16,ks3,stride1+norm,leaky_relu+conv_trans8,ks2,stride2\n"
              "conv8,ks3,stride1+norm,leaky_relu+conv8,ks3,stride1+norm,leaky_relu+conv%d,ks1,stride1")
MIX_ARCH = ("conv8,ks3,stride1+norm,elu+conv8,ks3,stride1+norm,leaky_relu\n"
            "conv16,ks3,stride2+norm,elu+conv16,ks3,stride1+norm,leaky_relu\n"
            "max_pool+conv16,ks3,stride1+norm,relu+upsample\n"
            "conv16,ks3,stride1+norm,leaky_relu+conv%d,ks1,stride1+conv_trans8,ks2,stride2\n"
            "conv8,ks3,stride1+norm,leaky_relu+conv%d,ks1,stride1")


# ---- the restatement -------------------------------------------------------------------------------------------------------------
def locate(map, dst_shape, src_shape):
    """oracle positions of every destination voxel in the source: (ok, fractions, lower, upper corners)"""
    D, H, W = dst_shape
    sd, sh, sw = src_shape
    x, y, z = R._grid(W, H, D)
    px, py, pz = R._affine(map, x, y, z)
    return R._locate(px, py, pz, sw, sh, sd)


def ref_resample(src, dst_shape, map, mode):
    loc = locate(map, dst_shape, src.shape[1:])
    fn = R._majority if mode == "majority" else R._trilinear
    return np.stack([fn(src[c], loc) for c in range(src.shape[0])]), loc[0]


def tri64(vol, loc):
    """R._trilinear's formula on float64 values (the fractions are the shared fp32 ones); outside -> 0"""
    ok, (tx, ty, tz), (x0, y0, z0), (x1, y1, z1) = loc
    tx, ty, tz = (t.astype(np.float64) for t in (tx, ty, tz))
    vol = vol.astype(np.float64)
    at = lambda x, y, z: vol[z, y, x]
    lerp = lambda t, a, b: a + t * (b - a)
    with np.errstate(invalid="ignore"):
        c00, c10 = lerp(tx, at(x0, y0, z0), at(x1, y0, z0)), lerp(tx, at(x0, y1, z0), at(x1, y1, z0))
        c01, c11 = lerp(tx, at(x0, y0, z1), at(x1, y0, z1)), lerp(tx, at(x0, y1, z1), at(x1, y1, z1))
        return lerp(tz, lerp(ty, c00, c10), lerp(ty, c01, c11))


def grid_map(dst_shape, dst_vs, src_shape, src_vs):
    """the model -> image map with dst as the model grid and src as the image; shapes are (d, h, w)"""
    return SP.model_to_image_map(dst_shape[::-1], dst_vs, src_shape[::-1], src_vs)


def dev_offset(a, offset, dtype=torch.float32):
    """a device copy of the numpy array a, or for a shape a buffer filled with 7, starting `offset` elements into its allocation:
    unaligned pointers"""
    shape = a.shape if isinstance(a, np.ndarray) else tuple(a)
    buf = torch.full((int(np.prod(shape)) + offset,), 7, dtype=dtype, device=DEV)
    v = buf[offset:].view(shape)
    if isinstance(a, np.ndarray):
        v.copy_(torch.from_numpy(a))
    return v


# ---- unet_space_resample ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["linear", "majority"])
def test_identity_and_integer_shifts_are_bit_exact(mode):
    rs = np.random.RandomState(1)
    src = rs.rand(2, 9, 11, 13).astype(F) if mode == "linear" else rs.randint(0, 5, (2, 9, 11, 13)).astype(F)
    d = torch.from_numpy(src).to(DEV)
    ident = (np.eye(3).reshape(9), np.zeros(3))
    assert np.array_equal(SP.resample(d, (9, 11, 13), ident, mode).cpu().numpy(), src)
    for sx, sy, sz in [(2, -1, 3), (-4, 0, 1), (0, 5, -2)]:
        got = SP.resample(d, (9, 11, 13), (np.eye(3).reshape(9), np.array([sx, sy, sz], F)), mode).cpu().numpy()
        exp = np.zeros_like(src)
        for z in range(9):
            for y in range(11):
                if 0 <= z + sz < 9 and 0 <= y + sy < 11:
                    lo, hi = max(0, -sx), min(13, 13 - sx)
                    exp[:, z, y, lo:hi] = src[:, z + sz, y + sy, lo + sx:hi + sx]
        assert np.array_equal(got, exp), (sx, sy, sz)


# (src shape, src voxel size, dst shape, dst voxel size, channels, flipped source axis or None, pointer offsets)
SWEEP = [
    ((20, 22, 24), (1, 1, 1), (24, 28, 24), (1, 1, 1), 1, None, 0),          # same scale, other size (align_top)
    ((37, 44, 40), (1.1, 1.0, 1.3), (24, 28, 24), (2, 2, 2), 2, None, 1),    # down-sampling, odd sizes
    ((12, 14, 12), (2, 2, 2), (37, 44, 40), (1.1, 1.0, 1.3), 3, None, 3),    # up-sampling
    ((19, 17, 23), (0.8, 1.2, 1.0), (16, 16, 16), (1, 1, 1), 1, 0, 0),       # flipped x
    ((19, 17, 23), (0.8, 1.2, 1.0), (15, 21, 9), (1.3, 0.7, 1.9), 2, 2, 2),  # flipped z, anisotropic both ways
    ((1, 17, 23), (1, 1, 1), (4, 16, 16), (1, 1, 1), 1, None, 0),            # 1-voxel source axis
    ((9, 1, 7), (1, 1, 1), (9, 1, 7), (1, 1, 1), 2, None, 1),                # 1-voxel axis on both sides
    ((5, 6, 1), (1, 1, 1), (5, 6, 3), (1, 1, 0.5), 1, None, 0),
    ((33, 35, 67), (1, 1, 1), (1, 1, 1), (30, 30, 30), 3, None, 0),          # one destination voxel
]


def sweep_map(case):
    sshape, svs, dshape, dvs, _, flip, _ = case
    m = grid_map(dshape, dvs, sshape, svs)
    if flip is not None:                                   # p' = (dim - 1) - p on that source axis (x, y, z order)
        f = np.eye(3)
        f[flip, flip] = -1
        t = np.zeros(3)
        t[flip] = sshape[::-1][flip] - 1
        m = SP.compose_map((f.reshape(9), t), m)
    return m


@pytest.mark.parametrize("k", range(len(SWEEP)))
def test_resample_sweep_against_the_restatement(k):
    sshape, _, dshape, _, ch, _, off = SWEEP[k]
    rs = np.random.RandomState(20 + k)
    m = sweep_map(SWEEP[k])
    img = rs.rand(ch, *sshape).astype(F)
    lab = rs.randint(0, 5, (ch,) + sshape).astype(F)
    for mode, src in (("linear", img), ("majority", lab)):
        exp, ok = ref_resample(src, dshape, m, mode)
        out = dev_offset((ch,) + dshape, off)
        got = SP.resample(dev_offset(src, off), dshape, m, mode, out=out).cpu().numpy()
        if mode == "linear":
            err = float(np.abs(got - exp).max())
            print("case %d linear: max |kernel - restatement| = %.3g, inside %.3f" % (k, err, ok.mean()))
            assert err <= LINEAR_TOL
        else:
            assert np.array_equal(got, exp), int((got != exp).sum())
        assert (got[:, ~ok] == 0).all()
    # normalize: the whole stacked buffer by its maximum
    exp, _ = ref_resample(img, dshape, m, "linear")
    mx = exp.max()
    sc = torch.empty(SP.space_scratch_bytes(int(np.prod(dshape)), ch) + off, dtype=torch.uint8, device=DEV)[off:]
    got = SP.resample(dev_offset(img, off), dshape, m, "linear", normalize=True, scratch=sc).cpu().numpy()
    if mx > 0:
        expn = R._norm(exp, mx)
        ulp = np.spacing(np.abs(expn).astype(F))
        print("case %d normalize: max %.9g, max |kernel - _norm| / ulp = %.3g" % (k, got.max(), float((np.abs(got - expn) / ulp).max())))
        assert got.max() == 1.0 and (np.abs(got - expn) <= ulp).all()
    else:
        assert (got == 0).all()


def test_normalize_of_a_buffer_without_a_positive_maximum_leaves_it():
    src = -np.random.RandomState(0).rand(1, 6, 6, 6).astype(F)
    ident = (np.eye(3).reshape(9), np.zeros(3))
    got = SP.resample(torch.from_numpy(src).to(DEV), (6, 6, 6), ident, "linear", normalize=True).cpu().numpy()
    assert np.array_equal(got, src)


def test_two_threads_on_two_streams():
    rs = np.random.RandomState(4)
    cases = []
    for k in (1, 2):
        sshape, _, dshape, _, ch, _, _ = SWEEP[k]
        src = torch.from_numpy(rs.rand(ch, *sshape).astype(F)).to(DEV)
        m = sweep_map(SWEEP[k])
        cases.append((src, dshape, m, SP.resample(src, dshape, m, "linear", normalize=True).clone()))
    torch.cuda.synchronize()
    bad = []

    def work(i):
        src, dshape, m, exp = cases[i]
        s = torch.cuda.Stream(DEV)
        sc = torch.empty(SP.space_scratch_bytes(int(np.prod(dshape)), src.shape[0]), dtype=torch.uint8, device=DEV)
        with torch.cuda.stream(s):
            for _ in range(20):
                got = SP.resample(src, dshape, m, "linear", normalize=True, scratch=sc)
                s.synchronize()
                if not torch.equal(got, exp):
                    bad.append(i)

    ts = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    [t.start() for t in ts]
    [t.join() for t in ts]
    assert not bad


def test_large_case_twice_the_same_bits():
    g = torch.Generator(device=DEV).manual_seed(0)
    src = torch.rand((1, 180, 256, 256), generator=g, device=DEV)
    lab = torch.randint(0, 6, (1, 180, 256, 256), generator=g, device=DEV).float()
    m = SP.model_to_image_map((192, 224, 192), (1, 1, 1), (256, 256, 180), (1, 1, 1.2))
    a = SP.resample(src, (192, 224, 192), m, "linear", normalize=True)
    b = SP.resample(src, (192, 224, 192), m, "linear", normalize=True)
    assert torch.equal(a, b) and float(a.max()) == 1.0 and float(a.min()) >= 0.0
    la, lb = SP.resample(lab, (192, 224, 192), m, "majority"), SP.resample(lab, (192, 224, 192), m, "majority")
    assert torch.equal(la, lb) and torch.equal(la, la.round()) and float(la.max()) == 5.0
    # one z-slab of it against the restatement (the whole volume is 8 M voxels of numpy gathers)
    loc = locate(m, (192, 224, 192), (180, 256, 256))
    sl = tuple(v[100:104] for v in (loc[0],)) + (tuple(t[100:104] for t in loc[1]), tuple(i[100:104] for i in loc[2]),
                                                  tuple(i[100:104] for i in loc[3]))
    raw = SP.resample(src, (192, 224, 192), m, "linear")
    assert float(np.abs(raw[0, 100:104].cpu().numpy() - R._trilinear(src[0].cpu().numpy(), sl)).max()) <= LINEAR_TOL
    assert np.array_equal(la[0, 100:104].cpu().numpy(), R._majority(lab[0].cpu().numpy(), sl))


# ---- unet_space_postproc ---------------------------------------------------------------------------------------------------------
MODEL_SHAPE, MODEL_VS = (24, 28, 24), (2, 2, 2)                  # (d, h, w); 2 mm
NATIVE_SHAPE, NATIVE_VS = (37, 44, 40), (1.1, 1.0, 1.3)          # part of it lies outside the model's field of view


def back_map():
    """native voxel -> model position"""
    return SP.invert_map(grid_map(MODEL_SHAPE, MODEL_VS, NATIVE_SHAPE, NATIVE_VS))


def make_logits(C, seed, special=False):
    g = torch.Generator().manual_seed(seed)
    lg = torch.randn((C,) + MODEL_SHAPE, generator=g) * 3
    if special:
        inf = float("inf")
        lg[0, 5, 6, 7] = float("nan")
        lg[C - 1, 10, 10, 10] = inf
        lg[:, 12, 20, 5] = -inf
        lg[1:, 15, 8, 18] = -inf
        lg[0, 18, 14, 12] = -inf
        lg[1, 20, 20, 20], lg[C - 1, 20, 20, 20] = inf, inf
        lg[C - 1, 8, 22, 16] = -inf
    return lg.numpy()


def ref_native(lg, thr=0.5):
    """the fp64 restatement on the native grid, and the plain fp32 CPU evaluation of the same formula.
    Returns (label_prob {C-1, S}, fg_prob {S}, label {S}, comparable {S}, inside {S}, fp32 distance)"""
    loc = locate(back_map(), NATIVE_SHAPE, MODEL_SHAPE)
    inside = torch.from_numpy(loc[0].reshape(-1))
    C = lg.shape[0]
    x64 = torch.from_numpy(np.stack([tri64(lg[c], loc) for c in range(C)]).reshape(C, -1))
    with np.errstate(invalid="ignore"):
        x32 = torch.from_numpy(np.stack([R._trilinear(lg[c], loc) for c in range(C)]).reshape(C, -1))
    assert x32.dtype == torch.float32
    p = torch.softmax(x64, 0)
    fg = p[1:].sum(0)
    p32 = torch.softmax(x32, 0)
    fg32 = p32[1:].sum(0)
    fin = ~torch.isnan(fg) & inside
    dist = max(float((p32.double() - p)[:, fin].abs().max()), float((fg32.double() - fg)[fin].abs().max())) if fin.any() else 0.0
    top = p[1:].topk(min(2, C - 1), 0).values
    am = p[1:].argmax(0) + 1
    lab = torch.where(fg > thr, am, torch.zeros_like(am))
    ok = (fg - thr).abs() >= GAP
    if top.shape[0] == 2:
        ok &= ((top[0] - top[1]) >= GAP) | (top[0] == top[1])
    ok |= torch.isnan(fg)
    # outside the model's field of view: background, every probability 0
    lp = torch.where(inside[None], p[1:], torch.zeros_like(p[1:]))
    fg = torch.where(inside, fg, torch.zeros_like(fg))
    lab = torch.where(inside, lab, torch.zeros_like(lab))
    return lp, fg, lab, ok | ~inside, inside, dist


def run_native(lg, thr=0.5, want=SP.OUTPUTS, offset=0):
    """unet_space_postproc into buffers pre-filled with 7 (so an output that was not wanted shows as untouched)"""
    C = lg.shape[0]
    S = int(np.prod(NATIVE_SHAPE))
    bufs = {"label_prob": dev_offset((C - 1,) + NATIVE_SHAPE, offset), "fg_prob": dev_offset(NATIVE_SHAPE, offset),
            "label": dev_offset(NATIVE_SHAPE, offset, torch.uint16)}
    res = SP.postproc_native(dev_offset(lg, offset), back_map(), NATIVE_SHAPE, thr, want, out={k: bufs[k] for k in want})
    torch.cuda.synchronize()
    assert sorted(res) == sorted(want)
    return bufs["label_prob"].view(C - 1, S), bufs["fg_prob"].view(S), bufs["label"].view(S)


def check_probs(got, exp, bound, what):
    got = got.cpu().double()
    assert torch.equal(torch.isnan(got), torch.isnan(exp)), what
    fin = ~torch.isnan(exp)
    err = float((got[fin] - exp[fin]).abs().max()) if fin.any() else 0.0
    print("  %s: max |kernel - fp64| = %.3g (bound %.3g)" % (what, err, bound))
    assert err <= bound, what


@pytest.mark.parametrize("special", [False, True])
@pytest.mark.parametrize("C", [2, 3, 6, 33, 130])
def test_native_pass_against_fp64(C, special):
    lg = make_logits(C, 100 + C, special)
    elp, efg, elab, ok, inside, dist = ref_native(lg)
    outside = 1.0 - float(inside.double().mean())
    assert 0.04 < outside < 0.07                               # the geometry the outside rule is tested on: 5.4 % outside
    bound = max(4 * dist, 2e-6)
    print("C = %d%s: outside %.4f, fp32 CPU evaluation is %.3g from fp64 -> bound %.3g" % (C, " special" if special else "", outside,
                                                                                            dist, bound))
    lp, fg, lab = run_native(lg, offset=C % 4)
    check_probs(lp, elp, bound, "label_prob")
    check_probs(fg, efg, bound, "fg_prob")
    got = lab.cpu().to(torch.int64)
    assert torch.equal(got[ok], elab[ok]), int((got[ok] != elab[ok]).sum())
    near = int((~ok & inside).sum())
    print("  voxels within %.0e of a tie: %d of %d inside" % (GAP, near, int(inside.sum())))
    assert near <= 1e-3 * int(inside.sum())
    # the outside rule, whatever the logits
    assert (got[~inside] == 0).all() and (fg.cpu()[~inside] == 0).all() and (lp.cpu()[:, ~inside] == 0).all()


@pytest.mark.parametrize("mask", range(1, 8))
def test_every_subset_of_outputs_and_untouched_ones(mask):
    want = tuple(n for i, n in enumerate(SP.OUTPUTS) if mask >> i & 1)
    lg = make_logits(4, 9)
    full = dict(zip(SP.OUTPUTS, run_native(lg)))
    part = dict(zip(SP.OUTPUTS, run_native(lg, want=want)))
    for n in SP.OUTPUTS:
        if n in want:
            assert torch.equal(part[n].to(torch.float32), full[n].to(torch.float32)), n
        else:
            assert (part[n].cpu().to(torch.float32) == 7).all(), n


def test_threshold_is_used():
    lg = make_logits(3, 5)
    _, fg, lab0 = run_native(lg, thr=0.2, want=("fg_prob", "label"))
    _, _, lab1 = run_native(lg, thr=0.9, want=("label",))
    fg = fg.cpu()
    assert torch.equal(lab0.cpu().to(torch.int32) != 0, fg > 0.2) and torch.equal(lab1.cpu().to(torch.int32) != 0, fg > 0.9)


@pytest.mark.parametrize("C", [2, 6, 33])
def test_fused_equals_resample_then_softmax_inside_and_the_composition_shows_the_artefact_outside(C):
    lg = make_logits(C, 40 + C)
    d = torch.from_numpy(lg).to(DEV)
    S = int(np.prod(NATIVE_SHAPE))
    inside = torch.from_numpy(locate(back_map(), NATIVE_SHAPE, MODEL_SHAPE)[0].reshape(-1)).to(DEV)
    fused = SP.postproc_native(d, back_map(), NATIVE_SHAPE, 0.5)
    nat = SP.resample(d, NATIVE_SHAPE, back_map(), "linear")
    lp = torch.empty((C - 1, S), device=DEV)
    fg = torch.empty(S, device=DEV)
    lab = torch.empty(S, dtype=torch.uint16, device=DEV)
    P.softmax_call(nat, C, S, 0.5, lp, fg, lab)
    torch.cuda.synchronize()
    bits = lambda t: t.contiguous().view(torch.int32)
    assert torch.equal(bits(fused["label_prob"].view(C - 1, S))[:, inside], bits(lp)[:, inside])
    assert torch.equal(bits(fused["fg_prob"].view(S))[inside], bits(fg)[inside])
    assert torch.equal(fused["label"].view(S).to(torch.int32)[inside], lab.to(torch.int32)[inside])
    # outside, all-zero logits give a uniform softmax: fg_prob (C-1)/C >= 0.5 and, above the threshold, label 1 everywhere
    out = ~inside
    assert int(out.sum()) > 0
    assert (fg[out] - (C - 1) / C).abs().max().item() < 1e-6
    if C > 2:
        assert (lab.to(torch.int32)[out] == 1).all()
    assert (fused["label"].view(S).to(torch.int32)[out] == 0).all() and (fused["fg_prob"].view(S)[out] == 0).all()


# ---- to_model_space ----------------------------------------------------------------------------------------------------------------
def small_model(in_count=1, out_c=8, dt="fp32", arch="smoke", dim=(24, 16, 16), vs=(1.5, 1.5, 1.5)):
    a = SMOKE_ARCH % out_c if arch == "smoke" else MIX_ARCH % (out_c, out_c)
    m = U.UNet3d(in_count, out_c, a, device=DEV, dtype=dt, seed=2)
    m.dim, m.voxel_size = dim, vs
    return m


@pytest.mark.parametrize("in_count", [1, 2])
@pytest.mark.parametrize("on_device", [False, True])
def test_to_model_space_against_the_restatement(in_count, on_device):
    m = small_model(in_count)
    W, H, D = m.dim
    rs = np.random.RandomState(7 + in_count)
    shape, vs = (21, 19, 30), (1.1, 1.2, 1.0)
    img = rs.rand(in_count, *shape).astype(F) * 0.8
    lab = rs.randint(0, 4, shape).astype(F)
    keep = img.copy(), lab.copy()
    a, b = (torch.from_numpy(img).to(DEV), torch.from_numpy(lab).to(DEV)) if on_device else (img, lab)
    gi, gl = SP.to_model_space(m, a, vs, b)
    assert gi.shape == (in_count, D, H, W) and gl.shape == (D, H, W) and gi.is_cuda and gl.is_cuda and gi.dtype == torch.float32
    mp = SP.model_to_image_map(m.dim, m.voxel_size, shape[::-1], vs)
    ei, _ = ref_resample(img, (D, H, W), mp, "linear")
    ei = R._norm(ei, ei.max())
    el, _ = ref_resample(lab[None], (D, H, W), mp, "majority")
    err = float(np.abs(gi.cpu().numpy() - ei).max())
    print("to_model_space: max |image - restatement| = %.3g" % err)
    assert err <= LINEAR_TOL and float(gi.max()) == 1.0
    assert np.array_equal(gl.cpu().numpy(), el[0])
    assert np.array_equal(np.asarray(torch.as_tensor(a).cpu()), keep[0]) and np.array_equal(np.asarray(torch.as_tensor(b).cpu()), keep[1])
    only, none = SP.to_model_space(m, a, vs)
    assert none is None and torch.equal(only, gi)


def test_to_model_space_results_are_cases_of_qc_and_the_feed():
    m = small_model(1, 8, dim=(16, 16, 16), vs=(1, 1, 1))
    rs = np.random.RandomState(3)
    cases_dev, cases_host = [], []
    for k, (shape, vs, tpl) in enumerate([((20, 18, 22), (0.9, 1.0, 0.8), True), ((15, 17, 19), (1.0, 0.9, 1.1), False)]):
        z, y, x = np.meshgrid(*(np.arange(n, dtype=F) for n in shape), indexing="ij")
        lab = np.zeros(shape, F)
        for c in range(1, 4):
            ctr = [rs.uniform(4, n - 4) for n in shape]
            lab[(z - ctr[0]) ** 2 + (y - ctr[1]) ** 2 + (x - ctr[2]) ** 2 < 12 + c] = c
        img = (rs.rand(1, *shape).astype(F) * 0.5 + lab[None] / 4).astype(F)
        gi, gl = SP.to_model_space(m, img, vs, lab)
        assert float(gl.max()) >= 1.0 and torch.equal(gl, gl.round())
        cases_dev.append(("c%d.nii.gz" % k, "c%d_label.nii.gz" % k, gi, gl, tpl))
        cases_host.append(("c%d.nii.gz" % k, "c%d_label.nii.gz" % k, gi.cpu().numpy(), gl.cpu().numpy(), tpl))
    sa, oa = U.calculate_qc(m, cases_dev[0][2], cases_dev[0][3])
    sb, ob = U.calculate_qc(m, cases_host[0][2], cases_host[0][3])
    assert sa == sb and oa == ob and oa.voxels == 16 ** 3
    opts = dict(U.augment.DEFAULT_OPTIONS, zero_background=0)
    fa = U.TrainingFeed(m, cases_dev, U.TrainingParam(batch_size=2, seed=5), opts)
    fb = U.TrainingFeed(m, cases_host, U.TrainingParam(batch_size=2, seed=5), opts)
    for i in range(3):
        (xa, ta), (xb, tb) = fa(i), fb(i)
        assert xa.shape == (1, 1, 16, 16, 16) and torch.equal(xa, xb) and torch.equal(ta, tb)


# ---- EvaluateUNet with NativeVolume entries ----------------------------------------------------------------------------------------
def manual(m, io, vs, chain, outputs):
    """to_model_space -> forward -> postproc_native -> the remaining commands, composed by hand from the public pieces"""
    d = io.shape[0] // m.in_count
    native = (d,) + io.shape[1:]
    fwd = SP.model_to_image_map(m.dim, m.voxel_size, native[::-1], vs)
    back = SP.invert_map(fwd)
    x = SP.to_model_space(m, torch.from_numpy(io).view(m.in_count, *native).to(DEV), vs)[0]
    W, H, D = m.dim
    with torch.no_grad():
        logits = m.forward(x.unsqueeze(0))[0].view(m.out_count, D, H, W)
    if not chain:
        return SP.resample(logits, native, back, "linear").cpu().numpy().reshape(m.out_count * d, *io.shape[1:])
    steps = P.parse_chain(chain)
    res = SP.postproc_native(logits, back, native, 0.5)
    for name, p in steps[3:]:
        assert name == "defragment"
        sc = torch.empty(P.postproc_scratch_bytes(m.out_count, d * io.shape[1] * io.shape[2]), dtype=torch.uint8, device=DEV)
        P.defragment_call(native[::-1], False, p["threshold"], p["size_ratio"], res["fg_prob"], res["label_prob"], m.out_count - 1,
                          res["label"], sc)
    torch.cuda.synchronize()
    return {k: res[k].cpu().view(torch.int16 if k == "label" else torch.float32).numpy() for k in outputs}


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("arch", ["smoke", "mix"])
@pytest.mark.parametrize("chain", [None, "model", "softmax+create_mask+argmax+defragment"])
def test_evaluate_native_volumes_equal_the_manual_sequence(arch, dt, chain):
    out_c = 5
    m = small_model(1, out_c, dt, arch)
    rs = np.random.RandomState(11)
    vols = [((20, 18, 30), (1.0, 1.2, 1.1)), ((26, 22, 38), (0.9, 1.0, 1.3))]
    ios = [[U.NativeVolume(rs.rand(*s).astype(F), vs) for s, vs in vols[:1]], [U.NativeVolume(rs.rand(*s).astype(F), vs) for s, vs in vols]]
    outputs = ("label", "fg_prob", "label_prob")
    ev = U.EvaluateUNet(m, postproc=chain, outputs=outputs)
    got = ev.start(ios)
    assert not ev.aborted and ev.error_msg == "" and ev.cur_prog == 2
    text = m.postproc if chain == "model" else chain
    for gf, nf in zip(got, ios):
        for g, nv in zip(gf, nf):
            d, h, w = nv.data.shape
            exp = manual(m, nv.data, nv.voxel_size, text, outputs)
            if chain is None:
                assert g.dtype == np.float32 and g.shape == (out_c * d, h, w) and g.tobytes() == exp.tobytes()
                continue
            assert sorted(g) == sorted(outputs)
            assert g["label"].dtype == np.uint16 and g["label"].shape == (d, h, w)
            assert g["fg_prob"].shape == (d, h, w) and g["label_prob"].shape == ((out_c - 1) * d, h, w)
            for k in outputs:
                assert g[k].tobytes() == exp[k].tobytes(), k


def test_evaluate_mixes_arrays_and_native_volumes_and_the_identity_volume_is_the_array_path():
    out_c = 4
    m = small_model(1, out_c, "fp32", "smoke", dim=(24, 16, 16), vs=(1.5, 1.5, 1.5))
    rs = np.random.RandomState(2)
    own = rs.rand(16, 16, 24).astype(F)
    own[3, 4, 5] = 1.0                                       # maximum 1: tipl::normalize changes nothing
    other = rs.rand(20, 18, 30).astype(F)
    ios = [[own, U.NativeVolume(own, m.voxel_size), U.NativeVolume(other, (1, 1.2, 1.1))]]
    raw = U.EvaluateUNet(m).start(ios)[0]
    assert raw[0].shape == raw[1].shape == (out_c * 16, 16, 24) and raw[2].shape == (out_c * 20, 18, 30)
    assert raw[0].tobytes() == raw[1].tobytes()
    ev = U.EvaluateUNet(m, postproc="model", outputs=("label", "fg_prob", "label_prob"))
    got = ev.start(ios)[0]
    assert not ev.aborted
    for k in ("label", "fg_prob", "label_prob"):
        assert got[0][k].tobytes() == got[1][k].tobytes(), k
    assert got[2]["label"].shape == (20, 18, 30) and got[2]["label_prob"].shape == ((out_c - 1) * 20, 18, 30)
    # the caller's entries are not written
    assert isinstance(ios[0][1], U.NativeVolume) and ios[0][1].data is own and own[3, 4, 5] == 1.0


def test_evaluate_native_errors_end_the_run():
    m = small_model(2, 3, "fp32", "smoke")
    good = U.NativeVolume(np.random.RandomState(0).rand(2 * 10, 12, 14).astype(F), (1, 1, 1))
    bad = U.NativeVolume(np.zeros((2 * 10, 12, 14), F), (1, 1, 1))
    bad.voxel_size = (1, 0, 1)
    ev = U.EvaluateUNet(m)
    out = ev.start([[good], [bad]])
    assert ev.aborted and "voxel_size" in ev.error_msg and ev.cur_prog == 1 and len(out) == 2
    ev = U.EvaluateUNet(m)
    ev.start([[U.NativeVolume(np.zeros((2 * 10 + 1, 12, 14), F), (1, 1, 1))]])
    assert ev.aborted and "model_io buffer must be (in_count*D, H, W)" in ev.error_msg
