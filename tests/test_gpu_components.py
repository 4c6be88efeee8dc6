"""GPU: a model's single_component_label on the device (include/unet_components.h) -- both implementations against the scipy
restatement of test_components_host.py and against each other, bit for bit, every case twice; `removed` wherever it is given;
run_postproc's and EvaluateUNet's single_component keywords.  Every comparison is exact equality of label maps or counts."""
import os
import sys
import threading

import numpy as np
import pytest
import torch

import unet_studio_amd as U
from unet_studio_amd import components as CMP
from unet_studio_amd import postproc as P

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_components_host import keep_largest_ref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F = np.float32
TX, TY, TZ = CMP.TILE
IMPLS = (CMP.IMPL_TILED, CMP.IMPL_GLOBAL, CMP.IMPL_DEFAULT)
# (W, H, D): the smallest shapes at which the tiling can go wrong, one odd mid-size volume and one of about 1 M voxels
SHAPES = [(1, 1, 1), (TX, TY, TZ), (TX + 1, TY + 1, TZ + 1), (2 * TX - 1, 1, 1), (1, 2 * TY + 1, 1), (1, 1, 2 * TZ + 1),
          (3, TY - 1, 2 * TZ), (130, 40, 7), (97, 113, 91)]


def dev_u16(a):
    return torch.from_numpy(np.ascontiguousarray(a).astype(np.int32)).to(DEV).to(torch.uint16)


def host_u16(t):
    return t.cpu().to(torch.int32).numpy().astype(np.uint16)


def check(a, classes, n_classes, impls=IMPLS, expect=None):
    """a: (D, H, W) uint16.  Every implementation twice against the restatement, the label map and the removed counts exactly;
    returns the restatement's (result, removed)."""
    a = np.ascontiguousarray(a, np.uint16)
    exp, exp_removed = expect if expect is not None else keep_largest_ref(a, classes, n_classes)
    src = dev_u16(a)
    for impl in impls:
        for rep in range(2):
            lab = src.clone()
            removed = torch.full((n_classes,), 0x7FFFFFFF - rep, dtype=torch.int32, device=DEV)     # the call must zero-fill it
            assert CMP.keep_largest(lab, classes, n_classes, removed=removed, impl=impl) is lab
            got, got_removed = host_u16(lab), removed.cpu().numpy().astype(np.uint32)
            assert got.dtype == np.uint16 and got.tobytes() == exp.tobytes(), (impl, rep, int((got != exp).sum()))
            assert got_removed.tobytes() == exp_removed.tobytes(), (impl, rep)
        lab = src.clone()
        CMP.keep_largest(lab, classes, n_classes, impl=impl)                                          # without removed
        assert host_u16(lab).tobytes() == exp.tobytes(), impl
    return exp, exp_removed


# ---- the patterns: shape (D, H, W) -> (label map, listed classes, n_classes) -------------------------------------------------------
def sprinkle(a, rng, value, p, where=None):
    m = rng.random(a.shape) < p
    a[m if where is None else m & where] = value


def pat_fill(shape, rng):
    """one listed value fills the volume: one component across every tile border"""
    return np.full(shape, 2, np.uint16), [2], 3


def snake(shape, v):
    """one voxel wide: rows along x at every other y joined at alternating ends, layers at every other z joined at alternating
    corners -- it crosses tile faces in all three directions"""
    D, H, W = shape
    a = np.zeros(shape, np.uint16)
    ylast = (H - 1) // 2 * 2
    for z in range(0, D, 2):
        for y in range(0, H, 2):
            a[z, y, :] = v
            if y + 2 < H:
                a[z, y + 1, W - 1 if (y // 2) % 2 == 0 else 0] = v
        if z + 2 < D:
            if (z // 2) % 2 == 0:
                a[z + 1, ylast, 0 if (ylast // 2) % 2 else W - 1] = v
            else:
                a[z + 1, 0, 0] = v
    return a


def pat_snake(shape, rng):
    a = snake(shape, 1)
    sprinkle(a, rng, 1, 0.05, a == 0)            # fragments of the listed class in the gaps (some touch the snake)
    sprinkle(a, rng, 3, 0.05, a == 0)            # an unlisted class with fragments
    return a, [1, 4], 6                          # 4: a listed class that does not occur


def pat_spiral(shape, rng):
    """in every other z-plane concentric rings two apart, each cut once and joined to the next one inside; planes joined at a corner"""
    D, H, W = shape
    a = np.zeros(shape, np.uint16)
    for z in range(0, D, 2):
        r = 0
        while W - 1 - 2 * r >= 0 and H - 1 - 2 * r >= 0:
            a[z, r, r:W - r] = a[z, H - 1 - r, r:W - r] = 2
            a[z, r:H - r, r] = a[z, r:H - r, W - 1 - r] = 2
            if r >= 2 and H - 1 - 2 * r >= 2 and W - 1 - 2 * r >= 2:
                a[z, r - 1, r - 2] = 0           # cut the ring outside just below its top-left corner
                a[z, r, r - 1] = 2               # and join it to this one
            r += 2
        if z + 2 < D:
            a[z + 1, 0, 0] = 2
    sprinkle(a, rng, 2, 0.03, a == 0)
    return a, [2], 3


def pat_adjacent(shape, rng):
    """two adjacent listed values must not merge; strays of each inside the other"""
    D, H, W = shape
    z, y, x = np.indices(shape)
    a = np.where(x * 2 + y + z < (2 * W + H + D) // 2, 1, 2).astype(np.uint16)
    strays = rng.random(shape) < 0.02
    a[strays] = 3 - a[strays]
    return a, [1, 2], 3


def pat_twins(shape, rng):
    """equal-sized twins along the longest axis, a smaller third piece and one voxel wide gaps: the lower index survives"""
    a = np.zeros(shape, np.uint16)
    ax = int(np.argmax(shape))
    k = shape[ax] // 4
    sl = [slice(None)] * 3
    for lo in (0, k + 1, 2 * k + 2):
        sl[ax] = slice(lo, lo + (k if lo < 2 * k + 2 else max(k - 1, 0)))
        a[tuple(sl)] = 5
    return a, [5], 6


def pat_diagonal(shape, rng):
    """2x2x2 cubes along the main diagonal touch at corners only"""
    z, y, x = np.indices(shape)
    a = ((x // 2 == y // 2) & (y // 2 == z // 2)).astype(np.uint16)
    return a, [1], 2


def pat_checker(shape, rng):
    z, y, x = np.indices(shape)
    return (1 + (x + y + z) % 2).astype(np.uint16), [1, 2], 3


def pat_foreign(shape, rng):
    """values >= n_classes and an unlisted class stay untouched among fragments of a listed one"""
    a = rng.integers(0, 4, shape).astype(np.uint16)
    sprinkle(a, rng, 4, 0.1)                     # == n_classes
    sprinkle(a, rng, 9, 0.1)
    sprinkle(a, rng, 65535, 0.1)
    return a, [3, 1], 4


def pat_random(shape, rng):
    """random maps with 2 to 6 values at several densities (one per call, by the generator's state)"""
    nv = int(rng.integers(2, 7))
    density = (0.2, 0.5, 0.9)[int(rng.integers(0, 3))]
    a = rng.integers(1, nv + 1, shape).astype(np.uint16)
    a[rng.random(shape) >= density] = 0
    listed = [int(v) for v in rng.permutation(np.arange(1, nv + 1))[:max(1, nv - 1)]]
    return a, listed + listed[:1], nv + 1        # a duplicate entry is allowed


def pat_blobs(shape, rng):
    """solid pieces of several classes: smoothed noise, thresholded into bands"""
    from scipy import ndimage
    g = ndimage.uniform_filter(rng.random(shape), size=5, mode="nearest")
    q = np.quantile(g, [0.3, 0.5, 0.7])
    return np.digitize(g, q).astype(np.uint16), [1, 2, 3], 4


PATTERNS = {"fill": pat_fill, "snake": pat_snake, "spiral": pat_spiral, "adjacent": pat_adjacent, "twins": pat_twins,
            "diagonal": pat_diagonal, "checker": pat_checker, "foreign": pat_foreign, "random": pat_random, "blobs": pat_blobs}


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("name", sorted(PATTERNS))
def test_both_implementations_are_bitwise_the_restatement(name, shape):
    W, H, D = shape
    rng = np.random.default_rng(1000 * sorted(PATTERNS).index(name) + SHAPES.index(shape))
    a, classes, n_classes = PATTERNS[name]((D, H, W), rng)
    exp, removed = check(a, classes, n_classes)
    listed = np.isin(a, classes)
    assert np.array_equal(exp[~listed], a[~listed])                       # what is not listed is never written
    for v in set(classes):
        assert removed[v] == int((a == v).sum()) - int((exp == v).sum())


@pytest.mark.parametrize("nv", [2, 3, 4, 5, 6])
def test_random_maps_at_three_densities(nv):
    rng = np.random.default_rng(nv)
    for density in (0.15, 0.5, 0.95):
        a = rng.integers(1, nv + 1, (2 * TZ + 3, TY + 5, 2 * TX + 7)).astype(np.uint16)
        a[rng.random(a.shape) >= density] = 0
        check(a, list(range(1, nv + 1)), nv + 1)
        check(a, [nv], nv + 2)


def test_patterns_are_what_they_claim():
    from scipy import ndimage
    faces = ndimage.generate_binary_structure(3, 1)
    shape = (TZ + 1, 2 * TY + 1, 2 * TX + 1)
    for build, v in ((lambda: snake(shape, 1), 1), (lambda: pat_spiral(shape, np.random.default_rng(0))[0], 2)):
        a = build()
        comp, n = ndimage.label(a == v, structure=faces)
        big = np.bincount(comp.reshape(-1))[1:].max()
        assert big > a.size // 8                                          # one long piece through many tiles
        z, y, x = np.nonzero(comp == 1 + np.bincount(comp.reshape(-1))[1:].argmax())
        assert x.max() >= 2 * TX and y.max() >= 2 * TY and z.max() >= TZ  # across tile faces in x, y and z
    a, classes, n = pat_twins((3, 4, 41), None)
    exp, removed = keep_largest_ref(a, classes, n)
    assert (exp[:, :, :10] == 5).all() and not exp[:, :, 10:].any() and removed[5] == 12 * (10 + 9)


def test_65536_classes_with_class_65535_listed():
    a = np.zeros((3, 4, 5), np.uint16)
    a[0, 0, :2] = a[2, 3, 2:] = 65535                                      # 2 and 3 voxels
    a[1, 1, 1] = 65534
    a[1, 2, 2] = 1
    a[1, 2, 4] = 1
    exp, removed = check(a, [65535, 1], 65536)
    assert (exp[2, 3, 2:] == 65535).all() and not exp[0].any() and exp[1, 1, 1] == 65534 and exp[1, 2, 2] == 1 and exp[1, 2, 4] == 0
    assert removed[65535] == 2 and removed[1] == 1 and removed.sum() == 3
    # a class at and above the LDS histogram's limit, with many voxels removed
    rng = np.random.default_rng(3)
    b = rng.choice(np.array([0, 2047, 2048, 40000], np.uint16), (9, 10, 37))
    check(b, [2047, 2048, 40000], 40001)


def test_an_empty_list_leaves_the_input_and_zero_fills_removed():
    rng = np.random.default_rng(4)
    a = rng.integers(0, 4, (9, 10, 37)).astype(np.uint16)
    exp, removed = check(a, [], 4)
    assert exp.tobytes() == a.tobytes() and not removed.any()


@pytest.mark.parametrize("shape", [(TX + 1, TY + 1, TZ + 1), (130, 40, 7)], ids=lambda s: "x".join(map(str, s)))
def test_a_label_pointer_2_bytes_off_16_byte_alignment(shape):
    W, H, D = shape
    rng = np.random.default_rng(5)
    a, classes, n_classes = pat_blobs((D, H, W), rng)
    exp, exp_removed = keep_largest_ref(a, classes, n_classes)
    for off in (1, 7):
        for impl in IMPLS:
            buf = torch.full((a.size + 16,), 77, dtype=torch.uint16, device=DEV)
            lab = buf[off:off + a.size].view(D, H, W)
            assert lab.data_ptr() % 16 == 2 * off
            lab.copy_(dev_u16(a))
            removed = torch.empty(n_classes, dtype=torch.int32, device=DEV)
            CMP.keep_largest(lab, classes, n_classes, removed=removed, impl=impl)
            assert host_u16(lab).tobytes() == exp.tobytes() and removed.cpu().numpy().astype(np.uint32).tobytes() == exp_removed.tobytes()
            whole = host_u16(buf)
            assert (whole[:off] == 77).all() and (whole[off + a.size:] == 77).all()                                    # nothing outside the map is written


def test_a_caller_scratch_is_reused_and_a_small_one_is_replaced():
    rng = np.random.default_rng(6)
    a, classes, n = pat_blobs((9, 12, 40), rng)
    exp, _ = keep_largest_ref(a, classes, n)
    sc = torch.empty(CMP.components_scratch_bytes(a.size, n) + 3, dtype=torch.uint8, device=DEV)
    for scratch in (sc, sc[3:], sc[:100]):                                # any alignment; too small: the wrapper makes its own
        lab = dev_u16(a)
        CMP.keep_largest(lab, classes, n, scratch=scratch)
        assert host_u16(lab).tobytes() == exp.tobytes()


def test_two_threads_on_two_streams_with_their_own_scratch():
    cases = []
    for k, impl in enumerate((CMP.IMPL_TILED, CMP.IMPL_GLOBAL)):
        a, classes, n = pat_blobs((41, 37, 70), np.random.default_rng(70 + k))
        exp, exp_removed = keep_largest_ref(a, classes, n)
        cases.append((dev_u16(a), classes, n, impl, exp, exp_removed))
    torch.cuda.synchronize()
    bad = []

    def work(i):
        src, classes, n, impl, exp, exp_removed = cases[i]
        s = torch.cuda.Stream(DEV)
        sc = torch.empty(CMP.components_scratch_bytes(src.numel(), n), dtype=torch.uint8, device=DEV)
        with torch.cuda.stream(s):
            removed = torch.empty(n, dtype=torch.int32, device=DEV)
            for _ in range(10):
                lab = src.clone()
                CMP.keep_largest(lab, classes, n, removed=removed, scratch=sc, impl=impl)
                s.synchronize()
                if host_u16(lab).tobytes() != exp.tobytes() or removed.cpu().numpy().astype(np.uint32).tobytes() != exp_removed.tobytes():
                    bad.append(i)

    ts = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    [t.start() for t in ts]
    [t.join() for t in ts]
    assert not bad


# ---- run_postproc ----------------------------------------------------------------------------------------------------------------
def smooth_logits(seed, c, shape):
    """low-frequency logits plus noise: label maps with solid pieces and stray fragments"""
    g = torch.Generator().manual_seed(seed)
    coarse = torch.randn((1, c) + tuple((s + 3) // 4 for s in shape), generator=g)
    x = torch.nn.functional.interpolate(coarse, size=shape, mode="trilinear", align_corners=False)[0] * 2
    return (x + 0.8 * torch.randn(x.shape, generator=g)).contiguous().to(DEV)


@pytest.mark.parametrize("chain", ["softmax+create_mask+argmax", "softmax+create_mask+defragment+argmax+defragment"])
def test_run_postproc_single_component_is_the_restatement_on_the_same_calls_label(chain):
    c, shape = 5, (13, 22, 41)
    logits = smooth_logits(11, c, shape)
    params = {"argmax": 0.3, "defragment": (0.3, 0.2)}
    base = P.run_postproc(logits, chain, params=params)
    lab = host_u16(base["label"])
    some = 0
    for listed in ([1, 3], [4], [1, 2, 3, 4]):
        exp, removed = keep_largest_ref(lab, listed, c)
        some += int(removed.sum())
        for scratch in (None, torch.empty(CMP.components_scratch_bytes(lab.size, c), dtype=torch.uint8, device=DEV)):
            got = P.run_postproc(logits, chain, params=params, single_component=listed, component_scratch=scratch)
            assert host_u16(got["label"]).tobytes() == exp.tobytes()
            assert torch.equal(got["fg_prob"], base["fg_prob"]) and torch.equal(got["label_prob"], base["label_prob"])   # not touched
    assert some > 0                                                       # the case has fragments to remove
    for nothing in (None, [], ()):
        got = P.run_postproc(logits, chain, params=params, single_component=nothing)
        assert all(torch.equal(got[k], base[k]) for k in base)
    got = P.run_postproc(logits, chain, params=params, outputs=("fg_prob",), single_component=[1])     # no label wanted: no call
    assert sorted(got) == ["fg_prob"] and torch.equal(got["fg_prob"], base["fg_prob"])
    for bad in (0, c):
        with pytest.raises(U.UNetError, match="class %d is not in" % bad):
            P.run_postproc(logits, chain, params=params, single_component=[1, bad])


# ---- EvaluateUNet ------------------------------------------------------------------------------------------------------------------
SMOKE_ARCH = ("conv8,ks3,stride1+norm,leaky_relu+conv8,ks3,stride1+norm,leaky_relu\n"
              "conv16,ks3,stride2+norm,leaky_relu+conv16,ks3,stride1+norm,leaky_relu+conv_trans8,ks2,stride2\n"
              "conv8,ks3,stride1+norm,leaky_relu+conv8,ks3,stride1+norm,leaky_relu+conv%d,ks1,stride1")
OUTPUTS = ("label", "fg_prob", "label_prob")
PARAMS = {"argmax": 0.0}                                                  # every voxel takes its best foreground class


def small_model(dt, out_c=4):
    m = U.UNet3d(1, out_c, SMOKE_ARCH % out_c, device=DEV, dtype=dt, seed=2)
    m.dim, m.voxel_size = (16, 16, 16), (1.0, 1.0, 1.0)
    return m


def volumes():
    rs = np.random.RandomState(7)
    return [[rs.rand(16, 16, 16).astype(F), U.NativeVolume(rs.rand(20, 18, 22).astype(F), (1.1, 0.9, 1.2))],
            [U.NativeVolume(rs.rand(13, 21, 17).astype(F), (0.8, 1.3, 1.0))]]


def same_results(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), k


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
def test_evaluate_single_component(dt):
    m = small_model(dt)
    ios = volumes()
    base = U.EvaluateUNet(m, postproc="model", outputs=OUTPUTS, params=PARAMS).start(ios)
    # None changes no bit against a run without the keyword; nor does an empty list, nor the model's empty list
    for nothing in (None, [], "model"):
        ev = U.EvaluateUNet(m, postproc="model", outputs=OUTPUTS, params=PARAMS, single_component=nothing)
        got = ev.start(ios)
        assert not ev.aborted and ev.error_msg == "" and ev.cur_prog == 2
        for gf, bf in zip(got, base):
            for g, b in zip(gf, bf):
                same_results(g, b)
    # "model" and an explicit list equal the restatement on the label map of that run, on the scan's own grid
    some = 0
    for spec, listed in (("model", [3, 1]), ([2, 1, 2], [1, 2]), ((3,), [3])):
        m.single_component_label = [3, 1, 3] if spec == "model" else []
        ev = U.EvaluateUNet(m, postproc="model", outputs=OUTPUTS, params=PARAMS, single_component=spec)
        got = ev.start(ios)
        assert not ev.aborted and ev.error_msg == "" and ev.cur_prog == 2
        for gf, bf, inf in zip(got, base, ios):
            for g, b, io in zip(gf, bf, inf):
                shape = io.data.shape if isinstance(io, U.NativeVolume) else io.shape
                assert g["label"].shape == b["label"].shape == shape
                exp, removed = keep_largest_ref(b["label"], listed, m.out_count)
                some += int(removed.sum())
                assert g["label"].dtype == np.uint16 and g["label"].tobytes() == exp.tobytes()
                assert g["fg_prob"].tobytes() == b["fg_prob"].tobytes() and g["label_prob"].tobytes() == b["label_prob"].tobytes()
    assert some > 0
    m.single_component_label = [1, 2, 3]
    # logits (no chain) and a chain without a label output have nothing to act on
    plain = U.EvaluateUNet(m).start(ios)
    got = U.EvaluateUNet(m, single_component="model").start(ios)
    assert all(g.tobytes() == p.tobytes() for gf, pf in zip(got, plain) for g, p in zip(gf, pf))
    got = U.EvaluateUNet(m, postproc="model", outputs=("fg_prob",), params=PARAMS, single_component="model").start(ios)
    assert got[0][1]["fg_prob"].tobytes() == base[0][1]["fg_prob"].tobytes()


def test_evaluate_a_bad_entry_ends_the_run_before_any_forward():
    m = small_model("fp32")
    calls = []
    real = m.forward
    m.forward = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
    ios = volumes()
    for spec, bad in (([1, 0], 0), ([4], 4), ("model", 7)):
        m.single_component_label = [2, 7]
        ev = U.EvaluateUNet(m, postproc="model", single_component=spec)
        out = ev.start(ios)
        assert ev.aborted and not ev.running and ev.cur_prog == 0 and out[0][0] is ios[0][0], spec
        assert ev.error_msg == "single_component: class %d is not in [1, 3]" % bad, spec
    ev = U.EvaluateUNet(m, single_component="model")                       # checked even where it has nothing to act on
    ev.start(ios)
    assert ev.aborted and "class 7" in ev.error_msg
    assert not calls
    m.single_component_label = [2]
    ev = U.EvaluateUNet(m, postproc="model", single_component="model")
    out = ev.start(ios)
    assert not ev.aborted and ev.error_msg == "" and len(calls) == 3 and out[1][0]["label"].shape == (13, 21, 17)
