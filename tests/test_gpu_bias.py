"""GPU: the intensity-inhomogeneity correction on the device (include/unet_bias.h) -- logcode, levels, residual, sweep under IMPL_NODE,
IMPL_VOXEL and the default, refine, cost, fit, apply and correct against the numpy restatements of tests/bias_ref.py and against the
stages called by hand.  Every case runs twice into 0x5A-filled outputs with guard bytes around them; every comparison is exact
equality of bytes.  Shapes are written (W, H, D) as in the header; the arrays are (D, H, W)."""
import os
import sys
import threading

import numpy as np
import pytest
import torch

from unet_studio_amd import bias as BS

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bias_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
IMPLS = (BS.IMPL_NODE, BS.IMPL_VOXEL, BS.IMPL_DEFAULT)
SHAPES = [(5, 6, 7), (17, 9, 33), (37, 29, 21)]                     # one cell, a partial last cell, odd sizes, at every spacing
SPACINGS = (4, 8, 16, 32)
LAMS = (0, 37, BS.MAX_LAM)
CLASSES = [1, 2, 3, 300, 9]                                         # 300: no uint8 label; 9: no voxel at all
G = 64                                                              # guard bytes on each side
GUARD = 0xC3
TORCH = {np.uint8: torch.uint8, np.uint16: torch.uint16}


def dev(a):
    a = np.array(a, order="C")                                      # a copy: the shared cases are read only
    if a.dtype == np.uint16:
        return torch.from_numpy(a.view(np.int16)).to(DEV).view(torch.uint16)
    return torch.from_numpy(a).to(DEV)


def host(t):
    if t.dtype == torch.uint16:
        return t.view(torch.int16).cpu().numpy().view(np.uint16)
    return t.cpu().numpy()


def same(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()


def guarded(n, dtype, rep, fill=None):
    """-> (the whole byte buffer, its inner n elements of `dtype`, every byte 0x5A + rep or the bytes of `fill`, between guard bytes)"""
    nbytes = n * torch.empty(0, dtype=dtype).element_size()
    buf = torch.full((nbytes + 2 * G,), GUARD, dtype=torch.uint8, device=DEV)
    buf[G:G + nbytes] = 0x5A + rep
    inner = buf[G:G + nbytes].view(dtype)
    if fill is not None:
        inner.copy_(dev(fill).reshape(-1))
    return buf, inner


def intact(*bufs):
    for buf in bufs:
        b = buf.cpu().numpy()
        assert (b[:G] == GUARD).all() and (b[-G:] == GUARD).all()


def offset_view(a):
    """a device tensor with the values of `a` that starts one element into its allocation"""
    flat = np.ascontiguousarray(a).reshape(-1)
    buf = torch.zeros(flat.size + 1, dtype=TORCH[a.dtype.type], device=DEV)
    buf[1:] = dev(flat)
    t = buf[1:].view(a.shape)
    assert t.data_ptr() % 4 != 0 and t.is_contiguous()
    return t


def case(shape, seed, dtype=np.uint8, noise=0.02):
    """-> (volume float32, labels, q): three classes in stripes with strays, a smooth gain, noise, and voxels without a logarithm"""
    rng = np.random.default_rng(seed)
    d, h, w = shape
    z, y, x = np.indices(shape).astype(np.float64)
    labels = (1 + ((x + y + z) % 3)).astype(dtype)
    labels[rng.random(shape) < 0.2] = 0
    if dtype == np.uint16:
        labels[rng.random(shape) < 0.1] = 300
    gain = np.exp2(0.3 * x / w - 0.2 * y / h + 0.1 * z / d)
    level = np.choose(np.minimum(labels, 4), [5.0, 100.0, 60.0, 30.0, 45.0])
    volume = (level * gain * (1 + noise * rng.standard_normal(shape))).astype(np.float32)
    bad = rng.random(shape) < 0.05
    volume[bad] = rng.choice(np.array([0.0, -3.0, np.nan, np.inf, 1e-40, 1e6, 1e-3], np.float32), int(bad.sum()))
    return volume, labels, ref.logcode_ref(volume)


def random_field(rng, shape, g, top=BS.MAX):
    return rng.integers(-top, top + 1, ref.lattice_ref(shape, g)).astype(np.int32)


def rev(shape):
    return tuple(reversed(shape))


# ---- logcode -------------------------------------------------------------------------------------------------------------------------------
def test_logcode_over_edge_floats():
    bits = [0x00000000, 0x80000000, 0x00000001, 0x007FFFFF, 0x00800000, 0x00800001, 0x3F800000, 0x3F800001, 0x3FFFFFFF, 0x40000000, 0x40400000,
            0x7F7FFFFF, 0x7F800000, 0xFF800000, 0x7FC00000, 0x7F800001, 0xFFC00000, 0xBF800000, 0x80800000, 0x3F000000, 0x3EFFFFFF, 0x3FB504F3]
    rng = np.random.default_rng(0)
    v = np.concatenate([np.array(bits, np.uint32), rng.integers(0, 2 ** 32, 4096 - len(bits), dtype=np.uint64).astype(np.uint32)]).view(np.float32)
    v = v.reshape(4, 8, 128)
    want = ref.logcode_ref(v)
    assert want.reshape(-1)[:13].tolist() == [ref.NONE] * 4 + [-126 * 4096, -126 * 4096, 0, 0, 4095, 4096, 6492, 128 * 4096 - 1, ref.NONE]
    for rep in range(2):
        buf, out = guarded(v.size, torch.int32, rep)
        got = BS.logcode(dev(v), out=out)
        assert got.data_ptr() == out.data_ptr() and same(host(got), want)
        intact(buf)


# ---- levels, residual, cost ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
@pytest.mark.parametrize("shape", SHAPES)
def test_levels_residual_and_cost_with_labels_from_an_offset_view(shape, dtype):
    ss = rev(shape)
    _, labels, q = case(ss, shape[0], dtype)
    rng = np.random.default_rng(shape[0] + 7)
    l_dev, q_dev = offset_view(labels), dev(q)
    for g in SPACINGS:
        for top in (0, 600, BS.MAX):
            B = random_field(rng, ss, g, top)
            want_lev = ref.levels_ref(q, labels, CLASSES, B, g)
            assert want_lev[4].tolist() == [ref.NONE, 0, 0] and (want_lev[3, 1] > 0) == (dtype == np.uint16) and want_lev[0, 1] > 0
            for rep in range(2):
                lbuf, lout = guarded(BS.MAX_CLASSES * 3, torch.int64, rep)
                lev = BS.levels(q_dev, l_dev, CLASSES, dev(B), g, out=lout)
                assert same(host(lev), want_lev), (g, top, rep, host(lev)[:5], want_lev[:5])
                for clip in (0, 200, BS.MAX):
                    want_r = ref.residual_ref(q, labels, CLASSES, want_lev, clip)
                    rbuf, rout = guarded(q.size, torch.int16, rep)
                    r = BS.residual(q_dev, l_dev, CLASSES, lev, clip, out=rout)
                    assert r.data_ptr() == rout.data_ptr() and same(host(r), want_r), (g, top, clip, rep)
                    cbuf, cout = guarded(2, torch.int64, rep)
                    c = BS.cost(r, dev(B), g, out=cout)
                    assert same(host(c), ref.cost_ref(want_r, B, g)), (g, top, clip, rep)
                    intact(rbuf, cbuf)
                intact(lbuf)
            assert (want_r != ref.SKIP).sum() > 0


# ---- sweep ---------------------------------------------------------------------------------------------------------------------------------
def check_sweep(r, B, g, lam, impls=IMPLS):
    want = ref.sweep_ref(r, B, g, lam)
    r_dev = dev(r)
    for impl in impls:
        for rep in range(2):
            buf, field = guarded(B.size, torch.int32, rep, fill=B)
            info = BS.sweep(r_dev, field.view(B.shape), g, lam, impl=impl)
            assert same(host(field.view(B.shape)), want[0]) and same(host(info), want[1]), (r.shape, g, lam, impl, rep, host(info), want[1])
            intact(buf)
    return want


@pytest.mark.parametrize("g", SPACINGS)
@pytest.mark.parametrize("shape", SHAPES)
def test_sweep_under_every_impl_against_the_restatement(shape, g):
    ss = rev(shape)
    _, labels, q = case(ss, shape[0] + g)
    rng = np.random.default_rng(shape[0] * 10 + g)
    start = zero = ref.zero_field(ss, g)
    r = ref.residual_ref(q, labels, CLASSES, ref.levels_ref(q, labels, CLASSES, zero, g), 2048)
    changed = 0
    for lam in LAMS:
        B, info = check_sweep(r, start, g, lam)
        changed += int(info[0])
        start = B                                                   # the next lam starts from where this one ended
    assert changed > 0
    # the extremes: every residual at +-8192, the field at +-8192 at random: the clamp and the widest sums
    wild = np.where(rng.random(ss) < 0.5, 8192, -8192).astype(np.int16)
    wild[rng.random(ss) < 0.1] = ref.SKIP
    for lam in LAMS:
        check_sweep(wild, (rng.integers(0, 2, zero.shape) * 16384 - 8192).astype(np.int32), g, lam, impls=IMPLS[:2])
    check_sweep(np.full(ss, 8192, np.int16), np.full(zero.shape, -8192, np.int32), g, BS.MAX_LAM, impls=IMPLS[:2])


def test_a_node_and_a_volume_that_are_all_skipped_stay_zero():
    ss, g = (21, 29, 37), 8
    _, labels, q = case(ss, 3)
    zero = ref.zero_field(ss, g)
    r = ref.residual_ref(q, labels, CLASSES, ref.levels_ref(q, labels, CLASSES, zero, g), 2048)
    r[0:16, 8:24, 16:32] = ref.SKIP                                 # the whole support of node (k, j, i) = (1, 2, 3), and more
    for lam in (0, 5):
        B, info = check_sweep(r, zero, g, lam)
        assert lam or B[1, 2, 3] == 0                               # without links the node stays; with them it follows its neighbours
        assert info[1] == zero.size if lam else 0 < info[1] < zero.size
    none = np.full(ss, ref.SKIP, np.int16)
    for g in SPACINGS:
        zero = ref.zero_field(ss, g)
        for lam in (0, 5):
            B, info = check_sweep(none, zero, g, lam)
            assert not B.any() and info.tolist() == [0, zero.size if lam else 0]
    # a fit over labels of which none is listed: the field stays zero, and the report is still filled
    q_dev, l_dev = dev(q), dev(labels)
    want = ref.fit_ref(q, labels, [77], 2048, [(16, 3, 1), (8, 3, 1)], 2)
    assert not want[0].any() and want[1][:4].tolist() == [[16, 0, 1, 0, 0, 0], [16, 1, 1, 0, 0, 0], [8, 0, 1, 0, 0, 0], [8, 1, 1, 0, 0, 0]]
    for impl in IMPLS:
        B, report = BS.fit(q_dev, l_dev, [77], [(16, 3, 1), (8, 3, 1)], 2, 2048, impl=impl)
        assert same(host(B), want[0]) and same(host(report), want[1])


# ---- refine ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_refine(shape):
    ss = rev(shape)
    rng = np.random.default_rng(shape[1])
    for g in (8, 16, 32):
        for top in (3, BS.MAX):
            B = random_field(rng, ss, g, top)
            want = ref.refine_ref(B, ss, g)
            for rep in range(2):
                buf, out = guarded(want.size, torch.int32, rep)
                got = BS.refine(dev(B), ss, g, out=out)
                assert got.data_ptr() == out.data_ptr() and same(host(got), want), (g, top, rep)
                intact(buf)


# ---- fit -------------------------------------------------------------------------------------------------------------------------------------
FIT_SHAPE = (33, 45, 70)                                            # (70, 45, 33): 32 -> 16 -> 8


def by_hand(q_dev, l_dev, classes, clip, levels, outer, impl):
    """the schedule of fit from the single calls, the early end decided on the host"""
    shape = tuple(q_dev.shape)
    report = np.full((BS.MAX_ROWS, 6), -1, np.int64)
    B = torch.zeros(BS.lattice(shape, levels[0][0]), dtype=torch.int32, device=DEV)
    row = 0
    for l, (g, sweeps, lam) in enumerate(levels):
        for o in range(outer):
            r = BS.residual(q_dev, l_dev, classes, BS.levels(q_dev, l_dev, classes, B, g), clip)
            for s in range(sweeps):
                info = host(BS.sweep(r, B, g, lam, impl=impl))
                if info[0] == 0:
                    break
            report[row] = (g, o, s + 1, info[0], *host(BS.cost(r, B, g)))
            row += 1
        if l + 1 < len(levels):
            B = BS.refine(B, shape, g)
    return host(B), report


@pytest.mark.parametrize("sweeps", [2, 16])
def test_fit_equals_the_restatement_and_the_kernels_called_by_hand(sweeps):
    _, labels, q = case(FIT_SHAPE, 1)
    levels = [(32, sweeps, 1), (16, sweeps, 1), (8, sweeps, 1)]
    classes, clip, outer = [1, 2, 3], 2048, 2
    want = ref.fit_ref(q, labels, classes, clip, levels, outer)
    ran = want[1][:6, 2]
    if sweeps == 16:                                                # long enough: rounds end early, and not at their first sweep only
        assert (ran < 16).any() and ((ran > 1) & (ran < 16)).any(), ran
    else:
        assert (ran == 2).all() and (want[1][:6, 3] > 0).all()
    assert (want[1][6:] == -1).all() and want[0].any()
    q_dev, l_dev = dev(q), dev(labels)
    for impl in IMPLS:
        for rep in range(2):
            B, report = BS.fit(q_dev, l_dev, classes, levels, outer, clip, impl=impl)
            assert same(host(B), want[0]) and same(host(report), want[1]), (impl, rep, host(report)[:6], want[1][:6])
    hand = by_hand(q_dev, l_dev, classes, clip, levels, outer, BS.IMPL_NODE)
    assert same(hand[0], want[0]) and same(hand[1], want[1])
    rows = BS.summary(report)
    assert len(rows) == 6 and [r["g"] for r in rows] == [32, 32, 16, 16, 8, 8] and rows[-1]["rms"] < rows[0]["rms"]


# ---- apply -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_apply_with_a_zero_field_returns_the_bits_of_the_volume(shape):
    ss = rev(shape)
    rng = np.random.default_rng(shape[2])
    v = rng.integers(0, 2 ** 32, ss, dtype=np.uint64).astype(np.uint32).view(np.float32)   # every kind of float, signalling NaNs too
    v.reshape(-1)[:3] = np.array([0x7F800001, 0xFFC12345, 0x00000001], np.uint32).view(np.float32)
    for g in SPACINGS:
        for rep in range(2):
            buf, out = guarded(v.size, torch.float32, rep)
            got = BS.apply(dev(v), dev(ref.zero_field(ss, g)), g, out=out)
            assert got.data_ptr() == out.data_ptr() and same(host(got), v), (g, rep)
            intact(buf)
        assert (host(BS.gain(dev(ref.zero_field(ss, g)), g, ss)) == 1).all()


@pytest.mark.parametrize("g", SPACINGS)
@pytest.mark.parametrize("shape", SHAPES)
def test_apply_against_the_restatement(shape, g):
    ss = rev(shape)
    rng = np.random.default_rng(shape[0] + 3 * g)
    v = np.exp2(rng.uniform(-20, 20, ss)).astype(np.float32) * rng.choice(np.array([1, -1], np.float32), ss)
    odd = rng.random(ss) < 0.1
    v[odd] = rng.choice(np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 3e38, 1.2e-38, 1e-40], np.float32), int(odd.sum()))
    v.reshape(-1)[:2] = np.array([0x7F800001, 0xFFC12345], np.uint32).view(np.float32)
    lattice = ref.lattice_ref(ss, g)
    fields = [random_field(rng, ss, g, top) for top in (40, 4000, BS.MAX)] + [np.full(lattice, BS.MAX, np.int32), np.full(lattice, -BS.MAX, np.int32)]
    lo, hi = np.inf, 0.0
    for top, B in enumerate(fields):
        want, want_gain = ref.apply_ref(v, B, g)
        lo, hi = min(lo, float(want_gain.min())), max(hi, float(want_gain.max()))
        assert np.isnan(want).sum() == np.isnan(v).sum() > 0 and np.isinf(want).sum() >= np.isinf(v).sum() > 0
        for rep in range(2):
            buf, out = guarded(v.size, torch.float32, rep)
            gbuf, gout = guarded(v.size, torch.float32, rep)
            got, gain = BS.apply(dev(v), dev(B), g, gain=gout, out=out)
            assert same(host(got), want) and same(host(gain), want_gain), (top, rep)
            intact(buf, gbuf)
            alone = BS.apply(dev(v), dev(B), g)
            assert same(host(alone), want) and same(host(BS.gain(dev(B), g, ss)), want_gain)
    assert lo == 0.25 and hi == 4                                   # k from -2 to +2


# ---- correct ---------------------------------------------------------------------------------------------------------------------------------
def test_correct_equals_its_stages_and_the_restatement_on_the_phantom():
    volume, labels, _ = ref.phantom()
    want = ref.phantom_fit()
    v_dev, l_dev = dev(volume), dev(labels)
    for impl in IMPLS:
        plan = BS.Plan([1, 2], impl=impl)
        out, B, g, report = BS.correct(v_dev, l_dev, plan)
        assert g == want[2] == 8 and same(host(out), want[0]) and same(host(B), want[1]) and same(host(report), want[3]), impl
    q = BS.logcode(v_dev)
    assert same(host(q), ref.logcode_ref(volume))
    B2, report2 = BS.fit(q, l_dev, [1, 2])
    assert same(host(B2), want[1]) and same(host(report2), want[3]) and same(host(BS.apply(v_dev, B2, 8)), want[0])
    before, after = BS.cv(v_dev, l_dev, 1), BS.cv(out, l_dev, 1)
    assert before == ref.cv_ref(volume, labels, 1) and after == ref.cv_ref(want[0], labels, 1) < before


# ---- two streams -----------------------------------------------------------------------------------------------------------------------------
def test_two_fits_on_two_streams_with_separate_scratch():
    cases = [case(FIT_SHAPE, 1), case((21, 29, 37), 2)]
    plans = [([(32, 3, 1), (16, 3, 1), (8, 3, 1)], 2, BS.IMPL_NODE), ([(8, 4, 2), (4, 4, 2)], 1, BS.IMPL_VOXEL)]
    wants = [ref.fit_ref(c[2], c[1], [1, 2, 3], 2048, p[0], p[1]) for c, p in zip(cases, plans)]
    on_dev = [(dev(c[2]), dev(c[1])) for c in cases]
    scratch = [torch.empty(BS.scratch_bytes(c[2].shape, p[0]) + 1, dtype=torch.uint8, device=DEV)[1:] for c, p in zip(cases, plans)]
    torch.cuda.synchronize()
    results, errors = [None, None], []

    def work(k):
        try:
            stream = torch.cuda.Stream(device=DEV)
            with torch.cuda.stream(stream):
                out = [BS.fit(*on_dev[k], [1, 2, 3], plans[k][0], plans[k][1], 2048, impl=plans[k][2], scratch=scratch[k]) for _ in range(4)]
                stream.synchronize()
            results[k] = [(host(B), host(rep)) for B, rep in out]
        except Exception as e:                                       # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for k in range(2):
        for B, rep in results[k]:
            assert same(B, wants[k][0]) and same(rep, wants[k][1]), k
