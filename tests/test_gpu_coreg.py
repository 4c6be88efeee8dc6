"""GPU: the co-registration of two intensity images on the device (include/unet_coreg.h) -- code against code_ref, joint_hist under
IMPL_LDS, IMPL_GLOBAL and the default against hist_ref, scores against Python integers, search against search_ref (the whole trace,
the 12 floats of the map as bits, info), align against space.resample and the phantom's true map; the restatements and the phantom
are those of tests/coreg_ref.py.  Every output is pre-filled with garbage; every comparison is exact equality of bytes.  Shapes are
written (W, H, D) as in the header; the arrays are (D, H, W)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import unet_studio_amd as U
from unet_studio_amd import coreg as CR
from unet_studio_amd import space as SP

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import coreg_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
IMPLS = (CR.IMPL_LDS, CR.IMPL_GLOBAL, CR.IMPL_DEFAULT)
IDENTITY = ref.IDENTITY
STRIDES = (1, 2, 4, 8)
GUARD = 0xA5C3A5C3
F = np.float32


def dev_u8(a):
    return torch.from_numpy(np.ascontiguousarray(a).astype(np.uint8)).to(DEV)


def host(t):
    if t.dtype == torch.uint32:
        return t.view(torch.int32).cpu().numpy().view(np.uint32)
    return t.cpu().numpy()


def same(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()


def shift(tx, ty=0, tz=0):
    return [1, 0, 0, 0, 1, 0, 0, 0, 1, tx, ty, tz]


def stream_ptr():
    return torch.cuda.current_stream().cuda_stream


# ---- code ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bins", [8, 16, 32])
def test_code_edges_lengths_alignments_and_guards(bins):
    rng = np.random.default_rng(bins)
    inf, nan = float("inf"), float("nan")
    for lo, hi in ((0.25, 3.0), (-2.5, -1.0)):
        lo32, hi32 = F(lo), F(hi)
        width = (hi32 - lo32) / F(bins)
        edges = lo32 + width * np.arange(bins + 1, dtype=F)         # the bins' edges, and the values next to them on either side
        special = [lo32, hi32, np.nextafter(lo32, F(-inf)), np.nextafter(lo32, F(inf)), np.nextafter(hi32, F(-inf)), np.nextafter(hi32, F(inf)),
                   F(inf), F(-inf), F(nan), F(-0.0), F(0.0), F(3e38), F(-3e38), F(1e-45), hi32 - width, np.nextafter(hi32 - width, F(-inf))]
        v = np.concatenate([np.array(special, F), edges, np.nextafter(edges, F(-inf)), np.nextafter(edges, F(inf)),
                            rng.uniform(lo - 1, hi + 1, 1100).astype(F)])
        v[rng.integers(len(special) + 3 * (bins + 1), v.size, 40)] = nan
        for n in (1, 63, 1025):
            for roll in (0, 5, 8):                                  # n = 1: lo, the value above hi, NaN
                img = np.ascontiguousarray(np.roll(v, -roll)[:n])
                want = ref.code_ref(img, lo, hi, bins)
                img_dev = torch.from_numpy(img).to(DEV)
                for off in (0, 1, 3):                               # the output at three alignments, between poisoned guard zones
                    G = 32
                    buf = torch.full((n + off + 2 * G,), 0xEE, dtype=torch.uint8, device=DEV)
                    U.engine.check(U.engine.lib.unet_coreg_code(img_dev.data_ptr(), n, lo, hi, bins, buf.data_ptr() + G + off, stream_ptr()))
                    got = buf.cpu().numpy()
                    assert (got[:G + off] == 0xEE).all() and (got[G + off + n:] == 0xEE).all(), (n, off)
                    assert got[G + off:G + off + n].tobytes() == want.tobytes(), (lo, hi, n, roll, off)
        assert set(ref.code_ref(v, lo, hi, bins).tolist()) == set(range(bins + 1))
    img = torch.from_numpy(v[:63].reshape(1, 7, 9).copy()).to(DEV)   # the wrapper: the image's shape, and `out`
    out = torch.full((63,), 0x5A, dtype=torch.uint8, device=DEV)
    got = CR.code(img, lo, hi, bins, out=out)
    assert got.data_ptr() == out.data_ptr() and tuple(got.shape) == (1, 7, 9) and same(host(got), ref.code_ref(v[:63].reshape(1, 7, 9), lo, hi, bins))


# ---- joint_hist ----------------------------------------------------------------------------------------------------------------------
def check_hist(fixed, moving, bins, maps, strides=STRIDES, impls=IMPLS):
    """every implementation twice into garbage against hist_ref, at every stride; every histogram's total is the counted voxels minus
    the skipped ones"""
    f_dev, m_dev = dev_u8(fixed), dev_u8(moving)
    K = len(maps)
    for stride in strides:
        want = ref.hist_ref(fixed, moving, bins, maps, stride)
        assert want.sum((1, 2)).tolist() == [ref.counted_kept(fixed, bins, stride)] * K
        for impl in impls:
            for rep in range(2):
                out = torch.full((K * bins * (bins + 1) * 4,), 0x5A + rep, dtype=torch.uint8, device=DEV).view(torch.uint32)
                got = CR.joint_hist(f_dev, m_dev, bins, maps, stride=stride, impl=impl, out=out)
                assert got.data_ptr() == out.data_ptr()
                assert same(host(got), want), (bins, K, stride, impl, rep)


def geometry_maps(mshape):
    """identity, a half-voxel shift (positions exactly on .5), everything outside, a NaN entry, half outside"""
    mw = mshape[2]
    nan_map = list(IDENTITY)
    nan_map[4] = float("nan")
    return [IDENTITY, shift(0.5, 0.5, 0.5), shift(mw + 3.0, 0, 0), nan_map, shift(mw / 2.0, 0, 0)]


def random_maps(rng, n):
    return [list(np.array(IDENTITY, F) + rng.normal(0, 0.15, 12).astype(F) * ([1] * 9 + [10] * 3)) for _ in range(n)]


def random_codes(rng, shape, bins):
    """runs of equal codes along x (a smooth image) with strays: every code, `none`, and values above bins"""
    D, H, W = shape
    z, y, x = np.indices(shape)
    c = ((x // 3 + y + 2 * z) % bins).astype(np.int64)
    stray = rng.random(shape) < 0.15
    c[stray] = rng.integers(0, bins + 1, int(stray.sum()))
    c[rng.random(shape) < 0.02] = 200
    return c


FSHAPE, MSHAPE = (9, 11, 13), (7, 12, 10)                           # fixed 13 x 11 x 9, moving 10 x 12 x 7


@pytest.mark.parametrize("bins", [8, 16, 32])
def test_hist_bins_k_strides_maps_and_both_impls(bins):
    rng = np.random.default_rng(100 + bins)
    fixed, moving = random_codes(rng, FSHAPE, bins), random_codes(rng, MSHAPE, bins)
    geo = geometry_maps(MSHAPE)
    for m in geo:                                                   # K = 1
        check_hist(fixed, moving, bins, [m])
    many = geo + random_maps(rng, 20)                               # K = 25
    assert len(many) == 25
    check_hist(fixed, moving, bins, many)
    want = ref.hist_ref(fixed, moving, bins, geo)
    inner = want[:, :, :bins].sum((1, 2))
    assert inner[2] == 0 and inner[3] == 0 and 0 < inner[4] < inner[0]         # all outside, NaN, half outside


@pytest.mark.parametrize("bins", [8, 16, 32])
def test_hist_a_constant_pair_none_codes_on_either_side_and_more_than_one_block(bins):
    rng = np.random.default_rng(200 + bins)
    many = geometry_maps(MSHAPE) + random_maps(rng, 20)
    # a constant pair: one counter per map takes every add
    fixed, moving = np.full(FSHAPE, 3), np.full(MSHAPE, bins - 1)
    check_hist(fixed, moving, bins, many, strides=(1, 2))
    assert ref.hist_ref(fixed, moving, bins, [IDENTITY])[0][3, bins - 1] == 7 * 11 * 10
    # `none` everywhere on the fixed side: empty tables; on the moving side: everything in the last column
    codes = random_codes(rng, FSHAPE, bins)
    check_hist(np.full(FSHAPE, bins), random_codes(rng, MSHAPE, bins), bins, many[:3], strides=(1,))
    check_hist(codes, np.full(MSHAPE, 255), bins, many[:3], strides=(1,))
    assert int(ref.hist_ref(codes, np.full(MSHAPE, 255), bins, [IDENTITY])[0][:, :bins].sum()) == 0
    # a grid of several blocks, 25 maps (at 32 bins: two groups of maps in the LDS table), 2 and 14 maps (one group, and 13 + 1)
    big_f, big_m = random_codes(rng, (19, 21, 45), bins), random_codes(rng, (17, 30, 33), bins)
    maps = [IDENTITY, shift(-6.5, 4, -1)] + random_maps(rng, 23)
    check_hist(big_f, big_m, bins, maps, strides=(1, 2), impls=(CR.IMPL_LDS, CR.IMPL_GLOBAL))
    check_hist(big_f, big_m, bins, maps[:14], strides=(1,), impls=(CR.IMPL_LDS,))
    check_hist(big_f, big_m, bins, maps[:2], strides=(1,), impls=(CR.IMPL_LDS,))


@pytest.mark.parametrize("off", [1, 3])
def test_hist_code_pointers_at_odd_addresses_and_guards_around_hist(off):
    rng = np.random.default_rng(20 + off)
    bins = 16
    fixed, moving = random_codes(rng, FSHAPE, bins), random_codes(rng, MSHAPE, bins)
    maps = geometry_maps(MSHAPE) + random_maps(rng, 2)
    K = len(maps)
    flat = np.ascontiguousarray(np.asarray(maps, F).reshape(-1))
    bufs = []
    for img in (fixed, moving):                                     # the codes at an odd address inside a byte buffer
        raw = img.astype(np.uint8).reshape(-1)
        buf = torch.full((raw.size + 16,), 0xEE, dtype=torch.uint8, device=DEV)
        buf[off:off + raw.size] = torch.from_numpy(raw.copy()).to(DEV)
        assert (buf.data_ptr() + off) % 2 == 1
        bufs.append(buf)
    G, n = 64, K * bins * (bins + 1)
    for impl in IMPLS:
        for stride in (1, 2):
            want = ref.hist_ref(fixed, moving, bins, maps, stride)
            for rep in range(2):
                out = torch.full((n + 2 * G,), GUARD - (1 << 32), dtype=torch.int64, device=DEV).to(torch.int32)
                U.engine.check(U.engine.lib.unet_coreg_hist(
                    bufs[0].data_ptr() + off, FSHAPE[2], FSHAPE[1], FSHAPE[0], bufs[1].data_ptr() + off, MSHAPE[2], MSHAPE[1], MSHAPE[0], bins,
                    flat.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), K, stride, out.data_ptr() + 4 * G, impl, None, 0, stream_ptr()))
                got = out.cpu().numpy().view(np.uint32)
                assert (got[:G] == GUARD).all() and (got[G + n:] == GUARD).all()
                assert got[G:G + n].tobytes() == want.tobytes(), (impl, stride, rep)


# ---- scores --------------------------------------------------------------------------------------------------------------------------
def dev_u32(a):
    return torch.from_numpy(np.ascontiguousarray(a).astype(np.int64).astype(np.uint32).view(np.int32)).to(DEV).view(torch.uint32)


def check_scores(tables):
    """the device scores of {K, bins, bins + 1} tables against Python integers, into garbage between guards"""
    tables = np.asarray(tables)
    K = tables.shape[0]
    want = np.array([ref.score_py(t) for t in tables], np.int64)
    G = 8
    buf = torch.full((K + 2 * G,), -0x5A5A5A5A5A5A, dtype=torch.int64, device=DEV)
    got = CR.scores(dev_u32(tables), out=buf[G:G + K])
    torch.cuda.synchronize()
    all_ = buf.cpu().numpy()
    assert (all_[:G] == -0x5A5A5A5A5A5A).all() and (all_[G + K:] == -0x5A5A5A5A5A5A).all()
    assert same(host(got), want), (host(got), want)
    return want


@pytest.mark.parametrize("bins", [8, 16, 32])
def test_scores_of_device_histograms_and_hand_made_tables(bins):
    rng = np.random.default_rng(300 + bins)
    fixed, moving = random_codes(rng, (19, 21, 45), bins), random_codes(rng, (17, 30, 33), bins)
    maps = [IDENTITY, shift(0.5, 0.5, 0.5), shift(40, 0, 0), shift(16, 0, 0)] + random_maps(rng, 21)
    hist = CR.joint_hist(dev_u8(fixed), dev_u8(moving), bins, maps)
    tables = host(hist)
    assert same(tables, ref.hist_ref(fixed, moving, bins, maps))
    want = np.array([ref.score_py(t) for t in tables], np.int64)
    assert same(host(CR.scores(hist)), want) and want[2] == 0 and len(set(want.tolist())) > 20
    assert same(host(CR.scores(hist[3:4].contiguous())), want[3:4])                               # K = 1

    def table(cells):
        h = np.zeros((bins, bins + 1), np.int64)
        for (a, b), n in cells.items():
            h[a, b] = n
        return h
    one = table({(bins - 1, bins - 1): (1 << 31) - 1})                                            # one cell holding 2^31 - 1
    diag = table({(i, i): 1000 + i for i in range(bins)})
    big_diag = table({(i, i): (1 << 30) // bins for i in range(bins)})                            # the largest magnitudes: N = 2^30
    uniform = np.concatenate([np.full((bins, bins), 7), np.zeros((bins, 1), np.int64)], 1)
    empty = table({})
    outside = table({(i, bins): 50 + i for i in range(bins)})                                     # everything in the outside column
    half = diag + outside
    noise = rng.integers(0, 3, (bins, bins + 1))                                                  # small counts: truncation shows, signs mix
    want = check_scores([one, diag, big_diag, uniform, empty, outside, half, noise])
    assert want[0] == 0 and want[4] == 0 and want[5] == 0 and want[1] > 0 and want[6] > 0
    assert want[2] == (1 << 30) // bins * bins * ref.ilog(bins) and abs(int(want[3])) < 7 * bins * bins * 4


# ---- search --------------------------------------------------------------------------------------------------------------------------
def check_search(fixed, moving, bins, init, step=ref.PHANTOM_STEP, stages=ref.PHANTOM_STAGES, max_iterations=400,
                 impls=(CR.IMPL_LDS, CR.IMPL_GLOBAL), want=None, traces=(True, False)):
    want = want or ref.search_ref(fixed, moving, bins, init, step, stages, max_iterations)
    f_dev, m_dev = dev_u8(fixed), dev_u8(moving)
    for impl in impls:
        for with_trace in traces:                                   # trace = NULL
            m, trace, info = CR.search(f_dev, m_dev, bins, init, step=step, stages=stages, max_iterations=max_iterations, impl=impl,
                                       trace=with_trace)
            assert same(host(m), want[0]), (impl, host(m), want[0])
            assert same(host(info), want[2]), (impl, host(info), want[2])
            if with_trace:
                assert same(host(trace), want[1]), impl
            else:
                assert trace is None
    return want


def test_search_the_phantom_at_32_with_the_defaults():
    fixed, moving = ref.phantom_codes(32, 16)
    want = ref.phantom_search(32, 16)
    check_search(fixed, moving, 16, IDENTITY, want=want, impls=IMPLS)
    n = int(want[2][0])
    assert n > 20 and want[2][1] == 1 and (want[1][n:] == -1).all() and (want[1][:n] >= 0).all()
    assert ref.corner_error(want[0], ref.true_map(32), (32, 32, 32)) <= 1.0


@pytest.mark.parametrize("bins", [8, 32])
def test_search_the_small_phantom_at_8_and_32_bins(bins):
    fixed, moving = ref.phantom_codes(16, bins)
    want = check_search(fixed, moving, bins, IDENTITY, traces=(True,))
    assert want[2][0] > 10


def test_search_a_frozen_matrix_a_budget_and_the_last_allowed_iteration():
    fixed, moving = ref.phantom_codes(16, 16)
    # a zero matrix step: a translation-only search, K = 7, the matrix stays as it was given
    start = [1.05, 0.02, 0, -0.03, 0.98, 0, 0, 0, 1, -0.5, 0.25, 0]
    frozen = check_search(fixed, moving, 16, start, step=[0] * 9 + [4, 4, 4])
    n = int(frozen[2][0])
    assert frozen[2][1] == 1 and frozen[1][:n, 2].max() <= 6 and set(frozen[1][:n, 2].tolist()) - {0}
    assert frozen[0][:9].tobytes() == np.array(start[:9], F).tobytes()
    # max_iterations cuts the run short: converged = 0; in the full run the rows never reached hold -1
    full = check_search(fixed, moving, 16, IDENTITY)
    n = int(full[2][0])
    assert full[2][1] == 1 and 3 < n < 400 and (full[1][n:] == -1).all()
    cut = check_search(fixed, moving, 16, IDENTITY, max_iterations=3, traces=(True,))
    assert cut[2].tolist()[:2] == [3, 0] and same(cut[1], full[1][:3])
    # the last allowed iteration finishes the last stage: converged = 1; one fewer: not
    assert check_search(fixed, moving, 16, IDENTITY, max_iterations=n, traces=(True,))[2].tolist()[:2] == [n, 1]
    assert check_search(fixed, moving, 16, IDENTITY, max_iterations=n - 1, traces=(True,))[2].tolist()[:2] == [n - 1, 0]
    check_search(fixed, moving, 16, IDENTITY, max_iterations=1, traces=(True,))
    # four stages, every stride, the deepest level, one parameter of each kind
    check_search(fixed, moving, 16, IDENTITY, step=[0.25, 0, 0, 0, 0, 0, 0, 0, 0.5, 0, 2, 0], stages=[(8, 0, 0), (2, 0, 5), (1, 3, 20), (4, 20, 20)],
                 max_iterations=70, impls=(CR.IMPL_LDS,), traces=(True,))


def test_search_on_a_second_stream_with_its_own_scratch():
    fixed, moving = ref.phantom_codes(16, 16)
    starts = (IDENTITY, shift(1, -1, 0.5))
    wants = [ref.search_ref(fixed, moving, 16, s, max_iterations=60) for s in starts]
    assert not same(wants[0][1], wants[1][1])
    f_dev, m_dev = dev_u8(fixed), dev_u8(moving)
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(device=DEV) for _ in starts]
    got = []
    for s, start in zip(streams, starts):                           # both enqueued before either is waited for
        with torch.cuda.stream(s):
            scratch = torch.empty(CR.coreg_scratch_bytes(f_dev.numel(), 16, 60) + 3, dtype=torch.uint8, device=DEV)[3:]   # any alignment
            got.append((CR.search(f_dev, m_dev, 16, start, max_iterations=60, scratch=scratch, stream=s.cuda_stream), scratch))
    for s in streams:
        s.synchronize()
    for (res, _), want in zip(got, wants):
        assert same(host(res[0]), want[0]) and same(host(res[1]), want[1]) and same(host(res[2]), want[2])


# ---- align ---------------------------------------------------------------------------------------------------------------------------
def test_align_the_phantom_and_an_image_with_itself():
    fixed, moving = ref.phantom(32)
    f_dev, m_dev = torch.from_numpy(fixed.copy()).to(DEV), torch.from_numpy(moving.copy()).to(DEV)
    map_dev, info, moved = CR.align(m_dev, (1, 1, 1), f_dev, (1, 1, 1))
    m, info_h = host(map_dev), host(info)
    assert map_dev.is_cuda and m.dtype == np.float32 and m.shape == (12,) and info_h.dtype == np.int64
    # moved is space.resample through the returned map, bit for bit
    again = SP.resample(m_dev, (32, 32, 32), (m[:9], m[9:]), mode="linear")
    assert tuple(moved.shape) == (32, 32, 32) and same(host(moved), host(again))
    err = ref.corner_error(m, ref.true_map(32), (32, 32, 32))
    print("align: %d iterations, converged %d, corner error %.3f voxel" % (info_h[0], info_h[1], err))
    assert info_h[1] == 1
    assert err <= 1.0
    # the steps in their order: the device's ranges, the restatement's codes and search from centre_init
    ranges = [CR.robust_range(f_dev), CR.robust_range(m_dev)]
    for (lo, hi), img in zip(ranges, (fixed, moving)):
        q = np.quantile(img.astype(np.float64), [0.01, 0.99])
        assert abs(lo - q[0]) < 0.02 and abs(hi - q[1]) < 0.02 and lo < hi
    fc, mc = ref.code_ref(fixed, *ranges[0], 16), ref.code_ref(moving, *ranges[1], 16)
    assert same(host(CR.code(f_dev, *ranges[0], 16)), fc) and same(host(CR.code(m_dev, *ranges[1], 16)), mc)
    want = ref.search_ref(fc, mc, 16, IDENTITY)
    assert same(m, want[0]) and same(info_h, want[2])
    # an image with itself, from the identity: candidate 0 at every level, the state stays where it was
    map_dev, info, moved = CR.align(f_dev, (1, 1, 1), f_dev, (1, 1, 1), init=IDENTITY)
    assert host(map_dev).tolist() == IDENTITY and host(info).tolist()[:2] == [4 + 6, 1] and host(info)[3] == 1
    assert same(host(moved), host(SP.resample(f_dev, (32, 32, 32), (IDENTITY[:9], IDENTITY[9:]), mode="linear")))
