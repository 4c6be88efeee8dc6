"""GPU: the non-linear refinement of a co-registration on the device (include/unet_cowarp.h) -- hist, weights, sweep, fit and resample
under IMPL_NODE, IMPL_VOXEL and the default against the numpy restatements of tests/cowarp_ref.py, the zero field against the
existing coreg.joint_hist and space.resample kernels, and coreg.align(warp=...) against the stages called by hand.  Every case runs
twice into garbage-filled outputs; every comparison is exact equality of bytes.  Shapes are written (W, H, D) as in the header; the
arrays are (D, H, W)."""
import ctypes
import os
import sys
import threading

import numpy as np
import pytest
import torch

import unet_studio_amd as U
from unet_studio_amd import coreg as CR
from unet_studio_amd import cowarp as CW
from unet_studio_amd import space as SP
from unet_studio_amd import warp as W

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import coreg_ref as cr  # noqa: E402
import cowarp_ref as ref  # noqa: E402
import test_gpu_register as gr  # noqa: E402
import warp_ref as wr  # noqa: E402
from test_gpu_register import geometry_maps, host, same, solid  # noqa: E402
from test_register_host import IDENTITY, TRUE_MAP, shift  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
IMPLS = (CW.IMPL_NODE, CW.IMPL_VOXEL, CW.IMPL_DEFAULT)
FIXED = [(1, 1, 1), (7, 5, 3), (33, 9, 9), (65, 3, 2), (40, 44, 38)]
MOVING = [(1, 1, 1), (5, 7, 3), (40, 48, 36)]
CASES = [(f, m, g) for f in FIXED for m in MOVING for g in (4, 8, 16)]
BINS = (8, 16, 32)
BIG = 1 << 20
G = 64                                                             # guard words on each side
GUARD16, GUARD32, GUARD64 = 0x25C3, 0x25C3A5C3, 0x25C3A5C3A5C3A5C3
_fp, _ip = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int)


def garbage(shape, dtype, rep):
    """a device tensor of `dtype` whose every byte is 0x5A + rep"""
    n = int(np.prod(shape)) * torch.empty(0, dtype=dtype).element_size()
    return torch.full((n,), 0x5A + rep, dtype=torch.uint8, device=DEV).view(dtype).view(shape)


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)         # a copy: the shared cases are read only


def codes(rng, shape, bins):
    """nested shells of codes (long runs along x) with 2 % strays, among them `bins`, values above it and 255"""
    c = solid(rng, shape, bins).astype(np.uint8)
    c[rng.random(shape) < 0.01] = 255
    return c


def fields(rng, fshape, g, limit):
    """zero, uniform random within `limit` of each other (half the limit about 0), random at +-32767 (for a limit that forbids nothing)"""
    shape = wr.lattice_ref(fshape, g) + (3,)
    return [np.zeros(shape, np.int32), rng.integers(-(limit // 2), limit // 2 + 1, shape).astype(np.int32),
            (rng.integers(0, 2, shape) * 65534 - 32767).astype(np.int32)]


def check_hist_and_weights(f_dev, m_dev, fixed, moving, bins, m, D, g):
    want = ref.hist_ref(fixed, moving, bins, m, D, g)
    want_w = ref.weights_ref(want)
    d_dev = dev(D)
    for rep in range(2):
        out = garbage((bins * (bins + 1),), torch.uint32, rep)
        got = CW.hist(f_dev, m_dev, bins, m, d_dev, g, out=out)
        assert got.data_ptr() == out.data_ptr() and same(host(got), want), (bins, g, rep)
        out_w = garbage((bins * (bins + 1),), torch.int16, rep)
        got_w = CW.weights(got, out=out_w)
        assert got_w.data_ptr() == out_w.data_ptr() and same(host(got_w), want_w), (bins, g, rep)
    assert int(want.sum()) == int((cr.read_code(fixed, bins) < bins).sum())
    return want


def check_sweep(f_dev, m_dev, fixed, moving, bins, m, D, g, step, limit, impls=IMPLS):
    want_d, want_info = ref.sweep_ref(fixed, moving, bins, m, D, g, step, limit, check_total=False)
    for impl in impls:
        for rep in range(2):
            d_dev = dev(D)
            info = CW.sweep(f_dev, m_dev, bins, m, d_dev, g, step, limit, impl=impl)
            assert same(host(d_dev), want_d), (bins, g, step, limit, impl, rep)
            assert same(host(info), want_info), (bins, g, step, limit, impl, rep, host(info), want_info)
    return want_d, want_info


def check_resample(v_dev, volume, fshape, m, D, g):
    want = ref.resample_ref(volume, fshape, m, D, g)
    d_dev = dev(D)
    for rep in range(2):
        out = garbage((int(np.prod(fshape)),), torch.float32, rep)
        got = CW.resample(v_dev, fshape, m, d_dev, g, out=out)
        assert got.data_ptr() == out.data_ptr() and same(host(got), want), (g, rep)
    return want


# ---- hist, weights, sweep and resample over the shapes ----------------------------------------------------------------------------------
@pytest.mark.parametrize("fshape,mshape,g", CASES)
def test_hist_weights_sweep_and_resample_shapes_fields_maps_and_bins(fshape, mshape, g):
    (fw, fh, fd), (mw, mh, md) = fshape, mshape
    rng = np.random.default_rng(fw * 1000 + mw * 10 + g)
    fs, ms = (fd, fh, fw), (md, mh, mw)
    images = {b: (codes(rng, fs, b), codes(rng, ms, b)) for b in BINS}
    on_dev = {b: (dev(f), dev(m)) for b, (f, m) in images.items()}
    volume = rng.standard_normal(ms).astype(np.float32)
    v_dev = dev(volume)
    maps = geometry_maps(fs, ms)                                   # identity, half-voxel shifts, outside, NaN, x3, 1/3, shear
    limit = 64 * g
    big = fd * fh * fw > 10000                                      # the large fixed grid: fewer combinations, every path still
    zero, within, extreme = fields(rng, fs, g, limit)
    for k, D in enumerate((zero, within, extreme)):
        for j, m in enumerate(maps):
            for b in (BINS[(j + k) % 3],) if big else BINS:
                check_hist_and_weights(*on_dev[b], *images[b], b, m, D, g)
            if not big or j in (0, 3, 6, 9):
                check_resample(v_dev, volume, fs, m, D, g)
    for k, (D, lim) in enumerate(((zero, limit), (within, limit), (extreme, BIG))):
        for j, m in enumerate((maps[-1],) if big else (maps[0], maps[1], maps[4], maps[6], maps[7], maps[-1])):
            b = BINS[(j + k) % 3]
            check_sweep(*on_dev[b], *images[b], b, m, D, g, 64, lim)
    # a fixed image that is all "none" (the code `bins`, and values above it): an empty histogram, zero weights, nothing visited
    b = BINS[g % 3]
    none = np.where(rng.random(fs) < 0.5, b, 255).astype(np.uint8)
    hist = check_hist_and_weights(dev(none), on_dev[b][1], none, images[b][1], b, maps[-1], within, g)
    _, info = check_sweep(dev(none), on_dev[b][1], none, images[b][1], b, maps[-1], within, g, 64, limit)
    assert not hist.any() and info.tolist() == [0, 0]


@pytest.mark.parametrize("off", [1, 3])
@pytest.mark.parametrize("bins", BINS)
def test_code_pointers_and_scratch_off_alignment_and_guards_around_every_output(bins, off):
    rng = np.random.default_rng(20 + off + bins)
    fshape, mshape, g = (9, 9, 33), (3, 7, 5), 8
    fixed, moving = codes(rng, fshape, bins), codes(rng, mshape, bins)
    m = [0.15, 0.01, 0, 0, 0.7, 0, 0, 0.02, 0.3, 0, 0, 0]
    flat = np.ascontiguousarray(np.asarray(m, np.float32))
    bufs = []
    for img in (fixed, moving):                                    # the image's bytes at an odd address inside a byte buffer
        buf = torch.full((img.size + 16,), 0xEE, dtype=torch.uint8, device=DEV)
        buf[off:off + img.size] = dev(img.reshape(-1))
        bufs.append(buf)
    grids = (bufs[0].data_ptr() + off, fshape[2], fshape[1], fshape[0], bufs[1].data_ptr() + off, mshape[2], mshape[1], mshape[0])
    stream = torch.cuda.current_stream().cuda_stream
    lib, check = U.engine.lib, U.engine.check
    D = fields(rng, fshape, g, 512)[1]
    levels = np.asarray([(8, 128, 64, 2, 512), (4, 64, 64, 1, 256)], np.int32)
    cells = bins * (bins + 1)
    want_hist = ref.hist_ref(fixed, moving, bins, m, D, g)
    want_w = ref.weights_ref(want_hist)
    want_d, want_info = ref.sweep_ref(fixed, moving, bins, m, D, g, 128, 512)
    want_fit, want_report = ref.fit_ref(fixed, moving, bins, m, [tuple(int(v) for v in lv) for lv in levels])
    scratch = torch.empty(CW.scratch_bytes(fshape, bins, levels) + 8, dtype=torch.uint8, device=DEV)

    def guarded(values, n, dtype=torch.int32, guard=GUARD32):
        buf = torch.full((n + 2 * G,), guard, dtype=dtype, device=DEV)
        if values is not None:
            buf[G:G + n] = dev(np.ascontiguousarray(values).reshape(-1))
        return buf

    def inner(buf, n):
        got = buf.cpu().numpy()
        guard = {2: GUARD16, 4: GUARD32, 8: GUARD64}[got.itemsize]
        assert (got[:G] == guard).all() and (got[G + n:] == guard).all()
        return got[G:G + n]

    for impl in IMPLS:
        for rep in range(2):
            hist, d_in = guarded(None, cells), guarded(D, D.size)
            check(lib.unet_cowarp_hist(*grids, bins, flat.ctypes.data_as(_fp), d_in.data_ptr() + 4 * G, g, hist.data_ptr() + 4 * G, stream))
            assert inner(hist, cells).view(np.uint32).tobytes() == want_hist.tobytes()
            wts = guarded(None, cells, torch.int16, GUARD16)
            check(lib.unet_cowarp_weights(hist.data_ptr() + 4 * G, bins, wts.data_ptr() + 2 * G, stream))
            assert inner(wts, cells).tobytes() == want_w.tobytes()
            info = guarded(None, 2, torch.int64, GUARD64)
            check(lib.unet_cowarp_sweep(*grids, bins, flat.ctypes.data_as(_fp), d_in.data_ptr() + 4 * G, g, 128, 512, info.data_ptr() + 8 * G, impl,
                                        scratch.data_ptr() + off, scratch.nbytes - off, stream))
            assert inner(d_in, D.size).tobytes() == want_d.tobytes() and inner(info, 2).tobytes() == want_info.tobytes(), (impl, rep)
            d_out = guarded(None, want_fit.size)
            report = guarded(None, CW.MAX_ROWS * 5, torch.int64, GUARD64)
            check(lib.unet_cowarp_fit(*grids, bins, flat.ctypes.data_as(_fp), levels.ctypes.data_as(_ip), 2, d_out.data_ptr() + 4 * G,
                                      report.data_ptr() + 8 * G, impl, scratch.data_ptr() + off, scratch.nbytes - off, stream))
            assert inner(d_out, want_fit.size).tobytes() == want_fit.tobytes(), (impl, rep)
            assert inner(report, CW.MAX_ROWS * 5).tobytes() == want_report.tobytes(), (impl, rep)
    # resample: guards around the output
    volume = rng.standard_normal(mshape).astype(np.float32)
    want = ref.resample_ref(volume, fshape, m, want_fit, 4)
    v_dev, d_dev = dev(volume), dev(want_fit)
    for rep in range(2):
        out = torch.full((fixed.size + 2 * G,), 0x5A5A5A5A + rep, dtype=torch.int32, device=DEV)
        check(lib.unet_cowarp_resample(v_dev.data_ptr(), mshape[2], mshape[1], mshape[0], fshape[2], fshape[1], fshape[0],
                                       flat.ctypes.data_as(_fp), d_dev.data_ptr(), 4, out.data_ptr() + 4 * G, stream))
        got = out.cpu().numpy()
        assert (got[:G] == 0x5A5A5A5A + rep).all() and (got[G + fixed.size:] == 0x5A5A5A5A + rep).all()
        assert got[G:G + fixed.size].view(np.float32).tobytes() == want.tobytes()


# ---- the existing kernels as an independent witness ------------------------------------------------------------------------------------
@pytest.mark.parametrize("g", [4, 8, 16])
def test_a_zero_field_equals_coreg_joint_hist_and_space_resample(g):
    rng = np.random.default_rng(g)
    for fshape, mshape in (((9, 9, 33), (3, 7, 5)), ((38, 44, 40), (36, 48, 40)), ((1, 1, 1), (1, 1, 1))):
        volume = dev(rng.standard_normal(mshape).astype(np.float32))
        zero = torch.zeros(wr.lattice_ref(fshape, g) + (3,), dtype=torch.int32, device=DEV)
        for bins in BINS:
            f_dev, m_dev = dev(codes(rng, fshape, bins)), dev(codes(rng, mshape, bins))
            for m in geometry_maps(fshape, mshape):
                assert same(host(CW.hist(f_dev, m_dev, bins, m, zero, g)), host(CR.joint_hist(f_dev, m_dev, bins, [m], stride=1))[0])
        for m in geometry_maps(fshape, mshape):
            if np.isfinite(m).all():                               # space.resample refuses a map that is not finite
                assert same(host(CW.resample(volume, fshape, m, zero, g)), host(SP.resample(volume, fshape, (m[:9], m[9:]), mode="linear")))


# ---- sweep: the steps and the limit --------------------------------------------------------------------------------------------------------
def test_sweep_at_step_1_at_16384_and_with_a_limit_of_0():
    fixed, moving = ref.warped_codes()
    f_dev, m_dev = dev(fixed), dev(moving)
    rng = np.random.default_rng(2)
    for g, first in ((16, 512), (4, 128)):
        within = fields(rng, fixed.shape, g, 64 * g)[1]
        limit = wr.default_limit_ref(TRUE_MAP, g)
        for D in (wr.zero_field(fixed.shape, g), within):
            for step in (1, first):
                want_d, info = check_sweep(f_dev, m_dev, fixed, moving, 16, TRUE_MAP, D, g, step, limit)
                assert step == 1 or info[0] > 0                    # the warped case: a coarse step moves nodes
        # the largest step of a schedule, 64 moving voxels: only a limit that forbids nothing admits it
        want_d, info = check_sweep(f_dev, m_dev, fixed, moving, 16, TRUE_MAP, within, g, 16384, BIG, impls=IMPLS[:2])
        want_d, info = check_sweep(f_dev, m_dev, fixed, moving, 16, TRUE_MAP, within, g, 16384, limit, impls=IMPLS[:2])
        assert info[0] == 0 and same(want_d, within)
        # a limit of 0: a moved candidate differs from a neighbour by the step at least, nothing may move
        want_d, info = check_sweep(f_dev, m_dev, fixed, moving, 16, TRUE_MAP, wr.zero_field(fixed.shape, g), g, first, 0)
        assert not want_d.any() and info[0] == 0 and info[1] > 0


# ---- fit ---------------------------------------------------------------------------------------------------------------------------------
def check_fit(fixed, moving, bins, m, levels, want, impls=IMPLS):
    f_dev, m_dev = dev(fixed), dev(moving)
    for impl in impls:
        D, report = CW.fit(f_dev, m_dev, bins, m, levels=levels, impl=impl)
        assert same(host(D), want[0]), impl
        assert same(host(report), want[1]), (impl, host(report)[:10], want[1][:10])


def test_fit_the_warped_contrast_pair_with_the_defaults():
    fixed, moving = ref.warped_codes()
    want = ref.warped_fit()
    check_fit(fixed, moving, 16, TRUE_MAP, None, want)
    rows = want[1][want[1][:, 0] >= 0]
    assert len(rows) == 8 and rows[-1, 4] > rows[0, 4]
    # the field is the tissue warp's: its refine takes it
    coarse = ref.fit_ref(fixed, moving, 16, TRUE_MAP, [(16, 512, 512, 1, 974)])[0]
    assert same(host(W.refine(dev(coarse), fixed.shape, 16)), wr.refine_ref(coarse, fixed.shape, 16))


def small_codes(bins=8):
    """(12, 10, 8) -> (10, 12, 9): test_gpu_register's small pair in two contrasts"""
    subject, template = gr.small_pair()
    rng = np.random.default_rng(7)
    fixed = cr.code_ref(np.asarray([0.1, 0.5, 0.9])[subject] + rng.normal(0, 0.05, subject.shape), 0, 1, bins)
    moving = cr.code_ref(np.asarray([0.2, 0.9, 0.4])[template] + rng.normal(0, 0.05, template.shape), 0, 1, bins)
    return fixed, moving


def test_fit_one_level_lists_one_sweep_and_a_schedule_whose_first_sweeps_change_nothing():
    fixed, moving = small_codes()
    for levels in ([(8, 256, 64, 3, 400)], [(4, 128, 128, 1, 200)], [(16, 512, 256, 2, 900), (8, 128, 128, 16, 400), (4, 64, 32, 2, 200)],
                   [(16, 16384, 8192, 1, BIG), (8, 1, 1, 2, 0), (4, 2, 1, 16, 3)]):
        want = ref.fit_ref(fixed, moving, 8, IDENTITY, levels)
        check_fit(fixed, moving, 8, IDENTITY, levels, want)
        assert want[0].any()
    # a limit of 0 admits no move: every first sweep changes nothing and is the only one run, the score stays the affine one
    levels = [(8, 256, 64, 6, 0), (4, 128, 64, 6, 0)]
    want = ref.fit_ref(fixed, moving, 8, IDENTITY, levels)
    rows = want[1][want[1][:, 0] >= 0]
    affine = cr.score_ref(ref.hist_ref(fixed, moving, 8, IDENTITY, wr.zero_field(fixed.shape, 8), 8))
    assert not want[0].any() and len(rows) == 5 and (rows[:, 2] == 1).all() and (rows[:, 3] == 0).all() and (rows[:, 4] == affine).all()
    check_fit(fixed, moving, 8, IDENTITY, levels, want)
    # a step of 1 changes nothing on the first level here, then the second level moves: the early end is per (level, step)
    levels = [(8, 1, 1, 6, 400), (4, 128, 64, 3, 200)]
    want = ref.fit_ref(fixed, moving, 8, shift(1.5, -1, 0.5), levels)
    rows = want[1][want[1][:, 0] >= 0]
    assert rows[0, 2:4].tolist() == [1, 0] and rows[1, 2] == 3 and rows[1, 3] > 0 and want[0].any()
    check_fit(fixed, moving, 8, shift(1.5, -1, 0.5), levels, want)


def test_fit_two_threads_on_two_streams_with_their_own_scratch():
    fixed, moving = small_codes()
    plans = ([(8, 256, 64, 3, 400), (4, 128, 64, 2, 200)], [(16, 512, 128, 2, 900), (8, 256, 256, 4, 400)])
    wants = [ref.fit_ref(fixed, moving, 8, IDENTITY, lv) for lv in plans]
    f_dev, m_dev = dev(fixed), dev(moving)
    torch.cuda.synchronize()
    results, errors = [None, None], []

    def work(k):
        try:
            stream = torch.cuda.Stream(device=DEV)
            with torch.cuda.stream(stream):
                scratch = torch.empty(CW.scratch_bytes(fixed.shape, 8, plans[k]), dtype=torch.uint8, device=DEV)
                out = []
                for _ in range(5):
                    impl = CW.IMPL_NODE if k == 0 else CW.IMPL_VOXEL
                    out.append(CW.fit(f_dev, m_dev, 8, IDENTITY, levels=plans[k], impl=impl, scratch=scratch))
                stream.synchronize()
            results[k] = [(host(d), host(r)) for d, r in out]
        except Exception as e:                                       # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for k in range(2):
        for d, r in results[k]:
            assert same(d, wants[k][0]) and same(r, wants[k][1]), k


# ---- coreg.align ---------------------------------------------------------------------------------------------------------------------------
SHORT = dict(stages=[(2, 0, 1)], max_iterations=12)                 # a search of a few iterations
SHORT_PLAN = CW.Plan(levels=[(8, 256, 128, 2), (4, 128, 128, 1)])


def test_align_with_a_warp_plan_against_the_stages_called_by_hand():
    fixed, moving = cr.phantom(32)
    f_dev, m_dev = dev(fixed.copy()), dev(moving.copy())
    plain = CR.align(m_dev, (1, 1, 1), f_dev, (1, 1, 1), **SHORT)
    none = CR.align(m_dev, (1, 1, 1), f_dev, (1, 1, 1), warp=None, **SHORT)
    assert len(plain) == len(none) == 3 and all(same(host(a), host(b)) for a, b in zip(plain, none))
    m = host(plain[0])
    fc, mc = CR.code(f_dev, *CR.robust_range(f_dev), 16), CR.code(m_dev, *CR.robust_range(m_dev), 16)
    levels = wr.levels_ref(m, SHORT_PLAN.levels)
    want_d, want_report = ref.fit_ref(host(fc), host(mc), 16, m, levels)
    affine = cr.score_ref(ref.hist_ref(host(fc), host(mc), 16, m, wr.zero_field(fixed.shape, 8), 8))
    for impl in IMPLS:
        for _ in range(2):
            map_dev, info, moved, w = CR.align(m_dev, (1, 1, 1), f_dev, (1, 1, 1), warp=SHORT_PLAN._replace(impl=impl), **SHORT)
            assert same(host(map_dev), m) and same(host(info), host(plain[1]))
            assert w["g"] == 4 and same(host(w["field"]), want_d) and same(host(w["report"]), want_report)
            assert host(w["score_affine"]).tolist() == [affine] and host(w["score_warped"]).tolist() == [int(want_report[2, 4])]
            assert int(w["max_disp_q8"]) == int(np.abs(want_d).max()) > 0
            # the stages by hand: fit on the code images, resample through map + field
            D, report = CW.fit(fc, mc, 16, m, levels=SHORT_PLAN.levels, impl=impl)
            assert same(host(D), want_d) and same(host(report), want_report)
            assert same(host(moved), host(CW.resample(m_dev, fixed.shape, m, D, 4)))
            assert same(host(moved), ref.resample_ref(moving, fixed.shape, m, want_d, 4)) and not same(host(moved), host(plain[2]))
