"""GPU: the non-linear refinement of a parcellation on the device (include/unet_warp.h) -- hist, sweep, refine, fit and carry under
IMPL_NODE, IMPL_VOXEL and the default against the numpy restatements of tests/warp_ref.py, the zero field against the existing
register kernels, parcellate(warp=...) against search_ref -> fit_ref -> carry_ref -> grow_ref, and EvaluateUNet(atlas_warp=...).
Every case runs twice into garbage-filled outputs; every comparison is exact equality of bytes.  Shapes are written (W, H, D) as in
the header; the arrays are (D, H, W)."""
import ctypes
import os
import sys
import threading

import numpy as np
import pytest
import torch

import unet_studio_amd as U
from unet_studio_amd import atlas as A
from unet_studio_amd import register as R
from unet_studio_amd import warp as W

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_register as gr  # noqa: E402
import warp_ref as ref  # noqa: E402
from test_atlas_host import grow_ref  # noqa: E402
from test_gpu_register import dev_int, geometry_maps, host, same, solid  # noqa: E402
from test_register_host import IDENTITY, TRUE_MAP, search_ref, shift  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
IMPLS = (W.IMPL_NODE, W.IMPL_VOXEL, W.IMPL_DEFAULT)
SUBJECTS = [(1, 1, 1), (7, 5, 3), (33, 9, 9), (65, 3, 2), (40, 44, 38)]
TEMPLATES = [(1, 1, 1), (5, 7, 3), (40, 48, 36)]
CASES = [(s, t, g) for s in SUBJECTS for t in TEMPLATES for g in (4, 8, 16, 32) if g < 32 or s in ((65, 3, 2), (40, 44, 38))]
BIG = 1 << 20
G = 64                                                             # guard words on each side
GUARD32, GUARD64 = 0x25C3A5C3, 0x25C3A5C3A5C3A5C3
_fp, _ip = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int)


def garbage(shape, dtype, rep):
    """a device tensor of `dtype` whose every byte is 0x5A + rep"""
    n = int(np.prod(shape)) * torch.empty(0, dtype=dtype).element_size()
    return torch.full((n,), 0x5A + rep, dtype=torch.uint8, device=DEV).view(dtype).view(shape)


def fields(rng, sshape, g, limit):
    """zero, uniform random within `limit` of each other (half the limit about 0), random at +-32767 (for a limit that forbids nothing)"""
    shape = ref.lattice_ref(sshape, g) + (3,)
    return [np.zeros(shape, np.int32), rng.integers(-(limit // 2), limit // 2 + 1, shape).astype(np.int32),
            (rng.integers(0, 2, shape) * 65534 - 32767).astype(np.int32)]


def check_hist(s_dev, t_dev, subject, template, T, m, D, g):
    want = ref.hist_ref(subject, template, T, m, D, g)
    d_dev = torch.from_numpy(D).to(DEV)
    for rep in range(2):
        out = garbage((T * T,), torch.uint32, rep)
        got = W.hist(s_dev, t_dev, T, m, d_dev, g, out=out)
        assert got.data_ptr() == out.data_ptr() and same(host(got), want), (g, rep)
    assert int(want.sum()) == subject.size
    return want


def check_sweep(s_dev, t_dev, subject, template, T, m, D, g, step, limit, impls=IMPLS):
    want_d, want_info = ref.sweep_ref(subject, template, T, m, D, g, step, limit)
    for impl in impls:
        for rep in range(2):
            d_dev = torch.from_numpy(D).to(DEV)
            info = W.sweep(s_dev, t_dev, T, m, d_dev, g, step, limit, impl=impl)
            assert same(host(d_dev), want_d), (g, step, limit, impl, rep)
            assert same(host(info), want_info), (g, step, limit, impl, rep, host(info), want_info)
    return want_d, want_info


def check_carry(s_dev, t_dev, a_dev, subject, template, atlas, T, m, D, g):
    want, counts = ref.carry_ref(subject, template, atlas, T, m, D, g)
    d_dev = torch.from_numpy(D).to(DEV)
    for rep in range(2):
        out = garbage((subject.size,), torch.uint16, rep)
        got, cnt = W.carry(s_dev, t_dev, a_dev, T, m, d_dev, g, out=out)
        assert got.data_ptr() == out.data_ptr() and same(host(got), want) and same(host(cnt), counts), (g, rep)
    got, cnt = W.carry(s_dev, t_dev, a_dev, T, m, d_dev, g, counts=False)
    assert cnt is None and same(host(got), want)
    return want, counts


def check_refine(D, sshape, g):
    want = ref.refine_ref(D, sshape, g)
    d_dev = torch.from_numpy(D).to(DEV)
    for rep in range(2):
        out = garbage(want.shape, torch.int32, rep)
        got = W.refine(d_dev, sshape, g, out=out.view(-1))
        assert got.data_ptr() == out.data_ptr() and same(host(got), want), (g, rep)


# ---- hist, sweep, refine and carry over the shapes ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("sshape,tshape,g", CASES)
def test_hist_sweep_refine_and_carry_shapes_fields_and_maps(sshape, tshape, g):
    (sw, sh, sd), (tw, th, td) = sshape, tshape
    rng = np.random.default_rng(sw * 1000 + tw * 10 + g)
    subject, template = solid(rng, (sd, sh, sw), 5), solid(rng, (td, th, tw), 5)
    atlas = np.where(template > 0, rng.integers(0, 4, template.shape), 0)
    s_dev, t_dev, a_dev = dev_int(subject, torch.uint8), dev_int(template, torch.uint8), dev_int(atlas, torch.uint16)
    maps = geometry_maps(subject.shape, template.shape)            # identity, half-voxel shifts, outside, NaN, x3, 1/3, shear
    limit = 64 * g
    zero, within, extreme = fields(rng, subject.shape, g, limit)
    for D in (zero, within, extreme):
        for m in maps:
            check_hist(s_dev, t_dev, subject, template, 5, m, D, g)
        if g > 4:
            check_refine(D, subject.shape, g)
    big = subject.size > 10000                                      # the large subject: fewer combinations, every path still
    for m in (maps[0], maps[-1]) if big else maps:
        check_carry(s_dev, t_dev, a_dev, subject, template, atlas, 5, m, within, g)
    check_carry(s_dev, t_dev, a_dev, subject, template, atlas, 5, maps[-1], extreme, g)
    for D, lim in ((zero, limit), (within, limit), (extreme, BIG)):
        for m in ((maps[-1],) if big else (maps[0], maps[1], maps[4], maps[6], maps[7], maps[-1])):
            check_sweep(s_dev, t_dev, subject, template, 5, m, D, g, 64, lim)


@pytest.mark.parametrize("tdt", [torch.uint8, torch.uint16])
@pytest.mark.parametrize("sdt", [torch.uint8, torch.uint16])
def test_uint8_and_uint16_tissue_with_values_of_t_or_more(sdt, tdt):
    rng = np.random.default_rng(11)
    subject, template = solid(rng, (9, 9, 33), 5), solid(rng, (3, 7, 5), 5)
    for img, dt in ((subject, sdt), (template, tdt)):               # values the type can hold and T cannot
        img[rng.random(img.shape) < 0.05] = 255 if dt == torch.uint8 else 65535
        img[rng.random(img.shape) < 0.05] = 5 if dt == torch.uint8 else 256
    atlas = np.where(template > 0, rng.integers(0, 4, template.shape), 0)
    s_dev, t_dev, a_dev = dev_int(subject, sdt), dev_int(template, tdt), dev_int(atlas, torch.uint16)
    m = [0.15, 0, 0, 0, 0.7, 0, 0, 0, 0.3, 0, 0, 0]                 # everything inside
    for g in (4, 8):
        D = fields(rng, subject.shape, g, 512)[1]
        check_hist(s_dev, t_dev, subject, template, 5, m, D, g)
        check_sweep(s_dev, t_dev, subject, template, 5, m, D, g, 128, 512)
        check_carry(s_dev, t_dev, a_dev, subject, template, atlas, 5, m, D, g)


@pytest.mark.parametrize("off", [1, 3])
@pytest.mark.parametrize("nbytes", [1, 2])
def test_tissue_pointers_off_alignment_and_guards_around_d_hist_info_and_report(nbytes, off):
    rng = np.random.default_rng(20 + off)
    sshape, tshape, T, g = (9, 9, 33), (3, 7, 5), 5, 8
    subject, template = solid(rng, sshape, T), solid(rng, tshape, T)
    np_dt = np.uint8 if nbytes == 1 else np.uint16
    m = [0.15, 0.01, 0, 0, 0.7, 0, 0, 0.02, 0.3, 0, 0, 0]
    flat = np.ascontiguousarray(np.asarray(m, np.float32))
    bufs = []
    for img in (subject, template):                                 # the image's bytes at an odd address inside a byte buffer
        raw = np.frombuffer(img.astype(np_dt).tobytes(), np.uint8)
        buf = torch.full((raw.size + 16,), 0xEE, dtype=torch.uint8, device=DEV)
        buf[off:off + raw.size] = torch.from_numpy(raw.copy()).to(DEV)
        bufs.append(buf)
    grids = (bufs[0].data_ptr() + off, nbytes, sshape[2], sshape[1], sshape[0], bufs[1].data_ptr() + off, nbytes, tshape[2], tshape[1], tshape[0])
    stream = torch.cuda.current_stream().cuda_stream
    lib, check = U.engine.lib, U.engine.check
    D = fields(rng, sshape, g, 512)[1]
    levels = np.asarray([(8, 128, 64, 2, 512), (4, 64, 64, 1, 256)], np.int32)
    want_hist = ref.hist_ref(subject, template, T, m, D, g)
    want_d, want_info = ref.sweep_ref(subject, template, T, m, D, g, 128, 512)
    want_fit, want_report = ref.fit_ref(subject, template, T, m, [tuple(int(v) for v in lv) for lv in levels])
    scratch = torch.empty(W.scratch_bytes(sshape, T, levels) + 8, dtype=torch.uint8, device=DEV)

    def guarded32(values, n):
        buf = torch.full((n + 2 * G,), GUARD32, dtype=torch.int32, device=DEV)
        if values is not None:
            buf[G:G + n] = torch.from_numpy(np.ascontiguousarray(values).reshape(-1)).to(DEV)
        return buf

    def inner(buf, n):
        got = buf.cpu().numpy()
        guard = GUARD32 if got.dtype == np.int32 else GUARD64
        assert (got[:G] == guard).all() and (got[G + n:] == guard).all()
        return got[G:G + n]

    for impl in IMPLS:
        for rep in range(2):
            hist = guarded32(None, T * T)
            d_in = guarded32(D, D.size)
            check(lib.unet_warp_hist(*grids, T, flat.ctypes.data_as(_fp), d_in.data_ptr() + 4 * G, g, hist.data_ptr() + 4 * G, stream))
            assert inner(hist, T * T).view(np.uint32).tobytes() == want_hist.tobytes()
            info = torch.full((2 + 2 * G,), GUARD64, dtype=torch.int64, device=DEV)
            check(lib.unet_warp_sweep(*grids, T, flat.ctypes.data_as(_fp), d_in.data_ptr() + 4 * G, g, 128, 512, info.data_ptr() + 8 * G, impl,
                                      scratch.data_ptr() + off, scratch.nbytes - off, stream))
            assert inner(d_in, D.size).tobytes() == want_d.tobytes() and inner(info, 2).tobytes() == want_info.tobytes(), (impl, rep)
            d_out = guarded32(None, want_fit.size)
            report = torch.full((W.MAX_ROWS * 5 + 2 * G,), GUARD64, dtype=torch.int64, device=DEV)
            check(lib.unet_warp_fit(*grids, T, flat.ctypes.data_as(_fp), levels.ctypes.data_as(_ip), 2, d_out.data_ptr() + 4 * G,
                                    report.data_ptr() + 8 * G, impl, scratch.data_ptr() + off, scratch.nbytes - off, stream))
            assert inner(d_out, want_fit.size).tobytes() == want_fit.tobytes(), (impl, rep)
            assert inner(report, W.MAX_ROWS * 5).tobytes() == want_report.tobytes(), (impl, rep)


# ---- the existing kernels as an independent witness ------------------------------------------------------------------------------------
@pytest.mark.parametrize("g", [4, 8, 16, 32])
def test_a_zero_field_equals_register_joint_hist_and_register_carry(g):
    rng = np.random.default_rng(g)
    for sshape, tshape in (((9, 9, 33), (3, 7, 5)), ((38, 44, 40), (36, 48, 40)), ((1, 1, 1), (1, 1, 1))):
        subject, template = solid(rng, sshape, 5), solid(rng, tshape, 5)
        atlas = np.where(template > 0, rng.integers(0, 4, template.shape), 0)
        s_dev, t_dev, a_dev = dev_int(subject, torch.uint8), dev_int(template, torch.uint16), dev_int(atlas, torch.uint16)
        zero = torch.zeros(ref.lattice_ref(sshape, g) + (3,), dtype=torch.int32, device=DEV)
        for m in geometry_maps(sshape, tshape):
            assert same(host(W.hist(s_dev, t_dev, 5, m, zero, g)), host(R.joint_hist(s_dev, t_dev, 5, [m], stride=1))[0])
            got, cnt = W.carry(s_dev, t_dev, a_dev, 5, m, zero, g)
            old, old_cnt = R.carry(s_dev, t_dev, a_dev, 5, m)
            assert same(host(got), host(old)) and same(host(cnt), host(old_cnt))


# ---- sweep: the steps and the limit --------------------------------------------------------------------------------------------------------
def test_sweep_at_step_1_at_the_first_step_and_with_a_limit_of_0():
    subject, template = ref.warped_case()
    s_dev, t_dev = dev_int(subject, torch.uint8), dev_int(template, torch.uint8)
    rng = np.random.default_rng(2)
    for g, first in ((16, 512), (4, 128)):
        within = fields(rng, subject.shape, g, 64 * g)[1]
        for D in (ref.zero_field(subject.shape, g), within):
            for step in (1, first):
                want_d, info = check_sweep(s_dev, t_dev, subject, template, 5, TRUE_MAP, D, g, step, ref.default_limit_ref(TRUE_MAP, g))
                assert step == 1 or info[0] > 0                    # the warped case: a coarse step moves nodes
        # a limit of 0: a moved candidate differs from a neighbour by the step at least, nothing may move
        want_d, info = check_sweep(s_dev, t_dev, subject, template, 5, TRUE_MAP, ref.zero_field(subject.shape, g), g, first, 0)
        assert not want_d.any() and info[0] == 0 and info[1] > 0


# ---- fit ---------------------------------------------------------------------------------------------------------------------------------
def check_fit(subject, template, T, m, levels, want, impls=IMPLS, dt=torch.uint8):
    s_dev, t_dev = dev_int(subject, dt), dev_int(template, dt)
    for impl in impls:
        D, report = W.fit(s_dev, t_dev, T, m, levels=levels, impl=impl)
        assert same(host(D), want[0]), impl
        assert same(host(report), want[1]), (impl, host(report)[:10], want[1][:10])


def test_fit_the_warped_ellipsoid_case_with_the_defaults():
    subject, template = ref.warped_case()
    want = ref.warped_fit()
    check_fit(subject, template, 5, TRUE_MAP, W.DEFAULT_LEVELS, want)
    rows = want[1][want[1][:, 0] >= 0]
    assert len(rows) == 8 and (rows[:, 2] < 6).any() and rows[-1, 4] > rows[0, 4]        # some (level, step) ends early


def test_fit_a_one_level_list_one_sweep_and_a_schedule_whose_first_sweep_changes_nothing():
    subject, template = gr.small_pair()                             # (12, 10, 8) -> (10, 12, 9)
    moved = shift(1.5, -1, 0.5)
    for levels in ([(8, 256, 64, 3, 400)], [(4, 128, 128, 1, 200)], [(16, 512, 256, 2, 900), (8, 128, 128, 16, 400), (4, 64, 32, 2, 200)],
                   [(32, 1024, 1024, 1, BIG), (16, 16384, 8192, 1, BIG), (8, 1, 1, 2, 0), (4, 2, 1, 16, 3)]):
        want = ref.fit_ref(subject, template, 3, IDENTITY, levels)
        check_fit(subject, template, 3, IDENTITY, levels, want, dt=torch.uint16)
        assert want[0].any() or levels[0][0] == 32
    # at the map the subject was sampled through nothing can improve: every first sweep changes nothing and is the only one run
    levels = [(8, 256, 64, 6, 400), (4, 128, 64, 6, 200)]
    want = ref.fit_ref(subject, template, 3, moved, levels)
    rows = want[1][want[1][:, 0] >= 0]
    assert not want[0].any() and len(rows) == 5 and (rows[:, 2] == 1).all() and (rows[:, 3] == 0).all()
    check_fit(subject, template, 3, moved, levels, want)


def test_fit_two_threads_on_two_streams_with_their_own_scratch():
    subject, template = gr.small_pair()
    plans = ([(8, 256, 64, 3, 400), (4, 128, 64, 2, 200)], [(16, 512, 128, 2, 900), (8, 256, 256, 4, 400)])
    wants = [ref.fit_ref(subject, template, 3, IDENTITY, lv) for lv in plans]
    s_dev, t_dev = dev_int(subject, torch.uint8), dev_int(template, torch.uint8)
    torch.cuda.synchronize()
    results, errors = [None, None], []

    def work(k):
        try:
            stream = torch.cuda.Stream(device=DEV)
            with torch.cuda.stream(stream):
                scratch = torch.empty(W.scratch_bytes(subject.shape, 3, W.levels_of(plans[k], None, IDENTITY)), dtype=torch.uint8, device=DEV)
                out = []
                for _ in range(5):
                    impl = W.IMPL_NODE if k == 0 else W.IMPL_VOXEL
                    out.append(W.fit(s_dev, t_dev, 3, IDENTITY, levels=plans[k], impl=impl, scratch=scratch))
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


# ---- parcellate and the evaluation loop ---------------------------------------------------------------------------------------------------
SHORT = dict(init=TRUE_MAP, stages=[(2, 3, 4)], max_iterations=30)  # a search of a few iterations: the restatement stays quick
SHORT_PLAN = W.Plan(levels=[(8, 256, 128, 2), (4, 128, 128, 1)])


def test_parcellate_with_a_warp_plan_against_the_restatements_chained():
    subject, template = ref.warped_case()
    z, y, x = np.indices(template.shape)
    atlas = np.where(template > 0, 1 + (x > 14).astype(np.int64) + (x + y > 50) + 3 * (z > 20) + 6 * (template == 4), 0)   # cut by planes
    atlas[np.random.default_rng(9).random(template.shape) < 0.08] = 0
    m, _, info = search_ref(subject, template, 5, TRUE_MAP, stages=SHORT["stages"], max_iterations=SHORT["max_iterations"])
    levels = ref.levels_ref(m, SHORT_PLAN.levels)
    D, rows = ref.fit_ref(subject, template, 5, m, levels)
    carried, counts = ref.carry_ref(subject, template, atlas, 5, m, D, 4)
    exp, filled, _, ginfo = grow_ref(subject, carried, 5, [1, 2, 3, 4], A.CLAMP | A.PRESERVE, None, 1)
    affine = ref.score_ref(ref.hist_ref(subject, template, 5, m, ref.zero_field(subject.shape, 4), 4))
    s_dev, t_dev, a_dev = dev_int(subject, torch.uint8), dev_int(template, torch.uint8), dev_int(atlas, torch.uint16)
    for _ in range(2):
        got, rep = R.parcellate(s_dev, (1, 1, 1), t_dev, (1, 1, 1), a_dev, warp=SHORT_PLAN, **SHORT)
        assert got.dtype == torch.uint16 and tuple(got.shape) == subject.shape and same(host(got), exp)
        assert same(np.concatenate(rep["map"]), m) and rep["score"] == int(info[2])
        assert same(rep["direct"], counts[0]) and same(rep["rescued"], counts[1]) and same(rep["left"], counts[2])
        assert same(rep["filled"], filled) and (rep["rounds"], rep["grow_converged"]) == (int(ginfo[0]), bool(ginfo[1]))
        w = rep["warp"]
        assert w["levels"].tolist() == [list(lv) for lv in levels] and same(w["report"], rows[rows[:, 0] >= 0])
        assert w["score_affine"] == affine and w["score_warped"] == int(rows[2, 4]) > affine and w["max_disp_q8"] == int(np.abs(D).max()) > 0
    # the warp carries more voxels directly than the affine map alone
    plain, plain_rep = R.parcellate(s_dev, (1, 1, 1), t_dev, (1, 1, 1), a_dev, **SHORT)
    assert int(rep["direct"].sum()) > int(plain_rep["direct"].sum())
    # warp=None is the existing call, byte for byte
    none, none_rep = R.parcellate(s_dev, (1, 1, 1), t_dev, (1, 1, 1), a_dev, warp=None, **SHORT)
    assert same(host(none), host(plain)) and "warp" not in none_rep and "warp" not in plain_rep
    assert same(np.concatenate(none_rep["map"]), np.concatenate(plain_rep["map"])) and same(none_rep["direct"], plain_rep["direct"])
    assert not same(host(none), exp)


def test_evaluate_with_atlas_warp_equals_parcellate_with_warp_called_by_hand():
    import test_gpu_table as tt
    atlas, template = tt.make_atlas()
    m = tt.small_model()
    io = tt.inputs()["plain"][0]
    ev = U.EvaluateUNet(m, postproc="model", outputs=("label", "atlas", "regions"), atlas=atlas, atlas_options=tt.OPTIONS, atlas_warp=SHORT_PLAN)
    got = ev.start([[io]])[0][0]
    assert not ev.aborted and ev.error_msg == ""
    label = tt.dev_map(got["label"], torch.uint16)
    parc, report = R.parcellate(label, m.voxel_size, atlas.template, atlas.template_vs, atlas.regions, 5, warp=SHORT_PLAN, **tt.OPTIONS)
    assert same(np.ascontiguousarray(got["atlas"]), host(parc))
    rep = got["regions"]["report"]
    assert same(np.concatenate(rep["map"]), np.concatenate(report["map"])) and rep["score"] == report["score"]
    assert same(rep["warp"]["report"], report["warp"]["report"]) and len(rep["warp"]["report"]) == 3
    assert rep["warp"]["score_warped"] >= rep["warp"]["score_affine"] == report["warp"]["score_affine"]
    # without atlas_warp the loop is what it was
    old = U.EvaluateUNet(m, postproc="model", outputs=("atlas", "regions"), atlas=atlas, atlas_options=tt.OPTIONS).start([[io]])[0][0]
    base, _ = R.parcellate(label, m.voxel_size, atlas.template, atlas.template_vs, atlas.regions, 5, **tt.OPTIONS)
    assert same(np.ascontiguousarray(old["atlas"]), host(base)) and "warp" not in old["regions"]["report"]
