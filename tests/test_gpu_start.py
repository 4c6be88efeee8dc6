"""GPU: the starts of a registration on the device (include/unet_start.h) -- moments against moments_ref, pick against pick_ref,
search (IMPL_BATCHED, IMPL_SEQUENTIAL and the default) against n separate runs of search_ref and of register.search, find and
parcellate(starts=...) against the restatements chained, coreg.align(starts=...) on a phantom the centre start fails.  The
restatements are those of tests/start_ref.py, tests/test_register_host.py, tests/test_atlas_host.py and tests/coreg_ref.py.  Every
comparison is exact equality of bytes.  Shapes are written (W, H, D) as in the header; the arrays are (D, H, W)."""
import os
import sys
import threading

import numpy as np
import pytest
import torch

import unet_studio_amd as U  # noqa: F401
from unet_studio_amd import atlas as A
from unet_studio_amd import coreg as CR
from unet_studio_amd import register as R
from unet_studio_amd import start as ST

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import start_ref as ref  # noqa: E402
from test_atlas_host import grow_ref  # noqa: E402
from test_register_host import DEFAULT_STAGES, DEFAULT_STEP, carry_ref, hist_ref, locate, nearest, search_ref, shift  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
IMPLS = (ST.IMPL_BATCHED, ST.IMPL_SEQUENTIAL, ST.IMPL_DEFAULT)
GUARD = 0x5AC3A5C35AC3A5C3


def dev_int(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a).astype(np.int32)).to(DEV).to(dtype)


def host(t):
    if t.dtype == torch.uint16:
        return t.view(torch.int16).cpu().numpy().view(np.uint16)
    if t.dtype == torch.uint32:
        return t.view(torch.int32).cpu().numpy().view(np.uint32)
    return t.cpu().numpy()


def same(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()


# ---- moments -------------------------------------------------------------------------------------------------------------------------
def raw_moments(ptr, nbytes, shape, lo, hi, poison):
    """unet_start_moments into ten words between poisoned guards -> the ten words; the guards are checked here"""
    G = 8
    out = torch.full((10 + 2 * G,), poison, dtype=torch.int64, device=DEV)
    d, h, w = shape
    U.engine.check(U.engine.lib.unet_start_moments(ptr, nbytes, w, h, d, lo, hi, out.data_ptr() + 8 * G, torch.cuda.current_stream().cuda_stream))
    got = out.cpu().numpy()
    assert (got[:G] == poison).all() and (got[G + 10:] == poison).all()
    return got[G:G + 10]


# (96, 64, 48) has more voxels than one round of the capped grid (1024 blocks of 256 threads) takes
@pytest.mark.parametrize("nbytes", [1, 2])
@pytest.mark.parametrize("sshape", [(1, 1, 1), (7, 5, 3), (65, 3, 2), (33, 9, 9), (40, 44, 38), (96, 64, 48)])
def test_moments_shapes_types_ranges_and_alignments(sshape, nbytes):
    w, h, d = sshape
    rng = np.random.default_rng(w * 10 + nbytes)
    top = 255 if nbytes == 1 else 65535
    vol = rng.integers(0, 8, (d, h, w))
    vol[rng.random(vol.shape) < 0.05] = top                          # the largest value the type holds
    if vol.size > 1:
        vol[rng.random(vol.shape) < 0.3] = 0
    np_dt = np.uint8 if nbytes == 1 else np.uint16
    raw = np.frombuffer(vol.astype(np_dt).tobytes(), np.uint8)
    assert w * h * d <= 1024 * 256 or sshape == (96, 64, 48)
    for off in (0, 1, 3):                                            # the volume's bytes at any address inside a byte buffer
        buf = torch.full((raw.size + 16,), 0xEE, dtype=torch.uint8, device=DEV)
        buf[off:off + raw.size] = torch.from_numpy(raw.copy()).to(DEV)
        for lo, hi in ((1, 4), (0, top), (top, top), (0, 0), (3, 3), (7, 65535), (5, 4)) if off == 0 else ((1, 4),):
            want = ref.moments_ref(vol, lo, hi)
            for poison in (GUARD, -1):                               # twice into garbage
                got = raw_moments(buf.data_ptr() + off, nbytes, vol.shape, lo, hi, poison)
                assert same(got, want), (off, lo, hi, got, want)
            if (lo, hi) == (0, top):
                assert want[0] == vol.size
            if lo > hi:
                assert not want.any()
    # the wrapper, into a tensor of the caller
    t = dev_int(vol, torch.uint8 if nbytes == 1 else torch.uint16)
    out = torch.full((10,), -7, dtype=torch.int64, device=DEV)
    got = ST.moments(t, 1, 4, out=out)
    assert got.data_ptr() == out.data_ptr() and same(host(got), ref.moments_ref(vol, 1, 4))


# ---- pick ----------------------------------------------------------------------------------------------------------------------------
def check_pick(hist_dev, maps, scores_want, ns=(1, 2, 3, 4), always=(13, -1, 0)):
    S = len(maps)
    maps_dev = torch.from_numpy(np.ascontiguousarray(maps)).to(DEV)
    for n in ns:
        for alw in always:
            if n > S or alw >= S:
                continue
            scores, inits, picked = ST.pick(hist_dev, maps_dev, n=n, always=alw)
            want = ref.pick_ref(scores_want, n, alw)
            assert same(host(scores), np.asarray(scores_want, np.int64)), (n, alw)
            assert host(picked).tolist() == want and host(picked).dtype == np.int32, (n, alw, host(picked), want)
            assert same(host(inits), np.ascontiguousarray(maps[want])), (n, alw)


def test_rank_and_pick_on_the_27_candidates_of_the_hard_case():
    subject, template = ref.case("hard")
    maps = ref.candidates_ref(ref.moments_ref(subject, 1, 4), ref.moments_ref(template, 1, 4))
    assert maps.shape == (27, 12)
    s_dev, t_dev = dev_int(subject, torch.uint8), dev_int(template, torch.uint8)
    hist = ST.rank(s_dev, t_dev, 5, maps, stride=2)                  # two passes of register.joint_hist: 25 maps, then 2
    want = hist_ref(subject, template, 5, maps, 2)
    assert same(host(hist), want)
    scores = ref.scores_ref(subject, template, 5, maps, 2)
    order = sorted(range(27), key=lambda k: (-int(scores[k]), k))
    assert order.index(13) == 2                                      # the unrotated start ranks third here and wins after the search
    check_pick(hist, maps, scores)
    assert ref.pick_ref(scores, 2, 13) == [order[0], 13] and ref.pick_ref(scores, 4, 13) == order[:4]


def table_of_scores(scores, T=3):
    """uint32 {S, T, T} whose register scores are `scores`: s >= 0 agrees on tissue 1 (and some background agreement, which counts
    nothing), s < 0 disagrees"""
    h = np.zeros((len(scores), T, T), np.uint32)
    for k, s in enumerate(scores):
        h[k, 0, 0] = 1000 + k
        if s >= 0:
            h[k, 1, 1] = s
        else:
            h[k, 2, 1] = -s
    return h


@pytest.mark.parametrize("scores", [[7] * 27, [5, 9, 9, 1, 9, 7] + [0] * 21, [3, 3, 8, 3, 3], [-4, -2, -9], [6], list(range(125)),
                                    [2 ** 31 + 5, 2 ** 31 + 5, 1]])
def test_pick_on_hand_made_tables(scores):
    S = len(scores)
    h = table_of_scores(scores)
    assert [ref.score_ref(t) for t in h] == scores
    maps = np.random.default_rng(S).normal(0, 1, (S, 12)).astype(np.float32)
    maps[0, 3] = np.nan                                              # copied as bits
    hist = torch.from_numpy(h.view(np.int32)).to(DEV).view(torch.uint32)
    check_pick(hist, maps, scores, always=(13, -1, 0, S - 1))


# ---- search --------------------------------------------------------------------------------------------------------------------------
def check_states(subject, template, T, inits, step=DEFAULT_STEP, stages=DEFAULT_STAGES, max_iterations=400, impls=IMPLS, want=None,
                 dt=torch.uint8, traces=(True, False)):
    """every implementation with and without traces against one search_ref per state; best against best_ref"""
    inits = np.ascontiguousarray(np.asarray(inits, np.float32).reshape(-1, 12))
    want = want or [search_ref(subject, template, T, i, step, stages, max_iterations) for i in inits]
    best = ref.best_ref([w[2] for w in want])
    s_dev, t_dev, i_dev = dev_int(subject, dt), dev_int(template, dt), torch.from_numpy(inits).to(DEV)
    for impl in impls:
        for with_trace in traces:
            maps, trace, info, b, best_map = ST.search(s_dev, t_dev, T, i_dev, step=step, stages=stages, max_iterations=max_iterations,
                                                       impl=impl, trace=with_trace)
            m_h, i_h = host(maps), host(info)
            for s, w in enumerate(want):
                assert same(m_h[s], w[0]), (impl, s, m_h[s], w[0])
                assert same(i_h[s], w[2]), (impl, s, i_h[s], w[2])
                if with_trace:
                    assert same(host(trace)[s], w[1]), (impl, s)
            assert trace is None or with_trace
            assert host(b).tolist() == [best] and host(b).dtype == np.int32, (impl, host(b), best)
            assert same(host(best_map), want[best][0]), impl
            assert same(host(i_dev), inits)                          # read only
    return want


def sampled(template, sshape, m):
    """the template seen through the map m on a (D, H, W) = sshape grid: the nearest sample, 0 outside"""
    z, y, x = (v.reshape(-1) for v in np.indices(sshape))
    inside, ix, iy, iz = nearest(locate(m, x, y, z), template.shape)
    return np.where(inside, template[np.where(inside, iz, 0), np.where(inside, iy, 0), np.where(inside, ix, 0)], 0).reshape(sshape)


def small_pair(moved=shift(1.5, -1, 0.5)):
    """template (10, 12, 9) [W, H, D]: two nested ellipsoids; subject (12, 10, 8): the template sampled through `moved`"""
    z, y, x = np.indices((9, 12, 10))
    d = ((x - 4.5) / 4.2) ** 2 + ((y - 5.5) / 5.2) ** 2 + ((z - 4) / 3.6) ** 2
    template = np.where(d < 0.35, 2, np.where(d < 1, 1, 0))
    return sampled(template, (8, 10, 12), moved), template


def small_inits():
    subject, template = small_pair()
    m, t = R.centre_init(subject.shape, (1, 1, 1), template.shape, (1, 1, 1))
    centre = list(m) + list(t)
    return [centre, shift(3, 2, -1), [0.9, 0.1, 0, -0.1, 1.1, 0, 0, 0.05, 1, 0.5, -2, 1], shift(-4, 0, 3)]


def test_search_the_four_picked_starts_of_rot15_are_at_different_strides_in_flight():
    """What pins k_start_hist's reuse of one LDS table: the four states leave the stride-4 and stride-2 stages at different
    iterations, so a block counts one state at stride 1 right after another at stride 4; counters left behind by one state would
    change the next state's scores, its trace and its map."""
    subject, template = ref.case("rot15")
    found = ref.case_find("rot15")
    runs = found["runs"]
    its = [int(r[2][0]) for r in runs]
    assert found["picked"] == [5, 8, 4, 13] and len(set(its)) == 4
    mixed = [it for it in range(min(its)) if len({int(r[1][it][0]) for r in runs}) > 1]
    assert len(mixed) > 10                                           # iterations with states at different stages, hence strides
    check_states(subject, template, 5, found["candidates"][found["picked"]], want=runs)
    assert found["best"] == 0 and ref.case_dice("rot15", runs[0][0]) > 0.99


@pytest.mark.parametrize("n", [1, 2, 4])
def test_search_the_small_pair_with_1_2_and_4_states(n):
    subject, template = small_pair()
    inits = small_inits()[:n]
    want = check_states(subject, template, 3, inits, dt=torch.uint16 if n == 2 else torch.uint8)
    assert all(w[2][1] == 1 for w in want)
    if n == 1:                                                       # one state is the single search of the register module
        s_dev, t_dev = dev_int(subject, torch.uint8), dev_int(template, torch.uint8)
        m1, tr1, i1 = R.search(s_dev, t_dev, 3, inits[0])
        for impl in IMPLS:
            maps, trace, info, best, best_map = ST.search(s_dev, t_dev, 3, torch.tensor(inits, dtype=torch.float32, device=DEV), impl=impl)
            assert same(host(maps)[0], host(m1)) and same(host(trace)[0], host(tr1)) and same(host(info)[0], host(i1))
            assert host(best).tolist() == [0] and same(host(best_map), host(m1))


def test_search_identical_inits_a_nan_beside_a_good_one_and_budgets_of_3_and_1():
    subject, template = small_pair()
    inits = small_inits()
    want = check_states(subject, template, 3, [inits[0]] * 4, impls=(ST.IMPL_BATCHED, ST.IMPL_SEQUENTIAL))
    assert all(same(w[0], want[0][0]) for w in want) and ref.best_ref([w[2] for w in want]) == 0      # equal keys: the lowest index
    nan = list(inits[0])
    nan[4] = float("nan")
    want = check_states(subject, template, 3, [nan, inits[0], nan], impls=(ST.IMPL_BATCHED, ST.IMPL_SEQUENTIAL))
    assert np.isnan(want[0][0][4]) and not np.isnan(want[1][0]).any() and ref.best_ref([w[2] for w in want]) == 1
    for budget in (3, 1):                                            # unconverged states: the key falls back on stage and score
        want = check_states(subject, template, 3, inits, max_iterations=budget)
        assert all(w[2].tolist()[:2] == [budget, 0] for w in want)
    # a budget that cuts some states short and lets others finish: a converged state beats an unconverged one
    done = [int(w[2][0]) for w in check_states(subject, template, 3, inits, impls=())]
    cut = sorted(done)[1]
    want = check_states(subject, template, 3, inits, max_iterations=cut, impls=(ST.IMPL_BATCHED, ST.IMPL_SEQUENTIAL), traces=(True,))
    assert 0 < sum(int(w[2][1]) for w in want) < 4


def test_search_a_one_stage_list_and_a_four_stage_list_with_frozen_parameters():
    subject, template = small_pair()
    inits = small_inits()
    want = check_states(subject, template, 3, inits, stages=[(1, 0, 3)])
    assert all(w[2][1] == 1 and w[2][3] == 0 for w in want)
    check_states(subject, template, 3, inits[:3], step=[0.25, 0, 0, 0, 0, 0, 0, 0, 0.5, 0, 2, 0],
                 stages=[(8, 0, 0), (2, 0, 5), (1, 3, 20), (4, 20, 20)], max_iterations=60)
    check_states(subject, template, 3, inits, step=[0] * 9 + [4, 4, 4], impls=(ST.IMPL_BATCHED,))


def test_search_two_threads_on_two_streams_with_their_own_misaligned_scratch():
    cases, errors = [], []
    for k, moved in enumerate((shift(1.5, -1, 0.5), shift(-0.5, 1, 0))):
        subject, template = small_pair(moved)
        inits = np.asarray(small_inits()[k:k + 3], np.float32)
        want = [search_ref(subject, template, 3, i) for i in inits]
        cases.append((dev_int(subject, torch.uint8), dev_int(template, torch.uint8), torch.from_numpy(inits).to(DEV), want))
    assert not same(cases[0][3][0][0], cases[1][3][0][0])
    torch.cuda.synchronize()

    def work(k):
        try:
            s_dev, t_dev, i_dev, want = cases[k]
            stream = torch.cuda.Stream(device=DEV)
            with torch.cuda.stream(stream):
                scratch = torch.empty(ST.start_scratch_bytes(3, 3) + 8, dtype=torch.uint8, device=DEV)[1 + 2 * k:]
                assert scratch.data_ptr() % 4 in (1, 3)
                for rep in range(3):
                    impl = (ST.IMPL_BATCHED, ST.IMPL_SEQUENTIAL, ST.IMPL_BATCHED)[rep]
                    maps, trace, info, best, best_map = ST.search(s_dev, t_dev, 3, i_dev, impl=impl, scratch=scratch[:ST.start_scratch_bytes(3, 3)],
                                                                  stream=stream.cuda_stream)
                    stream.synchronize()
                    for s, w in enumerate(want):
                        assert same(host(maps)[s], w[0]) and same(host(trace)[s], w[1]) and same(host(info)[s], w[2])
                    assert host(best).tolist() == [ref.best_ref([w[2] for w in want])]
        except BaseException as e:  # noqa: BLE001
            errors.append((k, repr(e)))

    threads = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors


# ---- find and parcellate ---------------------------------------------------------------------------------------------------------------
def rot15_atlas(template):
    z, y, x = np.indices(template.shape)
    atlas = np.where(template > 0, 1 + (x > 14).astype(np.int64) + (x + y > 50) + 3 * (z > 20) + 6 * (template == 4), 0)   # cut by planes
    rng = np.random.default_rng(9)
    atlas[rng.random(template.shape) < 0.08] = 0                    # holes
    atlas[:, 18:26, :] = 0                                          # a slab the cube does not bridge: left for the growth
    return atlas


def test_find_and_parcellate_with_starts_against_the_restatements_chained():
    subject, template = ref.case("rot15")
    found = ref.case_find("rot15")
    runs, best = found["runs"], found["best"]
    s_dev, t_dev = dev_int(subject, torch.uint8), dev_int(template, torch.uint8)
    for kw in ({}, dict(template_moments=ref.moments_ref(template, 1, 4)), dict(subject_moments=ST.moments(s_dev, 1, 4), impl=ST.IMPL_SEQUENTIAL)):
        best_map, pending = ST.find(s_dev, t_dev, 5, **kw)
        rep = ST.report(pending)
        assert best_map.is_cuda and same(host(best_map), runs[best][0])
        assert same(rep["candidates"], found["candidates"]) and not rep["degenerate"]
        assert same(rep["subject_moments"], ref.moments_ref(subject, 1, 4)) and same(rep["template_moments"], ref.moments_ref(template, 1, 4))
        assert same(rep["scores"], found["scores"]) and rep["picked"].tolist() == found["picked"] and rep["best"] == best
        for s, w in enumerate(runs):
            assert same(rep["maps"][s], w[0]) and same(rep["info"][s], w[2])
    # a foreground without extent: the fallback alone, one search, what register.search gives from it
    flat = np.zeros(subject.shape, np.uint8)
    flat[5, 6, :] = 1
    f_dev = dev_int(flat, torch.uint8)
    centre = ref.centre_map(flat.shape, template.shape)
    best_map, pending = ST.find(f_dev, t_dev, 5, max_iterations=5)
    rep = ST.report(pending)
    assert rep["degenerate"] and rep["picked"].tolist() == [0] and rep["best"] == 0 and rep["candidates"].tolist() == [centre]
    assert same(host(best_map), host(R.search(f_dev, t_dev, 5, centre, max_iterations=5)[0]))
    # parcellate: the best map carried, then grown
    atlas = rot15_atlas(template)
    a_dev = dev_int(atlas, torch.uint16)
    carried, counts = carry_ref(subject, template, atlas, 5, runs[best][0])
    exp, filled, _, ginfo = grow_ref(subject, carried, 5, [1, 2, 3, 4], A.CLAMP | A.PRESERVE, None, 1)
    assert (exp[subject > 0] != 0).mean() > 0.99
    atl = R.Atlas(t_dev, (1, 1, 1), a_dev, n_regions=int(atlas.max()))
    assert same(atl.moments(), ref.moments_ref(template, 1, 4)) and atl.moments() is atl.moments()
    for kw in ({}, dict(template_moments=atl.moments())):
        got, rep = R.parcellate(s_dev, (1, 1, 1), t_dev, (1, 1, 1), a_dev, starts=ST.Plan(), **kw)
        assert got.dtype == torch.uint16 and tuple(got.shape) == subject.shape and same(host(got), exp)
        assert same(np.concatenate(rep["map"]), runs[best][0])
        info = runs[best][2]
        assert (rep["iterations"], rep["converged"], rep["score"]) == (int(info[0]), bool(info[1]), int(info[2]))
        assert same(rep["direct"], counts[0]) and same(rep["rescued"], counts[1]) and same(rep["left"], counts[2])
        assert same(rep["filled"], filled) and (rep["rounds"], rep["grow_converged"]) == (int(ginfo[0]), bool(ginfo[1]))
        assert rep["starts"]["picked"].tolist() == found["picked"] and rep["starts"]["best"] == best
    # starts=None is the existing call, byte for byte: the search from centre_init, which stalls on this case
    base, base_rep = R.parcellate(s_dev, (1, 1, 1), t_dev, (1, 1, 1), a_dev)
    none, none_rep = R.parcellate(s_dev, (1, 1, 1), t_dev, (1, 1, 1), a_dev, starts=None)
    old = ref.case_centre_search("rot15")
    assert same(host(none), host(base)) and same(np.concatenate(none_rep["map"]), np.concatenate(base_rep["map"]))
    assert same(np.concatenate(none_rep["map"]), old[0]) and "starts" not in none_rep and none_rep["score"] == int(old[2][2])
    assert not same(host(none), exp)


def test_evaluate_with_atlas_starts_equals_parcellate_with_starts_called_by_hand():
    import test_gpu_table as tt
    atlas, template = tt.make_atlas()
    m = tt.small_model()
    io = tt.inputs()["plain"][0]
    ev = U.EvaluateUNet(m, postproc="model", outputs=("label", "atlas", "regions"), atlas=atlas, atlas_options=tt.OPTIONS,
                        atlas_starts=ST.Plan(12.0, 3, 2))
    got = ev.start([[io]])[0][0]
    assert not ev.aborted and ev.error_msg == ""
    label = tt.dev_map(got["label"], torch.uint16)
    parc, report = R.parcellate(label, m.voxel_size, atlas.template, atlas.template_vs, atlas.regions, 5, starts=ST.Plan(12.0, 3, 2),
                                **tt.OPTIONS)
    assert same(np.ascontiguousarray(got["atlas"]), host(parc))
    rep = got["regions"]["report"]
    assert same(np.concatenate(rep["map"]), np.concatenate(report["map"])) and rep["score"] == report["score"]
    assert same(rep["starts"]["scores"], report["starts"]["scores"]) and same(rep["starts"]["picked"], report["starts"]["picked"])
    assert len(rep["starts"]["picked"]) == (1 if rep["starts"]["degenerate"] else 3)
    assert same(rep["starts"]["template_moments"], atlas.moments())
    # without atlas_starts the loop is what it was
    old = U.EvaluateUNet(m, postproc="model", outputs=("atlas", "regions"), atlas=atlas, atlas_options=tt.OPTIONS).start([[io]])[0][0]
    base, base_rep = R.parcellate(label, m.voxel_size, atlas.template, atlas.template_vs, atlas.regions, 5, **tt.OPTIONS)
    assert same(np.ascontiguousarray(old["atlas"]), host(base)) and "starts" not in old["regions"]["report"]


# ---- coreg.align -----------------------------------------------------------------------------------------------------------------------
def test_align_with_starts_on_the_phantom_turned_by_20_degrees():
    """tests/coreg_ref.py's 32^3 phantom with its moving image turned by a further 20 degrees about z.  Measured on the restatement
    (quantile ranges, 16 bins): turned by 15 degrees the search from centre_init still arrives (corner error 0.528 voxel), so the
    case is 20 degrees, where it ends 8.799 voxels off and the best of four ranked starts 0.305.  On the device, whose ranges are
    robust_range's: 0.591 with starts, 8.799 without."""
    fixed, moving = ref.turned_phantom(20.0)
    truth = ref.turned_true_map(32, 20.0)
    f_dev, m_dev = torch.from_numpy(fixed.copy()).to(DEV), torch.from_numpy(moving.copy()).to(DEV)
    map_dev, info, moved = CR.align(m_dev, (1, 1, 1), f_dev, (1, 1, 1), starts=ST.Plan())
    m, info_h = host(map_dev), host(info)
    err = ref.cref.corner_error(m, truth, (32, 32, 32))
    old_map, old_info, _ = CR.align(m_dev, (1, 1, 1), f_dev, (1, 1, 1))
    old_err = ref.cref.corner_error(host(old_map), truth, (32, 32, 32))
    print("align on the turned phantom: corner error %.3f voxel with starts (%d iterations), %.3f from centre_init" % (err, info_h[0], old_err))
    assert info_h[1] == 1 and tuple(moved.shape) == (32, 32, 32)
    assert err <= 1.0
    assert old_err > 1.0
    # the steps in their order with two starts: the device's ranges, then the restatement's codes, moments, rank, pick and searches
    ranges = [CR.robust_range(f_dev), CR.robust_range(m_dev)]
    fc, mc = ref.cref.code_ref(fixed, *ranges[0], 16), ref.cref.code_ref(moving, *ranges[1], 16)
    want = ref.coreg_find_ref(fc, mc, 16, n=2)
    map_dev, info, _ = CR.align(m_dev, (1, 1, 1), f_dev, (1, 1, 1), starts=ST.Plan(12.0, 2, 2))
    assert 13 in want["picked"] and same(host(map_dev), want["runs"][want["best"]][0]) and same(host(info), want["runs"][want["best"]][2])
