"""CPU: the host half of the starts of a registration (include/unet_start.h, unet-studio_amd/start.py) -- the ABI the library
exports, argument errors found before any device call, `start.candidates` and the restatements of tests/start_ref.py on hand-worked
answers, and the quality of the definition: the four cases on which a search from the centre start fails, measured on the numpy
restatement.  No device calls."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

import unet_studio_amd as U
from unet_studio_amd import register as R
from unet_studio_amd import start as ST

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import start_ref as ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDENTITY = [1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0]


# ---- the ABI -------------------------------------------------------------------------------------------------------------------------
def test_unet_start_h_declares_exactly_the_exports_and_the_library_exports_exactly_them():
    hdr = open(os.path.join(ROOT, "include", "unet_start.h")).read()
    body = hdr[hdr.index("#ifndef UNET_START_H"):]
    declared = set(re.findall(r"\b(unet_[a-z0-9_]+)\s*\(", body))
    assert declared == set(ST.EXPORTS) == {"unet_start_scratch_bytes", "unet_start_moments", "unet_start_pick", "unet_start_search"}
    assert len(ST.EXPORTS) == len(set(ST.EXPORTS))
    lib = ctypes.CDLL(U.engine.LIB_PATH)
    for name in sorted(declared):
        assert hasattr(lib, name), "libunet_hip.so does not export " + name
    # every name with the prefix that the library's file holds (its dynamic symbols, and its messages, which name them) is declared
    in_file = set(m.decode() for m in re.findall(rb"unet_start_[a-z0-9_]+", open(U.engine.LIB_PATH, "rb").read()))
    assert in_file == declared, in_file ^ declared
    enums = {k: int(v) for k, v in re.findall(r"UNET_START_([A-Z_]+) = (\d+)", hdr)}
    assert enums == {"IMPL_DEFAULT": ST.IMPL_DEFAULT, "IMPL_BATCHED": ST.IMPL_BATCHED, "IMPL_SEQUENTIAL": ST.IMPL_SEQUENTIAL}
    assert (ST.IMPL_DEFAULT, ST.IMPL_BATCHED, ST.IMPL_SEQUENTIAL) == (0, 1, 2)
    limits = {k: int(v) for k, v in re.findall(r"#define UNET_START_MAX_([A-Z]+) (\d+)", hdr)}
    assert limits == {"STATES": ST.MAX_STATES, "STARTS": ST.MAX_STARTS, "DIM": ST.MAX_DIM}
    assert ST.MAX_STATES == 4 and ST.MAX_STARTS == 5 * R.MAX_MAPS and ST.ALWAYS == ref.ALWAYS == 13
    assert U.start is ST and tuple(ST.Plan()) == (12.0, 4, 2)


def test_the_other_headers_do_not_mention_the_new_prefix_and_this_one_mentions_no_other():
    for h in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if h != "unet_start.h":
            assert "unet_start" not in open(os.path.join(ROOT, "include", h)).read().lower(), h
    mine = open(os.path.join(ROOT, "include", "unet_start.h")).read().lower()
    for p in ("reg", "coreg", "stats", "space", "atlas", "components", "preproc", "conn", "calib", "recal", "inst", "tiles", "dist", "mirror",
              "table", "ens", "morph"):                            # what the other host tests forbid
        assert "unet_%s_" % p not in mine, p
    assert "unet_coreg" not in mine


# ---- argument errors, before any device call -------------------------------------------------------------------------------------
P = [ctypes.c_void_p(0x1000 * (i + 1)) for i in range(10)]         # never dereferenced


def test_scratch_bytes_grows_with_t_and_n_and_checks_its_arguments():
    assert ST.start_scratch_bytes(5, 1) < ST.start_scratch_bytes(5, 4) < ST.start_scratch_bytes(16, 4)
    # n states, n tables of 25 candidates, n scratches of the register module's search
    assert ST.start_scratch_bytes(16, 4) >= 4 * (25 * 16 * 16 * 4 + R.reg_scratch_bytes(1, 16, 1))
    for t, n, msg in ((1, 1, "n_tissues"), (17, 1, "n_tissues"), (5, 0, "n must be"), (5, 5, "n must be")):
        with pytest.raises(U.UNetError, match=msg):
            ST.start_scratch_bytes(t, n)
    rc = U.engine.lib.unet_start_scratch_bytes(5, 1, None)
    assert rc != 0 and "null output" in U.engine.lib.unet_last_error().decode()


def test_moments_argument_errors_need_no_device():
    lib = U.engine.lib

    def call(volume=P[0], vbytes=1, dims=(4, 4, 4), lo=1, hi=4, sums=P[1]):
        rc = lib.unet_start_moments(volume, vbytes, *dims, lo, hi, sums, None)
        assert rc != 0
        return lib.unet_last_error().decode()

    assert "null volume" in call(volume=None) and "null sums" in call(sums=None)
    assert "vbytes must be 1 or 2, got 4" in call(vbytes=4)
    assert "dimensions must be positive" in call(dims=(0, 4, 4)) and "dimensions must be positive" in call(dims=(4, 4, -1))
    assert "dimensions must stay below 65536" in call(dims=(65536, 1, 1))
    assert "2^31 voxels" in call(dims=(2048, 1024, 1024))
    assert "lo must be in [0, 65535], got -1" in call(lo=-1) and "hi must be in [0, 65535], got 65536" in call(hi=65536)
    assert "sums must be 8-byte aligned" in call(sums=ctypes.c_void_p(0x3004))


def test_pick_argument_errors_need_no_device():
    lib = U.engine.lib

    def call(hist=P[0], S=27, T=5, maps=P[1], n=4, always=13, scores=P[2], inits=P[3], picked=P[4]):
        rc = lib.unet_start_pick(hist, S, T, maps, n, always, scores, inits, picked, None)
        assert rc != 0
        return lib.unet_last_error().decode()

    for name in ("hist", "maps", "scores", "inits", "picked"):
        assert "null " + name in call(**{name: None})
    assert "S must be in [1, 125], got 0" in call(S=0) and "S must be" in call(S=126)
    assert "n_tissues must be in [2, 16], got 17" in call(T=17)
    assert "n must be in [1, min(S, 4)], got 5" in call(n=5) and "n must be" in call(n=0) and "n must be" in call(S=3, n=4, always=0)
    assert "always must be -1 or in [0, S), got 27" in call(always=27) and "always" in call(always=-2)
    assert "hist must be 4-byte aligned" in call(hist=ctypes.c_void_p(0x3002))
    assert "scores must be 8-byte aligned" in call(scores=ctypes.c_void_p(0x3004))
    assert "picked must be 4-byte aligned" in call(picked=ctypes.c_void_p(0x3002))


def test_search_argument_errors_need_no_device():
    lib = U.engine.lib
    step = (ctypes.c_float * 12)(*R.DEFAULT_STEP)
    stages = (ctypes.c_int * 9)(4, 0, 2, 2, 1, 4, 1, 2, 6)

    def floats(v):
        return (ctypes.c_float * 12)(*v)

    def ints(v):
        return (ctypes.c_int * len(v))(*v)

    def call(subject=P[0], sbytes=1, s=(4, 4, 4), template=P[1], tbytes=2, t=(4, 4, 4), T=5, inits=P[2], n=4, step=step, stages=stages,
             n_stages=3, n_it=10, maps_out=P[3], trace=P[4], info=P[5], best=P[6], best_map=P[7], impl=0, scratch=P[8],
             scratch_bytes=1 << 40):
        rc = lib.unet_start_search(subject, sbytes, *s, template, tbytes, *t, T, inits, n, step, stages, n_stages, n_it, maps_out, trace, info,
                                   best, best_map, impl, scratch, scratch_bytes, None)
        assert rc != 0
        return lib.unet_last_error().decode()

    assert "null subject" in call(subject=None) and "null template" in call(template=None)
    assert "sbytes must be 1 or 2, got 4" in call(sbytes=4) and "tbytes must be 1 or 2, got 0" in call(tbytes=0)
    assert "subject dimensions" in call(s=(0, 4, 4)) and "template dimensions" in call(t=(4, 0, 4))
    assert "subject grid" in call(s=(2048, 1024, 1024)) and "template grid" in call(t=(2048, 1024, 1024))
    assert "n_tissues must be in [2, 16], got 1" in call(T=1)
    assert "null inits" in call(inits=None) and "inits must be 4-byte aligned" in call(inits=ctypes.c_void_p(0x3002))
    assert "n must be in [1, 4], got 0" in call(n=0) and "n must be in [1, 4], got 5" in call(n=5)
    assert "null step" in call(step=None) and "null stages" in call(stages=None)
    assert "step[3] must be finite and >= 0" in call(step=floats([1, 1, 1, -1] + [0] * 8))
    assert "at least one step" in call(step=floats([0] * 12))
    assert "n_stages must be in [1, 4], got 5" in call(n_stages=5)
    assert "stage 1: stride must be 1, 2, 4 or 8, got 3" in call(stages=ints([4, 0, 2, 3, 1, 4, 1, 2, 6]))
    assert "stage 2: levels" in call(stages=ints([4, 0, 2, 2, 1, 4, 1, 2, 21]))
    assert "max_iterations" in call(n_it=0) and "max_iterations" in call(n_it=1025)
    for name in ("maps_out", "info", "best", "best_map"):
        assert "null " + name in call(**{name: None})
    assert "trace must be 8-byte aligned" in call(trace=ctypes.c_void_p(0x4004)) and "info must be 8-byte aligned" in call(info=ctypes.c_void_p(0x5004))
    assert "best_map must be 4-byte aligned" in call(best_map=ctypes.c_void_p(0x5002))
    assert "unknown impl 3" in call(impl=3) and "unknown impl -1" in call(impl=-1)
    assert "null scratch" in call(scratch=None)
    assert "scratch too small" in call(scratch_bytes=ST.start_scratch_bytes(5, 4) - 1)
    assert "scratch too small" in call(scratch_bytes=ST.start_scratch_bytes(5, 1))


def test_wrapper_errors_need_no_device():
    t8, a16 = torch.zeros((2, 2, 2), dtype=torch.uint8), torch.zeros((2, 2, 2), dtype=torch.uint16)
    with pytest.raises(U.UNetError, match="start.moments: volume"):
        ST.moments(t8, 1, 4)
    with pytest.raises(U.UNetError, match="start.pick: hist"):
        ST.pick(torch.zeros((27, 5, 5), dtype=torch.int32), torch.zeros((27, 12)))
    with pytest.raises(U.UNetError, match="subject"):
        ST.search(t8, t8, 5, torch.zeros((4, 12)))
    with pytest.raises(U.UNetError, match="subject"):
        ST.find(t8, t8, 5)
    with pytest.raises(U.UNetError, match="start.rank: S"):
        ST.rank(t8, t8, 5, np.zeros((126, 12)))
    for bad, msg in ((ST.Plan(0.0, 4, 2), "degrees"), (ST.Plan(12.0, 5, 2), "starts.n"), (ST.Plan(12.0, 4, 3), "rank_stride"), ("x", "start.Plan")):
        with pytest.raises(U.UNetError, match=msg):
            ST._plan(bad, "register.parcellate")
    with pytest.raises(U.UNetError, match="degrees"):
        ST.candidates([1] * 10, [1] * 10, degrees=float("nan"))
    with pytest.raises(U.UNetError, match="10 sums"):
        ST.candidates([1] * 9, [1] * 10)
    with pytest.raises(U.UNetError, match="device tensor"):
        R.parcellate(t8, (1, 1, 1), t8, (1, 1, 1), a16, starts=ST.Plan())


# ---- moments_ref and candidates on hand-worked answers -----------------------------------------------------------------------------
def test_moments_ref_one_voxel_a_bar_and_the_range():
    v = np.zeros((4, 5, 6), np.uint8)                               # (D, H, W)
    v[3, 2, 5] = 1
    assert ref.moments_ref(v, 1, 4).tolist() == [1, 5, 2, 3, 25, 4, 9, 10, 15, 6] and ref.moments_ref(v, 1, 4).dtype == np.int64
    bar = np.zeros((1, 1, 2), np.uint8) + 3                         # the 2 x 1 x 1 bar: x = 0 and x = 1
    assert ref.moments_ref(bar, 1, 4).tolist() == [2, 1, 0, 0, 1, 0, 0, 0, 0, 0]
    assert ref.moments_ref(bar, 3, 3).tolist()[0] == 2 and ref.moments_ref(bar, 4, 4).tolist() == [0] * 10      # both edges count
    assert ref.moments_ref(bar, 2, 1).tolist() == [0] * 10          # an empty range
    v[0, 0, 0] = 9                                                  # above hi: background
    assert ref.moments_ref(v, 1, 4).tolist()[0] == 1 and ref.moments_ref(v, 1, 9).tolist()[0] == 2


def block_moments(x0, nx, y0, ny, z0, nz):
    v = np.zeros((z0 + nz + 1, y0 + ny + 1, x0 + nx + 1), np.uint8)
    v[z0:z0 + nz, y0:y0 + ny, x0:x0 + nx] = 1
    return ref.moments_ref(v, 1, 1)


def test_candidates_on_hand_worked_answers():
    # subject: a 2 x 2 x 2 block at (2, 4, 6): centroid (2.5, 4.5, 6.5), variance 1/4 per axis.  template: a 4 x 2 x 6 block at
    # (10, 0, 1): centroid (11.5, 0.5, 3.5), variances (5/4, 1/4, 35/12): sc = (sqrt 5, 1, sqrt(35/3))
    sm, tm = block_moments(2, 2, 4, 2, 6, 2), block_moments(10, 4, 0, 2, 1, 6)
    for maps in (ST.candidates(sm, tm), ref.candidates_ref(sm, tm)):
        assert maps.shape == (27, 12) and maps.dtype == np.float32
        sc = np.sqrt([5.0, 1.0, 35.0 / 3.0])
        want = np.concatenate([np.diag(sc).reshape(9), np.array([11.5, 0.5, 3.5]) - sc * np.array([2.5, 4.5, 6.5])])
        assert np.abs(maps[13].astype(np.float64) - want).max() < 1e-6
        for m in maps:                                              # every start puts the centroids on each other
            got = m[:9].astype(np.float64).reshape(3, 3) @ np.array([2.5, 4.5, 6.5]) + m[9:]
            assert np.abs(got - np.array([11.5, 0.5, 3.5])).max() < 1e-4
    assert ST.candidates(sm, tm).tobytes() == ref.candidates_ref(sm, tm).tobytes()
    # the order of the grid and the sense of a rotation: index 14 is (0, 0, +d) about axis 2, index 22 is (+d, 0, 0) about axis 0
    maps = ST.candidates(sm, sm, degrees=30.0)
    c, s = np.cos(np.pi / 6), 0.5
    assert np.abs(maps[14][:9] - np.array([c, -s, 0, s, c, 0, 0, 0, 1])).max() < 1e-6
    assert np.abs(maps[12][:9] - np.array([c, s, 0, -s, c, 0, 0, 0, 1])).max() < 1e-6
    assert np.abs(maps[22][:9] - np.array([1, 0, 0, 0, c, -s, 0, s, c])).max() < 1e-6
    assert np.abs(maps[16][:9] - np.array([c, 0, -s, 0, 1, 0, s, 0, c])).max() < 1e-6
    assert maps[13].tolist() == IDENTITY
    # one voxel: variance 0; the bar: variance 0 on two axes; an empty foreground: the fallback alone
    one = np.array([1, 5, 2, 3, 25, 4, 9, 10, 15, 6])
    bar = np.array([2, 1, 0, 0, 1, 0, 0, 0, 0, 0])
    for bad in (one, bar, np.zeros(10, np.int64)):
        for f in (ST.candidates, ref.candidates_ref):
            for args in ((bad, tm), (sm, bad)):
                got = f(*args, fallback=[2, 0, 0, 0, 2, 0, 0, 0, 2, 1, 2, 3])
                assert got.shape == (1, 12) and got.dtype == np.float32 and got[0].tolist() == [2, 0, 0, 0, 2, 0, 0, 0, 2, 1, 2, 3]
        with pytest.raises(U.UNetError, match="no fallback"):
            ST.candidates(bad, tm)


# ---- pick_ref and best_ref ------------------------------------------------------------------------------------------------------------
def test_pick_ref_ties_and_always():
    scores = [5, 9, 9, 1, 9, 7] + [0] * 21
    assert ref.pick_ref(scores, 4, -1) == [1, 2, 4, 5]              # equal scores: the lowest index first
    assert ref.pick_ref(scores, 2, -1) == [1, 2]                    # a tie across the n-th place
    assert ref.pick_ref(scores, 4, 13) == [1, 2, 4, 13]             # not among them: replaces the last
    assert ref.pick_ref(scores, 4, 2) == [1, 2, 4, 5]               # already among them
    assert ref.pick_ref(scores, 1, 13) == [13]
    assert ref.pick_ref([3] * 27, 4, 13) == [0, 1, 2, 13] and ref.pick_ref([3] * 27, 4, -1) == [0, 1, 2, 3]
    assert ref.pick_ref([-5, -2], 2, 0) == [1, 0]
    with pytest.raises(ValueError):
        ref.pick_ref([1, 2, 3], 4, 0)                               # n > S
    with pytest.raises(ValueError):
        ref.pick_ref(scores, 5, 0)
    with pytest.raises(ValueError):
        ref.pick_ref([1, 2, 3], 2, 3)


def test_best_ref_converged_then_stage_then_score():
    # info = (iterations, converged, score, stage)
    assert ref.best_ref([[400, 0, 9000, 2], [50, 1, 100, 2]]) == 1       # converged beats a higher score
    assert ref.best_ref([[400, 0, 9000, 1], [400, 0, 100, 2]]) == 1      # a later stage beats an earlier one
    assert ref.best_ref([[10, 1, 100, 2], [10, 1, 101, 2], [10, 1, 101, 2]]) == 1      # the score, then the lowest index
    assert ref.best_ref([[10, 1, 5, 2]]) == 0
    for infos in ([[400, 0, 9000, 2], [50, 1, 100, 2]], [[1, 1, 7, 0], [1, 1, 7, 0]], [[3, 0, -4, 1], [3, 0, -2, 1], [3, 1, -9, 0]]):
        assert ST.best_of(infos) == ref.best_ref(infos)


# ---- the quality of the definition ----------------------------------------------------------------------------------------------------------
# Dice at stride 1 after a full search, measured on the restatement (T = 5, default step and stages, 12 degrees, n = 4, rank
# stride 2): from the centre start, from the moments start alone (candidate 13), and the best final state of the four picked starts
MEASURED = {   # name: (centre, moments alone, four starts)
    "hard": (0.8829, 0.9840, 0.9840),
    "offcentre": (0.9585, 1.0000, 1.0000),
    "rot15": (0.8776, 0.8918, 0.9944),
    "rot20sc": (0.9055, 0.8812, 0.9928),
}


@pytest.mark.parametrize("name", ["hard", "offcentre", "rot15", "rot20sc"])
def test_four_ranked_starts_find_what_the_centre_start_misses(name):
    centre = ref.case_dice(name, ref.case_centre_search(name)[0])
    found = ref.case_find(name)
    dices = [ref.case_dice(name, r[0]) for r in found["runs"]]
    alone, best = dices[found["picked"].index(13)], dices[found["best"]]
    print("%s: centre %.4f, moments alone %.4f, four starts %.4f (picked %s, best state %d)" % (name, centre, alone, best, found["picked"],
                                                                                          found["best"]))
    assert all(abs(a - b) < 5e-5 for a, b in zip((centre, alone, best), MEASURED[name]))          # the table of DESIGN.md §33, as measured
    assert 13 in found["picked"] and len(found["picked"]) == 4 and found["candidates"].shape == (27, 12)
    assert centre < 0.96                                            # a case the old start fails
    assert best >= max(MEASURED[name][2] - 0.01, 0.97)
    assert found["runs"][found["best"]][2][1] == 1                  # the winner converged
