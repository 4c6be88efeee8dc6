"""CPU: the host half of the patch feed (include/unet_patches.h) -- the ABI the library exports for it, the draws and the
per-sample decisions against an independent restatement in Python integers (tests/patches_ref.py), the origin arithmetic checked
exhaustively on small axes, and the windows of the test set.  No device calls."""
import ctypes
import os
import re

import numpy as np
import pytest

import patches_ref as R
import unet_studio_amd as U
from unet_studio_amd import patches as P
from unet_studio_amd import tiles as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_unet_patches_h_declares_exactly_the_exports_and_the_library_has_them():
    lib = ctypes.CDLL(U.engine.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "unet_patches.h")).read()
    declared = set(re.findall(r"\b(unet_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(P.EXPORTS) == {"unet_patches_index_bytes", "unet_patches_index", "unet_patches_pick", "unet_patches_crop",
                                          "unet_patches_draws"}
    for name in sorted(declared):
        assert hasattr(lib, name), "libunet_hip.so does not export " + name
    assert U.WindowFeed is P.WindowFeed and U.patches is P
    assert (P.SEGMENT, P.MAX_CLASSES, P.MAX_PICKS) == tuple(
        int(re.search(r"#define %s (\d+)" % n, hdr).group(1)) for n in ("UNET_PATCHES_SEGMENT", "UNET_PATCHES_MAX_CLASSES", "UNET_PATCHES_MAX_PICKS"))
    assert ctypes.sizeof(P.UnetPatchPick) == 20


@pytest.mark.parametrize("seed", [0, 1, 2 ** 64 - 1])
@pytest.mark.parametrize("index", [0, 1, 2 ** 32, 2 ** 63])
def test_draws_equal_the_python_restatement(seed, index):
    got = P.draws(seed, index, 0, 40)
    assert got.dtype == np.uint32 and [int(v) for v in got] == [R.draw(seed, index, k) for k in range(40)]
    # a pure function of (seed, index, k): any sub-range is the same numbers
    assert [int(v) for v in P.draws(seed, index, 7, 5)] == [int(v) for v in got[7:12]]
    assert len(P.draws(seed, index, 3, 0)) == 0


def test_draws_look_uniform_and_differ_between_neighbours():
    # 4096 draws in 16 bins: each within 6 binomial standard deviations (sqrt(4096 * 15 / 256) = 15.5) of 256
    u = np.concatenate([P.draws(12345, i, 0, 8) for i in range(512)]).astype(np.uint64)
    assert np.abs(np.bincount((u >> np.uint64(28)).astype(np.int64), minlength=16) - 256).max() <= 93
    assert len({tuple(P.draws(s, i, 0, 2)) for s in range(8) for i in range(8)}) == 64


def test_size_queries_and_argument_errors_need_no_device():
    assert P.index_layout(1, 8) == (8, 1) and P.index_layout(1024, 8) == (8, 1) and P.index_layout(1025, 1) == (1, 2)
    assert P.index_layout(5, 0) == (2, 1)                                # continuous labels: two classes
    assert P.index_layout(2 ** 31 - 1, 256) == (256, 2 ** 21)
    with pytest.raises(U.UNetError, match="below 2\\^31 voxels"):
        P.index_layout(2 ** 31, 8)
    with pytest.raises(U.UNetError, match="classes must be in \\[0, 256\\]"):
        P.index_layout(10, 257)
    with pytest.raises(U.UNetError, match="voxels must be positive"):
        P.index_layout(0, 2)
    with pytest.raises(U.UNetError, match="must not be negative"):
        P.draws(0, -1, 0, 1)
    for bad in [(2, 1), (-1, 3), (1, 0), "x", (1,)]:
        with pytest.raises(U.UNetError, match="foreground"):
            P.decide(0, 0, [1], bad)
    lib = U.engine.lib
    assert lib.unet_patches_draws(0, 0, 0, 1, None) != 0 and b"null output" in lib.unet_last_error()
    # refused before any device call: a window larger than the canvas, too many picks, a null pointer
    pk = (P.UnetPatchPick * 1)()
    assert lib.unet_patches_pick(8, 8, 2, 4, 4, 4, 5, 4, 4, pk, 1, 8, None) != 0 and b"must fit the canvas" in lib.unet_last_error()
    assert lib.unet_patches_pick(8, 8, 2, 4, 4, 4, 4, 4, 4, pk, 33, 8, None) != 0 and b"n must be in [1, 32]" in lib.unet_last_error()
    assert lib.unet_patches_pick(8, 8, 2, 2048, 2048, 512, 4, 4, 4, pk, 1, 8, None) != 0 and b"2^31" in lib.unet_last_error()
    assert lib.unet_patches_crop(None, 1, None, 4, 4, 4, 4, 4, 4, 8, 8, None, None) != 0 and b"null device pointer" in lib.unet_last_error()
    assert lib.unet_patches_crop(8, 1, None, 4, 4, 4, 4, 4, 4, 8, 8, 8, None) != 0 and b"lab without a label" in lib.unet_last_error()
    assert lib.unet_patches_crop(8, 1, None, 4, 4, 4, 4, 4, 0, 8, 8, None, None) != 0 and b"must be positive" in lib.unet_last_error()
    assert lib.unet_patches_index(8, 2048, 2, 8, 4 * (2 + 2 * 2) - 1, None) != 0 and b"index too small" in lib.unet_last_error()


@pytest.mark.parametrize("seed,fg,frac", [(0, [1, 2, 5], (1, 3)), (7, [3], (1, 3)), (2 ** 40 + 3, [1, 2, 3, 4, 5, 6, 7], (2, 5)),
                                          (9, [2, 4], (0, 1)), (9, [2, 4], (1, 1))])
def test_decisions_equal_the_python_restatement(seed, fg, frac):
    seen = set()
    for i in list(range(300)) + [2 ** 32 + 1, 2 ** 62]:
        got = P.decide(seed, i, fg, frac)
        assert got == R.decide(seed, i, fg, *frac), i
        assert got[0] == -1 or got[0] in fg
        seen.add(got[0])
    if frac == (0, 1):
        assert seen == {-1}                      # never forced
    elif frac == (1, 1):
        assert seen == set(fg)                   # always forced, every class drawn
    else:
        assert seen == set(fg) | {-1}


def test_forced_share_is_one_third_and_no_foreground_class_means_uniform():
    # binomial(3000, 1/3): sd = sqrt(3000 * 2 / 9) = 25.8; 5 sd = 129
    forced = sum(P.decide(11, i, [1, 2])[0] >= 0 for i in range(3000))
    print("forced-foreground samples: %d of 3000" % forced)
    assert abs(forced - 1000) <= 129
    # the classes of the forced samples are spread evenly: binomial(forced, 1/2), 5 sd
    ones = sum(P.decide(11, i, [1, 2])[0] == 1 for i in range(3000))
    assert abs(ones - forced / 2) <= 5 * (forced / 4) ** 0.5
    # m = 0: always the uniform rule, whatever the fraction
    for frac in [(1, 3), (1, 1)]:
        assert all(P.decide(11, i, [], frac)[0] == -1 for i in range(300))


def test_origin_arithmetic_exhaustively_on_small_axes():
    for Tn in range(1, 10):
        for Cn in range(Tn, 3 * Tn + 1):
            # the class rule: every centre and every jitter j = (u * T) >> 32, reached by its smallest and its largest draw
            for j in range(Tn):
                lo, hi = R.u_for(j, Tn), R.u_for(j + 1, Tn) - 1
                assert (lo * Tn) >> 32 == j and (hi * Tn) >> 32 == j and 0 <= lo <= hi < 2 ** 32
                assert lo == 0 or ((lo - 1) * Tn) >> 32 == j - 1
                for c in range(Cn):
                    for u in (lo, hi):
                        o = R.origin_class(c, u, Tn, Cn)
                        assert 0 <= o <= Cn - Tn
                        assert o <= c < o + Tn                       # the chosen voxel is inside the window
                        if 0 <= c - j <= Cn - Tn:
                            assert c - o == j                        # and at the drawn position, unless the canvas' edge forbids it
            # the uniform rule: in range, monotone, and every origin reachable
            n = Cn - Tn + 1
            reached = set()
            for o in range(n):
                lo, hi = R.u_for(o, n), R.u_for(o + 1, n) - 1
                assert R.origin_uniform(lo, Tn, Cn) == o == R.origin_uniform(hi, Tn, Cn)
                reached.add(o)
            assert reached == set(range(n))
            assert R.origin_uniform(0, Tn, Cn) == 0 and R.origin_uniform(2 ** 32 - 1, Tn, Cn) == Cn - Tn


def test_reference_index_and_pick_agree_with_plain_numpy():
    # the restatement the GPU tests compare against, on a case small enough to check by eye
    lab = np.array([0, 1, 1.9, -0.5, -1, np.nan, 2, 3, 1e30, 1], np.float32)
    assert R.class_map(lab, 3).tolist() == [0, 1, 1, 0, -1, -1, 2, -1, -1, 1]
    assert R.class_map(lab, 0).tolist() == [0, 1, 1, 0, 0, 0, 1, 1, 1, 1]
    tot, pre = R.index_ref(lab, 3)
    assert tot.tolist() == [2, 3, 1] and pre.shape == (3, 1) and not pre.any()
    cm = R.class_map(lab, 3)
    # rank 2 of class 1 is voxel 9; a canvas of 10 x 1 x 1, a window of 4: jitter 0 puts it at the window's start, clamped to 6
    assert R.pick_ref(cm, (10, 1, 1), (4, 1, 1), (1, R.u_for(2, 3), 0, 0, 0)) == (6, 0, 0, 1)
    assert R.pick_ref(cm, (10, 1, 1), (4, 1, 1), (1, R.u_for(1, 3), 2 ** 32 - 1, 0, 0)) == (0, 0, 0, 1)     # voxel 2, jitter 3
    assert R.pick_ref(cm, (10, 1, 1), (4, 1, 1), (-1, 0, 2 ** 32 - 1, 0, 0)) == (6, 0, 0, 0)


@pytest.mark.parametrize("canvas,dim", [((40, 24, 16), (16, 16, 16)), ((16, 16, 48), (16, 16, 16)), ((16, 16, 16), (16, 16, 16)),
                                        ((37, 16, 50), (16, 16, 24))])
def test_test_set_windows_are_the_overlap_free_tile_plan(canvas, dim):
    wins = P.test_windows(canvas, dim)
    px, py, pz = T.plan_tiles(canvas, dim, overlap=0)
    assert wins == [(x, y, z) for z in pz for y in py for x in px]
    # they cover the canvas and stay inside it
    seen = np.zeros(canvas[::-1], bool)
    for x, y, z in wins:
        assert 0 <= x <= canvas[0] - dim[0] and 0 <= y <= canvas[1] - dim[1] and 0 <= z <= canvas[2] - dim[2]
        seen[z:z + dim[2], y:y + dim[1], x:x + dim[0]] = True
    assert seen.all()
    assert len(wins) == int(np.prod([-(-c // d) for c, d in zip(canvas, dim)]))      # no more windows than the sizes ask for
