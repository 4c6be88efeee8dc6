"""CPU: the host half of test-time mirroring (include/unet_mirror.h, unet-studio_amd/mirror.py) -- the ABI the library exports, the
members of an axes string, the swap's rules, argument errors found before any device call, and the numpy restatement the GPU tests
compare the kernels with, checked here against an independent restatement in explicit loops and on the involution property.  No
device calls.  Shapes are (D, H, W)."""
import ctypes
import os
import re

import numpy as np
import pytest

import unet_studio_amd as U
from unet_studio_amd import mirror as MR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
FORBIDDEN = ("unet_inst_", "unet_dist_", "unet_table_", "unet_reg_", "unet_atlas_", "unet_components_", "unet_preproc_", "unet_tiles_",
             "unet_space_", "unet_postproc_", "unet_qc_", "unet_feed_", "unet_morph_", "unet_conn_")


# ---- the ABI -------------------------------------------------------------------------------------------------------------------------
def test_unet_mirror_h_declares_exactly_the_exports_and_the_library_has_them():
    lib = ctypes.CDLL(U.engine.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "unet_mirror.h")).read()
    declared = set(re.findall(r"\b(unet_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(MR.EXPORTS) == {"unet_mirror_combine", "unet_mirror_postproc"}
    for name in sorted(declared):
        assert hasattr(lib, name), "libunet_hip.so does not export " + name
    defines = {k: int(v) for k, v in re.findall(r"#define UNET_MIRROR_([A-Z_]+) (\d+)", hdr)}
    assert defines == {"MAX_PAIRS": MR.MAX_PAIRS, "MAX_MEMBERS": MR.MAX_MEMBERS} and MR.MAX_PAIRS == 64 and MR.MAX_MEMBERS == 8
    assert "this project's" in hdr and "NOT pinned" in hdr
    assert U.mirror is MR


def test_the_new_prefix_stays_in_its_header():
    for h in sorted(os.listdir(os.path.join(ROOT, "include"))):
        text = open(os.path.join(ROOT, "include", h)).read().lower()
        if h != "unet_mirror.h":
            assert "unet_mirror_" not in text, h
        else:                                                      # what the other host tests forbid
            for other in FORBIDDEN:
                assert other not in text, other


# ---- the members ---------------------------------------------------------------------------------------------------------------------
def test_parse_axes():
    assert MR.parse_axes("") == [0] and MR.parse_axes(None) == [0]
    assert MR.parse_axes("x") == [0, 1] and MR.parse_axes("y") == [0, 2] and MR.parse_axes("z") == [0, 4]
    assert MR.parse_axes("zx") == [0, 1, 4, 5] == MR.parse_axes("xz")
    assert MR.parse_axes("xyz") == list(range(8)) == MR.parse_axes("zyx")
    assert MR.parse_axes("yz") == [0, 2, 4, 6]
    for bad, word in (("xx", "repeated"), ("xa", "unknown axis"), ("X", "unknown axis"), ("x,y", "unknown axis")):
        with pytest.raises(U.UNetError, match=word):
            MR.parse_axes(bad)
    with pytest.raises(U.UNetError, match="mirror_axes"):
        MR.parse_axes(3)
    assert MR.stack_bytes(MR.parse_axes("xyz"), 6, 128 ** 3) == 8 * 6 * 128 ** 3 * 4 == 402653184


def test_check_swap():
    ms = MR.parse_axes("xz")
    assert MR.check_swap("x", [(1, 2)], 3, ms) == (0, [(1, 2)])
    assert MR.check_swap(2, [(0, 1), (2, 5)], 6, ms) == (2, [(0, 1), (2, 5)])
    assert MR.check_swap(None, None, 3, ms) == (-1, []) == MR.check_swap(-1, [], 3, ms)
    assert MR.check_swap("z", [], 3, ms) == (2, [])
    assert MR.check_swap("x", [(2 * i, 2 * i + 1) for i in range(64)], 128, ms)[0] == 0
    for axis, pairs, c, word in (("x", [(1, 2), (2, 3)], 6, "more than one pair"),        # overlapping pairs
                                 ("x", [(1, 2), (1, 3)], 6, "more than one pair"),
                                 ("x", [(1, 1)], 3, "two different classes"),             # a == b
                                 ("x", [(1, 3)], 3, r"class 3 is not in \[0, 3\)"),       # a class >= C
                                 ("x", [(-1, 2)], 3, "class -1 is not in"),
                                 ("y", [(1, 2)], 3, "axis y is not among the mirrored axes"),
                                 ("y", [], 3, "axis y is not among the mirrored axes"),
                                 (None, [(1, 2)], 3, "without a swap axis"),              # pairs without an axis
                                 (-1, [(1, 2)], 3, "without a swap axis"),
                                 ("w", [(1, 2)], 3, "the axis must be"),
                                 (3, [(1, 2)], 3, "the axis must be"),
                                 ("x", [(2 * i, 2 * i + 1) for i in range(65)], 200, "at most 64 pairs"),
                                 ("x", [1, 2], 3, "pairs must be a list")):
        with pytest.raises(U.UNetError, match=word):
            MR.check_swap(axis, pairs, c, ms)
    with pytest.raises(U.UNetError, match="axis x is not among"):
        MR.check_swap("x", [(1, 2)], 3, [0])
    for bad in ([1, 2], [0, 0], [0, 2, 1, 3], [0, 1, 2], [0, 8], []):
        with pytest.raises(U.UNetError, match="masks"):
            MR.check_swap(None, None, 3, bad)


# ---- argument errors, before any device call -------------------------------------------------------------------------------------
P = [ctypes.c_void_p(0x1000 * (i + 1)) for i in range(6)]          # never dereferenced


def ints(*v):
    return (ctypes.c_int * len(v))(*v)


def failing(f, *args):
    assert f(*args) != 0
    return U.engine.lib.unet_last_error().decode()


def combine_args(stack=P[0], c=3, dims=(8, 6, 5), masks=(0, 1), n=None, axis=-1, pairs=None, mean=P[1], agr=P[2]):
    return (stack, c, dims[0], dims[1], dims[2], len(masks) if n is None else n, ints(*masks) if masks is not None else None, axis,
            ints(*pairs) if pairs else None, len(pairs) // 2 if pairs else 0, mean, agr, None)


def postproc_args(**kw):
    a = combine_args(**kw)
    return a[:10] + (0.5, P[3], P[4], P[5], a[11], None)


BAD = [(dict(stack=None), "null stack"),
       (dict(n=3, masks=(0, 1, 2)), "n_members must be 1, 2, 4 or 8, got 3"),
       (dict(n=0), "n_members must be 1, 2, 4 or 8, got 0"),
       (dict(n=16, masks=tuple(range(16))), "n_members must be 1, 2, 4 or 8, got 16"),
       (dict(masks=(1, 2)), "masks must start at 0"),
       (dict(masks=(0, 2, 1, 3)), "masks must strictly ascend"),
       (dict(masks=(0, 0)), "masks must strictly ascend"),
       (dict(masks=(0, 8)), "a mask must be in [0, 7], got 8"),
       (dict(masks=None, n=2), "null masks"),
       (dict(c=1), "out_c must be at least 2"),
       (dict(c=65537), "65535 foreground classes"),
       (dict(dims=(0, 6, 5)), "dimensions (w, h, d) must be positive"),
       (dict(dims=(8, -1, 5)), "dimensions"),
       (dict(dims=(2048, 1024, 1024)), "below 2^31 voxels"),
       (dict(axis=3), "swap_axis must be -1 (none), 0, 1 or 2, got 3"),
       (dict(axis=1), "swap_axis y is not mirrored by any member"),
       (dict(axis=-1, pairs=(1, 2)), "pairs given without a swap_axis"),
       (dict(axis=0, pairs=(1, 1)), "appears twice"),
       (dict(axis=0, pairs=(0, 1, 1, 2)), "appears twice"),
       (dict(axis=0, pairs=(1, 3)), "class 3 is not in [0, out_c)"),
       (dict(axis=0, pairs=tuple(range(130)), c=200), "n_pairs must be in [0, 64], got 65")]


@pytest.mark.parametrize("kw,msg", BAD)
def test_abi_argument_errors_come_before_any_device_call(kw, msg):
    lib = U.engine.lib
    assert msg in failing(lib.unet_mirror_combine, *combine_args(**kw)), kw
    m = failing(lib.unet_mirror_postproc, *postproc_args(**kw))
    assert msg in m and m.startswith("unet_mirror_postproc: "), kw


def test_abi_wants_an_output_and_pairs_when_it_is_told_of_some():
    lib = U.engine.lib
    assert "no output wanted" in failing(lib.unet_mirror_combine, *combine_args(mean=None, agr=None))
    a = postproc_args(agr=None)
    assert "no output wanted" in failing(lib.unet_mirror_postproc, *(a[:11] + (None, None, None, None, None)))
    a = list(combine_args(axis=0))
    a[9] = 1                                                       # n_pairs 1 with a NULL pairs pointer
    assert "null pairs" in failing(lib.unet_mirror_combine, *a)


def test_python_calls_name_the_bad_argument_before_any_device_work():
    with pytest.raises(U.UNetError, match="contiguous float32 device tensor"):
        MR.combine(np.zeros((2, 3, 2, 2, 2), F), [0, 1])
    with pytest.raises(U.UNetError, match="masks"):
        MR.combine(None, [0, 3, 1, 2])
    with pytest.raises(U.UNetError, match="unknown output"):
        MR.postproc_mirror(None, [0, 1], outputs=("mask",))
    with pytest.raises(U.UNetError, match="no output wanted"):
        MR.postproc_mirror(None, [0, 1], outputs=())
    with pytest.raises(U.UNetError, match="agreement needs mirror"):
        U.run_postproc(None, "softmax+argmax", outputs=("label", "agreement"))
    with pytest.raises(U.UNetError, match=r"in \[0, 7\]"):
        MR.flip_input(None, 8)


# ---- the restatement -----------------------------------------------------------------------------------------------------------------
def loops_reference(stack, masks, axis, pairs):
    """COMBINE and AGREEMENT of include/unet_mirror.h voxel by voxel, with np.flip and Python loops only"""
    K, C, D, H, W = stack.shape
    sigma = list(range(C))
    for a, b in pairs:
        sigma[a], sigma[b] = b, a
    back = []
    for k, m in enumerate(masks):
        v = stack[k]
        for bit, ax in ((0, 3), (1, 2), (2, 1)):
            if m >> bit & 1:
                v = np.flip(v, axis=ax)
        if axis >= 0 and m >> axis & 1:
            v = np.stack([v[sigma[c]] for c in range(C)])
        back.append(v)
    mean = np.zeros((C, D, H, W), F)
    agr = np.zeros((D, H, W), np.uint8)

    def amax(x):
        best = 0
        for c in range(1, C):
            if x[c] > x[best]:
                best = c
        return best

    with np.errstate(invalid="ignore", over="ignore"):
        for z in range(D):
            for y in range(H):
                for x in range(W):
                    for c in range(C):
                        s = F(back[0][c, z, y, x])
                        for k in range(1, K):
                            s = F(s + back[k][c, z, y, x])
                        mean[c, z, y, x] = s if K == 1 else F(s * F(1.0 / K))
                    top = amax(mean[:, z, y, x])
                    agr[z, y, x] = sum(amax(b[:, z, y, x]) == top for b in back)
    return mean, agr


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("axes,swap", [("", None), ("x", ("x", [(1, 2)])), ("yz", ("z", [(0, 2)])), ("xyz", ("y", [(1, 2)])),
                                       ("xyz", None), ("z", ("z", []))])
def test_combine_reference_against_loops(axes, swap):
    ms = MR.parse_axes(axes)
    st = (np.random.RandomState(len(axes) + 1).randn(len(ms), 3, 2, 2, 3) * 2).astype(F)        # W x H x D = 3 x 2 x 2, C = 3
    st[0, 1, 0, 0, 0] = np.nan
    st[-1, 2, 1, 1, 2] = np.inf
    st[0, 0, 1, 0, 1] = -np.inf
    st[0, :, 0, 1, 1] = 1.5                                        # a tie over all channels: the first index wins
    axis, pairs = MR.check_swap(swap[0], swap[1], 3, ms) if swap else (-1, [])
    mean, agr = MR._combine_reference(st, ms, swap)
    emean, eagr = loops_reference(st, ms, axis, pairs)
    assert mean.dtype == F and agr.dtype == np.uint8 and agr.shape == (2, 2, 3)
    assert np.array_equal(np.isnan(mean), np.isnan(emean)) and same(np.nan_to_num(mean, nan=7), np.nan_to_num(emean, nan=7))
    assert same(agr, eagr) and int(agr.max()) <= len(ms)
    if len(ms) == 1:
        assert same(mean, st[0])                                   # K = 1 copies member 0 bit for bit


def members_of(vol, masks, axis, pairs):
    """the stack whose member m is the FLIP_m / sigma_m image of one volume {C, D, H, W}"""
    sigma = np.arange(vol.shape[0])
    for a, b in pairs:
        sigma[a], sigma[b] = b, a
    out = []
    for m in masks:
        v = vol
        for bit, ax in ((0, 3), (1, 2), (2, 1)):
            if m >> bit & 1:
                v = np.flip(v, axis=ax)
        if axis >= 0 and m >> axis & 1:
            v = v[sigma]
        out.append(v)
    return np.ascontiguousarray(np.stack(out))


@pytest.mark.parametrize("axes", ["", "x", "y", "z", "xy", "xz", "yz", "xyz"])
def test_the_involution_returns_the_volume_and_full_agreement(axes):
    # the volume's values are multiples of 1/64 below 8 in size: every partial sum 2a .. 8a is then exact in fp32, as the scale is.
    # (For arbitrary fp32 values 3a, 5a, 6a and 7a round, and K = 8 equal terms need not give a back to the last bit.)
    ms = MR.parse_axes(axes)
    vol = (np.round(np.random.RandomState(3).randn(6, 3, 4, 5) * 64) / 64).astype(F)
    assert np.abs(vol).max() < 8 and len(np.unique(vol)) > 100
    for swap in (None, (axes[0], [(0, 1), (2, 5)])) if axes else (None,):
        axis, pairs = MR.check_swap(swap[0], swap[1], 6, ms) if swap else (-1, [])
        mean, agr = MR._combine_reference(members_of(vol, ms, axis, pairs), ms, swap)
        assert same(mean, vol)
        assert (agr == len(ms)).all()
