"""CPU: the host half of the post-processing chain (include/unet_postproc.h, unet-studio_amd/postproc.py) -- the ABI the library
exports, the scratch sizes, argument errors found before any device call, the chain parser, and the numpy union-find restatement of
the connected components checked against scipy.ndimage.label.  No device calls."""
import ctypes
import os
import re

import numpy as np
import pytest

import unet_studio_amd as U
from unet_studio_amd import postproc as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the numpy restatement of the chain (shared with tests/test_gpu_postproc.py) -----------------------------------------------
def components(mask):
    """6-connected components of a boolean {D, H, W} mask by vectorised union-find: every voxel starts as its own root; each
    round hooks every root onto the smallest root among its face neighbours' roots (np.minimum.at), then pointer jumping
    flattens the forest.  Returns int64 roots (the component's smallest linear index) with -1 outside the mask."""
    D, H, W = mask.shape
    idx = np.arange(mask.size, dtype=np.int64).reshape(mask.shape)
    parent = np.where(mask, idx, -1).reshape(-1)
    pairs = []
    for ax in range(3):
        a = [slice(None)] * 3
        b = [slice(None)] * 3
        a[ax], b[ax] = slice(1, None), slice(None, -1)
        both = mask[tuple(a)] & mask[tuple(b)]
        pairs.append((idx[tuple(a)][both], idx[tuple(b)][both]))
    u = np.concatenate([p[0] for p in pairs]) if pairs else np.zeros(0, np.int64)
    v = np.concatenate([p[1] for p in pairs]) if pairs else np.zeros(0, np.int64)

    def flatten():
        while True:
            q = parent[np.maximum(parent, 0)]
            q = np.where(parent >= 0, q, -1)
            if np.array_equal(q, parent):
                return
            parent[:] = q

    while True:
        ru, rv = parent[u], parent[v]
        diff = ru != rv
        if not diff.any():
            return parent.reshape(mask.shape)
        lo, hi = np.minimum(ru, rv)[diff], np.maximum(ru, rv)[diff]
        np.minimum.at(parent, hi, lo)     # every hooked root points at a smaller one: parents stay below their children
        flatten()


def kept_mask(mask, size_ratio):
    """mask voxels whose component has count >= size_ratio * largest count (in double)"""
    roots = components(mask)
    flat = roots.reshape(-1)
    counts = np.bincount(flat[flat >= 0], minlength=mask.size) if mask.any() else np.zeros(mask.size, np.int64)
    largest = counts.max() if mask.any() else 0
    keep = np.zeros(mask.size, bool)
    inm = flat >= 0
    keep[inm] = counts[flat[inm]].astype(np.float64) >= float(size_ratio) * float(largest)
    return keep.reshape(mask.shape)


# ---- the ABI ---------------------------------------------------------------------------------------------------------------------
def test_unet_postproc_h_declares_exactly_the_exports_and_the_library_has_them():
    lib = ctypes.CDLL(U.engine.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "unet_postproc.h")).read()
    declared = set(re.findall(r"\b(unet_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(P.EXPORTS) == {"unet_postproc_scratch_bytes", "unet_postproc_softmax", "unet_postproc_argmax_planes",
                                          "unet_postproc_defragment", "unet_postproc_plane_op"}
    for name in sorted(declared):
        assert hasattr(lib, name), "libunet_hip.so does not export " + name
    # the op numbers the Python side passes are the header's
    for name, val in re.findall(r"UNET_PP_([A-Z_]+) = (\d+)", hdr):
        assert getattr(P, "PP_" + name) == int(val)


def _slot(S):
    a = lambda b: (b + 255) // 256 * 256
    return 2 * a(4 * S) + a(4 * 2049)


def test_scratch_bytes_are_chunked_and_do_not_grow_with_the_classes():
    S = 192 * 224 * 192
    assert P.postproc_scratch_bytes(2, S) == 256 + 1 * _slot(S)
    assert P.postproc_scratch_bytes(4, 7) == 256 + 3 * _slot(7)
    assert P.postproc_scratch_bytes(6, S) == 256 + 4 * _slot(S)
    assert P.postproc_scratch_bytes(130, S) == P.postproc_scratch_bytes(6, S)      # UNET_POSTPROC_CHUNK planes at a time
    assert P.postproc_scratch_bytes(65536, 1) == 256 + 4 * _slot(1)


def test_argument_errors_need_no_device():
    with pytest.raises(U.UNetError, match="at least 2"):
        P.postproc_scratch_bytes(1, 100)
    with pytest.raises(U.UNetError, match="65535"):
        P.postproc_scratch_bytes(65537, 100)
    with pytest.raises(U.UNetError, match="voxels must be positive"):
        P.postproc_scratch_bytes(6, 0)
    with pytest.raises(U.UNetError, match="voxels must be positive"):
        P.postproc_scratch_bytes(6, -5)
    # the entry points refuse before touching the (fake, never dereferenced) pointers
    fake = ctypes.c_void_p(0x1000)
    lib = U.engine.lib

    def err(rc):
        assert rc != 0
        return lib.unet_last_error().decode()

    assert "at least 2" in err(lib.unet_postproc_softmax(fake, 1, 10, ctypes.c_float(0.5), fake, None, None, None))
    assert "65535" in err(lib.unet_postproc_softmax(fake, 70000, 10, ctypes.c_float(0.5), fake, None, None, None))
    assert "voxels must be positive" in err(lib.unet_postproc_softmax(fake, 3, 0, ctypes.c_float(0.5), fake, None, None, None))
    assert "no output" in err(lib.unet_postproc_softmax(fake, 3, 10, ctypes.c_float(0.5), None, None, None, None))
    assert "unknown op 7" in err(lib.unet_postproc_plane_op(7, ctypes.c_float(0), 2, 2, 2, fake, 1, fake, 1 << 20, None))
    assert "unknown op 0" in err(lib.unet_postproc_plane_op(0, ctypes.c_float(0), 2, 2, 2, fake, 1, fake, 1 << 20, None))
    assert "scratch too small" in err(lib.unet_postproc_plane_op(1, ctypes.c_float(0), 64, 64, 64, fake, 5, fake, 1000, None))
    assert "dimensions must be positive" in err(lib.unet_postproc_plane_op(1, ctypes.c_float(0), 0, 2, 2, fake, 1, fake, 1 << 20, None))
    assert "2^31" in err(lib.unet_postproc_plane_op(1, ctypes.c_float(0), 2048, 1024, 1024, fake, 1, fake, 1 << 20, None))
    assert "needs fg_prob" in err(lib.unet_postproc_defragment(4, 4, 4, 0, ctypes.c_float(0.5), ctypes.c_double(0.05), None, fake, 1,
                                                               None, fake, 1 << 20, None))
    assert "needs label_prob" in err(lib.unet_postproc_defragment(4, 4, 4, 1, ctypes.c_float(0.5), ctypes.c_double(0.05), fake, None, 0,
                                                                  None, fake, 1 << 20, None))
    assert "null scratch" in err(lib.unet_postproc_defragment(4, 4, 4, 0, ctypes.c_float(0.5), ctypes.c_double(0.05), fake, None, 0,
                                                              None, None, 1 << 20, None))


# ---- the chain parser ----------------------------------------------------------------------------------------------------------
def test_parse_chain_default_string_and_parameters():
    assert P.parse_chain("softmax+create_mask+argmax") == [("softmax", {}), ("create_mask", {}), ("argmax", {"threshold": 0.5})]
    assert P.parse_chain("") == [] and P.parse_chain(None) == []
    steps = P.parse_chain(" softmax + defragment_each+ minus+gaussian_smoothing ", {"minus": 0.25, "defragment_each": (0.5, 0.1)})
    assert steps == [("softmax", {}), ("defragment_each", {"threshold": 0.5, "size_ratio": 0.1}), ("minus", {"v": 0.25}),
                     ("gaussian_smoothing", {})]
    assert P.parse_chain("argmax", {"argmax": {"threshold": 0}}) == [("argmax", {"threshold": 0.0})]
    assert P.parse_chain("upper_threshold+lower_threshold+binarize+normalize_each+defragment") == [
        ("upper_threshold", {"t": 1.0}), ("lower_threshold", {"t": 0.0}), ("binarize", {"t": 0.5}), ("normalize_each", {}),
        ("defragment", {"threshold": 0.5, "size_ratio": 0.05})]
    with pytest.raises(U.UNetError, match="has no parameter"):
        P.parse_chain("argmax", {"argmax": {"t": 0}})
    with pytest.raises(U.UNetError, match="takes 1 parameter"):
        P.parse_chain("minus", {"minus": (1, 2)})


@pytest.mark.parametrize("chain,name", [("softmax+create_mask+argmax+soft_max", "soft_max"), ("anisotropic_smoothing", "anisotropic_smoothing"),
                                        ("softmax+Argmax", "Argmax"), ("defragment_smoothing", "defragment_smoothing")])
def test_parse_chain_refuses_unknown_commands_with_the_reference_message(chain, name):
    with pytest.raises(U.UNetError) as e:
        P.parse_chain(chain)
    assert str(e.value) == "unknown command " + name
    with pytest.raises(U.UNetError, match="^unknown command nope$"):
        P.parse_chain("softmax", {"nope": 1})


def test_chain_order_rules():
    P.check_chain(P.parse_chain("softmax+create_mask+argmax+defragment+defragment_each+normalize_each"))
    for chain, msg in [("argmax", "argmax needs softmax"), ("create_mask", "create_mask needs softmax"),
                       ("softmax+defragment", "defragment needs create_mask"), ("minus+softmax", "minus needs softmax")]:
        with pytest.raises(U.UNetError, match=msg):
            P.check_chain(P.parse_chain(chain))


def test_argmax_after_a_change_reads_the_state_and_create_mask_may_not_follow_one():
    ok = P.parse_chain("softmax+create_mask+defragment+argmax")
    P.check_chain(ok)
    assert P.argmax_after_change(ok) and P.needs_scratch(ok)
    default = P.parse_chain("softmax+create_mask+argmax+defragment")
    assert not P.argmax_after_change(default) and not P.needs_scratch(P.parse_chain("softmax+create_mask+argmax"))
    with pytest.raises(U.UNetError, match="^argmax after minus needs create_mask before it$"):
        P.check_chain(P.parse_chain("softmax+minus+argmax"))
    with pytest.raises(U.UNetError, match="^create_mask after defragment_each is not supported"):
        P.check_chain(P.parse_chain("softmax+defragment_each+create_mask+argmax"))


def test_outputs_the_chain_does_not_produce_are_refused():
    steps = P.parse_chain("softmax+create_mask")
    P.check_outputs(steps, ("label_prob", "fg_prob"))
    with pytest.raises(U.UNetError, match="^output label is not produced by the chain \\(it needs argmax\\)$"):
        P.check_outputs(steps, ("label",))
    with pytest.raises(U.UNetError, match="unknown output mask"):
        P.check_outputs(steps, ("mask",))
    with pytest.raises(U.UNetError, match="output label_prob is not produced"):
        P.check_outputs([], ("label_prob",))


def test_volume_limits_are_refused_before_the_device():
    fake = ctypes.c_void_p(0x1000)
    lib = U.engine.lib
    rc = lib.unet_postproc_plane_op(6, ctypes.c_float(0), 1, 4 * 65535 + 1, 1, fake, 1, fake, 1 << 30, None)
    assert rc != 0 and "4 x 65535 rows" in lib.unet_last_error().decode()
    rc = lib.unet_postproc_defragment(1, 1, 65536, 0, ctypes.c_float(0.5), ctypes.c_double(0.05), fake, None, 0, None, fake, 1 << 30, None)
    assert rc != 0 and "65535 slices" in lib.unet_last_error().decode()
    rc = lib.unet_postproc_argmax_planes(fake, 0, 10, fake, ctypes.c_float(0.5), fake, None)
    assert rc != 0 and "at least 2" in lib.unet_last_error().decode()
    rc = lib.unet_postproc_argmax_planes(fake, 3, 10, None, ctypes.c_float(0.5), fake, None)
    assert rc != 0 and "null device pointer" in lib.unet_last_error().decode()


def test_default_model_chain_is_the_reference_default():
    assert "softmax+create_mask+argmax" in open(os.path.join(ROOT, "unet-studio_amd", "unet3d.py")).read()


# ---- the union-find restatement against scipy ----------------------------------------------------------------------------------
def test_union_find_restatement_matches_scipy_label():
    nd = pytest.importorskip("scipy.ndimage")
    rs = np.random.RandomState(0)
    shapes = [(1, 1, 1), (1, 1, 17), (3, 5, 7), (8, 8, 8), (5, 1, 9), (12, 10, 11)]
    for shape in shapes:
        for density in (0.0, 0.2, 0.31, 0.5, 1.0):
            mask = rs.rand(*shape) < density
            roots = components(mask)
            lab, n = nd.label(mask)       # default structure: 6-connectivity in 3-D
            assert ((roots >= 0) == (lab > 0)).all()
            # the same partition: a bijection between the two labelings, and every root is its component's smallest index
            pairs = set(zip(roots[mask].tolist(), lab[mask].tolist()))
            assert len(pairs) == n == len(set(roots[mask].tolist()))
            flat = roots.reshape(-1)
            for r in set(flat[flat >= 0].tolist()):
                assert flat[r] == r and np.flatnonzero(flat == r).min() == r


def test_kept_mask_size_ratio_boundary():
    # components of 20, 10 and 1 voxels: 10 >= 0.5 * 20 is kept, 1 is not; 1 >= 0.05 * 20 is kept
    mask = np.zeros((1, 3, 25), bool)
    mask[0, 0, :20] = True
    mask[0, 2, :10] = True
    mask[0, 2, 24] = True
    k = kept_mask(mask, 0.5)
    assert k[0, 0, :20].all() and k[0, 2, :10].all() and not k[0, 2, 24]
    assert kept_mask(mask, 0.05)[0, 2, 24]
    assert not kept_mask(np.zeros((2, 2, 2), bool), 0.05).any()
