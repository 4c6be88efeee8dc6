"""CPU: the host half of connected components with a chosen connectivity (include/unet_connectivity.h,
unet-studio_amd/connectivity.py) -- this file's restatements (`label_ref`, `keep_largest_ref`, `holes_ref`: scipy.ndimage.label with
generate_binary_structure(3, 1 | 2 | 3), importing nothing of the package's kernels), the half neighbourhoods the kernels hook to, the
maps the GPU tests share, the ABI the library exports, every argument error before any device call (and the whole text of each,
as tests/golden/conn_abi_errors.json records it), the ops `check_ops` accepts, and the facts the definitions rest on.  No device
calls.  Shapes are (D, H, W)."""
import ctypes
import json
import os
import re
import sys

import numpy as np
import pytest
import torch
from scipy import ndimage

import unet_studio_amd as U
from unet_studio_amd import connectivity as CN
from unet_studio_amd import morph as MO

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_instances_host as TIH  # noqa: E402
import test_morph_host as TMH  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONNS = (6, 18, 26)
RANK = {6: 1, 18: 2, 26: 3}
TILE = (32, 8, 8)                                                  # (TX, TY, TZ) of the tiled labelling


def structure(c):
    return ndimage.generate_binary_structure(3, RANK[c])


# ---- the restatements ------------------------------------------------------------------------------------------------------------
def label_ref(labels, classes, c, n_classes=None):
    """(inst int32 (D, H, W), N): per listed class scipy.ndimage.label with the structure of c; the components of all classes
    together renumbered 1..N in the order of their smallest linear index; 0 elsewhere"""
    lab = np.asarray(labels)
    firsts, comps = [], []
    for v in sorted(set(int(k) for k in classes)):
        assert v > 0 and (n_classes is None or v < n_classes)
        comp, n = ndimage.label(lab == v, structure=structure(c))
        flat = comp.reshape(-1)
        idx = np.flatnonzero(flat)                                 # ascending: the first occurrence of an id is its smallest index
        ids, at = np.unique(flat[idx], return_index=True)
        assert ids.tolist() == list(range(1, n + 1))
        firsts.append(idx[at])
        comps.append(comp)
    inst = np.zeros(lab.shape, np.int32)
    if not firsts:
        return inst, 0
    order = np.argsort(np.concatenate(firsts), kind="stable")
    new_id = np.empty(order.size, np.int64)
    new_id[order] = np.arange(1, order.size + 1)
    base = 0
    for comp, first in zip(comps, firsts):
        table = np.concatenate([[0], new_id[base:base + first.size]])
        inst += table[comp].astype(np.int32)
        base += first.size
    return inst, int(order.size)


def keep_largest_ref(labels, classes, n_classes, c):
    """(result uint16, removed uint32[n_classes]) from label_ref: per listed class the instance with the most voxels stays, among
    equal counts the one with the smaller id (ids increase with the smallest linear index); the others become 0"""
    lab = np.asarray(labels)
    inst, n = label_ref(lab, classes, c, n_classes)
    out = lab.astype(np.uint16).copy()
    removed = np.zeros(n_classes, np.uint32)
    counts = np.bincount(inst.reshape(-1), minlength=n + 1)
    cls = np.zeros(n + 1, np.int64)
    cls[inst.reshape(-1)] = lab.reshape(-1)
    for v in sorted(set(int(k) for k in classes)):
        ids = np.flatnonzero(cls[1:] == v) + 1
        if ids.size == 0:
            continue
        best = ids[np.argmax(counts[ids])]                          # argmax returns the first maximum: the smallest id
        gone = (lab == v) & (inst != best)
        out[gone] = 0
        removed[v] = int(gone.sum())
    return out, removed


def holes_ref(m, c):
    """(the voxels of the holes, their number): the c-connected components of the complement minus those with a voxel on a face"""
    m = np.asarray(m, bool)
    lab, n = ndimage.label(~m, structure=structure(c))
    face = np.zeros(n + 1, bool)
    for axis in range(3):
        for side in (0, -1):
            face[np.unique(np.take(lab, side, axis=axis))] = True
    face[0] = True                                                 # the mask itself is no hole
    return ~face[lab], int(n + 1 - face.sum())


# ---- the maps, shared with the GPU tests --------------------------------------------------------------------------------------------
NC = 4                                                             # classes 1, 2 listed; 3 is a value of the maps that is not
LISTED = [1, 2]
SHAPES = [(1, 1, 1), (3, 5, 7), (2, 2, 33), (2, 9, 3), (9, 2, 3), (9, 9, 33), (17, 17, 65), (38, 44, 40), (2, 3, 70000)]
HOST_SHAPES = SHAPES[:7]


def checkerboard(shape):
    z, y, x = np.indices(shape)
    return ((x + y + z) % 2 == 0).astype(np.int64)


def random_map(shape, density):
    rng = np.random.default_rng(int(density * 100) + shape[2])
    return np.where(rng.random(shape) < density, rng.integers(1, NC, shape), 0)


def diagonal(shape, planar, start=(0, 0, 0), n=20):
    """the line x = x0 + t, y = y0 + t (and z = z0 + t unless planar), clipped to the grid; class 1"""
    lab = np.zeros(shape, np.int64)
    for t in range(n):
        z, y, x = start[0] + (0 if planar else t), start[1] + t, start[2] + t
        if 0 <= z < shape[0] and 0 <= y < shape[1] and 0 <= x < shape[2]:
            lab[z, y, x] = 1
    return lab


def corner_start(shape):
    """where a diagonal starts so that, in a grid with room, it crosses the tile corner at x = 31|32, y = 7|8, z = 7|8"""
    return tuple(max(0, min(t, n) - 4) for t, n in zip((TILE[2], TILE[1], TILE[0]), shape))


MAPS = {
    "empty": lambda s: np.zeros(s, np.int64),
    "full": lambda s: np.ones(s, np.int64),
    "random10": lambda s: random_map(s, 0.1),
    "random30": lambda s: random_map(s, 0.3),
    "random50": lambda s: random_map(s, 0.5),
    "checkerboard": checkerboard,
    "space_diagonal": lambda s: diagonal(s, False, corner_start(s), 10),
    "plane_diagonal": lambda s: diagonal(s, True, corner_start(s), 10),
}


def pair_cases():
    """(shape, p, o, crossed): a grid of 2 x 2 x 2 tiles (the last ones partial), a voxel p = (x, y, z) and an offset o = (dx, dy, dz)
    of N-(26) with p + o inside, for every o and every subset of its non-zero axes as the tile boundaries the pair crosses: along a
    crossed axis p sits right above the boundary for a step down (the neighbour across p's low face) and right below it for a step up
    (across its high face); along the others p is inside a tile"""
    shape = (12, 12, 40)                                           # (D, H, W)
    cases = []
    for o in CN.backward_offsets(26):
        axes = [a for a in range(3) if o[a]]
        for mask in range(1, 1 << len(axes)):
            crossed = [axes[i] for i in range(len(axes)) if mask >> i & 1]
            p = tuple((TILE[a] if o[a] < 0 else TILE[a] - 1) if a in crossed else 3 for a in range(3))
            cases.append((shape, p, o, tuple(crossed)))
    return cases


def pair_map(shape, p, o):
    lab = np.zeros(shape, np.int64)
    lab[p[2], p[1], p[0]] = 1
    lab[p[2] + o[2], p[1] + o[1], p[0] + o[0]] = 1
    return lab


# ---- the restatements against each other and scipy -----------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", HOST_SHAPES, ids=str)
def test_label_ref_at_6_is_the_older_restatement_and_ids_follow_the_smallest_index(shape):
    for name, f in MAPS.items():
        lab = f(shape)
        inst, n = label_ref(lab, LISTED, 6, NC)
        old, n_old = TIH.label_ref(lab, NC, LISTED)
        assert n == n_old and inst.tobytes() == old.astype(np.int32).tobytes(), name
        for c in CONNS:
            inst, n = label_ref(lab, LISTED, c, NC)
            flat = inst.reshape(-1)
            first = [int(np.flatnonzero(flat == k)[0]) for k in range(1, min(n, 50) + 1)]
            assert first == sorted(first) and ((inst > 0) == np.isin(lab, LISTED)).all(), (name, c)
            # two touching components of different classes never merge
            both = ndimage.label(np.isin(lab, LISTED), structure=structure(c))[1]
            assert n >= both, (name, c)


@pytest.mark.parametrize("shape", HOST_SHAPES, ids=str)
def test_one_mask_is_numbered_as_scipy_numbers_it(shape):
    for c in CONNS:
        for name in ("random30", "checkerboard", "space_diagonal"):
            m = MAPS[name](shape) > 0
            inst, n = label_ref(m.astype(np.int64), [1], c)
            want, n_want = ndimage.label(m, structure=structure(c))
            assert n == n_want and (inst == want).all(), (c, name)


@pytest.mark.parametrize("shape", HOST_SHAPES, ids=str)
def test_keep_largest_ref_at_6_is_the_older_restatement(shape):
    import test_components_host as TCH
    for name, f in MAPS.items():
        lab = f(shape)
        got, removed = keep_largest_ref(lab, LISTED, NC, 6)
        want, want_removed = TCH.keep_largest_ref(lab, LISTED, NC)
        assert got.tobytes() == want.tobytes() and removed.tobytes() == want_removed.tobytes(), name


@pytest.mark.parametrize("shape", TMH.HOST_SHAPES + [(38, 44, 40)], ids=str)
def test_holes_ref_is_binary_fill_holes_with_the_structure(shape):
    for name, f in TMH.MAPS.items():
        m = f(shape)
        old = TMH.holes_ref(m)
        got = holes_ref(m, 6)
        assert (got[0] == old[0]).all() and got[1] == old[1], name
        for c in CONNS:
            holes, n = holes_ref(m, c)
            assert not (holes & m).any() and ((m | holes) == ndimage.binary_fill_holes(m, structure=structure(c))).all(), (name, c)
            assert n == ndimage.label(holes, structure=structure(c))[1], (name, c)


# ---- the half neighbourhoods ---------------------------------------------------------------------------------------------------------
def test_the_backward_halves_make_the_structures():
    for c, size in zip(CONNS, (3, 9, 13)):
        back = CN.backward_offsets(c)
        assert len(back) == len(set(back)) == size
        whole = set(back) | {(-dx, -dy, -dz) for dx, dy, dz in back}
        want = {(x - 1, y - 1, z - 1) for z, y, x in zip(*np.nonzero(structure(c)))} - {(0, 0, 0)}
        assert whole == want and len(whole) == c
        for dx, dy, dz in back:                                    # the neighbour's linear index is smaller in every grid
            assert dz * 10000 + dy * 100 + dx < 0
            assert dz == -1 or (dz == 0 and dy == -1) or (dz == 0 and dy == 0 and dx == -1)
    assert set(CN.backward_offsets(6)) < set(CN.backward_offsets(18)) < set(CN.backward_offsets(26))
    assert (1, 0, -1) in CN.backward_offsets(18) and (0, 1, -1) in CN.backward_offsets(18) and (1, -1, 0) in CN.backward_offsets(18)
    for bad in (7, 0, 27, -6, None, 6.0, True, "26"):
        with pytest.raises(U.UNetError, match="connectivity must be 6, 18 or 26, got"):
            CN.check(bad)
    # the kernels' enumeration is the same rule
    src = open(os.path.join(ROOT, "unet-studio_amd", "csrc", "cc_union_find.h")).read()
    assert "cc_for_backward" in src and "dz < 0 || (dz == 0 && (dy < 0 || (dy == 0 && dx < 0)))" in src


def test_the_pair_cases_cover_every_offset_every_boundary_subset_and_both_sides():
    cases = pair_cases()
    assert len(cases) == 3 * 1 + 6 * 3 + 4 * 7 == 49
    seen = set()
    for shape, p, o, crossed in cases:
        q = tuple(p[a] + o[a] for a in range(3))
        assert all(0 <= q[a] < shape[2 - a] and 0 <= p[a] < shape[2 - a] for a in range(3))
        differ = tuple(a for a in range(3) if p[a] // TILE[a] != q[a] // TILE[a])
        assert differ == crossed and 1 <= len(crossed) <= sum(1 for v in o if v)
        seen.add((o, crossed))
        lab = pair_map(shape, p, o)
        for c in CONNS:
            assert label_ref(lab, [1], c)[1] == (1 if sum(abs(v) for v in o) <= RANK[c] else 2)
    assert len(seen) == 49
    high = [(o, cr) for _, p, o, cr in cases if any(o[a] > 0 and a in cr for a in range(3))]
    low = [(o, cr) for _, p, o, cr in cases if any(o[a] < 0 and a in cr for a in range(3))]
    assert high and low and any(len(cr) == 3 for _, cr in low)      # a neighbour across a high face, a low face, three faces at once


# ---- the ABI -------------------------------------------------------------------------------------------------------------------------
OLDER = ("unet_morph_", "unet_inst_", "unet_dist_", "unet_table_", "unet_reg_", "unet_atlas_", "unet_components_", "unet_preproc_",
         "unet_tiles_", "unet_space_", "unet_postproc_", "unet_qc_", "unet_feed_")


def test_unet_connectivity_h_declares_exactly_the_exports_and_the_library_has_them():
    lib = ctypes.CDLL(U.engine.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "unet_connectivity.h")).read()
    declared = set(re.findall(r"\b(unet_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(CN.EXPORTS) == {"unet_conn_scratch_bytes", "unet_conn_keep_largest", "unet_conn_label_scratch_bytes",
                                           "unet_conn_label", "unet_conn_holes_scratch_bytes", "unet_conn_holes"}
    for name in sorted(declared):
        assert hasattr(lib, name), "libunet_hip.so does not export " + name
    enums = {k: int(v) for k, v in re.findall(r"UNET_CONN_([A-Z_]+) = (\d+)", hdr)}
    assert enums == {"IMPL_DEFAULT": CN.IMPL_DEFAULT, "IMPL_TILED": CN.IMPL_TILED, "IMPL_GLOBAL": CN.IMPL_GLOBAL}
    assert (CN.IMPL_DEFAULT, CN.IMPL_TILED, CN.IMPL_GLOBAL) == (0, 1, 2)
    defines = {k: int(v) for k, v in re.findall(r"#define UNET_CONN_(\d+) (\d+)", hdr)}
    assert defines == {"6": CN.CONN_6, "18": CN.CONN_18, "26": CN.CONN_26} and CN.CONNECTIVITIES == (6, 18, 26)
    assert "this project's" in hdr and "NOT pinned" in hdr
    assert U.connectivity is CN
    # the older modules' lists stay as they are
    assert U.components.EXPORTS == ["unet_components_scratch_bytes", "unet_components_keep_largest"]
    assert len(U.instances.EXPORTS) == 5 and len(MO.EXPORTS) == 7


def test_the_new_prefix_stays_in_its_header_and_names_the_others_by_file_only():
    for h in sorted(os.listdir(os.path.join(ROOT, "include"))):
        text = open(os.path.join(ROOT, "include", h)).read().lower()
        if h != "unet_connectivity.h":
            assert "unet_conn_" not in text, h
        else:
            for other in OLDER:
                assert other not in text, other
            for name in ("unet_components.h", "unet_instances.h", "unet_morph.h"):
                assert name in text, name


# ---- argument errors, before any device call -------------------------------------------------------------------------------------
P = [ctypes.c_void_p(0x1000 * (i + 1)) for i in range(8)]          # never dereferenced
ODD = ctypes.c_void_p(0x7004)                                      # 4-byte aligned only
ODD2 = ctypes.c_void_p(0x7002)                                     # 2-byte aligned only
BIG = 1 << 40
GRID_ERRORS = (((0, 4, 4), "dimensions (w, h, d) must be positive"), ((4, -1, 4), "dimensions"), ((4, 4, 0), "dimensions"),
               ((2048, 1024, 1024), "voxels must be in [1, 2^31), got 2147483648"))
BAD_CONNS = (7, 0, 8, 27, -6, 1)


def failing(f, *args):
    assert f(*args) != 0
    return U.engine.lib.unet_last_error().decode()


def test_scratch_sizes_are_the_siblings_and_check_their_arguments():
    lib = U.engine.lib
    for S, nc in ((1, 1), (4096, 3), (256 ** 3, 200), ((1 << 31) - 1, 65536)):
        assert CN.keep_largest_scratch_bytes(S, nc) == U.components.components_scratch_bytes(S, nc)
        for M in (0, 1, 65535):
            assert CN.label_scratch_bytes(S, nc, M) == U.instances.inst_scratch_bytes(S, nc, M)
    for shape in ((1, 1, 1), (3, 5, 7), (256, 256, 256), (1, 1, (1 << 31) - 1)):
        assert CN.holes_scratch_bytes(shape) == MO.morph_scratch_bytes(shape)
    n = ctypes.c_size_t()
    for S, nc, msg in ((0, 3, "voxels must be in [1, 2^31), got 0"), (1 << 31, 3, "voxels must be in [1, 2^31), got 2147483648"),
                       (8, 0, "n_classes must be in [1, 65536], got 0"), (8, 65537, "n_classes must be in [1, 65536], got 65537")):
        assert "unet_conn_scratch_bytes: " + msg in failing(lib.unet_conn_scratch_bytes, S, nc, ctypes.byref(n))
        assert "unet_conn_label_scratch_bytes: " + msg in failing(lib.unet_conn_label_scratch_bytes, S, nc, 4, ctypes.byref(n))
    assert "unet_conn_scratch_bytes: null bytes" in failing(lib.unet_conn_scratch_bytes, 8, 3, None)
    assert "unet_conn_label_scratch_bytes: null bytes" in failing(lib.unet_conn_label_scratch_bytes, 8, 3, 4, None)
    assert "max_instances must be in [0, 2147483646], got -1" in failing(lib.unet_conn_label_scratch_bytes, 8, 3, -1, ctypes.byref(n))
    assert "max_instances must be in [0, 2147483646], got 2147483647" in failing(lib.unet_conn_label_scratch_bytes, 8, 3, (1 << 31) - 1,
                                                                                 ctypes.byref(n))
    for dims, msg in GRID_ERRORS:
        assert "unet_conn_holes_scratch_bytes: " + msg in failing(lib.unet_conn_holes_scratch_bytes, *dims, ctypes.byref(n))
        with pytest.raises(U.UNetError, match=re.escape(msg)):
            CN.holes_scratch_bytes(dims[::-1])
    assert "unet_conn_holes_scratch_bytes: null bytes" in failing(lib.unet_conn_holes_scratch_bytes, 4, 4, 4, None)


def test_keep_largest_argument_errors_need_no_device():
    lib = U.engine.lib
    small = CN.keep_largest_scratch_bytes(64, 3)

    def call(dims=(4, 4, 4), label=P[0], nc=3, listed=(1, 2), n_listed=None, removed=P[1], c=26, impl=0, scratch=P[2], scratch_bytes=BIG):
        arr = (ctypes.c_uint32 * max(1, len(listed)))(*listed) if listed is not None else None
        msg = failing(lib.unet_conn_keep_largest, *dims, label, nc, arr, len(listed) if n_listed is None else n_listed, removed, c, impl,
                      scratch, scratch_bytes, None)
        assert msg.startswith("unet_conn_keep_largest: "), msg
        return msg

    for dims, msg in GRID_ERRORS:
        assert msg in call(dims=dims)
    assert "n_classes must be in [1, 65536], got 0" in call(nc=0) and "n_classes must be in [1, 65536], got 65537" in call(nc=65537)
    assert "null label" in call(label=None)
    assert "n_listed must not be negative, got -1" in call(n_listed=-1) and "null listed" in call(listed=None, n_listed=2)
    for c in BAD_CONNS:
        assert "connectivity must be 6, 18 or 26, got %d" % c in call(c=c)
    assert "unknown impl 3" in call(impl=3) and "unknown impl -1" in call(impl=-1)
    assert "null scratch" in call(scratch=None) and "null scratch" in call(removed=None, scratch=None)     # removed is optional
    assert "scratch too small (see unet_conn_scratch_bytes)" in call(scratch_bytes=small - 1)
    assert "scratch too small" in call(dims=(40, 40, 40), scratch_bytes=small)
    assert "listed class 0 is not in [1, 2]" in call(listed=(1, 0)) and "listed class 3 is not in [1, 2]" in call(listed=(3,))
    assert "listed class 1 is not in [1, 0]" in call(nc=1, listed=(1,))


def test_label_argument_errors_need_no_device():
    lib = U.engine.lib
    small = CN.label_scratch_bytes(64, 3, 5)

    def call(dims=(4, 4, 4), label=P[0], nc=3, listed=(1, 2), n_listed=None, inst=P[1], rows=P[2], M=5, info=P[3], c=18, impl=0,
             scratch=P[4], scratch_bytes=BIG):
        arr = (ctypes.c_uint32 * max(1, len(listed)))(*listed) if listed is not None else None
        msg = failing(lib.unet_conn_label, *dims, label, nc, arr, len(listed) if n_listed is None else n_listed, inst, rows, M, info, c, impl,
                      scratch, scratch_bytes, None)
        assert msg.startswith("unet_conn_label: "), msg
        return msg

    for dims, msg in GRID_ERRORS:
        assert msg in call(dims=dims)
    assert "n_classes must be in [1, 65536], got 0" in call(nc=0) and "n_classes must be in [1, 65536], got 65537" in call(nc=65537)
    assert "max_instances must be in [0, 2147483646], got -1" in call(M=-1)
    assert "null label" in call(label=None)
    assert "n_listed must not be negative, got -1" in call(n_listed=-1) and "null listed" in call(listed=None, n_listed=2)
    assert "null inst" in call(inst=None) and "inst must be 4-byte aligned" in call(inst=ODD2)
    assert "null rows" in call(rows=None) and "rows must be 8-byte aligned" in call(rows=ODD)
    assert "null info" in call(info=None) and "info must be 8-byte aligned" in call(info=ODD)
    for c in BAD_CONNS:
        assert "connectivity must be 6, 18 or 26, got %d" % c in call(c=c)
    assert "unknown impl 3" in call(impl=3) and "unknown impl -1" in call(impl=-1)
    assert "null scratch" in call(scratch=None)
    assert "scratch too small (see unet_conn_label_scratch_bytes)" in call(scratch_bytes=small - 1)
    assert "scratch too small" in call(M=6, scratch_bytes=small - 1) and "scratch too small" in call(dims=(40, 40, 40), scratch_bytes=small)
    assert "listed class 0 is not in [1, 2]" in call(listed=(1, 0)) and "listed class 3 is not in [1, 2]" in call(listed=(3,))


def test_holes_argument_errors_need_no_device():
    lib = U.engine.lib
    small = CN.holes_scratch_bytes((4, 4, 4))

    def call(dims=(4, 4, 4), src=P[0], dst=P[1], info=P[2], c=26, impl=0, scratch=P[3], scratch_bytes=BIG):
        msg = failing(lib.unet_conn_holes, *dims, src, dst, info, c, impl, scratch, scratch_bytes, None)
        assert msg.startswith("unet_conn_holes: "), msg
        return msg

    for dims, msg in GRID_ERRORS:
        assert msg in call(dims=dims)
    assert "null in" in call(src=None) and "in must be 8-byte aligned" in call(src=ODD)
    assert "null out" in call(dst=None) and "out must be 8-byte aligned" in call(dst=ODD)
    assert "info must be 8-byte aligned" in call(info=ODD)
    for c in BAD_CONNS:
        assert "connectivity must be 6, 18 or 26, got %d" % c in call(c=c)
    assert "unknown impl 3" in call(impl=3) and "unknown impl -1" in call(impl=-1)
    assert "null scratch" in call(scratch=None) and "null scratch" in call(info=None, scratch=None)    # info is optional
    assert "scratch too small (see unet_conn_holes_scratch_bytes)" in call(scratch_bytes=small - 1)
    assert "scratch too small" in call(dims=(40, 40, 40), scratch_bytes=small)


def test_wrapper_errors_need_no_device():
    t16 = torch.zeros((2, 2, 2), dtype=torch.uint16)                # a host tensor
    for c in (7, 0, None, 6.0):                                      # the connectivity is refused before the tensor is looked at
        for f, args in ((CN.keep_largest, (t16, [1], 3)), (U.components.keep_largest, (t16, [1], 3)), (CN.label, (t16, 3)),
                        (U.instances.label, (t16, 3)), (U.instances.lesion_scores, (t16, t16, 3)), (MO.fill_holes_label, (t16, [1], 1, 3))):
            with pytest.raises(U.UNetError, match="connectivity must be 6, 18 or 26, got"):
                f(*args, connectivity=c)
    for c in CONNS:
        with pytest.raises(U.UNetError, match="device tensor"):
            CN.keep_largest(t16, [1], 3, c)
        with pytest.raises(U.UNetError, match="device tensor"):
            U.components.keep_largest(t16, [1], 3, connectivity=c)
        with pytest.raises(U.UNetError, match="device tensor"):
            CN.label(t16, 3, connectivity=c)
        with pytest.raises(U.UNetError, match="device tensor"):
            U.instances.label(t16, 3, connectivity=c)
        with pytest.raises(U.UNetError, match="must be a morph.Mask"):
            CN.fill_holes(t16, c)
        with pytest.raises(U.UNetError, match="must be a morph.Mask"):
            MO.fill_holes(t16, connectivity=c)
        with pytest.raises(U.UNetError, match="device tensor"):
            MO.fill_holes_label(t16, [1], 1, 3, connectivity=c)
    with pytest.raises(U.UNetError, match="single_component: connectivity must be 6, 18 or 26, got 7"):
        U.run_postproc(torch.zeros((3, 2, 2, 2)), "softmax+create_mask+argmax", single_component=[1], single_component_connectivity=7)
    assert U.qc.lesion_qc(None, "m.nz", [], connectivity=7) == (1, "lesion_qc: connectivity must be 6, 18 or 26, got 7")
    assert "6, 18 or 26" in U.qc.lesion_qc.__doc__ and "6-connected" not in U.qc.lesion_qc.__doc__


# ---- the whole texts of those errors (tests/golden/conn_abi_errors.json) -------------------------------------------------------------
class ClaimsDevice(torch.Tensor):
    """a host tensor that answers is_cuda with True: it passes a wrapper's check of the tensor, so the checks behind it (the scratch
    size, the listed classes) are reached on a machine without a device"""
    is_cuda = True


def abi_error(case):
    """unet_last_error() after one recorded C call.  args: an int or null as it is, a list as a uint32 array, "out" as a size_t
    to write to"""
    args = [(ctypes.c_uint32 * max(1, len(a)))(*a) if isinstance(a, list) else ctypes.byref(ctypes.c_size_t()) if a == "out" else a
            for a in case["args"]]
    return failing(getattr(U.engine.lib, case["fn"]), *args)


def python_error(case):
    """the UNetError text of one recorded call of a wrapper: its first argument is a (2, 2, 2) uint16 host tensor ("host") or the
    same as a ClaimsDevice ("claims_device")"""
    t = torch.zeros((2, 2, 2), dtype=torch.uint16)
    if case["tensor"] == "claims_device":
        t = t.as_subclass(ClaimsDevice)
    module, name = case["fn"].split(".")
    with pytest.raises(U.UNetError) as e:
        getattr(getattr(U, module), name)(t, *case["args"], **case["kwargs"])
    return str(e.value)


def test_every_argument_error_of_the_twelve_calls_and_six_wrappers_reads_as_recorded():
    """The file was recorded from the commit before keep-largest, instance labelling and hole filling got one body per operation: the
    cases the argument-error tests of test_components_host, test_instances_host, test_morph_host and this file drive through
    unet_components_* / unet_inst_scratch_bytes / unet_inst_label / unet_morph_scratch_bytes / unet_morph_holes / unet_conn_*, and
    through the six wrappers a bad connectivity, a host tensor and a listed class of -1 and of 2^32.  Every case fails before any
    device call."""
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "conn_abi_errors.json")))
    assert {c["fn"] for c in golden["abi"]} == set(CN.EXPORTS) | set(U.components.EXPORTS) | {
        "unet_inst_scratch_bytes", "unet_inst_label", "unet_morph_scratch_bytes", "unet_morph_holes"}
    assert {c["fn"] for c in golden["python"]} == {"components.keep_largest", "instances.label", "morph.fill_holes",
                                                    "connectivity.keep_largest", "connectivity.label", "connectivity.fill_holes"}
    for case in golden["abi"]:
        assert abi_error(case) == case["error"], case
    for case in golden["python"]:
        assert python_error(case) == case["error"], case


# ---- check_ops -----------------------------------------------------------------------------------------------------------------------
def test_check_ops_accepts_the_four_element_fill_holes_and_refuses_a_bad_connectivity_naming_the_op():
    ops = MO.check_ops([("fill_holes", (1, 2), 1, 26), ["fill_holes", [2], 2, 18], ("fill_holes", [1], 1, 6), ("fill_holes", (1, 2), 1)], 3)
    assert ops == [("fill_holes", [1, 2], 1, 26), ("fill_holes", [2], 2, 18), ("fill_holes", [1], 1, 6), ("fill_holes", [1, 2], 1)]
    labels = torch.zeros((2, 2, 2), dtype=torch.uint16)            # a host tensor: the ops are refused before it is looked at
    for bad in (("fill_holes", [1], 1, 7), ("fill_holes", [1], 1, 0), ("fill_holes", [1], 1, 26.0), ("fill_holes", [1], 1, True),
                ("fill_holes", [1], 1, 26, 1), ("fill_holes", [1], 1, None)):
        with pytest.raises(U.UNetError, match=re.escape("morphology: op 1 %r" % (bad,))):
            MO.run(labels, [("close", 1, 26, 1), bad], 3)
    with pytest.raises(U.UNetError, match=re.escape("morphology: op 0 ('fill_holes', [1], 1, 7): connectivity must be 6, 18 or 26")):
        MO.check_ops([("fill_holes", [1], 1, 7)], 3)
    with pytest.raises(U.UNetError, match="device tensor"):        # good ops: now the label map is looked at
        MO.run(labels, [("fill_holes", [1], 1, 26)], 3)


# ---- the facts the definitions rest on -------------------------------------------------------------------------------------------------
def shell(opening=None):
    """a 5^3 shell with a 3^3 cavity in a 9^3 grid; opening removes one voxel of the shell: the middle of a face, the middle of an
    edge, or a corner"""
    m = np.zeros((9, 9, 9), bool)
    m[2:7, 2:7, 2:7] = True
    m[3:6, 3:6, 3:6] = False
    at = {"face": (2, 4, 4), "edge": (2, 2, 4), "corner": (2, 2, 2)}
    if opening:
        m[at[opening]] = False
    return m


def test_the_facts_the_definitions_rest_on():
    def count(lab, c):
        return label_ref(lab, [1], c)[1]

    board = checkerboard((9, 9, 33))
    assert [count(board, c) for c in CONNS] == [1337, 1, 1]
    space = diagonal((20, 20, 40), False, (0, 0, 20))               # x = y + 20 = z + 20
    assert space.sum() == 20 and [count(space, c) for c in CONNS] == [20, 20, 1]
    plane = diagonal((20, 20, 40), True, (3, 0, 20))                # in one z plane, x = y + 20
    assert plane.sum() == 20 and [count(plane, c) for c in CONNS] == [20, 1, 1]
    for opening, want in ((None, (27, 27, 27)), ("face", (0, 0, 0)), ("edge", (27, 0, 0)), ("corner", (27, 27, 0))):
        m = shell(opening)
        assert tuple(int(holes_ref(m, c)[0].sum()) for c in CONNS) == want, opening
        assert tuple(int((ndimage.binary_fill_holes(m, structure=structure(c)) & ~m).sum()) for c in CONNS) == want, opening
    # the shifted lines of the GPU tests cross the corner where eight tiles meet
    for shape in ((9, 9, 33), (17, 17, 65), (38, 44, 40)):
        z, y, x = np.nonzero(MAPS["space_diagonal"](shape))
        assert {(int(a) // 8, int(b) // 8, int(c) // 32) for a, b, c in zip(z, y, x)} == {(0, 0, 0), (1, 1, 1)}
        n = int(MAPS["space_diagonal"](shape).sum())
        assert 5 <= n <= 10 and [count(MAPS["space_diagonal"](shape), c) for c in CONNS] == [n, n, 1]
        n = int(MAPS["plane_diagonal"](shape).sum())
        assert 5 <= n <= 10 and [count(MAPS["plane_diagonal"](shape), c) for c in CONNS] == [n, 1, 1]
