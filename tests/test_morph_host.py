"""CPU: the host half of binary morphology on bit-packed masks (include/unet_morph.h, unet-studio_amd/morph.py) -- this file's own
restatements of the header's definitions (`step_ref`, `holes_ref`, `pack_ref` / `unpack_ref`: plain numpy on booleans, importing nothing
of the package's kernels) checked against scipy.ndimage as the second witness and on their properties, the maps the GPU tests share,
the ABI the library exports, argument errors found before any device call, and the ops `run` refuses.  No device calls.
Shapes are (D, H, W)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
from scipy import ndimage

import unet_studio_amd as U
from unet_studio_amd import morph as MO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONNECTIVITIES = (6, 18, 26)


# ---- the restatements ------------------------------------------------------------------------------------------------------------
def offsets(c):
    """the (dz, dy, dx) of a neighbourhood: 1 <= |dx| + |dy| + |dz| <= 1, 2, 3 for 6, 18, 26"""
    reach = {6: 1, 18: 2, 26: 3}[c]
    return [(dz, dy, dx) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if 1 <= abs(dz) + abs(dy) + abs(dx) <= reach]


def step_ref(m, op, c, border=0):
    """one step on a boolean (D, H, W) array: pad with the outside value, OR (dilate) / AND (erode) the shifted copies"""
    m = np.asarray(m, bool)
    D, H, W = m.shape
    p = np.pad(m, 1, constant_values=bool(border) if op == "erode" else False)
    out = m.copy()
    for dz, dy, dx in offsets(c):
        nb = p[1 + dz:1 + dz + D, 1 + dy:1 + dy + H, 1 + dx:1 + dx + W]
        out = out & nb if op == "erode" else out | nb
    return out


def steps_ref(m, op, c, n, border=0):
    m = np.asarray(m, bool).copy()
    for _ in range(n):
        m = step_ref(m, op, c, border)
    return m


def open_ref(m, c, n):
    return steps_ref(steps_ref(m, "erode", c, n, 1), "dilate", c, n)


def close_ref(m, c, n):
    return steps_ref(steps_ref(m, "dilate", c, n), "erode", c, n, 1)


def holes_ref(m):
    """(the voxels of the holes, their number): the 6-connected components of the complement minus those on a face"""
    m = np.asarray(m, bool)
    lab, n = ndimage.label(~m)
    face = np.zeros(n + 1, bool)
    for axis in range(3):
        for side in (0, -1):
            face[np.unique(np.take(lab, side, axis=axis))] = True
    face[0] = True                                                 # the mask itself is no hole
    return ~face[lab], int(n + 1 - face.sum())


def pack_ref(m):
    """uint64 (D, H, ceil(W / 64)): voxel x of a line is bit (x & 63) of word (x >> 6); the bits at and above W are zero"""
    m = np.asarray(m, bool)
    D, H, W = m.shape
    wpl = (W + 63) // 64
    p = np.zeros((D, H, wpl * 64), np.uint64)
    p[:, :, :W] = m
    return np.bitwise_or.reduce(p.reshape(D, H, wpl, 64) << np.arange(64, dtype=np.uint64), axis=3)


def unpack_ref(words, W):
    words = np.asarray(words).view(np.uint64)
    D, H, wpl = words.shape
    bits = (words[..., None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)
    return bits.reshape(D, H, wpl * 64)[:, :, :W].astype(bool)


# ---- the maps, shared with the GPU tests: (D, H, W) -> bool ------------------------------------------------------------------------
def box_bounds(shape):
    """per axis the first and last index of the shell: one voxel inside the grid where the axis has room for a cavity and a margin"""
    return [(1, n - 2) if n >= 5 else (0, n - 1) for n in shape]


def hollow_box(shape, opening=None):
    """a shell one voxel thick; opening: "face", "edge" or "corner" removes that one voxel of the shell"""
    b = box_bounds(shape)
    m = np.zeros(shape, bool)
    m[b[0][0]:b[0][1] + 1, b[1][0]:b[1][1] + 1, b[2][0]:b[2][1] + 1] = True
    if all(hi - lo >= 2 for lo, hi in b):
        m[b[0][0] + 1:b[0][1], b[1][0] + 1:b[1][1], b[2][0] + 1:b[2][1]] = False
    mid = [(lo + hi) // 2 for lo, hi in b]
    if opening == "face":
        m[b[0][0], mid[1], mid[2]] = False
    elif opening == "edge":
        m[b[0][0], b[1][0], mid[2]] = False
    elif opening == "corner":
        m[b[0][0], b[1][0], b[2][0]] = False
    return m


def corners(shape):
    m = np.zeros(shape, bool)
    m[np.ix_(*[[0, n - 1] for n in shape])] = True
    return m


def checkerboard(shape):
    z, y, x = np.indices(shape)
    return (x + y + z) % 2 == 0


def random_map(shape, density):
    return np.random.default_rng(int(density * 100) + shape[2]).random(shape) < density


MAPS = {
    "empty": lambda s: np.zeros(s, bool),
    "full": lambda s: np.ones(s, bool),
    "corners": corners,
    "checkerboard": checkerboard,
    "random20": lambda s: random_map(s, 0.2),
    "random50": lambda s: random_map(s, 0.5),
    "random70": lambda s: random_map(s, 0.7),
    "random85": lambda s: random_map(s, 0.85),
    "box": hollow_box,
    "box_face": lambda s: hollow_box(s, "face"),
    "box_edge": lambda s: hollow_box(s, "edge"),
    "box_corner": lambda s: hollow_box(s, "corner"),
}
SHAPES = [(1, 1, 1), (3, 5, 7), (4, 3, 63), (5, 4, 64), (2, 3, 65), (3, 2, 129), (9, 9, 33), (38, 44, 40), (2, 3, 70000)]
HOST_SHAPES = [(1, 1, 1), (3, 5, 7), (2, 3, 65), (9, 9, 33), (12, 20, 40)]


# ---- the restatements against scipy --------------------------------------------------------------------------------------------------
def test_the_neighbourhoods_are_scipys_structures():
    for k, c in ((1, 6), (2, 18), (3, 26)):
        s = ndimage.generate_binary_structure(3, k)
        want = {(z - 1, y - 1, x - 1) for z, y, x in zip(*np.nonzero(s))} - {(0, 0, 0)}
        assert set(offsets(c)) == want and len(offsets(c)) == c


@pytest.mark.parametrize("shape", HOST_SHAPES)
@pytest.mark.parametrize("k,c", [(1, 6), (2, 18), (3, 26)])
def test_step_ref_against_scipy(shape, k, c):
    s = ndimage.generate_binary_structure(3, k)
    for name in ("corners", "checkerboard", "random20", "random50", "random85", "box", "full", "empty"):
        m = MAPS[name](shape)
        for n in (1, 2, 3):
            assert (steps_ref(m, "dilate", c, n) == ndimage.binary_dilation(m, s, iterations=n)).all(), (name, n)
            for b in (0, 1):
                assert (steps_ref(m, "erode", c, n, b) == ndimage.binary_erosion(m, s, iterations=n, border_value=b)).all(), (name, n, b)
        assert (steps_ref(m, "dilate", c, 0) == m).all()


@pytest.mark.parametrize("shape", HOST_SHAPES + [(38, 44, 40)])
def test_holes_ref_against_scipy(shape):
    for name, f in MAPS.items():
        m = f(shape)
        holes, n = holes_ref(m)
        assert not (holes & m).any() and ((m | holes) == ndimage.binary_fill_holes(m)).all(), name
        assert n == ndimage.label(holes)[1], name


def test_holes_of_the_boxes_and_of_the_dense_random_maps():
    # the closed 5 x 5 x 50 box with its 3 x 3 x 48 cavity
    m = np.ones((5, 5, 50), bool)
    m[1:4, 1:4, 1:49] = False
    assert holes_ref(m)[0].sum() == 432 and holes_ref(m)[1] == 1
    for shape in ((9, 9, 33), (12, 20, 40), (38, 44, 40)):
        cavity = int(np.prod([n - 4 for n in shape]))
        assert holes_ref(hollow_box(shape))[0].sum() == cavity and holes_ref(hollow_box(shape))[1] == 1
        assert holes_ref(hollow_box(shape, "face"))[0].sum() == 0                  # the cavity leaks through the face: not filled
        for opening in ("edge", "corner"):                                           # no 6-connected path out: filled, and the
            holes, n = holes_ref(hollow_box(shape, opening))                        # removed voxel is outside, not a hole
            assert holes.sum() == cavity and n == 1
        for d in (0.7, 0.85):
            assert holes_ref(random_map(shape, d))[0].sum() > 0                      # a test of nothing cannot pass


# ---- properties ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", HOST_SHAPES)
def test_close_never_removes_and_open_never_adds_with_border_1(shape):
    for name, f in MAPS.items():
        m = f(shape)
        for c in CONNECTIVITIES:
            for n in (1, 2):
                assert (close_ref(m, c, n) | m).sum() == close_ref(m, c, n).sum(), (name, c, n)
                assert (open_ref(m, c, n) & m).sum() == open_ref(m, c, n).sum(), (name, c, n)
    # with border 0 the closing of a full volume would lose its faces
    full = np.ones(shape, bool)
    assert close_ref(full, 26, 1).all() and (steps_ref(full, "erode", 26, 1, 0).sum() == np.prod([max(n - 2, 0) for n in shape]))


@pytest.mark.parametrize("shape", SHAPES)
def test_pack_round_trip_and_the_bits_above_w_are_zero(shape):
    D, H, W = shape
    for name in ("full", "random50", "corners"):
        m = MAPS[name](shape)
        words = pack_ref(m)
        assert words.dtype == np.uint64 and words.shape == (D, H, (W + 63) // 64)
        assert (unpack_ref(words, W) == m).all()
        if W % 64:
            assert not (words[:, :, -1] >> np.uint64(W % 64)).any()
        assert int(np.unpackbits(words.view(np.uint8)).sum()) == int(m.sum())                  # the population count
    one = np.zeros((1, 1, 130), bool)
    one[0, 0, [0, 63, 64, 129]] = True
    assert pack_ref(one).reshape(-1).tolist() == [1 | 1 << 63, 1, 2]


# ---- the ABI -------------------------------------------------------------------------------------------------------------------------
FORBIDDEN = ("unet_inst_", "unet_dist_", "unet_table_", "unet_reg_", "unet_atlas_", "unet_components_", "unet_preproc_", "unet_tiles_",
             "unet_space_", "unet_postproc_", "unet_qc_", "unet_feed_")


def test_unet_morph_h_declares_exactly_the_exports_and_the_library_has_them():
    lib = ctypes.CDLL(U.engine.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "unet_morph.h")).read()
    declared = set(re.findall(r"\b(unet_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(MO.EXPORTS) == {"unet_morph_scratch_bytes", "unet_morph_pack", "unet_morph_unpack", "unet_morph_count",
                                           "unet_morph_step", "unet_morph_holes", "unet_morph_apply"}
    for name in sorted(declared):
        assert hasattr(lib, name), "libunet_hip.so does not export " + name
    enums = {k: int(v) for k, v in re.findall(r"UNET_MORPH_([A-Z_]+) = (\d+)", hdr)}
    assert enums == {"IMPL_DEFAULT": MO.IMPL_DEFAULT, "IMPL_LDS": MO.IMPL_LDS, "IMPL_GLOBAL": MO.IMPL_GLOBAL, "DILATE": MO.DILATE,
                     "ERODE": MO.ERODE, "SET": MO.SET, "KEEP": MO.KEEP}
    assert (MO.IMPL_DEFAULT, MO.IMPL_LDS, MO.IMPL_GLOBAL) == (0, 1, 2) and (MO.DILATE, MO.ERODE) == (0, 1) and (MO.SET, MO.KEEP) == (0, 1)
    defines = {k: int(v) for k, v in re.findall(r"#define UNET_MORPH_([A-Z_]+) (\d+)", hdr)}
    assert defines == {"FUSE_MAX": MO.FUSE_MAX, "BRICK_XW": MO.BRICK_XW, "BRICK_Y": MO.BRICK_Y, "BRICK_Z": MO.BRICK_Z,
                       "MAX_ITERATIONS": MO.MAX_ITERATIONS}
    assert MO.MAX_ITERATIONS == 255 and 1 <= MO.FUSE_MAX < 64
    # the two LDS copies of a brick with its halo
    assert 2 * 8 * (MO.BRICK_XW + 2) * (MO.BRICK_Y + 2 * MO.FUSE_MAX) * (MO.BRICK_Z + 2 * MO.FUSE_MAX) <= 64 * 1024
    assert "this project's" in hdr and "NOT pinned" in hdr
    assert U.morph is MO


def test_the_new_prefix_stays_in_its_header():
    for h in sorted(os.listdir(os.path.join(ROOT, "include"))):
        text = open(os.path.join(ROOT, "include", h)).read().lower()
        if h != "unet_morph.h":
            assert "unet_morph_" not in text, h
        else:                                                      # what the other host tests forbid
            for other in FORBIDDEN:
                assert other not in text, other


# ---- argument errors, before any device call -------------------------------------------------------------------------------------
P = [ctypes.c_void_p(0x1000 * (i + 1)) for i in range(8)]          # never dereferenced
ODD = ctypes.c_void_p(0x7004)                                      # 4-byte aligned only
BIG = 1 << 40
GRID_ERRORS = (((0, 4, 4), "dimensions (w, h, d) must be positive"), ((4, -1, 4), "dimensions"), ((4, 4, 0), "dimensions"),
               ((2048, 1024, 1024), "voxels must be in [1, 2^31), got 2147483648"))


def test_scratch_bytes_grow_and_check_their_arguments():
    sizes = [MO.morph_scratch_bytes(s) for s in ((1, 1, 1), (1, 1, 64), (1, 1, 65), (16, 16, 16), (100, 100, 100), (256, 256, 256),
                                                 (1, 1, (1 << 31) - 1))]
    assert all(a <= b for a, b in zip(sizes, sizes[1:]))
    S = 256 ** 3
    assert sizes[5] >= S // 8 + 2 * S + U.components.components_scratch_bytes(S, 2)    # a mask, the background map, the labelling
    for dims, msg in GRID_ERRORS:
        with pytest.raises(U.UNetError, match=re.escape(msg)):
            MO.morph_scratch_bytes(dims[::-1])
    lib = U.engine.lib
    assert lib.unet_morph_scratch_bytes(4, 4, 4, None) != 0 and "null bytes" in lib.unet_last_error().decode()


def failing(f, *args):
    assert f(*args) != 0
    return U.engine.lib.unet_last_error().decode()


def test_pack_argument_errors_need_no_device():
    lib = U.engine.lib
    small = MO.morph_scratch_bytes((4, 4, 4))

    def call(dims=(4, 4, 4), labels=P[0], lb=2, nc=3, listed=(1, 2), n_listed=None, bits=P[1], scratch=P[2], scratch_bytes=BIG):
        arr = (ctypes.c_uint32 * max(1, len(listed)))(*listed) if listed is not None else None
        return failing(lib.unet_morph_pack, *dims, labels, lb, nc, arr, len(listed) if n_listed is None else n_listed, bits, scratch,
                       scratch_bytes, None)

    for dims, msg in GRID_ERRORS:
        assert msg in call(dims=dims)
    assert "null labels" in call(labels=None)
    assert "label_bytes must be 1 or 2, got 4" in call(lb=4) and "label_bytes" in call(lb=0)
    assert "n_classes must be in [1, 65536], got 0" in call(nc=0) and "n_classes must be in [1, 65536], got 65537" in call(nc=65537)
    assert "n_listed must not be negative, got -1" in call(n_listed=-1) and "null listed" in call(listed=None, n_listed=2)
    assert "null bits" in call(bits=None) and "bits must be 8-byte aligned" in call(bits=ODD)
    assert "null scratch" in call(scratch=None)
    assert "scratch too small" in call(scratch_bytes=small - 1) and "scratch too small" in call(dims=(40, 40, 40), scratch_bytes=small)
    assert "listed class 0 is not in [1, 2]" in call(listed=(1, 0)) and "listed class 3 is not in [1, 2]" in call(listed=(3,))
    assert "listed class 1 is not in [1, 0]" in call(nc=1, listed=(1,))


def test_unpack_and_count_argument_errors_need_no_device():
    lib = U.engine.lib
    for dims, msg in GRID_ERRORS:
        assert msg in failing(lib.unet_morph_unpack, *dims, P[0], P[1], None)
        assert msg in failing(lib.unet_morph_count, *dims, P[0], P[1], None)
    assert "null bits" in failing(lib.unet_morph_unpack, 4, 4, 4, None, P[1], None)
    assert "bits must be 8-byte aligned" in failing(lib.unet_morph_unpack, 4, 4, 4, ODD, P[1], None)
    assert "null mask" in failing(lib.unet_morph_unpack, 4, 4, 4, P[0], None, None)
    assert "null bits" in failing(lib.unet_morph_count, 4, 4, 4, None, P[1], None)
    assert "bits must be 8-byte aligned" in failing(lib.unet_morph_count, 4, 4, 4, ODD, P[1], None)
    assert "null count" in failing(lib.unet_morph_count, 4, 4, 4, P[0], None, None)
    assert "count must be 8-byte aligned" in failing(lib.unet_morph_count, 4, 4, 4, P[0], ODD, None)


def test_step_argument_errors_need_no_device():
    lib = U.engine.lib
    small = MO.morph_scratch_bytes((4, 4, 4))

    def call(dims=(4, 4, 4), src=P[0], dst=P[1], op=MO.DILATE, c=6, n=1, border=0, impl=0, scratch=P[2], scratch_bytes=BIG):
        return failing(lib.unet_morph_step, *dims, src, dst, op, c, n, border, impl, scratch, scratch_bytes, None)

    for dims, msg in GRID_ERRORS:
        assert msg in call(dims=dims)
    assert "null in" in call(src=None) and "in must be 8-byte aligned" in call(src=ODD)
    assert "null out" in call(dst=None) and "out must be 8-byte aligned" in call(dst=ODD)
    assert "in and out must not be the same mask" in call(dst=P[0])
    assert "unknown op 2" in call(op=2) and "unknown op -1" in call(op=-1)
    for c in (7, 0, 8, 27, -6):
        assert "connectivity must be 6, 18 or 26, got %d" % c in call(c=c)
    assert "iterations must be in [0, 255], got 256" in call(n=256) and "iterations must be in [0, 255], got -1" in call(n=-1)
    assert "border must be 0 or 1, got 2" in call(border=2)
    assert "unknown impl 3" in call(impl=3) and "unknown impl -1" in call(impl=-1)
    assert "null scratch" in call(scratch=None)
    assert "scratch too small" in call(scratch_bytes=small - 1) and "scratch too small" in call(dims=(40, 40, 40), scratch_bytes=small)


def test_holes_argument_errors_need_no_device():
    lib = U.engine.lib
    small = MO.morph_scratch_bytes((4, 4, 4))

    def call(dims=(4, 4, 4), src=P[0], dst=P[1], info=P[2], impl=0, scratch=P[3], scratch_bytes=BIG):
        return failing(lib.unet_morph_holes, *dims, src, dst, info, impl, scratch, scratch_bytes, None)

    for dims, msg in GRID_ERRORS:
        assert msg in call(dims=dims)
    assert "null in" in call(src=None) and "in must be 8-byte aligned" in call(src=ODD)
    assert "null out" in call(dst=None) and "out must be 8-byte aligned" in call(dst=ODD)
    assert "info must be 8-byte aligned" in call(info=ODD)
    assert "unknown impl 3" in call(impl=3) and "unknown impl -1" in call(impl=-1)
    assert "null scratch" in call(scratch=None) and "null scratch" in call(info=None, scratch=None)    # info is optional
    assert "scratch too small" in call(scratch_bytes=small - 1) and "scratch too small" in call(dims=(40, 40, 40), scratch_bytes=small)


def test_apply_argument_errors_need_no_device():
    lib = U.engine.lib

    def call(dims=(4, 4, 4), labels=P[0], bits=P[1], value=1, mode=MO.SET, changed=P[2]):
        return failing(lib.unet_morph_apply, *dims, labels, bits, value, mode, changed, None)

    for dims, msg in GRID_ERRORS:
        assert msg in call(dims=dims)
    assert "null labels" in call(labels=None) and "labels must be 2-byte aligned" in call(labels=ctypes.c_void_p(0x1001))
    assert "null bits" in call(bits=None) and "bits must be 8-byte aligned" in call(bits=ODD)
    assert "value must be in [1, 65535], got 0" in call(value=0) and "value must be in [1, 65535], got 65536" in call(value=65536)
    assert "unknown mode 2" in call(mode=2) and "unknown mode -1" in call(mode=-1)
    assert "changed must be 8-byte aligned" in call(changed=ODD)
    assert "unknown mode 2" in call(mode=2, changed=None)                                              # changed is optional


def test_wrapper_errors_need_no_device():
    t16 = torch.zeros((2, 2, 2), dtype=torch.uint16)
    with pytest.raises(U.UNetError, match="device tensor"):
        MO.pack(t16, 3)
    with pytest.raises(U.UNetError, match="device tensor"):
        MO.Mask(torch.zeros((2, 2, 1), dtype=torch.int64), (2, 2, 2))
    for f in (MO.unpack, MO.count, MO.dilate, MO.erode, MO.fill_holes):
        with pytest.raises(U.UNetError, match="must be a morph.Mask"):
            f(t16)
    with pytest.raises(U.UNetError, match="device tensor"):
        MO.dilate_label(t16, 1)
    with pytest.raises(U.UNetError, match="device tensor"):
        MO.fill_holes_label(t16, [1], 1, 3)


BAD_OPS = [
    ("smooth", 1, 6, 1),
    ("dilate", 1, 6),
    ("dilate", 0, 6, 1),
    ("dilate", 3, 6, 1),
    ("erode", 1, 7, 1),
    ("open", 1, 6, 256),
    ("close", 1, 6, -1),
    ("close", 1.0, 6, 1),
    ("fill_holes", [1, 3], 1),
    ("fill_holes", [1], 0),
    ("fill_holes", 1, 1),
    ("fill_holes", [1]),
    "dilate",
    (),
]


@pytest.mark.parametrize("bad", BAD_OPS, ids=[repr(b) for b in BAD_OPS])
def test_run_refuses_a_bad_op_naming_it_before_any_device_work(bad):
    good = ("close", 1, 26, 1)
    labels = torch.zeros((2, 2, 2), dtype=torch.uint16)            # a host tensor: the ops are refused before it is looked at
    with pytest.raises(U.UNetError, match=re.escape("op 1 %r" % (bad,))):
        MO.run(labels, [good, bad], 3)
    with pytest.raises(U.UNetError, match="morphology: op 0"):
        MO.check_ops([bad], 3)


def test_check_ops_accepts_and_normalises():
    ops = MO.check_ops([["dilate", 2, 18, 0], ("fill_holes", (1, 2), 1)], 3)
    assert ops == [("dilate", 2, 18, 0), ("fill_holes", [1, 2], 1)]
    assert MO.check_ops([], 3) == []
    for nc in (1, 65537):
        with pytest.raises(U.UNetError, match="n_classes"):
            MO.check_ops([], nc)
    with pytest.raises(U.UNetError, match="list of tuples"):
        MO.check_ops("dilate", 3)
    with pytest.raises(U.UNetError, match="device tensor"):        # good ops: now the label map is looked at
        MO.run(torch.zeros((2, 2, 2), dtype=torch.uint16), [("dilate", 1, 6, 1)], 3)
