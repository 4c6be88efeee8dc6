"""CPU: the host half of a model's single_component_label (include/unet_components.h, unet-studio_amd/components.py) -- the ABI the
library exports, `resolve` known answers (with a list that came from a `.nz` file), argument errors found before any device call,
the scratch size, this file's own restatement of the definition checked on hand-written answers, and a sequential transcription of
the tile and border phases of the TILED kernels checked against that restatement.  No device calls."""
import ctypes
import gzip
import os
import re
import threading

import numpy as np
import pytest
import torch
from scipy import ndimage

import unet_studio_amd as U
from unet_studio_amd import components as CMP
from unet_studio_amd import nz

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARCH = ("conv8,ks3,stride1+norm,leaky_relu\nconv16,ks3,stride2+norm,leaky_relu+conv_trans8,ks2,stride2\n"
        "conv8,ks3,stride1+norm,leaky_relu+conv5,ks1,stride1")
FACES = ndimage.generate_binary_structure(3, 1)      # 6-connectivity


# ---- the restatement (never imports the package's kernels) ---------------------------------------------------------------------------
def keep_largest_ref(label, classes, n_classes):
    """label: (D, H, W) integer array, x fastest.  Returns (result uint16, removed uint32[n_classes]): per listed class
    scipy.ndimage.label with face connectivity, the largest count kept, among equal counts the component holding the smallest
    linear index, every other voxel of the class 0.  Unlisted values (0 and values >= n_classes among them) are never touched."""
    label = np.asarray(label)
    out = label.astype(np.uint16).copy()
    removed = np.zeros(n_classes, np.uint32)
    for v in sorted(set(int(c) for c in classes)):
        assert 0 < v < n_classes
        comp, n = ndimage.label(label == v, structure=FACES)
        if n == 0:
            continue
        flat = comp.reshape(-1)
        counts = np.bincount(flat, minlength=n + 1)[1:]
        idx = np.flatnonzero(flat)                                # ascending: a component's first occurrence is its smallest index
        ids, at = np.unique(flat[idx], return_index=True)
        first = idx[at]
        assert np.array_equal(ids, np.arange(1, n + 1))
        best = 1 + int(np.lexsort((first, -counts.astype(np.int64)))[0])     # the largest count, then the smallest first index
        gone = (comp != 0) & (comp != best)
        out[gone] = 0
        removed[v] = int(gone.sum())
    return out, removed


def test_restatement_two_equal_blobs_the_lower_index_survives():
    a = np.zeros((3, 4, 9), np.uint16)
    a[1, 1:3, 1:3] = 2                                            # 4 voxels, first linear index 1*36 + 1*9 + 1 = 46
    a[1, 1:3, 5:7] = 2                                            # 4 voxels, first linear index 50
    a[2, 3, 8] = 2                                                # a single voxel
    out, removed = keep_largest_ref(a, [2], 3)
    want = np.zeros_like(a)
    want[1, 1:3, 1:3] = 2
    assert np.array_equal(out, want) and removed.tolist() == [0, 0, 5]
    # the larger one wins wherever it lies
    a[0, 0, 8] = a[0, 1, 8] = a[0, 2, 8] = a[0, 3, 8] = a[1, 3, 8] = 2      # joins the single voxel: 6 voxels through (2, 3, 8)
    out, removed = keep_largest_ref(a, [2], 3)
    want = np.zeros_like(a)
    want[0, :, 8] = want[1, 3, 8] = want[2, 3, 8] = 2
    assert np.array_equal(out, want) and removed.tolist() == [0, 0, 8]


def test_restatement_diagonal_contact_is_no_contact():
    a = np.zeros((2, 3, 3), np.uint16)
    a[0, 0, 0] = a[0, 1, 1] = a[1, 2, 2] = 1                      # edge and corner neighbours only
    a[0, 2, 2] = 1                                                # a face neighbour of (1, 2, 2): one piece of two
    out, removed = keep_largest_ref(a, [1], 2)
    want = np.zeros_like(a)
    want[0, 2, 2] = want[1, 2, 2] = 1
    assert np.array_equal(out, want) and removed.tolist() == [0, 2]


def test_restatement_checkerboard_keeps_voxel_0_and_voxel_1():
    z, y, x = np.indices((4, 5, 6))
    a = (1 + (x + y + z) % 2).astype(np.uint16)                   # every component is one voxel
    out, removed = keep_largest_ref(a, [1, 2], 3)
    want = np.zeros_like(a)
    want[0, 0, 0], want[0, 0, 1] = 1, 2
    assert np.array_equal(out, want) and removed.tolist() == [0, 59, 59]
    # unlisted values, 0 and values >= n_classes are never touched; a listed class that does not occur changes nothing
    a[3, 4, 5] = 7
    out, removed = keep_largest_ref(a, [2, 4], 5)
    assert np.array_equal(out == 1, a == 1) and out[3, 4, 5] == 7 and removed.tolist() == [0, 0, 59, 0, 0]


# ---- a sequential transcription of k_cmp_tile and k_cmp_border ---------------------------------------------------------------------
def tiled_roots(label, listed, n_classes):
    """parent (root per member, -1 elsewhere) and count per root as the TILED kernels build them, one voxel at a time: the tile
    phase over local indices, the local root written as a global index with the piece count, the border phase over the voxels on a
    low face of a tile, the flatten that moves the piece counts to the global roots.  Asserts parent[j] <= j throughout."""
    TX, TY, TZ = CMP.TILE
    D, H, W = label.shape
    flat = label.reshape(-1)
    member = np.isin(flat, sorted(listed)) & (flat < n_classes)
    parent = np.full(flat.size, -2, np.int64)
    count = np.full(flat.size, -2, np.int64)

    def find(p, i):
        while p[i] != i:
            assert 0 <= p[i] < i
            i = p[i]
        return i

    def union(p, a, b):
        ra, rb = find(p, a), find(p, b)
        if ra != rb:
            p[max(ra, rb)] = min(ra, rb)

    for z0 in range(0, D, TZ):
        for y0 in range(0, H, TY):
            for x0 in range(0, W, TX):
                val = np.zeros(TX * TY * TZ, np.int64)
                for l in range(val.size):
                    x, y, z = x0 + l % TX, y0 + (l // TX) % TY, z0 + l // (TX * TY)
                    if x < W and y < H and z < D and member[(z * H + y) * W + x]:
                        val[l] = flat[(z * H + y) * W + x]
                lpar = np.where(val > 0, np.arange(val.size), -1)
                for l in np.flatnonzero(val):
                    lx, ly, lz = l % TX, (l // TX) % TY, l // (TX * TY)
                    if lx > 0 and val[l - 1] == val[l]:
                        union(lpar, l, l - 1)
                    if ly > 0 and val[l - TX] == val[l]:
                        union(lpar, l, l - TX)
                    if lz > 0 and val[l - TX * TY] == val[l]:
                        union(lpar, l, l - TX * TY)
                lcnt = np.zeros(val.size, np.int64)
                roots = np.full(val.size, -1, np.int64)
                for l in np.flatnonzero(val):
                    roots[l] = find(lpar, l)
                    lcnt[roots[l]] += 1
                for l in range(val.size):
                    x, y, z = x0 + l % TX, y0 + (l // TX) % TY, z0 + l // (TX * TY)
                    if x < W and y < H and z < D:
                        g, r = (z * H + y) * W + x, roots[l]
                        assert parent[g] == -2                            # every voxel is written by exactly one tile
                        parent[g] = -1 if r < 0 else ((z0 + r // (TX * TY)) * H + y0 + (r // TX) % TY) * W + x0 + r % TX
                        count[g] = lcnt[l]
                        assert parent[g] <= g
    assert (parent > -2).all() and ((parent >= 0) == member).all()
    nfx, nfy, nfz = (W + TX - 1) // TX - 1, (H + TY - 1) // TY - 1, (D + TZ - 1) // TZ - 1
    A, B = nfx * H * D, W * nfy * D
    seen = set()
    for idx in range(A + B + W * H * nfz):
        if idx < A:
            j = idx
            x, j = (j % nfx + 1) * TX, j // nfx
            y, z, back = j % H, j // H, 1
        elif idx < A + B:
            j = idx - A
            x, j = j % W, j // W
            y, z, back = (j % nfy + 1) * TY, j // nfy, W
        else:
            j = idx - A - B
            x, j = j % W, j // W
            y, z, back = j % H, (j // H + 1) * TZ, W * H
        assert 0 <= x < W and 0 <= y < H and 0 <= z < D
        i = (z * H + y) * W + x
        seen.add((i, back))
        if parent[i] >= 0 and parent[i - back] >= 0 and flat[i] == flat[i - back]:
            union(parent, i, i - back)
    # exactly the pairs that straddle a tile face, each once
    want = set()
    for z in range(D):
        for y in range(H):
            for x in range(W):
                i = (z * H + y) * W + x
                if x and x % TX == 0:
                    want.add((i, 1))
                if y and y % TY == 0:
                    want.add((i, W))
                if z and z % TZ == 0:
                    want.add((i, W * H))
    assert seen == want and len(seen) == A + B + W * H * nfz
    total = count.copy()
    root = np.full(flat.size, -1, np.int64)
    for i in np.flatnonzero(parent >= 0):
        root[i] = find(parent, i)
        if root[i] != i and count[i]:
            total[root[i]] += count[i]
    return root, total


@pytest.mark.parametrize("shape", [(1, 1, 1), (9, 9, 33), (17, 1, 3), (3, 17, 31), (7, 12, 40)])
def test_the_tile_and_border_phases_transcribed_give_the_components_of_the_restatement(shape):
    rng = np.random.default_rng(sum(shape))
    for density, listed in ((0.0, [1, 2, 3]), (0.5, [1, 3]), (0.8, [2])):
        a = rng.integers(1, 4, shape).astype(np.uint16)
        a[rng.random(shape) < 0.1] = 9                              # a value >= n_classes
        if density:
            blob = ndimage.binary_dilation(rng.random(shape) < 0.02, iterations=2)
            a[blob & (rng.random(shape) < density)] = listed[0]
        root, total = tiled_roots(a, listed, 4)
        flat = a.reshape(-1)
        for v in (1, 2, 3):
            comp, n = ndimage.label(a == v, structure=FACES)
            comp = comp.reshape(-1)
            if v not in listed:
                assert (root[flat == v] == -1).all()
                continue
            for k in range(1, n + 1):
                idx = np.flatnonzero(comp == k)
                assert (root[idx] == idx[0]).all() and total[idx[0]] == idx.size     # the smallest linear index; the voxel count
        assert (root[flat == 9] == -1).all()


# ---- the ABI ---------------------------------------------------------------------------------------------------------------------
def test_unet_components_h_declares_exactly_the_exports_and_the_library_has_them():
    lib = ctypes.CDLL(U.engine.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "unet_components.h")).read()
    declared = set(re.findall(r"\b(unet_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(CMP.EXPORTS) == {"unet_components_scratch_bytes", "unet_components_keep_largest"}
    for name in sorted(declared):
        assert hasattr(lib, name), "libunet_hip.so does not export " + name
    enums = {k: int(v) for k, v in re.findall(r"UNET_COMPONENTS_(IMPL_[A-Z]+) = (\d+)", hdr)}
    assert enums == {"IMPL_DEFAULT": CMP.IMPL_DEFAULT, "IMPL_TILED": CMP.IMPL_TILED, "IMPL_GLOBAL": CMP.IMPL_GLOBAL}
    assert (CMP.IMPL_DEFAULT, CMP.IMPL_TILED, CMP.IMPL_GLOBAL) == (0, 1, 2)
    tile = {k: int(v) for k, v in re.findall(r"#define UNET_COMPONENTS_TILE_([XYZ]) (\d+)", hdr)}
    assert (tile["X"], tile["Y"], tile["Z"]) == CMP.TILE
    assert U.components is CMP


def test_the_other_headers_do_not_mention_the_new_prefix():
    for h in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if h != "unet_components.h":
            assert "unet_components_" not in open(os.path.join(ROOT, "include", h)).read().lower(), h


# ---- resolve ---------------------------------------------------------------------------------------------------------------------
class HostModel:
    """the fields and calls load_from_file / save_to_file touch (unet.hpp:16-40), with CPU tensors in parameters() order"""

    def __init__(self, in_count, out_count, architecture):
        self.in_count, self.out_count, self.architecture = in_count, out_count, architecture
        plan = U.Plan(architecture, in_count, out_count, (32, 32, 32))
        g = torch.Generator().manual_seed(1)
        self._p = [torch.randn(s, generator=g) for s in plan.param_shapes]
        self.fov_strategy, self.preproc, self.postproc, self.orientation, self.error_msg = "align_top", "", "softmax+create_mask+argmax", "", ""
        self.voxel_size, self.dim = (1.0, 1.0, 1.0), (32, 32, 32)
        self.testing_errors, self.training_errors, self.single_component_label = [], [], []
        self.error_mutex, self.training = threading.Lock(), False

    def parameters(self):
        return self._p

    def train(self):
        self.training = True

    def load_parameters(self, arrays):
        self._p = [torch.from_numpy(np.array(a, np.float32)).reshape(p.shape) for a, p in zip(arrays, self._p)]


def test_resolve_known_answers_with_a_list_from_a_model_file(tmp_path):
    f = str(tmp_path / "net.nz")
    assert nz.save_to_file(HostModel(1, 5, ARCH), f)
    assert nz.load_from_file(f, HostModel).single_component_label == []          # save_to_file does not write the record
    with gzip.open(f, "ab") as g:                                                 # a file that carries it
        nz.write_record(g, "single_component_label", np.array([3, 1, 3, 4], np.int32))
    m = nz.load_from_file(f, HostModel)
    assert m.out_count == 5 and m.single_component_label == [3, 1, 3, 4]
    assert CMP.resolve("model", m) == [1, 3, 4]
    assert CMP.resolve(None, m) == [] and CMP.resolve((), m) == [] and CMP.resolve([], m) == []
    assert CMP.resolve([4, 2, 2, 1], m) == [1, 2, 4] and CMP.resolve(np.array([2, 1], np.uint32), m) == [1, 2]
    assert CMP.resolve(iter([3]), m) == [3]
    m.single_component_label = []
    assert CMP.resolve("model", m) == []


def test_resolve_raises_on_0_and_on_out_count():
    m = HostModel(1, 5, ARCH)
    for bad in (0, 5, 6, -1, 70000):
        with pytest.raises(U.UNetError) as e:
            CMP.resolve([1, bad, 2], m)
        assert str(bad) in str(e.value)
    m.single_component_label = [2, 5]
    with pytest.raises(U.UNetError, match="class 5 is not in \\[1, 4\\]"):
        CMP.resolve("model", m)
    with pytest.raises(U.UNetError):
        CMP.resolve("all", m)
    with pytest.raises(U.UNetError):
        CMP.resolve([1.5], m)


# ---- argument errors, before any device call -------------------------------------------------------------------------------------
def test_scratch_bytes_grows_with_voxels_and_with_classes():
    sizes = [CMP.components_scratch_bytes(v, 130) for v in (1, 2, 63, 64, 65, 1000, 4096, 10 ** 6, 192 * 224 * 192, (1 << 31) - 1)]
    assert all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[0] < sizes[5] < sizes[-1]
    assert sizes[8] >= 8 * 192 * 224 * 192                                         # parent and count
    by_class = [CMP.components_scratch_bytes(1000, c) for c in (1, 2, 3, 130, 4096, 65535, 65536)]
    assert all(a <= b for a, b in zip(by_class, by_class[1:])) and by_class[0] < by_class[3] < by_class[-1]
    for v, c, msg in ((0, 3, "voxels"), (-1, 3, "voxels"), (1 << 31, 3, "voxels"), (10, 0, "n_classes"), (10, 65537, "n_classes")):
        with pytest.raises(U.UNetError, match=msg):
            CMP.components_scratch_bytes(v, c)
    rc = U.engine.lib.unet_components_scratch_bytes(10, 3, None)
    assert rc != 0 and "null output" in U.engine.lib.unet_last_error().decode()


def test_argument_errors_need_no_device():
    a, b, c = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x2000), ctypes.c_void_p(0x3000)      # never dereferenced
    lib = U.engine.lib
    big = 1 << 40

    def call(s=(4, 4, 4), label=a, n_classes=5, listed=(1, 2), n_listed=None, removed=c, impl=0, scratch=b, scratch_bytes=big):
        arr = (ctypes.c_uint32 * max(1, len(listed)))(*listed) if listed is not None else None
        rc = lib.unet_components_keep_largest(s[0], s[1], s[2], label, n_classes, arr, len(listed or ()) if n_listed is None else n_listed,
                                              removed, impl, scratch, scratch_bytes, None)
        assert rc != 0
        return lib.unet_last_error().decode()

    assert "dimensions must be positive" in call(s=(0, 4, 4))
    assert "dimensions must be positive" in call(s=(4, 4, -1))
    assert "2^31" in call(s=(2048, 1024, 1024))
    assert "n_classes" in call(n_classes=0)
    assert "n_classes" in call(n_classes=65537)
    assert "null label" in call(label=None)
    assert "null list" in call(listed=None, n_listed=2)
    assert "n_listed" in call(n_listed=-1)
    assert "unknown impl 3" in call(impl=3)
    assert "unknown impl -1" in call(impl=-1)
    assert "null scratch" in call(scratch=None)
    assert "scratch too small" in call(scratch_bytes=CMP.components_scratch_bytes(64, 5) - 1)
    assert "scratch too small" in call(listed=(), scratch_bytes=16)                 # the same checks with an empty list
    assert "listed class 0 " in call(listed=(1, 0))
    assert "listed class 5 " in call(listed=(5,))
    assert "listed class 65535 " in call(listed=(1, 65535), n_classes=65535)
    assert "listed class 4294967295 " in call(listed=(4294967295,))


def test_wrapper_errors_need_no_device():
    host = torch.zeros((4, 4, 4), dtype=torch.uint16)
    with pytest.raises(U.UNetError, match="device tensor"):
        CMP.keep_largest(host, [1], 3)
    with pytest.raises(U.UNetError, match="device tensor"):
        CMP.keep_largest(np.zeros((4, 4, 4), np.uint16), [1], 3)
