"""GPU: connected components with a chosen connectivity on the device (include/unet_connectivity.h) -- `label`, `keep_largest` and
`fill_holes` of connectivity.py with 6, 18 and 26 under IMPL_TILED, IMPL_GLOBAL (the second witness) and the default against the
scipy restatements of test_connectivity_host.py, into garbage-filled outputs between guard words; the two-voxel pair maps that cross
one, two and three tile boundaries across low and high faces; connectivity 6 against the older siblings byte for byte; then the keyword
through components, instances, morph, run_postproc and EvaluateUNet.  Every comparison is exact equality of bytes.  Shapes are
(D, H, W); the tile of the tiled labelling is 32 x 8 x 8 (x, y, z)."""
import ctypes
import itertools
import os
import sys

import numpy as np
import pytest
import torch

import unet_studio_amd as U
from unet_studio_amd import components as CMP
from unet_studio_amd import connectivity as CN
from unet_studio_amd import instances as IN
from unet_studio_amd import morph as MO
from unet_studio_amd import postproc as P

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_morph_host as TMH  # noqa: E402
from test_connectivity_host import (CONNS, LISTED, MAPS, NC, RANK, SHAPES, holes_ref, keep_largest_ref, label_ref, pair_cases,  # noqa: E402
                                    pair_map, shell)
from test_instances_host import match_ref, rows_ref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
IMPLS = (CN.IMPL_TILED, CN.IMPL_GLOBAL, CN.IMPL_DEFAULT)
LARGE = ((38, 44, 40), (2, 3, 70000))
G = 64                                                             # guard words on each side
GUARD = {torch.int32: -0x5A3C5A3D, torch.int64: -0x5A3C5A3C5A3C5A3D}
GARBAGE = {torch.int32: 0x7B7B7B7B, torch.int64: 0x7B7B7B7B7B7B7B7B}
F = np.float32
PRODUCT = list(itertools.product(MAPS, CONNS, IMPLS))
SPARSE = PRODUCT[::5]
HOLE_MAPS = ("random70", "random85", "box", "box_face", "box_edge", "box_corner", "empty", "full")
HOLE_PRODUCT = list(itertools.product(HOLE_MAPS, CONNS, IMPLS))
HOLE_SPARSE = HOLE_PRODUCT[::5]


def same(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()


def guarded(n, dtype):
    """a buffer of G + n + G words: guards outside, garbage inside; -> (buffer, the view a call writes)"""
    buf = torch.full((n + 2 * G,), GUARD[dtype], dtype=dtype, device=DEV)
    buf[G:G + n] = GARBAGE[dtype]
    return buf, buf[G:G + n]


def guards_intact(buf, n):
    b = buf.cpu().numpy()
    g = GUARD[buf.dtype]
    return bool((b[:G] == g).all() and (b[G + n:] == g).all())


def dev_labels(a):
    return torch.from_numpy(np.ascontiguousarray(a).astype(np.int32)).to(DEV).to(torch.uint16)


def host_u16(t):
    return t.cpu().view(torch.int16).numpy().view(np.uint16)


def dev_mask(m):
    return MO.Mask(torch.from_numpy(TMH.pack_ref(m).view(np.int64)).to(DEV), m.shape)


def same_mask(mask, want):
    return mask.bits.cpu().numpy().view(np.uint64).tobytes() == TMH.pack_ref(want).tobytes()


_CACHE = {}


def case(shape, name, c):
    """(labels, inst, N) of a map under a connectivity, computed once and shared; never changed"""
    key = (shape, name, c)
    if key not in _CACHE:
        if (shape, name) not in _CACHE:
            lab = MAPS[name](shape)
            lab.setflags(write=False)
            _CACHE[(shape, name)] = lab
        lab = _CACHE[(shape, name)]
        inst, n = label_ref(lab, LISTED, c, NC)
        inst.setflags(write=False)
        _CACHE[key] = (lab, inst, n)
    return _CACHE[key]


def cases_of(shape, product=PRODUCT, sparse=SPARSE):
    return sparse if shape in LARGE else product


def test_the_trimmed_products_hold_every_value_of_every_factor():
    for full, part in ((PRODUCT, SPARSE), (HOLE_PRODUCT, HOLE_SPARSE)):
        for k in range(3):
            assert {p[k] for p in part} == {p[k] for p in full}


# ---- label -----------------------------------------------------------------------------------------------------------------------------
def check_label(lab, want_inst, n, M, c, impl, lab_dev=None):
    S = lab.size
    lab_dev = dev_labels(lab) if lab_dev is None else lab_dev
    ibuf, inst = guarded(S, torch.int32)
    rbuf, rows = guarded((M + 1) * 12, torch.int64)
    fbuf, info = guarded(2, torch.int64)
    got = CN.label(lab_dev, NC, LISTED, c, max_instances=M, impl=impl, out=(inst, rows, info))
    assert got[0].data_ptr() == inst.data_ptr() and tuple(got[0].shape) == lab.shape and tuple(got[1].shape) == (M + 1, 12)
    assert info.cpu().numpy().tolist() == [n, min(n, M)], (c, impl, info.cpu().numpy())
    assert same(got[0].cpu().numpy(), want_inst), (c, impl)
    assert same(got[1].cpu().numpy(), rows_ref(want_inst, lab, M)), (c, impl)
    assert guards_intact(ibuf, S) and guards_intact(rbuf, (M + 1) * 12) and guards_intact(fbuf, 2)
    return got


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_label_is_the_restatement_under_every_impl_and_connectivity(shape):
    some = set()
    for name, c, impl in cases_of(shape):
        lab, want_inst, n = case(shape, name, c)
        lab_dev = dev_labels(lab)
        M = n + 2
        inst, rows, info = check_label(lab, want_inst, n, M, c, impl, lab_dev)
        assert same(host_u16(lab_dev), lab.astype(np.uint16))                    # the label map is left alone
        if c == 6:                                                               # the older sibling's bytes
            old = IN.label(lab_dev, NC, LISTED, max_instances=M, impl=impl)
            assert all(torch.equal(a, b) for a, b in zip(old, (inst, rows, info))), (name, impl)
        elif n != case(shape, name, 6)[2]:
            some.add(c)
    if min(shape) >= 2 and shape not in LARGE:
        assert some == {18, 26}                                                  # the connectivity matters on this shape


def test_label_with_fewer_rows_than_instances_and_the_lists():
    shape = (9, 9, 33)
    for c in CONNS:
        lab, want_inst, n = case(shape, "random30", c)
        assert n > 3
        for M in (0, 1, n - 1):
            for impl in IMPLS:
                check_label(lab, want_inst, n, M, c, impl)
    lab = case(shape, "random50", 26)[0]
    t = dev_labels(lab)
    inst, rows, info = CN.label(t, NC, None, 26, max_instances=2000)             # None lists 1..n_classes-1
    want, n = label_ref(lab, [1, 2, 3], 26, NC)
    assert same(inst.cpu().numpy(), want) and info.cpu().tolist() == [n, n] and same(rows.cpu().numpy(), rows_ref(want, lab, 2000))
    inst, rows, info = CN.label(t, NC, [], 26, max_instances=3)                  # an empty list: nothing is a member
    assert not inst.any() and info.cpu().tolist() == [0, 0] and same(rows.cpu().numpy(), rows_ref(np.zeros(shape, np.int32), lab, 3))
    inst8 = CN.label(t.to(torch.uint8), NC, LISTED, 18)[0]                       # uint8 is cast
    assert same(inst8.cpu().numpy(), case(shape, "random50", 18)[1])


def test_the_pair_maps_every_offset_across_one_two_and_three_tile_boundaries():
    """the direct test of the border enumeration: {p, p + o} for the 13 offsets of N-(26), the pair crossing every subset of the
    boundaries it can cross, the neighbour across a low face for a step down and a high face for a step up"""
    cases = pair_cases()
    assert len(cases) == 49
    for shape, p, o, crossed in cases:
        lab = pair_map(shape, p, o)
        lab_dev = dev_labels(lab)
        for c in CONNS:
            want_n = 1 if sum(abs(v) for v in o) <= RANK[c] else 2
            want_inst, n = label_ref(lab, [1], c)
            assert n == want_n
            for impl in (CN.IMPL_TILED, CN.IMPL_GLOBAL):
                inst, rows, info = CN.label(lab_dev, 2, [1], c, max_instances=2, impl=impl)
                assert info.cpu().tolist() == [n, n], (p, o, crossed, c, impl)
                assert same(inst.cpu().numpy(), want_inst), (p, o, crossed, c, impl)
                work = lab_dev.clone()
                CN.keep_largest(work, [1], 2, c, impl=impl)
                assert int(work.to(torch.int32).sum()) == (2 if n == 1 else 1), (p, o, crossed, c, impl)


# ---- keep_largest ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_keep_largest_is_the_restatement_under_every_impl_and_connectivity(shape):
    S = shape[0] * shape[1] * shape[2]
    scratch = torch.empty(CN.keep_largest_scratch_bytes(S, NC), dtype=torch.uint8, device=DEV)
    wants = {}
    for name, c, impl in cases_of(shape):
        lab = case(shape, name, c)[0]
        if (name, c) not in wants:
            wants[(name, c)] = keep_largest_ref(lab, LISTED, NC, c)
        want, want_removed = wants[(name, c)]
        work = dev_labels(lab)
        removed = torch.full((NC,), 0x7B7B7B7B, dtype=torch.int32, device=DEV)
        assert CN.keep_largest(work, LISTED, NC, c, removed=removed, scratch=scratch, impl=impl) is work
        assert same(host_u16(work), want), (name, c, impl)
        assert same(removed.cpu().numpy().view(np.uint32), want_removed), (name, c, impl)
        if c == 6:                                                               # the older sibling's bytes
            old, old_removed = dev_labels(lab), torch.full((NC,), -1, dtype=torch.int32, device=DEV)
            CMP.keep_largest(old, LISTED, NC, removed=old_removed, impl=impl)
            assert torch.equal(old.view(torch.int16), work.view(torch.int16)) and torch.equal(old_removed, removed), (name, impl)


def test_keep_largest_ties_go_to_the_smallest_index_and_an_empty_list_changes_nothing():
    shape = (12, 12, 40)
    lab = np.zeros(shape, np.int64)
    lab[3, 3, 30], lab[3, 4, 31] = 1, 1                            # two voxels joined across an edge ...
    lab[8, 8, 32], lab[7, 7, 31] = 1, 1                            # ... and two joined across a corner of the tiles: a tie at 26
    lab[10, 2, 5], lab[10, 2, 6] = 2, 2
    lab[1, 10, 20] = 2
    for c, kept in ((6, [(3, 3, 30)]), (18, [(3, 3, 30), (3, 4, 31)]), (26, [(3, 3, 30), (3, 4, 31)])):
        want = np.zeros(shape, np.uint16)
        for at in kept:
            want[at] = 1
        want[10, 2, 5], want[10, 2, 6] = 2, 2
        assert same(keep_largest_ref(lab, LISTED, NC, c)[0], want)
        for impl in IMPLS:
            work = dev_labels(lab)
            removed = torch.zeros(NC, dtype=torch.int32, device=DEV)
            CN.keep_largest(work, [2, 1, 2], NC, c, removed=removed, impl=impl)                # duplicates are allowed
            assert same(host_u16(work), want) and removed.cpu().tolist() == [0, 4 - len(kept), 1, 0], (c, impl)
    for c in CONNS:
        work = dev_labels(lab)
        removed = torch.full((NC,), 5, dtype=torch.int32, device=DEV)
        CN.keep_largest(work, [], NC, c, removed=removed)
        assert same(host_u16(work), lab.astype(np.uint16)) and removed.cpu().tolist() == [0] * NC    # still zero-filled


@pytest.mark.parametrize("off", [1, 3])
def test_label_map_and_scratch_pointers_off_alignment(off):
    """through the raw ABI: the label map at an odd address, the scratch 1 and 3 bytes off"""
    shape = (9, 9, 33)
    lib = U.engine.lib
    stream = torch.cuda.current_stream().cuda_stream
    listed = (ctypes.c_uint32 * len(LISTED))(*LISTED)
    for c in CONNS:
        lab, want_inst, n = case(shape, "random50", c)
        want, want_removed = keep_largest_ref(lab, LISTED, NC, c)
        raw = np.frombuffer(lab.astype(np.uint16).tobytes(), np.uint8)
        S, M = lab.size, n + 1
        need = CN.keep_largest_scratch_bytes(S, NC)
        lneed = CN.label_scratch_bytes(S, NC, M)
        scratch = torch.empty(max(need, lneed) + 8, dtype=torch.uint8, device=DEV)
        for impl in (1, 2, 0):
            lbuf = torch.full((raw.size + 16,), 0xEE, dtype=torch.uint8, device=DEV)
            lbuf[off:off + raw.size] = torch.from_numpy(raw.copy()).to(DEV)
            assert (lbuf.data_ptr() + off) % 2 == 1
            ibuf, inst = guarded(S, torch.int32)
            rbuf, rows = guarded((M + 1) * 12, torch.int64)
            fbuf, info = guarded(2, torch.int64)
            U.engine.check(lib.unet_conn_label(shape[2], shape[1], shape[0], lbuf.data_ptr() + off, NC, listed, len(LISTED), inst.data_ptr(),
                                               rows.data_ptr(), M, info.data_ptr(), c, impl, scratch.data_ptr() + off, lneed, stream))
            assert same(inst.cpu().numpy().reshape(shape), want_inst) and info.cpu().tolist() == [n, n]
            assert same(rows.cpu().numpy().reshape(M + 1, 12), rows_ref(want_inst, lab, M))
            assert guards_intact(ibuf, S) and guards_intact(rbuf, (M + 1) * 12) and guards_intact(fbuf, 2)
            removed = torch.zeros(NC, dtype=torch.int32, device=DEV)
            U.engine.check(lib.unet_conn_keep_largest(shape[2], shape[1], shape[0], lbuf.data_ptr() + off, NC, listed, len(LISTED),
                                                      removed.data_ptr(), c, impl, scratch.data_ptr() + off, need, stream))
            got = lbuf.cpu().numpy()
            assert got[off:off + raw.size].tobytes() == want.tobytes() and (got[:off] == 0xEE).all() and (got[off + raw.size:] == 0xEE).all()
            assert same(removed.cpu().numpy().view(np.uint32), want_removed)


# ---- holes -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_holes_are_the_restatement_under_every_impl_and_connectivity(shape):
    scratch = torch.empty(CN.holes_scratch_bytes(shape), dtype=torch.uint8, device=DEV)
    D, H, W = shape
    n_words = D * H * ((W + 63) // 64)
    wants = {}
    for name, c, impl in cases_of(shape, HOLE_PRODUCT, HOLE_SPARSE):
        m = TMH.MAPS[name](shape)
        if (name, c) not in wants:
            wants[(name, c)] = holes_ref(m, c)
        holes, n = wants[(name, c)]
        src = dev_mask(m)
        buf, view = guarded(n_words, torch.int64)
        out = MO.Mask(view.view(D, H, (W + 63) // 64), shape)
        got, info = CN.fill_holes(src, c, impl=impl, scratch=scratch, out=out)
        assert got is out and same_mask(out, m | holes), (name, c, impl)
        assert info.cpu().tolist() == [int(holes.sum()), n], (name, c, impl)
        assert guards_intact(buf, n_words) and same_mask(src, m)
        if c == 6:                                                               # the older sibling's bytes
            old, old_info = MO.fill_holes(src, impl=impl)
            assert torch.equal(old.bits, out.bits) and torch.equal(old_info, info), (name, impl)
        CN.fill_holes(src, c, impl=impl, out=src)                                # in place
        assert same_mask(src, m | holes), (name, c, impl)
    if shape in ((17, 17, 65), (38, 44, 40)):                                    # a test of nothing cannot pass: the dense map has
        n = [holes_ref(TMH.MAPS["random85"](shape), c)[1] for c in CONNS]        # holes under every connectivity, fewer with more
        assert n[0] > n[1] > n[2] > 0                                            # ways out (at 0.7 a 26-connected background may leave none)


def test_the_shells_fill_as_the_definitions_say():
    stream = torch.cuda.current_stream().cuda_stream
    for opening, want in ((None, (27, 27, 27)), ("face", (0, 0, 0)), ("edge", (27, 0, 0)), ("corner", (27, 27, 0))):
        m = shell(opening)
        for c, filled in zip(CONNS, want):
            for impl in IMPLS:
                got, info = CN.fill_holes(dev_mask(m), c, impl=impl)
                assert info.cpu().tolist() == [filled, 1 if filled else 0], (opening, c, impl)
                assert same_mask(got, m | holes_ref(m, c)[0])
            got, info = MO.fill_holes(dev_mask(m), connectivity=c)               # the keyword of morph.fill_holes
            assert info.cpu().tolist() == [filled, 1 if filled else 0]
            # without info
            src, out = dev_mask(m), dev_mask(np.zeros(m.shape, bool))
            scratch = torch.empty(CN.holes_scratch_bytes(m.shape), dtype=torch.uint8, device=DEV)
            U.engine.check(U.engine.lib.unet_conn_holes(9, 9, 9, src.bits.data_ptr(), out.bits.data_ptr(), None, c, 0, scratch.data_ptr(),
                                                        scratch.numel(), stream))
            assert int(MO.count(out)) == int(m.sum()) + filled
        assert MO.fill_holes(dev_mask(m))[1].cpu().tolist() == [want[0], 1 if want[0] else 0]      # without the keyword: 6


# ---- connectivity 6 is the older headers' ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_connectivity_6_writes_the_older_siblings_bytes_on_every_shape_and_map(shape):
    for name in MAPS:
        lab = case(shape, name, 6)[0]
        lab_dev = dev_labels(lab)
        for impl in IMPLS:
            new, old = CN.label(lab_dev, NC, LISTED, 6, max_instances=50, impl=impl), IN.label(lab_dev, NC, LISTED, max_instances=50, impl=impl)
            assert all(torch.equal(a, b) for a, b in zip(new, old)), (name, impl)
            a, b = lab_dev.clone(), lab_dev.clone()
            ra, rb = torch.zeros(NC, dtype=torch.int32, device=DEV), torch.zeros(NC, dtype=torch.int32, device=DEV)
            CN.keep_largest(a, LISTED, NC, 6, removed=ra, impl=impl)
            CMP.keep_largest(b, LISTED, NC, removed=rb, impl=impl)
            assert torch.equal(a.view(torch.int16), b.view(torch.int16)) and torch.equal(ra, rb), (name, impl)
    for name in HOLE_MAPS:
        src = dev_mask(TMH.MAPS[name](shape))
        for impl in IMPLS:
            (new, new_info), (old, old_info) = CN.fill_holes(src, 6, impl=impl), MO.fill_holes(src, impl=impl)
            assert torch.equal(new.bits, old.bits) and torch.equal(new_info, old_info), (name, impl)


# ---- the keyword through the public callers --------------------------------------------------------------------------------------------
def three_class_map(shape, opening):
    """specks of classes 1, 2 and 3 around a shell of class 1 that is open at a face, an edge or a corner voxel"""
    rng = np.random.default_rng(5)
    r = rng.random(shape)
    lab = np.where(r < 0.25, 1, np.where(r < 0.45, 2, np.where(r < 0.5, 3, 0)))
    lab[1:8, 1:8, 1:8] = 0
    lab[2:7, 2:7, 2:7] = np.where(shell(opening)[2:7, 2:7, 2:7], 1, 0)
    return lab.astype(np.uint16)


def test_components_instances_and_morph_take_the_keyword():
    shape = (12, 20, 40)
    for opening in ("edge", "corner"):
        lab = three_class_map(shape, opening)
        for c in CONNS:
            want, want_removed = keep_largest_ref(lab, LISTED, NC, c)
            work, removed = dev_labels(lab), torch.zeros(NC, dtype=torch.int32, device=DEV)
            assert CMP.keep_largest(work, LISTED, NC, removed=removed, connectivity=c) is work
            assert same(host_u16(work), want) and same(removed.cpu().numpy().view(np.uint32), want_removed)
            want_inst, n = label_ref(lab, LISTED, c, NC)
            inst, rows, info = IN.label(dev_labels(lab), NC, LISTED, max_instances=n, connectivity=c)
            assert same(inst.cpu().numpy(), want_inst) and same(rows.cpu().numpy(), rows_ref(want_inst, lab, n)) and info.cpu().tolist() == [n, n]
            # fill_holes_label and run: a hole voxel that reads 0 becomes the value
            write = holes_ref(np.isin(lab, LISTED), c)[0] & (lab == 0)
            filled = np.where(write, 2, lab).astype(np.uint16)
            t = dev_labels(lab)
            changed = MO.fill_holes_label(t, LISTED, 2, NC, connectivity=c)
            assert same(host_u16(t), filled) and int(changed) == int(write.sum())
            t = dev_labels(lab)
            changed = MO.run(t, [("fill_holes", LISTED, 2, c)], NC)
            assert same(host_u16(t), filled) and changed.cpu().tolist() == [int(write.sum())]
        # without the keyword: the previous output, which is connectivity 6
        work = dev_labels(lab)
        CMP.keep_largest(work, LISTED, NC)
        assert same(host_u16(work), keep_largest_ref(lab, LISTED, NC, 6)[0])
        assert same(IN.label(dev_labels(lab), NC, LISTED)[0].cpu().numpy(), label_ref(lab, LISTED, 6, NC)[0])
        t = dev_labels(lab)
        MO.run(t, [("fill_holes", LISTED, 2)], NC)
        assert same(host_u16(t), np.where(holes_ref(np.isin(lab, LISTED), 6)[0] & (lab == 0), 2, lab).astype(np.uint16))
    # the shell opened at an edge voxel is closed to 6 and open to 18 and 26
    lab = three_class_map(shape, "edge")
    counts = [int((holes_ref(np.isin(lab, LISTED), c)[0] & (lab == 0)).sum()) for c in CONNS]
    assert counts[0] >= 27 > counts[1] >= counts[2]


def scores_equal(a, b):
    assert sorted(a) == sorted(b)
    return all(same(np.asarray(a[k]), np.asarray(b[k])) for k in a)


def test_lesion_scores_with_the_keyword_and_an_edge_touching_lesion():
    shape = (9, 9, 33)
    pred, ref = case(shape, "random30", 6)[0], np.roll(case(shape, "random30", 6)[0], 1, axis=1)
    for c in CONNS:
        ri, rn = label_ref(ref, [1, 2, 3], c, NC)
        pi, pn = label_ref(pred, [1, 2, 3], c, NC)
        want = IN.detection(rows_ref(ri, ref, rn), rows_ref(pi, pred, pn), match_ref(ri, pi), NC)
        assert scores_equal(IN.lesion_scores(dev_labels(pred), dev_labels(ref), NC, connectivity=c), want)
        assert scores_equal(IN.lesion_scores(dev_labels(pred), dev_labels(ref), NC, max_instances=3, max_pairs=2, connectivity=c), want)
        if c == 6:
            assert scores_equal(IN.lesion_scores(dev_labels(pred), dev_labels(ref), NC), want)           # without the keyword
    # one lesion of two cubes that touch across an edge, at the corner of the tiles; the prediction finds one cube and invents a speck
    ref = np.zeros((12, 12, 40), np.int64)
    ref[2:4, 6:8, 30:32] = 1
    ref[2:4, 8:10, 32:34] = 1
    pred = np.zeros_like(ref)
    pred[2:4, 6:8, 30:32] = 1
    pred[9, 2, 5] = 1
    for c, n_ref, detected, missed in ((6, 2, 1, 1), (18, 1, 1, 0), (26, 1, 1, 0)):
        got = IN.lesion_scores(dev_labels(pred), dev_labels(ref), 2, connectivity=c)
        assert (int(got["n_ref"][1]), int(got["detected"][1]), int(got["missed"][1])) == (n_ref, detected, missed), c
        assert (int(got["n_pred"][1]), int(got["false_pos"][1])) == (2, 1) and float(got["sensitivity"][1]) == detected / n_ref, c
        assert IN.label(dev_labels(ref), 2, connectivity=c)[2].cpu().tolist()[0] == n_ref


def test_lesion_qc_takes_the_keyword_and_keeps_its_report_format(tmp_path):
    from unet_studio_amd import qc as Q
    dim, C = (16, 16, 16), 4
    W, H, D = dim
    m = small_model(C)
    m.prepare_for_inference()
    g = torch.Generator().manual_seed(3)
    lab = torch.randint(0, 3, (D, H, W), generator=g).to(torch.float32)
    lab[torch.rand(D, H, W, generator=g) < 0.6] = 0.0
    lab.view(-1)[0] = 2
    cases = [("/data/tpl/t0_T1w.nii.gz", "/data/tpl/t0_label.nii.gz", torch.randn(1, D, H, W, generator=g).numpy(), lab.numpy(), True)]
    path, report = str(tmp_path / "qc_model.nz"), str(tmp_path / "qc_model.lesion_report.tsv")
    x = torch.from_numpy(cases[0][2]).view(1, 1, D, H, W).to(DEV)
    pred = torch.argmax(m._forward_level0(x)[0], dim=0).to(torch.int32).to(torch.uint16).contiguous()
    reports = {}
    for c in CONNS:
        assert Q.lesion_qc(m, path, cases, connectivity=c) == (0, report)
        reports[c] = open(report, "rb").read()
        scores = IN.lesion_scores(pred, dev_labels(cases[0][3]), C, connectivity=c)
        assert Q.format_lesion_report(C, [(cases[0][0], cases[0][1], scores)]).encode() == reports[c]
        ri, rn = label_ref(cases[0][3].astype(np.int64), [1, 2, 3], c, C)
        assert int(scores["n_ref"][1:].sum()) == rn
    assert Q.lesion_qc(m, path, cases) == (0, report) and open(report, "rb").read() == reports[6]      # without the keyword: 6
    assert reports[6] != reports[26]                                                                   # the case tells them apart
    assert [len(r.decode().splitlines()[1].split("\t")) for r in reports.values()] == [2 + 7 * (C - 1)] * 3
    assert Q.lesion_qc(m, path, cases, connectivity=7) == (1, "lesion_qc: connectivity must be 6, 18 or 26, got 7")


# ---- run_postproc and EvaluateUNet -----------------------------------------------------------------------------------------------------
def noisy_logits(seed, c, shape):
    """low-frequency logits plus strong noise: label maps with pieces that touch across edges and corners only"""
    g = torch.Generator().manual_seed(seed)
    coarse = torch.randn((1, c) + tuple((s + 3) // 4 for s in shape), generator=g)
    x = torch.nn.functional.interpolate(coarse, size=shape, mode="trilinear", align_corners=False)[0]
    return (x + 1.5 * torch.randn(x.shape, generator=g)).contiguous().to(DEV)


def test_run_postproc_single_component_connectivity():
    c, shape = 4, (13, 22, 41)
    logits = noisy_logits(11, c, shape)
    chain, params = "softmax+create_mask+argmax", {"argmax": 0.45}
    base = P.run_postproc(logits, chain, params=params)
    results = {}
    for conn in CONNS:
        want = base["label"].clone()
        CN.keep_largest(want, [1, 3], c, conn)
        assert same(host_u16(want), keep_largest_ref(host_u16(base["label"]), [1, 3], c, conn)[0])
        got = P.run_postproc(logits, chain, params=params, single_component=[1, 3], single_component_connectivity=conn)
        assert torch.equal(got["label"].view(torch.int16), want.view(torch.int16)), conn
        assert torch.equal(got["fg_prob"], base["fg_prob"]) and torch.equal(got["label_prob"], base["label_prob"])    # not touched
        results[conn] = host_u16(want)
    assert not same(results[6], results[18]) and not same(results[18], results[26])                 # the case tells them apart
    today = P.run_postproc(logits, chain, params=params, single_component=[1, 3])                        # without the keyword: 6
    assert same(host_u16(today["label"]), results[6])
    got = P.run_postproc(logits, chain, params=params, single_component_connectivity=26)                 # nothing listed: no call
    assert same(host_u16(got["label"]), host_u16(base["label"]))
    with pytest.raises(U.UNetError, match="single_component: connectivity must be 6, 18 or 26, got 7"):
        P.run_postproc(logits, chain, params=params, single_component=[1], single_component_connectivity=7)


SMOKE_ARCH = ("conv8,ks3,stride1+norm,leaky_relu+conv8,ks3,stride1+norm,leaky_relu\n"
              "conv16,ks3,stride2+norm,leaky_relu+conv16,ks3,stride1+norm,leaky_relu+conv_trans8,ks2,stride2\n"
              "conv8,ks3,stride1+norm,leaky_relu+conv8,ks3,stride1+norm,leaky_relu+conv%d,ks1,stride1")
OUTPUTS = ("label", "fg_prob", "label_prob")
PARAMS = {"argmax": 0.0}                                                  # every voxel takes its best foreground class


def small_model(out_c=4):
    m = U.UNet3d(1, out_c, SMOKE_ARCH % out_c, device=DEV, dtype="fp32", seed=2)
    m.dim, m.voxel_size = (16, 16, 16), (1.0, 1.0, 1.0)
    return m


def volumes():
    rs = np.random.RandomState(7)
    return [[rs.rand(16, 16, 16).astype(F), U.NativeVolume(rs.rand(20, 18, 22).astype(F), (1.1, 0.9, 1.2))],
            [U.NativeVolume(rs.rand(13, 21, 17).astype(F), (0.8, 1.3, 1.0))]]


def test_evaluate_single_component_connectivity():
    m = small_model()
    ios = volumes()
    base = U.EvaluateUNet(m, postproc="model", outputs=OUTPUTS, params=PARAMS).start(ios)
    listed = [1, 2, 3]
    today = U.EvaluateUNet(m, postproc="model", outputs=OUTPUTS, params=PARAMS, single_component=listed).start(ios)
    differ = 0
    for conn in CONNS:
        ev = U.EvaluateUNet(m, postproc="model", outputs=OUTPUTS, params=PARAMS, single_component=listed, single_component_connectivity=conn)
        got = ev.start(ios)
        assert not ev.aborted and ev.error_msg == "" and ev.cur_prog == 2
        for gf, bf, tf in zip(got, base, today):
            for g, b, t in zip(gf, bf, tf):
                want = dev_labels(b["label"])
                CN.keep_largest(want, listed, 4, conn)
                assert g["label"].dtype == np.uint16 and g["label"].tobytes() == host_u16(want).tobytes(), conn
                assert g["label"].tobytes() == keep_largest_ref(b["label"], listed, 4, conn)[0].tobytes(), conn
                assert g["fg_prob"].tobytes() == b["fg_prob"].tobytes() and g["label_prob"].tobytes() == b["label_prob"].tobytes()
                if conn == 6:
                    assert g["label"].tobytes() == t["label"].tobytes()             # without the keyword: 6
                else:
                    differ += int((g["label"] != t["label"]).sum())
    assert differ > 0                                                               # the case tells 6 from 18 and 26


def test_evaluate_a_bad_connectivity_ends_the_run_before_any_forward():
    m = small_model()
    calls = []
    real = m.forward
    m.forward = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
    ios = volumes()
    for bad in (7, 0, None, "26", 6.0):
        for chain, listed in (("model", [1]), (None, None)):                   # checked even where it has nothing to act on
            ev = U.EvaluateUNet(m, postproc=chain, single_component=listed, single_component_connectivity=bad)
            out = ev.start(ios)
            assert ev.aborted and not ev.running and ev.cur_prog == 0 and out[0][0] is ios[0][0], bad
            assert ev.error_msg == "single_component: connectivity must be 6, 18 or 26, got %r" % (bad,), bad
    assert not calls
    ev = U.EvaluateUNet(m, postproc="model", single_component=[1], single_component_connectivity=26)
    out = ev.start(ios)
    assert not ev.aborted and ev.error_msg == "" and len(calls) == 3 and out[1][0]["label"].shape == (13, 21, 17)
