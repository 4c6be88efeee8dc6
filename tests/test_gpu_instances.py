"""GPU: the instances of a label map on the device (include/unet_instances.h) -- `label` under LABEL_TILED, LABEL_GLOBAL and the
default and `match` under IMPL_LDS, IMPL_GLOBAL and the default against label_ref, rows_ref and match_ref (the restatements of
test_instances_host.py), every case twice into garbage-filled outputs with guard words on both sides (the second time at an address
that is 4-byte aligned only); capacities below what the map holds; remove_small; single_component_label against the rows; then
qc.lesion_qc against instances.lesion_scores called by hand on the same run's argmax.  Every comparison is exact equality of bytes.
Shapes are (D, H, W).

No kernel of kernels_instances.hip caps its grid: every block takes a fixed stretch (4096 voxels in the scan, gather and remove
kernels, 512 * 8 units of 8 voxels in the table and match kernels), so there is no grid-stride path to cross; (38, 44, 40) and
(2, 3, 70000) run 17 and 103 scan blocks and 3 and 13 table blocks."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import unet_studio_amd as U
from unet_studio_amd import components as CMP
from unet_studio_amd import instances as IN
from unet_studio_amd import qc as Q

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_instances_host import label_ref, match_ref, remove_small_ref, rows_ref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LABEL_IMPLS = (IN.LABEL_TILED, IN.LABEL_GLOBAL, IN.LABEL_DEFAULT)
MATCH_IMPLS = (IN.IMPL_LDS, IN.IMPL_GLOBAL, IN.IMPL_DEFAULT)
SHAPES = [(1, 1, 1), (3, 5, 7), (9, 9, 33), (2, 3, 65), (38, 44, 40), (2, 3, 70000)]
NC = 4                                                             # classes 1, 2 listed; 3 is a value of the maps that is not
LISTED = [1, 2]
G = 64                                                             # guard words on each side
GUARD = {torch.int32: -0x5A3C5A3D, torch.int64: -0x5A3C5A3C5A3C5A3D}
GARBAGE = {torch.int32: (0x7B7B7B7B, -3), torch.int64: (0x7B7B7B7B7B7B7B7B, -3)}


def same(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()


def guarded(n, dtype, rep):
    """a buffer of G + 1 + n + G words: guards outside, garbage inside; rep 1 starts the view one word later, so an int32 view is
    4-byte aligned only; -> (buffer, the view a call writes, where it starts)"""
    at = G + rep
    buf = torch.full((n + 2 * G + 1,), GUARD[dtype], dtype=dtype, device=DEV)
    buf[at:at + n] = GARBAGE[dtype][rep]
    return buf, buf[at:at + n], at


def guards_intact(buf, at, n):
    b = buf.cpu().numpy()
    g = GUARD[buf.dtype]
    return bool((b[:at] == g).all() and (b[at + n:] == g).all())


def dev_labels(a):
    return torch.from_numpy(np.ascontiguousarray(a).astype(np.int32)).to(DEV).to(torch.uint16)


def dev_inst(a, rep=0):
    """an int32 map on the device; rep 1: at an address that is 4-byte aligned only"""
    flat = torch.from_numpy(np.ascontiguousarray(a).astype(np.int32).reshape(-1))
    buf = torch.zeros(flat.numel() + 4, dtype=torch.int32, device=DEV)
    buf[rep:rep + flat.numel()] = flat.to(DEV)
    return buf[rep:rep + flat.numel()]


# ---- the maps: (D, H, W) -> labels with values in 0..3 ---------------------------------------------------------------------------------
def solid(shape, rng):
    """one instance: every update on one row and one pair"""
    return np.ones(shape, np.int64)


def checkerboard(shape, rng):
    """ceil(S / 2) singletons: the most instances a grid can hold"""
    z, y, x = np.indices(shape)
    return ((x + y + z) % 2 == 0).astype(np.int64)


def slabs(shape, rng):
    """two listed classes in touching slabs along x: they stay two instances"""
    x = np.indices(shape)[2]
    return (1 + (x >= (shape[2] + 1) // 2)).astype(np.int64)


def split(shape, rng):
    """a listed class cut in two by a plane of an unlisted one"""
    lab = np.ones(shape, np.int64)
    lab[:, :, shape[2] // 2] = 3
    return lab


def serpentine(shape, rng):
    """a one-voxel-wide path through all tiles: even rows of even slices in full, joined at alternating ends, the slices joined through
    one voxel of the odd slices: one instance, the longest union chains"""
    z, y, x = np.indices(shape)
    end = np.where((y // 2) % 2 == 0, shape[2] - 1, 0)
    return np.where(z % 2 == 0, (y % 2 == 0) | (x == end), (x == 0) & (y == 0)).astype(np.int64)


def random_02(shape, rng):
    return np.where(rng.random(shape) < 0.2, rng.integers(1, 4, shape), 0)


def random_05(shape, rng):
    return np.where(rng.random(shape) < 0.5, rng.integers(1, 4, shape), 0)


KINDS = (solid, checkerboard, slabs, split, serpentine, random_02, random_05)
_CACHE = {}


def case(shape, make):
    """(labels, inst, N) of a map, computed once and shared; never changed"""
    key = (shape, make.__name__)
    if key not in _CACHE:
        lab = make(shape, np.random.default_rng(shape[2] + len(make.__name__)))
        inst, n = label_ref(lab, NC, LISTED)
        for a in (lab, inst):
            a.setflags(write=False)
        _CACHE[key] = (lab, inst, n)
    return _CACHE[key]


def check_label(lab, want_inst, n, M, impls=LABEL_IMPLS, classes=LISTED):
    want_rows = rows_ref(want_inst, lab, M)
    want_info = np.asarray([n, min(n, M)], np.int64)
    lab_dev = dev_labels(lab)
    S = lab.size
    for impl in impls:
        for rep in range(2):
            ibuf, inst, iat = guarded(S, torch.int32, rep)
            rbuf, rows, rat = guarded((M + 1) * 12, torch.int64, rep)
            fbuf, info, fat = guarded(2, torch.int64, rep)
            got = IN.label(lab_dev, NC, classes, max_instances=M, impl=impl, out=(inst, rows, info))
            assert got[0].data_ptr() == inst.data_ptr() and tuple(got[0].shape) == lab.shape and tuple(got[1].shape) == (M + 1, 12)
            assert same(info.cpu().numpy(), want_info), (impl, rep, info.cpu().numpy(), want_info)
            assert same(got[0].cpu().numpy(), want_inst), (impl, rep)
            assert same(got[1].cpu().numpy(), want_rows), (impl, rep)
            assert guards_intact(ibuf, iat, S) and guards_intact(rbuf, rat, (M + 1) * 12) and guards_intact(fbuf, fat, 2)
    return want_rows


def check_match(ia, ib, max_pairs=None, impls=MATCH_IMPLS):
    want = match_ref(ia, ib)
    P = want.shape[0] + 5 if max_pairs is None else max_pairs
    assert P >= want.shape[0]
    want_keys = (want[:, 0] << 32) | want[:, 1]
    for impl in impls:
        for rep in range(2):
            a, b = dev_inst(ia, rep), dev_inst(ib, rep)
            kbuf, keys, kat = guarded(P, torch.int64, rep)
            cbuf, counts, cat = guarded(P, torch.int64, rep)
            fbuf, info, fat = guarded(2, torch.int64, rep)
            IN.match_raw(a, b, P, impl=impl, out=(keys, counts, info))
            assert same(info.cpu().numpy(), np.asarray([want.shape[0], 0], np.int64)), (impl, rep, info.cpu().numpy())
            k, c = keys.cpu().numpy(), counts.cpu().numpy()
            n = want.shape[0]
            order = np.argsort(k[:n], kind="stable")
            assert same(k[:n][order], want_keys) and same(c[:n][order], np.ascontiguousarray(want[:, 2])), (impl, rep)
            assert (k[n:] == GARBAGE[torch.int64][rep]).all() and (c[n:] == GARBAGE[torch.int64][rep]).all()      # not written
            assert guards_intact(kbuf, kat, P) and guards_intact(cbuf, cat, P) and guards_intact(fbuf, fat, 2)
    return want


# ---- label ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("make", KINDS, ids=[k.__name__ for k in KINDS])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_label_shapes_and_maps(shape, make):
    lab, inst, n = case(shape, make)
    S = lab.size
    if make is solid:
        assert n == 1
    if make is checkerboard:
        assert n == (S + 1) // 2
    if make is slabs:
        assert n == (2 if shape[2] > 1 else 1)
    if make is split and shape[2] >= 3:
        assert n == 2
    if make is serpentine:
        assert n == 1 and inst[-1].any() and inst[:, -1].any()
    rows = check_label(lab, inst, n, n + 3)
    assert rows[1:n + 1, 1].sum() == (inst > 0).sum() and (rows[n + 1:, 1] == 0).all()
    if shape == (2, 3, 70000) and make is solid:
        assert rows[1, 2] == 6 * (70000 * 69999 // 2) > 2 ** 32       # the sum of x passes 32 bits


def test_label_none_lists_every_class_and_an_empty_list_lists_nothing_and_uint8_is_cast():
    shape = (9, 9, 33)
    lab = case(shape, random_05)[0]
    inst_all, n_all = label_ref(lab, NC)
    assert n_all > case(shape, random_05)[2]
    check_label(lab, inst_all, n_all, n_all, classes=None)
    check_label(lab, np.zeros(shape, np.int32), 0, 4, classes=[])
    got = IN.label(torch.from_numpy(lab.astype(np.uint8)).to(DEV), NC)
    assert same(got[0].cpu().numpy(), inst_all) and int(got[2][0]) == n_all and tuple(got[1].shape) == (IN.DEFAULT_MAX_INSTANCES + 1, 12)
    assert same(got[1].cpu().numpy(), rows_ref(inst_all, lab, IN.DEFAULT_MAX_INSTANCES))


@pytest.mark.parametrize("M", [0, 1, 100, IN.LDS_ROWS - 1, IN.LDS_ROWS, 1336])
def test_label_with_fewer_rows_than_instances(M):
    """info[0] is the true N, inst is complete, the rows up to the capacity are exact and nothing outside rows is written"""
    lab, inst, n = case((9, 9, 33), checkerboard)
    assert n == 1337 > M
    check_label(lab, inst, n, M)


@pytest.mark.parametrize("off", [1, 3])
def test_label_map_and_scratch_pointers_off_alignment(off):
    """through the raw ABI: the label map at an odd address, both scratches 1 and 3 bytes off"""
    shape = (9, 9, 33)
    lab, want_inst, n = case(shape, random_05)
    raw = np.frombuffer(lab.astype(np.uint16).tobytes(), np.uint8)
    lbuf = torch.full((raw.size + 16,), 0xEE, dtype=torch.uint8, device=DEV)
    lbuf[off:off + raw.size] = torch.from_numpy(raw.copy()).to(DEV)
    assert (lbuf.data_ptr() + off) % 2 == 1
    M, S = n + 2, lab.size
    need = IN.inst_scratch_bytes(S, NC, M)
    scratch = torch.empty(need + 8, dtype=torch.uint8, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    lib = U.engine.lib
    listed = (ctypes.c_uint32 * len(LISTED))(*LISTED)
    want_rows = rows_ref(want_inst, lab, M)
    other = case(shape, random_02)[1]
    want_pairs = match_ref(want_inst, other)
    P = want_pairs.shape[0] + 1
    mneed = IN.match_scratch_bytes(P)
    mscratch = torch.empty(mneed + 8, dtype=torch.uint8, device=DEV)
    for impl in (1, 2, 0):
        ibuf, inst, iat = guarded(S, torch.int32, 0)
        rbuf, rows, rat = guarded((M + 1) * 12, torch.int64, 0)
        fbuf, info, fat = guarded(2, torch.int64, 0)
        U.engine.check(lib.unet_inst_label(shape[2], shape[1], shape[0], lbuf.data_ptr() + off, NC, listed, len(LISTED), inst.data_ptr(),
                                           rows.data_ptr(), M, info.data_ptr(), impl, scratch.data_ptr() + off, need, stream))
        assert same(inst.cpu().numpy().reshape(shape), want_inst) and same(rows.cpu().numpy().reshape(M + 1, 12), want_rows)
        assert info.cpu().numpy().tolist() == [n, n]
        assert guards_intact(ibuf, iat, S) and guards_intact(rbuf, rat, (M + 1) * 12) and guards_intact(fbuf, fat, 2)
        kbuf, keys, kat = guarded(P, torch.int64, 0)
        cbuf, counts, cat = guarded(P, torch.int64, 0)
        U.engine.check(lib.unet_inst_match(inst.data_ptr(), dev_inst(other).data_ptr(), S, keys.data_ptr(), counts.data_ptr(), P, info.data_ptr(),
                                           impl, mscratch.data_ptr() + off, mneed, stream))
        assert info.cpu().numpy().tolist() == [P - 1, 0]
        k, c = keys.cpu().numpy()[:P - 1], counts.cpu().numpy()[:P - 1]
        order = np.argsort(k, kind="stable")
        assert same(k[order], (want_pairs[:, 0] << 32) | want_pairs[:, 1]) and same(c[order], np.ascontiguousarray(want_pairs[:, 2]))
        assert guards_intact(kbuf, kat, P) and guards_intact(cbuf, cat, P) and guards_intact(fbuf, fat, 2)


# ---- match ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_match_checkerboard_against_solid_shares_the_low_word(shape):
    ia, ib = case(shape, checkerboard)[1], case(shape, solid)[1]
    want = check_match(ia, ib)
    assert want.shape[0] == (ia.size + 1) // 2 and (want[:, 1] == 1).all() and (want[:, 2] == 1).all()
    want = check_match(ib, ia)                                      # and the high word
    assert (want[:, 0] == 1).all()


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_match_a_comb_random_against_its_shift_and_disjoint_maps(shape):
    blobs = case(shape, random_05)[1]
    z, y, x = np.indices(shape)
    comb = label_ref(((x % 2 == 0) | (y == 0)).astype(np.int64), 2)[0]
    assert comb.max() == 1
    want = check_match(blobs, comb)
    assert want[:, 2].sum() == ((blobs > 0) & (comb > 0)).sum()
    lab = case(shape, random_02)[0]
    shifted = label_ref(np.roll(lab, 1, axis=2), NC, LISTED)[0]
    check_match(case(shape, random_02)[1], shifted)
    check_match(case(shape, solid)[1], case(shape, solid)[1])       # one pair holding every voxel
    ia, ib = np.where(x % 2 == 0, blobs, 0), np.where(x % 2 == 1, blobs, 0)
    assert check_match(ia, ib).shape == (0, 3)
    assert check_match(ia, ib, max_pairs=0).shape == (0, 3)


@pytest.mark.parametrize("impl", MATCH_IMPLS)
@pytest.mark.parametrize("max_pairs", [0, 7, 32, 33, 668, 1336])
def test_match_with_room_for_fewer_pairs_than_there_are(max_pairs, impl):
    """the flag is set, nothing outside keys and counts is written and the call returns: with 7 the table of 64 slots fills up and the
    probing gives up, with 1336 the table holds all 1337 pairs and the cursor passes the capacity"""
    ia, ib = case((9, 9, 33), checkerboard)[1], case((9, 9, 33), solid)[1]
    for rep in range(2):
        kbuf, keys, kat = guarded(max_pairs, torch.int64, rep)
        cbuf, counts, cat = guarded(max_pairs, torch.int64, rep)
        fbuf, info, fat = guarded(2, torch.int64, rep)
        IN.match_raw(dev_inst(ia, rep), dev_inst(ib, rep), max_pairs, impl=impl, out=(keys, counts, info))
        got = info.cpu().numpy()
        assert 0 <= got[0] <= max_pairs and got[1] != 0
        assert guards_intact(kbuf, kat, max_pairs) and guards_intact(cbuf, cat, max_pairs) and guards_intact(fbuf, fat, 2)
    got = IN.match(dev_inst(ia), dev_inst(ib), max_pairs=max_pairs, impl=impl)     # succeeds by calling again with more
    assert same(got, match_ref(ia, ib)) and got.shape == (1337, 3)


def test_match_wrapper_returns_the_pairs_sorted():
    for shape in ((3, 5, 7), (38, 44, 40)):
        ia, ib = case(shape, random_05)[1], case(shape, random_02)[1]
        assert same(IN.match(dev_inst(ia), dev_inst(ib)), match_ref(ia, ib))
    z = np.zeros((3, 5, 7), np.int32)
    assert IN.match(dev_inst(z), dev_inst(z)).shape == (0, 3)


# ---- remove_small --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(3, 5, 7), (9, 9, 33), (38, 44, 40)], ids=str)
def test_remove_small_against_its_restatement(shape):
    lab, want_inst, n = case(shape, random_05)
    for M in (n, n // 2):                                           # n // 2: the ids above it have no row and are left alone
        inst, rows, info = IN.label(dev_labels(lab), NC, LISTED, max_instances=M)
        assert same(rows.cpu().numpy(), rows_ref(want_inst, lab, M))
        for min_voxels in (1, 2, 4, 10 ** 9):
            want, want_removed = remove_small_ref(lab.astype(np.uint16), want_inst, rows_ref(want_inst, lab, M), min_voxels, NC)
            for rep, removed in enumerate((torch.full((NC,), 77, dtype=torch.int32, device=DEV), None)):
                work = dev_labels(lab)
                out = IN.remove_small(work, inst.view(-1), rows, min_voxels, removed=removed, n_classes=NC)
                assert out is work and same(work.view(torch.int16).cpu().numpy().view(np.uint16), want), (M, min_voxels, rep)
                if removed is not None:
                    assert removed.cpu().numpy().astype(np.int64).tolist() == want_removed.tolist()
            if min_voxels == 10 ** 9 and M < n:
                assert (want[(want_inst > M)] == lab[want_inst > M]).all() and (want[(want_inst >= 1) & (want_inst <= M)] == 0).all()


# ---- the shared labelling stage, from the other side ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("make", [checkerboard, slabs, random_02, random_05], ids=lambda k: k.__name__)
@pytest.mark.parametrize("shape", [(3, 5, 7), (9, 9, 33), (38, 44, 40)], ids=str)
def test_keep_largest_equals_the_largest_row_per_class(shape, make):
    """single_component_label keeps, per class, the instance with the largest count, the smaller id among equal counts"""
    lab, want_inst, n = case(shape, make)
    inst, rows, info = IN.label(dev_labels(lab), NC, LISTED, max_instances=n)
    rows = rows.cpu().numpy()
    assert same(rows, rows_ref(want_inst, lab, n))
    keep = np.zeros(n + 1, bool)
    for c in LISTED:
        ids = np.flatnonzero(rows[:, 0] == c)
        ids = ids[ids > 0]
        if ids.size:
            keep[ids[np.argmax(rows[ids, 1])]] = True               # argmax: the first, so the smaller id, among equal counts
    want = np.where((want_inst > 0) & ~keep[want_inst], 0, lab).astype(np.uint16)
    for impl in (CMP.IMPL_TILED, CMP.IMPL_GLOBAL, CMP.IMPL_DEFAULT):
        work = dev_labels(lab)
        CMP.keep_largest(work, LISTED, NC, impl=impl)
        assert same(work.view(torch.int16).cpu().numpy().view(np.uint16), want), impl


# ---- lesion_scores and qc.lesion_qc --------------------------------------------------------------------------------------------------
def scores_equal(a, b):
    assert sorted(a) == sorted(b)
    return all(same(np.asarray(a[k]), np.asarray(b[k])) for k in a)


def test_lesion_scores_equal_detection_on_the_restated_tables():
    shape = (9, 9, 33)
    pred, ref = case(shape, random_05)[0], np.roll(case(shape, random_05)[0], 1, axis=1)
    ri, rn = label_ref(ref, NC)
    pi, pn = label_ref(pred, NC)
    for kw in (dict(), dict(rule="iou", threshold=0.3), dict(min_voxels=3)):
        want = IN.detection(rows_ref(ri, ref, rn), rows_ref(pi, pred, pn), match_ref(ri, pi), NC, **kw)
        got = IN.lesion_scores(dev_labels(pred), dev_labels(ref), NC, **kw)
        assert scores_equal(got, want)
        # capacities below what the maps hold: the calls are repeated with more
        assert scores_equal(IN.lesion_scores(dev_labels(pred), dev_labels(ref), NC, max_instances=10, max_pairs=3, **kw), want)
    assert want["n_ref"][1:].sum() > 0 and want["detected"][1:].sum() > 0 and want["false_pos"][1:].sum() > 0


SMOKE_ARCH = ("conv8,ks3,stride1+norm,leaky_relu+conv8,ks3,stride1+norm,leaky_relu\n"
              "conv16,ks3,stride2+norm,leaky_relu+conv16,ks3,stride1+norm,leaky_relu+conv_trans8,ks2,stride2\n"
              "conv8,ks3,stride1+norm,leaky_relu+conv8,ks3,stride1+norm,leaky_relu+conv%d,ks1,stride1")


def test_lesion_qc_report_equals_lesion_scores_on_the_same_argmax_maps(tmp_path):
    dim, C = (16, 16, 16), 4
    W, H, D = dim
    m = U.UNet3d(1, C, SMOKE_ARCH % C, device=DEV, dtype="fp32", seed=9)
    m.dim, m.voxel_size = dim, (1.0, 1.0, 1.0)
    m.prepare_for_inference()
    g = torch.Generator().manual_seed(3)

    def vol(max_label):
        lab = torch.randint(0, max_label + 1, (D, H, W), generator=g).to(torch.float32)
        lab[torch.rand(D, H, W, generator=g) < 0.4] = 0.0
        lab.view(-1)[0] = max_label
        return torch.randn(1, D, H, W, generator=g).numpy(), lab.numpy()

    cases = [("/data/tpl/t0_T1w.nii.gz", "/data/tpl/t0_label.nii.gz") + vol(2) + (True,),
             ("/data/sub-01/anat/sub-01_T1w.nii.gz", "/data/sub-01/anat/sub-01_dseg.nii.gz") + vol(1) + (False,)]     # 1 < 2, 1 + 2 < 4: shifted
    mtl, shift = Q.label_plan(cases, C)
    assert mtl == 2 and shift == [False, True]
    path = str(tmp_path / "qc_model.nz")
    report = str(tmp_path / "qc_model.lesion_report.tsv")
    for kw in (dict(), dict(rule="iou", threshold=0.1, min_voxels=2), dict(labels=[2])):
        assert Q.lesion_qc(m, path, cases, **kw) == (0, report)
        got = open(report, "rb").read()
        assert sorted(os.listdir(tmp_path)) == ["qc_model.lesion_report.tsv"]      # no .tmp left behind
        # by hand on the argmax of a second forward of the same model: the engine's fp32 forward is deterministic
        x = torch.from_numpy(cases[0][2]).view(1, 1, D, H, W).to(DEV)
        pred = torch.argmax(m._forward_level0(x)[0], dim=0).to(torch.int32).to(torch.uint16).contiguous()
        want = dev_labels(cases[0][3])
        hand = dict(kw)
        classes = hand.pop("labels", None)
        scores = IN.lesion_scores(pred, want, C, classes=classes, **hand)
        assert Q.format_lesion_report(C, [(cases[0][0], cases[0][1], scores), (cases[1][0], cases[1][1], None)]).encode() == got
        ri, rn = label_ref(cases[0][3].astype(np.int64), C, classes)
        pi, pn = label_ref(pred.cpu().numpy().astype(np.int64), C, classes)
        assert scores_equal(scores, IN.detection(rows_ref(ri, cases[0][3], rn), rows_ref(pi, pred.cpu().numpy(), pn), match_ref(ri, pi), C, **hand))
        lines = got.decode().splitlines()
        assert len(lines) == 3 and lines[0].split("\t")[:4] == ["image", "ground_truth", "n_ref1", "n_pred1"]
        assert lines[2].split("\t") == ["sub-01_T1w.nii.gz", "sub-01_dseg.nii.gz"] + ["N/A"] * (7 * (C - 1)) and "N/A" not in lines[1]
        if classes == [2]:
            assert lines[1].split("\t")[2:9] == ["0", "0", "0", "0", "nan", "nan", "nan"] and int(lines[1].split("\t")[9]) > 0
    assert Q.lesion_qc(m, path, []) == (1, "no image/label pairs found")
    m1 = U.UNet3d(1, 1, SMOKE_ARCH % 1, device=DEV, dtype="fp32", seed=9)
    assert Q.lesion_qc(m1, path, cases) == (1, "QC requires a categorical model")
    bad = [cases[0][:2] + (cases[0][2][:, :8], cases[0][3], True)]
    assert Q.lesion_qc(m, path, bad) == (1, "/data/tpl/t0_T1w.nii.gz: training data dimension mismatch")
