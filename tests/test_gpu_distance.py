"""GPU: the boundary distances of label maps on the device (include/unet_distance.h) -- transform under IMPL_LDS, IMPL_GLOBAL and the
default against transform_ref, surface_distances against surface_distances_ref (the restatements of test_distance_host.py), every
transform twice into a garbage-filled volume with guard words on both sides; then qc.surface_qc against the restatement on the same
run's argmax maps.  Every comparison is exact equality of bytes.  Shapes are (D, H, W)."""
import os
import sys
import threading

import numpy as np
import pytest
import torch

import unet_studio_amd as U
from unet_studio_amd import distance as DS
from unet_studio_amd import qc as Q

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_distance_host import ball, blobs, surface_distances_ref, surface_ref, transform_ref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
IMPLS = (DS.IMPL_LDS, DS.IMPL_GLOBAL, DS.IMPL_DEFAULT)
# line lengths on both sides of a 64-bit mask word (63, 64, 65, 130) and of a slab width (33, 40), a line longer than a block's threads
SHAPES = [(1, 1, 1), (1, 1, 130), (3, 5, 7), (2, 65, 63), (66, 3, 64), (9, 9, 33), (2, 3, 300), (38, 44, 40)]
G = 64                                                             # guard words on each side of out
GUARD = -0x5A3C5A3D
INF = DS.INF


def dev_map(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a).astype(np.int32)).to(DEV).to(dtype)


def same(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()


def guarded(n, rep):
    """an int32 buffer of G + n + G words: guards outside, garbage inside; -> (buffer, the view a call writes)"""
    buf = torch.full((n + 2 * G,), GUARD, dtype=torch.int32, device=DEV)
    buf[G:G + n] = 0x7B7B7B7B if rep == 0 else -3
    return buf, buf[G:G + n]


def guards_intact(buf, n):
    b = buf.cpu().numpy()
    return (b[:G] == GUARD).all() and (b[G + n:] == GUARD).all()


# ---- the maps: rng, (D, H, W) -> labels; the label under test is 2 ------------------------------------------------------------------
def corners(rng, shape):
    """one voxel in each of two opposite corners: the outward search walks a whole line"""
    m = np.zeros(shape, np.int64)
    m[0, 0, 0] = m[-1, -1, -1] = 2
    return m


def solid(rng, shape):
    return np.full(shape, 2, np.int64)


def absent(rng, shape):
    """no voxel reads the label: INF everywhere"""
    return rng.integers(0, 2, shape) * 3


def checker(rng, shape):
    return np.indices(shape).sum(axis=0) % 2 * 2


def random_blobs(rng, shape):
    return np.where(blobs(rng, shape), 2, rng.integers(0, 2, shape) * 7)


def enclosed(rng, shape):
    """label 1 encloses label 2: 2 touches no background, and 1 has an inner and an outer surface"""
    D, H, W = shape
    c = ((W - 1) / 2, (H - 1) / 2, (D - 1) / 2)
    m = np.zeros(shape, np.int64)
    m[ball(shape, c, 0.45 * max(shape))] = 1
    m[ball(shape, c, 0.2 * max(shape))] = 2
    return m


KINDS = (corners, solid, absent, checker, random_blobs, enclosed)
REFS = {}                                                          # a reference is computed once and shared


def ref(kind, shape, weights, of, label=2):
    key = (kind.__name__, shape, weights, of, label)
    if key not in REFS:
        REFS[key] = transform_ref(kind(np.random.default_rng(shape[2]), shape), label, weights, of)
    return REFS[key]


def check_transform(labels, want, label, weights, of, dtype):
    lab = dev_map(labels, dtype)
    n = labels.size
    for impl in IMPLS:
        for rep in range(2):
            buf, out = guarded(n, rep)
            got = DS.transform(lab, label, weights, of=of, impl=impl, out=out)
            assert got.data_ptr() == out.data_ptr() and tuple(got.shape) == labels.shape
            assert same(got.cpu().numpy(), want), (impl, rep, of, int((got.cpu().numpy() != want).sum()))
            assert guards_intact(buf, n)


@pytest.mark.parametrize("weights", [(1, 1, 1), (4, 9, 25)])
@pytest.mark.parametrize("shape", SHAPES)
def test_transform_shapes_weights_and_maps(shape, weights):
    for k, kind in enumerate(KINDS):
        labels = kind(np.random.default_rng(shape[2]), shape)
        for j, of in enumerate(("surface", "label")):
            dtype = (torch.uint8, torch.uint16)[(k + j) % 2]        # every kind sees both types
            want = ref(kind, shape, weights, of)
            check_transform(labels, want, 2, weights, of, dtype)
            if kind is absent:
                assert (want == INF).all()
            if kind is enclosed and min(shape) > 8:                  # the enclosing label too: features on both sides of a voxel
                check_transform(labels, ref(kind, shape, weights, of, 1), 1, weights, of, dtype)


def test_transform_under_the_finest_weights_of_an_anisotropic_grid():
    shape, weights = (5, 6, 7), (1024, 1531, 9216)
    for kind in KINDS:
        labels = kind(np.random.default_rng(7), shape)
        for of in ("surface", "label"):
            check_transform(labels, transform_ref(labels, 2, weights, of), 2, weights, of, torch.uint8)
    # at the edge of the metric bound the corner-to-corner distance is the largest int32 below INF
    shape = (7, 5, 3)
    weights = (4, 9, 59652319)
    assert DS.metric_bound(weights, shape[::-1]) == INF - 3
    labels = np.zeros(shape, np.int64)
    labels[0, 0, 0] = 2
    want = transform_ref(labels, 2, weights, "label")
    assert want[-1, -1, -1] == INF - 3
    check_transform(labels, want, 2, weights, "label", torch.uint16)
    with pytest.raises(U.UNetError, match="weights"):
        DS.transform(dev_map(labels, torch.uint8), 2, (4, 9, 59652320))
    with pytest.raises(U.UNetError, match="weights"):
        DS.transform(dev_map(labels, torch.uint8), 2, (1, 0, 1))


def test_a_label_above_what_a_uint8_map_holds_and_other_labels_do_not_matter():
    rng = np.random.default_rng(5)
    shape = (9, 9, 33)
    labels = np.where(blobs(rng, shape), 700, rng.integers(0, 65536, shape))
    labels[labels == 2] = 0
    want = transform_ref(labels, 700, (1, 1, 1), "surface")
    check_transform(labels, want, 700, (1, 1, 1), "surface", torch.uint16)
    as8 = dev_map(labels & 0xFF, torch.uint8)                       # 700 is not a value of a uint8 map: INF everywhere
    assert (DS.transform(as8, 700, (1, 1, 1)).cpu().numpy() == INF).all()


@pytest.mark.parametrize("off", [1, 3])
@pytest.mark.parametrize("nbytes", [1, 2])
def test_map_pointers_off_alignment(nbytes, off):
    rng = np.random.default_rng(20 + off)
    shape, weights = (9, 9, 33), (4, 9, 25)
    a, b = random_blobs(rng, shape), enclosed(rng, shape)
    np_dt = np.uint8 if nbytes == 1 else np.uint16
    bufs = []
    for img in (a, b):                                              # the map's bytes at an odd address inside a byte buffer
        raw = np.frombuffer(img.astype(np_dt).tobytes(), np.uint8)
        buf = torch.full((raw.size + 16,), 0xEE, dtype=torch.uint8, device=DEV)
        buf[off:off + raw.size] = torch.from_numpy(raw.copy()).to(DEV)
        assert (buf.data_ptr() + off) % 2 == 1
        bufs.append(buf)
    D, H, W = shape
    need = DS.distance_scratch_bytes((W, H, D))
    scratch = torch.empty(need + 8, dtype=torch.uint8, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    lib = U.engine.lib
    want = transform_ref(a, 2, weights, "surface")
    L = 300
    want_counts = surface_distances_ref(a, b, L, weights, labels=[])["counts"]
    want_list = np.sort(want[surface_ref(b == 2)])
    for impl in IMPLS:
        for rep in range(2):
            buf, out = guarded(a.size, rep)                         # the scratch off alignment too
            U.engine.check(lib.unet_dist_transform(bufs[0].data_ptr() + off, nbytes, W, H, D, 2, DS.OF_SURFACE, *weights, out.data_ptr(), impl,
                                                   scratch.data_ptr() + off, need, stream))
            assert same(out.cpu().numpy().reshape(shape), want) and guards_intact(buf, a.size)
            # the gather at b's surface of what was just written; a capacity below the count is never overrun
            for capacity in (want_list.size, want_list.size - 5):
                vbuf, values = guarded(want_list.size, rep)
                cursor = torch.zeros(1, dtype=torch.int64, device=DEV)
                U.engine.check(lib.unet_dist_gather(bufs[1].data_ptr() + off, nbytes, W, H, D, 2, out.data_ptr(), values.data_ptr(), capacity,
                                                    cursor.data_ptr(), stream))
                assert int(cursor.item()) == want_list.size and guards_intact(vbuf, want_list.size)
                got = values.cpu().numpy()
                if capacity == want_list.size:
                    assert same(np.sort(got), want_list)
                else:
                    assert (got[capacity:] == (0x7B7B7B7B if rep == 0 else -3)).all()
    rows = torch.full(((L + 1) * 2 + 2,), -7, dtype=torch.int64, device=DEV)
    U.engine.check(lib.unet_dist_surface_counts(bufs[0].data_ptr() + off, nbytes, bufs[1].data_ptr() + off, nbytes, W, H, D, L,
                                                rows.data_ptr() + 8, stream))
    got = rows.cpu().numpy()
    assert got[0] == got[-1] == -7 and same(got[1:-1].reshape(L + 1, 2), want_counts)


# ---- surface_distances -------------------------------------------------------------------------------------------------------------
def same_result(got, want):
    assert same(got["counts"], want["counts"])
    assert sorted(got["values"]) == sorted(want["values"])
    for l in want["values"]:
        for g, w in zip(got["values"][l], want["values"][l]):
            assert same(g, w), l


def random_maps(seed=11):
    """two maps of 5 labels at (20, 22, 24), mostly agreeing; label 4 is missing from a, 5 from b, and values above 5 read as 0"""
    rng = np.random.default_rng(seed)
    shape = (20, 22, 24)
    z, y, x = np.indices(shape)
    a = (x // 7 + 2 * (y // 12) + (z // 11)) % 6
    b = np.where(blobs(rng, shape, 0.55), (a + 1) % 6, a)
    a[a == 4] = 0
    b[b == 5] = 9                                                   # above n_labels: reads 0
    return a, b


def shifted_balls():
    shape = (38, 44, 40)
    a, b = np.zeros(shape, np.int64), np.zeros(shape, np.int64)
    a[ball(shape, (18, 20, 17), 12)] = 1
    b[ball(shape, (22, 23, 19), 13)] = 1
    a[ball(shape, (18, 20, 17), 5)] = 2                             # in a only
    return a, b


@pytest.mark.parametrize("weights", [(1, 1, 1), (4, 4, 9)])
def test_surface_distances_equal_the_restatement(weights):
    a, b = random_maps()
    want = surface_distances_ref(a, b, 5, weights)
    assert sorted(want["values"]) == [1, 2, 3] and want["counts"][4, 0] == 0 < want["counts"][4, 1] and want["counts"][5, 1] == 0 < want["counts"][5, 0]
    a_dev, b_dev = dev_map(a, torch.uint8), dev_map(b, torch.uint16)
    for impl in IMPLS:
        for rep in range(2):                                        # the call twice: the same bytes
            same_result(DS.surface_distances(a_dev, b_dev, 5, weights, impl=impl), want)
    assert same(DS.surface_counts(a_dev, b_dev, 5).cpu().numpy(), want["counts"])
    part = DS.surface_distances(a_dev, b_dev, 5, weights, labels=[3, 4])
    same_result(part, surface_distances_ref(a, b, 5, weights, labels=[3, 4]))
    assert sorted(part["values"]) == [3]
    table = DS.summary(DS.surface_distances(a_dev, b_dev, 5, weights), 0.25)
    assert np.array_equal(table, DS.summary(want, 0.25), equal_nan=True) and np.isinf(table[4:6]).all() and np.isfinite(table[1:4]).all()


def test_surface_distances_of_two_shifted_balls_and_missing_labels():
    a, b = shifted_balls()
    want = surface_distances_ref(a, b, 3, (1, 1, 1))
    assert sorted(want["values"]) == [1] and want["counts"][2, 1] == 0 < want["counts"][2, 0] and want["counts"][3].tolist() == [0, 0]
    a_dev, b_dev = dev_map(a, torch.uint8), dev_map(b, torch.uint8)
    for impl in IMPLS:
        same_result(DS.surface_distances(a_dev, b_dev, 3, (1, 1, 1), impl=impl), want)
    table = DS.summary(want, 1.0)
    assert np.isinf(table[2]).all() and np.isnan(table[3]).all() and 0 < table[1, 2] < table[1, 1] <= table[1, 0]
    # nothing to measure: no list, the counts still filled
    none = DS.surface_distances(a_dev, b_dev, 3, (1, 1, 1), labels=[2, 3])
    assert none["values"] == {} and same(none["counts"], want["counts"])


def test_surface_distances_with_300_labels_needs_an_explicit_list():
    a, b = random_maps(12)
    a, b = a * 59, b * 59                                           # 59, 118, 177, 236 (a: not), 295 (b: reads 9 * 59 = 531 > 300)
    a[0, 0, :3] = 300
    b[0, 0, 1:5] = 300
    a_dev, b_dev = dev_map(a, torch.uint16), dev_map(b, torch.uint16)
    with pytest.raises(U.UNetError, match="explicit list"):
        DS.surface_distances(a_dev, b_dev, 300, (1, 1, 1))
    labels = [300, 59, 236, 295, 7, 118]
    want = surface_distances_ref(a, b, 300, (1, 1, 1), labels=labels)
    assert sorted(want["values"]) == [59, 118, 300]
    for impl in IMPLS:
        same_result(DS.surface_distances(a_dev, b_dev, 300, (1, 1, 1), labels=labels, impl=impl), want)
    # rows at and above the LDS table's last: the same counts with n_labels = 2035, ids on both sides of row 1024
    a2, b2 = a.copy(), b.copy()
    for v, to in ((59, DS.LDS_ROWS - 1), (118, DS.LDS_ROWS), (177, 2035)):
        a2[a == v], b2[b == v] = to, to
    want2 = surface_distances_ref(a2, b2, 2035, (1, 1, 1), labels=[DS.LDS_ROWS - 1, DS.LDS_ROWS, 2035])
    assert sorted(want2["values"]) == [DS.LDS_ROWS - 1, DS.LDS_ROWS, 2035]
    same_result(DS.surface_distances(dev_map(a2, torch.uint16), dev_map(b2, torch.uint16), 2035, (1, 1, 1),
                                     labels=[DS.LDS_ROWS - 1, DS.LDS_ROWS, 2035]), want2)
    for bad in ([0], [301], [59, 59]):
        with pytest.raises(U.UNetError, match="labels must be"):
            DS.surface_distances(a_dev, b_dev, 300, (1, 1, 1), labels=bad)


def test_two_threads_on_two_streams_with_their_own_scratch():
    cases, errors = [], []
    for seed, weights in ((1, (1, 1, 1)), (2, (4, 4, 9))):
        a, b = random_maps(seed)
        cases.append((dev_map(a, torch.uint8), dev_map(b, torch.uint8), weights, surface_distances_ref(a, b, 5, weights)))
    torch.cuda.synchronize()

    def work(k):
        try:
            a, b, weights, want = cases[k]
            stream = torch.cuda.Stream(device=DEV)
            with torch.cuda.stream(stream):
                scratch = torch.empty(DS.distance_scratch_bytes(a.shape[::-1]), dtype=torch.uint8, device=DEV)
                for rep in range(3):
                    same_result(DS.surface_distances(a, b, 5, weights, impl=IMPLS[rep], scratch=scratch), want)
        except BaseException as e:  # noqa: BLE001
            errors.append((k, repr(e)))

    threads = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors


# ---- qc.surface_qc -------------------------------------------------------------------------------------------------------------------
SMOKE_ARCH = ("conv8,ks3,stride1+norm,leaky_relu+conv8,ks3,stride1+norm,leaky_relu\n"
              "conv16,ks3,stride2+norm,leaky_relu+conv16,ks3,stride1+norm,leaky_relu+conv_trans8,ks2,stride2\n"
              "conv8,ks3,stride1+norm,leaky_relu+conv8,ks3,stride1+norm,leaky_relu+conv%d,ks1,stride1")


def test_surface_qc_report_equals_the_restatement_on_the_same_argmax_maps(tmp_path):
    dim, C = (24, 16, 20), 6
    W, H, D = dim
    m = U.UNet3d(1, C, SMOKE_ARCH % C, device=DEV, dtype="fp32", seed=9)
    m.dim, m.voxel_size = dim, (1.0, 1.0, 2.5)
    m.prepare_for_inference()
    g = torch.Generator().manual_seed(3)

    def vol(max_label):
        lab = torch.randint(0, max_label + 1, (D, H, W), generator=g).to(torch.float32)
        lab[torch.rand(D, H, W, generator=g) < 0.4] = 0.0
        lab.view(-1)[0] = max_label
        return torch.randn(1, D, H, W, generator=g).numpy(), lab.numpy()

    cases = [("/data/tpl/t0_T1w.nii.gz", "/data/tpl/t0_label.nii.gz") + vol(2) + (True,),
             ("/data/sub-01/anat/sub-01_T1w.nii.gz", "/data/sub-01/anat/sub-01_dseg.nii.gz") + vol(1) + (False,),     # 1 < 2, 1 + 2 < 6: shifted
             ("/data/sub-02/anat/sub-02_T1w.nii.gz", "/data/sub-02/anat/sub-02_dseg.nii.gz") + vol(4) + (False,)]
    mtl, shift = Q.label_plan(cases, C)
    assert mtl == 2 and shift == [False, True, False]
    path = str(tmp_path / "qc_model.nz")
    error_report = str(tmp_path / "qc_model.error_report.tsv")
    assert Q.run_qc(m, path, cases) == (0, error_report)
    before = open(error_report, "rb").read()

    report = str(tmp_path / "qc_model.surface_report.tsv")
    assert Q.surface_qc(m, path, cases) == (0, report)
    got = open(report, "rb").read()
    assert sorted(os.listdir(tmp_path)) == ["qc_model.error_report.tsv", "qc_model.surface_report.tsv"]      # no .tmp left behind
    # the restatement on the argmax maps of a second forward of the same model: the engine's fp32 forward is deterministic
    weights, unit = DS.metric(m.voxel_size, dim)
    assert weights != (1, 1, 1) and DS.metric_bound(weights, dim) < INF
    rows = []
    for c, sh in zip(cases, shift):
        summary = None
        if not sh:
            x = torch.from_numpy(c[2]).view(1, 1, D, H, W).to(DEV)
            pred = torch.argmax(m._forward_level0(x)[0], dim=0).cpu().numpy()
            summary = DS.summary(surface_distances_ref(pred, c[3].astype(np.int64), C - 1, weights), unit)
        rows.append((c[0], c[1], summary))
    assert Q.format_surface_report(C, rows).encode() == got
    lines = got.decode().splitlines()
    assert len(lines) == 4 and lines[0].split("\t")[:5] == ["image", "ground_truth", "hd1", "hd951", "assd1"]
    assert lines[2].split("\t") == ["sub-01_T1w.nii.gz", "sub-01_dseg.nii.gz"] + ["N/A"] * (3 * (C - 1)) and "N/A" not in lines[1] + lines[3]
    # a subset of the classes: the others read nan
    assert Q.surface_qc(m, path, cases, labels=[2]) == (0, report)
    cols = open(report).read().splitlines()[1].split("\t")
    assert cols[2:5] == ["nan"] * 3 and cols[5:8] == lines[1].split("\t")[5:8]
    # run_qc on the same cases still writes the same error report
    assert Q.run_qc(m, path, cases) == (0, error_report) and open(error_report, "rb").read() == before
