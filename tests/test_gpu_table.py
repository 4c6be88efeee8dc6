"""GPU: the tables of a label map on the device (include/unet_table.h) -- regions and overlap under IMPL_LDS, IMPL_GLOBAL and the
default against regions_ref and overlap_ref (the restatements of test_table_host.py), every case twice into garbage-filled rows with
guard words on both sides; then the atlas stage of EvaluateUNet against register.parcellate and table.regions called by hand on
the same run's label.  Every comparison is exact equality of bytes.  Shapes are (D, H, W)."""
import os
import sys
import threading

import numpy as np
import pytest
import torch

import unet_studio_amd as U
from unet_studio_amd import atlas as A
from unet_studio_amd import register as R
from unet_studio_amd import table as T

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_table_host import overlap_ref, regions_ref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F = np.float32
IMPLS = (T.IMPL_LDS, T.IMPL_GLOBAL, T.IMPL_DEFAULT)
SHAPES = [(1, 1, 1), (3, 5, 7), (9, 9, 33), (2, 3, 65), (2, 3, 70000), (38, 44, 40)]
LABELS = [1, 255, T.LDS_ROWS - 1, T.LDS_ROWS, T.LDS_ROWS + 1, 65535]
G = 64                                                             # guard words on each side of rows
GUARD = -0x5A3C5A3C5A3C5A3D


def dev_map(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a).astype(np.int32)).to(DEV).to(dtype)


def same(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()


def guarded(n, rep):
    """an int64 buffer of G + n + G words: guards outside, garbage inside; -> (buffer, the view a call writes)"""
    buf = torch.full((n + 2 * G,), GUARD, dtype=torch.int64, device=DEV)
    buf[G:G + n] = 0x7B7B7B7B7B7B7B7B if rep == 0 else -3
    return buf, buf[G:G + n]


def guards_intact(buf, n):
    b = buf.cpu().numpy()
    return (b[:G] == GUARD).all() and (b[G + n:] == GUARD).all()


# ---- the maps: rng, (D, H, W), n_labels, the largest value the element type holds -> labels ------------------------------------------
def one_label(rng, shape, L, vmax):
    """every update contends for one row"""
    return np.full(shape, min(L, vmax), np.int64)


def thirds(rng, shape, L, vmax):
    """solid thirds along x: long runs, the first, a middle and the last label"""
    top = min(L, vmax)
    x = np.indices(shape)[2]
    return np.asarray([1, top // 2 + 1, top])[np.minimum(x * 3 // max(shape[2], 1), 2)].astype(np.int64)


def uniform(rng, shape, L, vmax):
    return rng.integers(0, min(L, vmax) + 1, shape)


def sparse(rng, shape, L, vmax):
    """a handful of ids on both sides of the LDS table's last row, in short runs"""
    ids = np.asarray([v for v in (0, 1, 77, T.LDS_ROWS - 1, T.LDS_ROWS, T.LDS_ROWS + 1, 2035, L) if v <= min(L, vmax)])
    return np.repeat(rng.choice(ids, int(np.prod(shape)) // 3 + 1), 3)[:int(np.prod(shape))].reshape(shape)


def above(rng, shape, L, vmax):
    """values the type can hold and n_labels cannot: they read 0"""
    return rng.integers(0, vmax + 1, shape)


KINDS = (one_label, thirds, uniform, sparse, above)


def check_regions(labels, L, dtype, impls=IMPLS):
    want = regions_ref(labels, L)
    lab = dev_map(labels, dtype)
    n = (L + 1) * 10
    for impl in impls:
        for rep in range(2):
            buf, out = guarded(n, rep)
            got = T.regions(lab, L, impl=impl, out=out)
            assert got.data_ptr() == out.data_ptr() and tuple(got.shape) == (L + 1, 10)
            assert same(got.cpu().numpy(), want), (impl, rep)
            assert guards_intact(buf, n)
    assert int(want[:, 0].sum()) == labels.size
    return want


def check_overlap(a, b, L, adt, bdt, impls=IMPLS):
    want = overlap_ref(a, b, L)
    a_dev, b_dev = dev_map(a, adt), dev_map(b, bdt)
    n = (L + 1) * 3
    for impl in impls:
        for rep in range(2):
            buf, out = guarded(n, rep)
            got = T.overlap(a_dev, b_dev, L, impl=impl, out=out)
            assert got.data_ptr() == out.data_ptr() and same(got.cpu().numpy(), want), (impl, rep)
            assert guards_intact(buf, n)
    assert int(want[:, 0].sum()) == int(want[:, 1].sum()) == a.size
    return want


# ---- regions and overlap -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_regions_shapes_label_counts_and_maps(shape):
    rng = np.random.default_rng(shape[2])
    for i, L in enumerate(LABELS):
        for k, make in enumerate(KINDS):
            dtype, vmax = ((torch.uint8, 255), (torch.uint16, 65535))[(i + k) % 2]     # every kind and every L sees both types
            want = check_regions(make(rng, shape, L, vmax), L, dtype)
            if shape == (2, 3, 70000) and make is one_label:
                assert want[min(L, vmax), 1] == 6 * (70000 * 69999 // 2) > 2 ** 32


@pytest.mark.parametrize("shape", SHAPES)
def test_overlap_shapes_label_counts_and_maps(shape):
    rng = np.random.default_rng(100 + shape[2])
    types = ((torch.uint8, 255), (torch.uint16, 65535))
    for i, L in enumerate(LABELS):
        for k, make in enumerate(KINDS):
            (adt, amax), (bdt, bmax) = types[(i + k) % 2], types[(i + k // 2) % 2]
            a = make(rng, shape, L, amax)
            b = np.where(rng.random(shape) < 0.7, np.minimum(a, bmax), KINDS[(k + 2) % 5](rng, shape, L, bmax))   # mostly agreeing
            check_overlap(a, b, L, adt, bdt)


@pytest.mark.parametrize("bdt", [torch.uint8, torch.uint16])
@pytest.mark.parametrize("adt", [torch.uint8, torch.uint16])
def test_uint8_and_uint16_maps_and_the_two_mixed(adt, bdt):
    rng = np.random.default_rng(3)
    shape = (9, 9, 33)
    amax, bmax = (255 if t == torch.uint8 else 65535 for t in (adt, bdt))
    for L in (5, 255, 2035):                                        # more labels than a uint8 map can hold is allowed
        a, b = thirds(rng, shape, L, amax), above(rng, shape, L, bmax)
        b[rng.random(shape) < 0.5] = 0
        want = check_overlap(a, b, L, adt, bdt)
        assert want[1, 0] > 0 and want[1:, 2].sum() >= 0
        check_overlap(a, np.minimum(a, bmax), L, adt, bdt)
        if adt == bdt:
            check_regions(a, L, adt)
            check_regions(b, L, bdt)


@pytest.mark.parametrize("off", [1, 3])
@pytest.mark.parametrize("nbytes", [1, 2])
def test_map_pointers_off_alignment(nbytes, off):
    rng = np.random.default_rng(20 + off)
    shape, L = (9, 9, 33), T.LDS_ROWS + 1
    vmax = 255 if nbytes == 1 else 65535
    a, b = sparse(rng, shape, L, vmax), above(rng, shape, L, vmax)
    np_dt = np.uint8 if nbytes == 1 else np.uint16
    bufs = []
    for img in (a, b):                                              # the map's bytes at an odd address inside a byte buffer
        raw = np.frombuffer(img.astype(np_dt).tobytes(), np.uint8)
        buf = torch.full((raw.size + 16,), 0xEE, dtype=torch.uint8, device=DEV)
        buf[off:off + raw.size] = torch.from_numpy(raw.copy()).to(DEV)
        assert (buf.data_ptr() + off) % 2 == 1
        bufs.append(buf)
    need = T.table_scratch_bytes(a.size, L)
    scratch = torch.empty(need + 8, dtype=torch.uint8, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    lib = U.engine.lib
    want_r, want_o = regions_ref(a, L), overlap_ref(a, b, L)
    for impl in IMPLS:
        for rep in range(2):
            buf, out = guarded((L + 1) * 10, rep)                   # the scratch off alignment too
            U.engine.check(lib.unet_table_regions(bufs[0].data_ptr() + off, nbytes, shape[2], shape[1], shape[0], L, out.data_ptr(), impl,
                                                  scratch.data_ptr() + off, need, stream))
            assert same(out.cpu().numpy().reshape(L + 1, 10), want_r) and guards_intact(buf, (L + 1) * 10)
            buf, out = guarded((L + 1) * 3, rep)
            U.engine.check(lib.unet_table_overlap(bufs[0].data_ptr() + off, nbytes, bufs[1].data_ptr() + off, nbytes, a.size, L, out.data_ptr(),
                                                  impl, scratch.data_ptr() + off, need, stream))
            assert same(out.cpu().numpy().reshape(L + 1, 3), want_o) and guards_intact(buf, (L + 1) * 3)


def test_two_threads_on_two_streams_with_their_own_scratch():
    cases, errors = [], []
    for seed, L in ((1, 400), (2, 2035)):
        rng = np.random.default_rng(seed)
        a, b = thirds(rng, (38, 44, 40), L, 65535), uniform(rng, (38, 44, 40), L, 65535)
        cases.append((dev_map(a, torch.uint16), dev_map(b, torch.uint16), L, regions_ref(a, L), overlap_ref(a, b, L)))
    torch.cuda.synchronize()

    def work(k):
        try:
            a, b, L, want_r, want_o = cases[k]
            stream = torch.cuda.Stream(device=DEV)
            with torch.cuda.stream(stream):
                scratch = torch.empty(T.table_scratch_bytes(a.numel(), L), dtype=torch.uint8, device=DEV)
                for rep in range(3):
                    rows = T.regions(a, L, impl=IMPLS[rep], scratch=scratch, stream=stream.cuda_stream)
                    rows3 = T.overlap(a, b, L, impl=IMPLS[rep], scratch=scratch, stream=stream.cuda_stream)
                    stream.synchronize()
                    assert same(rows.cpu().numpy(), want_r) and same(rows3.cpu().numpy(), want_o)
        except BaseException as e:  # noqa: BLE001
            errors.append((k, repr(e)))

    threads = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors


def test_the_host_arithmetic_on_device_rows():
    a = thirds(np.random.default_rng(0), (3, 5, 7), 3, 255)
    rows = T.regions(dev_map(a, torch.uint8), 3)
    want = regions_ref(a, 3)
    assert T.volumes_mm3(rows, (2, 1, 0.5)).tolist() == want[:, 0].astype(np.float64).tolist()
    c = T.centroids(rows)
    assert np.isnan(c[0]).all() and c[1].tolist() == (want[1, 1:4] / want[1, 0]).tolist()
    assert T.dice(T.overlap(dev_map(a, torch.uint8), dev_map(a, torch.uint16), 3)).tolist()[1:] == [1.0, 1.0, 1.0]


# ---- the atlas stage of EvaluateUNet -------------------------------------------------------------------------------------------------
SMOKE_ARCH = ("conv8,ks3,stride1+norm,leaky_relu+conv8,ks3,stride1+norm,leaky_relu\n"
              "conv16,ks3,stride2+norm,leaky_relu+conv16,ks3,stride1+norm,leaky_relu+conv_trans8,ks2,stride2\n"
              "conv8,ks3,stride1+norm,leaky_relu+conv8,ks3,stride1+norm,leaky_relu+conv%d,ks1,stride1")
OUT_C = 5                                                          # the background and the four tissues of the template
CHAIN_OUTPUTS = ("label", "fg_prob", "label_prob")
OPTIONS = dict(max_iterations=40)                                  # only determinism is claimed: a short search suffices


def ellipsoid_template():
    """uint8 (36, 48, 40): nested ellipsoids, tissues 1-4 (the template of the register tests, restated)"""
    D, H, W = 36, 48, 40
    z, y, x = np.meshgrid(np.arange(D), np.arange(H), np.arange(W), indexing="ij")
    d = ((x - 19.5) / 15) ** 2 + ((y - 23.5) / 19) ** 2 + ((z - 17.5) / 14) ** 2
    template = np.zeros((D, H, W), np.uint8)
    template[d < 1] = 2
    template[d < 0.6] = 1
    template[d < 0.15] = 4
    template[(d < 1) & (z < 17.5 - 0.55 * 14)] = 3
    return template


def hist_ref(subject, template, T_, map12):
    """int64 {T, T}: hist[a][b] = the subject voxels with tissue a whose nearest template sample under the map reads b (the
    definition of include/unet_register.h restated: fp32, left to right, one rounding per operation, q = p + 0.5, inside when
    0 <= q < float(dim))"""
    s, t = (np.where(np.asarray(v).astype(np.int64) >= T_, 0, np.asarray(v).astype(np.int64)) for v in (subject, template))
    m = np.asarray(map12, F).reshape(12)
    z, y, x = (v.reshape(-1).astype(F) for v in np.indices(s.shape))
    q = [(((m[3 * r] * x + m[3 * r + 1] * y) + m[3 * r + 2] * z) + m[9 + r]) + F(0.5) for r in range(3)]
    assert all(v.dtype == F for v in q)
    inside = np.ones(x.shape, bool)
    idx = []
    for v, dim in zip(q, t.shape[::-1]):
        inside &= (v >= F(0)) & (v < F(dim))
        idx.append(np.where(inside, np.floor(v), 0).astype(np.int64))
    b = np.where(inside, t[np.where(inside, idx[2], 0), np.where(inside, idx[1], 0), np.where(inside, idx[0], 0)], 0)
    return np.bincount(s.reshape(-1) * T_ + b, minlength=T_ * T_).reshape(T_, T_).astype(np.int64)


def make_atlas():
    template = ellipsoid_template()
    z, y, x = np.indices(template.shape)
    raw = np.where(template > 0, 1 + (x > 14).astype(np.int64) + (x + y > 50) + 3 * (z > 20) + 6 * (template == 4), 0)   # cut by planes
    t_dev = dev_map(template, torch.uint8)
    regions, rep = A.prepare_atlas(t_dev, dev_map(raw, torch.uint16), 5)
    atlas = R.Atlas(t_dev, (1, 1, 1), regions)
    assert 1 <= atlas.n_regions <= rep["n_regions"] == int(raw.max()) and atlas.n_tissues == 5 and atlas.template_vs == (1.0, 1.0, 1.0)
    return atlas, template


def small_model():
    m = U.UNet3d(1, OUT_C, SMOKE_ARCH % OUT_C, device=DEV, dtype="fp32", seed=2)
    m.dim, m.voxel_size = (16, 16, 16), (2.0, 2.0, 2.0)
    return m


def inputs():
    rs = np.random.RandomState(4)
    return {"plain": (rs.rand(16, 16, 16).astype(F), None, (2.0, 2.0, 2.0)),
            "native": (U.NativeVolume(rs.rand(14, 15, 17).astype(F), (2.0, 2.2, 1.8)), None, (2.0, 2.2, 1.8)),
            "tiles": (rs.rand(16, 18, 25).astype(F), "tiles", (2.0, 2.0, 2.0))}


@pytest.mark.parametrize("kind", ["plain", "native", "tiles"])
def test_evaluate_atlas_and_regions_equal_the_stages_called_by_hand(kind):
    atlas, template = make_atlas()
    m = small_model()
    io, fov, vs = inputs()[kind]
    ev = U.EvaluateUNet(m, postproc="model", outputs=CHAIN_OUTPUTS + ("atlas", "regions"), fov_strategy=fov, atlas=atlas,
                        atlas_options=OPTIONS)
    got = ev.start([[io]])[0][0]
    assert not ev.aborted and ev.error_msg == ""
    plain = U.EvaluateUNet(m, postproc="model", outputs=CHAIN_OUTPUTS, fov_strategy=fov)
    base = plain.start([[io]])[0][0]
    assert not plain.aborted
    for k in CHAIN_OUTPUTS:                                         # the chain's outputs do not know about the stage
        assert same(got[k], base[k]), k
    shape = got["label"].shape
    assert shape == ((io.data if kind == "native" else io).shape)
    # the stages by hand on this run's label, with the voxel size the loop must have used
    label = dev_map(got["label"], torch.uint16)
    parc, report = R.parcellate(label, vs, atlas.template, atlas.template_vs, atlas.regions, 5, **OPTIONS)
    want_atlas = parc.view(torch.int16).cpu().numpy().view(np.uint16)
    assert got["atlas"].dtype == np.uint16 and same(np.ascontiguousarray(got["atlas"]), want_atlas)
    assert (want_atlas[got["label"] == 0] == 0).all()
    reg = got["regions"]
    assert sorted(reg) == ["report", "table", "tissue_dice", "volume_mm3"]
    want_table = T.regions(parc, atlas.n_regions).cpu().numpy()
    assert same(np.ascontiguousarray(reg["table"]), want_table) and same(want_table, regions_ref(want_atlas, atlas.n_regions))
    assert same(reg["volume_mm3"], want_table[:, 0].astype(np.float64) * (vs[0] * vs[1] * vs[2]))
    for k in ("iterations", "converged", "score", "rounds", "grow_converged"):
        assert reg["report"][k] == report[k], k
    for k in ("direct", "rescued", "left", "filled"):
        assert same(reg["report"][k], report[k]), k
    assert same(np.concatenate(reg["report"]["map"]), np.concatenate(report["map"]))
    # tissue_dice from the restated histogram at the map found, to the last bit
    h = hist_ref(got["label"], template, 5, np.concatenate(report["map"]))
    agree, both = int(np.trace(h)) - int(h[0, 0]), int(h[1:].sum()) + int(h[:, 1:].sum())
    assert both > 0 and isinstance(reg["tissue_dice"], np.float64)
    assert np.float64(reg["tissue_dice"]).tobytes() == np.float64(2.0 * agree / both).tobytes()


def test_evaluate_wanting_only_regions_copies_back_no_volume_and_init_is_honoured():
    atlas, template = make_atlas()
    m = small_model()
    io = inputs()["plain"][0]
    init = [2, 0, 0, 0, 2, 0, 0, 0, 2, 3.5, 8.0, 2.5]
    ev = U.EvaluateUNet(m, postproc="model", outputs=("regions",), atlas=atlas, atlas_options=dict(OPTIONS, init=init))
    got = ev.start([[io], [io]])
    assert not ev.aborted and ev.error_msg == "" and ev.cur_prog == 2
    for res in (got[0][0], got[1][0]):
        assert sorted(res) == ["regions"] and sorted(res["regions"]) == ["report", "table", "tissue_dice", "volume_mm3"]
        assert all(np.asarray(v).size < io.size for v in (res["regions"]["table"], res["regions"]["volume_mm3"]))
    assert same(np.ascontiguousarray(got[0][0]["regions"]["table"]), np.ascontiguousarray(got[1][0]["regions"]["table"]))
    full = U.EvaluateUNet(m, postproc="model", outputs=("label", "regions"), atlas=atlas, atlas_options=dict(OPTIONS, init=init))
    ref = full.start([[io]])[0][0]
    label = dev_map(ref["label"], torch.uint16)
    parc, report = R.parcellate(label, m.voxel_size, atlas.template, atlas.template_vs, atlas.regions, 5, init=init, **OPTIONS)
    assert same(np.ascontiguousarray(got[0][0]["regions"]["table"]), T.regions(parc, atlas.n_regions).cpu().numpy())
    assert same(np.concatenate(got[0][0]["regions"]["report"]["map"]), np.concatenate(report["map"]))


def test_atlas_record_argument_errors():
    template = dev_map(ellipsoid_template(), torch.uint8)
    regions = torch.zeros(template.shape, dtype=torch.uint16, device=DEV)
    assert R.Atlas(template, (1, 2, 3), regions).n_regions == 1     # an empty atlas still has a row beside the background
    assert R.Atlas(template, (1, 2, 3), regions, n_regions=2035).n_regions == 2035
    for kw, msg in ((dict(regions=regions[:-1].contiguous()), "regions must be"), (dict(regions=regions.to(torch.int32)), "regions must be"),
                    (dict(template_vs=(1, 1)), "template_vs"), (dict(template_vs=(1, 0, 1)), "template_vs"),
                    (dict(template_vs="abc"), "template_vs"), (dict(n_tissues=1), "n_tissues"), (dict(n_tissues=17), "n_tissues"),
                    (dict(n_regions=0), "n_regions"), (dict(n_regions=65536), "n_regions"),
                    (dict(template=template.to(torch.float32)), "template must be")):
        args = dict(template=template, template_vs=(1, 1, 1), regions=regions)
        args.update(kw)
        with pytest.raises(U.UNetError, match=msg):
            R.Atlas(**args)
