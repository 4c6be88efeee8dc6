"""GPU: the geometry of a fitted lattice warp on the device (include/unet_deform.h) -- jacobian and pull under IMPL_GLOBAL, IMPL_TILE
and the default against the numpy restatements of tests/deform_ref.py, parcellate(warp=, geometry=), to_template and
coreg.align(warp=, geometry=) against the stages called by hand.  Every case runs twice into 0x5A-filled outputs with guard bytes
around them; every comparison is exact equality of bytes.  Shapes are written (W, H, D) as in the header; the arrays are (D, H, W)."""
import os
import sys
import threading

import numpy as np
import pytest
import torch

import unet_studio_amd as U
from unet_studio_amd import coreg as CR
from unet_studio_amd import cowarp as CW
from unet_studio_amd import deform as DF
from unet_studio_amd import register as R
from unet_studio_amd import stats as ST
from unet_studio_amd import warp as W

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import coreg_ref as cr  # noqa: E402
import deform_ref as ref  # noqa: E402
import warp_ref as wr  # noqa: E402
from test_gpu_register import dev_int, geometry_maps, host, same, solid  # noqa: E402
from test_register_host import IDENTITY, TRUE_MAP  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
IMPLS = (DF.IMPL_GLOBAL, DF.IMPL_TILE, DF.IMPL_DEFAULT)
SUBJECTS = [(5, 6, 7), (12, 10, 8), (16, 16, 16), (17, 9, 33), (38, 44, 40)]
TEMPLATES = [(10, 12, 9), (8, 8, 8), (36, 48, 40)]
SPACINGS = (4, 8, 16, 32)                                          # every shape allows every g: one cell, a partial last cell
ITERS = (0, 1, 8, 32)
DTYPES = (np.float32, np.uint8, np.uint16)
TORCH = {np.float32: torch.float32, np.uint8: torch.uint8, np.uint16: torch.uint16}
G = 64                                                             # guard bytes on each side
GUARD = 0xC3


def dev(a):
    a = np.array(a, order="C")                                      # a copy: the shared cases are read only
    if a.dtype == np.uint16:
        return torch.from_numpy(a.view(np.int16)).to(DEV).view(torch.uint16)
    return torch.from_numpy(a).to(DEV)


def guarded(n, dtype, rep):
    """-> (the whole byte buffer, its inner n elements of `dtype`, every byte 0x5A + rep, between two runs of guard bytes)"""
    nbytes = n * torch.empty(0, dtype=dtype).element_size()
    buf = torch.full((nbytes + 2 * G,), GUARD, dtype=torch.uint8, device=DEV)
    buf[G:G + nbytes] = 0x5A + rep
    return buf, buf[G:G + nbytes].view(dtype)


def intact(*bufs):
    for buf in bufs:
        b = buf.cpu().numpy()
        assert (b[:G] == GUARD).all() and (b[-G:] == GUARD).all()


def fields(rng, sshape, g):
    """zero, random within 600, random at +-32767 (threads leave their window, whole blocks take the global path), none"""
    shape = wr.lattice_ref(sshape, g) + (3,)
    return [np.zeros(shape, np.int32), rng.integers(-600, 601, shape).astype(np.int32),
            (rng.integers(0, 2, shape) * 65534 - 32767).astype(np.int32), None]


def inverse_of(m):
    """the float64 inverse rounded once; a singular or NaN map gets an arbitrary one: only the bits matter"""
    a = np.asarray(m, np.float64)
    if not np.isfinite(a).all() or abs(np.linalg.det(a[:9].reshape(3, 3))) < 1e-12:
        return np.asarray([0.9, 0.1, 0, -0.1, 1.1, 0, 0, 0.05, 1, 0.5, -0.25, 1], np.float32)
    return ref.inverse_map_ref(m)


def volume_of(rng, sshape, dt):
    if dt == np.float32:
        return rng.standard_normal(sshape).astype(np.float32)
    return (solid(rng, sshape, 5) * (1 if dt == np.uint8 else 1000)).astype(dt)


def check_jacobian(sshape, m, D, g, want=None):
    want = ref.jacobian_ref(sshape, m, D, g) if want is None else want
    d_dev, n = dev(D), int(np.prod(sshape))
    for with_det in (True, False):
        for rep in range(2):
            dbuf, det = guarded(n, torch.float32, rep)
            got, info = DF.jacobian(sshape, m, d_dev, g, det=det if with_det else False)
            assert same(host(info), want[1]), (g, with_det, rep, host(info), want[1])
            if with_det:
                assert got.data_ptr() == det.data_ptr() and same(host(got), want[0]), (g, rep)
            else:
                assert got is None and (host(det).view(np.uint8) == 0x5A + rep).all()
            intact(dbuf)
    return want


def check_pull(v_dev, volume, tshape, m, inv, D, g, iters, with_pos, want=None, impls=IMPLS):
    want = ref.pull_ref(volume, tshape, m, inv, D, g, iters) if want is None else want
    d_dev, n = (None if D is None else dev(D)), int(np.prod(tshape))
    for impl in impls:
        for rep in range(2):
            obuf, out = guarded(n, v_dev.dtype, rep)
            pbuf, pos = guarded(3 * n, torch.float32, rep)
            got, p, info = DF.pull(v_dev, tshape, m, d_dev, g, inv=inv, iters=iters, pos=pos if with_pos else False, impl=impl, out=out)
            tag = (volume.dtype, g, iters, impl, rep)
            assert got.data_ptr() == out.data_ptr() and same(host(got), want[0]), tag
            assert same(host(info), want[2]), (tag, host(info), want[2])
            if with_pos:
                assert p.data_ptr() == pos.data_ptr() and same(host(p), want[1]), tag
            else:
                assert p is None and (host(pos).view(np.uint8) == 0x5A + rep).all()
            intact(obuf, pbuf)
    return want


# ---- over the shapes ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g", SPACINGS)
@pytest.mark.parametrize("sshape", SUBJECTS)
def test_jacobian_shapes_fields_and_maps(sshape, g):
    sw, sh, sd = sshape
    rng = np.random.default_rng(sw * 100 + g)
    ss = (sd, sh, sw)
    maps = geometry_maps(ss, ss)
    big = sd * sh * sw > 10000
    for k, D in enumerate(fields(rng, ss, g)[:3]):
        for j, m in enumerate(maps):
            if not big or j in (0, 3, 6, 7, 9):
                det, info = check_jacobian(ss, m, D, g)
                if k == 0 and np.isfinite(m).all():
                    assert info[1] == 0 and info[2] == info[3]        # a zero field: one value everywhere
    nan_info = ref.jacobian_ref(ss, maps[6], fields(rng, ss, g)[1], g)[1]
    assert nan_info.tolist() == [sd * sh * sw, sd * sh * sw, 0xFFFFFFFF, 0]


@pytest.mark.parametrize("g", SPACINGS)
@pytest.mark.parametrize("tshape", TEMPLATES)
@pytest.mark.parametrize("sshape", SUBJECTS)
def test_pull_shapes_fields_maps_kinds_and_rounds(sshape, tshape, g):
    (sw, sh, sd), (tw, th, td) = sshape, tshape
    rng = np.random.default_rng(sw * 1000 + tw * 10 + g)
    ss, ts = (sd, sh, sw), (td, th, tw)
    volumes = {dt: volume_of(rng, ss, dt) for dt in DTYPES}
    on_dev = {dt: dev(v) for dt, v in volumes.items()}
    maps = geometry_maps(ss, ts)
    big = sd * sh * sw > 10000 or td * th * tw > 10000               # the large grids: fewer combinations, every path still
    open_seen = 0
    for k, D in enumerate(fields(rng, ss, g)):
        for j, m in enumerate(maps):
            if big and j not in (0, 3, 6, 7, 9):
                continue
            inv = inverse_of(m)
            for i, dt in enumerate(DTYPES if not big else (DTYPES[(j + k) % 3],)):
                iters = ITERS[(i + j + k) % 4]
                want = check_pull(on_dev[dt], volumes[dt], ts, m, inv, D, g, iters, with_pos=(i + j) % 2 == 0)
                open_seen += int(want[2][1])
    assert open_seen > 0                                            # the +-32767 fields do not converge, and say so


@pytest.mark.parametrize("off", [1, 3])
def test_pull_volumes_and_outputs_off_alignment(off):
    rng = np.random.default_rng(30 + off)
    ss, ts, g = (9, 9, 33), (7, 10, 30), 8
    m = [1.05, 0.1, 0, -0.08, 0.97, 0.04, 0.02, 0, 1.1, -1.25, 0.75, -0.5]
    inv = ref.inverse_map_ref(m)
    D = fields(rng, ss, g)[1]
    d_dev = dev(D)
    n_in, n_out = int(np.prod(ss)), int(np.prod(ts))
    for dt, step in ((np.uint8, off), (np.uint16, 1)):              # bytes off for uint8, one element off for uint16
        volume = volume_of(rng, ss, dt)
        want = ref.pull_ref(volume, ts, m, inv, D, g, 8)
        es = volume.itemsize
        vbuf = torch.zeros((n_in + 16) * es, dtype=torch.uint8, device=DEV)
        vbuf[step * es:(step + n_in) * es] = dev(volume.reshape(-1).view(np.uint8))
        v_dev = vbuf[step * es:(step + n_in) * es].view(TORCH[dt]).view(ss)
        assert v_dev.data_ptr() % 4 != 0 and v_dev.is_contiguous()
        for impl in IMPLS:
            for rep in range(2):
                obuf, inner = guarded(n_out + 8, TORCH[dt], rep)
                out = inner[step:step + n_out]
                got, _, info = DF.pull(v_dev, ts, m, d_dev, g, inv=inv, iters=8, impl=impl, out=out)
                assert got.data_ptr() == out.data_ptr() and same(host(got), want[0]) and same(host(info), want[2]), (dt, impl, rep)
                rest = host(inner).view(np.uint8)
                assert (rest[:step * es] == 0x5A + rep).all() and (rest[(step + n_out) * es:] == 0x5A + rep).all()
                intact(obuf)


# ---- the shared case ------------------------------------------------------------------------------------------------------------------------
def test_the_fitted_field_of_the_warped_ellipsoid_against_the_restatements_figures():
    subject, template = wr.warped_case()
    D, _ = wr.warped_fit()
    geo = ref.warped_geometry()
    check_jacobian(subject.shape, TRUE_MAP, D, 4, want=(geo["det"], geo["info"]))
    assert geo["info"].tolist()[:2] == [66880, 0] and geo["pull_info"].tolist() == [60091, 0]
    s_dev = dev(subject)
    check_pull(s_dev, subject, template.shape, TRUE_MAP, geo["inv"], D, 4, 8, True, want=(geo["out"], geo["pos"], geo["pull_info"]))
    # the wrapper's own inverse is the restatement's
    got, pos, info = DF.pull(s_dev, template.shape, TRUE_MAP, dev(D), 4, pos=True)
    assert same(host(got), geo["out"]) and same(host(pos), geo["pos"]) and same(host(info), geo["pull_info"])
    s = DF.summary(DF.jacobian(subject.shape, TRUE_MAP, dev(D), 4, det=False)[1])
    assert s == dict(voxels=66880, folded=0, det_min=float(geo["det"].min()), det_max=float(geo["det"].max()))
    # the float32 image of the same subject through the same inverse
    image = np.asarray(subject).astype(np.float32) * 0.25
    check_pull(dev(image), image, template.shape, TRUE_MAP, geo["inv"], D, 4, 8, False)


def test_two_threads_on_two_streams():
    subject, template = wr.warped_case()
    D, _ = wr.warped_fit()
    geo = ref.warped_geometry()
    rng = np.random.default_rng(5)
    wild = fields(rng, subject.shape, 8)[2]
    want_wild = ref.pull_ref(subject, template.shape, TRUE_MAP, geo["inv"], wild, 8, 32)
    s_dev, d_dev, w_dev = dev(subject), dev(D), dev(wild)
    torch.cuda.synchronize()
    results, errors = [None, None], []

    def work(k):
        try:
            stream = torch.cuda.Stream(device=DEV)
            with torch.cuda.stream(stream):
                out = []
                for _ in range(5):
                    if k == 0:
                        det, info = DF.jacobian(subject.shape, TRUE_MAP, d_dev, 4)
                        o, p, i = DF.pull(s_dev, template.shape, TRUE_MAP, d_dev, 4, inv=geo["inv"], pos=True, impl=DF.IMPL_TILE)
                        out.append((det, info, o, p, i))
                    else:
                        out.append(DF.pull(s_dev, template.shape, TRUE_MAP, w_dev, 8, inv=geo["inv"], iters=32, pos=True, impl=DF.IMPL_GLOBAL))
                stream.synchronize()
            results[k] = [tuple(host(t) for t in row) for row in out]
        except Exception as e:                                       # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for row in results[0]:
        assert all(same(a, b) for a, b in zip(row, (geo["det"], geo["info"], geo["out"], geo["pos"], geo["pull_info"])))
    for row in results[1]:
        assert all(same(a, b) for a, b in zip(row, want_wild))


# ---- parcellate, to_template, coreg.align ---------------------------------------------------------------------------------------------------
SHORT = dict(init=TRUE_MAP, stages=[(2, 3, 4)], max_iterations=30)  # a search of a few iterations
SHORT_PLAN = W.Plan(levels=[(8, 256, 128, 2), (4, 128, 128, 1)])


def test_parcellate_with_geometry_against_the_stages_by_hand_and_to_template():
    subject, template = wr.warped_case()
    z, y, x = np.indices(template.shape)
    atlas = np.where(template > 0, 1 + (x > 14).astype(np.int64) + (x + y > 50) + 3 * (z > 20), 0)
    s_dev, t_dev, a_dev = dev_int(subject, torch.uint8), dev_int(template, torch.uint8), dev_int(atlas, torch.uint16)
    plain, plain_rep = R.parcellate(s_dev, (1, 1, 1), t_dev, (1, 1, 1), a_dev, warp=SHORT_PLAN, **SHORT)
    none, none_rep = R.parcellate(s_dev, (1, 1, 1), t_dev, (1, 1, 1), a_dev, warp=SHORT_PLAN, geometry=None, **SHORT)
    assert same(host(none), host(plain)) and "geometry" not in none_rep and "geometry" not in plain_rep
    assert sorted(none_rep) == sorted(plain_rep) and same(none_rep["warp"]["report"], plain_rep["warp"]["report"])
    for plan in (DF.Plan(), DF.Plan(jacobian=False, iters=4, impl=DF.IMPL_TILE)):
        got, rep = R.parcellate(s_dev, (1, 1, 1), t_dev, (1, 1, 1), a_dev, warp=SHORT_PLAN, geometry=plan, **SHORT)
        assert same(host(got), host(plain)) and same(rep["warp"]["report"], plain_rep["warp"]["report"])
        geo, m = rep["geometry"], np.concatenate(rep["map"])
        # the stages by hand: fit from the map found, jacobian on its field
        field, _ = W.fit(s_dev, t_dev, 5, m, levels=rep["warp"]["levels"])
        assert geo["g"] == 4 and same(host(geo["field"]), host(field)) and (geo["iters"], geo["impl"]) == (plan.iters, plan.impl)
        det, info = DF.jacobian(subject.shape, m, field, 4)
        want_det, want_info = ref.jacobian_ref(subject.shape, m, host(field), 4)
        assert same(host(det), want_det) and same(host(info), want_info)
        s = DF.summary(want_info)
        assert (geo["folded"], geo["det_min"], geo["det_max"]) == (s["folded"], s["det_min"], s["det_max"]) and geo["det_min"] > 0
        assert (geo["det"] is None) if not plan.jacobian else same(host(geo["det"]), want_det)
        # to_template: the subject tissue map back on the template grid
        inv = ref.inverse_map_ref(m)
        want = ref.pull_ref(subject, template.shape, m, inv, host(field), 4, plan.iters)
        out, pos, pinfo = R.to_template(s_dev, rep, template.shape, kind=DF.KIND_U8, pos=True)
        assert same(host(out), want[0]) and same(host(pos), want[1]) and same(host(pinfo), want[2])
        by_hand = DF.pull(s_dev, template.shape, m, field, 4, iters=plan.iters, impl=plan.impl)
        assert same(host(by_hand[0]), want[0]) and by_hand[1] is None and same(host(by_hand[2]), want[2])
        with pytest.raises(U.UNetError, match="does not match"):
            R.to_template(s_dev, rep, template.shape, kind=DF.KIND_F32)
    inside, _ = ref.nearest_inside(list(want[1].reshape(3, -1)), subject.shape)
    affine = ref.pull_ref(subject, template.shape, m, inv, None, 4, 0)
    ainside, _ = ref.nearest_inside(list(affine[1].reshape(3, -1)), subject.shape)
    before = ref.dice_labels(affine[0].reshape(-1), np.asarray(template).reshape(-1), ainside)
    after = ref.dice_labels(want[0].reshape(-1), np.asarray(template).reshape(-1), inside)
    print("to_template after a short fit: Dice %.4f through inv alone, %.4f through the inverse; not converged %d" % (before, after, want[2][1]))
    assert after > before                                           # `before` is the searched map's, not TRUE_MAP's: no floor of its own
    # the volume change per region: stats over the det map and the regions, no kernel of its own
    det = rep_det = DF.jacobian(subject.shape, m, field, 4)[0]
    lo, hi = 0.0, 4.0
    rows = ST.moments(plain, rep_det, 8, lo, hi)
    table = ST.summary(rows, lo, hi)
    regions, d = host(plain), host(det)
    for r in range(1, 9):
        if (regions == r).any():
            assert table["n"][r] == (regions == r).sum() and table["min"][r] == d[regions == r].min() and table["max"][r] == d[regions == r].max()
            assert abs(table["mean"][r] - d[regions == r].astype(np.float64).mean()) < 2 * (hi - lo) / 65536
    assert table["n"][1:].sum() > 0


def test_to_template_with_the_default_fit_brings_the_tissue_map_onto_the_template():
    subject, template = wr.warped_case()
    atlas = (np.asarray(template) > 0).astype(np.int64)
    s_dev, t_dev, a_dev = dev_int(subject, torch.uint8), dev_int(template, torch.uint8), dev_int(atlas, torch.uint16)
    _, rep = R.parcellate(s_dev, (1, 1, 1), t_dev, (1, 1, 1), a_dev, warp=W.Plan(W.DEFAULT_LEVELS), geometry=DF.Plan(), **SHORT)
    m, field = np.concatenate(rep["map"]), host(rep["geometry"]["field"])
    want = ref.pull_ref(subject, template.shape, m, ref.inverse_map_ref(m), field, 4, 8)
    out, pos, info = R.to_template(s_dev, rep, template.shape, pos=True)
    assert same(host(out), want[0]) and same(host(pos), want[1]) and same(host(info), want[2])
    inside, _ = ref.nearest_inside(list(want[1].reshape(3, -1)), subject.shape)
    dice = ref.dice_labels(want[0].reshape(-1), np.asarray(template).reshape(-1), inside)
    print("to_template after the default fit: Dice %.4f, folded %d, det %.4f .. %.4f, not converged %d" % (
        dice, rep["geometry"]["folded"], rep["geometry"]["det_min"], rep["geometry"]["det_max"], want[2][1]))
    assert dice >= 0.90 and rep["geometry"]["folded"] == 0 and want[2][1] == 0


ALIGN = dict(stages=[(2, 0, 1)], max_iterations=12)
ALIGN_PLAN = CW.Plan(levels=[(8, 256, 128, 2), (4, 128, 128, 1)])


def test_align_with_geometry_against_the_stages_by_hand():
    fixed, moving = cr.phantom(32)
    f_dev, m_dev = dev(fixed.copy()), dev(moving.copy())
    plain = CR.align(m_dev, (1, 1, 1), f_dev, (1, 1, 1), warp=ALIGN_PLAN, **ALIGN)
    none = CR.align(m_dev, (1, 1, 1), f_dev, (1, 1, 1), warp=ALIGN_PLAN, geometry=None, **ALIGN)
    assert len(plain) == len(none) == 4 and all(same(host(a), host(b)) for a, b in zip(plain[:3], none[:3]))
    assert sorted(plain[3]) == sorted(none[3]) and "det" not in none[3] and same(host(plain[3]["field"]), host(none[3]["field"]))
    for plan in (DF.Plan(), DF.Plan(jacobian=False)):
        for _ in range(2):
            map_dev, info, moved, w = CR.align(m_dev, (1, 1, 1), f_dev, (1, 1, 1), warp=ALIGN_PLAN, geometry=plan, **ALIGN)
            assert all(same(host(a), host(b)) for a, b in zip((map_dev, info, moved), plain[:3])) and same(host(w["field"]), host(plain[3]["field"]))
            m = host(map_dev)
            want_det, want_info = ref.jacobian_ref(fixed.shape, m, host(w["field"]), w["g"])
            det, dinfo = DF.jacobian(fixed.shape, m, w["field"], w["g"])
            assert same(host(det), want_det) and same(host(dinfo), want_info)
            assert [host(w[k]).tolist() for k in ("folded", "det_min", "det_max")] == [[int(v)] for v in want_info[1:]]
            assert (w["det"] is None) if not plan.jacobian else same(host(w["det"]), want_det)


def test_more_bricks_than_blocks_a_block_walks_over_several():
    """(65, 70, 66) holds 5 x 18 x 17 = 1530 bricks of 16 x 4 x 4, more than the 1280 blocks a launch is capped at: some blocks take two
    bricks and restage their window, some one; the last bricks along every axis are partial"""
    rng = np.random.default_rng(11)
    big, small, g = (66, 70, 65), (8, 10, 12), 8
    m = [1.05, 0.1, 0, -0.08, 0.97, 0.04, 0.02, 0, 1.1, -1.25, 0.75, -0.5]
    check_jacobian(big, m, fields(rng, big, g)[1], g)
    # a small subject seen from a large template grid (most of it outside), and the large grid onto itself
    shrink = [0.15, 0.01, 0, 0, 0.14, 0, 0, 0.02, 0.12, 0.5, 0.25, 0]
    volume = volume_of(rng, small, np.uint8)
    for D in fields(rng, small, g)[1:3]:
        want = check_pull(dev(volume), volume, big, ref.inverse_map_ref(shrink), shrink, D, g, 8, True)
        assert 0 < want[2][0] < int(np.prod(big))
    image = volume_of(rng, big, np.float32)
    check_pull(dev(image), image, big, m, ref.inverse_map_ref(m), fields(rng, big, g)[1], g, 8, False)
