"""CPU: the host half of the geometry of a fitted lattice warp (include/unet_deform.h, unet-studio_amd/deform.py) -- the ABI the
library exports, argument errors found before any device call, and the restatements of tests/deform_ref.py checked on hand-written
answers.  The quality of the definition (does the fixed-point iteration invert the fitted field of the warped ellipsoid, does the
field fold) is measured here, on the restatement, not on the device.  No device calls."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

import unet_studio_amd as U
from unet_studio_amd import deform as DF
from unet_studio_amd import warp as W

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cowarp_ref as cwr  # noqa: E402
import deform_ref as ref  # noqa: E402
import warp_ref as wr  # noqa: E402
from test_register_host import IDENTITY, TRUE_MAP, counted, shift  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
SHEAR = [1.05, 0.1, 0, -0.08, 0.97, 0.04, 0.02, 0, 1.1, -1.25, 0.75, -0.5]


def det_written(m):
    """the determinant of a map's matrix in the header's order, float32"""
    a, b, c, d, e, f, g, h, i = (F(v) for v in m[:9])
    return (a * (e * i - f * h) - b * (d * i - f * g)) + c * (d * h - e * g)


# ---- the ABI -------------------------------------------------------------------------------------------------------------------------
def test_unet_deform_h_declares_exactly_the_exports_and_no_other_header_names_the_prefix():
    lib = ctypes.CDLL(U.engine.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "unet_deform.h")).read()
    declared = set(re.findall(r"\b(unet_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(DF.EXPORTS) == {"unet_deform_jacobian", "unet_deform_pull"}
    for name in sorted(declared):
        assert hasattr(lib, name), "libunet_hip.so does not export " + name
    impls = {k: int(v) for k, v in re.findall(r"UNET_DEFORM_(IMPL_[A-Z]+) = (\d+)", hdr)}
    assert impls == {"IMPL_DEFAULT": DF.IMPL_DEFAULT, "IMPL_GLOBAL": DF.IMPL_GLOBAL, "IMPL_TILE": DF.IMPL_TILE}
    assert (DF.IMPL_DEFAULT, DF.IMPL_GLOBAL, DF.IMPL_TILE) == (0, 1, 2)
    kinds = {k: int(v) for k, v in re.findall(r"UNET_DEFORM_(KIND_[A-Z0-9]+) = (\d+)", hdr)}
    assert kinds == {"KIND_F32": DF.KIND_F32, "KIND_U8": DF.KIND_U8, "KIND_U16": DF.KIND_U16} and (DF.KIND_F32, DF.KIND_U8, DF.KIND_U16) == (0, 1, 2)
    limits = {k: int(v) for k, v in re.findall(r"#define UNET_DEFORM_MAX_([A-Z]+) (\d+)", hdr)}
    assert limits == {"DISP": DF.MAX_DISP, "ITERS": DF.MAX_ITERS, "WINDOW": DF.MAX_WINDOW}
    assert DF.MAX_DISP == W.MAX_DISP and DF.MAX_ITERS == ref.MAX_ITERS == 32 and DF.SPACINGS == (4, 8, 16, 32)
    assert U.deform is DF and DF.Plan() == (True, 8, DF.IMPL_DEFAULT) and DF.Plan(iters=3).iters == 3
    assert "this project's" in hdr and "NOT pinned" in hdr
    # the header speaks of those it builds on by file name only
    low = hdr.lower()
    for other in ("unet_warp_", "unet_cowarp_", "unet_coreg", "unet_reg_", "unet_stats_", "unet_space_", "unet_start"):
        assert other not in low, other
    assert "unet_warp.h" in low and "unet_cowarp.h" in low
    for h in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if h != "unet_deform.h":
            assert "unet_deform" not in open(os.path.join(ROOT, "include", h)).read().lower(), h


# ---- argument errors, before any device call -------------------------------------------------------------------------------------
P = [ctypes.c_void_p(0x1000 * (i + 1)) for i in range(8)]          # never dereferenced
F12 = (ctypes.c_float * 12)(*IDENTITY)


def test_jacobian_and_pull_argument_errors_need_no_device():
    lib = U.engine.lib

    def jac(s=(4, 4, 4), map=F12, D=P[0], g=4, det=P[1], info=P[2]):
        rc = lib.unet_deform_jacobian(*s, map, D, g, det, info, None)
        assert rc != 0
        return lib.unet_last_error().decode()

    assert "subject dimensions" in jac(s=(0, 4, 4)) and "subject dimensions" in jac(s=(4, 4, -1)) and "subject grid" in jac(s=(2048, 1024, 1024))
    assert "null map" in jac(map=None) and "null D" in jac(D=None) and "null info" in jac(info=None)
    assert "D must be 4-byte aligned" in jac(D=ctypes.c_void_p(0x3002)) and "det must be 4-byte aligned" in jac(det=ctypes.c_void_p(0x3001))
    assert "info must be 8-byte aligned" in jac(info=ctypes.c_void_p(0x5004))
    assert "g must be 4, 8, 16 or 32, got 64" in jac(g=64) and "g must be" in jac(g=0) and "g must be" in jac(g=6)
    assert jac(g=3).startswith("unet_deform_jacobian: ")
    assert "null info" in jac(det=None, info=None)                  # a null det is no error of its own

    def pull(volume=P[0], kind=0, s=(4, 4, 4), t=(4, 4, 4), map=F12, inv=F12, D=P[1], g=4, iters=8, out=P[2], pos=P[3], info=P[4], impl=0):
        rc = lib.unet_deform_pull(volume, kind, *s, *t, map, inv, D, g, iters, out, pos, info, impl, None)
        assert rc != 0
        return lib.unet_last_error().decode()

    assert "unknown kind 3" in pull(kind=3) and "unknown kind -1" in pull(kind=-1)
    assert "null volume" in pull(volume=None) and "null map" in pull(map=None) and "null inv" in pull(inv=None) and "null out" in pull(out=None)
    assert "null info" in pull(info=None) and "null info" in pull(D=None, pos=None, info=None)   # a null D or pos is no error
    assert "subject dimensions" in pull(s=(4, 0, 4)) and "template dimensions" in pull(t=(-1, 4, 4))
    assert "subject grid" in pull(s=(2048, 1024, 1024)) and "template grid" in pull(t=(2048, 1024, 1024))
    assert "g must be 4, 8, 16 or 32, got 5" in pull(g=5) and "g must be" in pull(D=None, g=0)
    assert "iters must be in [0, 32], got 33" in pull(iters=33) and "iters must be in [0, 32], got -1" in pull(iters=-1)
    assert "unknown impl 3" in pull(impl=3) and "unknown impl -1" in pull(impl=-1)
    assert "D must be 4-byte aligned" in pull(D=ctypes.c_void_p(0x3002)) and "pos must be 4-byte aligned" in pull(pos=ctypes.c_void_p(0x3002))
    assert "info must be 8-byte aligned" in pull(info=ctypes.c_void_p(0x5004))
    # the volume and out: any multiple of their element size
    odd, even = ctypes.c_void_p(0x3001), ctypes.c_void_p(0x3002)
    assert "volume must be 4-byte aligned" in pull(volume=even) and "out must be 4-byte aligned" in pull(out=odd)
    assert "volume must be 2-byte aligned" in pull(kind=2, volume=odd) and "out must be 2-byte aligned" in pull(kind=2, out=odd)
    assert "null info" in pull(kind=2, volume=even, out=even, info=None) and "null info" in pull(kind=1, volume=odd, out=odd, info=None)
    assert pull(impl=9).startswith("unet_deform_pull: ")


def test_wrapper_errors_need_no_device():
    u8, f32 = torch.zeros((2, 2, 2), dtype=torch.uint8), torch.zeros((2, 2, 2), dtype=torch.float32)
    d = torch.zeros((2, 2, 2, 3), dtype=torch.int32)
    for call in (lambda: DF.jacobian((2, 2, 2), IDENTITY, d, 4), lambda: DF.pull(f32, (2, 2, 2), IDENTITY, d, 4),
                 lambda: DF.pull(u8, (2, 2, 2), IDENTITY, None, 4)):
        with pytest.raises(U.UNetError, match="device tensor"):
            call()
    with pytest.raises(U.UNetError, match="geometry needs warp"):
        U.register.parcellate(u8, (1, 1, 1), u8, (1, 1, 1), u8, geometry=DF.Plan())
    with pytest.raises(U.UNetError, match="geometry needs warp"):
        U.coreg.align(f32, (1, 1, 1), f32, (1, 1, 1), geometry=DF.Plan())
    with pytest.raises(U.UNetError, match="geometry must be a deform.Plan"):
        U.coreg.align(f32, (1, 1, 1), f32, (1, 1, 1), warp=U.cowarp.Plan(), geometry=7)
    with pytest.raises(U.UNetError, match="iters must be an integer in \\[0, 32\\], got 33"):
        U.register.parcellate(u8, (1, 1, 1), u8, (1, 1, 1), u8, warp=W.Plan(W.DEFAULT_LEVELS), geometry=DF.Plan(iters=33))
    with pytest.raises(U.UNetError, match="report must be parcellate's"):
        U.register.to_template(u8, dict(map=None), (2, 2, 2))
    # the host arithmetic
    for m in (IDENTITY, TRUE_MAP, SHEAR, shift(1.5, -2, 0.25)):
        inv = DF.inverse_map(m)
        assert inv.dtype == np.float32 and inv.tobytes() == ref.inverse_map_ref(m).tobytes()
        a, b = np.asarray(m, np.float64), inv.astype(np.float64)
        assert np.abs(a[:9].reshape(3, 3) @ b[:9].reshape(3, 3) - np.eye(3)).max() < 1e-6
        assert np.abs(a[:9].reshape(3, 3) @ b[9:] + a[9:]).max() < 1e-5
    assert DF.inverse_map((TRUE_MAP[:9], TRUE_MAP[9:])).tobytes() == DF.inverse_map(TRUE_MAP).tobytes()
    with pytest.raises(U.UNetError, match="singular"):
        DF.inverse_map([1, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0])
    rel = DF.relative(np.array([2.0, 1.0], np.float32), [2, 0, 0, 0, 1, 0, 0, 0, 1, 5, 5, 5])
    assert rel.dtype == np.float64 and rel.tolist() == [1.0, 0.5]
    s = DF.summary(np.array([10, 3, int(ref.key(F(-0.5))), int(ref.key(F(1.25)))], np.int64))
    assert s == dict(voxels=10, folded=3, det_min=-0.5, det_max=1.25)
    s = DF.summary(np.array([10, 10, ref.KEY_MIN0, ref.KEY_MAX0], np.int64))
    assert s["folded"] == 10 and np.isnan(s["det_min"]) and np.isnan(s["det_max"])
    # the keys order floats as floats
    v = np.array([-np.inf, -3.5, -0.0, 0.0, 1e-40, 0.25, 7, np.inf], F)
    k = ref.key(v)
    assert (np.diff(k) > 0).all() and k.min() >= 0 and k.max() <= 0xFFFFFFFF and [ref.unkey(x) for x in k] == v.tolist()


# ---- G and det by hand -----------------------------------------------------------------------------------------------------------------
def test_a_zero_field_gives_the_maps_determinant_in_the_written_order():
    for m in (IDENTITY, TRUE_MAP, SHEAR):
        for g, sshape in ((4, (5, 6, 7)), (8, (9, 3, 17)), (32, (2, 2, 2))):
            det, info = ref.jacobian_ref(sshape, m, wr.zero_field(sshape, g), g)
            want = det_written(m)
            assert det.dtype == np.float32 and det.shape == sshape and (det == want).all()
            assert info.tolist() == [int(np.prod(sshape)), 0, int(ref.key(want)), int(ref.key(want))]
    assert det_written(IDENTITY) == 1 and abs(float(det_written(TRUE_MAP)) - 1.0987) < 1e-4


def test_a_ramp_along_x_adds_a_constant_to_J00_only():
    sshape, g = (6, 7, 9), 4
    D = wr.zero_field(sshape, g)
    D[..., 0] = 96 * np.arange(D.shape[2])[None, None, :]           # 96 Q8 per node = 0.375 template voxels per 4 subject voxels
    x, y, z = counted(sshape, 1)
    G = ref.derivatives(D, g, x, y, z)
    assert (G[:, 0, 0] == 96 * g * g).all() and not G[:, 0, 1:].any() and not G[:, 1:].any()
    det, info = ref.jacobian_ref(sshape, IDENTITY, D, g)
    assert (det == F(1 + 0.375 / 4)).all() and info[1] == 0
    # the same ramp in the z component along y: J[2][1], which leaves the determinant of the identity alone
    D = wr.zero_field(sshape, g)
    D[..., 2] = -64 * np.arange(D.shape[1])[None, :, None]
    G = ref.derivatives(D, g, x, y, z)
    assert (G[:, 2, 1] == -64 * g * g).all() and int(np.abs(G).sum()) == 64 * g * g * x.size
    assert (ref.jacobian_ref(sshape, IDENTITY, D, g)[0] == 1).all()
    # the bound of the header: one node at +32767 among nodes at -32767
    D = np.full(wr.lattice_ref(sshape, 32) + (3,), -32767, np.int32)
    D[0, 0, 1] = 32767
    assert np.abs(ref.derivatives(D, 32, *counted(sshape, 1))).max() == 32 * 32 * 65534 < 1 << 31


def fold_case():
    """identity map, g = 4, one node's x component at +1536 and its +x neighbour at 0: between them x + e_x falls by half a voxel per
    voxel"""
    sshape = (5, 6, 13)
    D = wr.zero_field(sshape, 4)
    D[:, :, 1, 0] = 1536                                            # the whole plane of nodes at x = 4, so that the fold is a slab
    return sshape, D


def test_a_hand_made_fold_is_counted_and_sets_the_minimum():
    sshape, D = fold_case()
    det, info = ref.jacobian_ref(sshape, IDENTITY, D, 4)
    # cell 0 (x = 0..3): +1536 / 256 / 4 = +1.5 per voxel; cell 1 (x = 4..7): -1.5; beyond: 0
    assert (det[:, :, 0:4] == 2.5).all() and (det[:, :, 4:8] == -0.5).all() and (det[:, :, 8:] == 1).all()
    assert info.tolist() == [det.size, 5 * 6 * 4, int(ref.key(F(-0.5))), int(ref.key(F(2.5)))]
    # one node alone, as the issue words it: in the cell between it and its +x neighbour J[0][0] = -0.5 on the node's own row
    one = wr.zero_field(sshape, 4)
    one[1, 1, 1, 0] = 1536
    det1, info1 = ref.jacobian_ref(sshape, IDENTITY, one, 4)
    G = ref.derivatives(one, 4, *counted(sshape, 1)).reshape(sshape + (3, 3))
    assert G[4, 4, 5, 0, 0] == -1536 * 16 and det1[4, 4, 5] == -0.5 and info1[1] > 0 and ref.unkey(info1[2]) <= -0.5
    assert DF.summary(info)["det_min"] == -0.5 and DF.summary(info)["folded"] == 120


def test_a_nan_in_the_map_folds_everything_and_leaves_the_extremes_at_their_start():
    m = list(IDENTITY)
    m[4] = float("nan")
    sshape = (5, 6, 7)
    rng = np.random.default_rng(0)
    D = rng.integers(-300, 301, wr.lattice_ref(sshape, 4) + (3,)).astype(np.int32)
    det, info = ref.jacobian_ref(sshape, m, D, 4)
    assert np.isnan(det).all() and info.tolist() == [210, 210, 0xFFFFFFFF, 0]


# ---- the continuous field ----------------------------------------------------------------------------------------------------------------
def test_field_at_equals_the_corner_sums_at_every_integer_voxel():
    rng = np.random.default_rng(1)
    for sshape, g in (((5, 6, 7), 4), ((9, 10, 13), 4), ((17, 9, 33), 8), ((17, 9, 33), 16), ((3, 2, 5), 32), ((8, 8, 8), 8)):
        D = rng.integers(-32767, 32768, wr.lattice_ref(sshape, g) + (3,)).astype(np.int32)
        x, y, z = counted(sshape, 1)                               # the last cell is partial unless g divides the size
        e = ref.field_at(D, g, [v.astype(F) for v in (x, y, z)])
        n = wr.corner_sums(D, g, x, y, z)
        for r in range(3):
            want = np.ldexp(n[:, r].astype(F), -(8 + 3 * wr.LG[g]))
            assert e[r].dtype == F and want.dtype == F
            # the corner sum is exact; the three lerps round.  Equal wherever the sum fits a float: always, for |D| <= 600
            assert np.abs(e[r] - want).max() <= 2.0 ** -8 * 32767 * 2.0 ** -22
        small = (D % 601 - 300).astype(np.int32)
        e = ref.field_at(small, g, [v.astype(F) for v in (x, y, z)])
        n = wr.corner_sums(small, g, x, y, z)
        assert all((e[r] == np.ldexp(n[:, r].astype(F), -(8 + 3 * wr.LG[g]))).all() for r in range(3))
    D, _ = wr.warped_fit()                                          # the fitted field: difference 0, as the prototype found
    x, y, z = counted((38, 44, 40), 1)
    e, n = ref.field_at(D, 4, [v.astype(F) for v in (x, y, z)]), wr.corner_sums(D, 4, x, y, z)
    assert all((e[r] == np.ldexp(n[:, r].astype(F), -14)).all() for r in range(3))


def test_positions_outside_the_lattice_are_clamped_and_a_nan_reads_the_first_node():
    sshape, g = (5, 6, 7), 4                                        # nodes 3 x 3 x 3; the lattice spans 0..8 per axis
    rng = np.random.default_rng(2)
    D = rng.integers(-600, 601, (3, 3, 3, 3)).astype(np.int32)
    at = lambda sx, sy, sz: [float(v[0]) for v in ref.field_at(D, g, [np.array([s], F) for s in (sx, sy, sz)])]  # noqa: E731
    node = lambda k, j, i: (D[k, j, i] / 256.0).tolist()            # noqa: E731
    assert at(0, 0, 0) == node(0, 0, 0) and at(8, 8, 8) == node(2, 2, 2) and at(4, 0, 8) == node(2, 0, 1)
    assert at(-3, -1e30, -np.inf) == node(0, 0, 0) and at(9, 1e30, np.inf) == node(2, 2, 2) and at(100, -5, 4) == node(1, 0, 2)
    assert at(np.nan, np.nan, np.nan) == node(0, 0, 0) and at(np.nan, 8, 4) == node(1, 2, 0)
    c, f = ref.cell(np.array([-1, 0, 3.5, 4, 7.999, 8, 9, np.nan], F), g, 3)
    assert c.tolist() == [0, 0, 0, 1, 1, 1, 1, 0] and f.tolist() == [0, 0, 0.875, 0, float(F(7.999) * F(0.25) - F(1)), 1, 1, 0]
    assert at(2, 0, 0) == [(D[0, 0, 0, r] + 0.5 * (D[0, 0, 1, r] - D[0, 0, 0, r])) / 256 for r in range(3)]


# ---- pull_ref ---------------------------------------------------------------------------------------------------------------------------
def test_pull_a_null_and_a_zero_field_equal_resample_through_the_inverse():
    rng = np.random.default_rng(3)
    sshape, tshape = (5, 6, 7), (6, 5, 8)
    volume = rng.standard_normal(sshape).astype(F)
    for m in (IDENTITY, SHEAR, shift(0.5, -1.5, 2.5)):
        inv = ref.inverse_map_ref(m)
        want = cwr.resample_ref(volume, tshape, inv, wr.zero_field(tshape, 4), 4)   # the volume at inv(u), on the template grid
        for D, iters in ((None, 8), (wr.zero_field(sshape, 4), 0), (wr.zero_field(sshape, 8), 8), (wr.zero_field(sshape, 4), 32)):
            out, pos, info = ref.pull_ref(volume, tshape, m, inv, D, 4 if D is None else (8 if D.shape[0] == 2 else 4), iters)
            assert out.dtype == F and out.tobytes() == want.tobytes() and pos.shape == (3,) + tshape and pos.dtype == F
            assert all(pos[r].reshape(-1).tobytes() == wr.affine_ref(inv, *counted(tshape, 1))[r].tobytes() for r in range(3))
            assert info[1] == 0 and 0 < info[0] < out.size or m is IDENTITY


def test_pull_the_nearest_rule_by_hand():
    volume = (np.arange(12, dtype=np.uint8) + 10).reshape(1, 1, 12)
    for dt in (np.uint8, np.uint16):
        v = volume.astype(dt)
        # template voxel u sits at subject position 0.5 u + 0.74: q = 0.5 u + 1.24, floor 1, 1, 2, 2, .. ; the row leaves at u = 22
        m = [2, 0, 0, 0, 1, 0, 0, 0, 1, -1.48, 0, 0]
        inv = [0.5, 0, 0, 0, 1, 0, 0, 0, 1, 0.74, 0, 0]
        out, pos, info = ref.pull_ref(v, (1, 1, 26), m, inv, None, 4, 8)
        want = [10 + int(np.floor(F(0.5) * F(u) + F(0.74) + F(0.5))) if F(0.5) * F(u) + F(0.74) + F(0.5) < 12 else 0 for u in range(26)]
        assert out.dtype == dt and out.reshape(-1).tolist() == want and want[0] == 11 and want[21] == 21 and want[22:] == [0] * 4
        assert info.tolist() == [22, 0]
        # off the row along y by half a voxel: q_y = 1 is outside a volume of one row
        out, _, info = ref.pull_ref(v, (1, 1, 26), shift(0, -0.5, 0), shift(0, 0.5, 0), None, 4, 8)
        assert not out.any() and info.tolist() == [0, 0]
        out, _, info = ref.pull_ref(v, (1, 1, 26), shift(0, 0.5, 0), shift(0, -0.5, 0), None, 4, 8)   # q_y = 0: the row itself
        assert out.reshape(-1)[:12].tolist() == v.reshape(-1).tolist() and info.tolist() == [12, 0]


def test_pull_iters_0_is_the_affine_inverse_and_each_round_uses_the_field_at_the_last_position():
    sshape, tshape, g = (1, 1, 9), (1, 1, 12), 4
    D = wr.zero_field(sshape, g)
    D[:, :, 1, 0] = 256                                             # the node at x = 4 pushes one template voxel along +x
    volume = np.arange(9, dtype=F).reshape(sshape) * 10
    out0, pos0, info0 = ref.pull_ref(volume, tshape, IDENTITY, IDENTITY, D, g, 0)
    assert pos0[0].reshape(-1).tolist() == list(range(12)) and out0.reshape(-1)[:9].tolist() == volume.reshape(-1).tolist()
    # not converged where the field is not zero: |s + e(s) - u| = e(u) > 1/16 at u = 1..7, inside 0..8
    assert info0.tolist() == [9, 7]
    # one round: s = u - e(u); e(x) = x / 4 up to 4, then (8 - x) / 4
    _, pos1, _ = ref.pull_ref(volume, tshape, IDENTITY, IDENTITY, D, g, 1)
    assert pos1[0].reshape(-1)[:9].tolist() == [0, 0.75, 1.5, 2.25, 3, 4.25, 5.5, 6.75, 8]
    # the exact inverse of x + e(x): u = 1.25 x below 4 (u <= 5), u = 0.75 x + 2 above
    _, pos, info = ref.pull_ref(volume, tshape, IDENTITY, IDENTITY, D, g, 32)
    exact = [u / 1.25 if u <= 5 else (u - 2) / 0.75 for u in range(9)]
    assert np.abs(pos[0].reshape(-1)[:9] - np.asarray(exact)).max() < 1e-5 and info.tolist() == [9, 0]


def test_pull_the_hand_made_fold_reports_voxels_that_are_not_converged():
    sshape, D = fold_case()
    volume = np.zeros(sshape, np.uint8)
    for iters in (8, 32):
        _, pos, info = ref.pull_ref(volume, sshape, IDENTITY, IDENTITY, D, 4, iters)
        assert info[0] > 0 and info[1] > 0 and np.isfinite(pos).all(), info
    # a wild field: every node at +-32767 at random.  Nothing hangs, the count says so
    rng = np.random.default_rng(4)
    wild = (rng.integers(0, 2, D.shape) * 65534 - 32767).astype(np.int32)
    _, pos, info = ref.pull_ref(volume, sshape, IDENTITY, IDENTITY, wild, 4, 8)
    assert np.isfinite(pos).all() and (info[0] == 0 or info[1] > 0), info


# ---- the quality of the definition -------------------------------------------------------------------------------------------------------
def test_the_fitted_field_of_the_warped_ellipsoid_does_not_fold_and_its_inverse_converges():
    """Measured on the restatement, on warp_ref.warped_fit() (subject (38, 44, 40), template (36, 48, 40), g = 4, TRUE_MAP, det(M) =
    1.0987): the largest |G| is 3872; det runs from 0.6098 to 1.7426 over the 66880 subject voxels, none folded, mean 1.0869 over
    the foreground.  The largest residual |map(s) + e(s) - u| over the template voxels whose s is inside the subject is 3.71 at 0
    rounds, 0.92, 0.25, 0.073 (21 voxels above 1/16) after 1, 2, 3, then 0.023 at 4, 0.0028 at 6, 0.00037 at 8 and 1.1e-5 at 12;
    60091 of 69120 template voxels land inside at 8 rounds.  The subject tissue map pulled onto the template grid agrees with the
    template's own with Dice 0.7408 through inv alone and 0.9415 through 8 rounds.  Every figure equals the issue's prototype.  The
    floors asserted are the issue's."""
    subject, template = wr.warped_case()
    D, _ = wr.warped_fit()
    geo = ref.warped_geometry()
    det, info = geo["det"], geo["info"]
    G = ref.derivatives(D, 4, *counted(subject.shape, 1))
    fg = float(det[np.asarray(subject) > 0].astype(np.float64).mean())
    print("max |G| %d; det %.4f .. %.4f, folded %d, foreground mean %.4f" % (np.abs(G).max(), det.min(), det.max(), info[1], fg))
    assert info[0] == det.size == 66880 and info[1] == 0 and ref.unkey(info[2]) == det.min() > 0 and ref.unkey(info[3]) == det.max()
    assert DF.summary(info) == dict(voxels=66880, folded=0, det_min=float(det.min()), det_max=float(det.max()))
    assert abs(float(np.abs(G).max()) - 3872) < 1 and 0.55 < det.min() < 0.652 and 1.5 < det.max() < 2 and abs(fg - 1.0869) < 1e-3
    rel = DF.relative(det, TRUE_MAP)
    assert abs(rel.mean() * 1.0987 - det.astype(np.float64).mean()) < 1e-3
    # the inverse
    inside, _ = ref.nearest_inside(list(geo["pos"].reshape(3, -1)), subject.shape)
    res = geo["residual"][:, inside]
    affine, _, ainfo = ref.pull_ref(subject, template.shape, TRUE_MAP, geo["inv"], None, 4, 8)
    ainside, _ = ref.nearest_inside(wr.affine_ref(geo["inv"], *counted(template.shape, 1)), subject.shape)
    before = ref.dice_labels(affine.reshape(-1), np.asarray(template).reshape(-1), ainside)
    after = ref.dice_labels(geo["out"].reshape(-1), np.asarray(template).reshape(-1), inside)
    print("8 rounds: residual %.3g, inside %d of %d, not converged %d; Dice %.4f -> %.4f" % (
        res.max(), geo["pull_info"][0], inside.size, geo["pull_info"][1], before, after))
    assert geo["pull_info"].tolist() == [int(inside.sum()), 0] == [60091, 0] and ainfo.tolist() == [int(ainside.sum()), 0]
    assert res.max() < 1 / 256
    assert before < 0.80 and after >= 0.90
    # three rounds are not enough, four are: the count of the kernel says which
    for k, (lo, hi) in ((0, (1000, 69120)), (3, (1, 100)), (4, (0, 0))):
        _, _, kinfo = ref.pull_ref(subject, template.shape, TRUE_MAP, geo["inv"], D, 4, k)
        assert lo <= kinfo[1] <= hi, (k, kinfo)
