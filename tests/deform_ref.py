"""The numpy restatements of include/unet_deform.h, shared by tests/test_deform_host.py (which checks them on hand-written answers) and
tests/test_gpu_deform.py (which pins the device to them bit for bit): `jacobian_ref`, `field_at`, `pull_ref`, `inverse_map_ref`.
numpy only: nothing here calls the package's kernels.  The corner sums and the affine position are tests/warp_ref.py's; the trilinear
rule is oracle/augment_ref.py's, as in tests/cowarp_ref.py.  All position arithmetic is np.float32, one rounding per operation, left
to right as the header writes it; the derivatives are int64."""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import warp_ref as wr  # noqa: E402
from oracle import augment_ref as ar  # noqa: E402
from test_register_host import TRUE_MAP, counted  # noqa: E402

F = np.float32
MAX_ITERS = 32                                                     # written out: the restatements do not read the module's values
KEY_MIN0, KEY_MAX0 = 0xFFFFFFFF, 0                                 # the start values of the two extreme keys


def key(v):
    """the order-preserving key of float32 values, as Python-int-safe int64"""
    b = np.asarray(v, F).view(np.uint32).astype(np.int64)
    return np.where(b >> 31, b ^ 0xFFFFFFFF, b ^ 0x80000000)


def unkey(k):
    k = int(k)
    return float(np.array([k ^ (0x80000000 if k >> 31 else 0xFFFFFFFF)], np.uint32).view(F)[0])


def stored(v):
    """a float32 array as the device stores it: every NaN is the quiet NaN 0x7FC00000"""
    v = np.array(v, F)
    v.view(np.uint32)[np.isnan(v)] = 0x7FC00000
    return v


def derivatives(D, g, x, y, z):
    """G int64 {N, 3, 3}: G[:, r, a] the derivative of the corner sum n_r along axis a (x, y, z), exact integers"""
    D = np.asarray(D).astype(np.int64)
    lg = wr.LG[g]
    cx, cy, cz, fx, fy, fz = x >> lg, y >> lg, z >> lg, x & (g - 1), y & (g - 1), z & (g - 1)
    G = np.zeros((x.size, 3, 3), np.int64)
    for c in range(8):
        dx, dy, dz = c & 1, (c >> 1) & 1, c >> 2
        wx, wy, wz = (fx if dx else g - fx), (fy if dy else g - fy), (fz if dz else g - fz)
        v = D[cz + dz, cy + dy, cx + dx]                            # {N, 3}
        for a, w in enumerate(((1 if dx else -1) * wy * wz, (1 if dy else -1) * wx * wz, (1 if dz else -1) * wx * wy)):
            G[:, :, a] += w[:, None] * v
    return G


def jacobian_ref(sshape, map12, D, g):
    """-> (det float32 of sshape, info int64 {4} = voxels, folded, key of the smallest det, key of the largest)"""
    m = np.asarray(map12, F).reshape(12)
    x, y, z = counted(sshape, 1)
    G = derivatives(D, g, x, y, z)
    assert np.abs(G).max(initial=0) <= g * g * 65534
    with np.errstate(all="ignore"):
        J = [[m[3 * r + c] + np.ldexp(G[:, r, c].astype(F), -(8 + 3 * wr.LG[g])) for c in range(3)] for r in range(3)]
        (a, b, c), (d, e, f), (g_, h, i) = J
        det = (a * (e * i - f * h) - b * (d * i - f * g_)) + c * (d * h - e * g_)
    assert det.dtype == F
    ok = ~np.isnan(det)
    with np.errstate(invalid="ignore"):
        folded = int((~(det > 0)).sum())
    k = key(det[ok])
    info = np.array([det.size, folded, k.min(initial=KEY_MIN0), k.max(initial=KEY_MAX0)], np.int64)
    return stored(det).reshape(sshape), info


def cell(s, g, n):
    """(c int64, f float32) of positions s along an axis of n nodes"""
    with np.errstate(all="ignore"):
        t = np.asarray(s, F) * F(1.0 / g)
        t = np.where(t > 0, t, F(0)).astype(F)
        t = np.where(t < F(n - 1), t, F(n - 1)).astype(F)
        c = np.minimum(np.floor(t).astype(np.int64), n - 2)
        f = t - c.astype(F)
    assert f.dtype == F
    return c, f


def field_at(D, g, s):
    """e = [e_0, e_1, e_2] float32 {N} each: the continuous field at subject positions s = [s_x, s_y, s_z] (float32 {N} each)"""
    D = np.asarray(D)
    nz, ny, nx = D.shape[:3]
    (cx, fx), (cy, fy), (cz, fz) = cell(s[0], g, nx), cell(s[1], g, ny), cell(s[2], g, nz)
    lerp = lambda t, a, b: a + t * (b - a)  # noqa: E731
    out = []
    with np.errstate(all="ignore"):
        for r in range(3):
            at = lambda dx, dy, dz: D[cz + dz, cy + dy, cx + dx, r].astype(F)  # noqa: E731
            c00, c10 = lerp(fx, at(0, 0, 0), at(1, 0, 0)), lerp(fx, at(0, 1, 0), at(1, 1, 0))
            c01, c11 = lerp(fx, at(0, 0, 1), at(1, 0, 1)), lerp(fx, at(0, 1, 1), at(1, 1, 1))
            e = lerp(fz, lerp(fy, c00, c10), lerp(fy, c01, c11)) * F(1.0 / 256)
            assert e.dtype == F
            out.append(e)
    return out


def inverse_map_ref(map12):
    """float32 {12}: the inverse in float64, rounded once"""
    m = np.asarray(map12, F).reshape(12).astype(np.float64)
    a = np.linalg.inv(m[:9].reshape(3, 3))
    return np.concatenate([a.reshape(9), -(a @ m[9:])]).astype(F)


def mix(m, v):
    """((m[3r] v0 + m[3r+1] v1) + m[3r+2] v2) per row r, without the translation"""
    with np.errstate(all="ignore"):
        return [(m[3 * r] * v[0] + m[3 * r + 1] * v[1]) + m[3 * r + 2] * v[2] for r in range(3)]


def nearest_inside(s, sshape):
    sd, sh, sw = sshape
    with np.errstate(all="ignore"):
        q = [v + F(0.5) for v in s]
        inside = (q[0] >= 0) & (q[1] >= 0) & (q[2] >= 0) & (q[0] < F(sw)) & (q[1] < F(sh)) & (q[2] < F(sd))
        idx = [np.where(inside, np.floor(v), 0).astype(np.int64) for v in q]
    return inside, idx


def pull_ref(volume, tshape, map12, inv12, D, g, iters, residual_out=None):
    """-> (out of tshape in the volume's dtype, pos float32 {3} + tshape, info int64 {2} = inside, not converged).  D None: the affine
    inverse alone.  residual_out: a list that receives |(map(s) + e(s)) - u| float32 {3, N}"""
    volume = np.asarray(volume)
    assert 0 <= iters <= MAX_ITERS and volume.dtype in (np.float32, np.uint8, np.uint16)
    m, inv = np.asarray(map12, F).reshape(12), np.asarray(inv12, F).reshape(12)
    x, y, z = counted(tshape, 1)
    u = [v.astype(F) for v in (x, y, z)]
    s0 = wr.affine_ref(inv, x, y, z)
    s = list(s0)
    e = [np.zeros(x.size, F)] * 3
    with np.errstate(all="ignore"):
        if D is not None:
            for _ in range(iters):
                e = field_at(D, g, s)
                back = mix(inv, e)
                s = [s0[r] - back[r] for r in range(3)]
            e = field_at(D, g, s)
        fwd = mix(m, s)
        res = np.stack([np.abs(((fwd[r] + m[9 + r]) + e[r]) - u[r]) for r in range(3)])
    assert all(v.dtype == F for v in s) and res.dtype == F
    inside, idx = nearest_inside(s, volume.shape)
    if volume.dtype == np.float32:
        sd, sh, sw = volume.shape
        out = ar._trilinear(volume, ar._locate(s[0], s[1], s[2], sw, sh, sd))
    else:
        out = np.where(inside, volume[idx[2], idx[1], idx[0]], 0).astype(volume.dtype)
    with np.errstate(invalid="ignore"):
        open_ = inside & ~(res <= F(0.0625)).all(0)
    if residual_out is not None:
        residual_out.append(res)
    info = np.array([int(inside.sum()), int(open_.sum())], np.int64)
    return out.reshape(tshape), stored(np.stack(s)).reshape((3,) + tuple(tshape)), info


def dice_labels(a, b, where):
    """the Dice of the foregrounds of two label maps that agree in label, counted where `where`"""
    a, b = np.asarray(a)[where], np.asarray(b)[where]
    return 2.0 * int(((a == b) & (a > 0)).sum()) / (int((a > 0).sum()) + int((b > 0).sum()))


# ---- the shared case: the fitted field of the warped ellipsoid ---------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def warped_geometry(iters=8):
    """On warp_ref.warped_fit() (subject (38, 44, 40), template (36, 48, 40), g = 4, TRUE_MAP): dict(det, info, out (the subject
    tissue map pulled, U8), pos, pull_info, residual {3, N}, inv), computed once and left unchanged"""
    subject, template = wr.warped_case()
    D, _ = wr.warped_fit()
    inv = inverse_map_ref(TRUE_MAP)
    det, info = jacobian_ref(subject.shape, TRUE_MAP, D, 4)
    res = []
    out, pos, pinfo = pull_ref(subject, template.shape, TRUE_MAP, inv, D, 4, iters, residual_out=res)
    got = dict(det=det, info=info, out=out, pos=pos, pull_info=pinfo, residual=res[0], inv=inv)
    for a in got.values():
        a.setflags(write=False)
    return got
