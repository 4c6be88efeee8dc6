"""CPU: the float64 layer references of tests/layer_ref.py against torch's float64 autograd and the C oracle, and the conditions the input
generators of tests/layer_cases.py promise for every case of tests/test_gpu_layer_ops.py -- what the GPU tests rely on holds before a GPU
is involved."""
import ctypes as ct

import numpy as np
import pytest
import torch

import layer_cases as LC  # noqa: E402
import layer_ref as R  # noqa: E402

import unet_studio_amd as U  # noqa: E402
from oracle import oracle as O  # noqa: E402

F = torch.nn.functional


def t64(a):
    return torch.from_numpy(np.array(a, np.float64))


def cf(x):     # [D][H][W][C] -> torch [1][C][D][H][W]
    return t64(x).permute(3, 0, 1, 2)[None]


def cl(t):     # back
    return t[0].permute(1, 2, 3, 0).detach().numpy()


def act_t(z, a):
    return {0: lambda v: v, 1: torch.relu, 2: lambda v: F.leaky_relu(v, 0.01), 3: F.elu}[a](z)


def close(a, b, tol=1e-11):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape
    assert np.allclose(a, b, rtol=tol, atol=tol * (np.abs(b).max() + 1e-300), equal_nan=True), float(np.nanmax(np.abs(a - b)))


@pytest.mark.parametrize("a", [0, 1, 2, 3])
def test_activations_against_torch_and_the_conventions_at_zero(a):
    z = np.random.default_rng(a).standard_normal(1000) * 3
    zt = t64(z).requires_grad_(True)
    y = act_t(zt, a)
    y.sum().backward()
    close(R.act(z, a), y.detach().numpy())
    close(R.act_d(z, a), zt.grad.numpy())
    assert R.act(np.zeros(1), a)[0] == 0.0
    assert R.act_d(np.zeros(1), a)[0] == {0: 1.0, 1: 0.0, 2: 0.01, 3: 1.0}[a]      # elu' = exp(0)


@pytest.mark.parametrize("kind,S,C", [("in", 37, 5), ("bn", 37, 5), ("bn_eval", 37, 5), ("in", 1, 3), ("bn", 3, 4)])
@pytest.mark.parametrize("a", [0, 1, 2, 3])
def test_norm_against_torch_autograd(kind, S, C, a):
    rng = np.random.default_rng(S * 10 + C + a)
    u = rng.standard_normal((S, C)) + np.where(np.arange(C) % 4 == 1, 32.0, 0.3)
    gamma, beta = 1 + 0.2 * rng.standard_normal(C), 0.3 * rng.standard_normal(C)
    rm, rv, g = rng.standard_normal(C), 0.5 + rng.random(C), rng.standard_normal((S, C))
    eps = R.EPS[kind]
    f = R.norm_fwd(u, gamma, beta, eps, None if kind == "in" else rm, None if kind == "in" else rv, use_running=kind == "bn_eval")
    ut, gt, bt = t64(u).requires_grad_(True), t64(gamma).requires_grad_(True), t64(beta).requires_grad_(True)
    x5 = ut.t().reshape(1, C, S)      # (as [1][C][S][1][1] torch's CPU backward takes the tensor for channels-last and returns other numbers)
    if kind == "in" and S == 1:      # (torch refuses one voxel: the definition, written out)
        y = ((x5 - x5.mean(2, keepdim=True)) / torch.sqrt(x5.var(2, unbiased=False, keepdim=True) + eps)) * gt[None, :, None] + bt[None, :, None]
    elif kind == "in":
        y = F.instance_norm(x5, weight=gt, bias=bt, eps=eps)
    else:
        rmt, rvt = t64(rm), t64(rv)     # (torch refuses eps = 0: 1e-30 next to variances near 1 is 0 in float64)
        y = F.batch_norm(x5, rmt, rvt, gt, bt, training=kind == "bn", momentum=R.MOMENTUM, eps=1e-30)
        close(f["rm"], rmt.numpy())
        close(f["rv"], rvt.numpy())
    out = act_t(y, a)
    (out.reshape(C, S).t() * t64(g)).sum().backward()
    close(R.view(u, f["scale"], f["shift"], a), out.reshape(C, S).t().detach().numpy())
    if kind == "bn_eval":
        return
    b = R.norm_bwd(g, u, f["mean"], f["rstd"], f["scale"], f["shift"], gamma, a)
    tol = 1e-9 if S > 1 else 1e-6       # (one voxel: rstd = 316, the gradient is an exact 0 that autograd reaches by cancellation)
    close(b["du"], ut.grad.numpy(), tol)
    close(b["dgamma"], gt.grad.numpy(), tol)
    close(b["dbeta"], bt.grad.numpy(), tol)
    close(b["c0"], gamma * f["rstd"])


@pytest.mark.parametrize("C,S", [(3, 50), (8, 7)])
def test_norm_against_the_c_oracle(C, S):
    rng = np.random.default_rng(C * S)
    x = rng.standard_normal((C, S)).astype(np.float32)
    gamma, beta = (1 + 0.2 * rng.standard_normal(C)).astype(np.float32), rng.standard_normal(C).astype(np.float32)
    rm, rv = rng.standard_normal(C).astype(np.float32), (0.5 + rng.random(C)).astype(np.float32)
    dy = rng.standard_normal((C, S)).astype(np.float32)
    for eps, running in ((1e-5, False), (0.0, True)):
        y, mean, rstd = np.empty((C, S), np.float32), np.empty(C, np.float32), np.empty(C, np.float32)
        rmo, rvo = rm.copy(), rv.copy()
        O.lib().orc_norm_fwd(O._f(x), O._f(gamma), O._f(beta), O._f(y), O._f(mean), O._f(rstd), C, ct.c_int64(S), ct.c_double(eps),
                             O._f(rmo) if running else None, O._f(rvo) if running else None, ct.c_double(R.MOMENTUM))
        f = R.norm_fwd(x.T, gamma, beta, eps, rm if running else None, rv if running else None)
        close(f["mean"], mean, 1e-6)
        close(f["rstd"], rstd, 1e-6)
        close(R.view(x.T, f["scale"], f["shift"], 0).T, y, 1e-6)
        if running:
            close(f["rm"], rmo, 1e-6)
            close(f["rv"], rvo, 1e-6)
        dx, dg, db = np.empty((C, S), np.float32), np.ones(C, np.float32), np.ones(C, np.float32)
        O.lib().orc_norm_bwd(O._f(x), O._f(dy), O._f(gamma), O._f(mean), O._f(rstd), O._f(dx), O._f(dg), O._f(db), C, ct.c_int64(S))
        b = R.norm_bwd(dy.T, x.T, mean, rstd, gamma * rstd, beta - mean * gamma * rstd, gamma, 0)
        close(b["du"].T, dx, 1e-5)
        close(b["dgamma"] + 1, dg, 1e-5)
        close(b["dbeta"] + 1, db, 1e-5)


@pytest.mark.parametrize("a", [1, 2, 3])
def test_activations_against_the_c_oracle(a):
    x = np.concatenate([np.random.default_rng(a).standard_normal(500), [0.0]]).astype(np.float32)
    dy = np.random.default_rng(a + 9).standard_normal(501).astype(np.float32)
    y, dx = np.empty_like(x), np.empty_like(x)
    O.lib().orc_act_fwd(O._f(x), O._f(y), ct.c_int64(x.size), a)
    O.lib().orc_act_bwd(O._f(x), O._f(dy), O._f(dx), ct.c_int64(x.size), a)
    close(R.act(x, a), y, 1e-6)
    close(dy * R.act_d(x, a), dx, 1e-6)


def pool_volumes():
    for C_, dims in LC.VOLUME_CASES:
        v = LC.volume_inputs(C_, dims)
        yield (C_, dims, "grid"), v.x, v.gc
        if v.xn is not None:
            yield (C_, dims, "nan"), v.xn, v.gc


@pytest.mark.parametrize("name,x,gc", list(pool_volumes()), ids=lambda p: "%dx%s_%s" % (p[0], "x".join(map(str, p[1])), p[2]) if isinstance(p, tuple) else "")
def test_pool_against_torch_and_the_c_oracle(name, x, gc):
    C_, (D, H, W), what = name
    y, arg = R.maxpool_fwd(x)
    dx = R.maxpool_bwd(gc, arg, x.shape)
    xt = cf(x).requires_grad_(True)
    yt = F.max_pool3d(xt, 2, 2)
    close(y, cl(yt))
    if what == "grid":      # (torch's CPU kernel also gives a tied window's gradient to the first maximum; with NaN it is not asked)
        (yt * cf(gc)).sum().backward()
        close(dx, cl(xt.grad))
    x32 = np.ascontiguousarray(np.transpose(x, (3, 0, 1, 2)), np.float32)
    g32 = np.ascontiguousarray(np.transpose(gc, (3, 0, 1, 2)), np.float32)
    yo, ao = np.empty((C_, D // 2, H // 2, W // 2), np.float32), np.empty((C_, D // 2, H // 2, W // 2), np.int32)
    dxo = np.empty((C_, D, H, W), np.float32)
    O.lib().orc_maxpool_fwd(O._f(x32), O._f(yo), ao.ctypes.data_as(ct.POINTER(ct.c_int32)), C_, D, H, W)
    O.lib().orc_maxpool_bwd(O._f(g32), ao.ctypes.data_as(ct.POINTER(ct.c_int32)), O._f(dxo), C_, D, H, W)
    close(y, np.transpose(yo, (1, 2, 3, 0)))
    close(dx, np.transpose(dxo, (1, 2, 3, 0)))        # the oracle sends a NaN window's gradient to its last NaN as well
    for ax, n in enumerate((D, H, W)):
        if n % 2:
            assert not np.take(dx, n - 1, ax).any(), "the trailing plane of an odd extent takes no gradient"


def test_pool_ties_and_nan_by_hand():
    x = np.zeros((2, 2, 2, 1))
    x[0, 1, 0, 0] = x[1, 0, 1, 0] = 3.0          # elements 2 and 5
    y, arg = R.maxpool_fwd(x)
    assert y[0, 0, 0, 0] == 3.0 and arg[0, 0, 0, 0] == 2
    g = np.full((1, 1, 1, 1), 7.0)
    assert R.maxpool_bwd(g, arg, x.shape)[0, 1, 0, 0] == 7.0
    assert R.maxpool_bwd(g, arg, x.shape, second=True, x=x)[1, 0, 1, 0] == 7.0
    x[0, 0, 1, 0] = x[1, 1, 0, 0] = np.nan       # elements 1 and 6: a NaN wins, the last one takes the gradient
    y, arg = R.maxpool_fwd(x)
    assert np.isnan(y[0, 0, 0, 0]) and arg[0, 0, 0, 0] == 6
    x[:] = 1.5                                   # all equal: the first
    assert R.maxpool_fwd(x)[1][0, 0, 0, 0] == 0


@pytest.mark.parametrize("C_,dims", LC.VOLUME_CASES)
def test_upsample_concat_export_against_torch_and_the_c_oracle(C_, dims):
    v = LC.volume_inputs(C_, dims)
    D, H, W = dims
    xt = cf(v.x).requires_grad_(True)
    yt = F.interpolate(xt, scale_factor=2, mode="nearest")
    (yt * cf(v.gf)).sum().backward()
    close(R.upsample_fwd(v.x), cl(yt))
    close(R.upsample_bwd(v.gf), cl(xt.grad))
    x32 = np.ascontiguousarray(np.transpose(v.x, (3, 0, 1, 2)), np.float32)
    g32 = np.ascontiguousarray(np.transpose(v.gf, (3, 0, 1, 2)), np.float32)
    yo, dxo = np.empty((C_, 2 * D, 2 * H, 2 * W), np.float32), np.empty((C_, D, H, W), np.float32)
    O.lib().orc_upsample_fwd(O._f(x32), O._f(yo), C_, D, H, W)
    O.lib().orc_upsample_bwd(O._f(g32), O._f(dxo), C_, D, H, W)
    close(R.upsample_fwd(v.x), np.transpose(yo, (1, 2, 3, 0)))
    close(R.upsample_bwd(v.gf), np.transpose(dxo, (1, 2, 3, 0)))
    # concat of two views, its backward, export and import
    e, n = LC.exact_view(C_), LC.norm_view(C_, 3)
    a, b = t64(v.x).requires_grad_(True), t64(v.old).requires_grad_(True)
    cat = torch.cat([torch.relu(a * t64(e.scale) + t64(e.shift)), F.elu(b * t64(n.scale) + t64(n.shift))], -1)
    close(R.concat([R.view(v.x, e.scale, e.shift, 1), R.view(v.old, n.scale, n.shift, 3)]), cat.detach().numpy())
    gcat = np.concatenate([v.gs, v.old], -1)
    d0, d1 = R.concat_bwd(gcat, (C_, C_))
    assert np.array_equal(d0, v.gs) and np.array_equal(d1, v.old)
    ex = R.export(v.x)
    assert ex.shape == (C_, D * H * W) and np.array_equal(ex, cf(v.x)[0].reshape(C_, -1).numpy())
    assert np.array_equal(R.import_grad(ex, v.old.reshape(-1, C_)), (v.x + v.old).reshape(-1, C_))


# ---- the generators' conditions, for every GPU case ----
@pytest.mark.parametrize("case", LC.NORM_CASES + [c + ("bn_eval",) for c in LC.EVAL_CASES], ids=lambda c: "_".join(map(str, c)))
def test_norm_inputs_keep_their_promises(case):
    dt, C_, S = case[:3]
    for kind in (case[3:] or LC.NORM_KINDS):
        if S == 1 and kind != "in":
            continue
        d = LC.norm_inputs(dt, C_, S, kind)
        assert d.u.shape == d.g.shape == (S, C_)
        assert np.array_equal(LC.quant(d.u, dt), d.u) and np.array_equal(LC.quant(d.g, dt), d.g), "the element type holds the inputs"
        assert np.all(LC.kink_clear(d.u, d.stat[2], d.stat[3])), "a voxel within the kink margin"
        f = R.norm_fwd(d.u, d.gamma, d.beta, R.EPS[kind], d.rm, d.rv, use_running=kind == "bn_eval")
        assert np.array_equal(LC.stat_row(f), d.stat), "the stat row is that of the stored u"
        if S >= 64 and C_ >= 2 and kind != "bn_eval":
            far = np.abs(f["mean"]) * f["rstd"]
            # (32 as drawn; moving the middle of the distribution out of the kink margin, itself 2^-6 |mean scale| wide, widens the spread)
            assert far[1::4].min() >= LC.FAR_MEAN, "every fourth channel has its mean far outside its spread"
        assert np.all(np.isfinite(d.stat)) and np.all(f["var"] > 0 if S > 1 else True)


def test_norm_case_table_is_consistent():
    assert len(set(LC.NORM_CASES)) == len(LC.NORM_CASES) == 26
    for i, forms in enumerate(LC.STEPS):
        assert {LC.NORM_FORMS[c][i] for c in LC.NORM_CASES} == set(forms), "a form of step %d is named by no case" % i
    for dt, C_, S in LC.NORM_CASES:       # the rows boundary the table is built around
        assert (LC.stats_rows(S) <= 128) == (S <= 4096)
    assert all(c in LC.NORM_CASES for c in LC.EVAL_CASES)


def test_norm_choice_matches_the_case_table():
    """unet_op_norm_choice launches nothing, so the claim of every case can be held against the engine's own predicates here too"""
    for dt, C_, S in LC.NORM_CASES:
        out = (ct.c_int * 5)()
        U.engine.check(U.engine.lib.unet_op_norm_choice(1 if dt == "bf16" else 0, C_, S, out))
        got = tuple(LC.STEPS[i][out[i]] for i in range(5))
        assert got == LC.NORM_FORMS[(dt, C_, S)], "%s: the engine takes %s (%s)" % ((dt, C_, S), got, LC.NORM_WHY[(dt, C_, S)])
    with pytest.raises(U.engine.UNetError):
        U.engine.check(U.engine.lib.unet_op_norm_choice(1, 0, 10, (ct.c_int * 5)()))


@pytest.mark.parametrize("C_,dims", LC.VOLUME_CASES)
def test_volume_inputs_keep_their_promises(C_, dims):
    v = LC.volume_inputs(C_, dims)
    for name in ("x", "gc", "gs", "gf", "old", "old_fine"):
        a = getattr(v, name)
        assert np.array_equal(a * 8, np.rint(a * 8)) and np.abs(a).max() <= 9 / 8, name
    assert LC.tied_windows(v.x) > 0, "no tied window"
    y, arg = R.maxpool_fwd(v.x)
    assert not np.array_equal(R.maxpool_bwd(v.gc + 2, arg, v.x.shape), R.maxpool_bwd(v.gc + 2, arg, v.x.shape, second=True, x=v.x))
    if (C_, dims) == LC.ALL_EQUAL_CASE:
        assert np.ptp(R._windows(v.x)[1, 1, 1]) == 0
    if (C_, dims) == LC.NAN_CASE:
        assert np.isnan(R._windows(v.xn)[1, 1, 1, :, 2]).sum() == 2 and R.maxpool_fwd(v.xn)[1][1, 1, 1, 2] == 6
    # every exact result is a bf16 value: sums of up to nine grid values, views that stay on the grid
    e = LC.exact_view(C_)
    for r in (R.upsample_bwd(v.gf) + v.old, R.maxpool_bwd(v.gc, arg, v.x.shape) + v.old, R.view(v.x, e.scale, e.shift, 1), v.gs + v.old):
        assert np.array_equal(LC.bf16_round(r), r)
    assert C_ < 5 or (R.view(v.x, e.scale, e.shift, 0) == 0).any(), "the exact view has post-affine zeros"
    for a in (1, 2, 3):
        n = LC.norm_view(C_, a)
        assert np.all(LC.kink_clear(v.x, n.scale, n.shift)) and np.array_equal(LC.f32(n.scale), n.scale)


@pytest.mark.parametrize("c0,c1", LC.CONCAT_CASES)
def test_concat_inputs_keep_their_promises(c0, c1):
    d = LC.concat_inputs(c0, c1)
    for a in (d.x0, d.x1, d.gout, d.o0, d.o1):
        assert np.array_equal(a * 8, np.rint(a * 8)) and np.abs(a).max() <= 1
    for name, v0, v1 in d.views:
        for x, v in ((d.x0, v0), (d.x1, v1)):
            if v is None:
                continue
            if name == "norm":
                assert np.all(LC.kink_clear(x, v.scale, v.shift)), "a voxel within the kink margin"
                assert np.array_equal(LC.f32(v.scale), v.scale) and np.array_equal(LC.f32(v.shift), v.shift)
            else:
                r = R.view(x, v.scale, v.shift, v.act)
                assert np.array_equal(LC.bf16_round(r), r)
    (_, a0, a1), (_, b0, b1) = d.views
    assert b0.act != b1.act and not np.array_equal(b0.scale[:5], b1.scale[:5]), "the two sources have different views"
    for r, o in zip(R.concat_bwd(d.gout, (c0, c1)), (d.o0, d.o1)):
        assert np.array_equal(LC.bf16_round(r + o), r + o)


@pytest.mark.parametrize("dt", LC.DTYPES)
def test_pool_kink_windows_are_won_by_the_voxel_on_the_kink(dt):
    k = LC.kink_pool_inputs(dt)
    w = R._windows(k.special.astype(np.float64))
    assert np.all(w.sum(3) == 1) and not w[:, :, :, 0].any(), "one voxel on the kink per window, never its first element"
    gc = np.ones(w.shape[:3] + w.shape[4:])
    for a in (1, 2, 3):
        y, arg = R.maxpool_fwd(R.act(k.z, a))
        assert np.array_equal(y, np.take_along_axis(R._windows(R.act(k.z, a)), np.argmax(w, 3)[:, :, :, None], 3)[:, :, :, 0])
        if a != 1:      # under leaky and elu the seven others are negative: the voxel on the kink alone holds the maximum
            assert np.array_equal(arg, np.argmax(w, 3))
        if dt == "fp32":    # taking the other side of the kink (the product rounded before the add) changes what the pool returns
            hit = y == 2.0 ** -24
            assert hit.sum() == hit.size // 2
            yw, argw = R.maxpool_fwd(R.act(k.wrong, a))
            assert np.all(yw[hit] == 0) and np.array_equal(yw[~hit], y[~hit])
            if a == 1:
                assert np.all(arg[hit] > 0) and np.all(argw[hit] == 0)
                assert not np.array_equal(R.maxpool_bwd(gc, arg, k.u.shape), R.maxpool_bwd(gc, argw, k.u.shape))


@pytest.mark.parametrize("dt", LC.DTYPES)
def test_kink_voxels_are_what_they_claim(dt):
    k = LC.kink_inputs(dt)
    assert (k.z == 0).any() and k.special.sum() >= k.u.size // 4
    if dt == "fp32":
        hit = k.z == 2.0 ** -24
        assert hit.any()
        prod = (k.u.astype(np.float32) * k.scale.astype(np.float32)).astype(np.float32)      # the product rounded first: a tie, to even
        assert np.all((prod + k.shift.astype(np.float32))[hit] == 0), "multiply-then-add does not give 0 there"
    assert np.all(LC.kink_clear(k.u, k.scale, k.shift) | k.special), "only the voxels built on purpose lie on the kink"


def test_bf16_round_is_round_to_nearest_even():
    x = np.random.default_rng(0).standard_normal(10000) * 100
    assert np.array_equal(LC.bf16_round(x), torch.from_numpy(x.astype(np.float32)).to(torch.bfloat16).double().numpy())
    assert LC.bf16_round(np.array([1 + 2.0 ** -8]))[0] == 1.0 and LC.bf16_round(np.array([1 + 3 * 2.0 ** -8]))[0] == 1 + 2.0 ** -6
