"""GPU (-m gpu): the layer kernels of csrc/kernels_elem.hip, one op at a time, against the float64 references of tests/layer_ref.py.

The entries unet_op_norm_fwd / _bwd, unet_op_view / _view_bwd, unet_op_apply_view, unet_op_act_bwd, unet_op_maxpool_*, unet_op_upsample_*,
unet_op_export_view and unet_op_import_grad (include/unet_hip.h) launch through the functions the executor launches through.  Every
output is a Guarded buffer (tests/gpu_exact.py: NaN inside, a byte pattern around), the scratch is 0xFF bytes, and the guards are checked
after every call.  The shapes, the branch each is there for and the input generators are in tests/layer_cases.py; the conditions the
generators promise are asserted without a GPU in tests/test_layer_ref_host.py.

Exact where the operation is exact.  Pool, upsample, concat, export and import move values or add a few: on data k / 8, |k| <= 9, with no
view or with a relu view that stays on that grid, every fp32 sum is exact in any order and bf16 holds the result, so the output must
equal the single rounding of the float64 reference bit for bit -- forward, and backward written or added onto an older gradient.  Which
voxel of a tied window takes the gradient is exact under any view: equal inputs give equal view values in fp32 as in float64.

Bounds where it is not (eps32 = 2^-24, the fp32 unit roundoff; a bf16 store is half an ulp, <= 2^-8 |ref|):
  * a view value act(fma(x, scale, shift)): the fma rounds once (2^-24 |z|), leaky multiplies by 0.01f (two roundings), expm1f is within
    a few ulp: 2^-23 |z| + 2^-21 |ref| in fp32, plus 2^-8 |ref| (1 + 2^-10) where it is stored as bf16; a window's maximum moves by no
    more than its elements do;
  * act backward g act'(u): 2^-21 |ref| (0.01f, expf) plus the bf16 store;
  * the norm forward, bf16: the bounds of tests/test_gpu_norm_epilogues.py -- fp32 sums per thread, fp64 across: 1e-5 of A = sum|u| / S on
    the mean, dvar = 1e-5 (B + 2 |mean| A) (B = sum u^2 / S) on E[u^2] - mean^2, 0.5 dvar / (var + eps) + 1e-6 relative on rstd and scale,
    shift = beta - mean scale adds the two, the running statistics scale them by the momentum (+ 1e-6 of the terms);
    fp32: the rows are fp64 sums of exact products (relative 2^-36 with margin for 40000 terms) and only the rounding of each result to
    fp32 remains: the same formulas with 2^-36 for 1e-5 and 2^-23 for 1e-6;
  * the activated copy, from the kernel's own stat row: the view bound above;
  * the norm backward from the stat row it is given, bf16 as in the epilogue test: coef0 1e-6 relative; m1, m2, dgamma, dbeta 1e-4 of the
    sum of |terms| (+ 2^-23 |1 + sum| for the += onto 1.0); dL/d(raw) 2^-8 |ref| + 1e-3 max|ref| + 2^-20 |c0| (|dv| + |m1| + |m2| rstd (|u| +
    |mean|)) for the fp32 evaluation whose terms cancel, the max taken apart over the voxels whose gradient the generator draws 16 times
    larger and over the rest, so that the ordinary voxels keep the epilogue test's bound;
    fp32: dv and xhat are fp32 (one rounding, two roundings, expf within a few ulp of a pre-activation itself within 2^-24 |z|) and the
    sums fp64: 2^-20 of the sum of |terms|, coef0 2^-23 relative, dL/d(raw) 2^-22 |ref| + the same cancellation term + |c0| (bound(m1) +
    |xhat| bound(m2)).
No bound was fixed from what a kernel returned; the worst error-to-bound ratio of every quantity is printed (test_zz_report).

The mean dwarfs the spread: every fourth channel of a norm case is drawn with its mean 32 standard deviations out; moving voxels out of
the kink margin (half a gamma wide there) widens the spread, and as stored the mean is at least 22 standard deviations out in every
case (asserted in the host test).  The bounds carry the |mean| terms, so they hold there as well.

Kinks: the generators keep |u scale + shift| >= 2^-7 (|u scale| + |shift|) at every voxel, so no voxel is left out of any comparison.
test_voxels_on_the_kink has the exception: pre-activations of exactly 0, and fp32 voxels whose exact pre-activation is 2^-24 > 0 where a
product rounded before the add gives 0.  Through every forward that reads a view (materialize, apply_view in both vector forms,
upsample, export, and the pool on windows built so that the voxel on the kink wins them, forward and backward) the value, and through
the norm backward the derivative, must be those of the float64 reference.  At a pre-activation of exactly 0 every activation gives 0
on either side, so there a forward cannot tell the sides apart and the derivative check carries the case; bf16 has only such voxels.

Teeth: wrong references built in numpy -- statistics without voxels 32..63, without the last statistics row, channel c from c + 8, a
tied window's gradient at the second maximum, the concat sources swapped, accumulate ignored, relu' = 1 at 0 -- must miss the bounds by
10x (an exact comparison: differ after rounding).

Determinism: every norm case runs twice into NaN-filled outputs; the results must be bit-identical.

Not covered: BatchNorm in training at one voxel (the variance is 0 and eps is 0), as in the epilogue test."""
import ctypes as ct

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import unet_studio_amd as U  # noqa: E402

import gpu_exact as X  # noqa: E402
import layer_cases as LC  # noqa: E402
import layer_ref as R  # noqa: E402
from gpu_exact import DEV, TDT, Guarded, assert_exact, check_all  # noqa: E402

E = U.engine
L = E.lib
EDT = {"fp32": U.DTYPE_F32, "bf16": U.DTYPE_BF16}
F32 = torch.float32
RATIOS = {}
# the constants of the bounds (module docstring): sums, relative rounding of a result, backward sums, stored tensors
K = {"bf16": dict(sum=1e-5, rel=1e-6, bsum=1e-4, store=2.0 ** -8 * (1 + 2.0 ** -10)),
     "fp32": dict(sum=2.0 ** -36, rel=2.0 ** -23, bsum=2.0 ** -20, store=0.0)}


def stream():
    return torch.cuda.current_stream(DEV).cuda_stream


def dev(a, dtype):
    return torch.from_numpy(np.array(a, order="C")).to(dtype).to(DEV)      # (a copy: the shared inputs are read-only)


def host(t):
    t = t.t if isinstance(t, Guarded) else t
    return t.detach().float().cpu().numpy().astype(np.float64)


def bits(t):
    t = (t.t if isinstance(t, Guarded) else t).detach().cpu().contiguous()
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32).numpy().copy()


def ptr(t):
    return None if t is None else t.data_ptr()


def guards(what, *named, finite=True):
    """gpu_exact.check_all over the buffers of a call that are there (a NULL argument is None); finite = False: the guard bands alone,
    for outputs that hold a NaN on purpose"""
    torch.cuda.synchronize()
    named = [(name, gb) for name, gb in named if gb is not None]
    if finite:
        check_all(what, *named)
    else:
        for name, gb in named:
            gb.check("%s %s" % (what, name), finite=False)


def view_args(x, C, v):
    """the five arguments of a source seen as a view (v: None, or scale / shift / act) and the tensors that must stay alive"""
    if v is None:
        return (x.data_ptr(), C, None, None, 0), ()
    sc, sh = dev(v.scale, F32), dev(v.shift, F32)
    return (x.data_ptr(), C, sc.data_ptr(), sh.data_ptr(), v.act), (sc, sh)


def view_ref(x, v):
    return R.view(x, None, None, 0) if v is None else R.view(x, v.scale, v.shift, v.act)


def view_bound(x, v, dt):
    """the bound of a stored view value (module docstring); 0 where the view is exact"""
    if v is None or (v.act == 1 and np.array_equal(v.scale, np.rint(v.scale))):
        return None
    ref = view_ref(x, v)
    return 2.0 ** -23 * np.abs(x * v.scale + v.shift) + (2.0 ** -21 + K[dt]["store"]) * np.abs(ref) + 1e-30


def note(name, r):
    RATIOS[name] = max(RATIOS.get(name, 0.0), float(r))


def check(name, got, ref, bound):
    got = np.asarray(got, np.float64)
    assert np.all(np.isfinite(got)), name + ": not finite"
    err = np.abs(got - ref)
    worst = float(np.max(err / bound))
    note(name, worst)
    assert worst <= 1.0, "%s: error %.3g of the bound (max abs err %.3g)" % (name, worst, float(err.max()))


def same(name, got, ref, bound):
    """bit equality with the rounded reference where bound is None, else the bound"""
    if bound is None:
        assert_exact(got.t if isinstance(got, Guarded) else got, ref, name)
    else:
        check(name, host(got), ref, bound)


def miss(wrong, ref, bound):
    return float(np.max(np.abs(np.asarray(wrong, np.float64) - ref) / bound))


def teeth(bug, r):
    assert r >= 10, "%s misses the bounds by only %.1fx" % (bug, r)


def differs(bug, wrong, ref, dt):
    """a wrong reference of an exact comparison must differ from the right one after the rounding to the element type"""
    assert not np.array_equal(LC.quant(wrong, dt), LC.quant(ref, dt), equal_nan=True), bug + " would pass the exact comparison"


def scratch_for(C, S):
    return X.poisoned_scratch(1, C, 1, 1, S)


def case_id(c):
    return "_".join("x".join(map(str, p)) if isinstance(p, tuple) else str(p) for p in c)


# ---------------------------------------------------------------------------------------------------------------------------------
def choice(dt, C, S):
    out = (ct.c_int * 5)()
    E.check(L.unet_op_norm_choice(EDT[dt], C, S, out))
    return tuple(LC.STEPS[i][out[i]] for i in range(5))


def test_cases_reach_the_form_they_name():
    """launches nothing: the engine's own predicates (unet_op_norm_choice) give every norm case the forms its row of the table names,
    and over all cases every form of every step is reached"""
    reached = [set() for _ in LC.STEPS]
    for c in LC.NORM_CASES:
        got = choice(*c)
        assert got == LC.NORM_FORMS[c], "%s (%s): the engine takes %s, the table says %s" % (c, LC.NORM_WHY[c], got, LC.NORM_FORMS[c])
        for i, f in enumerate(got):
            reached[i].add(f)
    for i, forms in enumerate(LC.STEPS):
        assert reached[i] == set(forms), "step %d: no case reaches %s" % (i, sorted(set(forms) - reached[i]))
    with pytest.raises(E.UNetError):
        E.check(L.unet_op_norm_choice(U.DTYPE_BF16, 8, 0, (ct.c_int * 5)()))


# ---------------------------------------------------------------------------------------------------------------------------------
# norm forward
def fwd_expect(d, f, kind, dt):
    """{name: (ref, bound)} of the stat row and the running statistics (module docstring)"""
    k = K[dt]
    S = d.u.shape[0]
    A, B = np.abs(d.u).sum(0) / S, (d.u * d.u).sum(0) / S
    eps = R.EPS[kind]
    mean, var, rstd, scale, shift = f["mean"], f["var"], f["rstd"], f["scale"], f["shift"]
    if kind == "bn_eval":
        r_rel, dmean = k["rel"] + 0 * rstd, k["rel"] * np.abs(mean)
    else:
        dvar = k["sum"] * (B + 2 * np.abs(mean) * A)
        r_rel, dmean = 0.5 * dvar / (var + eps) + k["rel"], k["sum"] * A + (k["rel"] * np.abs(mean) if dt == "fp32" else 0)
    exp = {"mean": (mean, dmean + 1e-30), "rstd": (rstd, r_rel * rstd), "scale": (scale, r_rel * np.abs(scale) + 1e-30),
           "shift": (shift, dmean * np.abs(scale) + np.abs(mean) * r_rel * np.abs(scale) + k["rel"] * (np.abs(d.beta) + np.abs(mean * scale)))}
    if kind == "bn":
        ub = S / (S - 1.0)
        exp["rm"] = (f["rm"], R.MOMENTUM * dmean + k["rel"] * ((1 - R.MOMENTUM) * np.abs(d.rm) + R.MOMENTUM * A))
        exp["rv"] = (f["rv"], R.MOMENTUM * ub * dvar + k["rel"] * ((1 - R.MOMENTUM) * d.rv + R.MOMENTUM * B * ub))
    return exp


def lost_rows(S):
    """(name, the voxels the sums still see) of the two lost-row bugs"""
    out = []
    if S >= 64:
        m = np.ones(S, bool)
        m[32:64] = False
        out.append(("statistics without voxels 32..63", m))
    if LC.stats_rows(S) > 1:
        m = np.ones(S, bool)
        m[(LC.stats_rows(S) - 1) * LC.stats_vpb(S):] = False
        out.append(("statistics without the last row", m))
    return out


def run_norm_fwd(dt, C, S, kind, a, d, ud, gd, bd, sc):
    bn = kind != "in"
    outs = []
    for _ in range(2):
        sc.t.fill_(0xFF)
        rm = Guarded((C,), F32, d.rm) if bn else None
        rv = Guarded((C,), F32, d.rv) if bn else None
        ya, stat = Guarded((S, C), TDT[dt]), Guarded((4, C), F32)
        E.check(L.unet_op_norm_fwd(EDT[dt], ud.data_ptr(), gd.data_ptr(), bd.data_ptr(), R.EPS[kind], ptr(rm), ptr(rv),
                                   1 if kind == "bn_eval" else 0, a, ya.data_ptr(), stat.data_ptr(), C, S, sc.data_ptr(), stream()))
        guards("norm forward", ("activated copy", ya), ("stat", stat), ("rm", rm), ("rv", rv), ("scratch", sc))
        outs.append({"ya": ya, "stat": stat, "rm": rm, "rv": rv})
    for k in outs[0]:
        if outs[0][k] is not None:
            assert np.array_equal(bits(outs[0][k]), bits(outs[1][k])), "%s differs between two identical calls" % k
    return {k: (host(v) if v is not None else None) for k, v in outs[0].items()}


def norm_fwd_case(dt, C, S, kind):
    d = LC.norm_inputs(dt, C, S, kind)
    f, ev = d.f, kind == "bn_eval"
    ud, gd, bd, sc = dev(d.u, TDT[dt]), dev(d.gamma, F32), dev(d.beta, F32), scratch_for(C, S)
    exp = fwd_expect(d, f, kind, dt)
    p = (np.arange(C) + 8) % C
    for a in range(4):
        got = run_norm_fwd(dt, C, S, kind, a, d, ud, gd, bd, sc)
        st4 = got["stat"]
        for i, k in enumerate(("mean", "rstd", "scale", "shift")):
            check("%s norm forward %s" % (dt, k), st4[i], *exp[k])
        if ev:
            assert np.array_equal(got["rm"], d.rm) and np.array_equal(got["rv"], d.rv), "eval mode changed the running statistics"
        elif kind == "bn":
            check(dt + " running mean", got["rm"], *exp["rm"])
            check(dt + " running var", got["rv"], *exp["rv"])
        # the activated copy from the kernel's own stat row
        z = d.u * st4[2] + st4[3]
        ra = R.act(z, a)
        ba = 2.0 ** -23 * np.abs(z) + (2.0 ** -21 + K[dt]["store"]) * np.abs(ra) + 1e-30
        check(dt + " activated copy", got["ya"], ra, ba)
        if C > 8:
            teeth("the activated copy with channel c from c + 8", miss(R.act(d.u[:, p] * st4[2] + st4[3], a), ra, ba))
    # teeth of the statistics
    wrong = [] if ev else [(n, R.norm_fwd(d.u, d.gamma, d.beta, R.EPS[kind], d.rm if kind == "bn" else None, d.rv if kind == "bn" else None, keep=m))
                           for n, m in lost_rows(S)]
    if C > 8:
        w = {k: f[k][p] for k in ("mean", "rstd", "rm", "rv") if k in f}
        wrong.append(("statistics of channel c from c + 8", dict(w, scale=d.gamma * w["rstd"], shift=d.beta - w["mean"] * d.gamma * w["rstd"])))
    for n, w in wrong:
        teeth(n, max(miss(w[k], *exp[k]) for k in exp))


NORM_PARAMS = [c + (k,) for c in LC.NORM_CASES for k in LC.NORM_KINDS if not (c[2] == 1 and k == "bn")]


@pytest.mark.parametrize("case", NORM_PARAMS + [c + ("bn_eval",) for c in LC.EVAL_CASES], ids=case_id)
def test_norm_forward_against_fp64(case):
    norm_fwd_case(*case)


# ---------------------------------------------------------------------------------------------------------------------------------
# norm backward
def bwd_bounds(d, b, dt):
    k = K[dt]
    S = d.u.shape[0]
    mean, rstd = d.stat[0], d.stat[1]
    dv, xh = b["dv"], b["xhat"]
    s1, s2 = np.abs(dv).sum(0), np.abs(dv * xh).sum(0)
    bd = {"c0": k["rel"] * np.abs(b["c0"]) + 1e-30, "m1": k["bsum"] * s1 / S + 1e-30, "m2": k["bsum"] * s2 / S + 1e-30,
          "dgamma": k["bsum"] * s2 + 2.0 ** -23 * np.abs(1 + b["dgamma"]), "dbeta": k["bsum"] * s1 + 2.0 ** -23 * np.abs(1 + b["dbeta"])}
    cancel = 2.0 ** -20 * np.abs(b["c0"]) * (np.abs(dv) + np.abs(b["m1"]) + np.abs(b["m2"]) * rstd * (np.abs(d.u) + np.abs(mean)))
    if dt == "bf16":      # the 1e-3 max|ref| of the epilogue test, taken apart for the voxels whose gradient is 16 times larger and for the rest
        heavy = LC.heavy_voxels(S)
        top = np.where(heavy, np.abs(b["du"][heavy]).max() if heavy.any() else 0.0, np.abs(b["du"][~heavy]).max())[:, None]
        bd["du"] = 2.0 ** -8 * np.abs(b["du"]) + 1e-3 * top + cancel + 1e-30
    else:
        bd["du"] = 2.0 ** -22 * np.abs(b["du"]) + cancel + np.abs(b["c0"]) * (bd["m1"] + np.abs(xh) * bd["m2"]) + 1e-30
    return bd


def norm_bwd_case(dt, C, S, kind):
    d = LC.norm_inputs(dt, C, S, kind)
    ud, gam, st, sc = dev(d.u, TDT[dt]), dev(d.gamma, F32), dev(d.stat, F32), scratch_for(C, S)
    p = (np.arange(C) + 8) % C
    Q = ("du", "c0", "m1", "m2", "dgamma", "dbeta")
    for a in range(4):
        outs = []
        for _ in range(2):
            sc.t.fill_(0xFF)
            g = Guarded((S, C), TDT[dt], d.g)
            coef, dgam, dbet = Guarded((3, C), F32), Guarded((C,), F32, 1.0), Guarded((C,), F32, 1.0)
            E.check(L.unet_op_norm_bwd(EDT[dt], g.data_ptr(), ud.data_ptr(), st.data_ptr(), a, gam.data_ptr(), coef.data_ptr(), dgam.data_ptr(),
                                       dbet.data_ptr(), C, S, sc.data_ptr(), stream()))
            guards("norm backward", ("dL/d(raw)", g), ("coef", coef), ("dgamma", dgam), ("dbeta", dbet), ("scratch", sc))
            outs.append({"g": g, "coef": coef, "dgamma": dgam, "dbeta": dbet})
        for k in outs[0]:
            assert np.array_equal(bits(outs[0][k]), bits(outs[1][k])), "%s differs between two identical calls" % k
        o = {k: host(v) for k, v in outs[0].items()}
        b = R.norm_bwd(d.g, d.u, d.stat[0], d.stat[1], d.stat[2], d.stat[3], d.gamma, a)
        bd = bwd_bounds(d, b, dt)
        got = {"du": o["g"], "c0": o["coef"][0], "m1": o["coef"][1], "m2": o["coef"][2], "dgamma": o["dgamma"] - 1.0, "dbeta": o["dbeta"] - 1.0}
        if S == 1:
            assert np.all(b["du"] == 0)      # xhat = 0 and dv = mean(dv): no gradient reaches the raw tensor
        for k in Q:
            check("%s norm backward %s" % (dt, k), got[k], b[k], bd[k])

        def ratio(w):
            return max(miss(w[k], b[k], bd[k]) for k in Q)
        for n, m in lost_rows(S):
            teeth(n + " (backward)", ratio(R.norm_bwd(d.g, d.u, d.stat[0], d.stat[1], d.stat[2], d.stat[3], d.gamma, a, keep=m)))
        if C > 8:
            w = {k: b[k][p] for k in ("m1", "m2", "dgamma", "dbeta")}
            w["c0"] = b["c0"]
            w["du"] = b["c0"] * (b["dv"] - w["m1"] - b["xhat"] * w["m2"])
            teeth("backward sums of channel c from c + 8", ratio(w))


@pytest.mark.parametrize("case", NORM_PARAMS, ids=case_id)
def test_norm_backward_against_fp64(case):
    norm_bwd_case(*case)


# ---------------------------------------------------------------------------------------------------------------------------------
# pool, upsample, views, export / import
def views_of(C, i):
    """plain, the exact relu view, and one norm + activation view (the activation cycles over the cases)"""
    return [("plain", None), ("exact", LC.exact_view(C)), ("norm", LC.norm_view(C, 1 + i % 3))]


VOLUME_PARAMS = [(dt, i) for dt in LC.DTYPES for i in range(len(LC.VOLUME_CASES))]
vol_ids = lambda p: "%s_%s" % (p[0], case_id(LC.VOLUME_CASES[p[1]]))   # noqa: E731


def win_max(b):
    return None if b is None else R._windows(b).max(3)


@pytest.mark.parametrize("p", VOLUME_PARAMS, ids=vol_ids)
def test_maxpool(p):
    dt, i = p
    C, (D, H, W) = LC.VOLUME_CASES[i]
    v = LC.volume_inputs(C, (D, H, W))
    Do, Ho, Wo = D // 2, H // 2, W // 2
    gc, old = dev(v.gc, TDT[dt]), v.old
    variants = [(n, v.x, vw) for n, vw in views_of(C, i)] + ([("nan", v.xn, None)] if v.xn is not None else [])
    for name, x, vw in variants:
        what = "max pool (%s view)" % name
        xd = dev(x, TDT[dt])
        va, keep = view_args(xd, C, vw)
        xv = view_ref(x, vw)
        y_ref, arg = R.maxpool_fwd(xv)
        y = Guarded((Do, Ho, Wo, C), TDT[dt])
        E.check(L.unet_op_maxpool_fwd(EDT[dt], *va, y.data_ptr(), D, H, W, stream()))
        guards(what, ("output", y), finite=name != "nan")
        if name == "nan":
            assert np.array_equal(host(y), LC.quant(y_ref, dt), equal_nan=True) and np.isnan(y_ref).sum() == 1
        else:
            same(dt + " " + what, y, y_ref, win_max(view_bound(x, vw, dt)))
        for acc in (0, 1):
            dx = Guarded((D, H, W, C), TDT[dt], old if acc else float("nan"))
            E.check(L.unet_op_maxpool_bwd(EDT[dt], *va, gc.data_ptr(), dx.data_ptr(), acc, D, H, W, stream()))
            guards(what + " backward", ("dx", dx))
            ref = R.maxpool_bwd(v.gc, arg, x.shape) + (old if acc else 0)
            assert_exact(dx.t, ref, "%s backward, accumulate %d" % (what, acc))
            for ax, n in enumerate((D, H, W)):      # the trailing plane of an odd extent: zero when written, unchanged when added to
                if n % 2:
                    assert np.array_equal(np.take(host(dx), n - 1, ax), np.take(old if acc else 0 * old, n - 1, ax))
            if name != "nan":
                differs("a tied window's gradient at the second maximum", R.maxpool_bwd(v.gc, arg, x.shape, second=True, x=xv) + (old if acc else 0),
                        ref, dt)
            differs("accumulate ignored", R.maxpool_bwd(v.gc, arg, x.shape) + (0 if acc else old), ref, dt)


def test_maxpool_refuses_an_extent_of_one():
    """no plan pools an extent of 1 (unet_plan_create refuses a network in which a tensor becomes empty): the entries refuse and launch
    nothing -- the buffers keep their poison"""
    with pytest.raises(E.UNetError):
        U.Plan("conv8,ks3,stride1\nmax_pool+conv8,ks3,stride1+upsample\nconv8,ks3,stride1", 1, 2, (1, 8, 8))
    for dims in ((1, 4, 4), (4, 1, 4), (4, 4, 1)):
        x, y, dx = dev(np.ones((*dims, 8)), torch.bfloat16), Guarded((16, 8), torch.bfloat16), Guarded((*dims, 8), torch.bfloat16)
        with pytest.raises(E.UNetError):
            E.check(L.unet_op_maxpool_fwd(U.DTYPE_BF16, x.data_ptr(), 8, None, None, 0, y.data_ptr(), *dims, stream()))
        with pytest.raises(E.UNetError):
            E.check(L.unet_op_maxpool_bwd(U.DTYPE_BF16, x.data_ptr(), 8, None, None, 0, y.data_ptr(), dx.data_ptr(), 0, *dims, stream()))
        guards("refused max pool", ("output", y), ("dx", dx), finite=False)
        assert torch.isnan(y.t.float()).all() and torch.isnan(dx.t.float()).all()


@pytest.mark.parametrize("p", VOLUME_PARAMS, ids=vol_ids)
def test_upsample(p):
    dt, i = p
    C, (D, H, W) = LC.VOLUME_CASES[i]
    v = LC.volume_inputs(C, (D, H, W))
    xd, gf = dev(v.x, TDT[dt]), dev(v.gf, TDT[dt])
    for name, vw in views_of(C, i):
        va, keep = view_args(xd, C, vw)
        y = Guarded((2 * D, 2 * H, 2 * W, C), TDT[dt])
        E.check(L.unet_op_upsample_fwd(EDT[dt], *va, y.data_ptr(), D, H, W, stream()))
        guards("upsample", ("output", y))
        b = view_bound(v.x, vw, dt)
        same("%s upsample (%s view)" % (dt, name), y, R.upsample_fwd(view_ref(v.x, vw)), None if b is None else R.upsample_fwd(b))
    for acc in (0, 1):
        dx = Guarded((D, H, W, C), TDT[dt], v.old if acc else float("nan"))
        E.check(L.unet_op_upsample_bwd(EDT[dt], gf.data_ptr(), dx.data_ptr(), C, acc, D, H, W, stream()))
        guards("upsample backward", ("dx", dx))
        ref = R.upsample_bwd(v.gf) + (v.old if acc else 0)
        assert_exact(dx.t, ref, "upsample backward, accumulate %d" % acc)
        differs("accumulate ignored", R.upsample_bwd(v.gf) + (0 if acc else v.old), ref, dt)


@pytest.mark.parametrize("p", VOLUME_PARAMS, ids=vol_ids)
def test_single_view_copies_and_act_backward(p):
    """one source through launch_materialize and through launch_apply_view; its backward through launch_materialize_bwd; g act'(u)"""
    dt, i = p
    C, dims = LC.VOLUME_CASES[i]
    v = LC.volume_inputs(C, dims)
    S = int(np.prod(dims))
    x, gs, old = v.x.reshape(S, C), v.gs.reshape(S, C), v.old.reshape(S, C)
    xd, gd = dev(x, TDT[dt]), dev(gs, TDT[dt])
    for name, vw in views_of(C, i):
        va, keep = view_args(xd, C, vw)
        ref, b = view_ref(x, vw), view_bound(x, vw, dt)
        y1, y2 = Guarded((S, C), TDT[dt]), Guarded((S, C), TDT[dt])
        E.check(L.unet_op_view(EDT[dt], *va, None, 0, None, None, 0, y1.data_ptr(), S, stream()))
        E.check(L.unet_op_apply_view(EDT[dt], *va, y2.data_ptr(), S, stream()))
        guards("view copy", ("materialize", y1), ("apply_view", y2))
        same("%s materialize (%s view)" % (dt, name), y1, ref, b)
        same("%s apply_view (%s view)" % (dt, name), y2, ref, b)
    for acc in (0, 1):
        d0 = Guarded((S, C), TDT[dt], old if acc else float("nan"))
        E.check(L.unet_op_view_bwd(EDT[dt], gd.data_ptr(), d0.data_ptr(), C, acc, None, 0, 0, S, stream()))
        guards("view backward", ("d0", d0))
        assert_exact(d0.t, gs + (old if acc else 0), "view backward, accumulate %d" % acc)
        differs("accumulate ignored", gs + (0 if acc else old), gs + (old if acc else 0), dt)
    assert (x == 0).any() or C == 1
    for a in range(4):
        g = Guarded((S, C), TDT[dt], gs)
        E.check(L.unet_op_act_bwd(EDT[dt], g.data_ptr(), xd.data_ptr(), a, S * C, stream()))
        guards("act backward", ("g", g))
        ref = gs * R.act_d(x, a)
        same("%s act backward" % dt, g, ref, None if a < 2 else (2.0 ** -21 + K[dt]["store"]) * np.abs(ref) + 1e-30)
        if a == 1 and (x == 0).any():
            differs("relu' taken as 1 at 0", gs * np.where(x >= 0, 1.0, 0.0), ref, dt)


@pytest.mark.parametrize("p", VOLUME_PARAMS, ids=vol_ids)
def test_export_and_import(p):
    dt, i = p
    C, dims = LC.VOLUME_CASES[i]
    v = LC.volume_inputs(C, dims)
    S = int(np.prod(dims))
    x, old = v.x.reshape(S, C), v.old.reshape(S, C)
    xd = dev(x, TDT[dt])
    for name, vw in views_of(C, i):
        va, keep = view_args(xd, C, vw)
        y = Guarded((C, S), F32)
        E.check(L.unet_op_export_view(EDT[dt], *va, y.data_ptr(), S, stream()))
        guards("export", ("output", y))
        b = view_bound(x, vw, "fp32")        # the output is fp32 whatever the element type
        same("%s export (%s view)" % (dt, name), y, R.export(view_ref(x, vw)), None if b is None else R.export(b))
    g = v.gs.reshape(S, C).T.copy()          # [C][S]
    gd = dev(g, F32)
    for acc in (0, 1):
        o = Guarded((S, C), TDT[dt], old if acc else float("nan"))
        E.check(L.unet_op_import_grad(EDT[dt], gd.data_ptr(), o.data_ptr(), C, S, acc, stream()))
        guards("import", ("gradient", o))
        ref = R.import_grad(g, old if acc else None)
        assert_exact(o.t, ref, "import, accumulate %d" % acc)
        differs("accumulate ignored", R.import_grad(g, None if acc else old), ref, dt)


@pytest.mark.parametrize("p", [(dt, c) for dt in LC.DTYPES for c in LC.CONCAT_CASES], ids=lambda p: "%s_%d+%d" % (p[0], *p[1]))
def test_concat_of_two_views(p):
    dt, (c0, c1) = p
    S, d = LC.CONCAT_S, LC.concat_inputs(c0, c1)
    x0, x1, gout, o0, o1 = d.x0, d.x1, d.gout, d.o0, d.o1
    xd0, xd1, gd = dev(x0, TDT[dt]), dev(x1, TDT[dt]), dev(gout, TDT[dt])
    for name, v0, v1 in d.views:
        a0, k0 = view_args(xd0, c0, v0)
        a1, k1 = view_args(xd1, c1, v1)
        y = Guarded((S, c0 + c1), TDT[dt])
        E.check(L.unet_op_view(EDT[dt], *a0, *a1, y.data_ptr(), S, stream()))
        guards("concat", ("output", y))
        ref = R.concat([view_ref(x0, v0), view_ref(x1, v1)])
        b0, b1 = view_bound(x0, v0, dt), view_bound(x1, v1, dt)
        b = None if name == "exact" else R.concat([b0, b1])
        same("%s concat (%s views)" % (dt, name), y, ref, b)
        swapped = R.concat([view_ref(x1, v1), view_ref(x0, v0)])
        shifted = np.roll(ref, -8, 1)
        if b is None:
            differs("the two concat sources swapped", swapped, ref, dt)
            differs("channel c taken from c + 8", shifted, ref, dt)
        else:
            teeth("the two concat sources swapped", miss(swapped, ref, b))
            teeth("channel c taken from c + 8", miss(shifted, ref, b))
    # backward: both written / added to, then one destination NULL and the other accumulating
    r0, r1 = R.concat_bwd(gout, (c0, c1))
    for acc0, acc1, null in ((0, 1, None), (1, 0, None), (0, 1, 0), (1, 0, 1)):
        d0 = None if null == 0 else Guarded((S, c0), TDT[dt], o0 if acc0 else float("nan"))
        d1 = None if null == 1 else Guarded((S, c1), TDT[dt], o1 if acc1 else float("nan"))
        E.check(L.unet_op_view_bwd(EDT[dt], gd.data_ptr(), ptr(d0), c0, acc0, ptr(d1), c1, acc1, S, stream()))
        guards("concat backward", ("d0", d0), ("d1", d1))
        for dd, r, o, acc, nm in ((d0, r0, o0, acc0, "first"), (d1, r1, o1, acc1, "second")):
            if dd is not None:
                assert_exact(dd.t, r + (o if acc else 0), "concat backward, %s destination, accumulate %d, NULL %s" % (nm, acc, null))
                differs("accumulate ignored", r + (0 if acc else o), r + (o if acc else 0), dt)
    differs("the two concat gradients swapped", R.concat_bwd(np.roll(gout, c1, 1), (c0, c1))[0], r0, dt)


# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", LC.DTYPES)
def test_voxels_on_the_kink(dt):
    k = LC.kink_inputs(dt)
    D, H, W, C = k.u.shape
    S = D * H * W
    u2, sp2 = k.u.reshape(S, C), k.special.reshape(S, C)
    ud, sc, sh = dev(k.u, TDT[dt]), dev(k.scale, F32), dev(k.shift, F32)
    reps = (1 << 18) // (S * C)                       # the copy's voxel-walking form needs S C >= 2^18 (bf16)
    big = dev(np.tile(u2, (reps, 1)), TDT[dt])
    for a in (1, 2, 3):
        va = (ud.data_ptr(), C, sc.data_ptr(), sh.data_ptr(), a)
        ref = R.act(k.z, a)
        bound = None if a == 1 else (2.0 ** -21 + K[dt]["store"]) * np.abs(ref) + 1e-30
        ym, ya, yu, ye, yp, yb = (Guarded((S, C), TDT[dt]), Guarded((S, C), TDT[dt]), Guarded((2 * D, 2 * H, 2 * W, C), TDT[dt]),
                                  Guarded((C, S), F32), Guarded((D // 2, H // 2, W // 2, C), TDT[dt]), Guarded((reps * S, C), TDT[dt]))
        E.check(L.unet_op_view(EDT[dt], *va, None, 0, None, None, 0, ym.data_ptr(), S, stream()))
        E.check(L.unet_op_apply_view(EDT[dt], *va, ya.data_ptr(), S, stream()))
        E.check(L.unet_op_apply_view(EDT[dt], big.data_ptr(), *va[1:], yb.data_ptr(), reps * S, stream()))
        E.check(L.unet_op_upsample_fwd(EDT[dt], *va, yu.data_ptr(), D, H, W, stream()))
        E.check(L.unet_op_export_view(EDT[dt], *va, ye.data_ptr(), S, stream()))
        E.check(L.unet_op_maxpool_fwd(EDT[dt], *va, yp.data_ptr(), D, H, W, stream()))
        guards("kink", ("materialize", ym), ("apply_view", ya), ("apply_view 8g", yb), ("upsample", yu), ("export", ye), ("pool", yp))
        r2 = ref.reshape(S, C)
        b2 = None if bound is None else bound.reshape(S, C)
        for name, got, rr, bb, spc in (("materialize", host(ym), r2, b2, sp2), ("apply_view", host(ya), r2, b2, sp2),
                                       ("apply_view 8g", host(yb), np.tile(r2, (reps, 1)), None if b2 is None else np.tile(b2, (reps, 1)),
                                        np.tile(sp2, (reps, 1))),
                                       ("upsample", host(yu), R.upsample_fwd(ref), None if bound is None else R.upsample_fwd(bound),
                                        R.upsample_fwd(k.special) > 0),
                                       ("export", host(ye), R.export(r2), None if b2 is None else R.export(b2), R.export(sp2) > 0)):
            # on the kink the value is the reference's exactly: 0, or 2^-24 on the positive side
            assert np.array_equal(got[spc], rr[spc]), "%s, act %d: a voxel on the kink took the other side" % (name, a)
            if bb is None:
                assert np.array_equal(got, rr), "%s, act %d" % (name, a)
            else:
                check("%s kink %s" % (dt, name), got, rr, bb)
        same("%s kink pool" % dt, yp, R.maxpool_fwd(ref)[0], win_max(bound))
        # the pool again on windows that the voxel on the kink wins (the seven others are negative): the pooled value is 0, or 2^-24 where
        # a product rounded before the add would give 0, and under relu the gradient goes to that voxel, not to element 0 of a window of zeros
        kp = LC.kink_pool_inputs(dt)
        kd, gcp = dev(kp.u, TDT[dt]), np.ones((D // 2, H // 2, W // 2, C))
        vp = (kd.data_ptr(), C, sc.data_ptr(), sh.data_ptr(), a)
        assert np.array_equal(kp.scale, k.scale) and np.array_equal(kp.shift, k.shift)
        yk, dxk = Guarded((D // 2, H // 2, W // 2, C), TDT[dt]), Guarded((D, H, W, C), TDT[dt])
        gk = dev(gcp, TDT[dt])
        E.check(L.unet_op_maxpool_fwd(EDT[dt], *vp, yk.data_ptr(), D, H, W, stream()))
        E.check(L.unet_op_maxpool_bwd(EDT[dt], *vp, gk.data_ptr(), dxk.data_ptr(), 0, D, H, W, stream()))
        guards("kink pool", ("output", yk), ("dx", dxk))
        yr, argr = R.maxpool_fwd(R.act(kp.z, a))
        assert np.array_equal(host(yk), yr), "pool, act %d: a window won by a voxel on the kink took the other side" % a
        assert_exact(dxk.t, R.maxpool_bwd(gcp, argr, kp.u.shape), "pool backward on the kink, act %d" % a)
        if dt == "fp32":
            yw, argw = R.maxpool_fwd(R.act(kp.wrong, a))
            differs("the pool reading its view with the product rounded before the add", yw, yr, dt)
            if a == 1:
                differs("the pool backward doing so", R.maxpool_bwd(gcp, argw, kp.u.shape), R.maxpool_bwd(gcp, argr, kp.u.shape), dt)
    # the derivative, through the norm backward's statistics: g = a distinct power of two per voxel, so dbeta = sum g act' names the
    # voxels that took the slope 1
    g = np.repeat(2.0 ** (np.arange(S) - 8.0)[:, None], C, 1)
    stat = dev(np.stack([0 * k.scale, 1 + 0 * k.scale, k.scale, k.shift]), F32)
    scr = scratch_for(C, S)
    for a in (1, 2):
        gb, coef, dgam, dbet = Guarded((S, C), TDT[dt], g), Guarded((3, C), F32), Guarded((C,), F32, 0.0), Guarded((C,), F32, 0.0)
        E.check(L.unet_op_norm_bwd(EDT[dt], gb.data_ptr(), ud.data_ptr(), stat.data_ptr(), a, sc.data_ptr(), coef.data_ptr(), dgam.data_ptr(),
                                   dbet.data_ptr(), C, S, scr.data_ptr(), stream()))
        guards("kink backward", ("g", gb), ("coef", coef), ("dgamma", dgam), ("dbeta", dbet), ("scratch", scr))
        z2 = k.z.reshape(S, C)
        ref = (g * R.act_d(z2, a)).sum(0)
        tol = 2.0 ** -20 * g.sum(0)
        check("%s kink derivative" % dt, host(dbet), ref, tol)
        slope0 = 0.0 if a == 1 else 0.01
        teeth("act' taken as 1 at 0", miss((g * np.where(z2 >= 0, 1.0, slope0)).sum(0), ref, tol))
        if dt == "fp32":
            teeth("the product rounded before the add", miss((g * np.where(z2 > 2.0 ** -24, 1.0, slope0)).sum(0), ref, tol))


def test_zz_report():
    """the worst error-to-bound ratio of every bounded quantity over the tests of this file that ran before this one"""
    for k in sorted(RATIOS):
        print("ratio %-40s %.3g" % (k, RATIOS[k]))
    assert all(r <= 1.0 for r in RATIOS.values())
