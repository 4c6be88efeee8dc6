"""GPU (-m gpu): the conv / conv_trans op kernels on exact-arithmetic data, bit for bit against the C oracle, into poisoned and guarded
buffers (tests/gpu_exact.py), over the same shapes as the random-data op tests of test_gpu_parity.py (tests/conv_cases.py); and a
check that every shape reaches the kernel family its section is there for.

What the random-data tests cannot see and these can: one missing (tap, channel) product at one voxel (2e-3 of the output's scale at
Cin = 512, under the 1e-2 bound of the bf16 engine), a voxel the kernel never wrote (the caching allocator hands a freed block with
the previous, correct answer to the next test), scratch that is read before it is written, a write past either end of an output.

The same for what a plan runs and the one-source entries cannot: convs that read two sources as their concatenation and write a
gradient destination per source -- written, added to, or absent (unet_op_conv3d_fwd2 / _bwd_data2 / _bwd_weight2, the cases of
conv_cases.CONV2_SECTIONS), the accumulating conv_trans dgrad, and the heads (unet_op_head_fwd / _bwd), whose leaky_relu and elu views
go against float64 with a derived bound."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import unet_studio_amd as U  # noqa: E402

import conv_cases as CC  # noqa: E402
import gpu_exact as X  # noqa: E402
from gpu_exact import DEV, TDT, Guarded, assert_exact, cf, check_all, to_cl  # noqa: E402

E = U.engine
EDT = {"fp32": U.DTYPE_F32, "bf16": U.DTYPE_BF16}
F32 = torch.float32


def stream():
    return torch.cuda.current_stream(DEV).cuda_stream


def dev(a):
    return torch.tensor(a, device=DEV)


def repoison(sc):
    sc.t.fill_(0xFF)


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("impl", [U.IMPL_DIRECT, U.IMPL_AUTO])
@pytest.mark.parametrize("case", CC.CONV_CASES)
def test_conv3d_ops_exact(case, dt, impl):
    cin, cout, (D, H, W), ks, st = case
    ref = X.reference(case)
    X.check_preconditions(ref, dt, str(case))
    od = X.out_dims(case)
    sc = X.poisoned_scratch(cin, cout, D, H, W)
    wd, bd, xd, dyd = dev(ref.w), dev(ref.b), to_cl(ref.x, dt), to_cl(ref.dy, dt)
    y = Guarded((*od, cout), TDT[dt])
    E.check(E.lib.unet_op_conv3d_fwd(EDT[dt], impl, xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), y.data_ptr(), cin, cout, D, H, W,
                                     ks, st, sc.data_ptr(), stream()))
    check_all("forward", ("y", y), ("scratch", sc))
    assert_exact(cf(y.t), ref.y, "y [C,D,H,W]")
    repoison(sc)
    dx = Guarded((D, H, W, cin), TDT[dt])
    E.check(E.lib.unet_op_conv3d_bwd_data(EDT[dt], impl, dyd.data_ptr(), wd.data_ptr(), dx.data_ptr(), cin, cout, D, H, W, ks, st,
                                          sc.data_ptr(), stream()))
    check_all("dgrad", ("dx", dx), ("scratch", sc))
    assert_exact(cf(dx.t), ref.dx, "dx [C,D,H,W]")
    repoison(sc)
    dw, db = Guarded(ref.w.shape, F32, ref.dw0), Guarded((cout,), F32, ref.db0)   # += onto integer start values
    E.check(E.lib.unet_op_conv3d_bwd_weight(EDT[dt], impl, xd.data_ptr(), dyd.data_ptr(), dw.data_ptr(), db.data_ptr(), cin, cout,
                                            D, H, W, ks, st, sc.data_ptr(), stream()))
    check_all("wgrad", ("dw", dw), ("db", db), ("scratch", sc))
    assert_exact(dw.t, ref.dw, "dw [Cout,Cin,kz,ky,kx]")
    assert_exact(db.t, ref.db, "db")


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("case", CC.CONVT_CASES)
def test_convt_ops_exact(case, dt):
    cin, cout, (D, H, W) = case
    ref = X.reference(case)
    X.check_preconditions(ref, dt, str(case))
    sc = X.poisoned_scratch(cin, cout, D, H, W)
    wd, bd, xd, dyd = dev(ref.w), dev(ref.b), to_cl(ref.x, dt), to_cl(ref.dy, dt)
    y = Guarded((2 * D, 2 * H, 2 * W, cout), TDT[dt])
    E.check(E.lib.unet_op_convt_fwd(EDT[dt], 0, xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), y.data_ptr(), cin, cout, D, H, W,
                                    sc.data_ptr(), stream()))
    check_all("forward", ("y", y), ("scratch", sc))
    assert_exact(cf(y.t), ref.y, "y [C,D,H,W]")
    repoison(sc)
    dx = Guarded((D, H, W, cin), TDT[dt])
    E.check(E.lib.unet_op_convt_bwd_data(EDT[dt], 0, dyd.data_ptr(), wd.data_ptr(), dx.data_ptr(), cin, cout, D, H, W, sc.data_ptr(), stream()))
    check_all("dgrad", ("dx", dx), ("scratch", sc))
    assert_exact(cf(dx.t), ref.dx, "dx [C,D,H,W]")
    repoison(sc)
    dw, db = Guarded(ref.w.shape, F32, ref.dw0), Guarded((cout,), F32, ref.db0)
    E.check(E.lib.unet_op_convt_bwd_weight(EDT[dt], 0, xd.data_ptr(), dyd.data_ptr(), dw.data_ptr(), db.data_ptr(), cin, cout, D, H, W,
                                           sc.data_ptr(), stream()))
    check_all("wgrad", ("dw", dw), ("db", db), ("scratch", sc))
    assert_exact(dw.t, ref.dw, "dw [Cin,Cout,kz,ky,kx]")
    assert_exact(db.t, ref.db, "db")


def sources(ref, c0, dt, how):
    """the two sources of a case on the device: "adjacent" in one allocation, or "fenced" -- separately allocated inside NaN, the second
    one first and with the larger fence, so that a kernel that walks past source 0 finds NaN and not its neighbour"""
    x0, x1 = to_cl(ref.x[:c0], dt), to_cl(ref.x[c0:], dt)
    if how == "adjacent":
        return X.adjacent(x0, x1)
    f1 = X.Fenced(x1, 4096)
    f0 = X.Fenced(x0, 2048)
    return f0, f1


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("impl", [U.IMPL_DIRECT, U.IMPL_AUTO])
@pytest.mark.parametrize("case2", CC.CONV2_CASES)
def test_conv3d_two_source_ops_exact(case2, dt, impl):
    """forward and weight gradient of a conv that reads two sources as their concatenation (unet_op_conv3d_fwd2 / _bwd_weight2), bit
    for bit against the oracle's conv of c0 + c1 channels"""
    c0, c1, cout, (D, H, W), ks, st = case2
    case = X.merged(case2)
    ref = X.reference(case)
    X.check_preconditions(ref, dt, str(case2))
    od = X.out_dims(case)
    sc = X.poisoned_scratch(c0 + c1, cout, D, H, W)
    wd, bd, dyd = dev(ref.w), dev(ref.b), to_cl(ref.dy, dt)
    for how in ("adjacent", "fenced"):
        x0, x1 = sources(ref, c0, dt, how)
        y = Guarded((*od, cout), TDT[dt])
        repoison(sc)
        E.check(E.lib.unet_op_conv3d_fwd2(EDT[dt], impl, x0.data_ptr(), c0, x1.data_ptr(), c1, wd.data_ptr(), bd.data_ptr(), y.data_ptr(),
                                          cout, D, H, W, ks, st, sc.data_ptr(), stream()))
        check_all("forward, sources " + how, ("y", y), ("scratch", sc))
        assert_exact(cf(y.t), ref.y, "y [C,D,H,W], sources " + how)
        repoison(sc)
        dw, db = Guarded(ref.w.shape, F32, ref.dw0), Guarded((cout,), F32, ref.db0)
        E.check(E.lib.unet_op_conv3d_bwd_weight2(EDT[dt], impl, x0.data_ptr(), c0, x1.data_ptr(), c1, dyd.data_ptr(), dw.data_ptr(),
                                                 db.data_ptr(), cout, D, H, W, ks, st, sc.data_ptr(), stream()))
        check_all("wgrad, sources " + how, ("dw", dw), ("db", db), ("scratch", sc))
        assert_exact(dw.t, ref.dw, "dw [Cout,Cin,kz,ky,kx], sources " + how)
        assert_exact(db.t, ref.db, "db, sources " + how)


def destination(dims, C, dt, old, acc):
    """a guarded gradient destination [D,H,W,C]: NaN where it is written, the older gradient where it is added to"""
    return Guarded((*dims, C), TDT[dt], np.transpose(old, (1, 2, 3, 0)) if acc else float("nan"))


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("impl", [U.IMPL_DIRECT, U.IMPL_AUTO])
@pytest.mark.parametrize("case2", CC.CONV2_CASES)
def test_conv3d_split_dgrad_exact(case2, dt, impl):
    """the input gradient of a two-source conv (unet_op_conv3d_bwd_data2): a destination per source, each written or added to an older
    gradient of integers in [-2, 2]; one destination NULL (its partner must be complete, a poisoned buffer that stands in for the
    missing one is left alone); and one destination of all c0 + c1 channels, written and accumulated (what k_s2_scatter takes)"""
    c0, c1, cout, (D, H, W), ks, st = case2
    case = X.merged(case2)
    ref = X.reference(case)
    old = X.old_gradient(case)
    X.check_preconditions(ref, dt, str(case2))
    X.check_accumulate_precondition(ref, old, dt, str(case2))
    sc = X.poisoned_scratch(c0 + c1, cout, D, H, W)
    wd, dyd = dev(ref.w), to_cl(ref.dy, dt)
    dims = (D, H, W)

    def run(d0, a0, d1, a1, n0, n1, what):
        repoison(sc)
        E.check(E.lib.unet_op_conv3d_bwd_data2(EDT[dt], impl, 0, dyd.data_ptr(), wd.data_ptr(), d0.data_ptr() if d0 else None, n0, a0,
                                               d1.data_ptr() if d1 else None, n1, a1, cout, D, H, W, ks, st, sc.data_ptr(), stream()))
        sc.check(what + " scratch", finite=False)

    for a0, a1 in ((0, 0), (1, 0), (0, 1)):
        what = "dgrad acc (%d, %d)" % (a0, a1)
        d0, d1 = destination(dims, c0, dt, old[:c0], a0), destination(dims, c1, dt, old[c0:], a1)
        run(d0, a0, d1, a1, c0, c1, what)
        check_all(what, ("d0", d0), ("d1", d1))
        assert_exact(cf(d0.t), ref.dx[:c0] + a0 * old[:c0], what + ": d0 [C,D,H,W]")
        assert_exact(cf(d1.t), ref.dx[c0:] + a1 * old[c0:], what + ": d1 [C,D,H,W]")
    # one destination NULL
    for missing in (0, 1):
        what = "dgrad without d%d" % missing
        d0, d1 = destination(dims, c0, dt, None, 0), destination(dims, c1, dt, None, 0)
        run(None if missing == 0 else d0, 0, None if missing == 1 else d1, 0, c0, c1, what)
        kept, gone = (d1, d0) if missing == 0 else (d0, d1)
        kept.check(what + ": the destination that is there")
        gone.check(what + ": the buffer in the place of the missing one", finite=False)
        assert bool(torch.isnan(gone.t.float()).all()), what + ": the buffer in the place of the missing one was written"
        assert_exact(cf(kept.t), ref.dx[c0:] if missing == 0 else ref.dx[:c0], what + ": d%d [C,D,H,W]" % (1 - missing))
    # one destination of every channel
    for acc in (0, 1):
        what = "dgrad into one destination, acc %d" % acc
        d = destination(dims, c0 + c1, dt, old, acc)
        run(d, acc, None, 0, c0 + c1, 0, what)
        d.check(what)
        assert_exact(cf(d.t), ref.dx + acc * old, what + ": dx [C,D,H,W]")


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("case", CC.CONVT_ACC_CASES)
def test_convt_dgrad_accumulate_exact(case, dt):
    """the dgrad of a conv_trans ADDED to an older gradient (unet_op_conv3d_bwd_data2, transposed), and two destinations refused"""
    cin, cout, (D, H, W) = case
    ref = X.reference(case)
    old = X.old_gradient(case)
    X.check_preconditions(ref, dt, str(case))
    X.check_accumulate_precondition(ref, old, dt, str(case))
    sc = X.poisoned_scratch(cin, cout, D, H, W)
    wd, dyd = dev(ref.w), to_cl(ref.dy, dt)
    for acc in (1, 0):
        dx = destination((D, H, W), cin, dt, old, acc)
        repoison(sc)
        E.check(E.lib.unet_op_conv3d_bwd_data2(EDT[dt], U.IMPL_AUTO, 1, dyd.data_ptr(), wd.data_ptr(), dx.data_ptr(), cin, acc, None, 0, 0,
                                               cout, D, H, W, 2, 2, sc.data_ptr(), stream()))
        check_all("conv_trans dgrad acc %d" % acc, ("dx", dx), ("scratch", sc))
        assert_exact(cf(dx.t), ref.dx + acc * old, "dx [C,D,H,W], acc %d" % acc)
    with pytest.raises(RuntimeError):
        E.check(E.lib.unet_op_conv3d_bwd_data2(EDT[dt], U.IMPL_AUTO, 1, dyd.data_ptr(), wd.data_ptr(), dx.data_ptr(), cin - 16, 0, dx.data_ptr(),
                                               16, 0, cout, D, H, W, 2, 2, sc.data_ptr(), stream()))


def head_exact(r, cin, cout, S, dt, what):
    """every form of the head forward and backward on the exact data r (gpu_exact.head_reference), bit for bit: the forward into the
    channels-last result, the fp32 NCDHW one and both; the backward from either layout of dy, with the slab sum inside the call and
    deferred (identical bits), dL/d(view) written, added to integers in [-2, 2], or not asked for; dw / db added onto integer start
    values; and the calls the entries refuse.  r.scale None: the source is read plain, otherwise through a relu view"""
    X.check_preconditions(r, dt, what)
    X.check_accumulate_precondition(r, r.old, dt, what)
    plain = r.scale is None
    scale, shift = (None, None) if plain else (dev(r.scale), dev(r.shift))
    xd = to_cl(r.x, dt).view(-1, cin)
    view = (xd.data_ptr(), cin, None if plain else scale.data_ptr(), None if plain else shift.data_ptr(), 0 if plain else 1)
    wd, bd = dev(r.w), dev(r.b)
    ycl_ref, ync_ref = r.y.reshape(cout, S).T, r.y.reshape(cout, S)
    for want_cl, want_nc in ((1, 0), (0, 1), (1, 1)):
        ycl, ync = Guarded((S, cout), TDT[dt]), Guarded((cout, S), F32)
        E.check(E.lib.unet_op_head_fwd(EDT[dt], *view, wd.data_ptr(), bd.data_ptr(), ycl.data_ptr() if want_cl else None,
                                       ync.data_ptr() if want_nc else None, cout, S, stream()))
        for want, buf, ref, name in ((want_cl, ycl, ycl_ref, "y [S,C]"), (want_nc, ync, ync_ref, "y fp32 [C,S]")):
            buf.check("%s forward (%d, %d) %s" % (what, want_cl, want_nc, name), finite=bool(want))
            if want:
                assert_exact(buf.t, ref, "%s forward (%d, %d): %s" % (what, want_cl, want_nc, name))
            else:
                assert bool(torch.isnan(buf.t.float()).all()), what + ": an output that was not asked for was written"
    with pytest.raises(RuntimeError):
        E.check(E.lib.unet_op_head_fwd(EDT[dt], *view, wd.data_ptr(), bd.data_ptr(), None, None, cout, S, stream()))
    sc = X.poisoned_scratch(cin, cout)
    dy_nc, dy_cl = dev(r.dy.reshape(cout, S)), to_cl(r.dy, dt).view(S, cout)
    old_cl = r.old.reshape(cin, S).T
    dx_ref = r.dx.reshape(cin, S).T
    for layout in ("ncdhw", "cl"):
        for mode in ("written", "accumulated", "null"):
            got = {}
            for defer in (0, 1):
                w2 = "%s backward (dy %s, dx %s, defer %d)" % (what, layout, mode, defer)
                dx = Guarded((S, cin), TDT[dt], old_cl if mode == "accumulated" else float("nan"))
                dw, db = Guarded((cout, cin), F32, r.dw0.reshape(cout, cin)), Guarded((cout,), F32, r.db0)
                repoison(sc)
                E.check(E.lib.unet_op_head_bwd(EDT[dt], *view, dy_nc.data_ptr() if layout == "ncdhw" else None,
                                               dy_cl.data_ptr() if layout == "cl" else None, wd.data_ptr(),
                                               None if mode == "null" else dx.data_ptr(), 1 if mode == "accumulated" else 0,
                                               dw.data_ptr(), db.data_ptr(), cout, S, defer, sc.data_ptr(), stream()))
                check_all(w2, ("dw", dw), ("db", db), ("scratch", sc))
                dx.check(w2 + " dx", finite=mode != "null")
                assert_exact(dw.t, r.dw.reshape(cout, cin), w2 + ": dw [Cout,Cin]")
                assert_exact(db.t, r.db, w2 + ": db")
                if mode == "null":
                    assert bool(torch.isnan(dx.t.float()).all()), w2 + ": dx was not asked for and was written"
                else:
                    assert_exact(dx.t, dx_ref + (old_cl if mode == "accumulated" else 0), w2 + ": dx [S,Cin]")
                got[defer] = (dw.t.clone(), db.t.clone())
            assert torch.equal(got[0][0].view(torch.int32), got[1][0].view(torch.int32)) and \
                torch.equal(got[0][1].view(torch.int32), got[1][1].view(torch.int32)), what + ": the deferred slab sum gives other bits"
    with pytest.raises(RuntimeError):   # both forms of dy
        E.check(E.lib.unet_op_head_bwd(EDT[dt], *view, dy_nc.data_ptr(), dy_cl.data_ptr(), wd.data_ptr(), None, 0, dw.data_ptr(),
                                       db.data_ptr(), cout, S, 0, sc.data_ptr(), stream()))
    with pytest.raises(RuntimeError):   # a shape head_supported refuses
        E.check(E.lib.unet_op_head_fwd(EDT[dt], view[0], 48, *view[2:], wd.data_ptr(), bd.data_ptr(), ycl.data_ptr(), None, cout, 1, stream()))


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("cout", CC.HEAD_COUT)
@pytest.mark.parametrize("cin", CC.HEAD_CIN)
def test_head_ops_exact(cin, cout, dt):
    """k_head_fwd / k_head_bwd through unet_op_head_fwd / unet_op_head_bwd on a relu view with scale +-1 and shift in {-1, 0, 1}, bit
    for bit against the oracle's 1x1x1 conv on the activated input, in every form head_exact runs.  At these voxel counts a thread of
    either kernel takes one voxel (test_head_ops_exact_past_the_block_caps has the multi-voxel loop)"""
    for S in CC.HEAD_VOXELS:
        head_exact(X.head_reference(cin, cout, S), cin, cout, S, dt, "head %d -> %d, %d voxels" % (cin, cout, S))


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("case", CC.HEAD_CAP_CASES)
def test_head_ops_exact_past_the_block_caps(case, dt):
    """voxel counts past the 512-block cap of launch_head_bwd and the 2048-block cap of launch_head_fwd (conv_cases.HEAD_CAP_CASES): a
    thread walks several voxels -- the backward prefetches the next one, carries it over and sums its dw / db terms over all of them,
    the forward makes further strided passes -- and the last pass is ragged.  Every form of head_exact, bit for bit"""
    cin, cout, S = case
    lc = (cin // 16).bit_length() - 1
    assert (S << lc) > 131072 and (((S + 63) & ~63) << lc) > 524288, "the case does not reach the caps"
    assert S % ((512 * 256) >> lc) and S % ((2048 * 256) >> lc) and S % 64, "the last pass is not ragged"
    head_exact(X.head_reference(cin, cout, S), cin, cout, S, dt, "head %d -> %d, %d voxels" % (cin, cout, S))


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("case", CC.HEAD_PLAIN_CASES)
def test_head_ops_exact_on_a_plain_source(case, dt):
    """the head kernels on a source without scale, shift and activation (the plain branch of load_chunk16): every ternary input
    reaches the filter, so no column of dw is left at its start value"""
    cin, cout, S = case
    head_exact(X.head_reference(cin, cout, S, plain=True), cin, cout, S, dt, "plain head %d -> %d, %d voxels" % (cin, cout, S))


def act64(z, a):
    return np.where(z > 0, z, 0.01 * z) if a == 2 else np.where(z > 0, z, np.expm1(np.minimum(z, 0.0)))


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("act", [2, 3])
def test_head_ops_with_leaky_relu_and_elu_against_fp64(act, dt):
    """leaky_relu and elu leave the integers: one head forward (both outputs) and one backward (dy as fp32 NCDHW, dx accumulated) per
    activation, 32 -> 6 channels on 321 voxels, against float64.

    Inputs.  x = k / 8 (|k| <= 8), scale in {+-1/2, +-1, +-2}, shift = m / 8: the pre-activation z = x scale + shift is a multiple of
    1/16 of magnitude <= 3 that the view's fp32 fma computes exactly, so z sits ON the kink (z = 0) and next to it (|z| = 1/16) without
    any doubt about the side.  Filter 0.2 N(0,1), bias, dy, the older dx and the start values of dw / db N(0,1), dy and the older dx
    rounded to bf16 so that both engines read the same numbers.

    Bounds from the rounding points (e = 2^-24, the fp32 unit roundoff):
      * the view: the fma, 2^-23 (|x scale| + |shift|) (zero here, kept for the formula's sake); leaky_relu's product 0.01f z, 2^-23 |a|
        (e for the product and 2.2e-8 for 0.01f against 0.01); elu's exponential, 2^-21 absolute where z < 0 (expf of a value <= 1 to 2
        ulp of 1, whether the kernel forms expm1f or expf - 1, doubled): da per element;
      * a dot product of n terms t_i summed in fp32 in any order (per thread, across lanes, across blocks): (n + 2) e sum|t_i|, with the
        bias or the start value of a += as one more term;
      * y = sum_c w a + b: sum_c |w| da + (Cin + 2) e (sum_c |w a| + |b|);  dw += sum_v dy a: sum_v |dy| da + (S + 2) e (sum_v |dy a| +
        |dw0|);  db += sum_v dy: (S + 2) e (sum_v |dy| + |db0|);  dx = old + sum_co dy w: (Cout + 2) e (sum_co |dy w| + |old|);
      * a bf16 store (y channels-last and dx in the bf16 engine): half an ulp, <= 2^-8 |ref|.
    Teeth: the reference with scale and shift of channel c + 16 (the other 16-channel chunk's view) must miss the bounds of y and dw by
    at least 10x."""
    cin, cout, S = 32, 6, 321
    rng = np.random.default_rng(100 * act + 7)
    x = rng.integers(-8, 9, (S, cin)) / 8.0
    scale = rng.choice([-2.0, -1.0, -0.5, 0.5, 1.0, 2.0], cin)
    shift = rng.integers(-8, 9, cin) / 8.0
    f32 = lambda a: np.asarray(a, np.float32).astype(np.float64)
    b16 = lambda a: torch.from_numpy(np.asarray(a, np.float32)).to(torch.bfloat16).double().numpy()
    w, b = f32(0.2 * rng.standard_normal((cout, cin))), f32(rng.standard_normal(cout))
    dy, old = b16(rng.standard_normal((cout, S))), b16(rng.standard_normal((S, cin)))
    dw0, db0 = f32(rng.standard_normal((cout, cin))), f32(rng.standard_normal(cout))
    e = 2.0 ** -24
    bf = 2.0 ** -8 if dt == "bf16" else 0.0

    def expect(scale, shift):
        z = x * scale + shift
        a = act64(z, act)
        da = 2.0 ** -23 * (np.abs(x * scale) + np.abs(shift)) + (2.0 ** -23 * np.abs(a) if act == 2 else 2.0 ** -21 * (z < 0))
        y = a @ w.T + b
        by = da @ np.abs(w).T + (cin + 2) * e * (np.abs(a) @ np.abs(w).T + np.abs(b))
        dw = dw0 + dy @ a
        bdw = np.abs(dy) @ da + (S + 2) * e * (np.abs(dy) @ np.abs(a) + np.abs(dw0))
        return z, {"y": (y, by), "dw": (dw, bdw)}
    z, R = expect(scale, shift)
    assert np.count_nonzero(z == 0) > 50 and np.count_nonzero(np.abs(z) == 1 / 16) > 50 and np.all(z == np.rint(z * 16) / 16)
    R["db"] = (db0 + dy.sum(1), (S + 2) * e * (np.abs(dy).sum(1) + np.abs(db0)))
    dx = old + dy.T @ w
    R["dx"] = (dx, (cout + 2) * e * (np.abs(dy).T @ np.abs(w) + np.abs(old)) + bf * np.abs(dx))

    d32 = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(F32).to(DEV)
    xd = torch.from_numpy(x).to(TDT[dt]).to(DEV)
    sd, hd, wd, bd, dyd = d32(scale), d32(shift), d32(w), d32(b), d32(dy)
    ycl, ync = Guarded((S, cout), TDT[dt]), Guarded((cout, S), F32)
    E.check(E.lib.unet_op_head_fwd(EDT[dt], xd.data_ptr(), cin, sd.data_ptr(), hd.data_ptr(), act, wd.data_ptr(), bd.data_ptr(), ycl.data_ptr(),
                                   ync.data_ptr(), cout, S, stream()))
    sc = X.poisoned_scratch(cin, cout)
    dxg, dw, db = Guarded((S, cin), TDT[dt], old), Guarded((cout, cin), F32, dw0), Guarded((cout,), F32, db0)
    E.check(E.lib.unet_op_head_bwd(EDT[dt], xd.data_ptr(), cin, sd.data_ptr(), hd.data_ptr(), act, dyd.data_ptr(), None, wd.data_ptr(),
                                   dxg.data_ptr(), 1, dw.data_ptr(), db.data_ptr(), cout, S, 0, sc.data_ptr(), stream()))
    check_all("head with act %d" % act, ("y", ycl), ("y fp32", ync), ("dx", dxg), ("dw", dw), ("db", db), ("scratch", sc))
    got = {"y channels-last": (ycl.t.double().cpu().numpy(), R["y"][0], R["y"][1] + bf * np.abs(R["y"][0])),
           "y fp32 [C,S]": (ync.t.double().cpu().numpy().T, R["y"][0], R["y"][1]),
           "dw": (dw.t.double().cpu().numpy(), *R["dw"]), "db": (db.t.double().cpu().numpy(), *R["db"]),
           "dx": (dxg.t.double().cpu().numpy(), *R["dx"])}
    for name, (g, ref, bound) in got.items():
        worst = float(np.max(np.abs(g - ref) / bound))
        print("head act %d %s %s: worst error %.3g of the bound" % (act, dt, name, worst))
        assert worst <= 1.0, "%s: error %.3g of the bound" % (name, worst)
    p = (np.arange(cin) + 16) % cin
    _, Wr = expect(scale[p], shift[p])
    for name, key in (("y channels-last", "y"), ("y fp32 [C,S]", "y"), ("dw", "dw")):
        miss = float(np.max(np.abs(Wr[key][0] - got[name][1]) / got[name][2]))
        assert miss >= 10, "the view of channel c + 16 misses the bound of %s by only %.1fx" % (name, miss)


def stats_rows(stats, y_ref, what, rest_check):
    """exact rows where the reference alone shows the sums exact in fp32 (every channel at <= 4096 output voxels); the random-data
    test's own tolerance on the rest"""
    got = stats.t.cpu().numpy().astype(np.float64)
    rest0, rest1, sums = X.assert_exact_stats(got, y_ref, what, y_ref[0].size <= 4096)
    rest_check(got, sums, rest0, rest1)


@pytest.mark.parametrize("case", CC.PLAIN_STATS_CASES)
def test_conv3d_plain_with_statistics_exact(case):
    cin, cout, (D, H, W) = case
    ref = X.reference((cin, cout, (D, H, W), 3, 1), 0, ("fwd",))
    X.check_preconditions(ref, "bf16", str(case))
    sc = X.poisoned_scratch(cin, cout, D, H, W)
    wd, bd, xd = dev(ref.w), dev(ref.b), to_cl(ref.x, "bf16")
    y, stats = Guarded((D, H, W, cout), torch.bfloat16), Guarded((cout, 2), F32)
    E.check(E.lib.unet_op_conv3d_fwd_fused(U.DTYPE_BF16, U.IMPL_AUTO, xd.data_ptr(), None, None, 0, wd.data_ptr(), bd.data_ptr(),
                                           y.data_ptr(), stats.data_ptr(), cin, cout, D, H, W, 3, 1, sc.data_ptr(), stream()))
    check_all("plain + statistics", ("y", y), ("stats", stats), ("scratch", sc))
    assert_exact(cf(y.t), ref.y, "y [C,D,H,W]")

    def rest(got, sums, r0, r1):
        assert np.allclose(got[r0, 0], sums[r0, 0], rtol=1e-4, atol=1e-2)
        assert np.allclose(got[r1, 1], sums[r1, 1], rtol=1e-4, atol=1e-2)
    stats_rows(stats, ref.y, str(case), rest)


def test_conv3d_pack_then_kernel_only_exact():
    cin, cout, (D, H, W) = CC.PACKED_CASE
    ref = X.reference((cin, cout, (D, H, W), 3, 1), 0, ("fwd",))
    X.check_preconditions(ref, "bf16", str(CC.PACKED_CASE))
    wp, part = X.poisoned_scratch(cin, cout, D, H, W), X.poisoned_scratch(cin, cout, D, H, W)
    wd, bd, xd = dev(ref.w), dev(ref.b), to_cl(ref.x, "bf16")
    y = Guarded((D, H, W, cout), torch.bfloat16)
    E.check(E.lib.unet_op_conv3d_pack(U.DTYPE_BF16, wd.data_ptr(), wp.data_ptr(), cin, cout, D, H, W, 3, 1, stream()))
    E.check(E.lib.unet_op_conv3d_fwd_packed(U.DTYPE_BF16, xd.data_ptr(), wp.data_ptr(), bd.data_ptr(), y.data_ptr(), part.data_ptr(),
                                            cin, cout, D, H, W, 3, 1, stream()))
    check_all("pack + kernel only", ("y", y), ("wp", wp), ("part", part))
    assert_exact(cf(y.t), ref.y, "y [C,D,H,W]")


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("impl", [U.IMPL_DIRECT, U.IMPL_AUTO])
@pytest.mark.parametrize("case", [c[:5] for c in CC.FUSED_CASES])
def test_conv3d_fused_prologue_epilogue_exact(case, dt, impl):
    """relu only (leaky_relu and elu leave the integers): the shapes of the random-data test, each with act 1; scale in {-1, 1} and
    shift in {-1, 0, 1}, so what the contraction reads is 0, 1 or 2"""
    cin, cout, (D, H, W), ks, st = case
    ref = X.fused_reference(case)
    X.check_preconditions(ref, dt, str(case))
    od = X.out_dims(case)
    sc = X.poisoned_scratch(cin, cout, D, H, W)
    wd, bd, xd, sd, hd = dev(ref.w), dev(ref.b), to_cl(ref.x, dt), dev(ref.scale), dev(ref.shift)
    y, stats = Guarded((*od, cout), TDT[dt]), Guarded((cout, 2), F32)
    E.check(E.lib.unet_op_conv3d_fwd_fused(EDT[dt], impl, xd.data_ptr(), sd.data_ptr(), hd.data_ptr(), 1, wd.data_ptr(), bd.data_ptr(),
                                           y.data_ptr(), stats.data_ptr(), cin, cout, D, H, W, ks, st, sc.data_ptr(), stream()))
    check_all("fused", ("y", y), ("stats", stats), ("scratch", sc))
    assert_exact(cf(y.t), ref.y, "y [C,D,H,W]")

    def rest(got, sums, r0, r1):
        yy = np.asarray(ref.y, np.float64).reshape(cout, -1)
        assert np.allclose(got[r0, 0], sums[r0, 0], rtol=1e-4, atol=1e-3 * np.abs(yy).sum(1).max())
        assert np.allclose(got[r1, 1], sums[r1, 1], rtol=1e-4)
    stats_rows(stats, ref.y, str(case), rest)


@pytest.mark.parametrize("switch", ["UNET_NO_SLIDING_WINDOW", "UNET_NO_DEEP_KERNELS", "UNET_OP_POLITE"])
def test_exact_ops_on_the_kernels_behind_a_switch(switch):
    """The kernels a default run does not reach for these shapes: the halo-tile kernels under every sliding-window one
    (UNET_NO_SLIDING_WINDOW=1, the documented fallback), the MFMA convs under the deep levels' split-K kernels (UNET_NO_DEEP_KERNELS=1)
    and the polite launch configuration of the weight gradients (UNET_OP_POLITE=1).  The switches are read once per process: the bf16
    conv / conv_trans cases of this file -- the two-source, split-destination and accumulating ones included -- run again in a child, bit
    for bit and into poisoned buffers as above."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-m", "gpu", "-p", "no:cacheprovider", "--maxfail=10",
                          "-k", "(test_conv3d_ops_exact or test_convt_ops_exact or test_conv3d_two_source_ops_exact or test_conv3d_split_dgrad_exact "
                                "or test_convt_dgrad_accumulate_exact) and bf16"], capture_output=True, text=True, timeout=600,
                         env=dict(os.environ, **{switch: "1"}), cwd=root)
    assert out.returncode == 0, out.stdout[-6000:] + out.stderr[-2000:]
    assert " passed" in out.stdout and " failed" not in out.stdout


def choice(dt, impl, case):
    cin, cout, (D, H, W) = case[:3]
    ks, st, tr = (2, 2, 1) if X.is_convt(case) else (case[3], case[4], 0)
    out = (C.c_int * 3)()
    E.check(E.lib.unet_op_conv_choice(EDT[dt], impl, cin, cout, D, H, W, ks, st, tr, out))
    return {"fwd": CC.FWD[out[0]], "dgrad": CC.DGRAD[out[1]], "wgrad": CC.WGRAD[out[2]]}


def choice2(dt, impl, case2):
    c0, c1, cout, (D, H, W), ks, st = case2
    out = (C.c_int * 3)()
    E.check(E.lib.unet_op_conv_choice2(EDT[dt], impl, c0, c1, cout, D, H, W, ks, st, 0, out))
    return {"fwd": CC.FWD[out[0]], "dgrad": CC.DGRAD[out[1]], "wgrad": CC.WGRAD[out[2]]}


def test_cases_reach_the_family_their_section_names():
    """Launches nothing: asks the engine (unet_op_conv_choice) what choose_conv (conv_select.h) gives the op entry points.  With
    IMPL_AUTO and the element type a section's comment names, every case of the section lands on the family the comment is about, in
    the direction it is about; the cases a comment describes as falling back are listed in the section (`other`) with where they land.
    With IMPL_DIRECT every case lands on the direct kernels.  Over all cases and both element types every enumerator an op entry
    point can return is reached (Fwd::head belongs to plans only).

    Not visible to this query, and not checked: what a family's launcher decides by itself -- the halo-tile or the sliding-window
    form, the row kernel among the small wgrads, a deep-level launcher declining a shape so that the MFMA conv runs instead."""
    direct = {"fwd": "direct", "dgrad": "direct", "wgrad": "direct"}
    reached = {d: set() for d in CC.FAMILIES}
    claims = 0
    for sec in CC.CONV_SECTIONS + CC.CONVT_SECTIONS:
        for case in sec.cases:
            for dt in ("fp32", "bf16"):
                assert choice(dt, U.IMPL_DIRECT, case) == direct, (sec.name, case, dt)
                for d, fam in choice(dt, U.IMPL_AUTO, case).items():
                    reached[d].add(fam)
            if sec.dt:
                want = dict(sec.expect, **sec.other.get(case, {}))
                got = choice(sec.dt, U.IMPL_AUTO, case)
                for d, fam in want.items():
                    assert got[d] == fam, "%s %s, %s: %s runs on %s, the section says %s" % (sec.name, case, sec.dt, d, got[d], fam)
                    claims += 1
    assert claims >= len(CC.CONV_CASES) + len(CC.CONVT_CASES) - 11   # the two unlabelled lead sections claim nothing
    # the two-source sections, asked with both sources (unet_op_conv_choice2); c1 = 0 is the one-source query
    claims2 = 0
    for sec in CC.CONV2_SECTIONS:
        for case2 in sec.cases:
            for dt in ("fp32", "bf16"):
                assert choice2(dt, U.IMPL_DIRECT, case2) == direct, (sec.name, case2, dt)
            if sec.dt:
                got = choice2(sec.dt, U.IMPL_AUTO, case2)
                for d, fam in dict(sec.expect, **sec.other.get(case2, {})).items():
                    assert got[d] == fam, "%s %s, %s: %s runs on %s, the section says %s" % (sec.name, case2, sec.dt, d, got[d], fam)
                    claims2 += 1
    assert claims2 >= len(CC.CONV2_CASES) - 2
    one = (C.c_int * 3)()
    E.check(E.lib.unet_op_conv_choice2(U.DTYPE_BF16, U.IMPL_AUTO, 32, 0, 16, 9, 9, 19, 3, 1, 0, one))
    assert {"fwd": CC.FWD[one[0]], "dgrad": CC.DGRAD[one[1]], "wgrad": CC.WGRAD[one[2]]} == choice("bf16", U.IMPL_AUTO, (32, 16, (9, 9, 19), 3, 1))
    assert reached["fwd"] == set(CC.FWD) - {"head"}
    assert reached["dgrad"] == set(CC.DGRAD)
    assert reached["wgrad"] == set(CC.WGRAD)
    with pytest.raises(RuntimeError):
        E.check(E.lib.unet_op_conv_choice(U.DTYPE_BF16, U.IMPL_AUTO, 16, 16, 0, 8, 8, 3, 1, 0, (C.c_int * 3)()))
