"""GPU (-m gpu): the conv / conv_trans op kernels on exact-arithmetic data, bit for bit against the C oracle, into poisoned and guarded
buffers (tests/gpu_exact.py), over the same shapes as the random-data op tests of test_gpu_parity.py (tests/conv_cases.py); and a
check that every shape reaches the kernel family its section is there for.

What the random-data tests cannot see and these can: one missing (tap, channel) product at one voxel (2e-3 of the output's scale at
Cin = 512, under the 1e-2 bound of the bf16 engine), a voxel the kernel never wrote (the caching allocator hands a freed block with
the previous, correct answer to the next test), scratch that is read before it is written, a write past either end of an output."""
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
    conv / conv_trans cases of this file run again in a child, bit for bit and into poisoned buffers as above."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-m", "gpu", "-p", "no:cacheprovider", "--maxfail=10",
                          "-k", "(test_conv3d_ops_exact or test_convt_ops_exact) and bf16"], capture_output=True, text=True, timeout=600,
                         env=dict(os.environ, **{switch: "1"}), cwd=root)
    assert out.returncode == 0, out.stdout[-6000:] + out.stderr[-2000:]
    assert " passed" in out.stdout and " failed" not in out.stdout


def choice(dt, impl, case):
    cin, cout, (D, H, W) = case[:3]
    ks, st, tr = (2, 2, 1) if X.is_convt(case) else (case[3], case[4], 0)
    out = (C.c_int * 3)()
    E.check(E.lib.unet_op_conv_choice(EDT[dt], impl, cin, cout, D, H, W, ks, st, tr, out))
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
    assert reached["fwd"] == set(CC.FWD) - {"head"}
    assert reached["dgrad"] == set(CC.DGRAD)
    assert reached["wgrad"] == set(CC.WGRAD)
    with pytest.raises(RuntimeError):
        E.check(E.lib.unet_op_conv_choice(U.DTYPE_BF16, U.IMPL_AUTO, 16, 16, 0, 8, 8, 3, 1, 0, (C.c_int * 3)()))
