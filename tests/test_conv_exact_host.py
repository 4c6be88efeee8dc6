"""CPU: the exact-arithmetic recipe of tests/gpu_exact.py holds its preconditions on every case of the conv / conv_trans op tests, and
the bitwise comparison has teeth where the relative-error criterion of the random-data tests has none.

Preconditions (on the C oracle's results alone): every reference value is an integer; max|y| and max|dx| <= 256, so the bf16 engine's
results are exactly representable; weight and bias gradients (with their start values) below 2^24.  A case that misses a bound gets
a smaller filter density in gpu_exact.PW_FACTOR.

Teeth: three wrong forward results are built in numpy from the oracle's -- one (tap, channel) product left out at one corner voxel, one
16-channel chunk left out at the centre tap along the last output row, one output row left at the values of another seed -- and
assert_exact must reject each.  For the first two at Cin >= 128 the criterion the random-data tests use, max|err| / max|ref| < 1e-2
on N(0,1) activations and 0.2 N(0,1) filters, must ACCEPT the same mutation: that is the hole the exact mode closes."""
import os
import re

import numpy as np
import pytest

import conv_cases as CC
import gpu_exact as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_case_lists_are_the_sections_in_order():
    assert len(CC.CONV_CASES) == 74 and len(set(CC.CONV_CASES)) == 74
    assert len(CC.CONVT_CASES) == 25 and len(set(CC.CONVT_CASES)) == 25
    for sec in CC.CONV_SECTIONS + CC.CONVT_SECTIONS:
        assert set(sec.other) <= set(sec.cases), sec.name
        for d, fam in list(sec.expect.items()) + [kv for o in sec.other.values() for kv in o.items()]:
            assert fam in CC.FAMILIES[d], (sec.name, d, fam)
        assert (sec.dt is None) == (not sec.expect), sec.name


def test_family_names_mirror_conv_select_h():
    text = open(os.path.join(ROOT, "unet-studio_amd", "csrc", "conv_select.h")).read()
    for enum, names in (("Fwd", CC.FWD), ("Dgrad", CC.DGRAD), ("Wgrad", CC.WGRAD)):
        m = re.search(r"enum class %s : unsigned char \{([^}]*)\}" % enum, text)
        assert m and tuple(s.strip() for s in m.group(1).split(",")) == names, enum


@pytest.mark.parametrize("case", CC.CONV_CASES + CC.CONVT_CASES)
def test_exact_preconditions(case):
    """every direction of every case: integral, within the bf16 bound (which implies the fp32 one), gradients below 2^24; and the
    data is not degenerate (most outputs nonzero)"""
    ref = X.reference(case)
    X.check_preconditions(ref, "bf16", str(case))
    X.check_preconditions(ref, "fp32", str(case))
    for name in ("x", "w", "b", "dy", "dw0", "db0"):
        a = getattr(ref, name)
        assert np.all(a == np.rint(a)) and np.abs(a).max() <= 4
    assert np.count_nonzero(ref.y) > 0.5 * ref.y.size and np.count_nonzero(ref.dx) > 0.5 * ref.dx.size, "degenerate data"
    assert np.count_nonzero(ref.dw - ref.dw0) > 0 and np.count_nonzero(ref.db - ref.db0) > 0


@pytest.mark.parametrize("case", [c[:5] for c in CC.FUSED_CASES])
def test_exact_preconditions_fused(case):
    ref = X.fused_reference(case)
    X.check_preconditions(ref, "bf16", str(case))
    assert ref.xa.min() >= 0 and ref.xa.max() <= 2 and np.all(ref.xa == np.rint(ref.xa))
    assert set(np.unique(ref.scale)) <= {-1.0, 1.0} and set(np.unique(ref.shift)) <= {-1.0, 0.0, 1.0}


@pytest.mark.parametrize("case", [(c[0], c[1], c[2], 3, 1) for c in CC.PLAIN_STATS_CASES] + [c[:5] for c in CC.FUSED_CASES])
def test_small_cases_have_exact_statistics(case):
    """<= 4096 output voxels: every channel's {sum y, sum y^2} is exact in fp32 (the exact rule of the statistics rows applies)"""
    y = (X.fused_reference(case) if case in [c[:5] for c in CC.FUSED_CASES] else X.reference(case)).y
    ok0, ok1, _ = X.exact_stat_channels(y)
    if y[0].size <= 4096:
        assert ok0.all() and ok1.all()


# ---- teeth ----
def rel(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return float(np.abs(a - b).max()) / max(float(np.abs(b).max()), 1e-30)


def real_data(case):
    """the random-data tests' inputs (bf16 engine: activations rounded to bf16)"""
    import torch
    cin, cout, dims, ks, _ = case
    g = lambda shape, seed, scale=1.0: (np.random.default_rng(seed).standard_normal(shape) * scale).astype(np.float32)
    x = torch.from_numpy(g((cin, *dims), 1)).to(torch.bfloat16).float().numpy()
    return x, g((cout, cin, ks, ks, ks), 2, 0.2), g((cout,), 3)


def without_one_product(y, x, w, nonzero):
    """output voxel (0, 0, 0) of channel co without the product of one (tap, channel) that lies inside the volume"""
    out = y.copy()
    for ci in range(x.shape[0]):
        for co in range(w.shape[0]):
            p = float(x[ci, 0, 0, 0]) * float(w[co, ci, 1, 1, 1])   # centre tap: input voxel (0, 0, 0)
            if p != 0.0 or not nonzero:
                out[co, 0, 0, 0] -= p
                return out
    raise AssertionError("no nonzero product at the corner")


def without_one_chunk(y, x, w):
    """the last output row (z, y last; every x, every output channel) without the first 16 input channels at the centre tap"""
    out = y.copy()
    z, r = y.shape[1] - 1, y.shape[2] - 1
    out[:, z, r, :] -= np.einsum("oc,cx->ox", w[:, :16, 1, 1, 1].astype(np.float64), x[:16, z, r, :].astype(np.float64)).astype(np.float32)
    return out


def with_stale_row(y, y_other):
    out = y.copy()
    z, r = y.shape[1] - 1, y.shape[2] - 1
    out[:, z, r, :] = y_other[:, z, r, :]
    return out


TEETH_CASES = [(512, 32, (5, 6, 7), 3, 1), (128, 32, (2, 2, 2), 3, 1), (32, 32, (9, 7, 20), 3, 1)]
# (case, mutation) pairs at Cin >= 128 that the relative-error criterion accepts on the random data: the single product is 7e-4 and
# 2.5e-3 of the output's maximum.  Left out: the 16-channel chunk on both cases -- over a whole row and every output channel its
# largest term reaches 3.8e-2 and 9.6e-2 of the maximum, which that criterion does see
REL_ACCEPTS = {((512, 32, (5, 6, 7), 3, 1), "product"), ((128, 32, (2, 2, 2), 3, 1), "product")}


@pytest.mark.parametrize("case", TEETH_CASES)
def test_bitwise_comparison_rejects_what_the_relative_bound_accepts(case):
    assert case in CC.CONV_CASES
    ref = X.reference(case)
    other = X.reference(case, 1)
    X.assert_exact(ref.y.copy(), ref.y, "unchanged")
    mutants = {"product": without_one_product(ref.y, ref.x, ref.w, True), "chunk": without_one_chunk(ref.y, ref.x, ref.w),
               "stale row": with_stale_row(ref.y, other.y)}
    for name, wrong in mutants.items():
        assert not np.array_equal(wrong, ref.y), name
        with pytest.raises(AssertionError, match="differ bitwise"):
            X.assert_exact(wrong, ref.y, name)
        import torch
        with pytest.raises(AssertionError, match="differ bitwise"):   # ... and as the bf16 engine would store it
            X.assert_exact(torch.from_numpy(wrong).to(torch.bfloat16), ref.y, name)
    if case[0] >= 128:
        x, w, b = real_data(case)
        y = X.oracle_forward(case, x, w, b)
        errs = {"product": rel(without_one_product(y, x, w, False), y), "chunk": rel(without_one_chunk(y, x, w), y)}
        print("relative error of the mutants on random data, %s: %s" % (case, errs))
        for name, e in errs.items():
            if (case, name) in REL_ACCEPTS:
                assert 0 < e < 1e-2, "%s: %g" % (name, e)
