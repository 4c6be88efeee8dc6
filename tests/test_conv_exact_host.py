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
    assert len(CC.CONV2_CASES) == 28 and len(set(CC.CONV2_CASES)) == 28
    assert all(len(c) == 6 and c[0] > 0 and c[1] > 0 for c in CC.CONV2_CASES)
    for sec in CC.CONV_SECTIONS + CC.CONVT_SECTIONS + CC.CONV2_SECTIONS:
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


# ---- two sources, split and accumulated destinations, heads ----
@pytest.mark.parametrize("case2", CC.CONV2_CASES)
def test_exact_preconditions_two_sources(case2):
    """the merged case holds every precondition of the one-source recipe, and so does dx + old for the accumulating destinations
    (integers in [-2, 2]); both halves of the split tensors carry data"""
    case = X.merged(case2)
    ref, old = X.reference(case), X.old_gradient(case)
    for dt in ("bf16", "fp32"):
        X.check_preconditions(ref, dt, str(case2))
        X.check_accumulate_precondition(ref, old, dt, str(case2))
    assert np.all(old == np.rint(old)) and np.abs(old).max() == 2 and old.shape == ref.dx.shape
    c0 = case2[0]
    for part in (slice(0, c0), slice(c0, None)):
        assert np.count_nonzero(ref.x[part]) > 0.5 * ref.x[part].size and np.count_nonzero(ref.dx[part]) > 0.5 * ref.dx[part].size
        assert np.count_nonzero(ref.dw[:, part] - ref.dw0[:, part]) > 0
    assert np.count_nonzero(ref.y) > 0.5 * ref.y.size


@pytest.mark.parametrize("case", CC.CONVT_ACC_CASES)
def test_exact_preconditions_convt_accumulate(case):
    ref, old = X.reference(case), X.old_gradient(case)
    for dt in ("bf16", "fp32"):
        X.check_preconditions(ref, dt, str(case))
        X.check_accumulate_precondition(ref, old, dt, str(case))
    assert np.count_nonzero(ref.dx) > 0.5 * ref.dx.size and np.count_nonzero(old) > 0.5 * old.size


@pytest.mark.parametrize("cin", CC.HEAD_CIN)
def test_exact_preconditions_heads(cin):
    for cout in CC.HEAD_COUT:
        for S in CC.HEAD_VOXELS:
            r = X.head_reference(cin, cout, S)
            what = "head %d -> %d, %d voxels" % (cin, cout, S)
            for dt in ("bf16", "fp32"):
                X.check_preconditions(r, dt, what)
                X.check_accumulate_precondition(r, r.old, dt, what)
            assert r.xa.min() >= 0 and r.xa.max() <= 2 and np.all(r.xa == np.rint(r.xa))
            assert set(np.unique(r.scale)) <= {-1.0, 1.0} and set(np.unique(r.shift)) <= {-1.0, 0.0, 1.0}
            if S >= 63:     # (a channel with shift -1 is dead under the relu: a third of dw's columns stay at their start values)
                assert np.count_nonzero(r.y) > 0.5 * r.y.size and np.count_nonzero(r.dw - r.dw0) > 0.25 * r.dw.size
                assert np.count_nonzero(r.dx) > 0.25 * r.dx.size


@pytest.mark.parametrize("case,plain", [(c, False) for c in CC.HEAD_CAP_CASES] + [(c, True) for c in CC.HEAD_PLAIN_CASES])
def test_exact_preconditions_heads_past_the_caps_and_plain(case, plain):
    """the same preconditions where a thread sums many voxels (dw / db are sums over up to 530001 voxels: integers far below 2^24 in
    any order) and on a plain source; the cap cases exceed both block caps of the launchers with a ragged last pass"""
    cin, cout, S = case
    r = X.head_reference(cin, cout, S, plain=plain)
    what = "head %d -> %d, %d voxels" % (cin, cout, S)
    for dt in ("bf16", "fp32"):
        X.check_preconditions(r, dt, what)
        X.check_accumulate_precondition(r, r.old, dt, what)
    assert np.count_nonzero(r.y) > 0.5 * r.y.size and np.count_nonzero(r.dx) > 0.25 * r.dx.size
    if plain:
        assert r.scale is None and r.shift is None and r.xa is r.x
        assert np.count_nonzero(r.dw - r.dw0) > 0.5 * r.dw.size     # no dead channel: every column of dw moves
    else:
        nchunk = cin // 16
        assert S * nchunk > 512 * 256 and (S + 63) // 64 * 64 * nchunk > 2048 * 256          # launch_head_bwd / launch_head_fwd
        assert S % (512 * 256 // nchunk) and S % (2048 * 256 // nchunk) and S % 64
        assert 2 * S + 4 < X.F32_EXACT      # the largest |partial sum| of dw (xa <= 2, |dy| <= 1) and db


def boundary_chunk_swapped(x, c0):
    """what a conv reads when the 16 channels on either side of the source boundary come from the other source"""
    out = x.copy()
    out[c0 - 16:c0], out[c0:c0 + 16] = x[c0:c0 + 16], x[c0 - 16:c0]
    return out


def boundary_moved(x, c0):
    """what a conv reads when it tests `c >= c0 + 16` for the source and still offsets source 1 by c0: channels [c0, c0 + 16) come from
    source 0, whose voxel rows are c0 wide -- the first 16 channels of its NEXT voxel (zero behind the last one)"""
    x0 = np.transpose(x[:c0], (1, 2, 3, 0)).reshape(-1, c0)
    nxt = np.concatenate([x0[1:], np.zeros((1, c0), x.dtype)])[:, :16]
    out = x.copy()
    out[c0:c0 + 16] = nxt.T.reshape(16, *x.shape[1:])
    return out


def at_one_voxel(y, x_wrong, x, w):
    """the last output voxel (every output channel) with the centre tap's products taken from x_wrong"""
    out = y.copy()
    v = tuple(s - 1 for s in y.shape[1:])
    wc = w[:, :, 1, 1, 1].astype(np.float64)
    out[(slice(None),) + v] += (wc @ (x_wrong[(slice(None),) + v].astype(np.float64) - x[(slice(None),) + v])).astype(np.float32)
    return out


TEETH2_CASES = [(240, 272, 32, (5, 6, 7), 3, 1), (16, 48, 32, (5, 6, 7), 3, 1), (16, 16, 16, (9, 9, 19), 3, 1)]


@pytest.mark.parametrize("case2", TEETH2_CASES)
def test_bitwise_comparison_rejects_wrong_sources_and_destinations(case2):
    """assert_exact must reject: the two sources swapped and the source boundary moved by 16 channels, each over the whole volume; the
    same two confined to the centre tap of one output voxel (one tile edge), where the swap is the smaller one a kernel can make
    there -- the 16 channels on either side of the boundary exchanged, boundary_chunk_swapped, NOT the two whole sources; an
    accumulating destination whose old value was ignored or added twice; and the first 16-channel row tile of d1 written into d0's
    position.

    At c0 + c1 >= 128 the two confined source mutations, on the random data of the random-data tests (N(0,1) activations rounded
    to bf16, 0.2 N(0,1) filters), must stay under the bound that covers the two-source layers in test_gpu_parity.py.  That is the
    NETWORK bound, 8e-2 of a tensor's maximum for bf16 logits and gradients, not the 1e-2 of that file's op tests (which the teeth test
    above uses and which would see both mutants): no op test there runs two sources.  Expected from the data's scale
    at Cin = 512: 32 (16) wrong channels of one tap give an error of sigma = 0.2 sqrt(2 * 32) = 1.6 (1.1) per output channel, about 2.5
    sigma at the worst of 32, against max|y| of about 3.5 * 0.2 sqrt(27 * 512) = 82: 5e-2 and 3.5e-2.  The figures are printed."""
    import torch
    assert case2 in CC.CONV2_CASES
    c0, c1 = case2[:2]
    case = X.merged(case2)
    ref, old = X.reference(case), X.old_gradient(case)
    everywhere = {"sources swapped": X.oracle_forward(case, np.concatenate([ref.x[c0:], ref.x[:c0]]), ref.w, ref.b),
                  "boundary moved": X.oracle_forward(case, boundary_moved(ref.x, c0), ref.w, ref.b)}
    confined = {"16 channels on either side of the boundary exchanged at one voxel": at_one_voxel(ref.y, boundary_chunk_swapped(ref.x, c0), ref.x, ref.w),
                "boundary moved at one voxel": at_one_voxel(ref.y, boundary_moved(ref.x, c0), ref.x, ref.w)}
    for name, wrong in list(everywhere.items()) + list(confined.items()):
        assert wrong.shape == ref.y.shape and not np.array_equal(wrong, ref.y), name
        with pytest.raises(AssertionError, match="differ bitwise"):
            X.assert_exact(wrong, ref.y, name)
        with pytest.raises(AssertionError, match="differ bitwise"):
            X.assert_exact(torch.from_numpy(wrong).to(torch.bfloat16), ref.y, name)
    # destinations
    d0, d1 = ref.dx[:c0] + old[:c0], ref.dx[c0:]
    X.assert_exact(d0.copy(), ref.dx[:c0] + old[:c0], "unchanged")
    wrong0 = {"accumulate ignored": ref.dx[:c0], "old value added twice": ref.dx[:c0] + 2 * old[:c0]}
    tile = d0.copy()
    tile[:16] = d1[:16]
    wrong0["a row tile of d1 in d0's position"] = tile
    for name, wrong in wrong0.items():
        for cast in (lambda a: a, lambda a: torch.from_numpy(np.array(a)).to(torch.bfloat16)):
            with pytest.raises(AssertionError, match="differ bitwise"):
                X.assert_exact(cast(wrong), d0, name)
    if c0 + c1 >= 128:
        x, w, b = real_data(case)
        y = X.oracle_forward(case, x, w, b)
        errs = {"16 channels on either side of the boundary exchanged at one voxel": rel(at_one_voxel(y, boundary_chunk_swapped(x, c0), x, w), y),
                "boundary moved at one voxel": rel(at_one_voxel(y, boundary_moved(x, c0), x, w), y)}
        print("relative error of the confined mutants on random data, %s: %s (op tests: 1e-2, network tests: 8e-2)" % (case2, errs))
        for name, e in errs.items():
            assert 0 < e < 8e-2, "%s: %g" % (name, e)
