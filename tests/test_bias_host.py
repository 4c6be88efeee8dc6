"""CPU: the host half of the intensity-inhomogeneity correction (include/unet_bias.h, unet-studio_amd/bias.py) -- the ABI the library
exports, argument errors found before any device call, and the restatements of tests/bias_ref.py checked on hand-written answers.
The quality of the definition (how far the fit flattens a shaded phantom, how well the fitted gain follows the true one) is measured
here, on the restatement, not on the device.  No device calls."""
import ctypes
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

import unet_studio_amd as U
from unet_studio_amd import bias as BS

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bias_ref as ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


# ---- the ABI -------------------------------------------------------------------------------------------------------------------------
def test_unet_bias_h_declares_exactly_the_exports_and_no_other_header_names_the_prefix():
    lib = ctypes.CDLL(U.engine.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "unet_bias.h")).read()
    declared = set(re.findall(r"\b(unet_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(BS.EXPORTS) == {"unet_bias_" + n for n in ("lattice", "scratch_bytes", "logcode", "levels", "residual", "sweep",
                                                                     "refine", "cost", "fit", "apply")}
    for name in sorted(declared):
        assert hasattr(lib, name), "libunet_hip.so does not export " + name
    impls = {k: int(v) for k, v in re.findall(r"UNET_BIAS_(IMPL_[A-Z]+) = (\d+)", hdr)}
    assert impls == {"IMPL_DEFAULT": BS.IMPL_DEFAULT, "IMPL_NODE": BS.IMPL_NODE, "IMPL_VOXEL": BS.IMPL_VOXEL}
    assert (BS.IMPL_DEFAULT, BS.IMPL_NODE, BS.IMPL_VOXEL) == (0, 1, 2)
    limits = {k: int(v) for k, v in re.findall(r"#define UNET_BIAS_MAX_([A-Z]+) (\d+)", hdr)}
    assert limits == {"CLASSES": BS.MAX_CLASSES, "LAM": BS.MAX_LAM, "LEVELS": BS.MAX_LEVELS, "SWEEPS": BS.MAX_SWEEPS, "OUTER": BS.MAX_OUTER,
                      "ROWS": BS.MAX_ROWS}
    assert limits["LEVELS"] * limits["OUTER"] <= limits["ROWS"]
    assert int(re.search(r"#define UNET_BIAS_MAX (\d+)", hdr).group(1)) == BS.MAX == ref.MAX == 8192
    assert "#define UNET_BIAS_NONE (-2147483647 - 1)" in hdr and BS.NONE == ref.NONE == -2 ** 31
    assert "#define UNET_BIAS_SKIP (-32768)" in hdr and BS.SKIP == ref.SKIP == -2 ** 15
    assert (BS.MAX_CLASSES, BS.MAX_LAM, BS.MAX_ROWS) == (ref.MAX_CLASSES, ref.MAX_LAM, ref.MAX_ROWS) and BS.SPACINGS == (4, 8, 16, 32)
    assert BS.DEFAULT_LEVELS == ref.DEFAULT_LEVELS and (BS.DEFAULT_OUTER, BS.DEFAULT_CLIP) == (ref.DEFAULT_OUTER, ref.DEFAULT_CLIP)
    assert U.bias is BS and BS.Plan([1]) == ([1], BS.DEFAULT_LEVELS, BS.DEFAULT_OUTER, BS.DEFAULT_CLIP, BS.IMPL_DEFAULT)
    assert BS.Plan([1, 2], clip=100).clip == 100
    prose = re.sub(r"\s*\n \*\s+", " ", hdr)                        # the comment's lines joined
    assert "this project's definition" in prose and "NOT pinned" in prose
    # the header speaks of those it builds on by file name or DESIGN section only
    low = hdr.lower()
    for other in ("unet_deform", "unet_coreg", "unet_start", "unet_cowarp_", "unet_warp_", "unet_recal_", "unet_tiles_", "unet_space_",
                  "unet_components_", "unet_preproc_", "unet_stats_", "unet_reg_", "unet_table_", "unet_dist_", "unet_atlas_", "unet_postproc_"):
        assert other not in low, other
    assert "unet_warp.h" in low
    for h in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if h != "unet_bias.h":
            assert "unet_bias" not in open(os.path.join(ROOT, "include", h)).read().lower(), h


def test_the_table_is_exp2_in_float64_rounded_to_float32():
    text = open(os.path.join(ROOT, "unet-studio_amd", "csrc", "bias_table.h")).read()
    table = np.array([float.fromhex(v) for v in re.findall(r"(0x1\.[0-9a-f]+p\+0)f,", text)], np.float64)
    assert table.size == 4096 and (table == table.astype(F)).all()   # every literal is a float32
    want = np.exp2(np.arange(4096, dtype=np.float64) / 4096.0).astype(F)
    assert table.astype(F).tobytes() == want.tobytes() == ref.TABLE.tobytes()
    assert ref.TABLE[0] == 1 and ref.TABLE[2048] == F(math.sqrt(2.0)) and (np.diff(ref.TABLE.astype(np.float64)) > 0).all() and ref.TABLE[-1] < 2


# ---- argument errors, before any device call -------------------------------------------------------------------------------------
P = [ctypes.c_void_p(0x10000 * (i + 1)) for i in range(8)]          # never dereferenced
ODD = ctypes.c_void_p(0x30002)
CLS = (ctypes.c_int * 3)(1, 2, 3)
LV = (ctypes.c_int * 6)(16, 2, 1, 8, 2, 1)
BIG = 1 << 40


def err(rc):
    assert rc != 0
    return U.engine.lib.unet_last_error().decode()


def test_lattice_scratch_logcode_refine_cost_apply_argument_errors_need_no_device():
    lib = U.engine.lib
    n = [ctypes.c_int() for _ in range(3)]
    assert lib.unet_bias_lattice(5, 6, 7, 4, *(ctypes.byref(v) for v in n)) == 0 and [v.value for v in n] == [3, 3, 3]
    assert BS.lattice((7, 6, 5), 4) == (3, 3, 3) == ref.lattice_ref((7, 6, 5), 4) and BS.lattice((33, 9, 17), 32) == (3, 2, 2)
    assert "g must be 4, 8, 16 or 32, got 5" in err(lib.unet_bias_lattice(5, 6, 7, 5, *(ctypes.byref(v) for v in n)))
    assert "volume dimensions" in err(lib.unet_bias_lattice(0, 6, 7, 4, *(ctypes.byref(v) for v in n)))
    assert "volume grid" in err(lib.unet_bias_lattice(2048, 1024, 1024, 4, *(ctypes.byref(v) for v in n)))
    assert "null output" in err(lib.unet_bias_lattice(5, 6, 7, 4, None, None, None))

    size = ctypes.c_size_t()

    def sb(s=(20, 18, 14), levels=LV, nl=2, out=ctypes.byref(size)):
        return err(lib.unet_bias_scratch_bytes(*s, levels, nl, out))

    assert lib.unet_bias_scratch_bytes(20, 18, 14, LV, 2, ctypes.byref(size)) == 0 and size.value >= 2 * 20 * 18 * 14
    assert "n_levels must be in [1, 4], got 0" in sb(nl=0) and "n_levels" in sb(nl=5) and "null levels" in sb(levels=None)
    assert "volume dimensions" in sb(s=(20, -1, 14)) and "null output" in sb(out=None)
    assert "level 0: g must be 4, 8, 16 or 32, got 6" in sb(levels=(ctypes.c_int * 3)(6, 1, 0), nl=1)
    assert "level 1: g must be half the level before's, got 4" in sb(levels=(ctypes.c_int * 6)(16, 1, 0, 4, 1, 0))
    assert "level 1: sweeps must be in [1, 16], got 17" in sb(levels=(ctypes.c_int * 6)(16, 1, 0, 8, 17, 0))
    assert "sweeps must be" in sb(levels=(ctypes.c_int * 3)(16, 0, 0), nl=1)
    assert "level 0: lam must be in [0, 4096], got 4097" in sb(levels=(ctypes.c_int * 3)(16, 1, 4097), nl=1)
    assert "lam must be" in sb(levels=(ctypes.c_int * 3)(16, 1, -1), nl=1)
    assert sb(nl=9).startswith("unet_bias_scratch_bytes: ")

    assert "null v" in err(lib.unet_bias_logcode(None, 8, P[0], None)) and "null q" in err(lib.unet_bias_logcode(P[0], 8, None, None))
    assert "voxels must be in [1, 2^31), got 0" in err(lib.unet_bias_logcode(P[0], 0, P[1], None))
    assert "voxels must be" in err(lib.unet_bias_logcode(P[0], 1 << 31, P[1], None))
    assert "v must be 4-byte aligned" in err(lib.unet_bias_logcode(ODD, 8, P[1], None))
    assert "q must be 4-byte aligned" in err(lib.unet_bias_logcode(P[0], 8, ODD, None))

    def refine(B=P[0], s=(20, 18, 14), g=8, out=P[1]):
        return err(lib.unet_bias_refine(B, *s, g, out, None))

    assert "null B_coarse" in refine(B=None) and "null B_fine" in refine(out=None) and "g must be 8, 16 or 32, got 4" in refine(g=4)
    assert "B_coarse must be 4-byte aligned" in refine(B=ODD) and "B_fine must be 4-byte aligned" in refine(out=ODD)
    assert "volume dimensions" in refine(s=(0, 1, 1))

    def cost(r=P[0], s=(20, 18, 14), B=P[1], g=8, out=P[2]):
        return err(lib.unet_bias_cost(r, *s, B, g, out, None))

    assert "null r" in cost(r=None) and "null B" in cost(B=None) and "null cost" in cost(out=None) and "g must be" in cost(g=3)
    assert "r must be 2-byte aligned" in cost(r=ctypes.c_void_p(0x30001)) and "cost must be 8-byte aligned" in cost(out=ctypes.c_void_p(0x30004))
    assert "volume grid" in cost(s=(2048, 1024, 1024))

    def apply(v=P[0], s=(20, 18, 14), B=P[1], g=8, out=P[2], gain=P[3]):
        return err(lib.unet_bias_apply(v, *s, B, g, out, gain, None))

    assert "null B" in apply(B=None) and "g must be" in apply(g=64) and "volume dimensions" in apply(s=(1, 1, 0))
    assert "nothing to form" in apply(out=None, gain=None) and "both or neither" in apply(v=None) and "both or neither" in apply(out=None)
    for name in ("v", "B", "out", "gain"):
        assert name + " must be 4-byte aligned" in apply(**{name: ODD})
    assert apply(g=1).startswith("unet_bias_apply: ")


def test_levels_residual_sweep_and_fit_argument_errors_need_no_device():
    lib = U.engine.lib

    def levels(q=P[0], labels=P[1], lb=1, s=(20, 18, 14), cls=CLS, K=3, B=P[2], g=8, out=P[3]):
        return err(lib.unet_bias_levels(q, labels, lb, *s, cls, K, B, g, out, None))

    def residual(q=P[0], labels=P[1], lb=2, s=(20, 18, 14), cls=CLS, K=3, lev=P[2], clip=100, r=P[3]):
        return err(lib.unet_bias_residual(q, labels, lb, *s, cls, K, lev, clip, r, None))

    def fit(q=P[0], labels=P[1], lb=1, s=(20, 18, 14), cls=CLS, K=3, clip=100, lv=LV, nl=2, outer=2, B=P[2], report=P[3], impl=0, scratch=P[4],
            sbytes=BIG):
        return err(lib.unet_bias_fit(q, labels, lb, *s, cls, K, clip, lv, nl, outer, B, report, impl, scratch, sbytes, None))

    for call in (levels, residual, fit):                            # what the three share
        assert "null q" in call(q=None) and "q must be 4-byte aligned" in call(q=ODD) and "null labels" in call(labels=None)
        assert "lbytes must be 1 or 2, got 4" in call(lb=4) and "lbytes" in call(lb=0)
        assert "volume dimensions" in call(s=(20, 0, 14)) and "volume grid" in call(s=(2048, 1024, 1024))
        assert "K must be in [1, 16], got 0" in call(K=0) and "K must be" in call(cls=(ctypes.c_int * 17)(*range(17)), K=17)
        assert "null classes" in call(cls=None)
        assert "classes must be label values in [0, 65535], got 65536" in call(cls=(ctypes.c_int * 3)(1, 65536, 3))
        assert "classes must be label values" in call(cls=(ctypes.c_int * 3)(1, -1, 3))
        assert "classes must be distinct, got 2 twice" in call(cls=(ctypes.c_int * 3)(2, 1, 2))
        assert "null q" in call(q=None, labels=ctypes.c_void_p(0x30001))   # labels: any alignment
    assert "null B" in levels(B=None) and "B must be 4-byte aligned" in levels(B=ODD) and "g must be 4, 8, 16 or 32, got 0" in levels(g=0)
    assert "null levels_out" in levels(out=None) and "levels_out must be 8-byte aligned" in levels(out=ctypes.c_void_p(0x30004))
    assert "null levels_in" in residual(lev=None) and "levels_in must be 8-byte aligned" in residual(lev=ctypes.c_void_p(0x30004))
    assert "clip must be in [0, 8192], got 8193" in residual(clip=8193) and "clip must be" in residual(clip=-1)
    assert "null r" in residual(r=None) and "r must be 16-byte aligned" in residual(r=ctypes.c_void_p(0x30008))
    assert residual(K=99).startswith("unet_bias_residual: ") and levels(K=99).startswith("unet_bias_levels: ")

    def sweep(r=P[0], s=(20, 18, 14), B=P[1], g=8, lam=1, info=P[2], impl=0, scratch=P[3], sbytes=BIG):
        return err(lib.unet_bias_sweep(r, *s, B, g, lam, info, impl, scratch, sbytes, None))

    assert "null r" in sweep(r=None) and "r must be 16-byte aligned" in sweep(r=ctypes.c_void_p(0x30002)) and "null B" in sweep(B=None)
    assert "B must be 4-byte aligned" in sweep(B=ODD) and "volume dimensions" in sweep(s=(-20, 18, 14)) and "g must be" in sweep(g=12)
    assert "lam must be in [0, 4096], got 4097" in sweep(lam=4097) and "lam must be" in sweep(lam=-1)
    assert "null info" in sweep(info=None) and "info must be 8-byte aligned" in sweep(info=ctypes.c_void_p(0x30004))
    assert "unknown impl 3" in sweep(impl=3) and "unknown impl -1" in sweep(impl=-1) and "null scratch" in sweep(scratch=None)
    nodes = int(np.prod(BS.lattice((14, 18, 20), 8)))                # a sweep needs the counters alone: 256 + 16 B per node, rounded up
    need = 256 + (16 * nodes + 255) // 256 * 256
    assert "scratch too small (256 + 16 bytes per node" in sweep(sbytes=need - 1) and need <= BS.scratch_bytes((14, 18, 20), [(8, 1, 0)])
    assert "null r" in sweep(r=None, sbytes=need)                   # enough: the refusal is another argument's
    assert sweep(g=5).startswith("unet_bias_sweep: ")

    assert "clip must be in [0, 8192], got 9000" in fit(clip=9000) and "n_levels must be" in fit(nl=0) and "null levels" in fit(lv=None)
    assert "level 1: g must be half" in fit(lv=(ctypes.c_int * 6)(16, 1, 0, 4, 1, 0)) and "sweeps must be" in fit(lv=(ctypes.c_int * 6)(16, 0, 0, 8, 1, 0))
    assert "lam must be" in fit(lv=(ctypes.c_int * 6)(16, 1, 5000, 8, 1, 0))
    assert "outer must be in [1, 8], got 0" in fit(outer=0) and "outer must be in [1, 8], got 9" in fit(outer=9)
    assert "null B_out" in fit(B=None) and "B_out must be 4-byte aligned" in fit(B=ODD)
    assert "null report" in fit(report=None) and "report must be 8-byte aligned" in fit(report=ctypes.c_void_p(0x30004))
    assert "unknown impl 7" in fit(impl=7) and "null scratch" in fit(scratch=None)
    assert "scratch too small" in fit(sbytes=BS.scratch_bytes((14, 18, 20), [(16, 2, 1), (8, 2, 1)]) - 1)
    assert fit(outer=99).startswith("unet_bias_fit: ")


def test_wrapper_errors_need_no_device():
    f32, u8 = torch.zeros((2, 2, 2), dtype=torch.float32), torch.zeros((2, 2, 2), dtype=torch.uint8)
    q, r, B = torch.zeros((2, 2, 2), dtype=torch.int32), torch.zeros((2, 2, 2), dtype=torch.int16), torch.zeros((2, 2, 2), dtype=torch.int32)
    for call in (lambda: BS.logcode(f32), lambda: BS.levels(q, u8, [1], B, 4), lambda: BS.residual(q, u8, [1], q), lambda: BS.sweep(r, B, 4, 1),
                 lambda: BS.cost(r, B, 4), lambda: BS.fit(q, u8, [1]), lambda: BS.apply(f32, B, 4), lambda: BS.correct(f32, u8, BS.Plan([1])),
                 lambda: BS.refine(B, (2, 2, 2), 8), lambda: BS.gain(B, 4, (2, 2, 2))):
        with pytest.raises(U.UNetError, match="device tensor"):
            call()
    with pytest.raises(U.UNetError, match="plan must be a bias.Plan"):
        BS.correct(f32, u8, 7)
    with pytest.raises(U.UNetError, match="bias.outer must be an integer"):
        BS.correct(f32, u8, BS.Plan([1], outer=1.5))
    with pytest.raises(U.UNetError, match="levels must be rows of"):
        BS.scratch_bytes((4, 4, 4), [(8, 1)])
    with pytest.raises(U.UNetError, match="g must be 8, 16 or 32"):
        BS.refine(B, (2, 2, 2), 4)
    with pytest.raises(U.UNetError, match="g must be 4, 8, 16 or 32, got 3"):
        BS.lattice((4, 4, 4), 3)
    # the host arithmetic
    report = np.full((BS.MAX_ROWS, 6), -1, np.int64)
    report[0], report[1] = (16, 0, 3, 0, 4096 * 4096 * 10, 10), (8, 0, 2, 5, 0, 0)
    rows = BS.summary(report)
    assert rows[0] == dict(g=16, round=0, sweeps=3, changed=0, cost=4096 * 4096 * 10, count=10, rms=1.0) and len(rows) == 2
    assert rows[1]["changed"] == 5 and math.isnan(rows[1]["rms"])
    v, lab = np.array([[[1.0, 3.0, 100.0, 2.0]]], F), np.array([[[1, 1, 0, 1]]], np.uint8)
    assert BS.cv(v, lab, 1) == float(np.std([1.0, 3.0, 2.0]) / 2.0) == ref.cv_ref(v, lab, 1) and math.isnan(BS.cv(v, lab, 9))


# ---- the restatements by hand --------------------------------------------------------------------------------------------------------
def test_the_log_codes_by_hand():
    assert ref.logcode_ref(np.array([1, 2, 3], F)).tolist() == [0, 4096, 6492]
    with np.errstate(all="ignore"):
        none = np.array([0.0, -1.0, 1e-40, np.inf, np.nan, -0.0, -np.inf], F)
    assert ref.logcode_ref(none).tolist() == [ref.NONE] * 7
    # truncation towards minus infinity on both sides of 1, and the ends of the range
    assert ref.logcode_ref(np.array([0.5, 0.75, 1.5, 2.0 ** -126, 2.0 ** 127], F)).tolist() == [-4096, -1700, 2396, -126 * 4096, 127 * 4096]
    assert math.floor(4096 * math.log2(0.75)) == -1700 and math.floor(4096 * math.log2(3)) == 6492
    rng = np.random.default_rng(0)
    v = np.exp2(rng.uniform(-100, 100, 4000)).astype(F)
    q = ref.logcode_ref(v)
    exact = 4096 * np.log2(v.astype(np.float64))
    assert q.dtype == np.int32 and (q <= exact + 1e-6).all() and (exact - q < 1 + 1.0 / 16).all()   # f is truncated at 16 bits, then 4 are dropped


def test_a_node_pair_field_and_a_level_with_a_negative_sum_by_hand():
    shape, g = (1, 1, 5), 4
    assert ref.lattice_ref(shape, g) == (2, 2, 3)
    B = ref.zero_field(shape, g)
    B[0, 0, 0], B[0, 0, 1] = 64, 128
    # voxel x on the row y = z = 0: n = (4 - x) * 4 * 4 * 64 + x * 4 * 4 * 128 up to x = 3; x = 4 sits on the second node
    assert ref.corner_sum(B, g, *ref.coords(shape)).tolist() == [4096, 3 * 16 * 64 + 16 * 128, 2 * 16 * 64 + 2 * 16 * 128, 16 * 64 + 3 * 16 * 128, 8192]
    q = np.array([[[-7, -2, 100, ref.NONE, 5]]], np.int32)
    labels = np.array([[[1, 1, 2, 1, 3]]], np.uint8)
    lev = ref.levels_ref(q, labels, [1, 2, 7], ref.zero_field(shape, g), g)
    assert lev[0].tolist() == [-5, 2, -9] and lev[1].tolist() == [100, 1, 100]      # floor(-9 / 2) = -5, not -4
    assert lev[2].tolist() == [ref.NONE, 0, 0] and (lev[3:] == [ref.NONE, 0, 0]).all()
    # under the field: b = n >> 6 = 64, 80, 96, 112, 128
    lev = ref.levels_ref(q, labels, [1, 2, 7], B, g)
    assert lev[0].tolist() == [(-7 - 64 - 2 - 80) // 2, 2, -153] and lev[1].tolist() == [4, 1, 4]
    r = ref.residual_ref(q, labels, [1, 2, 7], ref.levels_ref(q, labels, [1, 2, 7], ref.zero_field(shape, g), g), 2)
    assert r.dtype == np.int16 and r.tolist() == [[[-2, ref.SKIP, 0, ref.SKIP, ref.SKIP]]]   # -2 + 5 = 3 > clip; no q; class 3 not listed
    assert ref.cost_ref(r, B, g).tolist() == [(-2 - 64) ** 2 + (0 - 96) ** 2, 2]


def test_the_rounding_at_an_exact_half_and_the_clamp_by_hand():
    shape, g = (1, 1, 5), 4                                         # lattice (2, 2, 3); no voxel counts: the links alone move the nodes
    r = np.full(shape, ref.SKIP, np.int16)
    for value, want in ((2, 1), (-2, 0), (6, 2), (-6, -1), (1, 0), (-1, 0), (3, 1), (-3, -1)):
        B = ref.zero_field(shape, g)
        B[0, 1, 1] = value                                          # a neighbour of node (k, j, i) = (0, 0, 1) that moves after it
        seen = {}
        ref.sweep_ref(r, B, g, 1, after_node_pass=lambda c, before, after: seen.setdefault(c, (before.copy(), after.copy())))
        before, after = seen[1]                                     # node (0, 0, 1) has colour 1 and 4 neighbours: d = floor(value / 4 + 1 / 2)
        assert before[0, 0, 1] == 0 and before[0, 1, 1] == value and after[0, 0, 1] == want, (value, want)
    B, info = ref.sweep_ref(r, ref.zero_field(shape, g), g, 0)
    assert not B.any() and info.tolist() == [0, 0]                  # den = 0: not visited
    B, info = ref.sweep_ref(r, ref.zero_field(shape, g), g, 5)
    assert not B.any() and info.tolist() == [0, 12]
    # the clamp: one voxel at x = 2 with r = 8192 between node 0 at -8192 and node 1 at 0: d = 2 r - B_0 - B_1 = 24576
    r = np.full(shape, ref.SKIP, np.int16)
    r[0, 0, 2] = 8192
    B = ref.zero_field(shape, g)
    B[0, 0, 0] = -8192
    seen = {}
    ref.sweep_ref(r, B, g, 0, after_node_pass=lambda c, before, after: seen.setdefault(c, after.copy()))
    assert seen[0][0, 0, 0] == 8192 and seen[0][0, 0, 1] == 0
    assert seen[1][0, 0, 1] == 8192                                 # then d = 16384 - 8192 - 0 for the second node: exactly the bound


def test_apply_by_hand():
    shape, g = (2, 3, 5), 4
    v = np.array([1.0, 3.0, -2.5, 1e-3, 100.0] * 6, F).reshape(shape)
    out, gain = ref.apply_ref(v, ref.zero_field(shape, g), g)
    assert out.tobytes() == v.tobytes() and (gain == 1).all()
    B = np.full(ref.lattice_ref(shape, g), 4096, np.int32)          # twice too bright everywhere: c = -4096, k = -1, j = 0
    out, gain = ref.apply_ref(v, B, g)
    assert (out == v / 2).all() and (gain == 0.5).all()
    B[:] = 4096 + 100                                               # c = -4196: k = -2, j = 3996
    out, gain = ref.apply_ref(v, B, g)
    assert (-4196 >> 12, -4196 & 4095) == (-2, 3996) and (gain == ref.TABLE[3996] / 4).all() and (out == (v * ref.TABLE[3996]) / 4).all()
    assert abs(float(gain[0, 0, 0]) - 2.0 ** (-4196 / 4096)) < 1e-7
    B[:] = -5000                                                    # too dark: k = +1
    out, gain = ref.apply_ref(v, B, g)
    assert (gain == ref.TABLE[5000 - 4096] * 2).all() and (out == (v * ref.TABLE[904]) * 2).all()
    with np.errstate(all="ignore"):
        odd = np.array([np.nan, np.inf, -np.inf, 0.0, 3e38] * 6, F).reshape(shape)
        odd.reshape(-1).view(np.uint32)[0] = 0x7F800001             # a signalling NaN
        out, _ = ref.apply_ref(odd, B, g)
    assert out.view(np.uint32).reshape(-1)[:5].tolist() == [0x7FC00000, 0x7F800000, 0xFF800000, 0, 0x7F800000]
    out, _ = ref.apply_ref(odd, ref.zero_field(shape, g), g)
    assert out.tobytes() == odd.tobytes()                           # a zero field: the bits, of a signalling NaN too
    # the rounding of c: n / g^3 = 0.5 rounds up, -0.5 too (towards plus infinity)
    half = np.zeros(ref.lattice_ref((1, 1, 5), 4), np.int32)
    half[0, 0, 0] = 2                                               # at x = 1: n = 48 * 2 = 96 = 1.5 * 64 -> -n / 64 = -1.5 -> c = -1
    lg3 = 6
    n = ref.corner_sum(half, 4, *ref.coords((1, 1, 5)))
    assert n.tolist() == [128, 96, 64, 32, 0] and ((-n + 32) >> lg3).tolist() == [-2, -1, -1, 0, 0]


def test_refine_by_hand():
    shape = (1, 1, 9)                                               # coarse g = 8: (2, 2, 3); fine g = 4: (2, 2, 4)
    B = np.zeros(ref.lattice_ref(shape, 8), np.int32)
    B[:, :, 0], B[:, :, 1], B[:, :, 2] = 8, 17, -3
    fine = ref.refine_ref(B, shape, 8)
    assert fine.shape == (2, 2, 4) and fine[0, 0].tolist() == [8, (8 * 4 + 17 * 4 + 4) >> 3, 17, (17 * 4 - 3 * 4 + 4) >> 3] == [8, 13, 17, 7]


# ---- the energy, the bounds, the early end ---------------------------------------------------------------------------------------
def small_case():
    rng = np.random.default_rng(5)
    shape = (14, 18, 20)                                            # 20 x 18 x 14
    z, y, x = np.indices(shape).astype(np.float64)
    labels = (1 + ((x // 3 + y // 2 + z) % 2)).astype(np.uint8)
    labels[rng.random(shape) < 0.15] = 0
    volume = (np.choose(labels, [7.0, 90.0, 50.0]) * np.exp2(0.4 * x / 20 - 0.3 * (y / 18) ** 2) * (1 + 0.03 * rng.standard_normal(shape))).astype(F)
    volume[rng.random(shape) < 0.02] = 0
    return volume, labels


def test_the_exact_energy_never_rises_over_a_fit():
    volume, labels = small_case()
    q = ref.logcode_ref(volume)
    trace = []

    def watch(r, before, after, g, lam):
        e0, e1 = ref.energy(r, before, g, lam), ref.energy(r, after, g, lam)
        assert isinstance(e0, int) and e1 <= e0, (g, lam, e0, e1)
        trace.append((g, e0, e1))

    for lam in (0, 3):
        B, report = ref.fit_ref(q, labels, [1, 2], 2048, [(8, 3, lam), (4, 3, lam)], 2, watch=watch)
        assert B.any() and (report[:4, 3] > 0).all()
    assert len(trace) == 24 and any(e1 < e0 for _, e0, e1 in trace)
    # and across every colour pass of one sweep from a wild start, clamped nodes among them
    rng = np.random.default_rng(6)
    r = ref.residual_ref(q, labels, [1, 2], ref.levels_ref(q, labels, [1, 2], ref.zero_field(q.shape, 8), 8), 2048)
    wild = rng.integers(-8192, 8193, ref.lattice_ref(q.shape, 8)).astype(np.int32)
    steps = []
    out, _ = ref.sweep_ref(r, wild, 8, 2, after_node_pass=lambda c, b, a: steps.append((ref.energy(r, b, 8, 2), ref.energy(r, a, 8, 2))))
    assert len(steps) == 8 and all(e1 <= e0 for e0, e1 in steps) and steps[-1][1] < steps[0][0]


def test_the_int64_bounds_hold_at_the_worst_case_support():
    for g in (4, 8, 16, 32):
        b = ref.worst_case_bounds(g)
        assert b["sum_w"] == g ** 6 and b["e"] == 2 * 8192 * g ** 3 <= 2 ** 29
        assert b["S1"] <= 2 ** 59 and b["S2"] <= g ** 9 <= 2 ** 45 and b["Lam"] <= 2 ** 42
        assert b["num"] < 2 ** 60 and b["den"] < 2 ** 46 and b["top"] < 2 ** 62 < 2 ** 63 - 1
    # the restatement at that worst case, in int64, equals Python integers: a full support at g = 32 around the middle node
    shape, g = (64, 64, 64), 32
    r = np.full(shape, 8192, np.int16)
    B = np.full(ref.lattice_ref(shape, g), -8192, np.int32)
    after, info = ref.sweep_ref(r, B, g, ref.MAX_LAM, colours=(7,))  # the pass of the middle node's colour alone, from this state
    b = ref.worst_case_bounds(g)
    S1, S2, Lam = b["S1"], b["S2"], b["Lam"]                        # every neighbour equal: the links add nothing to num
    d = (2 * S1 + (S2 + 6 * Lam)) // (2 * (S2 + 6 * Lam))
    assert after[1, 1, 1] == max(-8192, min(8192, -8192 + d)) == 7461 and info.tolist() == [1, 1]


def test_ending_early_changes_nothing():
    volume, labels = small_case()
    q = ref.logcode_ref(volume)
    levels = [(8, 16, 1), (4, 16, 1)]
    early = ref.fit_ref(q, labels, [1, 2], 2048, levels, 2)
    full = ref.fit_ref(q, labels, [1, 2], 2048, levels, 2, early=False)
    assert early[0].tobytes() == full[0].tobytes() and early[1].tobytes() == full[1].tobytes()
    assert (early[1][:4, 2] < 16).any(), early[1][:4]


# ---- the quality of the definition -------------------------------------------------------------------------------------------------------
def fitted_gain(B, g, shape):
    """what the fit takes the shading to be: the inverse of the gain apply multiplies by"""
    return 1.0 / ref.apply_ref(np.ones(shape, F), B, g)[1].astype(np.float64)


def test_the_default_plan_flattens_the_phantom():
    """Measured on the restatement, on bias_ref.phantom() ((36, 40, 48), classes 1 and 2 at 100 and 60, a gain of 0.77 .. 1.30, 3 %
    noise) under the default plan (32 -> 16 -> 8, 4 sweeps, lam 1, 2 outer rounds, clip 2048): the coefficient of variation of class
    1 falls from 0.0734 to 0.0301 (the noise alone: 0.0301), a factor of 2.44; class 2 from 0.0456 to 0.0303; the fitted gain
    correlates with the true one at 0.9987 over classes 1 and 2.  The factor asserted is the measured one less a quarter: 1.83; the
    correlation's floor leaves a quarter of its distance from 1."""
    volume, labels, gain = ref.phantom()
    out, B, g, report = ref.phantom_fit()
    before, after = BS.cv(volume, labels, 1), BS.cv(out, labels, 1)
    before2, after2 = BS.cv(volume, labels, 2), BS.cv(out, labels, 2)
    sel = (labels == 1) | (labels == 2)
    corr = float(np.corrcoef(fitted_gain(B, g, volume.shape)[sel], gain[sel])[0, 1])
    print("class 1: cv %.4f -> %.4f, a factor of %.2f; class 2: %.4f -> %.4f; correlation %.4f; rows %s" % (
        before, after, before / after, before2, after2, corr, [(r["g"], r["sweeps"], round(r["rms"], 4)) for r in BS.summary(report)]))
    assert g == 8 and volume.shape == (36, 40, 48) and 0.76 < gain.min() < 0.78 and 1.29 < gain.max() < 1.31
    assert abs(before - 0.0734) < 5e-4 and after < before / (2.44 * 0.75)
    assert after2 < before2 and corr > 1 - (1 - 0.9987) * 1.25
    rows = BS.summary(report)
    assert len(rows) == 6 and rows[-1]["rms"] < rows[0]["rms"] and all(r["count"] > 0 for r in rows)


def test_a_class_that_is_not_listed_is_left_out_of_every_sum():
    volume, labels, gain = ref.phantom()
    out, B, g, report = ref.phantom_fit((1,))
    n1 = int(((labels == 1) & (ref.logcode_ref(volume) != ref.NONE)).sum())
    assert (report[:6, 5] <= n1).all() and (report[:6, 5] > 0.9 * n1).all()     # the count of the cost: class 1 within the clip, nothing else
    # class 2's intensities do not matter at all: garbage there gives the same field
    spoiled = np.array(volume)
    spoiled[labels == 2] = np.random.default_rng(1).uniform(1, 1000, int((labels == 2).sum())).astype(F)
    spoiled[labels == 0] = 0
    B2, report2 = ref.fit_ref(ref.logcode_ref(spoiled), labels, [1])
    assert B2.tobytes() == B.tobytes() and report2.tobytes() == report.tobytes()
    lev = ref.levels_ref(ref.logcode_ref(volume), labels, [1], ref.zero_field(volume.shape, 32), 32)
    assert lev[0, 1] == n1 and (lev[1:] == [ref.NONE, 0, 0]).all()
    r = ref.residual_ref(ref.logcode_ref(volume), labels, [1], lev, 2048)
    assert (r[labels != 1] == ref.SKIP).all() and (r[labels == 1] != ref.SKIP).mean() > 0.9
    before, after = BS.cv(volume, labels, 1), BS.cv(out, labels, 1)
    print("class 1 alone: cv %.4f -> %.4f" % (before, after))
    assert after < before / (2.44 * 0.75)
