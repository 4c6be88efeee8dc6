"""The shapes of the conv / conv_trans op tests, grouped by the kernel family each group is there for.

A section names the element type and the directions its comment is about and the family (the enumerator names of
unet-studio_amd/csrc/conv_select.h) that direction must reach with IMPL_AUTO; `other` lists the cases of a section that by design
land elsewhere.  The flat lists the op tests are parametrised over are the sections in order.  tests/test_gpu_conv_exact.py checks
the claims against the engine (unet_op_conv_choice; unet_op_conv_choice2 for the sections with two sources)."""
from collections import namedtuple

# enumerators of conv_select.h, in order (tests/test_conv_exact_host.py holds them against the header)
FWD = ("deep", "mfma", "head", "first_mfma", "first_f32_mfma", "f32_mfma", "direct")
DGRAD = ("mfma", "f32_mfma", "direct")
WGRAD = ("first_mfma", "mfma", "f32_mfma", "small", "direct")
FAMILIES = {"fwd": FWD, "dgrad": DGRAD, "wgrad": WGRAD}

# expect: {direction: family} for every case of the section (dt: the element type the claim is about; None: the section claims nothing)
# other: {case: {direction: family}} -- the cases that the section's comment (or the selection's own rule) sends elsewhere
Section = namedtuple("Section", "name dt expect cases other")


def _s(name, dt, expect, cases, other=None):
    return Section(name, dt, expect, tuple(cases), other or {})


CONV_SECTIONS = [  # cases: cin, cout, (D,H,W), ks, stride
    _s("general", None, {}, [
        (1, 16, (9, 10, 12), 3, 1), (16, 16, (8, 8, 16), 3, 1), (5, 7, (6, 7, 9), 3, 1), (16, 32, (8, 10, 12), 3, 2),
        (3, 4, (7, 9, 11), 3, 2), (16, 6, (5, 6, 7), 1, 1), (32, 16, (4, 8, 16), 3, 1), (24, 40, (5, 5, 6), 3, 1)]),
    # MFMA-eligible shapes: every tile configuration (W >= 12, 5..11, <= 4), both channel-chunk widths, NT 1/2/4, ragged edges
    _s("MFMA-eligible shapes", "bf16", {"fwd": "mfma", "dgrad": "mfma", "wgrad": "mfma"}, [
        (32, 32, (9, 7, 20), 3, 1), (64, 64, (6, 9, 8), 3, 1), (48, 16, (5, 6, 4), 3, 1), (16, 48, (12, 12, 13), 3, 1),
        (128, 64, (4, 4, 4), 3, 1), (16, 16, (3, 5, 7), 3, 1), (32, 16, (16, 16, 32), 3, 1)],
       # 64 output voxels with Cin % 32 == 0: the selection offers the forward to the deep levels' split-K kernel first
       {(128, 64, (4, 4, 4), 3, 1): {"fwd": "deep"}}),
    # stride-2 MFMA wgrad: every tile configuration (Wo >= 12, 5..11, <= 4), PJ 1/2/4, odd input sizes
    _s("stride-2 MFMA wgrad", "bf16", {"wgrad": "mfma"}, [
        (16, 32, (12, 16, 32), 3, 2), (32, 64, (9, 11, 13), 3, 2), (64, 16, (8, 8, 8), 3, 2), (16, 16, (5, 7, 25), 3, 2)]),
    # output-stationary wgrad that adds straight into the gradient (tile side 4^3 / 8^3: no slab, no reduce): stride 2 with an 8^3
    # output from an even and from an odd input (4 tiles along z per block), stride 1 at 8^3 with several (ca, cb) pairs
    _s("output-stationary wgrad", "bf16", {"wgrad": "mfma"}, [
        (32, 32, (16, 16, 16), 3, 2), (16, 32, (15, 15, 15), 3, 2), (48, 32, (8, 8, 8), 3, 1)]),
    # stride-2 forward with 32-channel chunks (outputs of 8^3 voxels or fewer): eight and four chunks, both tiles, several row tiles
    _s("stride-2 forward with 32-channel chunks", "bf16", {"fwd": "mfma"}, [
        (256, 64, (8, 8, 8), 3, 2), (128, 48, (16, 16, 16), 3, 2), (96, 32, (13, 12, 15), 3, 2)],
       # a 4^3 output: offered to the split-K kernel first
       {(256, 64, (8, 8, 8), 3, 2): {"fwd": "deep"}}),
    # register-accumulating small wgrads: first conv (Cin = 1; W % 4 != 0 falls back to the row kernel) and 1x1x1 heads
    # (fp32 engine: in bf16 the first convs of 16 / 32 channels take the first-conv MFMA wgrad.  The row kernel is one of the small
    # kernels: the W % 4 != 0 case is listed under `other` with the same family, the step inside the launcher is not visible)
    _s("register-accumulating small wgrads", "fp32", {"wgrad": "small"}, [
        (1, 8, (6, 5, 8), 3, 1), (1, 16, (5, 6, 7), 3, 1), (1, 32, (17, 9, 16), 3, 1), (64, 6, (4, 5, 6), 1, 1), (256, 6, (3, 4, 5), 1, 1),
        (32, 3, (5, 6, 7), 1, 1), (16, 8, (33, 8, 9), 1, 1)],
       {(1, 16, (5, 6, 7), 3, 1): {"wgrad": "small"}}),
    # small-volume MFMA kernel: 8 chunks (two per wave, fragment refill), 16 chunks (two super-stages), 4^3 tile
    _s("small-volume MFMA kernel", "bf16", {"fwd": "mfma"}, [
        (256, 16, (8, 8, 8), 3, 1), (512, 32, (5, 6, 7), 3, 1), (256, 32, (4, 4, 4), 3, 1), (96, 32, (3, 4, 10), 3, 1)],
       # exactly 64 voxels: offered to the split-K kernel first
       {(256, 32, (4, 4, 4), 3, 1): {"fwd": "deep"}}),
    # sliding-window MFMA wgrad (bf16, stride 1, W >= 24): every (ca-tiles, cb-tiles) pairing 1x1 / 2x1 / 1x2 / 2x2, several pair
    # groups per launch, ragged footprints in y and x, z segments of unequal length, volumes narrower than one 32-voxel row
    _s("sliding-window MFMA wgrad", "bf16", {"wgrad": "mfma"}, [
        (16, 16, (9, 11, 37), 3, 1), (32, 16, (13, 9, 33), 3, 1), (16, 32, (5, 12, 40), 3, 1), (32, 32, (6, 9, 40), 3, 1),
        (64, 32, (8, 8, 24), 3, 1), (48, 16, (4, 10, 70), 3, 1), (16, 16, (40, 8, 32), 3, 1), (32, 64, (11, 5, 29), 3, 1)]),
    # ... above 32^3 voxels (at or below, the kernel uses single pairs): the 2x2, 2x1 and 1x2 pair blocks
    _s("sliding-window MFMA wgrad above 32^3 voxels", "bf16", {"wgrad": "mfma"}, [
        (32, 32, (20, 40, 48), 3, 1), (32, 16, (24, 30, 48), 3, 1), (16, 32, (18, 40, 48), 3, 1)]),
    # sliding window for a single 16-channel chunk (bf16; forward Cin = 16, dgrad Cout = 16; W >= 12, D >= 8): one and two row tiles,
    # ragged footprints, z segments of unequal length
    _s("sliding window for a single 16-channel chunk", "bf16", {"fwd": "mfma", "dgrad": "mfma"}, [
        (16, 16, (11, 9, 19), 3, 1), (16, 32, (10, 17, 33), 3, 1), (32, 16, (9, 10, 18), 3, 1), (16, 16, (37, 8, 16), 3, 1)]),
    # stride-2 sliding-window kernels (kernels_mfma_s2.hip; bf16, output >= 16 wide, >= 4 deep): forward with 16- and 32-channel planes and
    # 1 / 2 / 4 row tiles per block, dgrad with 32 and 64 dy channels and 1..3 row-tile blocks, odd input sizes (last fine plane / row /
    # voxel without a partner), ragged footprints, z segments of unequal length; Cin 48 / Cout 16 fall back to the halo-tile kernel
    # (Cin 48: a step inside the MFMA forward's launcher, same family.  Cout 16, and Cout 48 likewise: the stride-2 MFMA dgrad needs
    # Cout % 32 == 0 -- the comment's 32 and 64 dy channels -- so those two dgrads run on the direct kernel)
    _s("stride-2 sliding-window kernels", "bf16", {"fwd": "mfma", "dgrad": "mfma"}, [
        (16, 32, (16, 20, 40), 3, 2), (32, 64, (9, 13, 35), 3, 2), (16, 16, (8, 8, 32), 3, 2), (32, 48, (11, 10, 33), 3, 2),
        (16, 64, (12, 9, 38), 3, 2), (48, 32, (8, 12, 32), 3, 2), (32, 32, (37, 7, 31), 3, 2)],
       {(48, 32, (8, 12, 32), 3, 2): {"fwd": "mfma"}, (16, 16, (8, 8, 32), 3, 2): {"fwd": "mfma", "dgrad": "direct"},
        (32, 48, (11, 10, 33), 3, 2): {"dgrad": "direct"}}),
    # ... and their sliding-window weight gradient (kernels_mfma_s2_wgrad.hip; output >= 24 wide): (ca, cb) pairings 1x2 / 2x2 / 2x1, several
    # pair groups, ragged 32-voxel K-steps, odd input sizes, z segments of unequal length
    _s("stride-2 sliding-window wgrad", "bf16", {"wgrad": "mfma"}, [
        (16, 32, (9, 12, 64), 3, 2), (32, 32, (12, 9, 50), 3, 2), (32, 16, (8, 8, 48), 3, 2), (16, 64, (21, 7, 70), 3, 2)]),
    # split-K kernels of the deep levels (kernels_mfma_deep.hip; bf16, Cin % 32 == 0): 27-tap kinds at <= 64 output voxels (ragged
    # last 64-voxel group, one- and two-voxel extents, K splits of 8..32, one and two row tiles per block), stride 2 from odd extents,
    # and their dgrads (stride-2 dgrad up to a 512-voxel coarse grid)
    _s("split-K deep", "bf16", {"fwd": "deep", "dgrad": "mfma"}, [
        (64, 48, (3, 4, 5), 3, 1), (128, 32, (2, 2, 2), 3, 1), (512, 64, (1, 2, 3), 3, 1), (32, 128, (4, 4, 3), 3, 1),
        (32, 64, (7, 6, 5), 3, 2), (128, 128, (8, 8, 8), 3, 2), (64, 32, (3, 2, 2), 3, 2), (32, 32, (13, 15, 16), 3, 2)],
       # the 448-voxel output is there for the stride-2 dgrad on a coarse grid of up to 512 voxels; its forward is the plain MFMA conv
       {(32, 32, (13, 15, 16), 3, 2): {"fwd": "mfma"}}),
    # fp32 matrix-core conv (fp32 engine, volumes >= 4096 voxels): NT 1 / 2, ragged tile edges in z, y and x, 8-channel chunk tail
    _s("fp32 matrix-core conv", "fp32", {"fwd": "f32_mfma"}, [
        (16, 16, (16, 16, 32), 3, 1), (32, 64, (17, 19, 21), 3, 1), (24, 48, (9, 23, 22), 3, 1), (64, 32, (18, 17, 16), 3, 1)]),
]

CONVT_SECTIONS = [  # cases: cin, cout, (D,H,W) of the coarse grid
    _s("general", None, {}, [(16, 16, (4, 5, 6)), (7, 3, (3, 4, 5)), (32, 16, (4, 4, 8))]),
    # MFMA conv_trans (Cin % 32 == 0): every tile configuration, ragged edges
    _s("MFMA conv_trans", "bf16", {"fwd": "mfma", "dgrad": "mfma", "wgrad": "mfma"}, [
        (64, 32, (3, 5, 19)), (32, 32, (4, 4, 4)), (128, 64, (2, 3, 2)), (32, 48, (5, 9, 7))]),
    # output-stationary conv_trans wgrad (coarse side 4^3 above, 8^3 here: 4 tiles along z per block)
    _s("output-stationary conv_trans wgrad", "bf16", {"wgrad": "mfma"}, [(32, 48, (8, 8, 8))]),
    # conv_trans dgrad with 32-channel chunks (Cout % 32 == 0 on coarse grids of 8^3 or less): both tiles
    _s("conv_trans dgrad with 32-channel chunks", "bf16", {"dgrad": "mfma"}, [
        (64, 64, (5, 6, 7)), (32, 96, (8, 8, 8)), (256, 256, (4, 4, 4))]),
    # split-K kernels of the deep levels (coarse grids of <= 512 voxels, Cin % 32 == 0): ragged groups, one-voxel extents
    # (conv_trans has no enumerator of its own for them: the MFMA family, whose launcher tries the split-K kernel first)
    _s("split-K deep conv_trans", "bf16", {"fwd": "mfma", "dgrad": "mfma"}, [
        (64, 32, (3, 3, 5)), (32, 16, (1, 2, 3)), (256, 128, (2, 2, 2)), (96, 64, (7, 8, 8))]),
    # sliding-window conv_trans kernels (kernels_mfma_s2.hip; coarse grid >= 16 wide, >= 4 deep): forward with 1 / 2 / 4
    # k-steps and 1..4 row-tile blocks, dgrad with 16- and 32-channel planes and 2 / 4 row tiles per block, ragged edges
    _s("sliding-window conv_trans kernels", "bf16", {"fwd": "mfma", "dgrad": "mfma"}, [
        (32, 16, (4, 6, 16)), (64, 32, (5, 9, 19)), (128, 64, (4, 4, 16)), (32, 48, (6, 7, 17)), (64, 16, (7, 5, 20)),
        (32, 32, (9, 4, 18))]),
    # ... and their sliding-window weight gradient (coarse grid >= 24 wide): pairings 1x2 / 2x2, several pair groups, ragged
    _s("sliding-window conv_trans wgrad", "bf16", {"wgrad": "mfma"}, [
        (32, 16, (4, 5, 24)), (64, 32, (5, 3, 33)), (32, 32, (4, 4, 26)), (32, 48, (9, 6, 25))]),
]

# ---- layers with two sources (the decoder's convs read cat(skip, x) without materialising it) and their split destinations ----
# cases: c0, c1, cout, (D,H,W), ks, stride.  The oracle computes the conv of c0 + c1 channels; the test splits its tensors.  The
# claims are checked with both sources given (unet_op_conv_choice2); what a family's launcher decides by itself was read off the
# launcher named in the comment.
CONV2_SECTIONS = [
    # sliding window, bf16 (W >= 12, D >= 8).  Forward: Cin 32 in all -> k_mfma_conv_z32 (launch_conv_z32: g.Cin == 32, sources % 8) with
    # the source boundary in the middle of its one 32-channel chunk; Cin 48 -> the halo tile with 16-channel chunks.  Dgrad (GEMM view: Cin
    # = the forward's Cout): Cout 16 -> k_mfma_conv_z16 writing 16 + 16 (conv_z16_blocks: view Cout 32, outC[0] % 16), Cout 32 ->
    # k_mfma_conv_z32 writing 16 + 16 and 16 + 32
    _s("two sources, sliding window", "bf16", {"fwd": "mfma", "dgrad": "mfma", "wgrad": "mfma"}, [
        (16, 16, 16, (9, 9, 19), 3, 1), (16, 16, 32, (8, 10, 13), 3, 1), (16, 32, 32, (8, 9, 20), 3, 1)]),
    # halo tile and small volumes, bf16 (launch_s1k3): Cin 48 -> k_mfma_conv_p with 16-channel chunks; Cin 64 in volumes of few tiles
    # (small_s1k3) -> k_mfma_conv_small with the boundary inside a 32-channel chunk (16 | 48 in chunk 0, 48 | 16 in chunk 1); Cin 256 ->
    # its 8-wave form (nchunk >= 8), boundary at chunk 4.5, and with Cin 512 in two super-stages, boundary at chunk 7.5; Cin 64 -> 64 on 64 tiles of 4x4x16 (x 4 row tiles = 256: not small) ->
    # k_mfma_conv_p with 32-channel chunks in the default configuration.  Their dgrads: the same kernels writing two destinations
    _s("two sources, halo tile and small volumes", "bf16", {"fwd": "mfma", "dgrad": "mfma", "wgrad": "mfma"}, [
        (16, 32, 16, (5, 6, 9), 3, 1), (16, 48, 32, (5, 6, 7), 3, 1), (48, 16, 16, (6, 9, 8), 3, 1), (144, 112, 16, (4, 5, 6), 3, 1),
        (240, 272, 32, (5, 6, 7), 3, 1), (16, 48, 64, (14, 29, 17), 3, 1)]),
    # stride 2, bf16: Cin 32 on a coarse grid >= 16 wide and >= 4 deep -> k_s2_gather with two sources (launch_s2_conv_fwd), at the smallest
    # grid it serves and from odd extents; Cin 48 -> the halo tile.  Dgrad: k_s2_scatter takes ONE destination of every channel
    # (s2_dgrad_plan: ndst == 1) -- the test also runs the dgrad into one destination of c0 + c1 channels, written and accumulated -- and
    # two destinations run on the k_mfma_conv_p scatter kind (launch_k2sc); on coarse grids of <= 512 voxels (the first and the last case)
    # mfma_dgrad offers both forms to the split-K scatter kind first, and they reach the kernels named under UNET_NO_DEEP_KERNELS
    _s("two sources, stride 2", "bf16", {"fwd": "mfma", "dgrad": "mfma", "wgrad": "mfma"}, [
        (16, 16, 32, (8, 8, 32), 3, 2), (16, 16, 32, (9, 13, 35), 3, 2), (16, 32, 32, (9, 7, 11), 3, 2)]),
    # deep levels, bf16 (<= 64 output voxels, Cin % 32 == 0).  The split-K forward takes sources of 32-channel granularity only
    # (deep_src_ok): 32 + 32 runs on it, the 16-granular splits fall to k_mfma_conv_small (the selection still says deep: its launcher
    # declines).  The split-K dgrad (deep_dgrad_view: Cout % 32, Cin % 16) writes / accumulates both 16-granular destinations (deep_store)
    _s("two sources, deep levels", "bf16", {"fwd": "deep", "dgrad": "mfma", "wgrad": "mfma"}, [
        (16, 48, 32, (3, 4, 4), 3, 1), (48, 16, 64, (2, 3, 3), 3, 1), (32, 32, 32, (3, 4, 4), 3, 1)]),
    # weight gradients over two sources, bf16: sliding window (wgrad_z_cfg: W >= 24, D >= 4; <= 32^3 voxels single pairs on
    # k_mfma_wgrad_zd); above 32^3 voxels the 2x1 pair block of decode0.0 (16 + 16 -> 16: k_mfma_wgrad_z<32,4,2,1>, launched politely
    # k_mfma_wgrad_zd<2,2,1>); the slab form of k_mfma_wgrad (W < 24, not a cube); output-stationary at 8^3 and 4^3 (wgrad_direct_cfg);
    # stride 2 on a coarse grid 32 wide -> k_s2_wgrad with its second fine source
    _s("two sources, weight gradients", "bf16", {"wgrad": "mfma"}, [
        (16, 16, 16, (8, 9, 33), 3, 1), (16, 32, 32, (5, 12, 40), 3, 1), (16, 16, 16, (20, 40, 48), 3, 1), (16, 32, 16, (6, 9, 8), 3, 1),
        (16, 32, 32, (8, 8, 8), 3, 1), (32, 96, 32, (4, 4, 4), 3, 1), (16, 16, 32, (9, 12, 64), 3, 2)]),
    # fp32 engine: the matrix-core forward takes sources of 8-channel granularity (k_conv_f32_mfma) ...
    _s("two sources, fp32 matrix-core forward", "fp32", {"fwd": "f32_mfma"}, [
        (8, 24, 16, (16, 16, 16), 3, 1), (24, 8, 32, (9, 23, 22), 3, 1)]),
    # ... its dgrad and wgrad (k_wgrad_f32_mfma) need 16
    _s("two sources, fp32 matrix-core dgrad and wgrad", "fp32", {"fwd": "f32_mfma", "dgrad": "f32_mfma", "wgrad": "f32_mfma"}, [
        (16, 16, 16, (16, 16, 16), 3, 1), (16, 32, 16, (9, 17, 16), 3, 1)]),
    # direct kernels: channel counts no matrix-core kernel takes (and IMPL_DIRECT runs every case of this list on them)
    _s("two sources, direct kernels", None, {}, [(5, 3, 7, (4, 5, 6), 3, 1), (3, 4, 4, (7, 9, 11), 3, 2)]),
]

# conv_trans dgrad ADDED to an older gradient, one case per family of CONVT_SECTIONS: the halo tile with 16-channel chunks (D < 4 keeps
# the sliding window out), with 32-channel chunks (coarse grid 7 wide, 630 voxels: above the split-K kernel's 512), the split-K kernel,
# and a shape of the sliding-window kernel, which declines an accumulating destination (launch_s2_convt_dgrad) and leaves it to the halo tile
CONVT_ACC_CASES = [(64, 32, (3, 5, 19)), (32, 64, (9, 10, 7)), (64, 32, (3, 3, 5)), (32, 16, (4, 6, 16))]

CONV_CASES = [c for s in CONV_SECTIONS for c in s.cases]
CONVT_CASES = [c for s in CONVT_SECTIONS for c in s.cases]
CONV2_CASES = [c for s in CONV2_SECTIONS for c in s.cases]

# (cin, cout, (D,H,W)): plain bf16 input with the statistics epilogue
PLAIN_STATS_CASES = [(1, 16, (9, 13, 21)), (1, 32, (4, 8, 16)), (32, 16, (6, 9, 20)), (16, 16, (5, 8, 17)),
                     (16, 16, (9, 13, 21)), (16, 32, (12, 9, 20)), (16, 16, (33, 8, 16))]
PACKED_CASE = (32, 16, (6, 9, 20))
# (cin, cout, (D,H,W), ks, stride, act): norm + activation applied on read, statistics of the stored output
FUSED_CASES = [(16, 16, (6, 9, 20), 3, 1, 2), (32, 32, (8, 8, 8), 3, 2, 3), (16, 32, (5, 6, 4), 3, 1, 1), (5, 7, (4, 5, 6), 3, 1, 2)]

# heads (conv k1 s1 writing a network result; k_head_fwd / k_head_bwd): every CO template (2, 4, 6, 8) and a Cout below its template;
# every chunk count (Cin / 16 = 1, 2, 8, 16); voxel counts around the 64-voxel rounding of the forward's items and one whose tail ends
# inside a block (16 * 17 * 9 + 1)
HEAD_CIN = (16, 32, 128, 256)
HEAD_COUT = (1, 2, 3, 6, 8)
HEAD_VOXELS = (1, 63, 64, 65, 16 * 17 * 9 + 1)
# At those sizes every thread of either kernel runs its grid-stride loop ONCE: launch_head_bwd has one (voxel, chunk) item per thread
# until 512 blocks (S * Cin / 16 > 131072), launch_head_fwd until 2048 blocks (S * Cin / 16 > 524288).  (cin, cout, S) past both caps,
# where a thread walks several voxels -- the backward's prefetch of the next voxel, its carry and the sum of acc[] over voxels, the
# forward's strided further passes -- with a ragged tail (S no multiple of the voxel stride, nor of 64):
#   256 -> 6 on 40001 voxels: backward stride 512 * 256 / 16 = 8192 voxels, 4 or 5 voxels per thread; forward stride 32768, 1 or 2;
#   128 -> 3 on 70001 voxels: backward stride 16384, 4 or 5 voxels per thread; forward stride 65536, 1 or 2 (Cout below its template);
#   16 -> 1 on 530001 voxels: one chunk, a thread per voxel; backward stride 131072, 4 or 5 voxels per thread; forward stride 524288, 1 or 2
HEAD_CAP_CASES = ((256, 6, 40001), (128, 3, 70001), (16, 1, 530001))
# a head whose source is plain (no scale / shift, no activation: how a plan reads a head behind an activated copy), the other branch of
# load_chunk16; (cin, cout, S), one chunk and sixteen
HEAD_PLAIN_CASES = ((16, 3, 321), (256, 8, 65))
