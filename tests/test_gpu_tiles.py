"""GPU: a scan larger than the model's field of view in blended tiles (include/unet_tiles.h, unet-studio_amd/tiles.py).

unet_tiles_blend against a float64 numpy restatement of the header's BLEND: a voxel one tile covers must carry that tile's bits;
every other voxel lies within 32 * 2^-24 * max|x_t| of the restatement -- at most 27 exact-weight products, 26 additions in each of
the two sums and one division, each within 2^-24 relative, on terms no larger than w_t * max|x_t| against a denominator sum w_t.
Special values follow the restatement's IEEE arithmetic.  unet_tiles_postproc equals blend + unet_postproc_softmax bit for bit.
EvaluateUNet(fov_strategy="tiles") equals the sequence composed by hand from the public pieces, bit for bit, for plain arrays and
NativeVolumes; a volume that fits takes today's path; and the voxels today's path leaves outside its crop are now evaluated."""
import numpy as np
import pytest
import torch

import unet_studio_amd as U
from unet_studio_amd import postproc as P
from unet_studio_amd import preproc as PRE
from unet_studio_amd import space as SP
from unet_studio_amd import tiles as TL

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F = np.float32
TILE = (8, 6, 5)                 # (tw, th, td): no multiple of the 16 x 4 x 4 brick on any axis
TOL = 32 * 2.0 ** -24

SMOKE_ARCH = ("conv8,ks3,stride1+norm,leaky_relu+conv8,ks3,stride1+norm,leaky_relu\n"
              "conv16,ks3,stride2+norm,leaky_relu+conv16,ks3,stride1+norm,leaky_relu+conv_trans8,ks2,stride2\n"
              "conv8,ks3,stride1+norm,leaky_relu+conv8,ks3,stride1+norm,leaky_relu+conv%d,ks1,stride1")

# (x origins, y origins, z origins) from plan_axis with the canvas size and overlap of each axis: 1, 2 and 3 covering tiles mixed
AXES = {"x": {1: (8, .25), 2: (13, .25), 3: (15, .25), "2b": (17, 0)},        # [0] [0,5] [0,4,7] [0,5,9]
        "y": {1: (6, .25), 2: (9, .25), 3: (11, .25), "2b": (11, 0)},         # [0] [0,3] [0,3,5] [0,5]
        "z": {1: (5, .25), 2: (8, .25), 3: (9, .25), "2b": (8, 0)}}           # [0] [0,3] [0,2,4] [0,3]
CASES = [(1, 3, 3), (2, 1, 3), (3, 3, 1), (3, 2, 2), ("2b", "2b", "2b"), (1, 1, 1), (3, 3, 3), (2, 3, "2b")]


def case_plan(k):
    spec = [AXES[a][c] for a, c in zip("xyz", CASES[k])]
    plan = tuple(TL.plan_axis(C, T, ov) for (C, ov), T in zip(spec, TILE))
    canvas = tuple(C for C, _ in spec)                  # (cw, ch, cd)
    return plan, canvas


def test_the_cases_give_the_covers_they_are_named_for():
    for k, names in enumerate(CASES):
        plan, canvas = case_plan(k)
        for a in range(3):
            cover = np.zeros(canvas[a], int)
            for o in plan[a]:
                cover[o:o + TILE[a]] += 1
            want = 2 if names[a] == "2b" else names[a]
            assert cover.min() == 1 and cover.max() == want, (k, a, plan[a])


# ---- the restatement -------------------------------------------------------------------------------------------------------------
def ref_blend(stack, plan, canvas):
    """include/unet_tiles.h BLEND in float64: (value {C, cd, ch, cw}, cover count {cd, ch, cw}, the value of the last covering tile
    float32 {C, ...}, max |finite x_t| {C, ...})"""
    tw, th, td = TILE
    cw, ch, cd = canvas
    C = stack.shape[1]
    num, den = np.zeros((C, cd, ch, cw)), np.zeros((cd, ch, cw))
    cnt = np.zeros((cd, ch, cw), int)
    one, mx = np.zeros((C, cd, ch, cw), F), np.zeros((C, cd, ch, cw))
    w3 = (TL.weights(td).astype(np.float64)[:, None, None] * TL.weights(th).astype(np.float64)[None, :, None]
          * TL.weights(tw).astype(np.float64)[None, None, :])
    with np.errstate(invalid="ignore"):
        for t, (ox, oy, oz) in enumerate(TL.tile_origins(plan)):              # ascending tile index
            sl = (slice(oz, oz + td), slice(oy, oy + th), slice(ox, ox + tw))
            x = stack[t].astype(np.float64)
            num[(slice(None),) + sl] += w3 * x
            den[sl] += w3
            cnt[sl] += 1
            one[(slice(None),) + sl] = stack[t]
            mx[(slice(None),) + sl] = np.maximum(mx[(slice(None),) + sl], np.where(np.isfinite(x), np.abs(x), 0))
        val = num / den
    return val, cnt, one, mx


def make_stack(plan, C, seed, special=False):
    n = len(TL.tile_origins(plan))
    tw, th, td = TILE
    st = (np.random.RandomState(seed).randn(n, C, td, th, tw) * 3).astype(F)
    if special:                         # planted at fixed tile-local places: corners are single-cover, the far faces multi-cover
        inf = float("inf")
        st[0, 0, 0, 0, 0] = np.nan
        st[0, 1, 0, 0, 1] = inf
        st[0, C - 1, 0, 1, 0] = -inf
        st[n - 1, 0, td - 1, th - 1, tw - 1] = -inf
        st[0, 0, td - 1, th - 1, tw - 1] = inf              # in the overlap with the next tiles when there are any
        st[0, 1, td - 1, th - 1, tw - 2] = np.nan
        st[0, C - 1, td - 1, th - 2, tw - 1] = -inf
        if n > 1:
            st[1, C - 1, 0, 0, 0] = inf
            st[1, 0, td - 1, th - 1, 0] = -inf
            st[n - 1, 1, 0, 0, 0] = inf                     # +inf against a possible -inf of another tile: NaN
            st[n - 2, 1, 0, 0, 1] = -inf
    return st


def guarded(shape, guard=4099, dtype=torch.float32):
    """a buffer of 7s with `guard` elements on either side of the view that is handed out"""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * guard,), 7, dtype=dtype, device=DEV)
    return buf, buf[guard:guard + n].view(shape)


def guards_untouched(buf, shape, guard=4099):
    n = int(np.prod(shape))
    b = buf.cpu().to(torch.float32)
    return bool((b[:guard] == 7).all()) and bool((b[guard + n:] == 7).all())


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def check_blend(k, C, special):
    plan, canvas = case_plan(k)
    cshape = canvas[::-1]
    st = make_stack(plan, C, 10 * k + C, special)
    val, cnt, one, mx = ref_blend(st, plan, canvas)
    dst = torch.from_numpy(st).to(DEV)
    keep = dst.clone()
    buf, out = guarded((C,) + cshape)
    got_t = TL.blend(dst, plan, cshape, out=out)
    torch.cuda.synchronize()
    assert got_t.data_ptr() == out.data_ptr() and guards_untouched(buf, (C,) + cshape)
    assert torch.equal(dst.view(torch.int32), keep.view(torch.int32))            # the stack is only read
    got = got_t.cpu().numpy()
    again = TL.blend(dst, plan, cshape).cpu().numpy()
    assert np.array_equal(bits(got), bits(again))                                # twice the same bits
    single = np.broadcast_to(cnt == 1, got.shape)
    assert np.array_equal(bits(got)[single], bits(one)[single])                  # one tile: copied bit for bit (NaN payloads too)
    multi = ~single
    fin = np.isfinite(val)
    assert np.array_equal(np.isnan(got)[multi], np.isnan(val)[multi]) and np.array_equal(np.isinf(got)[multi], np.isinf(val)[multi])
    assert np.array_equal(got[multi & np.isinf(val)], val[multi & np.isinf(val)].astype(F))      # the same signed infinity
    sel = multi & fin
    with np.errstate(invalid="ignore"):
        err = np.abs(got.astype(np.float64) - val)[sel]
    bound = (TOL * mx)[sel]
    if sel.any():
        print("case %d %s C=%d%s: covers up to %d, %d blended values, max err / bound = %.3g" % (
            k, CASES[k], C, " special" if special else "", cnt.max(), int(sel.sum()), float((err / np.maximum(bound, 1e-300)).max())))
        assert (err <= bound).all()
    if special:
        assert np.isnan(got).any() and np.isinf(got).any()
        # the finite voxels are the ones no planted value reaches
        clean = ref_blend(np.where(np.isfinite(st), st, 0).astype(F), plan, canvas)[0]
        untouched = fin & (clean == val)
        assert untouched.sum() > 0.5 * val.size
    return cnt


# ---- 1, 2: the blend ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [2, 3])
@pytest.mark.parametrize("k", range(len(CASES)))
def test_blend_against_the_restatement(k, C):
    cnt = check_blend(k, C, False)
    names = [2 if c == "2b" else c for c in CASES[k]]
    assert cnt.max() == names[0] * names[1] * names[2]


@pytest.mark.parametrize("k", [0, 3, 4, 5, 6])
def test_blend_special_values(k):
    check_blend(k, 3, True)


# ---- 3: the fused pass ---------------------------------------------------------------------------------------------------------------
def run_fused(dst, plan, cshape, thr=0.5, want=TL.OUTPUTS):
    C = dst.shape[1]
    bufs = {"label_prob": guarded((C - 1,) + cshape), "fg_prob": guarded(cshape), "label": guarded(cshape, dtype=torch.uint16)}
    res = TL.postproc_tiles(dst, plan, cshape, thr, want, out={n: bufs[n][1] for n in want})
    torch.cuda.synchronize()
    assert sorted(res) == sorted(want)
    for n, shape in (("label_prob", (C - 1,) + cshape), ("fg_prob", cshape), ("label", cshape)):
        assert guards_untouched(bufs[n][0], shape), n
    return {n: bufs[n][1] for n in TL.OUTPUTS}


def run_unfused(dst, plan, cshape, thr=0.5):
    C = dst.shape[1]
    S = int(np.prod(cshape))
    canvas = TL.blend(dst, plan, cshape)
    lp = torch.empty((C - 1,) + cshape, device=DEV)
    fg = torch.empty(cshape, device=DEV)
    lab = torch.empty(cshape, dtype=torch.uint16, device=DEV)
    P.softmax_call(canvas, C, S, thr, lp, fg, lab)
    torch.cuda.synchronize()
    return {"label_prob": lp, "fg_prob": fg, "label": lab}


def same_bits(a, b):
    v = torch.int16 if a.dtype == torch.uint16 else torch.int32
    return torch.equal(a.contiguous().view(v), b.contiguous().view(v))


@pytest.mark.parametrize("special", [False, True])
@pytest.mark.parametrize("k,C", [(6, 3), (3, 2), (4, 6), (5, 3)])
def test_fused_postproc_equals_blend_then_softmax(k, C, special):
    plan, canvas = case_plan(k)
    cshape = canvas[::-1]
    dst = torch.from_numpy(make_stack(plan, C, 70 + k, special)).to(DEV)
    exp = run_unfused(dst, plan, cshape)
    got = run_fused(dst, plan, cshape)
    for n in TL.OUTPUTS:
        assert same_bits(got[n], exp[n]), n
    if special:
        assert bool(torch.isnan(exp["fg_prob"]).any())


@pytest.mark.parametrize("mask", range(1, 8))
def test_fused_every_subset_of_outputs_and_untouched_ones(mask):
    want = tuple(n for i, n in enumerate(TL.OUTPUTS) if mask >> i & 1)
    plan, canvas = case_plan(3)
    cshape = canvas[::-1]
    dst = torch.from_numpy(make_stack(plan, 4, 5, True)).to(DEV)
    full = run_unfused(dst, plan, cshape)
    part = run_fused(dst, plan, cshape, want=want)
    for n in TL.OUTPUTS:
        if n in want:
            assert same_bits(part[n], full[n]), n
        else:
            assert bool((part[n].cpu().to(torch.float32) == 7).all()), n


def test_fused_threshold_is_used():
    plan, canvas = case_plan(6)
    cshape = canvas[::-1]
    dst = torch.from_numpy(make_stack(plan, 3, 8)).to(DEV)
    a = run_fused(dst, plan, cshape, thr=0.2, want=("fg_prob", "label"))
    b = run_fused(dst, plan, cshape, thr=0.9, want=("label",))
    fg = a["fg_prob"].cpu()
    la, lb = a["label"].cpu().to(torch.int32), b["label"].cpu().to(torch.int32)
    assert torch.equal(la != 0, fg > 0.2) and torch.equal(lb != 0, fg > 0.9) and not torch.equal(la, lb)


# ---- 4-7: EvaluateUNet ---------------------------------------------------------------------------------------------------------------
OUT_C = 3
OUTPUTS = ("label", "fg_prob", "label_prob")
CHAINS = [None, "model", "softmax+create_mask+argmax+defragment"]
BIG = (30, 18, 37)               # (d, h, w)


def small_model(dt="fp32", in_count=1):
    m = U.UNet3d(in_count, OUT_C, SMOKE_ARCH % OUT_C, device=DEV, dtype=dt, seed=2)
    m.dim, m.voxel_size = (16, 16, 16), (1.0, 1.0, 1.0)
    return m


def forward_tiles(m, xc, plan):
    """slice -> m.forward for every tile, in tile-index order: the stack {tiles, out_c, D, H, W}"""
    W, H, D = m.dim
    outs = []
    with torch.no_grad():
        for ox, oy, oz in TL.tile_origins(plan):
            crop = xc[:, oz:oz + D, oy:oy + H, ox:ox + W].contiguous().unsqueeze(0)
            outs.append(m.forward(crop)[0].view(m.out_count, D, H, W).clone())
    return torch.stack(outs).contiguous()


def host(res, outputs=OUTPUTS):
    torch.cuda.synchronize()
    return {k: res[k].cpu().view(torch.int16 if k == "label" else torch.float32).numpy() for k in outputs}


def check_against(g, exp, chain, shape):
    d, h, w = shape
    if chain is None:
        assert g.dtype == np.float32 and g.shape == (OUT_C * d, h, w) and g.tobytes() == exp.tobytes()
        return
    assert sorted(g) == sorted(OUTPUTS)
    assert g["label"].dtype == np.uint16 and g["label"].shape == (d, h, w) and g["fg_prob"].shape == (d, h, w)
    assert g["label_prob"].shape == ((OUT_C - 1) * d, h, w)
    for k in OUTPUTS:
        assert g[k].tobytes() == exp[k].tobytes(), k


def manual_array(m, io, chain):
    d, h, w = io.shape
    plan = TL.plan_tiles((w, h, d), m.dim, 0.25)
    stack = forward_tiles(m, torch.from_numpy(io).view(1, d, h, w).to(DEV), plan)
    logits = TL.blend(stack, plan, (d, h, w))
    if not chain:
        return logits.cpu().numpy().reshape(OUT_C * d, h, w)
    return host(P.run_postproc(logits, chain, outputs=OUTPUTS))


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("chain", CHAINS)
def test_a_plain_array_under_tiles_equals_the_manual_sequence(dt, chain):
    m = small_model(dt)
    assert TL.plan_tiles(BIG[::-1], m.dim, 0.25) == ([0, 11, 21], [0, 2], [0, 7, 14])          # 18 forwards
    io = np.random.RandomState(5).rand(*BIG).astype(F)
    keep = io.copy()
    ev = U.EvaluateUNet(m, postproc=chain, outputs=OUTPUTS, fov_strategy="tiles")
    got = ev.start([[io]])[0][0]
    assert not ev.aborted and ev.error_msg == "" and ev.cur_prog == 1
    check_against(got, manual_array(m, io, m.postproc if chain == "model" else chain), chain, BIG)
    assert np.array_equal(io, keep)
    m.fov_strategy = "tiles"                                 # "model" takes the model's field
    again = U.EvaluateUNet(m, postproc=chain, outputs=OUTPUTS, fov_strategy="model").start([[io]])[0][0]
    if chain is None:
        assert again.tobytes() == got.tobytes()
    else:
        assert all(again[k].tobytes() == got[k].tobytes() for k in OUTPUTS)


def test_one_tile_is_todays_path():
    m = small_model()
    m.fov_strategy = "tiles"                                 # ignored unless fov_strategy="model" asks for it
    rs = np.random.RandomState(9)
    fits = U.NativeVolume(rs.rand(14, 15, 16).astype(F), m.voxel_size)
    exact = rs.rand(16, 16, 16).astype(F)
    for chain in (None, "model"):
        a = U.EvaluateUNet(m, postproc=chain, outputs=OUTPUTS, fov_strategy=None)
        b = U.EvaluateUNet(m, postproc=chain, outputs=OUTPUTS, fov_strategy="tiles")
        ra, rb = a.start([[fits, exact]])[0], b.start([[fits, exact]])[0]
        assert not a.aborted and not b.aborted
        for x, y in zip(ra, rb):
            if chain is None:
                assert x.tobytes() == y.tobytes()
            else:
                assert all(x[k].tobytes() == y[k].tobytes() for k in OUTPUTS)


def manual_native(m, nv, chain, pre="", ori=""):
    """preproc -> ONE resample with normalize to the canvas -> crops -> forwards -> blend -> the way back, from the public pieces"""
    d, h, w = nv.data.shape
    native = (d, h, w)
    pre, ori = PRE.active(PRE.parse_chain(pre)), PRE.parse_orientation(ori)
    x = torch.from_numpy(nv.data).view(1, *native).to(DEV)
    pdims, pvs, G = PRE.geometry(pre, native[::-1], nv.voxel_size)
    if pre:
        x = PRE.run_preproc(x, pre)
    canvas = TL.canvas_dims(m.dim, m.voxel_size, pdims, pvs, orientation=ori)
    plan = TL.plan_tiles(canvas, m.dim, 0.25)
    fwd = SP.model_to_image_map(*(PRE.orientation_map(ori, canvas, m.voxel_size)[:2] if ori else (canvas, m.voxel_size)), pdims, pvs)
    if ori:
        fwd = SP.compose_map(fwd, PRE.orientation_map(ori, canvas, m.voxel_size)[2])
    back = SP.invert_map(SP.compose_map(G, fwd))
    xc = SP.resample(x, canvas[::-1], fwd, "linear", normalize=True)
    assert float(xc.max()) == 1.0                            # one normalisation over the whole scan
    logits = TL.blend(forward_tiles(m, xc, plan), plan, canvas[::-1])
    if not chain:
        return SP.resample(logits, native, back, "linear").cpu().numpy().reshape(OUT_C * d, h, w), canvas
    return host(P.run_postproc(logits, chain, outputs=OUTPUTS, native=(back, native))), canvas


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("chain", CHAINS)
def test_a_native_volume_larger_than_the_model_equals_the_manual_sequence(dt, chain):
    m = small_model(dt)
    data = np.random.RandomState(6).rand(*BIG).astype(F)
    keep = data.copy()
    nv = U.NativeVolume(data, (1.0, 1.1, 0.9))
    ev = U.EvaluateUNet(m, postproc=chain, outputs=OUTPUTS, fov_strategy="tiles")
    got = ev.start([[nv]])[0][0]
    assert not ev.aborted and ev.error_msg == ""
    exp, canvas = manual_native(m, nv, m.postproc if chain == "model" else chain)
    assert canvas == (37, 20, 27)
    check_against(got, exp, chain, BIG)
    assert nv.data is data and np.array_equal(data, keep)    # the caller's data is not written
    if chain == "model":
        # what the feature is for: voxels today's path leaves outside its crop (label 0, fg_prob exactly 0) are now evaluated
        old = U.EvaluateUNet(m, postproc=chain, outputs=OUTPUTS).start([[nv]])[0][0]
        outside = (old["fg_prob"] == 0) & (old["label"] == 0)
        assert outside.mean() > 0.5
        assert (got["fg_prob"][outside] > 0).any()
        # (the scan's first and last z-slice lie 0.05 voxel beyond the canvas's outermost voxel centres: background, as any
        # position outside the grid the logits live on)
        assert (got["fg_prob"][1:-1] > 0).all() and (got["fg_prob"] > 0).mean() > 0.9


def test_a_native_volume_with_preproc_and_orientation_under_tiles():
    m = small_model()
    nv = U.NativeVolume(np.random.RandomState(7).rand(*BIG).astype(F), (1.0, 1.1, 0.9))
    pre, ori = "gaussian_filter", "swap_xy+flip_z"
    for chain in (None, "model"):
        ev = U.EvaluateUNet(m, postproc=chain, outputs=OUTPUTS, preproc=pre, orientation=ori, fov_strategy="tiles")
        got = ev.start([[nv]])[0][0]
        assert not ev.aborted and ev.error_msg == ""
        exp, canvas = manual_native(m, nv, m.postproc if chain == "model" else chain, pre, ori)
        assert canvas == (20, 37, 27)                        # the extents, swapped into the model's frame
        check_against(got, exp, chain, BIG)


def test_errors_end_the_run():
    m = small_model()
    rs = np.random.RandomState(0)
    good = rs.rand(*BIG).astype(F)
    later = rs.rand(16, 16, 16).astype(F)
    ev = U.EvaluateUNet(m, fov_strategy="spiral")
    out = ev.start([[good], [later]])
    assert ev.aborted and ev.error_msg == "unknown fov_strategy spiral" and out[0][0] is good and out[1][0] is later
    ev = U.EvaluateUNet(m, fov_strategy="tiles", tile_overlap=0.5)
    out = ev.start([[good], [later]])
    assert ev.aborted and "tile_overlap" in ev.error_msg and out[0][0] is good and out[1][0] is later
    mapped = U.NativeVolume(good, (1, 1, 1), map=(np.eye(3).reshape(9), np.zeros(3)))
    ev = U.EvaluateUNet(m, fov_strategy="tiles")
    out = ev.start([[good], [mapped], [later]])
    assert ev.aborted and "a caller's map and tiles do not combine" in ev.error_msg and ev.cur_prog == 1
    assert out[1][0] is mapped and out[2][0] is later
    small = rs.rand(16, 15, 16).astype(F)
    ev = U.EvaluateUNet(m, fov_strategy="tiles")
    out = ev.start([[small], [later]])
    assert ev.aborted and "smaller than the model's" in ev.error_msg and ev.cur_prog == 0 and out[1][0] is later
