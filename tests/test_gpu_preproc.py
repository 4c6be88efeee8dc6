"""GPU: a model's pre-processing commands and orientation (include/unet_preproc.h, unet-studio_amd/preproc.py) against a numpy
restatement, bit for bit, and EvaluateUNet's preproc / orientation keywords.

The restatement of the commands is below; it shares the smoothing and the sampler with the augmentation's (oracle/augment_ref.py:
_smooth, _affine, _locate, _trilinear, _norm) and never calls the package.  Everything is compared bitwise: the kernels accumulate
in the restatement's order with contraction off, the cell counts of downsampling are powers of two, and the positions of
upsampling (x/2 - 1/4) and of the flips / swaps (integers) are exact in fp32."""
import threading

import numpy as np
import pytest
import torch

import unet_studio_amd as U
from unet_studio_amd import postproc as P
from unet_studio_amd import preproc as PRE
from unet_studio_amd import space as SP
from oracle import augment_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F = np.float32

SMOKE_ARCH = ("conv8,ks3,stride1+norm,leaky_relu+conv8,ks3,stride1+norm,leaky_relu\n"
              "conv16,ks3,stride2+norm,leaky_relu+conv16,ks3,stride1+norm,leaky_relu+conv_trans8,ks2,stride2\n"
              "conv8,ks3,stride1+norm,leaky_relu+conv8,ks3,stride1+norm,leaky_relu+conv%d,ks1,stride1")


# ---- the restatement: one channel volume {d, h, w} -> one channel volume -----------------------------------------------------------
def ref_mean(v):
    D, H, W = v.shape
    p = np.pad(v, 1, mode="edge")
    acc = np.zeros_like(v)
    for kz in range(3):
        for ky in range(3):
            for kx in range(3):
                acc = acc + p[kz:kz + D, ky:ky + H, kx:kx + W]
    return (acc * (F(1) / F(27))).astype(F)


def ref_down(v):
    D, H, W = v.shape
    d, h, w = (D + 1) // 2, (H + 1) // 2, (W + 1) // 2
    p = np.zeros((2 * d, 2 * h, 2 * w), F)
    e = np.zeros((2 * d, 2 * h, 2 * w), bool)
    p[:D, :H, :W], e[:D, :H, :W] = v, True
    acc, n = np.zeros((d, h, w), F), np.zeros((d, h, w), F)
    for kz in range(2):
        for ky in range(2):
            for kx in range(2):
                here = e[kz::2, ky::2, kx::2]
                acc = np.where(here, acc + p[kz::2, ky::2, kx::2], acc)
                n = n + here.astype(F)
    return (acc / n).astype(F)


def ref_up(v, z0=0, z1=None):
    """the z-slab [z0, z1) of the upsampled volume"""
    D, H, W = v.shape
    z1 = 2 * D if z1 is None else z1
    z, y, x = np.meshgrid(np.arange(z0, z1), np.arange(2 * H), np.arange(2 * W), indexing="ij")
    pos = lambda i, n: np.minimum(np.maximum(F(0.5) * i.astype(F) - F(0.25), F(0)), F(n - 1))
    return R._trilinear(v, R._locate(pos(x, W), pos(y, H), pos(z, D), W, H, D))


def ref_norm(stack):
    """the whole stacked buffer"""
    with np.errstate(invalid="ignore"):
        mx = np.fmax.reduce(stack.ravel())      # NaN skipped
    return R._norm(stack, mx)


REF = {
    "gaussian_filter": R._smooth,
    "smoothing_filter": ref_mean,
    "downsampling": ref_down,
    "upsampling": ref_up,
    "flip_x": lambda v: np.flip(v, 2), "flip_y": lambda v: np.flip(v, 1), "flip_z": lambda v: np.flip(v, 0),
    "swap_xy": lambda v: np.swapaxes(v, 1, 2), "swap_yz": lambda v: np.swapaxes(v, 0, 1), "swap_xz": lambda v: np.swapaxes(v, 0, 2),
}


def ref_command(name, stack):
    if name == "none":
        return stack
    if name == "normalize":
        return ref_norm(stack)
    return np.ascontiguousarray(np.stack([REF[name](stack[c]) for c in range(stack.shape[0])]))


def ref_chain(names, stack):
    for name in names:
        stack = ref_command(name, stack)
    return stack


def dev_offset(a, offset):
    """a device copy of a starting `offset` floats into its allocation: a base that is only 4-byte aligned"""
    buf = torch.full((a.size + offset,), 7, dtype=torch.float32, device=DEV)
    v = buf[offset:].view(a.shape)
    v.copy_(torch.from_numpy(a))
    return v


def volume(seed, c, shape, special=True):
    rs = np.random.RandomState(seed)
    v = (rs.rand(c, *shape).astype(F) - F(0.25)) * F(3)
    if special and v.size >= 8:                 # denormals, zeros of both signs, large values
        flat = v.reshape(-1)
        flat[rs.randint(0, flat.size, 6)] = [0.0, -0.0, 1e-42, -3e-39, 1e30, -1e30]
    return v


def same(got, exp):
    """bit for bit; a NaN matches a NaN (its payload is not part of any definition)"""
    assert got.shape == exp.shape, (got.shape, exp.shape)
    got, exp = np.ascontiguousarray(got, dtype=F), np.ascontiguousarray(exp, dtype=F)
    nan = np.isnan(exp)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.uint32)[~nan], exp.view(np.uint32)[~nan])


# (d, h, w), channels, base offset in floats
CASES = [((1, 1, 1), 1, 0), ((3, 1, 5), 2, 1), ((1, 7, 1), 3, 0), ((2, 2, 2), 1, 3), ((13, 11, 9), 3, 1), ((33, 9, 35), 2, 0),
         ((34, 17, 67), 1, 1), ((7, 40, 130), 2, 2), ((65, 8, 32), 3, 0), ((40, 33, 31), 1, 1)]
OUT_OF_PLACE = ["gaussian_filter", "smoothing_filter", "downsampling", "upsampling"] + list(PRE.PERMUTES)


# ---- every command ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(len(CASES)))
@pytest.mark.parametrize("name", OUT_OF_PLACE)
def test_command_is_bitwise_the_restatement(name, k):
    shape, c, off = CASES[k]
    v = volume(100 + k, c, shape)
    src = dev_offset(v, off)
    exp = ref_command(name, v)
    out = dev_offset(np.full(exp.shape, 5, F), off)            # the destination is only 4-byte aligned too
    got = PRE.apply(name, src, out=out)
    assert got.data_ptr() == out.data_ptr() and tuple(got.shape) == exp.shape
    assert same(got.cpu().numpy(), exp), (name, shape, c)
    assert same(src.cpu().numpy(), v)                          # the source is not written
    assert same(PRE.apply(name, src).cpu().numpy(), exp)       # a result of its own


@pytest.mark.parametrize("k", range(len(CASES)))
@pytest.mark.parametrize("name", ["gaussian_filter", "smoothing_filter"])
def test_both_filter_kernels_give_the_same_bits(name, k):
    shape, c, off = CASES[k]
    v = volume(200 + k, c, shape)
    src = dev_offset(v, off)
    exp = ref_command(name, v)
    for impl in (PRE.IMPL_LDS, PRE.IMPL_VOXEL):
        assert same(PRE.apply(name, src, impl=impl).cpu().numpy(), exp), (name, shape, impl)


def test_filters_do_not_cross_a_channel_boundary():
    v = np.zeros((3, 4, 5, 6), F)
    v[1] = 64.0
    src = torch.from_numpy(v).to(DEV)
    for name in ("gaussian_filter", "smoothing_filter", "downsampling", "upsampling"):
        got = PRE.apply(name, src).cpu().numpy()
        assert not got[0].any() and not got[2].any() and got[1].min() > 63.9, name


@pytest.mark.parametrize("k", range(len(CASES)))
def test_normalize_is_bitwise_the_restatement(k):
    shape, c, off = CASES[k]
    v = np.abs(volume(300 + k, c, shape, special=False)) + F(0.01)
    if v.size > 4:
        v.reshape(-1)[[1, v.size // 2]] = np.nan                # skipped by the maximum
    buf = dev_offset(v, off)
    exp = ref_norm(v)
    got = PRE.normalize_(buf)
    assert got.data_ptr() == buf.data_ptr()
    g = got.cpu().numpy()
    assert same(g, exp) and float(np.nanmax(g)) == 1.0


def test_normalize_of_a_buffer_without_a_positive_maximum_leaves_it():
    for v in (-np.random.RandomState(0).rand(2, 6, 6, 6).astype(F), np.zeros((1, 3, 4, 5), F), np.full((1, 2, 2, 2), np.nan, F)):
        got = PRE.normalize_(torch.from_numpy(v.copy()).to(DEV)).cpu().numpy()
        assert same(got, v)
        assert same(PRE.run_preproc(torch.from_numpy(v.copy()).to(DEV), "normalize").cpu().numpy(), v)


# ---- chains ----------------------------------------------------------------------------------------------------------------------
CHAINS = ["gaussian_filter+downsampling+normalize", "normalize+smoothing_filter+flip_x+swap_yz", "none+upsampling+gaussian_filter+flip_z",
          "downsampling+downsampling+upsampling+swap_xz+normalize", "swap_xy+none+flip_y+smoothing_filter+gaussian_filter+downsampling",
          "normalize", "none", "flip_x"]


@pytest.mark.parametrize("chain", CHAINS)
@pytest.mark.parametrize("c, shape", [(1, (9, 11, 13)), (2, (12, 7, 35)), (3, (5, 1, 3))])
def test_chains_are_bitwise_the_restatement_and_the_caller_keeps_its_tensor(chain, c, shape):
    v = np.abs(volume(400 + c, c, shape, special=False))
    x = dev_offset(v, 1)
    got = PRE.run_preproc(x, chain)
    names = PRE.parse_chain(chain)
    exp = ref_chain(names, v)
    assert tuple(got.shape) == exp.shape and got.is_contiguous() and same(got.cpu().numpy(), exp), chain
    assert same(x.cpu().numpy(), v)                            # the caller's tensor is unchanged
    assert (got.data_ptr() == x.data_ptr()) == (not PRE.active(names))
    # parsed steps and a caller's scratch give the same
    sc = torch.empty(PRE.preproc_scratch_bytes(8 * v.size), dtype=torch.uint8, device=DEV)
    assert torch.equal(PRE.run_preproc(x, names, scratch=sc), got)
    # the geometry the chain reports is the grid it produced
    dims, _, _ = PRE.geometry(chain, shape[::-1], (1, 1, 1))
    assert dims == tuple(got.shape[1:])[::-1]


# ---- the large case, determinism, concurrency ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [1, 2])
def test_large_case_bitwise_and_twice_the_same_bits(c):
    g = torch.Generator(device=DEV).manual_seed(c)
    buf = torch.rand((c * 180 * 256 * 256 + 1,), generator=g, device=DEV) - 0.3
    src = buf[1:].view(c, 180, 256, 256)                       # 4 bytes off
    v = src.cpu().numpy()
    # two channels: the filters, whose one launch covers them; one channel: every command
    for name in ("gaussian_filter", "smoothing_filter") + (("downsampling", "flip_x", "swap_xz") if c == 1 else ()):
        a, b = PRE.apply(name, src), PRE.apply(name, src)
        assert torch.equal(a, b), name
        assert same(a.cpu().numpy(), ref_command(name, v)), name
    assert torch.equal(PRE.apply("gaussian_filter", src, impl=PRE.IMPL_LDS), PRE.apply("gaussian_filter", src, impl=PRE.IMPL_VOXEL))
    if c > 1:
        return
    a, b = PRE.apply("upsampling", src), PRE.apply("upsampling", src)
    assert torch.equal(a, b) and a.shape == (c, 360, 512, 512)
    for z0, z1 in ((0, 3), (177, 181), (357, 360)):            # slabs of it against the restatement (94 M voxels of numpy gathers)
        assert same(a[0, z0:z1].cpu().numpy(), ref_up(v[0], z0, z1)), z0
    n = PRE.normalize_(src.clone())
    assert torch.equal(n, PRE.normalize_(src.clone())) and same(n.cpu().numpy(), ref_norm(v))


def test_two_threads_on_two_streams():
    chains = ["gaussian_filter+downsampling+normalize", "normalize+upsampling+smoothing_filter+swap_xy"]
    cases = []
    for k, chain in enumerate(chains):
        x = torch.from_numpy(np.abs(volume(500 + k, 2, (40, 37, 70), special=False))).to(DEV)
        cases.append((x, chain, PRE.run_preproc(x, chain).clone()))
    torch.cuda.synchronize()
    bad = []

    def work(i):
        x, chain, exp = cases[i]
        s = torch.cuda.Stream(DEV)
        sc = torch.empty(PRE.preproc_scratch_bytes(8 * x.numel()), dtype=torch.uint8, device=DEV)
        with torch.cuda.stream(s):
            for _ in range(20):
                got = PRE.run_preproc(x, chain, scratch=sc)
                s.synchronize()
                if not torch.equal(got, exp):
                    bad.append(i)

    ts = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    [t.start() for t in ts]
    [t.join() for t in ts]
    assert not bad


# ---- EvaluateUNet ------------------------------------------------------------------------------------------------------------------
OUTPUTS = ("label", "fg_prob", "label_prob")


def small_model(in_count=1, out_c=5, dt="fp32", dim=(24, 16, 32), vs=(1.5, 1.2, 1.0)):
    m = U.UNet3d(in_count, out_c, SMOKE_ARCH % out_c, device=DEV, dtype=dt, seed=2)
    m.dim, m.voxel_size = dim, vs                              # non-cubic, anisotropic
    return m


def assert_same_results(a, b, chain):
    if not chain:
        assert a.dtype == b.dtype == np.float32 and a.shape == b.shape and a.tobytes() == b.tobytes()
        return
    assert sorted(a) == sorted(b) == sorted(OUTPUTS)
    for k in OUTPUTS:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), k


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("chain", [None, "model"])
def test_evaluate_noop_keywords_change_no_bit(dt, chain):
    m = small_model(2, 5, dt)
    rs = np.random.RandomState(5)
    own = (np.eye(3).reshape(9) * 1.1, np.array([0.5, -1.0, 2.0]))            # a caller's float64 map, not fp32-representable
    ios = [[U.NativeVolume(rs.rand(2 * 20, 18, 30).astype(F), (1.0, 1.2, 1.1)), rs.rand(2 * 32, 16, 24).astype(F)],
           [U.NativeVolume(rs.rand(2 * 26, 22, 38).astype(F), (0.9, 1.0, 1.3), map=own)]]
    base = U.EvaluateUNet(m, postproc=chain, outputs=OUTPUTS).start(ios)
    for pre in ("", "none", None, " none + none "):
        ev = U.EvaluateUNet(m, postproc=chain, outputs=OUTPUTS, preproc=pre, orientation="")
        got = ev.start(ios)
        assert not ev.aborted and ev.error_msg == "" and ev.cur_prog == 2
        for gf, bf in zip(got, base):
            for g, b in zip(gf, bf):
                assert_same_results(g, b, chain)
    m.preproc, m.orientation = "none", ""                                      # and through the model's own strings
    got = U.EvaluateUNet(m, postproc=chain, outputs=OUTPUTS, preproc="model", orientation="model").start(ios)
    assert_same_results(got[1][0], base[1][0], chain)


ORIENT = {   # name -> (orient a {d, h, w} array, undo it)
    "flip_x": (lambda v: np.flip(v, -1), lambda v: np.flip(v, -1)),
    "flip_y": (lambda v: np.flip(v, -2), lambda v: np.flip(v, -2)),
    "flip_z": (lambda v: np.flip(v, -3), lambda v: np.flip(v, -3)),
    "swap_xy": (lambda v: np.swapaxes(v, -1, -2), lambda v: np.swapaxes(v, -1, -2)),
    "swap_yz": (lambda v: np.swapaxes(v, -2, -3), lambda v: np.swapaxes(v, -2, -3)),
    "swap_xz": (lambda v: np.swapaxes(v, -1, -3), lambda v: np.swapaxes(v, -1, -3)),
}


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("chain", [None, "model"])
@pytest.mark.parametrize("orient", ["flip_x+swap_yz", "swap_xy+flip_x", "swap_xz+flip_y+swap_xy+flip_z"])
def test_evaluate_orientation_on_an_identity_grid_is_the_materialised_orientation(orient, chain, dt):
    """V lives on the grid the orientation turns into the model's (D0 at vs0): every sample in and out is at an integer position, so
    evaluating V under the orientation equals evaluating O(V) with none and un-orienting the results in numpy, bit for bit."""
    out_c = 5
    m = small_model(1, out_c, dt)
    names = orient.split("+")
    W, H, D = m.dim
    d0 = np.zeros((D, H, W), F)
    for n in reversed(names):                                                  # the model's grid through the inverse orientation
        d0 = ORIENT[n][1](d0)
    vs0 = list(m.voxel_size)
    for n in reversed(names):
        if n.startswith("swap"):
            a, b = ("xyz".index(n[-2]), "xyz".index(n[-1]))
            vs0[a], vs0[b] = vs0[b], vs0[a]
    V = np.random.RandomState(3).rand(*d0.shape).astype(F)
    OV = V
    for n in names:
        OV = ORIENT[n][0](OV)
    OV = np.ascontiguousarray(OV)
    assert OV.shape == (D, H, W)
    ev = U.EvaluateUNet(m, postproc=chain, outputs=OUTPUTS, orientation=orient)
    got = ev.start([[U.NativeVolume(V, tuple(vs0))]])[0][0]
    assert not ev.aborted and ev.error_msg == ""
    ev = U.EvaluateUNet(m, postproc=chain, outputs=OUTPUTS)
    plain = ev.start([[U.NativeVolume(OV, m.voxel_size)]])[0][0]
    assert not ev.aborted and ev.error_msg == ""

    def undo(a, planes):
        a = a.reshape((planes, D, H, W))
        for n in reversed(names):
            a = ORIENT[n][1](a)
        return np.ascontiguousarray(a).reshape((planes * V.shape[0],) + V.shape[1:])

    if chain is None:
        assert got.shape == (out_c * V.shape[0],) + V.shape[1:] and got.tobytes() == undo(plain, out_c).tobytes()
        return
    for k, planes in (("label", 1), ("fg_prob", 1), ("label_prob", out_c - 1)):
        exp = undo(plain[k], planes).reshape(got[k].shape)
        assert got[k].dtype == plain[k].dtype and got[k].tobytes() == exp.tobytes(), k
    assert got["label"].shape == V.shape


def manual(m, nv, pre, orient, chain, calls=None):
    """run_preproc -> the composed maps -> to_model_space -> forward -> the way back, by hand from the public pieces"""
    io = nv.data
    d = io.shape[0] // m.in_count
    native = (d,) + io.shape[1:]
    x = torch.from_numpy(io).view(m.in_count, *native).to(DEV)
    xp = PRE.run_preproc(x, pre)
    pdims, pvs, G = PRE.geometry(pre, native[::-1], nv.voxel_size)
    assert tuple(xp.shape[1:]) == pdims[::-1]
    D0, vs0, M = PRE.orientation_map(orient, m.dim, m.voxel_size)
    Fm = nv.map if nv.map is not None else SP.model_to_image_map(D0, vs0, pdims, pvs)
    fwd = SP.compose_map(Fm, M)
    back = SP.invert_map(SP.compose_map(G, fwd))
    xm = SP.to_model_space(m, xp, pvs, map=fwd)[0]
    W, H, D = m.dim
    with torch.no_grad():
        logits = m.forward(xm.unsqueeze(0))[0].view(m.out_count, D, H, W)
    if not chain:
        return SP.resample(logits, native, back, "linear").cpu().numpy().reshape(m.out_count * d, *io.shape[1:])
    res = SP.postproc_native(logits, back, native, 0.5)
    for name, p in P.parse_chain(chain)[3:]:
        assert name == "defragment"
        sc = torch.empty(P.postproc_scratch_bytes(m.out_count, d * io.shape[1] * io.shape[2]), dtype=torch.uint8, device=DEV)
        P.defragment_call(native[::-1], False, p["threshold"], p["size_ratio"], res["fg_prob"], res["label_prob"], m.out_count - 1,
                          res["label"], sc)
    torch.cuda.synchronize()
    shapes = {"label": (d,) + io.shape[1:], "fg_prob": (d,) + io.shape[1:], "label_prob": ((m.out_count - 1) * d,) + io.shape[1:]}
    return {k: res[k].cpu().view(torch.int16 if k == "label" else torch.float32).numpy().view(np.uint16 if k == "label" else F)
            .reshape(shapes[k]) for k in OUTPUTS}


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("chain", [None, "model", "softmax+create_mask+argmax+defragment"])
@pytest.mark.parametrize("pre, orient", [("gaussian_filter+downsampling+normalize", "swap_xy+flip_z"),
                                         ("smoothing_filter+flip_y+upsampling", ""), ("", "swap_yz+flip_x"),
                                         ("normalize+swap_xz+gaussian_filter", "flip_y")])
def test_evaluate_general_case_equals_the_manual_sequence(pre, orient, chain, dt):
    out_c = 5
    m = small_model(2, out_c, dt)
    m.preproc, m.orientation = pre, orient
    rs = np.random.RandomState(11)
    own = SP.model_to_image_map(m.dim, m.voxel_size, (30, 20, 24), (1.3, 1.1, 0.9))
    ios = [[U.NativeVolume(rs.rand(2 * 20, 18, 30).astype(F), (1.0, 1.2, 1.1))],
           [U.NativeVolume(rs.rand(2 * 26, 22, 38).astype(F), (0.9, 1.0, 1.3)), U.NativeVolume(rs.rand(2 * 21, 19, 33).astype(F), (1, 1, 1), map=own)]]
    keep = [[nv.data.copy() for nv in f] for f in ios]
    ev = U.EvaluateUNet(m, postproc=chain, outputs=OUTPUTS, preproc="model", orientation="model")
    got = ev.start(ios)
    assert not ev.aborted and ev.error_msg == "" and ev.cur_prog == 2
    text = m.postproc if chain == "model" else chain
    for gf, nf, kf in zip(got, ios, keep):
        for g, nv, k in zip(gf, nf, kf):
            d, h, w = nv.data.shape                                            # the scan's ORIGINAL stacked shape
            exp = manual(m, nv, pre, orient, text)
            if chain is None:
                assert g.shape == (out_c * d // 2, h, w)
            else:
                assert g["label"].shape == (d // 2, h, w) and g["label_prob"].shape == ((out_c - 1) * d // 2, h, w)
            assert_same_results(g, exp, chain)
            assert np.array_equal(nv.data, k)                                  # the caller's scan is not written
    # explicit strings are the model's strings
    ev = U.EvaluateUNet(m, postproc=chain, outputs=OUTPUTS, preproc=pre, orientation=orient)
    assert_same_results(ev.start(ios[:1])[0][0], got[0][0], chain)


def test_evaluate_preproc_is_not_ignored():
    """what the issue is about: a model that carries an orientation labels a scan differently from one that does not"""
    m = small_model(1, 4, "fp32")
    nv = U.NativeVolume(np.random.RandomState(1).rand(22, 18, 30).astype(F), (1.0, 1.2, 1.1))
    a = U.EvaluateUNet(m).start([[nv]])[0][0]
    m.orientation = "swap_xy"
    b = U.EvaluateUNet(m, orientation="model").start([[nv]])[0][0]
    c = U.EvaluateUNet(m).start([[nv]])[0][0]                                  # opt-in: without the keyword nothing changes
    assert a.shape == b.shape and a.tobytes() == c.tobytes() and a.tobytes() != b.tobytes()


def test_evaluate_errors_end_the_run_before_any_forward():
    m = small_model(1, 3, "fp32")
    calls = []
    real = m.forward
    m.forward = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
    good = U.NativeVolume(np.random.RandomState(0).rand(10, 12, 14).astype(F), (1, 1, 1))
    for kw, msg in ((dict(preproc="gaussian_filter+sharpen"), "unknown command sharpen"), (dict(orientation="flip_x+normalize"), "unknown command normalize"),
                    (dict(preproc="model"), "unknown command oops")):
        m.preproc = "oops"
        ev = U.EvaluateUNet(m, **kw)
        out = ev.start([[good]])
        assert ev.aborted and not ev.running and ev.error_msg == msg and ev.cur_prog == 0 and out[0][0] is good, kw
    m.preproc = ""
    plain = np.zeros((32, 16, 24), F)
    for kw in (dict(preproc="gaussian_filter"), dict(orientation="flip_x"), dict(preproc="none+normalize", orientation="swap_xy")):
        ev = U.EvaluateUNet(m, **kw)
        out = ev.start([[plain, good]])
        assert ev.aborted and not ev.running and "NativeVolume" in ev.error_msg and ev.cur_prog == 0 and out[0][0] is plain, kw
    assert not calls
    ev = U.EvaluateUNet(m, preproc="none", orientation="")                     # `none` is not in force: the array path is untouched
    out = ev.start([[plain]])
    assert not ev.aborted and ev.cur_prog == 1 and len(calls) == 1 and out[0][0].shape == (3 * 32, 16, 24)
