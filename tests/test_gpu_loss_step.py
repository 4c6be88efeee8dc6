"""GPU (-m gpu): the loss kernels and the optimizer-step kernels of kernels_elem.hip against fp64, at their edges.

Loss (unet_loss -> launch_loss_partial / k_loss_finalize / launch_loss_grad, k_target_half): every dispatch branch -- the
four-voxels-per-thread kernels (v4), k_loss_partial_reg<8>, k_loss_partial_reg<32>, the LDS-atomic k_loss_partial, the generic
k_loss_grad with and without collapse_before, the alignment fallback out of v4 and the grid-stride second trip -- against
oracle.calc_losses / oracle.deep_supervision, which compute in fp64 from the same fp32 logits.  Tolerances are those of
test_gpu_parity.test_fused_loss_vs_oracle: ce / dice / mse rtol = atol = 2e-5, total 3 * 2e-5, dL/dlogits within 1e-4 of the
level's largest reference gradient.

Inputs (make_logits / make_target): non-winner logits uniform in [-2, 2]; every voxel has a random winner class whose logit is
raised by 25 ("peaked": every other probability is clamped to 1e-6 and the winner's to 1 - 1e-6) or by 3 ("plain": nothing is
clamped); ~15 % of the targets are masked labels in [C, C + 2].  The clamp's gradient is discontinuous at its boundary, where a
float and a double evaluation may land on opposite sides -- a property of the operation, not of a kernel -- so the builder asserts
in fp64 that no (merged) probability q has q or 1 - q inside (0.5e-6, 2e-6).

Optimizer step (unet_sgd_step -> k_sumsq_partial, k_sgd with sgd_update.h) against numpy float64 on plans whose parameter
segments are no multiples of 4: 16-byte groups that straddle a decayed and an undecayed segment, the n % 4 tail, more than one
block, and the grid-stride second trip of both kernels."""
import functools
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import unet_studio_amd as U  # noqa: E402
from oracle import oracle as O  # noqa: E402

E = U.engine
DEV = "cuda:0"
ALL_MASKS = ((1, 1, 1), (1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 0, 0))
EPS = float(np.float32(1e-5))      # the dice epsilon is a float32 1e-5 in the reference


def stream():
    return torch.cuda.current_stream(DEV).cuda_stream


# ------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------
def merged_softmax64(lg, collapse):
    """fp64 softmax over the merged classes of [C, S] logits (class 0 = logsumexp of classes 0 .. collapse-1)"""
    x = lg.astype(np.float64)
    if collapse:
        head = x[:collapse]
        mx = head.max(0)
        x = np.concatenate([(mx + np.log(np.exp(head - mx).sum(0)))[None], x[collapse:]], 0)
    e = np.exp(x - x.max(0))
    return e / e.sum(0)


def make_logits(C, size, seed, collapse=0, peaked=0.5, winners=None):
    """fp32 [C, D, H, W] logits and the winner class per voxel; asserts the clamp-boundary condition (no exclusions)."""
    rng = np.random.default_rng(seed)
    S = math.prod(size)
    lg = rng.uniform(-2.0, 2.0, (C, S)).astype(np.float32)
    pool = np.arange(C) if winners is None else np.asarray(winners)
    win = pool[rng.integers(0, len(pool), S)]
    pk = rng.random(S) < peaked
    lg[win, np.arange(S)] += np.where(pk, np.float32(25.0), np.float32(3.0))
    q = merged_softmax64(lg, collapse)
    for x in (q, 1.0 - q):
        assert not ((x > 0.5e-6) & (x < 2e-6)).any(), "a probability lies at the clamp boundary: the builder was changed"
    if 0.0 < peaked < 1.0:      # both clamps are in play: in a peaked voxel every class but the winner sits on the low one
        assert (q < 1e-6).mean() > 0.6 * peaked * (len(q) - 1) / len(q) and (q > 1.0 - 1e-6).any()
    return lg.reshape(C, *size), win


def make_target(C, size, seed, allowed=None, masked=0.15):
    """int64 [D, H, W]: classes drawn from `allowed` (default: all), a fraction `masked` of them replaced by labels in [C, C+2]"""
    rng = np.random.default_rng(seed + 1000)
    S = math.prod(size)
    pool = np.arange(C) if allowed is None else np.asarray(allowed)
    t = pool[rng.integers(0, len(pool), S)].astype(np.int64)
    m = rng.random(S) < masked
    t[m] = rng.integers(C, C + 3, int(m.sum()))
    return t.reshape(size)


def absent_every_third(C):
    """targets without the classes 2, 5, 8, ...: dice terms with an empty intersection"""
    return [c for c in range(C) if c % 3 != 2]


# ------------------------------------------------------------------------------------------------
# loss: engine call and comparison
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def model_for(C, arch=None):
    # the architecture only fixes the class count and the level sizes: no forward is run, no workspace is allocated
    return U.UNet3d(1, C, arch or "conv4\nconv4\nconv%d,ks1" % C, device=DEV, dtype="fp32", seed=0)


def run_loss(C, logits_dev, target_dev, mask, collapse, arch=None, grad_into=None):
    """m.loss(...) as test_fused_loss_vs_oracle calls it; grad_into: unet_loss with the caller's own gradient buffers"""
    m = model_for(C, arch)
    plan = m.plan_for(tuple(logits_dev[0].shape[2:]))
    ce, dice, mse = mask
    if grad_into is None:
        losses, gouts = m.loss(logits_dev, target_dev, bool(ce), bool(dice), bool(mse), collapse, plan=plan)
    else:
        losses, gouts = torch.empty(4, dtype=torch.float32, device=DEV), grad_into
        E.check(E.lib.unet_loss(plan.handle, E.ptr_array([l.data_ptr() for l in logits_dev]), target_dev.data_ptr(),
                                ce | 2 * dice | 4 * mse, collapse, E.ptr_array([g.data_ptr() for g in gouts]), losses.data_ptr(),
                                m._loss_scratch(plan).data_ptr(), stream()))
    torch.cuda.synchronize()
    return losses.cpu().numpy().astype(np.float64), [g[0].cpu().numpy() for g in gouts]


def weights_of(mask):
    return tuple(float(x) for x in mask) if any(mask) else (1.0, 0.0, 0.0)      # train.cpp:696-697


def assert_level(lo, grad, oracle_losses, dl, w, what):
    """one level against the oracle, at test_fused_loss_vs_oracle's tolerances; every figure is printed before it is asserted"""
    oce, odice, omse = oracle_losses
    gmax = float(np.abs(dl).max())
    gerr = float(np.abs(grad.astype(np.float64) - dl).max())
    total = w[0] * oce + w[1] * odice + w[2] * omse
    print("%s: ce %.3e dice %.3e mse %.3e total %.3e (abs. errors; values %.4f %.6f %.4f)  grad %.3e of its max %.3e"
          % (what, abs(lo[1] - oce), abs(lo[2] - odice), abs(lo[3] - omse), abs(lo[0] - total), oce, odice, omse,
             gerr / max(gmax, 1e-300), gmax))
    assert np.allclose(lo[1:], [oce, odice, omse], rtol=2e-5, atol=2e-5), what
    assert abs(lo[0] - total) < 2e-5 * 3, what
    if gmax == 0.0:
        assert not grad.any(), what
    else:
        assert gerr < 1e-4 * gmax, what


def check_single_level(C, size, collapse=0, masks=ALL_MASKS, seed=0, peaked=0.5, allowed=None, winners=None, masked=0.15,
                       logits=None, target=None, place=None, grad_into=None):
    """builder inputs (or the given ones) through unet_loss and the oracle for every cost mask; returns {mask: gradient}.
    place: puts the logits on the device; grad_into: the gradient buffer to use instead of one that m.loss allocates"""
    if logits is None:
        logits, _ = make_logits(C, size, seed, collapse, peaked, winners)
    if target is None:
        target = make_target(C, size, seed, allowed, masked)
    ld = torch.from_numpy(logits)[None].to(DEV) if place is None else place(logits)
    td = torch.from_numpy(target)[None].to(DEV)
    grads = {}
    for mask in masks:
        w = weights_of(mask)
        lo, g = run_loss(C, [ld], td, mask, collapse, grad_into=None if grad_into is None else [grad_into])
        ol, dl = O.calc_losses(logits, target, C, collapse, w, True)
        assert_level(lo, g[0], ol, dl, w, "C=%d %s collapse=%d cost=%s" % (C, size, collapse, mask))
        grads[mask] = g[0]
    return grads


# ------------------------------------------------------------------------------------------------
# loss: cases
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [6, 8, 2])
def test_v4_kernels_with_masked_labels(C):
    """v4: k_loss_partial_v4 / k_loss_grad_v4 at 16^3 (S = 4096, the smallest volume that takes them), masked labels included.
    C = 8 fills every slot of the 8-wide register arrays; C = 2 has the dice denominator max(1, oc - 1) = 1."""
    check_single_level(C, (16, 16, 16), seed=10 + C)


@pytest.mark.parametrize("size", [(16, 16, 15), (17, 17, 15)])
def test_below_and_beside_the_v4_threshold(size):
    """reg<8> and the generic gradient kernel (no collapse_before) where v4 just does not apply: S = 3840 < 4096, and S = 4335 with
    S % 4 != 0 and a ragged last block"""
    check_single_level(6, size, seed=20 + size[0])


@pytest.mark.parametrize("C,collapse,absent", [(9, 0, True), (32, 0, True), (33, 0, True), (40, 9, True), (12, 5, True), (5, 4, False)])
def test_class_count_dispatch(C, collapse, absent):
    """launch_loss_partial by merged class count oc, all at (17,17,15), gradients from the generic k_loss_grad:
    C = 9 and 32: reg<32> (its first and last class count); C = 33: the LDS-atomic k_loss_partial; C = 40 with collapse_before 9:
    oc = 32, reg<32> again; C = 12 with collapse_before 5: oc = 8, reg<8> with C > 8; C = 5 with collapse_before 4: oc = 2.
    The five large class counts leave every third class out of the targets (empty intersections)."""
    check_single_level(C, (17, 17, 15), collapse, seed=30 + C, allowed=absent_every_third(C) if absent else None)


def dice_fp64(logits, target, C, clamp):
    """dice of calc_losses in numpy fp64 (no collapse_before), with or without the probability clamp in the sums"""
    S = target.size
    q = merged_softmax64(logits.reshape(C, S), 0)
    p = np.clip(q, 1e-6, 1.0 - 1e-6) if clamp else q
    t = target.reshape(S)
    valid = t < C
    terms = []
    for c in range(1, C):
        hit = valid & (t == c)
        inter, card = p[c][hit].sum(), p[c][valid].sum() + hit.sum()
        terms.append((2.0 * inter + EPS) / (card + EPS))
    return 1.0 - sum(terms) / max(1, C - 1), terms


@pytest.mark.parametrize("size", [(16, 16, 16), (17, 17, 15)])
def test_clamp_decides_the_dice_of_an_absent_class(size):
    """v4 at 16^3, reg<8> at (17,17,15).  Every voxel is peaked and class 3 is never a target and never a winner: its fp64
    cardinality is n_valid * 1e-6 and its dice term eps / (card + eps) ~ 3e-3; without the clamp in the partial sums the term is ~ 1
    and dice moves by ~ 0.2."""
    C, a = 6, 3
    rest = [c for c in range(C) if c != a]
    logits, win = make_logits(C, size, 41, peaked=1.0, winners=rest)
    target = make_target(C, size, 41, allowed=rest)
    assert not (win == a).any() and not (target == a).any()
    # the case is sharp: the reference's dice without the clamp is further away than 100 times the tolerance
    (_, odice, _), _ = O.calc_losses(logits, target, C, 0, (1.0, 1.0, 1.0), False)
    with_clamp, terms = dice_fp64(logits, target, C, True)
    without, _ = dice_fp64(logits, target, C, False)
    n_valid = int((target < C).sum())
    assert abs(with_clamp - odice) < 1e-9
    assert abs(terms[a - 1] - EPS / (n_valid * 1e-6 + EPS)) < 1e-6 * terms[a - 1]
    assert abs(without - odice) > 100 * (2e-5 + 2e-5 * abs(odice))
    check_single_level(C, size, logits=logits, target=target)


@pytest.mark.parametrize("n", [16, 12])
def test_no_valid_voxel(n):
    """every target >= C, at 16^3 (v4) and at 12^3 (reg<8>): n clamps to 1, the losses equal the oracle's (ce = mse = 0,
    dice = 1 - (C-1) * (eps/eps) / (C-1) = 0) and every gradient element is exactly 0"""
    C, size = 6, (n, n, n)
    logits, _ = make_logits(C, size, 50 + n)
    target = make_target(C, size, 50 + n, masked=1.0)
    assert (target >= C).all()
    grads = check_single_level(C, size, logits=logits, target=target)
    for mask, g in grads.items():
        assert not g.any(), mask


@pytest.mark.parametrize("C,size", [(6, (104, 104, 100)), (6, (65, 65, 63)), (33, (65, 65, 63))])
def test_grid_stride_second_trip(C, size):
    """more work than 1024 blocks of 256 threads take in one trip, cost (1,1,1):
    v4 at (104,104,100): S / 4 = 270 400 > 262 144 groups of four voxels, so some threads make two trips and some one;
    reg<8> at (65,65,63): S = 266 175 (odd) > 262 144 voxels; the LDS-atomic kernel (C = 33) at the same size.
    A kernel without its grid-stride loop loses 3 % (1.5 %) of the voxels: n, and with it every gradient element, is off by that."""
    S = math.prod(size)
    assert (S // 4 if (C <= 8 and S % 4 == 0) else S) > 1024 * 256
    check_single_level(C, size, masks=((1, 1, 1),), seed=60 + C + size[0])


def test_alignment_fallback_out_of_v4():
    """The v4 kernels need 16-byte aligned logits, targets and gradients.  The same C = 6, 16^3 inputs three ways, each against the
    oracle: (a) all aligned: v4; (b) logits in a buffer one float past a 16-byte boundary: reg<8> and the generic k_loss_grad at a
    v4 size; (c) only the gradient buffer misaligned: k_loss_partial_v4, then the generic k_loss_grad.

    k_loss_grad_v4 promises the gradients of k_loss_grad bit for bit: per voxel the same expressions in the same order, on the same
    level sums.  (c) against (a) is that promise, for every cost mask.  In (b) the level sums come from k_loss_partial_reg, which
    adds the same terms in another order than k_loss_partial_v4: the intersections and cardinalities may differ in their last bit,
    and with them the dice part of the gradient (measured on the MI355X: 573 of 24 576 elements at cost (1,1,1), 4245 at (0,1,0),
    none further apart than 2.9e-11, 1e-7 of the largest gradient).  So (b) equals (a) bit for bit where the gradient reads only n
    from the sums, a count and exact -- the cost masks without dice -- and meets the oracle tolerance with dice, as the loss
    scalars do."""
    C, size = 6, (16, 16, 16)
    logits, _ = make_logits(C, size, 16)          # the inputs of test_v4_kernels_with_masked_labels[6]
    target = make_target(C, size, 16)
    n = logits.size

    def misaligned(a=None):
        buf = torch.zeros(n + 8, dtype=torch.float32, device=DEV)
        v = buf[1:1 + n].view(1, *logits.shape)
        if a is not None:
            v.copy_(torch.from_numpy(a)[None])
        assert v.data_ptr() % 16 == 4 and v.is_contiguous()
        return v

    g_v4 = check_single_level(C, size, logits=logits, target=target)
    g_fb = check_single_level(C, size, logits=logits, target=target, place=misaligned)
    g_gen = check_single_level(C, size, logits=logits, target=target, grad_into=misaligned())
    for mask in ALL_MASKS:
        differ = int((g_v4[mask] != g_fb[mask]).sum())
        print("cost %s: %d of %d gradient elements differ between v4 and the whole fallback, largest difference %.3e"
              % (mask, differ, n, float(np.abs(g_v4[mask] - g_fb[mask]).max())))
        assert np.array_equal(g_v4[mask], g_gen[mask]), mask
        if not mask[1]:
            assert differ == 0, mask


ARCH_DS3 = ("conv4,ks3,stride1\nconv4,ks3,stride2\nconv4,ks3,stride2\n"
            "conv4,ks3,stride2+conv_trans4,ks2,stride2\n"
            "conv4,ks3,stride1+conv5,ks1,stride1+conv_trans4,ks2,stride2\n"
            "conv4,ks3,stride1+conv5,ks1,stride1+conv_trans4,ks2,stride2\n"
            "conv4,ks3,stride1+conv5,ks1,stride1")


@pytest.mark.parametrize("collapse", [0, 2])
def test_deep_supervision_three_levels(collapse):
    """Three heads at (32,16,16): 8192 voxels (v4 without collapse_before, reg<8> and the generic gradient kernel with it), 1024
    and 128 (reg<8>, generic gradient).  The level-0 target, masked labels included, goes through k_target_half twice.  Against
    oracle.deep_supervision: the total, the level-0 ce / dice / mse and every level's gradient at 1e-4 of that level's own largest
    reference gradient (the oracle folds the level weight 2^-k / sum into it).  Every cost mask without collapse_before, (1,1,1)
    with collapse_before 2."""
    C, size = 5, (32, 16, 16)
    sizes = [tuple(s >> k for s in size) for k in range(3)]
    assert [math.prod(s) for s in sizes] == [8192, 1024, 128]
    logits = [make_logits(C, s, 70 + k, collapse)[0] for k, s in enumerate(sizes)]      # the boundary condition holds per level
    target = make_target(C, size, 70)
    assert (target >= C).any() and (O.target_half(O.target_half(target)) >= C).any()   # masked labels reach the coarsest level
    ld = [torch.from_numpy(l)[None].to(DEV) for l in logits]
    td = torch.from_numpy(target)[None].to(DEV)
    for mask in (ALL_MASKS if collapse == 0 else ((1, 1, 1),)):
        lo, grads = run_loss(C, ld, td, mask, collapse, ARCH_DS3)
        total, stats, dls = O.deep_supervision(logits, target, C, tuple(bool(x) for x in mask), collapse)
        gerr = [float(np.abs(g.astype(np.float64) - dl).max()) / float(np.abs(dl).max()) for g, dl in zip(grads, dls)]
        print("collapse=%d cost=%s: total %.3e ce %.3e dice %.3e mse %.3e (abs. errors), gradients per level %s of the level's max"
              % (collapse, mask, abs(lo[0] - total), abs(lo[1] - stats[0]), abs(lo[2] - stats[1]), abs(lo[3] - stats[2]),
                 ["%.3e" % e for e in gerr]))
        assert abs(lo[0] - total) < 2e-5 * 3, mask
        assert np.allclose(lo[1:], stats, rtol=2e-5, atol=2e-5), mask
        for k, e in enumerate(gerr):
            assert e < 1e-4, (mask, k)


# ------------------------------------------------------------------------------------------------
# optimizer step
# ------------------------------------------------------------------------------------------------
WD, CLIP, LR, MOMENTUM = 3e-5, 12.0, 0.05, 0.99
# flat parameter counts 835, 4895 and 2 368 791, all with n % 4 == 3: one block; five blocks; more than k_sgd's 2048 blocks of 256
# groups and more than k_sumsq_partial's 1024 blocks of 1024 elements take in one trip
ARCH_STEP = {w: "conv%d,ks3,stride1+norm,leaky_relu\nconv%d,ks3,stride1\nconv5,ks1,stride1" % (w, w2)
             for w, w2 in ((7, 3), (42, 3), (290, 301))}


@functools.lru_cache(maxsize=None)
def step_plan(width):
    return E.Plan(ARCH_STEP[width], 1, 5, (8, 8, 8), U.DTYPE_F32, 0)


def segment_layout(plan):
    """flat offsets of the parameter segments and the weight-decay factor (0 / 1) of every flat element, read from the plan"""
    offs = [0]
    for s in plan.param_shapes:
        offs.append(offs[-1] + math.prod(s))
    return offs, np.repeat(np.asarray(plan.param_decay, np.float64), np.diff(offs))


def reference_step(p, g, m, decay, lr, momentum, nesterov, wd, clip, grad_scale):
    """train.cpp:759-766 with the optimizer of unet.cpp:246-277 in float64, from the same fp32 values"""
    p, g, m = p.astype(np.float64), g.astype(np.float64), m.astype(np.float64)
    gs = g * grad_scale
    norm = math.sqrt(float((gs * gs).sum()))
    coef = min(1.0, clip / (norm + 1e-6))
    d = gs * coef + wd * decay * p
    b = momentum * m + d
    return p - lr * ((d + momentum * b) if nesterov else b), b, norm


def step_bound(ref):
    return 1e-5 * max(1e-3, float(np.abs(ref).max()))      # the bound of test_golden_step_and_eval_modes


def run_steps(width, clipped, nesterov, grad_scale):
    plan = step_plan(width)
    offs, decay = segment_layout(plan)
    n = offs[-1]
    assert n % 4 != 0 and all(math.prod(s) % 4 for s in plan.param_shapes[:2])
    # 16-byte groups in which the decay factor changes
    groups = decay[:n - n % 4].reshape(-1, 4)
    straddle = np.flatnonzero(groups.min(1) != groups.max(1))
    assert len(straddle) >= 2 and decay[n - n % 4:].size == n % 4
    rng = np.random.default_rng(100 * width + 10 * int(clipped) + int(nesterov))
    p0 = (2.0 * rng.standard_normal(n)).astype(np.float32)
    for q in straddle:       # lanes whose decay differs from lane 0's: parameters large enough that the wrong decay shows
        lanes = 4 * q + np.flatnonzero(groups[q] != groups[q, 0])
        p0[lanes] = np.where(p0[lanes] < 0, -1.0, 1.0) * (4.0 + np.abs(p0[lanes]))
    m0 = (0.01 * rng.standard_normal(n)).astype(np.float32)
    p = torch.tensor(p0, device=DEV); m = torch.tensor(m0, device=DEV)
    norm_out = torch.zeros(1, device=DEV)
    scratch = torch.empty(65536, dtype=torch.uint8, device=DEV)      # as UNetOptimizer
    for step in range(2):    # the second step starts from the parameters and the momentum that the kernel itself produced
        target_norm = CLIP * 3.0 if clipped else CLIP / 3.0
        g0 = (rng.standard_normal(n) * (target_norm / (grad_scale * math.sqrt(n)))).astype(np.float32)
        g = torch.tensor(g0, device=DEV)
        p_in, m_in = p.cpu().numpy().copy(), m.cpu().numpy().copy()
        E.check(E.lib.unet_sgd_step(plan.handle, p.data_ptr(), g.data_ptr(), m.data_ptr(), LR, MOMENTUM, int(nesterov), WD, CLIP,
                                    grad_scale, norm_out.data_ptr(), scratch.data_ptr(), stream()))
        torch.cuda.synchronize()
        p_ref, m_ref, norm_ref = reference_step(p_in, g0, m_in, decay, LR, MOMENTUM, nesterov, WD, CLIP, grad_scale)
        assert (norm_ref > CLIP) == clipped and 0.8 * target_norm < norm_ref < 1.25 * target_norm
        # the case is sharp: with lane 0's decay in all four lanes of a group the momentum is further away than the bound
        wrong = decay.copy()
        wrong[:n - n % 4] = np.repeat(groups[:, 0], 4)
        _, m_wrong, _ = reference_step(p_in, g0, m_in, wrong, LR, MOMENTUM, nesterov, WD, CLIP, grad_scale)
        assert float(np.abs(m_wrong - m_ref).max()) > 3 * step_bound(m_ref)
        got_norm = float(norm_out)
        ep = float(np.abs(p.cpu().numpy() - p_ref).max()); em = float(np.abs(m.cpu().numpy() - m_ref).max())
        print("n=%d clipped=%d nesterov=%d grad_scale=%g step %d: norm %.3e relative, params %.3e (bound %.3e), momentum %.3e (bound %.3e)"
              % (n, clipped, nesterov, grad_scale, step, abs(got_norm - norm_ref) / norm_ref, ep, step_bound(p_ref), em, step_bound(m_ref)))
        assert abs(got_norm - norm_ref) < 1e-5 * norm_ref          # float squares summed in double: ~1e-7 expected
        assert ep < step_bound(p_ref) and em < step_bound(m_ref)
        assert not g.any()                                         # zero_grad: every gradient is exactly 0


@pytest.mark.parametrize("grad_scale", [1.0, 0.5])
@pytest.mark.parametrize("nesterov", [True, False])
@pytest.mark.parametrize("clipped", [True, False])
@pytest.mark.parametrize("width", [7, 42])
def test_sgd_step_against_fp64(width, clipped, nesterov, grad_scale):
    """unet_sgd_step on 835 and 4895 flat elements: segment sizes 189, 7 (1134, 42), ... are no multiples of 4, so 16-byte groups
    straddle decayed filters and undecayed biases / norm parameters, and block 0 handles a tail of n % 4 = 3.  Clip active (norm
    ~ 3 x clip) and inactive, Nesterov on and off, grad_scale 1 and 0.5, weight decay 3e-5; two steps in a row."""
    run_steps(width, clipped, nesterov, grad_scale)


def test_sgd_step_grid_stride_against_fp64():
    """2 368 791 flat elements: k_sgd's 2048 blocks and k_sumsq_partial's 1024 blocks each make more than one trip"""
    n = segment_layout(step_plan(290))[0][-1]
    assert n // 4 > 2048 * 256 and n > 1024 * 1024
    run_steps(290, True, True, 0.5)
