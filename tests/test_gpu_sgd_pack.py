"""unet_sgd_step_packed (include/unet_hip.h, kernels_sgd_pack.hip): the optimizer update that also writes the next forward's filter
packs.  It performs the same arithmetic on the same values as unet_sgd_step followed by unet_pack_filters, so everything here is
compared bit for bit."""
import ctypes as C
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

import unet_studio_amd as U  # noqa: E402

E = U.engine
DEV = "cuda:0"

# widths that are multiples of 16 but not of 32 (48) on both sides of stride-1, stride-2 and conv_trans layers: ragged last tiles
ARCH_48 = ("conv48,ks3,stride1+norm,leaky_relu+conv48,ks3,stride1+norm,leaky_relu\n"
           "conv96,ks3,stride2+norm,leaky_relu+conv96,ks3,stride1+norm,leaky_relu+conv_trans48,ks2,stride2\n"
           "conv48,ks3,stride1+norm,leaky_relu+conv48,ks3,stride1+norm,leaky_relu+conv4,ks1,stride1")
ARCH_SMALL = ("conv16,ks3,stride1+norm,leaky_relu+conv16,ks3,stride1+norm,leaky_relu\n"
              "conv32,ks3,stride2+norm,leaky_relu+conv32,ks3,stride1+norm,leaky_relu+conv_trans16,ks2,stride2\n"
              "conv16,ks3,stride1+norm,leaky_relu+conv16,ks3,stride1+norm,leaky_relu+conv4,ks1,stride1")

_plans = {}


def _plan(arch, out_c, n, dtype):
    key = (arch, out_c, n, dtype)
    if key not in _plans:
        _plans[key] = E.Plan(arch, 1, out_c, (n, n, n), dtype, 0)
    return _plans[key]


def stream():
    return torch.cuda.current_stream(DEV).cuda_stream


def _both_ways(plan, clipped, nesterov, with_dgrad):
    """copy A: unet_sgd_step then unet_pack_filters; copy B: unet_sgd_step_packed.  Returns made_B and the two states."""
    n = sum(math.prod(s) for s in plan.param_shapes)
    gen = torch.Generator(device=DEV).manual_seed(11 + 2 * int(clipped) + int(nesterov))
    p0 = torch.randn(n, generator=gen, device=DEV) * 0.1
    m0 = torch.randn(n, generator=gen, device=DEV) * 0.01
    # clip_norm 12: ||g|| = sqrt(n) * sigma is either far above or far below it
    g0 = torch.randn(n, generator=gen, device=DEV) * ((100.0 if clipped else 0.01) * 12.0 / math.sqrt(n))
    offs = [0]
    for s in plan.param_shapes:
        offs.append(offs[-1] + math.prod(s))
    out = []
    for fused in (False, True):
        p, g, m = p0.clone(), g0.clone(), m0.clone()
        ws = torch.full((plan.workspace_bytes,), 0xA5, dtype=torch.uint8, device=DEV)   # unwritten fragments / counters stay visible
        norm = torch.zeros(1, device=DEV)
        scratch = torch.empty(65536, dtype=torch.uint8, device=DEV)
        made = C.c_int(-1)
        args = (plan.handle, p.data_ptr(), g.data_ptr(), m.data_ptr(), 0.05, 0.99, int(nesterov), 3e-5, 12.0, 0.5, norm.data_ptr())
        if fused:
            E.check(E.lib.unet_sgd_step_packed(*args, ws.data_ptr(), int(with_dgrad), C.byref(made), scratch.data_ptr(), stream()))
        else:
            E.check(E.lib.unet_sgd_step(*args, scratch.data_ptr(), stream()))
            pp = E.ptr_array([p.data_ptr() + 4 * o for o in offs[:-1]])
            E.check(E.lib.unet_pack_filters(plan.handle, pp, ws.data_ptr(), int(with_dgrad), C.byref(made), stream()))
        torch.cuda.synchronize()
        out.append((made.value, p, g, m, norm, ws))
    gnorm = float(out[0][4]) * 1.0
    assert (gnorm > 12.0) == clipped
    return out


def _assert_identical(a, b):
    for name, x, y in zip(("params", "grads", "momentum", "norm_out", "workspace"), a[1:], b[1:]):
        assert torch.equal(x, y), name
    assert float(a[2].abs().max()) == 0.0 and float(b[2].abs().max()) == 0.0      # zero_grad


@pytest.mark.parametrize("nesterov", [True, False])
@pytest.mark.parametrize("clipped", [True, False])
@pytest.mark.parametrize("n", [32, 64])
def test_default_arch_update_and_packs_equal_the_two_calls(n, clipped, nesterov):
    """Default architecture, bf16.  32^3: the halo-tile and deep kinds; 64^3: the sliding-window stride-2 kinds (PK_CONV_S2_DGRAD and the
    conv_trans packs of the 128^3 workload).  Parameters, momentum, gradients (zero), norm_out and the WHOLE workspace, filled with one
    byte pattern beforehand, must be byte-identical, with and without the dgrad packs."""
    plan = _plan(U.default_feature(6), 6, n, U.DTYPE_BF16)
    for with_dgrad in (1, 0):
        a, b = _both_ways(plan, clipped, nesterov, with_dgrad)
        assert a[0] == 1 and b[0] == 1
        _assert_identical(a, b)


@pytest.mark.parametrize("with_dgrad", [1, 0])
def test_ragged_tiles_widths_of_48(with_dgrad):
    """layer widths that are multiples of 16 but not of 32: the last tile of a tensor is 16 wide on either side"""
    plan = _plan(ARCH_48, 4, 32, U.DTYPE_BF16)
    a, b = _both_ways(plan, True, True, with_dgrad)
    assert a[0] == 1 and b[0] == 1
    _assert_identical(a, b)


def test_fp32_engine_has_no_packs_and_runs_the_plain_update():
    plan = _plan(ARCH_SMALL, 4, 16, U.DTYPE_F32)
    a, b = _both_ways(plan, True, True, 1)
    assert a[0] == 0 and b[0] == 0
    _assert_identical(a, b)


def _trainer(sizes, batch, fused):
    m = U.UNet3d(1, 4, ARCH_SMALL, device=DEV, dtype="bf16", seed=0)
    srcs = [U.SyntheticVolumes(1, 4, (s, s, s), DEV, cache=4) for s in sizes]
    t = U.Trainer(m, U.TrainingParam(batch_size=batch, epoch=100, learning_rate=0.05), lambda i: srcs[(i // batch) % len(srcs)](i % 4))
    t.pack_in_update = fused
    claimed = []                       # per micro-step: did the trainer tell the forward that the packs are current?
    inner = m.forward_backward
    m.forward_backward = lambda *a, **kw: (claimed.append(bool(kw.get("packs_current"))), inner(*a, **kw))[1]
    return m, t, claimed


@pytest.mark.parametrize("batch", [1, 2])
def test_trainer_with_the_packs_from_the_update_equals_repacking(batch):
    """three steps at 32^3: bit-identical parameters and loss statistics; with the fused update every forward after the first step's
    first one finds current packs (batch 2: the second micro-step reuses them as before)"""
    ma, ta, ca = _trainer([32], batch, True)
    mb, tb, cb = _trainer([32], batch, False)
    assert U.Trainer(ma, ta.param, ta.source).pack_in_update       # the default
    for _ in range(3):
        sa, sb = ta.step().clone(), tb.step().clone()
        assert torch.equal(sa, sb)
        assert ta._packed_size == (32, 32, 32) and tb._packed_size is None
    torch.cuda.synchronize()
    assert torch.equal(ma.flat_params, mb.flat_params)
    assert torch.equal(ma.optimizer.momentum_buffer, mb.optimizer.momentum_buffer)
    assert ca == [False] + [True] * (3 * batch - 1)
    assert cb == ([False] + [True] * (batch - 1)) * 3


def test_trainer_repacks_at_another_size():
    """a step at 16^3 leaves packs in the 16^3 workspace only: the next step, at 32^3, must repack and not claim current packs"""
    ma, ta, ca = _trainer([16, 32], 1, True)
    mb, tb, cb = _trainer([16, 32], 1, False)
    for _ in range(4):
        sa, sb = ta.step().clone(), tb.step().clone()
        assert torch.equal(sa, sb)
    torch.cuda.synchronize()
    assert torch.equal(ma.flat_params, mb.flat_params)
    assert ca == [False] * 4 and cb == [False] * 4
    assert ta._packed_size == (32, 32, 32)
