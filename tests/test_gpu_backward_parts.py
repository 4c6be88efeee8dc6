"""GPU (-m gpu): a backward issued in parts (unet_backward_part) makes the choices of the whole one (unet_backward).

Which dgrad epilogue leaves a norm backward's statistics rows, or runs all of it, is a value the engine computes from the launchers'
outcome queries (csrc/kernels.h: DgradOutcome); a part rebuilds the hand-off of the parts before it from those queries alone.  A
wrong predicted row count or a lost "done" flag in any part changes bits, so equality with the whole backward is the assertion."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import unet_studio_amd as U  # noqa: E402

E = U.engine
DEV = "cuda:0"

SMALL = ("conv16,ks3,stride1+norm,leaky_relu+conv16,ks3,stride1+norm,leaky_relu\n"
         "conv32,ks3,stride2+norm,leaky_relu+conv32,ks3,stride1+norm,leaky_relu+conv_trans16,ks2,stride2\n"
         "conv16,ks3,stride1+norm,leaky_relu+conv16,ks3,stride1+norm,leaky_relu+conv6,ks1,stride1")
DEEP2 = ("conv32,ks3,stride1+norm,leaky_relu+conv32,ks3,stride1+norm,leaky_relu\n"
         "conv64,ks3,stride2+norm,leaky_relu+conv64,ks3,stride1+norm,leaky_relu+conv_trans32,ks2,stride2\n"
         "conv32,ks3,stride1+norm,leaky_relu+conv32,ks3,stride1+norm,leaky_relu+conv6,ks1,stride1")
ARCHS = {"small": SMALL, "default": U.default_feature(6), "deep2": DEEP2}
OP_CONV = 1     # csrc/graph.hpp: OpKind


# the shapes at which the switch tests of test_gpu_parity.py show each epilogue live
@pytest.mark.parametrize("arch,n", [
    ("small", 16),      # k_mfma_conv_z16's statistics rows
    ("small", 64),      # k_s2_scatter's rows, accumulating into the skip gradient
    ("default", 64),    # k_mfma_conv_small's rows at its 16^3 level
    ("default", 32),    # the deep kernels' whole norm backward at the 4^3 .. 1^3 levels
    ("deep2", 8),       # deep conv dgrad (27 taps, one accumulating) and conv_trans dgrad
    ("deep2", 16),      # the short deep kinds only: conv_trans dgrad, stride-2 dgrad
])
def test_backward_cut_at_every_op_boundary_equals_one_backward(arch, n):
    m = U.UNet3d(1, 6, ARCHS[arch], device=DEV, dtype="bf16", seed=0)
    x, t = U.SyntheticVolumes(1, 6, (n, n, n), DEV)(0)
    m.train()
    plan = m.plan_for((n, n, n))
    ws = m._workspace(plan)
    _, l1, gouts = m._run_forward_loss(plan, ws, x, t, True, True, True, 0)
    m._run_backward(plan, ws, gouts)
    g1 = m.flat_grads.clone()
    m.flat_grads.zero_()
    _, l2, gouts = m._run_forward_loss(plan, ws, x, t, True, True, True, 0)
    nops = len(plan.ops())
    op_hi = 1 << 30
    for op_lo in range(nops - 1, -1, -1):
        m._run_backward_part(plan, ws, gouts, op_hi, op_lo)
        op_hi = op_lo
    torch.cuda.synchronize()
    assert torch.equal(l1, l2)
    assert torch.equal(m.flat_grads, g1)


def test_two_workspaces_on_one_plan_with_their_backward_parts_interleaved():
    """A.forward, B.forward, A.part1, B.part1, A.part2, B.part2 on one stream, through the C ABI: each workspace's gradients equal
    those of its own uninterleaved backward.  The cut is at the last 3x3x3 conv: its dgrad (part 1) leaves statistics rows in the
    workspace for the view backward of its source (part 2), while the other workspace's part runs in between."""
    n = 16
    m = U.UNet3d(1, 6, SMALL, device=DEV, dtype="bf16", seed=0)
    m.train()
    plan = m.plan_for((n, n, n))
    ops = plan.ops()
    cut = max(i for i, o in enumerate(ops) if o["kind"] == OP_CONV and o["ks"] == 3)
    gen = torch.Generator(device=DEV)
    gen.manual_seed(7)
    gouts = [torch.randn(s, generator=gen, device=DEV, dtype=torch.float32) if s[1] > 0 else None for s in plan.output_shapes]
    go = E.ptr_array([g.data_ptr() if g is not None else None for g in gouts])
    xs = [U.SyntheticVolumes(1, 6, (n, n, n), DEV)(k)[0].contiguous() for k in range(2)]
    assert not torch.equal(xs[0], xs[1])
    wss = [torch.empty(plan.workspace_bytes, dtype=torch.uint8, device=DEV) for _ in range(2)]
    outs = [[torch.empty(s, dtype=torch.float32, device=DEV) if s[1] > 0 else None for s in plan.output_shapes] for _ in range(2)]
    ops_ptr = [E.ptr_array([o.data_ptr() if o is not None else None for o in oo]) for oo in outs]
    st = E.stream(torch.device(DEV))

    def forward(k):
        E.check(E.lib.unet_forward(plan.handle, m._pp, m._bp, xs[k].data_ptr(), ops_ptr[k], wss[k].data_ptr(), 1, st))

    def grads():
        flat = [torch.zeros_like(m.flat_grads) for _ in range(2)]
        return flat, [m.grad_pointers(f) for f in flat]

    ref, ref_p = grads()
    for k in range(2):
        forward(k)
        E.check(E.lib.unet_backward(plan.handle, m._pp, go, ref_p[k], None, wss[k].data_ptr(), st))
    got, got_p = grads()
    forward(0)
    forward(1)
    for op_hi, op_lo in ((1 << 30, cut), (cut, 0)):
        for k in range(2):
            E.check(E.lib.unet_backward_part(plan.handle, m._pp, go, got_p[k], None, wss[k].data_ptr(), op_hi, op_lo, st))
    torch.cuda.synchronize()
    assert not torch.equal(ref[0], ref[1])
    for k in range(2):
        assert torch.equal(got[k], ref[k]), "workspace %d" % k
