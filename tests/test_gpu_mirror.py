"""g2s_mirror_pair (csrc/mirror.hip, fused_geometry.mirror_pair) alone: the symmetry pair of a flipped step.
x [N,C,H,W], repeat -> y [2 N repeat, C, H, W]: `repeat` copies of every sample, then `repeat` copies of its mirror
along W.  The torch composition cat / flip / repeat_interleave is the specification."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# (N, C, H, W, repeat): one float4; W no multiple of 4 (scalar path); two samples, three channels; more than one
# workgroup's worth of rows with repeat > 1; repeat > 1 with N > 1
SHAPES = [(1, 1, 1, 4, 1), (1, 3, 2, 6, 1), (2, 3, 3, 8, 1), (1, 1, 5, 128, 3), (2, 3, 4, 12, 2)]
EPS32 = float(np.finfo(np.float32).eps)


def _ref(x, repeat):
    return torch.cat([x.repeat_interleave(repeat, 0), x.flip(-1).repeat_interleave(repeat, 0)], 0)


def _inputs(N, C, H, W, seed, offset=False):
    g = torch.Generator().manual_seed(seed)
    if not offset:
        return torch.randn(N, C, H, W, generator=g).cuda()
    # a view that starts one float into its storage: contiguous, W % 4 == 0, but not 16-byte aligned
    flat = torch.randn(N * C * H * W + 1, generator=g).cuda()
    x = flat[1:].view(N, C, H, W)
    assert x.is_contiguous() and x.data_ptr() % 16 == 4
    return x


def _run(x, repeat, gy=None):
    """(y, gx) of the kernel for a single tensor (the depth slot of the launch)."""
    from gan2shape_amd.fused_geometry import mirror_pair
    xr = x.detach().requires_grad_(True)
    y, none = mirror_pair(xr, None, repeat)
    assert none is None
    if gy is None:
        return y.detach(), None
    (gx,) = torch.autograd.grad(y, xr, gy)
    return y.detach(), gx


CASES = [(s, False) for s in SHAPES] + [((2, 3, 3, 8, 2), True)]


@pytest.mark.parametrize("shape,offset", CASES)
def test_mirror_pair_forward_and_backward(shape, offset):
    N, C, H, W, repeat = shape
    x = _inputs(N, C, H, W, 3, offset)
    gy = torch.randn(2 * N * repeat, C, H, W, generator=torch.Generator().manual_seed(4)).cuda()
    if offset:      # the incoming gradient off the 16-byte grid too
        flat = torch.empty(gy.numel() + 1, device="cuda")
        flat[1:].copy_(gy.reshape(-1))
        gy = flat[1:].view_as(gy)
    y, gx = _run(x, repeat, gy)
    assert y.shape == (2 * N * repeat, C, H, W)
    assert torch.equal(y, _ref(x, repeat))                        # a copy: exact
    ga, gb = gy[:N * repeat], gy[N * repeat:]
    if repeat == 1:
        assert torch.equal(gx, ga + gb.flip(-1))                  # one float32 addition
    else:
        terms = torch.cat([ga.double().view(N, repeat, C, H, W), gb.flip(-1).double().view(N, repeat, C, H, W)], 1)
        exact, mag = terms.sum(1), terms.abs().sum(1)
        err = (gx.double() - exact).abs()
        bound = 2 * repeat * EPS32 * mag
        print(f"[mirror {shape}] backward: max err / bound = {float((err / bound).max()):.3f}")
        assert bool((err <= bound).all())
    y2, gx2 = _run(x, repeat, gy)                                 # bit-reproducible
    assert torch.equal(y, y2) and torch.equal(gx, gx2)


@pytest.mark.parametrize("shape", [(1, 3, 2, 6, 1), (2, 3, 3, 8, 1), (1, 1, 5, 128, 3), (2, 3, 4, 12, 2)])
def test_mirror_pair_two_tensor_launch_equals_two_single_launches(shape):
    """Depth [N,H,W] and albedo [N,C,H,W] through one launch each way = each through a launch of its own."""
    from gan2shape_amd.fused_geometry import mirror_pair
    N, C, H, W, repeat = shape
    depth = _inputs(N, 1, H, W, 5)[:, 0].contiguous().requires_grad_(True)
    albedo = _inputs(N, C, H, W, 6).requires_grad_(True)
    d2, a2 = mirror_pair(depth, albedo, repeat)
    assert d2.shape == (2 * N * repeat, H, W) and a2.shape == (2 * N * repeat, C, H, W)
    gd = torch.randn(d2.shape, generator=torch.Generator().manual_seed(7)).cuda()
    ga = torch.randn(a2.shape, generator=torch.Generator().manual_seed(8)).cuda()
    g_depth, g_albedo = torch.autograd.grad([d2, a2], [depth, albedo], [gd, ga])
    d_single, gd_single = _run(depth, repeat, gd)
    a_single, ga_single = _run(albedo, repeat, ga)
    assert torch.equal(d2.detach(), d_single) and torch.equal(a2.detach(), a_single)
    assert torch.equal(g_depth, gd_single) and torch.equal(g_albedo, ga_single)
    assert torch.equal(d2.detach(), _ref(depth.detach().unsqueeze(1), repeat)[:, 0])
    # only the albedo takes part in the loss (step 1: the depth is detached): the launch runs on what is there
    d3, a3 = mirror_pair(depth.detach(), albedo, repeat)
    assert not d3.requires_grad and a3.requires_grad      # an output follows its own input
    (g_only,) = torch.autograd.grad(a3, albedo, ga)
    assert torch.equal(g_only, ga_single)


def test_mirror_pair_rejects_bad_arguments():
    from gan2shape_amd.fused_geometry import mirror_pair
    x = torch.zeros(1, 1, 2, 4, device="cuda")
    with pytest.raises(ValueError):
        mirror_pair(x, None, 0)
    with pytest.raises(ValueError):
        mirror_pair(x, torch.zeros(2, 3, 2, 4, device="cuda"), 1)
    with pytest.raises(RuntimeError):
        mirror_pair(torch.zeros(1, 1, 2, 4), None, 1)
