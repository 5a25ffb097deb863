"""-m gpu: the one-launch Adam step (csrc/adam.hip behind optim.Adam) on its scalar path and at chunk borders.

The kernel updates 16 bytes per lane when the parameter, its gradient and both moments are 16-byte aligned, and one
float at a time otherwise and for the last n % 4 elements; a block takes a chunk of 16384 elements, and the block of a
tensor that finishes last advances the tensor's device step counter.  test_one_launch_adam_equals_torch_adam only
sees fresh allocations, which are aligned; networks.pair_parameters moves parameters into shared storage, where they
start at any float.

Each layout runs every size as one optimiser (one launch per step over all tensors) for 3 steps against
torch.optim.Adam in float64 on the same float32 start values and gradients, within the older test's tolerance.  Every
parameter and gradient lives inside a buffer with 8 sentinel floats on each side, which must come back unchanged;
one multi-chunk tensor gets no gradient on the second step, and every tensor's step counter must equal the steps it
took (with its arrival ticket back at 0)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SIZES = [1, 3, 4, 5, 1023, 16383, 16384, 16385, 32775]     # vector tail 0..3, below / at / above one chunk, 3 chunks
STEPS, SKIPPED = 3, (16385, 1)                              # the tensor of 16385 elements has no gradient on step 1
KW = dict(lr=1e-2, betas=(0.9, 0.999), weight_decay=5e-4)
PAD, SENTINEL = 8, -77.25
# layout -> (parameter misaligned, gradient misaligned)
LAYOUTS = dict(aligned=(False, False), param_offset=(True, False), grad_offset=(False, True))


def guarded(values, misaligned):
    """`values` on the device inside a buffer of sentinels: (buffer, view).  The view starts 8 floats into the
    buffer (16-byte aligned) or 9 (one float past a 16-byte boundary)."""
    start = PAD + (1 if misaligned else 0)
    buf = torch.full((start + values.numel() + PAD,), SENTINEL, dtype=torch.float32, device="cuda")
    view = buf[start:start + values.numel()]
    view.copy_(values)
    assert view.data_ptr() % 16 == (4 if misaligned else 0)
    return buf, view


def sentinels_intact(buf, view):
    start = (view.data_ptr() - buf.data_ptr()) // 4
    out = torch.cat([buf[:start], buf[start + view.numel():]])
    return out.numel() >= 2 * PAD and bool((out == SENTINEL).all())


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_adam_paths_equal_torch_adam_float64(layout):
    import gan2shape_amd  # noqa: F401
    from gan2shape_amd.optim import Adam
    p_off, g_off = LAYOUTS[layout]
    gen = torch.Generator().manual_seed(17)
    start = [torch.randn(n, generator=gen) for n in SIZES]
    bufs = [guarded(s, p_off) for s in start]
    ours = [view.detach().requires_grad_(True) for _, view in bufs]
    ref = [s.double().requires_grad_(True) for s in start]
    for a, (_, view) in zip(ours, bufs):
        assert a.data_ptr() == view.data_ptr() and a.is_leaf
    o_ours, o_ref = Adam(ours, **KW), torch.optim.Adam(ref, **KW)
    gbufs, taken = [], [0] * len(SIZES)
    for it in range(STEPS):
        for i, (a, b) in enumerate(zip(ours, ref)):
            if (SIZES[i], it) == SKIPPED:          # torch skips a tensor without a gradient, count included
                a.grad = b.grad = None
                continue
            g = torch.randn(SIZES[i], generator=gen) * (1 + it)
            gbuf, gview = guarded(g, g_off)
            gbufs.append((gbuf, gview))
            a.grad, b.grad = gview, g.double()
            taken[i] += 1
        o_ours.step()
        o_ref.step()
    torch.cuda.synchronize()
    assert sorted(set(taken)) == [STEPS - 1, STEPS]
    for i, (a, b) in enumerate(zip(ours, ref)):
        np.testing.assert_allclose(a.detach().cpu().numpy(), b.detach().numpy(), rtol=2e-5, atol=2e-6,
                                   err_msg=f"{layout}: parameter of {SIZES[i]} elements")
        st = o_ours.state[a]
        assert float(st["step"]) == taken[i] == float(o_ref.state[b]["step"]), (layout, SIZES[i], float(st["step"]))
        assert int(st["ticket"]) == 0, (layout, SIZES[i])
    for i, (buf, view) in enumerate(bufs):
        assert sentinels_intact(buf, view), f"{layout}: sentinels around the parameter of {SIZES[i]} elements"
    for buf, view in gbufs:
        assert sentinels_intact(buf, view), f"{layout}: sentinels around a gradient of {view.numel()} elements"
