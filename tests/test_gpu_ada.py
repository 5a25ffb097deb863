"""ADA augmentation on the GPU (csrc/ada.hip through gan2shape_amd.augment): forward and image gradient against the
reference's float64 results on every case of tests/golden/ada.npz, the adjoint identity, the public contract of
`augment`, and run-to-run identity of the forward.  Bounds: ada_cases.py."""
import numpy as np
import pytest
import torch

import ada_cases as ac

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def aug():
    import gan2shape_amd  # noqa: F401
    from gan2shape_amd import augment, lib
    lib.load()
    return augment


@pytest.mark.parametrize("name", ac.names())
def test_kernels_match_the_float64_golden(aug, name):
    c = ac.case(name)
    y, gx = ac.run(aug, c, c["x"].cuda().requires_grad_(True))
    assert y.is_cuda and y.dtype == torch.float32 and y.shape == c["x"].shape
    ey, eg = float((y.cpu().double() - c["y"]).abs().max()), float((gx.cpu().double() - c["gx"]).abs().max())
    print(name, "kernel error / e32: y", ey / c["e32_y"], "gx", eg / c["e32_gx"])
    assert ey <= ac.E32_MULTIPLE * c["e32_y"], (ey, c["e32_y"])
    assert eg <= ac.E32_MULTIPLE * c["e32_gx"], (eg, c["e32_gx"])


@pytest.mark.parametrize("name", ["rot30", "pad_clamp", "batch3"])
def test_backward_is_the_adjoint_of_the_forward(aug, name):
    """<L x, y> = <x, L^T y> for the linear part L of the map (the colour offset is A(0), exact in the kernel).
    Bound: each side carries at most E32_MULTIPLE * e32 of error per element (x is drawn no larger than the case's
    own image, which is what e32 was measured on), so the two inner products differ by at most
    E32_MULTIPLE * (e32_y |y|_1 + e32_gx |x|_1)."""
    c = ac.case(name)
    g = torch.Generator().manual_seed(1)
    x = (torch.rand(c["x"].shape, generator=g) * 2 - 1) * float(c["x"].abs().max()) * 0.75
    y = torch.randn(c["x"].shape, generator=g)
    xd = x.cuda().requires_grad_(True)
    run = (lambda t: aug.random_apply_affine(t, 1.0, c["G"])[0]) if c["C"] is None else \
        (lambda t: aug.augment(t, 0.5, (c["G"], c["C"]))[0])
    ax = run(xd)
    aty, = torch.autograd.grad(ax, xd, y.cuda())
    lx = (ax.detach() - run(torch.zeros_like(xd))).cpu().double()
    lhs, rhs = float((lx * y.double()).sum()), float((x.double() * aty.cpu().double()).sum())
    bound = ac.E32_MULTIPLE * (c["e32_y"] * float(y.abs().sum()) + c["e32_gx"] * float(x.abs().sum()))
    print(name, "<Lx,y>", lhs, "<x,L^T y>", rhs, "difference", abs(lhs - rhs), "bound", bound,
          "relative", abs(lhs - rhs) / float(lx.norm() * y.double().norm()))
    assert abs(lhs - rhs) <= bound


def test_augment_contract_on_the_gpu(aug):
    c = ac.case("batch3")
    x = c["x"].cuda().requires_grad_(True)
    y, (G, C) = aug.augment(x, 0.5, (c["G"], c["C"]))
    assert G is c["G"] and C is c["C"]
    assert float((y.detach().cpu().double() - c["y"]).abs().max()) <= ac.E32_MULTIPLE * c["e32_y"]
    y.backward(c["gy"].cuda())
    assert float((x.grad.cpu().double() - c["gx"]).abs().max()) <= ac.E32_MULTIPLE * c["e32_gx"]
    # sampled colour: the stored seed gives the stored C and the stored image
    s = ac.case("pad_clamp")
    torch.manual_seed(s["seed"])
    y, (G, C) = aug.augment(s["x"].cuda(), s["p"], (s["G"], None))
    assert torch.equal(C, s["C"]) and not C.is_cuda
    assert float((y.cpu().double() - s["y"]).abs().max()) <= ac.E32_MULTIPLE * s["e32_y"]
    # nothing given: shapes and finiteness
    y, (G, C) = aug.augment(s["x"].cuda(), 0.9)
    assert y.shape == s["x"].shape and G.shape == (1, 3, 3) and C.shape == (1, 4, 4) and bool(torch.isfinite(y).all())


def test_double_backward_raises(aug):
    c = ac.case("rot30")
    x = c["x"].cuda().requires_grad_(True)
    y, _ = aug.augment(x, 0.5, (c["G"], c["C"]))
    g, = torch.autograd.grad(y.square().sum(), x, create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable"):
        g.square().sum().backward()


def test_backward_refuses_deterministic_mode(aug):
    from gan2shape_amd import lib
    c = ac.case("gray")
    x = c["x"].cuda().requires_grad_(True)
    y, _ = aug.random_apply_affine(x, 1.0, c["G"])
    prev = lib.set_deterministic(True)
    try:
        with pytest.raises(lib.G2SError, match="deterministic"):
            y.backward(c["gy"].cuda())
    finally:
        lib.set_deterministic(prev)


@pytest.mark.parametrize("name", ["batch3", "tiles40x24"])
def test_forward_is_bit_identical_from_run_to_run(aug, name):
    c = ac.case(name)
    x = c["x"].cuda()
    run = (lambda: aug.random_apply_affine(x, 1.0, c["G"])[0]) if c["C"] is None else \
        (lambda: aug.augment(x, 0.5, (c["G"], c["C"]))[0])
    a, b = run(), run()
    assert np.array_equal(a.cpu().numpy(), b.cpu().numpy())
