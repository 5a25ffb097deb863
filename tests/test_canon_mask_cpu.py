"""Renderer.canon_mask on the CPU (the torch composition: the specification of g2s_canon_mask) against the float64
fixture tests/golden/canon_mask.npz, which tests/golden/make_canon_mask_golden.py composed from the reference's own
Renderer parts.

Bounds.  The float64 route repeats the fixture's operations in the same precision and order, but for the pixel rays:
the reference multiplies (u, v, 1) K^-T by the depth per call, this package keeps the product (u, v, 1) K^-T and
multiplies it by the depth — the same two operations.  What is left is the rounding of a float64 chain of about
twenty operations on numbers of size <= S, read through a mask of slope <= 1 per pixel: 1e-12 leaves three orders
of magnitude over 20 x S x 2^-53 = 7e-14.  The float32 route is held to the fixture's own float32 result the same
way (it is the same composition), with the bound the GPU test uses: 4 x the float32 composition's error, floor one
float32 ulp of 1.0."""
import numpy as np
import pytest
import torch

import canon_mask_cases as cc

EPS32 = float(np.finfo(np.float32).eps)


@pytest.fixture(scope="module")
def fixture(golden):
    return golden("canon_mask")


def _run(g, name, dtype):
    S = cc.CASES[name][0]
    r = cc.package_renderer(S, "cpu", dtype)
    depth = torch.tensor(g[f"{name}.depth"]).to(dtype)
    return cc.run_package(r, torch.tensor(g[f"{name}.view"]), depth, torch.tensor(g[f"{name}.mask"]))


def test_fixture_holds_the_cases_of_the_module(fixture):
    for name, (S, views, _kind, shared) in cc.CASES.items():
        B = len(views)
        assert fixture[f"{name}.depth"].shape == (B, S, S) and fixture[f"{name}.view"].shape == (B, 6)
        assert fixture[f"{name}.mask"].shape == (1 if shared else B, 1, S, S)
        assert fixture[f"{name}.out"].dtype == np.float64 and fixture[f"{name}.out32"].dtype == np.float32
        np.testing.assert_array_equal(fixture[f"{name}.depth"], cc.depth_of(name).numpy())
        np.testing.assert_array_equal(fixture[f"{name}.mask"], cc.mask_of(name).numpy())
    sizes = {c[0] for c in cc.CASES.values()}
    batches = {len(c[1]) for c in cc.CASES.values()}
    assert sizes == {16, 32} and batches == {1, 2, 3}
    assert {v for c in cc.CASES.values() for v in c[1]} == set(cc.VIEWS)
    assert {c[2] for c in cc.CASES.values()} == {"disc", "rect", "soft", "ones"}
    assert any(c[3] and len(c[1]) == 3 for c in cc.CASES.values())


@pytest.mark.parametrize("name", list(cc.CASES))
def test_cpu_route_reproduces_the_float64_fixture(fixture, name):
    out = _run(fixture, name, torch.float64)
    S, views, _, _ = cc.CASES[name]
    assert out.dtype == torch.float64 and tuple(out.shape) == (len(views), 1, S, S) == fixture[f"{name}.out"].shape
    err = cc.max_err(out.numpy(), fixture[f"{name}.out"])
    print(f"[canon_mask cpu f64] {name}: max |err| {err:.3e}")
    assert err <= 1e-12


@pytest.mark.parametrize("name", list(cc.CASES))
def test_cpu_float32_route_is_within_the_float32_bound(fixture, name):
    out = _run(fixture, name, torch.float32)
    assert out.dtype == torch.float32
    e32 = cc.max_err(fixture[f"{name}.out32"], fixture[f"{name}.out"])
    err = cc.max_err(out.numpy(), fixture[f"{name}.out"])
    print(f"[canon_mask cpu f32] {name}: max |err| {err:.3e}, composition's own {e32:.3e}")
    assert err <= max(4 * e32, EPS32)


@pytest.mark.parametrize("name", [n for n, c in cc.CASES.items() if set(c[1]) == {"identity"}])
def test_identity_view_returns_the_mask(fixture, name):
    out = _run(fixture, name, torch.float64)
    mask = torch.tensor(fixture[f"{name}.mask"]).expand_as(out)
    assert cc.max_err(out.numpy(), mask.numpy()) <= 1e-12


def test_broadcast_mask_and_shapes(fixture):
    name = "broadcast_disc_s32_b3"
    S, views, _, shared = cc.CASES[name]
    assert shared and fixture[f"{name}.mask"].shape[0] == 1
    out = _run(fixture, name, torch.float64)
    assert tuple(out.shape) == (3, 1, S, S)
    # the shared mask gives what three copies of it give
    r = cc.package_renderer(S, "cpu", torch.float64)
    depth = torch.tensor(fixture[f"{name}.depth"])
    full = cc.run_package(r, torch.tensor(fixture[f"{name}.view"]), depth,
                          torch.tensor(fixture[f"{name}.mask"]).expand(3, 1, S, S).contiguous())
    assert torch.equal(out, full)
    with pytest.raises(ValueError):
        r.canon_mask(depth, torch.ones(2, 1, S, S))
    with pytest.raises(ValueError):
        r.canon_mask(depth, torch.ones(3, 1, S, S + 1))


def test_result_carries_no_gradient(fixture):
    name = "small_disc_s32_b2"
    S = cc.CASES[name][0]
    r = cc.package_renderer(S, "cpu")
    depth = torch.tensor(fixture[f"{name}.depth"]).float().requires_grad_(True)
    view = torch.tensor(fixture[f"{name}.view"]).float().requires_grad_(True)
    mask = torch.tensor(fixture[f"{name}.mask"]).float().requires_grad_(True)
    r.set_transform_matrices(view)
    assert r.rot_mat.requires_grad
    out = r.canon_mask(depth, mask)
    assert out.grad_fn is None and not out.requires_grad
