"""g2s_canon_mask (csrc/canon_mask.hip, Renderer.canon_mask on CUDA float32) against the float64 fixture
tests/golden/canon_mask.npz — the reference's own Renderer parts composed as DESIGN.md §4.25 defines the canonical
mask (tests/golden/make_canon_mask_golden.py).

Bound: the kernel's maximum absolute error against the float64 result stays within 4 x the error of the reference's
own float32 composition against that result (`<case>.out32`; the multiple the ADA tests use), floor one float32 ulp
of 1.0 for a case the composition gets exactly.  Bilinear sampling is continuous in the grid position, so there is
no outlier allowance: every element is held to the bound."""
import numpy as np
import pytest
import torch

import canon_mask_cases as cc

pytestmark = pytest.mark.gpu

MULTIPLE = 4
EPS32 = float(np.finfo(np.float32).eps)


@pytest.fixture(scope="module")
def fixture(golden):
    return golden("canon_mask")


def _run(g, name, fused=True):
    S = cc.CASES[name][0]
    r = cc.package_renderer(S, "cuda")
    r.fused = fused
    depth = torch.tensor(g[f"{name}.depth"]).float().cuda()
    return cc.run_package(r, torch.tensor(g[f"{name}.view"]), depth, torch.tensor(g[f"{name}.mask"]))


def test_symbol_is_bound():
    from gan2shape_amd import lib
    assert "g2s_canon_mask" in lib.SIGNATURES
    assert lib.load().g2s_canon_mask is not None


@pytest.mark.parametrize("name", list(cc.CASES))
def test_kernel_vs_float64_fixture(fixture, name):
    ref = fixture[f"{name}.out"]
    e32 = cc.max_err(fixture[f"{name}.out32"], ref)
    out = _run(fixture, name)
    assert out.dtype == torch.float32 and tuple(out.shape) == ref.shape and out.is_cuda and out.grad_fn is None
    err = cc.max_err(out.cpu().numpy(), ref)
    composed = cc.max_err(_run(fixture, name, fused=False).cpu().numpy(), ref)
    print(f"[canon_mask gpu] {name}: kernel max |err| {err:.3e}, the package's composed route {composed:.3e}, "
          f"the reference's float32 composition {e32:.3e}, bound {max(MULTIPLE * e32, EPS32):.3e}")
    assert err <= max(MULTIPLE * e32, EPS32)


@pytest.mark.parametrize("name", ["yaw60_ones_s32_b3", "broadcast_disc_s32_b3"])
def test_two_calls_are_bit_identical(fixture, name):
    assert torch.equal(_run(fixture, name), _run(fixture, name))


def test_shared_mask_equals_its_copies_and_bad_shapes_are_refused(fixture):
    name = "broadcast_disc_s32_b3"
    S = cc.CASES[name][0]
    r = cc.package_renderer(S, "cuda")
    depth = torch.tensor(fixture[f"{name}.depth"]).float().cuda()
    view, mask = torch.tensor(fixture[f"{name}.view"]), torch.tensor(fixture[f"{name}.mask"])
    shared = cc.run_package(r, view, depth, mask)
    full = cc.run_package(r, view, depth, mask.expand(3, 1, S, S).contiguous())
    assert torch.equal(shared, full)
    with pytest.raises(ValueError):
        r.canon_mask(depth, torch.ones(2, 1, S, S, device="cuda"))
    r.set_transform_matrices(view[:2].float().cuda())       # two poses for three depth maps
    with pytest.raises(ValueError):
        r.canon_mask(depth, mask.float().cuda())


def test_kernel_records_into_a_graph(fixture):
    """Stateless and on the caller's stream: a captured launch replays onto new inputs."""
    name = "small_disc_s32_b2"
    S = cc.CASES[name][0]
    r = cc.package_renderer(S, "cuda")
    depth = torch.tensor(fixture[f"{name}.depth"]).float().cuda()
    mask = torch.tensor(fixture[f"{name}.mask"]).float().cuda()
    r.set_transform_matrices(torch.tensor(fixture[f"{name}.view"]).float().cuda())
    want = r.canon_mask(depth, mask.flip(3).contiguous())
    static = mask.clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        r.canon_mask(depth, static)      # warm-up: library handle, ray constants
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = r.canon_mask(depth, static)
    static.copy_(mask.flip(3))
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, want)
