"""Golden vectors of the canonical object mask (Renderer.canon_mask, g2s_canon_mask): tests/golden/canon_mask.npz.

    python tests/golden/make_canon_mask_golden.py

The reference reads `use_mask` and leaves the canonical mask at None (`FIXME include use_mask bool?`,
GAN2Shape/model.py:165-172), so the oracle is composed here from the reference's OWN parts, as
make_symmetry_golden.py composes the flipped steps: its renderer/utils.get_transform_matrices, its
Renderer.get_warped_2d_grid (depth_to_3d_grid, rotate_pts, translate_pts, grid_3d_to_2d) and torch's F.grid_sample in
the torch-1.2 convention the reference relies on (align_corners=True), as DESIGN.md §4.25 defines the mask:

    canon_mask = grid_sample(mask, get_warped_2d_grid(depth), bilinear, zeros padding)

Cases, operands: tests/canon_mask_cases.py.  Every case runs once in float64 — `<case>.out`, the stored value — and
once in float32 — `<case>.out32`, the reference's own float32 result, from whose distance to the float64 value the
GPU test takes its bound.  Only data is written.
"""
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, OUT)
sys.path.insert(0, os.path.dirname(OUT))
import make_golden as mg            # noqa: E402
import canon_mask_cases as cc       # noqa: E402


def reference_renderer(S, dtype):
    """The reference's Renderer without its __init__ (it calls .cuda() and builds the external rasterizer,
    renderer.py:33-54): the attributes its geometry methods read, intrinsics in `dtype`."""
    sys.modules.setdefault("neural_renderer", types.ModuleType("neural_renderer"))
    pkg = types.ModuleType("ref_renderer_pkg")
    pkg.__path__ = [os.path.join(mg.REF, "GAN2Shape/renderer")]
    sys.modules["ref_renderer_pkg"] = pkg
    sys.modules["ref_renderer_pkg.utils"] = mg._load_by_path(
        "ref_renderer_pkg.utils", os.path.join(mg.REF, "GAN2Shape/renderer/utils.py"))
    rr = mg._load_by_path("ref_renderer_pkg.renderer", os.path.join(mg.REF, "GAN2Shape/renderer/renderer.py"))
    R = object.__new__(rr.Renderer)
    R.image_size, R.min_depth, R.max_depth = S, cc.MIN_DEPTH, cc.MAX_DEPTH
    R.rot_center_depth, R.fov = cc.ROT_CENTER, cc.FOV
    K = cc.intrinsics(S).to(dtype)
    R.K, R.inv_K = K.unsqueeze(0), torch.inverse(K).unsqueeze(0)
    return R


def compose(name, dtype):
    """-> (canon_mask (B,1,S,S), fraction of the bilinear taps that fall outside the image)."""
    S = cc.CASES[name][0]
    depth, mask, view = cc.depth_of(name).to(dtype), cc.mask_of(name).to(dtype), cc.view_of(name).to(dtype)
    # the reference builds its rotation matrices with torch.zeros of the DEFAULT dtype (renderer/utils.py:34-36)
    torch.set_default_dtype(dtype)
    try:
        R = reference_renderer(S, dtype)
        R.set_transform_matrices(view)
        grid = R.get_warped_2d_grid(depth)
        with mg._torch12_grid_sample():
            out = F.grid_sample(mask.expand(len(depth), 1, S, S), grid, mode='bilinear', padding_mode='zeros')
    finally:
        torch.set_default_dtype(torch.float32)
    px = (grid + 1) / 2 * (S - 1)
    outside = ((px < 0) | (px > S - 1)).any(-1).double().mean()
    return out, float(outside)


def main():
    out = {}
    for name in cc.CASES:
        v64, outside = compose(name, torch.float64)
        v32, _ = compose(name, torch.float32)
        assert v64.dtype == torch.float64 and v32.dtype == torch.float32
        out[f"{name}.depth"], out[f"{name}.mask"], out[f"{name}.view"] = (
            cc.depth_of(name).numpy(), cc.mask_of(name).numpy(), cc.view_of(name).numpy())
        out[f"{name}.out"], out[f"{name}.out32"] = v64.numpy(), v32.numpy()
        e32 = cc.max_err(v32.numpy(), v64.numpy())
        print(f"{name:28s} out {tuple(v64.shape)}  mean {float(v64.mean()):.3f}  samples outside {outside:.2f}  "
              f"e32 {e32:.3e}")
        views = cc.CASES[name][1]
        if all(v == "identity" for v in views):     # the identity view reproduces the mask
            assert cc.max_err(v64.numpy(), cc.mask_of(name).expand_as(v64).numpy()) < 1e-12, name
        if views == ("yaw60",):                     # the zero padding is exercised
            assert outside > 0.1, (name, outside)
    path = os.path.join(OUT, "canon_mask.npz")
    np.savez_compressed(path, **out)
    print("canon_mask.npz", os.path.getsize(path))


if __name__ == "__main__":
    main()
