"""ADA augmentation benchmark: gan2shape_amd.augment.augment (two launches each way, csrc/ada.hip)
against the composed route on the same commit — F.pad(reflect), the project's upfirdn2d (two 12-tap up passes),
F.affine_grid + F.grid_sample at double resolution, two 12-tap down passes, the matmul colour step — for the SAME
matrices, at [8, 3, 128, 128] and [32, 3, 256, 256], forward and forward + backward.
Per route: HIP-event pairs around one Python call after a warm-up, the two routes in ALTERNATING rounds so that clock
and cache state are shared; reported is the median over all samples and the lowest and highest per-round median.
Launches come from the torch profiler.  Writes profiles/augment_g128.json.

    python tools/bench_augment.py [--quick] [--out profiles/augment_g128.json]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import torch.nn.functional as F

import gan2shape_amd  # noqa
from gan2shape_amd import augment as aug
from gan2shape_amd import lib
from gan2shape_amd.op.upfirdn2d import _Resample

from bench_manipulate import alternating
from bench_sweep import launches


def composed(img, G, C, k_row, k_col, kf_row, kf_col):
    """The reference's chain on the project's own ops, with the pads and the warp matrix of the fused route."""
    B, ch, H, W = img.shape
    g_host = G.float().cpu()
    x0, x1, y0, y1 = pads = aug._pads(g_host, H, W, 12)
    warp = aug._warp_matrix(g_host, pads, H, W).to(img.device)
    x = F.pad(img, (x0, x1, y0, y1), mode="reflect")
    x = _Resample.apply(x, k_row, (2, 1), (1, 1), (6, 5, 0, 0), None)
    x = _Resample.apply(x, k_col, (1, 2), (1, 1), (0, 0, 6, 5), None)
    grid = F.affine_grid(warp, (B, ch, 2 * (H + 6), 2 * (W + 6)), align_corners=False)
    a = F.grid_sample(x, grid, mode="bilinear", padding_mode="zeros", align_corners=False)
    a = _Resample.apply(a, kf_row, (1, 1), (2, 1), (-1, -1, 0, 0), None)
    a = _Resample.apply(a, kf_col, (1, 1), (1, 2), (0, 0, -1, -1), None)
    m = C.to(img)
    y = a.permute(0, 2, 3, 1) @ m[:, :3, :3].transpose(1, 2).view(B, 1, 3, 3) + m[:, :3, 3].view(B, 1, 1, 3)
    return y.permute(0, 3, 1, 2)


def main():
    quick = "--quick" in sys.argv
    path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(
        ROOT, "profiles", "augment_g128.json")
    lib.load()
    dev = torch.device("cuda")
    k = torch.tensor(aug.SYM6, device=dev)
    ks = (k.view(1, -1).contiguous(), k.view(-1, 1).contiguous(),
          k.flip(0).view(1, -1).contiguous(), k.flip(0).view(-1, 1).contiguous())
    rounds, n = (3, 5) if quick else (5, 20)
    result = dict(rounds=rounds, samples_per_round=n, p=0.8, shapes=[])
    for shape in ((8, 3, 128, 128), (32, 3, 256, 256)):
        B, _, H, W = shape
        torch.manual_seed(B)
        G = torch.inverse(aug.sample_affine(0.8, B, H, W))
        C = aug.sample_color(0.8, B)
        img = torch.randn(shape, device=dev).requires_grad_(True)
        gy = torch.randn(shape, device=dev)

        def fused_fwd():
            with torch.no_grad():
                return aug.augment(img, 0.8, (G, C))[0]

        def composed_fwd():
            with torch.no_grad():
                return composed(img, G, C, *ks)

        def fused_fwd_bwd():
            return torch.autograd.grad(aug.augment(img, 0.8, (G, C))[0], img, gy)[0]

        def composed_fwd_bwd():
            return torch.autograd.grad(composed(img, G, C, *ks), img, gy)[0]
        dy = float((fused_fwd() - composed_fwd()).abs().max())
        dg = float((fused_fwd_bwd() - composed_fwd_bwd()).abs().max())
        row = dict(shape=list(shape), pads=list(aug._pads(G, H, W, 12)), max_abs_diff_forward=dy, max_abs_diff_grad=dg)
        for label, routes in (("forward", dict(fused=fused_fwd, composed=composed_fwd)),
                              ("forward_backward", dict(fused=fused_fwd_bwd, composed=composed_fwd_bwd))):
            t = alternating(routes, rounds, n)
            row[label] = dict({name: dict(v, launches=launches(routes[name])) for name, v in t.items()},
                              composed_over_fused=t["composed"]["median_ms"] / t["fused"]["median_ms"])
        result["shapes"].append(row)
        print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
