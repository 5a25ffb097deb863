"""Depth and normal accuracy of a recovered depth against a ground-truth depth: the figures of the BFM
table of the GAN2Shape / Unsup3D papers — masked depth MAE and MSE, scale-invariant depth error (SIDE) and
mean angle deviation of the normals (MAD, degrees) — per image.

CUDA tensors go to g2s_depth_metrics (csrc/metrics.hip; include/g2s.h states the definitions): two launches
for the whole batch, no host synchronisation, bit-identical from run to run.  CPU tensors take the torch
composition of the same definitions below (`_depth_metrics_torch`), which is also the specification the kernel
is tested against.  There is no fallback on the GPU.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

from . import lib as _lib
from .renderer.renderer import EPS

METRICS = ("mae", "mse", "side", "mad")
KEYS = ("count",) + METRICS


def gt_mask_from_depth(depth_gt):
    """(B, H, W) float mask of the pixels nearer than the image's farthest value: the BFM convention that the
    farthest depth is background.  A helper for callers; `depth_metrics` never applies it by itself."""
    return (depth_gt < depth_gt.amax((1, 2), keepdim=True)).float()


def _normals_interior(rays, depth):
    """Renderer.get_normal_from_depth for the interior pixels: (B, H-2, W-2, 3)."""
    grid_3d = rays * depth.unsqueeze(-1)
    tu = grid_3d[:, 1:-1, 2:] - grid_3d[:, 1:-1, :-2]
    tv = grid_3d[:, 2:, 1:-1] - grid_3d[:, :-2, 1:-1]
    normal = torch.linalg.cross(tu, tv, dim=3)
    return normal / (((normal ** 2).sum(3, keepdim=True)) ** 0.5 + EPS)


def _depth_metrics_torch(pred, gt, mask_pred, mask_gt, rays, erode):
    """The definitions of include/g2s.h (g2s_depth_metrics) as torch ops, in the tensors' dtype.  rays (1, H, W, 3)."""
    finite = torch.isfinite(pred) & torch.isfinite(gt)
    valid = finite & (pred > 0) & (gt > 0)
    if mask_pred is not None:
        valid = valid & (mask_pred > 0.5)
    if mask_gt is not None:
        valid = valid & (mask_gt > 0.5)
    if erode:    # zero padding: outside the image is invalid
        counted = F.avg_pool2d(valid.to(pred.dtype).unsqueeze(1), 3, 1, 1).squeeze(1) > 0.99
    else:
        counted = valid
    stencil = torch.zeros_like(valid)
    stencil[:, 1:-1, 1:-1] = finite[:, 1:-1, 2:] & finite[:, 1:-1, :-2] & finite[:, 2:, 1:-1] & finite[:, :-2, 1:-1]
    with_normal = counted & stencil
    zero = torch.zeros((), dtype=pred.dtype, device=pred.device)

    def masked_sum(v, m):
        return torch.where(m, v, zero).sum((1, 2))
    n = counted.sum((1, 2)).to(pred.dtype)
    diff = pred - gt
    mae = masked_sum(diff.abs(), counted) / n
    mse = masked_sum(diff * diff, counted) / n
    delta = torch.log(pred) - torch.log(gt)
    centred = delta - (masked_sum(delta, counted) / n).view(-1, 1, 1)      # centre before squaring
    side = (masked_sum(centred * centred, counted) / n).clamp(min=0).sqrt()
    n_p, n_g = _normals_interior(rays, pred), _normals_interior(rays, gt)
    # the angle as atan2(|n_p x n_g|, n_p . n_g): independent of the EPS that leaves the normals shorter than 1
    angle = torch.atan2(torch.linalg.cross(n_p, n_g, dim=3).pow(2).sum(3).sqrt(), (n_p * n_g).sum(3))
    angle = F.pad(angle, (1, 1, 1, 1))
    mad = masked_sum(angle, with_normal) / with_normal.sum((1, 2)).to(pred.dtype) * (180.0 / math.pi)
    nan = torch.full_like(n, float("nan"))
    empty = n == 0
    return {"count": n.float(), "mae": torch.where(empty, nan, mae).float(), "mse": torch.where(empty, nan, mse).float(),
            "side": torch.where(empty, nan, side).float(), "mad": torch.where(empty, nan, mad).float()}


def _workspace(device, nbytes):
    """Scratch of one call, from the renderer plugin's per-call allocation (see its docstring: a free-list hit
    under the caching allocator, a block of the graph's pool during a capture)."""
    from .plugins.neural_renderer import _workspace as alloc
    return alloc(device, max(int(nbytes), 8))


def _as_bhw(t, shape, what):
    if t is None:
        return None
    if t.dim() == 4 and t.shape[1] == 1:
        t = t[:, 0]
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"depth_metrics: {what} has shape {tuple(t.shape)}, expected {tuple(shape)} "
                         f"(or with a channel axis of 1)")
    return t


def depth_metrics(depth_pred, depth_gt, mask_pred=None, mask_gt=None, *, renderer, erode=True):
    """Per-image accuracy of `depth_pred` against `depth_gt`, both (B, H, W); masks (B, H, W) or (B, 1, H, W),
    counted where > 0.5; NaN or non-positive depths are "outside the object".  erode: a pixel counts only if its
    whole 3x3 neighbourhood is valid (the papers' evaluation).  The pixel rays are `renderer`'s — the same
    intrinsics as training, `downscale_K` included.

    Returns {"count", "mae", "mse", "side", "mad"}: (B,) float32 tensors on the inputs' device; an image without a
    counted pixel has count 0 and NaN metrics."""
    if depth_pred.dim() != 3 or depth_pred.shape != depth_gt.shape:
        raise ValueError(f"depth_metrics: depths must be (B, H, W) of one shape, got {tuple(depth_pred.shape)} "
                         f"and {tuple(depth_gt.shape)}")
    B, H, W = depth_pred.shape
    if H < 3 or W < 3:
        raise ValueError("depth_metrics: H and W must be at least 3")
    device = depth_pred.device
    tensors = [depth_pred, depth_gt, _as_bhw(mask_pred, depth_pred.shape, "mask_pred"),
               _as_bhw(mask_gt, depth_pred.shape, "mask_gt")]
    if any(t is not None and t.device != device for t in tensors):
        raise ValueError("depth_metrics: depths and masks must be on one device")
    if B == 0:
        return {k: torch.empty(0, dtype=torch.float32, device=device) for k in KEYS}
    with torch.no_grad():
        tensors = [None if t is None else t.detach().to(torch.float32) for t in tensors]
        rays = renderer._pixel_rays(H, W, device)
        if device.type != "cuda":
            return _depth_metrics_torch(*tensors, rays, bool(erode))
        L = _lib.load()
        pred, gt, mp, mg = [None if t is None else t.contiguous() for t in tensors]
        rays = rays.reshape(-1, 3).contiguous()
        out = torch.empty(B, 5, dtype=torch.float32, device=device)
        with torch.cuda.device(device):
            ws = _workspace(device, L.g2s_depth_metrics_workspace_bytes(B, H, W))
            _lib.check(L.g2s_depth_metrics(_lib.ptr(pred), _lib.ptr(gt), _lib.ptr(mp), _lib.ptr(mg), _lib.ptr(rays),
                                           B, H, W, int(bool(erode)), _lib.ptr(out), _lib.ptr(ws), ws.numel(),
                                           _lib.stream()))
        return {k: out[:, i] for i, k in enumerate(KEYS)}


class DepthMetrics():
    """Accumulates the per-image values of `depth_metrics` over batches; `summary()` is what a results table
    prints: mean and standard deviation over the images that had a counted pixel."""

    def __init__(self):
        self.values = {k: [] for k in KEYS}

    def update(self, metrics):
        """metrics: a dict as `depth_metrics` returns it, (B,) tensors (any device) or arrays."""
        rows = {k: np.atleast_1d(np.asarray(metrics[k].detach().cpu() if torch.is_tensor(metrics[k]) else metrics[k],
                                            dtype=np.float64)) for k in KEYS}
        if len({len(v) for v in rows.values()}) != 1:
            raise ValueError("DepthMetrics.update: the entries differ in length")
        for k in KEYS:
            self.values[k].extend(rows[k].tolist())

    def __len__(self):
        return len(self.values["count"])

    def summary(self):
        """{"mae" | "mse" | "side" | "mad": (mean, std), "images": used, "skipped": images with count == 0}, in
        float64 on the host; std is the population one (numpy's default, as the reference's loss statistics).
        An image that counts pixels but has no normal (erode off, no stencil) has a NaN mad and is left out of
        mad's two figures only."""
        count = np.asarray(self.values["count"], np.float64)
        keep = count > 0
        out = {"images": int(keep.sum()), "skipped": int((~keep).sum())}
        for k in METRICS:
            v = np.asarray(self.values[k], np.float64)[keep]
            v = v[~np.isnan(v)]
            out[k] = (float(v.mean()), float(v.std())) if v.size else (float("nan"), float("nan"))
        return out
