"""Depth and normal accuracy of a recovered depth against a ground-truth depth: the figures of the BFM
table of the GAN2Shape / Unsup3D papers — masked depth MAE and MSE, scale-invariant depth error (SIDE) and
mean angle deviation of the normals (MAD, degrees) — per image.  And, where no ground-truth depth exists, how well
the recovered depth, albedo, view and light re-render the input: `image_metrics`, masked MAE, MSE, PSNR and SSIM of
one image against another (g2s_image_metrics, csrc/image_metrics.hip; `_image_metrics_torch` on CPU tensors).

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


def _as_bhw(t, shape, what, who="depth_metrics"):
    if t is None:
        return None
    if t.dim() == 4 and t.shape[1] == 1:
        t = t[:, 0]
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"{who}: {what} has shape {tuple(t.shape)}, expected {tuple(shape)} "
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


class _PerImageRows():
    """Accumulates per-image values (the (B,) entries of a metrics dict under `keys`) over batches."""
    keys = ()

    def __init__(self):
        self.values = {k: [] for k in self.keys}

    def update(self, metrics):
        """metrics: a dict as the metric function returns it, (B,) tensors (any device) or arrays."""
        rows = {k: np.atleast_1d(np.asarray(metrics[k].detach().cpu() if torch.is_tensor(metrics[k]) else metrics[k],
                                            dtype=np.float64)) for k in self.keys}
        if len({len(v) for v in rows.values()}) != 1:
            raise ValueError(f"{type(self).__name__}.update: the entries differ in length")
        for k in self.keys:
            self.values[k].extend(rows[k].tolist())

    def __len__(self):
        return len(self.values["count"])

    def _column(self, key, keep):
        return np.asarray(self.values[key], np.float64)[keep]


def _mean_std(v):
    """(mean, population std) of the non-NaN entries; (nan, nan) of none."""
    v = v[~np.isnan(v)]
    return (float(v.mean()), float(v.std())) if v.size else (float("nan"), float("nan"))


class DepthMetrics(_PerImageRows):
    """Accumulates the per-image values of `depth_metrics` over batches; `summary()` is what a results table
    prints: mean and standard deviation over the images that had a counted pixel."""
    keys = KEYS

    def summary(self):
        """{"mae" | "mse" | "side" | "mad": (mean, std), "images": used, "skipped": images with count == 0}, in
        float64 on the host; std is the population one (numpy's default, as the reference's loss statistics).
        An image that counts pixels but has no normal (erode off, no stencil) has a NaN mad and is left out of
        mad's two figures only."""
        keep = np.asarray(self.values["count"], np.float64) > 0
        out = {"images": int(keep.sum()), "skipped": int((~keep).sum())}
        for k in METRICS:
            out[k] = _mean_std(self._column(k, keep))
        return out


# ----------------------------------------------------------------------------------------- image against image
IMAGE_METRICS = ("mae", "mse", "psnr", "ssim")
IMAGE_KEYS = ("count", "mae", "mse", "psnr", "ssim_count", "ssim")
SSIM_WINDOW, SSIM_SIGMA, SSIM_K1, SSIM_K2 = 11, 1.5, 0.01, 0.03


def ssim_window(dtype=torch.float64, device="cpu"):
    """The 11 taps of the Gaussian window (sigma 1.5) normalised to sum 1, computed in float64."""
    x = torch.arange(SSIM_WINDOW, dtype=torch.float64) - SSIM_WINDOW // 2
    g = torch.exp(-(x * x) / (2 * SSIM_SIGMA ** 2))
    return (g / g.sum()).to(device=device, dtype=dtype)


def _image_metrics_torch(a, b, mask, data_range, out_dtype=torch.float32):
    """The definitions of include/g2s.h (g2s_image_metrics) as torch ops, in the tensors' dtype: a, b (B, C, H, W),
    mask (B, H, W) or None.  In float64, with out_dtype float64, this is the oracle the kernel is tested against."""
    B, C, H, W = a.shape
    dtype, device = a.dtype, a.device
    counted = torch.ones((B, H, W), dtype=torch.bool, device=device) if mask is None else mask > 0.5
    n = counted.sum((1, 2)).to(dtype)
    zero = torch.zeros((), dtype=dtype, device=device)
    nan = torch.full_like(n, float("nan"))
    d = a - b
    on = counted.unsqueeze(1)
    mae = torch.where(on, d.abs(), zero).sum((1, 2, 3)) / (n * C)
    mse = torch.where(on, d * d, zero).sum((1, 2, 3)) / (n * C)
    psnr = 10.0 * torch.log10(float(data_range) ** 2 / mse)      # +inf where mse == 0
    empty = n == 0
    out = {"count": n.to(out_dtype), "mae": torch.where(empty, nan, mae).to(out_dtype), "mse": torch.where(empty, nan, mse).to(out_dtype),
           "psnr": torch.where(empty, nan, psnr).to(out_dtype)}
    r = SSIM_WINDOW // 2
    if H < SSIM_WINDOW or W < SSIM_WINDOW:
        out["ssim_count"], out["ssim"] = torch.zeros_like(n).to(out_dtype), nan.to(out_dtype)
        return out
    w = ssim_window(dtype, device)
    wx, wy = w.view(1, 1, 1, -1), w.view(1, 1, -1, 1)

    def filt(u):        # F(u): along x, then along y; valid windows only.  One plane per call: five identical calls
        u = F.conv2d(F.conv2d(u.reshape(B * C, 1, H, W), wx), wy)
        return u.reshape(B, C, H - 2 * r, W - 2 * r)
    mu_a, mu_b = filt(a), filt(b)
    var_a, var_b, cov = filt(a * a) - mu_a * mu_a, filt(b * b) - mu_b * mu_b, filt(a * b) - mu_a * mu_b
    c1, c2 = (SSIM_K1 * float(data_range)) ** 2, (SSIM_K2 * float(data_range)) ** 2
    s = ((2.0 * mu_a * mu_b + c1) * (2.0 * cov + c2)) / ((mu_a * mu_a + mu_b * mu_b + c1) * (var_a + var_b + c2))
    centres = counted[:, r:H - r, r:W - r]
    nw = centres.sum((1, 2)).to(dtype)
    ssim = torch.where(centres.unsqueeze(1), s, zero).sum((1, 2, 3)) / (nw * C)
    out["ssim_count"], out["ssim"] = nw.to(out_dtype), torch.where(nw == 0, nan, ssim).to(out_dtype)
    return out


def image_metrics(recon, target, mask=None, *, data_range):
    """Per-image fidelity of `recon` against `target`, both (B, C, H, W), 1 <= C <= 4, finite; mask (B, H, W) or
    (B, 1, H, W), counted where > 0.5 (None: everywhere).  `data_range` is the width of the images' value range (2 for
    images in [-1, 1]).  SSIM is Wang et al.'s with an 11 x 11 Gaussian window of sigma 1.5 over the windows that lie
    wholly inside the image and whose centre is counted (include/g2s.h, g2s_image_metrics, states every operation).

    Returns {"count", "mae", "mse", "psnr", "ssim_count", "ssim"}: (B,) float32 tensors on the inputs' device.  An
    image without a counted pixel has count 0 and NaN mae / mse / psnr; psnr is +inf where mse is 0; an image smaller
    than a window, or without a counted window centre, has ssim_count 0 and a NaN ssim."""
    who = "image_metrics"
    if recon.dim() != 4 or recon.shape != target.shape:
        raise ValueError(f"{who}: images must be (B, C, H, W) of one shape, got {tuple(recon.shape)} "
                         f"and {tuple(target.shape)}")
    B, C, H, W = recon.shape
    if not 1 <= C <= 4:
        raise ValueError(f"{who}: C = {C} outside [1, 4]")
    if H < 1 or W < 1:
        raise ValueError(f"{who}: H and W must be at least 1")
    if not (math.isfinite(float(data_range)) and float(data_range) > 0):
        raise ValueError(f"{who}: data_range = {data_range} must be positive and finite")
    device = recon.device
    tensors = [recon, target, _as_bhw(mask, (B, H, W), "mask", who)]
    if any(t is not None and t.device != device for t in tensors):
        raise ValueError(f"{who}: images and mask must be on one device")
    if B == 0:
        return {k: torch.empty(0, dtype=torch.float32, device=device) for k in IMAGE_KEYS}
    with torch.no_grad():
        if device.type != "cuda":
            dtype = recon.dtype if recon.dtype in (torch.float32, torch.float64) else torch.float32
            return _image_metrics_torch(*[None if t is None else t.detach().to(dtype) for t in tensors], float(data_range))
        L = _lib.load()
        a, b, m = [None if t is None else t.detach().to(torch.float32).contiguous() for t in tensors]
        out = torch.empty(B, 6, dtype=torch.float32, device=device)
        with torch.cuda.device(device):
            ws = _workspace(device, L.g2s_image_metrics_workspace_bytes(B, C, H, W))
            _lib.check(L.g2s_image_metrics(_lib.ptr(a), _lib.ptr(b), _lib.ptr(m), B, C, H, W, float(data_range),
                                           _lib.ptr(out), _lib.ptr(ws), ws.numel(), _lib.stream()))
        return {k: out[:, i] for i, k in enumerate(IMAGE_KEYS)}


class ImageMetrics(_PerImageRows):
    """Accumulates the per-image values of `image_metrics` over batches, as DepthMetrics does for `depth_metrics`."""
    keys = IMAGE_KEYS

    def summary(self):
        """{"mae" | "mse" | "psnr" | "ssim": (mean, std), "images": images with count > 0, "skipped": the others,
        "exact": images whose psnr is +inf (mse 0; left out of psnr's two figures), "ssim_images": images with
        ssim_count > 0, the only ones in ssim's two figures}; float64 on the host, population std."""
        keep = np.asarray(self.values["count"], np.float64) > 0
        windows = keep & (np.asarray(self.values["ssim_count"], np.float64) > 0)
        psnr = self._column("psnr", keep)
        out = {"images": int(keep.sum()), "skipped": int((~keep).sum()), "exact": int(np.isposinf(psnr).sum()),
               "ssim_images": int(windows.sum())}
        out["mae"], out["mse"] = _mean_std(self._column("mae", keep)), _mean_std(self._column("mse", keep))
        out["psnr"] = _mean_std(psnr[~np.isposinf(psnr)])
        out["ssim"] = _mean_std(self._column("ssim", windows))
        return out
