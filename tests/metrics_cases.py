"""Cases and the float64 oracle of the depth metrics (gan2shape_amd.metrics, csrc/metrics.hip), shared by
test_metrics_cpu.py and test_gpu_metrics.py.  Nothing here imports the package: the oracle restates the
definitions of include/g2s.h (g2s_depth_metrics) in numpy float64, and `metrics64_loops` once more pixel by pixel.

Depths look like the model's: smooth fields in [0.9, 1.1] plus small noise.  The rays are those of
Renderer.__init__ / Renderer._pixel_rays for fov 10 (float32 K, its inverse, (x, y, 1) K^-T).

Tolerance.  For a metric m the error figure is e = |got - want| / (A_m + |want|) with the natural units A below.
TORCH_FP32_ERROR holds, per metric, the largest e of the torch float32 composition on the CPU
(gan2shape_amd.metrics.depth_metrics on CPU tensors: the route a user without the kernel takes) against `metrics64`
over all of CASES, measured by `python tests/metrics_cases.py` (which prints the table) on an x86-64 host with
the torch build of this project.  The kernel, and the GPU-against-CPU comparison, are allowed MARGIN = 4 times
that figure: the device's sqrtf / atan2f differ from the host's by a few ulp and the sums run in another order.
The bound stays small enough that an fp32 E[d^2] - E[d]^2 (test_metrics_cpu) or a dropped erosion ring fails it.
"""
import math

import numpy as np

EPS = 1e-7                       # Renderer.get_normal_from_depth
A = {"mae": 1e-2, "mse": 1e-4, "side": 1e-2, "mad": 1.0}
METRICS = ("mae", "mse", "side", "mad")
KEYS = ("count",) + METRICS
MARGIN = 4.0
# largest e of the torch fp32 CPU composition over CASES (measured values; see the module docstring)
TORCH_FP32_ERROR = {
    "mae": 1.22e-7,     # measured 1.215e-07 (no_mask_gt)
    "mse": 1.03e-7,     # measured 1.027e-07 (16x16x17)
    "side": 6.41e-8,    # measured 6.403e-08 (16x16x17)
    "mad": 1.05e-6,     # measured 1.047e-06 (p_scaled)
}
BOUND = {k: MARGIN * v for k, v in TORCH_FP32_ERROR.items()}


# ------------------------------------------------------------------------------------------- rays
def pixel_rays(H, W, image_size=None, fov=10.0):
    """(H, W, 3) float32: K^-1 (x, y, 1)^T per pixel, K the pinhole of a square image of `image_size` (default
    max(H, W)) as Renderer.__init__ builds it; float32 arithmetic as Renderer._pixel_rays."""
    S = max(H, W) if image_size is None else image_size
    f = (S - 1) / 2 / math.tan(fov / 2 * math.pi / 180)
    c = (S - 1) / 2
    K = np.array([[f, 0., c], [0., f, c], [0., 0., 1.]], np.float32)
    inv_K = np.linalg.inv(K).astype(np.float32)
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
    grid = np.stack([xx, yy, np.ones_like(xx)], -1)
    return (grid @ inv_K.T).astype(np.float32)


class CaseRenderer():
    """Stands in for renderer.Renderer where only `_pixel_rays` is needed: hands out the case's own rays, so
    that the oracle and the code under test read the same bits on every device."""

    def __init__(self, image_size=None):
        self.image_size = image_size
        self._rays = {}

    def _pixel_rays(self, h, w, device):
        import torch
        key = (h, w, str(device))
        if key not in self._rays:
            self._rays[key] = torch.from_numpy(pixel_rays(h, w, self.image_size)).to(device)[None]
        return self._rays[key]


# ------------------------------------------------------------------------------------------- cases
def smooth_depth(rng, B, H, W, noise=2e-3):
    """Smooth field in [0.9, 1.1] plus small noise, float32."""
    y, x = np.meshgrid(np.linspace(-1, 1, H), np.linspace(-1, 1, W), indexing="ij")
    out = np.empty((B, H, W), np.float64)
    for b in range(B):
        a = rng.uniform(-1, 1, 6)
        out[b] = (1.0 + 0.04 * a[0] * np.sin(2.5 * x + a[1]) + 0.04 * a[2] * np.cos(2.0 * y + a[3])
                  + 0.03 * a[4] * x * y - 0.04 * np.exp(-((x - 0.2 * a[5]) ** 2 + y ** 2) / 0.3))
    out += noise * rng.standard_normal(out.shape)
    return np.clip(out, 0.9, 1.1).astype(np.float32)


def _case(seed, B, H, W, erode=True, masks="none", holes=0.0, nan_patches=0):
    rng = np.random.default_rng(seed)
    gt = smooth_depth(rng, B, H, W)
    pred = smooth_depth(rng, B, H, W)
    mp = mg = None
    if masks in ("both", "pred"):
        mp = (rng.random((B, H, W)) >= holes).astype(np.float32)
    if masks in ("both", "gt"):
        mg = (rng.random((B, H, W)) >= holes).astype(np.float32)
    for _ in range(nan_patches):
        b, y, x = rng.integers(B), rng.integers(H - 3), rng.integers(W - 3)
        pred[b, y:y + 1 + rng.integers(3), x:x + 1 + rng.integers(3)] = np.nan
    return {"pred": pred, "gt": gt, "mask_pred": mp, "mask_gt": mg, "erode": erode}


def _build():
    C = {}
    C["3x3"] = _case(1, 1, 3, 3)                                   # one counted pixel
    C["8x8_erode"] = _case(2, 1, 8, 8)
    C["8x8_raw"] = _case(2, 1, 8, 8, erode=False)
    C["5x9"] = _case(3, 2, 5, 9, masks="both", holes=0.04)         # non-square, narrower than a wavefront
    C["5x9_raw"] = _case(3, 2, 5, 9, erode=False, masks="both", holes=0.04)
    C["33x33"] = _case(4, 3, 33, 33, masks="both", holes=0.02, nan_patches=6)
    C["33x33_raw"] = _case(4, 3, 33, 33, erode=False, masks="both", holes=0.02, nan_patches=6)
    many = _case(5, 17, 16, 16, masks="both", holes=0.01)
    many["mask_gt"][3] = 0.0                                       # empty: count 0, NaN
    many["mask_pred"][5] = 0.0                                     # two pixel wide bars: erosion empties it
    many["mask_pred"][5, :, 2:4] = 1.0
    many["mask_pred"][5, 7:9, :] = 1.0
    many["gt"][8, 4, 4] = -1.0                                     # a non-positive and an infinite depth
    many["pred"][9, 10, 3] = np.inf
    C["16x16x17"] = many
    big = _case(6, 2, 128, 128, masks="both", holes=0.002, nan_patches=4)
    y, x = np.meshgrid(np.linspace(-1, 1, 128), np.linspace(-1, 1, 128), indexing="ij")
    big["mask_gt"] *= ((x / 0.7) ** 2 + (y / 0.85) ** 2 < 1).astype(np.float32)   # an object mask
    C["128x128"] = big
    same = _case(7, 2, 32, 32)
    same["pred"] = same["gt"].copy()
    C["p_eq_g"] = same
    scaled = _case(8, 1, 64, 64)
    scaled["pred"] = (np.float32(1.07) * scaled["gt"]).astype(np.float32)
    C["p_scaled"] = scaled
    C["no_mask_pred"] = _case(9, 2, 20, 24, masks="gt", holes=0.03)
    C["no_mask_gt"] = _case(10, 2, 20, 24, masks="pred", holes=0.03)
    C["no_masks"] = _case(11, 2, 20, 24, nan_patches=3)
    for c in C.values():
        c["rays"] = pixel_rays(*c["pred"].shape[1:])
    return C


CASES = _build()


# ------------------------------------------------------------------------------------------- float64 oracle
def raw_valid(pred, gt, mask_pred, mask_gt):
    with np.errstate(invalid="ignore"):
        v = np.isfinite(pred) & np.isfinite(gt) & (pred > 0) & (gt > 0)
    if mask_pred is not None:
        v &= mask_pred > 0.5
    if mask_gt is not None:
        v &= mask_gt > 0.5
    return v


def _normals64(rays, depth):
    """(B, H-2, W-2, 3): cross(P(y, x+1) - P(y, x-1), P(y+1, x) - P(y-1, x)) / (norm + EPS), P = rays * depth."""
    P = rays[None].astype(np.float64) * depth.astype(np.float64)[..., None]
    n = np.cross(P[:, 1:-1, 2:] - P[:, 1:-1, :-2], P[:, 2:, 1:-1] - P[:, :-2, 1:-1])
    return n / (np.sqrt((n ** 2).sum(-1, keepdims=True)) + EPS)


def metrics64(pred, gt, mask_pred, mask_gt, rays, erode):
    """{count, mae, mse, side, mad}: (B,) float64 arrays, straight from the definitions of include/g2s.h."""
    B, H, W = pred.shape
    valid = raw_valid(pred, gt, mask_pred, mask_gt)
    finite = np.isfinite(pred) & np.isfinite(gt)
    if erode:
        padded = np.zeros((B, H + 2, W + 2), bool)
        padded[:, 1:-1, 1:-1] = valid
        counted = np.ones((B, H, W), bool)
        for dy in range(3):
            for dx in range(3):
                counted &= padded[:, dy:dy + H, dx:dx + W]
    else:
        counted = valid
    stencil = np.zeros((B, H, W), bool)
    stencil[:, 1:-1, 1:-1] = finite[:, 1:-1, 2:] & finite[:, 1:-1, :-2] & finite[:, 2:, 1:-1] & finite[:, :-2, 1:-1]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        n_p, n_g = _normals64(rays, pred), _normals64(rays, gt)
        # angle between the two normals; atan2 form (equal to acos of the dot product for unit vectors): the
        # EPS in the normalisation leaves both shorter than 1, which must not read as an angle
        ang = np.zeros((B, H, W))
        ang[:, 1:-1, 1:-1] = np.degrees(np.arctan2(np.sqrt((np.cross(n_p, n_g) ** 2).sum(-1)), (n_p * n_g).sum(-1)))
    out = {k: np.full(B, np.nan) for k in KEYS}
    for b in range(B):
        m = counted[b]
        n = int(m.sum())
        out["count"][b] = n
        if n == 0:
            continue
        p, g = pred[b][m].astype(np.float64), gt[b][m].astype(np.float64)
        out["mae"][b] = np.abs(p - g).sum() / n
        out["mse"][b] = ((p - g) ** 2).sum() / n
        delta = np.log(p) - np.log(g)
        out["side"][b] = math.sqrt(max(0.0, ((delta - delta.sum() / n) ** 2).sum() / n))
        mm = m & stencil[b]
        if mm.any():
            out["mad"][b] = ang[b][mm].sum() / int(mm.sum())
    return out


def metrics64_loops(pred, gt, mask_pred, mask_gt, rays, erode):
    """The same definitions pixel by pixel, with Python floats: the oracle's own check."""
    B, H, W = pred.shape
    r64 = rays.astype(np.float64)

    def ok(b, y, x):
        if not (0 <= y < H and 0 <= x < W):
            return False
        p, g = float(pred[b, y, x]), float(gt[b, y, x])
        return (math.isfinite(p) and math.isfinite(g) and p > 0 and g > 0
                and (mask_pred is None or mask_pred[b, y, x] > 0.5) and (mask_gt is None or mask_gt[b, y, x] > 0.5))

    def normal(d, b, y, x):
        P = lambda yy, xx: r64[yy, xx] * float(d[b, yy, xx])    # noqa: E731
        tu, tv = P(y, x + 1) - P(y, x - 1), P(y + 1, x) - P(y - 1, x)
        n = np.array([tu[1] * tv[2] - tu[2] * tv[1], tu[2] * tv[0] - tu[0] * tv[2], tu[0] * tv[1] - tu[1] * tv[0]])
        return n / (math.sqrt(float(n @ n)) + EPS)
    out = {k: np.full(B, np.nan) for k in KEYS}
    for b in range(B):
        px, angles = [], []
        for y in range(H):
            for x in range(W):
                if erode:
                    counted = all(ok(b, y + dy, x + dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1))
                else:
                    counted = ok(b, y, x)
                if not counted:
                    continue
                px.append((float(pred[b, y, x]), float(gt[b, y, x])))
                nb = [(y, x + 1), (y, x - 1), (y + 1, x), (y - 1, x)]
                if all(0 <= yy < H and 0 <= xx < W and math.isfinite(float(pred[b, yy, xx]))
                       and math.isfinite(float(gt[b, yy, xx])) for yy, xx in nb):
                    a, c = normal(pred, b, y, x), normal(gt, b, y, x)
                    cr = np.array([a[1] * c[2] - a[2] * c[1], a[2] * c[0] - a[0] * c[2], a[0] * c[1] - a[1] * c[0]])
                    angles.append(math.degrees(math.atan2(math.sqrt(float(cr @ cr)), float(a @ c))))
        n = len(px)
        out["count"][b] = n
        if n == 0:
            continue
        out["mae"][b] = sum(abs(p - g) for p, g in px) / n
        out["mse"][b] = sum((p - g) ** 2 for p, g in px) / n
        delta = [math.log(p) - math.log(g) for p, g in px]
        mean = sum(delta) / n
        out["side"][b] = math.sqrt(max(0.0, sum((d - mean) ** 2 for d in delta) / n))
        if angles:
            out["mad"][b] = sum(angles) / len(angles)
    return out


def oracle(name):
    """metrics64 of CASES[name], computed once per process and shared (callers must not modify it)."""
    if name not in _ORACLE:
        c = CASES[name]
        _ORACLE[name] = metrics64(c["pred"], c["gt"], c["mask_pred"], c["mask_gt"], c["rays"], c["erode"])
    return _ORACLE[name]


_ORACLE = {}


# ------------------------------------------------------------------------------------------- error figure
def error_figures(got, want):
    """{metric: largest e over the images}.  count must be equal and NaN must sit exactly where the oracle has NaN:
    a violation returns inf for that metric (and for "count")."""
    out = {}
    gc, wc = np.asarray(got["count"], np.float64), np.asarray(want["count"], np.float64)
    out["count"] = 0.0 if gc.shape == wc.shape and np.array_equal(gc, wc) else math.inf
    for k in METRICS:
        g, w = np.asarray(got[k], np.float64), np.asarray(want[k], np.float64)
        if g.shape != w.shape or not np.array_equal(np.isnan(g), np.isnan(w)):
            out[k] = math.inf
            continue
        keep = ~np.isnan(w)
        out[k] = float((np.abs(g[keep] - w[keep]) / (A[k] + np.abs(w[keep]))).max()) if keep.any() else 0.0
    return out


def check(got, want, what, bound=None):
    """Print the figures, then assert them against `bound` (default BOUND)."""
    bound = BOUND if bound is None else bound
    e = error_figures(got, want)
    print(f"{what}: " + ", ".join(f"e_{k} {e[k]:.3e} (bound {bound[k]:.3e})" for k in METRICS)
          + f", count {'equal' if e['count'] == 0 else 'DIFFERS'}")
    assert e["count"] == 0, f"{what}: count {got['count']} != {want['count']}"
    for k in METRICS:
        assert e[k] <= bound[k], f"{what}: e_{k} = {e[k]:.3e} > {bound[k]:.3e}\n got {got[k]}\nwant {want[k]}"
    return e


def to_numpy(metrics):
    return {k: np.asarray(v.detach().cpu().numpy() if hasattr(v, "detach") else v, np.float64) for k, v in metrics.items()}


def run_case(depth_metrics, name, device="cpu"):
    """depth_metrics of the package on CASES[name] -> dict of float64 arrays."""
    import torch
    c = CASES[name]
    t = lambda a: None if a is None else torch.from_numpy(a).to(device)    # noqa: E731
    return to_numpy(depth_metrics(t(c["pred"]), t(c["gt"]), t(c["mask_pred"]), t(c["mask_gt"]),
                                  renderer=CaseRenderer(), erode=c["erode"]))


if __name__ == "__main__":      # the measurement behind TORCH_FP32_ERROR
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import gan2shape_amd  # noqa: F401
    from gan2shape_amd.metrics import depth_metrics
    worst = {k: 0.0 for k in METRICS}
    for name in CASES:
        e = error_figures(run_case(depth_metrics, name), oracle(name))
        print(f"{name:14s} " + " ".join(f"{k} {e[k]:.3e}" for k in KEYS))
        worst = {k: max(worst[k], e[k]) for k in METRICS}
    print("largest:", worst)
