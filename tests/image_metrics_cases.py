"""Cases, the float64 oracle and the error figure of the image metrics (gan2shape_amd.metrics.image_metrics,
csrc/image_metrics.hip), shared by test_image_metrics_cpu.py and test_gpu_image_metrics.py.

Oracle: `gan2shape_amd.metrics._image_metrics_torch` on float64 copies of a case — the torch composition is the
specification (include/g2s.h states the same operations).  It is itself checked twice: against `ssim64_direct`
below (numpy float64, the 2-D window applied window by window, nothing shared with the composition) and, where
scikit-image is installed, against skimage.metrics.structural_similarity on the unmasked cases.

Images look like the model's: smooth fields in [-1, 1] (or [0, 1]) plus noise, the second image a perturbed copy of
the first, so that SSIM lands between 0.2 and 0.95.

Tolerance, the convention of metrics_cases.py.  For a metric m the error figure is e = |got - want| / (A_m + |want|)
with the natural units A below.  `bound()` measures, per metric, the largest e of the torch float32 composition on the
CPU (image_metrics on float32 CPU tensors: the route a user without the kernel takes) against the oracle over all of
CASES, and allows MARGIN = 4 times that: computed here, in the test process, not written down.  count and ssim_count
must be equal; NaN and +-inf must sit exactly where the oracle has them.
"""
import math

import numpy as np

A = {"mae": 1e-2, "mse": 1e-4, "psnr": 1.0, "ssim": 1e-2}
METRICS = ("mae", "mse", "psnr", "ssim")
COUNTS = ("count", "ssim_count")
KEYS = ("count", "mae", "mse", "psnr", "ssim_count", "ssim")
MARGIN = 4.0
TILE_Y, TILE_X = 16, 32          # the kernel's tile of window centres (IM_TY, IM_TX of csrc/image_metrics.hip);
#                                  test_gpu_image_metrics.py pins them through the workspace size
WIN, R, SIGMA = 11, 5, 1.5


# ------------------------------------------------------------------------------------------- cases
def smooth_pair(rng, B, C, H, W, lo=-1.0, hi=1.0, noise=0.08, shift=0.25):
    """(a, b) float32 (B, C, H, W) in [lo, hi]: b a smooth field plus noise, a the same field slightly deformed and
    rescaled plus its own noise — what a reconstruction is to its image."""
    y, x = np.meshgrid(np.linspace(-1, 1, H), np.linspace(-1, 1, W), indexing="ij")
    a, b = np.empty((B, C, H, W)), np.empty((B, C, H, W))
    for i in range(B):
        for c in range(C):
            p = rng.uniform(-1, 1, 8)

            def field(dx, gain):
                return gain * (0.45 * np.sin(3.0 * (x + dx) + 3 * p[0]) * np.cos(2.5 * y + 3 * p[1])
                               + 0.35 * np.cos(4.0 * (x + dx) * y + 3 * p[2]) + 0.2 * p[3] * (x + dx) + 0.15 * p[4] * y)
            b[i, c] = field(0.0, 1.0) + noise * rng.standard_normal((H, W))
            a[i, c] = field(shift * 0.2 * p[5], 0.9 + 0.08 * p[6]) + 0.03 * p[7] + noise * rng.standard_normal((H, W))
    mid, half = (hi + lo) / 2, (hi - lo) / 2
    return (np.clip(mid + half * a, lo, hi).astype(np.float32), np.clip(mid + half * b, lo, hi).astype(np.float32))


def ellipse(H, W, cx=0.1, cy=-0.05, rx=0.7, ry=0.8):
    y, x = np.meshgrid(np.linspace(-1, 1, H), np.linspace(-1, 1, W), indexing="ij")
    return ((((x - cx) / rx) ** 2 + ((y - cy) / ry) ** 2) < 1).astype(np.float32)


def _case(seed, B, C, H, W, data_range=2.0, mask=None):
    rng = np.random.default_rng(seed)
    lo, hi = (-1.0, 1.0) if data_range == 2.0 else (0.0, 1.0)
    a, b = smooth_pair(rng, B, C, H, W, lo, hi)
    m = None
    if mask == "ellipse":
        m = np.stack([ellipse(H, W, cx=0.1 - 0.1 * i, ry=0.8 - 0.05 * i) for i in range(B)])
    elif mask == "random":
        m = (rng.random((B, H, W)) >= 0.1).astype(np.float32)
    return {"a": a, "b": b, "mask": m, "data_range": data_range}


def _build():
    C = {}
    C["11x11"] = _case(1, 1, 3, 11, 11)                                     # exactly one window
    C["10x12"] = _case(2, 2, 3, 10, 12)                                     # no window: ssim NaN, psnr finite
    C["12x11"] = _case(3, 1, 2, 12, 11, data_range=1.0)
    C["11x12"] = _case(4, 1, 2, 11, 12, data_range=1.0)
    C["one_tile"] = _case(5, 2, 3, TILE_Y + 10, TILE_X + 10)                # the last shape with one tile per axis
    C["two_tiles"] = _case(6, 2, 3, TILE_Y + 11, TILE_X + 11, mask="random")  # the first with two
    for ch in (1, 3, 4):
        C[f"33x47_c{ch}"] = _case(7 + ch, 2, ch, 33, 47, mask="ellipse")
    many = _case(12, 17, 3, 16, 16, mask="random")
    many["mask"][3] = 0.0                                                   # empty: count 0, everything NaN
    many["mask"][11] = 0.0
    many["mask"][5] = 0.0                                                   # counted pixels, but no counted window centre
    many["mask"][5, :5, :] = 1.0                                            # (centres are [5, 10] x [5, 10])
    many["mask"][5, :, 11:] = 1.0
    C["16x16x17"] = many
    same = _case(13, 2, 3, 20, 24)
    same["a"] = same["b"].copy()                                            # mae = mse = 0, psnr +inf, ssim 1 exactly
    C["a_eq_b"] = same
    const = _case(14, 1, 2, 14, 15)
    const["a"] = np.full_like(const["a"], 0.3)                              # zero variances: the C2 terms decide
    const["b"] = np.full_like(const["b"], -0.2)
    C["constants"] = const
    C["128x128"] = _case(15, 2, 3, 128, 128, mask="ellipse")
    return C


CASES = _build()
UNMASKED = [k for k, c in CASES.items() if c["mask"] is None and min(c["a"].shape[2:]) >= WIN]


# ------------------------------------------------------------------------------------------- oracles
def _torch_args(name, device="cpu", dtype=None):
    import torch
    c = CASES[name]
    t = lambda v: None if v is None else torch.from_numpy(v).to(device=device, dtype=dtype or torch.float32)  # noqa: E731
    return t(c["a"]), t(c["b"]), t(c["mask"])


def to_numpy(metrics):
    return {k: np.asarray(v.detach().cpu().numpy() if hasattr(v, "detach") else v, np.float64) for k, v in metrics.items()}


def oracle(name):
    """_image_metrics_torch on float64 copies of CASES[name], computed once per process and shared (callers must not
    modify it)."""
    if name not in _ORACLE:
        _ORACLE[name] = _oracle64(name)
    return _ORACLE[name]


def _oracle64(name):
    import torch
    import gan2shape_amd  # noqa: F401
    from gan2shape_amd import metrics
    a, b, m = _torch_args(name, dtype=torch.float64)
    return to_numpy(metrics._image_metrics_torch(a, b, m, CASES[name]["data_range"], out_dtype=torch.float64))


_ORACLE = {}


def window64():
    x = np.arange(WIN, dtype=np.float64) - R
    g = np.exp(-(x * x) / (2 * SIGMA ** 2))
    return g / g.sum()


def ssim64_direct(a, b, mask, data_range):
    """{count, mae, mse, psnr, ssim_count, ssim} in numpy float64, straight from the definitions: each window is cut
    out and weighted with the 2-D window outer(w, w); Python loops over images, channels and centres."""
    a, b = a.astype(np.float64), b.astype(np.float64)
    B, C, H, W = a.shape
    w2 = np.outer(window64(), window64())
    c1, c2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    out = {k: np.full(B, np.nan) for k in KEYS}
    for i in range(B):
        m = np.ones((H, W), bool) if mask is None else mask[i] > 0.5
        n = int(m.sum())
        out["count"][i] = n
        if n:
            d = (a[i] - b[i])[:, m]
            out["mae"][i] = np.abs(d).sum() / (n * C)
            out["mse"][i] = (d * d).sum() / (n * C)
            out["psnr"][i] = math.inf if out["mse"][i] == 0 else 10 * math.log10(data_range ** 2 / out["mse"][i])
        vals, nw = [], 0
        for y in range(R, H - R):
            for x in range(R, W - R):
                if not m[y, x]:
                    continue
                nw += 1
                for c in range(C):
                    pa, pb = a[i, c, y - R:y + R + 1, x - R:x + R + 1], b[i, c, y - R:y + R + 1, x - R:x + R + 1]
                    ma, mb = (w2 * pa).sum(), (w2 * pb).sum()
                    va, vb, cov = (w2 * pa * pa).sum() - ma * ma, (w2 * pb * pb).sum() - mb * mb, (w2 * pa * pb).sum() - ma * mb
                    vals.append(((2 * ma * mb + c1) * (2 * cov + c2)) / ((ma * ma + mb * mb + c1) * (va + vb + c2)))
        out["ssim_count"][i] = nw
        if nw:
            out["ssim"][i] = sum(vals) / (nw * C)
    return out


# ------------------------------------------------------------------------------------------- error figure
def error_figures(got, want):
    """{metric: largest e over the images}; "counts" is 0 if count and ssim_count are equal, else inf.  NaN and +-inf
    must sit exactly where the oracle has them: a violation returns inf for that metric."""
    out = {"counts": 0.0}
    for k in COUNTS:
        g, w = np.asarray(got[k], np.float64), np.asarray(want[k], np.float64)
        if g.shape != w.shape or not np.array_equal(g, w):
            out["counts"] = math.inf
    for k in METRICS:
        g, w = np.asarray(got[k], np.float64), np.asarray(want[k], np.float64)
        special = ~np.isfinite(w)
        if g.shape != w.shape or not np.array_equal(np.isnan(g), np.isnan(w)) or not np.array_equal(np.isfinite(g), np.isfinite(w)) \
                or not np.array_equal(g[special & ~np.isnan(w)], w[special & ~np.isnan(w)]):
            out[k] = math.inf
            continue
        keep = ~special
        out[k] = float((np.abs(g[keep] - w[keep]) / (A[k] + np.abs(w[keep]))).max()) if keep.any() else 0.0
    return out


def run_case(image_metrics, name, device="cpu", dtype=None):
    """image_metrics of the package on CASES[name] -> dict of float64 arrays."""
    a, b, m = _torch_args(name, device, dtype)
    return to_numpy(image_metrics(a, b, m, data_range=CASES[name]["data_range"]))


def torch_fp32_error():
    """Per metric, the largest e of the float32 torch composition on the CPU against the oracle over CASES (and the
    case that shows it); measured once per process."""
    if not _FP32:
        import gan2shape_amd  # noqa: F401
        from gan2shape_amd.metrics import image_metrics
        worst = {k: (0.0, None) for k in METRICS}
        for name in CASES:
            e = error_figures(run_case(image_metrics, name), oracle(name))
            assert e["counts"] == 0 and all(math.isfinite(e[k]) for k in METRICS), (name, e)
            for k in METRICS:
                if e[k] > worst[k][0]:
                    worst[k] = (e[k], name)
        _FP32.update(worst)
    return _FP32


_FP32 = {}


def bound():
    return {k: MARGIN * v[0] for k, v in torch_fp32_error().items()}


def check(got, want, what, limit=None):
    """Print the figures, then assert them against `limit` (default bound())."""
    limit = bound() if limit is None else limit
    e = error_figures(got, want)
    print(f"{what}: " + ", ".join(f"e_{k} {e[k]:.3e} (bound {limit[k]:.3e})" for k in METRICS)
          + f", counts {'equal' if e['counts'] == 0 else 'DIFFER'}")
    assert e["counts"] == 0, f"{what}: counts {got['count']}, {got['ssim_count']} != {want['count']}, {want['ssim_count']}"
    for k in METRICS:
        assert e[k] <= limit[k], f"{what}: e_{k} = {e[k]:.3e} > {limit[k]:.3e}\n got {got[k]}\nwant {want[k]}"
    return e


if __name__ == "__main__":      # the table behind bound(), and where SSIM lands
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    for name in CASES:
        w = oracle(name)
        print(f"{name:12s} psnr {np.round(w['psnr'], 2)} ssim {np.round(w['ssim'], 3)}")
    print({k: (f"{v[0]:.3e}", v[1]) for k, v in torch_fp32_error().items()})
