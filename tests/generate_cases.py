"""Cases of the sample generator's tests (test_generate_cpu.py, test_gpu_generate.py) and a numpy float64 statement
of its three kernels: the mapping network with skip / depth / truncation, the ordered mean, the quantiser.
tests/golden/make_generate_golden.py writes the reference Generator's float64 results to tests/golden/generate.npz."""
import math

import numpy as np

ALPHA, GAIN = 0.2, math.sqrt(2.0)
LR_MLP = 0.01                         # Generator's lr_mlp: EqualLinear.scale = lr_mul / sqrt(D), bias * lr_mul

G_CFG = dict(size=8, style_dim=32, n_mlp=4, channel_multiplier=1, seed=31)      # the fixture's generator
N_Z, N_MEAN, TRUNCATION = 5, 70, 0.7


# ------------------------------------------------------------------------------------------ float64 statement
def scaled(weights, biases, lr_mul=LR_MLP):
    """Raw EqualLinear parameters [L, D, D] / [L, D] -> what g2s_mapping_fwd takes, float64."""
    w = np.asarray(weights, np.float64)
    return w * (lr_mul / math.sqrt(w.shape[-1])), np.asarray(biases, np.float64) * lr_mul


def mapping64(z, w, b, pixel_norm=True, alpha=ALPHA, gain=GAIN, center=None, truncation=1.0):
    """g2s_mapping_fwd's semantics in float64: w [L, D, D] and b [L, D] already scaled."""
    h = np.asarray(z, np.float64)
    if pixel_norm:
        h = h / np.sqrt((h * h).mean(1, keepdims=True) + 1e-8)
    for wl, bl in zip(np.asarray(w, np.float64), np.asarray(b, np.float64)):
        y = h @ wl.T + bl
        h = gain * np.where(y > 0, y, alpha * y)
    if center is not None:
        c = np.asarray(center, np.float64).reshape(1, -1)
        h = c + truncation * (h - c)
    return h


def style_forward64(z, w, b, skip=0, depth=100, **kw):
    """Generator.style_forward(z, skip, depth) on the scaled stacks: entry 0 of G.style is PixelNorm."""
    n = len(w) + 1
    lo, hi = max(skip, 0), min(depth, n)
    first = max(lo, 1)
    return mapping64(z, w[first - 1:max(hi, first) - 1], b[first - 1:max(hi, first) - 1],
                     pixel_norm=lo == 0 and hi > 0, **kw)


def partial_sums64(out, tile):
    """[ceil(N / tile), D]: column sums of each row tile."""
    out = np.asarray(out, np.float64)
    return np.stack([out[t:t + tile].sum(0) for t in range(0, len(out), tile)])


def ordered_mean64(out, tile):
    """g2s_rows_mean over partial_sums64: tiles added in ascending order, divided by N."""
    s = np.zeros(np.shape(out)[1])
    for row in partial_sums64(out, tile):
        s = s + row
    return s / len(out)


def quantise(x):
    """save_image(normalize=True, range=(-1, 1)) on a float32 array [B, 3, H, W], each step rounded to float32 ->
    uint8 [B, H, W, 3]."""
    x = np.asarray(x, np.float32)
    one, two = np.float32(1), np.float32(2)
    x = (np.clip(x, -one, one) + one) / two
    x = np.clip(x * np.float32(255) + np.float32(0.5), np.float32(0), np.float32(255))
    return np.moveaxis(x.astype(np.uint8), 1, -1).copy()


# ------------------------------------------------------------------------------------------------------ inputs
def mapping_inputs(N, D, L, seed=0, zero_row=None):
    """float32 z [N, D], raw weights [L, D, D] (as EqualLinear draws them: randn / lr_mul) and biases [L, D]."""
    rng = np.random.default_rng([41, N, D, L, seed])
    z = rng.standard_normal((N, D)).astype(np.float32)
    if zero_row is not None:
        z[zero_row] = 0
    w = (rng.standard_normal((L, D, D)) / LR_MLP).astype(np.float32)
    b = (rng.standard_normal((L, D)) * 10).astype(np.float32)      # * lr_mul: biases of 0.1, as fill_deterministic's
    return z, w, b


def mapping_cases(T):
    """(name, N, D, L, options) for a tile height T: one row, the tile edge and one past it, more than one workgroup
    with a ragged last tile at the product's size, few rows at the product's size, truncation, a row of zeros."""
    return [
        ("n1", 1, 32, 1, {}),
        ("tile", T, 64, 2, {}),
        ("tile+1", T + 1, 64, 2, {}),
        ("2tile+1.d512", 2 * T + 1, 512, 8, {}),
        ("n5.d512", 5, 512, 8, {}),
        ("truncation", T + 3, 96, 3, {"truncation": TRUNCATION}),
        ("zero-row", 4, 64, 2, {"zero_row": 2}),
    ]


def image_inputs(B, H, W, seed=0):
    """float32 [B, 3, H, W] over [-1.5, 1.5] with exact -1, 1, 0 and values whose * 255 + 0.5 lands on an integer
    ((2 k + 1) / 255 - 1 up to rounding, and k / 127.5 - 1 half-way cases) sprinkled in.  No NaN."""
    rng = np.random.default_rng([43, B, H, W, seed])
    x = rng.uniform(-1.5, 1.5, (B, 3, H, W)).astype(np.float32)
    flat = x.reshape(-1)
    k = np.arange(256, dtype=np.float64)
    special = np.concatenate([[-1.0, 1.0, 0.0, -0.0, -1.5, 1.5], (k + 0.5) / 127.5 - 1, k / 127.5 - 1]).astype(np.float32)
    idx = rng.permutation(flat.size)[:min(flat.size // 2, special.size)]
    flat[idx] = special[:idx.size]
    return x


IMAGE_SHAPES = [(1, 4, 4), (2, 8, 12), (1, 128, 128), (2, 5, 7), (1, 6, 6)]   # (2,5,7), (1,6,6): W no multiple of 4
