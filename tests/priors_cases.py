"""Shared by tests/test_priors_cpu.py and tests/test_gpu_priors.py: the mask sources of the batch tests and
a float64 restatement of the two priors that are more than one expression (PriorGenerator._smooth and
._ellipsoid_prior, GAN2Shape/priors.py:47-97)."""
import math

import numpy as np
import torch

from model_cases import parsing_mask

NEAR, FAR, THRESHOLD, RADIUS, TAPS, PASSES = 0.91, 1.02, 0.7, 0.4, 11, 3
# the bound the project holds the host path to against the reference fixtures (test_host_cpu.test_priors_golden)
RTOL, ATOL = 2e-6, 1e-6

# (cx, cy, rx, ry) of parsing_mask: different centres and radii; the fourth ellipse runs over the right
# and the bottom border of the image
BATCH_MASKS = [(0.55, 0.45, 0.3, 0.38), (0.4, 0.5, 0.25, 0.3), (0.5, 0.6, 0.35, 0.2), (0.85, 0.8, 0.3, 0.4),
               (0.3, 0.35, 0.2, 0.25)]


# the map each smoothed prior smooths (priors.py:69-72,105-107)
SMOOTHED_FROM = {"smoothed_box": "masked_box", "smoothed_confidence": "confidence"}


def batch_masks(size):
    """(5, 1, S, S) soft masks in [0, 1]."""
    return torch.cat([parsing_mask(size, *p) for p in BATCH_MASKS])


def first_channel(image):
    """Mask source that is a pure function of the image: its first channel (the batch tests put the
    mask there).  Accepts one image or a batch."""
    return image[:, :1]


def images_of(masks):
    """(B, 3, S, S) images whose first channel is the mask."""
    return masks.expand(-1, 3, -1, -1).contiguous()


def smooth64(prior, taps=TAPS, passes=PASSES, near=NEAR, far=FAR):
    """float64 PriorGenerator._smooth of one (S, S) map: direct 121-tap sums."""
    x = np.asarray(prior, np.float64)
    h = taps // 2
    for _ in range(passes):
        S = x.shape[0]
        V = S - taps + 1
        f = np.zeros((V, V))
        for i in range(taps):
            for j in range(taps):
                f += x[i:i + V, j:j + V]
        f /= taps
        lo, hi = f.min(), f.max()
        x = np.full((S, S), float(far))
        x[h:S - h, h:S - h] = near + (f - lo) * (far - near) / (hi - lo)
    return x


def ellipsoid64(mask, threshold=THRESHOLD, radius=RADIUS, near=NEAR, far=FAR):
    """float64 PriorGenerator._ellipsoid_prior of one (S, S) fp32 mask (the comparison with the threshold is
    the fp32 one, like the host path's)."""
    mask = np.asarray(mask, np.float32)
    S = mask.shape[0]
    ys, xs = np.nonzero(mask >= np.float32(threshold))
    top, bottom, right, left = float(ys.max()), float(ys.min()), float(xs.max()), float(xs.min())
    half_width = (right - left) / 2
    aspect = (top - bottom) / (right - left)
    cx, cy = (right + left) / 2, (top + bottom) / 2
    axis = np.arange(S, dtype=np.float64)
    rows = (axis[:, None] - S / 2) / aspect + S / 2
    dist = np.sqrt((rows - cy) ** 2 + (axis[None, :] - cx) ** 2)
    rim = math.sqrt(radius ** 2 - (radius - (far - near)) ** 2)
    rho = dist / half_width * rim
    cap = radius - np.sqrt(np.abs(radius ** 2 - rho ** 2)) + near
    return np.where(dist <= half_width, cap, float(far))

