"""Cases of the parsing-network tests (tests/golden/make_parsing_golden.py writes the reference's results to
tests/golden/parsing.npz; test_parsing_cpu.py and test_gpu_parsing.py read them): the seed recipe of the weights and
inputs (no weight is stored), and float64 torch restatements of MaskingModel's rules in this package's own words —
the oracle of the kernel tests."""
import math

import numpy as np
import torch
import torch.nn.functional as F

# net -> (constructor arguments, input side of the logits case, `size` of the MaskingModel case, category, weight seed)
NETS = {
    "bisenet": dict(side=128, category="face", weight_seed=0),
    "pspnet": dict(side=97, category="car", weight_seed=16),
}
B = 2
S = 32                  # image side of the MaskingModel cases: resized up to `side`, masks area-averaged back to S
N_SEEDS = 16            # ref_fp32_err is the maximum over this many inputs
MARGIN_REL = 1e-4       # a pixel whose float64 top-2 margin is below MARGIN_REL * max|logit| may flip in float32
EXCLUDED_CAP = 1e-3     # and such pixels are at most this share of all pixels (a condition on the inputs)
NET_ERR_FACTOR = 4.0    # whole-net bound: this many times the reference's own float32-vs-float64 error


def seeded_state(state, seed):
    """The recipe of the weights: walk the state dict in sorted key order with one numpy Generator; 4-D weights
    N(0, 2 / fan_in), BatchNorm weight and running_var U(0.5, 1.5), BatchNorm bias, running_mean and convolution
    biases U(-0.2, 0.2), all rounded to float32; counters stay."""
    rng = np.random.default_rng(seed)
    out = {}
    for key in sorted(state):
        v = state[key]
        shape = tuple(v.shape)
        if not v.dtype.is_floating_point:
            out[key] = v.clone()
            continue
        if v.dim() == 4:
            a = rng.standard_normal(shape) * math.sqrt(2.0 / (shape[1] * shape[2] * shape[3]))
        elif key.endswith("running_var") or key.endswith(".weight"):
            a = rng.uniform(0.5, 1.5, shape)
        else:
            a = rng.uniform(-0.2, 0.2, shape)
        out[key] = torch.from_numpy(a.astype(np.float32))
    return out


def fill(net, seed):
    state = seeded_state(net.state_dict(), seed)
    net.load_state_dict({k: v.to(net.state_dict()[k].dtype) for k, v in state.items()})
    return net


def images(name, side, seed=0):
    """(B, 3, side, side) float32 images in [-1, 1]: smooth blobs plus noise, distinct per sample."""
    rng = np.random.default_rng([len(name), side, seed])
    coarse = torch.from_numpy(rng.uniform(-1, 1, (B, 3, 5, 5)))
    smooth = F.interpolate(coarse, (side, side), mode="bicubic", align_corners=True).clamp(-1, 1)
    noise = torch.from_numpy(rng.uniform(-1, 1, (B, 3, side, side)))
    return (0.7 * smooth + 0.3 * noise).float()


def state_list(state, skip=()):
    """Ordered 'name shape' strings of a state dict."""
    return np.array([f"{k} {tuple(v.shape)}" for k, v in state.items() if not k.startswith(tuple(skip))])


def l2_rel(a, ref):
    return float((a.double() - ref.double()).norm() / ref.double().norm())


# ----------------------------------------------------------------------------- MaskingModel's rules, float64
FACE_DROP = 17
FACE_CLASSES = tuple(range(1, 14))
FACE_CONFIDENCE = tuple(range(1, 13))
VOC = ['aeroplane', 'bicycle', 'bird', 'boat', 'bottle', 'bus', 'car', 'cat', 'chair', 'cow', 'diningtable', 'dog',
       'horse', 'motorbike', 'person', 'pottedplant', 'sheep', 'sofa', 'train', 'tvmonitor']


def rule_of(category):
    """(dropped channel or -1, classes of the hard mask, channels of the confidence sum)."""
    if category == "face":
        return FACE_DROP, FACE_CLASSES, FACE_CONFIDENCE
    n = VOC.index(category) + 1
    return -1, (n,), (n,)


def as_set(classes):
    return sum(1 << c for c in classes)


def hard_oracle(logits, drop, classes, S_out):
    """From float64 full-resolution logits (B, C, size, size): the bool mask (with the per-sample all-ones
    fallback), the (B,) fallback flags, the top-2 margin after the channel drop, and the area-averaged
    (B, 1, S_out, S_out) mask."""
    z = logits.double().clone()
    if drop >= 0:
        z[:, drop] = float("-inf")
    top = z.topk(2, dim=1).values
    margin = top[:, 0] - top[:, 1]
    member = torch.zeros(z.shape[1], dtype=torch.bool)
    member[list(classes)] = True
    mask = member[z.argmax(1, keepdim=True)]
    empty = ~mask.flatten(1).any(1)
    mask = mask | empty[:, None, None, None]
    return mask, empty, margin, F.adaptive_avg_pool2d(mask.double(), S_out)


def confidence_oracle(logits, channels, S_out):
    v = logits.double()[:, list(channels)].sum(1, keepdim=True)
    v = v - v.amin((1, 2, 3), keepdim=True)
    v = v / v.amax((1, 2, 3), keepdim=True)
    return F.adaptive_avg_pool2d(v, S_out)


def upsample64(low, size):
    return F.interpolate(low.double(), (size, size), mode="bilinear", align_corners=True)


def excluded_pixels(logits, margin):
    """Bool (B, size, size): pixels whose margin is below MARGIN_REL * max|logit| (max over the whole tensor)."""
    return margin < MARGIN_REL * float(logits.abs().max())


def soft_bound(excluded, S_out):
    """Per output pixel: (excluded pixels in its area bin) / (bin area) + 1e-6."""
    return F.adaptive_avg_pool2d(excluded.double()[:, None], S_out) + 1e-6
