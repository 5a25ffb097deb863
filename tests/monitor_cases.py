"""Cases of the training monitor's tests (test_monitor_cpu.py, test_gpu_monitor.py) and float64 numpy statements of
what monitor.py computes, written from its specification: the sample grid (`grid64`), the path-length latents
(`latents64`, which takes the float32-rounded t1), the percentile filter (`trimmed_mean64`), and the path-length loop
in plain torch at any dtype (`ppl_loop`)."""
import math

import numpy as np
import torch
import torch.nn.functional as F

import generate_cases as gc
import projector_cases as pc

# --------------------------------------------------------------------------------------------------------- grid
# (N, C, H, W, nrow, padding, pad_value)
GRID_SHAPES = [
    (1, 3, 4, 4, 8, 2, 0.0),
    (5, 3, 5, 7, 2, 2, 0.0),         # odd W, last row partly empty
    (4, 1, 6, 6, 4, 0, 0.0),         # grey, no padding
    (7, 3, 8, 12, 3, 1, 0.3),
    (64, 3, 16, 16, 8, 2, 1.0),
]
NEAR = 2.0 ** -16      # a float64 pre-truncation value this close to an integer may fall on either side in float32
CAP = 0.01             # of the pixels of a case


def grid_geometry(N, H, W, nrow, padding):
    if N == 1:
        return 1, 1, H, W
    xmaps = min(nrow, N)
    ymaps = int(math.ceil(N / xmaps))
    return xmaps, ymaps, ymaps * (H + padding) + padding, xmaps * (W + padding) + padding


def raw64(x, lo=-1.0, hi=1.0):
    """u * 255 + 0.5 in float64, before its clamp to [0, 255]."""
    x = np.asarray(x, np.float64)
    return (np.clip(x, lo, hi) - lo) / max(hi - lo, 1e-5) * 255 + 0.5


def pre64(x, lo=-1.0, hi=1.0):
    """The value whose truncation is the byte, float64."""
    return np.clip(raw64(x, lo, hi), 0, 255)


def grid64(x, nrow=8, padding=2, lo=-1.0, hi=1.0, pad_value=0.0):
    """(bytes uint8 [Hg, Wg, 3], pre float64 [Hg, Wg, 3]): the grid and, at image pixels, the float64 value that was
    truncated (NaN at pad pixels, whose byte involves no rounding question)."""
    x = np.asarray(x)
    N, C, H, W = x.shape
    pre = np.moveaxis(pre64(x, lo, hi), 1, -1)                  # [N, H, W, C]
    if C == 1:
        pre = np.repeat(pre, 3, axis=-1)
    if N == 1:
        return np.floor(pre[0]).astype(np.uint8), pre[0].copy()
    xmaps, ymaps, Hg, Wg = grid_geometry(N, H, W, nrow, padding)
    pad = np.uint8(np.floor(np.clip(np.float64(pad_value) * 255 + 0.5, 0, 255)))
    out = np.full((Hg, Wg, 3), pad, np.uint8)
    where = np.full((Hg, Wg, 3), np.nan)
    for k in range(N):
        y0, x0 = (k // xmaps) * (H + padding) + padding, (k % xmaps) * (W + padding) + padding
        out[y0:y0 + H, x0:x0 + W] = np.floor(pre[k]).astype(np.uint8)
        where[y0:y0 + H, x0:x0 + W] = pre[k]
    return out, where


def quantise32(x, lo=-1.0, hi=1.0):
    """The byte of each value with every step rounded to float32 (numpy): the model by which `grid_inputs` picks
    boundary values that a float32 route resolves as float64 does."""
    f = np.float32
    x = np.asarray(x, f)
    u = (np.clip(x, f(lo), f(hi)) - f(lo)) / np.maximum(f(hi) - f(lo), f(1e-5))
    return np.clip(u * f(255) + f(0.5), f(0), f(255)).astype(np.uint8)


def grid_inputs(N, C, H, W, seed=0):
    """float32 [N, C, H, W] over [-1.5, 1.5] (a third of the values outside [-1, 1]) with exact -1, 1, 0 and values ON
    quantisation boundaries, v = 2 (k + 0.5) / 255 - 1 rounded to float32, sprinkled in.

    The float64 pre-truncation value of a boundary input is within 127.5 * 2^-25 = 3.8e-6 of an integer, inside NEAR:
    a float32 route may resolve it either way.  So that the float32 arithmetic itself stays under CAP at every size,
      * floor(0.9 % of the images' pixels) boundary values are taken as they come (64 x 16 x 16: 147 of them),
      * further ones (at least 4) only where `quantise32` agrees with float64, so the small cases have them too,
      * an ordinary value whose float64 pre-truncation value is within 2^-12 of an integer is moved a quarter of a
        quantisation cell up: the float32 steps (subtract, divide, multiply by 255, add 0.5) err by at most
        255 * 2^-25 + 2 * 2^-17 = 2.3e-5 in total, 10 times less, so no ordinary value sits in doubt."""
    rng = np.random.default_rng([47, N, C, H, W, seed])
    x = rng.uniform(-1.5, 1.5, (N, C, H, W)).astype(np.float32)
    flat = x.reshape(-1)
    frac = np.abs(raw64(flat) - np.round(raw64(flat)))          # 0.5 outside [-1, 1], where the first clamp decides
    flat[frac < 2.0 ** -12] += np.float32(0.5 / 255)
    assert (np.abs(raw64(flat) - np.round(raw64(flat))) >= 2.0 ** -12).all()
    k = rng.permutation(255)
    bound = (2 * (k + 0.5) / 255 - 1).astype(np.float32)
    agree = bound[quantise32(bound) == np.floor(pre64(bound)).astype(np.uint8)]
    n_free = int(0.009 * (H * W * N))                 # fewer than CAP of the grid's pixels (the grid has more than N H W)
    n_safe = max(4, flat.size // 100)
    special = np.concatenate([np.float32([-1.0, 1.0, 0.0, -0.0, -1.5, 1.5]), bound[:n_free], np.resize(agree, n_safe)])
    special = special[:flat.size // 2]
    idx = rng.permutation(flat.size)[:special.size]
    flat[idx] = special
    return x


def check_grid(got, want, pre, what=""):
    """Bytes equal to the oracle's; where the float64 pre-truncation value is within NEAR of an integer a byte may
    differ by one, at no more than CAP of the pixels.  Returns the number of differing pixels."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == np.uint8, (what, got.shape, want.shape, got.dtype)
    diff = got != want
    near = np.abs(pre - np.round(pre)) <= NEAR                  # NaN (pad pixels): False
    assert not (diff & ~near).any(), (what, np.argwhere(diff & ~near)[:4].tolist())
    assert (np.abs(got.astype(np.int64) - want.astype(np.int64))[diff] == 1).all(), what
    pixels = int(diff.any(-1).sum())
    assert pixels <= CAP * got.shape[0] * got.shape[1], (what, pixels, got.shape)
    return pixels


# ------------------------------------------------------------------------------------------------------ latents
LATENT_SHAPES = [(1, 32), (3, 33), (2, 512), (5, 7)]
EPS = 1e-4


def t1_of(t, eps):
    """t + eps as a float32 tensor add rounds it."""
    return (np.asarray(t, np.float32) + np.float32(eps)).astype(np.float32)


def _unit64(x):
    return x / np.sqrt((x * x).sum(-1, keepdims=True))


def latents64(pairs, t, t1, space):
    """[2B, D] float64: row 2i the point of pair i at t[i], row 2i + 1 the point at t1[i] (given, already rounded)."""
    p = np.asarray(pairs, np.float64)
    a, b = p[0::2], p[1::2]
    out = np.empty_like(p)
    for rows, tt in ((slice(0, None, 2), t), (slice(1, None, 2), t1)):
        tt = np.asarray(tt, np.float64)[:, None]
        if space == "w":
            out[rows] = a + (b - a) * tt
        else:
            ua, ub = _unit64(a), _unit64(b)
            d = (ua * ub).sum(-1, keepdims=True)
            ph = tt * np.arccos(d)
            c = _unit64(ub - d * ua)
            out[rows] = _unit64(ua * np.cos(ph) + c * np.sin(ph))
    return out


def latent_inputs(B, D, seed=0):
    """float32 pairs [2B, D] and t [B]: t[0] = 0, t[1] close to 1, the rest uniform; with B > 1 the LAST pair's ends are nearly
    parallel (b = 1.3 a + 1e-3 noise: d within 1e-6 of 1, where acos and b - d a are badly conditioned)."""
    rng = np.random.default_rng([53, B, D, seed])
    pairs = rng.standard_normal((2 * B, D)).astype(np.float32)
    if B > 1:
        pairs[-1] = (1.3 * pairs[-2] + 1e-3 * rng.standard_normal(D)).astype(np.float32)
    t = rng.uniform(0, 1, B).astype(np.float32)
    t[0] = 0.0
    if B > 1:
        t[1] = np.float32(1.0 - 2.0 ** -20)
    return pairs, t


# ----------------------------------------------------------------------------------------------- percentile filter
def trimmed_mean64(d):
    """(mean, lo, hi, kept): lo = the 1st percentile with 'lower', hi = the 99th with 'higher' interpolation, the mean
    over lo <= d <= hi — by sorting, without numpy.percentile."""
    d = np.sort(np.asarray(d, np.float64))
    n = len(d)
    lo = d[int(math.floor(0.01 * (n - 1)))]
    hi = d[int(math.ceil(0.99 * (n - 1)))]
    kept = d[(d >= lo) & (d <= hi)]
    return float(kept.mean()), float(lo), float(hi), int(len(kept))


# ------------------------------------------------------------------------------------------------- the path length
# The LPIPS trunk pools four times, so an 8 x 8 image (generate_cases.G_CFG as it stands) leaves it nothing at the last
# slice (torch refuses the 1 x 1 -> 0 x 0 pool): the small generator is G_CFG at size 16, the smallest the metric
# takes.  The second one has side 32.
PPL_GENERATORS = {
    "g16": dict(gc.G_CFG, size=16),
    "g32": dict(size=32, style_dim=32, n_mlp=4, channel_multiplier=1, seed=37),
}
PPL_N, PPL_BATCH = 6, 4            # a full batch and a short one
PPL_SEEDS = {"percept": 5, "draws": 11}


def ppl_generator(sg2, name):
    cfg = PPL_GENERATORS[name]
    return pc.fixture_generator(sg2, cfg["size"], cfg["style_dim"], cfg["n_mlp"], cfg["seed"])


def ppl_percept(seed=PPL_SEEDS["percept"]):
    """PerceptualLoss with seeded random weights; the lin layers non-negative, as the trained ones are."""
    from gan2shape_amd.lpips import PerceptualLoss
    g = torch.Generator().manual_seed(seed)
    p = PerceptualLoss()
    with torch.no_grad():
        for name, t in sorted(p.state_dict().items()):
            if name.endswith("weight") and ".lin" in "." + name:
                t.copy_(torch.rand(t.shape, generator=g) / t.shape[1])
            elif name.endswith("weight"):
                fan_in = t.shape[1] * t.shape[2] * t.shape[3]
                t.copy_(torch.randn(t.shape, generator=g) * math.sqrt(2.0 / fan_in))
            elif name.endswith("bias"):
                t.copy_(0.05 * torch.randn(t.shape, generator=g))
    return p.eval()


def ppl_draws(G, sampling="full", seed=PPL_SEEDS["draws"], n=PPL_N, batch=PPL_BATCH):
    """CPU float32 draws, one (noise, z, t) per batch, made as monitor.ppl_draw orders them."""
    g = torch.Generator().manual_seed(seed)
    sides = [4] + [2 ** (3 + j // 2) for j in range(G.num_layers - 1)]
    draws = []
    for s in range(0, n, batch):
        b = min(batch, n - s)
        noise = [torch.randn(1, 1, r, r, generator=g) for r in sides]
        z = torch.randn(2 * b, G.style_dim, generator=g)
        t = torch.rand(b, generator=g) if sampling == "full" else torch.zeros(b)
        draws.append((noise, z, t))
    return draws


def draws_to(draws, device=None, dtype=None):
    return [([m.to(device=device, dtype=dtype) for m in noise], z.to(device=device, dtype=dtype),
             t.to(device=device, dtype=dtype)) for noise, z, t in draws]


def _unit(x):
    return x / x.pow(2).sum(-1, keepdim=True).sqrt()


def ppl_loop(G, percept, draws, space="w", eps=EPS, crop=False):
    """The path-length loop in plain torch, in the dtype of G and percept: per-pair distances, float64 numpy.  t1 is
    t + eps rounded to float32 whatever the dtype, as the specification has it."""
    dtype = next(G.parameters()).dtype
    out = []
    with torch.no_grad():
        for noise, z, t in draws:
            t1 = (t.float() + eps).to(dtype)[:, None]
            z, t0 = z.to(dtype), t.to(dtype)[:, None]
            noise = [m.to(dtype) for m in noise]
            ends = G.style_forward(z) if space == "w" else z
            a, b = ends[0::2], ends[1::2]
            lat = torch.empty_like(ends)
            if space == "w":
                lat[0::2], lat[1::2] = a + (b - a) * t0, a + (b - a) * t1
            else:
                a, b = _unit(a), _unit(b)
                d = (a * b).sum(-1, keepdim=True)
                om, c = torch.acos(d), _unit(b - d * a)
                lat[0::2] = _unit(a * torch.cos(t0 * om) + c * torch.sin(t0 * om))
                lat[1::2] = _unit(a * torch.cos(t1 * om) + c * torch.sin(t1 * om))
                lat = G.style_forward(lat)
            image, _ = G([lat], input_is_w=True, noise=noise)
            if crop:
                c8 = image.shape[2] // 8
                image = image[:, :, 3 * c8:7 * c8, 2 * c8:6 * c8]
            if image.shape[2] // 256 > 1:
                image = F.interpolate(image, size=(256, 256), mode="bilinear", align_corners=False)
            out.append(percept(image[0::2], image[1::2]).reshape(-1) / eps ** 2)
    return torch.cat(out).double().numpy()


# ------------------------------------------------------------------------------------------------ watching a run
TRAIN_NET = ["--channel-multiplier", "1", "--latent", "32", "--n-mlp", "2"]


def spy_on_monitor(monkeypatch, train):
    """Record, at every Monitor.after call, a copy of g_ema's state BEFORE anything is monitored, and what
    Monitor.samples returns: ([(iteration, state)], [images])."""
    states, images = [], []
    after, samples = train.Monitor.after, train.Monitor.samples

    def spy_after(self, i):
        states.append((i, {k: v.detach().clone() for k, v in self.g_ema.state_dict().items()}))
        return after(self, i)

    def spy_samples(self):
        images.append(samples(self))
        return images[-1]
    monkeypatch.setattr(train.Monitor, "after", spy_after)
    monkeypatch.setattr(train.Monitor, "samples", spy_samples)
    return states, images


def fresh_generator(sg2, size, state, device="cpu"):
    """A new Generator of TRAIN_NET's shape holding `state`: no forward has run on it, so it has derived nothing."""
    G = sg2.Generator(size, 32, 2, channel_multiplier=1)
    G.load_state_dict(state)
    return G.to(device).eval().requires_grad_(False)
