"""What a GAN training run shows of its generator while it runs: sample grids and the perceptual path length.

    grid = image_grid(images, nrow=8)                       # [N, C, H, W] float32 -> uint8 [Hg, Wg, 3]
    save_grid(images, "sample/000100.png", nrow=8)          # torchvision.utils.save_image(normalize=True, range=(-1, 1))
    out = ppl_latents(pairs, t, eps, "w")                   # [2B, D], [B] -> [2B, D]: the points at t and at t + eps
    r = perceptual_path_length(G, percept, 5000)            # {'ppl', 'n', 'kept', 'lo', 'hi', 'distances'}

`image_grid` is torchvision's make_grid followed by save_image's quantiser (torchvision is not a dependency): image
k of the batch sits in row k // xmaps, column k % xmaps of a grid of xmaps = min(nrow, N) columns, `padding` pixels of
`pad_value` around and between the cells; one image comes back bare.  On the device it is ONE launch of
g2s_image_grid_u8 (csrc/monitor.hip), so a quarter of the bytes of the samples, already laid out, crosses to the host.

The perceptual path length is StyleGAN2's own measure of a generator (the vendored stylegan2-pytorch/ppl.py): the
LPIPS distance of two images whose latents lie `eps` apart on a line between two random latents (w space), or on a
great circle between two random z, divided by eps^2; the mean over the samples between the 1st and 99th percentile.
`ppl_latents` builds both ends of every pair in ONE launch of g2s_ppl_latents; the generator runs its one-node path
on the 2b latents with one shared set of noise maps, LPIPS its batch-2N trunk.  Generators of 512 pixels and more are
reduced to 256 x 256 (bilinear, align_corners=False), together with the optional car crop, by ONE launch of
op.resample.resample_sep on the band tables `ppl_resize_tables` makes.

CPU tensors take torch compositions of the same arithmetic throughout, as in op/cpu_tensors.py."""
import math

import numpy as np
import torch
import torch.nn.functional as F

from . import generate, lib

SPACES = ("w", "z")
SAMPLINGS = ("full", "end")


# ------------------------------------------------------------------------------------------------------ the grid
def grid_shape(N, H, W, nrow=8, padding=2):
    """(xmaps, ymaps, Hg, Wg) of make_grid; one image has no border."""
    if N == 1:
        return 1, 1, H, W
    xmaps = min(int(nrow), N)
    ymaps = -(-N // xmaps)
    return xmaps, ymaps, ymaps * (H + padding) + padding, xmaps * (W + padding) + padding


def pad_byte(pad_value):
    """uint8(clamp(pad_value * 255 + 0.5, 0, 255)) in float32, as the kernel's launcher computes it."""
    v = np.float32(pad_value) * np.float32(255) + np.float32(0.5)
    return int(np.uint8(min(max(v, np.float32(0)), np.float32(255))))


def _image_grid_torch(images, nrow, padding, lo, hi, pad_value):
    N, C, H, W = images.shape
    den = float(max(np.float32(hi) - np.float32(lo), np.float32(1e-5)))
    u = images.clamp(lo, hi).sub(lo).div(den)
    q = u.mul(255).add(0.5).clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1)
    if C == 1:
        q = q.expand(N, H, W, 3)
    if N == 1:
        return q[0].contiguous()
    xmaps, ymaps, Hg, Wg = grid_shape(N, H, W, nrow, padding)
    grid = torch.full((Hg, Wg, 3), pad_byte(pad_value), dtype=torch.uint8, device=images.device)
    for k in range(N):
        y0, x0 = (k // xmaps) * (H + padding) + padding, (k % xmaps) * (W + padding) + padding
        grid[y0:y0 + H, x0:x0 + W] = q[k]
    return grid


def image_grid(images, nrow=8, padding=2, value_range=(-1.0, 1.0), pad_value=0.0, out=None):
    """[N, C, H, W] float32, C in {1, 3} -> uint8 [Hg, Wg, 3]: save_image(images, nrow=nrow, padding=padding,
    normalize=True, range=value_range, pad_value=pad_value) up to its uint8.  One launch on the device; `out`: a
    contiguous uint8 tensor of the result's shape to write into (every byte is written)."""
    if images.dim() != 4 or images.shape[1] not in (1, 3) or images.dtype != torch.float32:
        raise ValueError(f"image_grid takes float32 [N, C, H, W] with C in (1, 3), got {images.dtype} {tuple(images.shape)}")
    N, C, H, W = images.shape
    if N < 1 or H < 1 or W < 1 or int(nrow) < 1 or int(padding) < 0:
        raise ValueError("image_grid needs N, H, W, nrow >= 1 and padding >= 0")
    lo, hi = float(value_range[0]), float(value_range[1])
    if any(math.isnan(v) for v in (lo, hi, float(pad_value))):
        raise ValueError("image_grid: value_range and pad_value must not be NaN")
    nrow, padding = int(nrow), int(padding)
    if not images.is_cuda:
        grid = _image_grid_torch(images, nrow, padding, lo, hi, float(pad_value))
        return grid if out is None else out.copy_(grid)
    _, _, Hg, Wg = grid_shape(N, H, W, nrow, padding)
    if out is None:
        out = torch.empty(Hg, Wg, 3, dtype=torch.uint8, device=images.device)
    elif (tuple(out.shape) != (Hg, Wg, 3) or out.dtype != torch.uint8 or out.device != images.device
          or not out.is_contiguous()):
        raise ValueError(f"out must be a contiguous uint8 {(Hg, Wg, 3)} tensor on {images.device}")
    images = images.contiguous()
    lib.check(lib.load().g2s_image_grid_u8(lib.ptr(images), lib.ptr(out), N, C, H, W, nrow, padding, lo, hi,
                                           float(pad_value), lib.stream()))
    return out


def save_grid(images, path, nrow=8, **kw):
    """Write image_grid(images, nrow, **kw) as a PNG; returns the uint8 array written."""
    from PIL import Image
    pixels = image_grid(images, nrow, **kw).cpu().numpy()
    Image.fromarray(pixels).save(path)
    return pixels


# ------------------------------------------------------------------------------------------- path-length latents
def _unit(x):
    return x / x.pow(2).sum(-1, keepdim=True).sqrt()


def _ppl_latents_torch(pairs, t, eps, space):
    a, b = pairs[0::2], pairs[1::2]
    t0 = t[:, None]
    t1 = (t + eps)[:, None]            # a float32 tensor add: t1 is rounded to the dtype of t
    out = torch.empty_like(pairs)
    if space == "w":
        out[0::2], out[1::2] = a + (b - a) * t0, a + (b - a) * t1
        return out
    a, b = _unit(a), _unit(b)
    d = (a * b).sum(-1, keepdim=True)
    om = torch.acos(d)
    c = _unit(b - d * a)
    out[0::2] = _unit(a * torch.cos(t0 * om) + c * torch.sin(t0 * om))
    out[1::2] = _unit(a * torch.cos(t1 * om) + c * torch.sin(t1 * om))
    return out


def ppl_latents(pairs, t, eps, space, out=None):
    """pairs [2B, D] (rows 2i, 2i + 1: the ends of pair i), t [B] -> [2B, D]: row 2i the point at t[i], row 2i + 1
    the point at t[i] + eps (the sum rounded to float32).  space 'w': a + (b - a) t; 'z': slerp of the normalised
    ends.  One launch of g2s_ppl_latents on the device; `out`: a contiguous tensor like pairs to write into."""
    if space not in SPACES:
        raise ValueError(f"space must be one of {SPACES}, got {space!r}")
    if pairs.dim() != 2 or pairs.shape[0] % 2 or pairs.shape[0] < 2 or pairs.shape[1] < 1:
        raise ValueError(f"ppl_latents takes pairs [2B, D], got {tuple(pairs.shape)}")
    B, D = pairs.shape[0] // 2, pairs.shape[1]
    if tuple(t.shape) != (B,) or t.device != pairs.device or t.dtype != pairs.dtype:
        raise ValueError(f"t must be [{B}] on {pairs.device} with the dtype of pairs, got {t.dtype} {tuple(t.shape)} on {t.device}")
    if not pairs.is_cuda or pairs.dtype != torch.float32:
        r = _ppl_latents_torch(pairs, t, eps, space)
        return r if out is None else out.copy_(r)
    pairs, t = pairs.contiguous(), t.contiguous()
    if out is None:
        out = torch.empty_like(pairs)
    elif out.shape != pairs.shape or out.dtype != torch.float32 or out.device != pairs.device or not out.is_contiguous():
        raise ValueError("out must be a contiguous float32 tensor like pairs")
    if out.data_ptr() == pairs.data_ptr():
        raise ValueError("ppl_latents does not work in place")
    lib.check(lib.load().g2s_ppl_latents(lib.ptr(pairs), lib.ptr(t), float(eps), SPACES.index(space), lib.ptr(out),
                                         B, D, lib.stream()))
    return out


# ------------------------------------------------------------------------------------------- crop and 256 x 256
def crop_box(S):
    """(y0, y1, x0, x1) of ppl.py's --crop on an S x S image: rows 3c .. 7c, columns 2c .. 6c with c = S // 8."""
    c = S // 8
    return 3 * c, 7 * c, 2 * c, 6 * c


def bilinear_matrix(n_in, n_out, offset=0, n_src=None):
    """float64 [n_out, n_src]: F.interpolate(mode='bilinear', align_corners=False, no antialiasing) from n_in to n_out
    positions along one axis, reading positions offset .. offset + n_in - 1 of a source of n_src positions."""
    n_src = n_in + offset if n_src is None else n_src
    A = np.zeros((n_out, n_src), dtype=np.float64)
    scale = n_in / n_out
    for i in range(n_out):
        src = max((i + 0.5) * scale - 0.5, 0.0)
        i0 = min(int(math.floor(src)), n_in - 1)
        i1 = min(i0 + 1, n_in - 1)
        lam = src - i0
        A[i, offset + i0] += 1.0 - lam
        A[i, offset + i1] += lam
    return A


def bilinear_bands(n_in, n_out, offset=0, n_src=None):
    """(lo, len, w float32 [n_out, K]) of `bilinear_matrix` for op.resample.make_bands.  A two-tap band that ends short
    of the next band's start (a reduction by more than 2) is widened up to it with zero weights: consecutive bands of
    g2s_resample_sep must overlap or abut."""
    A = bilinear_matrix(n_in, n_out, offset, n_src)
    lo = np.array([np.flatnonzero(row)[0] for row in A], dtype=np.int32)
    ln = np.array([np.flatnonzero(row)[-1] for row in A], dtype=np.int32) - lo + 1
    ln[:-1] = np.maximum(ln[:-1], lo[1:] - lo[:-1])
    w = np.zeros((n_out, int(ln.max())), dtype=np.float32)
    for i in range(n_out):
        w[i, :ln[i]] = A[i, lo[i]:lo[i] + ln[i]].astype(np.float32)
    return lo, ln, w


_resize_tables = {}


def ppl_resize_tables(S, crop, device, size=256):
    """(ybands, xbands) for op.resample.resample_sep: the crop of `crop_box` (when `crop`) composed with the bilinear
    resize of what is left to size x size.  Cached per (S, crop, size, device); build them before a capture."""
    from .op import resample
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    key = (int(S), bool(crop), int(size), str(device))
    tab = _resize_tables.get(key)
    if tab is None:
        y0, y1, x0, x1 = crop_box(S) if crop else (0, S, 0, S)
        tab = _resize_tables[key] = tuple(
            resample.make_bands(*bilinear_bands(b - a, size, a, S), n_in=S, device=device)
            for a, b in ((y0, y1), (x0, x1)))
    return tab


def ppl_images(image, crop=False):
    """Steps 6 and 7 of the path length: the car crop, then 256 x 256 when what is left has 512 rows or more."""
    S = image.shape[2]
    y0, y1, x0, x1 = crop_box(S) if crop else (0, S, 0, image.shape[3])
    if (y1 - y0) // 256 > 1:
        if image.is_cuda and image.dtype == torch.float32 and image.shape[3] == S:
            from .op import resample
            return resample.resample_sep(image, *ppl_resize_tables(S, crop, image.device))
        return F.interpolate(image[:, :, y0:y1, x0:x1], size=(256, 256), mode="bilinear", align_corners=False)
    return image[:, :, y0:y1, x0:x1] if crop else image


# ------------------------------------------------------------------------------------------------- the path length
def ppl_draw(G, b, sampling="full", generator=None):
    """The draws of one batch of b pairs, in order: one [1, 1, r, r] noise map per styled layer (shared by the batch),
    z [2b, D], t [b] (uniform for 'full', zeros for 'end')."""
    device = G.input.input.device
    noise = [torch.randn(1, 1, r, r, device=device, generator=generator) for r in generate.noise_sides(G)]
    z = torch.randn(2 * b, G.style_dim, device=device, generator=generator)
    t = torch.rand(b, device=device, generator=generator) if sampling == "full" else torch.zeros(b, device=device)
    return noise, z, t


def trimmed_mean(distances):
    """(mean of the distances within [lo, hi], lo, hi, number kept): lo the 1st percentile with 'lower', hi the 99th
    with 'higher' interpolation, in float64."""
    d = np.asarray(distances, dtype=np.float64)
    lo = float(np.percentile(d, 1, method="lower"))
    hi = float(np.percentile(d, 99, method="higher"))
    kept = d[(lo <= d) & (d <= hi)]
    return float(kept.mean()), lo, hi, int(kept.size)


def perceptual_path_length(G, percept, n_samples, batch=64, space="w", sampling="full", eps=1e-4, crop=False,
                           generator=None, draws=None):
    """StyleGAN2's perceptual path length of G under the LPIPS metric `percept`, over n_samples pairs in batches of
    `batch` (the last one shorter).  `draws`: a list with one (noise, z, t) per batch, as `ppl_draw` returns them, to
    use instead of fresh draws from `generator`.  Returns {'ppl', 'n', 'kept', 'lo', 'hi', 'distances'}; the
    distances are float64 numpy, read from the device once.  A non-finite distance raises FloatingPointError."""
    if space not in SPACES or sampling not in SAMPLINGS:
        raise ValueError(f"space must be one of {SPACES} and sampling one of {SAMPLINGS}")
    if int(n_samples) < 1 or int(batch) < 1:
        raise ValueError("perceptual_path_length needs n_samples >= 1 and batch >= 1")
    sizes = [min(int(batch), int(n_samples) - s) for s in range(0, int(n_samples), int(batch))]
    if draws is not None and len(draws) != len(sizes):
        raise ValueError(f"{len(sizes)} batches need {len(sizes)} draws, got {len(draws)}")
    dists = []
    with torch.no_grad():
        for k, b in enumerate(sizes):
            noise, z, t = ppl_draw(G, b, sampling, generator) if draws is None else draws[k]
            if z.shape[0] != 2 * b or t.shape[0] != b:
                raise ValueError(f"batch {k}: draws for {b} pairs expected, got z {tuple(z.shape)}, t {tuple(t.shape)}")
            if space == "w":
                latents = ppl_latents(generate.map_latents(G, z), t, eps, "w")
            else:
                latents = generate.map_latents(G, ppl_latents(z, t, eps, "z"))
            image, _ = G([latents], input_is_w=True, noise=list(noise))
            image = ppl_images(image, crop)
            dists.append(percept(image[0::2], image[1::2]).view(b) / (eps ** 2))
    d = torch.cat(dists).double().cpu().numpy()
    if not np.isfinite(d).all():
        bad = int(np.flatnonzero(~np.isfinite(d))[0])
        raise FloatingPointError(f"perceptual_path_length: batch {bad // int(batch)} gave a distance that is not finite")
    ppl, lo, hi, kept = trimmed_mean(d)
    return {"ppl": ppl, "n": int(d.size), "kept": kept, "lo": lo, "hi": hi, "distances": d}
