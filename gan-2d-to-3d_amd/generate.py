"""Sample a dataset from a StyleGAN2 generator — the counterpart of the reference's stylegan2-pytorch/generate.py,
which made GAN2Shape's car, cat and church data: every image comes with the latent that produced it, so no
projection is needed.

    python -m gan2shape_amd.generate --ckpt <file> --size 128 --channel-multiplier 1 --out <root>/<category>
           [--pics 20] [--sample 1] [--batched] [--truncation 0.7] [--truncation-mean 4096] [--seed 0] [--device cuda]

Written under --out, ready for `dataset.ImageLatentDataset(<out>)`:
    %06d.png          --pics * --sample images
    latents/%06d.pt   the truncated w [style_dim] of each (generate.py:20,30)
    list.txt          the image names, one per line

On the device the mapping network is ONE launch (g2s_mapping_fwd, csrc/mapping.hip: PixelNorm, the 8 linears with
their bias + leaky ReLU and the truncation lerp, the activations of a 16-row tile staying in LDS), the mean latent of
--truncation-mean samples is that launch plus g2s_rows_mean (per-tile column sums added in tile order: the same bits
on every run), and the images are quantised by g2s_image_to_u8 with save_image's arithmetic, so that a quarter of
the bytes crosses to the host.  Noise follows the reference's default (randomize_noise=True): one [n, 1, r, r] normal
draw per styled layer, in layer order.  The fused epilogues of the one-node generator read ONE noise map per launch
(DESIGN.md §4.13), so by default each sample goes through Generator.forward on its own with [1, 1, r, r] views of those
draws; --batched (sample(batched=True)) runs ONE forward for the n samples on the [n, 1, r, r] draws through the
one-node path with one map per sample (synthesis.per_sample_noise).  CPU tensors take plain torch ops throughout, as in
op/cpu_tensors.py.  `Generator.style_forward`, `Generator.mean_latent` and `projector.mean_latent_stats` are
unchanged: training's latent projection needs the mapping backward, which this kernel does not have.
"""
import argparse
import math
import os

import torch

from . import lib

# Rows from which g2s_mapping_fwd is ahead of the style_forward route (17 launches of F.linear + fused_leaky_relu) at
# D = 512, L = 8 on the MI355X: measured by tools/bench_generate.py, profiles/generate_g128.json (276 us against 343 us
# at N = 1, 278 against 338 at N = 4096: ahead at every measured N).  Below it map_latents takes the torch ops.
KERNEL_MIN_ROWS = 1

LRELU_ALPHA, LRELU_GAIN = 0.2, math.sqrt(2.0)      # fused_leaky_relu's defaults (EqualLinear, activation='fused_lrelu')


# --------------------------------------------------------------------------------------------------------- kernels
def mapping_tile():
    """Rows per workgroup tile of g2s_mapping_fwd: the height of a `partial` row."""
    return int(lib.load().g2s_mapping_tile())


def mapping_fwd(z, w, b, pixel_norm=True, alpha=LRELU_ALPHA, gain=LRELU_GAIN, center=None, truncation=1.0,
                out=None, partial=None):
    """g2s_mapping_fwd on contiguous f32 CUDA tensors: z [N, D], w [L, D, D], b [L, D] -> out [N, D]."""
    lib.require_cuda(z, w, b, center, out, partial)
    N, D = z.shape
    L = w.shape[0]
    if tuple(w.shape) != (L, D, D) or tuple(b.shape) != (L, D):
        raise ValueError(f"mapping_fwd: w {tuple(w.shape)} / b {tuple(b.shape)} do not fit z {tuple(z.shape)}")
    for t in (z, w, b, center, out, partial):
        if t is not None and (t.dtype != torch.float32 or not t.is_contiguous()):
            raise ValueError("mapping_fwd takes contiguous float32 tensors")
    if out is None:
        out = torch.empty_like(z)
    lib.check(lib.load().g2s_mapping_fwd(lib.ptr(z), lib.ptr(w), lib.ptr(b), lib.ptr(center), lib.ptr(out),
                                         lib.ptr(partial), N, D, L, int(bool(pixel_norm)), alpha, gain,
                                         float(truncation), lib.stream()))
    return out


def rows_mean(partial, n):
    """g2s_rows_mean: [tiles, D] per-tile column sums -> their sum in tile order / n, [D]."""
    lib.require_cuda(partial)
    out = torch.empty(partial.shape[1], dtype=torch.float32, device=partial.device)
    lib.check(lib.load().g2s_rows_mean(lib.ptr(partial), lib.ptr(out), partial.shape[0], partial.shape[1], n,
                                       lib.stream()))
    return out


def _quantise_torch(x):
    """torchvision.utils.save_image(normalize=True, range=(-1, 1)) up to its uint8: [B, 3, H, W] -> [B, H, W, 3]."""
    x = x.clamp(-1, 1).add(1).div(2)
    return x.mul(255).add(0.5).clamp(0, 255).permute(0, 2, 3, 1).to(torch.uint8).contiguous()


def image_to_u8(x):
    """[B, 3, H, W] float32 in [-1, 1] -> [B, H, W, 3] uint8, save_image's arithmetic (g2s_image_to_u8 on the device)."""
    if x.dim() != 4 or x.shape[1] != 3:
        raise ValueError(f"image_to_u8 takes [B, 3, H, W], got {tuple(x.shape)}")
    if not x.is_cuda:
        return _quantise_torch(x.float())
    x = x.float().contiguous()
    B, _, H, W = x.shape
    out = torch.empty(B, H, W, 3, dtype=torch.uint8, device=x.device)
    lib.check(lib.load().g2s_image_to_u8(lib.ptr(x), lib.ptr(out), B, H, W, lib.stream()))
    return out


# --------------------------------------------------------------------------------------------------------- mapping
def mapping_weights(G):
    """(w [L, D, D], b [L, D]) of G's mapping network, multiplied by EqualLinear.scale / lr_mul; rebuilt only when a
    weight or bias changes (pointer and _version, as Generator._batched_styles caches its stacks)."""
    layers = list(G.style)[1:]
    key = tuple((m.weight.data_ptr(), m.weight._version, m.bias.data_ptr(), m.bias._version) for m in layers)
    if getattr(G, "_mapping_key", None) != key:
        with torch.no_grad():
            w = torch.stack([m.weight * m.scale for m in layers]).contiguous()
            b = torch.stack([m.bias * m.lr_mul for m in layers]).contiguous()
        G._mapping_stacks, G._mapping_key = (w, b), key
    return G._mapping_stacks


def _mapping_frozen(G):
    return not any(p.requires_grad for m in list(G.style)[1:] for p in (m.weight, m.bias))


def _layer_range(G, skip, depth):
    """style_forward(x, skip, depth) as (pixel_norm, first linear, number of linears): entry 0 of G.style is PixelNorm."""
    n = len(G.style)
    lo, hi = max(skip, 0), min(depth, n)
    first = max(lo, 1)
    return lo == 0 and hi > 0, first - 1, max(hi - first, 0)


def map_latents(G, z, skip=0, depth=100, center=None, truncation=1.0):
    """No-grad style_forward(z, skip, depth), then center + truncation * (w - center) when `center` is given.  One
    g2s_mapping_fwd for a CUDA float32 z of at least KERNEL_MIN_ROWS rows and frozen mapping weights; torch ops
    otherwise (CPU tensors always)."""
    with torch.no_grad():
        pixel_norm, first, count = _layer_range(G, skip, depth)
        if center is not None:
            center = center.reshape(-1)
        D = z.shape[-1]
        fits = D % 32 == 0 and 32 <= D <= 512 and 1 <= count <= 16
        if (z.is_cuda and z.dtype == torch.float32 and z.dim() == 2 and z.shape[0] >= KERNEL_MIN_ROWS and fits
                and _mapping_frozen(G)):
            w, b = mapping_weights(G)
            c = None if center is None else center.float().contiguous()
            return mapping_fwd(z.contiguous(), w[first:first + count], b[first:first + count], pixel_norm,
                               center=c, truncation=truncation)
        out = G.style_forward(z, skip=skip, depth=depth)
        if center is not None:
            out = center + truncation * (out - center)
        return out


def mean_latent(G, n, generator=None):
    """[1, D]: the mean of n mapped normal draws (Generator.mean_latent).  On the device one g2s_mapping_fwd that also
    writes its tiles' column sums, and g2s_rows_mean over them."""
    device = G.input.input.device
    with torch.no_grad():
        z = torch.randn(n, G.style_dim, device=device, generator=generator)
        if not z.is_cuda:
            return G.style_forward(z).mean(0, keepdim=True)
        if not _mapping_frozen(G):
            raise RuntimeError("mean_latent: the mapping network's weights require a gradient; freeze the generator")
        w, b = mapping_weights(G)
        T = mapping_tile()
        partial = torch.empty((n + T - 1) // T, G.style_dim, dtype=torch.float32, device=device)
        mapping_fwd(z, w, b, True, out=z, partial=partial)        # a tile reads its rows of z before it writes them
        return rows_mean(partial, n)[None]


# ---------------------------------------------------------------------------------------------------------- sample
def noise_sides(G):
    """Side of each styled layer's noise map, in layer order (Generator.make_noise)."""
    return [4] + [2 ** (3 + j // 2) for j in range(G.num_layers - 1)]


def draw(G, n, generator=None):
    """(z [n, D], [n, 1, r, r] per styled layer): the normal draws of n samples, in the order `sample` makes them."""
    device = G.input.input.device
    z = torch.randn(n, G.style_dim, device=device, generator=generator)
    return z, [torch.randn(n, 1, r, r, device=device, generator=generator) for r in noise_sides(G)]


def sample(G, n, truncation=1.0, mean_latent=None, generator=None, draws=None, batched=False):
    """(images [n, 3, S, S], w [n, D]) with w the truncated latent.  `draws`: the (z, noise maps) to use instead of
    fresh ones from `draw`.  Each sample is one Generator.forward with its own [1, 1, r, r] noise views (the one-node
    path on a frozen generator on the device); batched: ONE Generator.forward for all n on the [n, 1, r, r] draws (the
    one-node path with one map per sample on the device, the layer loop on CPU tensors).  The draws are the same."""
    with torch.no_grad():
        z, noise = draw(G, n, generator) if draws is None else draws
        center = mean_latent if truncation < 1 else None
        if truncation < 1 and center is None:
            raise ValueError("sample: truncation < 1 needs the mean latent")
        w = map_latents(G, z, center=center, truncation=truncation)
        if batched:
            from . import synthesis
            with synthesis.per_sample_noise():
                return G([w], input_is_w=True, noise=list(noise))[0], w
        images = [G([w[i:i + 1]], input_is_w=True, noise=[m[i:i + 1] for m in noise])[0] for i in range(n)]
        return torch.cat(images), w


# --------------------------------------------------------------------------------------------------------- command
def write_samples(G, out_dir, pics, per_batch=1, truncation=0.7, truncation_mean=4096, generator=None, log=None,
                  batched=False):
    """What the command does after G is built: pics * per_batch samples into `out_dir` in ImageLatentDataset's
    layout; batched: each chunk of per_batch samples is one forward (`sample`).  Returns the image names."""
    from PIL import Image
    os.makedirs(os.path.join(out_dir, "latents"), exist_ok=True)
    center = mean_latent(G, truncation_mean, generator) if truncation < 1 else None
    names = []
    for _ in range(pics):
        images, w = sample(G, per_batch, truncation, center, generator, batched=batched)
        pixels = image_to_u8(images).cpu().numpy()
        w = w.cpu()
        for j in range(per_batch):
            stem = "%06d" % len(names)
            Image.fromarray(pixels[j]).save(os.path.join(out_dir, stem + ".png"))
            torch.save(w[j].clone(), os.path.join(out_dir, "latents", stem + ".pt"))
            names.append(stem + ".png")
        if log is not None:
            log(f"{len(names)} of {pics * per_batch}")
    with open(os.path.join(out_dir, "list.txt"), "w") as f:
        f.write("".join(name + "\n" for name in names))
    return names


def build_parser():
    parser = argparse.ArgumentParser(prog="python -m gan2shape_amd.generate",
                                     description="Sample images and their latents from a StyleGAN2 generator")
    parser.add_argument("--ckpt", required=True, help="checkpoint with the generator under 'g_ema'")
    parser.add_argument("--size", type=int, required=True, help="image side of the generator")
    parser.add_argument("--channel-multiplier", dest="channel_multiplier", type=int, default=2)
    parser.add_argument("--out", required=True, help="<root>/<category>: the dataset directory to write")
    parser.add_argument("--pics", type=int, default=20, help="number of batches")
    parser.add_argument("--sample", type=int, default=1, help="samples per batch")
    parser.add_argument("--batched", action="store_true",
                        help="one generator forward per batch of --sample images instead of one per image")
    parser.add_argument("--truncation", type=float, default=0.7)
    parser.add_argument("--truncation-mean", dest="truncation_mean", type=int, default=4096,
                        help="draws behind the mean latent (not computed with --truncation 1)")
    parser.add_argument("--seed", type=int, default=0)
    parser.add_argument("--device", default="cuda")
    return parser


def main(argv=None, G=None):
    """`G`: a generator to use instead of the one --ckpt describes.  Returns the list of image names."""
    args = build_parser().parse_args(argv)
    device = torch.device(args.device)
    if G is None:
        from .stylegan2 import Generator
        G = Generator(args.size, 512, 8, channel_multiplier=args.channel_multiplier)
        state = torch.load(args.ckpt, map_location="cpu", weights_only=True)
        G.load_state_dict(state["g_ema"], strict=False)
    G = G.to(device).eval().requires_grad_(False)
    generator = torch.Generator(device=device).manual_seed(args.seed)
    return write_samples(G, args.out, args.pics, args.sample, args.truncation, args.truncation_mean, generator,
                         log=print, batched=args.batched)


if __name__ == "__main__":
    main()
