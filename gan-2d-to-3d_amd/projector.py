"""The StyleGAN2 latent projector (stylegan2-pytorch/projector.py): optimise one w — or one w per layer — and the
noise maps of a frozen generator against an image, with LPIPS + 1e5 * noise regulariser (+ optional MSE), Adam under
the reference's learning-rate ramp, latent jitter and noise re-normalisation after every step.  Its result is the
`latents/<stem>.pt` file that dataset.LatentDataset reads:

    python -m gan2shape_amd.projector --ckpt G.pt --size 128 --channel_multiplier 1 [--batch N] root/img0.png root/img1.png

What runs on the GPU: the generator as one autograd node with noise-map gradients (synthesis._Synthesis,
g2s_noise_grad), the LPIPS node (lpips._VggLpips), the regulariser of ALL maps in three launches each way
(g2s_noise_regularize: value and gradient together in forward), the re-normalisation of all maps in two
(g2s_noise_normalize) and the one-launch Adam (optim.Adam).  CPU tensors take plain torch ops (op/cpu_tensors.py's rule).

`project` takes one image.  `project_batch` (--batch N) is the reference's loop as the reference runs it on several
files: B images in one batch with [B, 1, s, s] noise maps, the generator as ONE node with one map per sample
(synthesis.per_sample_noise), one LPIPS, one regulariser, one Adam step and one re-normalisation per step.  As in the
reference the images of a batch are coupled: the regulariser's means and the re-normalisation's mean and standard
deviation run over all B maps of a layer, so a file's result depends on the files it shares a batch with."""
import argparse
import math
import os

import torch
import torch.nn.functional as F
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import lib as _lib


# ----------------------------------------------------------------------------------------------- noise functions
def _noise_regularize_torch(noises):
    """projector.py:16-36, operation by operation."""
    loss = 0
    for noise in noises:
        size = noise.shape[2]
        while True:
            loss = (loss + (noise * torch.roll(noise, shifts=1, dims=3)).mean().pow(2)
                    + (noise * torch.roll(noise, shifts=1, dims=2)).mean().pow(2))
            if size <= 8:
                break
            noise = noise.reshape([-1, 1, size // 2, 2, size // 2, 2]).mean([3, 5])
            size //= 2
    return loss


def _map_table(noises):
    """(pointer array, side array, maps, B) of a list of contiguous CUDA float32 [B, 1, S, S] maps for libg2s."""
    B = noises[0].shape[0]
    for n in noises:
        if n.dim() != 4 or n.shape[0] != B or n.shape[1] != 1 or n.shape[2] != n.shape[3]:
            raise ValueError(f"noise maps must be [B, 1, S, S] with one B; got {tuple(n.shape)}")
        if n.dtype != torch.float32 or not n.is_cuda or not n.is_contiguous():
            raise RuntimeError("the noise kernels take contiguous CUDA float32 maps")
    ptrs = (_lib.C.c_void_p * len(noises))(*[n.data_ptr() for n in noises])
    sides = (_lib.C.c_int * len(noises))(*[n.shape[2] for n in noises])
    return ptrs, sides, len(noises), B


def _workspace(nbytes, device):
    return torch.empty(max(1, (nbytes + 3) // 4), dtype=torch.float32, device=device)


class _NoiseRegularize(Function):
    """g2s_noise_regularize: the value and d value / d map of every map in forward (three launches); backward scales."""

    @staticmethod
    def forward(ctx, *noises):
        L = _lib.load()
        maps = [n.contiguous() for n in noises]
        ptrs, sides, count, B = _map_table(maps)
        dev = maps[0].device
        want = any(ctx.needs_input_grad)
        grads = [torch.empty_like(m) for m in maps] if want else None
        gptrs = (_lib.C.c_void_p * count)(*[g.data_ptr() for g in grads]) if want else None
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        nbytes = L.g2s_noise_regularize_workspace_bytes(sides, count, B)
        ws = _workspace(nbytes, dev)
        _lib.check(L.g2s_noise_regularize(ptrs, gptrs, sides, count, B, _lib.ptr(loss), _lib.ptr(ws), ws.numel() * 4,
                                          _lib.stream()))
        ctx.grads = grads
        return loss.view(())

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        grads, ctx.grads = ctx.grads, None
        scaled = torch._foreach_mul(grads, gout)        # one launch for all maps
        return tuple(g if need else None for g, need in zip(scaled, ctx.needs_input_grad))


def noise_regularize(noises):
    """projector.py:16-36: per map and pyramid level (2x2 means down to the first side <= 8) the squared means of
    n * roll(n, 1, x) and n * roll(n, 1, y), summed over levels and maps.  CUDA float32 maps: libg2s; CPU: torch."""
    noises = list(noises)
    if noises and noises[0].is_cuda:
        return _NoiseRegularize.apply(*noises)
    return _noise_regularize_torch(noises)


def noise_normalize_(noises):
    """projector.py:39-44: every map to zero mean and unit (unbiased) standard deviation, in place, without autograd.
    CUDA float32 maps: all of them in two launches (g2s_noise_normalize); CPU: torch."""
    noises = list(noises)
    if noises and noises[0].is_cuda:
        L = _lib.load()
        data = [n.data for n in noises]
        ptrs, sides, count, B = _map_table(data)
        ws = _workspace(L.g2s_noise_normalize_workspace_bytes(sides, count, B), data[0].device)
        _lib.check(L.g2s_noise_normalize(ptrs, sides, count, B, _lib.ptr(ws), ws.numel() * 4, _lib.stream()))
        return
    for noise in noises:
        mean = noise.mean()
        std = noise.std()
        noise.data.add_(-mean).div_(std)


def get_lr(t, initial_lr, rampdown=0.25, rampup=0.05):
    """projector.py:47-52: cosine ramp-down over the last `rampdown` of the run, linear warm-up over the first `rampup`."""
    lr_ramp = min(1, (1 - t) / rampdown)
    lr_ramp = 0.5 - 0.5 * math.cos(lr_ramp * math.pi)
    lr_ramp = lr_ramp * min(1, t / rampup)
    return initial_lr * lr_ramp


def latent_noise(latent, strength, generator=None):
    """projector.py:55-58: latent + strength * N(0, 1)."""
    noise = torch.randn(latent.shape, dtype=latent.dtype, device=latent.device, generator=generator) * strength
    return latent + noise


def make_image(tensor):
    """projector.py:61-72: [-1, 1] float (B, 3, H, W) -> uint8 numpy (B, H, W, 3)."""
    return (tensor.detach().clamp(min=-1, max=1).add(1).div_(2).mul(255).type(torch.uint8)
            .permute(0, 2, 3, 1).to("cpu").numpy())


# ----------------------------------------------------------------------------------------------- the projection
def mean_latent_stats(G, n=10000, generator=None):
    """(latent_mean [style_dim], latent_std scalar) of W from n mapped samples (projector.py:155-160):
    std = sqrt(sum (w - mean)^2 / n) — ONE scalar over all coordinates, the reference's formula."""
    device = G.input.input.device
    with torch.no_grad():
        z = torch.randn(n, G.style_dim, device=device, generator=generator)
        w = G.style_forward(z)
        mean = w.mean(0)
        std = ((w - mean).pow(2).sum() / n) ** 0.5
    return mean, std


def _generate(G, latent, noises):
    """G's image from w [1, 512] / [1, n_latent, 512], as the loss sees it: area mean down to 256 (projector.py:193-203)."""
    img, _ = G([latent], input_is_w=True, noise=noises)
    batch, channel, height, width = img.shape
    if height > 256:
        factor = height // 256
        img = img.reshape(batch, channel, height // factor, factor, width // factor, factor).mean([3, 5])
    return img


def evaluate(G, percept, image, latent, noises):
    """The perceptual term of the projector's loss for (latent, noises) without jitter (a 0-dim tensor)."""
    with torch.no_grad():
        if latent.dim() == 1 or (latent.dim() == 2 and latent.shape[0] == G.n_latent):
            latent = latent.unsqueeze(0)             # (512,) or (n_latent, 512), as project returns and the dataset stores
        return percept(_generate(G, latent, noises), image).sum()


def _adam(params, lr):
    if params[0].is_cuda:
        from .optim import Adam
        return Adam(params, lr=lr)
    return torch.optim.Adam(params, lr=lr)


def project(G, percept, image, steps=1000, lr=0.1, noise=0.05, noise_ramp=0.75, noise_regularize=1e5, mse=0.0,
            w_plus=False, lr_rampup=0.05, lr_rampdown=0.25, latent_stats=None, generator=None):
    """The loop of projector.py:166-227 for ONE image (1, 3, H, W) in [-1, 1] (H = min(G.size, 256)): the latent starts
    at the mean w, the noise maps at fresh N(0, 1); every step sets Adam's lr from get_lr, jitters the latent by
    latent_std * noise * max(0, 1 - t / noise_ramp)^2, and minimises percept + noise_regularize * regulariser (+ mse *
    MSE, computed only when mse != 0), then re-normalises the maps.  G must be frozen (eval, requires_grad_(False)).

    latent_stats: (mean, std) of mean_latent_stats, computed when None; generator: a torch.Generator on G's device
    for the maps, the jitter and the statistics (None: the global one).
    Returns {'img': the final image (1, 3, S, S) of the un-jittered latent, 'latent': (512,) or (n_latent, 512),
    'noise': the maps [(1, 1, s, s)], 'history': the latent after every 100th step} — detached.  (The reference renders
    its image from the last history entry, so it needs steps >= 100; this is the same latent whenever steps % 100 == 0.)"""
    if image.dim() != 4 or image.shape[0] != 1:
        raise ValueError("project takes one image (1, 3, H, W); loop over a batch")
    reg_weight, reg = noise_regularize, globals()["noise_regularize"]
    device = G.input.input.device
    image = image.to(device)
    if latent_stats is None:
        latent_stats = mean_latent_stats(G, generator=generator)
    latent_mean, latent_std = latent_stats
    latent_std = float(latent_std)
    noises = [n.normal_(generator=generator).requires_grad_(True) for n in G.make_noise()]
    latent_in = latent_mean.detach().clone().unsqueeze(0)
    if w_plus:
        latent_in = latent_in.unsqueeze(1).repeat(1, G.n_latent, 1)
    latent_in = latent_in.contiguous().requires_grad_(True)
    optimizer = _adam([latent_in] + noises, lr)
    history = []
    for i in range(steps):
        t = i / steps
        optimizer.param_groups[0]["lr"] = get_lr(t, lr, lr_rampdown, lr_rampup)
        strength = latent_std * noise * max(0, 1 - t / noise_ramp) ** 2
        latent_n = latent_noise(latent_in, strength, generator)
        img_gen = _generate(G, latent_n, noises)
        loss = percept(img_gen, image).sum() + reg_weight * reg(noises)
        if mse != 0:
            loss = loss + mse * F.mse_loss(img_gen, image)
        optimizer.zero_grad()
        loss.backward()
        optimizer.step()
        noise_normalize_(noises)
        if (i + 1) % 100 == 0:
            history.append(latent_in.detach().clone())
    with torch.no_grad():
        img, _ = G([latent_in], input_is_w=True, noise=noises)
    return {'img': img.detach(), 'latent': latent_in.detach()[0].clone(), 'noise': [n.detach().clone() for n in noises],
            'history': history}


def project_batch(G, percept, images, steps=1000, lr=0.1, noise=0.05, noise_ramp=0.75, noise_regularize=1e5, mse=0.0,
                  w_plus=False, lr_rampup=0.05, lr_rampdown=0.25, latent_stats=None, generator=None):
    """The loop of projector.py:166-227 for B images (B, 3, H, W) at once, as the reference runs it when it is given
    several files: latent_in is [B, D] ([B, n_latent, D] with w_plus), the maps are [B, 1, s, s] normal draws, the
    jitter is drawn per sample, the loss is percept(...).sum() over the batch + noise_regularize * regulariser (+ mse *
    the mean squared error over the batch), one Adam over all of it, then noise_normalize_.  The regulariser's means and
    the normalisation's statistics run OVER THE BATCH (the reference's behaviour): the B projections are coupled through
    them, and a batch of B is not B runs of `project`.  On CUDA tensors the generator is the one-node path with one map
    per sample (synthesis.per_sample_noise); CPU tensors take the layer loop.  With the same `generator` seed B = 1 draws
    what `project` draws, in its order and shapes, and gives its result bit for bit in deterministic mode.

    Returns what `project` returns with a leading B: {'img': (B, 3, S, S), 'latent': (B, D) or (B, n_latent, D),
    'noise': [(B, 1, s, s)], 'history': [latent_in after every 100th step]} — detached.  `split_projection` gives the
    per-image dictionaries that `save_projection` writes."""
    from . import synthesis
    if images.dim() != 4 or images.shape[0] < 1:
        raise ValueError("project_batch takes images (B, 3, H, W)")
    reg_weight, reg = noise_regularize, globals()["noise_regularize"]
    device = G.input.input.device
    images = images.to(device)
    B = images.shape[0]
    if latent_stats is None:
        latent_stats = mean_latent_stats(G, generator=generator)
    latent_mean, latent_std = latent_stats
    latent_std = float(latent_std)
    noises = [(n if B == 1 else n.new_empty((B,) + tuple(n.shape[1:]))).normal_(generator=generator).requires_grad_(True)
              for n in G.make_noise()]
    latent_in = latent_mean.detach().clone().unsqueeze(0).repeat(B, 1)
    if w_plus:
        latent_in = latent_in.unsqueeze(1).repeat(1, G.n_latent, 1)
    latent_in = latent_in.contiguous().requires_grad_(True)
    optimizer = _adam([latent_in] + noises, lr)
    history = []
    for i in range(steps):
        t = i / steps
        optimizer.param_groups[0]["lr"] = get_lr(t, lr, lr_rampdown, lr_rampup)
        strength = latent_std * noise * max(0, 1 - t / noise_ramp) ** 2
        latent_n = latent_noise(latent_in, strength, generator)
        with synthesis.per_sample_noise():
            img_gen = _generate(G, latent_n, noises)
        loss = percept(img_gen, images).sum() + reg_weight * reg(noises)
        if mse != 0:
            loss = loss + mse * F.mse_loss(img_gen, images)
        optimizer.zero_grad()
        loss.backward()
        optimizer.step()
        noise_normalize_(noises)
        if (i + 1) % 100 == 0:
            history.append(latent_in.detach().clone())
    with torch.no_grad(), synthesis.per_sample_noise():
        img, _ = G([latent_in], input_is_w=True, noise=noises)
    return {'img': img.detach(), 'latent': latent_in.detach().clone(), 'noise': [n.detach().clone() for n in noises],
            'history': history}


def split_projection(result):
    """project_batch's result -> one dictionary per image in `project`'s layout: 'img' (1, 3, S, S), 'latent' (D,) or
    (n_latent, D), 'noise' [(1, 1, s, s)], 'history' [(1, ...)]."""
    return [{'img': result['img'][j:j + 1], 'latent': result['latent'][j].clone(),
             'noise': [n[j:j + 1].clone() for n in result['noise']], 'history': [h[j:j + 1] for h in result['history']]}
            for j in range(result['img'].shape[0])]


def save_projection(root, filename, result):
    """Write `root/latents/<stem>.pt` = {filename: {'img', 'latent', 'noise'}} of detached CPU tensors, <stem> =
    filename up to its first dot — the name dataset.LatentDataset reads (and loads with weights_only=True).  The
    reference's script names its file `<basename with extension>.pt` (projector.py:229-231), which its own dataset
    class (GAN2Shape/dataset.py:50-58) does not find; the dataset's naming is used here.  Returns the path."""
    folder = os.path.join(root, "latents")
    os.makedirs(folder, exist_ok=True)
    img = result['img'].detach().cpu()
    entry = {'img': img[0] if img.dim() == 4 else img, 'latent': result['latent'].detach().cpu(),
             'noise': [n.detach().cpu() for n in result['noise']]}
    path = os.path.join(folder, os.path.basename(filename).split('.')[0] + '.pt')
    torch.save({filename: entry}, path)
    return path


def load_image(path, size):
    """An image file -> (1, 3, size, size) in [-1, 1]: dataset.default_transform (smaller edge to `size`) + centre crop."""
    from PIL import Image
    from .dataset import default_transform
    with Image.open(path) as im:
        x = default_transform(size)(im.convert("RGB"))
    top, left = (x.shape[1] - size) // 2, (x.shape[2] - size) // 2
    return (x[:, top:top + size, left:left + size] * 2 - 1).unsqueeze(0)


def main(argv=None):
    parser = argparse.ArgumentParser(description="Image projector to the generator latent spaces")
    parser.add_argument("--ckpt", type=str, required=True, help="path to the model checkpoint ('g_ema' state dict)")
    parser.add_argument("--size", type=int, default=256, help="output image size of the generator")
    parser.add_argument("--channel_multiplier", type=int, default=2)
    parser.add_argument("--lr_rampup", type=float, default=0.05, help="duration of the learning rate warmup")
    parser.add_argument("--lr_rampdown", type=float, default=0.25, help="duration of the learning rate decay")
    parser.add_argument("--lr", type=float, default=0.1, help="learning rate")
    parser.add_argument("--noise", type=float, default=0.05, help="strength of the noise level")
    parser.add_argument("--noise_ramp", type=float, default=0.75, help="duration of the noise level decay")
    parser.add_argument("--step", type=int, default=1000, help="optimize iterations")
    parser.add_argument("--noise_regularize", type=float, default=1e5, help="weight of the noise regularization")
    parser.add_argument("--mse", type=float, default=0, help="weight of the mse loss")
    parser.add_argument("--w_plus", action="store_true", help="allow to use distinct latent codes to each layers")
    parser.add_argument("--lpips_lin_weights", type=str, default=None, help="lpips/weights/v0.1/vgg.pth")
    parser.add_argument("--lpips_vgg_weights", type=str, default=None, help="torchvision vgg16 state dict")
    parser.add_argument("--device", type=str, default="cuda")
    parser.add_argument("--batch", type=int, default=1,
                        help="files projected together (the reference's batch: their noise statistics are shared); "
                             "1: one file at a time")
    parser.add_argument("files", metavar="FILES", nargs="+", help="path to image files to be projected")
    args = parser.parse_args(argv)

    from .lpips import PerceptualLoss
    from .stylegan2 import Generator
    device = torch.device(args.device)
    G = Generator(args.size, 512, 8, channel_multiplier=args.channel_multiplier)
    G.load_state_dict(torch.load(args.ckpt, map_location="cpu", weights_only=True)["g_ema"], strict=False)
    G = G.to(device).eval().requires_grad_(False)
    percept = PerceptualLoss(model='net-lin', net='vgg', lin_weights_path=args.lpips_lin_weights,
                             vgg_weights_path=args.lpips_vgg_weights).to(device)
    if args.batch < 1:
        parser.error("--batch must be at least 1")
    stats = mean_latent_stats(G)
    options = dict(steps=args.step, lr=args.lr, noise=args.noise, noise_ramp=args.noise_ramp,
                   noise_regularize=args.noise_regularize, mse=args.mse, w_plus=args.w_plus, lr_rampup=args.lr_rampup,
                   lr_rampdown=args.lr_rampdown, latent_stats=stats)
    paths = []
    # --batch 1: one `project` per file; N > 1: the files N at a time through project_batch (the last group may be shorter)
    for first in range(0, len(args.files), args.batch):
        group = args.files[first:first + args.batch]
        images = [load_image(path, min(args.size, 256)).to(device) for path in group]
        if args.batch == 1:
            results = [project(G, percept, images[0], **options)]
        else:
            results = split_projection(project_batch(G, percept, torch.cat(images), **options))
        for path, image, result in zip(group, images, results):
            paths.append(_write_result(G, percept, path, image, result))
    return paths


def _write_result(G, percept, path, image, result):
    """One file's outputs: latents/<stem>.pt, the preview image, the printed perceptual distance.  Returns the .pt path."""
    from PIL import Image
    p_loss = float(evaluate(G, percept, image, result['latent'], result['noise']))
    out = save_projection(os.path.dirname(path) or ".", os.path.basename(path), result)
    Image.fromarray(make_image(result['img'])[0]).save(os.path.splitext(os.path.basename(path))[0] + "-project.png")
    print(f"{path}: perceptual {p_loss:.4f} -> {out}")
    return out


if __name__ == "__main__":
    main()
