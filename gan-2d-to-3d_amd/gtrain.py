"""The generator half of stylegan2-pytorch/train.py: non-saturating loss every step, lazy path-length regularisation
every `g_reg_every`-th, and the exponential moving average `g_ema` (train.py:222-268).

`g_nonsaturating_loss`, `g_path_regularize`, `accumulate`, `make_noise`, `mixing_noise`: train.py:50-55 and 81-117,
values and signatures.  On CUDA float32 tensors the two losses are one autograd node each on csrc/gtrain.hip
(g2s_g_nonsaturating: loss and gradient in one launch; g2s_path_penalty: lengths, the new running mean, the penalty and
its gradient in one launch, the running mean read from the device) and `accumulate` is one launch over a device table
of all parameters (g2s_ema_accumulate; the reference: two launches per parameter).  CPU tensors and other dtypes take
the reference's torch composition.

`g_path_regularize` differentiates the generator twice: `GeneratorTrainer.step` runs it under `conv2d_gradfix.use()`,
where the modulated convolutions are nodes whose gradients can be differentiated again (op/conv2d_gradfix.py).  The
noise product (fake_img * noise).sum() needs no kernel: its gradient is `noise`."""
import math
import random

import numpy as np
import torch
import torch.nn.functional as F
from torch import autograd
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import augment as _aug
from . import lib as _lib
from .dtrain import _native, _pred, requires_grad
from .op import conv2d_gradfix


# ------------------------------------------------------------------------------------------------------ losses
class _GNonSaturating(Function):
    @staticmethod
    def forward(ctx, fake_pred):
        fake = fake_pred.contiguous()
        out = torch.empty((), dtype=torch.float32, device=fake.device)
        g_fake = torch.empty_like(fake)
        _lib.check(_lib.load().g2s_g_nonsaturating(_lib.ptr(fake), _lib.ptr(out), _lib.ptr(g_fake), fake.numel(),
                                                   _lib.stream()))
        ctx.save_for_backward(g_fake)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, gl):
        g_fake, = ctx.saved_tensors
        return g_fake * gl


def g_nonsaturating_loss(fake_pred):
    if _native(fake_pred):
        return _GNonSaturating.apply(fake_pred)
    return F.softplus(-fake_pred).mean()


class _PathPenalty(Function):
    """grad [B, L, D], the running mean (device scalar) -> (penalty, stats [3] = penalty, new mean, mean length,
    lengths [B]); gradient to grad through the penalty: the stored d penalty / d grad, scaled."""

    @staticmethod
    def forward(ctx, grad, mean_path, decay):
        g = grad.contiguous()
        B, L, D = g.shape
        lengths = torch.empty(B, dtype=torch.float32, device=g.device)
        stats = torch.empty(3, dtype=torch.float32, device=g.device)
        dgrad = torch.empty_like(g)
        _lib.check(_lib.load().g2s_path_penalty(_lib.ptr(g), _lib.ptr(mean_path), float(decay), _lib.ptr(lengths),
                                                _lib.ptr(stats), _lib.ptr(dgrad), B, L, D, _lib.stream()))
        ctx.save_for_backward(dgrad)
        ctx.mark_non_differentiable(stats, lengths)
        return stats[0].clone(), stats, lengths

    @staticmethod
    @once_differentiable
    def backward(ctx, gp, _s, _l):
        dgrad, = ctx.saved_tensors
        return dgrad * gp, None, None


def path_penalty(grad, mean_path_length, decay=0.01):
    """(penalty, new running mean (detached), lengths [B]) of a latent gradient [B, L, D]: train.py:94-100."""
    if _native(grad) and grad.dim() == 3:
        mean = torch.as_tensor(mean_path_length, dtype=torch.float32).to(grad.device).reshape(1)
        penalty, stats, lengths = _PathPenalty.apply(grad, mean, decay)
        return penalty, stats[1], lengths
    path_lengths = torch.sqrt(grad.pow(2).sum(2).mean(1))
    path_mean = mean_path_length + decay * (path_lengths.mean() - mean_path_length)
    path_penalty = (path_lengths - path_mean).pow(2).mean()
    return path_penalty, path_mean.detach(), path_lengths


def g_path_regularize(fake_img, latents, mean_path_length, decay=0.01, noise=None):
    """train.py:87-100.  `noise` (own addition): the image-shaped normal draw, for tests; None draws it."""
    if noise is None:
        noise = torch.randn_like(fake_img)
    noise = noise / math.sqrt(fake_img.shape[2] * fake_img.shape[3])
    with conv2d_gradfix.no_weight_gradients():   # asks for the latent gradient only: no discarded weight gradients
        grad, = autograd.grad(outputs=(fake_img * noise).sum(), inputs=latents, create_graph=True)
    return path_penalty(grad, mean_path_length, decay)


# --------------------------------------------------------------------------------------------------------- EMA
# (dst pointers, src pointers, sizes) -> (device table, device chunk prefix, n_chunks).  A table holds addresses and
# sizes only, so it stays right for whatever tensors have that key, and the cache keeps no parameter alive.
_EMA_TABLES = {}


def _ema_table(dst, src):
    key = (tuple(p.data_ptr() for p in dst), tuple(p.data_ptr() for p in src), tuple(p.numel() for p in dst))
    ent = _EMA_TABLES.get(key)
    if ent is None:
        if len(_EMA_TABLES) > 8:
            _EMA_TABLES.clear()
        chunk = int(_lib.load().g2s_ema_chunk())
        rows = [(d.data_ptr(), s.data_ptr(), d.numel()) for d, s in zip(dst, src)]
        prefix = np.zeros(len(rows) + 1, dtype=np.int32)
        prefix[1:] = np.cumsum([(r[2] + chunk - 1) // chunk for r in rows])
        dev = dst[0].device
        ent = _EMA_TABLES[key] = (torch.from_numpy(np.asarray(rows, dtype=np.int64)).to(dev),
                                  torch.from_numpy(prefix).to(dev), int(prefix[-1]))
    return ent


@torch.no_grad()
def ema_accumulate(dst, src, decay):
    """dst[j] = dst[j] * decay + src[j] * (1 - decay) for lists of CUDA float32 contiguous tensors: one launch."""
    dst, src = [t for t in dst if t.numel()], [t for t in src if t.numel()]
    for d, s in zip(dst, src):
        _lib.require_cuda(d, s)
        if not (d.dtype == s.dtype == torch.float32 and d.is_contiguous() and s.is_contiguous()
                and d.numel() == s.numel()):
            raise RuntimeError("ema_accumulate: contiguous float32 tensors of equal size only")
    if not dst:
        return
    table, prefix, n_chunks = _ema_table(dst, src)
    _lib.check(_lib.load().g2s_ema_accumulate(_lib.ptr(table), _lib.ptr(prefix), len(dst), n_chunks, float(decay),
                                              float(1 - decay), _lib.stream()))


def accumulate(model1, model2, decay=0.999):
    par1 = dict(model1.named_parameters())
    par2 = dict(model2.named_parameters())
    names = list(par1.keys())
    tensors = [par1[k].data for k in names] + [par2[k].data for k in names]
    if tensors and all(_native(t) and t.is_contiguous() for t in tensors):
        return ema_accumulate(tensors[:len(names)], tensors[len(names):], decay)
    for k in names:
        par1[k].data.mul_(decay).add_(par2[k].data, alpha=1 - decay)


# ------------------------------------------------------------------------------------------------------- noise
def make_noise(batch, latent_dim, n_noise, device):
    if n_noise == 1:
        return torch.randn(batch, latent_dim, device=device)
    return torch.randn(n_noise, batch, latent_dim, device=device).unbind(0)


def mixing_noise(batch, latent_dim, prob, device):
    if prob > 0 and random.random() < prob:
        return make_noise(batch, latent_dim, 2, device)
    return [make_noise(batch, latent_dim, 1, device)]


# ----------------------------------------------------------------------------------------------------- trainer
class GeneratorTrainer:
    """train.py:222-268: `step(i)`, the generator iteration against a discriminator that is held fixed."""

    EMA_DECAY = 0.5 ** (32 / (10 * 1000))

    def __init__(self, generator, g_ema, discriminator, batch=16, lr=0.002, path_regularize=2, g_reg_every=4,
                 path_batch_shrink=2, mixing=0.9, augment=False):
        self.g, self.g_ema, self.d = generator, g_ema, discriminator
        self.batch, self.mixing, self.augment = batch, mixing, augment
        self.path_regularize, self.g_reg_every, self.path_batch_shrink = path_regularize, g_reg_every, path_batch_shrink
        c = g_reg_every / (g_reg_every + 1)          # lazy regularisation: train.py:460-471
        params = list(generator.parameters())
        self.native = bool(params) and all(_native(p) for p in params)
        if self.native:
            from .optim import Adam
        else:
            from torch.optim import Adam
        self.g_optim = Adam(params, lr=lr * c, betas=(0 ** c, 0.99 ** c))
        self.device = params[0].device if params else torch.device("cpu")
        self.ada_aug_p = 0.0                          # the discriminator trainer's current probability, set by the loop
        self.mean_path_length = torch.zeros((), device=self.device)
        self.path_loss = torch.zeros((), device=self.device)
        self.path_lengths = torch.zeros((), device=self.device)

    def regularizes(self, i):
        return i % self.g_reg_every == 0

    def step(self, i, noise=None, maps=None, path_noise=None, path_maps=None, image_noise=None):
        """One generator iteration; returns {g, path, path_length} (device scalars).  For tests, what the reference
        draws can be passed: `noise` / `path_noise`, the latent lists of the two passes (default: mixing_noise);
        `maps` / `path_maps`, their noise maps (default: the generator's buffers); `image_noise`, the path pass's
        image-shaped draw."""
        requires_grad(self.g, True)
        requires_grad(self.d, False)
        latent_dim = self.g.style_dim
        with conv2d_gradfix.use(self.native):
            if noise is None:
                noise = mixing_noise(self.batch, latent_dim, self.mixing, self.device)
            fake_img, _ = self.g(noise, noise=maps)
            if self.augment:
                # order=2: the same four kernels while deterministic mode is off, the fixed-order adjoint while on
                fake_img, _ = _aug.augment(fake_img, self.ada_aug_p, order=2)
            fake_pred = _pred(self.d(fake_img))
            g_loss = g_nonsaturating_loss(fake_pred)
            loss = {"g": g_loss.detach()}
            self.g.zero_grad()
            g_loss.backward()
            self.g_optim.step()

            if self.regularizes(i):
                if path_noise is None:
                    path_batch_size = max(1, self.batch // self.path_batch_shrink)
                    path_noise = mixing_noise(path_batch_size, latent_dim, self.mixing, self.device)
                fake_img, latents = self.g(path_noise, return_latents=True, noise=path_maps)
                path_loss, self.mean_path_length, path_lengths = g_path_regularize(
                    fake_img, latents, self.mean_path_length, noise=image_noise)
                self.g.zero_grad()
                weighted_path_loss = self.path_regularize * self.g_reg_every * path_loss
                if self.path_batch_shrink:
                    weighted_path_loss = weighted_path_loss + 0 * fake_img[0, 0, 0, 0]
                weighted_path_loss.backward()
                self.g_optim.step()
                self.path_loss, self.path_lengths = path_loss.detach(), path_lengths.detach().mean()
        loss["path"], loss["path_length"] = self.path_loss, self.path_lengths
        accumulate(self.g_ema, self.g, self.EMA_DECAY)
        return loss

    def state_dict(self):
        return {"g": self.g.state_dict(), "g_ema": self.g_ema.state_dict(), "g_optim": self.g_optim.state_dict()}

    def load_state_dict(self, state, strict=True):
        self.g.load_state_dict(state["g"], strict=strict)
        self.g_ema.load_state_dict(state["g_ema"], strict=strict)
        if "g_optim" in state:
            self.g_optim.load_state_dict(state["g_optim"])
            if hasattr(self.g_optim, "_tables"):
                self.g_optim._tables.clear()     # the device table points at the moments it replaced
