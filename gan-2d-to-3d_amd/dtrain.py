"""The discriminator half of stylegan2-pytorch/train.py: logistic loss every step, lazy R1 every `d_reg_every`-th,
ADA on both — enough to adapt the discriminator whose features drive GAN2Shape's step-3 loss to a few thousand images
of one's own.  The generator half (modulated weight gradients, path-length regularisation, g_ema) is gtrain.py.

    python -m gan2shape_amd.dtrain --ckpt G_D.pt --size 128 --channel-multiplier 1 --data root/car --iter 2000 \
        --batch 16 [--augment] [--augment-p 0] [--r1 10] [--d-reg-every 16] [--seed 0] --out ckpts/d_ft.pt

`d_logistic_loss`, `d_r1_loss`, `requires_grad`: train.py:45-78, values and signatures.  On CUDA float32 tensors the
two losses are one autograd node each on csrc/dtrain.hip (g2s_d_logistic: loss, both scores, the sign statistic ADA
accumulates and both gradients in one launch; g2s_r1_penalty: the per-sample sums of squares in two stages); on CPU
tensors or other dtypes the reference's torch composition.  The backward of the R1 penalty, 2 g[b] grad / B, is a
torch.mul: one elementwise launch over B x n that a kernel of ours would not make cheaper.

`DiscriminatorTrainer.step` runs the discriminator under `conv2d_gradfix.use()`: trainable, twice-differentiable
convolutions and the one-launch minibatch stddev.  The R1 pass with augmentation — one step in `d_reg_every` —
differentiates the augmentation twice: it takes `augment(..., order=2)`, whose node and gradient node are each other's
gradients on the kernels of csrc/ada.hip.  CPU tensors take `augment._augment_twice`, a torch composition with the
bilinear sample written as gathers (torch's grid_sampler backward has no derivative).  `--deterministic` switches
libg2s to its fixed-order routes before the first step."""
import argparse
import math
import os

import torch
import torch.nn.functional as F
from torch import autograd
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import augment as _aug
from . import lib as _lib
from .op import conv2d_gradfix


def requires_grad(model, flag=True):
    for p in model.parameters():
        p.requires_grad = flag


def _native(*tensors):
    return all(t.is_cuda and t.dtype == torch.float32 for t in tensors)


# ------------------------------------------------------------------------------------------------- logistic loss
class _DLogistic(Function):
    """(loss, stats [4] = loss, mean real, mean fake, sum sign(real)); gradient to both predictions through loss."""

    @staticmethod
    def forward(ctx, real_pred, fake_pred):
        real, fake = real_pred.contiguous(), fake_pred.contiguous()
        stats = torch.empty(4, dtype=torch.float32, device=real.device)
        g_real, g_fake = torch.empty_like(real), torch.empty_like(fake)
        _lib.check(_lib.load().g2s_d_logistic(_lib.ptr(real), _lib.ptr(fake), _lib.ptr(stats), _lib.ptr(g_real),
                                              _lib.ptr(g_fake), real.numel(), fake.numel(), _lib.stream()))
        ctx.save_for_backward(g_real, g_fake)
        ctx.mark_non_differentiable(stats)
        return stats[0].clone(), stats

    @staticmethod
    @once_differentiable
    def backward(ctx, gl, _):
        g_real, g_fake = ctx.saved_tensors
        return g_real * gl, g_fake * gl


def d_logistic(real_pred, fake_pred):
    """(loss, stats): stats is None on the torch route, else the device vector [loss, mean real, mean fake,
    sum sign(real)] of the same launch."""
    if _native(real_pred, fake_pred):
        return _DLogistic.apply(real_pred, fake_pred)
    return F.softplus(-real_pred).mean() + F.softplus(fake_pred).mean(), None


def d_logistic_loss(real_pred, fake_pred):
    return d_logistic(real_pred, fake_pred)[0]


# ------------------------------------------------------------------------------------------------------ R1
class _R1Penalty(Function):
    """grad [B, ...] -> (mean over b of sum of squares, the per-sample sums [B])."""

    @staticmethod
    def forward(ctx, grad):
        B = grad.shape[0]
        g = grad.contiguous()
        n = g.numel() // B
        L = _lib.load()
        per = torch.empty(B, dtype=torch.float32, device=g.device)
        mean = torch.empty((), dtype=torch.float32, device=g.device)
        partial = torch.empty(B * int(L.g2s_r1_penalty_chunks(n)), dtype=torch.float32, device=g.device)
        _lib.check(L.g2s_r1_penalty(_lib.ptr(g), _lib.ptr(per), _lib.ptr(mean), _lib.ptr(partial), B, n, _lib.stream()))
        ctx.save_for_backward(grad)
        ctx.mark_non_differentiable(per)
        return mean, per

    @staticmethod
    def backward(ctx, gm, _):
        grad, = ctx.saved_tensors
        return grad * (gm * (2.0 / grad.shape[0]))


def r1_penalty(grad_real):
    """(grad_real.pow(2).reshape(B, -1).sum(1).mean(), the per-sample sums)."""
    if _native(grad_real):
        return _R1Penalty.apply(grad_real)
    per = grad_real.pow(2).reshape(grad_real.shape[0], -1).sum(1)
    return per.mean(), per.detach()


def d_r1_loss(real_pred, real_img):
    with conv2d_gradfix.no_weight_gradients():
        grad_real, = autograd.grad(outputs=real_pred.sum(), inputs=real_img, create_graph=True)
    return r1_penalty(grad_real)[0]


# ------------------------------------------------------------------------------------------------- the trainer
class _Ada(_aug.AdaptiveAugment):
    """AdaptiveAugment.tune fed with the sign statistic the loss launch already holds: no reduction of its own and a
    read-back only every `update_every` calls."""

    @torch.no_grad()
    def tune_stat(self, sign_sum, n):
        self.ada_aug_buf[0] += sign_sum
        self.ada_aug_buf[1] += n
        self.ada_update += 1
        if self.ada_update % self.update_every == 0:
            self.ada_aug_buf = _aug._reduce_sum(self.ada_aug_buf)
            signs, seen = self.ada_aug_buf.tolist()
            self.r_t_stat = signs / seen
            step = seen / self.ada_aug_len
            self.ada_aug_p += step if self.r_t_stat > self.ada_aug_target else -step
            self.ada_aug_p = min(1, max(0, self.ada_aug_p))
            self.ada_aug_buf.mul_(0)
            self.ada_update = 0
        return self.ada_aug_p


_bilinear_zeros = _aug._bilinear_zeros
_augment_twice = _aug._augment_twice          # the torch composition; it lives beside the nodes it restates


def augment_differentiable(img, p, transform_matrix=(None, None), composed=False):
    """augment.augment's result in a form that can be differentiated twice (the R1 pass), with the same draws, pads
    and matrices: `augment(..., order=2)` — on a CUDA float32 image the node pair of csrc/ada.hip, else the torch
    composition `_augment_twice`.  composed=True forces the composition on any tensor (measurements, cross-checks)."""
    if not composed:
        return _aug.augment(img, p, transform_matrix, order=2)
    G, C = transform_matrix
    if G is None:
        G = torch.inverse(_aug.sample_affine(p, img.shape[0], img.shape[2], img.shape[3]))
    if C is None:
        C = _aug.sample_color(p, img.shape[0])
    H, W = img.shape[2:]
    g_host = G.detach().float().cpu()
    pads = _aug._pads(g_host, H, W, _aug._TAPS)
    warp = _aug._warp_matrix(g_host, pads, H, W)
    cmat = C.detach().float().cpu()[:, :3, :].contiguous()
    return _augment_twice(img, warp, pads, cmat), (G, C)


def _pred(out):
    return out[0] if isinstance(out, (tuple, list)) else out


class DiscriminatorTrainer:
    """train.py:126-220 without the generator: `step(real_img, fake_img, i)`."""

    def __init__(self, discriminator, lr=0.002, r1=10, d_reg_every=16, augment=False, augment_p=0, ada_target=0.6,
                 ada_length=500_000):
        self.d = discriminator
        self.r1, self.d_reg_every = r1, d_reg_every
        self.augment, self.augment_p = augment, augment_p
        c = d_reg_every / (d_reg_every + 1)           # lazy regularisation: train.py:460-471
        params = list(discriminator.parameters())
        on_device = bool(params) and all(p.is_cuda and p.dtype == torch.float32 for p in params)
        if on_device:
            from .optim import Adam
        else:
            from torch.optim import Adam
        self.d_optim = Adam(params, lr=lr * c, betas=(0 ** c, 0.99 ** c))
        self.ada_aug_p = augment_p if augment_p > 0 else 0.0
        device = params[0].device if params else torch.device("cpu")
        self.ada = _Ada(ada_target, ada_length, 8, device) if augment and augment_p == 0 else None
        self.r1_loss = torch.zeros((), device=device)

    def regularizes(self, i):
        return i % self.d_reg_every == 0

    def step(self, real_img, fake_img, i):
        """One discriminator iteration; returns the loss dict {d, real_score, fake_score, r1} (device scalars)."""
        requires_grad(self.d, True)
        real_img, fake_img = real_img.detach(), fake_img.detach()
        with conv2d_gradfix.use(_native(real_img, fake_img)):
            if self.augment:
                real_aug, _ = _aug.augment(real_img, self.ada_aug_p)
                fake_img, _ = _aug.augment(fake_img, self.ada_aug_p)
            else:
                real_aug = real_img
            fake_pred = _pred(self.d(fake_img))
            real_pred = _pred(self.d(real_aug))
            d_loss, stats = d_logistic(real_pred, fake_pred)
            loss = {"d": d_loss.detach()}
            if stats is None:
                loss["real_score"], loss["fake_score"] = real_pred.detach().mean(), fake_pred.detach().mean()
            else:
                loss["real_score"], loss["fake_score"] = stats[1], stats[2]
            self.d.zero_grad()
            d_loss.backward()
            self.d_optim.step()

            if self.ada is not None:
                if stats is None:
                    self.ada_aug_p = self.ada.tune(real_pred)
                else:
                    self.ada_aug_p = self.ada.tune_stat(stats[3], real_pred.shape[0])

            if self.regularizes(i):
                real_img = real_img.detach().requires_grad_(True)
                if self.augment:
                    real_aug, _ = augment_differentiable(real_img, self.ada_aug_p)
                else:
                    real_aug = real_img
                real_pred = _pred(self.d(real_aug))
                r1_loss = d_r1_loss(real_pred, real_img)
                self.d.zero_grad()
                (self.r1 / 2 * r1_loss * self.d_reg_every + 0 * real_pred[0]).backward()
                self.d_optim.step()
                self.r1_loss = r1_loss.detach()
        loss["r1"] = self.r1_loss
        return loss

    def state_dict(self):
        return {"d": self.d.state_dict(), "d_optim": self.d_optim.state_dict(), "ada_aug_p": self.ada_aug_p}

    def load_state_dict(self, state):
        self.d.load_state_dict(state["d"])
        self.d_optim.load_state_dict(state["d_optim"])
        if hasattr(self.d_optim, "_tables"):
            self.d_optim._tables.clear()     # the device table points at the moments it replaced
        self.ada_aug_p = state["ada_aug_p"]
        if self.ada is not None:
            self.ada.ada_aug_p = self.ada_aug_p


# ----------------------------------------------------------------------------------------------------- command
def real_batches(root, size, batch, generator):
    """Endless batches [batch, 3, size, size] in [-1, 1] from the image list of an ImageLatentDataset-style folder,
    each image flipped horizontally with probability 1/2 (train.py:503-509); a shuffled pass per epoch."""
    from .dataset import ImageDataset, default_transform
    data = ImageDataset(root, transform=default_transform(size))
    if len(data) == 0:
        raise ValueError(f"{root}: the image list is empty")
    while True:
        order = torch.randperm(len(data), generator=generator).tolist()
        while len(order) < batch:
            order += torch.randperm(len(data), generator=generator).tolist()
        for lo in range(0, len(order) - batch + 1, batch):
            images = []
            for j in order[lo:lo + batch]:
                image = data[j][:, :size, :size]
                if image.shape[1:] != (size, size):
                    raise ValueError(f"{data.file_list[j]}: smaller than {size} x {size} after the resize")
                flip = torch.rand((), generator=generator).item() < 0.5
                images.append(image.flip(2) if flip else image)
            yield torch.stack(images)


def batches(root, size, batch, generator, device):
    """The real batches of a run: a folder packed by prepare_data.py (it holds `<size>.npy`) is served from device memory
    by dataset.DeviceBatches; any other folder goes through real_batches.  Same draws from `generator` either way.
    The batches may be on `device` already; `.to(device)` is then free."""
    from .dataset import DeviceBatches, is_packed
    if is_packed(root, size):
        return DeviceBatches(root, size, batch, generator, device)
    return real_batches(root, size, batch, generator)


def build_parser():
    parser = argparse.ArgumentParser(prog="python -m gan2shape_amd.dtrain",
                                     description="Fine-tune a StyleGAN2 discriminator: logistic loss, lazy R1, ADA")
    parser.add_argument("--ckpt", required=True, help="checkpoint with 'g_ema' and 'd' ('g' is copied through)")
    parser.add_argument("--size", type=int, required=True)
    parser.add_argument("--channel-multiplier", dest="channel_multiplier", type=int, default=2)
    parser.add_argument("--data", required=True,
                        help="dataset folder with list.txt, or one packed by prepare_data (it holds <size>.npy)")
    parser.add_argument("--iter", type=int, default=2000)
    parser.add_argument("--batch", type=int, default=16)
    parser.add_argument("--lr", type=float, default=0.002)
    parser.add_argument("--augment", action="store_true")
    parser.add_argument("--augment-p", dest="augment_p", type=float, default=0)
    parser.add_argument("--ada-target", dest="ada_target", type=float, default=0.6)
    parser.add_argument("--ada-length", dest="ada_length", type=int, default=500_000)
    parser.add_argument("--r1", type=float, default=10)
    parser.add_argument("--d-reg-every", dest="d_reg_every", type=int, default=16)
    parser.add_argument("--seed", type=int, default=0)
    parser.add_argument("--deterministic", action="store_true",
                        help="fixed-order kernels throughout (lib.set_deterministic): reproducible, slower")
    parser.add_argument("--log-every", dest="log_every", type=int, default=100)
    parser.add_argument("--device", default="cuda")
    parser.add_argument("--out", required=True)
    return parser


def main(argv=None):
    from . import generate
    from .stylegan2 import Discriminator, Generator
    args = build_parser().parse_args(argv)
    device = torch.device(args.device)
    torch.manual_seed(args.seed)
    if args.deterministic:
        _lib.set_deterministic(True)
    ckpt = torch.load(args.ckpt, map_location="cpu", weights_only=True)
    g_ema = Generator(args.size, 512, 8, channel_multiplier=args.channel_multiplier)
    g_ema.load_state_dict(ckpt["g_ema"], strict=False)
    g_ema = g_ema.to(device).eval().requires_grad_(False)
    d = Discriminator(args.size, channel_multiplier=args.channel_multiplier)
    d.load_state_dict(ckpt["d"])
    trainer = DiscriminatorTrainer(d.to(device).train(), args.lr, args.r1, args.d_reg_every, args.augment,
                                   args.augment_p, args.ada_target, args.ada_length)
    host_rng = torch.Generator().manual_seed(args.seed)
    dev_rng = torch.Generator(device=device).manual_seed(args.seed)
    reals = batches(args.data, args.size, args.batch, host_rng, device)
    for i in range(args.iter):
        real = next(reals).to(device)
        fake, _ = generate.sample(g_ema, args.batch, generator=dev_rng, batched=True)
        loss = trainer.step(real, fake, i)
        if args.log_every and (i % args.log_every == 0 or i == args.iter - 1):
            print(f"{i}: d {loss['d'].item():.4f} r1 {loss['r1'].item():.4f} real {loss['real_score'].item():.3f} "
                  f"fake {loss['fake_score'].item():.3f} augment {trainer.ada_aug_p:.4f}")
            if not all(math.isfinite(v.item()) for v in loss.values()):
                raise FloatingPointError(f"step {i}: a loss is not finite")
    state = trainer.state_dict()
    out = {"g": ckpt.get("g", ckpt["g_ema"]), "d": state["d"], "g_ema": ckpt["g_ema"], "d_optim": state["d_optim"],
           "ada_aug_p": state["ada_aug_p"]}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    torch.save(out, args.out)
    return args.out


if __name__ == "__main__":
    main()
