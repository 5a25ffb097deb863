"""stylegan2-pytorch/train.py on one device: per iteration `DiscriminatorTrainer.step` (dtrain.py), then
`GeneratorTrainer.step` (gtrain.py).

    python -m gan2shape_amd.train --size 128 --channel-multiplier 1 --data root/car --iter 2000 --batch 16 \
        [--ckpt G_D.pt] [--augment] [--mixing 0.9] [--path-regularize 2] [--g-reg-every 4] [--save-every 10000] \
        [--sample-every 100 [--n-sample 64] [--sample-dir DIR]] \
        [--ppl-every 1000 --lpips-lin vgg.pth --lpips-vgg vgg16.pth [--ppl-samples 512]] \
        [--deterministic] --out ckpts/train.pt

The checkpoint has train.py's keys: g, d, g_ema, g_optim, d_optim, ada_aug_p.  Without --ckpt the weights are fresh
(torch.manual_seed(--seed)) and g_ema starts as a copy of g (train.py:419-421).

Monitoring (monitor.py), off by default: every --sample-every-th iteration g_ema's images of a fixed `sample_z` go to
<sample dir>/%06d.png as one grid (train.py:303-316), every --ppl-every-th iteration the perceptual path length of
g_ema (w space, full sampling) goes on the log line and into <dir of --out>/ppl.jsonl.  sample_z and the path
length's draws come from generators of their own, seeded with --seed, and g_ema runs on its fixed noise buffers: the
global random stream, and with it the trained weights, are the same with monitoring on or off.

Not built: distributed training, wandb, fp16."""
import argparse
import contextlib
import json
import math
import os

import torch

from . import dtrain, gtrain

CHECKPOINT_KEYS = ("g", "d", "g_ema", "g_optim", "d_optim", "ada_aug_p")


def build_parser():
    parser = argparse.ArgumentParser(prog="python -m gan2shape_amd.train",
                                     description="Train a StyleGAN2 generator and discriminator on one device")
    parser.add_argument("--ckpt", default=None, help="checkpoint to resume from (keys g, d, g_ema[, g_optim, d_optim])")
    parser.add_argument("--size", type=int, required=True)
    parser.add_argument("--channel-multiplier", dest="channel_multiplier", type=int, default=2)
    parser.add_argument("--latent", type=int, default=512)
    parser.add_argument("--n-mlp", dest="n_mlp", type=int, default=8)
    parser.add_argument("--data", required=True,
                        help="dataset folder with list.txt, or one packed by prepare_data (it holds <size>.npy)")
    parser.add_argument("--iter", type=int, default=800000)
    parser.add_argument("--batch", type=int, default=16)
    parser.add_argument("--lr", type=float, default=0.002)
    parser.add_argument("--mixing", type=float, default=0.9)
    parser.add_argument("--r1", type=float, default=10)
    parser.add_argument("--d-reg-every", dest="d_reg_every", type=int, default=16)
    parser.add_argument("--path-regularize", dest="path_regularize", type=float, default=2)
    parser.add_argument("--path-batch-shrink", dest="path_batch_shrink", type=int, default=2)
    parser.add_argument("--g-reg-every", dest="g_reg_every", type=int, default=4)
    parser.add_argument("--augment", action="store_true")
    parser.add_argument("--augment-p", dest="augment_p", type=float, default=0)
    parser.add_argument("--ada-target", dest="ada_target", type=float, default=0.6)
    parser.add_argument("--ada-length", dest="ada_length", type=int, default=500_000)
    parser.add_argument("--seed", type=int, default=0)
    parser.add_argument("--deterministic", action="store_true",
                        help="fixed-order kernels throughout (lib.set_deterministic): reproducible, slower")
    parser.add_argument("--log-every", dest="log_every", type=int, default=100)
    parser.add_argument("--save-every", dest="save_every", type=int, default=10000,
                        help="also write --out every this many iterations (train.py: 10000); 0: only at the end")
    parser.add_argument("--sample-every", dest="sample_every", type=int, default=0,
                        help="write a grid of g_ema samples every this many iterations (train.py: 100); 0: never")
    parser.add_argument("--n-sample", dest="n_sample", type=int, default=64)
    parser.add_argument("--sample-dir", dest="sample_dir", default=None, help="default: <dir of --out>/sample")
    parser.add_argument("--ppl-every", dest="ppl_every", type=int, default=0,
                        help="measure g_ema's perceptual path length every this many iterations; 0: never")
    parser.add_argument("--ppl-samples", dest="ppl_samples", type=int, default=512)
    parser.add_argument("--lpips-lin", dest="lpips_lin", default=None, help="lpips/weights/v0.1/vgg.pth")
    parser.add_argument("--lpips-vgg", dest="lpips_vgg", default=None, help="a torchvision vgg16 state dict")
    parser.add_argument("--device", default="cuda")
    parser.add_argument("--out", required=True)
    return parser


def build_trainers(args, device):
    """(DiscriminatorTrainer, GeneratorTrainer) from fresh weights or from args.ckpt."""
    from .stylegan2 import Discriminator, Generator
    g = Generator(args.size, args.latent, args.n_mlp, channel_multiplier=args.channel_multiplier)
    g_ema = Generator(args.size, args.latent, args.n_mlp, channel_multiplier=args.channel_multiplier)
    d = Discriminator(args.size, channel_multiplier=args.channel_multiplier)
    g_ema.load_state_dict(g.state_dict())               # accumulate(g_ema, generator, 0)
    g, d = g.to(device).train(), d.to(device).train()
    g_ema = g_ema.to(device).eval()
    dt = dtrain.DiscriminatorTrainer(d, args.lr, args.r1, args.d_reg_every, args.augment, args.augment_p,
                                     args.ada_target, args.ada_length)
    gt = gtrain.GeneratorTrainer(g, g_ema, d, args.batch, args.lr, args.path_regularize, args.g_reg_every,
                                 args.path_batch_shrink, args.mixing, args.augment)
    if args.ckpt:      # through the trainers' own load_state_dict: they drop the optimisers' device tables
        ckpt = torch.load(args.ckpt, map_location="cpu", weights_only=True)
        state = {"g": ckpt.get("g", ckpt["g_ema"]), "g_ema": ckpt["g_ema"]}
        if "g_optim" in ckpt:
            state["g_optim"] = ckpt["g_optim"]
        gt.load_state_dict(state, strict=False)
        if "d_optim" in ckpt:
            dt.load_state_dict({"d": ckpt["d"], "d_optim": ckpt["d_optim"], "ada_aug_p": ckpt.get("ada_aug_p", 0.0)})
        else:
            d.load_state_dict(ckpt["d"])
    return dt, gt


def checkpoint(dt, gt):
    ds, gs = dt.state_dict(), gt.state_dict()
    return {"g": gs["g"], "d": ds["d"], "g_ema": gs["g_ema"], "g_optim": gs["g_optim"], "d_optim": ds["d_optim"],
            "ada_aug_p": ds["ada_aug_p"]}


def iteration(dt, gt, real_img, i):
    """train.py:169-268: the discriminator step on fresh fakes of the frozen generator, then the generator step."""
    dtrain.requires_grad(gt.g, False)
    dtrain.requires_grad(dt.d, True)
    with torch.no_grad():
        noise = gtrain.mixing_noise(real_img.shape[0], gt.g.style_dim, gt.mixing, real_img.device)
        fake_img, _ = gt.g(noise)
    loss = dt.step(real_img, fake_img, i)
    gt.ada_aug_p = dt.ada_aug_p
    loss.update(gt.step(i))
    dtrain.requires_grad(dt.d, True)
    return loss


@contextlib.contextmanager
def _frozen(module):
    """`module` as it is NOW, in eval mode with no parameter requiring a gradient (what the generator's one-node path
    asks for); both are put back on exit.

    A frozen forward keeps what it derives from the weights (the scaled weights of EqualLinear and ModulatedConv2d,
    their squared sums, the style and mapping stacks) and knows them stale by `(data_ptr, _version)`.  The moving
    average writes g_ema through `.data` (gtrain.accumulate), which moves neither, so every tensor's version is
    advanced here: a host-side counter, no launch, and nothing the training path reads."""
    torch.autograd.graph.increment_version(list(module.parameters()) + list(module.buffers()))
    flags = [(p, p.requires_grad) for p in module.parameters()]
    training = module.training
    module.eval().requires_grad_(False)
    try:
        yield module
    finally:
        for p, flag in flags:
            p.requires_grad_(flag)
        module.train(training)


class Monitor:
    """The sample grids and path lengths of a run.  Draws nothing from the global generators."""

    def __init__(self, args, g_ema, device, percept=None):
        self.args, self.g_ema, self.device = args, g_ema, device
        out_dir = os.path.dirname(os.path.abspath(args.out))
        self.sample_dir = args.sample_dir or os.path.join(out_dir, "sample")
        self.ppl_path = os.path.join(out_dir, "ppl.jsonl")
        self.sample_z, self.percept = None, percept
        if args.sample_every:
            if args.n_sample < 1:
                raise SystemExit("train: --n-sample must be positive")
            g = torch.Generator(device=device).manual_seed(args.seed)
            self.sample_z = torch.randn(args.n_sample, args.latent, device=device, generator=g)
            os.makedirs(self.sample_dir, exist_ok=True)
        if args.ppl_every and percept is None:
            from .lpips import PerceptualLoss
            self.percept = PerceptualLoss(lin_weights_path=args.lpips_lin, vgg_weights_path=args.lpips_vgg)
        if self.percept is not None:
            self.percept = self.percept.to(device).eval()

    @staticmethod
    def check_args(args, percept=None):
        if args.ppl_every and percept is None and not (args.lpips_lin and args.lpips_vgg):
            raise SystemExit("train: --ppl-every needs --lpips-lin and --lpips-vgg (a path length under random LPIPS "
                             "weights is not a PPL)")

    def samples(self):
        with torch.no_grad(), _frozen(self.g_ema) as g:
            return g([self.sample_z])[0]

    def after(self, i):
        """What iteration i leaves behind; returns the text to add to its log line."""
        from . import monitor
        args, text = self.args, ""
        if args.sample_every and i % args.sample_every == 0:
            monitor.save_grid(self.samples(), os.path.join(self.sample_dir, "%06d.png" % i),
                              nrow=max(int(args.n_sample ** 0.5), 1))
        if args.ppl_every and i % args.ppl_every == 0:
            g = torch.Generator(device=self.device).manual_seed(args.seed)    # the same pairs at every measurement
            with _frozen(self.g_ema) as g_ema:
                r = monitor.perceptual_path_length(g_ema, self.percept, args.ppl_samples, generator=g)
            with open(self.ppl_path, "a") as f:
                f.write(json.dumps({"iter": i, **{k: r[k] for k in ("ppl", "n", "kept", "lo", "hi")}}) + "\n")
            text = f" ppl {r['ppl']:.4f}"
        return text


def main(argv=None, percept=None):
    """`percept`: a PerceptualLoss for --ppl-every to use instead of the one --lpips-lin / --lpips-vgg describe."""
    args = build_parser().parse_args(argv)
    Monitor.check_args(args, percept)
    device = torch.device(args.device)
    torch.manual_seed(args.seed)
    if args.deterministic:
        from . import lib
        lib.set_deterministic(True)
    dt, gt = build_trainers(args, device)
    reals = dtrain.batches(args.data, args.size, args.batch, torch.Generator().manual_seed(args.seed), device)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    watch = Monitor(args, gt.g_ema, device, percept) if args.sample_every or args.ppl_every else None
    for i in range(args.iter):
        loss = iteration(dt, gt, next(reals).to(device), i)
        seen = watch.after(i) if watch is not None else ""
        if args.save_every and i and i % args.save_every == 0:
            torch.save(checkpoint(dt, gt), args.out)
        if seen or (args.log_every and (i % args.log_every == 0 or i == args.iter - 1)):
            print(f"{i}: d {loss['d'].item():.4f} g {loss['g'].item():.4f} r1 {loss['r1'].item():.4f} "
                  f"path {loss['path'].item():.4f} mean path {float(gt.mean_path_length):.4f} "
                  f"augment {dt.ada_aug_p:.4f}{seen}")
            if not all(math.isfinite(float(v)) for v in loss.values()):
                raise FloatingPointError(f"step {i}: a loss is not finite")
    torch.save(checkpoint(dt, gt), args.out)
    return args.out


if __name__ == "__main__":
    main()
