"""stylegan2-pytorch/train.py on one device: per iteration `DiscriminatorTrainer.step` (dtrain.py), then
`GeneratorTrainer.step` (gtrain.py).

    python -m gan2shape_amd.train --size 128 --channel-multiplier 1 --data root/car --iter 2000 --batch 16 \
        [--ckpt G_D.pt] [--augment] [--mixing 0.9] [--path-regularize 2] [--g-reg-every 4] [--save-every 10000] \
        [--deterministic] --out ckpts/train.pt

The checkpoint has train.py's keys: g, d, g_ema, g_optim, d_optim, ada_aug_p.  Without --ckpt the weights are fresh
(torch.manual_seed(--seed)) and g_ema starts as a copy of g (train.py:419-421).  Not built: distributed training,
wandb, sample grids, fp16."""
import argparse
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


def main(argv=None):
    args = build_parser().parse_args(argv)
    device = torch.device(args.device)
    torch.manual_seed(args.seed)
    if args.deterministic:
        from . import lib
        lib.set_deterministic(True)
    dt, gt = build_trainers(args, device)
    reals = dtrain.batches(args.data, args.size, args.batch, torch.Generator().manual_seed(args.seed), device)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for i in range(args.iter):
        loss = iteration(dt, gt, next(reals).to(device), i)
        if args.save_every and i and i % args.save_every == 0:
            torch.save(checkpoint(dt, gt), args.out)
        if args.log_every and (i % args.log_every == 0 or i == args.iter - 1):
            print(f"{i}: d {loss['d'].item():.4f} g {loss['g'].item():.4f} r1 {loss['r1'].item():.4f} "
                  f"path {loss['path'].item():.4f} mean path {float(gt.mean_path_length):.4f} "
                  f"augment {dt.ada_aug_p:.4f}")
            if not all(math.isfinite(float(v)) for v in loss.values()):
                raise FloatingPointError(f"step {i}: a loss is not finite")
    torch.save(checkpoint(dt, gt), args.out)
    return args.out


if __name__ == "__main__":
    main()
