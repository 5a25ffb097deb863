"""Perceptual path length of a trained generator — the counterpart of the reference's stylegan2-pytorch/ppl.py.

    python -m gan2shape_amd.ppl --ckpt G.pt --size 128 --channel-multiplier 1 --lpips-lin vgg.pth --lpips-vgg vgg16.pth \
        [--n-sample 5000] [--batch 64] [--space w|z] [--sampling full|end] [--eps 1e-4] [--crop] [--seed 0] \
        [--out ppl.json] [--save-distances] [--allow-random-lpips] [--device cuda]

Prints `ppl: <value>` and, with --out, writes what monitor.perceptual_path_length returns as JSON (the per-pair
distances only with --save-distances).  The number means something only under the trained LPIPS weights
(lpips/weights/v0.1/vgg.pth and a torchvision VGG16 state dict): without both files the command refuses to run unless
--allow-random-lpips is given, and the JSON then says so."""
import argparse
import json

import torch

from . import monitor


def build_parser():
    parser = argparse.ArgumentParser(prog="python -m gan2shape_amd.ppl",
                                     description="Perceptual path length of a StyleGAN2 generator")
    parser.add_argument("--ckpt", required=True, help="checkpoint with the generator under 'g_ema'")
    parser.add_argument("--size", type=int, required=True, help="image side of the generator")
    parser.add_argument("--channel-multiplier", dest="channel_multiplier", type=int, default=2)
    parser.add_argument("--latent", type=int, default=512)
    parser.add_argument("--n-mlp", dest="n_mlp", type=int, default=8)
    parser.add_argument("--lpips-lin", dest="lpips_lin", default=None, help="lpips/weights/v0.1/vgg.pth")
    parser.add_argument("--lpips-vgg", dest="lpips_vgg", default=None, help="a torchvision vgg16 state dict")
    parser.add_argument("--allow-random-lpips", dest="allow_random_lpips", action="store_true",
                        help="run with a randomly initialised LPIPS network: the result is not a PPL")
    parser.add_argument("--n-sample", dest="n_sample", type=int, default=5000)
    parser.add_argument("--batch", type=int, default=64)
    parser.add_argument("--space", choices=monitor.SPACES, default="w")
    parser.add_argument("--sampling", choices=monitor.SAMPLINGS, default="full")
    parser.add_argument("--eps", type=float, default=1e-4)
    parser.add_argument("--crop", action="store_true")
    parser.add_argument("--seed", type=int, default=0)
    parser.add_argument("--out", default=None, help="JSON file for the result")
    parser.add_argument("--save-distances", dest="save_distances", action="store_true")
    parser.add_argument("--device", default="cuda")
    return parser


def check_percept(percept, allow_random=False):
    """Refuse a PerceptualLoss without its trained weights: a PPL from random weights is not a PPL."""
    if not getattr(percept, "pretrained", False) and not allow_random:
        raise SystemExit("ppl: the LPIPS network has no trained weights (give --lpips-lin and --lpips-vgg); a path length "
                         "under random weights is not a PPL.  --allow-random-lpips runs anyway.")


def main(argv=None, G=None, percept=None):
    """`G`, `percept`: modules to use instead of the ones the arguments describe.  Returns the result dict."""
    args = build_parser().parse_args(argv)
    device = torch.device(args.device)
    if percept is None:
        from .lpips import PerceptualLoss
        percept = PerceptualLoss(lin_weights_path=args.lpips_lin, vgg_weights_path=args.lpips_vgg)
    check_percept(percept, args.allow_random_lpips)
    if G is None:
        from .stylegan2 import Generator
        G = Generator(args.size, args.latent, args.n_mlp, channel_multiplier=args.channel_multiplier)
        state = torch.load(args.ckpt, map_location="cpu", weights_only=True)
        G.load_state_dict(state["g_ema"], strict=False)
    G = G.to(device).eval().requires_grad_(False)
    percept = percept.to(device).eval()
    generator = torch.Generator(device=device).manual_seed(args.seed)
    result = monitor.perceptual_path_length(G, percept, args.n_sample, args.batch, args.space, args.sampling, args.eps,
                                            args.crop, generator)
    print(f"ppl: {result['ppl']}")
    if args.out:
        record = {k: v for k, v in result.items() if k != "distances"}
        record.update(space=args.space, sampling=args.sampling, eps=args.eps, crop=args.crop, seed=args.seed,
                      lpips_pretrained=bool(getattr(percept, "pretrained", False)))
        if args.save_distances:
            record["distances"] = result["distances"].tolist()
        with open(args.out, "w") as f:
            json.dump(record, f, indent=1)
            f.write("\n")
    return result


if __name__ == "__main__":
    main()
