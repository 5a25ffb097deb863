"""Fit view_mvn.pth and light_mvn.pth from a trained model's estimates over a dataset.

    python -m gan2shape_amd.fit_view_light --config car.yml --ckpt <file> [--ckpt <file> ...] --out checkpoints/view_light
                                           [--batch 64] [--images 0 3 7] [--ridge 0] [--device cuda]

For every listed image: `model.estimate_view_light`, the raw view (6) and light (4) parameters with the means of the
prior the model was trained with added — the config must therefore still carry that prior, as `view_mvn_path` /
`light_mvn_path` files or inline `view_mvn` / `light_mvn`.  Then ONE `view_light.mvn_fit` over the [N, 10] rows.

--ckpt as in evaluate: the checkpoint file of any one net, the others are found beside it.  One --ckpt serves every
image (a model trained over the whole list, GeneralizingTrainer2); as many as there are listed images pair up with
them in order (instance training: one model per image); any other count is refused before anything runs.

Written: <out>/view_mvn.pth, <out>/light_mvn.pth ({'mean', 'cov'}, float32: what ViewLightSampler loads),
<out>/estimates.npy ([N, 10] float32, one row per image in list order: view, then light), <out>/view_light.json
(n, both means, the smallest eigenvalue of each covariance, the stems, the ridge).  With fewer than 2 images or a
covariance that has no Cholesky factor nothing is written and the exit status is 1; --ridge adds to the diagonal.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

from .evaluate import checkpoint_path_of
from .view_light import VIEW_LIGHT_BLOCKS, estimate_rows, light_of, mvn_fit, save_mvn, view_of


def _stems(dataset):
    return [os.path.splitext(os.path.basename(name))[0] for name in dataset.file_list]


def build_parser():
    parser = argparse.ArgumentParser(prog="python -m gan2shape_amd.fit_view_light",
                                     description="Fit the view and light priors from a trained GAN2Shape model")
    parser.add_argument("--config", required=True, help="one yml file with the model's and the dataset's keys")
    parser.add_argument("--ckpt", required=True, action="append",
                        help="checkpoint file of one net; once for all images, or once per listed image")
    parser.add_argument("--images", type=int, nargs="+", default=None, help="indices into list.txt (default: all)")
    parser.add_argument("--batch", type=int, default=64)
    parser.add_argument("--ridge", type=float, default=0.0, help="added to the diagonal of the joint covariance")
    parser.add_argument("--out", required=True, help="output directory")
    parser.add_argument("--device", default="cuda")
    return parser


def main(argv=None, model=None, log=print):
    """`model`: an object to use instead of the one the config describes; with it one --ckpt is not loaded (tests; a
    caller that holds a loaded model), several still are, one per image.  Returns the exit status."""
    args = build_parser().parse_args(argv)
    import yaml
    from .dataset import ImageDataset, default_transform
    with open(args.config) as f:
        config = yaml.safe_load(f)
    device = torch.device(args.device)
    dataset = ImageDataset(os.path.join(config["root_path"], config.get("category")), subset=args.images,
                           transform=default_transform(config["image_size"], config.get("crop"), config.get("origin_size")))
    n = len(dataset)
    if n < 2:
        log(f"fit_view_light: a covariance needs at least 2 images, the list has {n}")
        return 1
    if len(args.ckpt) not in (1, n):
        log(f"fit_view_light: {len(args.ckpt)} --ckpt for {n} images: give one for all of them, or one per image")
        return 1
    given = model is not None
    if not given:
        from .model import GAN2Shape
        model = GAN2Shape(config, device=device)
    if len(args.ckpt) == 1:
        if not given:
            model.load_from_checkpoint(checkpoint_path_of(args.ckpt[0]))
        rows = estimate_rows(model, dataset, args.batch)
    else:
        parts = []
        for i, path in enumerate([checkpoint_path_of(c) for c in args.ckpt]):     # a bad name fails before any runs
            model.load_from_checkpoint(path)
            parts.append(estimate_rows(model, dataset, 1, [i]))
        rows = torch.cat(parts)
    try:
        fit = mvn_fit(rows, VIEW_LIGHT_BLOCKS, args.ridge)
    except ValueError as e:
        log(f"fit_view_light: {e}\n  columns 0-5 are the view, 6-9 the light; --ridge <small positive number> adds "
            f"to the diagonal of the covariance")
        return 1
    (vm, vc), (lm, lc) = view_of(fit), light_of(fit)
    os.makedirs(args.out, exist_ok=True)
    save_mvn(os.path.join(args.out, "view_mvn.pth"), vm, vc)
    save_mvn(os.path.join(args.out, "light_mvn.pth"), lm, lc)
    np.save(os.path.join(args.out, "estimates.npy"), rows.cpu().numpy().astype(np.float32))
    report = {"n": fit.n, "ridge": args.ridge, "stems": _stems(dataset),
              "view_mean": [float(v) for v in vm.cpu()], "light_mean": [float(v) for v in lm.cpu()],
              "view_min_eig": float(np.linalg.eigvalsh(vc.cpu().double().numpy()).min()),
              "light_min_eig": float(np.linalg.eigvalsh(lc.cpu().double().numpy()).min())}
    with open(os.path.join(args.out, "view_light.json"), "w") as f:
        json.dump(report, f, indent=1)
    log(f"{fit.n} images -> {args.out}: smallest eigenvalue view {report['view_min_eig']:.3g}, "
        f"light {report['light_min_eig']:.3g}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
