"""Evaluate a trained model over a dataset: the counterpart of the reference's evaluate_results.py, without
its plotting.

    python -m gan2shape_amd.evaluate --config configs/face.yml --ckpt <file> --out results/eval
                                     [--images 0 3 7] [--mask] [--gt-depth <dir> [--gt-background]]
                                     [--record-loss <name>] [--recon-metrics]

For every image: `model.evaluate_results` (or `evaluate_results_masked` with --mask, NaN outside the object
mask of MaskingModel), optionally the step-1 loss (evaluate_results.py:92-94,107-114).  Images go through the
model one at a time, as in the reference: `get_clamped_depth` centres over the whole batch, so batching would
change the depths.  The recovered depths stay on the device and are scored against `--gt-depth` with ONE
batched `metrics.depth_metrics` call at the end.

Written: <out>/depth/<stem>.npy (float32 (H, W)), <out>/metrics.json ({"images": {stem: {count, mae, mse, side,
mad}}, "summary": DepthMetrics.summary()}; with no --gt-depth only the names), <out>/step1_<name>_model.npy.

--recon-metrics scores what needs no ground truth: the reconstruction `recon_im` that `evaluate_results` renders from
the recovered depth, albedo, view and light, against the input image — `metrics.image_metrics` (MAE, MSE, PSNR, SSIM),
ONE batched call over all images at the end, inside the MaskingModel mask (the finite pixels of the masked depth) with
--mask.  data_range is 2: dataset.ImageDataset hands out images in [-1, 1] and the model's reconstruction is clamped
to [-1, 1] (model.py, `grid_sample(texture, ..., -1, 1)`).  Per image the six values go to images[stem]["recon"], their
`ImageMetrics.summary()` to "recon_summary"; a model with a `perceptual_loss` module (the LPIPS of step 1) also gets
images[stem]["recon"]["lpips"].  Without the flag nothing of this is computed, written or logged.

--config is one yml file (`reconstruct` merges minimal_config.yml with configs/<category>.yml as the reference's
command line does; `config.load_config` reads either form).  Keys read here: image_size, root_path + category (the dataset is
<root_path>/<category>/list.txt), parsing_ckpt_dir / parsing_size (--mask), and everything GAN2Shape reads.
--ckpt is the checkpoint file of any one net (`<net>_image_..._stage_..._it_....pth`); the other four are
found beside it under their own names, as `load_from_checkpoint` expects.  --gt-depth holds <image stem>.npy:
float depth (H, W) already in the model's range; NaN or non-positive values are "no ground truth here".
--gt-background additionally drops each map's farthest value as background (`gt_mask_from_depth`, the BFM convention).
metrics.json is strict JSON: a NaN metric (an image without a counted pixel) is written as null.
"""
import argparse
import json
import os

import numpy as np
import torch

from .metrics import IMAGE_KEYS, KEYS, DepthMetrics, ImageMetrics, depth_metrics, gt_mask_from_depth, image_metrics

IMAGE_DATA_RANGE = 2.0      # images and reconstructions live in [-1, 1]


def checkpoint_path_of(ckpt):
    """net name -> file, from the file of any one net (model.build_checkpoint_path's naming)."""
    from .model import GAN2Shape
    folder, base = os.path.split(ckpt)
    for net in GAN2Shape.NETS:
        if base.startswith(net + "_"):
            rest = base[len(net):]
            return lambda name: os.path.join(folder, name + rest)
    if "{net}" in ckpt:
        return lambda name: ckpt.format(net=name)
    raise ValueError(f"--ckpt {ckpt!r}: expected the file of one net ({', '.join(GAN2Shape.NETS)}_image_...pth) "
                     f"or a pattern with {{net}}")


def _json_number(v):
    v = float(v)
    return v if np.isfinite(v) else None


def summary_json(summary):
    """A `summary()` dict of metrics.DepthMetrics / ImageMetrics with its (mean, std) tuples as JSON lists."""
    return {k: [_json_number(x) for x in v] if isinstance(v, tuple) else v for k, v in summary.items()}


def recon_scores(recons, images, masks=None, perceptual=None):
    """One `image_metrics` call over all reconstructions (N, 3, H, W) against their images -> (per-image list of
    {count, mae, mse, psnr, ssim_count, ssim[, lpips]} with JSON numbers, ImageMetrics.summary()).  perceptual: the
    model's LPIPS module or None; it runs image by image, as in step 1."""
    scores = image_metrics(recons, images, masks, data_range=IMAGE_DATA_RANGE)
    acc = ImageMetrics()
    acc.update(scores)
    host = {k: scores[k].cpu().numpy().astype(np.float64) for k in IMAGE_KEYS}
    rows = [{k: _json_number(host[k][j]) for k in IMAGE_KEYS} for j in range(len(recons))]
    if perceptual is not None:
        with torch.no_grad():
            for j, row in enumerate(rows):
                row["lpips"] = _json_number(perceptual(recons[j:j + 1], images[j:j + 1]).mean())
    return rows, acc.summary()


def log_recon_summary(s, log):
    log(f"{s['images']} reconstructions scored, {s['skipped']} skipped (no counted pixel), {s['exact']} exact")
    for k in ("mae", "mse", "psnr", "ssim"):
        log(f"  {k:5s} {s[k][0]:.6g} +- {s[k][1]:.6g}")


def _stems(dataset):
    return [os.path.splitext(os.path.basename(name))[0] for name in dataset.file_list]


def evaluate(model, dataset, out_dir, masking_model=None, gt_depth_dir=None, gt_background=False, record_loss=None,
             device=None, log=print, recon_metrics=False):
    """The loop of evaluate_results.py:88-114 over `dataset` (an ImageDataset).  Returns the dict written to
    metrics.json.  recon_metrics: also score each reconstruction against its image (module docstring)."""
    device = torch.device(device if device is not None else model.device)
    stems = _stems(dataset)
    os.makedirs(os.path.join(out_dir, "depth"), exist_ok=True)
    depths, losses, recons, images = [], [], [], []
    for i in range(len(dataset)):
        image = dataset[i].unsqueeze(0).to(device)
        if masking_model is not None:
            recon_im, depth = model.evaluate_results_masked(image, masking_model)
        else:
            recon_im, depth = model.evaluate_results(image)
        depths.append(depth.detach().reshape(depth.shape[-2], depth.shape[-1]).float())
        if recon_metrics:
            recons.append(recon_im.detach()[0].float())
            images.append(image[0].float())
        if record_loss is not None:
            loss, _ = model.forward_step1(image, None, None, step1=True, eval=False)
            losses.append(float(loss.detach().cpu()))
    result = {"images": {stem: {} for stem in stems}}
    if not depths:
        log("no images")
    else:
        depths = torch.stack(depths)             # (N, H, W), still on the device
        for stem, d in zip(stems, depths.cpu().numpy()):
            np.save(os.path.join(out_dir, "depth", stem + ".npy"), d)
    if gt_depth_dir is not None and len(stems):
        gt = torch.from_numpy(np.stack([np.load(os.path.join(gt_depth_dir, stem + ".npy")).astype(np.float32)
                                        for stem in stems])).to(device)
        if gt.shape != depths.shape:
            raise ValueError(f"--gt-depth maps are {tuple(gt.shape[1:])}, the model's depth is {tuple(depths.shape[1:])}")
        mask_gt = gt_mask_from_depth(gt) if gt_background else None
        scores = depth_metrics(depths, gt, None, mask_gt, renderer=model.renderer, erode=True)   # one call
        acc = DepthMetrics()
        acc.update(scores)
        host = {k: scores[k].cpu().numpy().astype(np.float64) for k in KEYS}
        for j, stem in enumerate(stems):
            result["images"][stem] = {k: _json_number(host[k][j]) for k in KEYS}
        s = acc.summary()
        result["summary"] = summary_json(s)
        log(f"{s['images']} images scored, {s['skipped']} skipped (no counted pixel)")
        for k in ("mae", "mse", "side", "mad"):
            log(f"  {k:5s} {s[k][0]:.6g} +- {s[k][1]:.6g}")
    if recon_metrics and recons:
        masks = torch.isfinite(depths).float() if masking_model is not None else None
        rows, s = recon_scores(torch.stack(recons), torch.stack(images), masks, getattr(model, "perceptual_loss", None))
        for stem, row in zip(stems, rows):
            result["images"][stem]["recon"] = row
        result["recon_summary"] = summary_json(s)
        log_recon_summary(s, log)
    if record_loss is not None:
        losses = np.array(losses)
        log(f"mean =  {np.mean(losses) if len(losses) else float('nan')}")
        log(f"std =  {np.std(losses) if len(losses) else float('nan')}")
        np.save(os.path.join(out_dir, "step1_" + record_loss + "_model"), losses)
        result["step1_loss"] = {"mean": float(np.mean(losses)) if len(losses) else None,
                                "std": float(np.std(losses)) if len(losses) else None}
    with open(os.path.join(out_dir, "metrics.json"), "w") as f:
        json.dump(result, f, indent=1)
    return result


def build_parser():
    parser = argparse.ArgumentParser(prog="python -m gan2shape_amd.evaluate",
                                     description="Evaluate a trained GAN2Shape model: depths, depth / normal metrics")
    parser.add_argument("--config", required=True, help="one yml file with the model's and the dataset's keys")
    parser.add_argument("--ckpt", required=True, help="checkpoint file of one net; the others are found beside it")
    parser.add_argument("--images", type=int, nargs="+", default=None, help="indices into list.txt (default: all)")
    parser.add_argument("--mask", action="store_true",
                        help="mask the depth with MaskingModel (config: parsing_ckpt_dir, parsing_size)")
    parser.add_argument("--gt-depth", dest="gt_depth", default=None,
                        help="directory of <image stem>.npy ground-truth depths in the model's range")
    parser.add_argument("--gt-background", dest="gt_background", action="store_true",
                        help="the farthest value of each ground-truth map is background (BFM convention)")
    parser.add_argument("--record-loss", dest="record_loss", default=None,
                        help="name: record the step-1 loss per image, save <out>/step1_<name>_model.npy")
    parser.add_argument("--recon-metrics", dest="recon_metrics", action="store_true",
                        help="score each reconstruction against its image: MAE, MSE, PSNR, SSIM (inside the mask with --mask)")
    parser.add_argument("--out", required=True, help="output directory")
    parser.add_argument("--device", default="cuda")
    return parser


def main(argv=None, model=None, masking_model=None):
    """`model` / `masking_model`: objects to use instead of the ones the config and --ckpt describe (tests; a
    caller that holds a loaded model).  Returns the dict written to metrics.json."""
    args = build_parser().parse_args(argv)
    import yaml
    from .dataset import ImageDataset, default_transform
    with open(args.config) as f:
        config = yaml.safe_load(f)
    device = torch.device(args.device)
    category = config.get("category")
    if model is None:
        from .model import GAN2Shape
        model = GAN2Shape(config, device=device)
        model.load_from_checkpoint(checkpoint_path_of(args.ckpt))
    if args.mask and masking_model is None:
        from .parsing import MaskingModel
        masking_model = MaskingModel(category, device=device, ckpt_dir=config["parsing_ckpt_dir"],
                                     size=config.get("parsing_size"))
    dataset = ImageDataset(os.path.join(config["root_path"], category), subset=args.images,
                           transform=default_transform(config["image_size"], config.get("crop"), config.get("origin_size")))
    return evaluate(model, dataset, args.out, masking_model=masking_model if args.mask else None,
                    gt_depth_dir=args.gt_depth, gt_background=args.gt_background, record_loss=args.record_loss, device=device,
                    recon_metrics=args.recon_metrics)


if __name__ == "__main__":
    main()
