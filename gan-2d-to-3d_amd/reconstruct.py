"""Train GAN2Shape from the command line: the counterpart of the reference's main.py, without wandb and plotting.

    python -m gan2shape_amd.reconstruct --category car --config-dir . --save-ckpts --graphs --out results/car
    python -m gan2shape_amd.reconstruct --config-file config.yml [--generalize] [--images 0 3 7] ...

Configuration (config.load_config): with --category, <config-dir>/minimal_config.yml overlaid with
<config-dir>/configs/<category>.yml; otherwise the one file --config-file.  --prior overrides `prior_name`.  The dataset
is ImageLatentDataset(<root_path>/<category>) with default_transform(image_size, crop, origin_size), restricted to
--images.  Without --generalize a `Trainer` runs image by image with main.py's four stages (700,700,600 then three times
200,500,400); with it a `GeneralizingTrainer2` runs `n_epochs_generalized` epochs of 13,22,18.  --stages
"700,700,600;200,500,400" replaces the schedule: stages separated by ';', each `step1,step2,step3` iterations.
--save-ckpts writes the checkpoints `evaluate --ckpt` reads (config `our_nets_ckpts.VLADE_nets`); --load-pretrained
loads the latest ones first.

--graphs replays the step blocks as HIP graphs (graphs.py): the trainer is built with capturable=True and a non-default
stream is made current before anything runs, as captures require; it needs a CUDA device.  --deterministic puts libg2s
in its reproducible mode (lib.set_deterministic); with --seed, a run then repeats bit for bit, graphs or not.

--out DIR: after the last stage of each image (with --generalize: after the last epoch) `model.evaluate_results` gives
the reconstruction and the depth, written as DIR/recon/<stem>.png (8 bits, to look at; beside it <stem>.npy, float32
(3, H, W) in [-1, 1]: the values the report scores) and DIR/depth/<stem>.npy (float32 (H, W), what
`visualize --depth-dir` reads).  The reconstructions stay on the device; after the fit ONE `metrics.image_metrics` call
scores them all against their images (data_range 2: both live in [-1, 1]) and DIR/report.json holds, per image, the
trainer's `history` rows and {count, mae, mse, psnr, ssim_count, ssim}, their `ImageMetrics.summary()`, the merged
config, the schedule and `total_it`.  Non-finite numbers are written as null, as `evaluate` does.  Without --out the
command trains and writes checkpoints only.
"""
import argparse
import json
import logging
import os
import sys

import numpy as np
import torch

STAGES_INSTANCE = [(700, 700, 600), (200, 500, 400), (200, 500, 400), (200, 500, 400)]     # main.py:148-151
STAGES_GENERALIZE = [(13, 22, 18)]                                                        # main.py:141


def _stage_dicts(rows):
    return [{'step1': a, 'step2': b, 'step3': c} for a, b, c in rows]


def default_stages(generalize):
    """main.py's schedule: four stages for `Trainer`, one of 13,22,18 for `GeneralizingTrainer2`."""
    return _stage_dicts(STAGES_GENERALIZE if generalize else STAGES_INSTANCE)


def parse_stages(text):
    """"700,700,600;200,500,400" -> [{'step1': 700, 'step2': 700, 'step3': 600}, {...}].  A malformed string raises
    ValueError naming the offending field."""
    rows = []
    for s, stage in enumerate(text.split(";")):
        fields = [f.strip() for f in stage.split(",")]
        if len(fields) != 3:
            raise ValueError(f"--stages: stage {s + 1} {stage.strip()!r} has {len(fields)} fields, expected "
                             f"step1,step2,step3")
        for k, field in enumerate(fields):
            if not field.isdigit():
                raise ValueError(f"--stages: stage {s + 1}, step{k + 1}: {field!r} is not a non-negative integer")
        rows.append(tuple(int(f) for f in fields))
    return _stage_dicts(rows)


def build_parser():
    parser = argparse.ArgumentParser(prog="python -m gan2shape_amd.reconstruct",
                                     description="Run GAN2Shape: recover depth, albedo, view and light of images")
    parser.add_argument("--config-file", dest="config_file", default="config.yml", help="path of the config yaml file")
    parser.add_argument("--category", default=None,
                        help="the object category: merges minimal_config.yml with configs/<category>.yml")
    parser.add_argument("--config-dir", dest="config_dir", default=".",
                        help="directory of minimal_config.yml and configs/ (with --category)")
    parser.add_argument("--prior", default=None, help="the prior to use; overrides the config's prior_name")
    parser.add_argument("--save-ckpts", dest="save_ckpts", action="store_true", help="save the nets' weights")
    parser.add_argument("--debug", action="store_true", help="debug the model (skips the prior pre-training)")
    parser.add_argument("--log-file", dest="log_file", default=None, help="name of the logging file")
    parser.add_argument("--load-pretrained", dest="load_pretrained", action="store_true",
                        help="load pretrained weights before training")
    parser.add_argument("--generalize", action="store_true", help="the joint training procedure that favours generalisation")
    parser.add_argument("--images", action="append", type=int, nargs="+", default=None,
                        help="image numbers (indices into list.txt) on which to run")
    parser.add_argument("--device", default="cuda")
    parser.add_argument("--seed", type=int, default=None, help="torch.manual_seed before the nets are built")
    parser.add_argument("--deterministic", action="store_true", help="reproducible launch partitions in libg2s")
    parser.add_argument("--graphs", action="store_true", help="replay the step blocks as HIP graphs (needs a CUDA device)")
    parser.add_argument("--stages", default=None,
                        help='the schedule, "step1,step2,step3;..." iterations per stage (default: main.py\'s)')
    parser.add_argument("--out", default=None, help="directory for depths, reconstructions and report.json")
    return parser


def _stem_of(dataset, index):
    files = getattr(getattr(dataset, "image_dataset", None), "file_list", None)
    return os.path.splitext(os.path.basename(files[index]))[0] if files is not None else f"image_{index}"


def _save_png(path, image):
    """image (3, H, W) in [-1, 1] -> 8-bit PNG."""
    from PIL import Image
    a = ((image.detach().float().clamp(-1, 1) + 1) * 127.5).round().to(torch.uint8).permute(1, 2, 0).cpu().numpy()
    Image.fromarray(np.ascontiguousarray(a)).save(path)


class _Results():
    """The on_image_done callback of --out: writes each image's depth and reconstruction, keeps what the report scores."""

    def __init__(self, out_dir, dataset):
        self.out_dir, self.dataset = out_dir, dataset
        self.indices, self.recons, self.images = [], [], []
        os.makedirs(os.path.join(out_dir, "depth"), exist_ok=True)
        os.makedirs(os.path.join(out_dir, "recon"), exist_ok=True)

    def __call__(self, data_index, image, trainer):
        recon, depth = trainer.model.evaluate_results(image)
        stem = _stem_of(self.dataset, data_index)
        depth = depth.detach().reshape(depth.shape[-2], depth.shape[-1]).float()
        np.save(os.path.join(self.out_dir, "depth", stem + ".npy"), depth.cpu().numpy())
        _save_png(os.path.join(self.out_dir, "recon", stem + ".png"), recon[0])
        np.save(os.path.join(self.out_dir, "recon", stem + ".npy"), recon.detach()[0].float().cpu().numpy())
        self.indices.append(data_index)
        self.recons.append(recon.detach()[0].float())
        self.images.append(image.detach()[0].float())

    def report(self, trainer, config, stages, total_it, args):
        from .evaluate import _json_number, log_recon_summary, recon_scores, summary_json
        report = {"images": {}, "summary": None, "config": config, "stages": stages, "total_it": total_it,
                  "generalize": bool(args.generalize), "graphs": bool(args.graphs)}
        if self.recons:
            rows, summary = recon_scores(torch.stack(self.recons), torch.stack(self.images))      # one call
            for index, row in zip(self.indices, rows):
                history = [[list(i) if isinstance(i, tuple) else i, stage, step, None if loss is None else _json_number(loss)]
                           for i, stage, step, loss in trainer.history
                           if i == index or (isinstance(i, tuple) and index in i)]
                report["images"][_stem_of(self.dataset, index)] = {"index": index, "history": history, "recon": row}
            report["summary"] = summary_json(summary)
            log_recon_summary(summary, print)
        with open(os.path.join(self.out_dir, "report.json"), "w") as f:
            json.dump(report, f, indent=1, default=str)
        return report


def main(argv=None, model=None, masking_model=None, dataset=None):
    """`model`: the model class (anything with GAN2Shape's constructor signature) the trainer builds instead of GAN2Shape;
    `masking_model`: handed to the trainer; `dataset`: (image, latent, index) items to use instead of the folder the
    config names (tests; a caller that holds these objects).  Returns the dict written to report.json, or
    {"total_it": n} without --out."""
    parser = build_parser()
    args = parser.parse_args(argv)
    device = torch.device(args.device)
    if args.graphs and device.type != "cuda":
        parser.error("--graphs replays HIP graphs and needs a CUDA device, not --device " + args.device)
    try:
        stages = parse_stages(args.stages) if args.stages is not None else default_stages(args.generalize)
    except ValueError as e:
        parser.error(str(e))
    if device.type == "cuda" and not torch.cuda.is_available():
        print("A CUDA-enabled GPU is required to run this model")
        sys.exit(1)

    from .config import load_config
    config = load_config(args.config_file, args.category, args.config_dir)
    category = config.get('category')
    if args.prior is not None:
        config['prior_name'] = args.prior
    logging.basicConfig(filename=args.log_file, format='%(asctime)s %(levelname)-8s %(message)s', level=logging.INFO)

    if args.graphs:      # before anything runs: a backward on the default stream would break every later capture
        torch.cuda.set_stream(torch.cuda.Stream(device))
    if args.deterministic and device.type == "cuda":
        from . import lib
        lib.set_deterministic(True)
    if args.seed is not None:
        torch.manual_seed(args.seed)

    load_dict = None
    if args.load_pretrained:
        load_dict = {'category': category, 'base_path': config.get('our_nets_ckpts')['VLADE_nets'],
                     'stage': config.get('stage', '*'), 'iteration': config.get('iteration', '*'),
                     'time': config.get('time', '*')}
    if not args.save_ckpts:
        print(">>> Warning, not saving checkpoints.")
        print("If this is a real run you want to rerun with --save-ckpts <<<")

    subset = args.images
    if subset is not None:
        subset = [image for image_list in subset for image in image_list]
    if dataset is None:
        from .dataset import ImageLatentDataset, default_transform
        try:
            dataset = ImageLatentDataset(os.path.join(config.get('root_path'), category), subset=subset,
                                         transform=default_transform(config.get('image_size'), config.get('crop'),
                                                                     config.get('origin_size')))
        except IndexError as e:
            print(e, ": Invalid image subset indices specified \nExiting...")
            sys.exit(1)

    from .trainer import GeneralizingTrainer2, Trainer
    if model is None:
        from .model import GAN2Shape
        model = GAN2Shape
    if args.generalize and subset is not None:
        print(">>> Warning, using a subset with a generalizing trainer.")
        print("It is always better to use the whole dataset.<<<")
    trainer = (GeneralizingTrainer2 if args.generalize else Trainer)(
        model=model, model_config=config, debug=args.debug, save_ckpts=args.save_ckpts, load_dict=load_dict,
        masking_model=masking_model, device=device, capturable=args.graphs)
    results = _Results(args.out, dataset) if args.out is not None else None
    total_it = trainer.fit(dataset, stages=stages, batch_size=config.get('batch_size', 2), graphs=args.graphs,
                           on_image_done=results)
    if results is None:
        return {"total_it": total_it}
    return results.report(trainer, config, stages, total_it, args)


if __name__ == "__main__":
    main()
