"""3D-aware image manipulation through the GAN, GAN2Shape's headline result: the recovered shape of an image is
rotated or relit, each rendered frame goes through the trained offset encoder E and the frozen generator G, and a
photo-realistic novel view comes back (`GAN2Shape.manipulate`; the frames are rendered by
`Renderer.render_pseudo_sweep`, the renderer E was trained on).

    python -m gan2shape_amd.manipulate --config <yml> --ckpt <file> --out <dir> [--images ...] [--frames 60]
           [--yaw 60] [--relight] [--light-radius 0.5] [--relative] [--gan-batch 8] [--device cuda]

The images and their latents come from `ImageLatentDataset` (<root_path>/<category>/list.txt and latents/<stem>.pt);
the checkpoint is loaded as `evaluate` loads it.  Written per image, under <out>/<stem>/:
    gan_rotate.gif      --frames frames, yaw from -<yaw> to +<yaw> degrees: the generator's images
    pseudo_rotate.gif   the rendered frames the encoder saw
    gan_relight.gif, pseudo_relight.gif   --relight: fixed pose, the light direction runs once round a circle of
                        --light-radius with the predicted ambient and diffuse terms
    latents.pt          the (frames, style_dim) latents w = latent + offset of the rotation
--relative composes every pose after the view predicted for the image (the zero pose is then the input's own pose);
without it the poses are about the canonical frame.
"""
import argparse
import os

import torch


def manipulate_image(model, image, latent, out_dir, stem, frames=60, yaw=60.0, relight=False, light_radius=0.5,
                     relative=False, gan_batch=8, log=print):
    """Everything the command writes for one image (3, H, W) in [-1, 1] and its latent."""
    from .model import light_sweep, rotation_views
    from .visualize import save_gif
    os.makedirs(out_dir, exist_ok=True)
    out = model.manipulate(image[None], latent, rotation_views(yaw, frames), relative=relative, gan_batch=gan_batch)
    save_gif(out["gan"], os.path.join(out_dir, "gan_rotate.gif"))
    save_gif(out["pseudo"], os.path.join(out_dir, "pseudo_rotate.gif"))
    torch.save(out["w"].detach().cpu(), os.path.join(out_dir, "latents.pt"))
    if relight:
        a, b = (float(v) for v in out["light"][0, :2])
        lit = model.manipulate(image[None], latent, torch.zeros(frames, 6), light_sweep(a, b, frames, light_radius),
                               relative=relative, gan_batch=gan_batch)
        save_gif(lit["gan"], os.path.join(out_dir, "gan_relight.gif"))
        save_gif(lit["pseudo"], os.path.join(out_dir, "pseudo_relight.gif"))
    log(f"{stem}: {frames} frames -> {out_dir}")


def build_parser():
    parser = argparse.ArgumentParser(prog="python -m gan2shape_amd.manipulate",
                                     description="Rotate and relight an image through the GAN")
    parser.add_argument("--config", required=True, help="one yml file with the model's and the dataset's keys")
    parser.add_argument("--ckpt", default=None, help="checkpoint file of one net; the others are found beside it")
    parser.add_argument("--out", required=True, help="output directory")
    parser.add_argument("--images", type=int, nargs="+", default=None, help="indices into list.txt (default: all)")
    parser.add_argument("--frames", type=int, default=60, help="frames per animation")
    parser.add_argument("--yaw", type=float, default=60.0, help="the rotation runs from -yaw to +yaw degrees")
    parser.add_argument("--relight", action="store_true", help="also write gan_relight.gif and pseudo_relight.gif")
    parser.add_argument("--light-radius", dest="light_radius", type=float, default=0.5,
                        help="radius of the circle the light's (dx, dy) runs round")
    parser.add_argument("--relative", action="store_true", help="compose the poses after the predicted view")
    parser.add_argument("--gan-batch", dest="gan_batch", type=int, default=8, help="frames per generator forward")
    parser.add_argument("--device", default="cuda")
    return parser


def main(argv=None, model=None):
    """`model`: an object to use instead of the one the config and --ckpt describe, as in evaluate.main.  Returns the
    list of per-image output directories."""
    args = build_parser().parse_args(argv)
    if args.frames < 1:
        raise ValueError("--frames must be at least 1")
    import yaml
    from .dataset import ImageLatentDataset, default_transform
    from .evaluate import _stems, checkpoint_path_of
    with open(args.config) as f:
        config = yaml.safe_load(f)
    device = torch.device(args.device)
    if model is None:
        if args.ckpt is None:
            raise ValueError("--ckpt is required when no model is given")
        from .model import GAN2Shape
        model = GAN2Shape(config, device=device)
        model.load_from_checkpoint(checkpoint_path_of(args.ckpt))
    dataset = ImageLatentDataset(os.path.join(config["root_path"], config.get("category")), subset=args.images,
                                 transform=default_transform(config["image_size"], config.get("crop"),
                                                             config.get("origin_size")))
    written = []
    for i, stem in enumerate(_stems(dataset.image_dataset)):
        image, latent, _ = dataset[i]
        out_dir = os.path.join(args.out, stem)
        manipulate_image(model, image.to(device), latent.to(device), out_dir, stem, frames=args.frames, yaw=args.yaw,
                         relight=args.relight, light_radius=args.light_radius, relative=args.relative,
                         gan_batch=args.gan_batch)
        written.append(out_dir)
    return written


if __name__ == "__main__":
    main()
