"""Look at the recovered shape: turntable and relighting animations, still images and a mesh file — the counterpart
of the reference's plotting.py (plot_reconstructions, plotly_3d_animate), drawn with the package's own rasterizer
through `Renderer.render_sweep` (all frames of a sweep in three launches) instead of plotly.

    python -m gan2shape_amd.visualize --config <yml> (--ckpt <file> | --depth-dir <dir>) --out <dir>
           [--images ...] [--mask] [--modes texture shaded shape normal] [--relight] [--frames 60] [--obj]
           [--device cuda]

--ckpt recovers the depth as `evaluate` does (`model.evaluate_results`, or `evaluate_results_masked` with --mask).
--depth-dir reads the <stem>.npy files `evaluate` wrote (<evaluate's out>/depth), NaN = masked; no model is built.
In both cases "shaded" uses the image as albedo.  Written per image, under <out>/<stem>/:
    turntable_<mode>.gif   2 * --frames frames along the camera path of plotting.py:99-107, one file per mode
    depth.png, normal.png  the depth (min / max over its finite values, masked pixels white) and its normals
    recon.png              the model's reconstruction (only when a model ran)
    relight.gif            --relight: frontal view, the light direction runs round `light_circle`
    <stem>.obj/.mtl/.png   --obj: the depth mesh with the image as texture

Masked depths: a NaN vertex is invalid.  It gets a finite STAND-IN, the farthest finite depth of its image
(`fill_masked_depth`), so that every vertex and every normal stays finite, and the mesh is rendered with an explicit
face list that holds only the faces whose three vertices are valid (`valid_faces`): no face touches a stand-in
vertex, so it is never drawn.  The normals of valid vertices next to the mask are computed across the stand-in
depth and lean towards the back plane there.  The box plot, the plotly HTML and wandb logging of the reference are
not rebuilt.
"""
import argparse
import math
import os

import numpy as np
import torch

MODES = ("texture", "shaded", "shape", "normal")
MIN_DEPTH, MAX_DEPTH = 0.9, 1.1                    # GAN2Shape's depth range (model.py:120-121)
HEADLIGHT = (0.35, 0.65, 0.0, 0.0, 1.0)            # la, lb, direction: the light of the turntables, fixed to the camera


# ------------------------------------------------------------------------------------------------- poses and lights
def turntable_rotations(n=60, max_x=0.75, eye_z=1.5):
    """(2n, 3) angle triples: the camera path of plotting.py:99-107.  The eye moves along x_i = arange(-max_x, max_x,
    2 max_x / n) and back along -x_i at height eye_z; frame i is the yaw atan2(x_i, eye_z)."""
    x = np.arange(-max_x, max_x, 2 * max_x / n)
    x = np.concatenate([x, max_x + (-max_x) - x])
    rot = np.zeros((len(x), 3), np.float32)
    rot[:, 1] = np.arctan2(x, eye_z)
    return torch.from_numpy(rot)


def yaw_pitch_rotations(maxr=(20, 90), nsample=(5, 9)):
    """(nsample[1] + nsample[0], 3): the poses of Renderer.render_view — a yaw sweep to +-maxr[1] degrees, then a
    pitch sweep to +-maxr[0]."""
    pitch = torch.linspace(-math.pi / 180 * maxr[0], math.pi / 180 * maxr[0], nsample[0])
    yaw = torch.linspace(-math.pi / 180 * maxr[1], math.pi / 180 * maxr[1], nsample[1])
    rot = torch.zeros(nsample[1] + nsample[0], 3)
    rot[:nsample[1], 1] = yaw
    rot[nsample[1]:, 0] = pitch
    return rot


def light_circle(n=60, la=0.35, lb=0.65, radius=1.0):
    """(n, 5) lights (la, lb, lx, ly, lz) whose (lx, ly) run once round a circle of `radius`; the direction is
    (lx, ly, 1) normalised, as get_lighting_directions builds it (model.py:347-353)."""
    phi = torch.arange(n, dtype=torch.float64) * (2 * math.pi / n)
    d = torch.stack([radius * phi.cos(), radius * phi.sin(), torch.ones(n, dtype=torch.float64)], 1)
    d = d / (d ** 2).sum(1, keepdim=True) ** 0.5
    ab = torch.tensor([la, lb], dtype=torch.float64).expand(n, 2)
    return torch.cat([ab, d], 1).float()


# ------------------------------------------------------------------------------------------------------ image files
def _numpy(x):
    return x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)


def to_uint8(frames, alpha=None):
    """(..., C, H, W) in [-1, 1] -> (..., H, W, 3) uint8 (one channel is repeated, a fourth is dropped).  `alpha`
    (..., H, W): the colour is composited over a white background, as the reference's plots do."""
    x = np.clip(_numpy(frames).astype(np.float32) / 2 + 0.5, 0.0, 1.0)
    if x.shape[-3] == 1:
        x = np.repeat(x, 3, -3)
    x = x[..., :3, :, :]
    if alpha is not None:
        a = np.clip(_numpy(alpha).astype(np.float32), 0.0, 1.0)[..., None, :, :]
        x = x * a + (1.0 - a)
    return np.moveaxis(np.rint(x * 255).astype(np.uint8), -3, -1)


def save_png(frame, path, alpha=None):
    """One (C, H, W) frame in [-1, 1] -> PNG."""
    from PIL import Image
    Image.fromarray(to_uint8(frame, alpha)).save(path)


def save_gif(frames, path, duration_ms=50, alpha=None):
    """(V, C, H, W) frames in [-1, 1] -> a looping GIF, `duration_ms` per frame.  Each frame gets an adaptive palette
    of 255 colours without dithering plus one entry that is pure white, which every exactly-white pixel is given: the
    background neither flickers nor picks up a tint from the palette."""
    from PIL import Image
    images = []
    for f in to_uint8(frames, alpha):
        q = Image.fromarray(f).quantize(colors=255, dither=Image.Dither.NONE)
        palette = (list(q.getpalette()) + [0] * 768)[:765] + [255, 255, 255]
        index = np.asarray(q).copy()
        index[(f == 255).all(-1)] = 255
        q = Image.fromarray(index, mode="P")
        q.putpalette(palette)
        images.append(q)
    images[0].save(path, save_all=True, append_images=images[1:], duration=int(duration_ms), loop=0)


def depth_to_png(depth, path):
    """(H, W) depth -> grey PNG, black = nearest and white = farthest over the finite values; a pixel that is not
    finite (masked) is white."""
    from PIL import Image
    d = _numpy(depth).astype(np.float64)
    ok = np.isfinite(d)
    out = np.full(d.shape, 255, np.uint8)
    if ok.any():
        lo, hi = d[ok].min(), d[ok].max()
        out[ok] = np.rint((d[ok] - lo) / (hi - lo if hi > lo else 1.0) * 255).astype(np.uint8)
    Image.fromarray(out, mode="L").save(path)


def normal_to_png(normal, path, valid=None):
    """(H, W, 3) unit normals -> RGB PNG, n / 2 + 0.5; pixels outside `valid` (H, W) are white."""
    from PIL import Image
    n = np.rint(np.clip(_numpy(normal).astype(np.float32) / 2 + 0.5, 0.0, 1.0) * 255).astype(np.uint8)
    if valid is not None:
        n[~_numpy(valid).astype(bool)] = 255
    Image.fromarray(n).save(path)


# ------------------------------------------------------------------------------------------------------------- mesh
def fill_masked_depth(depth):
    """(B, H, W) depth with NaN = masked -> (filled, valid): `valid` marks the finite pixels; the others get the
    stand-in documented above, the farthest finite depth of their image.  An image without a finite pixel is an
    error."""
    valid = torch.isfinite(depth)
    if not bool(valid.flatten(1).any(1).all()):
        raise ValueError("a depth map has no finite pixel")
    far = torch.where(valid, depth, torch.full_like(depth, -float("inf"))).flatten(1).max(1).values
    return torch.where(valid, depth, far.view(-1, 1, 1).expand_as(depth)), valid


def valid_faces(valid):
    """(H, W) bool -> (F', 3) int32 on its device: the faces of get_face_idx whose three vertices are valid (one
    host synchronisation, for the size of the result)."""
    from .renderer.utils import get_face_idx
    h, w = valid.shape
    faces = get_face_idx(1, h, w, device=valid.device)[0]
    keep = valid.reshape(-1)[faces.long()].all(1)
    return faces[keep].contiguous()


def depth_mesh(renderer, depth):
    """One (H, W) depth (NaN = masked) -> (verts (n, 3), faces (F', 3), uv (n, 2)) with only the valid vertices, in
    the order of the grid, and the faces between them.  Vertices are `depth_to_3d_grid` points (camera space: x
    right, y down, z forward); uv has u to the right and v up, (0, 0) at the image's bottom-left pixel centre."""
    h, w = depth.shape
    filled, valid = fill_masked_depth(depth[None])
    verts = renderer.depth_to_3d_grid(filled)[0].reshape(-1, 3)
    faces = valid_faces(valid[0]).long()
    flat = valid[0].reshape(-1)
    new_id = torch.cumsum(flat.long(), 0) - 1
    ii, jj = torch.meshgrid(torch.arange(h, device=depth.device), torch.arange(w, device=depth.device), indexing="ij")
    uv = torch.stack([jj.float() / max(w - 1, 1), 1.0 - ii.float() / max(h - 1, 1)], -1).reshape(-1, 2)
    return verts[flat], new_id[faces].int(), uv[flat]


def write_obj(path, verts, faces, uv=None, texture_png=None):
    """Wavefront OBJ with `v`, `vt` and `f` records only (1-based `f a/a b/b c/c`), plus <stem>.mtl and the texture
    when `texture_png` is given: a (C, H, W) image in [-1, 1], written to <stem>.png, or the name of an existing
    image file.  Camera-space vertices are written as (x, -y, -z): y up and the surface facing +z, which is how
    mesh viewers expect an object to stand."""
    v = _numpy(verts).astype(np.float64).reshape(-1, 3) * np.array([1.0, -1.0, -1.0])
    f = _numpy(faces).astype(np.int64).reshape(-1, 3) + 1
    t = None if uv is None else _numpy(uv).astype(np.float64).reshape(-1, 2)
    if f.size and (f.min() < 1 or f.max() > len(v)):
        raise ValueError("write_obj: a face names a vertex that does not exist")
    if t is not None and len(t) != len(v):
        raise ValueError("write_obj: one uv per vertex")
    stem = os.path.splitext(path)[0]
    lines = []
    if texture_png is not None and t is not None:
        if isinstance(texture_png, str):
            image_name = texture_png
        else:
            image_name = os.path.basename(stem) + ".png"
            save_png(texture_png, stem + ".png")
        with open(stem + ".mtl", "w") as m:
            m.write("newmtl surface\nKa 1 1 1\nKd 1 1 1\nKs 0 0 0\nillum 1\nmap_Kd " + image_name + "\n")
        lines += ["mtllib " + os.path.basename(stem) + ".mtl", "usemtl surface"]
    lines += ["v %.7g %.7g %.7g" % tuple(p) for p in v]
    if t is not None:
        lines += ["vt %.7g %.7g" % tuple(p) for p in t]
        lines += ["f %d/%d %d/%d %d/%d" % (a, a, b, b, c, c) for a, b, c in f]
    else:
        lines += ["f %d %d %d" % tuple(p) for p in f]
    with open(path, "w") as o:
        o.write("\n".join(lines) + "\n")


# ---------------------------------------------------------------------------------------------------------- command
def visualize_image(renderer, image, depth, out_dir, stem, modes=MODES, frames=60, relight=False, obj=False,
                    recon_im=None, log=print):
    """Everything the command writes for one image (3, H, W) in [-1, 1] and its depth (H, W), NaN = masked."""
    os.makedirs(out_dir, exist_ok=True)
    image, depth = image.float(), depth.float()
    filled, valid = fill_masked_depth(depth[None])
    faces = None if bool(valid.all()) else valid_faces(valid[0])
    normal = renderer.get_normal_from_depth(filled.contiguous())
    depth_to_png(depth, os.path.join(out_dir, "depth.png"))
    normal_to_png(normal[0], os.path.join(out_dir, "normal.png"), valid[0])
    if recon_im is not None:
        save_png(recon_im.reshape(recon_im.shape[-3:]).clamp(-1, 1), os.path.join(out_dir, "recon.png"))
    rot = turntable_rotations(frames)
    head = torch.tensor([HEADLIGHT]).expand(len(rot), 5)
    for mode in modes:
        seq = renderer.render_sweep(image[None], filled, rot, mode=mode, light=head, normal=normal, faces=faces)
        save_gif(seq[0], os.path.join(out_dir, f"turntable_{mode}.gif"))
    if relight:
        lights = light_circle(2 * frames)
        seq = renderer.render_sweep(image[None], filled, torch.zeros(len(lights), 3), mode="shaded", light=lights,
                                    normal=normal, faces=faces)
        save_gif(seq[0], os.path.join(out_dir, "relight.gif"))
    if obj:
        v, f, uv = depth_mesh(renderer, depth)
        write_obj(os.path.join(out_dir, stem + ".obj"), v, f, uv, image)
    log(f"{stem}: {int(valid.sum())} of {valid.numel()} vertices -> {out_dir}")


def build_parser():
    parser = argparse.ArgumentParser(prog="python -m gan2shape_amd.visualize",
                                     description="Animations, still images and a mesh of the recovered shape")
    parser.add_argument("--config", required=True, help="one yml file with the model's and the dataset's keys")
    source = parser.add_mutually_exclusive_group(required=True)
    source.add_argument("--ckpt", default=None, help="checkpoint file of one net; the others are found beside it")
    source.add_argument("--depth-dir", dest="depth_dir", default=None,
                        help="directory of the <image stem>.npy depths `evaluate` wrote (NaN = masked); no model")
    parser.add_argument("--out", required=True, help="output directory")
    parser.add_argument("--images", type=int, nargs="+", default=None, help="indices into list.txt (default: all)")
    parser.add_argument("--mask", action="store_true", help="with --ckpt: mask the depth with MaskingModel")
    parser.add_argument("--modes", nargs="+", choices=MODES, default=list(MODES))
    parser.add_argument("--relight", action="store_true", help="also write relight.gif")
    parser.add_argument("--frames", type=int, default=60, help="n of turntable_rotations: 2n frames per animation")
    parser.add_argument("--obj", action="store_true", help="also write <stem>.obj, .mtl and .png")
    parser.add_argument("--device", default="cuda")
    return parser


def main(argv=None, model=None, masking_model=None):
    """`model` / `masking_model`: objects to use instead of the ones the config and --ckpt describe, as in
    evaluate.main.  Returns the list of per-image output directories."""
    args = build_parser().parse_args(argv)
    import yaml
    from .dataset import ImageDataset, default_transform
    from .evaluate import _stems, checkpoint_path_of
    with open(args.config) as f:
        config = yaml.safe_load(f)
    device = torch.device(args.device)
    category = config.get("category")
    use_model = args.depth_dir is None
    if use_model and model is None:
        from .model import GAN2Shape
        model = GAN2Shape(config, device=device)
        model.load_from_checkpoint(checkpoint_path_of(args.ckpt))
    if use_model and args.mask and masking_model is None:
        from .parsing import MaskingModel
        masking_model = MaskingModel(category, device=device, ckpt_dir=config["parsing_ckpt_dir"],
                                     size=config.get("parsing_size"))
    if use_model:
        renderer = model.renderer
    else:
        from .renderer import Renderer
        renderer = Renderer(config, config["image_size"], MIN_DEPTH, MAX_DEPTH, device=device)
    dataset = ImageDataset(os.path.join(config["root_path"], category), subset=args.images,
                           transform=default_transform(config["image_size"], config.get("crop"), config.get("origin_size")))
    written = []
    for i, stem in enumerate(_stems(dataset)):
        image = dataset[i].to(device)
        recon_im = None
        if use_model:
            if args.mask:
                recon_im, depth = model.evaluate_results_masked(image[None], masking_model)
            else:
                recon_im, depth = model.evaluate_results(image[None])
            depth = depth.detach().reshape(depth.shape[-2], depth.shape[-1])
        else:
            depth = torch.from_numpy(np.load(os.path.join(args.depth_dir, stem + ".npy")).astype(np.float32)).to(device)
        if tuple(depth.shape) != tuple(image.shape[-2:]):
            raise ValueError(f"{stem}: the depth is {tuple(depth.shape)}, the image {tuple(image.shape[-2:])}")
        out_dir = os.path.join(args.out, stem)
        visualize_image(renderer, image, depth, out_dir, stem, modes=args.modes, frames=args.frames,
                        relight=args.relight, obj=args.obj, recon_im=recon_im)
        written.append(out_dir)
    return written


if __name__ == "__main__":
    main()
