"""stylegan2-pytorch/prepare_data.py for this package: resize every image of a folder once (Lanczos, smaller edge to
`size`, centre crop) and store one packed uint8 array per resolution, which `dataset.DeviceBatches` keeps in device
memory and `dataset.MultiResolutionDataset` serves as PIL images.

    python -m gan2shape_amd.prepare_data --out DIR [--size 128,256] [--resample lanczos|bilinear] \
        [--device cuda|cpu] [--n-worker 8] PATH

PATH is an image folder (walked recursively, in torchvision ImageFolder's order) or a folder with `list.txt`.  Written
are `DIR/<size>.npy` (uint8 [N, 3, size, size], planar: the layout g2s_u8_batch reads) and `DIR/list.txt` (the source
names in order).  The reference stores a JPEG re-encode (quality 100) of every resized image in LMDB; here the raw
bytes of the resize are stored: no second lossy step, and no decoder between the file and the kernel.

The resize is Pillow's 8-bit resampler (ImagingResample) restated: `resample_coeffs` builds its fixed-point tables on
the host, `g2s_resize_u8` (csrc/dataprep.hip) runs the two integer passes on the device, and the numpy statement of the
same passes serves CPU tensors and the tests."""
import argparse
import math
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

PRECISION_BITS = 32 - 8 - 2
IMG_EXTENSIONS = (".jpg", ".jpeg", ".png", ".ppm", ".bmp", ".pgm", ".tif", ".tiff", ".webp")


def _bilinear(x):
    x = abs(x)
    return 1.0 - x if x < 1.0 else 0.0


def _sinc(x):
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x          # math.sin: the libm that rounds Pillow's sines


def _lanczos(x):
    return _sinc(x) * _sinc(x / 3) if -3.0 <= x < 3.0 else 0.0


FILTERS = {"lanczos": (_lanczos, 3.0), "bilinear": (_bilinear, 1.0)}


def resample_coeffs(in_size, out_size, resample="lanczos"):
    """Pillow's precompute_coeffs + normalize_coeffs_8bpc (libImaging/Resample.c) in Python floats:
    (kk int32 [out_size, ksize], bounds int32 [out_size, 2]); bounds[i] = (first tap, tap count) and
    kk[i, :count] the coefficients in 22-bit fixed point, zero beyond."""
    filt, support = FILTERS[resample]
    scale = float(in_size) / out_size
    filterscale = max(scale, 1.0)
    support = support * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    kk = np.zeros((out_size, ksize), np.int32)
    bounds = np.zeros((out_size, 2), np.int32)
    ss = 1.0 / filterscale
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        k = [filt((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for w in k:
            ww += w
        if ww != 0.0:
            k = [w / ww for w in k]
        q = [int(-0.5 + w * (1 << PRECISION_BITS)) if w < 0 else int(0.5 + w * (1 << PRECISION_BITS)) for w in k]
        # the int32 accumulator of a pass starts at 1 << 21 and adds at most 255 * |k| per tap
        assert 255 * sum(abs(v) for v in q) + 2 ** 21 < 2 ** 31, (in_size, out_size, xx)
        kk[xx, :xmax] = q
        bounds[xx] = (xmin, xmax)
    return kk, bounds


def _pass_numpy(a, axis, kk, bounds, lo, n):
    """One integer pass along `axis` of a (u8): outputs lo .. lo + n."""
    shape = list(a.shape)
    shape[axis] = n
    out = np.empty(shape, np.uint8)
    src = np.moveaxis(a, axis, -1)
    dst = np.moveaxis(out, axis, -1)
    for i in range(n):
        first, count = bounds[lo + i]
        acc = (src[..., first:first + count].astype(np.int32) * kk[lo + i, :count]).sum(-1, dtype=np.int32)
        dst[..., i] = np.clip((acc + (1 << (PRECISION_BITS - 1))) >> PRECISION_BITS, 0, 255)
    return out


def _resize_plan(H, W, oh, ow, window, resample):
    left, top, ow_c, oh_c = (0, 0, ow, oh) if window is None else window
    if not (0 <= left and 0 <= top and 0 < ow_c and 0 < oh_c and left + ow_c <= ow and top + oh_c <= oh):
        raise ValueError(f"window {window} outside the {oh} x {ow} output")
    tx = resample_coeffs(W, ow, resample) if ow != W else None
    ty = resample_coeffs(H, oh, resample) if oh != H else None
    if ty is None:
        row0, rows = top, oh_c
    else:       # the source rows that the vertical windows of the crop touch
        b = ty[1][top:top + oh_c]
        row0 = int(b[:, 0].min())
        rows = int((b[:, 0] + b[:, 1]).max()) - row0
    return (left, top, ow_c, oh_c), tx, ty, row0, rows


def resize(images, oh, ow, resample="lanczos", window=None):
    """`PIL.Image.resize((ow, oh), resample)` of every image of a uint8 [N, H, W, 3] tensor, byte for byte, as planar
    uint8 [N, 3, oh_c, ow_c]; `window` = (left, top, ow_c, oh_c) keeps that part of the output (only it is computed).
    CUDA tensors run g2s_resize_u8, CPU tensors the numpy statement of the same passes."""
    if images.dtype != torch.uint8 or images.dim() != 4 or images.shape[3] != 3:
        raise ValueError("images: uint8 [N, H, W, 3]")
    N, H, W = (int(v) for v in images.shape[:3])
    (left, top, ow_c, oh_c), tx, ty, row0, rows = _resize_plan(H, W, oh, ow, window, resample)
    if not images.is_cuda:
        a = images.numpy()[:, row0:row0 + rows]
        a = _pass_numpy(a, 2, tx[0], tx[1], left, ow_c) if tx else a[:, :, left:left + ow_c]
        if ty:
            a = _pass_numpy(a, 1, ty[0], ty[1] - np.array([row0, 0], np.int32), top, oh_c)
        return torch.from_numpy(np.ascontiguousarray(a.transpose(0, 3, 1, 2)))
    from . import lib
    L = lib.load()
    images = images.contiguous()
    dev = images.device
    out = torch.empty((N, 3, oh_c, ow_c), dtype=torch.uint8, device=dev)
    tabs = [None if t is None else (torch.from_numpy(t[0]).to(dev), torch.from_numpy(t[1]).to(dev)) for t in (tx, ty)]
    tmp = torch.empty((N, 3, rows, ow_c), dtype=torch.uint8, device=dev) if tx and ty else None
    kx, bx = tabs[0] or (None, None)
    ky, by = tabs[1] or (None, None)
    with torch.cuda.device(dev):
        lib.check(L.g2s_resize_u8(lib.ptr(images), lib.ptr(out), lib.ptr(tmp), N, H, W, oh, ow,
                                  lib.ptr(kx), lib.ptr(bx), 0 if kx is None else kx.shape[1],
                                  lib.ptr(ky), lib.ptr(by), 0 if ky is None else ky.shape[1],
                                  left, top, ow_c, oh_c, row0, rows, lib.stream()))
    return out


def output_geometry(H, W, size):
    """(oh, ow, left, top) of torchvision's Resize(size) then CenterCrop(size), the reference's resize_and_convert:
    the smaller edge goes to `size`, the other to int(size * long / short); the crop offset is
    int(round((extent - size) / 2.0))."""
    if W <= H:
        ow, oh = size, int(size * H / W)
    else:
        oh, ow = size, int(size * W / H)
    return oh, ow, int(round((ow - size) / 2.0)), int(round((oh - size) / 2.0))


def resize_and_crop(images_u8, size, resample="lanczos"):
    """uint8 [N, H, W, 3] -> uint8 [N, 3, size, size]: resize the smaller edge to `size`, centre crop."""
    oh, ow, left, top = output_geometry(int(images_u8.shape[1]), int(images_u8.shape[2]), size)
    return resize(images_u8, oh, ow, resample, (left, top, size, size))


def list_images(path):
    """Relative names of the images under `path`: the lines of `list.txt` if there is one, else every image file in
    ImageFolder's order (sub-folders sorted, each walked in sorted order, names sorted); files of `path` itself first."""
    listing = os.path.join(path, "list.txt")
    if os.path.exists(listing):
        from .dataset import _ListedFiles
        return _ListedFiles(path, "list.txt", None).file_list
    names = sorted(f for f in os.listdir(path)
                   if os.path.isfile(os.path.join(path, f)) and f.lower().endswith(IMG_EXTENSIONS))
    for d in sorted(e.name for e in os.scandir(path) if e.is_dir()):
        for root, _, files in sorted(os.walk(os.path.join(path, d), followlinks=True)):
            names += [os.path.relpath(os.path.join(root, f), path) for f in sorted(files)
                      if f.lower().endswith(IMG_EXTENSIONS)]
    return names


def _decode(file):
    from PIL import Image
    with Image.open(file) as image:
        return np.asarray(image.convert("RGB"), dtype=np.uint8)


def prepare(path, out, sizes=(128,), resample="lanczos", device="cpu", n_worker=8, chunk=64):
    """Writes out/<size>.npy for every size and out/list.txt; returns the number of images."""
    from numpy.lib.format import open_memmap
    names = list_images(path)
    if not names:
        raise ValueError(f"{path}: no images")
    os.makedirs(out, exist_ok=True)
    device = torch.device(device)
    packed = {s: open_memmap(os.path.join(out, f"{s}.npy"), mode="w+", dtype=np.uint8, shape=(len(names), 3, s, s))
              for s in sizes}
    with ThreadPoolExecutor(max_workers=max(1, n_worker)) as pool:
        for lo in range(0, len(names), chunk):
            decoded = list(pool.map(_decode, [os.path.join(path, n) for n in names[lo:lo + chunk]]))
            groups = {}                     # images of one size go through the kernel together
            for j, a in enumerate(decoded):
                groups.setdefault(a.shape[:2], []).append(j)
            for (H, W), members in groups.items():
                if min(H, W) < 1:
                    raise ValueError(f"{names[lo + members[0]]}: empty image")
                batch = torch.from_numpy(np.stack([decoded[j] for j in members])).to(device)
                for s in sizes:
                    packed[s][[lo + j for j in members]] = resize_and_crop(batch, s, resample).cpu().numpy()
    for m in packed.values():
        m.flush()
    with open(os.path.join(out, "list.txt"), "w") as f:
        f.writelines(n + "\n" for n in names)
    return len(names)


def build_parser():
    parser = argparse.ArgumentParser(prog="python -m gan2shape_amd.prepare_data",
                                     description="Resize an image folder once into packed uint8 arrays")
    parser.add_argument("--out", required=True, help="folder for <size>.npy and list.txt")
    parser.add_argument("--size", default="128,256,512,1024", help="comma-separated resolutions")
    parser.add_argument("--resample", choices=sorted(FILTERS), default="lanczos")
    parser.add_argument("--device", default="cuda")
    parser.add_argument("--n-worker", dest="n_worker", type=int, default=8, help="decoder threads")
    parser.add_argument("path")
    return parser


def main(argv=None):
    args = build_parser().parse_args(argv)
    sizes = tuple(int(s) for s in args.size.split(",") if s.strip())
    n = prepare(args.path, args.out, sizes, args.resample, args.device, args.n_worker)
    print(f"{n} images -> {args.out} at {', '.join(str(s) for s in sizes)}")
    return args.out


if __name__ == "__main__":
    main()
