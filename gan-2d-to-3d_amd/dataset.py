"""On-disk layout of a GAN2Shape dataset (behaviour of GAN2Shape/dataset.py:8-79): `root/list.txt`
names the image files, one per line; `root/latents/<stem>.pt` holds each image's StyleGAN2 latent.
Items are `(image in [-1, 1] of shape (3,H,W), latent (512,) or (n_latent, 512), index)`.

Written for this package: `list.txt` is read with the csv module (no pandas); latents are loaded
with `torch.load(weights_only=True)` (tensor or dict-of-tensor files only — nothing is unpickled);
an invalid subset raises `IndexError` instead of exiting the process.  `default_transform` restates
main.py:98-103 (`transforms.Resize(size)` + `ToTensor()`) without torchvision."""
import csv
import os

import numpy as np
import torch
from PIL import Image
from torch.utils.data import Dataset


def default_transform(image_size, crop=None, origin_size=None):
    """PIL image -> float tensor (3,H,W) in [0,1]; the smaller edge is resized to `image_size`
    (bilinear), as torchvision's Resize(int) + ToTensor do.
    With `crop` (config keys `crop` / `origin_size`, the framing of GAN2Shape/model.py:197-200 applied to the input
    image): the smaller edge goes to `origin_size` (default `image_size`), the centre crop x crop window is cut
    (margin (edge - crop) // 2 per axis, as utils.crop) and resized to image_size x image_size (bilinear)."""
    if crop is None:
        edge = image_size
    else:
        edge = image_size if origin_size is None else int(origin_size)
        crop = int(crop)
        if not 0 < crop <= edge:
            raise ValueError(f"crop must satisfy 0 < crop <= origin_size, got crop {crop}, origin_size {edge}")

    def transform(image):
        w, h = image.size
        if w <= h:
            size = (edge, max(1, int(edge * h / w)))
        else:
            size = (max(1, int(edge * w / h)), edge)
        if (w, h) != size:
            image = image.resize(size, Image.BILINEAR)
        if crop is not None:
            left, top = (size[0] - crop) // 2, (size[1] - crop) // 2
            image = image.crop((left, top, left + crop, top + crop))
            if crop != image_size:
                image = image.resize((image_size, image_size), Image.BILINEAR)
        a = np.asarray(image.convert('RGB'), dtype=np.uint8)
        return torch.from_numpy(a.copy()).permute(2, 0, 1).float().div(255)
    return transform


class _ListedFiles(Dataset):
    """The entries of `root/list.txt` (first column), optionally restricted to `subset` indices."""

    def __init__(self, root_dir, list_filename, subset):
        self.root_dir = root_dir
        with open(os.path.join(root_dir, list_filename), newline='') as f:
            names = [row[0] for row in csv.reader(f) if row]
        self.file_list = names if subset is None else [names[i] for i in subset]

    def __len__(self):
        return len(self.file_list)


class ImageDataset(_ListedFiles):
    """Images scaled to [-1, 1] (the transform is expected to produce [0, 1])."""

    def __init__(self, root_dir, list_filename='list.txt', transform=None, subset=None):
        super().__init__(root_dir, list_filename, subset)
        self.transform = transform

    def __getitem__(self, index):
        with Image.open(os.path.join(self.root_dir, self.file_list[index])) as image:
            data = image if self.transform is None else self.transform(image)
            return data * 2 - 1


class LatentDataset(_ListedFiles):
    """`latents/<stem>.pt`: a tensor, {'latent': w}, or {name: {'latent': w}} (dataset.py:50-58)."""

    def __init__(self, root_dir, list_filename='list.txt', latent_folder='latents', subset=None):
        super().__init__(root_dir, list_filename, subset)
        self.latent_folder = latent_folder

    def __getitem__(self, index):
        stem = self.file_list[index].split('.')[0]
        obj = torch.load(os.path.join(self.root_dir, self.latent_folder, stem + '.pt'),
                         map_location='cpu', weights_only=True)
        if isinstance(obj, dict):
            inner = obj if 'latent' in obj else obj.popitem()[1]
            obj = inner['latent']
        latent = obj.detach()
        return latent.squeeze(0) if latent.dim() == 2 else latent   # (1, 512) -> (512,)


class ImageLatentDataset(Dataset):
    """(image, latent, index) triples over the same list."""

    def __init__(self, root_dir, list_filename='list.txt', transform=None, latent_folder='latents',
                 subset=None):
        self.image_dataset = ImageDataset(root_dir, list_filename, transform, subset)
        self.latent_dataset = LatentDataset(root_dir, list_filename, latent_folder, subset)
        assert len(self.image_dataset) == len(self.latent_dataset)

    def __len__(self):
        return len(self.image_dataset)

    def __getitem__(self, index):
        return self.image_dataset[index], self.latent_dataset[index], index


class MultiResolutionDataset(Dataset):
    """stylegan2-pytorch/dataset.py's dataset over what prepare_data.py wrote: `path/<resolution>.npy` (uint8
    [N, 3, S, S]) memory-mapped; an item is `transform(PIL image)`."""

    def __init__(self, path, transform, resolution=256):
        file = os.path.join(path, f"{resolution}.npy")
        if not os.path.exists(file):
            raise IOError(f"Cannot open packed dataset {file}")
        self.data = np.load(file, mmap_mode="r")
        self.resolution = resolution
        self.transform = transform

    def __len__(self):
        return self.data.shape[0]

    def __getitem__(self, index):
        image = Image.fromarray(np.ascontiguousarray(self.data[index].transpose(1, 2, 0)))
        return self.transform(image)


def is_packed(path, resolution):
    """Whether `path` holds the packed array of this resolution (prepare_data.py)."""
    return os.path.exists(os.path.join(path, f"{resolution}.npy"))


class DeviceBatches:
    """Endless iterator of float32 batches [batch, 3, S, S] in [-1, 1] on `device` from `path/<resolution>.npy`.

    It makes the draws of dtrain.real_batches from `generator` (a CPU generator) in the same sequence — one randperm
    per pass, extended while shorter than the batch, and one torch.rand(()) per image in batch order — so for equal
    seeds its batches are real_batches' bit for bit when the source images already have the target size.

    On a CUDA device a batch is one g2s_u8_batch launch on the current stream, which reads the sampled indices and the
    flip flags from device memory.  If the array fits `max_resident_bytes` it is uploaded once; otherwise the rows of
    a batch are gathered from the memory map into a pinned buffer, copied, and converted by the same kernel with
    idx = arange.  On a CPU device the torch expression of dataset.ImageDataset runs."""

    def __init__(self, path, resolution, batch, generator, device, max_resident_bytes=8 << 30):
        file = os.path.join(path, f"{resolution}.npy")
        self.data = np.load(file, mmap_mode="r")
        if self.data.dtype != np.uint8 or self.data.ndim != 4 or self.data.shape[1:] != (3, resolution, resolution):
            raise ValueError(f"{file}: expected uint8 [N, 3, {resolution}, {resolution}]")
        if len(self.data) == 0:
            raise ValueError(f"{file}: the dataset is empty")
        self.size, self.batch, self.generator = resolution, batch, generator
        self.device = torch.device(device)
        self.resident = None
        if self.device.type == "cuda":
            if self.data.nbytes <= max_resident_bytes:
                self.resident = torch.empty(self.data.shape, dtype=torch.uint8, device=self.device)
                step = max(1, (256 << 20) // max(1, self.data[0].nbytes))      # upload in slices of about 256 MB
                for lo in range(0, len(self.data), step):
                    self.resident[lo:lo + step] = torch.from_numpy(np.array(self.data[lo:lo + step]))
            else:       # two pinned buffers: one is filled while the copy out of the other may still run
                shape = (batch, 3, resolution, resolution)
                self._pinned = [torch.empty(shape, dtype=torch.uint8).pin_memory() for _ in range(2)]
                self._copied = [None, None]
                self._arange = torch.arange(batch, device=self.device)
                self._turn = 0
        self._draws = self._draw()

    def _draw(self):
        n, batch, generator = len(self.data), self.batch, self.generator
        while True:
            order = torch.randperm(n, generator=generator).tolist()
            while len(order) < batch:
                order += torch.randperm(n, generator=generator).tolist()
            for lo in range(0, len(order) - batch + 1, batch):
                idx = order[lo:lo + batch]
                yield idx, [torch.rand((), generator=generator).item() < 0.5 for _ in idx]

    def __iter__(self):
        return self

    def __next__(self):
        idx, flip = next(self._draws)
        if self.device.type != "cuda":
            rows = torch.from_numpy(self.data[idx])       # fancy indexing: a copy
            out = rows.float().div(255) * 2 - 1
            for b, f in enumerate(flip):
                if f:
                    out[b] = out[b].flip(2)
            return out.to(self.device)
        from . import lib
        B, S = self.batch, self.size
        with torch.cuda.device(self.device):
            # indices (int64) and flags (u8) cross in one copy
            draws = torch.cat([torch.tensor(idx, dtype=torch.int64).view(torch.uint8),
                               torch.tensor(flip, dtype=torch.uint8)]).to(self.device)
            index, flips = draws[:8 * B].view(torch.int64), draws[8 * B:]
            if self.resident is not None:
                data, n = self.resident, len(self.data)
            else:
                t = self._turn
                self._turn = 1 - t
                if self._copied[t] is not None:
                    self._copied[t].synchronize()
                np.take(self.data, idx, axis=0, out=self._pinned[t].numpy())
                data, n, index = self._pinned[t].to(self.device, non_blocking=True), B, self._arange
                self._copied[t] = torch.cuda.Event()
                self._copied[t].record()
            out = torch.empty((B, 3, S, S), dtype=torch.float32, device=self.device)
            lib.check(lib.load().g2s_u8_batch(lib.ptr(data), n, lib.ptr(index), lib.ptr(flips), lib.ptr(out), B, S,
                                              lib.stream()))
        return out
