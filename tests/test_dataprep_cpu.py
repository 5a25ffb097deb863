"""The data path without a GPU: the coefficient tables and the integer passes against Pillow, the crop geometry, the
prepare command, both datasets, and the two new symbols of the C ABI.  Every comparison is exact."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch
from PIL import Image

import gan2shape_amd  # noqa: F401
from gan2shape_amd import dataset, dtrain, lib, prepare_data

import dataprep_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PIL_FILTER = {"lanczos": Image.LANCZOS, "bilinear": Image.BILINEAR}


def pil_resize(images, oh, ow, resample):
    """[N, H, W, 3] -> planar [N, 3, oh, ow] through PIL.Image.resize."""
    out = [np.asarray(Image.fromarray(a).resize((ow, oh), PIL_FILTER[resample])) for a in images]
    return np.stack(out).transpose(0, 3, 1, 2)


@pytest.mark.parametrize("resample", cases.FILTERS)
@pytest.mark.parametrize("name,make,out", cases.resize_cases(), ids=[c[0] for c in cases.resize_cases()])
def test_cpu_route_equals_pillow(name, make, out, resample):
    images = make(2)
    got = prepare_data.resize(torch.from_numpy(images), out[0], out[1], resample).numpy()
    ref = pil_resize(images, out[0], out[1], resample)
    assert got.shape == ref.shape and got.dtype == np.uint8
    assert np.array_equal(got, ref), f"{int((got != ref).sum())} bytes differ"


def test_checkerboard_hits_both_clips():
    """The Lanczos accumulator leaves 0..255 on both sides on the checkerboard: both clips are exercised."""
    (H, W), (oh, ow) = cases.CHECKER_SIZES[2]
    images = cases.checkerboard(1, H, W)
    kx, bx = prepare_data.resample_coeffs(W, ow, "lanczos")
    row = images[0, :, :, 0].astype(np.int64)
    acc = np.array([[(row[y, bx[x, 0]:bx[x, 0] + bx[x, 1]] * kx[x, :bx[x, 1]]).sum() + (1 << 21) for x in range(ow)]
                    for y in range(H)]) >> 22
    assert acc.min() < 0 and acc.max() > 255


def test_coefficient_tables():
    kk, bounds = prepare_data.resample_coeffs(1024, 128, "lanczos")
    assert kk.dtype == np.int32 and bounds.dtype == np.int32
    assert kk.shape == (128, 49) and bounds.shape == (128, 2)       # 2 * ceil(3 * 8) + 1 taps
    assert (bounds[:, 0] >= 0).all() and (bounds[:, 0] + bounds[:, 1] <= 1024).all()
    assert (np.abs(kk.sum(1) - (1 << 22)) <= 49).all()               # rows sum to one, up to the rounding of each tap
    for i in range(128):
        assert not kk[i, bounds[i, 1]:].any()
    kk, bounds = prepare_data.resample_coeffs(16, 16, "bilinear")
    assert kk.shape == (16, 3)
    with pytest.raises(KeyError):
        prepare_data.resample_coeffs(16, 8, "bicubic")


@pytest.mark.parametrize("resample", cases.FILTERS)
@pytest.mark.parametrize("hw,size", cases.CROP_CASES)
def test_resize_and_crop_equals_pillow_resize_then_crop(hw, size, resample):
    H, W = hw
    images = cases.random_images(2, H, W, seed=H + W)
    if W <= H:
        ow, oh = size, int(size * H / W)
    else:
        oh, ow = size, int(size * W / H)
    top, left = int(round((oh - size) / 2.0)), int(round((ow - size) / 2.0))
    assert prepare_data.output_geometry(H, W, size) == (oh, ow, left, top)
    ref = pil_resize(images, oh, ow, resample)[:, :, top:top + size, left:left + size]
    got = prepare_data.resize_and_crop(torch.from_numpy(images), size, resample)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (2, 3, size, size) and got.is_contiguous()
    assert np.array_equal(got.numpy(), ref)


def write_folder(root, sizes, seed=0, listed=False):
    """PNG files of the given (H, W) in two sub-folders (or flat with list.txt); returns {relative name: array}."""
    rng = np.random.default_rng(seed)
    files = {}
    for i, (H, W) in enumerate(sizes):
        name = f"{i:02d}.png" if listed else os.path.join("b" if i % 2 else "a", f"{len(sizes) - i:02d}.png")
        os.makedirs(os.path.dirname(os.path.join(root, name)), exist_ok=True)
        a = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        Image.fromarray(a).save(os.path.join(root, name))
        files[name] = a
    if listed:
        with open(os.path.join(root, "list.txt"), "w") as f:
            f.writelines(n + "\n" for n in files)
    return files


@pytest.fixture(scope="module")
def prepared(tmp_path_factory):
    src = str(tmp_path_factory.mktemp("images"))
    out = str(tmp_path_factory.mktemp("packed"))
    files = write_folder(src, [(20, 31), (16, 16), (20, 31), (33, 18), (8, 8), (16, 16)])
    assert prepare_data.main(["--out", out, "--size", "8,16", "--device", "cpu", "--n-worker", "2", src]) == out
    return src, out, files


def test_prepare_command_writes_arrays_and_list(prepared):
    src, out, files = prepared
    names = open(os.path.join(out, "list.txt")).read().split()
    assert names == sorted(files)                # a/.. before b/.., names sorted within each: ImageFolder's order
    for size in (8, 16):
        a = np.load(os.path.join(out, f"{size}.npy"))
        assert a.dtype == np.uint8 and a.shape == (6, 3, size, size)
        for i, name in enumerate(names):
            ref = prepare_data.resize_and_crop(torch.from_numpy(files[name][None]), size)[0].numpy()
            assert np.array_equal(a[i], ref), (size, name)
    a = np.load(os.path.join(out, "16.npy"))        # an image already at size is stored untouched
    i = names.index(next(n for n in names if files[n].shape[:2] == (16, 16)))
    assert np.array_equal(a[i], files[names[i]].transpose(2, 0, 1))


def test_prepare_command_reads_a_listed_folder(tmp_path):
    src, out = str(tmp_path / "src"), str(tmp_path / "out")
    os.makedirs(src)
    files = write_folder(src, [(8, 8), (9, 12), (8, 8)], listed=True)
    prepare_data.main(["--out", out, "--size", "8", "--device", "cpu", src])
    assert open(os.path.join(out, "list.txt")).read().split() == list(files)
    assert np.load(os.path.join(out, "8.npy")).shape == (3, 3, 8, 8)


def test_multi_resolution_dataset_returns_the_prepared_images(prepared):
    _, out, _ = prepared
    a = np.load(os.path.join(out, "16.npy"))
    data = dataset.MultiResolutionDataset(out, lambda image: image, resolution=16)
    assert len(data) == 6
    for i in range(6):
        image = data[i]
        assert isinstance(image, Image.Image) and image.size == (16, 16) and image.mode == "RGB"
        assert np.array_equal(np.asarray(image), a[i].transpose(1, 2, 0))
    t = dataset.MultiResolutionDataset(out, dataset.default_transform(8), resolution=8)[2]
    assert t.shape == (3, 8, 8) and t.dtype == torch.float32
    with pytest.raises(IOError):
        dataset.MultiResolutionDataset(out, None, resolution=32)


@pytest.fixture(scope="module")
def small_set(tmp_path_factory):
    """N = 5 images of 8 x 8, as a list.txt folder and packed: with batch = 4 a pass has one batch and drops an image,
    with batch = 7 a pass needs a second permutation."""
    src = str(tmp_path_factory.mktemp("small"))
    out = str(tmp_path_factory.mktemp("small_packed"))
    write_folder(src, [(8, 8)] * 5, seed=3, listed=True)
    prepare_data.prepare(src, out, sizes=(8,), device="cpu")
    return src, out


@pytest.mark.parametrize("batch", [4, 7])
def test_device_batches_on_cpu_equal_real_batches(small_set, batch):
    src, out = small_set
    old = dtrain.real_batches(src, 8, batch, torch.Generator().manual_seed(11))
    new = dataset.DeviceBatches(out, 8, batch, torch.Generator().manual_seed(11), "cpu")
    staged = dataset.DeviceBatches(out, 8, batch, torch.Generator().manual_seed(11), "cpu", max_resident_bytes=0)
    seen = set()
    for _ in range(6):                      # several passes
        a, b = next(old), next(new)
        assert b.dtype == torch.float32 and tuple(b.shape) == (batch, 3, 8, 8)
        assert torch.equal(a, b) and torch.equal(a, next(staged))
        seen.add(a.numpy().tobytes())
    assert len(seen) > 1


def test_batches_chooses_the_route_by_the_folder(small_set):
    src, out = small_set
    g = torch.Generator().manual_seed(0)
    assert isinstance(dtrain.batches(out, 8, 4, g, torch.device("cpu")), dataset.DeviceBatches)
    assert not isinstance(dtrain.batches(src, 8, 4, g, torch.device("cpu")), dataset.DeviceBatches)
    assert not isinstance(dtrain.batches(out, 16, 4, g, torch.device("cpu")), dataset.DeviceBatches)  # no 16.npy


def test_table_of_the_batch_kernel_is_the_torch_expression():
    """The arithmetic that csrc/dataprep.hip's table states (IEEE f32: v / 255, * 2, - 1) gives torch's bits."""
    v = np.arange(256, dtype=np.float32)
    table = v / np.float32(255) * np.float32(2) - np.float32(1)
    ref = torch.arange(256, dtype=torch.uint8).float().div(255) * 2 - 1
    assert np.array_equal(table, ref.numpy())


def test_new_symbols_declared_and_validated():
    header = open(os.path.join(ROOT, "include", "g2s.h")).read()
    declared = set(re.findall(r"\b(g2s_[a-z0-9_]+)\s*\(", header))
    assert {"g2s_u8_batch", "g2s_resize_u8"} <= declared and {"g2s_u8_batch", "g2s_resize_u8"} <= set(lib.SIGNATURES)
    assert "#define G2S_ABI_VERSION 1" in header
    L = lib.load()
    assert L.g2s_abi_version() == 1
    buf = (C.c_uint8 * 64)()        # stands in for device memory: every call below is refused before a launch
    p = C.cast(buf, C.c_void_p)
    assert L.g2s_u8_batch(None, 1, p, p, p, 1, 8, None) == -1 and b"NULL" in L.g2s_last_error()
    assert L.g2s_u8_batch(p, 1, None, p, p, 1, 8, None) == -1
    assert L.g2s_u8_batch(p, 1, p, None, p, 1, 8, None) == -1
    assert L.g2s_u8_batch(p, 1, p, p, None, 1, 8, None) == -1
    for N, B, S in ((0, 1, 8), (1, 0, 8), (1, 1, 0), (1, -1, 8)):
        assert L.g2s_u8_batch(p, N, p, p, p, B, S, None) == -1

    def resize(src=p, dst=p, tmp=p, N=1, H=8, W=8, oh=4, ow=4, kx=p, bx=p, ksx=3, ky=p, by=p, ksy=3, left=0, top=0,
               ow_c=4, oh_c=4, row0=0, rows=8):
        return L.g2s_resize_u8(src, dst, tmp, N, H, W, oh, ow, kx, bx, ksx, ky, by, ksy, left, top, ow_c, oh_c, row0,
                               rows, None)
    assert resize(src=None) == -1 and b"NULL" in L.g2s_last_error()
    assert resize(dst=None) == -1
    assert resize(tmp=None) == -1               # both passes run
    assert resize(kx=None) == -1 and resize(by=None) == -1
    for kw in ({"N": 0}, {"H": 0}, {"W": -1}, {"oh": 0}, {"ow": 0}, {"ow_c": 0}, {"oh_c": 0}, {"ksx": 0},
               {"left": 1}, {"top": -1}, {"rows": 9}, {"row0": -1}, {"rows": 0}):
        assert resize(**kw) == -1, kw
