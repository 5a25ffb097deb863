"""csrc/dataprep.hip on the GPU: g2s_resize_u8 against the numpy statement of the same integer passes (which
test_dataprep_cpu.py pins to Pillow), g2s_u8_batch against the torch expression of dataset.ImageDataset,
DeviceBatches against its CPU twin, and train.main on a packed folder.  Every comparison is exact."""
import os
import re

import numpy as np
import pytest
import torch

import gan2shape_amd  # noqa: F401
from gan2shape_amd import dataset, lib, prepare_data, train

import dataprep_cases as cases

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("resample", cases.FILTERS)
@pytest.mark.parametrize("name,make,out", cases.resize_cases(), ids=[c[0] for c in cases.resize_cases()])
def test_resize_equals_the_cpu_route(name, make, out, resample):
    for n in (1, 3):
        images = torch.from_numpy(make(n))
        ref = prepare_data.resize(images, out[0], out[1], resample)
        got = prepare_data.resize(images.cuda(), out[0], out[1], resample)
        assert got.is_cuda and got.dtype == torch.uint8 and got.shape == ref.shape
        assert torch.equal(got.cpu(), ref), f"{name} n={n}: {int((got.cpu() != ref).sum())} bytes differ"


@pytest.mark.parametrize("resample", cases.FILTERS)
@pytest.mark.parametrize("hw,size", cases.CROP_CASES)
def test_resize_and_crop_equals_the_cpu_route(hw, size, resample):
    images = torch.from_numpy(np.concatenate([cases.random_images(2, hw[0], hw[1], seed=sum(hw)),
                                              cases.checkerboard(1, hw[0], hw[1])]))
    ref = prepare_data.resize_and_crop(images, size, resample)
    got = prepare_data.resize_and_crop(images.cuda(), size, resample)
    assert tuple(got.shape) == (3, 3, size, size)
    assert torch.equal(got.cpu(), ref)


def torch_batch(data, idx, flip):
    rows = torch.from_numpy(data)[idx].float().div(255) * 2 - 1
    return torch.stack([r.flip(2) if f else r for r, f in zip(rows, flip)])


def run_u8_batch(data, n, idx, flip, S):
    out = torch.full((len(idx), 3, S, S), float("nan"), device="cuda")
    index = torch.tensor(idx, dtype=torch.int64, device="cuda")
    flips = torch.tensor(flip, dtype=torch.uint8, device="cuda")
    lib.check(lib.load().g2s_u8_batch(lib.ptr(data), n, lib.ptr(index), lib.ptr(flips), lib.ptr(out), len(idx), S,
                                      lib.stream()))
    return out.cpu()


@pytest.mark.parametrize("S,N,idx,flip", cases.BATCH_CASES)
def test_u8_batch_equals_the_torch_expression(S, N, idx, flip):
    data = cases.packed_dataset(N, S, seed=S + N)
    ref = torch_batch(data, idx, flip)
    assert torch.equal(run_u8_batch(torch.from_numpy(data).cuda(), N, idx, flip, S), ref)


@pytest.mark.parametrize("S", [64, 16])
def test_u8_batch_with_an_unaligned_base(S):
    """A data pointer one row past an aligned one (S = 64: still 16-byte aligned, the wide kernel) and one byte past
    it (the scalar kernel) read the right bytes."""
    N, idx, flip = 4, [3, 0, 1, 1, 3], [1, 0, 1, 0, 0]
    data = cases.packed_dataset(N, S, seed=7)
    for shift in (S, 1, S + 4):
        buf = torch.zeros(shift + data.size, dtype=torch.uint8, device="cuda")
        view = buf[shift:]
        view.copy_(torch.from_numpy(data).reshape(-1))
        assert view.data_ptr() % 16 == shift % 16
        assert torch.equal(run_u8_batch(view, N, idx, flip, S), torch_batch(data, idx, flip)), shift


def test_u8_batch_every_byte_value():
    """All 256 table entries, through both kernels."""
    for S in (16, 10):
        data = (np.arange(2 * 3 * S * S) % 256).astype(np.uint8).reshape(2, 3, S, S)
        assert torch.equal(run_u8_batch(torch.from_numpy(data).cuda(), 2, [1, 0], [0, 1], S),
                           torch_batch(data, [1, 0], [0, 1]))


def test_u8_batch_index_outside_the_dataset_reads_nothing():
    data = cases.packed_dataset(2, 16)
    out = run_u8_batch(torch.from_numpy(data).cuda(), 2, [1, 2, -1], [0, 0, 1], 16)
    assert torch.equal(out[0], torch_batch(data, [1], [0])[0]) and out[1:].isnan().all()


@pytest.fixture(scope="module")
def packed(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("packed"))
    for S, N in ((16, 5), (8, 5)):
        np.save(os.path.join(out, f"{S}.npy"), cases.packed_dataset(N, S, seed=S))
    return out


@pytest.mark.parametrize("S,batch", [(16, 4), (8, 7)])
def test_device_batches_equal_their_cpu_twin(packed, S, batch):
    twin = dataset.DeviceBatches(packed, S, batch, torch.Generator().manual_seed(5), "cpu")
    resident = dataset.DeviceBatches(packed, S, batch, torch.Generator().manual_seed(5), "cuda")
    staged = dataset.DeviceBatches(packed, S, batch, torch.Generator().manual_seed(5), "cuda", max_resident_bytes=0)
    assert resident.resident is not None and staged.resident is None
    for _ in range(5):
        ref, a, b = next(twin), next(resident), next(staged)
        assert a.is_cuda and b.is_cuda and a.dtype == torch.float32
        assert torch.equal(a.cpu(), ref) and torch.equal(b.cpu(), ref)


def test_train_runs_on_a_packed_folder(packed, tmp_path, capsys):
    out = str(tmp_path / "train.pt")
    train.main(["--size", "8", "--channel-multiplier", "1", "--data", packed, "--iter", "2", "--batch", "4",
                "--log-every", "1", "--out", out])
    ckpt = torch.load(out, map_location="cpu", weights_only=True)
    assert set(ckpt) == set(train.CHECKPOINT_KEYS)
    lines = [line for line in capsys.readouterr().out.splitlines() if line[:1].isdigit()]
    assert len(lines) == 2
    for line in lines:      # "i: d .. g .. r1 .. path .. mean path .. augment .." (main also raises on a non-finite loss)
        assert "nan" not in line and "inf" not in line
        values = [float(v) for v in re.findall(r"-?\d+\.\d+", line)]
        assert len(values) == 6 and all(np.isfinite(values))
