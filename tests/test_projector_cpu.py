"""-m "not gpu": the latent projector's host side — the torch path of the noise functions and get_lr against the
reference's results (tests/golden/projector.npz), the file it writes against the dataset classes, the argument checks
of its C entries, and the loop itself on CPU tensors (layer loop + torch noise functions)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import gan2shape_amd  # noqa: F401
from gan2shape_amd import dataset, lib, projector
from gan2shape_amd import stylegan2 as sg2

import projector_cases as pc


@pytest.fixture(scope="module")
def fx(golden):
    return golden("projector")


def test_get_lr_equals_the_reference(fx):
    assert [projector.get_lr(t, 0.1) for t in pc.LR_T] == list(fx["get_lr.lr"])
    assert [projector.get_lr(t, 0.05, rampdown=0.5, rampup=0.1) for t in pc.LR_T] == list(fx["get_lr.lr_ramps"])
    assert projector.get_lr(0.0, 0.1) == 0.0 and abs(projector.get_lr(0.5, 0.1) - 0.1) < 1e-15


@pytest.mark.parametrize("lst,B,kind", pc.CASES)
def test_torch_noise_functions_equal_the_reference_in_float64(fx, lst, B, kind):
    name = pc.case_name(lst, B, kind)
    maps = [torch.from_numpy(m).double() for m in pc.make_maps(pc.SIDE_LISTS[lst], B, kind)]
    for own in (projector.noise_regularize, pc.noise_regularize):       # the package's CPU path, the tests' restatement
        xs = [m.clone().requires_grad_(True) for m in maps]
        v = own(xs)
        grads = torch.autograd.grad(v, xs)
        assert abs(float(v.detach()) - float(fx[f"{name}.value"])) <= 1e-12 * abs(float(fx[f"{name}.value"]))
        for i, g in enumerate(grads):
            ref = torch.from_numpy(fx[f"{name}.grad{i}"])
            assert float((g - ref).abs().max()) <= 1e-12 * float(ref.abs().max()), (name, i)
    for own in (projector.noise_normalize_, pc.noise_normalize_):
        xs = [m.clone().requires_grad_(True) for m in maps]
        own(xs)
        for i, x in enumerate(xs):
            assert float((x.detach() - torch.from_numpy(fx[f"{name}.norm{i}"])).abs().max()) <= 1e-12, (name, i)


def test_latent_noise_and_make_image():
    g = torch.Generator().manual_seed(3)
    w = torch.zeros(1, 512)
    j = projector.latent_noise(w, 0.5, g)
    assert j.shape == w.shape and 0.4 < float(j.std()) < 0.6
    assert torch.equal(projector.latent_noise(w, 0.0), w)
    x = torch.tensor([-2.0, -1.0, 0.0, 1.0, 3.0]).view(1, 1, 1, 5).expand(1, 3, 1, 5)
    im = projector.make_image(x)
    assert im.shape == (1, 1, 5, 3) and im.dtype == np.uint8 and list(im[0, 0, :, 0]) == [0, 0, 127, 255, 255]
    assert float(x.min()) == -2.0          # the argument is left alone


@pytest.mark.parametrize("w_plus", [False, True])
def test_save_projection_round_trips_through_the_dataset(tmp_path, w_plus):
    from PIL import Image
    root = str(tmp_path)
    Image.fromarray(np.full((16, 16, 3), 128, np.uint8)).save(os.path.join(root, "face.01.png"))
    with open(os.path.join(root, "list.txt"), "w") as f:
        f.write("face.01.png\n")
    latent = torch.randn(6, 512) if w_plus else torch.randn(512)
    result = {"img": torch.randn(1, 3, 16, 16), "latent": latent.clone().requires_grad_(True),
              "noise": [torch.randn(1, 1, s, s) for s in (4, 8, 8, 16, 16)], "history": []}
    path = projector.save_projection(root, "face.01.png", result)
    assert path == os.path.join(root, "latents", "face.pt")           # the dataset's stem: up to the first dot
    ds = dataset.ImageLatentDataset(root, transform=dataset.default_transform(16))
    image, lat, index = ds[0]
    assert image.shape == (3, 16, 16) and index == 0 and torch.equal(lat, latent)
    stored = torch.load(path, weights_only=True)["face.01.png"]
    assert set(stored) == {"img", "latent", "noise"} and stored["img"].shape == (3, 16, 16)
    assert all(torch.equal(a, b) for a, b in zip(stored["noise"], result["noise"]))


def test_new_entries_refuse_bad_arguments_before_any_launch():
    L = lib.load()
    d = (C.c_float * 64)()                 # a host buffer stands in for device memory: nothing is launched
    p = C.cast(d, C.c_void_p)

    def ptrs(n, v=p):
        return (C.c_void_p * n)(*[v] * n)

    def ints(*v):
        return (C.c_int * len(v))(*v)
    # g2s_noise_grad: NULL pointers, empty sizes
    for args in ((None, p, p, 1, 1, 16), (p, None, p, 1, 1, 16), (p, p, None, 1, 1, 16), (p, p, p, 0, 1, 16),
                 (p, p, p, 1, 0, 16), (p, p, p, 1, 1, 0)):
        assert L.g2s_noise_grad(*args, None) == -1, args
    assert b"NULL" in L.g2s_last_error() or b"positive" in L.g2s_last_error()
    big = lib.C.c_size_t(1 << 30)
    bad_sides = [(12,), (3,), (2,), (1024,), (8, 0), (8, -4)]            # not a power of two, < 4, > 512
    for sides in bad_sides:
        n = len(sides)
        assert L.g2s_noise_regularize(ptrs(n), ptrs(n), ints(*sides), n, 1, p, p, big, None) == -1, sides
        assert b"power of two" in L.g2s_last_error()
        assert L.g2s_noise_normalize(ptrs(n), ints(*sides), n, 1, p, big, None) == -1, sides
        assert L.g2s_noise_regularize_workspace_bytes(ints(*sides), n, 1) == 0
        assert L.g2s_noise_normalize_workspace_bytes(ints(*sides), n, 1) == 0
    # NULL tables, NULL entries, NULL loss
    assert L.g2s_noise_regularize(None, None, ints(8), 1, 1, p, p, big, None) == -1
    assert L.g2s_noise_regularize(ptrs(1), None, None, 1, 1, p, p, big, None) == -1
    assert L.g2s_noise_regularize(ptrs(1), None, ints(8), 1, 1, None, p, big, None) == -1
    assert L.g2s_noise_regularize(ptrs(2, None), None, ints(8, 8), 2, 1, p, p, big, None) == -1
    assert L.g2s_noise_regularize(ptrs(1), ptrs(1, None), ints(8), 1, 1, p, p, big, None) == -1
    assert L.g2s_noise_normalize(None, ints(8), 1, 1, p, big, None) == -1
    assert L.g2s_noise_normalize(ptrs(1), None, 1, 1, p, big, None) == -1
    assert L.g2s_noise_normalize(ptrs(1, None), ints(8), 1, 1, p, big, None) == -1
    # the table limit (G2S_NOISE_MAX_MAPS = 32), no maps, no batch
    for n, B in ((33, 1), (0, 1), (1, 0), (1, 65)):
        m = max(n, 1)
        assert L.g2s_noise_regularize(ptrs(m), None, ints(*[8] * m), n, B, p, p, big, None) == -1, (n, B)
        assert L.g2s_noise_normalize(ptrs(m), ints(*[8] * m), n, B, p, big, None) == -1, (n, B)
    # a missing or short workspace is its own error, also before any launch
    assert L.g2s_noise_regularize_workspace_bytes(ints(16), 1, 1) == (64 + 2 * 2) * 4
    assert L.g2s_noise_regularize(ptrs(1), None, ints(16), 1, 1, p, None, 0, None) == -3
    assert L.g2s_noise_regularize(ptrs(1), None, ints(16), 1, 1, p, p, lib.C.c_size_t(8), None) == -3
    assert L.g2s_noise_normalize_workspace_bytes(ints(64, 4), 2, 3) == (3 + 1) * 2 * 4
    assert L.g2s_noise_normalize(ptrs(1), ints(16), 1, 1, None, 0, None) == -3


def test_generator_on_cpu_tensors_equals_the_reference(fx):
    """CPU tensors take plain torch ops through the layer loop (op/cpu_tensors.py): image, latent gradient and the
    noise-map gradients of the size-16 generator against the reference's float64 run."""
    G = pc.fixture_generator(sg2)
    w, noises, gy = pc.generator_inputs()
    w = torch.from_numpy(w).requires_grad_(True)
    nz = [torch.from_numpy(n).requires_grad_(True) for n in noises]
    img, _ = G([w], input_is_w=True, noise=nz)
    grads = torch.autograd.grad(img, [w] + nz, torch.from_numpy(gy))
    ref = torch.from_numpy(fx["g16.img"])
    assert float((img.detach() - ref).abs().max()) <= 1e-5 * float(ref.abs().max())
    assert pc.l2_rel(grads[0], torch.from_numpy(fx["g16.gw"])) <= 1e-5
    for k in range(len(nz)):
        assert pc.l2_rel(grads[1 + k], torch.from_numpy(fx[f"g16.gnoise{k}"])) <= 1e-5, k


def _small_generator():
    torch.manual_seed(0)
    G = sg2.Generator(16, 32, 3, channel_multiplier=1)
    with torch.no_grad():
        for k, v in G.state_dict().items():
            if "noise" in k and "weight" in k:
                v.fill_(0.3)                  # NoiseInjection starts at 0: let the maps matter
    return G.eval().requires_grad_(False)


def test_project_runs_on_cpu_tensors():
    """Three steps on CPU tensors: the layer loop of Generator.forward and the torch noise functions."""
    from model_cases import fake_perceptual
    G = _small_generator()
    gen = torch.Generator().manual_seed(1)
    stats = projector.mean_latent_stats(G, n=256, generator=gen)
    assert stats[0].shape == (32,) and stats[1].dim() == 0 and float(stats[1]) > 0
    target, _ = G([stats[0][None] + 0.5 * torch.randn(1, 32, generator=gen)], input_is_w=True)
    for w_plus in (False, True):
        res = projector.project(G, fake_perceptual, target, steps=3, w_plus=w_plus, mse=0.1 if w_plus else 0.0,
                                latent_stats=stats, generator=gen)
        assert res["img"].shape == (1, 3, 16, 16) and bool(torch.isfinite(res["img"]).all())
        assert res["latent"].shape == ((G.n_latent, 32) if w_plus else (32,)) and res["history"] == []
        assert not torch.equal(res["latent"].reshape(-1, 32)[0], stats[0])          # it moved
        assert [n.shape[-1] for n in res["noise"]] == [4, 8, 8, 16, 16]
        for n in res["noise"]:
            assert bool(torch.isfinite(n).all()) and not n.requires_grad
            assert abs(float(n.double().mean())) <= 1e-6 and abs(float(n.double().std()) - 1) <= 1e-5
        e = projector.evaluate(G, fake_perceptual, target, res["latent"], res["noise"])
        assert e.dim() == 0 and bool(torch.isfinite(e))
    with pytest.raises(ValueError):
        projector.project(G, fake_perceptual, target.repeat(2, 1, 1, 1), steps=1, latent_stats=stats)


def test_command_line_projects_a_file_into_the_dataset_layout(tmp_path, monkeypatch):
    """The reference's options on a size-16 random-weight checkpoint and a generated picture (no real checkpoint or
    photograph exists offline): the run leaves latents/<stem>.pt that the dataset reads, and the preview image."""
    from PIL import Image
    root = tmp_path / "data"
    root.mkdir()
    torch.manual_seed(0)
    G = sg2.Generator(16, 512, 8, channel_multiplier=1)
    torch.save({"g_ema": G.state_dict()}, str(tmp_path / "g.pt"))
    rng = np.random.default_rng(0)
    Image.fromarray(rng.integers(0, 255, (20, 28, 3), dtype=np.uint8)).save(str(root / "img.png"))
    (root / "list.txt").write_text("img.png\n")
    monkeypatch.chdir(tmp_path)
    paths = projector.main(["--ckpt", str(tmp_path / "g.pt"), "--size", "16", "--channel_multiplier", "1", "--step", "2",
                            "--lr", "0.05", "--noise", "0.05", "--noise_ramp", "0.75", "--noise_regularize", "1e5",
                            "--mse", "0.5", "--w_plus", "--device", "cpu", str(root / "img.png")])
    assert paths == [str(root / "latents" / "img.pt")] and os.path.exists(tmp_path / "img-project.png")
    image, latent, _ = dataset.ImageLatentDataset(str(root), transform=dataset.default_transform(16))[0]
    assert latent.shape == (G.n_latent, 512) and bool(torch.isfinite(latent).all())
    assert projector.load_image(str(root / "img.png"), 16).shape == (1, 3, 16, 16)
