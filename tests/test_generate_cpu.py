"""-m "not gpu": the sample generator's host side — the float64 statement of its kernels (generate_cases.py) against
the reference's results (tests/golden/mapping.npz, generate.npz), map_latents / sample on CPU tensors against
style_forward and Generator.forward, the files the command writes against ImageLatentDataset, and the C ABI."""
import os
import re

import numpy as np
import pytest
import torch

import gan2shape_amd  # noqa: F401
from gan2shape_amd import dataset, generate, lib
from gan2shape_amd import stylegan2 as sg2

import generate_cases as gc
import projector_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fx(golden):
    return golden("generate")


def fixture_generator():
    cfg = gc.G_CFG
    return pc.fixture_generator(sg2, cfg["size"], cfg["style_dim"], cfg["n_mlp"], cfg["seed"])


def _stacks(G):
    layers = list(G.style)[1:]
    return gc.scaled(np.stack([m.weight.detach().numpy() for m in layers]),
                     np.stack([m.bias.detach().numpy() for m in layers]))


# ------------------------------------------------------------------------------------------- float64 statement
def test_statement_reproduces_the_mapping_fixture(golden):
    """mapping.npz is the reference's float32 run: the float64 statement is within a few float32 roundings of it."""
    m = golden("mapping")
    w, b = gc.scaled(np.stack([m[f"style.{i}.weight"] for i in range(1, 5)]),
                     np.stack([m[f"style.{i}.bias"] for i in range(1, 5)]))
    z = m["style.z"]
    full = gc.style_forward64(z, w, b)
    depth3 = gc.style_forward64(z, w, b, depth=3)
    skip3 = gc.style_forward64(depth3, w, b, skip=3)
    for name, got in (("full", full), ("depth3", depth3), ("skip3", skip3)):
        ref = m[f"style.{name}"]
        assert np.abs(got - ref).max() <= 1e-5 * np.abs(ref).max(), name
    assert np.abs(skip3 - full).max() <= 1e-12          # depth=3 then skip=3 is the whole network
    assert np.array_equal(gc.mapping64(z, w[:2], b[:2], pixel_norm=True), depth3)


def test_statement_reproduces_the_generate_fixture(fx):
    G = fixture_generator()
    w, b = _stacks(G)
    full = gc.style_forward64(fx["z"], w, b)
    assert np.abs(full - fx["w"]).max() <= 1e-12 * np.abs(fx["w"]).max()
    mapped = gc.style_forward64(fx["z_mean"], w, b)
    T = 16
    mean = gc.ordered_mean64(mapped, T)
    assert np.abs(mean - fx["mean_latent"][0]).max() <= 1e-12 * np.abs(fx["mean_latent"]).max()
    assert gc.partial_sums64(mapped, T).shape == (5, 32)
    wt = gc.style_forward64(fx["z"], w, b, center=fx["mean_latent"], truncation=gc.TRUNCATION)
    assert np.abs(wt - fx["w_truncated"]).max() <= 1e-12 * np.abs(fx["w_truncated"]).max()
    assert np.array_equal(gc.quantise(fx["image"].astype(np.float32)), fx["image_u8"])
    assert fx["image_u8"].shape == (gc.N_Z, 8, 8, 3) and fx["image_u8"].dtype == np.uint8


@pytest.mark.parametrize("B,H,W", gc.IMAGE_SHAPES)
def test_quantiser_statement_equals_the_torch_expression(B, H, W):
    x = gc.image_inputs(B, H, W)
    got = generate.image_to_u8(torch.from_numpy(x))              # CPU tensors: the torch expression
    assert got.dtype == torch.uint8 and tuple(got.shape) == (B, H, W, 3)
    assert np.array_equal(got.numpy(), gc.quantise(x))
    one = np.array([-2.0, -1.0, 0.0, 1.0, 3.0], np.float32).reshape(1, 1, 1, 5).repeat(3, 1)
    assert list(gc.quantise(one)[0, 0, :, 0]) == [0, 0, 128, 255, 255]    # 0 -> 127.5 + 0.5 = 128


# ---------------------------------------------------------------------------------------------------- CPU path
@pytest.mark.parametrize("skip,depth", [(0, 100), (0, 3), (3, 100), (1, 4), (0, 1)])
def test_map_latents_on_cpu_equals_style_forward_and_the_lerp(fx, skip, depth):
    G = fixture_generator()
    z = torch.from_numpy(fx["z"])
    with torch.no_grad():
        ref = G.style_forward(z, skip=skip, depth=depth)
    assert torch.equal(generate.map_latents(G, z, skip=skip, depth=depth), ref)
    center = torch.from_numpy(fx["mean_latent"]).float()
    got = generate.map_latents(G, z, skip=skip, depth=depth, center=center, truncation=0.7)
    assert torch.equal(got, center + 0.7 * (ref - center))
    w, b = _stacks(G)
    want = gc.style_forward64(fx["z"], w, b, skip=skip, depth=depth, center=fx["mean_latent"], truncation=0.7)
    assert np.abs(got.numpy() - want).max() <= 1e-5 * np.abs(want).max()


def test_layer_range_and_weight_cache():
    G = fixture_generator()
    assert generate._layer_range(G, 0, 100) == (True, 0, 4)
    assert generate._layer_range(G, 0, 3) == (True, 0, 2)
    assert generate._layer_range(G, 3, 100) == (False, 2, 2)
    assert generate._layer_range(G, 0, 1) == (True, 0, 0)
    w, b = generate.mapping_weights(G)
    assert tuple(w.shape) == (4, 32, 32) and tuple(b.shape) == (4, 32)
    w64, b64 = _stacks(G)
    assert np.allclose(w.numpy(), w64, rtol=1e-6, atol=0) and np.allclose(b.numpy(), b64, rtol=1e-6, atol=0)
    assert generate.mapping_weights(G)[0] is w                       # cached
    with torch.no_grad():
        G.style[2].bias.add_(1.0)
    w2, b2 = generate.mapping_weights(G)                             # a changed parameter rebuilds the stacks
    assert w2 is not w and float((b2[1] - b[1]).abs().min()) > 0.009


def test_mean_latent_on_cpu(fx):
    G = fixture_generator()
    g = torch.Generator().manual_seed(5)
    got = generate.mean_latent(G, 70, g)
    z = torch.randn(70, 32, generator=torch.Generator().manual_seed(5))
    with torch.no_grad():
        assert torch.equal(got, G.style_forward(z).mean(0, keepdim=True))


def test_sample_on_cpu_equals_generator_forward_by_hand(fx):
    G = fixture_generator()
    center = torch.from_numpy(fx["mean_latent"]).float()
    images, w = generate.sample(G, 3, 0.7, center, torch.Generator().manual_seed(9))
    g = torch.Generator().manual_seed(9)
    z = torch.randn(3, 32, generator=g)
    noise = [torch.randn(3, 1, r, r, generator=g) for r in (4, 8, 8)]        # one draw per styled layer, in layer order
    assert generate.noise_sides(G) == [4, 8, 8]
    with torch.no_grad():
        wt = center + 0.7 * (G.style_forward(z) - center)
        by_hand, _ = G([wt], input_is_w=True, noise=noise)
    assert torch.equal(w, wt) and tuple(images.shape) == (3, 3, 8, 8)
    assert float((images - by_hand).abs().max()) <= 2e-6 * float(by_hand.abs().max())
    # the fixture's draws reproduce the reference's float64 image and latent to float32 accuracy
    draws = (torch.from_numpy(fx["z"]), [torch.from_numpy(fx[f"noise{i}"]) for i in range(3)])
    images, w = generate.sample(G, gc.N_Z, gc.TRUNCATION, center, draws=draws)
    assert np.abs(w.numpy() - fx["w_truncated"]).max() <= 4 * float(fx["ref_fp32_err.wt"]) * np.abs(fx["w_truncated"]).max()
    assert np.abs(images.numpy() - fx["image"]).max() <= 4 * float(fx["ref_fp32_err.img"]) * np.abs(fx["image"]).max()
    with pytest.raises(ValueError):
        generate.sample(G, 1, 0.7, None)
    images1, w1 = generate.sample(G, 2, 1.0, None, torch.Generator().manual_seed(9))   # truncation 1: no mean latent
    z2 = torch.randn(2, 32, generator=torch.Generator().manual_seed(9))
    with torch.no_grad():
        assert torch.equal(w1, G.style_forward(z2)) and tuple(images1.shape) == (2, 3, 8, 8)


# ---------------------------------------------------------------------------------------------- dataset round trip
def test_written_samples_read_back_through_the_dataset(tmp_path):
    G = fixture_generator()
    out = str(tmp_path / "root" / "toy")
    seen = []
    orig = generate.sample

    def recording(*a, **k):
        seen.append(orig(*a, **k))
        return seen[-1]
    generate.sample = recording
    try:
        names = generate.main(["--ckpt", "unused", "--size", "8", "--out", out, "--pics", "2", "--sample", "2",
                               "--truncation", "0.7", "--truncation-mean", "64", "--seed", "3", "--device", "cpu"], G=G)
    finally:
        generate.sample = orig
    assert names == ["%06d.png" % i for i in range(4)]
    assert open(os.path.join(out, "list.txt")).read().split() == names
    ds = dataset.ImageLatentDataset(out, transform=dataset.default_transform(8))
    assert len(ds) == 4
    images = torch.cat([s[0] for s in seen])
    latents = torch.cat([s[1] for s in seen])
    pixels = generate.image_to_u8(images)
    for i in range(4):
        image, latent, index = ds[i]
        assert index == i and tuple(latent.shape) == (32,)
        assert torch.equal(latent, latents[i])
        assert torch.equal(image, pixels[i].permute(2, 0, 1).float().div(255) * 2 - 1)
    assert float((latents[0] - latents[1]).abs().max()) > 0 and float((images[0] - images[2]).abs().max()) > 0


def test_truncation_one_computes_no_mean_latent(tmp_path):
    G = fixture_generator()
    orig = generate.mean_latent
    generate.mean_latent = lambda *a, **k: pytest.fail("mean latent computed at truncation 1")
    try:
        names = generate.write_samples(G, str(tmp_path / "d"), 1, 1, truncation=1.0,
                                       generator=torch.Generator().manual_seed(0))
    finally:
        generate.mean_latent = orig
    assert names == ["000000.png"]


# ------------------------------------------------------------------------------------------------------- C ABI
def test_abi_declares_the_new_symbols_and_rejects_bad_sizes():
    header = open(os.path.join(ROOT, "include", "g2s.h")).read()
    declared = set(re.findall(r"\b(g2s_[a-z0-9_]+)\s*\(", header))
    new = {"g2s_mapping_fwd", "g2s_rows_mean", "g2s_image_to_u8", "g2s_mapping_tile"}
    assert new <= declared and new <= set(lib.SIGNATURES)
    L = lib.load()
    assert L.g2s_abi_version() == 1
    T = L.g2s_mapping_tile()
    assert T >= 1 and T == generate.mapping_tile()
    d = (lib.C.c_float * 4)()        # stands in for device memory: every call below is refused before a launch
    for N, D, layers, word in ((0, 32, 1, b"N ="), (1, 48, 1, b"D ="), (1, 16, 1, b"D ="), (1, 544, 1, b"D ="),
                               (1, 32, 0, b"L ="), (1, 32, 17, b"L =")):
        rc = L.g2s_mapping_fwd(d, d, d, None, d, None, N, D, layers, 1, 0.2, 1.0, 1.0, None)
        assert rc == -1 and word in L.g2s_last_error(), (N, D, layers, L.g2s_last_error())
    assert L.g2s_mapping_fwd(None, d, d, None, d, None, 1, 32, 1, 1, 0.2, 1.0, 1.0, None) == -1
    assert b"NULL" in L.g2s_last_error()
    assert L.g2s_rows_mean(None, d, 1, 32, 1, None) == -1 and L.g2s_rows_mean(d, d, 0, 32, 1, None) == -1
    assert L.g2s_image_to_u8(None, d, 1, 4, 4, None) == -1 and L.g2s_image_to_u8(d, d, 1, 0, 4, None) == -1
