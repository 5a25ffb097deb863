"""-m gpu: the sample generator on the device — g2s_mapping_fwd and g2s_rows_mean against the float64 statement of
tests/generate_cases.py, g2s_image_to_u8 against the torch expression, and generate.sample against the layer loop and
the reference's float64 fixture (tests/golden/generate.npz).

Bound of the float64 comparisons: for each case the existing float32 route (PixelNorm, then F.linear +
fused_leaky_relu per layer, on the GPU — what Generator.style_forward runs) is measured against the same float64
values, and the kernel has to stay within MARGIN = 4 x that, the margin the projector's and the reduction kernels'
tests use for another summation order.  Two figures are held: the largest absolute error (an absolute figure, so the
smallest-magnitude outputs are held to the float32 route's own error there) and the L2 error relative to |reference|.
Both routes and the statement get the SAME float32 scaled weights, so only the kernel's own rounding is compared."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import generate_cases as gc
import projector_cases as pc

pytestmark = pytest.mark.gpu

MARGIN = 4.0
SENTINEL = -12345.5


@pytest.fixture(scope="module")
def g2s():
    import gan2shape_amd  # noqa: F401
    from gan2shape_amd import lib
    lib.load()
    return gan2shape_amd


@pytest.fixture(scope="module")
def T(g2s):
    from gan2shape_amd import generate
    return generate.mapping_tile()


def _scaled32(w_raw, b_raw):
    """float32 stacks as EqualLinear forms them: weight * scale, bias * lr_mul, rounded to float32."""
    scale = np.float32(gc.LR_MLP / math.sqrt(w_raw.shape[-1]))
    return (w_raw * scale).astype(np.float32), (b_raw * np.float32(gc.LR_MLP)).astype(np.float32)


def _torch_route(z, w, b, pixel_norm, center=None, truncation=1.0):
    from gan2shape_amd.op import fused_leaky_relu
    h = z
    if pixel_norm:
        h = h * torch.rsqrt(torch.mean(h ** 2, dim=1, keepdim=True) + 1e-8)
    for wl, bl in zip(w, b):
        h = fused_leaky_relu(F.linear(h, wl), bl)
    if center is not None:
        h = center + truncation * (h - center)
    return h


def _errors(a, ref):
    d = a.astype(np.float64) - ref
    return float(np.abs(d).max()), float(np.linalg.norm(d) / np.linalg.norm(ref))


def _run_mapping(z, w, b, pixel_norm, center=None, truncation=1.0, with_partial=False, T=16):
    """The kernel on `z` with guard bands round `out` (and `partial`): returns (out, partial) as numpy after checking
    that nothing outside them was written."""
    from gan2shape_amd import generate
    N, D = z.shape
    guard = 2 * T * D
    buf = torch.full((guard + N * D + guard,), SENTINEL, device="cuda")
    out = buf[guard:guard + N * D].view(N, D)
    tiles = (N + T - 1) // T
    pbuf = torch.full((D + tiles * D + D,), SENTINEL, device="cuda")
    partial = pbuf[D:D + tiles * D].view(tiles, D) if with_partial else None
    got = generate.mapping_fwd(z, w, b, pixel_norm, center=center, truncation=truncation, out=out, partial=partial)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr()
    assert bool((buf[:guard] == SENTINEL).all()) and bool((buf[guard + N * D:] == SENTINEL).all())
    assert bool((pbuf[:D] == SENTINEL).all()) and bool((pbuf[D + tiles * D:] == SENTINEL).all())
    if not with_partial:
        assert bool((pbuf == SENTINEL).all())
    assert not bool((out == SENTINEL).any())
    return out.cpu().numpy(), None if partial is None else partial.cpu().numpy()


def _check_case(name, z, w32, b32, pixel_norm, T, center=None, truncation=1.0):
    ref = gc.mapping64(z, w32, b32, pixel_norm=pixel_norm, center=center, truncation=truncation)
    zc, wc, bc = (torch.from_numpy(a).cuda() for a in (z, w32, b32))
    cc = None if center is None else torch.from_numpy(center).cuda()
    with torch.no_grad():
        route = _torch_route(zc, wc, bc, pixel_norm, cc, truncation).cpu().numpy()
    got, _ = _run_mapping(zc, wc, bc, pixel_norm, cc, truncation, T=T)
    assert np.isfinite(got).all()
    (ra, rl), (ka, kl) = _errors(route, ref), _errors(got, ref)
    print(f"[mapping {name}] N {z.shape[0]} D {z.shape[1]} L {len(w32)}: max abs kernel {ka:.2e} / torch {ra:.2e}; "
          f"L2 rel kernel {kl:.2e} / torch {rl:.2e}; max |ref| {np.abs(ref).max():.2e}")
    assert ka <= MARGIN * ra and kl <= MARGIN * rl, name
    return got


# ------------------------------------------------------------------------------------------------ g2s_mapping_fwd
@pytest.mark.parametrize("index", range(7))
def test_mapping_against_the_float64_statement(g2s, T, index):
    name, N, D, L, opt = gc.mapping_cases(T)[index]
    z, w_raw, b_raw = gc.mapping_inputs(N, D, L, zero_row=opt.get("zero_row"))
    w32, b32 = _scaled32(w_raw, b_raw)
    center = None
    if "truncation" in opt:
        center = np.random.default_rng(5).standard_normal(D).astype(np.float32)
    got = _check_case(name, z, w32, b32, True, T, center, opt.get("truncation", 1.0))
    if "zero_row" in opt:      # PixelNorm's 1e-8 keeps the row finite: it is the network's answer to a zero input
        ref0 = gc.mapping64(np.zeros((1, D), np.float32), w32, b32)
        assert np.abs(got[opt["zero_row"]] - ref0[0]).max() <= 1e-5 * np.abs(ref0).max()


@pytest.mark.parametrize("which", ["full", "depth3", "skip3"])
def test_mapping_fixture_slices(g2s, T, golden, which):
    """The (3, 32, 4) network of tests/golden/mapping.npz: whole, depth=3 (PixelNorm + 2 linears), skip=3 (the last two
    linears, no PixelNorm) — and map_latents' translation of skip / depth onto the kernel's arguments."""
    from gan2shape_amd import generate
    from gan2shape_amd import stylegan2 as sg2
    m = golden("mapping")
    w_raw = np.stack([m[f"style.{i}.weight"] for i in range(1, 5)])
    b_raw = np.stack([m[f"style.{i}.bias"] for i in range(1, 5)])
    w32, b32 = _scaled32(w_raw, b_raw)
    z = m["style.z"]
    if which == "full":
        got = _check_case(which, z, w32, b32, True, T)
    elif which == "depth3":
        got = _check_case(which, z, w32[:2], b32[:2], True, T)
    else:
        got = _check_case(which, m["style.depth3"], w32[2:], b32[2:], False, T)
    assert np.abs(got - m[f"style.{which}"]).max() <= 1e-5 * np.abs(m[f"style.{which}"]).max()
    G = sg2.Generator(8, 32, 4, channel_multiplier=1)
    with torch.no_grad():
        for i in range(1, 5):
            G.style[i].weight.copy_(torch.from_numpy(w_raw[i - 1]))
            G.style[i].bias.copy_(torch.from_numpy(b_raw[i - 1]))
    G = G.cuda().eval().requires_grad_(False)
    kw = {"full": {}, "depth3": {"depth": 3}, "skip3": {"skip": 3}}[which]
    x = torch.from_numpy(m["style.depth3"] if which == "skip3" else z).cuda()
    calls = []
    orig = generate.mapping_fwd
    generate.mapping_fwd = lambda *a, **k: calls.append(1) or orig(*a, **k)
    floor = generate.KERNEL_MIN_ROWS
    generate.KERNEL_MIN_ROWS = 1
    try:
        mapped = generate.map_latents(G, x, **kw)
    finally:
        generate.mapping_fwd, generate.KERNEL_MIN_ROWS = orig, floor
    assert calls == [1]
    # the same launch up to the last bit of scale (two ways of writing lr_mul / sqrt(D))
    assert np.abs(mapped.cpu().numpy() - got).max() <= 1e-6 * np.abs(got).max()


def test_map_latents_routing(g2s):
    from gan2shape_amd import generate
    from gan2shape_amd import stylegan2 as sg2
    G = pc.fixture_generator(sg2).cuda()
    calls = []
    orig = generate.mapping_fwd
    generate.mapping_fwd = lambda *a, **k: calls.append(1) or orig(*a, **k)
    floor = generate.KERNEL_MIN_ROWS
    try:
        generate.KERNEL_MIN_ROWS = 4
        z = torch.randn(4, 32, device="cuda")
        a = generate.map_latents(G, z)
        assert calls == [1]
        b = generate.map_latents(G, z[:3])                       # below the threshold: torch ops
        assert calls == [1]
        with torch.no_grad():
            ref = G.style_forward(z)
        assert float((a - ref).abs().max()) <= 1e-5 * float(ref.abs().max())
        assert float((b - ref[:3]).abs().max()) <= 1e-5 * float(ref.abs().max())
        G.style[1].weight.requires_grad_(True)                   # trainable mapping weights: torch ops
        generate.map_latents(G, z)
        assert calls == [1]
    finally:
        generate.mapping_fwd, generate.KERNEL_MIN_ROWS = orig, floor


# ----------------------------------------------------------------------------------------------------------- mean
@pytest.fixture(scope="module")
def mean_net():
    _, w_raw, b_raw = gc.mapping_inputs(1, 512, 1, seed=3)
    return _scaled32(w_raw, b_raw)


@pytest.mark.parametrize("n", ["1", "T+1", "4096"])
def test_ordered_mean(g2s, T, mean_net, n):
    from gan2shape_amd import generate, lib
    N = {"1": 1, "T+1": T + 1, "4096": 4096}[n]
    w32, b32 = mean_net
    z = np.random.default_rng([47, N]).standard_normal((N, 512)).astype(np.float32)
    mapped64 = gc.mapping64(z, w32, b32)
    ref = mapped64.mean(0)
    assert np.abs(gc.ordered_mean64(mapped64, T) - ref).max() <= 1e-12 * np.abs(ref).max()
    zc, wc, bc = (torch.from_numpy(a).cuda() for a in (z, w32, b32))
    with torch.no_grad():
        route = _torch_route(zc, wc, bc, True).mean(0).cpu().numpy()
    results = []
    prev = lib.set_deterministic(False)
    try:
        for det in (False, True, False):
            lib.set_deterministic(det)
            out, partial = _run_mapping(zc, wc, bc, True, with_partial=True, T=T)
            mean = generate.rows_mean(torch.from_numpy(partial).cuda(), N)
            results.append((out, partial, mean.cpu().numpy()))
    finally:
        lib.set_deterministic(prev)
    out, partial, mean = results[0]
    for o, p, m in results[1:]:
        assert np.array_equal(o, out) and np.array_equal(p, partial) and np.array_equal(m, mean)
    assert partial.shape == ((N + T - 1) // T, 512)
    p64 = gc.partial_sums64(out, T)                       # of the kernel's own rows: the sums alone
    assert np.abs(partial - p64).max() <= (T - 1) * T * 2.0 ** -24 * np.abs(out).max()   # T - 1 roundings of sums <= T max
    (ra, rl), (ka, kl) = _errors(route, ref), _errors(mean, ref)
    print(f"[mean N {N}] max abs kernel {ka:.2e} / torch {ra:.2e}; L2 rel kernel {kl:.2e} / torch {rl:.2e}")
    assert ka <= MARGIN * ra and kl <= MARGIN * rl


def test_mean_latent_is_one_mapping_launch_and_one_mean(g2s, T):
    from gan2shape_amd import generate
    from gan2shape_amd import stylegan2 as sg2
    G = pc.fixture_generator(sg2).cuda()
    gen = torch.Generator(device="cuda").manual_seed(3)
    got = generate.mean_latent(G, 70, gen)
    z = torch.randn(70, 32, device="cuda", generator=torch.Generator(device="cuda").manual_seed(3))
    with torch.no_grad():
        ref = G.style_forward(z).mean(0, keepdim=True)
    assert tuple(got.shape) == (1, 32)
    assert float((got - ref).abs().max()) <= 1e-5 * float(ref.abs().max())
    again = generate.mean_latent(G, 70, torch.Generator(device="cuda").manual_seed(3))
    assert torch.equal(got, again)


# ------------------------------------------------------------------------------------------------ g2s_image_to_u8
@pytest.mark.parametrize("B,H,W", gc.IMAGE_SHAPES)
def test_image_to_u8_equals_the_torch_expression(g2s, B, H, W):
    from gan2shape_amd import generate
    x = torch.from_numpy(gc.image_inputs(B, H, W)).cuda()
    buf = torch.full((64 + B * H * W * 3 + 64,), 77, dtype=torch.uint8, device="cuda")
    from gan2shape_amd import lib
    out = buf[64:64 + B * H * W * 3].view(B, H, W, 3)
    lib.check(lib.load().g2s_image_to_u8(lib.ptr(x), lib.ptr(out), B, H, W, lib.stream()))
    torch.cuda.synchronize()
    want = generate._quantise_torch(x)
    assert torch.equal(out, want)
    assert torch.equal(generate.image_to_u8(x), want)
    assert bool((buf[:64] == 77).all()) and bool((buf[64 + B * H * W * 3:] == 77).all())
    assert np.array_equal(want.cpu().numpy(), gc.quantise(x.cpu().numpy()))
    # an input whose planes are not 16-byte aligned takes the narrow path
    if (H * W) % 4 == 0:
        shifted = torch.empty(x.numel() + 1, device="cuda")[1:].view_as(x).copy_(x)
        out2 = torch.empty(B, H, W, 3, dtype=torch.uint8, device="cuda")
        lib.check(lib.load().g2s_image_to_u8(lib.ptr(shifted), lib.ptr(out2), B, H, W, lib.stream()))
        assert torch.equal(out2, want)


# --------------------------------------------------------------------------------------------------------- sample
def test_sample_equals_the_layer_loop_with_the_same_draws(g2s):
    """Size-16 generator of test_generator_golden (fill_deterministic, seed 123), n = 3, fixed draws: each sample's
    one-node forward against the layer-loop Generator.forward on the [3, 1, r, r] noise batch, within the 2e-6 of max
    that test_gpu_projector.py holds one-node against layer loop to; w equals map_latents."""
    from gan2shape_amd import generate, synthesis
    from gan2shape_amd import stylegan2 as sg2
    G = pc.fixture_generator(sg2).cuda()
    g = torch.Generator().manual_seed(21)
    z = torch.randn(3, 32, generator=g).cuda()
    noise = [torch.randn(3, 1, r, r, generator=g).cuda() for r in generate.noise_sides(G)]
    center = generate.mean_latent(G, 64, torch.Generator(device="cuda").manual_seed(1))
    calls = []
    orig = synthesis.synthesize
    synthesis.synthesize = lambda *a: calls.append(1) or orig(*a)
    try:
        images, w = generate.sample(G, 3, 0.7, center, draws=(z, noise))
    finally:
        synthesis.synthesize = orig
    assert calls == [1, 1, 1]                                   # one one-node forward per sample
    assert torch.equal(w, generate.map_latents(G, z, center=center, truncation=0.7))
    with torch.no_grad():
        wt = center + 0.7 * (G.style_forward(z) - center)
        try:
            sg2.Generator.ONE_NODE = False
            loop, _ = G([w], input_is_w=True, noise=noise)
        finally:
            sg2.Generator.ONE_NODE = True
    assert float((w - wt).abs().max()) <= 1e-5 * float(wt.abs().max())
    assert tuple(images.shape) == (3, 3, 16, 16)
    assert float((images - loop).abs().max()) <= 2e-6 * float(loop.abs().max())
    assert float((images[0] - images[1]).abs().max()) > 1e-3 * float(loop.abs().max())
    # fresh draws come from the generator in the documented order
    gen = torch.Generator(device="cuda").manual_seed(8)
    im2, w2 = generate.sample(G, 2, 0.7, center, gen)
    gen = torch.Generator(device="cuda").manual_seed(8)
    z2 = torch.randn(2, 32, device="cuda", generator=gen)
    n2 = [torch.randn(2, 1, r, r, device="cuda", generator=gen) for r in (4, 8, 8, 16, 16)]
    im3, w3 = generate.sample(G, 2, 0.7, center, draws=(z2, n2))
    assert torch.equal(w2, w3) and float((im2 - im3).abs().max()) <= 2e-6 * float(im3.abs().max())


def test_sample_matches_the_reference_fixture(g2s, golden):
    """generate.npz: the reference's Generator(8, 32, 4) in float64.  Truncated w and image within 4 x the reference's
    own float32 error.  The uint8 image: equal wherever the float64 pixel is farther from a rounding boundary than
    the image bound allows it to move (255 / 2 x the bound, in units of one grey level), at most one level off
    elsewhere."""
    from gan2shape_amd import generate
    from gan2shape_amd import stylegan2 as sg2
    fx = golden("generate")
    cfg = gc.G_CFG
    G = pc.fixture_generator(sg2, cfg["size"], cfg["style_dim"], cfg["n_mlp"], cfg["seed"]).cuda()
    zm = torch.from_numpy(fx["z_mean"]).cuda()
    w_, b_ = generate.mapping_weights(G)
    T = generate.mapping_tile()
    partial = torch.empty((gc.N_MEAN + T - 1) // T, 32, device="cuda")
    generate.mapping_fwd(zm, w_, b_, True, partial=partial)
    center = generate.rows_mean(partial, gc.N_MEAN)[None]
    ref = fx["mean_latent"]
    assert np.abs(center.cpu().numpy() - ref).max() <= MARGIN * float(fx["ref_fp32_err.mean"]) * np.abs(ref).max()
    draws = (torch.from_numpy(fx["z"]).cuda(), [torch.from_numpy(fx[f"noise{i}"]).cuda() for i in range(3)])
    center64 = torch.from_numpy(ref).float().cuda()
    images, w = generate.sample(G, gc.N_Z, gc.TRUNCATION, center64, draws=draws)
    e_w = np.abs(w.cpu().numpy() - fx["w_truncated"]).max() / np.abs(fx["w_truncated"]).max()
    e_i = np.abs(images.cpu().numpy() - fx["image"]).max() / np.abs(fx["image"]).max()
    print(f"[generate.npz] w {e_w:.2e}/{MARGIN * float(fx['ref_fp32_err.wt']):.2e} "
          f"image {e_i:.2e}/{MARGIN * float(fx['ref_fp32_err.img']):.2e}")
    assert e_w <= MARGIN * float(fx["ref_fp32_err.wt"])
    assert e_i <= MARGIN * float(fx["ref_fp32_err.img"])
    u8 = generate.image_to_u8(images).cpu().numpy().astype(np.int64)
    want = fx["image_u8"].astype(np.int64)
    level = (np.clip(np.moveaxis(fx["image"], 1, -1), -1, 1) + 1) / 2 * 255 + 0.5
    slack = MARGIN * float(fx["ref_fp32_err.img"]) * np.abs(fx["image"]).max() * 255 / 2
    near = np.abs(level - np.rint(level)) <= slack
    assert np.array_equal(u8[~near], want[~near])
    assert np.abs(u8 - want).max() <= 1
