"""-m gpu: the latent projector on the device — g2s_noise_grad, g2s_noise_regularize and g2s_noise_normalize against
float64 (tests/golden/projector.npz holds the reference's results and how far the reference's OWN float32 run is from
them; bounds are 4 x that distance: the margin for another summation order), the generator's noise-map gradients
on the one-node path, per-sample noise, one projector step against its op-by-op form, and a short projection."""
import os

import numpy as np
import pytest
import torch

import projector_cases as pc

pytestmark = pytest.mark.gpu

MARGIN = 4.0     # x the reference's own float32 error


@pytest.fixture(scope="module")
def g2s():
    import gan2shape_amd  # noqa: F401
    from gan2shape_amd import lib
    lib.load()
    return gan2shape_amd


@pytest.fixture(scope="module")
def fx(golden):
    return golden("projector")


def _cuda(arrays, grad=False):
    return [torch.from_numpy(a).cuda().requires_grad_(grad) for a in arrays]


# ----------------------------------------------------------------------------------------------- g2s_noise_grad
@pytest.mark.parametrize("B,C,n", [(1, 1, 16), (1, 512, 16), (3, 64, 64), (2, 33, 49), (1, 512, 4096)])
def test_noise_grad_against_float64(g2s, B, C, n):
    """gnoise = noise_w * sum_c gpre within the bound of a sequential float32 sum of C terms and one product:
    |err| <= C 2^-24 |noise_w| sum_c |gpre| per element (any summation order stays inside it; derived, not measured).
    n = 49 takes the scalar path, the others 16-byte loads."""
    from gan2shape_amd import lib
    g = torch.Generator().manual_seed(B * 1000 + C)
    gpre = torch.randn(B, C, n, generator=g).cuda()
    nw = torch.tensor([-0.37], device="cuda")
    out = torch.full((B, n), float("nan"), device="cuda")
    lib.check(lib.load().g2s_noise_grad(lib.ptr(gpre), lib.ptr(nw), lib.ptr(out), B, C, n, lib.stream()))
    ref = nw.double() * gpre.double().sum(1)
    bound = C * 2.0 ** -24 * nw.double().abs() * gpre.double().abs().sum(1)
    ratio = float(((out.double() - ref).abs() / bound).max())
    print(f"[noise_grad B {B} C {C} n {n}] max |err| / bound {ratio:.3f}")
    assert bool(torch.isfinite(out).all()) and ratio <= 1.0


# ----------------------------------------------------------------------------------------------- regulariser
def _device_regularize(maps):
    """(value, gradients) through the package's autograd Function on CUDA maps."""
    from gan2shape_amd import projector
    xs = [m.detach().clone().requires_grad_(True) for m in maps]
    v = projector.noise_regularize(xs)
    return v.detach(), list(torch.autograd.grad(v, xs))


def _check_regularize(tag, maps, v64, g64, e_val, e_grad):
    from gan2shape_amd import lib
    v, grads = _device_regularize(maps)
    assert v.dim() == 0 and all(g.shape == m.shape for g, m in zip(grads, maps))
    r_val = abs(float(v.double()) - float(v64)) / abs(float(v64))
    r_grad = [pc.l2_rel(g, ref) for g, ref in zip(grads, g64)]
    print(f"[noise_regularize {tag}] value {r_val:.2e} / {MARGIN * e_val:.2e}; gradients " +
          " ".join(f"{r:.2e}/{MARGIN * e:.2e}" for r, e in zip(r_grad, e_grad)))
    # the same inputs give the same bits, whatever g2s_set_deterministic says
    prev = lib.set_deterministic(True)
    try:
        v_d, g_d = _device_regularize(maps)
        lib.set_deterministic(False)
        v_n, g_n = _device_regularize(maps)
        v_n2, g_n2 = _device_regularize(maps)
    finally:
        lib.set_deterministic(prev)
    for other_v, other_g in ((v_d, g_d), (v_n, g_n), (v_n2, g_n2)):
        assert torch.equal(other_v, v) and all(torch.equal(a, b) for a, b in zip(other_g, grads)), tag
    assert r_val <= MARGIN * e_val, tag
    for i, (r, e) in enumerate(zip(r_grad, e_grad)):
        assert r <= MARGIN * e, (tag, i)


@pytest.mark.parametrize("lst,B,kind", pc.CASES)
def test_noise_regularize_against_the_reference_float64(g2s, fx, lst, B, kind):
    name = pc.case_name(lst, B, kind)
    sides = pc.SIDE_LISTS[lst]
    maps = _cuda(pc.make_maps(sides, B, kind))
    g64 = [torch.from_numpy(fx[f"{name}.grad{i}"]).cuda() for i in range(len(sides))]
    _check_regularize(name, maps, fx[f"{name}.value"], g64, float(fx[f"{name}.ref_fp32_err.value"]),
                      fx[f"{name}.ref_fp32_err.grad"])


@pytest.mark.parametrize("side", [256, 512])
@pytest.mark.parametrize("kind", pc.KINDS)
def test_noise_regularize_large_sides_against_the_float64_restatement(g2s, side, kind):
    """Sides 256 and 512 (G(256), the car configuration's G(512)): the fixture has no entry, so the float64 value is
    the restatement of tests/projector_cases.py and the bar is ITS float32 run against it, maximum over N_SEEDS inputs."""
    e_val, e_grad, case = 0.0, 0.0, None
    for seed in range(pc.N_SEEDS):
        maps = _cuda(pc.make_maps((side,), 1, kind, seed))
        v64, g64 = pc.regularize_with_grads(maps, torch.float64)
        v32, g32 = pc.regularize_with_grads(maps, torch.float32)
        e_val = max(e_val, abs(float(v32.double()) - float(v64)) / abs(float(v64)))
        e_grad = max(e_grad, pc.l2_rel(g32[0], g64[0]))
        if seed == 0:
            case = (maps, v64, g64)
    _check_regularize(f"side {side} {kind}", case[0], case[1], case[2], e_val, [e_grad])


def test_noise_regularize_backward_scales_and_skips(g2s):
    """The weight of the projector's loss reaches every gradient; a map that asks for none gets none; a value-only
    call (no map requires a gradient) returns the same value."""
    from gan2shape_amd import projector
    maps = _cuda(pc.make_maps((4, 16, 32), 1, "corr"))
    _, unit = _device_regularize(maps)
    xs = [m.clone().requires_grad_(i != 1) for i, m in enumerate(maps)]
    v = projector.noise_regularize(xs)
    (1e5 * v).backward()
    assert xs[1].grad is None
    for i in (0, 2):
        assert float((xs[i].grad - 1e5 * unit[i]).abs().max()) <= 1e-6 * float((1e5 * unit[i]).abs().max())
    with torch.no_grad():
        assert torch.equal(projector.noise_regularize(maps), v.detach())


# ----------------------------------------------------------------------------------------------- normalisation
@pytest.mark.parametrize("lst,B,kind", pc.CASES)
def test_noise_normalize_against_the_reference_float64(g2s, fx, lst, B, kind):
    from gan2shape_amd import projector
    name = pc.case_name(lst, B, kind)
    sides = pc.SIDE_LISTS[lst]
    maps = _cuda(pc.make_maps(sides, B, kind), grad=True)        # the projector normalises leaves that require grad
    before = [m.data_ptr() for m in maps]
    projector.noise_normalize_(maps)
    assert [m.data_ptr() for m in maps] == before and all(m.requires_grad and m.is_leaf for m in maps)
    for i, m in enumerate(maps):
        d = m.detach().double()
        ref = torch.from_numpy(fx[f"{name}.norm{i}"]).cuda()
        r, e = pc.l2_rel(d, ref), float(fx[f"{name}.ref_fp32_err.norm"][i])
        print(f"[noise_normalize {name} map {i}] mean {float(d.mean()):.1e} std - 1 {float(d.std()) - 1:.1e}; "
              f"vs float64 {r:.2e} / {MARGIN * e:.2e}")
        assert abs(float(d.mean())) <= 1e-6 and abs(float(d.std()) - 1) <= 1e-6, (name, i)
        assert r <= MARGIN * e, (name, i)


@pytest.mark.parametrize("side", [256, 512])
def test_noise_normalize_large_sides(g2s, side):
    """More than one chunk per map (the merge of chunk statistics), with an offset so that a one-pass variance would show."""
    from gan2shape_amd import projector
    m = (3.0 + 0.5 * torch.from_numpy(pc.make_maps((side,), 1, "corr")[0])).cuda()
    ref = (m.double() - m.double().mean()) / m.double().std()
    e = pc.l2_rel(((m - m.mean()) / m.std()), ref)               # torch's own float32 run
    projector.noise_normalize_([m])
    d = m.double()
    print(f"[noise_normalize side {side}] mean {float(d.mean()):.1e} std - 1 {float(d.std()) - 1:.1e}; "
          f"vs float64 {pc.l2_rel(d, ref):.2e} / {MARGIN * e:.2e}")
    assert abs(float(d.mean())) <= 1e-6 and abs(float(d.std()) - 1) <= 1e-6
    assert pc.l2_rel(d, ref) <= MARGIN * e


# ----------------------------------------------------------------------------------------------- generator
def _agree(a, ref):
    a, ref = a.double().flatten(), ref.double().flatten()
    return float((a - ref).norm() / ref.norm()), float((a * ref).sum() / (a.norm() * ref.norm()))


def test_generator_noise_gradients_against_the_reference_float64(g2s, fx):
    """Size-16 generator of the fixture, B = 1, one-node path: image, latent gradient and every noise-map gradient
    against the reference's float64 run, each within 4 x the reference's own float32 error.  (On the parent commit the
    node returned no gradient for the maps and torch.autograd.grad raised.)"""
    from gan2shape_amd import stylegan2 as sg2, synthesis
    G = pc.fixture_generator(sg2).cuda()
    w, noises, gy = pc.generator_inputs()
    w = torch.from_numpy(w).cuda().requires_grad_(True)
    nz = _cuda(noises, grad=True)
    calls = []
    orig = synthesis.synthesize
    synthesis.synthesize = lambda *a: calls.append(1) or orig(*a)
    try:
        img, _ = G([w], input_is_w=True, noise=nz)
    finally:
        synthesis.synthesize = orig
    assert calls == [1]                                            # the one-node path took it
    grads = torch.autograd.grad(img, [w] + nz, torch.from_numpy(gy).cuda())
    ref = torch.from_numpy(fx["g16.img"]).cuda()
    measured = {"img": float((img.detach().double() - ref).abs().max() / ref.abs().max()),
                "gw": pc.l2_rel(grads[0], torch.from_numpy(fx["g16.gw"]).cuda())}
    for k in range(len(nz)):
        measured[f"gnoise{k}"] = pc.l2_rel(grads[1 + k], torch.from_numpy(fx[f"g16.gnoise{k}"]).cuda())
    allowed = {k: MARGIN * float(fx[f"g16.ref_fp32_err.{k}"]) for k in measured}
    print("[G(16) one node vs float64] " + " ".join(f"{k} {measured[k]:.2e}/{allowed[k]:.2e}" for k in measured))
    for k in measured:
        assert measured[k] <= allowed[k], k


def _grads_both_ways(G, sg2, latent0, noises0, gy, mask=None):
    """{one_node: (image, [latent gradient, map gradients...])}; mask[i] False: map i asks for no gradient."""
    out = {}
    try:
        for one in (True, False):
            sg2.Generator.ONE_NODE = one
            lat = latent0.clone().requires_grad_(True)
            nz = [n.clone().requires_grad_(mask is None or mask[i]) for i, n in enumerate(noises0)]
            img, _ = G([lat], input_is_w=True, noise=nz)
            img.backward(gy)
            out[one] = (img.detach(), [lat.grad] + [n.grad for n in nz])
    finally:
        sg2.Generator.ONE_NODE = True
    return out


@pytest.mark.parametrize("w_plus", [False, True])
def test_generator_noise_gradients_one_node_equals_the_layer_loop(g2s, w_plus):
    """Size 64, B = 1: the one-node path against the op-by-op layer loop under test_generator_one_node_equals_op_by_op's
    bounds (image 2e-6 of max; gradients L2 1.5e-3, cosine >= 0.999999), for the latent — one w, or one per layer — and
    for each noise map; a map that asks for no gradient gets None."""
    from gan2shape_amd import stylegan2 as sg2
    G = pc.fixture_generator(sg2, size=64, style_dim=512, n_mlp=8, seed=77).cuda()
    g = torch.Generator().manual_seed(11)
    latent = 0.5 * torch.randn(1, 512, generator=g)
    if w_plus:
        latent = latent[:, None] + 0.2 * torch.randn(1, G.n_latent, 512, generator=g)
    noises = [torch.randn(n.shape, generator=g).cuda() for n in G.make_noise()]
    gy = torch.randn(1, 3, 64, 64, generator=g).cuda()
    mask = [i != 2 for i in range(len(noises))] if w_plus else None
    out = _grads_both_ways(G, sg2, latent.cuda(), noises, gy, mask)
    (img1, g1), (img0, g0) = out[True], out[False]
    e_img = float((img1 - img0).abs().max() / img0.abs().max())
    print(f"[G(64) noise gradients, w_plus {w_plus}] image {e_img:.2e}")
    assert e_img <= 2e-6
    assert g1[0].shape == latent.shape
    for i, (a, b) in enumerate(zip(g1, g0)):
        if i > 0 and mask is not None and not mask[i - 1]:
            assert a is None and b is None
            continue
        rel, cos = _agree(a, b)
        print(f"    {'latent' if i == 0 else f'map {i - 1}'}: rel {rel:.2e} cosine {cos:.9f}")
        assert a.shape == b.shape and rel <= 1.5e-3 and cos >= 0.999999, i


def test_per_sample_noise_takes_the_layer_loop_and_shared_maps_keep_their_bits(g2s):
    """B = 2 with [2, 1, H, W] maps: every sample gets ITS map (the one-node path's kernels read one map, so these calls
    take the layer loop) — equal to the layer loop run sample by sample.  The project's own case, [1, 1, H, W] maps
    without a gradient at B = 3, stays the one-node forward bit for bit in deterministic mode: explicit maps equal to
    the generator's buffers give the image the buffers give, and maps that require a gradient do not change the forward."""
    from gan2shape_amd import lib, stylegan2 as sg2
    G = pc.fixture_generator(sg2).cuda()
    g = torch.Generator().manual_seed(4)
    w = torch.randn(2, pc.G_CFG["style_dim"], generator=g).cuda()
    maps = [torch.randn(2, 1, s, s, generator=g).cuda() for s in (4, 8, 8, 16, 16)]
    with torch.no_grad():
        img, _ = G([w], input_is_w=True, noise=maps)
        try:
            sg2.Generator.ONE_NODE = False
            each = torch.cat([G([w[i:i + 1]], input_is_w=True, noise=[m[i:i + 1] for m in maps])[0] for i in range(2)])
        finally:
            sg2.Generator.ONE_NODE = True
    assert float((img - each).abs().max()) <= 2e-6 * float(each.abs().max())
    assert float((img[0] - img[1]).abs().max()) > 1e-3 * float(each.abs().max())
    # gradients reach per-sample maps through the layer loop
    pm = [m.clone().requires_grad_(True) for m in maps]
    gp = torch.autograd.grad(G([w], input_is_w=True, noise=pm)[0].sum(), pm)
    assert all(a.shape == m.shape and float(a.abs().max()) > 0 for a, m in zip(gp, maps))

    w3 = torch.randn(3, pc.G_CFG["style_dim"], generator=g).cuda()
    buffers = [getattr(G.noises, f"noise_{i}") for i in range(G.num_layers)]
    prev = lib.set_deterministic(True)
    try:
        with torch.no_grad():
            base, _ = G([w3], input_is_w=True, randomize_noise=False)
            again, _ = G([w3], input_is_w=True, noise=[b.clone() for b in buffers])
        with_grad, _ = G([w3], input_is_w=True, noise=[b.clone().requires_grad_(True) for b in buffers])
    finally:
        lib.set_deterministic(prev)
    assert torch.equal(base, again) and torch.equal(base, with_grad.detach())


# ----------------------------------------------------------------------------------------------- the projector
def _percept():
    """LPIPS with a seeded random trunk (no pretrained weights offline) and non-negative `lin` weights: a distance."""
    from gan2shape_amd.lpips import PerceptualLoss
    torch.manual_seed(7)
    p = PerceptualLoss()
    with torch.no_grad():
        for k in range(5):
            getattr(p.net, f"lin{k}").model[-1].weight.abs_()
    return p.cuda()


def test_one_projector_step_against_the_op_by_op_step(g2s):
    """Step 0 of the projector at G(64) (jitter strength 0): total loss, latent gradient and every noise-map gradient of
    the fused path (one-node generator with noise gradients, g2s_noise_regularize) against the op-by-op step (ONE_NODE
    off, the torch noise functions of tests/projector_cases.py).  Gradient bounds as for the generator above; the loss
    is two float32 evaluations of a sum the regulariser dominates: 4 x 4.2e-7 (the device's bound) + 4.2e-7 (torch's own
    float32 error, both from the fixture) = 2.1e-6, held to 1e-5.  Parameters after Adam are not compared."""
    from gan2shape_amd import projector, stylegan2 as sg2
    G = pc.fixture_generator(sg2, size=64, style_dim=512, n_mlp=8, seed=77).cuda()
    percept = _percept()
    g = torch.Generator().manual_seed(21)
    target, _ = G([(0.5 * torch.randn(1, 512, generator=g)).cuda()], input_is_w=True)
    latent0 = (0.1 * torch.randn(1, 512, generator=g)).cuda()
    noises0 = [torch.randn(n.shape, generator=g).cuda() for n in G.make_noise()]
    projector.noise_normalize_(noises0)
    res = {}
    try:
        for fused in (True, False):
            sg2.Generator.ONE_NODE = fused
            leaf = latent0.clone().requires_grad_(True)
            lat = projector.latent_noise(leaf, 0.0)
            nz = [n.clone().requires_grad_(True) for n in noises0]
            reg = projector.noise_regularize(nz) if fused else pc.noise_regularize(nz)
            loss = percept(projector._generate(G, lat, nz), target).sum() + 1e5 * reg
            res[fused] = (loss.detach(), torch.autograd.grad(loss, [leaf] + nz))
    finally:
        sg2.Generator.ONE_NODE = True
    (l1, g1), (l0, g0) = res[True], res[False]
    e_loss = abs(float(l1) - float(l0)) / abs(float(l0))
    print(f"[projector step 0] loss {float(l1):.6e} vs {float(l0):.6e}: rel {e_loss:.2e}")
    assert e_loss <= 1e-5
    for i, (a, b) in enumerate(zip(g1, g0)):
        rel, cos = _agree(a, b)
        print(f"    {'latent' if i == 0 else f'map {i - 1}'}: rel {rel:.2e} cosine {cos:.9f}")
        assert rel <= 1.5e-3 and cos >= 0.999999, i


def test_projection_lowers_its_loss_and_round_trips_through_the_dataset(g2s, tmp_path):
    """G(32) with deterministic weights, target = G(w*) with G's own noise buffers, w* = mean + 0.5 randn: 40 steps
    lower the perceptual term (no jitter) from where the projection starts; the maps end normalised; the saved file
    loads through LatentDataset and G reproduces the returned image from it."""
    from gan2shape_amd import dataset, projector, stylegan2 as sg2
    G = pc.fixture_generator(sg2, size=32, style_dim=512, n_mlp=8, seed=77).cuda()
    percept = _percept()
    gen = torch.Generator(device="cuda").manual_seed(5)
    stats = projector.mean_latent_stats(G, n=2000, generator=gen)
    with torch.no_grad():
        target, _ = G([stats[0][None] + 0.5 * torch.randn(1, 512, device="cuda", generator=gen)], input_is_w=True)
    state = gen.get_state()
    start = [n.normal_(generator=gen) for n in G.make_noise()]      # the maps project draws first
    before = float(projector.evaluate(G, percept, target, stats[0], start))
    gen.set_state(state)
    res = projector.project(G, percept, target, steps=40, latent_stats=stats, generator=gen)
    after = float(projector.evaluate(G, percept, target, res["latent"], res["noise"]))
    print(f"[projection G(32), 40 steps] perceptual {before:.5f} -> {after:.5f}")
    assert np.isfinite(after) and after < before
    assert res["latent"].shape == (512,) and res["history"] == [] and res["img"].shape == (1, 3, 32, 32)
    for n in res["noise"]:
        d = n.double()
        assert abs(float(d.mean())) <= 1e-5 and abs(float(d.std()) - 1) <= 1e-5
    root = str(tmp_path)
    with open(os.path.join(root, "list.txt"), "w") as f:
        f.write("photo.png\n")
    path = projector.save_projection(root, "photo.png", res)
    latent = dataset.LatentDataset(root)[0]
    stored = torch.load(path, weights_only=True)["photo.png"]
    with torch.no_grad():
        img, _ = G([latent[None].cuda()], input_is_w=True, noise=[n.cuda() for n in stored["noise"]])
    assert float((img - res["img"]).abs().max()) <= 2e-6 * float(res["img"].abs().max())
    assert torch.equal(stored["img"], res["img"][0].cpu())
