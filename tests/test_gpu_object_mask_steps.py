"""Object masks inside steps 1-3 on the GPU (config `object_mask`): the model of
tests/model_cases.STEP_CFG (128 x 128, channel multiplier 1, n_proj = 2; seeded nets, the smooth depth net) with
the switch off, on, with flips, through both routes of the renderer and through HIP graphs.

Tolerances.  Fused against composed: the form tests/test_gpu_model.py holds that pair to where the quantity sits
downstream of a sampling grid (test_fused_normal_and_shading_match_torch_path: rtol 1e-4, atol 1e-5 (1 + |value|)).
Graphs against eager: test_trainer_fit_with_hip_graphs' 5e-3 of the step-1 losses (the draws of steps 2 / 3 differ
between a replay and an eager call, so only step 1 is comparable, as there)."""
import math

import pytest
import torch

import model_cases as mc

pytestmark = pytest.mark.gpu

S = mc.STEP_CFG["image_size"]


def disc(cx=0.55, cy=0.45, r=0.3, batch=1):
    yy, xx = torch.meshgrid(torch.linspace(0, 1, S), torch.linspace(0, 1, S), indexing="ij")
    m = (((xx - cx) ** 2 + (yy - cy) ** 2) < r * r).float()
    return m[None, None].expand(batch, 1, S, S).contiguous().cuda()


def build(**over):
    import bench
    from gan2shape_amd.model import GAN2Shape
    cfg = bench.face_config(n_proj=mc.STEP_CFG["n_proj"])
    cfg.update(over)
    torch.manual_seed(0)
    m = GAN2Shape(cfg, device="cuda")
    for name in m.NETS:
        mc.fill_scaled(getattr(m, f"{name}_net"), mc.STEP_CFG["seeds"][name])
    mc.smooth_depth_net(m.depth_net)
    return m


@pytest.fixture(scope="module")
def deterministic():
    from gan2shape_amd import lib
    prev = lib.set_deterministic(True)      # the nets' forwards repeat bit for bit from call to call
    yield
    lib.set_deterministic(prev)


@pytest.fixture(scope="module")
def sample(golden):
    g = golden("steps")
    draws = tuple(torch.tensor(g[f"s2.draw.{k}"]).cuda() for k in ("dxy", "rand", "views"))
    return torch.tensor(g["image"]).cuda(), torch.tensor(g["latent"]).cuda(), draws


@pytest.fixture(scope="module")
def m_on(deterministic):
    return build(object_mask=True)


def test_switch_off_changes_nothing(deterministic, sample):
    image, latent, _ = sample
    plain = build()
    assert not plain.masks_live and "object_mask" not in __import__("bench").face_config()
    with torch.no_grad():
        loss0, c0 = plain.forward_step1(image, latent, None)
        loss0m, c0m = plain.forward_step1(image, latent, None, object_mask=disc())     # given, but the switch is off
    assert c0[-1] is None and c0m[-1] is None and torch.equal(loss0, loss0m)
    for over in (dict(object_mask=False), dict(object_mask=True, use_mask=False)):
        m = build(**over)
        assert not m.masks_live
        with torch.no_grad():
            loss, c = m.forward_step1(image, latent, None)
            _, cb = m.forward_step1(torch.cat([image, image.flip(3)]), None, None)
        assert c[-1] is None and cb[-1] == [None, None]
        assert torch.equal(loss, loss0), (over, float(loss), float(loss0))
        for a, b in zip(c[:5], c0[:5]):
            assert torch.equal(a, b)
    assert plain.use_mask is True and plain.object_mask is False       # use_mask alone switches nothing on


def test_switch_on_puts_the_canonical_mask_into_collected(m_on, sample):
    image, latent, _ = sample
    mask = disc()
    assert m_on.masks_live
    with torch.no_grad():
        loss, c = m_on.forward_step1(image, latent, None, object_mask=mask)
        want = m_on.renderer.canon_mask(c[4], mask)       # the renderer still holds the step's view
    assert torch.is_tensor(c[-1]) and tuple(c[-1].shape) == (1, 1, S, S) and c[-1].grad_fn is None
    assert torch.equal(c[-1], want)
    assert 0.05 < float(c[-1].mean()) < 0.95 and not torch.equal(c[-1], mask)      # a mask, and a warped one
    # the step's own loss terms do not read it
    with torch.no_grad():
        loss_ones, _ = m_on.forward_step1(image, latent, None, object_mask=torch.ones_like(mask))
    assert torch.equal(loss, loss_ones)
    # a batch: a list of (1,1,S,S), each sample's own mask under its own view
    images = torch.cat([image, image.flip(3)])
    masks = torch.cat([mask, disc(0.4, 0.6, 0.25)])
    with torch.no_grad():
        _, cb = m_on.forward_step1(images, None, None, object_mask=masks)
        wantb = m_on.renderer.canon_mask(cb[4], masks)
    assert isinstance(cb[-1], list) and len(cb[-1]) == 2
    for i in range(2):
        assert tuple(cb[-1][i].shape) == (1, 1, S, S) and torch.equal(cb[-1][i], wantb[i:i + 1])
    assert not torch.equal(cb[-1][0], cb[-1][1])


def test_step2_mask_is_cut_by_the_object_mask(m_on, sample):
    image, latent, draws = sample
    got = {}
    for name, mask in (("disc", disc()), ("ones", torch.ones(1, 1, S, S, device="cuda"))):
        with torch.no_grad():
            _, c1 = m_on.forward_step1(image, latent, None, object_mask=mask)
            _, (projected, m2) = m_on.forward_step2(image, latent, c1, n_proj_samples=draws[2].shape[0], _draws=draws)
        assert tuple(m2.shape) == (draws[2].shape[0], 1, S, S)
        got[name] = m2
    assert not torch.equal(got["disc"], got["ones"])
    assert bool((got["disc"] <= got["ones"]).all())
    assert float(got["disc"].mean()) < 0.9 * float(got["ones"].mean())


def test_fused_and_composed_routes_agree_on_the_losses(m_on, sample):
    image, latent, draws = sample
    mask = disc()
    losses = {}
    try:
        for fused in (True, False):
            m_on.renderer.fused = fused
            with torch.no_grad():
                l1, c1 = m_on.forward_step1(image, latent, None, object_mask=mask)
                l2, c2 = m_on.forward_step2(image, latent, c1, n_proj_samples=draws[2].shape[0], _draws=draws)
                l3, _ = m_on.forward_step3(image, latent, c2, object_mask=mask)
            losses[fused] = (l1, l2, l3)
    finally:
        m_on.renderer.fused = True
    for k, (a, b) in enumerate(zip(losses[True], losses[False]), 1):
        print(f"[object mask] step {k}: fused {float(a):.8f} composed {float(b):.8f} relative difference "
              f"{abs(float(a) - float(b)) / abs(float(b)):.2e}")
    for a, b in zip(losses[True], losses[False]):
        torch.testing.assert_close(a, b, rtol=1e-4, atol=1e-5 * (1 + float(b.abs())))


def test_flips_leave_the_canonical_mask_alone(m_on, sample):
    image, latent, _ = sample
    mask = disc()
    got = {}
    try:
        for flip in (False, True):
            m_on.flip1 = m_on.flip3 = flip
            with torch.no_grad():
                _, c = m_on.forward_step1(image, latent, None, object_mask=mask)                     # flip1
                _, c3 = m_on.forward_step1(image, None, None, step1=False, object_mask=mask)        # flip3's inner pass
            got[flip] = (c[-1], c3[-1])
    finally:
        m_on.flip1 = m_on.flip3 = False
    for off, on in zip(got[False], got[True]):
        assert torch.is_tensor(on) and torch.equal(on, off)


def test_missing_mask_raises(m_on, sample):
    image, latent, draws = sample
    with pytest.raises(ValueError, match="object_mask"):
        m_on.forward_step1(image, latent, None)
    c2 = (image.expand(2, 3, S, S).contiguous(), torch.ones(2, 1, S, S, device="cuda"))
    with pytest.raises(ValueError, match="object_mask"):
        m_on.forward_step3(image, latent, c2)
    with torch.no_grad():       # evaluation takes no mask
        m_on.evaluate_results(image)


def test_trainer_without_a_mask_source_raises_at_construction():
    import bench
    from gan2shape_amd.model import GAN2Shape
    from gan2shape_amd.trainer import Trainer
    cfg = bench.face_config(n_proj=2)
    cfg.update(object_mask=True)
    with pytest.raises(ValueError, match="parsing_ckpt_dir"):
        Trainer(GAN2Shape, cfg, device="cuda")


def test_graphed_fit_with_object_masks_reproduces_eager(deterministic):
    """Trainer.fit(graphs=True) over two images with different masks: the mask is a static buffer of the graphs, made
    eagerly once per image; the history reproduces the eager run's."""
    import bench
    from gan2shape_amd.model import GAN2Shape
    from gan2shape_amd.trainer import Trainer
    dev = torch.device("cuda")
    torch.cuda.set_stream(torch.cuda.Stream(dev))     # captures need a non-default stream
    try:
        cfg = bench.face_config(n_proj=2)
        cfg.update(object_mask=True)
        stages = [{'step1': 4, 'step2': 4, 'step3': 4}]
        losses = {}
        for graphs in (False, True):
            calls = []

            def mask_fn(images, calls=calls):     # synthetic: a disc placed by the image's content
                shift = 0.1 * float(images[:, 0].mean().tanh())
                m = disc(0.5 + shift + 0.1 * len(calls), 0.5 - shift, 0.3 - 0.05 * len(calls), batch=len(images))
                calls.append(m)
                return m
            torch.manual_seed(0)
            t = Trainer(GAN2Shape, cfg, device=dev, capturable=True, object_mask_fn=mask_fn)
            data = []
            for i in range(2):
                image, latent = bench.synthetic_sample(t.model, 1234 + i, dev)
                data.append((image[0].cpu(), latent[0].cpu(), i))
            n = t.fit(data, stages=stages, graphs=graphs)
            assert n == 24 and len(calls) == 2 and not torch.equal(calls[0], calls[1])       # once per image
            losses[graphs] = [h[3] for h in t.history]
            assert all(math.isfinite(v) for v in losses[graphs])
        print("[object mask] history eager", losses[False], "graphed", losses[True])
        # step 1 is deterministic given the weights: its losses agree for both images (the second follows 12 iterations)
        for k in (0, 3):
            assert abs(losses[True][k] - losses[False][k]) < 5e-3 * abs(losses[False][k]), (losses[True], losses[False])
    finally:
        torch.cuda.set_stream(torch.cuda.default_stream(dev))
