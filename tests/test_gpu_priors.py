"""-m gpu: the depth priors built on the device (PriorGenerator(on_device=True), csrc/priors.hip,
include/g2s.h g2s_prior_*) against the reference fixtures of tests/golden/model.npz, against the host path,
image by image, from run to run, inside a captured HIP graph, and through the trainers.

Bounds.  The fixtures and the host path are compared at the bound the project already holds the host path
to (test_host_cpu.test_priors_golden: rtol 2e-6, atol 1e-6, i.e. 2.8e-6 - 3.0e-6 over [near, far]).  box,
masked_box and confidence are single fp32 expressions restated operation by operation: bit-equal to the
host path (rtol 0).  An fp32 restatement of the kernels' summation order, run on a CPU, sits 1.8e-6 - 1.9e-6
from the two smoothed fixtures and 6e-8 from the ellipsoid ones (torch's CPU sqrt is not always correctly
rounded; the kernel's is); each test prints the figure it measured before it asserts.
"""
import math

import numpy as np
import pytest
import torch

import priors_cases as pc
from model_cases import PRIOR_NAMES, FakeMaskingModel

pytestmark = pytest.mark.gpu

MAPS = ("box", "masked_box", "confidence")


@pytest.fixture(scope="module")
def g2s():
    import gan2shape_amd  # noqa: F401
    from gan2shape_amd import lib
    lib.load()
    return lib


def _gen(name, size, source=None, **kw):
    from gan2shape_amd import priors
    return priors.PriorGenerator(size, "face", name, masking_model=source, **kw)


def _close(got, want, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    err = np.abs(got - want)
    print(f"{what}: max abs {err.max():.3e}, max of err / (atol + rtol |want|) "
          f"{(err / (pc.ATOL + pc.RTOL * np.abs(want))).max():.3f}")
    np.testing.assert_allclose(got, want, rtol=pc.RTOL, atol=pc.ATOL, err_msg=what)


# ------------------------------------------------------------------------------------- 1. reference fixtures
def test_device_priors_equal_the_reference_fixtures(golden, g2s):
    g = golden("model")
    keys = sorted(k for k in g if k.startswith("p."))
    assert len(keys) == 8
    for key in keys:
        _, name, size = key.split(".")
        size = int(size)
        fm = FakeMaskingModel(size)
        source = fm.confidence_mask if "confidence" in name else fm
        img = torch.zeros(1, 3, size, size, device="cuda")
        p = _gen(name, size, source, on_device=True)(img, device="cuda")
        assert p.shape == (1, size, size) and p.is_cuda and p.dtype == torch.float32
        p = p.cpu().numpy()
        _close(p, g[key], key)
        if name in MAPS:
            host = _gen(name, size, source)(img.cpu(), device="cpu").numpy()
            np.testing.assert_array_equal(p, host, err_msg=key)
        elif name == "ellipsoid":
            _close(p[0], pc.ellipsoid64(fm.mask[0, 0].numpy()), key + " vs float64")
        else:
            base = _gen(pc.SMOOTHED_FROM[name], size, source)(img.cpu(), device="cpu")[0].numpy()
            _close(p[0], pc.smooth64(base), key + " vs float64")


# ------------------------------------------------------------------------------------- 2. batch
@pytest.mark.parametrize("size", [64, 96, 128, 256])
def test_batch_equals_single_images_bitwise_and_the_host_path(size, g2s):
    """Five different masks (one ellipse runs over the image border): nothing leaks between the images of a
    batch, a list of images equals a batch tensor, and every image agrees with the host path."""
    masks = pc.batch_masks(size)
    images = pc.images_of(masks).cuda()
    for name in PRIOR_NAMES:
        source = (lambda im: pc.first_channel(im) ** 2) if "confidence" in name else pc.first_channel
        gen = _gen(name, size, source, on_device=True)
        out = gen.batch(images, device="cuda")
        assert out.shape == (5, size, size)
        listed = gen.batch([images[i:i + 1] for i in range(5)], device="cuda")
        whole = _gen(name, size, source, on_device=True, mask_accepts_batch=True).batch(images, device="cuda")
        assert torch.equal(out, listed) and torch.equal(out, whole), name
        host = _gen(name, size, source)
        for i in range(5):
            alone = gen(images[i:i + 1], device="cuda")
            assert alone.shape == (1, size, size)
            assert torch.equal(out[i:i + 1], alone), (name, i)
            want = host(images[i:i + 1].cpu(), device="cpu").numpy()
            if name in MAPS:
                np.testing.assert_array_equal(out[i:i + 1].cpu().numpy(), want, err_msg=f"{name} {i}")
            else:
                _close(out[i:i + 1].cpu().numpy(), want, f"{name} S={size} image {i} vs host")
        if name not in MAPS:
            assert not torch.equal(out[0], out[1])
    assert _gen("ellipsoid", size, pc.first_channel, on_device=True).batch(images[:0], device="cuda").shape == (0, size, size)


# ------------------------------------------------------------------------------------- 3. run to run
@pytest.mark.parametrize("deterministic", [False, True])
def test_two_runs_are_bit_equal(deterministic, g2s):
    prev = g2s.set_deterministic(deterministic)
    try:
        for size in (96, 256):
            images = pc.images_of(pc.batch_masks(size)).cuda()
            for name in ("smoothed_box", "ellipsoid"):
                gen = _gen(name, size, pc.first_channel, on_device=True)
                a = gen.batch(images, device="cuda")
                for _ in range(3):
                    assert torch.equal(a, gen.batch(images, device="cuda")), (name, size)
    finally:
        g2s.set_deterministic(prev)


# ------------------------------------------------------------------------------------- 4. degenerate masks
def _smooth_raw(g2s, x, taps, passes, near=pc.NEAR, far=pc.FAR):
    L = g2s.load()
    B, S, _ = x.shape
    out = torch.empty_like(x)
    ws = torch.empty(max(L.g2s_prior_smooth_workspace_bytes(B, S, taps, passes), 1), dtype=torch.uint8, device="cuda")
    g2s.check(L.g2s_prior_smooth(g2s.ptr(x), B, S, taps, passes, near, far, g2s.ptr(out), g2s.ptr(ws), ws.numel(),
                                 g2s.stream()))
    return out


def test_degenerate_masks(g2s):
    """Stated in include/g2s.h: `ellipsoid` gives `far` everywhere for an image without a pixel at or above
    the threshold and for a bounding box of zero width or height (the host path raises / divides by zero),
    while the other images of the batch are untouched; a constant filtered map (hi == lo, 0 / 0 on the host)
    rescales to `near`."""
    S = 64
    far32, near32 = np.float32(pc.FAR), np.float32(pc.NEAR)
    masks = pc.batch_masks(S)[:4].clone()
    masks[1] = 0                                   # empty
    masks[2] = 0
    masks[2, 0, 10:40, 17] = 1.0                   # one column
    masks[3] = 0
    masks[3, 0, 23, 5:50] = 0.7                    # one row, exactly at the threshold
    images = pc.images_of(masks).cuda()
    gen = _gen("ellipsoid", S, pc.first_channel, on_device=True)
    out = gen.batch(images, device="cuda").cpu().numpy()
    for i in (1, 2, 3):
        assert (out[i] == far32).all(), i
    alone = gen(images[:1], device="cuda").cpu().numpy()
    np.testing.assert_array_equal(out[:1], alone)
    assert out[0].min() < 0.92

    # constant mask through smoothed_confidence: pass 1 has hi == lo -> `near` inside, `far` on the border of
    # width 5; the remaining two passes smooth that map as usual
    const = torch.full((2, 1, S, S), 0.25)
    const[1] = 1.0                                 # far - far * 1 = 0 everywhere
    got = _gen("smoothed_confidence", S, pc.first_channel, on_device=True).batch(pc.images_of(const).cuda(), device="cuda")
    assert torch.isfinite(got).all()
    flat = torch.full((2, S, S), float(far32), device="cuda")
    one = _smooth_raw(g2s, flat * 0.5, pc.TAPS, 1)
    want1 = flat.clone()
    want1[:, 5:S - 5, 5:S - 5] = float(near32)
    assert torch.equal(one, want1)
    assert torch.equal(got, _smooth_raw(g2s, want1, pc.TAPS, 2))
    _close(got[0].cpu().numpy(), pc.smooth64(want1[0].cpu().numpy(), passes=2), "constant mask, passes 2 and 3 vs float64")
    # passes = 0 copies; taps = S leaves one filtered value per image, hence `near` at ... nowhere but the centre
    x = torch.rand(3, 17, 17, device="cuda")
    assert torch.equal(_smooth_raw(g2s, x, 3, 0), x)
    centre = _smooth_raw(g2s, x, 17, 2)
    want = torch.full_like(x, float(far32))
    want[:, 8, 8] = float(near32)
    assert torch.equal(centre, want)


@pytest.mark.parametrize("size,taps", [(16, 5), (37, 5), (250, 11)])
def test_smoothing_other_sizes_against_float64(size, taps, g2s):
    """S from 16 to 256, not only powers of two, against the float64 restatement.  The direct sums are at most
    a few 1e-7 from it; the bound is the fixtures' bound.  (S = 16 with 11 taps is no case: from the second
    pass on every 11 x 11 window holds the whole 6 x 6 interior and border otherwise, all filtered values are equal
    in exact arithmetic, and the rescale divides rounding noise by rounding noise — on the host as well.)"""
    rng = np.random.default_rng(size)
    x = (pc.FAR * rng.random((3, size, size))).astype(np.float32)
    got = _smooth_raw(g2s, torch.from_numpy(x).cuda(), taps, 3).cpu().numpy()
    for i in range(3):
        _close(got[i], pc.smooth64(x[i], taps=taps), f"S={size} taps={taps} image {i} vs float64")


# ------------------------------------------------------------------------------------- 5. no synchronisation
@pytest.mark.parametrize("name", ["ellipsoid", "smoothed_box"])
def test_device_path_is_capturable_and_replays_on_new_masks(name, g2s):
    """A host synchronisation during a capture makes the capture fail.  The replay reads the mask buffer as
    it is then: after the buffer was overwritten with other masks it reproduces the eager result bitwise."""
    S = 128
    masks = pc.batch_masks(S).cuda()
    buf = masks[:3].clone()
    gen = _gen(name, S, lambda image: buf, on_device=True, mask_accepts_batch=True)
    images = torch.zeros(3, 3, S, S, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        first = gen.batch(images, device="cuda").clone()          # warm-up: code objects
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        captured = gen.batch(images, device="cuda")
    buf.copy_(masks[2:5])
    graph.replay()
    torch.cuda.synchronize()
    replayed = captured.clone()
    eager = gen.batch(images, device="cuda")
    torch.cuda.synchronize()
    assert torch.equal(replayed, eager)
    assert not torch.equal(replayed, first) and torch.equal(replayed[0], first[2])


# ------------------------------------------------------------------------------------- 6. C ABI validation
def test_rejected_arguments_launch_nothing(g2s):
    L = g2s.load()
    S, B, SENTINEL = 32, 2, -7.5
    x = torch.rand(B, S, S, device="cuda")
    out = torch.full((B, S, S), SENTINEL, device="cuda")
    ws = torch.full((1 << 20,), 0x5A, dtype=torch.uint8, device="cuda")
    p, st, n = g2s.ptr, g2s.stream, ws.numel()

    def smooth(x_=x, B_=B, S_=S, taps=11, passes=3, near=pc.NEAR, far=pc.FAR, out_=out, ws_=ws, n_=n):
        return L.g2s_prior_smooth(p(x_), B_, S_, taps, passes, near, far, p(out_), p(ws_), n_, st())

    def ellipsoid(m=x, radius=pc.RADIUS, near=pc.NEAR, far=pc.FAR, out_=out, ws_=ws, n_=n):
        return L.g2s_prior_ellipsoid(p(m), B, S, pc.THRESHOLD, radius, near, far, p(out_), p(ws_), n_, st())
    rejected = [
        (lambda: smooth(taps=10), -1, "taps"), (lambda: smooth(taps=33), -1, "taps"), (lambda: smooth(taps=-1), -1, "taps"),
        (lambda: smooth(passes=-1), -1, "passes"), (lambda: smooth(near=pc.FAR), -1, "near"),
        (lambda: smooth(near=1.5), -1, "near"), (lambda: smooth(x_=None), -1, "NULL"),
        (lambda: smooth(out_=None), -1, "NULL"), (lambda: smooth(ws_=None), -3, "workspace"),
        (lambda: smooth(n_=64), -3, "workspace"), (lambda: smooth(B_=-1), -1, "B ="), (lambda: smooth(S_=0), -1, "S ="),
        (lambda: L.g2s_prior_map(None, B, S, 1, pc.THRESHOLD, pc.FAR, p(out), st()), -1, "NULL"),
        (lambda: L.g2s_prior_map(p(x), B, S, 2, pc.THRESHOLD, pc.FAR, None, st()), -1, "NULL"),
        (lambda: L.g2s_prior_map(p(x), B, S, 5, pc.THRESHOLD, pc.FAR, p(out), st()), -1, "kind"),
        (lambda: ellipsoid(m=None), -1, "NULL"), (lambda: ellipsoid(out_=None), -1, "NULL"),
        (lambda: ellipsoid(near=pc.FAR), -1, "near"), (lambda: ellipsoid(radius=0.0), -1, "radius"),
        (lambda: ellipsoid(ws_=None), -3, "workspace"), (lambda: ellipsoid(n_=B * 16 - 1), -3, "workspace"),
    ]
    for call, code, word in rejected:
        rc = call()
        assert rc == code and word in L.g2s_last_error().decode(), (rc, code, word, L.g2s_last_error())
        with pytest.raises(g2s.G2SError):
            g2s.check(rc)
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()) and bool((ws == 0x5A).all())
    # B = 0 succeeds and writes nothing either
    assert smooth(B_=0) == 0 and L.g2s_prior_map(p(x), 0, S, 1, pc.THRESHOLD, pc.FAR, p(out), st()) == 0
    assert L.g2s_prior_ellipsoid(p(x), 0, S, pc.THRESHOLD, pc.RADIUS, pc.NEAR, pc.FAR, p(out), p(ws), n, st()) == 0
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()) and bool((ws == 0x5A).all())
    assert smooth() == 0                     # the accepted call does write
    torch.cuda.synchronize()
    assert not bool((out == SENTINEL).any())


# ------------------------------------------------------------------------------------- 7. trainers
def test_trainer_pretrains_on_device_priors():
    """Same initial weights, priors about 1e-6 apart: the first pre-training loss of the device-prior run
    equals the host-prior run's to 1e-5 relative."""
    import bench
    from gan2shape_amd.model import GAN2Shape
    from gan2shape_amd.trainer import Trainer
    dev = torch.device("cuda")
    losses = {}
    for on_device in (False, True):
        cfg = bench.face_config(n_proj=2)
        cfg.update(n_epochs_prior=3, prior_on_device=on_device)
        torch.manual_seed(0)
        t = Trainer(GAN2Shape, cfg, device=dev)
        assert t.prior_generator.on_device is on_device
        image, _latent = bench.synthetic_sample(t.model, 1234, dev)
        losses[on_device] = t.pretrain_on_prior(image, 0)
        prior = t.prior_generator(image, device=dev)
        assert prior.is_cuda and prior.shape == (1, t.image_size, t.image_size)
    print("pre-training losses, host priors %s, device priors %s" % (losses[False], losses[True]))
    assert len(losses[True]) == 3 and all(math.isfinite(v) for v in losses[True])
    assert abs(losses[True][0] - losses[False][0]) <= 1e-5 * abs(losses[False][0])


def test_joint_trainer_builds_its_priors_in_batches():
    """pretrain_on_prior_all with prior_on_device: four images in chunks of batch_size = 2 -> two calls of
    `batch`, four calls of the mask source, no per-image call of the generator."""
    import bench
    from gan2shape_amd import priors
    from gan2shape_amd.model import GAN2Shape
    from gan2shape_amd.trainer import GeneralizingTrainer2
    dev = torch.device("cuda")
    cfg = bench.face_config(n_proj=2)
    cfg.update(n_epochs_prior=1, n_epochs_generalized=1, prior_on_device=True)
    calls = {"mask": 0, "batch": []}

    def mask_source(image):
        calls["mask"] += 1
        assert image.shape[0] == 1 and image.is_cuda
        return priors.synthetic_mask(image)

    torch.manual_seed(0)
    t = GeneralizingTrainer2(GAN2Shape, cfg, masking_model=mask_source, device=dev)
    gen = t.prior_generator
    assert gen.on_device and gen.masking_model is mask_source
    batch0 = gen.batch

    def counting_batch(images, device='cuda'):
        calls["batch"].append(len(images))
        return batch0(images, device=device)
    gen.batch = counting_batch
    data = []
    for i in range(4):
        image, latent = bench.synthetic_sample(t.model, 100 + i, dev)
        data.append((image[0].cpu(), latent[0].cpu(), i))
    loss = t.pretrain_on_prior_all(data, 2)
    assert math.isfinite(loss)
    assert calls["batch"] == [2, 2] and calls["mask"] == 4
    # the host-side default builds the same four priors one by one
    cfg.update(prior_on_device=False)
    torch.manual_seed(0)
    t2 = GeneralizingTrainer2(GAN2Shape, cfg, masking_model=mask_source, device=dev)
    calls["mask"] = 0
    loss2 = t2.pretrain_on_prior_all(data, 2)
    assert calls["mask"] == 4 and not t2.prior_generator.on_device
    print(f"joint pre-training loss after one epoch: device priors {loss}, host priors {loss2}")
    assert math.isfinite(loss2)
