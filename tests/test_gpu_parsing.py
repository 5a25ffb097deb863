"""-m gpu: the kernels of csrc/parsing.hip, the libg2s route of BiSeNet / PSPNet and MaskingModel on the device.
Oracles: float64 torch on the CPU, or tests/golden/parsing.npz (the reference's float64 results; weights regenerated
from the seed recipe of parsing_cases).

Tolerances.  Pools, resizes and the gate are single roundings or short sums: 1e-6 relative to max|y|.  The 7x7 stem
takes the direct convolution kernel's bound of tests/test_gpu_conv_tiles.py: rtol 2e-4, atol 2e-5 * max(1, sqrt(K /
1152)), K = 147.  Hard masks must equal the float64 oracle on every pixel whose float64 top-2 margin is at least
1e-4 * max|logit|; the test first asserts that the pixels below it are at most 0.1 % (a condition on the inputs, met
by the oracle alone).  Soft masks: (such pixels in the bin) / (bin area) + 1e-6 per output pixel.  Whole nets:
L2-relative logit error <= 4 x the reference's own float32-vs-float64 error (the margin the projector tests grant a
different summation order)."""
import itertools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import gan2shape_amd  # noqa: F401
from gan2shape_amd import parsing
from gan2shape_amd.priors import PriorGenerator

import parsing_cases as pc
from priors_cases import ATOL, FAR, RTOL, THRESHOLD

pytestmark = pytest.mark.gpu
DEV = "cuda"


def rel_close(got, want, tol=1e-6):
    want = want.double()
    err = float((got.double().cpu() - want).abs().max())
    print(f"max abs error {err:.3e}, bound {tol * float(want.abs().max()):.3e}")
    assert got.shape == want.shape
    assert err <= tol * float(want.abs().max())


# ----------------------------------------------------------------------------- kernels
@pytest.mark.parametrize("hw", [(9, 9), (10, 11), (40, 35)])
@pytest.mark.parametrize("relu,bias", [(True, True), (False, False)])
def test_conv_stem7(hw, relu, bias):
    """(40, 35): more than one 16 x 16 tile in each direction, with ragged edges."""
    rng = np.random.default_rng(sum(hw))
    x = torch.from_numpy(rng.standard_normal((2, 3, *hw)).astype(np.float32))
    w = torch.from_numpy((rng.standard_normal((64, 3, 7, 7)) / math.sqrt(147)).astype(np.float32))
    b = torch.from_numpy(rng.standard_normal(64).astype(np.float32)) if bias else None
    want = F.conv2d(x.double(), w.double(), None if b is None else b.double(), stride=2, padding=3)
    want = F.relu(want) if relu else want
    got = parsing.conv_stem7(x.to(DEV), w.to(DEV), None if b is None else b.to(DEV), relu).cpu()
    print("max abs error", float((got.double() - want).abs().max()))
    np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=2e-4, atol=2e-5 * max(1.0, math.sqrt(147 / 1152.0)))


def test_conv_stem7_channel_tail():
    """M = 20: the second group of 16 output channels is partly empty."""
    rng = np.random.default_rng(5)
    x = torch.from_numpy(rng.standard_normal((1, 3, 12, 9)).astype(np.float32))
    w = torch.from_numpy((rng.standard_normal((20, 3, 7, 7)) / math.sqrt(147)).astype(np.float32))
    want = F.conv2d(x.double(), w.double(), stride=2, padding=3)
    got = parsing.conv_stem7(x.to(DEV), w.to(DEV), None, False).cpu()
    np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=2e-4, atol=2e-5)


@pytest.mark.parametrize("hw", [(5, 5), (6, 6), (7, 9)])
def test_maxpool_all_negative(hw):
    """Every value is negative: padding with zeros instead of -inf would win the border windows."""
    rng = np.random.default_rng(hw[1])
    x = torch.from_numpy(-rng.uniform(0.5, 2.0, (2, 5, *hw)).astype(np.float32))
    got = parsing.maxpool3x3s2(x.to(DEV))
    assert torch.equal(got.cpu(), F.max_pool2d(x, 3, 2, 1))


@pytest.mark.parametrize("src,dst", [(5, 1), (5, 2), (5, 3), (5, 6), (7, 3), (65, 16), (13, 6)])
def test_adaptive_avgpool(src, dst):
    rng = np.random.default_rng(src * 10 + dst)
    x = torch.from_numpy(rng.standard_normal((2, 5, src, src + 1)).astype(np.float32))
    rel_close(parsing.adaptive_avgpool(x.to(DEV), (dst, dst)), F.adaptive_avg_pool2d(x.double(), (dst, dst)))


@pytest.mark.parametrize("src,dst,align", [(1, 7, True), (3, 8, True), (6, 13, True), (8, 32, False), (5, 12, False)])
def test_resize_bilinear(src, dst, align):
    rng = np.random.default_rng(src * 10 + dst)
    x = torch.from_numpy(rng.standard_normal((2, 5, src, src)).astype(np.float32))
    want = F.interpolate(x.double(), (dst, dst + 1), mode="bilinear", align_corners=align)
    rel_close(parsing.resize_bilinear(x.to(DEV), (dst, dst + 1), align), want)


@pytest.mark.parametrize("shape", [(2, 5, 3, 7), (2, 5, 2, 4)])        # scalar and float4 paths
def test_gate_add_act_every_combination(shape):
    rng = np.random.default_rng(3)
    x, r = [torch.from_numpy(rng.standard_normal(shape).astype(np.float32)) for _ in range(2)]
    s, t = [torch.from_numpy(rng.standard_normal(shape[:2] + (1, 1)).astype(np.float32)) for _ in range(2)]
    n = 0
    for has_s, has_t, has_r, sig, plus, relu in itertools.product((0, 1), repeat=6):
        if (sig or plus) and not has_s:
            continue
        g = s.double() if has_s else None
        if sig:
            g = torch.sigmoid(g)
        if plus:
            g = g + 1
        want = x.double() * g if has_s else x.double()
        want = want + (t.double() if has_t else 0) + (r.double() if has_r else 0)
        want = F.relu(want) if relu else want
        got = parsing.gate_add_act(x.to(DEV), s.to(DEV) if has_s else None, t.to(DEV) if has_t else None,
                                   r.to(DEV) if has_r else None, bool(sig), bool(plus), bool(relu))
        err = float((got.double().cpu() - want).abs().max())
        assert err <= 1e-6 * float(want.abs().max()), (has_s, has_t, has_r, sig, plus, relu, err)
        n += 1
    assert n == 40


# ----------------------------------------------------------------------------- parse head
def head_logits(C, h, size, S, drop, classes, no_class_in_sample_1=False):
    """Low-resolution logits (B = 2) built so that the float64 oracle ALONE meets the tests' conditions: seeds are
    tried in order until the pixels below the margin are at most half the cap, every sample that should have the
    class covers 2 % .. 98 % of the pixels, and the two samples differ.  Per-channel offsets plus noise, the first
    class favoured; with no_class_in_sample_1 that class lies below every other channel of sample 1."""
    for seed in range(100):
        rng = np.random.default_rng([C, h, size, seed])
        z = rng.standard_normal((2, C, h, h)) * 2.0 + rng.standard_normal((2, C, 1, 1))
        z[:, classes[0]] += 1.5
        low = torch.from_numpy(z.astype(np.float32))
        if no_class_in_sample_1:
            low[1, classes[0]] = low[1].min(0).values - 1.0
        full = pc.upsample64(low, size)
        mask, empty, margin, soft = pc.hard_oracle(full, drop, classes, S)
        cover = mask.double().flatten(1).mean(1)[~empty]
        if (float(pc.excluded_pixels(full, margin).double().mean()) <= pc.EXCLUDED_CAP / 2
                and empty.tolist() == [False, no_class_in_sample_1] and 0.02 < float(cover.min())
                and float(cover.max()) < 0.98 and not torch.equal(soft[0], soft[1])):
            return low
    raise AssertionError("no seed gives logits that meet the conditions")


HEAD_CASES = [  # C, h, size, S, category
    (19, 8, 32, 8, "face"),
    (21, 9, 65, 16, "car"),        # 65 -> 16: non-integer, overlapping area bins
]


@pytest.mark.parametrize("C,h,size,S,category", HEAD_CASES)
def test_parse_head_hard_and_confidence(C, h, size, S, category):
    drop, classes, channels = pc.rule_of(category)
    low = head_logits(C, h, size, S, drop, classes)
    full = pc.upsample64(low, size)
    mask, empty, margin, soft = pc.hard_oracle(full, drop, classes, S)
    excluded = pc.excluded_pixels(full, margin)
    share = float(excluded.double().mean())
    cover = mask.double().flatten(1).mean(1)
    print("excluded share", share, "coverage", cover.tolist())
    assert share <= pc.EXCLUDED_CAP
    assert not bool(empty.any()) and float(cover.min()) > 0.02 and float(cover.max()) < 0.98
    assert not torch.equal(soft[0], soft[1])                  # B = 2 with different answers per sample
    out, fm, flag = parsing.parse_head(low.to(DEV), size, S, parsing.PARSE_HARD, drop, pc.as_set(classes), True)
    assert flag.tolist() == [0, 0]
    keep = ~excluded[:, None]
    assert torch.equal(fm.cpu().bool()[keep], mask[keep])
    assert bool(((out.double().cpu() - soft).abs() <= pc.soft_bound(excluded, S)).all())
    out2, fm2, _ = parsing.parse_head(low.to(DEV), size, S, parsing.PARSE_HARD, drop, pc.as_set(classes), False)
    assert fm2 is None and torch.equal(out2, out)
    conf = parsing.parse_head(low.to(DEV), size, S, parsing.PARSE_CONFIDENCE, -1, pc.as_set(channels))[0]
    want = pc.confidence_oracle(full, channels, S)
    err = float((conf.double().cpu() - want).abs().max())
    print("confidence max abs error", err)
    assert err <= 1e-6


def test_parse_head_sample_without_the_class():
    """Sample 1 never has the class on top: all ones there, flag set; sample 0 keeps its own mask."""
    C, h, size, S = 21, 9, 65, 16
    low = head_logits(C, h, size, S, -1, (7,), no_class_in_sample_1=True)
    full = pc.upsample64(low, size)
    mask, empty, margin, soft = pc.hard_oracle(full, -1, (7,), S)
    excluded = pc.excluded_pixels(full, margin)
    assert float(excluded.double().mean()) <= pc.EXCLUDED_CAP and empty.tolist() == [False, True]
    out, fm, flag = parsing.parse_head(low.to(DEV), size, S, parsing.PARSE_HARD, -1, 1 << 7, True)
    assert flag.tolist() == [0, 1]
    assert torch.equal(out[1].cpu(), torch.ones(1, S, S)) and bool(fm[1].all())
    keep = ~excluded[:, None]
    assert torch.equal(fm.cpu().bool()[keep], mask[keep])
    assert bool(((out.double().cpu() - soft).abs() <= pc.soft_bound(excluded, S)).all())
    assert 0 < float(out[0].mean()) < 1


# ----------------------------------------------------------------------------- whole nets
@pytest.fixture(scope="module")
def device_nets():
    nets = {}
    for name in pc.NETS:
        net = parsing.BiSeNet(19) if name == "bisenet" else parsing.PSPNet(50, 21)
        nets[name] = pc.fill(net, pc.NETS[name]["weight_seed"]).to(DEV)
    return nets


@pytest.mark.parametrize("name", list(pc.NETS))
def test_whole_net_logits(golden, device_nets, name):
    g, net, side = golden("parsing"), device_nets[name], pc.NETS[name]["side"]
    x = pc.images(name, side).to(DEV)
    keys = ("feat8", "feat16", "feat32") if name == "bisenet" else ("layer1", "layer2", "layer3", "layer4")
    for key, feat in zip(keys, net.features(x)):          # printed to localise a failure
        print(key, "norm relative deviation", abs(float(feat.double().norm()) / float(g[f"{name}.norm.{key}"]) - 1))
    ref_low = torch.from_numpy(g[f"{name}.low"])
    bound = pc.NET_ERR_FACTOR * float(g[f"{name}.ref_fp32_err"])
    low_err = pc.l2_rel(net.logits_lowres(x).cpu(), ref_low)
    full = net(x)
    assert full.shape == (pc.B, ref_low.shape[1], side, side)
    err = pc.l2_rel(full.cpu(), pc.upsample64(ref_low, side))
    native_err = pc.l2_rel(net(x, native=True).cpu(), pc.upsample64(ref_low, side))
    print(f"{name}: L2-relative logit error {err:.3e} (before the up-sampling {low_err:.3e}; native route "
          f"{native_err:.3e}); bound {bound:.3e}")
    assert err <= bound


def fixture_masks(g, name):
    side = pc.NETS[name]["side"]
    full = np.unpackbits(g[f"{name}.mm.full_mask"])[:pc.B * side * side].reshape(pc.B, 1, side, side)
    excluded = torch.from_numpy(g[f"{name}.mm.margin"]).double() < pc.MARGIN_REL * float(g[f"{name}.mm.max_abs"])
    return torch.from_numpy(full).bool(), excluded


def confidence_bound(g, name):
    """Confidence map of a whole net, per output pixel.  The nets are held to an L2-relative logit error of
    4 x ref_fp32_err; read per pixel, relative to max|logit|, that is e = 4 ref_fp32_err max|logit| per channel.  The
    map is (v - min v) / (max v - min v) with v the sum of n channels: an error n e in v, in its minimum and in its
    maximum moves the quotient by at most 3 n e / (max v - min v) to first order.  Plus the kernel's own 1e-6."""
    n = len(pc.rule_of(pc.NETS[name]["category"])[2])
    e = pc.NET_ERR_FACTOR * float(g[f"{name}.ref_fp32_err"]) * float(g[f"{name}.mm.max_abs"])
    return 1e-6 + 3 * n * e / float(g[f"{name}.mm.conf_range"].min())


@pytest.mark.parametrize("name", list(pc.NETS))
def test_masking_model_against_the_fixture(golden, device_nets, name):
    g, cfg = golden("parsing"), pc.NETS[name]
    mm = parsing.MaskingModel(cfg["category"], device=DEV, size=cfg["side"], net=device_nets[name])
    image = pc.images(name + ".mm", pc.S).to(DEV)
    want_full, excluded = fixture_masks(g, name)
    share = float(excluded.double().mean())
    cover = float(want_full.double().mean())
    print("excluded share", share, "coverage", cover)
    assert share <= pc.EXCLUDED_CAP and 0.05 <= cover <= 0.95
    soft = mm.image_mask(image)
    assert soft.shape == (pc.B, 1, pc.S, pc.S) and soft.is_cuda and mm.last_fallback.tolist() == [0, 0]
    bound = pc.soft_bound(excluded, pc.S)
    assert bool(((soft.double().cpu() - torch.from_numpy(g[f"{name}.mm.image_mask"])).abs() <= bound).all())
    _, full = mm._hard(image, True)
    keep = ~excluded[:, None]
    assert torch.equal(full.cpu()[keep], want_full[keep])
    conf = mm.confidence_mask(image)
    err = float((conf.double().cpu() - torch.from_numpy(g[f"{name}.mm.confidence_mask"])).abs().max())
    print("confidence max abs error", err)
    assert err <= confidence_bound(g, name)
    depth = torch.ones(pc.B, pc.S, pc.S, device=DEV)
    masked = mm.image_mask(image, depth)
    assert masked.shape == (pc.B, 1, pc.S, pc.S) and bool(torch.isnan(masked).any()) and not bool(torch.isnan(masked).all())


@pytest.mark.parametrize("prior", ["ellipsoid", "smoothed_box", "smoothed_confidence"])
def test_priors_from_the_masking_model(golden, device_nets, prior):
    """PriorGenerator on the device with MaskingModel as its batched mask source == the host path fed with the
    fixture's masks (float64 reference results, rounded to float32)."""
    name = "bisenet"
    g, cfg = golden("parsing"), pc.NETS[name]
    mm = parsing.MaskingModel(cfg["category"], device=DEV, size=cfg["side"], net=device_nets[name])
    confidence = "confidence" in prior
    source = mm.confidence_mask if confidence else mm.image_mask
    image = pc.images(name + ".mm", pc.S).to(DEV)
    gen = PriorGenerator(pc.S, cfg["category"], prior, masking_model=source, on_device=True, mask_accepts_batch=True)
    got = gen(image, device=DEV)
    masks = torch.from_numpy(g[f"{name}.mm.{'confidence_mask' if confidence else 'image_mask'}"]).float()
    _, excluded = fixture_masks(g, name)
    # The mask source is held to its own bound first (that of test_masking_model_against_the_fixture).  What its
    # deviation does to a prior: the maps are far - far * m (or / (1 - threshold) for the box), the three smoothing
    # passes average (no gain) and rescale to a span of far - near = 0.11 from the span of the map, about far, then
    # from spans the 11-tap filter shrinks by less than 1 / 0.11: the product of the gains stays below 1.  On top of
    # it the bound the project holds the host path to (priors_cases.RTOL, ATOL).  The ellipsoid reads only the
    # bounding box of mask >= threshold: equal boxes wherever the masks agree on that.
    deviation = (source(image).double().cpu() - masks.double()).abs()
    allowed = confidence_bound(g, name) if confidence else pc.soft_bound(excluded, pc.S)
    assert bool((deviation <= allowed).all())
    atol = ATOL + FAR / (1 - THRESHOLD) * float(deviation.max())
    for b in range(pc.B):
        host = PriorGenerator(pc.S, cfg["category"], prior, masking_model=lambda im, b=b: masks[b:b + 1])
        want = host(image[b:b + 1].cpu(), device="cpu")
        err = float((got[b].cpu() - want[0]).abs().max())
        print(prior, "sample", b, "max abs error", err, "bound", atol)
        np.testing.assert_allclose(got[b].cpu().numpy(), want[0].numpy(), rtol=RTOL, atol=atol)


def test_image_mask_in_a_graph_replays_bit_for_bit(device_nets):
    """image_mask at the small size, captured once and replayed on a second input, equals the eager result bit for
    bit: nothing in it synchronises with the host or depends on it."""
    name = "bisenet"
    cfg = pc.NETS[name]
    mm = parsing.MaskingModel(cfg["category"], device=DEV, size=cfg["side"], net=device_nets[name])
    first, second = pc.images(name + ".mm", pc.S, 1).to(DEV), pc.images(name + ".mm", pc.S, 2).to(DEV)
    eager = mm.image_mask(second).clone()
    eager_flag = mm.last_fallback.clone()
    static = first.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        mm.image_mask(static)                    # warm-up: folded weights, allocator, split workspaces
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = mm.image_mask(static)
        flag = mm.last_fallback
    static.copy_(second)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager) and torch.equal(flag, eager_flag)
    assert not torch.equal(mm.image_mask(first), eager)
