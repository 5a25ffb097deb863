"""-m gpu: round-3 additions of the C ABI — reproducible launch partitions (g2s_set_deterministic),
the step-wide cleared pool (g2s_modconv's y_is_zero / g2s_modconv_needs_zero, zeropool.py) — against the
oracle and against the default launch mode."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import capi  # noqa: E402


@pytest.fixture(scope="module")
def L():
    import gan2shape_amd  # noqa: F401
    from gan2shape_amd import lib
    return lib.load()


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


# Small layers: few tiles -> the default mode splits K and adds partial sums with float atomics.
SMALL = [(1, 512, 512, 16, 3, 0), (8, 512, 512, 4, 3, 0), (8, 512, 512, 8, 3, 1), (1, 256, 512, 16, 3, 0)]


@pytest.mark.parametrize("B,cin,cout,H,k,mode", SMALL)
def test_deterministic_mode_repeats_bitwise_and_matches_oracle(L, B, cin, cout, H, k, mode):
    """g2s_set_deterministic(1): split-K 1 in the direct kernel, Winograd partial sums only as stored
    slices -> the same bits on every run; the values equal the oracle's (and the default mode's)
    within the fp32 summation-order tolerance of tests/test_gpu_conv_tiles.py."""
    from gan2shape_amd import lib
    from gan2shape_amd import modconv as mc
    rng = np.random.default_rng(B + cin + H + mode)
    w = (rng.standard_normal((cout, cin, k, k)) / math.sqrt(cin * k * k)).astype(np.float32)
    x = rng.standard_normal((B, cin, H, H)).astype(np.float32)
    s = (1 + 0.3 * rng.standard_normal((B, cin))).astype(np.float32)
    exp = capi.modconv(x, w, s, 1.0, False, mode)
    xd, wd, sd = dev(x), dev(w), dev(s)
    assert L.g2s_modconv_needs_zero(B, cin, cout, H, H, k, mode, 0, 1, 0) == 1   # default mode: adds into y
    prev = lib.set_deterministic(True)
    try:
        assert L.g2s_get_deterministic() == 1
        if mode == 0:   # a polyphase scatter leaves holes whatever the split
            assert L.g2s_modconv_needs_zero(B, cin, cout, H, H, k, mode, 0, 1, 0) == 0
        saved = mc.WINO_FORCE
        runs = []
        for force in ("direct", saved):
            mc.WINO_FORCE = force
            ys = [mc.modconv_raw(xd, wd, sd, None, mode, 0).clone() for _ in range(4)]
            assert all(torch.equal(ys[0], y) for y in ys[1:]), f"run-to-run differences ({force})"
            runs.append(ys[0])
        mc.WINO_FORCE = saved
    finally:
        lib.set_deterministic(prev)
    assert L.g2s_get_deterministic() == int(prev)
    y_default = mc.modconv_raw(xd, wd, sd, None, mode, 0)
    tol = 2e-5 * max(1.0, math.sqrt(cin * k * k / 1152))
    for y in runs + [y_default]:
        np.testing.assert_allclose(y.cpu().numpy(), exp, rtol=2e-4, atol=tol * max(1.0, float(np.abs(exp).max())))


def test_deterministic_weight_gradient_repeats_bitwise(L):
    """The weight-gradient GEMM without its pixel split: one workgroup owns every dw element."""
    from gan2shape_amd import lib
    from gan2shape_amd.op import conv as gconv
    torch.manual_seed(0)
    A = torch.randn(9, 64, 32, 32, device="cuda")
    G = torch.randn(9, 128, 16, 16, device="cuda")
    ref = torch.nn.grad.conv2d_weight(A.double().cpu(), (128, 64, 4, 4), G.double().cpu(), stride=2, padding=1)
    prev = lib.set_deterministic(True)
    try:
        dws = [gconv._wgrad(G, A, 4, 2, 1).clone() for _ in range(3)]
    finally:
        lib.set_deterministic(prev)
    assert torch.equal(dws[0], dws[1]) and torch.equal(dws[0], dws[2])
    dflt = gconv._wgrad(G, A, 4, 2, 1)
    for dw in (dws[0], dflt):
        assert float((dw.double().cpu() - ref).norm()) <= 2e-5 * float(ref.norm())


def test_zero_pool_hands_out_cleared_slices_and_results_do_not_change(L):
    """zeropool: the second step of a kind gets a pool as large as the first one asked for; launches
    that add partial sums take their output from it (no clear of their own) and produce what the
    library's own clear produces."""
    from gan2shape_amd import modconv as mc
    from gan2shape_amd import zeropool
    torch.manual_seed(0)
    x = torch.randn(1, 512, 16, 16, device="cuda")
    w = torch.randn(512, 512, 3, 3, device="cuda") / 68
    b = torch.randn(512, device="cuda")
    saved = mc.WINO_FORCE
    mc.WINO_FORCE = "direct"
    try:
        zeropool.end()
        y0 = mc.conv_bias_relu(x, w, b)               # no step active: the library clears y itself
        zeropool.begin("test", x.device)              # first step of this kind: nothing to hand out yet
        assert zeropool.take((4,), x.device) is None
        y1 = mc.conv_bias_relu(x, w, b)
        zeropool.begin("test", x.device)              # second step: pool sized by the first
        y2 = mc.conv_bias_relu(x, w, b)
        pool = zeropool._state["buf"]
        assert pool is not None and pool.numel() >= y2.numel()
        assert y2.data_ptr() >= pool.data_ptr() and y2.data_ptr() < pool.data_ptr() + pool.numel() * 4
        extra = zeropool.take((4,), x.device)
        assert extra is None or float(extra.abs().max()) == 0.0
    finally:
        mc.WINO_FORCE = saved
        zeropool.end()
    ref = torch.relu(torch.nn.functional.conv2d(x.double().cpu(), w.double().cpu(), b.double().cpu(), padding=1))
    for y in (y0, y1, y2):
        assert float((y.double().cpu() - ref).norm()) <= 2e-5 * float(ref.norm())
    # a large layer overwrites its output: never taken from the pool
    assert L.g2s_modconv_needs_zero(8, 128, 128, 128, 128, 3, 0, 0, 0, 0) == 0


def test_clamp_matches_torch_including_the_bounds(L):
    """g2s_clamp: forward bit-equal to torch.clamp, backward = torch's rule (gradient passes where
    lo <= x <= hi, bounds inclusive), odd sizes and unaligned views included."""
    from gan2shape_amd.op import clamp
    torch.manual_seed(0)
    for shape in [(8, 3, 128, 128), (1, 128, 128), (3, 5, 7)]:
        x0 = torch.randn(*shape, device="cuda") * 1.5
        x0.view(-1)[:6] = torch.tensor([-1.0, 1.0, -1.0000001, 1.0000001, 0.0, float("nan")], device="cuda")
        g = torch.randn_like(x0)
        xa = x0.clone().requires_grad_(True)
        xb = x0.clone().requires_grad_(True)
        ya, yb = clamp(xa, -1, 1), xb.clamp(min=-1, max=1)
        assert torch.equal(torch.nan_to_num(ya.detach(), nan=7.0), torch.nan_to_num(yb.detach(), nan=7.0))
        ya.backward(g)
        yb.backward(g)
        assert torch.equal(xa.grad, xb.grad)
    x = torch.randn(1001, device="cuda")[1:].requires_grad_(True)      # 4-byte aligned only
    y = clamp(x, -0.5, 0.25)
    assert torch.equal(y.detach(), x.detach().clamp(-0.5, 0.25))


# test_every_step_kind_actually_optimises moved to tests/test_gpu_round4.py (test_every_step_kind_lowers_its_own_loss:
# real descent bounds at the reference's learning rate; the cause of round 3's red run is recorded there)


@pytest.mark.parametrize("masked", [True, False])
def test_discriminator_loss_one_node_equals_op_by_op(masked):
    """losses._DFeatureL1 (fake + real through D as one batch of 2N, hand-written backward over the fake
    half) against DiscriminatorLoss's op-by-op autograd form (losses.py:6-36 on stylegan2-pytorch/
    model.py:630-750): the value to 1e-6; the image gradient equal except under leaky-ReLU units that sit
    within rounding of their kink (the batch-2N launches sum in another order) — L2 2e-3, all but 0.1 %
    of the elements to 5e-3 of the largest, as in the D(128) fixture test."""
    from gan2shape_amd import losses
    from gan2shape_amd import stylegan2 as sg2
    from test_gpu_model import fill_deterministic
    torch.manual_seed(0)
    D = sg2.Discriminator(128, channel_multiplier=1)
    fill_deterministic(D, 78)
    D = D.cuda().eval().requires_grad_(False)
    N = 4
    base = torch.tanh(torch.nn.functional.interpolate(torch.randn(N, 3, 16, 16), scale_factor=8, mode="bilinear"))
    fake0 = (base + 0.1 * torch.randn(N, 3, 128, 128)).clamp(-1, 1).cuda()
    real = (base * 0.9 + 0.1 * torch.randn(N, 3, 128, 128)).clamp(-1, 1).cuda()
    mask = (torch.rand(N, 1, 128, 128, device="cuda") > 0.3).float() if masked else None
    loss_fn = losses.DiscriminatorLoss()
    out = {}
    try:
        for one in (True, False):
            losses.DiscriminatorLoss.ONE_NODE = one
            fake = fake0.clone().requires_grad_(True)
            val = loss_fn(D, fake, real, mask=mask)
            (gx,) = torch.autograd.grad(val * 1.7, fake)
            out[one] = (float(val.detach()), gx)
    finally:
        losses.DiscriminatorLoss.ONE_NODE = True
    assert abs(out[True][0] - out[False][0]) <= 2e-6 * abs(out[False][0])
    a, b = out[True][1].double(), out[False][1].double()
    err = (a - b).abs()
    assert float((a - b).norm() / b.norm()) <= 2e-3
    assert float((err > 5e-3 * b.abs().max()).double().mean()) <= 1e-3
    assert float(err.max()) <= 5e-2 * float(b.abs().max())


# ----------------------------------------------------------------------- reconstruction warp (grid_sample.hip)
def _warp_inputs(B, C, IH, IW, H, W, seed, spill=1.15):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(B, C, IH, IW, generator=g) * 0.9).cuda()
    # a smooth warp plus jitter; `spill` > 1 pushes some samples outside the texture (zero padding)
    ys, xs = torch.meshgrid(torch.linspace(-1, 1, H), torch.linspace(-1, 1, W), indexing="ij")
    base = torch.stack([xs, ys], -1)[None].repeat(B, 1, 1, 1) * spill
    grid = (base + 0.05 * torch.randn(B, H, W, 2, generator=g)).cuda()
    gy = torch.randn(B, C, H, W, generator=g).cuda()
    return x, grid, gy


@pytest.mark.parametrize("B,C,IH,IW,H,W,bounds", [(8, 3, 128, 128, 128, 128, (-1.0, 1.0)), (2, 3, 64, 64, 64, 64, None),
                                                  (3, 1, 17, 23, 40, 31, (-0.3, 0.4)), (1, 5, 32, 32, 8, 8, None)])
def test_grid_sample_matches_torch(L, B, C, IH, IW, H, W, bounds):
    """g2s_grid_sample_* against F.grid_sample(.., 'bilinear', align_corners=True)[.clamp(lo, hi)] — the
    reference's own calls (GAN2Shape/model.py:147-150, 267-270) — forward, texture gradient and grid
    gradient, including samples that fall off the texture and values on either side of the clamp."""
    import torch.nn.functional as F
    from gan2shape_amd.op import grid_sample
    x, grid, gy = _warp_inputs(B, C, IH, IW, H, W, 5)
    outs = []
    for mine in (True, False):
        xx, gg = x.clone().requires_grad_(True), grid.clone().requires_grad_(True)
        if mine:
            y = grid_sample(xx, gg, *(bounds or (None, None)))
        else:
            y = F.grid_sample(xx, gg, mode="bilinear", align_corners=True)
            y = y if bounds is None else y.clamp(*bounds)
        y.backward(gy)
        outs.append((y.detach(), xx.grad, gg.grad))
    (y, gx, ggr), (y0, gx0, ggr0) = outs
    assert float((y - y0).abs().max()) <= 2e-6 * max(1.0, float(y0.abs().max()))
    if bounds is not None:
        assert float((y0 == bounds[0]).float().mean()) > 0.01 and float((y0 == bounds[1]).float().mean()) > 0.01
    assert float((y0 == 0).float().mean()) > 0.005                       # some samples are off the texture
    # a clamp decision can differ where the sample is within one rounding of a bound: bounded count
    for a, b, name in ((gx, gx0, "gx"), (ggr, ggr0, "ggrid")):
        e = (a - b).abs()
        scale = float(b.abs().max())
        loose = int((e > 2e-5 * scale).sum())
        assert loose <= (4 * C if bounds is not None else 0), (name, loose, float(e.max()), scale)
        assert float((a - b).norm() / b.norm()) <= 2e-4, name


def test_grid_sample_gradient_is_bitwise_reproducible_in_deterministic_mode(L):
    from gan2shape_amd import lib
    from gan2shape_amd.op import grid_sample
    x, grid, gy = _warp_inputs(8, 3, 128, 128, 128, 128, 6)

    def grads():
        xx, gg = x.clone().requires_grad_(True), grid.clone().requires_grad_(True)
        grid_sample(xx, gg, -1.0, 1.0).backward(gy)
        return xx.grad, gg.grad
    ref = grads()
    lib.set_deterministic(True)
    try:
        runs = [grads() for _ in range(4)]
    finally:
        lib.set_deterministic(False)
    for r in runs[1:]:
        assert torch.equal(r[0], runs[0][0]) and torch.equal(r[1], runs[0][1])
    # fixed point at 2^-40 against the float-atomic sum: fp32 rounding apart
    assert float((runs[0][0] - ref[0]).abs().max()) <= 2e-6 * float(ref[0].abs().max())
    assert torch.equal(runs[0][1], ref[1])                                # the grid gradient has no scatter


def test_raster_backward_is_bitwise_reproducible_in_deterministic_mode(L):
    """g2s_raster_depth_bwd_ex with its fixed-point workspace: identical vertex gradients from run to run
    (the float-atomic default differs in the last bits), equal to the default up to fp32 rounding; without
    the workspace deterministic mode refuses (G2S_ERR_WORKSPACE)."""
    from gan2shape_amd import lib
    from gan2shape_amd.plugins import neural_renderer as nr
    S, B = 64, 4
    g = torch.Generator().manual_seed(9)
    ys, xs = torch.meshgrid(torch.linspace(-0.3, 0.3, S), torch.linspace(-0.3, 0.3, S), indexing="ij")
    z = 1.0 + 0.05 * torch.randn(B, S, S, generator=g).cumsum(1).cumsum(2) / S
    verts = torch.stack([xs[None] * z, ys[None] * z, z], -1).reshape(B, S * S, 3).cuda()
    K = [2.0 * S, 0.0, S / 2.0, 0.0, 2.0 * S, S / 2.0, 0.0, 0.0, 1.0]
    gd = torch.randn(B, S, S, generator=g).cuda()

    def grad():
        v = verts.clone().requires_grad_(True)
        d = nr.RenderDepthFunction.apply(v, None, K, float(S), S, True, True, 0.1, 100.0)
        d.backward(gd)
        return v.grad
    ref = grad()
    assert float(ref.abs().max()) > 0
    lib.set_deterministic(True)
    try:
        runs = [grad() for _ in range(4)]
        v = verts.clone()
        fidx = torch.zeros(B, 2 * S, 2 * S, dtype=torch.int32, device="cuda")
        bary = torch.zeros(B, 2 * S, 2 * S, 3, device="cuda")
        Kc = (lib.C.c_float * 9)(*K)
        rc = L.g2s_raster_depth_bwd(lib.ptr(v), None, lib.ptr(gd), lib.ptr(fidx), lib.ptr(bary), B, S * S,
                                    2 * (S - 1) * (S - 1), S, Kc, float(S), 2, lib.ptr(torch.empty_like(v)), lib.stream())
        assert rc == -3 and b"workspace" in L.g2s_last_error()
    finally:
        lib.set_deterministic(False)
    for r in runs[1:]:
        assert torch.equal(r, runs[0])
    assert float((runs[0] - ref).abs().max()) <= 1e-5 * float(ref.abs().max())


def test_training_steps_are_bitwise_reproducible_in_deterministic_mode():
    """The switch the reference lacks: with g2s_set_deterministic(1) every step kind returns the same loss
    and the same parameter gradients, bit for bit, when run twice from the same state (two Adam updates
    then land on identical parameters).  The default mode is checked to differ only at fp32 rounding."""
    import bench
    from gan2shape_amd import lib
    from gan2shape_amd.model import GAN2Shape
    from gan2shape_amd.trainer import Trainer
    torch.manual_seed(0)
    t = Trainer(GAN2Shape, bench.face_config(n_proj=4), device="cuda")
    m = t.model
    image, latent = bench.synthetic_sample(m, 99, torch.device("cuda"))

    def grads_of(step, collected):
        for p in m.parameters():
            p.grad = None
        torch.manual_seed(5)
        loss, out = getattr(m, f"forward_step{step}")(image, latent, collected, n_proj_samples=4)
        loss.backward()
        return float(loss.detach()), [p.grad.clone() for p in m.parameters() if p.grad is not None], out

    for det in (True, False):
        lib.set_deterministic(det)
        try:
            collected = None
            for step in (1, 2, 3):
                l1, g1, out = grads_of(step, collected)
                l2, g2, _ = grads_of(step, collected)
                assert len(g1) == len(g2) and len(g1) > 0
                if det:
                    assert l1 == l2, (step, l1, l2)
                    differing = sum(int(not torch.equal(a, b)) for a, b in zip(g1, g2))
                    assert differing == 0, (step, differing, len(g1))
                else:
                    worst = max(float((a - b).norm() / (a.norm() + 1e-30)) for a, b in zip(g1, g2))
                    assert abs(l1 - l2) <= 1e-5 * abs(l1) and worst <= 1e-2, (step, l1, l2, worst)
                collected = out
        finally:
            lib.set_deterministic(False)


def test_graph_replayed_training_run_is_bitwise_reproducible_in_deterministic_mode():
    """Two whole runs — build, capture, replay 1 1 2 2 3 3 — from the same seed end on identical
    parameters in every trained net (the Adam updates included), bit for bit."""
    import bench
    from gan2shape_amd import lib
    from gan2shape_amd.graphs import GraphedSteps
    from gan2shape_amd.model import GAN2Shape
    from gan2shape_amd.trainer import Trainer

    def run():
        torch.manual_seed(0)
        t = Trainer(GAN2Shape, bench.face_config(n_proj=4), device="cuda", capturable=True)
        image, latent = bench.synthetic_sample(t.model, 77, torch.device("cuda"))
        g = GraphedSteps(trainer=t, image=image, latent=latent, warmup=2)
        for kind in (1, 2, 3):
            g.capture(kind)
        torch.manual_seed(11)
        losses = [float(g.run(kind)) for kind in (1, 1, 2, 2, 3, 3)]
        torch.cuda.synchronize()
        params = {f"{n}.{k}": p.detach().clone() for n in t.model.NETS
                  for k, p in getattr(t.model, n + "_net").named_parameters()}
        return losses, params

    dev_ = torch.device("cuda")
    torch.cuda.set_stream(torch.cuda.Stream(dev_))     # captures need a non-default stream
    lib.set_deterministic(True)
    try:
        la, pa = run()
        lb, pb = run()
    finally:
        lib.set_deterministic(False)
        torch.cuda.set_stream(torch.cuda.default_stream(dev_))
    assert la == lb, (la, lb)
    differing = [k for k in pa if not torch.equal(pa[k], pb[k])]
    assert not differing, (len(differing), len(pa), differing[:5])


# ----------------------------------------------------------------------- launch-count kernels of round 3
@pytest.mark.parametrize("masked", [True, False])
def test_weighted_l1_with_denominator_and_joined_gradient(L, masked):
    """g2s_weighted_l1_fwd2 / _bwd2 against the reference's expression (losses.py:40-51:
    (|a - b| * mask.expand_as).sum() / mask.expand_as.sum()), plus the gradient that joins in."""
    from gan2shape_amd import lib
    g = torch.Generator().manual_seed(3)
    B, C, H, W = 4, 6, 16, 24
    x, y = torch.randn(B, C, H, W, generator=g).cuda(), torch.randn(B, C, H, W, generator=g).cuda()
    w = (torch.rand(B, 1, H, W, generator=g) > 0.3).float().cuda() if masked else None
    gadd = torch.randn(B, C, H, W, generator=g).cuda()
    numden = torch.zeros(2, device="cuda")
    lib.check(L.g2s_weighted_l1_fwd2(lib.ptr(x), lib.ptr(y), lib.ptr(w), lib.ptr(numden), B, C, H * W, lib.stream()))
    xr = x.double().requires_grad_(True)
    wd = torch.ones(B, 1, H, W, device="cuda", dtype=torch.float64) if w is None else w.double()
    err = (xr - y.double()).abs()
    ref = (err * wd.expand_as(err)).sum() / wd.expand_as(err).sum()
    assert abs(float(numden[0] / numden[1]) - float(ref)) <= 1e-6 * abs(float(ref))
    assert abs(float(numden[1]) - float(wd.expand_as(err).sum())) <= 1e-6 * float(numden[1])
    gout = torch.tensor([0.7], device="cuda")
    (gref,) = torch.autograd.grad(ref, xr, gout.double()[0])
    gx = torch.empty_like(x)
    lib.check(L.g2s_weighted_l1_bwd2(lib.ptr(x), lib.ptr(y), lib.ptr(w), lib.ptr(gout), lib.ptr(numden[1:]), lib.ptr(gadd),
                                     lib.ptr(gx), B, C, H * W, lib.stream()))
    assert float((gx.double() - (gref + gadd.double())).abs().max()) <= 1e-6


@pytest.mark.parametrize("clamp_border", [True, False])
def test_depth_head_matches_the_op_by_op_chain(L, clamp_border):
    """g2s_depth_head_* against get_clamped_depth's torch chain (GAN2Shape/model.py:337-345): values and the
    gradient w.r.t. the raw map, the whole-batch centring included."""
    from gan2shape_amd.fused_geometry import depth_head
    g = torch.Generator().manual_seed(4)
    B, H, W = 3, 32, 32
    raw = (torch.randn(B, H, W, generator=g) * 0.8 + 0.3).cuda()
    gout = torch.randn(B, H, W, generator=g).cuda()
    lo, hi, bd = 0.9, 1.1, 0.7 * 1.1 + 0.3 * 0.9

    def chain(r):
        mean = r.view(1, -1).mean(1)
        t = torch.tanh(r - mean.view(1, 1, 1))
        d = (1 + t) / 2 * hi + (1 - t) / 2 * lo
        if clamp_border:
            border = torch.nn.functional.pad(torch.zeros(1, H, W - 4, device=r.device), (2, 2), mode="constant", value=1.02)
            d = d * (1 - border) + border * bd
        return d
    outs = []
    for fn in (lambda r: depth_head(r, W, lo, hi, clamp_border, bd), chain):
        r = raw.clone().requires_grad_(True)
        d = fn(r)
        d.backward(gout)
        outs.append((d.detach(), r.grad))
    (d1, g1), (d0, g0) = outs
    assert float((d1 - d0).abs().max()) <= 2e-7
    assert float((g1 - g0).abs().max()) <= 1e-6 * float(g0.abs().max()) + 1e-9


def test_res_split_matches_relu_and_avg_pool(L):
    import torch.nn.functional as F
    from gan2shape_amd.networks import _ResSplit
    g = torch.Generator().manual_seed(5)
    x = torch.randn(4, 32, 16, 24, generator=g).cuda()
    gr, gp = torch.randn(4, 32, 16, 24, generator=g).cuda(), torch.randn(4, 32, 8, 12, generator=g).cuda()
    xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    r, p = _ResSplit.apply(xa)
    torch.autograd.backward([r, p], [gr, gp])
    r0, p0 = F.relu(xb), F.avg_pool2d(xb, 2, 2)
    torch.autograd.backward([r0, p0], [gr, gp])
    assert torch.equal(r, r0) and torch.equal(p, p0)
    assert torch.equal(xa.grad, xb.grad)
    # one branch only
    xc = x.clone().requires_grad_(True)
    _ResSplit.apply(xc)[1].backward(gp)
    xd = x.clone().requires_grad_(True)
    F.avg_pool2d(xd, 2, 2).backward(gp)
    assert torch.equal(xc.grad, xd.grad)


def test_modconv_demod_one_node_equals_two_nodes(L):
    """ModConvDemodFunction (style gradient joined inside g2s_demod_bwd_add) against demodulation + modconv
    as two autograd nodes: identical outputs, input gradients and style gradients."""
    from gan2shape_amd import modconv as mc
    g = torch.Generator().manual_seed(6)
    B, cin, cout, H = 4, 64, 32, 16
    x = torch.randn(B, cin, H, H, generator=g).cuda()
    w = (torch.randn(cout, cin, 3, 3, generator=g) / (cin * 9) ** 0.5).cuda()
    s = (1 + 0.3 * torch.randn(B, cin, generator=g)).cuda()
    wsq = w.pow(2).sum((2, 3))
    gy = torch.randn(B, cout, H, H, generator=g).cuda()
    from gan2shape_amd import lib
    res = []
    lib.set_deterministic(True)      # fixed partitions: the two forms can be compared bit for bit
    try:
        for one in (True, False):
            xx, ss = x.clone().requires_grad_(True), s.clone().requires_grad_(True)
            y = mc.modconv_demod(xx, w, ss, wsq, 1e-8, mc.PLAIN) if one else \
                mc.modconv(xx, w, ss, mc.demodulation(ss, wsq, 1e-8), mc.PLAIN)
            y.backward(gy)
            res.append((y.detach(), xx.grad, ss.grad))
    finally:
        lib.set_deterministic(False)
    for a, b in zip(*res):
        assert torch.equal(a, b)


@pytest.mark.parametrize("levels,shape", [(4, (8, 1, 128, 128)), (3, (2, 3, 32, 48)), (1, (1, 1, 2, 2))])
def test_avg_pyramid_equals_successive_avg_pools(L, levels, shape):
    import torch.nn.functional as F
    from gan2shape_amd.losses import _mask_pyramid
    g = torch.Generator().manual_seed(8)
    m = torch.rand(*shape, generator=g).cuda()
    got = _mask_pyramid(m, levels)
    w = m
    for l in range(levels):
        w = F.avg_pool2d(w, 2, 2)
        assert got[l].shape == w.shape and torch.equal(got[l], w), l


def test_generator_shared_latent_path_equals_per_layer_latents():
    """One w for every layer (GAN2Shape's only case): the modulations from an expanded view of it equal the
    per-layer-latent route, values and the gradient that reaches w."""
    from gan2shape_amd.stylegan2 import Generator
    torch.manual_seed(3)
    G = Generator(64, 512, 8, channel_multiplier=1).cuda().eval()
    for p in G.parameters():
        p.requires_grad_(False)
    w = torch.randn(2, 512, device="cuda")
    res = []
    for shared in (True, False):
        ww = w.clone().requires_grad_(True)
        styles = [ww] if shared else [ww[:, None].expand(-1, G.n_latent, -1).contiguous()]
        img, _ = G(styles, input_is_w=True, randomize_noise=False)
        img.square().mean().backward()
        res.append((img.detach(), ww.grad))
    (i1, g1), (i0, g0) = res
    assert float((i1 - i0).abs().max()) <= 1e-5 * float(i0.abs().max())
    assert float((g1 - g0).norm() / g0.norm()) <= 1e-3      # split-K order noise through 13 random-weight layers
