"""Discriminator training on the GPU: the twice-differentiable convolution nodes (op/conv2d_gradfix.py), the
minibatch-stddev kernels and loss heads (csrc/dtrain.hip), the whole discriminator against the reference's float64
fixture (tests/golden/dtrain.npz), every parameter gradient against this package's CPU float64 route, and two trainer
steps.  Statements and bounds: dtrain_cases.py."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dtrain_cases as dc

pytestmark = pytest.mark.gpu

EPS32 = float(np.finfo(np.float32).eps)


@pytest.fixture(scope="module")
def pkg():
    import gan2shape_amd  # noqa: F401
    from gan2shape_amd import dtrain, lib
    from gan2shape_amd.op import conv2d_gradfix, mbstd
    from gan2shape_amd.stylegan2 import Discriminator
    lib.load()
    return dtrain, conv2d_gradfix, mbstd, Discriminator


@pytest.fixture(scope="module")
def fx(golden):
    return golden("dtrain")


def dev(a, grad=False):
    return torch.as_tensor(a).float().cuda().requires_grad_(grad)


# ------------------------------------------------------------------------------------------- convolution nodes
def conv64(x, w, mode):
    return F.conv2d(x, w, padding=w.shape[2] // 2) if mode == 0 else F.conv2d(x, w, stride=2)


CONV_SHAPES = [(2, 3, 16), (2, 16, 24), (2, 513, 8)]


@pytest.mark.parametrize("mode", ["PLAIN", "DOWN2"])
@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("B,cin,cout", CONV_SHAPES)
def test_convolution_node(pkg, mode, k, B, cin, cout):
    """Forward, data gradient, weight gradient, and the weight gradient of the second backward against F.conv2d in
    float64; the adjoint identity and the bilinearity of the weight gradient in relative terms.  Bound: a float32 dot
    product of n terms, accumulated in float32 in any order, is within n * eps32 * sum |terms| of the exact one;
    sum |terms| <= |a|_2 |b|_2 per output, so each result is held to n * eps32 * (product of the operands' largest
    per-output norms), n the length of its reduction."""
    gradfix = pkg[1]
    m = gradfix.PLAIN if mode == "PLAIN" else gradfix.DOWN2
    sides = [4] if cin == 513 else [4, 6, 16]
    for side in sides:
        H = side + 1 if mode == "DOWN2" else side      # DOWN2 takes (H - k) even, as after the blur pad: 5, 7, 17
        g = torch.Generator().manual_seed(1000 * cin + 10 * side + k)
        x64 = torch.randn(B, cin, H, H, generator=g, dtype=torch.float64).float().double().requires_grad_(True)
        w64 = (torch.randn(cout, cin, k, k, generator=g, dtype=torch.float64) / (cin * k * k) ** 0.5).float().double()
        w64.requires_grad_(True)
        y64 = conv64(x64, w64, 0 if mode == "PLAIN" else 2)
        gy64 = torch.randn(y64.shape, generator=g, dtype=torch.float64).float().double()
        ggx64 = torch.randn(x64.shape, generator=g, dtype=torch.float64).float().double()
        gx64, gw64 = torch.autograd.grad(y64, (x64, w64), gy64, create_graph=True)
        gw2_64, = torch.autograd.grad(gx64, w64, ggx64)                  # d <conv^T(gy, w), ggx> / dw

        x, w = dev(x64.detach(), True), dev(w64.detach(), True)
        y = gradfix.conv2d(x, w, m)
        gx, gw = torch.autograd.grad(y, (x, w), dev(gy64), create_graph=True)
        gw2, = torch.autograd.grad(gx, w, dev(ggx64))
        n_fwd, n_px = cin * k * k, B * y64.shape[2] * y64.shape[3]

        def check(got, want, n, scale, what):
            err = float((got.detach().cpu().double() - want.detach()).abs().max())
            bound = n * EPS32 * scale
            print(mode, k, (B, cin, cout, H), what, "error", err, "bound", bound)
            assert got.dtype == torch.float32 and got.shape == want.shape
            assert err <= bound, (what, err, bound)

        xn = float(x64.detach().flatten(1).norm(dim=1).max())
        wn = float(w64.detach().norm())
        gn = float(gy64.flatten(1).norm(dim=1).max())
        ggn = float(ggx64.flatten(1).norm(dim=1).max())
        check(y, y64, n_fwd, xn * wn, "forward")
        check(gx, gx64, cout * k * k, gn * wn, "data gradient")
        check(gw, gw64, n_px, float(gy64.norm()) * float(x64.detach().norm()), "weight gradient")
        check(gw2, gw2_64, n_px, float(gy64.norm()) * float(ggx64.norm()), "weight gradient, second backward")

        # <conv(x, w), gy> = <x, conv^T(gy, w)>  and  <wgrad(gy, x), w'> = <conv(x, w'), gy>
        lhs = float((y.detach().double() * dev(gy64).double()).sum())
        rhs = float((x.detach().double() * gx.detach().double()).sum())
        rel = abs(lhs - rhs) / (float(y.detach().double().norm()) * float(gy64.norm()))
        print("adjoint identity, relative", rel)
        assert rel <= max(n_fwd, cout * k * k) * EPS32
        w2 = dev(torch.randn(w64.shape, generator=g) / n_fwd ** 0.5)
        lhs = float((gw.detach().double() * w2.double()).sum())
        rhs = float((gradfix.conv2d(x.detach(), w2, m).double() * dev(gy64).double()).sum())
        rel = abs(lhs - rhs) / (float(gw.detach().double().norm()) * float(w2.double().norm()))
        print("bilinearity, relative", rel)
        assert rel <= max(n_fwd, n_px) * EPS32


def test_weight_gradient_ends_the_chain(pkg):
    gradfix = pkg[1]
    x, w = dev(torch.randn(2, 8, 4, 4), True), dev(torch.randn(8, 8, 3, 3), True)
    gw, = torch.autograd.grad(gradfix.conv2d(x, w, gradfix.PLAIN).sum(), w, create_graph=True)
    with pytest.raises(RuntimeError, match="gradient of a weight gradient is not built"):
        gw.sum().backward()
    with gradfix.no_weight_gradients():
        y = gradfix.conv2d(x, w, gradfix.PLAIN)
        gx, gw = torch.autograd.grad(y.sum(), (x, w), allow_unused=True)
    assert gw is None and gx is not None


def test_conv_bias_act_trains_and_differentiates_twice(pkg):
    gradfix = pkg[1]
    g = torch.Generator().manual_seed(5)
    x64 = torch.randn(2, 16, 24, 24, generator=g).double().requires_grad_(True)       # B H W >= 1024: the fused form
    w64 = (torch.randn(24, 16, 3, 3, generator=g) / 12).double().requires_grad_(True)
    b64 = (0.1 * torch.randn(24, generator=g)).double().requires_grad_(True)
    gy64, ggx64 = torch.randn(2, 24, 24, 24, generator=g).double(), torch.randn(2, 16, 24, 24, generator=g).double()

    def run(x, w, b, gy, ggx, fused):
        if fused:
            y = gradfix.conv_bias_act(x, w, b, gradfix.PLAIN, 0.2, 2 ** 0.5)
        else:
            y = F.leaky_relu(F.conv2d(x, w, padding=1) + b.view(1, -1, 1, 1), 0.2) * 2 ** 0.5
        gx, gw, gb = torch.autograd.grad(y, (x, w, b), gy, create_graph=True)
        gw2, = torch.autograd.grad(gx, w, ggx)
        return y, gx, gw, gb, gw2

    want = run(x64, w64, b64, gy64, ggx64, False)
    got = run(dev(x64.detach(), True), dev(w64.detach(), True), dev(b64.detach(), True), dev(gy64), dev(ggx64), True)
    # a pre-activation nearer to zero than its float32 error (144 terms of size <= 1/12: below 144 eps32 / 12 = 1.4e-6)
    # could take the other slope on the device; the draw has none
    safe = (F.conv2d(x64, w64, padding=1) + b64.view(1, -1, 1, 1)).detach().abs().min() > 2e-6
    assert bool(safe), "the draw has a pre-activation at the kink"
    for name, a, b, n in zip(("y", "gx", "gw", "gb", "gw2"), got, want, (144, 216, 1152, 1152, 1152)):
        err = float((a.detach().cpu().double() - b.detach()).abs().max())
        bound = n * EPS32 * max(1.0, float(b.detach().abs().max()))
        print(name, "error", err, "bound", bound)
        assert err <= bound, name


# ------------------------------------------------------------------------------------------ minibatch stddev
MB_SHAPES = [(8, 512, 4, 4, 1), (4, 8, 4, 4, 1), (2, 8, 4, 4, 1), (1, 8, 4, 4, 1), (8, 8, 4, 4, 2)]


def mb_results(fn, x, gout, ggx):
    """(out, gx, ggout, xg) of a stddev function: forward, backward, and the backward of the backward."""
    x = x.clone().requires_grad_(True)
    gout = gout.clone().requires_grad_(True)
    out = fn(x)
    gx, = torch.autograd.grad(out, x, gout, create_graph=True)
    ggout, xg = torch.autograd.grad(gx, (gout, x), ggx, allow_unused=True)
    xg = torch.zeros_like(x) if xg is None else xg
    return [t.detach() for t in (out, gx, ggout, xg)]


@pytest.mark.parametrize("B,C,H,W,feat", MB_SHAPES)
def test_minibatch_stddev(pkg, B, C, H, W, feat):
    """fwd, bwd, bwd2 against the float64 statement; bound: 4 x the error of the float32 torch composition on the
    GPU in the same case (the rule of the project's other small reduction kernels)."""
    mb = pkg[2]
    g = torch.Generator().manual_seed(B * 100 + C)
    x = torch.randn(B, C, H, W, generator=g)
    gout, ggx = torch.randn(B, C + feat, H, W, generator=g), torch.randn(B, C, H, W, generator=g)
    want = mb_results(lambda t: dc.mbstd(t, feat), x.double(), gout.double(), ggx.double())
    comp = mb_results(lambda t: dc.mbstd(t, feat), x.cuda(), gout.cuda(), ggx.cuda())
    assert mb.supported(x.cuda(), 4, feat)
    got = mb_results(lambda t: mb.minibatch_stddev(t, feat), x.cuda(), gout.cuda(), ggx.cuda())
    again = mb_results(lambda t: mb.minibatch_stddev(t, feat), x.cuda(), gout.cuda(), ggx.cuda())
    for name, a, c, w, r in zip(("fwd", "bwd", "bwd2 gout", "bwd2 x"), got, comp, want, again):
        err = float((a.cpu().double() - w).abs().max())
        ref = float((c.cpu().double() - w).abs().max())
        print((B, C, H, W, feat), name, "kernel error", err, "composition error", ref)
        assert a.shape == w.shape and torch.equal(a, r)
        assert err <= 4 * ref or err == 0.0, (name, err, ref)


# -------------------------------------------------------------------------------------------------- loss heads
@pytest.mark.parametrize("B", [1, 16])
def test_loss_heads(pkg, B):
    dtrain = pkg[0]
    g = torch.Generator().manual_seed(B)
    real, fake = 3 * torch.randn(B, 1, generator=g), 3 * torch.randn(B, 1, generator=g)
    real[0], fake[0] = 40.0, 40.0                      # softplus(40), softplus(-40): the overflow-safe form
    if B > 2:
        real[1], fake[1], real[2] = -40.0, -40.0, 0.0
    r64, f64 = real.double().requires_grad_(True), fake.double().requires_grad_(True)
    l64 = dc.d_logistic(r64, f64)
    gr64, gf64 = torch.autograd.grad(l64, (r64, f64))
    r, f = dev(real, True), dev(fake, True)
    loss, stats = dtrain.d_logistic(r, f)
    gr, gf = torch.autograd.grad(loss, (r, f))
    loss2, stats2 = dtrain.d_logistic(r, f)
    assert torch.equal(loss, loss2) and torch.equal(stats, stats2)
    want = [float(l64), float(r64.mean()), float(f64.mean()), float(torch.sign(r64).sum())]
    # each mean of B terms of size <= 40 + log 2 in float32: (B + 4) eps32 per unit of the largest term
    tol = (B + 4) * EPS32 * 41.0
    print("stats", stats.tolist(), "want", want)
    assert np.abs(np.array(stats.tolist()) - want).max() <= tol and float(loss) == float(stats[0])
    assert float((gr.cpu().double() - gr64).abs().max()) <= 4 * EPS32 / B
    assert float((gf.cpu().double() - gf64).abs().max()) <= 4 * EPS32 / B

    grad = torch.randn(B, 3, 40, 41, generator=g)      # n = 4920: two chunks, the second partly filled
    g64 = grad.double().requires_grad_(True)
    per64 = dc.r1_per_sample(g64)
    gg64, = torch.autograd.grad(per64.mean(), g64)
    gd = dev(grad, True)
    mean, per = dtrain.r1_penalty(gd)
    gg, = torch.autograd.grad(mean, gd)
    mean2, per2 = dtrain.r1_penalty(gd)
    assert torch.equal(mean, mean2) and torch.equal(per, per2)
    n = grad[0].numel()
    assert float((per.cpu().double() - per64.detach()).abs().max()) <= n * EPS32 * float(per64.max()) / 16
    assert abs(float(mean) - float(per64.mean())) <= (n / 16 + B) * EPS32 * float(per64.max())
    assert float((gg.cpu().double() - gg64).abs().max()) <= 2 * EPS32 * float(gg64.abs().max())


# ------------------------------------------------------------------------------------------ whole discriminator
@pytest.fixture(scope="module")
def d16(pkg):
    d = pkg[3](dc.SIZE, channel_multiplier=dc.CHANNEL_MULTIPLIER)
    dc.fill_weights(d)
    return d.cuda(), dc.draw_like(d, dc.PROBE_SEED)


def native_passes(pkg, d, real, fake):
    dtrain, gradfix = pkg[0], pkg[1]
    with gradfix.use():
        lg = dc.logistic_pass(d, real, fake, dtrain.d_logistic_loss)
        rp = dc.r1_pass(d, real, loss_fn=dtrain.d_r1_loss)
    return lg, rp


@pytest.mark.parametrize("name", list(dc.CASES))
def test_whole_discriminator_against_the_reference(pkg, fx, d16, name):
    """Every stored quantity of both passes within dtrain_cases.bound: MULTIPLE x its e32, e32 floored at one float32
    rounding of the quantity."""
    d, probe = d16
    lg, rp = native_passes(pkg, d, dev(fx[f"{name}.real"]), dev(fx[f"{name}.fake"]))
    got = {"real_pred": lg["real_pred"], "fake_pred": lg["fake_pred"], "loss": lg["loss"],
           "r1.real_pred": rp["real_pred"], "r1.grad_real": rp["grad_real"], "r1.per_sample": rp["per_sample"],
           "r1.r1": rp["r1"]}
    got = {k: v.cpu().double().numpy() for k, v in got.items()}
    got["log.norms"], got["log.proj"] = dc.summarize(lg["grads"], probe)
    got["r1.norms"], got["r1.proj"] = dc.summarize(rp["grads"], probe)
    worst = {}
    for k, v in got.items():
        want, e32 = fx[f"{name}.{k}"], float(fx[f"{name}.e32_{k}"])
        err = float(np.abs(v.reshape(want.shape) - want).max())
        print(name, k, "error", err, "e32", e32, "ratio", err / e32, "bound", dc.bound(want, e32))
        if err > dc.bound(want, e32):
            worst[k] = (err, dc.bound(want, e32))
    assert not worst, worst


def test_every_parameter_gradient_at_d8(pkg):
    """D(8), B = 8 (below the size rule: the unfused route): every element of every parameter gradient of both passes
    against this package's CPU float64 route.  Bound per tensor: MULTIPLE x the distance of the CPU float32 route from
    the CPU float64 route for that tensor (measured here, as e32 is in the fixture), and no tighter than one float32
    rounding of the tensor's largest entry."""
    dtrain, gradfix, _, D = pkg
    d64 = dc.fill_weights(D(8, channel_multiplier=1).double())
    rs = np.random.RandomState(7)
    real, fake = np.tanh(rs.standard_normal((8, 3, 8, 8))), np.tanh(rs.standard_normal((8, 3, 8, 8)))
    real, fake = real.astype(np.float32), fake.astype(np.float32)
    t = torch.from_numpy
    want = (dc.logistic_pass(d64, t(real).double(), t(fake).double()), dc.r1_pass(d64, t(real).double()))
    d32 = dc.fill_weights(D(8, channel_multiplier=1))
    cpu32 = (dc.logistic_pass(d32, t(real), t(fake)), dc.r1_pass(d32, t(real)))
    got = native_passes(pkg, dc.fill_weights(D(8, channel_multiplier=1)).cuda(), dev(real), dev(fake))
    bad = {}
    for tag, w, c, g in zip(("logistic", "r1"), want, cpu32, got):
        for n in w["grads"]:
            e32 = float((c["grads"][n].double() - w["grads"][n]).abs().max())
            err = float((g["grads"][n].cpu().double() - w["grads"][n]).abs().max())
            bound = dc.MULTIPLE * max(e32, EPS32 * float(w["grads"][n].abs().max()))
            print(tag, n, "error", err, "cpu float32 error", e32, "bound", bound)
            if err > bound:
                bad[(tag, n)] = (err, bound)
    assert not bad, bad


def test_r1_needs_the_feature(pkg, fx, d16):
    """With the switch off the R1 pass on the GPU does not see the convolutions in its second backward (their
    backward calls the kernels outside autograd): the double backward raises or gives wrong weight gradients — which of
    the two is printed (on an MI355X: wrong, without an error).  With the switch on it matches the fixture."""
    dtrain, gradfix = pkg[0], pkg[1]
    d, probe = d16
    real = dev(fx["b4.real"])
    want = fx["b4.r1.norms"]
    try:
        rp = dc.r1_pass(d, real, loss_fn=dtrain.d_r1_loss)
        norms, _ = dc.summarize(rp["grads"], probe)
        off = "wrong: largest deviation of a gradient norm %.3g of the largest norm" % (
            float(np.abs(norms - want).max()) / float(want.max()))
        wrong = float(np.abs(norms - want).max()) > 1e3 * float(fx["b4.e32_r1.norms"])
    except (RuntimeError, KeyError, AttributeError) as e:
        off, wrong = "raises: %s" % str(e).splitlines()[0], True
    print("switch off:", off)
    assert wrong
    with gradfix.use():
        rp = dc.r1_pass(d, real, loss_fn=dtrain.d_r1_loss)
    norms, _ = dc.summarize(rp["grads"], probe)
    assert float(np.abs(norms - want).max()) <= dc.bound(want, fx["b4.e32_r1.norms"])


def test_two_trainer_steps(pkg, fx):
    """i = 0 (with R1) and i = 1 (without) at D(16), B = 4: the weights against a float64 CPU trainer (torch.optim.Adam
    and the statements); per parameter within dtrain_cases.bound of the reference float32 trainer's own deviation."""
    dtrain, _, _, D = pkg
    steps = []
    for off, i in ((100, 0), (200, 1)):
        r, f = dc.images(4, dc.IMAGE_SEED + off)
        steps.append((r, f, i))
    d64 = dc.fill_weights(D(dc.SIZE, channel_multiplier=1).double())
    want = dc.reference_trainer(d64, [(torch.from_numpy(r).double(), torch.from_numpy(f).double(), i)
                                      for r, f, i in steps])
    d = dc.fill_weights(D(dc.SIZE, channel_multiplier=1)).cuda()
    trainer = dtrain.DiscriminatorTrainer(d)
    for r, f, i in steps:
        out = trainer.step(dev(r), dev(f), i)
        assert all(torch.isfinite(v).item() for v in out.values())
    bad = {}
    for (n, p), e32 in zip(d.named_parameters(), fx["trainer.e32"]):
        err = float((p.detach().cpu().double() - want[n]).abs().max())
        print(n, "error", err, "e32", float(e32), "ratio", err / float(e32))
        if err > dc.bound(want[n], e32):
            bad[n] = (err, float(e32))
    assert not bad, bad
