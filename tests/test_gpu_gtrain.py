"""Generator training on the GPU: the twice-differentiable modulated convolution (op/conv2d_gradfix.py), the
modulated weight gradient, loss heads and EMA (csrc/gtrain.hip), the whole generator against the reference's float64
fixture (tests/golden/gtrain.npz), every parameter gradient against this package's CPU float64 route, and two trainer
steps.  Statements and bounds: gtrain_cases.py.

Bound of the convolution-shaped quantities: a float32 dot product of n terms, accumulated in float32 in any order, is
within n * eps32 * sum |terms| of the exact one (the rule of test_gpu_dtrain.py).  Every quantity here is a sum of
products of the inputs with coefficients +1, so sum |terms| of each output element is the same float64 computation on
the inputs' absolute values (and 1 / |demod| for the division), and a chain of reductions (a second-order result: two
convolutions and a row pass) is within (n_1 + n_2 + ...) * eps32 * sum |terms| to first order: the rule applied to
both factors.  n of a first-order result is the length of its own reduction (`own_length`: y and gx one convolution,
gw the pixels, gs and gd a convolution and a row sum), plus 4 for the roundings of the scale multiplications and the
division; n of a second-order result is the sum of the lengths of every reduction its chain can hold, plus 16
(`chain_length`)."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dtrain_cases as dc
import gtrain_cases as gc

pytestmark = pytest.mark.gpu

EPS32 = float(np.finfo(np.float32).eps)
CONV_SHAPES = [(2, 3, 16), (2, 16, 24), (2, 513, 8)]     # tests/test_gpu_dtrain.py's


@pytest.fixture(scope="module")
def pkg():
    import gan2shape_amd  # noqa: F401
    from gan2shape_amd import gtrain, lib
    from gan2shape_amd.op import conv2d_gradfix
    from gan2shape_amd.stylegan2 import Discriminator, Generator
    lib.load()
    return gtrain, conv2d_gradfix, lib, Generator, Discriminator


@pytest.fixture(scope="module")
def fx(golden):
    return golden("gtrain")


def dev(a, grad=False):
    return torch.as_tensor(a).float().cuda().requires_grad_(grad)


def r32(shape, g, scale=1.0):
    """float64 values that float32 holds exactly."""
    return (scale * torch.randn(shape, generator=g, dtype=torch.float64)).float().double()


# ------------------------------------------------------------------------------------ modulated convolution node
def modconv64(x, w, s, demod, mode):
    xs = x if s is None else x * s[:, :, None, None]
    k = w.shape[2]
    if mode == "PLAIN":
        y = F.conv2d(xs, w, padding=k // 2)
    elif mode == "DOWN2":
        y = F.conv2d(xs, w, stride=2)
    else:
        y = F.conv_transpose2d(xs, w.transpose(0, 1), stride=2)
    return y if demod is None else y * demod[:, :, None, None]


def node_results(fn, x, w, s, demod, gy, ggx, ggs):
    """Forward, the four gradients, and the gradients to (w, s, x) of <gx, ggx> + <gs, ggs>.  Missing scales: None."""
    leaves = [t.clone().requires_grad_(True) if t is not None else None for t in (x, w, s, demod)]
    x, w, s, demod = leaves
    y = fn(x, w, s, demod)
    present = [t for t in leaves if t is not None]
    grads = list(torch.autograd.grad(y, present, gy, create_graph=True))
    gx, gw = grads[0], grads[1]
    gs = grads[2] if s is not None else None
    gd = grads[-1] if demod is not None else None
    f = (gx * ggx).sum() + ((gs * ggs).sum() if gs is not None else 0)
    second_in = [w, x] + ([s] if s is not None else [])
    second = torch.autograd.grad(f, second_in, allow_unused=True)
    out = {"y": y, "gx": gx, "gw": gw, "gs": gs, "gd": gd, "2.w": second[0], "2.x": second[1],
           "2.s": second[2] if s is not None else None}
    return {k: (None if v is None else v.detach()) for k, v in out.items()}


def node_case(mode, k, B, cin, cout, side, scales, seed):
    g = torch.Generator().manual_seed(seed)
    H = side + 1 if mode == "DOWN2" else side      # DOWN2 takes (H - k) even, as after the blur pad: 5, 9
    x = r32((B, cin, H, H), g)
    w = r32((cout, cin, k, k), g, 1 / (cin * k * k) ** 0.5)
    s = (1 + 0.5 * r32((B, cin), g)) if scales in ("s", "both") else None
    demod = (0.5 + torch.rand((B, cout), generator=g, dtype=torch.float64)).float().double() if scales == "both" else None
    y = modconv64(x, w, s, demod, mode)
    gy, ggx = r32(y.shape, g), r32(x.shape, g)
    ggs = r32((B, cin), g) if s is not None else None
    return x, w, s, demod, gy, ggx, ggs


def chain_length(x, y, w):
    B, cin, H, W = x.shape
    cout, _, k, _ = w.shape
    return cin * k * k + cout * k * k + B * min(H * W, y.shape[2] * y.shape[3]) + H * W + y.shape[2] * y.shape[3] + 16


def own_length(name, x, y, w):
    """Terms of the reduction behind one element of a first-order result, plus 4 (scales and division)."""
    B, cin, H, W = x.shape
    cout, _, k, _ = w.shape
    hw_in, hw_out = H * W, y.shape[2] * y.shape[3]
    return {"y": cin * k * k, "gx": cout * k * k, "gw": B * min(hw_in, hw_out), "gs": cout * k * k + hw_in,
            "gd": cin * k * k + hw_out}[name] + 4


# 4 x 4: two samples in one 32-pixel K tile; UP2 from 4: a 9 x 9 output, boundaries inside a tile; 8 x 8: several K
# tiles, so (2, 513, 8) runs its nine M tiles with a split pixel sum
NODE_SIDES = [4, 8]


@pytest.mark.parametrize("scales", ["none", "s", "both"])
@pytest.mark.parametrize("mode", ["PLAIN", "DOWN2", "UP2"])
@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("B,cin,cout", CONV_SHAPES)
def test_modulated_convolution_node(pkg, scales, mode, k, B, cin, cout):
    gradfix = pkg[1]
    m = {"PLAIN": gradfix.PLAIN, "DOWN2": gradfix.DOWN2, "UP2": gradfix.UP2}[mode]
    for side in NODE_SIDES:
        case = node_case(mode, k, B, cin, cout, side, scales, 1000 * cin + 10 * side + k)
        x, w, s, demod = case[:4]
        want = node_results(lambda *a: modconv64(*a, mode), *case)
        absd = [None if t is None else t.abs() for t in case]
        mag = node_results(lambda *a: modconv64(*a, mode), *absd)
        got = node_results(lambda *a: gradfix.modulated_conv2d(*a, m), *[None if t is None else dev(t) for t in case])
        for name, wv in want.items():
            n = chain_length(x, want["y"], w) if name.startswith("2.") else own_length(name, x, want["y"], w)
            if wv is None:
                assert got[name] is None
                continue
            gv = got[name]
            assert gv.dtype == torch.float32 and gv.shape == wv.shape, name
            err = (gv.cpu().double() - wv).abs()
            ratio = float((err / (n * EPS32 * mag[name]).clamp_min(1e-300)).max())
            print(scales, mode, k, (B, cin, cout, x.shape[2]), name, "n", n, "max error", float(err.max()),
                  "error / bound", ratio)
            assert ratio <= 1.0, (name, ratio)


def test_modulated_weight_gradient_ends_the_chain(pkg):
    gradfix = pkg[1]
    x, w = dev(torch.randn(2, 8, 4, 4), True), dev(torch.randn(8, 8, 3, 3), True)
    s, d = dev(torch.rand(2, 8) + 0.5, True), dev(torch.rand(2, 8) + 0.5, True)
    gw, = torch.autograd.grad(gradfix.modulated_conv2d(x, w, s, d, gradfix.UP2).sum(), w, create_graph=True)
    with pytest.raises(RuntimeError, match="gradient of a weight gradient is not built"):
        gw.sum().backward()
    calls = []
    orig = gradfix._modconv_wgrad_launch
    gradfix._modconv_wgrad_launch = lambda *a: calls.append(1) or orig(*a)
    try:
        with gradfix.no_weight_gradients():
            y = gradfix.modulated_conv2d(x, w, s, d, gradfix.PLAIN)
            gx, gw, gs = torch.autograd.grad(y.sum(), (x, w, s), allow_unused=True)
        assert gw is None and gx is not None and gs is not None and not calls
        torch.autograd.grad(gradfix.modulated_conv2d(x, w, s, d, gradfix.PLAIN).sum(), w)
        assert calls == [1]
    finally:
        gradfix._modconv_wgrad_launch = orig
    with pytest.raises(RuntimeError, match="float32 only"):
        gradfix.modulated_conv2d(x.half(), w.half(), None, None, gradfix.PLAIN)


def test_up2_conv2d(pkg):
    gradfix = pkg[1]
    g = torch.Generator().manual_seed(3)
    x64, w64 = r32((2, 16, 4, 4), g).requires_grad_(True), r32((24, 16, 3, 3), g, 1 / 12).requires_grad_(True)
    y64 = F.conv_transpose2d(x64, w64.transpose(0, 1), stride=2)
    gy = r32(y64.shape, g)
    gx64, gw64 = torch.autograd.grad(y64, (x64, w64), gy)
    x, w = dev(x64.detach(), True), dev(w64.detach(), True)
    y = gradfix.conv2d(x, w, gradfix.UP2)
    gx, gw = torch.autograd.grad(y, (x, w), dev(gy))
    for name, a, b, n in (("y", y, y64, 144), ("gx", gx, gx64, 216), ("gw", gw, gw64, 32)):
        err = float((a.detach().cpu().double() - b.detach()).abs().max())
        bound = n * EPS32 * float(b.detach().abs().max()) * 4
        print(name, err, bound)
        assert a.shape == b.shape and err <= bound


# -------------------------------------------------------------------------------------- the weight gradient alone
def wgrad_launch(lib, A, sa, G, sg, k, stride, pad, plain=False):
    L = lib.load()
    B, Ca, PH, PW = A.shape
    _, Cg, GH, GW = G.shape
    dw = torch.full((Ca, Cg, k, k), float("nan"), device="cuda")
    p = lib.ptr
    if plain:
        lib.check(L.g2s_conv2d_wgrad(p(A), p(G), p(dw), B, Ca, Cg, PH, PW, GH, GW, k, stride, pad, 0, 1, lib.stream()))
    else:
        lib.check(L.g2s_modconv_wgrad(p(A), p(sa), p(G), p(sg), p(dw), B, Ca, Cg, PH, PW, GH, GW, k, stride, pad, 0,
                                      lib.stream()))
    return dw


@pytest.mark.parametrize("mode", ["PLAIN", "DOWN2", "UP2"])
@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("B,cin,cout", CONV_SHAPES)
def test_modconv_wgrad_kernel(pkg, mode, k, B, cin, cout):
    lib = pkg[2]
    for side in NODE_SIDES:
        x, w, s, demod, gy, _, _ = node_case(mode, k, B, cin, cout, side, "both", 77 * cin + side + k)
        if mode == "UP2":
            A, sa, G, sg, stride, pad = x, s, gy, demod, 2, 0
        else:
            A, sa, G, sg, stride, pad = gy, demod, x, s, 1 if mode == "PLAIN" else 2, k // 2 if mode == "PLAIN" else 0

        def exact(A, sa, G, sg):
            wv = torch.zeros(A.shape[1], G.shape[1], k, k, dtype=torch.float64, requires_grad=True)
            out = F.conv2d(G * sg[:, :, None, None], wv, stride=stride, padding=pad)
            return torch.autograd.grad(out, wv, A * sa[:, :, None, None])[0]
        want, mag = exact(A, sa, G, sg), exact(A.abs(), sa.abs(), G.abs(), sg.abs())
        n = B * A.shape[2] * A.shape[3] + 4
        dA, dsa, dG, dsg = dev(A), dev(sa), dev(G), dev(sg)
        prev = lib.set_deterministic(False)
        try:
            for det in (False, True):
                lib.set_deterministic(det)
                got = wgrad_launch(lib, dA, dsa, dG, dsg, k, stride, pad)
                ratio = float(((got.cpu().double() - want).abs() / (n * EPS32 * mag).clamp_min(1e-300)).max())
                print(mode, k, (B, cin, cout, side), "deterministic" if det else "split", "error / bound", ratio)
                assert ratio <= 1.0
            assert torch.equal(got, wgrad_launch(lib, dA, dsa, dG, dsg, k, stride, pad))
            assert torch.equal(wgrad_launch(lib, dA, None, dG, None, k, stride, pad),
                               wgrad_launch(lib, dA, None, dG, None, k, stride, pad, plain=True))
        finally:
            lib.set_deterministic(prev)


# ---------------------------------------------------------------------------------------------- heads and EMA
@pytest.mark.parametrize("B,L,D", [(1, 1, 1), (2, 6, 64), (16, 14, 512)])
def test_path_penalty_kernel(pkg, B, L, D):
    """Against the float64 composition, within 4 x the float32 composition's own error on the GPU in the same case
    (the rule of the stddev kernels)."""
    gtrain = pkg[0]
    g = torch.Generator().manual_seed(B * L + D)
    grad = torch.randn(B, L, D, generator=g) * (0.5 + torch.rand(B, 1, 1, generator=g))
    mean0 = 0.7

    def run(t, fn):
        t = t.clone().requires_grad_(True)
        pen, pm, lengths = fn(t, torch.tensor(mean0, dtype=t.dtype, device=t.device))
        dg, = torch.autograd.grad(pen, t)
        return [v.detach() for v in (pen, pm, lengths, lengths.mean(), dg)]
    want = run(grad.double(), gc.path_penalty)
    comp = run(grad.cuda(), gc.path_penalty)
    got = run(grad.cuda(), gtrain.path_penalty)
    again = run(grad.cuda(), gtrain.path_penalty)
    for name, a, c, w, r in zip(("penalty", "path mean", "lengths", "mean length", "gradient"), got, comp, want, again):
        err = float((a.cpu().double() - w).abs().max())
        ref = float((c.cpu().double() - w).abs().max())
        print((B, L, D), name, "kernel error", err, "composition error", ref)
        assert a.shape == w.shape and torch.equal(a, r)
        assert err <= 4 * ref or err == 0.0, (name, err, ref)


@pytest.mark.parametrize("B", [1, 16])
def test_g_nonsaturating_kernel(pkg, B):
    gtrain = pkg[0]
    g = torch.Generator().manual_seed(B)
    fake = 3 * torch.randn(B, 1, generator=g)
    fake[0] = 40.0
    if B > 2:
        fake[1], fake[2] = -40.0, 0.0

    def run(t, fn):
        t = t.clone().requires_grad_(True)
        loss = fn(t)
        return loss.detach(), torch.autograd.grad(loss, t)[0]
    want, comp = run(fake.double(), gc.g_nonsaturating), run(fake.cuda(), gc.g_nonsaturating)
    got, again = run(fake.cuda(), gtrain.g_nonsaturating_loss), run(fake.cuda(), gtrain.g_nonsaturating_loss)
    for name, a, c, w, r in zip(("loss", "gradient"), got, comp, want, again):
        err = float((a.cpu().double() - w).abs().max())
        ref = float((c.cpu().double() - w).abs().max())
        print(B, name, "kernel error", err, "composition error", ref)
        assert a.shape == w.shape and torch.equal(a, r)
        assert err <= 4 * ref or err == 0.0, (name, err, ref)


def test_ema_accumulate_kernel(pkg):
    """dst * decay + src * (1 - decay): three roundings, so within 3 eps32 (|dst| + |src|) elementwise.  The tensors
    lie in one buffer with guard floats between them: the issue's five sizes at offsets that are no multiple of 16
    bytes (the scalar path), then one of four chunks at a 16-byte boundary (the vector path, the bisection with a base
    above 0).  A second call on views that start at the same addresses with other lengths must not reuse the table."""
    gtrain = pkg[0]
    sizes = [1, 3, 513, 4097, 2359296]
    aligned = 3 * 8192 + 4           # one more tensor, at a 16-byte boundary: four chunks of the 16-byte path
    g = torch.Generator().manual_seed(11)
    guard = 5
    views, at = [], guard
    for n in sizes:
        views.append((at, n))
        at += n + guard
    at += -at % 4
    views.append((at, aligned))
    total = at + aligned + guard
    dst_buf, src_buf = torch.randn(total, generator=g), torch.randn(total, generator=g)
    dst_dev, src_dev = dst_buf.cuda(), src_buf.cuda()
    assert all((a % 4 != 0) for a, _ in views[:-1]) and dst_dev.data_ptr() % 16 == 0 and src_dev.data_ptr() % 16 == 0
    decay = gc.EMA_DECAY
    gtrain.ema_accumulate([dst_dev[a:a + n] for a, n in views], [src_dev[a:a + n] for a, n in views], decay)
    out = dst_dev.cpu()
    inside = torch.zeros(total, dtype=torch.bool)
    for a, n in views:
        inside[a:a + n] = True
        want = dst_buf[a:a + n].double() * decay + src_buf[a:a + n].double() * (1 - decay)
        err = (out[a:a + n].double() - want).abs()
        bound = 3 * EPS32 * (dst_buf[a:a + n].abs() + src_buf[a:a + n].abs()).double()
        print(n, "largest error / bound", float((err / bound).max()))
        assert bool((err <= bound).all())
    assert torch.equal(out[~inside], dst_buf[~inside]) and torch.equal(src_dev.cpu(), src_buf)
    # the same start addresses, shorter: a table of its own, the tails stay
    before = dst_dev.cpu()
    a0, n0 = views[2]
    gtrain.ema_accumulate([dst_dev[a0:a0 + 10]], [src_dev[a0:a0 + 10]], decay)
    gtrain.ema_accumulate([dst_dev[a0:a0 + n0]], [src_dev[a0:a0 + n0]], 0.0)
    after = dst_dev.cpu()
    assert torch.equal(after[a0:a0 + n0], src_buf[a0:a0 + n0])          # decay 0: dst = src over all n0 elements
    keep = torch.ones(total, dtype=torch.bool)
    keep[a0:a0 + n0] = False
    assert torch.equal(after[keep], before[keep])
    # aligned tensors of their own: the 16-byte path
    a, b = torch.randn(4097, generator=g), torch.randn(4097, generator=g)
    da, db = a.cuda(), b.cuda()
    gtrain.ema_accumulate([da], [db], 0.999)
    want = a.double() * 0.999 + b.double() * (1 - 0.999)
    assert bool(((da.cpu().double() - want).abs() <= 3 * EPS32 * (a.abs() + b.abs()).double()).all())


# -------------------------------------------------------------------------------------------- whole generator
def nets(pkg, size=gc.SIZE, dtype=torch.float32):
    G, D = pkg[3], pkg[4]
    g = dc.fill_weights(G(size, gc.STYLE_DIM, gc.N_MLP, channel_multiplier=gc.CHANNEL_MULTIPLIER).to(dtype), gc.G_SEED)
    d = dc.fill_weights(D(size, channel_multiplier=gc.CHANNEL_MULTIPLIER).to(dtype), gc.D_SEED)
    return g, d.requires_grad_(False)


@pytest.fixture(scope="module")
def g16(pkg):
    g, d = nets(pkg)
    return g.cuda(), d.cuda(), dc.draw_like(g, gc.PROBE_SEED)


def native_passes(pkg, g, d, name, which=("ns", "path")):
    gtrain, gradfix = pkg[0], pkg[1]
    zs, maps, img = gc.inputs(name)
    inject = gc.CASES[name][2]
    like = torch.zeros((), device="cuda")
    out = {}
    with gradfix.use():
        if "ns" in which:
            out["ns"] = gc.nonsaturating_pass(g, d, gc.to(zs, like), gc.to(maps, like), inject,
                                              gtrain.g_nonsaturating_loss)
        if "path" in which:
            out["path"] = gc.path_pass(g, gc.to(zs, like), gc.to(maps, like), inject, gc.to([img], like)[0],
                                       loss_fn=gtrain.g_path_regularize)
    return out


def compare(fx, name, got, keys=None):
    worst, ratio = {}, 0.0
    for k, v in got.items():
        want, e32 = fx[f"{name}.{k}"], float(fx[f"{name}.e32_{k}"])
        err = float(np.abs(np.asarray(v, dtype=np.float64).reshape(want.shape) - want).max())
        floor = 0.5 * EPS32 * float(np.abs(want).max())
        ratio = max(ratio, err / max(e32, floor))
        print(name, k, "error", err, "e32", e32, "error / max(e32, rounding)", err / max(e32, floor))
        if err > gc.bound(want, e32):
            worst[k] = (err, gc.bound(want, e32))
    print(name, "largest ratio", ratio)
    return worst


@pytest.mark.parametrize("name", list(gc.CASES))
def test_whole_generator_against_the_reference(pkg, fx, g16, name):
    """Every stored quantity of both passes within gtrain_cases.bound: MULTIPLE x its e32, e32 floored at one float32
    rounding of the quantity."""
    g, d, probe = g16
    res = native_passes(pkg, g, d, name)
    ns, pp = res["ns"], res["path"]
    got = {"image": ns["image"], "loss": ns["loss"], "path.lengths": pp["lengths"], "path.path_mean": pp["path_mean"],
           "path.penalty": pp["penalty"]}
    got = {k: v.cpu().double().numpy() for k, v in got.items()}
    got["ns.norms"], got["ns.proj"] = gc.summarize(ns["grads"], probe)
    got["path.norms"], got["path.proj"] = gc.summarize(pp["grads"], probe)
    worst = compare(fx, name, got)
    assert not worst, worst


def test_every_parameter_gradient_at_g8(pkg):
    """G(8), B = 4: every element of every parameter gradient of both passes against this package's CPU float64 route.
    Bound per tensor: MULTIPLE x the distance of the CPU float32 route from the CPU float64 route for that tensor, no
    tighter than one float32 rounding of the tensor's largest entry."""
    gtrain = pkg[0]
    rs = np.random.RandomState(9)
    zs = [rs.standard_normal((4, gc.STYLE_DIM)).astype(np.float32)]
    maps = [rs.standard_normal((1, 1, r, r)).astype(np.float32) for r in (4, 8, 8)]
    img = rs.standard_normal((4, 3, 8, 8)).astype(np.float32)

    def passes(g, d, like, use):
        with pkg[1].use(use):
            ns = gc.nonsaturating_pass(g, d, gc.to(zs, like), gc.to(maps, like), None, gtrain.g_nonsaturating_loss)
            pp = gc.path_pass(g, gc.to(zs, like), gc.to(maps, like), None, gc.to([img], like)[0],
                              loss_fn=gtrain.g_path_regularize)
        return ns, pp
    want = passes(*nets(pkg, 8, torch.float64), torch.zeros((), dtype=torch.float64), False)
    cpu32 = passes(*nets(pkg, 8), torch.zeros(()), False)
    g, d = nets(pkg, 8)
    got = passes(g.cuda(), d.cuda(), torch.zeros((), device="cuda"), True)
    bad = {}
    for tag, w, c, r in zip(("nonsaturating", "path"), want, cpu32, got):
        for n in w["grads"]:
            e32 = float((c["grads"][n].double() - w["grads"][n]).abs().max())
            err = float((r["grads"][n].cpu().double() - w["grads"][n]).abs().max())
            bound = gc.MULTIPLE * max(e32, EPS32 * float(w["grads"][n].abs().max()))
            print(tag, n, "error", err, "cpu float32 error", e32, "bound", bound)
            if err > bound:
                bad[(tag, n)] = (err, bound)
    assert not bad, bad


def test_path_regularize_needs_the_feature(pkg, fx, g16):
    """With the switch off the generator's nodes call their kernels outside autograd in backward: the path pass on the
    GPU raises or gives gradients that miss the bound (which of the two is printed).  With it on, it passes."""
    gtrain = pkg[0]
    g, d, probe = g16
    want, e32 = fx["b2.path.norms"], fx["b2.e32_path.norms"]
    zs, maps, img = gc.inputs("b2")
    like = torch.zeros((), device="cuda")
    try:
        pp = gc.path_pass(g, gc.to(zs, like), gc.to(maps, like), None, gc.to([img], like)[0],
                          loss_fn=gtrain.g_path_regularize)
        norms, _ = gc.summarize(pp["grads"], probe)
        dev_ = float(np.abs(norms - want).max())
        off, wrong = "wrong: largest deviation of a gradient norm %.3g" % dev_, dev_ > gc.bound(want, e32)
    except (RuntimeError, KeyError, AttributeError) as e:
        off, wrong = "raises: %s" % str(e).splitlines()[0], True
    print("switch off:", off)
    assert wrong
    pp = native_passes(pkg, g, d, "b2", ("path",))["path"]
    norms, _ = gc.summarize(pp["grads"], probe)
    assert float(np.abs(norms - want).max()) <= gc.bound(want, e32)


def test_two_trainer_steps(pkg, fx):
    """i = 0 (with the path pass) and i = 1 at G(16), B = 4: the probe projections of the generator's and g_ema's
    parameters against the reference's float64 trainer, per parameter within gtrain_cases.bound of the reference
    float32 trainer's own deviation."""
    gtrain = pkg[0]
    g, d = nets(pkg)
    g, d = g.cuda(), d.cuda()
    g_ema = copy.deepcopy(g)
    start_d = {n: p.detach().clone() for n, p in d.named_parameters()}
    start_g = {n: p.detach().clone() for n, p in g.named_parameters()}
    like = torch.zeros((), device="cuda")
    trainer = gtrain.GeneratorTrainer(g, g_ema, d, batch=4)
    for (zs, maps, _), path_in, i in gc.trainer_inputs():
        kw = {}
        if path_in is not None:
            kw = dict(path_noise=gc.to(path_in[0], like), path_maps=gc.to(path_in[1], like),
                      image_noise=gc.to([path_in[2]], like)[0])
        out = trainer.step(i, noise=gc.to(zs, like), maps=gc.to(maps, like), **kw)
        assert all(torch.isfinite(v).item() for v in out.values())
    probe = dc.draw_like(g, gc.PROBE_SEED)
    bad, ratio = {}, 0.0
    for tag, net in (("g", g), ("g_ema", g_ema)):
        proj = gc.projections(net, probe)
        want, e32s = fx[f"trainer.{tag}"], fx[f"trainer.e32_{tag}"]
        for (n, _), p, w, e32 in zip(net.named_parameters(), proj, want, e32s):
            err = abs(p - w)
            ratio = max(ratio, err / max(float(e32), 0.5 * EPS32 * abs(w)))
            if err > gc.bound(w, e32):
                bad[(tag, n)] = (err, gc.bound(w, e32))
    print("trainer: largest error / max(e32, rounding)", ratio)
    assert not bad, bad
    for n, p in d.named_parameters():
        assert torch.equal(p, start_d[n]), n
    moved = [n for n, p in g_ema.named_parameters() if not torch.equal(p, start_g[n])]
    differs = [n for (n, p), q in zip(g_ema.named_parameters(), g.parameters()) if not torch.equal(p, q)]
    assert moved and differs
