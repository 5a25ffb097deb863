"""g2s_resample_sep (csrc/resample.hip; op/resample.py crop_resize on CUDA float32) against the float64 fixture
tests/golden/crop_resize.npz — the reference's utils.resize / utils.crop run as the three lines behind
`# FIXME: add back cropping` (tests/golden/make_crop_resize_golden.py) — and the crop inside step 2.

Bound, forward and gradient, every element: max |kernel - float64| <= max(4 x err32, floor).  err32 is the error of the
reference's own float32 composition against the float64 value (`.out32` against `.out`, `.gin32` against `.gin`); 4 is
the multiple the ADA and canon-mask tests use.  floor = (taps_y + taps_x + 2) eps32 max|x|: the kernel evaluates two
nested convex combinations (weights >= 0 summing to 1 for the forward; the transposed weights are bounded alike by
the band sums), each fmaf chain of k taps rounds k times and each weight carries one rounding from float64, so
(taps_y + 1) + (taps_x + 1) roundings of values no larger than max|x| bound the error where err32 happens to be tiny.

Step level: fused against composed under identical draws, at the tolerance tests/test_gpu_object_mask_steps.py holds
that pair to (rtol 1e-4, atol 1e-5 (1 + |value|))."""
import ctypes as C

import numpy as np
import pytest
import torch

import crop_resize_cases as cc
import model_cases as mc

pytestmark = pytest.mark.gpu

MULTIPLE = 4
EPS32 = float(np.finfo(np.float32).eps)


@pytest.fixture(scope="module")
def fixture(golden):
    return golden("crop_resize")


@pytest.fixture(scope="module")
def rs():
    import gan2shape_amd  # noqa: F401
    from gan2shape_amd.op import resample
    return resample


def launches(fn):
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA
               and not e.name.lower().startswith(("memcpy", "memset")))


def test_symbol_is_bound():
    from gan2shape_amd import lib
    assert "g2s_resample_sep" in lib.SIGNATURES and "g2s_resample_bands_check" in lib.SIGNATURES
    L = lib.load()
    assert L.g2s_resample_sep is not None and L.g2s_resample_max_taps() == 8


@pytest.mark.parametrize("name", list(cc.CASES))
def test_kernel_vs_float64_fixture(fixture, rs, name):
    gan, origin, crop, image, planes = cc.CASES[name]
    x64, g64 = cc.operands(fixture, name)
    t = rs.crop_resize_tables(gan, origin, crop, image, "cuda")
    x = x64.float().cuda().requires_grad_(True)
    y = rs.crop_resize(x, origin, crop, image)
    assert y.dtype == torch.float32 and y.is_cuda and tuple(y.shape) == (1, planes, image, image)
    gin, = torch.autograd.grad(y, x, g64.float().cuda())
    assert tuple(gin.shape) == (1, planes, gan, gan)
    for what, got, bands, operand in (("out", y.detach(), t.fwd, x64), ("gin", gin, t.tr, g64)):
        ref = fixture[f"{name}.{what}"]
        e32 = cc.max_err(fixture[f"{name}.{what}32"], ref)
        floor = (2 * bands.K + 2) * EPS32 * float(operand.abs().max())
        err = cc.max_err(got.cpu().numpy(), ref)
        print(f"[crop_resize gpu] {name} {what}: kernel max |err| {err:.3e} = {err / e32:.2f} x the reference's float32 "
              f"composition ({e32:.3e}); floor {floor:.3e}, bound {max(MULTIPLE * e32, floor):.3e}")
        assert err <= max(MULTIPLE * e32, floor)
    assert launches(lambda: rs.crop_resize(x.detach(), origin, crop, image)) == 1


@pytest.mark.parametrize("name", ["odd_crop_odd_margin_64_40_33_32", "small_40_30_21_16"])
def test_two_calls_are_bit_identical(fixture, rs, name):
    gan, origin, crop, image, _ = cc.CASES[name]
    x64, g64 = cc.operands(fixture, name)
    x, g = x64.float().cuda().requires_grad_(True), g64.float().cuda()
    runs = []
    for _ in range(2):
        y = rs.crop_resize(x, origin, crop, image)
        runs.append((y.detach(), torch.autograd.grad(y, x, g)[0]))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])


@pytest.mark.parametrize("name", ["down_crop_down_64_48_40_32", "small_40_30_21_16", "no_rows_dropped_24_24_24_32"])
def test_gradient_writes_exact_zeros_outside_the_crop(fixture, rs, name):
    gan, origin, crop, image, planes = cc.CASES[name]
    _, g64 = cc.operands(fixture, name)
    t = rs.crop_resize_tables(gan, origin, crop, image, "cuda")
    out = torch.full((1, planes, gan, gan), float("nan"), device="cuda")
    got = rs.resample_sep(g64.float().cuda(), t.tr, t.tr, out=out)
    assert got is out and not bool(torch.isnan(out).any())
    dropped = torch.tensor(t.tr.host[1] == 0)
    assert (int(dropped.sum()) == 0) == name.startswith("no_rows")
    outside = (dropped[:, None] | dropped[None, :]).cuda()
    vals = out[0, :, outside]
    assert bool((vals == 0).all()) and not bool(torch.signbit(vals).any())
    ref = torch.tensor(fixture[f"{name}.gin"])
    assert bool((ref[0, :, outside.cpu()] == 0).all())


def test_double_backward_is_the_forward_on_the_cotangent(fixture, rs):
    name = "up_crop_down_32_48_40_32"
    gan, origin, crop, image, planes = cc.CASES[name]
    x64, g64 = cc.operands(fixture, name)
    x = x64.float().cuda().requires_grad_(True)
    g = g64.float().cuda().requires_grad_(True)
    y = rs.crop_resize(x, origin, crop, image)
    gin, = torch.autograd.grad(y, x, g, create_graph=True)
    assert gin.requires_grad
    gen = torch.Generator("cuda").manual_seed(5)
    v = (torch.rand(1, planes, gan, gan, device="cuda", generator=gen) * 2 - 1).requires_grad_(True)
    gg, = torch.autograd.grad(gin, g, v, create_graph=True)
    assert torch.equal(gg, rs.crop_resize(v.detach(), origin, crop, image))        # the same launch, the same table
    # one order further: the derivative of that is the transposed launch again
    w = torch.rand(1, planes, image, image, device="cuda", generator=gen) * 2 - 1
    h, = torch.autograd.grad(gg, v, w)
    t = rs.crop_resize_tables(gan, origin, crop, image, "cuda")
    assert torch.equal(h, rs.resample_sep(w, t.tr, t.tr))


def test_call_records_into_a_graph(fixture, rs):
    """Stateless and on the caller's stream: a captured forward + backward replays onto new data."""
    name = "crop_up_32_32_24_32"
    gan, origin, crop, image, _ = cc.CASES[name]
    x64, g64 = cc.operands(fixture, name)
    x_new, g = x64.float().cuda().flip(3).contiguous(), g64.float().cuda()
    xr = x_new.clone().requires_grad_(True)
    want = rs.crop_resize(xr, origin, crop, image)
    want_gin, = torch.autograd.grad(want, xr, g)
    static = x64.float().cuda().requires_grad_(True)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):                # warm-up: library handle, the tables' upload
        torch.autograd.grad(rs.crop_resize(static, origin, crop, image), static, g)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = rs.crop_resize(static, origin, crop, image)
        gin, = torch.autograd.grad(out, static, g)
    with torch.no_grad():
        static.copy_(x_new)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out.detach(), want.detach()) and torch.equal(gin, want_gin)


def test_bad_tables_are_refused(rs):
    from gan2shape_amd import lib
    t = rs.crop_resize_tables(32, 32, 24, 32, "cuda")
    lo, ln, w = (a.copy() for a in t.fwd.host)
    n = len(lo)
    bad = []
    b = lo.copy()
    b[-1] = 32 - ln[-1] + 1
    bad.append((b, ln, w, 32))                                                    # the last band leaves the input
    b = lo.copy()
    b[0] = -1
    bad.append((b, ln, w, 32))                                                    # the first one starts before it
    bad.append((lo, ln, w, int(lo[-1] + ln[-1]) - 1))                             # an input shorter than the bands
    b = ln.copy()
    b[3] = w.shape[1] + 1
    bad.append((lo, b, w, 32))                                                    # more taps than the table holds
    bad.append((lo, np.minimum(ln, 8), np.zeros((n, 9), np.float32), 32))         # K above the kernel's cap of 8
    bad.append((lo[::-1].copy(), ln[::-1].copy(), w[::-1].copy(), 32))            # descending
    bad.append((lo * 3, ln, w, 200))                                              # gaps between consecutive bands
    for args in bad:
        with pytest.raises(ValueError):
            rs.make_bands(*args, device="cuda")
    x = torch.zeros(1, 2, 32, 32, device="cuda")
    with pytest.raises(ValueError):
        rs.resample_sep(x[:, :, :24], t.fwd, t.fwd)                               # the tables read 32 rows
    with pytest.raises(ValueError):
        rs.resample_sep(x.double(), t.fwd, t.fwd)
    with pytest.raises(ValueError):
        rs.resample_sep(x, t.fwd, t.fwd, out=torch.empty(1, 2, 32, 31, device="cuda"))
    # the C launcher itself: error codes, nothing launched
    L, p = lib.load(), lib.ptr
    y = torch.empty_like(x)
    tab = (p(t.fwd.lo), p(t.fwd.len), p(t.fwd.w))
    assert L.g2s_resample_sep(p(x), p(y), 2, 32, 32, 32, 32, *tab, 9, *tab, t.fwd.K, lib.stream()) < 0
    assert L.g2s_resample_sep(p(x), p(y), 2, 32, 32, 32, 32, *tab, t.fwd.K, *tab, 0, lib.stream()) < 0
    assert L.g2s_resample_sep(None, p(y), 2, 32, 32, 32, 32, *tab, t.fwd.K, *tab, t.fwd.K, lib.stream()) < 0
    assert L.g2s_resample_sep(p(x), p(y), 2, 32, 32, 32, 32, None, *tab[1:], t.fwd.K, *tab, t.fwd.K, lib.stream()) < 0
    assert L.g2s_resample_sep(p(x), p(y), 0, 32, 32, 32, 32, *tab, t.fwd.K, *tab, t.fwd.K, lib.stream()) < 0
    assert b"taps" in L.g2s_last_error() or b"size" in L.g2s_last_error()
    assert L.g2s_resample_bands_check(lo.ctypes.data_as(C.c_void_p), ln.ctypes.data_as(C.c_void_p), n, w.shape[1], 32) == 0
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------- step 2 with the crop on
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


def test_step2_fused_against_composed_with_the_crop_on(golden):
    """One forward_step2 + backward at STEP_CFG with crop = 112 under identical draws, the crop on its fused route
    against the crop on its composed route; loss and every offset-encoder gradient element within rtol 1e-4,
    atol 1e-5 (1 + |value|).

    What is switched is the crop's route alone (GAN2Shape.crop_fused), the rest of the step staying on the renderer's
    fused route.  Switching Renderer.fused for the whole step compares something else as well: the pseudo samples
    are then rendered by the composed renderer, and the offset-encoder gradients of the two renderers differ by more
    than this tolerance whether or not there is a crop — measured on an MI355X, worst |difference| / tolerance over
    all gradient elements: 19.4 with `crop` absent (the parent's code paths only), 21.3 with crop = 112, against 0.015
    when only the crop's route changes.  The whole-step switch is still run here: its losses must agree to the
    tolerance (as tests/test_gpu_object_mask_steps.py asks of that pair) and it must launch less."""
    from gan2shape_amd import lib, zeropool
    prev = lib.set_deterministic(True)
    try:
        g = golden("steps")
        draws = tuple(torch.tensor(g[f"s2.draw.{k}"]).cuda() for k in ("dxy", "rand", "views"))
        image, latent = torch.tensor(g["image"]).cuda(), torch.tensor(g["latent"]).cuda()
        m = build(crop=112)
        assert m.crop == 112 and m.origin_size == 128 and m.crop_fused is None
        with torch.no_grad():
            _, c1 = m.forward_step1(image, latent, None)
        zeropool.end()
        params = [p for p in m.offset_encoder_net.parameters() if p.requires_grad]
        got = {}

        def step(route):
            m.renderer.fused, m.crop_fused = {"fused": (True, None), "crop_composed": (True, False),
                                              "all_composed": (False, None)}[route]
            try:
                for p in params:
                    p.grad = None
                loss, _ = m.forward_step2(image, latent, c1, n_proj_samples=draws[2].shape[0], _draws=draws)
                loss.backward()
                zeropool.end()
                got[route] = (loss.detach(), [p.grad.clone() for p in params])
            finally:
                m.renderer.fused, m.crop_fused = True, None
        count = {}
        for route in ("fused", "crop_composed", "all_composed"):
            step(route)                                   # warm-up of the route, and the values
            count[route] = launches(lambda: step(route))
        la, ga = got["fused"]
        for route in ("crop_composed", "all_composed"):
            lb, gb = got[route]
            worst = 0.0
            for a, b in zip(ga, gb):
                assert bool(torch.isfinite(a).all()) and float(b.abs().max()) > 0
                tol = 1e-4 * b.abs() + 1e-5 * (1 + b.abs())
                worst = max(worst, float(((a - b).abs() / tol).max()))
            print(f"[crop_resize gpu] step 2, crop 112, fused against {route}: loss {float(la):.8f} / {float(lb):.8f}, "
                  f"launches {count['fused']} / {count[route]}, offset-encoder gradients worst |difference| / tolerance "
                  f"{worst:.3f}")
            torch.testing.assert_close(la, lb, rtol=1e-4, atol=1e-5 * (1 + float(lb.abs())))
            assert count["fused"] < count[route]
            if route == "crop_composed":
                assert worst <= 1.0
        # the crop changes the step: without it the projected image differs
        plain = build()
        assert plain.crop is None
        with torch.no_grad():
            _, (proj_c, _) = m.forward_step2(image, latent, c1, n_proj_samples=draws[2].shape[0], _draws=draws)
            _, (proj_p, _) = plain.forward_step2(image, latent, c1, n_proj_samples=draws[2].shape[0], _draws=draws)
        zeropool.end()
        assert proj_c.shape == proj_p.shape and not torch.equal(proj_c, proj_p)
    finally:
        lib.set_deterministic(prev)


def test_graphed_fit_captures_step2_with_the_crop_on():
    """Trainer.fit(graphs=True) with `crop`: the tables are uploaded at construction, the crop's launches are captured
    with the rest of step 2; step 1 is deterministic given the weights, so its first loss reproduces the eager run's
    (the bound test_trainer_fit_with_hip_graphs uses: 5e-3)."""
    import math

    import bench
    from gan2shape_amd.model import GAN2Shape
    from gan2shape_amd.trainer import Trainer
    dev = torch.device("cuda")
    torch.cuda.set_stream(torch.cuda.Stream(dev))     # captures need a non-default stream
    try:
        cfg = bench.face_config(n_proj=2)
        cfg.update(crop=112, origin_size=128)
        stages = [{'step1': 2, 'step2': 2, 'step3': 2}]
        losses = {}
        for graphs in (False, True):
            torch.manual_seed(0)
            t = Trainer(GAN2Shape, cfg, device=dev, capturable=True)
            image, latent = bench.synthetic_sample(t.model, 1234, dev)
            n = t.fit([(image[0].cpu(), latent[0].cpu(), 0)], stages=stages, graphs=graphs)
            assert n == 6
            losses[graphs] = [h[3] for h in t.history]
            assert all(math.isfinite(v) for v in losses[graphs])
        print("[crop_resize gpu] history eager", losses[False], "graphed", losses[True])
        assert abs(losses[True][0] - losses[False][0]) < 5e-3 * abs(losses[False][0]), (losses[True], losses[False])
    finally:
        torch.cuda.set_stream(torch.cuda.default_stream(dev))
