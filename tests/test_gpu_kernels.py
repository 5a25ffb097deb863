"""-m gpu parity tests: the HIP kernels (through the C ABI of libg2s.so) against the CPU oracle and
the golden vectors generated from the reference's own Python.

Tolerances: integer/index outputs (face ids) bit-exact; rasterizer floats bit-exact against the
fp32 oracle (same operation order, no FMA contraction); elementwise ops exact or 1 ulp;
convolutions / FIR within 1e-5 relative of the fp32 reference (summation order differs)."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import capi  # noqa: E402
from oracle import geometry as og  # noqa: E402
from raster_cases import scene, soup  # noqa: E402

FAR = 100.0


@pytest.fixture(scope="module")
def g2s():
    import gan2shape_amd  # noqa: F401
    from gan2shape_amd import lib
    lib.load()  # fails loudly if libg2s.so is missing
    assert torch.cuda.is_available()
    return gan2shape_amd


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


# ----------------------------------------------------------------------------- fused_bias_act
@pytest.mark.parametrize("name", ["4d", "2d"])
def test_fused_leaky_relu_golden(g2s, golden, name):
    from gan2shape_amd.op import fused_leaky_relu
    g = golden("ops")
    x = dev(g[f"fused.{name}.x"]).requires_grad_(True)
    b = dev(g[f"fused.{name}.b"]).requires_grad_(True)
    y = fused_leaky_relu(x, b)
    gx, gb = torch.autograd.grad(y, (x, b), dev(g[f"fused.{name}.gy"]))
    np.testing.assert_allclose(y.detach().cpu().numpy(), g[f"fused.{name}.y"], rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(gx.cpu().numpy(), g[f"fused.{name}.gx"], rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(gb.cpu().numpy(), g[f"fused.{name}.gb"], rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("shape", [(8, 128, 32, 32), (3, 5, 7, 9), (4, 512), (1, 3, 1, 1)])
@pytest.mark.parametrize("act,grad", [(3, 0), (3, 1), (1, 0), (3, 2), (7, 0)])
def test_fused_bias_act_vs_oracle(g2s, shape, act, grad):
    from gan2shape_amd.plugins import fused
    rng = np.random.default_rng(0)
    x = rng.standard_normal(shape).astype(np.float32)
    b = rng.standard_normal(shape[1]).astype(np.float32)
    ref = rng.standard_normal(shape).astype(np.float32)
    for use_b in (True, False):
        exp = capi.fused_bias_act(x, b if use_b else None, ref if grad == 1 else None, act, grad, 0.2, 1.4142135)
        empty = torch.empty(0, device="cuda")
        y = fused.fused_bias_act(dev(x), dev(b) if use_b else empty, dev(ref) if grad == 1 else empty,
                                 act, grad, 0.2, 1.4142135)
        np.testing.assert_array_equal(y.cpu().numpy(), exp)


def test_fused_bias_act_f16_and_errors(g2s):
    from gan2shape_amd.plugins import fused
    x = torch.randn(2, 4, 6, 6, device="cuda").half()
    b = torch.randn(4, device="cuda").half()
    y = fused.fused_bias_act(x, b, x.new_empty(0), 3, 0, 0.2, 2 ** 0.5)
    exp = torch.nn.functional.leaky_relu((x + b.view(1, -1, 1, 1)).float(), 0.2) * 2 ** 0.5
    torch.testing.assert_close(y.float(), exp, rtol=2e-3, atol=2e-3)
    with pytest.raises(RuntimeError):
        fused.fused_bias_act(x.cpu(), b, x.new_empty(0), 3, 0, 0.2, 1.0)  # CHECK_CUDA


def test_noise_bias_act(g2s):
    from gan2shape_amd.op import fused_noise_bias_act
    torch.manual_seed(0)
    for shape in [(2, 8, 16, 16), (2, 5, 3, 3)]:
        x = torch.randn(*shape, device="cuda", requires_grad=True)
        noise = torch.randn(1, 1, *shape[2:], device="cuda")
        nw = torch.randn(1, device="cuda")
        b = torch.randn(shape[1], device="cuda")
        y = fused_noise_bias_act(x, noise, nw, b)
        exp = 2 ** 0.5 * torch.nn.functional.leaky_relu(x + nw * noise + b.view(1, -1, 1, 1), 0.2)
        torch.testing.assert_close(y, exp, rtol=1e-6, atol=1e-6)
        gy = torch.randn_like(y)
        (gx,) = torch.autograd.grad(y, x, gy)
        (gexp,) = torch.autograd.grad(exp, x, gy)
        torch.testing.assert_close(gx, gexp, rtol=1e-6, atol=1e-6)


# ----------------------------------------------------------------------------- upfirdn2d
UP_CASES = ["blur_up", "rgb_up", "d_blur3", "d_blur1", "down2", "crop"]


@pytest.mark.parametrize("name", UP_CASES)
def test_upfirdn2d_golden(g2s, golden, name):
    from gan2shape_amd.op import upfirdn2d
    g = golden("ops")
    up, down, p0, p1 = (int(v) for v in g[f"upfirdn2d.{name}.args"])
    x = dev(g[f"upfirdn2d.{name}.x"]).requires_grad_(True)
    y = upfirdn2d(x, dev(g[f"upfirdn2d.{name}.k"]), up=up, down=down, pad=(p0, p1))
    (gx,) = torch.autograd.grad(y, x, dev(g[f"upfirdn2d.{name}.gy"]))
    np.testing.assert_allclose(y.detach().cpu().numpy(), g[f"upfirdn2d.{name}.y"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(gx.cpu().numpy(), g[f"upfirdn2d.{name}.gx"], rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("shape,up,down,pad", [
    ((2, 16, 65, 65), 1, 1, (1, 1)),     # G blur after up-conv
    ((2, 3, 32, 32), 2, 1, (2, 1)),      # ToRGB skip upsample
    ((2, 8, 64, 64), 1, 1, (2, 2)),      # D blur before 3x3 s2
    ((2, 8, 33, 47), 1, 2, (1, 1)),      # downsample, ragged
    ((1, 2, 5, 3), 1, 1, (2, 2)),        # smaller than a tile
    ((1, 1, 40, 40), 3, 2, (2, 3)),      # generic fallback path
])
def test_upfirdn2d_vs_oracle(g2s, shape, up, down, pad):
    from gan2shape_amd.op import upfirdn2d
    rng = np.random.default_rng(1)
    x = rng.standard_normal(shape).astype(np.float32)
    k = np.outer([1, 3, 3, 1], [1, 3, 3, 1]).astype(np.float32)
    k = k / k.sum() * up * up + 0.01 * rng.standard_normal((4, 4)).astype(np.float32)  # asymmetric
    exp = capi.upfirdn2d(x, k, (up, up), (down, down), (pad[0], pad[1], pad[0], pad[1]))
    y = upfirdn2d(dev(x), dev(k), up=up, down=down, pad=pad)
    np.testing.assert_allclose(y.cpu().numpy(), exp, rtol=1e-5, atol=1e-6)


# ----------------------------------------------------------------------------- rasterizer
def _render(verts, faces, S, K, ssaa=2, fill_back=True, implicit=False, grad=None):
    from gan2shape_amd.plugins import neural_renderer as nr
    v = dev(verts).requires_grad_(grad is not None)
    f = None if implicit else dev(faces, torch.int32)
    d = nr.RenderDepthFunction.apply(v, f, tuple(np.asarray(K, np.float32).reshape(9).tolist()),
                                     float(S), S, ssaa == 2, fill_back, 0.1, FAR)
    if grad is None:
        return d.cpu().numpy()
    (gv,) = torch.autograd.grad(d, v, dev(grad))
    return d.detach().cpu().numpy(), gv.cpu().numpy()


@pytest.mark.parametrize("S,ssaa,fill_back,implicit", [
    (16, 2, True, True), (16, 2, True, False), (20, 2, True, True), (32, 2, True, True),
    (16, 1, True, True), (16, 2, False, True), (12, 1, False, False), (36, 2, True, True)])
def test_raster_forward_bit_exact(g2s, S, ssaa, fill_back, implicit):
    geo, verts, faces = scene(S, B=2, seed=S + ssaa)
    ref = capi.render_depth(verts, faces, S, geo.K[0], ssaa=ssaa, fill_back=fill_back, far=FAR)
    d = _render(verts, faces, S, geo.K[0], ssaa, fill_back, implicit)
    np.testing.assert_array_equal(d, ref["depth"])


def test_raster_saved_maps_and_backward(g2s):
    from gan2shape_amd import lib
    S = 32
    geo, verts, faces = scene(S, B=2, seed=5)
    ref = capi.render_depth(verts, faces, S, geo.K[0], far=FAR)
    rng = np.random.default_rng(0)
    g = rng.standard_normal((2, S, S)).astype(np.float32)
    g[ref["depth"] > 1.2] = 0
    gref = capi.render_depth_bwd(verts.astype(np.float64), faces, g.astype(np.float64),
                                 ref["face_idx"], ref["bary"].astype(np.float64), S,
                                 geo.K[0].astype(np.float64), dtype=np.float64)
    scale = np.abs(gref).max()
    for implicit in (True, False):
        d, gv = _render(verts, faces, S, geo.K[0], implicit=implicit, grad=g)
        np.testing.assert_array_equal(d, ref["depth"])
        np.testing.assert_allclose(gv, gref, atol=3e-5 * scale)
    # the saved maps themselves (index work: bit-exact)
    L = lib.load()
    v = dev(verts)
    depth = torch.empty(2, S, S, device="cuda")
    fidx = torch.empty(2, 2 * S, 2 * S, dtype=torch.int32, device="cuda")
    bary = torch.empty(2, 2 * S, 2 * S, 3, device="cuda")
    ws = torch.empty(L.g2s_raster_workspace_bytes(2, S * S, faces.shape[0], S), dtype=torch.uint8, device="cuda")
    Kc = (lib.C.c_float * 9)(*np.asarray(geo.K[0], np.float32).reshape(9).tolist())
    lib.check(L.g2s_raster_depth_fwd(lib.ptr(v), None, 2, S * S, faces.shape[0], S, Kc, float(S), 2, 1,
                                     0.1, FAR, lib.ptr(depth), lib.ptr(fidx), lib.ptr(bary), lib.ptr(ws),
                                     ws.numel(), lib.stream()))
    np.testing.assert_array_equal(fidx.cpu().numpy(), ref["face_idx"])
    np.testing.assert_array_equal(bary.cpu().numpy(), ref["bary"])


def test_raster_triangle_soup(g2s):
    verts, faces = soup(n_faces=700, n_verts=300)
    S = 24
    K = og.Geometry(S).K[0]
    for fill_back in (True, False):
        ref = capi.render_depth(verts, faces, S, K, fill_back=fill_back, far=FAR)
        d = _render(verts, faces, S, K, 2, fill_back, implicit=False)
        np.testing.assert_array_equal(d, ref["depth"])


def test_raster_full_size_properties(g2s):
    """S = 128 (BASELINE face config), B = 8: properties that need no brute-force oracle."""
    S, B = 128, 8
    geo = og.Geometry(S)
    fx, cx = geo.K[0, 0, 0], geo.K[0, 0, 2]
    v, u = np.meshgrid(np.arange(S), np.arange(S), indexing="ij")

    def plane(uu, vv, a, b):
        return 1.0 / (1 - a * (uu - cx) / fx - b * (vv - cx) / fx)

    coef = [(0.0, 0.0), (0.5, -0.3), (-0.8, 0.2), (0.1, 0.9), (0, 0), (0.3, 0.3), (-0.2, -0.6), (0.7, 0.1)]
    depth = np.stack([plane(u, v, a, b) for a, b in coef]).astype(np.float32)
    geo.set_transform_matrices(np.zeros((B, 6), np.float32))
    verts = geo.get_warped_3d_grid(depth).reshape(B, -1, 3)
    faces = og.get_face_idx(1, S, S)[0]
    d = _render(verts, faces, S, geo.K[0], implicit=True)
    for i, (a, b) in enumerate(coef):
        exp = sum(plane(u + dc, v + dr, a, b) for dr in (.25, .75) for dc in (.25, .75)) / 4
        np.testing.assert_allclose(d[i, :S - 1, :S - 1], exp[:S - 1, :S - 1], rtol=3e-5)
    np.testing.assert_array_equal(d[:, S - 1, :], FAR)
    np.testing.assert_array_equal(d[:, :, S - 1], FAR)
    # explicit topology gives the same image as the implicit one, batch entries are independent
    geo2, verts2, _ = scene(S, B=B, seed=11)
    d_imp = _render(verts2, faces, S, geo2.K[0], implicit=True)
    d_exp = _render(verts2, faces, S, geo2.K[0], implicit=False)
    np.testing.assert_array_equal(d_imp, d_exp)
    d_one = _render(verts2[3:4], faces, S, geo2.K[0], implicit=True)
    np.testing.assert_array_equal(d_one[0], d_imp[3])
    assert ((d_imp > 0.8) & (d_imp < 1.2)).mean() > 0.2


# ----------------------------------------------------------------------------- modulated conv
def _style_mod(g, name):
    w, b, s = g[f"{name}.mod_weight"], g[f"{name}.mod_bias"], g[f"{name}.s"]
    return (s @ (w * (1 / math.sqrt(w.shape[1]))).T + b).astype(np.float32)


@pytest.mark.parametrize("name", ["plain", "up", "rgb", "down"])
def test_modulated_conv_golden(g2s, golden, name):
    """Module-level parity with the reference's ModulatedConv2d (outputs and gradients w.r.t.
    input and style) on the fixtures generated by tests/golden/make_golden.py."""
    from gan2shape_amd import stylegan2 as sg2
    g = golden("modconv")
    cout, cin, k = g[f"{name}.weight"].shape[1:4]
    kw = dict(plain={}, up=dict(upsample=True), rgb=dict(demodulate=False), down=dict(downsample=True))[name]
    m = sg2.ModulatedConv2d(cin, cout, k, 16, **kw).cuda()
    with torch.no_grad():
        m.weight.copy_(dev(g[f"{name}.weight"]))
        m.modulation.weight.copy_(dev(g[f"{name}.mod_weight"]))
        m.modulation.bias.copy_(dev(g[f"{name}.mod_bias"]))
    x = dev(g[f"{name}.x"]).requires_grad_(True)
    s = dev(g[f"{name}.s"]).requires_grad_(True)
    y = m(x, s)
    gx, gs, gw = torch.autograd.grad(y, (x, s, m.weight), dev(g[f"{name}.gy"]))
    np.testing.assert_allclose(y.detach().cpu().numpy(), g[f"{name}.y"], rtol=1e-4, atol=2e-5)
    np.testing.assert_allclose(gx.cpu().numpy(), g[f"{name}.gx"], rtol=1e-4, atol=2e-5)
    np.testing.assert_allclose(gs.cpu().numpy(), g[f"{name}.gs"], rtol=1e-4, atol=5e-5)
    np.testing.assert_allclose(gw.cpu().numpy(), g[f"{name}.gw"], rtol=1e-3, atol=5e-5)


@pytest.mark.parametrize("B,cin,cout,h,k,mode", [
    (2, 64, 96, 16, 3, 0), (3, 40, 130, 9, 3, 0), (2, 64, 64, 8, 3, 1), (2, 32, 48, 13, 3, 2),
    (2, 128, 3, 32, 1, 0), (8, 512, 512, 4, 3, 0), (2, 256, 128, 16, 3, 1), (1, 8, 8, 5, 3, 1),
    # <= 4 channels on one side
    (2, 3, 40, 32, 1, 0), (2, 3, 24, 33, 3, 0), (2, 21, 3, 32, 3, 0), (2, 66, 2, 40, 3, 0), (1, 4, 130, 32, 3, 0)])
def test_modconv_vs_oracle(g2s, B, cin, cout, h, k, mode):
    from gan2shape_amd.modconv import modconv_raw
    rng = np.random.default_rng(2)
    x = rng.standard_normal((B, cin, h, h)).astype(np.float32)
    w = rng.standard_normal((cout, cin, k, k)).astype(np.float32)
    s = (1 + 0.3 * rng.standard_normal((B, cin))).astype(np.float32)
    scale = 1 / math.sqrt(cin * k * k)
    exp = capi.modconv(x, w, s, scale, True, mode)
    ws = w * scale
    demod = 1 / np.sqrt((s[:, None, :] ** 2 * (ws ** 2).sum((2, 3))[None]).sum(2) + 1e-8)
    y = modconv_raw(dev(x), dev(ws), dev(s), dev(demod), mode, 0)
    np.testing.assert_allclose(y.cpu().numpy(), exp, rtol=2e-4, atol=2e-5)


@pytest.mark.parametrize("mode,h", [(0, 12), (1, 7), (2, 11)])
def test_modconv_transpose_is_adjoint(g2s, mode, h):
    """<conv(x), g> == <x, conv^T(g)> for every geometry (the data-gradient kernel)."""
    from gan2shape_amd.modconv import modconv_raw
    torch.manual_seed(0)
    B, cin, cout = 2, 24, 40
    x = torch.randn(B, cin, h, h, device="cuda")
    w = torch.randn(cout, cin, 3, 3, device="cuda") / 10
    y = modconv_raw(x, w, None, None, mode, 0)
    g = torch.randn_like(y)
    xt = modconv_raw(g, w, None, None, mode, 1)
    assert xt.shape == x.shape
    lhs, rhs = (y.double() * g.double()).sum().item(), (x.double() * xt.double()).sum().item()
    assert abs(lhs - rhs) < 1e-4 * max(1.0, abs(lhs))


@pytest.mark.parametrize("cin,cout,k", [(3, 40, 3), (40, 3, 3), (3, 24, 1), (130, 2, 1)])
def test_thin_conv_transpose_is_adjoint(g2s, cin, cout, k):
    """Same identity with <= 4 channels on one side (toRGB / fromRGB / first VGG layer shapes)."""
    from gan2shape_amd.modconv import modconv_raw
    torch.manual_seed(1)
    x = torch.randn(2, cin, 34, 34, device="cuda")
    w = torch.randn(cout, cin, k, k, device="cuda") / 10
    y = modconv_raw(x, w, None, None, 0, 0)
    g = torch.randn_like(y)
    xt = modconv_raw(g, w, None, None, 0, 1)
    lhs, rhs = (y.double() * g.double()).sum().item(), (x.double() * xt.double()).sum().item()
    assert abs(lhs - rhs) < 1e-4 * max(1.0, abs(lhs))


# ----------------------------------------------------------------------------- row ops
@pytest.mark.parametrize("shape", [(2, 5, 7, 9), (3, 64, 16, 16), (1, 3, 129, 129), (8, 512, 4, 4)])
def test_rows_dot_scale(g2s, shape):
    from gan2shape_amd.modconv import rows_dot_scale
    torch.manual_seed(0)
    a, b = torch.randn(*shape, device="cuda"), torch.randn(*shape, device="cuda")
    s = torch.randn(shape[:2], device="cuda")
    inv = torch.rand(shape[:2], device="cuda") + 0.5
    out, dot = rows_dot_scale(a, b, s, inv)
    torch.testing.assert_close(out, b * s[:, :, None, None], rtol=1e-6, atol=1e-6)
    torch.testing.assert_close(dot, (a.double() * b.double()).sum((2, 3)).float() / inv, rtol=1e-4, atol=1e-4)
    out2, dot2 = rows_dot_scale(a, b, None, None, want_out=False)
    assert out2 is None
    torch.testing.assert_close(dot2, (a.double() * b.double()).sum((2, 3)).float(), rtol=1e-4, atol=1e-4)


def test_demodulation_matches_torch(g2s):
    from gan2shape_amd.modconv import demodulation
    torch.manual_seed(0)
    for B, cin, cout in [(2, 16, 24), (8, 512, 512), (3, 130, 7)]:
        s = (torch.randn(B, cin, device="cuda") * 0.5 + 1).requires_grad_(True)
        wsq = torch.rand(cout, cin, device="cuda") / cin
        d = demodulation(s, wsq)
        ref = torch.rsqrt(torch.nn.functional.linear(s * s, wsq) + 1e-8)
        torch.testing.assert_close(d, ref, rtol=1e-5, atol=1e-6)
        g = torch.randn_like(d)
        (gs,) = torch.autograd.grad(d, s, g)
        (gref,) = torch.autograd.grad(ref, s, g)
        torch.testing.assert_close(gs, gref, rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize("B,cin,cout,h,k,stride", [
    (2, 16, 24, 20, 3, 1), (2, 32, 48, 35, 3, 2), (2, 24, 40, 17, 1, 2), (8, 3, 128, 16, 1, 1),
    (1, 130, 70, 9, 3, 2)])
def test_plain_conv_matches_torch(g2s, B, cin, cout, h, k, stride):
    """EqualConv2d path of the discriminator: forward and data-gradient vs torch's conv."""
    from gan2shape_amd.modconv import conv2d, conv2d_supported
    torch.manual_seed(0)
    x = torch.randn(B, cin, h, h, device="cuda", requires_grad=True)
    w = torch.randn(cout, cin, k, k, device="cuda") / (cin * k * k) ** 0.5
    pad = k // 2 if stride == 1 else 0
    mode = conv2d_supported(x, w, stride, pad)
    assert mode is not None
    y = conv2d(x, w, mode)
    ref = torch.nn.functional.conv2d(x, w, stride=stride, padding=pad)
    torch.testing.assert_close(y, ref, rtol=1e-4, atol=2e-5)
    g = torch.randn_like(ref)
    (gx,) = torch.autograd.grad(y, x, g)
    (gref,) = torch.autograd.grad(ref, x, g)
    torch.testing.assert_close(gx, gref, rtol=1e-4, atol=2e-5)


# ----------------------------------------------------------------------------- GroupNorm + act
@pytest.mark.gpu
@pytest.mark.parametrize("shape,groups,slope", [
    ((1, 32, 64, 64), 8, 0.2), ((1, 128, 16, 16), 32, 0.2), ((1, 32, 128, 128), 8, 0.0),
    ((3, 64, 32, 32), 16, 0.0), ((2, 6, 2, 2), 3, 0.0), ((1, 256, 6, 6), 32, 0.0)])
def test_groupnorm_act_vs_oracle(g2s, shape, groups, slope):
    """fp32 kernel vs the float64 oracle (oracle/nets.py): forward 2e-6 of the output scale,
    gradients 2e-5 of their scale (sums of up to 65536 fp32 terms)."""
    from gan2shape_amd.op.groupnorm import groupnorm_act
    from oracle import nets
    rng = np.random.default_rng(11)
    x = (rng.standard_normal(shape) * 2 + 0.5).astype(np.float32)
    gamma = rng.standard_normal(shape[1]).astype(np.float32)
    beta = rng.standard_normal(shape[1]).astype(np.float32)
    gy = rng.standard_normal(shape).astype(np.float32)
    xt, gt, bt = dev(x).requires_grad_(True), dev(gamma).requires_grad_(True), dev(beta).requires_grad_(True)
    y = groupnorm_act(xt, gt, bt, groups, 1e-5, True, slope)
    y.backward(dev(gy))
    ref = nets.group_norm_act(x, gamma, beta, groups, 1e-5, True, slope)
    dx, dg, db = nets.group_norm_act_grad(x, gamma, beta, gy, groups, 1e-5, True, slope)
    # samples whose pre-activation rounds across zero flip the slope: exclude |y| < 1e-5
    ok = np.abs(nets.group_norm_act(x, gamma, beta, groups, 1e-5, False)) > 1e-5
    np.testing.assert_allclose(y.detach().cpu().numpy()[ok], ref[ok], rtol=0, atol=2e-6 * np.abs(ref).max())
    for got, want in ((xt.grad, dx), (gt.grad, dg), (bt.grad, db)):
        np.testing.assert_allclose(got.cpu().numpy(), want, rtol=0, atol=2e-5 * np.abs(want).max() + 1e-6)


# ----------------------------------------------------------------------------- general conv (trained nets)
CONV_CASES = [  # B, Cin, Cout, H, k, stride, pad, transposed, slope
    (1, 3, 32, 128, 4, 2, 1, False, 0.2), (1, 32, 64, 64, 4, 2, 1, False, None), (1, 128, 256, 16, 4, 2, 1, False, 0.2),
    (1, 256, 256, 4, 4, 1, 0, False, 0.0), (1, 256, 256, 1, 4, 1, 0, True, 0.0), (1, 256, 128, 8, 4, 2, 1, True, None),
    (1, 64, 32, 32, 4, 2, 1, True, None), (1, 32, 32, 128, 5, 1, 2, False, None), (1, 32, 3, 128, 5, 1, 2, False, None),
    (1, 32, 32, 64, 3, 1, 1, False, None), (9, 3, 32, 128, 4, 2, 1, False, 0.0), (9, 512, 512, 4, 4, 1, 0, False, 0.0),
    (9, 512, 6, 1, 1, 1, 0, False, None), (9, 32, 64, 64, 3, 2, 1, False, None), (9, 32, 64, 32, 1, 1, 0, False, None),
    (2, 5, 7, 11, 3, 2, 1, False, None), (2, 5, 7, 9, 4, 2, 1, True, 0.0), (2, 6, 4, 7, 5, 1, 2, False, 0.1),
    (2, 3, 5, 10, 4, 2, 1, False, None), (3, 4, 6, 6, 5, 1, 0, True, None), (2, 7, 3, 12, 3, 2, 0, False, None),
]


@pytest.mark.gpu
@pytest.mark.parametrize("B,cin,cout,H,k,stride,pad,transposed,slope", CONV_CASES)
def test_conv_function_matches_torch_f64(g2s, B, cin, cout, H, k, stride, pad, transposed, slope):
    """g2s_conv2d (forward, data-gradient) and g2s_conv2d_wgrad against torch's float64 CPU
    convolution: 2e-5 of each tensor's L2 norm (fp32 MFMA sums of up to ~10^5 terms)."""
    import torch.nn.functional as F
    from gan2shape_amd.op.conv import ConvFunction
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(B, cin, H, H + (1 if H % 2 and H > 4 else 0), generator=gen, dtype=torch.float64)
    wshape = (cin, cout, k, k) if transposed else (cout, cin, k, k)
    w = torch.randn(wshape, generator=gen, dtype=torch.float64) / (cin * k * k) ** 0.5
    b = torch.randn(cout, generator=gen, dtype=torch.float64)
    xr, wr, br = x.clone().requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    ref = (F.conv_transpose2d if transposed else F.conv2d)(xr, wr, br, stride=stride, padding=pad)
    if slope is not None:
        ref = F.leaky_relu(ref, slope)
    gy = torch.randn(ref.shape, generator=gen, dtype=torch.float64)
    ref.backward(gy)
    xg, wg, bg = [t.float().cuda().requires_grad_(True) for t in (x, w, b)]
    y = ConvFunction.apply(xg, wg, bg, stride, pad, transposed, slope)
    assert y.shape == ref.shape
    y.backward(gy.float().cuda())

    def close(got, want, what):
        err = float((got.double().cpu() - want).norm())
        assert err <= 2e-5 * float(want.norm()) + 1e-7, (what, err, float(want.norm()))
    close(y.detach(), ref.detach(), "y")
    close(xg.grad, xr.grad, "gx")
    close(wg.grad, wr.grad, "gw")
    close(bg.grad, br.grad, "gb")


@pytest.mark.gpu
@pytest.mark.parametrize("B,groups,cin,cout,H,k,stride,pad,transposed", [
    (1, 2, 64, 128, 32, 4, 2, 1, False), (1, 2, 128, 64, 8, 4, 2, 1, True), (1, 2, 32, 32, 64, 5, 1, 2, False),
    (9, 2, 128, 256, 16, 4, 2, 1, False), (8, 1, 128, 128, 16, 3, 1, 1, False), (2, 1, 5, 7, 11, 3, 2, 1, False),
])
def test_fused_backward_launch_equals_the_two_launches(g2s, B, groups, cin, cout, H, k, stride, pad, transposed):
    """g2s_conv2d_bwd (data-gradient + weight-gradient of one layer in one grid) against
    g2s_conv2d + g2s_conv2d_wgrad, with the data-gradient on its 64x64 tile (one
    grid) and forced onto the 128-wide tiles (the entry point then launches the two kernels itself)."""
    from gan2shape_amd import lib
    from gan2shape_amd.op.conv import _conv2d_raw, _conv_bwd_raw, _wgrad
    L = lib.load()
    torch.manual_seed(B + cin + H)
    x = torch.randn(B, groups * cin, H, H, device="cuda")
    w = torch.randn((groups * cin, cout, k, k) if transposed else (groups * cout, cin, k, k), device="cuda") / (cin * k * k) ** 0.5
    y = _conv2d_raw(x, w, None, cin, cout, k, stride, pad, transposed, not transposed, None, False, 0.0, groups=groups)
    gy = torch.randn_like(y)
    try:
        L.g2s_modconv_tune(2, 1)   # unsplit reference
        gx_ref = _conv2d_raw(gy, w, None, cout, cin, k, stride, pad, not transposed, transposed, (H, H), False, 0.0,
                             groups=groups)
        gw_ref = _wgrad(x, gy, k, stride, pad, None, groups) if transposed else _wgrad(gy, x, k, stride, pad, None, groups)
        for tile, sk in [(-1, -1), (2, 1), (2, 3), (3, 1), (3, 2), (4, 1), (4, 3), (1, 1), (0, 2)]:
            L.g2s_modconv_tune(tile, sk)
            gx, gw = _conv_bwd_raw(gy, w, x, cin, cout, k, stride, pad, transposed, None, None, groups)
            assert gx.shape == x.shape and gw.shape == w.shape
            for got, want, what in ((gx, gx_ref, "gx"), (gw, gw_ref, "gw")):
                err = float((got - want).norm())
                assert err <= 1e-5 * float(want.norm()) + 1e-7, (tile, sk, what, err, float(want.norm()))
    finally:
        L.g2s_modconv_tune(-1, -1)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["DepthNet", "AlbedoNet", "ViewpointNet", "LightingNet", "OffsetEncoder"])
def test_trained_nets_fused_match_modules(g2s, name):
    """Each trained net on the GPU (libg2s convolutions + fused GroupNorm) equals its own module
    list evaluated op by op by torch on the CPU in float64: outputs to 1e-4 of their norm.
    Parameter gradients: an activation whose input lies within fp32 rounding of zero takes the other
    slope than in float64 (about one of the 1.7 M activations of a depth net per run); one such flip
    moves the bias gradient of its channel by up to ~1 %, so single tensors are held to 2e-2 and all
    gradients together to 5e-3 (the single ops are held to 2e-5 by the tests above)."""
    import copy
    from gan2shape_amd import networks
    torch.manual_seed(0)
    net = getattr(networks, name)(128)
    ref_net = copy.deepcopy(net).double()
    net = net.cuda()
    B = 1 if name in ("DepthNet", "AlbedoNet") else 3
    x = torch.randn(B, 3, 128, 128)
    gen_gy = torch.Generator().manual_seed(1)
    y = net(x.cuda())
    ref = ref_net(x.double())
    assert float((y.detach().double().cpu() - ref.detach()).norm()) <= 1e-4 * float(ref.norm()) + 1e-6
    gy = torch.randn(ref.shape, generator=gen_gy, dtype=torch.float64)
    g1 = torch.autograd.grad(y, list(net.parameters()), gy.float().cuda())
    g2 = torch.autograd.grad(ref, list(ref_net.parameters()), gy)
    err2 = ref2 = 0.0
    for (n, _), a, b in zip(net.named_parameters(), g1, g2):
        e = float((a.double().cpu() - b).norm())
        assert e <= 2e-2 * float(b.norm()) + 1e-7, n
        err2 += e * e
        ref2 += float(b.norm()) ** 2
    assert err2 ** 0.5 <= 5e-3 * ref2 ** 0.5


# ----------------------------------------------------------------------------- render_rgb (texture path)
@pytest.mark.parametrize("S,ts,C,fill_back,implicit", [
    (16, 2, 3, True, True), (16, 1, 3, True, True), (20, 2, 3, True, False), (12, 2, 1, False, True),
    (32, 2, 3, True, True)])
def test_render_rgb_vs_oracle(g2s, S, ts, C, fill_back, implicit):
    """nr.Renderer.render_rgb (g2s_raster_depth_fwd with saved maps + g2s_raster_rgb_fwd) against the
    oracle's texture pass on posed, folded meshes: same winners (bit-exact depth path) and the same
    arithmetic for the cube read -> 1e-6."""
    from gan2shape_amd.plugins import neural_renderer as nr
    geo, verts, faces = scene(S, B=2, seed=S + ts + C)
    rng = np.random.default_rng(S)
    tex = rng.uniform(-1, 1, (2, faces.shape[0], ts, ts, ts, C)).astype(np.float32)
    bg = [1.0, 0.5, -0.25][:C]
    ref = capi.render_rgb(verts, faces, tex, S, geo.K[0], fill_back=fill_back, near=0.1, far=10.0, background=bg)
    r = nr.Renderer(camera_mode='projection', K=dev(geo.K), image_size=S, orig_size=S, fill_back=fill_back,
                    near=0.1, far=10.0, light_intensity_ambient=1.0, light_intensity_directional=0.0,
                    background_color=bg)
    f = None if implicit else dev(faces, torch.int32)[None].expand(2, -1, -1)
    if implicit:
        from gan2shape_amd.renderer.utils import get_face_idx
        f = get_face_idx(2, S, S, device="cuda")
    out = r.render_rgb(dev(verts), f, dev(tex))
    assert tuple(out.shape) == (2, C, S, S) and not out.requires_grad
    np.testing.assert_allclose(out.cpu().numpy(), ref, rtol=1e-6, atol=1e-6)


def test_renderer_texture_helpers_on_gpu(g2s):
    """render_given_view(grid_sample=False), render_yaw, render_view (renderer.py:141-277): the mesh
    rendering of a smooth image under a small pose agrees with the inverse-warp sampling of the same
    pose away from silhouettes; the zero pose of a sweep reproduces the identity rendering; the
    sweeps have the reference's frame counts."""
    from gan2shape_amd.renderer import Renderer
    S = 64
    R = Renderer({"rot_center_depth": 1.0, "fov": 10, "tex_cube_size": 2}, S, 0.9, 1.1, device="cuda")
    yy, xx = torch.meshgrid(torch.linspace(-1, 1, S), torch.linspace(-1, 1, S), indexing="ij")
    depth = (1.0 - 0.06 * torch.exp(-(xx ** 2 + yy ** 2) * 2))[None].cuda()
    im = torch.stack([torch.sin(3 * xx), torch.cos(2 * yy), xx * yy])[None].cuda()
    # the reference builds the renderer with a white background (renderer.py:54): a ZERO mask marks
    # the covered pixels (0 inside, 1 where only background is seen).  The mesh renderer samples at
    # pixel + 0.5: compare with the warp shifted by half a pixel.
    for k, val in enumerate([0.0, 0.05, -0.08, 0.02, 0.01, -0.01, 0.02]):
        view = torch.zeros(1, 6, device="cuda")
        if k:
            view[0, k - 1] = val
        mesh, mesh_mask = R.render_given_view(im, depth, view, mask=torch.zeros_like(im), grid_sample=False)
        warp = R.render_given_view(im, depth, view, grid_sample=True)
        inside = (mesh_mask[:, :1] < 0.001).expand_as(im).clone()
        inside[..., :3, :] = inside[..., -3:, :] = False
        inside[..., :, :3] = inside[..., :, -3:] = False
        assert inside.float().mean() > 0.6
        shifted = torch.nn.functional.avg_pool2d(torch.nn.functional.pad(warp, (0, 1, 0, 1), mode="replicate"), 2, stride=1)
        err = float((mesh - shifted)[inside].abs().max())
        assert err < (1e-3 if k == 0 else 0.06), (k, err)     # identity pose: the same picture to 1e-4
    yaw = R.render_yaw(im, depth, maxr=20, nsample=5)
    assert tuple(yaw.shape) == (1, 5, 3, S, S)
    ident = R.render_given_view(im, depth, torch.zeros(1, 6, device="cuda"), grid_sample=False)
    torch.testing.assert_close(yaw[:, 2], ident, rtol=1e-5, atol=1e-5)
    sweep = R.render_view(im, depth, maxr=[10, 20], nsample=[3, 5])
    assert tuple(sweep.shape) == (1, 8, 3, S, S)
    torch.testing.assert_close(sweep[:, 2], ident, rtol=1e-5, atol=1e-5)     # middle yaw = 0
    torch.testing.assert_close(sweep[:, 6], ident, rtol=1e-5, atol=1e-5)     # middle pitch = 0
    gs = R.render_yaw(im, depth, maxr=20, nsample=3, grid_sample=True)
    assert tuple(gs.shape) == (1, 3, 3, S, S) and bool(torch.isfinite(gs).all())
    crop = R.render_yaw(im, depth, maxr=10, nsample=3, crop_mesh=(2, 2, 3, 3))
    assert tuple(crop.shape) == (1, 3, 3, S, S)


# ----------------------------------------------------------------------------- paired nets (grouped launches)
@pytest.mark.parametrize("names,B", [(("DepthNet", "AlbedoNet"), 1), (("ViewpointNet", "LightingNet"), 1),
                                     (("ViewpointNet", "LightingNet"), 5)])
def test_paired_nets_equal_the_two_nets(g2s, names, B):
    """forward_pair (one pass with twice the channels: g2s_conv2d / g2s_conv2d_wgrad with groups = 2,
    GroupNorm over twice the groups) against the same two nets run one after the other: outputs
    and every parameter gradient — also with one net frozen (step 1: only the albedo net trains)."""
    import copy
    from gan2shape_amd import networks
    torch.manual_seed(0)
    a, b = getattr(networks, names[0])(128).cuda(), getattr(networks, names[1])(128).cuda()
    a2, b2 = copy.deepcopy(a), copy.deepcopy(b)
    assert networks.pair_parameters(a, b) >= len(list(a.parameters())) - 1
    for p, q in zip(list(a.parameters()) + list(b.parameters()), list(a2.parameters()) + list(b2.parameters())):
        assert torch.equal(p, q)                                    # pairing moves storage, not values
    x = torch.randn(B, 3, 128, 128, device="cuda")
    for train_a in (True, False):
        ya, yb = networks.forward_pair(a, b, x, train_a=train_a)
        ra, rb = a2(x), b2(x)
        torch.testing.assert_close(ya, ra, rtol=1e-4, atol=1e-5 * float(ra.abs().max()))
        torch.testing.assert_close(yb, rb, rtol=1e-4, atol=1e-5 * float(rb.abs().max()))
        ga, gb = torch.randn_like(ra), torch.randn_like(rb)
        for net in (a, b, a2, b2):
            for p in net.parameters():
                p.grad = None
        ((ya * ga).sum() + (yb * gb).sum()).backward()
        ((ra * ga).sum() * (1.0 if train_a else 0.0) + (rb * gb).sum()).backward()
        frozen = set() if train_a else {id(p) for p in a.parameters()}
        rel = []
        for (n, p), q in zip(list(a.named_parameters()) + list(b.named_parameters()),
                             list(a2.parameters()) + list(b2.parameters())):
            if id(p) in frozen:
                assert p.grad is None or float(p.grad.abs().max()) == 0.0, n     # no gradient reaches a frozen net
                continue
            rel.append((float((p.grad - q.grad).norm()) / (float(q.grad.norm()) + 1e-12), n))
        # the grouped and the single launches sum in different orders (and split-K adds float-atomic
        # noise): an activation within rounding of zero then takes the other slope in one of the two
        # passes and moves the gradients below it by up to ~1 % (observed: one run in ~8 has such a
        # flip; 8e-3 on the first layer's weights).  Typical tensors agree to 1e-4.
        errs = sorted(e for e, _ in rel)
        assert errs[len(errs) // 2] <= 5e-4, rel
        assert errs[-1] <= 3e-2, max(rel)


@pytest.mark.gpu
def test_one_launch_adam_equals_torch_adam(g2s):
    """optim.Adam (g2s_adam_step: every tensor of the optimiser in one grid, device-side step counter)
    against torch.optim.Adam — the reference's optimiser, GAN2Shape/trainer.py:163-171 — over 6 steps
    with fresh gradients: ragged sizes (vector tail, chunk borders), a parameter without a gradient."""
    from gan2shape_amd.optim import Adam
    torch.manual_seed(3)
    shapes = [(64, 32, 4, 4), (1,), (7,), (3, 5, 5, 5), (16385,), (256, 257), (4,), (2, 3)]
    ref_p = [torch.randn(s, dtype=torch.float64) for s in shapes]
    ours = [p.float().cuda().requires_grad_(True) for p in ref_p]
    ref = [p.clone().requires_grad_(True) for p in ref_p]
    kw = dict(lr=1e-2, betas=(0.9, 0.999), weight_decay=5e-4)
    o_ours, o_ref = Adam(ours, **kw), torch.optim.Adam(ref, **kw)
    for it in range(6):
        for i, (a, b) in enumerate(zip(ours, ref)):
            if i == 4 and it % 2:       # no gradient this step: torch skips the tensor, so do we
                a.grad = b.grad = None
                continue
            g = torch.randn(b.shape, dtype=torch.float64) * (1 + it)
            b.grad = g.clone()
            a.grad = g.float().cuda()
        o_ours.step()
        o_ref.step()
    for a, b in zip(ours, ref):
        np.testing.assert_allclose(a.detach().cpu().numpy(), b.detach().numpy(), rtol=2e-5, atol=2e-6)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(8, 3, 64, 64), (2, 5, 7, 9), (3, 128, 16, 16)])
def test_add_bias_scale_matches_torch(g2s, shape):
    """(a + b + bias[c]) * scale — ToRGB's conv + bias + upsample(skip) and the ResBlock's
    (out + skip) / sqrt(2) (stylegan2-pytorch/model.py:371-377, 693-697) as one launch: values and
    gradients against the torch expressions, with and without b / bias."""
    from gan2shape_amd.op import add_bias_scale
    torch.manual_seed(1)
    for use_b, use_bias, scale in [(True, True, 1.0), (True, False, 2 ** -0.5), (False, True, 1.0)]:
        a = torch.randn(shape, device="cuda", requires_grad=True)
        b = torch.randn(shape, device="cuda", requires_grad=True) if use_b else None
        bias = torch.randn(1, shape[1], 1, 1, device="cuda", requires_grad=True) if use_bias else None
        y = add_bias_scale(a, b, bias, scale)
        ref = a if b is None else a + b
        if bias is not None:
            ref = ref + bias
        ref = ref * scale
        torch.testing.assert_close(y, ref, rtol=1e-6, atol=1e-6)
        g = torch.randn_like(y)
        ins = [t for t in (a, b, bias) if t is not None]
        for got, want in zip(torch.autograd.grad(y, ins, g), torch.autograd.grad(ref, ins, g)):
            torch.testing.assert_close(got, want, rtol=1e-5, atol=1e-5)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(9, 64, 128, 128), (2, 5, 6, 16), (1, 3, 2, 8)])
def test_maxpool2x2_equals_torch(g2s, shape):
    """g2s_maxpool2x2_fwd / _bwd against nn.MaxPool2d(2, 2) (the VGG16 trunk's pools, lpips/
    pretrained_networks.py:97-135): values and gradient, bit for bit — including the windows of equal
    values a ReLU feeds it (the first maximum in row-major order takes the gradient) and NaNs."""
    from gan2shape_amd.lpips import max_pool_2x2
    torch.manual_seed(2)
    x = torch.relu(torch.randn(shape, device="cuda"))        # ~half the windows contain ties at 0
    x[..., ::3, ::5] = 1.5                                       # more ties, away from zero
    if x.numel() > 64:
        x.view(-1)[7] = float("nan")
    pool = torch.nn.MaxPool2d(2, 2)
    xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    y, ref = max_pool_2x2(pool, xa), pool(xb)
    assert torch.equal(torch.nan_to_num(y, nan=-7.0), torch.nan_to_num(ref, nan=-7.0))
    g = torch.randn_like(ref)
    (ga,), (gb,) = torch.autograd.grad(y, xa, g), torch.autograd.grad(ref, xb, g)
    assert torch.equal(ga, gb)
