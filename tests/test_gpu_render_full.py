"""Renderer.render / render_silhouettes / lit render_rgb on the GPU: g2s_face_light_fwd / _bwd, g2s_raster_rgba_fwd /
_bwd and RenderFunction of plugins/neural_renderer.py.

Reference of every numeric comparison: the float64 restatement of render_full_cases.py (`restate` of
test_gpu_render_rgb_grad.py, its gathered colour multiplied by the float64 light of the winning face), on the
winners the kernel under test was given.  No element is excluded from a comparison.  The conditioning of the
cases is asserted on the CPU (test_render_full_cpu.py); the S = 20 case is used at twice the size of make_case's scene,
where its faces meet the |cross| threshold (render_full_cases.SCALES: a power of two, so its fp32 arithmetic is that
of the unscaled scene and its figures are the same).

Measured on the MI355X against the restatement (relative L2 over the whole tensor, default mode; every bound
below is 4x the measured figure rounded up to one digit; the factor covers the run-to-run spread of the atomic
summation order, 1e-7):

    case (S, ts, C, fill_back, implicit)   light fwd   light bwd   lit rgb fwd (unlit)    textures    vertices
    (16, 2, 3, True, True)                 4.56e-8     2.13e-7     9.84e-7 (2.86e-6)      9.92e-6     3.52e-5
    (20, 2, 3, True, False)                4.55e-8     1.73e-7     6.58e-7 (1.73e-6)      6.56e-6     2.46e-5
    (12, 2, 3, False, True)                3.63e-8     1.22e-7     5.16e-7 (1.34e-6)      4.95e-6     2.87e-5
    (16, 1, 3, True, True)                 4.73e-8     1.67e-7     2.62e-8 (7.16e-8)      3.91e-7     4.37e-7
    R, t on (16, 2, 3, True, True)                                 7.72e-7                            5.34e-5

"light" is g2s_face_light_fwd / _bwd alone; "textures" / "vertices" are the gradients of sum(w_rgb * rgb) through the
lit `render` (texture lookup and light together).  The lit forward error is BELOW the unlit render_rgb error of the
same case (in brackets; both relative, and the lit image is darker on the faces while the unlit background weighs the
same), far inside the 10x the light may add.  The texture gradient sits at the unlit path's figures
(test_gpu_render_rgb_grad.py: 1.03e-5, 6.23e-6, 4.82e-7 for the three cases it shares): the same adjoint times a
factor.  With ts = 1 the texture lookup has no vertex gradient, so that row's vertex figure is the light path alone,
at fp32 rounding.  Depth part of the vertex gradient against RenderDepthFunction's backward on the same maps: 1.4e-8 ..
2.9e-8 of max |g|; combined gradient minus the sum of the two separate ones: 7.2e-9 .. 2.7e-8 of max |g| (bar for
both: 3e-5, the depth backward's atomic-order bar).
"""
import ctypes as C

import numpy as np
import pytest
import torch

from render_full_cases import AMBIENT, BG, CA, CASES, CD, DIRECTIONAL, IA, ID, light, lit_case, restate_lit
from test_gpu_render_rgb_grad import EPS, FAR, NEAR, dev, g2s, raw_maps, rel_l2, restate  # noqa: F401 (g2s: fixture)

gpu = pytest.mark.gpu

# relative L2 over the whole tensor against the float64 restatement: 4x the measured figure, rounded up to one
# digit (module docstring)
LIGHT_FWD_BOUND = dict(zip(CASES, (2e-7, 2e-7, 2e-7, 2e-7)))
LIGHT_BWD_BOUND = dict(zip(CASES, (9e-7, 7e-7, 5e-7, 7e-7)))
RGB_FWD_BOUND = dict(zip(CASES, (4e-6, 3e-6, 3e-6, 2e-7)))
TEX_BOUND = dict(zip(CASES, (4e-5, 3e-5, 2e-5, 2e-6)))
VERT_BOUND = dict(zip(CASES, (2e-4, 1e-4, 2e-4, 2e-6)))
RT_FWD_BOUND, RT_VERT_BOUND = 4e-6, 3e-4
DEPTH_BAR = 3e-5    # of max |g|: the atomic-order bar of the depth backward's existing tests


# ------------------------------------------------------------------------------------- helpers
def _f3(v):
    return (C.c_float * 3)(*[float(x) for x in v])


def _dev_case(key):
    d = dict(lit_case(key))
    d["key"] = key
    d["dverts"], d["dtex"], d["dgrad"] = dev(d["verts"]), dev(d["tex"]), dev(d["grad"])
    d["dfaces"] = None if d["implicit"] else dev(d["faces"], torch.int32)
    return d


def _renderer(d, **kw):
    from gan2shape_amd.plugins import neural_renderer as nr
    args = dict(camera_mode='projection', K=dev(d["K"][None]), image_size=d["S"], orig_size=d["S"],
                fill_back=d["fill_back"], near=NEAR, far=FAR, light_intensity_ambient=IA,
                light_intensity_directional=ID, light_color_ambient=list(CA), light_color_directional=list(CD),
                light_direction=list(d["direction"]), background_color=list(BG))
    args.update(kw)
    return nr.Renderer(**args)


def _faces_arg(d):
    from gan2shape_amd.renderer.utils import get_face_idx
    B = d["dverts"].shape[0]
    if d["dfaces"] is None:
        return get_face_idx(B, d["S"], d["S"], device="cuda")
    return d["dfaces"][None].expand(B, -1, -1)


def _reference(d, fidx, verts64=None):
    """Lit float64 rendering on the winners `fidx`; (out, v64, t64) with v64, t64 requiring grad."""
    v64 = torch.tensor(d["verts"], dtype=torch.float64, requires_grad=True)
    t64 = torch.tensor(d["tex"], dtype=torch.float64, requires_grad=True)
    moved = v64 if verts64 is None else verts64(v64)
    out = restate_lit(moved, d["faces"], t64, fidx.cpu().numpy(), d["S"], d["K"], d["fill_back"], AMBIENT,
                      DIRECTIONAL, d["direction"])
    return out, v64, t64


def _face_light(lib, d, grad_light=None, acc_is_zero=0, into=None):
    """g2s_face_light_fwd, or _bwd when grad_light is given, through ctypes."""
    L = lib.load()
    verts, faces = d["dverts"], d["dfaces"]
    B, N, _ = verts.shape
    F = d["faces"].shape[0]
    fb = int(d["fill_back"])
    if grad_light is None:
        out = torch.full((B, F * (1 + fb), 3), float("nan"), device="cuda")
        lib.check(L.g2s_face_light_fwd(lib.ptr(verts), lib.ptr(faces), B, N, F, d["S"], fb, _f3(AMBIENT),
                                       _f3(DIRECTIONAL), _f3(d["direction"]), lib.ptr(out), lib.stream()))
        return out
    gv = torch.full_like(verts, float("nan")) if into is None else into
    ws, nbytes = None, 0
    if L.g2s_get_deterministic():
        nbytes = L.g2s_raster_bwd_workspace_bytes(B, N)
        ws = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    lib.check(L.g2s_face_light_bwd(lib.ptr(verts), lib.ptr(faces), lib.ptr(grad_light), B, N, F, d["S"], fb,
                                   _f3(DIRECTIONAL), _f3(d["direction"]), lib.ptr(gv), lib.ptr(ws), nbytes,
                                   acc_is_zero, lib.stream()))
    return gv


# ------------------------------------------------------------------------------------- 1. the light alone
@gpu
@pytest.mark.parametrize("key", CASES, ids=str)
def test_face_light_vs_restatement(g2s, key):
    """Forward and backward of the light alone, implicit and explicit topology, fill_back on and off.  The
    backward adds: with acc_is_zero = 1 onto what the buffer holds, bit-reproducibly in deterministic mode."""
    d = _dev_case(key)
    got = _face_light(g2s, d)
    v64 = torch.tensor(d["verts"], dtype=torch.float64, requires_grad=True)
    want, dot, _ = light(v64, d["faces"], d["fill_back"], AMBIENT, DIRECTIONAL, d["direction"])
    ef = rel_l2(got, want.detach())
    # both sides of the max are exercised, and a face lit from the front has a dark reversed copy
    assert 0.02 < float((dot > 0).double().mean()) < 0.98
    gl = torch.randn(want.shape, generator=torch.Generator().manual_seed(11), dtype=torch.float64)
    (want_v,) = torch.autograd.grad(want, v64, gl)
    gv = _face_light(g2s, d, dev(gl.numpy()))
    assert bool(torch.isfinite(gv).all())
    eb = rel_l2(gv, want_v)
    print(f"face light {key}: forward rel L2 {ef:.3e}  backward rel L2 {eb:.3e}")
    assert ef <= LIGHT_FWD_BOUND[key]
    assert eb <= LIGHT_BWD_BOUND[key]
    prev = g2s.set_deterministic(True)
    try:
        a = _face_light(g2s, d, dev(gl.numpy()))
        b = _face_light(g2s, d, dev(gl.numpy()))
        assert torch.equal(a, b) and rel_l2(a, want_v) <= LIGHT_BWD_BOUND[key]
        base = torch.randn(d["dverts"].shape, generator=torch.Generator().manual_seed(12)).cuda()
        added = _face_light(g2s, d, dev(gl.numpy()), acc_is_zero=1, into=base.clone())
        assert torch.equal(added, base + a)
    finally:
        g2s.set_deterministic(prev)


# ------------------------------------------------------------------------------------- 2. lit render_rgb, forward
@gpu
@pytest.mark.parametrize("key", CASES, ids=str)
def test_lit_render_rgb_forward(g2s, key):
    """The light adds one fp32 normalise and dot per face: the lit error stays within 10x the unlit render_rgb
    error of the same case (both against float64 on the same winners)."""
    d = _dev_case(key)
    fidx, _ = raw_maps(g2s, d["dverts"], d["dfaces"], d["S"], d["K"], d["fill_back"])
    out = _renderer(d).render_rgb(d["dverts"], _faces_arg(d), d["dtex"])
    want, _, _ = _reference(d, fidx)
    err = rel_l2(out, want.detach())
    plain = _renderer(d, light_intensity_ambient=1.0, light_intensity_directional=0.0,
                      light_color_ambient=[1, 1, 1]).render_rgb(d["dverts"], _faces_arg(d), d["dtex"])
    unlit = restate(torch.tensor(d["verts"], dtype=torch.float64), d["faces"], torch.tensor(d["tex"], dtype=torch.float64),
                    fidx.cpu().numpy(), d["S"], d["K"], background=BG)
    err_unlit = rel_l2(plain, unlit)
    print(f"lit render_rgb forward {key}: rel L2 {err:.3e}  (unlit {err_unlit:.3e})")
    assert err <= RGB_FWD_BOUND[key]
    assert err <= 10 * err_unlit


# ------------------------------------------------------------------------------------- 3.-5. unlit rgb, depth, alpha
@gpu
@pytest.mark.parametrize("key", CASES[:3], ids=str)
def test_render_outputs_exactly(g2s, key):
    """rgb of an unlit `render` is render_rgb's bit for bit; depth is g2s_raster_depth_fwd's with the
    constructor's near / far; alpha is the flipped mean over the 2x2 samples of (face_idx >= 0), exactly, without
    gradient, and render_silhouettes returns the same."""
    d = _dev_case(key)
    lib, L = g2s, g2s.load()
    verts, faces = d["dverts"], d["dfaces"]
    B, N, _ = verts.shape
    S, F = d["S"], d["faces"].shape[0]
    white = dict(light_intensity_ambient=1.0, light_intensity_directional=0.0, light_color_ambient=[1, 1, 1])
    r = _renderer(d, **white)
    v = verts.clone().requires_grad_(True)
    rgb, depth, alpha = r.render(v, _faces_arg(d), d["dtex"])
    assert torch.equal(rgb, r.render_rgb(verts, _faces_arg(d), d["dtex"]))
    want_depth = torch.empty((B, S, S), device="cuda")
    fidx = torch.empty((B, 2 * S, 2 * S), dtype=torch.int32, device="cuda")
    bary = torch.empty((B, 2 * S, 2 * S, 3), device="cuda")
    ws = torch.empty(L.g2s_raster_workspace_bytes(B, N, F, S), dtype=torch.uint8, device="cuda")
    Kc = (C.c_float * 9)(*np.asarray(d["K"], np.float32).reshape(9).tolist())
    lib.check(L.g2s_raster_depth_fwd(lib.ptr(verts), lib.ptr(faces), B, N, F, S, Kc, float(S), 2, int(d["fill_back"]),
                                     NEAR, FAR, lib.ptr(want_depth), lib.ptr(fidx), lib.ptr(bary), lib.ptr(ws),
                                     ws.numel(), lib.stream()))
    assert torch.equal(depth, want_depth)
    want_alpha = (fidx >= 0).float().flip(1).reshape(B, S, 2, S, 2).mean((2, 4))
    assert torch.equal(alpha, want_alpha)
    assert bool((alpha * 4 == (alpha * 4).round()).all()) and 0.1 < float(alpha.mean()) < 0.95
    assert not alpha.requires_grad and rgb.requires_grad and depth.requires_grad
    lit = _renderer(d)
    sil = lit.render_silhouettes(v, _faces_arg(d))
    assert torch.equal(sil, alpha) and not sil.requires_grad
    assert torch.equal(lit.render(verts, _faces_arg(d), d["dtex"])[2], alpha)


# ------------------------------------------------------------------------------------- 6. gradients through render
@gpu
@pytest.mark.parametrize("key", CASES, ids=str)
def test_render_gradients(g2s, key):
    """sum(w_rgb * rgb) + sum(w_d * depth) through the lit `render`: the rgb part against the restatement's
    autograd (texture lookup and light), the depth part against RenderDepthFunction's backward, the combined vertex
    gradient against the sum of the two."""
    from gan2shape_amd.plugins.neural_renderer import RenderDepthFunction
    d = _dev_case(key)
    r = _renderer(d)
    v = d["dverts"].clone().requires_grad_(True)
    t = d["dtex"].clone().requires_grad_(True)
    w_d = torch.randn((v.shape[0], d["S"], d["S"]), generator=torch.Generator().manual_seed(7)).cuda()
    rgb, depth, alpha = r.render(v, _faces_arg(d), t)
    gv_rgb, gt = torch.autograd.grad(rgb, (v, t), d["dgrad"], retain_graph=True)
    (gv_depth,) = torch.autograd.grad(depth, v, w_d, retain_graph=True)
    gv_all, gt_all = torch.autograd.grad((rgb, depth), (v, t), (d["dgrad"], w_d))
    fidx, _ = raw_maps(g2s, d["dverts"], d["dfaces"], d["S"], d["K"], d["fill_back"])
    want, v64, t64 = _reference(d, fidx)
    want_v, want_t = torch.autograd.grad(want, (v64, t64), torch.tensor(d["grad"], dtype=torch.float64))
    et, ev = rel_l2(gt, want_t), (rel_l2(gv_rgb, want_v) if float(want_v.abs().max()) > 0 else 0.0)
    # depth part: the existing backward on the same maps (same near / far)
    v2 = d["dverts"].clone().requires_grad_(True)
    dref = RenderDepthFunction.apply(v2, d["dfaces"], tuple(np.asarray(d["K"], np.float32).reshape(9).tolist()),
                                     d["S"], d["S"], True, d["fill_back"], NEAR, FAR)
    assert torch.equal(dref, depth)
    (want_depth_v,) = torch.autograd.grad(dref, v2, w_d)
    ed = float((gv_depth - want_depth_v).abs().max() / want_depth_v.abs().max())
    es = float((gv_all - (gv_rgb + gv_depth)).abs().max() / gv_all.abs().max())
    print(f"render gradients {key}: textures rel L2 {et:.3e}  vertices rel L2 {ev:.3e}  "
          f"depth part {ed:.3e} of max  combined - sum {es:.3e} of max")
    assert bool(torch.isfinite(gv_all).all())
    assert et <= TEX_BOUND[key]
    assert ev <= VERT_BOUND[key]
    assert ed <= DEPTH_BAR
    assert es <= DEPTH_BAR
    assert rel_l2(gt_all, want_t) <= TEX_BOUND[key]


# ------------------------------------------------------------------------------------- 7. deterministic mode
@gpu
def test_deterministic_render_is_bit_reproducible(g2s):
    d = _dev_case(CASES[1])
    r = _renderer(d)
    w_d = torch.randn((2, d["S"], d["S"]), generator=torch.Generator().manual_seed(7)).cuda()

    def run():
        v = d["dverts"].clone().requires_grad_(True)
        t = d["dtex"].clone().requires_grad_(True)
        rgb, depth, _ = r.render(v, _faces_arg(d), t)
        return torch.autograd.grad((rgb, depth), (v, t), (d["dgrad"], w_d))

    prev = g2s.set_deterministic(True)
    try:
        a, b = run(), run()
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        assert float(a[0].abs().max()) > 0 and float(a[1].abs().max()) > 0
    finally:
        g2s.set_deterministic(prev)


# ------------------------------------------------------------------------------------- 8. R, t
@gpu
def test_rotation_and_translation_reach_the_light(g2s):
    """R, t are applied before the light: forward and vertex gradient equal the restatement's on R v + t."""
    key = CASES[0]
    d = _dev_case(key)
    ang = 0.05
    Rm = np.array([[np.cos(ang), 0, np.sin(ang)], [0, 1, 0], [-np.sin(ang), 0, np.cos(ang)]], np.float32)
    tv = np.array([0.004, -0.003, 0.01], np.float32)
    r = _renderer(d, R=dev(Rm[None]), t=dev(tv[None]))
    v = d["dverts"].clone().requires_grad_(True)
    rgb, _, _ = r.render(v, _faces_arg(d), d["dtex"])
    (gv,) = torch.autograd.grad(rgb, v, d["dgrad"])
    with torch.no_grad():
        moved = (torch.matmul(d["dverts"], dev(Rm[None]).transpose(2, 1)) + dev(tv).reshape(1, 1, 3)).contiguous()
    fidx, _ = raw_maps(g2s, moved, d["dfaces"], d["S"], d["K"], d["fill_back"])
    R64, t64_ = torch.tensor(Rm, dtype=torch.float64), torch.tensor(tv, dtype=torch.float64)
    want, v64, _ = _reference(d, fidx, verts64=lambda x: torch.matmul(x, R64.T) + t64_)
    (want_v,) = torch.autograd.grad(want, v64, torch.tensor(d["grad"], dtype=torch.float64))
    ef, ev = rel_l2(rgb.detach(), want.detach()), rel_l2(gv, want_v)
    print(f"R, t: forward rel L2 {ef:.3e}  vertices rel L2 {ev:.3e}")
    assert ef <= RT_FWD_BOUND
    assert ev <= RT_VERT_BOUND
