"""Gradients of the texture pass (g2s_raster_rgb_bwd, nr.Renderer.render_rgb, Renderer.render_given_view
with grid_sample=False).

The oracle has no backward for this pass, so the reference gradient is the autograd of `restate`, a
float64 torch restatement of the texture pass that takes the winning face of every raster sample as
data and everything else (projection, screen-space barycentrics, clamp + renormalise, perspective
correction, cube coordinates and their clamps, trilinear read, background, flip, average) as
differentiable torch.  `test_restatement_equals_oracle` (CPU) pins it to the oracle's float64
render_rgb to 1e-9: both are float64 evaluations of the same formula.  The GPU tests hand the
restatement the winners the kernel under test was given (the maps of g2s_raster_depth_fwd, which are
bit-equal to the fp32 oracle's): the gradient is defined with the winners held fixed, so both sides
must hold the same ones.

Measured on the MI355X against the restatement (relative L2 over the whole tensor, default mode; each
bound below is 4x the measured figure rounded up to one digit):

    case (S, ts, C, fill_back, implicit)   textures    vertices   (1 - cosine, vertices)
    (16, 2, 3, True, True)                 1.03e-5     3.21e-5    5.1e-10
    (16, 1, 3, True, True)                 4.82e-7     exactly 0
    (20, 2, 3, True, False)                6.23e-6     1.89e-5    1.8e-10
    (12, 2, 1, False, True)                2.92e-6     9.61e-6    4.4e-11
    (32, 2, 3, True, True)                 4.78e-6     1.20e-4    5.7e-9
    (16, 3, 3, True, True)                 1.29e-5     -
    smooth64 (S = 64, no folds)            1.53e-4     9.40e-3    4.4e-5
    texture-sum identity                   <= 1.9e-8 in every case
    R, t, ambient on (16, 2, 3, T, T)      1.17e-5     6.70e-5

These figures are not summation rounding of the backward: a float64 evaluation of the kernel's formulas on
the same saved fp32 weights reproduces them to four digits (smooth64: 1.530e-4 / 9.397e-3), and on float64
weights it agrees with the restatement to 1e-14 / 4e-8.  They are the rounding of the barycentric weights
the depth pass saves: the pixel-space inverse vertex matrix has entries of order (raster side)^2 / area
that cancel to a weight in [0, 1], so the saved weights of smooth64 (128 x 128 raster, faces two samples
wide) differ from the float64 ones by up to 3.7e-4 (2.7e-5 on average), and forward and backward read the
cube at that slightly displaced position.  The vertex gradient differentiates the trilinear read, which
turns the displacement into a first-order error of every term, and divides by the faces' areas.  The
run-to-run spread of the atomic summation order (1e-7) is far inside the factor 4.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import capi
from oracle import geometry as og
from raster_cases import scene

gpu = pytest.mark.gpu

# (S, ts, C, fill_back, implicit): the sets of test_render_rgb_vs_oracle plus one with ts = 3
CASES = [(16, 2, 3, True, True), (16, 1, 3, True, True), (20, 2, 3, True, False), (12, 2, 1, False, True),
         (32, 2, 3, True, True), (16, 3, 3, True, True)]
SMOOTH = "smooth64"
NEAR, FAR, EPS = 0.1, 10.0, 1e-3

# 4x the measured relative L2 error, rounded up to one digit (module docstring)
TEX_BOUND = {(16, 2, 3, True, True): 5e-5, (16, 1, 3, True, True): 2e-6, (20, 2, 3, True, False): 3e-5,
             (12, 2, 1, False, True): 2e-5, (32, 2, 3, True, True): 2e-5, (16, 3, 3, True, True): 6e-5, SMOOTH: 7e-4}
VERT_BOUND = {(16, 2, 3, True, True): 2e-4, (20, 2, 3, True, False): 8e-5, (12, 2, 1, False, True): 4e-5,
              (32, 2, 3, True, True): 5e-4, SMOOTH: 4e-2}
FIT_RATIO = 0.01


# ------------------------------------------------------------------------------------- the restatement
def restate(verts, faces, tex, face_idx, S, K, ssaa=2, background=(1.0, 1.0, 1.0), eps=EPS, orig_size=None):
    """float64 texture pass.  verts [B,N,3], tex [B,F,ts,ts,ts,C] float64 tensors (differentiable);
    faces (F,3) and face_idx [B,is,is] integer arrays (data).  Returns [B,C,S,S].  Every operation runs in the
    dtype of `verts`, so float32 inputs give the float32 evaluation of the same formula (the yardstick of
    tests/test_raster_core_cpu.py)."""
    B, N, _ = verts.shape
    dt = verts.dtype
    F, ts, Cc = tex.shape[1], tex.shape[2], tex.shape[5]
    isz = S * ssaa
    osz = float(S if orig_size is None else orig_size)
    K = np.asarray(K, np.float64).reshape(3, 3)
    fidx = torch.as_tensor(np.asarray(face_idx), dtype=torch.long)
    faces = torch.as_tensor(np.asarray(faces), dtype=torch.long)
    # projection.py: camera xyz -> (u_n, v_n, z)
    x, y, z = verts[..., 0], verts[..., 1], verts[..., 2]
    x_, y_ = x / (z + 1e-9), y / (z + 1e-9)
    u = (x_ * K[0, 0] + y_ * K[0, 1]) + K[0, 2]
    v = (x_ * K[1, 0] + y_ * K[1, 1]) + K[1, 2]
    v = osz - v
    u = 2.0 * (u - osz / 2.0) / osz
    v = 2.0 * (v - osz / 2.0) / osz
    bn, yi, xi = torch.nonzero(fidx >= 0, as_tuple=True)
    fn = fidx[bn, yi, xi]
    g, rev = fn % F, fn >= F
    vid = faces[g]
    vid = torch.where(rev[:, None], vid.flip(1), vid)                      # [M, 3]
    pu, pv, pz = u[bn[:, None], vid], v[bn[:, None], vid], z[bn[:, None], vid]
    # kernel_1: inverse of the pixel-space vertex matrix; kernel_2: weights at the sample, clamp, renormalise
    p0 = 0.5 * (pu * isz + isz - 1.0)
    p1 = 0.5 * (pv * isz + isz - 1.0)
    den = p0[:, 2] * (p1[:, 0] - p1[:, 1]) + p0[:, 0] * (p1[:, 1] - p1[:, 2]) + p0[:, 1] * (p1[:, 2] - p1[:, 0])
    xf, yf = xi.to(dt), yi.to(dt)
    w = torch.stack([
        ((p1[:, 1] - p1[:, 2]) * xf + (p0[:, 2] - p0[:, 1]) * yf + (p0[:, 1] * p1[:, 2] - p0[:, 2] * p1[:, 1])) / den,
        ((p1[:, 2] - p1[:, 0]) * xf + (p0[:, 0] - p0[:, 2]) * yf + (p0[:, 2] * p1[:, 0] - p0[:, 0] * p1[:, 2])) / den,
        ((p1[:, 0] - p1[:, 1]) * xf + (p0[:, 1] - p0[:, 0]) * yf + (p0[:, 0] * p1[:, 1] - p0[:, 1] * p1[:, 0])) / den,
    ], 1)
    w = w.clamp(0.0, 1.0)
    w = w / w.sum(1, keepdim=True)
    depth = 1.0 / (w / pz).sum(1, keepdim=True)
    t = (w * float(ts - 1) * (depth / pz)).clamp(min=0.0)
    t = torch.minimum(t, torch.full_like(t, float(ts - 1) - eps))
    base = t.detach().to(torch.long)                                       # C cast: truncation
    frac = t - base.to(dt)
    col = torch.zeros((fn.shape[0], Cc), dtype=dt)
    for pn in range(8):
        wt = torch.ones_like(frac[:, 0])
        idx = []
        for k in range(3):
            if (pn >> k) % 2 == 0:
                wt = wt * (1.0 - frac[:, k])
                idx.append(base[:, k])
            else:
                wt = wt * frac[:, k]
                idx.append(torch.clamp(base[:, k] + 1, max=ts - 1))
        i0 = torch.where(rev, idx[2], idx[0])                              # reversed copy: axes 0 and 2 swapped
        i2 = torch.where(rev, idx[0], idx[2])
        col = col + wt[:, None] * tex[bn, g, i0, idx[1], i2]
    ss = torch.as_tensor(np.asarray(background, np.float64)[:Cc]).to(dt).expand(B, isz, isz, Cc).contiguous()
    ss = ss.index_put((bn, yi, xi), col)
    ss = ss.flip(1).permute(0, 3, 1, 2)                                    # vertical flip, [B, C, is, is]
    return ss.reshape(B, Cc, S, ssaa, S, ssaa).sum((3, 5)) * (1.0 / (ssaa * ssaa))


def make_case(S, ts, Cc, seed_extra=0):
    geo, verts, faces = scene(S, B=2, seed=S + ts + Cc)
    rng = np.random.default_rng(S + seed_extra)
    tex = rng.uniform(-1, 1, (2, faces.shape[0], ts, ts, ts, Cc)).astype(np.float32)
    grad = rng.standard_normal((2, Cc, S, S)).astype(np.float32)
    return geo, verts, faces, tex, grad


def smooth_case():
    """The Gaussian-bump depth of test_renderer_texture_helpers_on_gpu (no folds), S = 64, small view."""
    S = 64
    yy, xx = np.meshgrid(np.linspace(-1, 1, S), np.linspace(-1, 1, S), indexing="ij")
    depth = (1.0 - 0.06 * np.exp(-(xx ** 2 + yy ** 2) * 2))[None].astype(np.float32)
    geo = og.Geometry(S, 0.9, 1.1, rot_center_depth=1.0, fov=10)
    geo.set_transform_matrices(np.array([[0.05, -0.08, 0.02, 0.01, -0.01, 0.02]], np.float32))
    verts = geo.get_warped_3d_grid(depth).reshape(1, -1, 3).astype(np.float32)
    faces = og.get_face_idx(1, S, S)[0]
    rng = np.random.default_rng(64)
    tex = rng.uniform(-1, 1, (1, faces.shape[0], 2, 2, 2, 3)).astype(np.float32)
    grad = rng.standard_normal((1, 3, S, S)).astype(np.float32)
    return geo, verts, faces, tex, grad


def reference_grads(verts, faces, tex, face_idx, grad, S, K, bg=(1.0, 1.0, 1.0)):
    v = torch.tensor(verts, dtype=torch.float64, requires_grad=True)
    t = torch.tensor(tex, dtype=torch.float64, requires_grad=True)
    out = restate(v, faces, t, face_idx, S, K, background=bg)
    gv, gt = torch.autograd.grad(out, (v, t), torch.tensor(grad, dtype=torch.float64))
    return gt, gv


def rel_l2(got, want):
    return float((got.double().cpu() - want).norm() / want.norm())


# ------------------------------------------------------------------------------------- 1. CPU: restatement vs oracle
@pytest.mark.parametrize("S,ts,Cc,fill_back,implicit", CASES)
def test_restatement_equals_oracle(S, ts, Cc, fill_back, implicit):
    """Both are float64 evaluations of the same formula on the oracle's float64 winners: 1e-9 absolute on
    colours in [-1, 1] is loose by several orders."""
    geo, verts, faces, tex, _ = make_case(S, ts, Cc)
    bg = [1.0, 0.5, -0.25][:Cc]
    ref = capi.render_rgb(verts, faces, tex, S, geo.K[0], fill_back=fill_back, near=NEAR, far=FAR, background=bg,
                          dtype=np.float64)
    maps = capi.render_depth(verts, faces, S, geo.K[0], fill_back=fill_back, near=NEAR, far=FAR, dtype=np.float64)
    assert (maps["face_idx"] >= 0).mean() > 0.1
    out = restate(torch.tensor(verts, dtype=torch.float64), faces, torch.tensor(tex, dtype=torch.float64),
                  maps["face_idx"], S, geo.K[0], background=bg)
    err = float(np.abs(out.numpy() - ref).max())
    print(f"restatement vs oracle {(S, ts, Cc, fill_back, implicit)}: max abs {err:.3e}")
    assert err <= 1e-9


# ------------------------------------------------------------------------------------- 7. argument checks (no launch)
def _bwd_args(**over):
    """A call of g2s_raster_rgb_bwd whose pointers are never dereferenced on the host: every case below is
    rejected before anything is launched."""
    K = (C.c_float * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1)
    one = C.c_void_p(256)
    a = dict(verts=one, faces=None, face_idx=one, bary=one, textures=one, grad_rgb=one, B=1, n_verts=16, n_faces=18,
             S=4, K=K, orig_size=4.0, ssaa=2, ts=2, C=3, eps=EPS, grad_textures=one, grad_verts=one, workspace=None,
             workspace_bytes=0, acc_is_zero=0, stream=None)
    a.update(over)
    return list(a.values())


@pytest.mark.parametrize("over,msg", [
    (dict(textures=None), "NULL pointer argument"),
    (dict(grad_rgb=None), "NULL pointer argument"),
    (dict(ts=9), "texture size 1..8, 1..4 channels"),
    (dict(C=5), "texture size 1..8, 1..4 channels"),
    (dict(ssaa=3), "ssaa must be 1 or 2"),
    (dict(grad_textures=None, grad_verts=None), "both NULL: nothing to compute"),
    (dict(n_verts=15), "implicit topology needs S*S vertices and 2(S-1)^2 faces"),
    (dict(n_faces=17), "implicit topology needs S*S vertices and 2(S-1)^2 faces"),
    (dict(K=None), "K must be a host pointer to 9 floats"),
])
def test_bwd_argument_checks(over, msg):
    """include/g2s.h: a bad argument is G2S_ERR_INVALID (-1) with its message, and nothing is launched (the
    pointers here are not device memory).  Both outputs NULL is an error, not a no-op: a call that can
    compute nothing is a caller's mistake."""
    from gan2shape_amd import lib
    L = lib.load()
    assert L.g2s_raster_rgb_bwd(*_bwd_args(**over)) == -1
    assert msg in L.g2s_last_error().decode()


def test_bwd_workspace_query():
    from gan2shape_amd import lib
    L = lib.load()
    assert L.g2s_raster_rgb_bwd_workspace_bytes(2, 16, 18, 2, 3) == (2 * 18 * 8 * 3 + 2 * 16 * 3) * 8 + 256
    assert L.g2s_raster_rgb_bwd_workspace_bytes(0, 16, 18, 2, 3) == 0


# ------------------------------------------------------------------------------------- GPU helpers
@pytest.fixture(scope="module")
def g2s():
    import gan2shape_amd  # noqa: F401
    from gan2shape_amd import lib
    lib.load()
    assert torch.cuda.is_available()
    return lib


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


def raw_maps(lib, verts, faces, S, K, fill_back=True, ssaa=2):
    """face_idx, bary of g2s_raster_depth_fwd with the texture pass's near / far."""
    L = lib.load()
    B, N, _ = verts.shape
    F = 2 * (S - 1) * (S - 1) if faces is None else faces.shape[0]
    depth = torch.empty((B, S, S), device="cuda")
    fidx = torch.empty((B, S * ssaa, S * ssaa), dtype=torch.int32, device="cuda")
    bary = torch.empty((B, S * ssaa, S * ssaa, 3), device="cuda")
    ws = torch.empty(L.g2s_raster_workspace_bytes(B, N, F, S), dtype=torch.uint8, device="cuda")
    Kc = (C.c_float * 9)(*np.asarray(K, np.float32).reshape(9).tolist())
    lib.check(L.g2s_raster_depth_fwd(lib.ptr(verts), lib.ptr(faces), B, N, F, S, Kc, float(S), ssaa, int(fill_back),
                                     NEAR, FAR, lib.ptr(depth), lib.ptr(fidx), lib.ptr(bary), lib.ptr(ws), ws.numel(),
                                     lib.stream()))
    return fidx, bary


def raw_bwd(lib, verts, faces, fidx, bary, tex, grad, S, K, want_t=True, want_v=True, ssaa=2, workspace="auto"):
    """g2s_raster_rgb_bwd through ctypes -> (return code, grad_textures or None, grad_verts or None)."""
    L = lib.load()
    B, N, _ = verts.shape
    F, ts, Cc = tex.shape[1], tex.shape[2], tex.shape[5]
    gt = torch.full_like(tex, float("nan")) if want_t else None
    gv = torch.full_like(verts, float("nan")) if want_v else None
    ws, nbytes = None, 0
    if workspace == "auto" and L.g2s_get_deterministic():
        nbytes = L.g2s_raster_rgb_bwd_workspace_bytes(B, N, F, ts, Cc)
        ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    Kc = (C.c_float * 9)(*np.asarray(K, np.float32).reshape(9).tolist())
    rc = L.g2s_raster_rgb_bwd(lib.ptr(verts), lib.ptr(faces), lib.ptr(fidx), lib.ptr(bary), lib.ptr(tex),
                              lib.ptr(grad), B, N, F, S, Kc, float(S), ssaa, ts, Cc, EPS, lib.ptr(gt), lib.ptr(gv),
                              lib.ptr(ws), nbytes, 0, lib.stream())
    torch.cuda.synchronize()
    return rc, gt, gv


def gpu_case(lib, key):
    """Device tensors of a case, the kernel's maps and the restatement's two gradients on the same winners."""
    if key == SMOOTH:
        geo, verts, faces, tex, grad = smooth_case()
        S, fill_back, implicit = 64, True, True
    else:
        S, ts, Cc, fill_back, implicit = key
        geo, verts, faces, tex, grad = make_case(S, ts, Cc)
    f = None if implicit else dev(faces, torch.int32)
    d = dict(S=S, K=geo.K[0], verts=dev(verts), faces=f, tex=dev(tex), grad=dev(grad), fill_back=fill_back)
    d["fidx"], d["bary"] = raw_maps(lib, d["verts"], f, S, geo.K[0], fill_back)
    d["want_t"], d["want_v"] = reference_grads(verts, faces, tex, d["fidx"].cpu().numpy(), grad, S, geo.K[0])
    d["np"] = (verts, faces, tex, grad)
    return d


# ------------------------------------------------------------------------------------- 2. textures
@gpu
@pytest.mark.parametrize("key", CASES + [SMOOTH], ids=str)
def test_texture_gradient_vs_restatement(g2s, key):
    """The forward is affine in the textures: the float64 gradient is exact and the fp32 kernel differs by
    summation rounding only.  Structure, exactly: faces that win no sample get exact zeros.  The sum over
    texels equals the sum of grad_rgb over covered samples / ssaa^2 (trilinear weights sum to one); its
    error is taken relative to the sum of the magnitudes it adds (the signed sum itself may cancel)."""
    d = gpu_case(g2s, key)
    rc, gt, _ = raw_bwd(g2s, d["verts"], d["faces"], d["fidx"], d["bary"], d["tex"], d["grad"], d["S"], d["K"],
                        want_v=False)
    assert rc == 0
    err = rel_l2(gt, d["want_t"])
    F = d["tex"].shape[1]
    fidx = d["fidx"].cpu().long()
    covered = fidx >= 0
    wins = torch.zeros(fidx.shape[0], F, dtype=torch.bool)
    bn = torch.nonzero(covered, as_tuple=True)[0]
    wins[bn, fidx[covered] % F] = True
    assert bool((gt.cpu()[~wins] == 0).all())
    assert bool((gt.cpu()[wins].flatten(1).abs().sum(1) > 0).all())
    # grad_rgb seen from the raster: sample (yi, xi) belongs to pixel ((is - 1 - yi) / 2, xi / 2)
    g_ss = d["grad"].double().cpu().flip(2).repeat_interleave(2, 2).repeat_interleave(2, 3) / 4.0
    g_cov = g_ss * covered[:, None].double()
    want_sum, scale = float(g_cov.sum()), float(g_cov.abs().sum())
    sum_err = abs(float(gt.double().sum()) - want_sum) / scale
    print(f"texture gradient {key}: rel L2 {err:.3e}  sum rel {sum_err:.3e}")
    assert err <= TEX_BOUND[key]
    assert sum_err <= TEX_BOUND[key]


# ------------------------------------------------------------------------------------- 3. vertices
@gpu
@pytest.mark.parametrize("key", [c for c in CASES if c[1] == 2] + [SMOOTH], ids=str)
def test_vertex_gradient_vs_restatement(g2s, key):
    """Relative L2 error over the whole [B, N, 3] tensor and the cosine between the two.  A relative error e
    bounds the cosine from below by sqrt(1 - e^2) >= 1 - e^2."""
    d = gpu_case(g2s, key)
    rc, _, gv = raw_bwd(g2s, d["verts"], d["faces"], d["fidx"], d["bary"], d["tex"], d["grad"], d["S"], d["K"],
                        want_t=False)
    assert rc == 0 and bool(torch.isfinite(gv).all())
    err = rel_l2(gv, d["want_v"])
    a, b = gv.double().cpu().flatten(), d["want_v"].flatten()
    cos = float(a @ b / (a.norm() * b.norm()))
    print(f"vertex gradient {key}: rel L2 {err:.3e}  1 - cos {1 - cos:.3e}")
    assert err <= VERT_BOUND[key]
    assert cos >= 1.0 - VERT_BOUND[key] ** 2


@gpu
def test_vertex_gradient_of_a_constant_cube_is_zero(g2s):
    """ts = 1: a constant cube has no lookup derivative; every vertex gradient is exactly zero."""
    d = gpu_case(g2s, (16, 1, 3, True, True))
    rc, gt, gv = raw_bwd(g2s, d["verts"], d["faces"], d["fidx"], d["bary"], d["tex"], d["grad"], d["S"], d["K"])
    assert rc == 0
    assert bool((gv == 0).all())
    assert float(d["want_v"].abs().max()) == 0.0
    assert float(gt.abs().max()) > 0


# ------------------------------------------------------------------------------------- 5. autograd and the renderer
def _renderer(g2s, d, **kw):
    from gan2shape_amd.plugins import neural_renderer as nr
    args = dict(camera_mode='projection', K=dev(d["K"][None]), image_size=d["S"], orig_size=d["S"],
                fill_back=d["fill_back"], near=NEAR, far=FAR, light_intensity_ambient=1.0,
                light_intensity_directional=0.0, background_color=[1, 1, 1])
    args.update(kw)
    return nr.Renderer(**args)


def _faces_arg(d):
    from gan2shape_amd.renderer.utils import get_face_idx
    B = d["verts"].shape[0]
    if d["faces"] is None:
        return get_face_idx(B, d["S"], d["S"], device="cuda")
    return d["faces"][None].expand(B, -1, -1)


@gpu
@pytest.mark.parametrize("key", [(16, 2, 3, True, True), (20, 2, 3, True, False)], ids=str)
def test_autograd_equals_the_raw_entry_point(g2s, key):
    d = gpu_case(g2s, key)
    r = _renderer(g2s, d)
    prev = g2s.set_deterministic(True)      # bit-equal sums: autograd and the raw call must agree exactly
    try:
        rc, gt, gv = raw_bwd(g2s, d["verts"], d["faces"], d["fidx"], d["bary"], d["tex"], d["grad"], d["S"], d["K"])
        assert rc == 0
        v = d["verts"].clone().requires_grad_(True)
        t = d["tex"].clone().requires_grad_(True)
        out = r.render_rgb(v, _faces_arg(d), t)
        assert out.requires_grad
        av, at = torch.autograd.grad(out, (v, t), d["grad"])
        assert torch.equal(av, gv) and torch.equal(at, gt)
        out_t = r.render_rgb(d["verts"], _faces_arg(d), t)
        g_v, g_t = torch.autograd.grad(out_t, (v, t), d["grad"], allow_unused=True)
        assert g_v is None and torch.equal(g_t, gt)
        out_v = r.render_rgb(v, _faces_arg(d), d["tex"])
        g_v, g_t = torch.autograd.grad(out_v, (v, t), d["grad"], allow_unused=True)
        assert g_t is None and torch.equal(g_v, gv)
        plain = r.render_rgb(d["verts"], _faces_arg(d), d["tex"])
        assert not plain.requires_grad and plain.grad_fn is None
        assert torch.equal(plain, out.detach()) and torch.equal(plain, out_t.detach())
    finally:
        g2s.set_deterministic(prev)


@gpu
def test_rotation_translation_and_ambient_are_carried_by_autograd(g2s):
    """R, t and light_intensity_ambient are torch ops outside the function: the gradients w.r.t. the
    untransformed vertices and the unscaled textures equal the restatement's composed with the same ops."""
    key = (16, 2, 3, True, True)
    d = gpu_case(g2s, key)
    verts_np, faces_np, tex_np, grad_np = d["np"]
    ang = 0.05
    Rm = np.array([[np.cos(ang), 0, np.sin(ang)], [0, 1, 0], [-np.sin(ang), 0, np.cos(ang)]], np.float32)
    tv = np.array([0.004, -0.003, 0.01], np.float32)
    amb = 0.7
    r = _renderer(g2s, d, R=dev(Rm[None]), t=dev(tv[None]), light_intensity_ambient=amb)
    v = d["verts"].clone().requires_grad_(True)
    t = d["tex"].clone().requires_grad_(True)
    out = r.render_rgb(v, _faces_arg(d), t)
    gv, gt = torch.autograd.grad(out, (v, t), d["grad"])
    # the winners of the transformed mesh, from the same fp32 vertices the plugin hands the kernel
    with torch.no_grad():
        moved = (torch.matmul(d["verts"], dev(Rm[None]).transpose(2, 1)) + dev(tv).reshape(1, 1, 3)).contiguous()
    fidx, _ = raw_maps(g2s, moved, d["faces"], d["S"], d["K"], True)
    v64 = torch.tensor(verts_np, dtype=torch.float64, requires_grad=True)
    t64 = torch.tensor(tex_np, dtype=torch.float64, requires_grad=True)
    m64 = torch.matmul(v64, torch.tensor(Rm, dtype=torch.float64).T) + torch.tensor(tv, dtype=torch.float64)
    ref = restate(m64, faces_np, t64 * amb, fidx.cpu().numpy(), d["S"], d["K"])
    wv, wt = torch.autograd.grad(ref, (v64, t64), torch.tensor(grad_np, dtype=torch.float64))
    np.testing.assert_allclose(out.detach().cpu().numpy(), ref.detach().numpy(), atol=2e-5)
    ev, et = rel_l2(gv, wv), rel_l2(gt, wt)
    print(f"R, t, ambient: vertices rel L2 {ev:.3e}  textures rel L2 {et:.3e}")
    assert et <= TEX_BOUND[key]
    assert ev <= VERT_BOUND[key]


@gpu
def test_render_given_view_is_differentiable(g2s):
    """Renderer.render_given_view(im, depth, view, grid_sample=False): gradients reach im, depth and view;
    the one to im equals the restatement's texture gradient pulled back through get_textures_from_im
    (a fixed linear map with coefficients 0, 1/2, 1), under the smooth scene's texture bound."""
    from gan2shape_amd.renderer import Renderer
    from gan2shape_amd.renderer.utils import get_face_idx, get_textures_from_im, get_transform_matrices
    S = 64
    R = Renderer({"rot_center_depth": 1.0, "fov": 10, "tex_cube_size": 2}, S, 0.9, 1.1, device="cuda")
    yy, xx = torch.meshgrid(torch.linspace(-1, 1, S), torch.linspace(-1, 1, S), indexing="ij")
    depth = (1.0 - 0.06 * torch.exp(-(xx ** 2 + yy ** 2) * 2))[None].cuda().requires_grad_(True)
    # inside (-1, 1) with room: the clamp of the rendering to [-1, 1] is then never active
    im = (0.6 * torch.stack([torch.sin(3 * xx), torch.cos(2 * yy), xx * yy]))[None].cuda().requires_grad_(True)
    view = torch.tensor([[0.05, -0.08, 0.02, 0.01, -0.01, 0.02]], device="cuda", requires_grad=True)
    out = R.render_given_view(im, depth, view, grid_sample=False)
    assert out.grad_fn is not None
    grad = torch.randn(out.shape, generator=torch.Generator().manual_seed(5)).cuda()
    g_im, g_depth, g_view = torch.autograd.grad(out, (im, depth, view), grad)
    for name, g in (("im", g_im), ("depth", g_depth), ("view", g_view)):
        assert bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0, name
    with torch.no_grad():
        rot, trans = get_transform_matrices(view)
        verts = R.translate_pts(R.rotate_pts(R.depth_to_3d_grid(depth).reshape(1, -1, 3), rot), trans).contiguous()
        tex = get_textures_from_im(im, tx_size=2)
    fidx, _ = raw_maps(g2s, verts, None, S, R.K[0].cpu().numpy())
    faces = get_face_idx(1, S, S, device="cpu")[0].numpy()
    t64 = tex.double().cpu().requires_grad_(True)
    ref = restate(verts.double().cpu(), faces, t64, fidx.cpu().numpy(), S, R.K[0].cpu().numpy())
    # |cube values| <= 1.5 * 0.6: the rendering stays inside the clamp; sanity of the forward (fp32 weights)
    assert float(ref.detach()[ref.detach() != 1.0].abs().max()) <= 0.9 + 1e-9
    np.testing.assert_allclose(out.detach().cpu().numpy(), ref.detach().numpy(), atol=1e-3)
    (want_tex,) = torch.autograd.grad(ref, t64, grad.double().cpu())
    im_cpu = im.detach().double().cpu().requires_grad_(True)
    tl, tr, bl, br = im_cpu[:, :, :-1, :-1], im_cpu[:, :, :-1, 1:], im_cpu[:, :, 1:, :-1], im_cpu[:, :, 1:, 1:]
    # get_textures_from_im in float64 (its coefficient table is float32: restated through its own helper)
    from gan2shape_amd.renderer.utils import _cube_coefficients
    vc = torch.cat([torch.stack([tl, tr, bl], -1).reshape(1, 3, -1, 3), torch.stack([bl, tr, br], -1).reshape(1, 3, -1, 3)], 2)
    cube = torch.matmul(_cube_coefficients("cpu").double(), vc.permute(0, 2, 3, 1)).reshape(1, -1, 2, 2, 2, 3)
    torch.testing.assert_close(cube.detach().float(), get_textures_from_im(im.detach().cpu(), tx_size=2), rtol=0, atol=1e-6)
    (want_im,) = torch.autograd.grad(cube, im_cpu, want_tex)
    err = rel_l2(g_im, want_im)
    print(f"render_given_view: d/d im rel L2 {err:.3e}")
    assert err <= TEX_BOUND[SMOOTH]


@gpu
def test_texture_fit_by_gradient_descent(g2s):
    """Use-level check that depends on no tolerance above: fit textures, from zero, to a rendering of random
    textures on a fixed mesh by plain gradient descent on f(x) = 1/2 |render(x) - target|^2.  The rendering
    is affine in x, f is a linear least-squares objective with Hessian A^T A, and gradient descent with a
    step below 2 / L, L = lambda_max(A^T A), decreases f monotonically.  L comes from a power iteration on
    the GPU forward + backward pair (A v = render(v) - render(0), A^T r = the texture gradient for grad_rgb =
    r); the step is 1 / L_est (the power iteration approaches L from below, so this is below 2 / L once
    L_est > L / 2).

    Measured: L_est 0.4353; loss 13.21 -> 0.978 (5 steps) -> 0.219 (10) -> 0.0437 (20) -> 0.0121 (35) -> 0.00489
    (50 steps): monotone, 3.7e-4 of the initial loss, so the 1 % target holds with room."""
    d = gpu_case(g2s, (16, 2, 3, True, True))
    r = _renderer(g2s, d)
    faces = _faces_arg(d)
    target = r.render_rgb(d["verts"], faces, d["tex"])
    zero = r.render_rgb(d["verts"], faces, torch.zeros_like(d["tex"]))

    def value_and_grad(x):
        x = x.detach().requires_grad_(True)
        res = r.render_rgb(d["verts"], faces, x) - target
        f = 0.5 * (res.double() ** 2).sum()
        (g,) = torch.autograd.grad(res, x, res.detach())
        return float(f), g

    v = torch.randn(d["tex"].shape, generator=torch.Generator().manual_seed(3)).cuda()
    L_est = 0.0
    for _ in range(30):
        v = v / v.norm()
        x = v.detach().requires_grad_(True)
        av = r.render_rgb(d["verts"], faces, x) - zero
        (v,) = torch.autograd.grad(av, x, av.detach())
        L_est = float(v.norm())
    step = 1.0 / L_est
    x = torch.zeros_like(d["tex"])
    curve = []
    for _ in range(50):
        f, g = value_and_grad(x)
        curve.append(f)
        x = x - step * g
    curve.append(value_and_grad(x)[0])
    print("texture fit: L_est %.4f, loss %s" % (L_est, " ".join(f"{c:.4e}" for c in curve[::5])))
    assert all(b < a for a, b in zip(curve, curve[1:])), curve
    assert curve[-1] < FIT_RATIO * curve[0], (curve[0], curve[-1])


# ------------------------------------------------------------------------------------- 6. deterministic mode
@gpu
def test_deterministic_mode_is_bit_reproducible(g2s):
    d = gpu_case(g2s, (32, 2, 3, True, True))     # folded scene
    prev = g2s.set_deterministic(True)
    try:
        a = raw_bwd(g2s, d["verts"], d["faces"], d["fidx"], d["bary"], d["tex"], d["grad"], d["S"], d["K"])
        b = raw_bwd(g2s, d["verts"], d["faces"], d["fidx"], d["bary"], d["tex"], d["grad"], d["S"], d["K"])
        assert a[0] == 0 and b[0] == 0
        assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
        assert rel_l2(a[1], d["want_t"]) <= TEX_BOUND[(32, 2, 3, True, True)]
        assert rel_l2(a[2], d["want_v"]) <= VERT_BOUND[(32, 2, 3, True, True)]
        rc, _, _ = raw_bwd(g2s, d["verts"], d["faces"], d["fidx"], d["bary"], d["tex"], d["grad"], d["S"], d["K"],
                           workspace=None)
        assert rc == -3 and "workspace" in g2s.load().g2s_last_error().decode()
    finally:
        g2s.set_deterministic(prev)


# ------------------------------------------------------------------------------------- 8. graph capture
@gpu
def test_forward_and_backward_replay_in_a_captured_graph(g2s):
    """One capture on a side stream, one replay on new values in the same buffers: scratch, maps and
    gradient targets are allocated per call, so the replay computes what the eager call computes
    (bit-equal in deterministic mode)."""
    d = gpu_case(g2s, (16, 2, 3, True, True))
    other_verts = dev(scene(16, B=2, seed=99)[1])
    r = _renderer(g2s, d)
    faces = _faces_arg(d)
    prev = g2s.set_deterministic(True)
    try:
        v = d["verts"].clone().requires_grad_(True)
        t = d["tex"].clone().requires_grad_(True)
        g = d["grad"].clone()

        def run():
            out = r.render_rgb(v, faces, t)
            gv, gt = torch.autograd.grad(out, (v, t), g)
            return out.detach(), gv, gt

        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            run()                                      # warm-up: code objects, cached host copies of K / R / t
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            captured = run()
        with torch.no_grad():
            v.copy_(other_verts)
            t.copy_(d["tex"].flip(1))
            g.copy_(d["grad"].flip(3))
        graph.replay()
        torch.cuda.synchronize()
        replayed = [x.clone() for x in captured]
        eager = run()
        torch.cuda.synchronize()
        for a, b in zip(replayed, eager):
            assert torch.equal(a, b)
        assert float(replayed[1].abs().max()) > 0 and float(replayed[2].abs().max()) > 0
    finally:
        g2s.set_deterministic(prev)
