"""Case table and plain-torch restatement of what csrc/geometry.hip, csrc/lpips.hip and csrc/losses.hip
compute, shared by tests/test_reduce_cases_cpu.py and tests/test_gpu_reduce_kernels.py.

The restatement.  One function per operation, written from the reference lines the three .hip headers cite
(renderer/utils.py:33-73, renderer.py:61-139, model.py:337-360, losses.py:6-79, lpips/networks_basic.py:64-92,
lpips/__init__.py:40-42), with the dtype as a parameter (`Ops`):

  * float64: plain torch, autograd supplies every backward.  This is the value the kernels are held to.
  * float32: the same lines, but every reduction over pixels, channels or the batch — in the forward
    (`Ops.sum`) and in the backward of a broadcast (`Ops.bcast`: gradients of R, t, light, the mean) — is ONE
    sequential fp32 accumulation (np.add.accumulate).  e32 = max|f32 - f64| is then the reference's own
    distance from float64 in the most pessimistic summation order, the yardstick for kernels that sum in
    trees and float atomics: max|kernel - f64| <= 4 e32 + 5e-6 max|f64| per output tensor (the bound of
    raster_cases.Case.data, for the same reason: the kernels do this arithmetic in another order).

Fixed conventions of the restatement:

  * sign(0) = 0 (torch.abs's backward; the kernels' sgn()).
  * The ReLU gate is x > 0 (shading's diffuse term, the LPIPS tail's relu_gate, wl1_bwd3's leaky gate).
  * The gradient of the LPIPS channel norm is 0 where the squared sum is 0: the kernel's k2 = 0.  The
    reference's own autograd gives NaN there (sqrt'(0) * 0); the sqrt below is guarded by a `where` on both
    sides, so no NaN arises.  The remaining gradient at such a pixel, 2 w (u - v) / eps, is kept (eps = 1e-10:
    values of the order 1e10, which is why such pixels are compared as an output tensor of their own).
  * Smoothness terms with an empty extent (W <= 2: dx2; H <= 2: dy2; H or W = 1: the mixed terms) contribute
    0, the kernel's smooth_weights.  The reference's mean() of an empty tensor is NaN.

Inputs.  Exact-grid inputs (L1, smoothness loss where a count is a power of two): dyadic values, so every
term and every partial sum is an fp32 number, any summation order gives the same bits, and the kernel must
EQUAL float64; ties (x == y) and flat regions (second difference 0) exercise sign(0) = 0.  Random inputs:
seeded; each case takes the first seed of `SEEDS` for which the float64 restatement keeps every element away
from every kink (`Case.conditioned`); nothing is masked out.
"""
import math
import zlib

import numpy as np
import torch

F32, F64 = torch.float32, torch.float64
SEEDS = (0, 1, 2, 3, 4, 5, 6, 7)
KINK = dict(shading_dot=1e-4, normal_rel=1e-4, diff=1e-5)


# ----------------------------------------------------------------------------- sequential fp32 reductions
def _seq(x, dims, keepdim=False):
    """Sum of `x` over `dims`, accumulated sequentially (row-major over those dims) in x's own dtype."""
    dims = sorted(d % x.dim() for d in dims)
    keep = [d for d in range(x.dim()) if d not in dims]
    a = x.detach().permute(*keep, *dims).reshape([x.shape[d] for d in keep] + [-1]).contiguous().numpy()
    if a.shape[-1] == 0:
        out = torch.zeros(a.shape[:-1], dtype=x.dtype)
    else:
        out = torch.from_numpy(np.add.accumulate(a, axis=-1, dtype=a.dtype)[..., -1].copy())
    if keepdim:
        for d in dims:
            out = out.unsqueeze(d)
    return out


class _SeqSum(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, dims):
        ctx.shape, ctx.dims = x.shape, sorted(d % x.dim() for d in dims)
        return _seq(x, dims)

    @staticmethod
    def backward(ctx, g):
        for d in ctx.dims:
            g = g.unsqueeze(d)
        return g.expand(ctx.shape), None


class _SeqBcast(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, shape):
        ctx.dims = [d for d in range(x.dim()) if x.shape[d] == 1 and shape[d] != 1]
        return x.expand(shape).clone()

    @staticmethod
    def backward(ctx, g):
        return _seq(g, ctx.dims, keepdim=True), None


class Ops:
    """The dtype of a restatement run and its two reduction primitives."""

    def __init__(self, dtype):
        self.dt, self.seq = dtype, dtype == F32

    def t(self, a, grad=False):
        return torch.tensor(np.asarray(a), dtype=self.dt).requires_grad_(grad)

    def sum(self, x, dims=None):
        dims = tuple(range(x.dim())) if dims is None else tuple(dims)
        if self.seq:
            return _SeqSum.apply(x, dims)
        return x.sum(dims) if x.numel() else torch.zeros([s for d, s in enumerate(x.shape) if d not in dims], dtype=x.dtype)

    def bcast(self, x, shape):
        """x (same number of dims, size 1 where it is repeated) -> shape; the backward sums over the repeats."""
        return _SeqBcast.apply(x, tuple(shape)) if self.seq else x.expand(shape)


def _grads(outs, cots, wrt):
    live = [(y, c) for y, c in zip(outs, cots) if y.requires_grad]       # an all-border normal map depends on nothing
    if not live:
        return [torch.zeros_like(w) for w in wrt]
    g = torch.autograd.grad([y for y, _ in live], wrt, [c for _, c in live], allow_unused=True, retain_graph=True)
    return [torch.zeros_like(w) if x is None else x for x, w in zip(g, wrt)]


def f32(v):
    return float(np.float32(v))


# ----------------------------------------------------------------------------- the operations
def view_transform(o, view, rot, txy, tz):
    """model.py:330-335 + renderer/utils.py:33-73: R = Rz Ry Rx [B,3,3], t [B,3]."""
    a = view[:, :3] * rot
    zero, one = torch.zeros_like(a[:, 0]), torch.ones_like(a[:, 0])
    cx, sx, cy, sy, cz, sz = a[:, 0].cos(), a[:, 0].sin(), a[:, 1].cos(), a[:, 1].sin(), a[:, 2].cos(), a[:, 2].sin()
    m_x = torch.stack([one, zero, zero, zero, cx, -sx, zero, sx, cx], 1).view(-1, 3, 3)
    m_y = torch.stack([cy, zero, sy, zero, one, zero, -sy, zero, cy], 1).view(-1, 3, 3)
    m_z = torch.stack([cz, -sz, zero, sz, cz, zero, zero, zero, one], 1).view(-1, 3, 3)
    return m_z.matmul(m_y.matmul(m_x)), torch.cat([view[:, 3:5] * txy, view[:, 5:] * tz], 1)


def _centre(o, rcd):
    return o.t([0.0, 0.0, rcd])


def warp_verts(o, depth, rays, R, t, rcd):
    """renderer.py:64-80,90-95: R (d ray - c) + c + t.  depth [B,P], rays [P,3] -> [B,P,3]."""
    B, P = depth.shape
    x = rays[None] * depth[..., None] - _centre(o, rcd)
    m = o.bcast(R[:, None], (B, P, 3, 3)) * x[:, :, None, :]
    return (m[..., 0] + m[..., 1] + m[..., 2]) + _centre(o, rcd) + o.bcast(t[:, None], (B, P, 3))


def inv_warp_grid(o, depth, rays, R, t, K9, H, W, rcd):
    """renderer.py:82-88,97-114: R^T (d ray - t - c) + c, projected by K, normalised to [-1, 1].  -> [B,P,2]."""
    B, P = depth.shape
    z = rays[None] * depth[..., None] - o.bcast(t[:, None], (B, P, 3)) - _centre(o, rcd)
    m = o.bcast(R[:, None], (B, P, 3, 3)) * z[:, :, :, None]
    y = (m[..., 0, :] + m[..., 1, :] + m[..., 2, :]) + _centre(o, rcd)
    g = y / y[..., 2:]
    u = g[..., 0] * K9[0] + g[..., 1] * K9[1] + g[..., 2] * K9[2]
    v = g[..., 0] * K9[3] + g[..., 1] * K9[4] + g[..., 2] * K9[5]
    return torch.stack([u / (W - 1) * 2.0 - 1.0, v / (H - 1) * 2.0 - 1.0], -1)


def normal_from_depth(o, depth, rays, eps=1e-7):
    """renderer.py:127-139.  depth [B,H,W], rays [H*W,3] -> [B,H,W,3]; (0,0,1) on the border.  Returns the
    un-normalised interior normal too (for the conditioning check)."""
    B, H, W = depth.shape
    g = rays.view(1, H, W, 3) * depth[..., None]
    n = torch.zeros(B, H, W, 3, dtype=o.dt)
    n[..., 2] = 1.0
    raw = torch.zeros(B, 0, 0, 3, dtype=o.dt)
    if H > 2 and W > 2:
        tu = g[:, 1:-1, 2:] - g[:, 1:-1, :-2]
        tv = g[:, 2:, 1:-1] - g[:, :-2, 1:-1]
        raw = torch.linalg.cross(tu, tv, dim=3)
        n[:, 1:-1, 1:-1] = raw
    sq = n * n
    return n / (((sq[..., 0] + sq[..., 1]) + sq[..., 2]).sqrt()[..., None] + eps), raw


def shading(o, normal, light, albedo):
    """model.py:347-360.  normal [B,P,3], light [B,4], albedo [B,3,P] -> diffuse [B,P], texture [B,3,P], n.dir."""
    B, P, _ = normal.shape
    l = o.bcast(light[:, None], (B, P, 4))
    a, b = l[..., 0] / 2 + 0.5, l[..., 1] / 2 + 0.5
    d = torch.cat([l[..., 2:], torch.ones(B, P, 1, dtype=o.dt)], -1)
    sq = d * d
    d = d / ((sq[..., 0] + sq[..., 1]) + sq[..., 2]).sqrt()[..., None]
    dot = (normal[..., 0] * d[..., 0] + normal[..., 1] * d[..., 1]) + normal[..., 2] * d[..., 2]
    diffuse = torch.where(dot > 0, dot, torch.zeros_like(dot))
    sh = a + b * diffuse
    return diffuse, (albedo / 2 + 0.5) * sh[:, None] * 2 - 1, dot


def smooth_terms(p):
    dx, dy = p[:, :, 1:] - p[:, :, :-1], p[:, 1:] - p[:, :-1]
    return (dx[:, :, 1:] - dx[:, :, :-1], dx[:, 1:] - dx[:, :-1], dy[:, :, 1:] - dy[:, :, :-1], dy[:, 1:] - dy[:, :-1])


def smooth_loss(o, p):
    """losses.py:54-79 on a [N,H,W] map; an empty term contributes 0 (the reference: NaN)."""
    loss = torch.zeros((), dtype=o.dt)
    for t in smooth_terms(p):
        if t.numel():
            loss = loss + o.sum(t.abs()) / t.numel()
    return loss


def depth_head(o, raw, lo, hi, clamp_border, border_depth):
    """model.py:337-345 (+ :85-86).  raw [B,H,W] -> depth, and the centred map the gradient sum refers to."""
    W = raw.shape[-1]
    mean = o.sum(raw) / raw.numel()
    cen = raw - o.bcast(mean.view(1, 1, 1), raw.shape)
    t = torch.tanh(cen)
    d = (1 + t) / 2 * hi + (1 - t) / 2 * lo
    if clamp_border:
        border = torch.zeros(W, dtype=o.dt)
        border[:2] = 1.02
        border[W - 2:] = 1.02
        d = d * (1 - border) + border * border_depth
    return d, cen


def _lpips_normalize(o, f, eps):
    s = o.sum(f * f, (1,))
    pos = s > 0
    nrm = torch.where(pos, torch.where(pos, s, torch.ones_like(s)).sqrt(), torch.zeros_like(s))
    return f / (nrm[:, None] + eps), s


def lpips_layer(o, f0, f1, w, eps=1e-10):
    """networks_basic.py:64-92 for one layer, lpips/__init__.py:40-42.  f [N,C,HW], w [C] -> out [N]."""
    u, s0 = _lpips_normalize(o, f0, eps)
    v, s1 = _lpips_normalize(o, f1, eps)
    d = (u - v) ** 2 * w[None, :, None]
    return o.sum(o.sum(d, (1,)), (1,)) / f0.shape[2], s0, s1


def weighted_l1(o, x, y, w):
    """losses.py:40-51: numerator sum |x - y| * w.expand_as and denominator sum w.expand_as.  x [B,C,HW], w [B,HW]."""
    err = (x - y).abs()
    m = torch.ones_like(err) if w is None else w[:, None, :].expand_as(err)
    return o.sum(err * m), o.sum(m)


# ----------------------------------------------------------------------------- inputs
def pixel_rays(H, W, fov=10.0):
    """K^-1 (u, v, 1) for every pixel of an H x W image, (H*W, 3) fp32, and K (9 floats) — the table the
    kernels take as an input (renderer.py:35-46,61-72 for a non-square image: one focal length, centred)."""
    f = f32((max(H, W, 2) - 1) / 2 / math.tan(fov / 2 * math.pi / 180))
    cx, cy = f32((W - 1) / 2), f32((H - 1) / 2)
    v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    rays = np.stack([(u - cx) / f, (v - cy) / f, np.ones_like(u)], -1).reshape(-1, 3).astype(np.float32)
    return rays, (f, 0.0, cx, 0.0, f, cy, 0.0, 0.0, 1.0)


VIEW_SCALES = (f32(math.pi / 180 * 60), f32(0.1), f32(0.05))
RCD = 1.0


def _pose(rng, B):
    view = (rng.standard_normal((B, 6)) * 0.3).astype(np.float32)
    with torch.no_grad():
        R, t = view_transform(Ops(F64), torch.tensor(view, dtype=F64), *VIEW_SCALES)
    return R.numpy().astype(np.float32), t.numpy().astype(np.float32)


def _make_view(p, rng):
    B = p["B"]
    return dict(view=(rng.standard_normal((B, 6)) * 0.3).astype(np.float32),
                gR=rng.standard_normal((B, 3, 3)).astype(np.float32), gt=rng.standard_normal((B, 3)).astype(np.float32))


def _make_warp(p, rng):
    B, H, W = p["B"], p["H"], p["W"]
    rays, K9 = pixel_rays(H, W)
    R, t = _pose(rng, B)
    return dict(depth=(0.9 + 0.2 * rng.random((B, H * W))).astype(np.float32), rays=rays, R=R, t=t, K9=np.array(K9, np.float32),
                cot=rng.standard_normal((B, H * W, 2 if p.get("inv") else 3)).astype(np.float32))


def _make_normal(p, rng):
    B, H, W = p["B"], p["H"], p["W"]
    return dict(depth=(0.9 + 0.2 * rng.random((B, H, W))).astype(np.float32), rays=pixel_rays(H, W)[0],
                cot=rng.standard_normal((B, H, W, 3)).astype(np.float32))


def _make_shading(p, rng):
    B, Bn, Ba, P = p["B"], p["Bn"], p["Ba"], p["H"] * p["W"]
    n = rng.standard_normal((Bn, P, 3))
    return dict(normal=(n / np.linalg.norm(n, axis=2, keepdims=True)).astype(np.float32),
                light=(rng.standard_normal((B, 4)) * 0.5).astype(np.float32),
                albedo=np.tanh(rng.standard_normal((Ba, 3, P))).astype(np.float32),
                gt=rng.standard_normal((B, 3, P)).astype(np.float32), gd=rng.standard_normal((B, P)).astype(np.float32))


def _make_smooth(p, rng):
    N, H, W, kind = p["N"], p["H"], p["W"], p["kind"]
    y, x = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    if kind == "random":
        m = rng.random((N, H, W))
    elif kind == "grid":      # multiples of 2^-10 in [0, 1) with flat stretches (rows 2..4, columns 3..6): exact zeros
        m = rng.integers(0, 1024, (N, H, W)) / 1024.0
        m[:, 2:5] = m[:, 2:3]
        m[:, :, 3:7] = m[:, :, 3:4]
    else:                     # exact: only the term whose count is a power of two is non-zero
        a = rng.integers(0, 1024, (N, max(H, W))) / 1024.0
        a[:, 4:8] = a[:, 4:5]                               # a flat stretch: second difference exactly 0
        m = {"exact_x": a[:, None, :W] + 0 * y, "exact_y": a[:, :H, None] + 0 * x,
             "exact_xy": (rng.integers(1, 4, (N, 1, 1)) * (x * y)[None]) / 1024.0}[kind]
    return dict(p=m.astype(np.float32), gloss=np.array(0.75 if kind != "random" else 0.7, np.float32))


def _make_depth_head(p, rng):
    B, H, W = p["B"], p["H"], p["W"]
    return dict(raw=(rng.standard_normal((B, H, W)) * 0.8 + 0.3).astype(np.float32),
                cot=rng.standard_normal((B, H, W)).astype(np.float32))


def _make_lpips(p, rng):
    N, C, HW = p["N"], p["C"], p["HW"]
    f0, f1 = (np.maximum(rng.standard_normal((N, C, HW)), 0).astype(np.float32) for _ in range(2))
    if HW >= 4:                      # three kinds of zero-norm pixel in every image
        f0[:, :, HW // 3] = 0
        f1[:, :, HW // 2] = 0
        f0[:, :, HW - 1] = 0
        f1[:, :, HW - 1] = 0
    else:                            # one pixel: the kind is the case's
        if p["zero"] in ("f0", "both"):
            f0[:] = 0
        if p["zero"] in ("f1", "both"):
            f1[:] = 0
    w = (rng.random(C) + 0.1).astype(np.float32)
    w[C // 2] = 0
    return dict(f0=f0, f1=f1, w=w, gout=(rng.random(N) + 0.5).astype(np.float32),
                g_in=rng.standard_normal((N, C, HW)).astype(np.float32))


L1_GRID = dict(coef=0.25, g=0.75, den=64.0, add_scale=0.5, slope=0.25, gain=2.0)


def _make_l1(p, rng):
    B, C, HW, wk = p["B"], p["C"], p["HW"], p["w"]
    sh = (B, C, HW)
    if p["kind"] == "grid":
        x, y = rng.integers(-8, 9, sh) / 8.0, rng.integers(-8, 9, sh) / 8.0
        y = np.where(rng.random(sh) < 0.2, x, y)                       # exact ties
        w = {"none": None, "mask": rng.integers(0, 2, (B, HW)) * 1.0, "real": rng.integers(0, 3, (B, HW)) / 2.0}[wk]
        gadd, gadd2 = rng.integers(-64, 65, sh) / 64.0, rng.integers(-64, 65, sh) / 64.0
        sc = dict(L1_GRID)
    else:
        x, y = rng.standard_normal(sh), rng.standard_normal(sh)
        w = {"none": None, "real": rng.random((B, HW))}[wk]
        gadd, gadd2 = rng.standard_normal(sh), rng.standard_normal(sh)
        den = f32(C * float(np.float32(w).astype(np.float64).sum()) if w is not None else B * C * HW)
        sc = dict(coef=f32(0.37), g=f32(0.7), den=den, add_scale=f32(1 / math.sqrt(2)), slope=f32(0.2), gain=f32(math.sqrt(2)))
    gate_ref = rng.integers(-2, 3, sh) / 4.0                       # exact zeros, both signs
    gate_ref.flat[0] = 0.0
    out = dict(x=x, y=y, gadd=gadd, gadd2=gadd2, gate_ref=gate_ref)
    if w is not None:
        out["w"] = w
    return dict({k: v.astype(np.float32) for k, v in out.items()}, **{k: np.array(v, np.float32) for k, v in sc.items()})


# ----------------------------------------------------------------------------- reference runs: name -> tensor
def _ref_view(o, p, i):
    view = o.t(i["view"], True)
    R, t = view_transform(o, view, *VIEW_SCALES)
    (gview,) = _grads([R, t], [o.t(i["gR"]), o.t(i["gt"])], [view])
    return dict(R=R, t=t, gview=gview)


def _ref_warp(o, p, i):
    depth, R, t = o.t(i["depth"], True), o.t(i["R"], True), o.t(i["t"], True)
    rays = o.t(i["rays"])
    if p.get("inv"):
        y = inv_warp_grid(o, depth, rays, R, t, [float(k) for k in i["K9"]], p["H"], p["W"], RCD)
    else:
        y = warp_verts(o, depth, rays, R, t, RCD)
    gd, gR, gt = _grads([y], [o.t(i["cot"])], [depth, R, t])
    return {"out": y, "gdepth": gd, "gRt": torch.cat([gR.reshape(-1, 9), gt], 1)}


def _ref_normal(o, p, i):
    depth = o.t(i["depth"], True)
    n, raw = normal_from_depth(o, depth, o.t(i["rays"]))
    (gd,) = _grads([n], [o.t(i["cot"])], [depth])
    return dict(normal=n, gdepth=gd, _raw=raw)


def _ref_shading(o, p, i):
    B = p["B"]
    normal = o.t(np.broadcast_to(i["normal"], (B,) + i["normal"].shape[1:]), True)     # per-b gradients, as the kernel's
    albedo = o.t(np.broadcast_to(i["albedo"], (B,) + i["albedo"].shape[1:]), True)
    light = o.t(i["light"], True)
    dif, tex, dot = shading(o, normal, light, albedo)
    gn, gl, ga = _grads([tex, dif], [o.t(i["gt"]), o.t(i["gd"])], [normal, light, albedo])
    gn0, gl0, _ = _grads([tex], [o.t(i["gt"])], [normal, light, albedo])              # gdiffuse == NULL
    return dict(diffuse=dif, texture=tex, gnormal=gn, glight=gl, galbedo=ga, gnormal_nogd=gn0, glight_nogd=gl0, _dot=dot)


def _ref_smooth(o, p, i):
    m = o.t(i["p"], True)
    loss = smooth_loss(o, m)
    (gp,) = _grads([loss], [o.t(i["gloss"])], [m])
    return dict(loss=loss, gp=gp, _terms=smooth_terms(m))


HEAD = dict(lo=f32(0.9), hi=f32(1.1), bd=f32(0.7 * 1.1 + 0.3 * 0.9))


def _ref_depth_head(o, p, i):
    raw = o.t(i["raw"], True)
    d, cen = depth_head(o, raw, HEAD["lo"], HEAD["hi"], p["border"], HEAD["bd"])
    (g_raw,) = _grads([d], [o.t(i["cot"])], [raw])
    (gc,) = _grads([d], [o.t(i["cot"])], [cen])
    return dict(out=d, g_raw=g_raw, gsum=o.sum(gc), _mean=(raw.detach().sum() / raw.numel()))


def _ref_lpips(o, p, i):
    f0, f1, w = o.t(i["f0"], True), o.t(i["f1"]), o.t(i["w"])
    out, s0, s1 = lpips_layer(o, f0, f1, w, eps=f32(1e-10))
    (g,) = _grads([out], [o.t(i["gout"])], [f0])
    gate = (f0 > 0).to(o.dt)
    gin = o.t(i["g_in"])
    return dict(out=out, g_plain=g, g_gate=g * gate, g_in=g + gin, g_in_gate=(g + gin) * gate, _s0=s0, _s1=s1)


L1_COMBOS = [(xo, na) for xo in (1, 0) for na in (0, 1, 2) if xo or na]     # (x given, number of gadd tensors)


def _ref_l1(o, p, i):
    x, y = o.t(i["x"], True), o.t(i["y"])
    w = o.t(i["w"]) if "w" in i else None
    num, den = weighted_l1(o, x, y, w)
    (gnum,) = _grads([num], [torch.ones((), dtype=o.dt)], [x])
    s = {k: o.t(i[k]) for k in ("coef", "g", "den", "add_scale", "slope", "gain")}
    k = s["g"] / s["den"]
    gadd, gadd2, gate_ref = o.t(i["gadd"]), o.t(i["gadd2"]), o.t(i["gate_ref"])
    out = dict(num=num, den2=den, g_bwd=gnum * s["coef"], g_bwd2=gnum * k, g_bwd2_add=gadd + gnum * k,
               _diff=(x - y).detach())
    for xo, na in L1_COMBOS:
        r = gnum * k if xo else torch.zeros_like(gnum)
        if na:
            r = (gadd + gadd2 if na == 2 else gadd) * s["add_scale"] + r
        out[f"g3_x{xo}a{na}"] = r
        out[f"g3gate_x{xo}a{na}"] = r * s["gain"] * torch.where(gate_ref > 0, torch.ones_like(r), s["slope"] * torch.ones_like(r))
    return out


MAKE = dict(view=_make_view, warp=_make_warp, normal=_make_normal, shading=_make_shading, smooth=_make_smooth,
            depth_head=_make_depth_head, lpips=_make_lpips, l1=_make_l1)
REF = dict(view=_ref_view, warp=_ref_warp, normal=_ref_normal, shading=_ref_shading, smooth=_ref_smooth,
           depth_head=_ref_depth_head, lpips=_ref_lpips, l1=_ref_l1)


# ----------------------------------------------------------------------------- the table
class Case:
    """One row: an operation, its shape parameters and the seeds it may take.  `exact`: the outputs that
    must equal float64 bit for bit (exact-grid inputs); every other output is held to the bound."""

    def __init__(self, name, op, exact=(), seeds=SEEDS, **p):
        self.name, self.op, self.p, self.exact, self.seeds = name, op, p, tuple(exact), tuple(seeds)
        self._data = None

    def __repr__(self):
        return self.name

    def inputs(self, seed):
        return MAKE[self.op](self.p, np.random.default_rng([seed, zlib.crc32(self.name.encode())]))

    def conditioned(self, r64):
        """Every element away from every kink, on the float64 restatement; (ok, what was measured)."""
        if self.op == "shading":
            dot = r64["_dot"].detach()
            neg = float((dot < 0).double().mean())
            return bool(dot.abs().min() >= KINK["shading_dot"] and 0.2 <= neg <= 0.8), dict(min_dot=float(dot.abs().min()), negative=neg)
        if self.op == "normal":
            n = r64["_raw"].detach().norm(dim=3)
            if n.numel() == 0:
                return True, dict(interior=0)
            return bool(n.min() >= KINK["normal_rel"] * n.max()), dict(min_rel=float(n.min() / n.max()))
        if self.op == "smooth" and self.p["kind"] == "random":
            lo = min([float(t.detach().abs().min()) for t in r64["_terms"] if t.numel()] or [1.0])
            return lo >= KINK["diff"], dict(min_second_difference=lo)
        if self.op == "l1" and self.p["kind"] == "random":
            lo = float(r64["_diff"].abs().min())
            return lo >= KINK["diff"], dict(min_diff=lo)
        return True, {}

    def split(self, inp, outs):
        """LPIPS gradients: the pixels whose f0 norm is 0 carry values of the order 1 / eps and are an output
        tensor of their own (`name@z0`), so that their scale does not hide an error anywhere else."""
        if self.op != "lpips":
            return outs
        z0 = torch.as_tensor((inp["f0"].astype(np.float64) ** 2).sum(1) == 0)[:, None, :]
        res = {}
        for k, v in outs.items():
            if k.startswith("g_"):
                z = z0.to(v.device).expand_as(v)
                res[k], res[k + "@z0"] = torch.where(z, torch.zeros_like(v), v), torch.where(z, v, torch.zeros_like(v))
            else:
                res[k] = v
        return res

    def data(self):
        """inputs (np, fp32), seed, ref64 / ref32 (name -> np array), and per compared output e32, scale, bound."""
        if self._data is None:
            for seed in self.seeds:
                inp = self.inputs(seed)
                r64 = REF[self.op](Ops(F64), self.p, inp)
                ok, info = self.conditioned(r64)
                if ok:
                    break
            else:
                raise AssertionError(f"{self.name}: no seed of {self.seeds} keeps the case away from its kinks ({info})")
            r32 = REF[self.op](Ops(F32), self.p, inp)
            diag = {k: (tuple(t.detach() for t in v) if isinstance(v, tuple) else v.detach()) for k, v in r64.items() if k.startswith("_")}
            r64 = {k: v.detach().numpy() for k, v in self.split(inp, r64).items() if not k.startswith("_")}
            r32 = {k: v.detach().numpy() for k, v in self.split(inp, r32).items() if not k.startswith("_")}
            stats = {}
            for k in r64:
                e32 = float(np.abs(r32[k].astype(np.float64) - r64[k]).max()) if r64[k].size else 0.0
                scale = float(np.abs(r64[k]).max()) if r64[k].size else 0.0
                stats[k] = dict(e32=e32, scale=scale, bound=4 * e32 + 5e-6 * scale)
            for a in list(inp.values()) + list(r64.values()) + list(r32.values()):
                a.setflags(write=False)
            self._data = dict(inp=inp, seed=seed, info=info, ref64=r64, ref32=r32, stats=stats, diag=diag)
        return self._data


P_SHAPES = [(3, 85), (16, 16), (257, 1), (9, 33)]            # P = 255, 256, 257, 297
INV_SHAPES = [(3, 85), (16, 16), (9, 33), (2, 129)]          # H, W > 1; P = 255, 256, 297, 258
PATCH_SHAPES = [(3, 3), (8, 32), (9, 33), (17, 70)]
NORMAL_BORDER = [(1, 40), (40, 1), (2, 5)]                   # all border: (0, 0, 1), zero gradient
SMOOTH_EMPTY = [(1, 40), (2, 2), (2, 40), (40, 2)]           # empty terms


def _table():
    c = [Case(f"view_B{B}", "view", B=B) for B in (1, 64, 65)]
    for B in (1, 3):
        c += [Case(f"warp_{H}x{W}_B{B}", "warp", B=B, H=H, W=W) for H, W in P_SHAPES]
        c += [Case(f"invwarp_{H}x{W}_B{B}", "warp", B=B, H=H, W=W, inv=True) for H, W in INV_SHAPES]
        c += [Case(f"normal_{H}x{W}_B{B}", "normal", B=B, H=H, W=W) for H, W in PATCH_SHAPES + NORMAL_BORDER]
        c += [Case(f"smooth_{H}x{W}_N{B}", "smooth", N=B, H=H, W=W, kind="random") for H, W in PATCH_SHAPES + SMOOTH_EMPTY]
    c += [Case(f"smoothgrid_{H}x{W}_N{N}", "smooth", N=N, H=H, W=W, kind="grid") for H, W, N in ((3, 3, 1), (9, 33, 3), (17, 70, 1))]
    # exact: p depends on x only with N H (W-2) = 256 or 512; on y only; bilinear with N (H-1)(W-1) = 256 or 512
    for N in (1, 2):
        c += [Case(f"smoothexact_x_N{N}", "smooth", exact=("loss",), N=N, H=8, W=34, kind="exact_x"),
              Case(f"smoothexact_y_N{N}", "smooth", exact=("loss",), N=N, H=34, W=8, kind="exact_y"),
              Case(f"smoothexact_xy_N{N}", "smooth", exact=("loss",), N=N, H=9, W=33, kind="exact_xy")]
    c += [Case(f"shading_{H}x{W}_B3", "shading", B=3, Bn=3, Ba=3, H=H, W=W) for H, W in P_SHAPES]
    c += [Case(f"shading_9x33_B{B}n{Bn}a{Ba}", "shading", B=B, Bn=Bn, Ba=Ba, H=9, W=33) for B, Bn, Ba in ((3, 1, 1), (3, 1, 3), (1, 1, 1))]
    c += [Case("shading_257x1_B1", "shading", B=1, Bn=1, Ba=1, H=257, W=1)]
    for border in (1, 0):
        c += [Case(f"head_{B}x{H}x{W}_border{border}", "depth_head", B=B, H=H, W=W, border=border)
              for B, H, W in ((2, 3, 4), (2, 3, 5), (3, 32, 32))]
    c += [Case("head_1x1026x256_border1", "depth_head", B=1, H=1026, W=256, border=1)]     # 1027 workgroups > the 1024 cap
    c += [Case(f"lpips_1x5x1_{z}", "lpips", N=1, C=5, HW=1, zero=z) for z in ("none", "f0", "f1", "both")]
    c += [Case(f"lpips_{N}x{C}x{HW}", "lpips", N=N, C=C, HW=HW)
          for N, C, HW in ((2, 3, 64), (2, 64, 63), (3, 17, 65), (1, 64, 1024), (2, 8, 1025), (1, 64, 1088))]
    for B, C, HW in ((1, 1, 4), (2, 3, 4), (3, 2, 1028), (4, 6, 384)):
        ex = ("num", "den2", "g_bwd", "g_bwd2", "g_bwd2_add") + tuple(f"g3{g}_x{xo}a{na}" for g in ("", "gate") for xo, na in L1_COMBOS)
        c += [Case(f"l1grid_{B}x{C}x{HW}_{w}", "l1", exact=ex, B=B, C=C, HW=HW, w=w, kind="grid") for w in ("none", "mask", "real")]
        c += [Case(f"l1rand_{B}x{C}x{HW}_{w}", "l1", B=B, C=C, HW=HW, w=w, kind="random") for w in ("none", "real")]
    return c


CASES = _table()
CASE = {c.name: c for c in CASES}
assert len(CASE) == len(CASES)


def by_op(op):
    return [c for c in CASES if c.op == op]


# ----------------------------------------------------------------------------- the large L1 case
# (2, 9, 1024 * 1024), generated from index arithmetic (on the device by the GPU test, on one period here):
# with q = p & 4095,
#   w[b, p]      = 1 where ((5 q + (q >> 3) + b) & 3) == 0, else 0                      (about 25 % ones)
#   d[b, c, p]   = ((q >> 1) + 3 (q >> 5) + c + b) & 1                                  (|x - y| = 0.25 d)
#   x[b, c, p]   = 0.25 ((q + c) % 5 - 2),   y = x - 0.25 d (1 - 2 ((q >> 4) & 1))      (both signs, ties)
# Every term is 0 or one quarter, so the sum is exact while it stays below 2^24 quarter-units.
LARGE = dict(B=2, C=9, HW=1024 * 1024, period=4096, coef=0.5)
# launch geometry of csrc/losses.hip restated: total4 = B C HW / 4 float4 per tensor, 256 threads x 4 float4
# per workgroup before the cap (g2s_weighted_l1_fwd / _fwd2: min(.., 2048); _bwd / _bwd2 / _bwd3: min(.., 4096))
WL1_FLOAT4_PER_WORKGROUP, WL1_FWD_CAP, WL1_BWD_CAP = 256 * 4, 2048, 4096


def large_l1(xp, B, C, n, offset=0):
    """w (B, n), x, y (B, C, n) of the large case for pixels offset .. offset + n - 1, as integer quarter-units
    for x and y; `xp` is numpy or torch (int64 index arithmetic either way)."""
    if xp is np:
        p = np.arange(offset, offset + n, dtype=np.int64)
        b, c = np.arange(B, dtype=np.int64)[:, None, None], np.arange(C, dtype=np.int64)[None, :, None]
    else:
        p = torch.arange(offset, offset + n, dtype=torch.int64, device="cuda")
        b, c = (torch.arange(k, dtype=torch.int64, device="cuda") for k in (B, C))
        b, c = b[:, None, None], c[None, :, None]
    q = (p & 4095)[None, None, :]
    w = (((5 * q + (q >> 3) + b) & 3) == 0)[:, 0, :]
    d = ((q >> 1) + 3 * (q >> 5) + c + b) & 1
    x4 = (q + c) % 5 - 2 + 0 * b
    y4 = x4 - d * (1 - 2 * ((q >> 4) & 1))
    return w, x4, y4
