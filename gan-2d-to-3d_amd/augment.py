"""Adaptive discriminator augmentation (ADA): the geometric and colour pipeline of
stylegan2-pytorch/non_leaking.py (`augment`, `random_apply_affine`, `random_apply_color`, `sample_affine`,
`sample_color`, `get_padding`, `AdaptiveAugment`, the SYM6 filter) on libg2s.so (csrc/ada.hip).

A CUDA float32 image goes through two launches forward (g2s_ada_up2: reflect padding + 2x SYM6 upsampling;
g2s_ada_warp_down: affine warp at double resolution + 2x SYM6 downsampling + colour matrix) and two backward, as ONE
autograd node.  G and C get no gradient, as in the reference.

`order=1` (the default): the node's backward is once_differentiable — a double backward raises — and with
g2s_set_deterministic on it raises too (float-atomic scatter).  `order=2`: given its matrices the augmentation is affine
in the image, y = L x + c, so its gradient L^T and the gradient of that, L, are the same kernels again: `_AdaFwd` and
`_AdaAdj` are each other's backward and the result differentiates to any order (R1 through the augmentation).
`_AdaAdj` takes the scatter while deterministic mode is off and the fixed-order gather
(g2s_ada_warp_down_bwd_gather) while it is on.

The matrices are sampled on the CPU from torch's global CPU generator, as the reference does, in the same order and
with the same float32 arithmetic: equal seeds give equal G and C.  The pads and the matrix handed to the warp are
derived on the host from the CPU matrices.

A CPU tensor (any float dtype) takes `_augment_torch`, a torch composition of the same arithmetic; the tests use it
as the statement of what the kernels compute.
"""
import math

import torch
import torch.nn.functional as F
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import lib as _lib

# sym6 (PyWavelets), the low-pass the ADA paper uses for up- and downsampling
SYM6 = (
    0.015404109327027373, 0.0034907120842174702, -0.11799011114819057, -0.048311742585633,
    0.4910559419267466, 0.787641141030194, 0.3379294217276218, -0.07263752278646252,
    -0.021060292512300564, 0.04472490177066578, 0.0017677118642428036, -0.007800708325034148,
)
_TAPS = len(SYM6)
_PAD_K = _TAPS // 4          # the margin, in pixels, the warp keeps around the image for the filter


# ------------------------------------------------------------------------------------------ adaptive p
def _reduce_sum(t):
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() == 1:
        return t
    t = t.clone()
    dist.all_reduce(t, op=dist.ReduceOp.SUM)
    return t


class AdaptiveAugment:
    """p follows the sign statistic of the discriminator's output on real images: every `update_every` calls of
    tune(), r_t = sum(sign(real_pred)) / n over the calls since the last update (summed across ranks when
    torch.distributed is initialised) moves p by n / length towards more (r_t > target) or less augmentation."""

    def __init__(self, ada_aug_target, ada_aug_len, update_every, device):
        self.ada_aug_target = ada_aug_target
        self.ada_aug_len = ada_aug_len
        self.update_every = update_every
        self.ada_update = 0
        self.ada_aug_buf = torch.tensor([0.0, 0.0], device=device)
        self.r_t_stat = 0
        self.ada_aug_p = 0

    @torch.no_grad()
    def tune(self, real_pred):
        seen = (torch.sign(real_pred).sum().item(), real_pred.shape[0])
        self.ada_aug_buf += torch.tensor(seen, device=real_pred.device)
        self.ada_update += 1
        if self.ada_update % self.update_every == 0:
            self.ada_aug_buf = _reduce_sum(self.ada_aug_buf)
            signs, n = self.ada_aug_buf.tolist()
            self.r_t_stat = signs / n
            step = n / self.ada_aug_len
            self.ada_aug_p += step if self.r_t_stat > self.ada_aug_target else -step
            self.ada_aug_p = min(1, max(0, self.ada_aug_p))
            self.ada_aug_buf.mul_(0)
            self.ada_update = 0
        return self.ada_aug_p


# ------------------------------------------------------------------------------------------ sampling
def _eye(n, batch):
    return torch.eye(n).unsqueeze(0).repeat(batch, 1, 1)


def _translate2(tx, ty):
    m = _eye(3, tx.shape[0])
    m[:, :2, 2] = torch.stack((tx, ty), 1)
    return m


def _rotate2(theta):
    m = _eye(3, theta.shape[0])
    s, c = torch.sin(theta), torch.cos(theta)
    m[:, :2, :2] = torch.stack((c, -s, s, c), 1).view(-1, 2, 2)
    return m


def _scale2(sx, sy):
    m = _eye(3, sx.shape[0])
    m[:, 0, 0] = sx
    m[:, 1, 1] = sy
    return m


def _choice(size, values):
    return torch.tensor(values)[torch.randint(high=len(values), size=(size,))]


def _uniform(shape, lo, hi):
    return torch.empty(shape).uniform_(lo, hi)


def _normal(shape, std):
    return torch.empty(shape).normal_(0, std)


def _lognormal(shape, std):
    return torch.empty(shape).log_normal_(mean=0, std=std)


def _apply_with_probability(p, transform, prev):
    """Each sample takes `transform` with probability p (else the identity), composed onto `prev`."""
    n, side = transform.shape[0], transform.shape[-1]
    take = torch.empty(n).bernoulli_(p).view(n, 1, 1)
    return (take * transform + (1 - take) * _eye(side, n)) @ prev


def sample_affine(p, size, height, width, device="cpu"):
    """[size, 3, 3]: the ADA geometric transform in pixel units — x-flip, 90-degree rotation, integer translation,
    isotropic scale, rotation, anisotropic scale, rotation, fractional translation, each with probability p (the two
    free rotations with 1 - sqrt(1 - p), so that either occurs with p).  Drawn on the CPU."""
    G = _eye(3, size)
    G = _apply_with_probability(p, _scale2(1 - 2.0 * _choice(size, (0, 1)), torch.ones(size)), G)
    G = _apply_with_probability(p, _rotate2(-math.pi / 2 * _choice(size, (0, 3))), G)
    t = _uniform((2, size), -0.125, 0.125)
    G = _apply_with_probability(p, _translate2(torch.round(t[1] * width), torch.round(t[0] * height)), G)
    s = _lognormal(size, 0.2 * math.log(2))
    G = _apply_with_probability(p, _scale2(s, s), G)
    p_rot = 1 - math.sqrt(1 - p)
    G = _apply_with_probability(p_rot, _rotate2(-_uniform(size, -math.pi, math.pi)), G)
    s = _lognormal(size, 0.2 * math.log(2))
    G = _apply_with_probability(p, _scale2(s, 1 / s), G)
    G = _apply_with_probability(p_rot, _rotate2(-_uniform(size, -math.pi, math.pi)), G)
    t = _normal((2, size), 0.125)
    G = _apply_with_probability(p, _translate2(t[1] * width, t[0] * height), G)
    return G.to(device)


def sample_color(p, size):
    """[size, 4, 4]: brightness, contrast, luma flip, hue rotation and saturation, each with probability p, as one
    homogeneous matrix on (r, g, b, 1).  Drawn on the CPU."""
    C = _eye(4, size)
    v = torch.tensor((1 / math.sqrt(3),) * 3)           # the luma axis
    v4 = torch.cat((v, torch.zeros(1)))
    vv4 = torch.ger(v4, v4)

    b = _normal(size, 0.2)
    m = _eye(4, size)
    m[:, :3, 3] = torch.stack((b, b, b), 1)
    C = _apply_with_probability(p, m, C)

    s = _lognormal(size, 0.5 * math.log(2))
    m = _eye(4, size)
    m[:, 0, 0] = s
    m[:, 1, 1] = s
    m[:, 2, 2] = s
    C = _apply_with_probability(p, m, C)

    i = _choice(size, (0, 1))
    C = _apply_with_probability(p, _eye(4, size) - 2 * vv4 * i.view(-1, 1, 1), C)

    theta = _uniform(size, -math.pi, math.pi)
    a = v[0].item()
    cross = torch.tensor([(0, -a, a), (a, 0, -a), (-a, a, 0)]).unsqueeze(0)
    outer = (v.unsqueeze(1) * v).unsqueeze(0)
    sin_t, cos_t = torch.sin(theta).view(-1, 1, 1), torch.cos(theta).view(-1, 1, 1)
    m = _eye(4, size)
    m[:, :3, :3] = cos_t * torch.eye(3).unsqueeze(0) + sin_t * cross + (1 - cos_t) * outer
    C = _apply_with_probability(p, m, C)

    s = _lognormal(size, 1 * math.log(2))
    C = _apply_with_probability(p, vv4 + (_eye(4, size) - vv4) * s.view(-1, 1, 1), C)
    return C


# ------------------------------------------------------------------------------------------ host-side geometry
def _pads(G, height, width, kernel_size):
    """Reflect padding (x0, x1, y0, y1), as python ints, that the warp by G [B, 3, 3] (CPU, float32) can reach:
    the image's corners under G, plus the filter margin, at most size - 1, the maximum over the batch."""
    cx, cy = (width - 1) / 2, (height - 1) / 2
    corners = torch.tensor([(-cx, -cy, 1), (cx, -cy, 1), (cx, cy, 1), (-cx, cy, 1)])
    moved = (G @ corners.T)[:, :2, :].permute(1, 0, 2).flatten(1)          # [2, B * 4]: x row, y row
    reach = torch.cat((-moved, moved)).max(1).values                         # -x, -y, +x, +y
    margin = (kernel_size // 4) * 2
    reach = reach + torch.tensor([margin - cx, margin - cy] * 2)
    reach = reach.max(torch.tensor([0, 0] * 2)).min(torch.tensor([width - 1, height - 1] * 2))
    x0, y0, x1, y1 = (int(v) for v in reach.ceil().to(torch.int32))
    return x0, x1, y0, y1


def get_padding(G, height, width, kernel_size):
    """(pad_x1, pad_x2, pad_y1, pad_y2) as int32 scalars: see _pads."""
    return tuple(torch.tensor(v, dtype=torch.int32) for v in _pads(G.detach().float().cpu(), height, width, kernel_size))


def _t3(rows):
    return torch.tensor(rows, dtype=torch.float32)


def _scale1(sx, sy):
    return _t3(((sx, 0, 0), (0, sy, 0), (0, 0, 1)))


def _translate1(tx, ty):
    return _t3(((1, 0, tx), (0, 1, ty), (0, 0, 1)))


def _warp_matrix(G, pads, height, width):
    """[B, 2, 3] float32 (CPU): G, in pixels of the image about its centre, restated for
    affine_grid / grid_sample(align_corners=False) from the 2(H+6) x 2(W+6) output onto the padded 2x image —
    re-centred for unequal pads, scaled to the double resolution, shifted by the half pixel of its sample positions,
    then normalised by the two sizes.  float32 throughout, in this order: the reference's rounding."""
    x0, x1, y0, y1 = pads
    m = _translate1((x0 - x1) / 2, (y0 - y1) / 2) @ G
    m = _scale1(2, 2) @ m @ _scale1(1 / 2, 1 / 2)
    m = _translate1(-0.5, -0.5) @ m @ _translate1(0.5, 0.5)
    w2, h2 = 2 * (width + x0 + x1), 2 * (height + y0 + y1)
    ws, hs = 2 * (width + 2 * _PAD_K), 2 * (height + 2 * _PAD_K)
    m = _scale1(2 / w2, 2 / h2) @ m @ _scale1(1 / (2 / ws), 1 / (2 / hs))
    return m[:, :2, :].contiguous()


# ------------------------------------------------------------------------------------------ the two routes
def _augment_torch(img, warp, pads, cmat):
    """The arithmetic of the two kernels in torch ops, in img's dtype.  warp [B, 2, 3], cmat [B, 3, 4] or None."""
    B, C, H, W = img.shape
    x0, x1, y0, y1 = pads
    k = torch.tensor(SYM6).to(img)     # the taps are float32 values in every dtype, as in the reference and the kernels
    x = F.pad(img, (x0, x1, y0, y1), mode="reflect").reshape(B * C, 1, H + y0 + y1, W + x0 + x1)
    # 2x up: zero insertion, pad (6, 5), convolution with k — per axis
    up = x.new_zeros(B * C, 1, x.shape[2], 2 * x.shape[3])
    up[..., ::2] = x
    x = F.conv2d(F.pad(up, (_TAPS // 2, _TAPS // 2 - 1)), k.flip(0).view(1, 1, 1, -1))
    up = x.new_zeros(B * C, 1, 2 * x.shape[2], x.shape[3])
    up[..., ::2, :] = x
    x = F.conv2d(F.pad(up, (0, 0, _TAPS // 2, _TAPS // 2 - 1)), k.flip(0).view(1, 1, -1, 1))
    x = x.view(B, C, x.shape[2], x.shape[3])
    hs, ws = 2 * (H + 2 * _PAD_K), 2 * (W + 2 * _PAD_K)
    grid = F.affine_grid(warp.to(x), (B, C, hs, ws), align_corners=False)
    a = F.grid_sample(x, grid, mode="bilinear", padding_mode="zeros", align_corners=False)
    # 2x down: correlation with k from position 1, every second sample — per axis
    a = a.reshape(B * C, 1, hs, ws)[..., 1:-1, 1:-1]
    a = F.conv2d(a, k.view(1, 1, 1, -1), stride=(1, 2))
    a = F.conv2d(a, k.view(1, 1, -1, 1), stride=(2, 1))
    y = a.view(B, C, H, W)
    if cmat is not None:
        cmat = cmat.to(y)
        y = torch.einsum("bij,bjhw->bihw", cmat[:, :, :3], y) + cmat[:, :, 3].view(B, 3, 1, 1)
    return y


class _AdaFused(Function):
    """img -> colour(down2(warp(up2(reflect_pad(img))))): two launches each way (csrc/ada.hip)."""

    @staticmethod
    def forward(ctx, img, warp, cmat, pads):
        img = img.contiguous()
        B, C, H, W = img.shape
        x0, x1, y0, y1 = pads
        H2, W2 = 2 * (H + y0 + y1), 2 * (W + x0 + x1)
        L = _lib.load()
        x2 = torch.empty((B, C, H2, W2), dtype=torch.float32, device=img.device)
        _lib.check(L.g2s_ada_up2(_lib.ptr(img), _lib.ptr(x2), B, C, H, W, x0, x1, y0, y1, _lib.stream()))
        y = torch.empty_like(img)
        _lib.check(L.g2s_ada_warp_down(_lib.ptr(x2), _lib.ptr(warp), _lib.ptr(cmat), _lib.ptr(y), B, C, H, W, H2, W2,
                                       _lib.stream()))
        ctx.dims = (B, C, H, W, H2, W2)
        ctx.pads = pads
        ctx.save_for_backward(warp, cmat)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        warp, cmat = ctx.saved_tensors
        B, C, H, W, H2, W2 = ctx.dims
        L = _lib.load()
        gy = gy.contiguous()
        gx2 = torch.empty((B, C, H2, W2), dtype=torch.float32, device=gy.device)
        _lib.check(L.g2s_ada_warp_down_bwd(_lib.ptr(gy), _lib.ptr(warp), _lib.ptr(cmat), _lib.ptr(gx2), B, C, H, W,
                                           H2, W2, 0, _lib.stream()))
        gx = torch.empty_like(gy)
        _lib.check(L.g2s_ada_up2_bwd(_lib.ptr(gx2), _lib.ptr(gx), B, C, H, W, *ctx.pads, _lib.stream()))
        return gx, None, None, None


def _bilinear_zeros(x, grid):
    """F.grid_sample(x, grid, 'bilinear', 'zeros', align_corners=False) from gathers: torch's grid_sampler has no
    derivative of its backward, a gather's backward (scatter_add) has one, and the sample is linear in x."""
    B, C, H, W = x.shape
    ix = ((grid[..., 0] + 1) * W - 1) / 2
    iy = ((grid[..., 1] + 1) * H - 1) / 2
    x0, y0 = ix.floor(), iy.floor()
    flat = x.reshape(B, C, H * W)
    out = 0
    for dy in (0, 1):
        for dx in (0, 1):
            cx, cy = x0 + dx, y0 + dy
            wgt = (1 - (ix - cx).abs()) * (1 - (iy - cy).abs())
            inside = (cx >= 0) & (cx <= W - 1) & (cy >= 0) & (cy <= H - 1)
            at = (cy.clamp(0, H - 1) * W + cx.clamp(0, W - 1)).long().reshape(B, 1, -1).expand(B, C, -1)
            out = out + flat.gather(2, at) * (wgt * inside).reshape(B, 1, -1)
    return out.reshape(B, C, *grid.shape[1:3])


def _augment_twice(img, warp, pads, cmat):
    """_augment_torch's arithmetic, step for step, with `_bilinear_zeros` for its grid_sample: differentiable twice
    in img.  The order=2 route of CPU tensors and of dtypes the kernels do not take."""
    B, C, H, W = img.shape
    x0, x1, y0, y1 = pads
    k = torch.tensor(SYM6).to(img)
    x = F.pad(img, (x0, x1, y0, y1), mode="reflect").reshape(B * C, 1, H + y0 + y1, W + x0 + x1)
    up = torch.stack((x, torch.zeros_like(x)), -1).flatten(-2)                       # zero insertion along x
    x = F.conv2d(F.pad(up, (_TAPS // 2, _TAPS // 2 - 1)), k.flip(0).view(1, 1, 1, -1))
    up = torch.stack((x, torch.zeros_like(x)), -2).flatten(-3, -2)                   # along y
    x = F.conv2d(F.pad(up, (0, 0, _TAPS // 2, _TAPS // 2 - 1)), k.flip(0).view(1, 1, -1, 1))
    x = x.view(B, C, x.shape[2], x.shape[3])
    hs, ws = 2 * (H + 2 * _PAD_K), 2 * (W + 2 * _PAD_K)
    grid = F.affine_grid(warp.to(x), (B, C, hs, ws), align_corners=False)
    a = _bilinear_zeros(x, grid)
    a = a.reshape(B * C, 1, hs, ws)[..., 1:-1, 1:-1]
    a = F.conv2d(a, k.view(1, 1, 1, -1), stride=(1, 2))
    a = F.conv2d(a, k.view(1, 1, -1, 1), stride=(2, 1))
    y = a.view(B, C, H, W)
    if cmat is not None:
        cmat = cmat.to(y)
        y = torch.einsum("bij,bjhw->bihw", cmat[:, :, :3], y) + cmat[:, :, 3].view(B, 3, 1, 1)
    return y


class _AdaFwd(Function):
    """_AdaFused's forward as one half of a pair that differentiates to any order.  Given its matrices the map is
    affine in the image, y = L img + c (c: the colour offset): its gradient is _AdaAdj, L^T."""

    @staticmethod
    def forward(ctx, img, warp, cmat, pads):
        img = img.contiguous()
        B, C, H, W = img.shape
        x0, x1, y0, y1 = pads
        H2, W2 = 2 * (H + y0 + y1), 2 * (W + x0 + x1)
        L = _lib.load()
        x2 = torch.empty((B, C, H2, W2), dtype=torch.float32, device=img.device)
        _lib.check(L.g2s_ada_up2(_lib.ptr(img), _lib.ptr(x2), B, C, H, W, x0, x1, y0, y1, _lib.stream()))
        y = torch.empty_like(img)
        _lib.check(L.g2s_ada_warp_down(_lib.ptr(x2), _lib.ptr(warp), _lib.ptr(cmat), _lib.ptr(y), B, C, H, W, H2, W2,
                                       _lib.stream()))
        ctx.pads = pads
        ctx.save_for_backward(warp, cmat)
        return y

    @staticmethod
    def backward(ctx, gy):
        warp, cmat = ctx.saved_tensors
        return _AdaAdj.apply(gy, warp, cmat, ctx.pads), None, None, None


class _AdaAdj(Function):
    """gy -> L^T gy: the warp adjoint and g2s_ada_up2_bwd.  The warp adjoint is the float-atomic scatter while
    deterministic mode is off (the bits of _AdaFused's backward) and the fixed-order gather while it is on; the mode
    is read when the node runs.  Its gradient is L: _AdaFwd without the colour offset."""

    @staticmethod
    def forward(ctx, gy, warp, cmat, pads):
        gy = gy.contiguous()
        B, C, H, W = gy.shape
        x0, x1, y0, y1 = pads
        H2, W2 = 2 * (H + y0 + y1), 2 * (W + x0 + x1)
        L = _lib.load()
        gx2 = torch.empty((B, C, H2, W2), dtype=torch.float32, device=gy.device)
        if L.g2s_get_deterministic():
            ga = torch.empty((B, C, 2 * (H + 2 * _PAD_K), 2 * (W + 2 * _PAD_K)), dtype=torch.float32, device=gy.device)
            _lib.check(L.g2s_ada_warp_down_bwd_gather(_lib.ptr(gy), _lib.ptr(warp), _lib.ptr(cmat), _lib.ptr(gx2),
                                                      _lib.ptr(ga), B, C, H, W, H2, W2, _lib.stream()))
        else:
            _lib.check(L.g2s_ada_warp_down_bwd(_lib.ptr(gy), _lib.ptr(warp), _lib.ptr(cmat), _lib.ptr(gx2), B, C, H, W,
                                               H2, W2, 0, _lib.stream()))
        gx = torch.empty_like(gy)
        _lib.check(L.g2s_ada_up2_bwd(_lib.ptr(gx2), _lib.ptr(gx), B, C, H, W, x0, x1, y0, y1, _lib.stream()))
        ctx.pads = pads
        ctx.save_for_backward(warp, cmat)
        return gx

    @staticmethod
    def backward(ctx, ggx):
        warp, cmat = ctx.saved_tensors
        if cmat is not None:
            cmat = cmat.clone()
            cmat[:, :, 3] = 0          # the linear part: the offset does not depend on the image
        return _AdaFwd.apply(ggx, warp, cmat, ctx.pads), None, None, None


def _apply(img, G, C, order=1):
    """The pipeline for given CPU matrices G [B, 3, 3] and C [B, 4, 4] or None."""
    if order not in (1, 2):
        raise ValueError(f"order is 1 (once differentiable) or 2 (differentiable to any order), got {order!r}")
    if img.dim() != 4 or img.shape[0] != G.shape[0]:
        raise ValueError(f"img [B, C, H, W] and G [B, 3, 3] must agree in B (got {tuple(img.shape)}, {tuple(G.shape)})")
    if C is not None and img.shape[1] != 3:
        raise ValueError(f"the colour transform needs 3 channels, got {img.shape[1]}")
    H, W = img.shape[2:]
    g_host = G.detach().float().cpu()
    pads = _pads(g_host, H, W, _TAPS)
    warp = _warp_matrix(g_host, pads, H, W)
    cmat = None if C is None else C.detach().float().cpu()[:, :3, :].contiguous()
    if order == 2:
        if not (img.is_cuda and img.dtype == torch.float32):
            return _augment_twice(img, warp, pads, cmat)
        return _AdaFwd.apply(img, warp.to(img.device), None if cmat is None else cmat.to(img.device), pads)
    if not img.is_cuda:
        return _augment_torch(img, warp, pads, cmat)
    if img.dtype != torch.float32:
        raise TypeError(f"the augmentation kernels are float32, got {img.dtype}")
    return _AdaFused.apply(img, warp.to(img.device), None if cmat is None else cmat.to(img.device), pads)


# ------------------------------------------------------------------------------------------ public functions
def random_apply_affine(img, p, G=None, antialiasing_kernel=SYM6, order=1):
    """(warped image, G): G [B, 3, 3] maps output to input pixels about the image centre; None draws the inverse of
    sample_affine(p, ...).  order: see augment."""
    if tuple(antialiasing_kernel) != SYM6:
        raise ValueError("only the SYM6 filter is built into the kernels")
    if G is None:
        G = torch.inverse(sample_affine(p, img.shape[0], img.shape[2], img.shape[3]))
    return _apply(img, G, None, order), G


def random_apply_color(img, p, C=None, order=1):
    """(img with C [B, 4, 4] applied to its three channels, C); None draws sample_color(p, ...).  A single
    elementwise expression in torch on either device; `augment` folds it into the warp's store instead.  As a torch
    expression it is differentiable to any order whichever `order` is given."""
    if order not in (1, 2):
        raise ValueError(f"order is 1 or 2, got {order!r}")
    if C is None:
        C = sample_color(p, img.shape[0])
    m = C.to(img)
    out = torch.einsum("bij,bjhw->bihw", m[:, :3, :3], img) + m[:, :3, 3].view(-1, 3, 1, 1)
    return out, C


def augment(img, p, transform_matrix=(None, None), order=1):
    """(augmented image, (G, C)): random_apply_affine then random_apply_color, with the given matrices or fresh
    draws (G first, then C, from torch's CPU generator).  One autograd node on the GPU.

    order=1: the node's backward is once_differentiable and refuses deterministic mode.  order=2: the node and its
    gradient are each other's gradients (_AdaFwd / _AdaAdj), so the result differentiates to any order (R1 through the
    augmentation), and its backward runs in deterministic mode, on the fixed-order gather; a CPU tensor or another
    dtype takes the torch composition `_augment_twice`."""
    G, C = transform_matrix
    if G is None:
        G = torch.inverse(sample_affine(p, img.shape[0], img.shape[2], img.shape[3]))
    if C is None:
        C = sample_color(p, img.shape[0])
    return _apply(img, G, C, order), (G, C)
