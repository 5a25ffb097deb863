"""Minibatch-stddev feature of the discriminator (stylegan2-pytorch/model.py:756-765) on csrc/dtrain.hip: the copy of
the input and the appended constant maps in one launch, its backward in one launch, and the backward of that backward
(the R1 step differentiates the image gradient) in one launch.  The torch composition runs about a dozen small
launches forward and several dozen in double backward.

Autograd structure: `_Mbstd.backward` calls `_MbstdBwd`, a Function of (gout, x) whose own backward is
g2s_mbstd_bwd2, so a create_graph backward records the dependence of gx on both."""
import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from gan2shape_amd import lib as _lib

GROUP = 4   # the kernels' group size: min(B, 4) members


def supported(x, group, feat):
    B, C = x.shape[:2]
    return (x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and group == GROUP and B % min(B, GROUP) == 0
            and C % feat == 0)


class _MbstdBwd(Function):
    @staticmethod
    def forward(ctx, gout, x, feat):
        B, C, H, W = x.shape
        gx = torch.empty_like(x)
        _lib.check(_lib.load().g2s_mbstd_bwd(_lib.ptr(gout), _lib.ptr(x), _lib.ptr(gx), B, C, H, W, feat, _lib.stream()))
        ctx.feat = feat
        ctx.save_for_backward(gout, x)
        return gx

    @staticmethod
    @once_differentiable
    def backward(ctx, ggx):
        gout, x = ctx.saved_tensors
        B, C, H, W = x.shape
        ggx = ggx.contiguous()
        ggout = torch.empty_like(gout)
        xg = torch.empty_like(x)
        _lib.check(_lib.load().g2s_mbstd_bwd2(_lib.ptr(ggx), _lib.ptr(gout), _lib.ptr(x), _lib.ptr(ggout), _lib.ptr(xg),
                                              B, C, H, W, ctx.feat, _lib.stream()))
        return ggout, xg, None


class _Mbstd(Function):
    @staticmethod
    def forward(ctx, x, feat):
        B, C, H, W = x.shape
        out = torch.empty((B, C + feat, H, W), dtype=torch.float32, device=x.device)
        _lib.check(_lib.load().g2s_mbstd_fwd(_lib.ptr(x), _lib.ptr(out), B, C, H, W, feat, _lib.stream()))
        ctx.feat = feat
        ctx.save_for_backward(x)
        return out

    @staticmethod
    def backward(ctx, gout):
        x, = ctx.saved_tensors
        return _MbstdBwd.apply(gout.contiguous(), x, ctx.feat), None


def minibatch_stddev(x, feat=1):
    """x [B, C, H, W] -> [B, C + feat, H, W]: x and the `feat` stddev maps (group size min(B, 4))."""
    _lib.require_cuda(x)
    if x.dtype != torch.float32:
        raise RuntimeError("minibatch_stddev: float32 only")
    return _Mbstd.apply(x.contiguous(), feat)
