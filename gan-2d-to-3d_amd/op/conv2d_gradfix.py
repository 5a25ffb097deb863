"""`conv2d_gradfix` — the module stylegan2-pytorch/train.py imports for the discriminator's regulariser
(`conv2d_gradfix.no_weight_gradients()`, train.py:71-78): a convolution whose gradient can itself be differentiated
and whose weight can be trained, on libg2s.so.

The un-modulated convolution of EqualConv2d (PLAIN: stride 1, padding k // 2; DOWN2: stride 2, no padding; k 1 or 3)
is two `Function`s that are each other's data-gradient:

    _Conv   y  = conv(x, w)            modconv_raw(transpose = 0)
    _ConvT  gx = conv^T(gy, w)         modconv_raw(transpose = 1), the output size fixed to the forward's input size

so a second backward (R1: autograd.grad(create_graph=True), then backward()) walks the same two kernels again.  Both
keep modconv.wino_choice's kernel selection: stride-1 3x3 layers with enough tiles stay on Winograd.  The weight
gradient of either node is one launch of the pixel-reduction GEMM g2s_conv2d_wgrad,

    _Conv:   dw = wgrad(A = gy, G = x)          _ConvT:  dw = wgrad(A = gy of the layer, G = ggx)

and ends the chain: a gradient THROUGH a weight gradient (third order for the R1 step) is not built and raises.

`conv_bias_act` is the trainable, twice-differentiable form of modconv.ConvBiasActFunction: the same single forward
launch; backward = the activation's slope gate, then three independent launches (adjoint node, weight gradient,
channel sum for the bias), all differentiable, so its second backward needs no code of its own.

`use()` switches the discriminator's layers (stylegan2.EqualConv2d / ConvLayer / Discriminator) onto these functions;
off by default, so the frozen-network routes of training GAN2Shape are untouched.  fp32 operands only."""
import contextlib

import torch
from torch.autograd import Function

from gan2shape_amd import lib as _lib
from gan2shape_amd import modconv as _mc
from .conv import _wgrad as _wgrad_launch
from .fused_act import _SlopeGate

PLAIN, DOWN2 = _mc.PLAIN, _mc.DOWN2

ENABLED = False              # set by use(): the discriminator's layers take this module's functions
_NO_WEIGHT_GRADIENTS = False  # set by no_weight_gradients(): both nodes return None for the weight


@contextlib.contextmanager
def use(on=True):
    """Within the block, for CUDA float32 input, EqualConv2d, ConvLayer and Discriminator._group_stddev take the
    twice-differentiable, trainable nodes.  The choice is made in forward: a backward that runs after the block
    follows what forward recorded."""
    global ENABLED
    prev, ENABLED = ENABLED, bool(on)
    try:
        yield
    finally:
        ENABLED = prev


@contextlib.contextmanager
def no_weight_gradients(disable=True):
    """Within the block the backward of both nodes returns None for the weight (the launch is skipped): d_r1_loss
    wraps its autograd.grad, which asks for the image gradient only, in it.  Read when a backward RUNS."""
    global _NO_WEIGHT_GRADIENTS
    prev = _NO_WEIGHT_GRADIENTS
    if disable:
        _NO_WEIGHT_GRADIENTS = True
    try:
        yield
    finally:
        _NO_WEIGHT_GRADIENTS = prev


def _geometry(mode):
    """(stride, pad as a function of k) of the wgrad launch."""
    if mode == PLAIN:
        return 1, lambda k: k // 2
    if mode == DOWN2:
        return 2, lambda k: 0
    raise RuntimeError(f"conv2d_gradfix: mode must be PLAIN or DOWN2, got {mode}")


def _check(x, w):
    _lib.require_cuda(x, w)
    if _mc.OPERANDS != "f32":
        raise RuntimeError("conv2d_gradfix: fp32 operands only (modconv.OPERANDS is 'f16': the fp16-operand kernels "
                           "have no weight gradient and no second backward)")
    if x.dtype != torch.float32 or w.dtype != torch.float32:
        raise RuntimeError("conv2d_gradfix: float32 only")
    if w.shape[2] != w.shape[3] or w.shape[2] not in (1, 3):
        raise RuntimeError("conv2d_gradfix: 1x1 and 3x3 kernels only")


def _check_down2(x, w, mode):
    """DOWN2 covers its input exactly (modconv.conv2d_supported's rule): only then is the adjoint's output the
    forward's input size."""
    k = w.shape[2]
    if mode == DOWN2 and ((x.shape[2] - k) % 2 or (x.shape[3] - k) % 2):
        raise RuntimeError(f"conv2d_gradfix: DOWN2 needs (H - k) and (W - k) even, got {tuple(x.shape[2:])}, k = {k}")


def _forget_transform(w, transpose):
    """A weight under training is a new tensor every step: its Winograd transform must not stay in modconv's cache of
    constant tensors' transforms (which holds the tensor, too)."""
    key = (w.data_ptr(), w._version, tuple(w.shape), int(transpose))
    for cache in _mc._WINO_U.values():
        cache.pop(key, None)


class _WGrad(Function):
    """dw [Ca, Cg, k, k] = sum over pixels of A x shifted G (g2s_conv2d_wgrad); the end of the chain."""

    @staticmethod
    def forward(ctx, A, G, k, mode):
        stride, pad = _geometry(mode)
        return _wgrad_launch(A.contiguous(), G.contiguous(), k, stride, pad(k))

    @staticmethod
    def backward(ctx, gdw):
        raise RuntimeError("conv2d_gradfix: the gradient of a weight gradient is not built (third order for the R1 "
                           "step; the weight gradient is once differentiable)")


def _weight_grad(A, G, k, mode):
    return None if _NO_WEIGHT_GRADIENTS else _WGrad.apply(A, G, k, mode)


class _Conv(Function):
    @staticmethod
    def forward(ctx, x, w, mode):
        _check(x, w)
        _check_down2(x, w, mode)
        y = _mc.modconv_raw(x, w.detach(), None, None, mode, 0)     # saved below: the inputs themselves, with their graph
        if ctx.needs_input_grad[1]:
            _forget_transform(w, 0)
        ctx.mode = mode
        ctx.save_for_backward(x, w)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, w = ctx.saved_tensors
        gx = gw = None
        if ctx.needs_input_grad[0]:
            gx = _ConvT.apply(gy.contiguous(), w, ctx.mode, tuple(x.shape[2:]))
        if ctx.needs_input_grad[1]:
            gw = _weight_grad(gy, x, w.shape[2], ctx.mode)
        return gx, gw, None


class _ConvT(Function):
    """The adjoint: x [B, Cout, oh, ow] (a gradient of the layer's output) -> [B, Cin, H, W]."""

    @staticmethod
    def forward(ctx, x, w, mode, out_hw):
        _check(x, w)
        y = _mc.modconv_raw(x, w.detach(), None, None, mode, 1)
        if ctx.needs_input_grad[1]:
            _forget_transform(w, 1)
        if tuple(y.shape[2:]) != tuple(out_hw):
            raise RuntimeError(f"conv2d_gradfix: adjoint gives {tuple(y.shape[2:])}, the forward's input was {out_hw}")
        ctx.mode = mode
        ctx.save_for_backward(x, w)
        return y

    @staticmethod
    def backward(ctx, ggx):
        x, w = ctx.saved_tensors
        gx = gw = None
        if ctx.needs_input_grad[0]:
            gx = _Conv.apply(ggx.contiguous(), w, ctx.mode)
        if ctx.needs_input_grad[1]:
            gw = _weight_grad(x, ggx, w.shape[2], ctx.mode)
        return gx, gw, None, None


def conv2d(x, w, mode):
    """conv(x, w [Cout, Cin, k, k]) in mode PLAIN / DOWN2, as modconv.conv2d; trainable and twice differentiable."""
    return _Conv.apply(x.contiguous(), w.contiguous(), mode)


def conv_transpose2d(gy, w, mode, out_hw):
    """The adjoint of conv2d in its first argument: gy [B, Cout, oh, ow] -> [B, Cin, *out_hw]."""
    return _ConvT.apply(gy.contiguous(), w.contiguous(), mode, tuple(out_hw))


class _ChannelSum(Function):
    """g [B, C, H, W] -> [C] (g2s_channel_sum, fixed order): the bias gradient."""

    @staticmethod
    def forward(ctx, g):
        g = g.contiguous()
        ctx.shape = g.shape
        out = torch.empty(g.shape[1], dtype=torch.float32, device=g.device)
        _lib.check(_lib.load().g2s_channel_sum(_lib.ptr(g), _lib.ptr(out), g.shape[0], g.shape[1],
                                               g.shape[2] * g.shape[3], _lib.stream()))
        return out

    @staticmethod
    def backward(ctx, gg):
        return gg.view(1, -1, 1, 1).expand(ctx.shape)


class _ConvBiasAct(Function):
    @staticmethod
    def forward(ctx, x, w, bias, mode, alpha, gain):
        _check(x, w)
        _check_down2(x, w, mode)
        _lib.require_cuda(bias)
        y = _mc.conv_bias_act_raw(x, w.detach(), bias.detach(), mode, alpha, gain)
        if ctx.needs_input_grad[1]:
            _forget_transform(w, 0)
        ctx.cfg = (mode, float(alpha), float(gain))
        ctx.save_for_backward(x, w, y)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, w, y = ctx.saved_tensors
        mode, alpha, gain = ctx.cfg
        g = _SlopeGate.apply(gy.contiguous(), y, alpha, gain)
        gx = gw = gb = None
        if ctx.needs_input_grad[0]:
            gx = _ConvT.apply(g, w, mode, tuple(x.shape[2:]))
        if ctx.needs_input_grad[1]:
            gw = _weight_grad(g, x, w.shape[2], mode)
        if ctx.needs_input_grad[2]:
            gb = _ChannelSum.apply(g)
        return gx, gw, gb, None, None, None


def conv_bias_act(x, w, bias, mode=PLAIN, alpha=0.0, gain=1.0):
    """gain * leaky_relu(conv(x, w) + bias, alpha): one launch forward, gradients to x, w and bias, twice
    differentiable."""
    return _ConvBiasAct.apply(x.contiguous(), w.contiguous(), bias, mode, alpha, gain)
