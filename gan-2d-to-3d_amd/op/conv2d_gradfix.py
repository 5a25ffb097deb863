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

The generator's modulated convolution, demod[b, o] * conv(s[b, i] * x, w) in mode PLAIN / UP2 / DOWN2, is `_ModConv`:
one g2s_modconv launch in forward or adjoint form, linear in each of x, w and the two scales.  Its backward is built
from differentiable nodes only — the same node in the other form, the row pair `_RowDot` / `_RowScale` on
g2s_rows_dot_scale (the gradients to the scales) and `_ModWGrad` (g2s_modconv_wgrad: the weight-gradient GEMM with the
per-sample scales multiplied at operand load), which ends the chain as `_WGrad` does — so the second backward of the
path-length step needs no code of its own.  UP2 without scales, `conv2d(x, w, UP2)`, is `_ConvT` on the transposed
weight.

`use()` switches the layers of both networks (stylegan2.py) onto these functions: the discriminator's EqualConv2d /
ConvLayer / Discriminator._group_stddev, and the generator's ModulatedConv2d (onto `modulated_conv2d`), StyledConv (its
noise injection and activation as two differentiable modules, not the fused tail) and Generator.forward (the layer
loop, not the one-node synthesis).  Off by default, so the frozen-network routes of training GAN2Shape are untouched.
fp32 operands only."""
import contextlib

import torch
from torch.autograd import Function

from gan2shape_amd import lib as _lib
from gan2shape_amd import modconv as _mc
from .conv import _wgrad as _wgrad_launch
from .fused_act import _SlopeGate

PLAIN, DOWN2, UP2 = _mc.PLAIN, _mc.DOWN2, _mc.UP2

ENABLED = False              # set by use(): the discriminator's layers take this module's functions
_NO_WEIGHT_GRADIENTS = False  # set by no_weight_gradients(): both nodes return None for the weight


@contextlib.contextmanager
def use(on=True):
    """Within the block, for CUDA float32 input, the discriminator's EqualConv2d, ConvLayer and
    Discriminator._group_stddev and the generator's ModulatedConv2d, StyledConv and Generator.forward take the
    twice-differentiable, trainable nodes (the one-node synthesis and the fused noise / bias / activation tail are
    not eligible).  The choice is made in forward: a backward that runs after the block follows what forward
    recorded."""
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
    """conv(x, w [Cout, Cin, k, k]) in mode PLAIN / DOWN2 / UP2, as modconv.conv2d; trainable and twice
    differentiable.  UP2 — F.conv_transpose2d(x, w.transpose(0, 1), stride=2) — is the adjoint of the DOWN2
    convolution whose weight is w.transpose(0, 1): the `_ConvT` node with output size 2 H + k - 2, so its data
    gradient, weight gradient and second backward are those of the pair."""
    if mode == UP2:
        k = w.shape[2]
        out_hw = (2 * x.shape[2] + k - 2, 2 * x.shape[3] + k - 2)
        return _ConvT.apply(x.contiguous(), w.transpose(0, 1).contiguous(), DOWN2, out_hw)
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


# ------------------------------------------------------------------------------------- modulated convolution
class _RowDot(Function):
    """a, b [B, C, H, W] -> [B, C] = sum_hw a * b (g2s_rows_dot_scale); bilinear, its gradient is a row scale."""

    @staticmethod
    def forward(ctx, a, b):
        ctx.save_for_backward(a, b)
        return _mc.rows_dot_scale(a, b, want_out=False)[1]

    @staticmethod
    def backward(ctx, g):
        a, b = ctx.saved_tensors
        ga = _RowScale.apply(b, g) if ctx.needs_input_grad[0] else None
        gb = _RowScale.apply(a, g) if ctx.needs_input_grad[1] else None
        return ga, gb


class _RowScale(Function):
    """x [B, C, H, W], s [B, C] -> x * s[b, c] (g2s_rows_dot_scale); bilinear, its gradients are the pair's."""

    @staticmethod
    def forward(ctx, x, s):
        ctx.save_for_backward(x, s)
        return _mc.rows_dot_scale(None, x, s, want_dot=False)[0]

    @staticmethod
    def backward(ctx, g):
        x, s = ctx.saved_tensors
        gx = _RowScale.apply(g, s) if ctx.needs_input_grad[0] else None
        gs = _RowDot.apply(g, x) if ctx.needs_input_grad[1] else None
        return gx, gs


def rowdot(a, b):
    return _RowDot.apply(a.contiguous(), b.contiguous())


def rowscale(x, s):
    return _RowScale.apply(x.contiguous(), s.contiguous())


def _modconv_wgrad_launch(A, sa, G, sg, k, stride, pad):
    B, Ca, PH, PW = A.shape
    _, Cg, GH, GW = G.shape
    dw = torch.empty((Ca, Cg, k, k), dtype=torch.float32, device=A.device)
    _lib.check(_lib.load().g2s_modconv_wgrad(_lib.ptr(A), _lib.ptr(sa), _lib.ptr(G), _lib.ptr(sg), _lib.ptr(dw), B, Ca,
                                             Cg, PH, PW, GH, GW, k, stride, pad, 0, _lib.stream()))
    return dw


class _ModWGrad(Function):
    """The weight gradient [Cout, Cin, k, k] of `_ModConv` (g2s_modconv_wgrad): `side` = the tensor and scale on the
    Cout side (gy and demod in forward form), `data` = those on the Cin side.  The end of the chain."""

    @staticmethod
    def forward(ctx, side, s_side, data, s_data, k, mode):
        side, data = side.contiguous(), data.contiguous()
        s_side = None if s_side is None else s_side.contiguous()
        s_data = None if s_data is None else s_data.contiguous()
        if mode == UP2:      # the strided side is the output: dw[Cin][Cout] over the input's pixels
            return _modconv_wgrad_launch(data, s_data, side, s_side, k, 2, 0).transpose(0, 1).contiguous()
        return _modconv_wgrad_launch(side, s_side, data, s_data, k, 1 if mode == PLAIN else 2,
                                     k // 2 if mode == PLAIN else 0)

    @staticmethod
    def backward(ctx, gdw):
        raise RuntimeError("conv2d_gradfix: the gradient of a weight gradient is not built (third order for the path "
                           "length step; the weight gradient is once differentiable)")


class _ModConv(Function):
    """out_scale[b, .] * conv(in_scale[b, .] * x, w) in forward (transpose = 0) or adjoint (1) form: one g2s_modconv
    launch.  Linear in each of x, w and the two scales; the backward is built from this node in the other form, the
    row pair and `_ModWGrad`, so the second backward needs no code of its own."""

    @staticmethod
    def forward(ctx, x, w, in_scale, out_scale, mode, transpose, out_hw):
        _check(x, w)
        if (mode == DOWN2 and not transpose) or (mode == UP2 and transpose):
            _check_down2(x, w, DOWN2)
        y = _mc.modconv_raw(x, w.detach(), None if in_scale is None else in_scale.detach(),
                            None if out_scale is None else out_scale.detach(), mode, transpose)
        if ctx.needs_input_grad[1]:
            _forget_transform(w, transpose)
        if out_hw is not None and tuple(y.shape[2:]) != tuple(out_hw):
            raise RuntimeError(f"conv2d_gradfix: adjoint gives {tuple(y.shape[2:])}, the forward's input was {out_hw}")
        ctx.cfg = (mode, int(transpose))
        ctx.save_for_backward(x, w, in_scale, out_scale, y if out_scale is not None else None)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, w, si, so, y = ctx.saved_tensors
        mode, transpose = ctx.cfg
        need_x, need_w, need_si, need_so = ctx.needs_input_grad[:4]
        gy = gy.contiguous()
        gx = gw = gsi = gso = None
        hw = tuple(x.shape[2:])
        if si is not None and need_si:
            gxs = _ModConv.apply(gy, w, so, None, mode, 1 - transpose, hw)     # the gradient to in_scale * x
            gsi = _RowDot.apply(x, gxs)
            if need_x:
                gx = _RowScale.apply(gxs, si)
        elif need_x:
            gx = _ModConv.apply(gy, w, so, si, mode, 1 - transpose, hw)
        if so is not None and need_so:
            gso = _RowDot.apply(gy, y) / so
        if need_w and not _NO_WEIGHT_GRADIENTS:
            k = w.shape[2]
            gw = _ModWGrad.apply(x, si, gy, so, k, mode) if transpose else _ModWGrad.apply(gy, so, x, si, k, mode)
        return gx, gw, gsi, gso, None, None, None


def modulated_conv2d(x, w, s=None, demod=None, mode=PLAIN):
    """demod[b, o] * conv(s[b, i] * x, w [Cout, Cin, k, k]) in mode PLAIN / UP2 / DOWN2, either scale may be None:
    modconv.modconv's launch, with gradients to x, w, s and demod that can be differentiated again."""
    s = None if s is None else s.contiguous()
    demod = None if demod is None else demod.contiguous()
    return _ModConv.apply(x.contiguous(), w.contiguous(), s, demod, mode, 0, None)
