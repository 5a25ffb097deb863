"""The parsing networks behind the object masks of the depth priors, and MaskingModel on top of them
(behaviour of GAN2Shape/model.py:473-551 on the BiSeNet / PSPNet / ResNet definitions of
GAN2Shape/networks.py:247-586 and GAN2Shape/resnet.py).

Both nets are eval-mode convolutional nets.  Parameter and buffer names and shapes are those of the public
checkpoints (face-parsing.PyTorch `bisenet.pth`, semseg `pspnet_voc.pth`), so they load by name.  A `forward`
takes one of two routes, the rule of the op/ modules:

  - CPU tensors, or `native=True`: plain torch ops (any float dtype).  It pins the architecture on a machine
    without a GPU and is the baseline of tools/bench_masking.py;
  - CUDA tensors: libg2s only, fp32, under no_grad.  BatchNorm is folded into the preceding convolution once
    (first use, again after load_state_dict or a move); every convolution with k <= 5 is one g2s_conv2d launch
    with bias and ReLU in its epilogue; the 7x7 stem, the pools, the bilinear resizes and the elementwise
    gate / residual passes are the kernels of csrc/parsing.hip.  Nearest up-sampling, channel concatenation and
    the polyphase shuffle of the dilated convolutions stay in torch (copies).  A missing kernel is an error.
"""
import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import lib as _lib
from . import utils
from .op.conv import _conv2d_raw


# ======================================================================================= libg2s wrappers
def _f32c(x):
    if x.dtype != torch.float32:
        raise RuntimeError("parsing: the libg2s route is float32 only")
    return x.contiguous()


def conv_stem7(x, w, bias, relu=True):
    """7x7 stride-2 pad-3 convolution from 3 channels, bias and ReLU fused (g2s_conv_stem7)."""
    _lib.require_cuda(x, w, bias)
    x, w = _f32c(x), _f32c(w)
    B, _, H, W = x.shape
    M = w.shape[0]
    y = torch.empty(B, M, (H - 1) // 2 + 1, (W - 1) // 2 + 1, dtype=torch.float32, device=x.device)
    _lib.check(_lib.load().g2s_conv_stem7(_lib.ptr(x), _lib.ptr(w), _lib.ptr(bias), _lib.ptr(y), B, M, H, W,
                                          int(relu), _lib.stream()))
    return y


def maxpool3x3s2(x):
    """F.max_pool2d(x, 3, 2, 1) (g2s_maxpool3x3s2)."""
    _lib.require_cuda(x)
    x = _f32c(x)
    B, C, H, W = x.shape
    y = torch.empty(B, C, (H - 1) // 2 + 1, (W - 1) // 2 + 1, dtype=torch.float32, device=x.device)
    _lib.check(_lib.load().g2s_maxpool3x3s2(_lib.ptr(x), _lib.ptr(y), B * C, H, W, _lib.stream()))
    return y


def adaptive_avgpool(x, size):
    """F.adaptive_avg_pool2d(x, size) (g2s_adaptive_avgpool)."""
    _lib.require_cuda(x)
    x = _f32c(x)
    oh, ow = (size, size) if isinstance(size, int) else size
    B, C, H, W = x.shape
    y = torch.empty(B, C, oh, ow, dtype=torch.float32, device=x.device)
    _lib.check(_lib.load().g2s_adaptive_avgpool(_lib.ptr(x), _lib.ptr(y), B * C, H, W, oh, ow, _lib.stream()))
    return y


def resize_bilinear(x, size, align_corners):
    """F.interpolate(x, size, mode='bilinear', align_corners=align_corners) (g2s_resize_bilinear)."""
    _lib.require_cuda(x)
    x = _f32c(x)
    oh, ow = (size, size) if isinstance(size, int) else size
    B, C, H, W = x.shape
    y = torch.empty(B, C, oh, ow, dtype=torch.float32, device=x.device)
    _lib.check(_lib.load().g2s_resize_bilinear(_lib.ptr(x), _lib.ptr(y), B * C, H, W, oh, ow, int(align_corners),
                                               _lib.stream()))
    return y


def gate_add_act(x, s=None, t=None, r=None, sigmoid=False, plus_one=False, relu=False):
    """act(x * s' + t + r): s, t (B, C[, 1, 1]) per-channel gate and offset, r a tensor like x; s' = s, through
    a sigmoid and / or plus one on request (g2s_gate_add_act)."""
    _lib.require_cuda(x, s, t, r)
    x = _f32c(x)
    B, C, H, W = x.shape
    s, t = [None if v is None else _f32c(v).reshape(B * C) for v in (s, t)]
    if r is not None:
        r = _f32c(r)
        if r.shape != x.shape:
            raise RuntimeError("gate_add_act: r must have the shape of x")
    y = torch.empty_like(x)
    _lib.check(_lib.load().g2s_gate_add_act(_lib.ptr(x), _lib.ptr(s), _lib.ptr(t), _lib.ptr(r), _lib.ptr(y), B * C,
                                            H * W, int(sigmoid), int(plus_one), int(relu), _lib.stream()))
    return y


PARSE_HARD, PARSE_CONFIDENCE = 0, 1


def parse_head(logits, size, S, mode, drop, class_set, want_full_mask=False):
    """The full-resolution part of MaskingModel as one fused pass (g2s_parse_head): the (B, C, h, w) logits are
    interpolated to size x size (bilinear, align_corners=True) pixel by pixel, the rule is applied, and the
    area average over PyTorch's adaptive bins lands in the (B, 1, S, S) result.  mode PARSE_HARD: 1 where the
    argmax over the channels other than `drop` (-1: none) is in `class_set` (bit c = channel c of the logits);
    a sample without such a pixel becomes all ones and its `fallback` flag is set.  PARSE_CONFIDENCE: the sum of
    the channels in class_set, normalised per sample to [0, 1] by its full-resolution min and max.
    Returns (out, full_mask uint8 (B, 1, size, size) or None, fallback int32 (B,))."""
    _lib.require_cuda(logits)
    logits = _f32c(logits)
    B, C, h, w = logits.shape
    L = _lib.load()
    dev = logits.device
    out = torch.empty(B, 1, S, S, dtype=torch.float32, device=dev)
    full = torch.empty(B, 1, size, size, dtype=torch.uint8, device=dev) if want_full_mask else None
    flag = torch.empty(B, dtype=torch.int32, device=dev)
    ws = torch.empty(max(int(L.g2s_parse_head_workspace_bytes(B)), 1), dtype=torch.uint8, device=dev)
    _lib.check(L.g2s_parse_head(_lib.ptr(logits), B, C, h, w, size, S, mode, drop, class_set, _lib.ptr(out),
                                _lib.ptr(full), _lib.ptr(flag), _lib.ptr(ws), ws.numel(), _lib.stream()))
    return out, full, flag


# ======================================================================================= shared pieces
def fold_bn(conv, bn, dtype=torch.float32):
    """(weight, bias) of the convolution that equals bn(conv(x)) in eval mode; the arithmetic is float64."""
    w = conv.weight.detach().double()
    if bn is None:
        b = None if conv.bias is None else conv.bias.detach().to(dtype).contiguous()
        return w.to(dtype).contiguous(), b
    scale = bn.weight.detach().double() / torch.sqrt(bn.running_var.detach().double() + bn.eps)
    b = bn.bias.detach().double() - bn.running_mean.detach().double() * scale
    if conv.bias is not None:
        b = b + conv.bias.detach().double() * scale
    return (w * scale[:, None, None, None]).to(dtype).contiguous(), b.to(dtype).contiguous()


def polyphase_split(x, d):
    """(B, C, H, W) -> (d*d*B, C, ceil(H/d), ceil(W/d)): the d x d sub-grids x[..., i::d, j::d] (zero-padded to
    a multiple of d) stacked on the batch axis, sub-grid (i, j) at batch rows (i*d + j)*B ..."""
    B, C, H, W = x.shape
    Hp, Wp = -(-H // d) * d, -(-W // d) * d
    if (Hp, Wp) != (H, W):
        x = F.pad(x, (0, Wp - W, 0, Hp - H))
    x = x.reshape(B, C, Hp // d, d, Wp // d, d).permute(3, 5, 0, 1, 2, 4)
    return x.reshape(d * d * B, C, Hp // d, Wp // d)


def polyphase_merge(y, d, B, H, W):
    """Inverse of polyphase_split for the (d*d*B, M, ., .) result, cropped to H x W."""
    _, M, h, w = y.shape
    y = y.view(d, d, B, M, h, w).permute(2, 3, 4, 0, 5, 1).reshape(B, M, h * d, w * d)
    return y[:, :, :H, :W].contiguous()


def dilated_conv3x3(x, w, bias, d, conv=None):
    """3x3 convolution with dilation d, padding d, stride 1 as d*d dense pad-1 convolutions on the polyphase
    sub-grids of x, in one call of `conv(x, w, bias)` (default F.conv2d with padding 1)."""
    B, _, H, W = x.shape
    if conv is None:
        def conv(xs, w_, b_):
            return F.conv2d(xs, w_, b_, padding=1)
    if d == 1:
        return conv(x, w, bias)
    return polyphase_merge(conv(polyphase_split(x, d), w, bias), d, B, H, W)


class _ParsingNet(nn.Module):
    """Route selection and the folded-weight cache of the libg2s route."""

    def __init__(self):
        super().__init__()
        self._folded = {}

    def _apply(self, fn, *args, **kwargs):
        self._folded = {}
        return super()._apply(fn, *args, **kwargs)

    def load_state_dict(self, *args, **kwargs):
        self._folded = {}
        return super().load_state_dict(*args, **kwargs)

    def train(self, mode=True):
        if mode:
            raise RuntimeError("the parsing nets are eval-only")
        return super().train(False)

    def _use_native(self, x, native):
        return native or not x.is_cuda

    # one convolution (+ BatchNorm) (+ ReLU) on either route
    def _cbr(self, x, conv, bn, relu, native):
        d = conv.dilation[0]
        if native:
            y = conv(x)
            y = y if bn is None else bn(y)
            return F.relu(y) if relu else y
        key = id(conv)
        if key not in self._folded:
            self._folded[key] = fold_bn(conv, bn)
        w, b = self._folded[key]
        k, stride, pad = conv.kernel_size[0], conv.stride[0], conv.padding[0]
        M, Cr = w.shape[0], w.shape[1]
        if k == 7:
            if (stride, pad, Cr) != (2, 3, 3):
                raise RuntimeError("parsing: the only 7x7 kernel is the stride-2 pad-3 RGB stem")
            return conv_stem7(x, w, b, relu)

        def run(xs, w_, b_, stride_=stride, pad_=pad):
            return _conv2d_raw(xs.contiguous(), w_, b_, Cr, M, k, stride_, pad_, False, True, None, relu, 0.0)
        if d != 1:
            if (k, stride, pad) != (3, 1, d):
                raise RuntimeError("parsing: dilated convolutions are 3x3, stride 1, padding = dilation")
            return dilated_conv3x3(x, w, b, d, lambda xs, w_, b_: run(xs, w_, b_, 1, 1))
        return run(x, w, b)

    @staticmethod
    def _check_input(x):
        if x.dim() != 4 or x.shape[1] != 3:
            raise ValueError(f"parsing nets take (B, 3, H, W) images, got {tuple(x.shape)}")


def _conv(cin, cout, k, stride=1, pad=0, bias=False):
    return nn.Conv2d(cin, cout, k, stride, pad, bias=bias)


class BasicBlock(nn.Module):
    expansion = 1

    def __init__(self, cin, planes, stride=1, downsample=None):
        super().__init__()
        self.conv1 = _conv(cin, planes, 3, stride, 1)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = _conv(planes, planes, 3, 1, 1)
        self.bn2 = nn.BatchNorm2d(planes)
        self.downsample = downsample

    def run(self, net, x, native):
        y = net._cbr(x, self.conv1, self.bn1, True, native)
        y = net._cbr(y, self.conv2, self.bn2, False, native)
        return _residual(net, self, x, y, native)


class Bottleneck(nn.Module):
    expansion = 4

    def __init__(self, cin, planes, stride=1, downsample=None):
        super().__init__()
        self.conv1 = _conv(cin, planes, 1)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = _conv(planes, planes, 3, stride, 1)
        self.bn2 = nn.BatchNorm2d(planes)
        self.conv3 = _conv(planes, planes * 4, 1)
        self.bn3 = nn.BatchNorm2d(planes * 4)
        self.downsample = downsample

    def run(self, net, x, native):
        y = net._cbr(x, self.conv1, self.bn1, True, native)
        y = net._cbr(y, self.conv2, self.bn2, True, native)
        y = net._cbr(y, self.conv3, self.bn3, False, native)
        return _residual(net, self, x, y, native)


def _residual(net, block, x, y, native):
    if block.downsample is not None:
        x = net._cbr(x, block.downsample[0], block.downsample[1], False, native)
    return F.relu(y + x) if native else gate_add_act(y, r=x, relu=True)


def _make_layer(block, cin, planes, blocks, stride):
    down = None
    if stride != 1 or cin != planes * block.expansion:
        down = nn.Sequential(_conv(cin, planes * block.expansion, 1, stride), nn.BatchNorm2d(planes * block.expansion))
    layers = [block(cin, planes, stride, down)]
    layers += [block(planes * block.expansion, planes) for _ in range(1, blocks)]
    return nn.Sequential(*layers)


def _run_layer(net, layer, x, native):
    for block in layer:
        x = block.run(net, x, native)
    return x


def _maxpool(x, native):
    return F.max_pool2d(x, 3, 2, 1) if native else maxpool3x3s2(x)


def _global_avg(x, native):
    return F.adaptive_avg_pool2d(x, 1) if native else adaptive_avgpool(x, 1)


# ======================================================================================= BiSeNet
class _Resnet18(nn.Module):
    """ResNet-18 trunk, 7x7 stem, no classifier: feat8, feat16, feat32."""

    def __init__(self):
        super().__init__()
        self.conv1 = _conv(3, 64, 7, 2, 3)
        self.bn1 = nn.BatchNorm2d(64)
        self.layer1 = _make_layer(BasicBlock, 64, 64, 2, 1)
        self.layer2 = _make_layer(BasicBlock, 64, 128, 2, 2)
        self.layer3 = _make_layer(BasicBlock, 128, 256, 2, 2)
        self.layer4 = _make_layer(BasicBlock, 256, 512, 2, 2)


class ConvBNReLU(nn.Module):
    def __init__(self, cin, cout, ks=3, stride=1, padding=1):
        super().__init__()
        self.conv = _conv(cin, cout, ks, stride, padding)
        self.bn = nn.BatchNorm2d(cout)

    def run(self, net, x, native):
        return net._cbr(x, self.conv, self.bn, True, native)


class BiSeNetOutput(nn.Module):
    def __init__(self, cin, mid, n_classes):
        super().__init__()
        self.conv = ConvBNReLU(cin, mid)
        self.conv_out = _conv(mid, n_classes, 1)


class AttentionRefinementModule(nn.Module):
    def __init__(self, cin, cout):
        super().__init__()
        self.conv = ConvBNReLU(cin, cout)
        self.conv_atten = _conv(cout, cout, 1)
        self.bn_atten = nn.BatchNorm2d(cout)

    def run(self, net, x, native, add_channel=None, add_map=None):
        """feat * sigmoid(bn(conv(mean(feat)))) + (add_channel broadcast | add_map)."""
        feat = self.conv.run(net, x, native)
        atten = net._cbr(_global_avg(feat, native), self.conv_atten, self.bn_atten, False, native)
        if native:
            out = feat * torch.sigmoid(atten)
            return out + (add_channel if add_map is None else add_map)
        return gate_add_act(feat, s=atten, t=add_channel, r=add_map, sigmoid=True)


class ContextPath(nn.Module):
    def __init__(self):
        super().__init__()
        self.resnet = _Resnet18()
        self.arm16 = AttentionRefinementModule(256, 128)
        self.arm32 = AttentionRefinementModule(512, 128)
        self.conv_head32 = ConvBNReLU(128, 128)
        self.conv_head16 = ConvBNReLU(128, 128)
        self.conv_avg = ConvBNReLU(512, 128, 1, 1, 0)


class FeatureFusionModule(nn.Module):
    def __init__(self, cin, cout):
        super().__init__()
        self.convblk = ConvBNReLU(cin, cout, 1, 1, 0)
        self.conv1 = _conv(cout, cout // 4, 1)
        self.conv2 = _conv(cout // 4, cout, 1)


class BiSeNet(_ParsingNet):
    """BiSeNet with the ResNet-18 context path and feat8 in place of the spatial path (networks.py:357-586).
    forward(x (B, 3, H, W)) -> (B, n_classes, H, W) logits; logits_lowres(x) stops before the final bilinear
    up-sampling (H/8 x W/8).  The conv_out16 / conv_out32 heads are parameters only."""

    def __init__(self, n_classes=19):
        super().__init__()
        self.cp = ContextPath()
        self.ffm = FeatureFusionModule(256, 256)
        self.conv_out = BiSeNetOutput(256, 256, n_classes)
        self.conv_out16 = BiSeNetOutput(128, 64, n_classes)
        self.conv_out32 = BiSeNetOutput(128, 64, n_classes)
        self.eval()

    @torch.no_grad()
    def features(self, x, native=False):
        """feat8, feat16, feat32 of the trunk."""
        native = self._use_native(x, native)
        r = self.cp.resnet
        y = _maxpool(self._cbr(x, r.conv1, r.bn1, True, native), native)
        y = _run_layer(self, r.layer1, y, native)
        feat8 = _run_layer(self, r.layer2, y, native)
        feat16 = _run_layer(self, r.layer3, feat8, native)
        feat32 = _run_layer(self, r.layer4, feat16, native)
        return feat8, feat16, feat32

    def logits_lowres(self, x, native=False):
        self._check_input(x)
        native = self._use_native(x, native)
        with torch.no_grad():
            cp = self.cp
            feat8, feat16, feat32 = self.features(x, native)
            avg = cp.conv_avg.run(self, _global_avg(feat32, native), native)          # (B, 128, 1, 1)
            feat32_sum = cp.arm32.run(self, feat32, native, add_channel=avg)
            feat32_up = cp.conv_head32.run(self, F.interpolate(feat32_sum, feat16.shape[2:], mode='nearest'), native)
            feat16_sum = cp.arm16.run(self, feat16, native, add_map=feat32_up)
            feat16_up = cp.conv_head16.run(self, F.interpolate(feat16_sum, feat8.shape[2:], mode='nearest'), native)
            ffm = self.ffm
            feat = ffm.convblk.run(self, torch.cat([feat8, feat16_up], 1), native)
            a = self._cbr(_global_avg(feat, native), ffm.conv1, None, True, native)
            a = self._cbr(a, ffm.conv2, None, False, native)
            fuse = feat * torch.sigmoid(a) + feat if native else gate_add_act(feat, s=a, sigmoid=True, plus_one=True)
            y = self.conv_out.conv.run(self, fuse, native)
            return self._cbr(y, self.conv_out.conv_out, None, False, native)

    def forward(self, x, native=False):
        low = self.logits_lowres(x, native)
        size = tuple(x.shape[2:])
        with torch.no_grad():
            if self._use_native(x, native):
                return F.interpolate(low, size, mode='bilinear', align_corners=True)
            return resize_bilinear(low, size, True)

    @staticmethod
    def head_size(H):
        return H


# ======================================================================================= PSPNet
class PSPNet(_ParsingNet):
    """PSPNet on the deep-base ResNet-50 with dilated layer3 / layer4 and the pyramid pooling module
    (networks.py:247-354), eval only: no `aux` branch (load_checkpoint drops its keys).  forward(x) with
    (H - 1) % 8 == 0 -> (B, classes, H, W) logits; logits_lowres stops before the final up-sampling."""

    def __init__(self, layers=50, classes=21, bins=(1, 2, 3, 6), dropout=0.1):
        super().__init__()
        if layers != 50:
            raise NotImplementedError("PSPNet: ResNet-50 trunk only")
        self.bins = tuple(bins)
        self.layer0 = nn.Sequential(_conv(3, 64, 3, 2, 1), nn.BatchNorm2d(64), nn.ReLU(),
                                    _conv(64, 64, 3, 1, 1), nn.BatchNorm2d(64), nn.ReLU(),
                                    _conv(64, 128, 3, 1, 1), nn.BatchNorm2d(128), nn.ReLU(),
                                    nn.MaxPool2d(3, 2, 1))
        self.layer1 = _make_layer(Bottleneck, 128, 64, 3, 1)
        self.layer2 = _make_layer(Bottleneck, 256, 128, 4, 2)
        self.layer3 = _make_layer(Bottleneck, 512, 256, 6, 1)
        self.layer4 = _make_layer(Bottleneck, 1024, 512, 3, 1)
        for layer, d in ((self.layer3, 2), (self.layer4, 4)):
            for block in layer:
                block.conv2.dilation, block.conv2.padding = (d, d), (d, d)
        fea = 2048
        red = fea // len(self.bins)
        self.ppm = nn.Module()
        self.ppm.features = nn.ModuleList(
            nn.Sequential(nn.AdaptiveAvgPool2d(b), _conv(fea, red, 1), nn.BatchNorm2d(red), nn.ReLU())
            for b in self.bins)
        self.cls = nn.Sequential(_conv(2 * fea, 512, 3, 1, 1), nn.BatchNorm2d(512), nn.ReLU(), nn.Dropout2d(dropout),
                                 _conv(512, classes, 1, bias=True))
        self.eval()

    @torch.no_grad()
    def features(self, x, native=False):
        """Outputs of layer1 .. layer4."""
        native = self._use_native(x, native)
        l0 = self.layer0
        y = x
        for i in (0, 3, 6):
            y = self._cbr(y, l0[i], l0[i + 1], True, native)
        y = _maxpool(y, native)
        feats = []
        for layer in (self.layer1, self.layer2, self.layer3, self.layer4):
            y = _run_layer(self, layer, y, native)
            feats.append(y)
        return feats

    def logits_lowres(self, x, native=False):
        self._check_input(x)
        if (x.shape[2] - 1) % 8 or (x.shape[3] - 1) % 8:
            raise ValueError("PSPNet: input height and width must be 8 n + 1")
        native = self._use_native(x, native)
        with torch.no_grad():
            y = self.features(x, native)[-1]
            hw = tuple(y.shape[2:])
            pyramid = [y]
            for b, f in zip(self.bins, self.ppm.features):
                p = F.adaptive_avg_pool2d(y, b) if native else adaptive_avgpool(y, b)
                p = self._cbr(p, f[1], f[2], True, native)
                pyramid.append(F.interpolate(p, hw, mode='bilinear', align_corners=True) if native
                               else resize_bilinear(p, hw, True))
            y = self._cbr(torch.cat(pyramid, 1), self.cls[0], self.cls[1], True, native)
            return self._cbr(y, self.cls[4], None, False, native)

    def forward(self, x, native=False):
        low = self.logits_lowres(x, native)
        size = ((x.shape[2] - 1) // 8 * 8 + 1, (x.shape[3] - 1) // 8 * 8 + 1)
        with torch.no_grad():
            if self._use_native(x, native):
                return F.interpolate(low, size, mode='bilinear', align_corners=True)
            return resize_bilinear(low, size, True)


def load_checkpoint(net, path):
    """Load a parsing checkpoint by name: a plain state dict (bisenet.pth) or {'state_dict': ...} with the
    `module.` prefixes of DataParallel (pspnet_voc.pth, model.py:487-491).  Keys of the training-only `aux`
    branch are dropped; anything else missing or unexpected raises.  A missing file raises FileNotFoundError."""
    if not os.path.isfile(path):
        raise FileNotFoundError(f"parsing checkpoint not found: {path}")
    state = torch.load(path, map_location="cpu")
    if isinstance(state, dict) and "state_dict" in state:
        state = state["state_dict"]
    state = {(k[len("module."):] if k.startswith("module.") else k): v for k, v in state.items()}
    state = {k: v for k, v in state.items() if not k.startswith("aux.")}
    net.load_state_dict(state, strict=True)
    return net


# ======================================================================================= MaskingModel
class MaskingModel():
    """Object mask and confidence map of an image from the parsing net of its category (model.py:473-551):
    BiSeNet (19 classes, `bisenet.pth`) for 'face', PSPNet-50 (21 VOC classes, `pspnet_voc.pth`) otherwise.

    image_mask(image) -> (B, 1, S, S): the image is resized to `size` (512 face / 473 other; bilinear,
    align_corners=False, when that is larger, area otherwise, utils.resize), parsed, and the hard mask
    is resized back to S.  Face: channel 17 is dropped before the argmax and the classes 1..13 form the mask
    (the reference's `mask_all & mask_face`); VOC: the argmax equals CATEGORY2NUMBER[category]; any other
    category: all ones.  A sample without a single pixel of the class gets all ones.
    confidence_mask(image): the sum of channels 1..12 (face) or the category's channel, minus its minimum,
    divided by the maximum of that, resized back.
    image_mask(image, depth): the plotting variant — depth resized to `size`, NaN outside the mask, resized back.

    Differences from the reference:
      - `size` and `net` are arguments (tests run small; a caller may bring a loaded net);
      - a batch of B images is accepted; the result is (B, 1, S, S) on the image's device;
      - the min / max normalisation and the all-ones fallback are per sample (equal to the reference at B = 1,
        the only way it is called);
      - nothing synchronises with the host: the fallback is decided on the device, `last_fallback` holds an
        int32 flag per sample of the latest image_mask call for the caller to read later, no warning is logged;
      - image_mask(image, depth) masks every sample with its own mask (the reference uses mask[0]).
    CUDA images run on libg2s (the nets' libg2s route and g2s_parse_head, which never materialises the
    full-resolution logits); CPU images, or native=True, run the same rules in torch ops."""

    CATEGORIES = ['aeroplane', 'bicycle', 'bird', 'boat', 'bottle', 'bus', 'car', 'cat', 'chair', 'cow',
                  'diningtable', 'dog', 'horse', 'motorbike', 'person', 'pottedplant', 'sheep', 'sofa', 'train',
                  'tvmonitor']
    CATEGORY2NUMBER = {category: i + 1 for i, category in enumerate(CATEGORIES)}
    FACE_DROP = 17
    FACE_CLASSES = sum(1 << c for c in range(1, 14))
    FACE_CONFIDENCE = sum(1 << c for c in range(1, 13))

    def __init__(self, category, device="cuda", ckpt_dir="checkpoints/parsing", size=None, net=None, native=False):
        self.category = category
        self.device = torch.device(device)
        self.native = native
        self.size = size if size is not None else (512 if category == 'face' else 473)
        if net is None:
            if category == 'face':
                net = load_checkpoint(BiSeNet(19), os.path.join(ckpt_dir, "bisenet.pth"))
            else:
                net = load_checkpoint(PSPNet(50, 21), os.path.join(ckpt_dir, "pspnet_voc.pth"))
        self.mask_net = net.to(self.device).eval()
        self.last_fallback = None

    # ---- the rule as data: (drop channel or -1, class set) of the hard mask and of the confidence sum
    def _hard_rule(self):
        if self.category == 'face':
            return self.FACE_DROP, self.FACE_CLASSES
        if self.category in self.CATEGORY2NUMBER:
            return -1, 1 << self.CATEGORY2NUMBER[self.category]
        return None

    def _confidence_rule(self):
        if self.category == 'face':
            return self.FACE_CONFIDENCE
        if self.category in self.CATEGORY2NUMBER:
            return 1 << self.CATEGORY2NUMBER[self.category]
        return None

    def _resized_input(self, image):
        size = self.size
        if image.is_cuda and not self.native:
            image = image.float()
            if size > image.shape[-2]:
                return resize_bilinear(image, size, False)
            if size < image.shape[-2]:
                return adaptive_avgpool(image, size)
            return image
        return utils.resize(image, [size, size])

    @staticmethod
    def _members(class_set, C, device):
        return torch.tensor([(class_set >> c) & 1 for c in range(C)], dtype=torch.bool, device=device)

    def _full_hard_mask_torch(self, out):
        """(B, 1, size, size) bool mask and (B,) fallback flags from full-resolution logits, in torch ops."""
        rule = self._hard_rule()
        B = out.shape[0]
        if rule is None:
            return torch.ones_like(out[:, :1], dtype=torch.bool), torch.zeros(B, dtype=torch.int32, device=out.device)
        drop, class_set = rule
        scores = out
        if drop >= 0:
            scores = out.clone()
            scores[:, drop] = float('-inf')
        mask = self._members(class_set, out.shape[1], out.device)[scores.argmax(1, keepdim=True)]
        empty = ~mask.flatten(1).any(1)
        return mask | empty[:, None, None, None], empty.to(torch.int32)

    def _hard(self, image, want_full):
        """(soft (B, 1, S, S) mask, full-resolution bool mask or None) of a batch."""
        S = image.shape[-1]
        x = self._resized_input(image)
        rule = self._hard_rule()
        if image.is_cuda and not self.native and rule is not None and S <= self.size:
            low = self.mask_net.logits_lowres(x)
            soft, full, flag = parse_head(low, self.size, S, PARSE_HARD, rule[0], rule[1], want_full)
            self.last_fallback = flag
            return soft, (None if full is None else full.bool())
        full, self.last_fallback = self._full_hard_mask_torch(self.mask_net(x, native=self.native))
        return utils.resize(full.float(), [S, S]), full

    def image_mask(self, image, depth=None):
        with torch.no_grad():
            soft, full = self._hard(image, depth is not None)
            if depth is None:
                return soft
            S = image.shape[-1]
            d = utils.resize(depth.to(soft.dtype), [self.size, self.size])
            d = d[:, None] if d.dim() == 3 else d
            d = torch.where(full, d, torch.full_like(d, float('nan')))
            return utils.resize(d, [S, S])

    def confidence_mask(self, image, depth=None):
        with torch.no_grad():
            S = image.shape[-1]
            x = self._resized_input(image)
            class_set = self._confidence_rule()
            if class_set is None:
                return torch.full((image.shape[0], 1, S, S), float('nan'), device=image.device)  # (1 - 1) / 0
            if image.is_cuda and not self.native and S <= self.size:
                low = self.mask_net.logits_lowres(x)
                return parse_head(low, self.size, S, PARSE_CONFIDENCE, -1, class_set)[0]
            out = self.mask_net(x, native=self.native)
            conf = out[:, self._members(class_set, out.shape[1], out.device)].sum(1, keepdim=True)
            conf = conf - conf.amin((1, 2, 3), keepdim=True)
            conf = conf / conf.amax((1, 2, 3), keepdim=True)
            return utils.resize(conf, [S, S])


def masking_model_from_config(config, device="cuda"):
    """MaskingModel of config['category'] if config['parsing_ckpt_dir'] names an existing directory, else None
    (the caller keeps the synthetic mask)."""
    ckpt_dir = config.get('parsing_ckpt_dir')
    if not ckpt_dir or not os.path.isdir(ckpt_dir):
        return None
    return MaskingModel(config.get('category'), device=device, ckpt_dir=ckpt_dir, size=config.get('parsing_size'))


def mask_depth(masking_model, image, depth):
    """What evaluate_results.py:103 does with the depth of Model.evaluate_results: NaN outside the object."""
    return masking_model.image_mask(image, depth)
