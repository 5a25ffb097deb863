"""The reference's behaviour for CPU TENSORS in the Python op API: its `op` package answers a CPU
tensor with plain PyTorch (op/fused_act.py:86-92, op/upfirdn2d.py:144-154) and a CUDA tensor with
the native module.  Same split here — and only that: a CUDA tensor NEVER comes this way (it goes to
libg2s.so, and a missing library raises in lib.load()); this module is what lets the minimal config
(BASELINE.json configs[0]: CPU tensors, plumbing only) and CPU-side tooling call the op API.

Own formulation: the resampler is zero-insertion + padding/cropping + one depthwise correlation with
the flipped FIR + strided slicing, all differentiable torch ops."""
import torch
import torch.nn.functional as F


def fused_leaky_relu(x, bias, negative_slope=0.2, scale=2 ** 0.5):
    shape = [1, -1] + [1] * (x.dim() - 2)
    return F.leaky_relu(x + bias.view(*shape), negative_slope) * scale


def upfirdn2d(x, kernel, up=1, down=1, pad=(0, 0)):
    n, c, h, w = x.shape
    planes = x.reshape(n * c, 1, h, w)
    if up > 1:                                   # zero insertion: sample (i, j) -> (i * up, j * up)
        z = planes.new_zeros(n * c, 1, h * up, w * up)
        z[:, :, ::up, ::up] = planes
        planes = z
    p0, p1 = pad
    planes = F.pad(planes, [max(p0, 0), max(p1, 0), max(p0, 0), max(p1, 0)])
    hh, ww = planes.shape[-2:]
    planes = planes[:, :, max(-p0, 0):hh - max(-p1, 0), max(-p0, 0):ww - max(-p1, 0)]   # negative pad = crop
    taps = torch.flip(kernel, [0, 1])[None, None].to(planes.dtype)                       # FIR = correlation with the flip
    out = F.conv2d(planes, taps)
    out = out[:, :, ::down, ::down]
    return out.reshape(n, c, out.shape[-2], out.shape[-1])


def _conv(x, w, mode):
    if mode == 0:
        return F.conv2d(x, w, padding=w.shape[2] // 2)
    if mode == 1:
        return F.conv_transpose2d(x, w.transpose(0, 1), stride=2)
    return F.conv2d(x, w, stride=2)


def _conv_per_sample(x, wm, mode):
    """Sample b of x [B, Cin, H, W] convolved with ITS weight wm[b] [Cout, Cin, k, k]: one grouped convolution over
    the batch folded into the channels."""
    B, Cin, H, W = x.shape
    Cout, k = wm.shape[1], wm.shape[3]
    xg = x.reshape(1, B * Cin, H, W)
    if mode == 0:
        y = F.conv2d(xg, wm.reshape(B * Cout, Cin, k, k), padding=k // 2, groups=B)
    elif mode == 1:
        y = F.conv_transpose2d(xg, wm.transpose(1, 2).reshape(B * Cin, Cout, k, k), stride=2, groups=B)
    else:
        y = F.conv2d(xg, wm.reshape(B * Cout, Cin, k, k), stride=2, groups=B)
    return y.reshape(B, Cout, y.shape[-2], y.shape[-1])


def modconv(x, w, s=None, demod=None, mode=0):
    """The modulated convolution demod[b,o] * conv(s[b,c] * x[b,c], w[o,c]) on CPU tensors; mode 0: stride 1, padding
    k // 2; 1: transposed, stride 2 (model.py:264-275 before its Blur); 2: stride 2, no padding.  With a style it is
    computed in the WEIGHT-modulation form, as the reference does (model.py:253-262): each sample's weight is w * s[b]
    (* demod[b]) and the input stays as it is.  The device kernels scale the input instead (modconv.py), which is the
    same function; in float32 the style gradient of the weight form is the more exact one (its convolution and
    demodulation paths cancel inside small per-weight sums, not between two sums over the image: latent gradient of the
    size-16 generator 7e-7 from float64 against 7e-5), and the projector's CPU path follows the reference to that."""
    if s is None:
        y = _conv(x, w, mode)
        return y if demod is None else y * demod[:, :, None, None]
    wm = w[None] * s[:, None, :, None, None]
    if demod is not None:
        wm = wm * demod[:, :, None, None, None]
    return _conv_per_sample(x, wm, mode)


def modconv_demod(x, w, s, eps=1e-8, mode=0):
    """modconv with the demodulation rsqrt(sum over (i, taps) of (w[o,i] s[b,i])^2 + eps) (model.py:254-258) taken from
    the modulated weight itself."""
    wm = w[None] * s[:, None, :, None, None]
    wm = wm * torch.rsqrt(wm.pow(2).sum([2, 3, 4]) + eps)[:, :, None, None, None]
    return _conv_per_sample(x, wm, mode)
