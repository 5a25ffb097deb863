"""The centre crop of step 2 (GAN2Shape/model.py:197-200, 211-214, the lines behind `# FIXME: add back cropping`):

    x = utils.resize(x, [origin_size, origin_size])
    x = utils.crop(x, crop)
    x = utils.resize(x, [image_size, image_size])

The three steps are linear and separable: out = A x A^T per plane, with one matrix A [out_size, in_size] whose rows
and columns are contiguous bands of a few taps (`crop_resize_tables`).  On CUDA float32 `crop_resize` is therefore ONE
launch of g2s_resample_sep (csrc/resample.hip) with the band table of A, and its backward the same launch with the
table of A^T — a pair of autograd nodes that are each other's gradients, so the call differentiates to any order on
the one kernel.  Everything else (CPU, other dtypes, fused=False) runs the torch composition above, which is the
specification."""
import collections
import ctypes as C
import math

import numpy as np
import torch
from torch.autograd import Function

from .. import lib as _lib
from .. import utils

MAX_TAPS = 8        # g2s_resample_max_taps()

# one band table: position i of the output reads the input positions lo[i] .. lo[i] + len[i] - 1 with the weights
# w[i, :len[i]] (w [n_out, K] float32, zero beyond the band).  lo / len / w are tensors on the table's device, `host`
# the numpy triple they were made from.
Bands = collections.namedtuple("Bands", "lo len w n_in n_out K host")
# fwd: the table of A (indexed by output position), tr: the table of A^T (indexed by input position, holding its band
# of output positions); dense: A in float64
CropResizeTables = collections.namedtuple("CropResizeTables", "fwd tr dense in_size origin_size crop out_size")

_tables = {}


def resize_matrix(n_in, n_out):
    """The 1-D operator of utils.resize along one axis, float64 [n_out, n_in]: area (adaptive average pooling, windows
    [floor(i n_in / n_out), ceil((i + 1) n_in / n_out)) with uniform weights) towards a smaller size, bilinear with
    align_corners=False and the source position clamped at 0 towards a larger one, the identity for equal sizes."""
    A = np.zeros((n_out, n_in), dtype=np.float64)
    if n_out == n_in:
        A[np.arange(n_out), np.arange(n_in)] = 1.0
    elif n_out < n_in:
        for i in range(n_out):
            a, b = (i * n_in) // n_out, -((-(i + 1) * n_in) // n_out)
            A[i, a:b] = 1.0 / (b - a)
    else:
        scale = n_in / n_out
        for i in range(n_out):
            src = max((i + 0.5) * scale - 0.5, 0.0)
            i0 = min(int(math.floor(src)), n_in - 1)
            i1 = min(i0 + 1, n_in - 1)
            lam = src - i0
            A[i, i0] += 1.0 - lam
            A[i, i1] += lam
    return A


def crop_resize_matrix(in_size, origin_size, crop, out_size):
    """A [out_size, in_size] float64 of resize -> centre crop -> resize along one axis; the crop margin is
    (origin_size - crop) // 2 as in utils.crop."""
    in_size, origin_size, crop, out_size = int(in_size), int(origin_size), int(crop), int(out_size)
    if in_size < 1 or out_size < 1 or origin_size < 1:
        raise ValueError(f"sizes must be positive, got in {in_size}, origin_size {origin_size}, out {out_size}")
    if not 0 < crop <= origin_size:
        raise ValueError(f"crop must satisfy 0 < crop <= origin_size, got crop {crop}, origin_size {origin_size}")
    lo = (origin_size - crop) // 2
    return resize_matrix(crop, out_size) @ resize_matrix(in_size, origin_size)[lo:lo + crop]


def _bands_of(A):
    """Rows of a dense operator as (lo, len, w float32 [n, K]); every row must be one contiguous band."""
    n = A.shape[0]
    lo, ln = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
    for i in range(n):
        nz = np.flatnonzero(A[i])
        if len(nz):
            lo[i], ln[i] = nz[0], nz[-1] - nz[0] + 1
            assert len(nz) == ln[i], f"row {i} of the operator is not one contiguous band: {nz}"
    K = max(int(ln.max()), 1)
    w = np.zeros((n, K), dtype=np.float32)
    for i in range(n):
        w[i, :ln[i]] = A[i, lo[i]:lo[i] + ln[i]].astype(np.float32)      # rounded once, from float64
    return lo, ln, w


def make_bands(lo, ln, w, n_in, device):
    """Check a band table (g2s_resample_bands_check on a CUDA device: K within the kernel's cap, every band inside
    [0, n_in), ascending and without gaps) and put it on `device`.  A bad table raises ValueError."""
    lo = np.ascontiguousarray(lo, dtype=np.int32)
    ln = np.ascontiguousarray(ln, dtype=np.int32)
    w = np.ascontiguousarray(w, dtype=np.float32)
    if lo.ndim != 1 or ln.shape != lo.shape or w.ndim != 2 or w.shape[0] != len(lo) or len(lo) == 0:
        raise ValueError(f"band table shapes disagree: lo {lo.shape}, len {ln.shape}, w {w.shape}")
    K = w.shape[1]
    device = torch.device(device)
    if device.type == "cuda":
        L = _lib.load()
        rc = L.g2s_resample_bands_check(lo.ctypes.data_as(C.c_void_p), ln.ctypes.data_as(C.c_void_p), len(lo), K, int(n_in))
        if rc != 0:
            raise ValueError(f"bad band table: {L.g2s_last_error().decode()}")
    return Bands(torch.from_numpy(lo).to(device), torch.from_numpy(ln).to(device), torch.from_numpy(w).to(device),
                 int(n_in), len(lo), K, (lo, ln, w))


def crop_resize_tables(in_size, origin_size, crop, out_size, device="cpu"):
    """The band tables of resize(in -> origin_size), centre crop to `crop`, resize(-> out_size) along one axis, on
    `device`; cached per size tuple and device.  Build them before a graph capture: the upload is a copy."""
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    key = (int(in_size), int(origin_size), int(crop), int(out_size), str(device))
    t = _tables.get(key)
    if t is None:
        A = crop_resize_matrix(*key[:4])
        fwd = make_bands(*_bands_of(A), n_in=key[0], device=device)
        tr = make_bands(*_bands_of(A.T), n_in=key[3], device=device)
        t = _tables[key] = CropResizeTables(fwd, tr, A, *key[:4])
    return t


def resample_sep(x, ybands, xbands, out=None):
    """y[n, c] = Ay x[n, c] Ax^T with the band tables of Ay (rows) and Ax (columns): one launch of g2s_resample_sep on
    the current stream.  x [N, C, Hin, Win] CUDA float32.  No autograd.  `out`: a contiguous float32 tensor of the
    result's shape to write into (every element is written, whatever it held)."""
    _lib.require_cuda(x)
    if x.dim() != 4 or x.dtype != torch.float32:
        raise ValueError(f"resample_sep takes a float32 [N, C, H, W] tensor, got {x.dtype} {tuple(x.shape)}")
    if (x.shape[2], x.shape[3]) != (ybands.n_in, xbands.n_in):
        raise ValueError(f"the tables read a {ybands.n_in} x {xbands.n_in} plane, the input has {tuple(x.shape[2:])}")
    if max(ybands.K, xbands.K) > MAX_TAPS:
        raise ValueError(f"{max(ybands.K, xbands.K)} taps: the kernel holds at most {MAX_TAPS}")
    if ybands.lo.device != x.device or xbands.lo.device != x.device:
        raise ValueError("the band tables are on another device than the input")
    x = x.contiguous()
    N, Cn = x.shape[:2]
    shape = (N, Cn, ybands.n_out, xbands.n_out)
    if out is not None and (tuple(out.shape) != shape or out.dtype != torch.float32 or out.device != x.device
                            or not out.is_contiguous()):
        raise ValueError(f"out must be a contiguous float32 {shape} tensor on {x.device}")
    y = torch.empty(shape, dtype=torch.float32, device=x.device) if out is None else out
    if y.numel() == 0:
        return y
    p = _lib.ptr
    _lib.check(_lib.load().g2s_resample_sep(
        p(x), p(y), N * Cn, ybands.n_in, xbands.n_in, ybands.n_out, xbands.n_out,
        p(ybands.lo), p(ybands.len), p(ybands.w), ybands.K, p(xbands.lo), p(xbands.len), p(xbands.w), xbands.K,
        _lib.stream()))
    return y


class _CropResize(Function):
    """x -> A x A^T (transposed=False) or g -> A^T g A (transposed=True).  The map is linear, so nothing is saved, and
    each node's backward is the other node: the pair differentiates to any order."""

    @staticmethod
    def forward(ctx, x, tables, transposed):
        ctx.tables, ctx.transposed = tables, transposed
        b = tables.tr if transposed else tables.fwd
        return resample_sep(x, b, b)

    @staticmethod
    def backward(ctx, g):
        return _CropResize.apply(g, ctx.tables, not ctx.transposed), None, None


def crop_resize_reference(image, origin_size, crop, size):
    """The torch composition, as the reference writes it: the specification of crop_resize."""
    image = utils.resize(image, [origin_size, origin_size])
    image = utils.crop(image, crop)
    return utils.resize(image, [size, size])


def crop_resize(image, origin_size, crop, size, fused=True):
    """resize(image, origin_size) -> centre crop to crop x crop -> resize(., size) of a square [N, C, S, S] image.
    CUDA float32 with `fused`: one launch forward, one per derivative; otherwise the torch composition."""
    if image.dim() != 4 or image.shape[2] != image.shape[3]:
        raise ValueError(f"crop_resize takes square [N, C, S, S] images, got {tuple(image.shape)}")
    if not 0 < int(crop) <= int(origin_size):
        raise ValueError(f"crop must satisfy 0 < crop <= origin_size, got crop {crop}, origin_size {origin_size}")
    if fused and image.is_cuda and image.dtype == torch.float32 and image.numel() > 0:
        tables = crop_resize_tables(image.shape[2], origin_size, crop, size, image.device)
        return _CropResize.apply(image, tables, False)
    return crop_resize_reference(image, int(origin_size), int(crop), int(size))
