"""Fit the view and light priors from a trained model.

`view_mvn.pth` / `light_mvn.pth` hold the mean and covariance of the view (6) and light (4) parameters:
ViewLightSampler draws the pseudo views and lights of step 2 from them, and steps 1 and 3 add their means to the
nets' outputs.  The reference ships the files and no code that makes them; this module makes them from a model's own
estimates over a dataset:

    mvn_fit(rows, blocks, ridge)            rows [N, D] -> MvnFit(mean, cov, tril, n); on the device ONE launch of
                                            g2s_mvn_fit (csrc/mvn.hip), on the CPU the same arithmetic in float64
    fit_view_light(model, dataset, ...)     the model's estimates [N, 10] -> one mvn_fit with blocks (6, 4)
    save_mvn(path, mean, cov)               the file format ViewLightSampler (the reference's and ours) loads

The estimates are `GAN2Shape.estimate_view_light`: the raw parameters of forward_step1, V(x) + view mean and
L(x) + light mean.  The command is gan2shape_amd.fit_view_light.
"""
import collections
import ctypes as C

import torch

from . import lib

MvnFit = collections.namedtuple("MvnFit", "mean cov tril n")

MAX_D, MAX_BLOCKS = 16, 4       # G2S_MVN_MAX_D, G2S_MVN_MAX_BLOCKS (include/g2s.h)
VIEW_LIGHT_BLOCKS = (6, 4)


def _blocks_of(blocks, D):
    blocks = (D,) if blocks is None else tuple(int(b) for b in blocks)
    if not 1 <= len(blocks) <= MAX_BLOCKS or min(blocks) < 1 or sum(blocks) != D:
        raise ValueError(f"blocks {blocks}: 1 .. {MAX_BLOCKS} positive sizes that sum to D = {D}")
    return blocks


def _pivot_error(col, blocks, ridge):
    start = 0
    for k, size in enumerate(blocks):
        if col < start + size:
            break
        start += size
    return ValueError(f"mvn_fit: the pivot of column {col} (column {col - start} of block {k}, size {size}) is not "
                      f"positive: the covariance with ridge {ridge:g} has no Cholesky factor; a larger ridge helps")


def mvn_fit_launch(rows, N, D, ld, blocks, ridge, mean, cov, tril, status):
    """The bare g2s_mvn_fit launch on tensors the caller owns (tests hand in canary views)."""
    arr = (C.c_int * len(blocks))(*blocks)
    lib.check(lib.load().g2s_mvn_fit(lib.ptr(rows), N, D, ld, arr, len(blocks), float(ridge), lib.ptr(mean),
                                     lib.ptr(cov), lib.ptr(tril), lib.ptr(status), lib.stream()))


def mvn_fit(rows, blocks=None, ridge=0.0):
    """rows [N, D] float32 -> MvnFit(mean [D], cov [D, D], tril [D, D], n), all float32 on rows' device.

    cov is the joint covariance (divisor N - 1) plus `ridge` on its diagonal; tril is block diagonal, each diagonal
    block the lower Cholesky factor of that block of cov (blocks: sizes that sum to D, default one block).  Raises
    ValueError for a non-finite input and for a block without a factor, naming the column."""
    if rows.dim() != 2 or rows.dtype != torch.float32:
        raise ValueError(f"mvn_fit: rows must be a float32 [N, D] tensor, got {rows.dtype} {tuple(rows.shape)}")
    N, D = rows.shape
    if not 1 <= D <= MAX_D or N < 2:
        raise ValueError(f"mvn_fit: needs 1 <= D <= {MAX_D} and N >= 2, got N = {N}, D = {D}")
    blocks = _blocks_of(blocks, D)
    ridge = float(ridge)
    if not ridge >= 0.0 or ridge == float("inf"):
        raise ValueError(f"mvn_fit: ridge must be finite and >= 0, got {ridge}")
    if rows.is_cuda:
        if rows.stride(1) != 1 or rows.stride(0) < D:
            rows = rows.contiguous()
        out = torch.empty(D + 2 * D * D, dtype=torch.float32, device=rows.device)
        status = torch.empty(1, dtype=torch.int32, device=rows.device)
        mean, cov, tril = out[:D], out[D:D + D * D].view(D, D), out[D + D * D:].view(D, D)
        with torch.cuda.device(rows.device):
            mvn_fit_launch(rows, N, D, rows.stride(0), blocks, ridge, mean, cov, tril, status)
        code = int(status.item())           # the one synchronisation: this is not a training path
    else:
        x = rows.double()
        code = 0 if bool(torch.isfinite(x).all()) else -1
        m = x.mean(0)
        xc = x - m
        c = (xc.t() @ xc) / (N - 1)
        c = torch.triu(c) + torch.triu(c, 1).t() + ridge * torch.eye(D, dtype=torch.float64)
        t = torch.zeros(D, D, dtype=torch.float64)
        start = 0
        for size in blocks:
            if code != 0:
                break
            sl = slice(start, start + size)
            factor, info = torch.linalg.cholesky_ex(c[sl, sl])
            if int(info) != 0:
                code = start + int(info)    # info is the 1-based order of the failing leading minor
            t[sl, sl] = factor
            start += size
        mean, cov, tril = m.float(), c.float(), t.float()
    if code == -1:
        raise ValueError("mvn_fit: the rows hold a non-finite value (inf or NaN)")
    if code != 0:
        raise _pivot_error(code - 1, blocks, ridge)
    return MvnFit(mean, cov, tril, N)


def _image_of(item):
    return item[0] if isinstance(item, (tuple, list)) else item


def estimate_rows(model, dataset, batch=64, images=None):
    """`model.estimate_view_light` over `dataset` (items: an image [3, S, S], or a tuple that starts with one) in
    batches of `batch`, the last one short -> rows [N, 10] on the model's device: view in [:, :6], light in [:, 6:],
    one row per entry of `images` (indices into the dataset, default all) in that order."""
    idx = list(range(len(dataset))) if images is None else [int(i) for i in images]
    batch = max(1, int(batch))
    device = model.device
    rows = torch.empty(len(idx), 10, dtype=torch.float32, device=device)
    for lo in range(0, len(idx), batch):
        part = idx[lo:lo + batch]
        x = torch.stack([_image_of(dataset[i]) for i in part]).to(device)
        view, light = model.estimate_view_light(x)
        rows[lo:lo + len(part), :6] = view
        rows[lo:lo + len(part), 6:] = light
    return rows


def fit_view_light(model, dataset, batch=64, images=None, ridge=0.0):
    """The model's view and light estimates over `dataset` -> (MvnFit of the joint [N, 10] rows with blocks (6, 4),
    rows): `estimate_rows`, then ONE mvn_fit.  The rows stay on the model's device; `view_of` / `light_of` slice
    the fit."""
    n = len(dataset) if images is None else len(images)
    if n < 2:
        raise ValueError(f"fit_view_light: a covariance needs at least 2 images, got {n}")
    rows = estimate_rows(model, dataset, batch, images)
    return mvn_fit(rows, VIEW_LIGHT_BLOCKS, ridge), rows


def view_of(fit):
    """(mean [6], cov [6, 6]) of the view block of a joint fit."""
    return fit.mean[:6], fit.cov[:6, :6]


def light_of(fit):
    return fit.mean[6:], fit.cov[6:, 6:]


def save_mvn(path, mean, cov):
    """{'mean': float32 CPU [D], 'cov': float32 CPU [D, D]}: what ViewLightSampler loads (weights_only=True)."""
    mean = mean.detach().to("cpu", torch.float32).contiguous().clone()
    cov = cov.detach().to("cpu", torch.float32).contiguous().clone()
    if mean.dim() != 1 or cov.shape != (mean.shape[0], mean.shape[0]):
        raise ValueError(f"save_mvn: mean {tuple(mean.shape)} and cov {tuple(cov.shape)} do not belong together")
    torch.save({"mean": mean, "cov": cov}, path)
