"""Shared statements of the discriminator-training tests (no GPU needed): the weight rule, float64-capable torch
statements of the minibatch stddev, the two losses and the two passes of a training step, and the bounds of the
whole-discriminator tests.  Used by tests/golden/make_dtrain_golden.py (on the reference's Discriminator) and by the
tests (on this package's), so no weights are stored."""
import numpy as np
import torch
import torch.nn.functional as F
from torch import autograd

# ------------------------------------------------------------------------------------------------------ bounds
# Whole-discriminator quantities are held to MULTIPLE x e32, e32 being the distance of the reference's own float32 CPU
# run from its float64 run for that quantity (stored in the fixture).  A second float32 summation order (Winograd and
# MFMA tiles instead of the CPU's GEMM) cannot be expected inside 1 x that distance; the ADA precedent took the
# smallest of 2, 4, 8 the new route meets on the device.  MEASURED holds, per pass, the largest ratio error / e32 over
# cases and stored quantities seen on an MI355X for the float32 torch route of this package (switch off, torch's
# weight gradient; it has no second order, so no R1 figure) and for the new route.
# The new route met 4 on both passes and missed it on one tensor of the two trainer steps (a bias of 512 entries at
# 4.97: Adam with beta1 = 0 moves a weight by lr * g / (|g| + eps), which turns a relative gradient error into an
# absolute weight error wherever g is small); 8 is the smallest of 2, 4, 8 it meets everywhere.
MULTIPLE = 8
MEASURED = {
    "torch_route": {"logistic": 1.93, "r1": None},
    "new_route": {"logistic": 2.34, "r1": 3.72, "trainer": 4.97},
}

EPS32 = float(np.finfo(np.float32).eps)


def bound(want, e32):
    """MULTIPLE x e32, with e32 no smaller than the rounding of the exact value to float32 (half a spacing at the
    quantity's largest entry).  A scalar's e32 can fall below that by luck — the reference's float32 loss at B = 2 sits
    6.4e-9 from its float64 value, a nineteenth of the float32 spacing at 1.32 — and no float32 result, whose last
    bit moves with the summation order, can be held to a multiple of such a figure: the device result there is 0 to 2
    spacings away from run to run."""
    floor = 0.5 * EPS32 * float(np.abs(np.asarray(want, dtype=np.float64)).max())
    return MULTIPLE * max(float(e32), floor)


CASES = {"b8": 8, "b4": 4, "b2": 2}     # D(16), channel_multiplier 1: two stddev groups, one group, G = 2
SIZE, CHANNEL_MULTIPLIER = 16, 1
WEIGHT_SEED, PROBE_SEED, IMAGE_SEED = 2025, 2026, 2027
R1, D_REG_EVERY = 10.0, 16


# ------------------------------------------------------------------------------------------------- weight rule
def draw_like(module, seed):
    """{name: float64 array}: one numpy.random.RandomState(seed) draw per parameter, in named_parameters order;
    standard normal for weights, 0.1 x that for 1-D parameters (biases)."""
    rs = np.random.RandomState(seed)
    out = {}
    for name, p in module.named_parameters():
        v = rs.standard_normal(tuple(p.shape))
        out[name] = 0.1 * v if p.dim() == 1 else v
    return out


def fill_weights(module, seed=WEIGHT_SEED):
    with torch.no_grad():
        for name, v in draw_like(module, seed).items():
            p = dict(module.named_parameters())[name]
            p.copy_(torch.from_numpy(v).to(p.dtype))
    return module


def images(B, seed=IMAGE_SEED):
    """(real, fake) float32 arrays [B, 3, SIZE, SIZE] in about [-1, 1]."""
    rs = np.random.RandomState(seed + B)
    shape = (B, 3, SIZE, SIZE)
    return (np.tanh(rs.standard_normal(shape)).astype(np.float32),
            np.tanh(0.7 * rs.standard_normal(shape) + 0.2).astype(np.float32))


# -------------------------------------------------------------------------------------------------- statements
def mbstd(x, feat=1, group=4):
    """stylegan2-pytorch/model.py:756-765 for `feat` feature blocks: [B, C, H, W] -> [B, C + feat, H, W]."""
    B, C, H, W = x.shape
    G = min(B, group)
    s = x.view(G, -1, feat, C // feat, H, W)
    s = torch.sqrt(s.var(0, unbiased=False) + 1e-8)
    s = s.mean([2, 3, 4], keepdims=True).squeeze(2)
    return torch.cat([x, s.repeat(G, 1, H, W)], 1)


def d_logistic(real_pred, fake_pred):
    return F.softplus(-real_pred).mean() + F.softplus(fake_pred).mean()


def r1_per_sample(grad):
    return grad.pow(2).reshape(grad.shape[0], -1).sum(1)


def _pred(out):
    return out[0] if isinstance(out, (tuple, list)) else out


def _grads(d):
    return {name: p.grad.detach().clone() for name, p in d.named_parameters()}


def logistic_pass(d, real, fake, loss_fn=d_logistic):
    """train.py:185-194: the gradients of the logistic loss.  -> dict(real_pred, fake_pred, loss, grads)."""
    fake_pred = _pred(d(fake))
    real_pred = _pred(d(real))
    loss = loss_fn(real_pred, fake_pred)
    d.zero_grad()
    loss.backward()
    return dict(real_pred=real_pred.detach(), fake_pred=fake_pred.detach(), loss=loss.detach(), grads=_grads(d))


def r1_pass(d, real, r1=R1, every=D_REG_EVERY, loss_fn=None):
    """train.py:203-216.  -> dict(real_pred, grad_real, per_sample, r1, grads).  loss_fn(real_pred, real_img): a
    d_r1_loss to use instead of the statement (per_sample is then recomputed from its grad_real)."""
    real = real.detach().requires_grad_(True)
    real_pred = _pred(d(real))
    if loss_fn is None:
        grad_real, = autograd.grad(real_pred.sum(), real, create_graph=True)
        penalty = r1_per_sample(grad_real).mean()
    else:
        seen = {}
        orig = autograd.grad

        def spy(*a, **k):
            seen["g"] = orig(*a, **k)
            return seen["g"]
        autograd.grad = spy
        try:
            penalty = loss_fn(real_pred, real)
        finally:
            autograd.grad = orig
        grad_real = seen["g"][0]
    d.zero_grad()
    (r1 / 2 * penalty * every + 0 * real_pred[0]).backward()
    return dict(real_pred=real_pred.detach(), grad_real=grad_real.detach(),
                per_sample=r1_per_sample(grad_real.detach()), r1=penalty.detach(), grads=_grads(d))


def summarize(grads, probe):
    """(norms [P], projections [P]) in named_parameters order: the per-tensor norm of each gradient and its inner
    product with the probe tensor of the same name."""
    names = list(grads)
    norms = np.array([float(grads[n].double().norm()) for n in names])
    proj = np.array([float((grads[n].double().cpu() * torch.from_numpy(probe[n])).sum()) for n in names])
    return norms, proj


def reference_trainer(d, steps, lr=0.002, r1=R1, every=D_REG_EVERY):
    """The reference's loop (train.py:185-218) with torch.optim.Adam on `d` for `steps` = [(real, fake, i), ...]."""
    c = every / (every + 1)
    opt = torch.optim.Adam(d.parameters(), lr=lr * c, betas=(0 ** c, 0.99 ** c))
    for real, fake, i in steps:
        logistic_pass(d, real, fake)
        opt.step()
        if i % every == 0:
            r1_pass(d, real, r1, every)
            opt.step()
    return {name: p.detach().clone() for name, p in d.named_parameters()}
