"""Shared statements of the generator-training tests (no GPU needed): inputs, float64-capable torch statements of the
two generator losses, the two passes of a generator step and the EMA, and the bounds of the whole-generator tests.
Used by tests/golden/make_gtrain_golden.py (on the reference's Generator and Discriminator) and by the tests (on this
package's).  Weights come from dtrain_cases.draw_like, so none are stored."""
import math

import numpy as np
import torch
import torch.nn.functional as F
from torch import autograd

import dtrain_cases as dc

# ------------------------------------------------------------------------------------------------------ bounds
# As dtrain_cases: whole-generator quantities are held to MULTIPLE x e32 with dtrain_cases.bound's floor, e32 the
# distance of the reference's float32 CPU run from its float64 run.  MEASURED holds the largest error / max(e32, one
# float32 rounding) over cases and stored quantities seen on an MI355X, for the float32 torch route of this package
# (switch off; it has no second order, so no path figure) and for the new route per pass and for the two trainer steps.
# The torch route's 10.4 is the gradient norms of B = 4.  The new route's 11.7 is the loss of the mixing case: an error of
# 5.2e-7 on 0.41, of the size of the 3.0e-7 at B = 4, against the smallest e32 of the three cases (4.4e-8, 1.8 roundings);
# every other quantity of the new route is within 3.5.  16 is the smallest of 2, 4, 8, 16 it meets everywhere.
MULTIPLE = 16
MEASURED = {
    "torch_route": {"nonsaturating": 10.44, "path": None},
    "new_route": {"nonsaturating": 11.72, "path": 2.88, "trainer": 2.40},
}
EPS32 = float(np.finfo(np.float32).eps)


def bound(want, e32):
    floor = 0.5 * EPS32 * float(np.abs(np.asarray(want, dtype=np.float64)).max())
    return MULTIPLE * max(float(e32), floor)


SIZE, STYLE_DIM, N_MLP, CHANNEL_MULTIPLIER = 16, 64, 2, 1
# name: (batch, latents per sample, inject_index)
CASES = {"b4": (4, 1, None), "b2": (2, 1, None), "mix": (2, 2, 3)}
G_SEED, D_SEED, PROBE_SEED, INPUT_SEED = 3025, 3026, 3027, 3028
PATH_REGULARIZE, G_REG_EVERY = 2.0, 4
EMA_DECAY = 0.5 ** (32 / (10 * 1000))
NOISE_SIDES = [4, 8, 8, 16, 16]          # G(16): num_layers = 5


def inputs(name, seed=INPUT_SEED):
    """float32 arrays: zs (list of [B, STYLE_DIM]), noise maps (list of [1, 1, r, r]), image noise [B, 3, S, S]."""
    B, n_lat, _ = CASES[name]
    rs = np.random.RandomState(seed + 17 * B + n_lat)
    zs = [rs.standard_normal((B, STYLE_DIM)).astype(np.float32) for _ in range(n_lat)]
    maps = [rs.standard_normal((1, 1, r, r)).astype(np.float32) for r in NOISE_SIDES]
    img_noise = rs.standard_normal((B, 3, SIZE, SIZE)).astype(np.float32)
    return zs, maps, img_noise


def to(arrays, like):
    return [torch.from_numpy(a).to(like) for a in arrays]


# -------------------------------------------------------------------------------------------------- statements
def g_nonsaturating(fake_pred):
    return F.softplus(-fake_pred).mean()


def path_lengths_of(grad):
    return torch.sqrt(grad.pow(2).sum(2).mean(1))


def path_penalty(grad, mean_path_length, decay=0.01):
    lengths = path_lengths_of(grad)
    path_mean = mean_path_length + decay * (lengths.mean() - mean_path_length)
    return (lengths - path_mean).pow(2).mean(), path_mean.detach(), lengths


def g_path_regularize(fake_img, latents, mean_path_length, decay=0.01, noise=None):
    noise = noise / math.sqrt(fake_img.shape[2] * fake_img.shape[3])
    grad, = autograd.grad(outputs=(fake_img * noise).sum(), inputs=latents, create_graph=True)
    return path_penalty(grad, mean_path_length, decay)


def accumulate(model1, model2, decay=0.999):
    par1, par2 = dict(model1.named_parameters()), dict(model2.named_parameters())
    for k in par1.keys():
        par1[k].data.mul_(decay).add_(par2[k].data, alpha=1 - decay)


def _grads(g):
    return {n: (torch.zeros_like(p) if p.grad is None else p.grad.detach().clone()) for n, p in g.named_parameters()}


def nonsaturating_pass(g, d, zs, maps, inject, loss_fn=g_nonsaturating):
    """train.py:225-237.  -> dict(image, fake_pred, loss, grads)."""
    fake_img, _ = g(zs, inject_index=inject, noise=maps)
    fake_pred = dc._pred(d(fake_img))
    loss = loss_fn(fake_pred)
    g.zero_grad()
    loss.backward()
    return dict(image=fake_img.detach(), fake_pred=fake_pred.detach(), loss=loss.detach(), grads=_grads(g))


def path_pass(g, zs, maps, inject, img_noise, mean_path_length=0.0, loss_fn=g_path_regularize):
    """train.py:242-257.  -> dict(image, lengths, path_mean, penalty, grads)."""
    fake_img, latents = g(zs, return_latents=True, inject_index=inject, noise=maps)
    penalty, path_mean, lengths = loss_fn(fake_img, latents, mean_path_length, noise=img_noise)
    g.zero_grad()
    (PATH_REGULARIZE * G_REG_EVERY * penalty + 0 * fake_img[0, 0, 0, 0]).backward()
    return dict(image=fake_img.detach(), lengths=lengths.detach(), path_mean=path_mean.detach(),
                penalty=penalty.detach(), grads=_grads(g))


def summarize(grads, probe):
    return dc.summarize(grads, probe)


def projections(module, probe):
    """[P]: the inner product of every parameter with the probe tensor of its name."""
    return np.array([float((p.detach().double().cpu() * torch.from_numpy(probe[n])).sum())
                     for n, p in module.named_parameters()])


def trainer_inputs():
    """Two steps (i = 0 with the path pass, i = 1 without): case b4's inputs for the non-saturating passes, case b2's
    for the path pass (path_batch_shrink = 2), other seeds."""
    return [(inputs("b4", INPUT_SEED + 100), inputs("b2", INPUT_SEED + 150), 0),
            (inputs("b4", INPUT_SEED + 200), None, 1)]


def reference_trainer(g, g_ema, d, like, lr=0.002):
    """The reference's loop (train.py:222-268) with torch.optim.Adam on `g` over trainer_inputs()."""
    c = G_REG_EVERY / (G_REG_EVERY + 1)
    opt = torch.optim.Adam(g.parameters(), lr=lr * c, betas=(0 ** c, 0.99 ** c))
    for p in d.parameters():
        p.requires_grad = False
    mean_path = 0.0
    for (zs, maps, _), path_in, i in trainer_inputs():
        nonsaturating_pass(g, d, to(zs, like), to(maps, like), None)
        opt.step()
        if i % G_REG_EVERY == 0:
            pz, pmaps, pimg = path_in
            out = path_pass(g, to(pz, like), to(pmaps, like), None, to([pimg], like)[0], mean_path)
            mean_path = out["path_mean"]
            opt.step()
        accumulate(g_ema, g, EMA_DECAY)
    return g, g_ema
