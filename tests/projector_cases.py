"""Cases of the latent projector's tests (tests/golden/make_projector_golden.py writes their reference results to
tests/golden/projector.npz; test_projector_cpu.py and test_gpu_projector.py read them), and a torch restatement of
the two noise functions in this package's own words — the op-by-op form the GPU tests compare against where the
fixture has no entry (sides 256 and 512, the op-by-op projector step)."""
import numpy as np
import torch
import torch.nn.functional as F

LR_T = [0.0, 0.01, 0.05, 0.5, 0.75, 0.9, 0.999]
SIDE_LISTS = {"pyr": (4, 8, 8, 16, 16, 32, 32), "s64": (64,)}
BATCHES = (1, 3)
KINDS = ("white", "corr")
N_SEEDS = 16            # ref_fp32_err is the maximum over this many inputs: a lucky draw does not set the bar
CASES = [(lst, B, kind) for lst in SIDE_LISTS for B in BATCHES for kind in KINDS]

G_CFG = dict(size=16, style_dim=32, n_mlp=3, channel_multiplier=1, seed=123)   # two up-sampling octaves: sides 4, 8, 8, 16, 16


def case_name(lst, B, kind):
    return f"{lst}.b{B}.{kind}"


def make_maps(sides, B, kind, seed=0):
    """float32 numpy maps [B, 1, S, S]: white noise, or z + 0.5 roll(z, 1, x) + 0.5 roll(z, 1, y) — neighbours
    correlate, so both means are O(1) and a wrong wrap or shift shows."""
    rng = np.random.default_rng([seed, B, len(sides), sum(sides)])
    out = []
    for S in sides:
        z = rng.standard_normal((B, 1, S, S))
        if kind == "corr":
            z = z + 0.5 * np.roll(z, 1, 3) + 0.5 * np.roll(z, 1, 2)
        out.append(z.astype(np.float32))
    return out


def generator_inputs(seed=0):
    """(w [1, style_dim], noise maps, upstream gradient [1, 3, 16, 16]) of the size-16 generator case, float32 numpy."""
    rng = np.random.default_rng([77, seed])
    w = rng.standard_normal((1, G_CFG["style_dim"])).astype(np.float32)
    noises = [rng.standard_normal((1, 1, s, s)).astype(np.float32) for s in (4, 8, 8, 16, 16)]
    gy = rng.standard_normal((1, 3, G_CFG["size"], G_CFG["size"])).astype(np.float32)
    return w, noises, gy


def fill_deterministic(module, seed):
    """make_golden.fill_deterministic: seeded values for every parameter and buffer in sorted state-dict order (the
    fixture script fills the reference module the same way, so no weights are stored)."""
    g = torch.Generator().manual_seed(seed)
    sd = module.state_dict()
    with torch.no_grad():
        for k in sorted(sd.keys()):
            t = sd[k]
            if not t.is_floating_point() or k.endswith("kernel"):
                continue
            v = torch.randn(t.shape, generator=g)
            if "modulation.bias" in k:
                v = 1 + 0.1 * v
            elif k.endswith("bias") or "noise" in k:
                v = 0.1 * v
            t.copy_(v)


def fixture_generator(sg2, size=None, style_dim=None, n_mlp=None, seed=None):
    """This package's Generator with the fixture's weights (or the same recipe at another size), frozen, on the CPU."""
    from model_cases import prepare_generator
    G = sg2.Generator(size or G_CFG["size"], style_dim or G_CFG["style_dim"], n_mlp or G_CFG["n_mlp"],
                      channel_multiplier=G_CFG["channel_multiplier"])
    prepare_generator(G, seed or G_CFG["seed"], fill_deterministic)
    return G.eval().requires_grad_(False)


def l2_rel(a, ref):
    a, ref = a.double(), ref.double()
    return float((a - ref).norm() / ref.norm())


# ------------------------------------------------------------------------------------- torch restatement
def _shift(n, dim):
    """n(.., i - 1, ..) with wrap-around along `dim`, by slicing."""
    last = n.narrow(dim, n.shape[dim] - 1, 1)
    return torch.cat([last, n.narrow(dim, 0, n.shape[dim] - 1)], dim)


def noise_regularize(noises):
    total = 0
    for n in noises:
        while True:
            total = total + (n * _shift(n, 3)).mean() ** 2 + (n * _shift(n, 2)).mean() ** 2
            if n.shape[-1] <= 8:
                break
            n = F.avg_pool2d(n, 2)
    return total


def noise_normalize_(noises):
    with torch.no_grad():
        for n in noises:
            n.copy_((n - n.mean()) / n.std(unbiased=True))


def regularize_with_grads(noises, dtype):
    """(value, [gradient per map]) of noise_regularize above at `dtype`."""
    xs = [n.detach().to(dtype).requires_grad_(True) for n in noises]
    v = noise_regularize(xs)
    return v.detach(), list(torch.autograd.grad(v, xs))
