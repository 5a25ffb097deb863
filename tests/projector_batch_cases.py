"""Cases of the batched projector's tests (tests/golden/make_projector_batch_golden.py writes the reference's results
to tests/golden/projector_batch.npz; test_gpu_synth_batch.py and test_projector_batch_cpu.py read them).  Inputs are
not stored: they come from the seeds below.  The generator is the size-16 fixture of projector_cases.py."""
import numpy as np
import torch

import projector_cases as pc

N_SEEDS = pc.N_SEEDS     # ref_fp32_err is the maximum over this many inputs
SIDES = (4, 8, 8, 16, 16)
N_LATENT = 6             # size 16: log2(16) * 2 - 2

# ------------------------------------------------------------------------------------------- the generator, B = 3
GEN_B = 3
MODES = ("w", "wp")      # one w per sample; one w per sample and layer (w_plus)


def generator_inputs(mode, seed=0):
    """(latent [3, D] or [3, n_latent, D], per-sample maps [3, 1, s, s], cotangent [3, 3, 16, 16]), float32 numpy."""
    D = pc.G_CFG["style_dim"]
    rng = np.random.default_rng([1801, MODES.index(mode), seed])
    w = rng.standard_normal((GEN_B, D)).astype(np.float32)
    if mode == "wp":
        w = (w[:, None] + 0.3 * rng.standard_normal((GEN_B, N_LATENT, D))).astype(np.float32)
    noises = [rng.standard_normal((GEN_B, 1, s, s)).astype(np.float32) for s in SIDES]
    gy = rng.standard_normal((GEN_B, 3, pc.G_CFG["size"], pc.G_CFG["size"])).astype(np.float32)
    return w, noises, gy


def generator_keys():
    return ["img", "glatent"] + [f"gnoise{k}" for k in range(len(SIDES))]


# ------------------------------------------------------------------------------------------- the loop, B = 2
LOOP_B, LOOP_STEPS = 2, 3
LOOP = dict(lr=0.1, noise=0.05, noise_ramp=0.75, noise_regularize=1e5, mse=0.0)
LATENT_STD = 0.8         # the `latent_std` of the run (a fixed number: no 10000-sample statistics in a test)
LOOP_TORCH_SEED = 4242


def loop_inputs(seed=0):
    """What the three steps at B = 2 start from and draw, float32 torch tensors: the target images [2, 3, 16, 16],
    the mask of the stand-in perceptual term, latent_mean [D], and — from ONE torch.Generator in the order project_batch
    draws them — the initial maps [2, 1, s, s], then one jitter draw [2, D] per step."""
    D = pc.G_CFG["style_dim"]
    rng = np.random.default_rng([1802, seed])
    target = torch.from_numpy(np.tanh(rng.standard_normal((LOOP_B, 3, 16, 16))).astype(np.float32))
    mask = torch.from_numpy((rng.random((1, 3, 16, 16)) < 0.7).astype(np.float32))
    latent_mean = torch.from_numpy((0.3 * rng.standard_normal(D)).astype(np.float32))
    g = loop_generator(seed)
    maps = [torch.empty(LOOP_B, 1, s, s).normal_(generator=g) for s in SIDES]
    jitter = [torch.randn(LOOP_B, D, generator=g) for _ in range(LOOP_STEPS)]
    return dict(target=target, mask=mask, latent_mean=latent_mean, maps=maps, jitter=jitter)


def loop_generator(seed=0):
    """The torch.Generator whose stream loop_inputs reads: hand a fresh one to project_batch."""
    return torch.Generator().manual_seed(LOOP_TORCH_SEED + seed)


def standin_percept(mask):
    """The fixed differentiable stand-in for LPIPS (its weights are not available offline): a masked L2 to the target,
    with PerceptualLoss's call shape (pred, target) -> [B, 1, 1, 1]."""
    def percept(pred, target):
        m = mask.to(pred.dtype)
        return (((pred - target) ** 2) * m).mean((1, 2, 3)).view(-1, 1, 1, 1)
    return percept
