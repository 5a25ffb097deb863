"""Case table of tests/test_groupnorm_cases_cpu.py and tests/test_gpu_groupnorm_paths.py: GroupNorm + activation
(csrc/groupnorm.hip behind g2s_groupnorm_act_fwd / _bwd) at shapes that reach every launch path of either direction,
against the float64 restatement of oracle/nets.py.  Importable without a GPU.

A case is (name, shape (B, C, H, W), groups, act, slope, offset, scale): act = 0 is no activation, act = 1 with
slope 0 is ReLU, otherwise leaky ReLU.  Inputs are seeded numpy draws, rounded to float32 (the reference sees the
rounded values): x = offset + scale * N(0, 1), gamma, beta, gy ~ N(0, 1).

The paths (`paths` restates the dispatcher):

  forward   fused       one workgroup holds a group in registers              n = C/G * H*W <= 65536
            two-launch  gn_stats over 4096-element slices, gn_apply merges them (Chan) and normalises
  backward  fused       B = 1, n <= 16384, H*W % 256 == 0, C/G <= 16: wave k of the workgroup owns channel k
            two-launch  gn_bwd_sums per (b, c), gn_bwd_apply

  f_over4   n = 65540: 17 slices, the last one is a single float4
  f_ragged  n = 69312: slices cross channel borders (H*W = 23104), ragged last slice, B and G above 1
  f_exact   n = 131072: 32 full slices
  b_cpg1    one channel per group: one active wave, L = H*W / 256 = 1
  b_cpg16   16 channels per group: all 16 waves are channels
  b_cpg5    n = 5120: 2 passes, the second fills 256 of 1024 threads; b_cpg5_far: the same at x = 50 + 0.5 N(0, 1),
            where a one-pass variance would cancel
  b_cpg3    n = 12288: 3 passes, L = 16
  b_L64     n = 16384, the limit: 4 passes, L = 64
  out_B, out_cpg, out_hw, out_n    one step outside each condition of the fused backward: B = 2, 17 channels per
            group, H*W = 260, n = 18432

Sign flips.  Where the float64 pre-activation lies within GATE of zero a float32 kernel may take the other slope.
Those elements get gy = 0, so that a flipped slope moves no gradient, and are left out of the forward comparison;
`data` checks that they are at most MAX_GATED of a case.  Cases without an activation have no such elements.

Yardstick.  `data` also runs the same expression in torch's CPU float32 (F.group_norm + leaky_relu, autograd) and
records, per output (y, dx, dgamma, dbeta), e32 = max|float32 - float64| / max|float64|: the error of a plain float32
restatement.  The kernels are held to RATIO[output] * e32, and never to more than the bounds the older test of
tests/test_gpu_kernels.py uses (FLOOR)."""
import functools
import zlib

import numpy as np

from oracle import nets

EPS = 1e-5
GATE = 1e-4          # |float64 pre-activation| below which an element counts as able to flip
MAX_GATED = 1e-3     # at most 0.1 % of a case's elements
OUTPUTS = ("y", "dx", "dgamma", "dbeta")
FLOOR = dict(y=2e-6, dx=2e-5, dgamma=2e-5, dbeta=2e-5)      # of max|ref|: test_groupnorm_act_vs_oracle's bounds
RATIO = dict(y=4.0, dx=4.0, dgamma=4.0, dbeta=4.0)          # kernel error <= RATIO * e32
RELU, LEAKY, NONE =(1, 0.0), (1, 0.2), (0, 0.0)

CASES = [  # name, shape, groups, act, slope, offset, scale
    ("f_over4", (2, 2, 145, 452), 2, *RELU, 0.5, 2.0),
    ("f_ragged", (2, 6, 152, 152), 2, *NONE, 0.5, 2.0),
    ("f_exact", (1, 4, 256, 256), 2, *LEAKY, 0.5, 2.0),
    ("b_cpg1", (1, 3, 16, 16), 3, *RELU, 0.5, 2.0),
    ("b_cpg16", (1, 32, 16, 16), 2, *LEAKY, 0.5, 2.0),
    ("b_cpg5", (1, 10, 32, 32), 2, *NONE, 0.5, 2.0),
    ("b_cpg5_far", (1, 10, 32, 32), 2, *RELU, 50.0, 0.5),
    ("b_cpg3", (1, 6, 64, 64), 2, *LEAKY, 0.5, 2.0),
    ("b_L64", (1, 2, 128, 128), 2, *RELU, 0.5, 2.0),
    ("out_B", (2, 32, 16, 16), 2, *NONE, 0.5, 2.0),
    ("out_cpg", (1, 34, 16, 16), 2, *LEAKY, 0.5, 2.0),
    ("out_hw", (1, 8, 10, 26), 2, *RELU, 0.5, 2.0),
    ("out_n", (1, 16, 48, 48), 2, *LEAKY, 0.5, 2.0),
]
NAMES = [c[0] for c in CASES]
CASE = {c[0]: c for c in CASES}
assert len(CASE) == len(CASES)

# what the table is meant to reach: name -> (forward path, backward path)
EXPECTED_PATHS = dict(f_over4=("two", "two"), f_ragged=("two", "two"), f_exact=("two", "two"),
                      b_cpg1=("fused", "fused"), b_cpg16=("fused", "fused"), b_cpg5=("fused", "fused"),
                      b_cpg5_far=("fused", "fused"), b_cpg3=("fused", "fused"), b_L64=("fused", "fused"),
                      out_B=("fused", "two"), out_cpg=("fused", "two"), out_hw=("fused", "two"), out_n=("fused", "two"))


def paths(shape, groups):
    """(forward path, backward path) the dispatcher of csrc/groupnorm.hip takes, each "fused" or "two"."""
    B, C, H, W = shape
    hw, cpg = H * W, C // groups
    n = cpg * hw
    # g2s_groupnorm_act_fwd: `if (p.n <= GNF_MAX_N)`, GNF_MAX_N = GNF_THREADS * GNF_MAX4 * 4 = 1024 * 16 * 4
    fwd = "fused" if n <= 1024 * 16 * 4 else "two"
    # g2s_groupnorm_act_bwd: `if (B == 1 && p.n <= GNB_MAX_N && HW % 256 == 0 && C / G <= 16)`, GNB_MAX_N = 16384
    bwd = "fused" if B == 1 and n <= 16384 and hw % 256 == 0 and cpg <= 16 else "two"
    return fwd, bwd


def kind(act, slope):
    return "none" if not act else ("relu" if slope == 0.0 else "leaky")


def inputs(name):
    """x, gamma, beta, gy as float32 numpy draws of this case, before any gating of gy."""
    _, shape, _, _, _, offset, scale = CASE[name]
    rng = np.random.default_rng([20251, zlib.crc32(name.encode())])
    x = (offset + scale * rng.standard_normal(shape)).astype(np.float32)
    gamma = rng.standard_normal(shape[1]).astype(np.float32)
    beta = rng.standard_normal(shape[1]).astype(np.float32)
    gy = rng.standard_normal(shape).astype(np.float32)
    return x, gamma, beta, gy


def rel_err(got, want, keep=None):
    """max|got - want| / max|want|, over the elements of `keep` (all when None); `want` is float64."""
    err = np.abs(np.asarray(got, np.float64) - want)
    if keep is not None:
        err = err[keep]
    return float(err.max() / np.abs(want).max())


def bound(name, output):
    """What max|kernel - float64| / max|float64| of this output may be."""
    return min(RATIO[output] * data(name)["e32"][output], FLOOR[output])


def _torch_f32(x, gamma, beta, gy, groups, act, slope):
    import torch
    import torch.nn.functional as F
    xt, gt, bt = (torch.tensor(a, dtype=torch.float32, requires_grad=True) for a in (x, gamma, beta))
    y = F.group_norm(xt, groups, gt, bt, EPS)
    if act:
        y = F.leaky_relu(y, slope)
    y.backward(torch.tensor(gy, dtype=torch.float32))
    return dict(y=y.detach().numpy(), dx=xt.grad.numpy(), dgamma=gt.grad.numpy(), dbeta=bt.grad.numpy())


@functools.lru_cache(maxsize=None)
def data(name):
    """Everything the tests need of a case, computed once: inputs (gy gated), the float64 reference of every output,
    `keep` (the elements of y that are compared), the gated fraction and e32 per output.  Arrays are read-only."""
    _, shape, groups, act, slope, _, _ = CASE[name]
    x, gamma, beta, gy = inputs(name)
    pre = nets.group_norm_act(x, gamma, beta, groups, EPS, False)
    gated = (np.abs(pre) < GATE) if act else np.zeros(shape, bool)
    gy[gated] = 0.0
    ref = dict(y=nets.group_norm_act(x, gamma, beta, groups, EPS, bool(act), slope))
    ref["dx"], ref["dgamma"], ref["dbeta"] = nets.group_norm_act_grad(x, gamma, beta, gy, groups, EPS, bool(act), slope)
    keep = ~gated
    r32 = _torch_f32(x, gamma, beta, gy, groups, act, slope)
    e32 = {k: rel_err(r32[k], ref[k], keep if k == "y" else None) for k in OUTPUTS}
    for a in (x, gamma, beta, gy, keep, *ref.values()):
        a.setflags(write=False)
    return dict(x=x, gamma=gamma, beta=beta, gy=gy, ref=ref, keep=keep, gated=float(gated.mean()), e32=e32)
