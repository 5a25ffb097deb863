"""Cases, float64 oracle and error bounds shared by test_view_light_cpu.py and test_gpu_view_light.py.

Oracle (numpy float64): rows.mean(0), np.cov(rows, rowvar=False) (+ ridge on the diagonal), np.linalg.cholesky per
diagonal block.  Yardstick: the same composition in float32 torch on the CPU (rows.mean(0), torch.cov(rows.T),
torch.linalg.cholesky per block).  mvn_fit accumulates in double and rounds once, so for each output its max error
against the oracle is held to 1x the yardstick's max error; where the yardstick's error is zero or its Cholesky
fails, to 4 eps_f32 max|oracle| (one float32 rounding of a double result is eps / 2 relative; the rest is slack).

The rows are seeded draws: z A + offset with a fixed random mixing matrix A, so the columns correlate across the
blocks.  N = 3 with a 6-wide block has a covariance of rank 2, which no arithmetic can factor: that case carries a
ridge (an input of the kernel like any other; oracle and yardstick add the same one).
"""
import numpy as np
import torch

EPS32 = float(np.finfo(np.float32).eps)

# name, N, D, blocks, ld (None: D), ridge
CASES = [
    ("n2_d1", 2, 1, (1,), None, 0.0),                     # smallest input
    ("n3_d10", 3, 10, (6, 4), None, 1e-3),                # fewer rows than threads, more columns than rows per thread
    ("n255_d10", 255, 10, (6, 4), None, 0.0),             # either side of one row per thread
    ("n256_d10", 256, 10, (6, 4), None, 0.0),
    ("n257_d10", 257, 10, (6, 4), None, 0.0),
    ("n1000_d16", 1000, 16, (16,), None, 0.0),            # the widest D
    ("n1000_d10_ld12", 1000, 10, (6, 4), 12, 0.0),        # strided rows, NaN in the padding columns
    ("n4099_d10_4blocks", 4099, 10, (3, 3, 2, 2), None, 0.0),
    ("offset", 1000, 10, (6, 4), None, 0.0),              # rows 1000 + 0.01 z: a one-pass sum of squares cancels
]
IDS = [c[0] for c in CASES]


def rows_of(name):
    """float32 [N, ld] (read-only): columns D .. ld - 1 hold NaN and are never to be read."""
    i = IDS.index(name)
    _, N, D, _blocks, ld, _ridge = CASES[i]
    rng = np.random.default_rng(1000 + i)
    z = rng.standard_normal((N, D))
    if name == "offset":
        x = 1000.0 + 0.01 * z
    else:
        A = rng.standard_normal((D, D)) / np.sqrt(D) + 0.5 * np.eye(D)
        x = z @ A + rng.uniform(-2, 2, D)
    full = np.full((N, ld or D), np.nan, np.float32)
    full[:, :D] = x.astype(np.float32)
    full.setflags(write=False)
    return full


def block_slices(blocks):
    out, start = [], 0
    for size in blocks:
        out.append(slice(start, start + size))
        start += size
    return out


def oracle(rows, blocks, ridge=0.0):
    """rows [N, D] (any float dtype) -> dict(mean, cov, tril) in float64."""
    x = np.asarray(rows, np.float64)
    D = x.shape[1]
    cov = np.cov(x, rowvar=False).reshape(D, D) + ridge * np.eye(D)
    tril = np.zeros((D, D))
    for sl in block_slices(blocks):
        tril[sl, sl] = np.linalg.cholesky(cov[sl, sl])
    return {"mean": x.mean(0), "cov": cov, "tril": tril}


def yardstick(rows, blocks, ridge=0.0):
    """The float32 torch composition on the CPU -> dict(mean, cov, tril); tril is None where a Cholesky fails."""
    x = torch.from_numpy(np.array(rows, dtype=np.float32))      # a copy: the case data is read-only
    D = x.shape[1]
    cov = torch.cov(x.t()).reshape(D, D) + torch.tensor(ridge, dtype=torch.float32) * torch.eye(D)
    tril = torch.zeros(D, D)
    for sl in block_slices(blocks):
        factor, info = torch.linalg.cholesky_ex(cov[sl, sl])
        if int(info) != 0 or not bool(torch.isfinite(factor).all()):
            tril = None
            break
        tril[sl, sl] = factor
    return {"mean": x.mean(0).numpy(), "cov": cov.numpy(), "tril": None if tril is None else tril.numpy()}


def bounds(rows, blocks, ridge=0.0, want=None):
    """Per output: the scalar bound on max|got - oracle| (docstring of this module)."""
    want = oracle(rows, blocks, ridge) if want is None else want
    ref = yardstick(rows, blocks, ridge)
    out = {}
    for key in ("mean", "cov", "tril"):
        err = None if ref[key] is None else float(np.abs(ref[key].astype(np.float64) - want[key]).max())
        out[key] = err if err else 4 * EPS32 * float(np.abs(want[key]).max())
    return out


def check_fit(got, rows, blocks, ridge, what):
    """got: dict(mean, cov, tril) of arrays.  Asserts each within its bound; returns {output: error / bound}."""
    want = oracle(rows, blocks, ridge)
    bound = bounds(rows, blocks, ridge, want)
    ratios = {}
    for key in ("mean", "cov", "tril"):
        err = float(np.abs(np.asarray(got[key], np.float64) - want[key]).max())
        ratios[key] = err / bound[key]
        print(f"{what} {key}: max error {err:.3e}, bound {bound[key]:.3e}, ratio {ratios[key]:.3f}")
    for key, r in ratios.items():
        assert r <= 1.0, (what, key, r)
    return ratios


def check_structure(cov, tril, blocks, what):
    """cov symmetric bit for bit; tril exactly 0.0 above the diagonal and outside the diagonal blocks."""
    cov, tril = np.asarray(cov), np.asarray(tril)
    assert np.array_equal(cov.view(np.uint32), cov.T.copy().view(np.uint32)), f"{what}: cov is not symmetric"
    inside = np.zeros(tril.shape, bool)
    for sl in block_slices(blocks):
        inside[sl, sl] = True
    inside &= np.tril(np.ones(tril.shape, bool))
    assert (tril[~inside] == 0.0).all() and not np.signbit(tril[~inside]).any(), f"{what}: tril outside the blocks"


def offset_oracle_error():
    """Relative error of the float64 oracle's covariance on the offset case against the exact covariance: the rows
    are float32 numbers 1000 + 0.01 z, so z = (rows - 1000) / 0.01 is known exactly up to one double rounding and
    1e-4 cov(z), formed from numbers of order 1, has nothing to cancel."""
    rows = rows_of("offset").astype(np.float64)
    z = (rows - 1000.0) / 0.01
    exact = 1e-4 * np.cov(z, rowvar=False)
    return float(np.abs(np.cov(rows, rowvar=False) - exact).max() / np.abs(exact).max())


# ---- a model small enough for the CPU: bare_model plus linear V and L nets and an inline prior
VIEW_PRIOR = {"mean": [0.02, -0.1, 0.0, 0.01, 0.0, -0.03],
              "cov": [[v * v if i == j else 0.0 for j in range(6)] for i, v in enumerate([.05, .15, .03, .05, .05, .05])]}
LIGHT_PRIOR = {"mean": [0.1, 0.3, -0.05, 0.02], "cov": [[0.01 if i == j else 0.0 for j in range(4)] for i in range(4)]}


class LinearNet(torch.nn.Module):
    def __init__(self, size, cout, seed):
        super().__init__()
        self.lin = torch.nn.Linear(3 * size * size, cout)
        g = torch.Generator().manual_seed(seed)
        with torch.no_grad():
            self.lin.weight.copy_(torch.randn(self.lin.weight.shape, generator=g) / (3 * size * size) ** 0.5)
            self.lin.bias.copy_(0.1 * torch.randn(cout, generator=g))

    def forward(self, x):
        return torch.tanh(self.lin(x.reshape(len(x), -1)))


def toy_view_light_model(size):
    from gan2shape_amd.model import ViewLightSampler
    from model_cases import bare_model
    m = bare_model("cpu")
    m.paired_nets = False
    m.image_size = size
    m.viewpoint_net, m.lighting_net = LinearNet(size, 6, 11), LinearNet(size, 4, 12)
    m.view_light_sampler = ViewLightSampler(None, None, 1, "cpu", VIEW_PRIOR, LIGHT_PRIOR)
    return m


def batching_bound(model, x):
    """How far a row of a batched forward of the linear toy nets may sit from the single-image forward: the two
    differ only in the order of a K-term dot product, each order is within K eps / 2 sum|w_i x_i| of the exact value
    (tanh is 1-Lipschitz), plus the roundings of tanh and of the added mean (values below 2)."""
    flat = x.reshape(len(x), -1).abs().double()
    worst = max(float((flat @ net.lin.weight.detach().abs().double().t()).max())
                for net in (model.viewpoint_net, model.lighting_net))
    return flat.shape[1] * EPS32 * worst + 4 * EPS32
