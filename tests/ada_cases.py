"""Shared by test_ada_cpu.py and test_gpu_ada.py: the cases of tests/golden/ada.npz (make_ada_golden.py) and the
bound the float32 routes are held to.

BOUND: a float32 route (the torch composition on the CPU, the kernels on the GPU) may differ from the float64 golden
by E32_MULTIPLE times the case's stored e32 — the distance of the reference's OWN float32 run from its float64 run.
Every route sums the same 144 products per pixel (12 x 12 taps up, bilinear, 12 x 12 taps down) in a different order,
so each is one more draw from the same error distribution; the maximum over a few thousand pixels of such a draw
varies by a small factor.  The multiple is one of 2, 4, 8, fixed after ONE measurement of both float32 routes and
not moved since: the torch composition, which performs the reference's own float32 operations,
shows at most 1.00 x e32 forward and 1.07 x e32 in the gradient; the kernels, with their other summation order,
0.84 to 2.16 x e32 forward and 0.59 to 2.44 x e32 in the gradient (the maximum on identity16, where e32 itself is
at its smallest: the reference's bilinear weights are exactly 0 and 1 there).  2 does not cover a second summation
order; 4 is the smallest of the three that both routes meet."""
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ada.npz")
E32_MULTIPLE = 4

_cache = {}


def data():
    if "d" not in _cache:
        _cache["d"] = dict(np.load(GOLDEN, allow_pickle=False))
    return _cache["d"]


def names():
    return [str(n) for n in data()["names"]]


def case(name):
    """dict of torch tensors (CPU): x, G, gy float32; y, gx float64; C [B, 4, 4] float32 or None; pads tuple;
    e32_y, e32_gx floats; seed / p for the sampled-colour case (else None)."""
    d = data()
    t = lambda k: torch.from_numpy(d[f"{name}.{k}"])
    return dict(name=name, x=t("x"), G=t("G"), gy=t("gy"), y=t("y"), gx=t("gx"),
                C=t("C") if f"{name}.C" in d else None, pads=tuple(int(v) for v in d[f"{name}.pads"]),
                e32_y=float(d[f"{name}.e32_y"]), e32_gx=float(d[f"{name}.e32_gx"]),
                seed=int(d[f"{name}.seed"]) if f"{name}.seed" in d else None,
                p=float(d[f"{name}.p"]) if f"{name}.p" in d else None)


def run(aug, c, x):
    """The public route for a case on input x (requires_grad): (y, gx) with the case's cotangent."""
    if c["C"] is None:
        y, G = aug.random_apply_affine(x, 1.0, c["G"])
        assert G is c["G"]
    else:
        y, (G, C) = aug.augment(x, 0.5, (c["G"], c["C"]))
        assert G is c["G"] and C is c["C"]
    gx, = torch.autograd.grad(y, x, c["gy"].to(y))
    return y.detach(), gx
