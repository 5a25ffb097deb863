"""The case table of tests/groupnorm_cases.py, without a GPU: it reaches what it claims to reach, its float64 reference
is torch's own float64 GroupNorm + activation, and the float32 yardstick of every case is printed (-s shows it)."""
import numpy as np
import pytest

import groupnorm_cases as gc


def test_every_case_takes_the_paths_it_is_listed_for():
    assert set(gc.EXPECTED_PATHS) == set(gc.NAMES)
    for name, shape, groups, *_ in gc.CASES:
        assert shape[1] % groups == 0 and shape[2] * shape[3] % 4 == 0, name
        assert gc.paths(shape, groups) == gc.EXPECTED_PATHS[name], name


def test_every_reachable_pair_of_paths_is_present():
    # a group of more than 65536 elements cannot take the fused backward (at most 16384)
    assert {gc.paths(c[1], c[2]) for c in gc.CASES} == {("two", "two"), ("fused", "fused"), ("fused", "two")}


@pytest.mark.parametrize("direction", [0, 1])
@pytest.mark.parametrize("path", ["fused", "two"])
def test_every_activation_kind_occurs_on_every_path(direction, path):
    kinds = {gc.kind(c[3], c[4]) for c in gc.CASES if gc.paths(c[1], c[2])[direction] == path}
    assert kinds == {"none", "relu", "leaky"}


def test_the_gates_of_the_fused_backward_are_each_missed_by_one_step():
    missed = {}
    for name in ("out_B", "out_n", "out_hw", "out_cpg"):
        _, (B, C, H, W), G, *_ = gc.CASE[name]
        missed[name] = (B != 1, C // G * H * W > 16384, H * W % 256 != 0, C // G > 16)
    assert list(missed.values()) == [(True, False, False, False), (False, True, False, False),
                                     (False, False, True, False), (False, False, False, True)], missed


@pytest.mark.parametrize("name", gc.NAMES)
def test_case_reference_and_float32_yardstick(name):
    """The float64 reference equals torch's CPU float64 F.group_norm + leaky_relu and its autograd to 1e-9; at most
    0.1 % of the elements are gated; prints e32 per output."""
    import torch
    import torch.nn.functional as F
    _, shape, groups, act, slope, _, _ = gc.CASE[name]
    dt = gc.data(name)
    assert dt["gated"] <= gc.MAX_GATED, dt["gated"]
    assert (dt["gy"][~dt["keep"]] == 0).all()
    xt, gt, bt = (torch.tensor(dt[k], dtype=torch.float64, requires_grad=True) for k in ("x", "gamma", "beta"))
    y = F.group_norm(xt, groups, gt, bt, gc.EPS)
    if act:
        y = F.leaky_relu(y, slope)
    y.backward(torch.tensor(dt["gy"], dtype=torch.float64))
    for k, got in (("y", y.detach()), ("dx", xt.grad), ("dgamma", gt.grad), ("dbeta", bt.grad)):
        np.testing.assert_allclose(dt["ref"][k], got.numpy(), rtol=1e-9, atol=1e-9 * np.abs(got.numpy()).max(), err_msg=k)
    print(f"{name} {shape} G={groups} {gc.kind(act, slope)} paths={gc.paths(shape, groups)} gated={dt['gated']:.2e} e32: "
          + " ".join(f"{k}={dt['e32'][k]:.3e}" for k in gc.OUTPUTS))
    assert all(np.isfinite(v) and v > 0 for v in dt["e32"].values())
