"""-m gpu: GroupNorm + activation (csrc/groupnorm.hip) on every launch path of either direction against float64.

One test per case of tests/groupnorm_cases.py (the table, the paths each case takes and the gating of elements that
could flip the activation's slope are described there).  Each runs groupnorm_act forward and backward and compares
y, dx, dgamma, dbeta with oracle/nets.py in float64, as max|kernel - ref| / max|ref| per output.

Bound: groupnorm_cases.bound — RATIO x e32, where e32 is the error of torch's CPU float32 evaluation of the same
expression on the same inputs (a plain float32 restatement with another summation order), and never more than the
older test's 2e-6 (forward) / 2e-5 (gradients) of scale.  RATIO is 4 for every output: another summation order may
cost a few times a restatement's own error, and no path needed more.  Measured kernel error / e32 on an MI355X
(two cases are cut by the older test's cap instead: b_cpg5_far y 1.71e-6 against 2e-6, dgamma 7.0e-6 against 2e-5):

                    y      dx  dgamma   dbeta                        y      dx  dgamma   dbeta
    f_over4      1.00    0.90    0.15    1.05      b_cpg3         0.85    0.88    0.15    0.17
    f_ragged     0.90    0.82    0.42    0.27      b_L64          1.00    0.72    0.30    0.08
    f_exact      1.00    0.70    0.04    0.23      out_B          0.62    0.49    0.52    0.67
    b_cpg1       1.00    0.71    1.82    0.37      out_cpg        1.19    0.69    0.74    0.74
    b_cpg16      1.00    0.89    0.49    0.62      out_hw         1.10    0.93    1.69    0.52
    b_cpg5       1.40    0.94    0.60    0.20      out_n          1.06    0.70    0.41    0.43
    b_cpg5_far   1.31    0.52    0.36    0.71"""
import numpy as np
import pytest
import torch

import groupnorm_cases as gc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def groupnorm_act():
    import gan2shape_amd  # noqa: F401
    from gan2shape_amd import lib
    from gan2shape_amd.op.groupnorm import groupnorm_act
    lib.load()  # fails loudly if libg2s.so is missing
    return groupnorm_act


@pytest.mark.parametrize("name", gc.NAMES)
def test_groupnorm_act_path_vs_float64(groupnorm_act, name):
    _, shape, groups, act, slope, _, _ = gc.CASE[name]
    dt = gc.data(name)
    xt, gt, bt = (torch.from_numpy(dt[k].copy()).cuda().requires_grad_(True) for k in ("x", "gamma", "beta"))
    y = groupnorm_act(xt, gt, bt, groups, gc.EPS, bool(act), slope)
    y.backward(torch.from_numpy(dt["gy"].copy()).cuda())
    got = dict(y=y.detach(), dx=xt.grad, dgamma=gt.grad, dbeta=bt.grad)
    failed = []
    for k in gc.OUTPUTS:
        g = got[k].cpu().numpy()
        assert g.shape == dt["ref"][k].shape and np.isfinite(g).all(), k
        err = gc.rel_err(g, dt["ref"][k], dt["keep"] if k == "y" else None)
        bound = gc.bound(name, k)
        print(f"{name} {k}: error {err:.3e} of max|ref|, e32 {dt['e32'][k]:.3e}, ratio {err / dt['e32'][k]:.2f}, "
              f"bound {bound:.3e}")
        if not err <= bound:
            failed.append(f"{k}: {err:.3e} > {bound:.3e} ({err / dt['e32'][k]:.2f} x e32)")
    assert not failed, f"{name} {shape} paths {gc.paths(shape, groups)}: " + "; ".join(failed)
