"""Golden vectors of the centre crop of step 2 (op/resample.py crop_resize, g2s_resample_sep):
tests/golden/crop_resize.npz.

    python tests/golden/make_crop_resize_golden.py

The reference commented the crop out (`# FIXME: add back cropping`, GAN2Shape/model.py:197-200 and 211-214) and left
the three lines in place, so the oracle runs exactly them with the reference's OWN utils.resize and utils.crop
(GAN2Shape/utils.py, loaded by path):

    x = utils.resize(x, [origin_size, origin_size]);  x = utils.crop(x, crop);  x = utils.resize(x, [image_size] * 2)

Cases, operands: tests/crop_resize_cases.py.  Every case runs once in float64 — `<case>.out`, and `<case>.gin`, the
vector-Jacobian product of the three calls against the case's cotangent — and once in float32 —
`<case>.out32`, `<case>.gin32`: the reference's own float32 results, from whose distance to the float64 values the GPU
test takes its bounds.  Only data is written.
"""
import os
import sys

import numpy as np
import torch

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, OUT)
sys.path.insert(0, os.path.dirname(OUT))
import make_golden as mg            # noqa: E402
import crop_resize_cases as cc      # noqa: E402


def compose(gu, name, dtype):
    """-> (out, vector-Jacobian product against the case's cotangent), both in `dtype`."""
    _, origin, crop, image, _ = cc.CASES[name]
    x = cc.image_of(name).to(dtype).requires_grad_(True)
    y = gu.resize(x, [origin, origin])
    y = gu.crop(y, crop)
    y = gu.resize(y, [image, image])
    gin, = torch.autograd.grad(y, x, cc.cotangent_of(name).to(dtype))
    return y.detach(), gin


def main():
    gu = mg._load_by_path("ref_g2s_utils", os.path.join(mg.REF, "GAN2Shape/utils.py"))
    out = {}
    for name, (gan, origin, crop, image, planes) in cc.CASES.items():
        y64, g64 = compose(gu, name, torch.float64)
        y32, g32 = compose(gu, name, torch.float32)
        assert y64.dtype == g64.dtype == torch.float64 and y32.dtype == g32.dtype == torch.float32
        assert tuple(y64.shape) == (1, planes, image, image) and tuple(g64.shape) == (1, planes, gan, gan)
        out[f"{name}.operand_sums"] = cc.operand_sums(name)      # the operands are not stored (size): the tests compare these
        out[f"{name}.out"], out[f"{name}.out32"] = y64.numpy(), y32.numpy()
        out[f"{name}.gin"], out[f"{name}.gin32"] = g64.numpy(), g32.numpy()
        print(f"{name:34s} out {tuple(y64.shape)}  e32 {cc.max_err(y32.numpy(), y64.numpy()):.3e}   "
              f"gin {tuple(g64.shape)}  e32 {cc.max_err(g32.numpy(), g64.numpy()):.3e}  "
              f"zero-gradient pixels {float((g64 == 0).double().mean()):.2f}")
    path = os.path.join(OUT, "crop_resize.npz")
    np.savez_compressed(path, **out)
    print("crop_resize.npz", os.path.getsize(path))


if __name__ == "__main__":
    main()
