"""Reference results of the ADA augmentation for three more matrices -> tests/golden/ada_twice.npz (run where the
reference is; only DATA is written).

    python tests/golden/make_ada_twice_golden.py

Exactly as make_ada_golden.py (whose loader and helpers are imported, nothing of it is run or edited): the
reference's non_leaking.py in float64 and float32, first order only — its grid_sample has no second derivative —
with `x`, `G`, `C`, `pads`, `gy`, `y`, `gx`, `e32_y`, `e32_gx` per case.  The three matrices are the ones the gather
form of the warp adjoint (g2s_ada_warp_down_bwd_gather) is most exposed to and the eight cases of ada.npz do not
stress: G scales name the step between neighbouring sample positions in source pixels, so

    scale0.4   many sample positions per source pixel (a large candidate box), and source pixels nothing samples;
    scale2.5   most source pixels lie between the sample positions (an empty candidate set);
    aniso45    0.5 / 2.0 under a 45 degree rotation with a fractional shift (a sheared pre-image of the pixel square).

Each case is [2, 3, 20, 28] with the full colour matrix; the second sample carries a rotated variant."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_ada_golden as base                # noqa: E402  loader and helpers only
import make_golden as mg                      # noqa: E402

rot, scale, shift, mats = base.rot, base.scale, base.shift, base.mats

# name, C, H, W, G [B, 3, 3]
CASES = [
    ("scale0.4", 3, 20, 28, mats(scale(0.4, 0.4), (rot(20), scale(0.4, 0.4)))),
    ("scale2.5", 3, 20, 28, mats(scale(2.5, 2.5), (scale(2.5, 2.5), rot(-33)))),
    ("aniso45", 3, 20, 28, mats((shift(1.3, -0.7), rot(45), scale(0.5, 2.0)),
                                (rot(45), scale(2.0, 0.5), shift(-0.45, 2.2)))),
]


def main():
    ref = base.load_reference()
    rng = np.random.default_rng(2025)
    out = {}
    for name, C, H, W, G in CASES:
        B = G.shape[0]
        x = torch.from_numpy(base.image(rng, B, C, H, W))
        gy = torch.from_numpy(rng.standard_normal((B, C, H, W)).astype(np.float32))
        cmat = torch.tensor(base.FULL_C).unsqueeze(0).repeat(B, 1, 1)
        cmat[:, :3, 3] += 0.1 * torch.arange(B).view(B, 1)
        res = {}
        for dtype in (torch.float64, torch.float32):
            xi = x.to(dtype).requires_grad_(True)
            y, (g_out, c_out) = ref.augment(xi, 0.5, (G, cmat))
            assert g_out is G and c_out is cmat
            gx, = torch.autograd.grad(y, xi, gy.to(dtype))
            res[dtype] = (y.detach(), gx)
        (y64, gx64), (y32, gx32) = res[torch.float64], res[torch.float32]
        pads = [int(v) for v in ref.get_padding(G, H, W, 12)]
        out[f"{name}.x"], out[f"{name}.G"], out[f"{name}.gy"] = mg.np_(x), mg.np_(G), mg.np_(gy)
        out[f"{name}.C"] = mg.np_(cmat)
        out[f"{name}.pads"] = np.array(pads, dtype=np.int32)
        out[f"{name}.y"], out[f"{name}.gx"] = mg.np_(y64), mg.np_(gx64)
        out[f"{name}.e32_y"] = np.array(float((y32.double() - y64).abs().max()))
        out[f"{name}.e32_gx"] = np.array(float((gx32.double() - gx64).abs().max()))
        print(name, "pads", pads, "e32 y", float(out[f"{name}.e32_y"]), "gx", float(out[f"{name}.e32_gx"]))
    out["names"] = np.array([c[0] for c in CASES])
    path = os.path.join(HERE, "ada_twice.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
