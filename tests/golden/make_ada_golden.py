"""Reference results of the ADA augmentation -> tests/golden/ada.npz (run where the reference is; only DATA is written).

    python tests/golden/make_ada_golden.py

The reference's non_leaking.py is loaded by path, with `distributed.reduce_sum` stubbed in sys.modules (one
process: the identity) and `op.upfirdn2d` bound to the pure-torch route of the reference's own op/upfirdn2d.py
(upfirdn2d_native, which takes the per-axis factors and pads non_leaking.py passes).  Its grid_sample wrapper, which
exists for the double backward and reaches into a private torch operator whose signature has changed since, is
replaced by the F.grid_sample call it wraps: same forward, same first-order gradient.

Stored per case `name`: the float32 input `x`, `G` [B, 3, 3], the colour matrix `C` [B, 4, 4] (absent: no colour
stage), `pads` (x0, x1, y0, y1), the float64 output `y`, the cotangent `gy` and the float64 image gradient `gx` from the
reference's autograd, and `e32_y` / `e32_gx`: the maximum absolute difference between the reference's own float32 and
float64 results.  A case with sampled colour also stores `seed` and `p`.  Further: sample_affine / sample_color draws
for fixed seeds and p in {0, 0.5, 1}, and a 40-call AdaptiveAugment.tune trajectory."""
import math
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as mg                      # noqa: E402  helpers only; nothing of it is run or edited


def load_reference():
    saved = {name: sys.modules.get(name) for name in ("distributed", "op")}
    ref_up = mg._load_by_path("ref_upfirdn2d", os.path.join(mg.SG2, "op", "upfirdn2d.py"))

    def upfirdn2d(input, kernel, up=1, down=1, pad=(0, 0)):
        up = up if isinstance(up, (tuple, list)) else (up, up)
        down = down if isinstance(down, (tuple, list)) else (down, down)
        pad = tuple(pad) if len(pad) == 4 else (pad[0], pad[1], pad[0], pad[1])
        return ref_up.upfirdn2d_native(input, kernel, *up, *down, *pad)

    sys.modules["distributed"] = types.ModuleType("distributed")
    sys.modules["distributed"].reduce_sum = lambda t: t
    sys.modules["op"] = types.ModuleType("op")
    sys.modules["op"].upfirdn2d = upfirdn2d
    try:
        ref = mg._load_by_path("ref_non_leaking", os.path.join(mg.SG2, "non_leaking.py"))
    finally:
        for name, mod in saved.items():
            if mod is None:
                del sys.modules[name]
            else:
                sys.modules[name] = mod
    ref.grid_sample = lambda input, grid: F.grid_sample(input, grid, mode="bilinear", padding_mode="zeros",
                                                        align_corners=False)
    return ref


def rot(deg):
    a = math.radians(deg)
    return [[math.cos(a), -math.sin(a), 0], [math.sin(a), math.cos(a), 0], [0, 0, 1]]


def scale(sx, sy):
    return [[sx, 0, 0], [0, sy, 0], [0, 0, 1]]


def shift(tx, ty):
    return [[1, 0, tx], [0, 1, ty], [0, 0, 1]]


def mats(*ms):
    """One [3, 3] float32 matrix per argument; a tuple is the product of its members."""
    out = []
    for m in ms:
        m = m if isinstance(m, tuple) else (m,)
        acc = np.eye(3)
        for f in m:
            acc = acc @ np.array(f, dtype=np.float64)
        out.append(acc)
    return torch.tensor(np.stack(out), dtype=torch.float32)


EYE = scale(1, 1)
FULL_C = [[0.9, -0.2, 0.15, 0.05], [0.1, 1.1, -0.25, -0.1], [-0.3, 0.2, 0.8, 0.2], [0, 0, 0, 1]]

# name, C, H, W, G [B, 3, 3], colour: None (affine stage only) | "identity" | "full" | "sampled"
CASES = [
    ("identity16", 3, 16, 16, mats(EYE), None),
    ("rot30", 3, 16, 16, mats(rot(30)), "full"),
    ("aniso_shift", 3, 12, 20, mats((shift(2.3, -1.6), scale(0.7, 1.4))), "identity"),
    ("flip_rot90", 3, 12, 16, mats(scale(-1, 1), rot(90)), None),
    ("pad_clamp", 3, 16, 16, mats(scale(2.5, 2.5)), "sampled"),
    ("batch3", 3, 20, 28, mats((shift(1.5, 0.75), rot(17)), scale(1.3, 1.3), (rot(-40), scale(0.8, 1.25))), "full"),
    ("tiles40x24", 3, 40, 24, mats((rot(10), shift(-2.25, 3.5)), (scale(1.1, 0.9), rot(-5))), None),
    ("gray", 1, 16, 12, mats(rot(-20)), None),
]
SAMPLED_SEED, SAMPLED_P = 11, 0.8


def image(rng, B, C, H, W):
    """A smooth field plus noise, in about [-1, 1]."""
    y, x = np.meshgrid(np.linspace(-1, 1, H), np.linspace(-1, 1, W), indexing="ij")
    f = rng.uniform(1, 4, (B, C, 1, 1))
    ph = rng.uniform(0, 6, (B, C, 1, 1))
    return (0.6 * np.sin(f * x + ph) * np.cos(f * y - ph) + 0.3 * rng.standard_normal((B, C, H, W))).astype(np.float32)


def augment_cases(ref, out):
    rng = np.random.default_rng(2024)
    for name, C, H, W, G, colour in CASES:
        B = G.shape[0]
        x = torch.from_numpy(image(rng, B, C, H, W))
        gy = torch.from_numpy(rng.standard_normal((B, C, H, W)).astype(np.float32))
        cmat = None
        if colour == "identity":
            cmat = torch.eye(4).unsqueeze(0).repeat(B, 1, 1)
        elif colour == "full":
            cmat = torch.tensor(FULL_C).unsqueeze(0).repeat(B, 1, 1)
            cmat[:, :3, 3] += 0.1 * torch.arange(B).view(B, 1)       # a different offset per sample
        res = {}
        for dtype in (torch.float64, torch.float32):
            xi = x.to(dtype).requires_grad_(True)
            if colour is None:
                y, g_out = ref.random_apply_affine(xi, 1.0, G)
                c_out = None
            else:
                torch.manual_seed(SAMPLED_SEED)
                y, (g_out, c_out) = ref.augment(xi, SAMPLED_P, (G, cmat))
            gx, = torch.autograd.grad(y, xi, gy.to(dtype))
            res[dtype] = (y.detach(), gx)
            assert g_out is G
        y64, gx64 = res[torch.float64]
        y32, gx32 = res[torch.float32]
        pads = [int(v) for v in ref.get_padding(G, H, W, 12)]
        out[f"{name}.x"], out[f"{name}.G"], out[f"{name}.gy"] = mg.np_(x), mg.np_(G), mg.np_(gy)
        out[f"{name}.pads"] = np.array(pads, dtype=np.int32)
        out[f"{name}.y"], out[f"{name}.gx"] = mg.np_(y64), mg.np_(gx64)
        out[f"{name}.e32_y"] = np.array(float((y32.double() - y64).abs().max()))
        out[f"{name}.e32_gx"] = np.array(float((gx32.double() - gx64).abs().max()))
        if c_out is not None:
            out[f"{name}.C"] = mg.np_(c_out)
        if colour == "sampled":
            out[f"{name}.seed"], out[f"{name}.p"] = np.array(SAMPLED_SEED), np.array(SAMPLED_P)
        print(name, "pads", pads, "e32 y", float(out[f"{name}.e32_y"]), "gx", float(out[f"{name}.e32_gx"]))
    out["names"] = np.array([c[0] for c in CASES])


def draw_cases(ref, out):
    for p in (0.0, 0.5, 1.0):
        torch.manual_seed(7)
        out[f"draw.affine.p{p}"] = mg.np_(ref.sample_affine(p, 4, 20, 28))
        torch.manual_seed(7)
        out[f"draw.color.p{p}"] = mg.np_(ref.sample_color(p, 4))


def tune_case(ref, out):
    rng = np.random.default_rng(5)
    # mostly positive first (p rises), then mostly negative (p falls back towards 0)
    preds = rng.standard_normal((40, 8, 1)).astype(np.float32) + np.where(np.arange(40) < 24, 1.0, -1.0)[:, None, None]
    ada = ref.AdaptiveAugment(0.6, 200, 4, "cpu")
    ps, rs = [], []
    for pred in preds:
        ps.append(ada.tune(torch.from_numpy(pred)))
        rs.append(ada.r_t_stat)
    out["tune.real_pred"] = preds
    out["tune.p"] = np.array(ps, dtype=np.float64)
    out["tune.r_t_stat"] = np.array(rs, dtype=np.float64)
    out["tune.args"] = np.array([0.6, 200, 4])


def main():
    ref = load_reference()
    out = {}
    augment_cases(ref, out)
    draw_cases(ref, out)
    tune_case(ref, out)
    path = os.path.join(HERE, "ada.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
