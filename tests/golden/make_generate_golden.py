"""Reference results of the sample generator -> tests/golden/generate.npz (run where the reference is; only DATA is
written).

    python tests/golden/make_generate_golden.py

The reference's own Generator(8, 32, 4, channel_multiplier=1) with seeded weights (generate_cases.G_CFG; the tests
refill this package's state-dict-compatible module the same way, so no weights are stored) is evaluated in float64
on the CPU: style_forward of z [5, 32], the mean latent of a fixed z_mean [70, 32], the truncated w at 0.7 as
stylegan2-pytorch/generate.py:20 forms it, the image of those w for given per-sample noise maps (sides 4, 8, 8), and
the uint8 HWC image that save_image(normalize=True, range=(-1, 1)) makes of the float32 cast of that image
(torchvision is absent offline: its arithmetic, utils.py norm_ip + save_image, is written out here).  `ref_fp32_err.*`:
how far the reference's OWN float32 run is from its float64 run (maximum absolute difference over the five samples,
for w relative to max |w|, for the image relative to max |image|)."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden as mg                      # noqa: E402  helpers only; nothing of it is run or edited
import model_cases                            # noqa: E402
import generate_cases as gc                   # noqa: E402


def save_image_uint8(img):
    """[B, 3, H, W] float32 -> [B, H, W, 3] uint8: torchvision.utils.save_image(normalize=True, range=(-1, 1))."""
    img = img.clone().clamp_(min=-1, max=1)
    img = img.sub_(-1).div_(max(1 - (-1), 1e-5))
    return img.mul(255).add_(0.5).clamp_(0, 255).permute(0, 2, 3, 1).to(torch.uint8)


def main():
    sys.path.insert(0, mg.SG2)
    import model as sg2
    cfg = gc.G_CFG
    rng = np.random.default_rng(cfg["seed"])
    z = rng.standard_normal((gc.N_Z, cfg["style_dim"])).astype(np.float32)
    z_mean = rng.standard_normal((gc.N_MEAN, cfg["style_dim"])).astype(np.float32)
    noises = [rng.standard_normal((gc.N_Z, 1, s, s)).astype(np.float32) for s in (4, 8, 8)]
    res = {}
    for dtype in (torch.float64, torch.float32):
        g = sg2.Generator(cfg["size"], cfg["style_dim"], cfg["n_mlp"], channel_multiplier=cfg["channel_multiplier"])
        model_cases.prepare_generator(g, cfg["seed"], mg.fill_deterministic)
        g = g.eval().to(dtype).requires_grad_(False)
        with torch.no_grad():
            mean = g.style_forward(torch.from_numpy(z_mean).to(dtype)).mean(0, keepdim=True)
            w = g.style_forward(torch.from_numpy(z).to(dtype))
            img, _ = g([w], truncation=gc.TRUNCATION, truncation_latent=mean, input_is_w=True,
                       noise=[torch.from_numpy(n).to(dtype) for n in noises])
            wt = mean + gc.TRUNCATION * (w - mean)
        res[dtype] = dict(mean=mean, w=w, wt=wt, img=img)
    r64, r32 = res[torch.float64], res[torch.float32]
    out = {"z": z, "z_mean": z_mean, "mean_latent": mg.np_(r64["mean"]), "w": mg.np_(r64["w"]),
           "w_truncated": mg.np_(r64["wt"]), "image": mg.np_(r64["img"]),
           "image_u8": mg.np_(save_image_uint8(r64["img"].float()))}
    for i, n in enumerate(noises):
        out[f"noise{i}"] = n
    for key in ("mean", "w", "wt", "img"):
        err = float((r32[key].double() - r64[key]).abs().max() / r64[key].abs().max())
        out[f"ref_fp32_err.{key}"] = np.array(err)
        print(key, "fp32 vs fp64:", err)
    assert np.array_equal(out["image_u8"], gc.quantise(out["image"].astype(np.float32)))
    path = os.path.join(HERE, "generate.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path))


if __name__ == "__main__":
    main()
