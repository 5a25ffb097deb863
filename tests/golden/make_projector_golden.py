"""Reference results of the latent projector's pieces -> tests/golden/projector.npz (run where the reference is;
only DATA is written).

    python tests/golden/make_projector_golden.py

The reference's projector.py is loaded by path with import-only placeholders for what it imports at the top and
is absent offline (torchvision, lpips, tqdm, PIL) or heavy (its `model`); noise_regularize, noise_normalize_ and
get_lr are plain torch / math and run on the CPU.  Inputs are NOT stored: tests/projector_cases.py regenerates
them from seeds (numpy Generator streams).  Stored per case: the float64 value, per-map gradient and normalised maps,
and `ref_fp32_err` — how far the reference's OWN float32 run is from its float64 run, maximum over N_SEEDS inputs
(value: relative; gradients and normalised maps: L2 relative per map).  The generator case is the reference
Generator at size 16 (noise sides 4, 8, 8, 16, 16) with fill_deterministic weights: image, latent gradient and every
noise-map gradient in float64, and the same float32 errors."""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden as mg                      # noqa: E402  helpers only; nothing of it is run or edited
import model_cases                            # noqa: E402
import projector_cases as pc                  # noqa: E402


def load_reference_projector():
    names = ("torchvision", "lpips", "tqdm", "PIL", "model")
    saved = {name: sys.modules.get(name) for name in names}
    for name in names:
        sys.modules[name] = types.ModuleType(name)
    sys.modules["torchvision"].transforms = types.ModuleType("torchvision.transforms")
    sys.modules["PIL"].Image = types.ModuleType("PIL.Image")
    sys.modules["tqdm"].tqdm = lambda it, *a, **k: it
    sys.modules["model"].Generator = None
    try:
        return mg._load_by_path("ref_projector", os.path.join(mg.SG2, "projector.py"))
    finally:
        for name, mod in saved.items():
            if mod is None:
                del sys.modules[name]
            else:
                sys.modules[name] = mod


def l2_rel(a, ref):
    return float((a.double() - ref).norm() / ref.norm())


def noise_cases(ref, out):
    for lst, B, kind in pc.CASES:
        name = pc.case_name(lst, B, kind)
        sides = pc.SIDE_LISTS[lst]
        e_val, e_grad, e_norm = 0.0, np.zeros(len(sides)), np.zeros(len(sides))
        for seed in range(pc.N_SEEDS):
            maps = [torch.from_numpy(m) for m in pc.make_maps(sides, B, kind, seed)]
            res = {}
            for dtype in (torch.float64, torch.float32):
                xs = [m.to(dtype).requires_grad_(True) for m in maps]
                v = ref.noise_regularize(xs)
                g = torch.autograd.grad(v, xs)
                normed = [m.to(dtype).clone() for m in maps]
                ref.noise_normalize_(normed)
                res[dtype] = (v.detach(), g, normed)
            v64, g64, n64 = res[torch.float64]
            v32, g32, n32 = res[torch.float32]
            e_val = max(e_val, float(abs(v32.double() - v64) / abs(v64)))
            e_grad = np.maximum(e_grad, [l2_rel(a, b) for a, b in zip(g32, g64)])
            e_norm = np.maximum(e_norm, [l2_rel(a, b) for a, b in zip(n32, n64)])
            if seed == 0:                      # the case the tests run
                out[f"{name}.value"] = np.array(float(v64))
                for i, (g, n) in enumerate(zip(g64, n64)):
                    out[f"{name}.grad{i}"] = mg.np_(g)
                    out[f"{name}.norm{i}"] = mg.np_(n)
        out[f"{name}.ref_fp32_err.value"] = np.array(e_val)
        out[f"{name}.ref_fp32_err.grad"] = e_grad
        out[f"{name}.ref_fp32_err.norm"] = e_norm
        print(name, "fp32 vs fp64: value", e_val, "grad", e_grad.max(), "norm", e_norm.max())


def generator_case(out):
    sys.path.insert(0, mg.SG2)
    import model as sg2
    cfg = pc.G_CFG
    gens = {}
    for dtype in (torch.float64, torch.float32):
        g = sg2.Generator(cfg["size"], cfg["style_dim"], cfg["n_mlp"], channel_multiplier=cfg["channel_multiplier"])
        model_cases.prepare_generator(g, cfg["seed"], mg.fill_deterministic)
        gens[dtype] = g.eval().to(dtype).requires_grad_(False)
    err = {}
    for seed in range(pc.N_SEEDS):
        w, noises, gy = pc.generator_inputs(seed)
        res = {}
        for dtype, g in gens.items():
            wt = torch.from_numpy(w).to(dtype).requires_grad_(True)
            nz = [torch.from_numpy(n).to(dtype).requires_grad_(True) for n in noises]
            img, _ = g([wt], input_is_w=True, noise=nz)
            grads = torch.autograd.grad(img, [wt] + nz, torch.from_numpy(gy).to(dtype))
            res[dtype] = (img.detach(), grads)
        (i64, g64), (i32, g32) = res[torch.float64], res[torch.float32]
        e = {"img": float((i32.double() - i64).abs().max() / i64.abs().max()), "gw": l2_rel(g32[0], g64[0])}
        for k in range(len(noises)):
            e[f"gnoise{k}"] = l2_rel(g32[1 + k], g64[1 + k])
        for k_, v in e.items():
            err[k_] = max(err.get(k_, 0.0), v)
        if seed == 0:
            out["g16.img"] = mg.np_(i64)
            out["g16.gw"] = mg.np_(g64[0])
            for k in range(len(noises)):
                out[f"g16.gnoise{k}"] = mg.np_(g64[1 + k])
    for k_, v in err.items():
        out[f"g16.ref_fp32_err.{k_}"] = np.array(v)
    print("g16 fp32 vs fp64:", err)


def main():
    ref = load_reference_projector()
    out = {"get_lr.t": np.array(pc.LR_T), "get_lr.lr": np.array([ref.get_lr(t, 0.1) for t in pc.LR_T]),
           "get_lr.lr_ramps": np.array([ref.get_lr(t, 0.05, rampdown=0.5, rampup=0.1) for t in pc.LR_T])}
    noise_cases(ref, out)
    generator_case(out)
    path = os.path.join(HERE, "projector.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path))


if __name__ == "__main__":
    main()
