"""Reference results of the BATCHED projector's pieces -> tests/golden/projector_batch.npz (run where the reference is;
only DATA is written).

    python tests/golden/make_projector_batch_golden.py

The reference Generator (stylegan2-pytorch/model.py) and projector.py are loaded by path, as make_projector_golden.py
does.  Inputs are NOT stored: tests/projector_batch_cases.py regenerates them from seeds.  Stored:

  g16b.<mode>.*   the reference Generator at size 16 with the fixture's weights, B = 3, per-sample noise maps of sides
                  4, 8, 8, 16, 16, for one w per sample (mode `w`) and one per sample and layer (`wp`), in float64: the
                  image, and the gradients of sum(image * cotangent) to the latent and to every map;
  loop.*          three steps of the reference's projector loop (projector.py:166-218: its noise_regularize,
                  noise_normalize_, get_lr, latent_noise and torch.optim.Adam) at B = 2 in float64, with the stand-in
                  perceptual term of projector_batch_cases.py in the place of LPIPS (no weights offline) and the jitter
                  draws of projector_batch_cases.loop_inputs handed to latent_noise: the latent and the maps after each step;
  *.ref_fp32_err.*  how far the reference's OWN float32 run is from its float64 run for the same quantity, maximum over
                  N_SEEDS inputs (image: max-abs over max; everything else: L2 relative) — what the tests' bounds are
                  multiples of."""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden as mg                      # noqa: E402  helpers only; nothing of it is run or edited
import make_projector_golden as mpg           # noqa: E402  load_reference_projector
import model_cases                            # noqa: E402
import projector_cases as pc                  # noqa: E402
import projector_batch_cases as pb            # noqa: E402


def l2_rel(a, ref):
    return float((a.double() - ref).norm() / ref.norm())


def reference_generators():
    sys.path.insert(0, mg.SG2)
    import model as sg2
    cfg = pc.G_CFG
    gens = {}
    for dtype in (torch.float64, torch.float32):
        g = sg2.Generator(cfg["size"], cfg["style_dim"], cfg["n_mlp"], channel_multiplier=cfg["channel_multiplier"])
        model_cases.prepare_generator(g, cfg["seed"], mg.fill_deterministic)
        gens[dtype] = g.eval().to(dtype).requires_grad_(False)
    return gens


def generator_cases(gens, out):
    for mode in pb.MODES:
        err = {}
        for seed in range(pb.N_SEEDS):
            w, noises, gy = pb.generator_inputs(mode, seed)
            res = {}
            for dtype, g in gens.items():
                wt = torch.from_numpy(w).to(dtype).requires_grad_(True)
                nz = [torch.from_numpy(n).to(dtype).requires_grad_(True) for n in noises]
                img, _ = g([wt], input_is_w=True, noise=nz)
                grads = torch.autograd.grad(img, [wt] + nz, torch.from_numpy(gy).to(dtype))
                res[dtype] = [img.detach()] + list(grads)
            r64, r32 = res[torch.float64], res[torch.float32]
            for key, a, b in zip(pb.generator_keys(), r32, r64):
                e = float((a.double() - b).abs().max() / b.abs().max()) if key == "img" else l2_rel(a, b)
                err[key] = max(err.get(key, 0.0), e)
            if seed == 0:
                for key, b in zip(pb.generator_keys(), r64):
                    out[f"g16b.{mode}.{key}"] = mg.np_(b)
        for key, v in err.items():
            out[f"g16b.{mode}.ref_fp32_err.{key}"] = np.array(v)
        print("g16b", mode, "fp32 vs fp64:", err)


def run_loop(ref, g, inp, dtype):
    """[(latent, maps) after each step] of the reference's loop at `dtype`."""
    cfg = pb.LOOP
    target = inp["target"].to(dtype)
    percept = pb.standin_percept(inp["mask"])
    noises = [m.to(dtype).clone().requires_grad_(True) for m in inp["maps"]]
    latent_in = inp["latent_mean"].to(dtype).detach().clone().unsqueeze(0).repeat(pb.LOOP_B, 1)
    latent_in.requires_grad = True
    optimizer = torch.optim.Adam([latent_in] + noises, lr=cfg["lr"])
    steps, after = pb.LOOP_STEPS, []
    real_randn_like = torch.randn_like
    for i in range(steps):
        t = i / steps
        optimizer.param_groups[0]["lr"] = ref.get_lr(t, cfg["lr"])
        strength = pb.LATENT_STD * cfg["noise"] * max(0, 1 - t / cfg["noise_ramp"]) ** 2
        torch.randn_like = lambda x, i=i: inp["jitter"][i].to(x.dtype)       # latent_noise's draw: the stored one
        try:
            latent_n = ref.latent_noise(latent_in, strength)
        finally:
            torch.randn_like = real_randn_like
        img_gen, _ = g([latent_n], input_is_w=True, noise=noises)
        loss = (percept(img_gen, target).sum() + cfg["noise_regularize"] * ref.noise_regularize(noises)
                + cfg["mse"] * F.mse_loss(img_gen, target))
        optimizer.zero_grad()
        loss.backward()
        optimizer.step()
        ref.noise_normalize_(noises)
        after.append((latent_in.detach().clone(), [n.detach().clone() for n in noises]))
    return after


def loop_case(ref, gens, out):
    err = {}
    for seed in range(pb.N_SEEDS):
        inp = pb.loop_inputs(seed)
        a64 = run_loop(ref, gens[torch.float64], inp, torch.float64)
        a32 = run_loop(ref, gens[torch.float32], inp, torch.float32)
        for s, ((l64, m64), (l32, m32)) in enumerate(zip(a64, a32)):
            pairs = [(f"step{s}.latent", l32, l64)] + [(f"step{s}.noise{k}", a, b) for k, (a, b) in enumerate(zip(m32, m64))]
            for key, a, b in pairs:
                err[key] = max(err.get(key, 0.0), l2_rel(a, b))
                if seed == 0:
                    out[f"loop.{key}"] = mg.np_(b)
    for key, v in err.items():
        out[f"loop.ref_fp32_err.{key}"] = np.array(v)
    print("loop fp32 vs fp64:", err)


def main():
    ref = mpg.load_reference_projector()
    gens = reference_generators()
    out = {}
    generator_cases(gens, out)
    loop_case(ref, gens, out)
    path = os.path.join(HERE, "projector_batch.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path))


if __name__ == "__main__":
    main()
