"""Reference results of generator training -> tests/golden/gtrain.npz (run where the reference is; only DATA is
written).

    python tests/golden/make_gtrain_golden.py

The reference's model.py Generator(16, 64, 2, channel_multiplier=1) and Discriminator(16, channel_multiplier=1) are
loaded by path (make_golden.py's helpers), filled by dtrain_cases.draw_like's rule and run on the CPU in float64 and in
float32 through the two passes of train.py's generator step (gtrain_cases.nonsaturating_pass, path_pass) with seeded
latents, noise maps and image noise passed explicitly.

Stored per case `name` (gtrain_cases.CASES): `image`, `loss`, `path.lengths`, `path.path_mean`, `path.penalty`, and per
parameter (named_parameters order) the gradient norms and probe projections of both passes (`ns.norms`, `ns.proj`,
`path.norms`, `path.proj`); for every one `e32_<key>`, the distance of the float32 run from the float64 run.
`trainer.g`, `trainer.g_ema` [P]: the probe projections of the generator's and g_ema's parameters after two trainer
steps (gtrain_cases.reference_trainer), with `trainer.e32_g`, `trainer.e32_g_ema`.

Condition on the inputs, asserted here: every per-sample path length is at least 0.1 x their mean (the square root's
slope is unbounded at 0); pick another INPUT_SEED otherwise."""
import copy
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import dtrain_cases as dc                     # noqa: E402
import gtrain_cases as gc                     # noqa: E402
import make_golden as mg                      # noqa: E402  helpers only; nothing of it is run or edited


def reference_nets(dtype):
    if mg.SG2 not in sys.path:
        sys.path.insert(0, mg.SG2)
    import model as sg2
    g = sg2.Generator(gc.SIZE, gc.STYLE_DIM, gc.N_MLP, channel_multiplier=gc.CHANNEL_MULTIPLIER).to(dtype)
    d = sg2.Discriminator(gc.SIZE, channel_multiplier=gc.CHANNEL_MULTIPLIER).to(dtype)
    return dc.fill_weights(g, gc.G_SEED), dc.fill_weights(d, gc.D_SEED)


def main():
    torch.set_num_threads(8)
    out, runs = {}, {}
    for dtype in (torch.float64, torch.float32):
        g, d = reference_nets(dtype)
        for p in d.parameters():
            p.requires_grad = False
        like = torch.zeros((), dtype=dtype)
        probe = dc.draw_like(g, gc.PROBE_SEED)
        for name, (B, n_lat, inject) in gc.CASES.items():
            zs, maps, img_noise = gc.inputs(name)
            ns = gc.nonsaturating_pass(g, d, gc.to(zs, like), gc.to(maps, like), inject)
            pp = gc.path_pass(g, gc.to(zs, like), gc.to(maps, like), inject, gc.to([img_noise], like)[0])
            res = {"image": ns["image"], "loss": ns["loss"], "path.lengths": pp["lengths"],
                   "path.path_mean": pp["path_mean"], "path.penalty": pp["penalty"]}
            res = {k: mg.np_(v.double()) for k, v in res.items()}
            res["ns.norms"], res["ns.proj"] = gc.summarize(ns["grads"], probe)
            res["path.norms"], res["path.proj"] = gc.summarize(pp["grads"], probe)
            runs[(dtype, name)] = res
            if dtype == torch.float64:
                lengths = res["path.lengths"]
                assert lengths.min() >= 0.1 * lengths.mean(), (name, lengths)
        g, d = reference_nets(dtype)
        g_ema = copy.deepcopy(g)
        gc.reference_trainer(g, g_ema, d, like)
        runs[(dtype, "trainer")] = {"trainer.g": gc.projections(g, probe), "trainer.g_ema": gc.projections(g_ema, probe)}
    for name in gc.CASES:
        r64, r32 = runs[(torch.float64, name)], runs[(torch.float32, name)]
        for k, v in r64.items():
            out[f"{name}.{k}"] = v
            diff = np.abs(r32[k] - v)
            out[f"{name}.e32_{k}"] = np.array(diff.max())
            print(name, k, "e32 max", float(diff.max()), "scale", float(np.abs(v).max()))
    t64, t32 = runs[(torch.float64, "trainer")], runs[(torch.float32, "trainer")]
    for k, v in t64.items():
        out[k] = v
        out[k.replace("trainer.", "trainer.e32_")] = np.abs(t32[k] - v)
        print(k, "e32 max", float(np.abs(t32[k] - v).max()), "scale", float(np.abs(v).max()))
    out["names"] = np.array(list(gc.CASES))
    out["params"] = np.array([n for n, _ in reference_nets(torch.float32)[0].named_parameters()])
    path = os.path.join(HERE, "gtrain.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
