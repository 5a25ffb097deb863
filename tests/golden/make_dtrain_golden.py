"""Reference results of discriminator training -> tests/golden/dtrain.npz (run where the reference is; only DATA is
written).

    python tests/golden/make_dtrain_golden.py

The reference's model.py Discriminator is loaded by path (make_golden.py's helpers), filled by dtrain_cases.py's weight
rule and run on the CPU in float64 through the two passes of train.py's discriminator step: the logistic pass, and the
R1 pass (autograd.grad(create_graph=True), then backward of r1 / 2 * r1_loss * 16 + 0 * real_pred[0]).

Stored per case `name` (dtrain_cases.CASES, all D(16), channel_multiplier 1): the float32 images `real`, `fake`; of
the logistic pass `real_pred`, `fake_pred`, `loss`, and per parameter (named_parameters order) the gradient's norm
`log.norms` and its projection `log.proj` on the probe drawn by the same rule; of the R1 pass `r1.real_pred`,
`r1.grad_real`, `r1.per_sample`, `r1.r1`, `r1.norms`, `r1.proj`.  For every stored result `e32_<key>`: the distance of
the reference's own float32 run from its float64 run (the maximum absolute difference over the quantity's elements; for
norms and projections, over the parameters).  `trainer.e32` [P]: per parameter, the maximum absolute deviation of the weights after two steps
(i = 0 with R1, i = 1 without, B = 4) of the reference's float32 trainer from its float64 trainer."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import dtrain_cases as dc                     # noqa: E402
import make_golden as mg                      # noqa: E402  helpers only; nothing of it is run or edited


def reference_discriminator(dtype):
    if mg.SG2 not in sys.path:
        sys.path.insert(0, mg.SG2)
    import model as sg2
    d = sg2.Discriminator(dc.SIZE, channel_multiplier=dc.CHANNEL_MULTIPLIER).to(dtype)
    return dc.fill_weights(d)


def trainer_steps(B, dtype):
    (r0, f0), (r1, f1) = dc.images(B, dc.IMAGE_SEED + 100), dc.images(B, dc.IMAGE_SEED + 200)
    t = lambda a: torch.from_numpy(a).to(dtype)   # noqa: E731
    return [(t(r0), t(f0), 0), (t(r1), t(f1), 1)]


def main():
    torch.set_num_threads(8)
    out = {}
    runs = {}
    for dtype in (torch.float64, torch.float32):
        d = reference_discriminator(dtype)
        probe = dc.draw_like(d, dc.PROBE_SEED)
        for name, B in dc.CASES.items():
            real, fake = dc.images(B)
            lg = dc.logistic_pass(d, torch.from_numpy(real).to(dtype), torch.from_numpy(fake).to(dtype))
            rp = dc.r1_pass(d, torch.from_numpy(real).to(dtype))
            res = {"real_pred": lg["real_pred"], "fake_pred": lg["fake_pred"], "loss": lg["loss"],
                   "r1.real_pred": rp["real_pred"], "r1.grad_real": rp["grad_real"], "r1.per_sample": rp["per_sample"],
                   "r1.r1": rp["r1"]}
            res = {k: mg.np_(v.double()) for k, v in res.items()}
            res["log.norms"], res["log.proj"] = dc.summarize(lg["grads"], probe)
            res["r1.norms"], res["r1.proj"] = dc.summarize(rp["grads"], probe)
            runs[(dtype, name)] = res
            if dtype == torch.float64:
                out[f"{name}.real"], out[f"{name}.fake"] = real, fake
        runs[(dtype, "trainer")] = dc.reference_trainer(reference_discriminator(dtype), trainer_steps(4, dtype))
    for name in dc.CASES:
        r64, r32 = runs[(torch.float64, name)], runs[(torch.float32, name)]
        for k, v in r64.items():
            out[f"{name}.{k}"] = v
            diff = np.abs(r32[k] - v)
            out[f"{name}.e32_{k}"] = np.array(diff.max())
            print(name, k, "e32 max", float(diff.max()), "scale", float(np.abs(v).max()))
    w64, w32 = runs[(torch.float64, "trainer")], runs[(torch.float32, "trainer")]
    out["trainer.e32"] = np.array([float((w32[n].double() - w64[n]).abs().max()) for n in w64])
    print("trainer e32", out["trainer.e32"].min(), out["trainer.e32"].max())
    out["names"] = np.array(list(dc.CASES))
    out["params"] = np.array(list(w64))
    path = os.path.join(HERE, "dtrain.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
