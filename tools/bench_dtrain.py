"""Discriminator-training benchmark: the logistic step and the R1 step of
gan2shape_amd.dtrain.DiscriminatorTrainer at D(128), channel_multiplier 1, B = 16 and B = 8, against the route a user
has without it on the same commit — the same discriminator on torch ops (F.conv2d with autograd, a depthwise F.conv2d
blur, the composed minibatch stddev and losses, torch.optim.Adam).  Each step is forward, backward and the optimiser
step.  HIP-event pairs around one Python call after a warm-up, the two routes in ALTERNATING rounds; reported is the
median over all samples and the lowest and highest per-round median, and the launches of one call (torch profiler).
Separately: the time of the g2s_conv2d_wgrad launches inside one step of each kind (event pairs around every launch)
and torch's weight gradient (torch.nn.grad.conv2d_weight) at the same shapes.  Writes profiles/dtrain_d128.json.

    python tools/bench_dtrain.py [--quick] [--out profiles/dtrain_d128.json]"""
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import torch.nn.functional as F

import gan2shape_amd  # noqa
from gan2shape_amd import dtrain, lib
from gan2shape_amd.op import conv2d_gradfix
from gan2shape_amd.stylegan2 import Blur, Discriminator, EqualConv2d, ResBlock

from bench_manipulate import alternating
from bench_sweep import launches

SIZE, CM = 128, 1


def torch_layer(layer, x):
    for m in layer:
        if isinstance(m, Blur):
            C = x.shape[1]
            x = F.pad(x, (m.pad[0], m.pad[1], m.pad[0], m.pad[1]))
            x = F.conv2d(x, m.kernel.flip(0, 1)[None, None].expand(C, 1, -1, -1), groups=C)[:, :, ::m.down, ::m.down]
        elif isinstance(m, EqualConv2d):
            x = F.conv2d(x, m.weight * m.scale, m.bias, stride=m.stride, padding=m.padding)
        else:
            x = F.leaky_relu(x + m.bias.view(1, -1, 1, 1), m.negative_slope) * m.scale
    return x


def torch_d(d, x):
    """Discriminator.forward on torch ops only, over d's own parameters."""
    for block in d.convs:
        if isinstance(block, ResBlock):
            x = (torch_layer(block.conv2, torch_layer(block.conv1, x)) + torch_layer(block.skip, x)) / math.sqrt(2)
        else:
            x = torch_layer(block, x)
    x = torch.cat([x, d._group_stddev(x)], 1)
    x = torch_layer(d.final_conv, x).flatten(1)
    lin0, lin1 = d.final_linear
    x = F.leaky_relu(F.linear(x, lin0.weight * lin0.scale) + lin0.bias * lin0.lr_mul, 0.2) * math.sqrt(2)
    return F.linear(x, lin1.weight * lin1.scale, lin1.bias * lin1.lr_mul)


class TorchTrainer:
    def __init__(self, d):
        self.d = d
        c = 16 / 17
        self.opt = torch.optim.Adam(d.parameters(), lr=0.002 * c, betas=(0 ** c, 0.99 ** c))

    def logistic(self, real, fake):
        loss = F.softplus(-torch_d(self.d, real)).mean() + F.softplus(torch_d(self.d, fake)).mean()
        self.d.zero_grad()
        loss.backward()
        self.opt.step()

    def r1(self, real):
        real = real.detach().requires_grad_(True)
        pred = torch_d(self.d, real)
        grad, = torch.autograd.grad(pred.sum(), real, create_graph=True)
        r1 = grad.pow(2).reshape(grad.shape[0], -1).sum(1).mean()
        self.d.zero_grad()
        (10 / 2 * r1 * 16 + 0 * pred[0]).backward()
        self.opt.step()


def native_steps(trainer):
    """(logistic step, R1 step) of DiscriminatorTrainer as separate calls: step() with i off / the R1 half alone."""
    def logistic(real, fake):
        trainer.step(real, fake, 1)

    def r1(real):
        with conv2d_gradfix.use():
            real = real.detach().requires_grad_(True)
            pred = trainer.d(real)[0]
            loss = dtrain.d_r1_loss(pred, real)
            trainer.d.zero_grad()
            (trainer.r1 / 2 * loss * trainer.d_reg_every + 0 * pred[0]).backward()
            trainer.d_optim.step()
    return logistic, r1


def wgrad_share(fn):
    """(ms in g2s_conv2d_wgrad launches during fn, [(A shape, G shape, k, stride, pad, ms)])."""
    rec = []
    orig = conv2d_gradfix._wgrad_launch

    def timed(A, G, k, stride, pad):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = orig(A, G, k, stride, pad)
        e1.record()
        rec.append((tuple(A.shape), tuple(G.shape), k, stride, pad, e0, e1))
        return out
    conv2d_gradfix._wgrad_launch = timed
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        conv2d_gradfix._wgrad_launch = orig
    rows = [(a, g, k, s, p, e0.elapsed_time(e1)) for a, g, k, s, p, e0, e1 in rec]
    return sum(r[-1] for r in rows), rows


def torch_wgrad_ms(rows, n=5):
    """torch.nn.grad.conv2d_weight at the same shapes (median of n after a warm-up), summed."""
    total, per = 0.0, []
    for a, g, k, s, p, ms in rows:
        A, G = torch.randn(a, device="cuda"), torch.randn(g, device="cuda")
        fn = lambda: torch.nn.grad.conv2d_weight(G, (a[1], g[1], k, k), A, stride=s, padding=p)   # noqa: E731
        fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(n):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
        t = float(np.median(ts))
        total += t
        per.append(dict(A=list(a), G=list(g), k=k, stride=s, pad=p, g2s_ms=ms, torch_ms=t))
    return total, per


def main():
    quick = "--quick" in sys.argv
    path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(
        ROOT, "profiles", "dtrain_d128.json")
    lib.load()
    dev = torch.device("cuda")
    rounds, n = (2, 3) if quick else (4, 8)
    result = dict(size=SIZE, channel_multiplier=CM, rounds=rounds, samples_per_round=n, batches=[])
    for B in (16, 8):
        torch.manual_seed(B)
        d_new, d_old = Discriminator(SIZE, CM).to(dev), Discriminator(SIZE, CM).to(dev)
        d_old.load_state_dict(d_new.state_dict())
        real, fake = torch.rand(B, 3, SIZE, SIZE, device=dev) * 2 - 1, torch.rand(B, 3, SIZE, SIZE, device=dev) * 2 - 1
        new_log, new_r1 = native_steps(dtrain.DiscriminatorTrainer(d_new))
        old = TorchTrainer(d_old)
        row = dict(B=B)
        for label, routes in (("logistic_step", dict(native=lambda: new_log(real, fake), torch=lambda: old.logistic(real, fake))),
                              ("r1_step", dict(native=lambda: new_r1(real), torch=lambda: old.r1(real)))):
            t = alternating(routes, rounds, n, warmup=2)
            wg_ms, rows = wgrad_share(routes["native"])
            tw_ms, per = torch_wgrad_ms(rows)
            row[label] = dict({name: dict(v, launches=launches(routes[name])) for name, v in t.items()},
                              torch_over_native=t["torch"]["median_ms"] / t["native"]["median_ms"],
                              wgrad=dict(launches=len(rows), g2s_ms=wg_ms, share_of_native_step=wg_ms / t["native"]["median_ms"],
                                         torch_conv2d_weight_ms=tw_ms, per_launch=per))
            print(json.dumps({k: v for k, v in row[label].items() if k != "wgrad"}), flush=True)
            print("wgrad", json.dumps({k: v for k, v in row[label]["wgrad"].items() if k != "per_launch"}), flush=True)
        result["batches"].append(row)
        del d_new, d_old, old
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
