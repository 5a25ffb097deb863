"""Generator training steps at G(128), channel multiplier 1 -> profiles/gtrain_g128.json.

    python tools/bench_gtrain.py [--rounds 5] [--out profiles/gtrain_g128.json]

Per batch size (16, 8) and step kind (the non-saturating step; the path-length step at batch / 2): HIP-event medians
over alternating rounds of the native route (conv2d_gradfix.use(): the twice-differentiable modulated convolution with
g2s_modconv_wgrad) and of the same generator with its modulated convolutions on torch ops (x * s, F.conv2d /
F.conv_transpose2d autograd, * demod), with per-round ranges; kernel launch counts (`launches`; memsets and copies apart, as `memops`) and the share of device time in
g2s_modconv_wgrad from one profiled step; and `accumulate` in one launch against the per-parameter loop."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gan2shape_amd  # noqa: E402,F401
from gan2shape_amd import gtrain  # noqa: E402
from gan2shape_amd.op import conv2d_gradfix as gradfix  # noqa: E402
from gan2shape_amd.stylegan2 import Discriminator, Generator  # noqa: E402

SIZE, LATENT, N_MLP = 128, 512, 8


def torch_modconv(x, w, s=None, demod=None, mode=gradfix.PLAIN):
    xs = x if s is None else x * s[:, :, None, None]
    k = w.shape[2]
    if mode == gradfix.PLAIN:
        y = F.conv2d(xs, w, padding=k // 2)
    elif mode == gradfix.DOWN2:
        y = F.conv2d(xs, w, stride=2)
    else:
        y = F.conv_transpose2d(xs, w.transpose(0, 1), stride=2)
    return y if demod is None else y * demod[:, :, None, None]


class torch_route:
    """Within the block the modulated convolution under use() is the torch composition."""

    def __enter__(self):
        self.orig = gradfix.modulated_conv2d
        gradfix.modulated_conv2d = torch_modconv

    def __exit__(self, *exc):
        gradfix.modulated_conv2d = self.orig


def ns_step(g, d, zs):
    with gradfix.use():
        fake, _ = g(zs)
        loss = gtrain.g_nonsaturating_loss(gtrain._pred(d(fake)))
        g.zero_grad()
        loss.backward()


def path_step(g, d, zs):
    with gradfix.use():
        fake, latents = g(zs, return_latents=True)
        pen, _, _ = gtrain.g_path_regularize(fake, latents, 0.0)
        g.zero_grad()
        (8 * pen + 0 * fake[0, 0, 0, 0]).backward()


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def profile(fn):
    from torch.profiler import ProfilerActivity, profile as prof
    with prof(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as p:
        fn()
        torch.cuda.synchronize()
    launches, memops, total, wgrad = 0, 0, 0.0, 0.0
    for ev in p.events():
        if ev.device_type == torch.autograd.DeviceType.CUDA:
            total += ev.device_time
            if ev.name.startswith(("Memset", "Memcpy")):     # e.g. the clear before a split-K weight gradient
                memops += 1
                continue
            launches += 1
            if "modconv_wgrad" in ev.name:
                wgrad += ev.device_time
    return {"launches": launches, "memops": memops, "device_us": total,
            "modconv_wgrad_share": wgrad / total if total else 0.0}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(__file__), "..", "profiles", "gtrain_g128.json"))
    args = ap.parse_args()
    torch.manual_seed(0)
    g = Generator(SIZE, LATENT, N_MLP, channel_multiplier=1).cuda().train()
    g_ema = Generator(SIZE, LATENT, N_MLP, channel_multiplier=1).cuda().eval()
    d = Discriminator(SIZE, channel_multiplier=1).cuda().requires_grad_(False)
    result = {"size": SIZE, "channel_multiplier": 1, "rounds": args.rounds, "device": torch.cuda.get_device_name(0),
              "cases": []}
    for B in (16, 8):
        for kind, step, b in (("nonsaturating", ns_step, B), ("path", path_step, B // 2)):
            zs = [torch.randn(b, LATENT, device="cuda")]
            routes = {"native": lambda: step(g, d, zs)}

            def on_torch(step=step, zs=zs):
                with torch_route():
                    step(g, d, zs)
            routes["torch"] = on_torch
            for fn in routes.values():      # warm-up: tables, allocator
                fn()
                fn()
            torch.cuda.synchronize()
            times = {name: [] for name in routes}
            for _ in range(args.rounds):    # alternating rounds
                for name, fn in routes.items():
                    times[name].append(statistics.median(timed(fn) for _ in range(5)))
            row = {"batch": B, "step": kind, "step_batch": b}
            for name, fn in routes.items():
                row[name] = {"median_ms": statistics.median(times[name]), "round_min_ms": min(times[name]),
                             "round_max_ms": max(times[name]), **profile(fn)}
            row["native_over_torch"] = row["native"]["median_ms"] / row["torch"]["median_ms"]
            print(json.dumps(row))
            result["cases"].append(row)
    ema = {"one_launch": lambda: gtrain.accumulate(g_ema, g, gtrain.GeneratorTrainer.EMA_DECAY)}

    def per_parameter():
        par1, par2 = dict(g_ema.named_parameters()), dict(g.named_parameters())
        for k in par1:
            par1[k].data.mul_(0.999).add_(par2[k].data, alpha=0.001)
    ema["per_parameter"] = per_parameter
    row = {"parameters": sum(p.numel() for p in g.parameters()), "tensors": len(list(g.parameters()))}
    for name, fn in ema.items():
        fn()
        torch.cuda.synchronize()
        t = [statistics.median(timed(fn) for _ in range(5)) for _ in range(args.rounds)]
        row[name] = {"median_ms": statistics.median(t), "round_min_ms": min(t), "round_max_ms": max(t)}
    print(json.dumps(row))
    result["accumulate"] = row
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
