"""Training-monitor micro-benchmark: each fused call of monitor.py against the composition it replaces, written with
torch ops on the same CUDA tensors —

    grid      image_grid at [64, 3, 128, 128] (g2s_image_grid_u8: one launch) against monitor._image_grid_torch
    latents   ppl_latents at B = 64, D = 512 in both spaces (g2s_ppl_latents) against monitor._ppl_latents_torch
    batch     one path-length batch of 64 pairs at G(128, channel_multiplier 1) with a random LPIPS network: the route of
              perceptual_path_length (mapping kernel, latents kernel, one-node generator) against the same batch with
              style_forward, the latents composition and the generator's layer loop (Generator.ONE_NODE off; two
              forwards of 64 images, the most its noise kernel takes at 512 channels)

HIP-event pairs around one call; the routes alternate round by round so that a drift of the machine's clocks or load is
shared; reported is the median over all rounds and the lowest and highest per-round median; launches from the torch
profiler.  Writes profiles/monitor.json.

    python tools/bench_monitor.py [--quick] [--out profiles/monitor.json]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch

import gan2shape_amd  # noqa
from gan2shape_amd import generate, lib, monitor
from gan2shape_amd import stylegan2 as sg2
from gan2shape_amd.lpips import PerceptualLoss

from bench_manipulate import alternating
from bench_sweep import launches


def measure(routes, rounds, reps):
    times = alternating(routes, rounds, reps)
    row = {name: dict(v, launches=launches(routes[name])) for name, v in times.items()}
    row["composed_over_fused"] = row["composed"]["median_ms"] / row["fused"]["median_ms"]
    return row


def main():
    quick = "--quick" in sys.argv
    path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "monitor.json")
    lib.load()
    dev = torch.device("cuda")
    rounds, reps = (3, 10) if quick else (7, 50)
    result = dict(device=torch.cuda.get_device_name(0), rounds=rounds, samples_per_round=reps,
                  note="one call per sample, HIP events; composed = the torch composition on float32 CUDA tensors")
    g = torch.Generator(device=dev).manual_seed(0)

    x = torch.randn(64, 3, 128, 128, device=dev, generator=g)
    out = torch.empty(monitor.grid_shape(64, 128, 128)[2:] + (3,), dtype=torch.uint8, device=dev)
    routes = {"fused": lambda: monitor.image_grid(x, out=out),
              "composed": lambda: monitor._image_grid_torch(x, 8, 2, -1.0, 1.0, 0.0)}
    result["grid_64x3x128x128"] = measure(routes, rounds, reps)
    result["grid_64x3x128x128"]["bytes_differing"] = int((routes["fused"]() != routes["composed"]()).sum())
    print(json.dumps({"grid": result["grid_64x3x128x128"]}), flush=True)

    pairs = torch.randn(128, 512, device=dev, generator=g)
    t = torch.rand(64, device=dev, generator=g)
    for space in monitor.SPACES:
        routes = {"fused": lambda: monitor.ppl_latents(pairs, t, 1e-4, space),
                  "composed": lambda: monitor._ppl_latents_torch(pairs, t, 1e-4, space)}
        row = measure(routes, rounds, reps)
        row["max_abs_difference"] = float((routes["fused"]() - routes["composed"]()).abs().max())
        result[f"latents_b64_d512_{space}"] = row
        print(json.dumps({f"latents {space}": row}), flush=True)

    torch.manual_seed(0)
    G = sg2.Generator(128, 512, 8, channel_multiplier=1).to(dev).eval().requires_grad_(False)
    percept = PerceptualLoss().to(dev).eval()
    noise, z, t = monitor.ppl_draw(G, 64, "full", g)

    def fused():
        with torch.no_grad():
            lat = monitor.ppl_latents(generate.map_latents(G, z), t, 1e-4, "w")
            image, _ = G([lat], input_is_w=True, noise=list(noise))
            return percept(image[0::2], image[1::2]).view(64) / 1e-4 ** 2

    def composed():
        with torch.no_grad():
            lat = monitor._ppl_latents_torch(G.style_forward(z), t, 1e-4, "w")
            sg2.Generator.ONE_NODE = False
            try:        # the layer loop's noise kernel takes B * C < 65536: 128 images of 512 channels go as two halves
                image = torch.cat([G([h], input_is_w=True, noise=list(noise))[0] for h in (lat[:64], lat[64:])])
            finally:
                sg2.Generator.ONE_NODE = True
            return percept(image[0::2], image[1::2]).view(64) / 1e-4 ** 2

    routes = {"fused": fused, "composed": composed}
    row = measure(routes, max(rounds - 2, 3), max(reps // 5, 5))
    a, b = fused(), composed()
    row["max_relative_difference"] = float(((a - b).abs() / b.abs()).max())
    result["ppl_batch_64_g128"] = row
    print(json.dumps({"ppl batch": row}), flush=True)
    with open(path, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
