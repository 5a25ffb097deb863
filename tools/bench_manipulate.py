"""Manipulation-path benchmark at 128 x 128:
    (a) Renderer.render_pseudo_sweep (three launches per chunk, csrc/sweep.hip: g2s_sweep_pseudo) against the existing
        composition, GAN2Shape.sample_pseudo_imgs(_draws=...), for the SAME views and lights at V = 8 and V = 120;
    (b) GAN2Shape.manipulate end to end at V = 120 (decomposition, frames, encoder, generator in chunks of 8).
Per route: HIP-event pairs around one Python call after a warm-up, the two routes of (a) in ALTERNATING rounds so that
clock and cache state are shared; reported is the median over all rounds and the spread of the per-round medians.
Launches come from the torch profiler.  The model is the face configuration with random weights (the timings do not
depend on the values).  Writes profiles/manipulate_g128.json.

    python tools/bench_manipulate.py [--quick] [--out profiles/manipulate_g128.json]"""
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import bench
import gan2shape_amd  # noqa
from gan2shape_amd import lib
from gan2shape_amd.model import GAN2Shape, light_sweep, rotation_views

from bench_sweep import launches


def timed(fn, n):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
    for e0, e1 in ev:
        e0.record()
        fn()
        e1.record()
    torch.cuda.synchronize()
    return [e0.elapsed_time(e1) for e0, e1 in ev]


def alternating(routes, rounds, n, warmup=3):
    """{name: fn} -> {name: (median ms over all samples, lowest and highest per-round median)}."""
    for fn in routes.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    samples = {k: [] for k in routes}
    for _ in range(rounds):
        for k, fn in routes.items():
            samples[k].append(timed(fn, n))
    out = {}
    for k, rs in samples.items():
        per_round = [float(np.median(r)) for r in rs]
        out[k] = dict(median_ms=float(np.median(np.concatenate(rs))), round_min_ms=min(per_round),
                      round_max_ms=max(per_round))
    return out


def main():
    quick = "--quick" in sys.argv
    path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(
        ROOT, "profiles", "manipulate_g128.json")
    lib.load()
    dev = torch.device("cuda")
    torch.manual_seed(0)
    m = GAN2Shape(bench.face_config(n_proj=8), device=dev)
    image, latent = bench.synthetic_sample(m, 1234, dev)
    d = m.decompose(image)
    normal, la, lb, albedo, depth, _ = d["collected"]
    alpha = m.rand_light[6]
    rounds, n = (3, 5) if quick else (5, 20)
    result = dict(side=m.image_size, rounds=rounds, samples_per_round=n, sweep=[])
    for V in (8, 120):
        g = torch.Generator().manual_seed(V)
        draws = (torch.rand(V, 2, generator=g).to(dev) - 0.3, (torch.rand(V, 1, 1, 1, generator=g) * 0.7 - 0.1).to(dev),
                 (torch.randn(V, 6, generator=g) * 0.3).to(dev))
        views = m.get_view_transformation(draws[2])
        ab = torch.cat([la[:1].reshape(1, 1), lb[:1].reshape(1, 1)], 1) * 2 - 1
        lights = torch.cat([ab + draws[1].view(-1, 1) * torch.tensor([[2.0 * alpha, 2.0]], device=dev), draws[0]], 1)

        def fused():
            return m.renderer.render_pseudo_sweep(albedo, normal, depth, views, lights)

        def composed():
            with torch.no_grad():
                return m.sample_pseudo_imgs(V, normal, la, lb, albedo, depth, None, _draws=draws)
        a, b = fused(), composed()
        off = float(((a[0][0] - b[0]).abs() > 2e-3).float().mean())
        t = alternating(dict(render_pseudo_sweep=fused, sample_pseudo_imgs=composed), rounds, n)
        row = dict(V=V, **{k: dict(v, launches=launches(fn)) for (k, v), fn in zip(t.items(), (fused, composed))},
                   composed_over_fused=t["sample_pseudo_imgs"]["median_ms"] / t["render_pseudo_sweep"]["median_ms"],
                   share_of_pixels_off_by_2e3=off)
        result["sweep"].append(row)
        print(json.dumps(row), flush=True)
    views = rotation_views(60, 120).to(dev)

    def whole():
        return m.manipulate(image, latent, views, gan_batch=8)
    t = alternating(dict(manipulate=whole), rounds, max(2, n // 4), warmup=2)
    result["manipulate"] = dict(V=120, gan_batch=8, **t["manipulate"], launches=launches(whole))
    print(json.dumps(result["manipulate"]), flush=True)
    lit = m.manipulate(image, latent, torch.zeros(4, 6), light_sweep(0.0, 0.0, 4, 0.5).to(dev))
    assert math.isfinite(float(lit["gan"].abs().max()))
    with open(path, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
