"""Image-metrics micro-benchmark: one image_metrics call — the kernel route (g2s_image_metrics, csrc/image_metrics.hip:
two launches) against the float32 torch composition of the same definitions run on the GPU
(metrics._image_metrics_torch on CUDA tensors: what a user without the kernel would write) — at [1, 3, 128, 128],
[64, 3, 128, 128] and [8, 3, 256, 256], masked and unmasked.

HIP-event pairs around one call; the routes alternate round by round so that a drift of the machine's clocks or load is
shared; reported is the median over all rounds and the lowest and highest per-round median; launches from the torch
profiler.  Writes profiles/image_metrics.json.

    python tools/bench_image_metrics.py [--quick] [--out profiles/image_metrics.json]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch

import gan2shape_amd  # noqa
from gan2shape_amd import lib, metrics
import image_metrics_cases as ic

from bench_manipulate import alternating
from bench_sweep import launches

SHAPES = [(1, 3, 128, 128), (64, 3, 128, 128), (8, 3, 256, 256)]


def main():
    quick = "--quick" in sys.argv
    path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "image_metrics.json")
    lib.load()
    rounds, reps = (3, 10) if quick else (7, 50)
    result = dict(device=torch.cuda.get_device_name(0), rounds=rounds, samples_per_round=reps, data_range=2.0,
                  note="one call per sample, HIP events; composed = metrics._image_metrics_torch on float32 CUDA tensors",
                  shapes={})
    for B, C, H, W in SHAPES:
        rng = np.random.default_rng(B + H)
        a, b = (torch.from_numpy(v).cuda() for v in ic.smooth_pair(rng, B, C, H, W))
        ellipse = torch.from_numpy(np.stack([ic.ellipse(H, W)] * B)).cuda()
        for masked, mask in (("masked", ellipse), ("unmasked", None)):
            def kernel():
                return metrics.image_metrics(a, b, mask, data_range=2.0)

            def composed():
                return metrics._image_metrics_torch(a, b, mask, 2.0)
            k, c = kernel(), composed()
            torch.cuda.synchronize()
            diff = {key: float((k[key] - c[key]).abs().max()) for key in metrics.IMAGE_KEYS}
            routes = {"kernel": kernel, "composed": composed}
            times = alternating(routes, rounds, reps)
            row = {name: dict(v, launches=launches(routes[name])) for name, v in times.items()}
            row["composed_over_kernel"] = row["composed"]["median_ms"] / row["kernel"]["median_ms"]
            row["max_abs_difference"] = diff
            result["shapes"][f"{B}x{C}x{H}x{W}_{masked}"] = row
            print(json.dumps({f"{B}x{C}x{H}x{W} {masked}": row}), flush=True)
    with open(path, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
