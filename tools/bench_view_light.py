"""Cost of fitting the view and light priors.

  * mvn_fit alone: g2s_mvn_fit (ONE launch of one workgroup, csrc/mvn.hip) against the torch composition on the
    device (rows.mean(0), torch.cov(rows.T), torch.linalg.cholesky of the 6 x 6 and of the 4 x 4 block), on rows
    [1000, 10] and [100000, 10] already on the device.  Both routes are timed without the status read-back.
  * fit_view_light on the face-128 model over 256 synthetic images held on the host, at batch 1 and at batch 64:
    images per second of the whole call (stack, upload, V and L nets, the fit and its status read-back).

HIP-event pairs around one call after a warm-up, the variants in ALTERNATING rounds so that clock and cache state are
shared; reported is the median over all rounds and the lowest and highest per-round median; launches from the torch
profiler.  Random weights and rows (the timings do not depend on the values).  Writes profiles/view_light.json.

    python tools/bench_view_light.py [--quick] [--out profiles/view_light.json]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch

import bench
import gan2shape_amd  # noqa
from gan2shape_amd import lib, view_light
from gan2shape_amd.model import GAN2Shape
from gan2shape_amd.trainer import Trainer

from bench_manipulate import alternating
from bench_sweep import launches


def main():
    quick = "--quick" in sys.argv
    path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "view_light.json")
    lib.load()
    dev = torch.device("cuda")
    torch.manual_seed(0)
    rounds, reps = (3, 5) if quick else (7, 20)
    result = dict(device=torch.cuda.get_device_name(0), rounds=rounds,
                  samples_per_round=dict(mvn_fit=10 * reps, fit_view_light=2),
                  note="mvn_fit: both routes without the status read-back; fit_view_light: the whole call, 256 host images",
                  mvn_fit={}, fit_view_light={})

    # ---- the fit alone
    for N in (1000, 100000):
        g = torch.Generator().manual_seed(N)
        rows = (torch.randn(N, 10, generator=g) @ (torch.randn(10, 10, generator=g) / 3 + torch.eye(10))).to(dev)
        out = [torch.empty(n, device=dev) for n in (10, 100, 100)] + [torch.empty(1, dtype=torch.int32, device=dev)]

        def kernel():
            view_light.mvn_fit_launch(rows, N, 10, 10, (6, 4), 0.0, *out)
            return out

        def composed():
            cov = torch.cov(rows.t())
            return rows.mean(0), cov, torch.linalg.cholesky(cov[:6, :6]), torch.linalg.cholesky(cov[6:, 6:])
        k, c = kernel(), composed()
        torch.cuda.synchronize()
        assert int(k[3].item()) == 0 and torch.allclose(k[1].view(10, 10), c[1], rtol=1e-3, atol=1e-5)
        routes = {"mvn_fit": kernel, "composed": composed}
        times = alternating(routes, rounds, 10 * reps)
        row = {name: dict(v, launches=launches(routes[name])) for name, v in times.items()}
        row["composed_over_mvn_fit"] = row["composed"]["median_ms"] / row["mvn_fit"]["median_ms"]
        row["bytes_read_per_pass"] = 4 * N * 10
        result["mvn_fit"][f"N{N}"] = row
        print(json.dumps({f"mvn_fit N{N}": row}), flush=True)

    # ---- the whole fit on the face-128 model
    model = Trainer(GAN2Shape, bench.face_config(n_proj=2), device=dev).model
    S, n = model.image_size, 64 if quick else 256
    images = list(torch.tanh(torch.randn(n, 3, S, S, generator=torch.Generator().manual_seed(1))))
    routes = {f"batch{b}": (lambda b=b: view_light.fit_view_light(model, images, batch=b, ridge=1e-6)) for b in (1, 64)}
    times = alternating(routes, rounds, 2)
    for name, v in times.items():
        result["fit_view_light"][name] = dict(v, images=n, images_per_s=1e3 * n / v["median_ms"])
    print(json.dumps({"fit_view_light": result["fit_view_light"]}), flush=True)
    with open(path, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
