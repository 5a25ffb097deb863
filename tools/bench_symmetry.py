"""Cost of the symmetry flips on the face-128 workload: one training iteration (zero_grad, forward,
backward, Adam step) of step 1 and of step 3 with flips off, with flips on through the g2s_mirror_pair kernel
(renderer.fused = True) and with flips on through the torch composition cat / flip (renderer.fused = False: the
whole geometry chain then runs op by op, so a third variant keeps the fused geometry kernels and swaps ONLY the
mirror for cat / flip — the comparison the kernel answers for).  HIP-event pairs around one iteration after a warm-up,
the variants in ALTERNATING rounds so that clock and cache state are shared; reported is the median over all rounds
and the lowest and highest per-round median.  Launches come from the torch profiler.  Random weights (the timings
do not depend on the values).  Writes profiles/symmetry.json.

    python tools/bench_symmetry.py [--quick] [--out profiles/symmetry.json]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch

import bench
import gan2shape_amd  # noqa
from gan2shape_amd import lib, zeropool
from gan2shape_amd.model import GAN2Shape
from gan2shape_amd.trainer import Trainer

from bench_manipulate import alternating
from bench_sweep import launches


def main():
    quick = "--quick" in sys.argv
    path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "symmetry.json")
    lib.load()
    dev = torch.device("cuda")
    torch.manual_seed(0)
    n_proj = 8
    t = Trainer(GAN2Shape, bench.face_config(n_proj=n_proj), device=dev)
    m = t.model
    image, latent = bench.synthetic_sample(m, 1234, dev)
    with torch.no_grad():
        _, c1 = m.forward_step1(image, latent, None)
        _, c2 = m.forward_step2(image, latent, c1, n_proj_samples=n_proj)
    zeropool.end()
    torch_mirror = GAN2Shape._mirror_rows

    def mirror_by_cat(self, depth, albedo, repeat=1):      # the composed mirror with everything else fused
        fused, self.renderer.fused = self.renderer.fused, False
        try:
            return torch_mirror(self, depth, albedo, repeat)
        finally:
            self.renderer.fused = fused

    def iteration(kind, flip, fused, cat_mirror=False):
        optim = getattr(t, f"optim_step{kind}")
        src = {1: None, 3: c2}[kind]

        def run():
            m.flip1 = m.flip3 = flip
            m.renderer.fused = fused
            if cat_mirror:
                m._mirror_rows = mirror_by_cat.__get__(m)
            try:
                optim.zero_grad()
                loss, _ = getattr(m, f"forward_step{kind}")(image, latent, src, n_proj_samples=n_proj)
                loss.backward()
                optim.step()
                zeropool.end()
            finally:
                m.flip1 = m.flip3 = False
                m.renderer.fused = True
                if cat_mirror:
                    del m._mirror_rows
            return loss
        return run
    rounds, n = (3, 5) if quick else (7, 20)
    result = dict(workload="face128_n8", n_proj=n_proj, rounds=rounds, samples_per_round=n, eager=True, steps={})
    for kind in (1, 3):
        routes = {"flips_off": iteration(kind, False, True),
                  "flips_on_mirror_pair": iteration(kind, True, True),
                  "flips_on_cat_flip_mirror_only": iteration(kind, True, True, cat_mirror=True),
                  "flips_on_composed_route": iteration(kind, True, False),
                  "flips_off_composed_route": iteration(kind, False, False)}
        times = alternating(routes, rounds, n)
        row = {k: dict(v, launches=launches(routes[k])) for k, v in times.items()}
        off, on = row["flips_off"]["median_ms"], row["flips_on_mirror_pair"]["median_ms"]
        row["flipped_over_plain"] = on / off
        row["cat_flip_mirror_over_mirror_pair"] = row["flips_on_cat_flip_mirror_only"]["median_ms"] / on
        result["steps"][f"step{kind}"] = row
        print(json.dumps({f"step{kind}": row}), flush=True)
    with open(path, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
