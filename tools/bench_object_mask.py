"""Cost of the object masks inside the steps on the face-128 workload.

  * Renderer.canon_mask alone, fused (g2s_canon_mask, one launch) against composed (the torch composition it restates:
    renderer.fused = False for this call only), at B = 1 (the instance trainer's step 1) and B = 8 (a joint batch):
    launches from the torch profiler, HIP-event time.
  * One eager training iteration (zero_grad, forward, backward, Adam step) of steps 1, 2 and 3 with the switch on
    against off, on the same model and weights (the switch is flipped on the model between the rounds).

HIP-event pairs around one call after a warm-up, the variants in ALTERNATING rounds so that clock and cache state are
shared; reported is the median over all rounds and the lowest and highest per-round median.  Random weights (the
timings do not depend on the values), a synthetic disc as the object mask.  Writes profiles/object_mask.json.

    python tools/bench_object_mask.py [--quick] [--out profiles/object_mask.json]"""
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


def disc(S, batch, dev):
    yy, xx = torch.meshgrid(torch.linspace(0, 1, S), torch.linspace(0, 1, S), indexing="ij")
    m = (((xx - 0.55) ** 2 + (yy - 0.45) ** 2) < 0.09).float()
    return m[None, None].expand(batch, 1, S, S).contiguous().to(dev)


def main():
    quick = "--quick" in sys.argv
    path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "object_mask.json")
    lib.load()
    dev = torch.device("cuda")
    torch.manual_seed(0)
    n_proj = 8
    cfg = bench.face_config(n_proj=n_proj)
    S = cfg["image_size"]
    t = Trainer(GAN2Shape, cfg, device=dev)
    m = t.model
    image, latent = bench.synthetic_sample(m, 1234, dev)
    mask = disc(S, 1, dev)
    rounds, n = (3, 5) if quick else (7, 20)
    result = dict(device=torch.cuda.get_device_name(0), workload="face128_n8", n_proj=n_proj, rounds=rounds,
                  samples_per_round=n, eager=True, canon_mask={}, steps={})

    # ---- Renderer.canon_mask alone
    r = m.renderer
    for B in (1, 8):
        g = torch.Generator().manual_seed(B)
        depth = (0.9 + 0.2 * torch.rand(B, S, S, generator=g)).to(dev)
        view = (torch.randn(B, 6, generator=g) * 0.2).to(dev)
        masks = disc(S, B, dev)
        r.set_view(view, 1.0, 0.1, 0.1)

        def call(fused):
            def run():
                r.fused = fused
                try:
                    return r.canon_mask(depth, masks)
                finally:
                    r.fused = True
            return run
        routes = {"fused": call(True), "composed": call(False)}
        times = alternating(routes, rounds, 5 * n)
        row = {k: dict(v, launches=launches(routes[k])) for k, v in times.items()}
        row["composed_over_fused"] = row["composed"]["median_ms"] / row["fused"]["median_ms"]
        result["canon_mask"][f"B{B}"] = row
        print(json.dumps({f"canon_mask B{B}": row}), flush=True)

    # ---- one eager iteration of every step, switch on against off
    def hand_offs(on):
        m.object_mask = on
        kw = dict(object_mask=mask) if on else {}
        with torch.no_grad():
            _, c1 = m.forward_step1(image, latent, None, **kw)
            _, c2 = m.forward_step2(image, latent, c1, n_proj_samples=n_proj)
        zeropool.end()
        return c1, c2
    src = {on: dict(zip((2, 3), hand_offs(on))) for on in (False, True)}
    m.object_mask = False

    def iteration(kind, on):
        optim = getattr(t, f"optim_step{kind}")
        kw = dict(object_mask=mask) if on else {}

        def run():
            m.object_mask = on
            try:
                optim.zero_grad()
                loss, _ = getattr(m, f"forward_step{kind}")(image, latent, src[on].get(kind), n_proj_samples=n_proj, **kw)
                loss.backward()
                optim.step()
                zeropool.end()
            finally:
                m.object_mask = False
            return loss
        return run
    for kind in (1, 2, 3):
        routes = {"object_mask_off": iteration(kind, False), "object_mask_on": iteration(kind, True)}
        times = alternating(routes, rounds, n)
        row = {k: dict(v, launches=launches(routes[k])) for k, v in times.items()}
        row["on_over_off"] = row["object_mask_on"]["median_ms"] / row["object_mask_off"]["median_ms"]
        result["steps"][f"step{kind}"] = row
        print(json.dumps({f"step{kind}": row}), flush=True)
    with open(path, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
