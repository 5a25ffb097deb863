"""Cost of the projected-sample bank (config `collect_iters`).

  * The gather alone: SampleBank.gather_into (g2s_bank_gather, ONE launch: b image rows, b mask rows and the input
    image as row 0 of the step-3 batch) against the composed route (device index_select of the images, of the masks,
    and the cat of the image in front: three launches), from a bank of K * n = 800 rows, b = 8, at S = 128 and
    S = 256, the index already on the device in both routes.
  * One eager step-3 iteration (zero_grad, forward, backward, Adam step) on the face-128 workload in three forms:
    `bank_on` (host draw, upload, gather, forward_step3 on the prebuilt batch), `composed` (the same draw and upload,
    two index_selects, forward_step3 on the plain tuple: the cat runs inside the step) and `parent` (forward_step3 on
    one fixed step-2 hand-off, the step as it was before the bank: no draw, no gather; this commit's code on the old
    path, not a build of the parent commit).

HIP-event pairs around one call after a warm-up, the variants in ALTERNATING rounds so that clock and cache state are
shared; reported is the median over all rounds and the lowest and highest per-round median; launches from the torch
profiler.  Random weights and samples (the timings do not depend on the values).  Writes profiles/sample_bank.json.

    python tools/bench_sample_bank.py [--quick] [--out profiles/sample_bank.json]"""
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
from gan2shape_amd.bank import SampleBank
from gan2shape_amd.model import GAN2Shape
from gan2shape_amd.trainer import Trainer

from bench_manipulate import alternating
from bench_sweep import launches


def filled_bank(K, n, S, dev, seed):
    g = torch.Generator().manual_seed(seed)
    bank = SampleBank(K, n, S, device=dev)
    for _ in range(K):
        bank.put(torch.rand(n, 3, S, S, generator=g).mul_(2).sub_(1).to(dev), (torch.rand(n, 1, S, S, generator=g) > 0.3).float().to(dev))
    return bank


def main():
    quick = "--quick" in sys.argv
    path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "sample_bank.json")
    lib.load()
    dev = torch.device("cuda")
    torch.manual_seed(0)
    K, n, b = 100, 8, 8
    rounds, reps = (3, 5) if quick else (7, 20)
    result = dict(device=torch.cuda.get_device_name(0), bank_rows=K * n, b=b, rounds=rounds,
                  samples_per_round=dict(gather=10 * reps, step3=reps),
                  note="`parent` is this commit's forward_step3 fed one fixed step-2 hand-off (the step as it was before "
                       "the bank: no draw, no gather, the cat inside), not a build of the parent commit",
                  gather={}, step3={})

    # ---- the gather alone
    for S in (128, 256):
        bank = filled_bank(K, n, S, dev, S)
        image = torch.rand(1, 3, S, S, device=dev)
        idx = bank.indices(b).to(dev)
        batch = torch.empty(1 + b, 3, S, S, device=dev)
        masks = torch.empty(b, 1, S, S, device=dev)

        def fused():
            bank.gather_into(idx, image, batch, masks)
            return batch, masks

        def composed():
            return torch.cat([image, bank.images.index_select(0, idx)], 0), bank.masks.index_select(0, idx)
        a, c = fused(), composed()
        assert torch.equal(a[0], c[0]) and torch.equal(a[1], c[1])
        routes = {"gather": fused, "composed": composed}
        times = alternating(routes, rounds, 10 * reps)
        row = {k: dict(v, launches=launches(routes[k])) for k, v in times.items()}
        row["composed_over_gather"] = row["composed"]["median_ms"] / row["gather"]["median_ms"]
        row["bytes_moved"] = 2 * 4 * ((1 + b) * 3 + b) * S * S
        result["gather"][f"S{S}"] = row
        print(json.dumps({f"gather S{S}": row}), flush=True)
        del bank

    # ---- one eager step-3 iteration on the face-128 workload
    cfg = bench.face_config(n_proj=n)
    S = cfg["image_size"]
    t = Trainer(GAN2Shape, cfg, device=dev)
    m = t.model
    image, latent = bench.synthetic_sample(m, 1234, dev)
    with torch.no_grad():
        _, c1 = m.forward_step1(image, latent, None)
        _, c2 = m.forward_step2(image, latent, c1, n_proj_samples=n)
    zeropool.end()
    bank = filled_bank(K, n, S, dev, 7)
    bank.put(*c2)
    optim = t.optim_step3

    def iteration(source):
        def run():
            optim.zero_grad()
            loss, _ = m.forward_step3(image, latent, source())
            loss.backward()
            optim.step()
            zeropool.end()
            return loss
        return run

    def composed_source():
        idx = bank.indices(b).to(dev)
        return bank.images.index_select(0, idx), bank.masks.index_select(0, idx)
    routes = {"bank_on": iteration(lambda: bank.gather(bank.indices(b), image)),
              "composed": iteration(composed_source),
              "parent": iteration(lambda: c2)}
    times = alternating(routes, rounds, reps)
    row = {k: dict(v, launches=launches(routes[k])) for k, v in times.items()}
    row["bank_on_over_composed"] = row["bank_on"]["median_ms"] / row["composed"]["median_ms"]
    row["bank_on_over_parent"] = row["bank_on"]["median_ms"] / row["parent"]["median_ms"]
    result["step3"]["face128_n8"] = row
    print(json.dumps({"step3 face128_n8": row}), flush=True)
    with open(path, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
