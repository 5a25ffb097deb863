"""Cost of the centre crop of step 2: op/resample.py crop_resize, fused (g2s_resample_sep, one launch
each way) against composed (the torch composition resize -> crop -> resize it restates).

  * crop_resize alone, forward and forward + backward, at [8, 3, 128, 128] with crop 112 (origin 128, image 128) and
    at [8, 3, 512, 512] -> origin 160, crop 128, image 128: launches from the torch profiler, HIP-event time, and
    the time of a device copy that moves the same algorithmic bytes (the crop region read + the output written).
  * One eager training iteration of step 2 (zero_grad, forward, backward, Adam step) on face-128 with the crop on its
    fused route, on its composed route, and with the crop off.

HIP-event pairs around one call after a warm-up, the variants in ALTERNATING rounds so that clock and cache state are
shared; reported is the median over all rounds and the lowest and highest per-round median.  Random weights and
images (the timings do not depend on the values).  Writes profiles/crop_resize.json.

    python tools/bench_crop_resize.py [--quick] [--out profiles/crop_resize.json]"""
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
from gan2shape_amd.op import resample as rs
from gan2shape_amd.trainer import Trainer

from bench_manipulate import alternating
from bench_sweep import launches


def main():
    quick = "--quick" in sys.argv
    path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "crop_resize.json")
    lib.load()
    dev = torch.device("cuda")
    torch.manual_seed(0)
    rounds, n = (3, 5) if quick else (7, 20)
    result = dict(device=torch.cuda.get_device_name(0), rounds=rounds, samples_per_round=n, eager=True, crop_resize={},
                  step2={})

    # ---- crop_resize alone
    for tag, (N, gan, origin, crop, image) in (("g128_o128_c112_i128", (8, 128, 128, 112, 128)),
                                               ("g512_o160_c128_i128", (8, 512, 160, 128, 128))):
        x = (torch.rand(N, 3, gan, gan, device=dev) * 2 - 1).requires_grad_(True)
        g = torch.rand(N, 3, image, image, device=dev) * 2 - 1
        t = rs.crop_resize_tables(gan, origin, crop, image, dev)
        used = int((t.tr.host[1] > 0).sum())                       # input rows (= columns) inside the crop
        fwd_bytes = 4 * N * 3 * (used * used + image * image)     # crop region read + output written
        half = torch.empty(fwd_bytes // 8, device=dev), torch.empty(fwd_bytes // 8, device=dev)

        def fwd(fused):
            return lambda: rs.crop_resize(x.detach(), origin, crop, image, fused=fused)

        def fwd_bwd(fused):
            def run():
                y = rs.crop_resize(x, origin, crop, image, fused=fused)
                return torch.autograd.grad(y, x, g)
            return run
        row = dict(shape=[N, 3, gan, gan], origin_size=origin, crop=crop, image_size=image, rows_inside_crop=used,
                   taps_fwd=t.fwd.K, taps_transposed=t.tr.K, algorithmic_bytes_fwd=fwd_bytes,
                   tile_rows_fwd=lib.load().g2s_resample_tile_rows(gan, gan, image, image, t.fwd.K, t.fwd.K),
                   tile_rows_transposed=lib.load().g2s_resample_tile_rows(image, image, gan, gan, t.tr.K, t.tr.K))
        for what, make in (("forward", fwd), ("forward_backward", fwd_bwd)):
            routes = {"fused": make(True), "composed": make(False)}
            if what == "forward":
                routes["copy_same_bytes"] = lambda: half[0].copy_(half[1])
            times = alternating(routes, rounds, 5 * n)
            r = {k: dict(v, launches=launches(routes[k])) for k, v in times.items()}
            r["composed_over_fused"] = r["composed"]["median_ms"] / r["fused"]["median_ms"]
            if what == "forward":
                r["fused_over_copy"] = r["fused"]["median_ms"] / r["copy_same_bytes"]["median_ms"]
                r["fused_algorithmic_GBps"] = fwd_bytes / r["fused"]["median_ms"] / 1e6
            row[what] = r
        result["crop_resize"][tag] = row
        print(json.dumps({tag: row}), flush=True)

    # ---- one eager iteration of step 2: crop fused / crop composed / crop off
    n_proj = 8
    cfg = bench.face_config(n_proj=n_proj)
    cfg.update(crop=112, origin_size=128)
    t = Trainer(GAN2Shape, cfg, device=dev)
    m = t.model
    image, latent = bench.synthetic_sample(m, 1234, dev)
    with torch.no_grad():
        _, c1 = m.forward_step1(image, latent, None)
    zeropool.end()
    optim = t.optim_step2

    def iteration(crop, crop_fused):
        def run():
            m.crop, m.crop_fused = crop, crop_fused
            try:
                optim.zero_grad()
                loss, _ = m.forward_step2(image, latent, c1, n_proj_samples=n_proj)
                loss.backward()
                optim.step()
                zeropool.end()
            finally:
                m.crop, m.crop_fused = 112, None
            return loss
        return run
    routes = {"crop_fused": iteration(112, True), "crop_composed": iteration(112, False), "crop_off": iteration(None, None)}
    times = alternating(routes, rounds, n)
    row = {k: dict(v, launches=launches(routes[k])) for k, v in times.items()}
    row["composed_over_fused"] = row["crop_composed"]["median_ms"] / row["crop_fused"]["median_ms"]
    row["fused_over_off"] = row["crop_fused"]["median_ms"] / row["crop_off"]["median_ms"]
    result["step2"] = dict(workload="face128_n8", n_proj=n_proj, crop=112, origin_size=128, **row)
    print(json.dumps({"step2": result["step2"]}), flush=True)
    with open(path, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
