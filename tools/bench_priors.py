"""Depth-prior micro-benchmark: the host path of PriorGenerator (CPU mask, F.conv2d / torch.nonzero, a copy
to the device, one image after the other — what the joint trainer does per data set) against the device
path (PriorGenerator(on_device=True).batch, csrc/priors.hip), for `ellipsoid` and `smoothed_box` at
S = 128 with B = 1, 8, 64 and S = 256 with B = 8.  The masks are already on the device, as a parsing
network would leave them.  Wall times are medians over calls that start and end synchronised (the host
path is host work, HIP events would not see it); for the device path the HIP-event time of the launches
is printed as well."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import gan2shape_amd  # noqa
from gan2shape_amd import lib, priors
from model_cases import parsing_mask

CASES = [(128, 1), (128, 8), (128, 64), (256, 8)]


def wall(fn, warmup, n):
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return float(np.median(times)) * 1e6


def events(fn, warmup=20, n=200):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
    for e0, e1 in ev:
        e0.record()
        fn()
        e1.record()
    torch.cuda.synchronize()
    return float(np.median([e0.elapsed_time(e1) for e0, e1 in ev])) * 1e3


def main():
    lib.load()
    rng = np.random.default_rng(0)
    for S, B in CASES:
        masks = torch.cat([parsing_mask(S, *(0.5 + 0.1 * rng.uniform(-1, 1, 2)), *(0.3 + 0.08 * rng.uniform(-1, 1, 2)))
                           for _ in range(B)]).cuda()
        images = masks.expand(-1, 3, -1, -1).contiguous()

        def source(image):
            return image[:, :1]
        for name in ("ellipsoid", "smoothed_box"):
            host = priors.PriorGenerator(S, "face", name, masking_model=source)
            device = priors.PriorGenerator(S, "face", name, masking_model=source, on_device=True, mask_accepts_batch=True)

            def run_host():
                return [host(images[i:i + 1], device="cuda") for i in range(B)]

            def run_device():
                return device.batch(images, device="cuda")
            err = float((torch.cat(run_host()) - run_device()).abs().max())
            t_h = wall(run_host, 2, 5 if B >= 8 else 20)
            t_d = wall(run_device, 20, 100)
            t_e = events(run_device)
            print(f"S={S} B={B:2d} {name:13s}: host {t_h:10.1f} us | device {t_d:8.1f} us wall, {t_e:7.1f} us HIP events | "
                  f"host / device {t_h / t_d:7.1f}x | max |host - device| {err:.1e}", flush=True)


if __name__ == "__main__":
    main()
