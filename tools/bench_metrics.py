"""Depth-metrics micro-benchmark: one depth_metrics call at 128 x 128, B = 1 and B = 64 — the kernel route
(g2s_depth_metrics, csrc/metrics.hip: two launches) against the torch composition of the same definitions run on
the GPU (metrics._depth_metrics_torch on CUDA tensors: what a user without the kernel would write, about 40
launches).  Both masks are given, erosion is on.  Times are medians of HIP-event pairs around one call after a
warm-up; the wall time of a synchronised call is printed as well.

    python tools/bench_metrics.py [--quick]        # --quick: fewer repetitions"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import gan2shape_amd  # noqa
from gan2shape_amd import lib, metrics
import metrics_cases as mc

SIDE = 128


def events(fn, warmup, n):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
    for e0, e1 in ev:
        e0.record()
        fn()
        e1.record()
    torch.cuda.synchronize()
    return float(np.median([e0.elapsed_time(e1) for e0, e1 in ev]))


def wall(fn, n):
    times = []
    for _ in range(n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return float(np.median(times)) * 1e3


def main():
    quick = "--quick" in sys.argv
    lib.load()
    renderer = mc.CaseRenderer(SIDE)
    n = 20 if quick else 100
    for B in (1, 64):
        rng = np.random.default_rng(B)
        pred, gt = (torch.from_numpy(mc.smooth_depth(rng, B, SIDE, SIDE)).cuda() for _ in range(2))
        mp, mg = (torch.from_numpy((rng.random((B, SIDE, SIDE)) > 0.002).astype(np.float32)).cuda() for _ in range(2))
        rays = renderer._pixel_rays(SIDE, SIDE, pred.device)

        def kernel():
            return metrics.depth_metrics(pred, gt, mp, mg, renderer=renderer)

        def composed():
            return metrics._depth_metrics_torch(pred, gt, mp, mg, rays, True)
        a, b = kernel(), composed()
        diff = max(float((a[k] - b[k]).abs().max()) for k in metrics.KEYS)
        t_k, t_c = events(kernel, 5, n), events(composed, 5, n)
        w_k, w_c = wall(kernel, n), wall(composed, n)
        print(f"depth_metrics {SIDE}x{SIDE} B={B:3d}: kernel {t_k * 1e3:8.1f} us ({w_k * 1e3:8.1f} wall) | "
              f"torch on the GPU {t_c * 1e3:8.1f} us ({w_c * 1e3:8.1f} wall) | torch / kernel {t_c / t_k:5.1f}x | "
              f"max |difference| {diff:.1e}", flush=True)


if __name__ == "__main__":
    main()
