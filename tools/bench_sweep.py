"""Viewing-path micro-benchmark at 128 x 128: Renderer.render_sweep (csrc/sweep.hip: three launches per sweep) against
the loop it stands beside, for the same poses and mode "texture":
    B = 1, the 120-frame turntable of visualize.turntable_rotations   against render_yaw(rotations=...)
    B = 8, the 14 poses of render_view                                against render_view
with tex_cube_size as configured (2).  Reported per route: the median of HIP-event pairs around one call after a
warm-up, the kernel launches of one call (torch profiler), the peak of torch's allocator during one call, and the
largest difference between the two results (the loop reads texture cubes with a clamp and an eps, the sweep
interpolates the vertex colours directly).  Then g2s_sweep_verts alone: achieved bytes/s (B*V*N*12 written + B*N*12
read) to hold against the HBM figure tools/bench_hbm_kernels.py prints on the same machine.

    python tools/bench_sweep.py [--quick]        # --quick: fewer repetitions"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import gan2shape_amd  # noqa
from gan2shape_amd import lib, visualize
from gan2shape_amd.renderer.renderer import Renderer

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


def launches(fn):
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA
               and not e.name.lower().startswith(("memcpy", "memset")))


def peak_mb(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def main():
    quick = "--quick" in sys.argv
    lib.load()
    dev = torch.device("cuda")
    r = Renderer({}, SIDE, 0.9, 1.1, device=dev)
    n = 5 if quick else 20
    y, x = torch.meshgrid(torch.linspace(-1, 1, SIDE), torch.linspace(-1, 1, SIDE), indexing="ij")
    turn = visualize.turntable_rotations(60)
    for B, label in ((1, "turntable V=120"), (8, "render_view V=14")):
        g = torch.Generator().manual_seed(B)
        depth = (1.0 - 0.06 * (1.2 - x * x - y * y))[None].repeat(B, 1, 1) + 0.002 * torch.rand(B, SIDE, SIDE, generator=g)
        im, depth = (torch.rand(B, 3, SIDE, SIDE, generator=g) * 2 - 1).to(dev), depth.to(dev)
        if B == 1:
            rot = turn.to(dev)

            def loop():
                return r.render_yaw(im, depth, rotations=turn[:, 1])
        else:
            rot = visualize.yaw_pitch_rotations().to(dev)

            def loop():
                return r.render_view(im, depth)

        def sweep():
            return r.render_sweep(im, depth, rot)
        a, b = sweep(), loop()
        diff = float((a.clamp(-1, 1) - b).abs().max())
        mean = float((a.clamp(-1, 1) - b).abs().mean())
        t_s, t_l = events(sweep, 2, n), events(loop, 1, max(3, n // 4))
        print(f"{label} {SIDE}x{SIDE} B={B}: render_sweep {t_s:8.3f} ms, {launches(sweep):4d} launches, peak "
              f"{peak_mb(sweep):7.1f} MiB | loop {t_l:8.3f} ms, {launches(loop):4d} launches, peak {peak_mb(loop):7.1f} MiB"
              f" | loop / sweep {t_l / t_s:5.1f}x | |difference| max {diff:.2e} mean {mean:.2e}", flush=True)
    # g2s_sweep_verts alone
    L = lib.load()
    for B, V in ((1, 120), (8, 14), (8, 120)):
        N = SIDE * SIDE
        verts = torch.rand(B, N, 3, device=dev)
        pose = torch.rand(B, V, 12, device=dev)
        out = torch.empty(B * V, N, 3, device=dev)

        def kernel():
            lib.check(L.g2s_sweep_verts(lib.ptr(verts), lib.ptr(pose), lib.ptr(out), B, V, N, lib.stream()))
        t = events(kernel, 5, 10 * n)
        nbytes = (B * V + B) * N * 12
        print(f"g2s_sweep_verts B={B} V={V} N={N}: {t * 1e3:8.1f} us, {nbytes / 2 ** 20:6.1f} MiB moved, "
              f"{nbytes / (t * 1e-3) / 1e12:5.2f} TB/s", flush=True)


if __name__ == "__main__":
    main()
