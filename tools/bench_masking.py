"""MaskingModel micro-benchmark: ms per image of image_mask and confidence_mask at full size (BiSeNet at 512 for
'face', PSPNet at 473 for 'car'), image side 128, B = 1 and 8 — the libg2s route (folded convolutions on g2s_conv2d,
csrc/parsing.hip, g2s_parse_head) against the native=True route of the same module (torch / MIOpen ops, full-resolution
logits, argmax and resizes in torch).  Weights come from the seed recipe of tests/parsing_cases.py: timings do not
depend on their values.  Times are medians of HIP-event pairs around one call; wall time of a synchronised call is
printed as well (the native route of the reference synchronises three times per mask; this module's does not).

    python tools/bench_masking.py [--quick]        # --quick: B = 1 only, fewer repetitions"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import gan2shape_amd  # noqa
from gan2shape_amd import lib, parsing
import parsing_cases as pc

IMAGE_SIDE = 128
CASES = [("face", "bisenet"), ("car", "pspnet")]


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
    for category, name in CASES:
        net = parsing.BiSeNet(19) if name == "bisenet" else parsing.PSPNet(50, 21)
        net = pc.fill(net, pc.NETS[name]["weight_seed"]).cuda()
        fast = parsing.MaskingModel(category, net=net)
        native = parsing.MaskingModel(category, net=net, native=True)
        for B in (1,) if quick else (1, 8):
            images = torch.cat([pc.images(name, IMAGE_SIDE, s) for s in range((B + 1) // 2)])[:B].cuda()
            for method in ("image_mask", "confidence_mask"):
                f, g = getattr(fast, method), getattr(native, method)
                diff = float((f(images) - g(images)).abs().max())
                n = 5 if quick else 20
                t_f, t_g = events(lambda: f(images), 3, n), events(lambda: g(images), 3, n)
                w_f, w_g = wall(lambda: f(images), n), wall(lambda: g(images), n)
                print(f"{name} size {fast.size} B={B} {method:15s}: libg2s {t_f / B:8.3f} ms/image ({w_f / B:8.3f} wall) | "
                      f"native {t_g / B:8.3f} ms/image ({w_g / B:8.3f} wall) | native / libg2s {t_g / t_f:5.2f}x | "
                      f"max |difference| {diff:.1e}", flush=True)


if __name__ == "__main__":
    main()
