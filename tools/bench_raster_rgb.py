"""Texture-pass micro-benchmark at the BASELINE size (B = 8, S = 128, ssaa 2, ts = 2, C = 3) through the
C ABI: g2s_raster_rgb_fwd and g2s_raster_rgb_bwd (texture gradient only, and both gradients) on the
scenes of tools/bench_raster.py.  Times are medians of per-call HIP-event times after a warm-up; the
bytes are the algorithmic ones (every input read once, every output written once, the clearing
memset of an accumulation target counted as one more write)."""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import gan2shape_amd  # noqa
from gan2shape_amd import lib
from raster_cases import scene

B, S, TS, CH = 8, 128, 2, 3
N, F = S * S, 2 * (S - 1) ** 2


def timed(fn, warmup=20, n=200):
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
    L = lib.load()
    st = lib.stream()
    samples = B * (2 * S) ** 2
    maps = samples * 16 + B * N * 12                     # face_idx + bary per sample, vertices
    tex_bytes = B * F * TS ** 3 * CH * 4
    img = B * CH * S * S * 4
    for name, seed, rot in (("hard", 1, 60.0), ("easy", 1, 5.0)):
        geo, verts, _ = scene(S, B=B, seed=seed, rot=rot)
        K = (C.c_float * 9)(*np.asarray(geo.K[0], np.float32).reshape(9).tolist())
        v = torch.tensor(verts, device="cuda").contiguous()
        wsb = L.g2s_raster_workspace_bytes(B, N, F, S)
        ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
        d = torch.empty(B, S, S, device="cuda")
        fi = torch.empty(B, 2 * S, 2 * S, dtype=torch.int32, device="cuda")
        ba = torch.empty(B, 2 * S, 2 * S, 3, device="cuda")
        lib.check(L.g2s_raster_depth_fwd(lib.ptr(v), None, B, N, F, S, K, float(S), 2, 1, 0.1, 10.0, lib.ptr(d),
                                         lib.ptr(fi), lib.ptr(ba), lib.ptr(ws), wsb, st))
        tex = torch.rand(B, F, TS, TS, TS, CH, device="cuda") * 2 - 1
        rgb = torch.empty(B, CH, S, S, device="cuda")
        g = torch.randn(B, CH, S, S, device="cuda")
        gt, gv = torch.empty_like(tex), torch.empty_like(v)
        bg = (C.c_float * CH)(1, 1, 1)

        def fwd():
            lib.check(L.g2s_raster_rgb_fwd(lib.ptr(v), None, lib.ptr(fi), lib.ptr(ba), lib.ptr(tex), B, N, F, S, 2, TS,
                                           CH, bg, 1e-3, lib.ptr(rgb), st))

        def bwd(want_v):
            lib.check(L.g2s_raster_rgb_bwd(lib.ptr(v), None, lib.ptr(fi), lib.ptr(ba), lib.ptr(tex), lib.ptr(g), B, N,
                                           F, S, K, float(S), 2, TS, CH, 1e-3, lib.ptr(gt),
                                           lib.ptr(gv) if want_v else None, None, 0, 0, st))

        t_f, t_t, t_b = timed(fwd), timed(lambda: bwd(False)), timed(lambda: bwd(True))
        cov = float((fi >= 0).float().mean())
        b_f = maps + tex_bytes + img
        b_t = maps + img + 2 * tex_bytes
        b_b = b_t + tex_bytes + 3 * B * N * 12
        print(f"B={B} S={S} ts={TS} C={CH} {name}: coverage {cov:.2f} | fwd {t_f:6.1f} us ({b_f / 1e6:.1f} MB) | "
              f"bwd textures {t_t:6.1f} us ({b_t / 1e6:.1f} MB) | bwd textures + vertices {t_b:6.1f} us "
              f"({b_b / 1e6:.1f} MB)", flush=True)


if __name__ == "__main__":
    main()
