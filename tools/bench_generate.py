"""Sample-generator micro-benchmark (generate.py, csrc/mapping.hip).

  * g2s_mapping_fwd against the style_forward route (PixelNorm, then F.linear + fused_leaky_relu per layer, on the
    GPU) at N = 1, 8, 64, 512, 4096 rows, D = 512, L = 8;
  * mean_latent(4096) both ways (kernel: g2s_mapping_fwd with partial sums + g2s_rows_mean; torch:
    style_forward(z).mean(0)), the draw of z outside the timed region;
  * samples per second of generate.sample at G(128), n = 8, random weights, and g2s_image_to_u8 against the
    torch expression at [8, 3, 128, 128].

Times are medians of HIP-event pairs around one call; the two routes of a comparison are measured in alternating
rounds after a warm-up, so that a drift of the clocks meets both.  `crossover_rows`: the smallest measured N from
which the kernel is ahead at every larger measured N (null: nowhere) — generate.KERNEL_MIN_ROWS is set from it.

    python tools/bench_generate.py [--quick] [--out profiles/generate_g128.json]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import gan2shape_amd  # noqa
from gan2shape_amd import generate, lib
from gan2shape_amd import stylegan2 as sg2

ROWS = (1, 8, 64, 512, 4096)


def alternating(fns, warmup, rounds, per_round):
    """Median milliseconds of each fn: `rounds` rounds, in each of them every fn gets `per_round` event pairs."""
    for fn in fns:
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for _ in range(rounds):
        for i, fn in enumerate(fns):
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(per_round)]
            for e0, e1 in ev:
                e0.record()
                fn()
                e1.record()
            torch.cuda.synchronize()
            times[i] += [e0.elapsed_time(e1) for e0, e1 in ev]
    return [float(np.median(t)) for t in times]


def alternating_rounds(fns, warmup, rounds, per_round):
    """As `alternating`, but the median of each round per function: [[round medians] per function]."""
    for fn in fns:
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    out = [[] for _ in fns]
    for _ in range(rounds):
        for i, fn in enumerate(fns):
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(per_round)]
            for e0, e1 in ev:
                e0.record()
                fn()
                e1.record()
            torch.cuda.synchronize()
            out[i].append(float(np.median([e0.elapsed_time(e1) for e0, e1 in ev])))
    return out


def main():
    quick = "--quick" in sys.argv
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    rounds, per_round = (3, 10) if quick else (5, 40)
    lib.load()
    dev = torch.device("cuda")
    torch.manual_seed(0)
    G = sg2.Generator(128, 512, 8, channel_multiplier=1).to(dev).eval().requires_grad_(False)
    w, b = generate.mapping_weights(G)
    result = {"device": torch.cuda.get_device_name(0), "D": 512, "L": 8, "tile": generate.mapping_tile(),
              "mapping": [], "rounds": rounds, "per_round": per_round}
    with torch.no_grad():
        for N in ROWS:
            z = torch.randn(N, 512, device=dev)
            out = torch.empty_like(z)

            def kernel():
                return generate.mapping_fwd(z, w, b, True, out=out)

            def torch_route():
                return G.style_forward(z)
            diff = float((kernel() - torch_route()).abs().max())
            t_k, t_t = alternating([kernel, torch_route], 5, rounds, per_round)
            result["mapping"].append({"N": N, "kernel_us": t_k * 1e3, "torch_us": t_t * 1e3, "max_abs_diff": diff})
            print(f"mapping N={N:5d}: kernel {t_k * 1e3:8.1f} us | style_forward {t_t * 1e3:8.1f} us | "
                  f"torch / kernel {t_t / t_k:5.2f}x | max |difference| {diff:.1e}", flush=True)
        ahead = [m["kernel_us"] < m["torch_us"] for m in result["mapping"]]
        cross = None
        for i in range(len(ROWS) - 1, -1, -1):
            if not ahead[i]:
                break
            cross = ROWS[i]
        result["crossover_rows"] = cross
        print("kernel ahead from N =", cross, flush=True)

        z = torch.randn(4096, 512, device=dev)
        T = generate.mapping_tile()
        partial = torch.empty(4096 // T, 512, device=dev)
        out = torch.empty_like(z)

        def mean_kernel():
            generate.mapping_fwd(z, w, b, True, out=out, partial=partial)
            return generate.rows_mean(partial, 4096)

        def mean_torch():
            return G.style_forward(z).mean(0)
        diff = float((mean_kernel() - mean_torch()).abs().max())
        t_k, t_t = alternating([mean_kernel, mean_torch], 5, rounds, per_round)
        result["mean_latent_4096"] = {"kernel_us": t_k * 1e3, "torch_us": t_t * 1e3, "max_abs_diff": diff}
        print(f"mean_latent(4096): kernel {t_k * 1e3:8.1f} us | torch {t_t * 1e3:8.1f} us | max |difference| {diff:.1e}",
              flush=True)

        x = torch.randn(8, 3, 128, 128, device=dev)

        def quant_kernel():
            return generate.image_to_u8(x)

        def quant_torch():
            return generate._quantise_torch(x)
        assert torch.equal(quant_kernel(), quant_torch())
        t_k, t_t = alternating([quant_kernel, quant_torch], 5, rounds, per_round)
        result["image_to_u8_8x128"] = {"kernel_us": t_k * 1e3, "torch_us": t_t * 1e3}
        print(f"image_to_u8 [8,3,128,128]: kernel {t_k * 1e3:8.1f} us | torch {t_t * 1e3:8.1f} us", flush=True)

        center = generate.mean_latent(G, 4096)
        gen = torch.Generator(device=dev).manual_seed(0)

        def sample8():
            return generate.sample(G, 8, 0.7, center, gen)
        (t_s,) = alternating([sample8], 3, rounds, max(2, per_round // 4))
        result["sample_g128_n8"] = {"ms": t_s, "samples_per_s": 8 / (t_s * 1e-3)}
        print(f"sample G(128) n=8: {t_s:8.2f} ms = {8 / (t_s * 1e-3):8.1f} samples/s", flush=True)

        # one forward per sample against ONE forward for the n samples (sample(batched=True): per-sample noise maps on
        # the one-node path), alternating
        for n in (8, 32):
            def per_sample(n=n):
                return generate.sample(G, n, 0.7, center, gen)

            def batched(n=n):
                return generate.sample(G, n, 0.7, center, gen, batched=True)
            per_sample_rounds = alternating_rounds([per_sample, batched], 3, rounds, max(2, per_round // 4))
            for name, r in zip(("per_sample", "batched"), per_sample_rounds):
                result[f"sample_g128_n{n}_{name}"] = {"ms_median": float(np.median(r)), "ms_min_round": min(r),
                                                      "ms_max_round": max(r), "samples_per_s": n / (float(np.median(r)) * 1e-3)}
                print(f"sample G(128) n={n} {name}: {float(np.median(r)):8.2f} ms (rounds {min(r):.2f} .. {max(r):.2f})", flush=True)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
