"""The data path of train / dtrain -> profiles/dataprep.json.

    python tools/bench_dataprep.py [--rounds 5] [--out profiles/dataprep.json] [--skip-train]

On a synthetic PNG folder that the tool writes (seeded), alternating rounds, medians with per-round ranges:

routes   host wall time per batch (a device synchronise ends every batch) of dtrain.real_batches followed by
         .to(device) — PIL decode, host resize, stack, copy — against dataset.DeviceBatches on the packed folder, at
         [16, 3, 128, 128] and [32, 3, 256, 256], once with sources at the target size and once with 512 x 512
         sources; for DeviceBatches also the device time of a batch (HIP events).
kernel   g2s_u8_batch alone against a device-to-device copy that moves the same bytes (5 * 3 * S^2 * B read plus
         written; `d2d_copy`) and against a copy OF that many bytes (twice the traffic; `d2d_copy_of_all_bytes`), HIP
         events around 200 back-to-back launches, and the ratio to the former.
resize   g2s_resize_u8 (prepare_data.resize_and_crop on the device, tables included) at N = 16, 512^2 -> 128^2 and
         1024^2 -> 256^2 against PIL.Image.resize + crop of the same images on the host.
train    one train.iteration at G(128), channel multiplier 1, B = 16, wall clock, fed by either route."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gan2shape_amd  # noqa: E402,F401
from gan2shape_amd import dataset, dtrain, lib, prepare_data, train  # noqa: E402

DEV = "cuda"


def synthetic_image(rng, size):
    """Smooth colour fields plus a little noise: compresses (and decodes) like a photograph rather than like noise."""
    low = rng.integers(0, 256, (size // 16 + 1, size // 16 + 1, 3), dtype=np.uint8)
    a = np.asarray(Image.fromarray(low).resize((size, size), Image.BICUBIC), dtype=np.int16)
    a = a + rng.integers(-6, 7, a.shape, dtype=np.int16)
    return np.clip(a, 0, 255).astype(np.uint8)


def write_folder(root, n, size, seed):
    if os.path.exists(os.path.join(root, "list.txt")):
        return root
    rng = np.random.default_rng(seed)
    os.makedirs(root, exist_ok=True)
    names = [f"{i:04d}.png" for i in range(n)]
    for name in names:
        Image.fromarray(synthetic_image(rng, size)).save(os.path.join(root, name), compress_level=1)
    with open(os.path.join(root, "list.txt"), "w") as f:
        f.writelines(name + "\n" for name in names)
    return root


def summary(samples):
    return {"median_ms": statistics.median(samples), "round_min_ms": min(samples), "round_max_ms": max(samples)}


def wall_ms(fn, reps):
    """Median host wall time of fn(), each call ended by a device synchronise."""
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out)


def event_ms(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / inner


def alternate(routes, rounds, measure):
    for fn in routes.values():      # warm-up
        fn()
        fn()
    torch.cuda.synchronize()
    times = {name: [] for name in routes}
    for _ in range(rounds):
        for name, fn in routes.items():
            times[name].append(measure(fn))
    return {name: summary(t) for name, t in times.items()}


def bench_routes(work, rounds):
    rows = []
    for B, S in ((16, 128), (32, 256)):
        for src in sorted({S, 512}):
            folder = write_folder(os.path.join(work, f"png_{src}"), 64, src, seed=src)
            packed = os.path.join(work, f"packed_{src}")
            if not dataset.is_packed(packed, S):
                prepare_data.prepare(folder, packed, sizes=(S,), device=DEV)
            old = dtrain.real_batches(folder, S, B, torch.Generator().manual_seed(0))
            new = dataset.DeviceBatches(packed, S, B, torch.Generator().manual_seed(0), DEV)
            staged = dataset.DeviceBatches(packed, S, B, torch.Generator().manual_seed(0), DEV, max_resident_bytes=0)
            routes = {"real_batches_to_device": lambda: next(old).to(DEV), "device_batches": lambda: next(new),
                      "device_batches_staged": lambda: next(staged)}
            row = {"batch": [B, 3, S, S], "source": [src, src], "images": 64,
                   "host_wall": alternate(routes, rounds, lambda fn: wall_ms(fn, 3))}
            row["device_batches_device_time"] = alternate({"device_batches": routes["device_batches"]}, rounds,
                                                          lambda fn: event_ms(fn, 20))["device_batches"]
            w = row["host_wall"]
            row["old_over_new_wall"] = w["real_batches_to_device"]["median_ms"] / w["device_batches"]["median_ms"]
            print(json.dumps(row), flush=True)
            rows.append(row)
    return rows


def bench_kernel(rounds):
    rows = []
    L = lib.load()
    for B, S in ((16, 128), (32, 256)):
        N = 4096 if S == 128 else 1024
        data = torch.randint(0, 256, (N, 3, S, S), dtype=torch.uint8, device=DEV)
        idx = torch.randperm(N, device=DEV)[:B]
        flip = (torch.rand(B, device=DEV) < 0.5).to(torch.uint8)
        out = torch.empty((B, 3, S, S), device=DEV)
        nbytes = 5 * 3 * S * S * B
        a = torch.empty(nbytes // 2, dtype=torch.uint8, device=DEV)      # a copy reads and writes: half the bytes each way
        b = torch.empty_like(a)
        a2 = torch.empty(nbytes, dtype=torch.uint8, device=DEV)          # and a copy OF that many bytes: twice the traffic
        b2 = torch.empty_like(a2)

        def kernel():
            lib.check(L.g2s_u8_batch(lib.ptr(data), N, lib.ptr(idx), lib.ptr(flip), lib.ptr(out), B, S, lib.stream()))
        res = alternate({"g2s_u8_batch": kernel, "d2d_copy": lambda: b.copy_(a), "d2d_copy_of_all_bytes": lambda: b2.copy_(a2)},
                        rounds, lambda fn: event_ms(fn, 200))
        row = {"batch": [B, 3, S, S], "bytes": nbytes, "inner_launches": 200, **res}
        row["kernel_over_copy"] = res["g2s_u8_batch"]["median_ms"] / res["d2d_copy"]["median_ms"]
        row["kernel_gb_per_s"] = nbytes / res["g2s_u8_batch"]["median_ms"] / 1e6
        print(json.dumps(row), flush=True)
        rows.append(row)
    return rows


def bench_resize(rounds):
    rows = []
    for src, S in ((512, 128), (1024, 256)):
        rng = np.random.default_rng(src)
        images = np.stack([synthetic_image(rng, src) for _ in range(16)])
        dev = torch.from_numpy(images).to(DEV)

        def pillow():
            for a in images:
                Image.fromarray(a).resize((S, S), Image.LANCZOS)

        def kernel():
            prepare_data.resize_and_crop(dev, S)
        ref = np.stack([np.asarray(Image.fromarray(a).resize((S, S), Image.LANCZOS)) for a in images])
        same = bool(np.array_equal(prepare_data.resize_and_crop(dev, S).cpu().numpy(), ref.transpose(0, 3, 1, 2)))
        res = alternate({"g2s_resize_u8": kernel, "pillow_host": pillow}, rounds, lambda fn: wall_ms(fn, 3))
        row = {"images": 16, "source": [src, src], "size": S, "equal_to_pillow": same, **res,
               "device_time": alternate({"k": kernel}, rounds, lambda fn: event_ms(fn, 10))["k"]}
        row["pillow_over_kernel_wall"] = res["pillow_host"]["median_ms"] / res["g2s_resize_u8"]["median_ms"]
        print(json.dumps(row), flush=True)
        rows.append(row)
    return rows


def bench_train(work, rounds):
    S, B = 128, 16
    rows = []
    args = train.build_parser().parse_args(["--size", str(S), "--channel-multiplier", "1", "--data", "x", "--batch",
                                            str(B), "--out", "x"])
    torch.manual_seed(0)
    dt, gt = train.build_trainers(args, torch.device(DEV))
    for src in (S, 512):
        folder = write_folder(os.path.join(work, f"png_{src}"), 64, src, seed=src)
        packed = os.path.join(work, f"packed_{src}")
        if not dataset.is_packed(packed, S):
            prepare_data.prepare(folder, packed, sizes=(S,), device=DEV)
        old = dtrain.real_batches(folder, S, B, torch.Generator().manual_seed(0))
        new = dataset.DeviceBatches(packed, S, B, torch.Generator().manual_seed(0), DEV)
        step = [0]

        def iterate(batches):
            train.iteration(dt, gt, next(batches).to(DEV), step[0])
            step[0] += 1

        def window(batches):        # 16 iterations: one d_reg_every period, four g_reg_every periods
            def run():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(16):
                    iterate(batches)
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) * 1e3 / 16
            return run
        routes = {"real_batches_to_device": window(old), "device_batches": window(new)}
        for fn in routes.values():
            fn()
        times = {name: [] for name in routes}
        for _ in range(rounds):
            for name, fn in routes.items():
                times[name].append(fn())
        row = {"size": S, "batch": B, "source": [src, src], "iterations_per_sample": 16,
               **{name: summary(t) for name, t in times.items()}}
        row["old_over_new"] = row["real_batches_to_device"]["median_ms"] / row["device_batches"]["median_ms"]
        print(json.dumps(row), flush=True)
        rows.append(row)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--skip-train", action="store_true")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(__file__), "..", "profiles", "dataprep.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_dataprep.py measures on the GPU: no device visible")
    result = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds}
    with tempfile.TemporaryDirectory() as work:
        result["kernel"] = bench_kernel(args.rounds)
        result["resize"] = bench_resize(args.rounds)
        result["routes"] = bench_routes(work, args.rounds)
        if not args.skip_train:
            result["train_iteration"] = bench_train(work, args.rounds)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
