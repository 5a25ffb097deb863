"""Twice-differentiable ADA augmentation benchmark, three measurements on one commit:

1. the adjoint alone, g2s_ada_warp_down_bwd (float-atomic scatter, with its clear) against
   g2s_ada_warp_down_bwd_gather (two launches, fixed order), each followed by g2s_ada_up2_bwd, at [8, 3, 128, 128]
   and [32, 3, 256, 256] for matrices sampled with p = 0.8;
2. `augment` forward + backward (create_graph) + second backward at the same shapes: `order=2` (the node pair of
   csrc/ada.hip) against `dtrain.augment_differentiable(composed=True)` (the torch composition);
3. the R1 step of DiscriminatorTrainer with augmentation at D(128), channel multiplier 1, B = 16, as
   tools/bench_dtrain.py measures it, on the node pair against the composition (the route before the pair existed).

Per route: HIP-event pairs around one Python call after a warm-up, the routes in ALTERNATING rounds so that clock and
cache state are shared; reported is the median over all samples and the lowest and highest per-round median, and the
launches of one call (torch profiler).  The rounds are sized by one call of the composition; where that call takes more
than five seconds it stays the composition's only sample.  Writes profiles/augment_twice.json after every stage.

    python tools/bench_augment_twice.py [--quick] [--out profiles/augment_twice.json]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

import gan2shape_amd  # noqa
from gan2shape_amd import augment as aug
from gan2shape_amd import dtrain, lib
from gan2shape_amd.op import conv2d_gradfix
from gan2shape_amd.stylegan2 import Discriminator

from bench_manipulate import alternating
from bench_sweep import launches


def adjoints(G, C, gy):
    """(scatter, gather): gy -> gx through the C entries, on preallocated buffers."""
    B, ch, H, W = gy.shape
    g_host = G.float().cpu()
    x0, x1, y0, y1 = pads = aug._pads(g_host, H, W, 12)
    warp = aug._warp_matrix(g_host, pads, H, W).to(gy.device)
    cmat = C.float()[:, :3, :].contiguous().to(gy.device)
    H2, W2 = 2 * (H + y0 + y1), 2 * (W + x0 + x1)
    L = lib.load()
    gx2 = torch.empty((B, ch, H2, W2), device=gy.device)
    ga = torch.empty((B, ch, 2 * (H + 6), 2 * (W + 6)), device=gy.device)
    gx = torch.empty_like(gy)

    def up():
        lib.check(L.g2s_ada_up2_bwd(lib.ptr(gx2), lib.ptr(gx), B, ch, H, W, x0, x1, y0, y1, lib.stream()))
        return gx

    def scatter():
        lib.check(L.g2s_ada_warp_down_bwd(lib.ptr(gy), lib.ptr(warp), lib.ptr(cmat), lib.ptr(gx2), B, ch, H, W, H2, W2,
                                          0, lib.stream()))
        return up()

    def gather():
        lib.check(L.g2s_ada_warp_down_bwd_gather(lib.ptr(gy), lib.ptr(warp), lib.ptr(cmat), lib.ptr(gx2), lib.ptr(ga),
                                                 B, ch, H, W, H2, W2, lib.stream()))
        return up()
    return scatter, gather


def three_passes(route, img, r):
    """forward, backward with create_graph, second backward: the quantity of tests/ada_twice_cases.py."""
    x = img.detach().requires_grad_(True)
    y = route(x)
    g, = torch.autograd.grad((y.pow(2) * r).sum(), x, create_graph=True)
    g.pow(2).sum().backward()
    return x.grad


def r1_step(trainer, composed):
    def step(real):
        with conv2d_gradfix.use():
            real = real.detach().requires_grad_(True)
            torch.manual_seed(1)                      # the same matrices on both routes and in every call
            real_aug, _ = dtrain.augment_differentiable(real, 0.8, composed=composed)
            pred = trainer.d(real_aug)[0]
            loss = dtrain.d_r1_loss(pred, real)
            trainer.d.zero_grad()
            (trainer.r1 / 2 * loss * trainer.d_reg_every + 0 * pred[0]).backward()
            trainer.d_optim.step()
    return step


def once(fn):
    """Milliseconds of one call after one warm-up call, and its result."""
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def budget(ms, rounds, n, limit_ms=4000.0):
    """(rounds, samples per round, warm-up calls) such that one round of a route that takes `ms` stays near limit_ms:
    the composition takes hundreds of milliseconds per call where the kernels take a fraction of one."""
    fit = max(2, min(n, int(limit_ms / max(ms, 1e-3))))
    return (rounds if fit >= 5 else 3), fit, (3 if fit >= 5 else 1)


def compare(routes, slow, rounds, n, ratio):
    """Alternating rounds of the two routes, sized by one call of routes[slow].  Where that one call takes longer than
    five seconds it is the only sample of the slow route (no rounds, no launch count) and the other runs alone."""
    ms, out_slow = once(routes[slow])
    fast = next(k for k in routes if k != slow)
    diff = rel(routes[fast](), out_slow)
    del out_slow
    if ms > 5000.0:
        t = alternating({fast: routes[fast]}, rounds, n)
        t[slow] = dict(median_ms=ms, samples=1)
        t[fast]["launches"] = launches(routes[fast])
        rs, ns = rounds, n
    else:
        rs, ns, warm = budget(ms, rounds, n)
        t = alternating(routes, rs, ns, warmup=warm)
        for k in t:
            t[k]["launches"] = launches(routes[k])
    return dict(t, rounds=rs, samples_per_round=ns, rel_diff=diff, **{ratio: t[slow]["median_ms"] / t[fast]["median_ms"]})


def save(result, path):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


def rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


def main():
    quick = "--quick" in sys.argv
    path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(
        ROOT, "profiles", "augment_twice.json")
    lib.load()
    dev = torch.device("cuda")
    rounds, n = (3, 5) if quick else (5, 20)
    shapes = ((8, 3, 128, 128), (32, 3, 256, 256))
    result = dict(device=torch.cuda.get_device_name(0), rounds=rounds, samples_per_round=n, p=0.8, adjoint=[], second=[])

    def inputs(shape):
        B, _, H, W = shape
        torch.manual_seed(B)
        G = torch.inverse(aug.sample_affine(0.8, B, H, W))
        C = aug.sample_color(0.8, B)
        return G, C, torch.randn(shape, device=dev), torch.randn(shape, device=dev), torch.rand(shape, device=dev) + 0.5

    # 1. the adjoint alone
    for shape in shapes:
        G, C, img, gy, r = inputs(shape)
        scatter, gather = adjoints(G, C, gy)
        row = dict(shape=list(shape), pads=list(aug._pads(G, shape[2], shape[3], 12)),
                   rel_diff=rel(scatter().clone(), gather()))
        t = alternating(dict(scatter=scatter, gather=gather), rounds, n)
        row.update({k: dict(v, launches=launches(f)) for (k, v), f in zip(t.items(), (scatter, gather))},
                   scatter_over_gather=t["scatter"]["median_ms"] / t["gather"]["median_ms"])
        result["adjoint"].append(row)
        print(json.dumps(row), flush=True)
        save(result, path)

    # 3. the R1 step with augmentation
    B, size = 16, 128
    torch.manual_seed(B)
    d_new, d_old = Discriminator(size, 1).to(dev), Discriminator(size, 1).to(dev)
    d_old.load_state_dict(d_new.state_dict())
    real = torch.rand(B, 3, size, size, device=dev) * 2 - 1
    steps = dict(order2=r1_step(dtrain.DiscriminatorTrainer(d_new, augment=True, augment_p=0.8), False),
                 composed=r1_step(dtrain.DiscriminatorTrainer(d_old, augment=True, augment_p=0.8), True))
    routes = {k: (lambda f=f: f(real) or torch.ones(1)) for k, f in steps.items()}
    result["r1_step"] = dict(compare(routes, "composed", *((2, 3) if quick else (4, 8)), "composed_over_order2"),
                             size=size, B=B)
    del result["r1_step"]["rel_diff"]           # the steps return nothing to compare
    print(json.dumps(result["r1_step"]), flush=True)
    save(result, path)
    del d_new, d_old, steps, routes, real
    torch.cuda.empty_cache()

    # 2. forward + backward + second backward
    for shape in shapes:
        G, C, img, gy, r = inputs(shape)
        routes = dict(order2=lambda: three_passes(lambda x: aug.augment(x, 0.8, (G, C), order=2)[0], img, r),
                      composed=lambda: three_passes(
                          lambda x: dtrain.augment_differentiable(x, 0.8, (G, C), composed=True)[0], img, r))
        row = dict(compare(routes, "composed", rounds, n, "composed_over_order2"), shape=list(shape))
        result["second"].append(row)
        print(json.dumps(row), flush=True)
        save(result, path)


if __name__ == "__main__":
    main()
