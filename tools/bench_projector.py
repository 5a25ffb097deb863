"""ms per projector step at G(128), B = 1 (channel_multiplier 1, random weights, a random LPIPS trunk): the fused
path — the generator as one autograd node with noise-map gradients, g2s_noise_regularize / g2s_noise_normalize,
the one-launch Adam — against the op-by-op form: Generator.ONE_NODE = False plus the torch noise functions
(tests/projector_cases.py).  Both run the same step (projector.py's loop body, jitter included); they alternate in
rounds inside one process, each step timed by HIP events after a warm-up; medians and the spread over rounds are
printed, then the device launches of one step of each form, counted by the profiler in a run of its own.

    python tools/bench_projector.py [--size 128] [--steps 50] [--rounds 5] [--warmup 10] [--out profiles/FILE]

--batch 1 2 4 8 measures instead the step of projector.project_batch at each B (per-sample noise maps on the one-node
path) against the B = 1 step of projector.project, alternating in the same rounds, and counts each one's launches:

    python tools/bench_projector.py --batch 1 2 4 8 --out profiles/project_batch_g128.json"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import gan2shape_amd  # noqa
from gan2shape_amd import lib, projector
from gan2shape_amd import stylegan2 as sg2
from gan2shape_amd.lpips import PerceptualLoss
import projector_cases as pc


class Stepper:
    """One projector state (latent, maps, Adam) and its step in the fused or the op-by-op form."""

    def __init__(self, G, percept, target, stats, fused, seed):
        self.G, self.percept, self.target, self.fused = G, percept, target, fused
        self.std = float(stats[1])
        self.gen = torch.Generator(device="cuda").manual_seed(seed)
        self.noises = [n.normal_(generator=self.gen).requires_grad_(True) for n in G.make_noise()]
        self.latent = stats[0].detach().clone().unsqueeze(0).requires_grad_(True)
        self.opt = projector._adam([self.latent] + self.noises, 0.1)
        self.i = 0

    def step(self, total=1000):
        t = (self.i % total) / total
        self.i += 1
        sg2.Generator.ONE_NODE = self.fused
        self.opt.param_groups[0]["lr"] = projector.get_lr(t, 0.1)
        strength = self.std * 0.05 * max(0, 1 - t / 0.75) ** 2
        img = projector._generate(self.G, projector.latent_noise(self.latent, strength, self.gen), self.noises)
        reg = projector.noise_regularize(self.noises) if self.fused else pc.noise_regularize(self.noises)
        loss = self.percept(img, self.target).sum() + 1e5 * reg
        self.opt.zero_grad()
        loss.backward()
        self.opt.step()
        (projector.noise_normalize_ if self.fused else pc.noise_normalize_)(self.noises)
        sg2.Generator.ONE_NODE = True


class BatchStepper:
    """project_batch's state and step for B images (projector.py's loop body under synthesis.per_sample_noise)."""

    def __init__(self, G, percept, target, stats, B, seed):
        from gan2shape_amd import synthesis
        self.switch = synthesis.per_sample_noise
        self.G, self.percept, self.target = G, percept, target.repeat(B, 1, 1, 1).contiguous()
        self.std = float(stats[1])
        self.gen = torch.Generator(device="cuda").manual_seed(seed)
        self.noises = [n.new_empty((B,) + tuple(n.shape[1:])).normal_(generator=self.gen).requires_grad_(True)
                       for n in G.make_noise()]
        self.latent = stats[0].detach().clone().unsqueeze(0).repeat(B, 1).contiguous().requires_grad_(True)
        self.opt = projector._adam([self.latent] + self.noises, 0.1)
        self.i = 0

    def step(self, total=1000):
        t = (self.i % total) / total
        self.i += 1
        self.opt.param_groups[0]["lr"] = projector.get_lr(t, 0.1)
        strength = self.std * 0.05 * max(0, 1 - t / 0.75) ** 2
        with self.switch():
            img = projector._generate(self.G, projector.latent_noise(self.latent, strength, self.gen), self.noises)
        loss = self.percept(img, self.target).sum() + 1e5 * projector.noise_regularize(self.noises)
        self.opt.zero_grad()
        loss.backward()
        self.opt.step()
        projector.noise_normalize_(self.noises)


def timed(stepper, n):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
    for e0, e1 in ev:
        e0.record()
        stepper.step()
        e1.record()
    torch.cuda.synchronize()
    return [e0.elapsed_time(e1) for e0, e1 in ev]


def launches(stepper):
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        stepper.step()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if str(e.device_type).endswith("CUDA"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", type=str, default=None)
    ap.add_argument("--batch", type=int, nargs="+", default=None,
                    help="measure project_batch's step at these batch sizes against project's B = 1 step")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_projector needs a GPU"
    lib.load()
    torch.manual_seed(0)
    G = pc.fixture_generator(sg2, size=args.size, style_dim=512, n_mlp=8, seed=77).cuda()
    percept = PerceptualLoss().cuda()
    stats = projector.mean_latent_stats(G, n=2000)
    with torch.no_grad():
        target, _ = G([stats[0][None] + 0.5 * torch.randn(1, 512, device="cuda")], input_is_w=True)
        if args.size > 256:
            f = args.size // 256
            target = target.reshape(1, 3, 256, f, 256, f).mean([3, 5])
    if args.batch:
        forms = {"project_b1": Stepper(G, percept, target, stats, True, 1)}
        forms.update({f"project_batch_b{B}": BatchStepper(G, percept, target, stats, B, 1) for B in args.batch})
        what = (f"projector step, G({args.size}): project (B = 1) and project_batch at B = {args.batch}, ms per step (HIP "
                f"events; median of {args.steps} steps per round, {args.rounds} alternating rounds, {args.warmup} warm-up "
                "steps); ms_per_image = ms_median / B")
    else:
        forms, what = None, None
    forms = forms or {"fused": Stepper(G, percept, target, stats, True, 1), "op_by_op": Stepper(G, percept, target, stats, False, 1)}
    for s in forms.values():
        for _ in range(args.warmup):
            s.step()
    torch.cuda.synchronize()
    per_round = {k: [] for k in forms}
    for _ in range(args.rounds):                      # alternate the two forms: drift and neighbours hit both alike
        for k, s in forms.items():
            per_round[k].append(float(np.median(timed(s, args.steps))))
    result = {"what": what or f"projector step, G({args.size}), B = 1, ms per step (HIP events; median of {args.steps} steps per "
                      f"round, {args.rounds} alternating rounds, {args.warmup} warm-up steps)"}
    for k, v in per_round.items():
        result[k] = {"ms_median": float(np.median(v)), "ms_min_round": min(v), "ms_max_round": max(v)}
        if args.batch:
            B = 1 if k == "project_b1" else int(k.rsplit("b", 1)[1])
            result[k].update({"B": B, "ms_per_image": float(np.median(v)) / B, "ms_per_image_min_round": min(v) / B,
                              "ms_per_image_max_round": max(v) / B})
    for k, s in forms.items():
        try:
            result[k]["device_launches_per_step"] = launches(s)
        except Exception as e:                        # the count is an extra: say so instead of guessing
            result[k]["device_launches_per_step"] = f"not counted ({type(e).__name__})"
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
