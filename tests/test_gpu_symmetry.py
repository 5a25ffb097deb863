"""Symmetry flips on the GPU, whole steps: the flipped step 1 (flip1), the inner step-1 pass of step 3 (flip3,
step1=False) and step 3 (flip3) against the float64 golden tests/golden/symmetry.npz — the reference model's own
parts composed as the flipped steps (tests/golden/make_symmetry_golden.py) — through both routes of the package:
the g2s_mirror_pair kernel (renderer.fused = True) and the torch composition cat / flip (renderer.fused = False).

MEASURED on the MI355X: the worst ratio |value - float64 golden| / max(e32, one float32 rounding of the quantity)
over every stored quantity (e32: the distance of the reference's own float32 run from its float64 run) is

    pass    fused route                 composed route
    f1s1    3.53 (normal.proj)          2.14 (normal.proj)
    f3s1    4.67 (normal.proj)          4.13 (normal.proj)
    f3s3    2.97 (normal.proj)          3.08 (normal.proj)

so MULTIPLE = 8, the smallest of 2, 4, 8, 16 that holds, and the same for both routes."""
import math

import numpy as np
import pytest
import torch

import model_cases as mc
import symmetry_cases as sc

pytestmark = pytest.mark.gpu

MULTIPLE = 8
EPS32 = float(np.finfo(np.float32).eps)


def _zero_grads(m):
    for p in m.parameters():
        p.grad = None


@pytest.fixture(scope="module")
def case(golden):
    """The model of tests/test_gpu_golden.py's step tests (same seeded weights, the stand-in perceptual loss) with
    the smooth depth net of the symmetry golden."""
    from test_gpu_golden import build_step_model
    steps, g = golden("steps"), golden("symmetry")
    m = build_step_model(steps)
    mc.smooth_depth_net(m.depth_net)
    assert m.lam_flip == float(g["lam_flip"])
    image = torch.tensor(g["image"]).cuda()
    latent = torch.tensor(steps["latent"]).cuda()
    c2 = (torch.tensor(steps["s2.projected"]).cuda(), torch.tensor(steps["s2.mask"]).cuda())
    return m, g, image, latent, c2


def _ratios(got, g):
    out = {}
    for key, v in got.items():
        ref = g[key]
        assert v.shape == ref.shape, (key, v.shape, ref.shape)
        floor = max(float(g[f"e32_{key}"]), sc.rounding(ref))
        out[key] = sc.distance(v, ref) / floor if floor > 0 else (0.0 if sc.distance(v, ref) == 0 else math.inf)
    return out


@pytest.mark.parametrize("name", list(sc.PASSES))
def test_flipped_steps_vs_float64_golden(case, name):
    """Every stored quantity within MULTIPLE x max(e32, one float32 rounding of it) of the float64 golden, through
    the fused route; the torch-composed route of the package on the same case is the yardstick (printed)."""
    m, g, image, latent, c2 = case
    worst = {}
    try:
        for route, fused in (("fused", True), ("composed", False)):
            m.renderer.fused = fused
            r = _ratios(sc.run_pass(m, name, image, latent, c2, mc.grad_evidence, _zero_grads), g)
            top = sorted(r.items(), key=lambda kv: -kv[1])[:4]
            print(f"[symmetry {name}] {route:8s} route: worst ratios " + ", ".join(f"{k} {v:.2f}" for k, v in top))
            worst[route] = r
    finally:
        m.renderer.fused = True
    for route in ("fused", "composed"):
        bad = {k: round(v, 2) for k, v in worst[route].items() if not v <= MULTIPLE}
        assert not bad, (name, route, bad)


def test_fused_and_composed_routes_agree_on_collected(case):
    """With flips on, the two routes hand step 2 the same `collected`, bit for bit, wherever they already do with
    flips off (the mirror kernel is a copy; the rows it feeds go through the same kernels)."""
    from gan2shape_amd import lib
    m, g, image, latent, c2 = case
    got = {}
    prev = lib.set_deterministic(True)      # the nets' forwards repeat bit for bit from call to call
    try:
        for flip in (False, True):
            for fused in (True, False):
                m.renderer.fused, m.flip1 = fused, flip
                with torch.no_grad():
                    _, got[flip, fused] = m.forward_step1(image, latent, None)
    finally:
        m.renderer.fused, m.flip1 = True, False
        lib.set_deterministic(prev)
    same_off = [torch.equal(a, b) for a, b in zip(got[False, True][:5], got[False, False][:5])]
    same_on = [torch.equal(a, b) for a, b in zip(got[True, True][:5], got[True, False][:5])]
    print("[symmetry] collected (normal, light_a, light_b, albedo, depth) bit-equal between the routes: flips off",
          same_off, "flips on", same_on)
    assert all(on or not off for on, off in zip(same_on, same_off))
    # and the B plain rows of a flipped step are those of the plain step, route by route
    for fused in (True, False):
        for a, b in zip(got[True, fused][:5], got[False, fused][:5]):
            assert torch.equal(a, b)


def test_graphed_fit_with_a_flip_schedule_reproduces_eager():
    """Trainer.fit(graphs=True) over stages whose flips differ: the graphs are keyed by (kind, flip), each variant
    is captured once, and the history reproduces the eager run's (the agreement test_trainer_fit_with_hip_graphs
    asks of the deterministic step-1 loss, here of both stages')."""
    import bench
    from gan2shape_amd.model import GAN2Shape
    from gan2shape_amd.trainer import Trainer
    dev = torch.device("cuda")
    torch.cuda.set_stream(torch.cuda.Stream(dev))     # captures need a non-default stream
    try:
        cfg = bench.face_config(n_proj=2)
        cfg.update(flip1_cfg=[True, False], flip3_cfg=[True, False])
        stages = [{'step1': 4, 'step2': 4, 'step3': 4}] * 2
        losses, keys = {}, None
        for graphs in (False, True):
            torch.manual_seed(0)
            t = Trainer(GAN2Shape, cfg, device=dev, capturable=True)
            image, latent = bench.synthetic_sample(t.model, 1234, dev)
            seen = []
            if graphs:
                from gan2shape_amd import graphs as gmod
                record = gmod.GraphedSteps._record

                def spy(self, kind, src, record=record, seen=seen):
                    seen.append(self.key(kind))
                    return record(self, kind, src)
                gmod.GraphedSteps._record = spy
            try:
                n = t.fit([(image[0].cpu(), latent[0].cpu(), 0)], stages=stages, graphs=graphs)
            finally:
                if graphs:
                    gmod.GraphedSteps._record = record
            assert n == 24
            losses[graphs] = [h[3] for h in t.history]
            assert all(math.isfinite(v) for v in losses[graphs])
            keys = seen
        # a [True, False] schedule captures steps 1 and 3 twice, step 2 once
        assert keys == [(1, True), (2, False), (3, True), (1, False), (3, False)], keys
        # step 1 is deterministic given the weights: both stages' step-1 losses agree (stage 1 follows 12 iterations)
        assert abs(losses[True][0] - losses[False][0]) < 5e-3 * abs(losses[False][0]), (losses[True], losses[False])
        assert abs(losses[True][3] - losses[False][3]) < 5e-3 * abs(losses[False][3]), (losses[True], losses[False])
    finally:
        torch.cuda.set_stream(torch.cuda.default_stream(dev))


def test_flipped_step1_gradient_is_the_directional_derivative(case):
    """Central differences of the flipped step-1 loss against <g, d> along a fixed probe direction of the albedo net
    (model_cases.probe_direction, unit norm) and along g / |g| — the method and half-widths of
    tests/test_gpu_round4.py's whole-step test: the median quotient of the half-widths 2e-5, 5e-5, 1e-4, held to
    2 % + 6e-3."""
    from gan2shape_amd import lib
    m, g, image, latent, c2 = case
    ps = [p for _, p in sorted(m.albedo_net.named_parameters(), key=lambda kv: kv[0])]

    def flat(ts):
        return torch.cat([t.reshape(-1) for t in ts])

    def put(vec):
        off = 0
        with torch.no_grad():
            for p in ps:
                p.copy_(vec[off:off + p.numel()].view_as(p))
                off += p.numel()

    def evaluate(grad):
        _zero_grads(m)
        with torch.enable_grad() if grad else torch.no_grad():
            loss, _ = m.forward_step1(image, latent, None)
            if not grad:
                return float(loss)
            loss.backward()
        gr = flat([p.grad for p in ps]).double()
        _zero_grads(m)
        return float(loss.detach()), gr
    theta0 = flat([p.detach() for p in ps]).clone()
    prev = lib.set_deterministic(True)
    m.flip1 = True
    try:
        loss0, grad = evaluate(True)
        probe = torch.tensor(mc.probe_direction(theta0.numel(), 0), device="cuda")
        dirs = {"probe 0": probe / probe.norm(), "g / |g|": grad / grad.norm()}
        for name, d in dirs.items():
            want = float(grad @ d)
            quotients = []
            for half in (2e-5, 5e-5, 1e-4):
                put((theta0.double() + half * d).float())
                lp_ = evaluate(False)
                put((theta0.double() - half * d).float())
                lm_ = evaluate(False)
                quotients.append((lp_ - lm_) / (2 * half))
            got = float(np.median(quotients))
            print(f"[symmetry step 1, flipped] loss {loss0:.6f} {name:8s} <g, d> = {want:.5e}   central differences "
                  + " ".join(f"{q:.5e}" for q in quotients))
            assert abs(got - want) <= 2e-2 * abs(want) + 6e-3, (name, want, quotients)
    finally:
        put(theta0)
        m.flip1 = False
        lib.set_deterministic(prev)
