"""The twice-differentiable ADA augmentation and the fixed-order warp adjoint on the GPU: g2s_ada_warp_down_bwd_gather
against the reference's float64 gradients on the eleven cases of ada.npz and ada_twice.npz, the adjoint identity, run to
run identity, `augment(..., order=2)` in deterministic mode, its second derivative, the linearity of the node pair, the
route `dtrain.augment_differentiable` takes, and the two trainers with augmentation in deterministic mode.
Bounds: ada_cases.py (first order), ada_twice_cases.py (second order)."""
import copy
import random

import pytest
import torch

import ada_cases as ac
import ada_twice_cases as tc

pytestmark = pytest.mark.gpu

EPS32 = 2.0 ** -23


@pytest.fixture(scope="module")
def aug():
    import gan2shape_amd  # noqa: F401
    from gan2shape_amd import augment, lib
    lib.load()
    return augment


@pytest.fixture
def deterministic():
    from gan2shape_amd import lib
    prev = lib.set_deterministic(True)
    yield lib
    lib.set_deterministic(prev)


def gather_adjoint(aug, c, gy, keep_gx2=False):
    """L^T gy through the two C entries themselves: g2s_ada_warp_down_bwd_gather into a NaN-filled gx2 (the entry
    promises to write every element), then g2s_ada_up2_bwd."""
    from gan2shape_amd import lib
    L = lib.load()
    warp, pads, cmat = tc.host_matrices(aug, c)
    B, C, H, W = gy.shape
    x0, x1, y0, y1 = pads
    H2, W2 = 2 * (H + y0 + y1), 2 * (W + x0 + x1)
    warp = warp.cuda()
    cmat = None if cmat is None else cmat.cuda()
    gy = gy.contiguous()
    gx2 = torch.full((B, C, H2, W2), float("nan"), device="cuda")
    ga = torch.full((B, C, 2 * (H + 6), 2 * (W + 6)), float("nan"), device="cuda")
    lib.check(L.g2s_ada_warp_down_bwd_gather(lib.ptr(gy), lib.ptr(warp), lib.ptr(cmat), lib.ptr(gx2), lib.ptr(ga),
                                             B, C, H, W, H2, W2, lib.stream()))
    if keep_gx2:
        return gx2
    gx = torch.empty_like(gy)
    lib.check(L.g2s_ada_up2_bwd(lib.ptr(gx2), lib.ptr(gx), B, C, H, W, x0, x1, y0, y1, lib.stream()))
    return gx


@pytest.mark.parametrize("name", tc.names())
def test_gather_matches_the_float64_golden(aug, name):
    c = tc.case(name)
    gx = gather_adjoint(aug, c, c["gy"].cuda())
    assert bool(torch.isfinite(gx).all())
    eg = float((gx.cpu().double() - c["gx"]).abs().max())
    print(name, "gather error / e32_gx", eg / c["e32_gx"])
    assert eg <= ac.E32_MULTIPLE * c["e32_gx"], (eg, c["e32_gx"])


@pytest.mark.parametrize("name", ["rot30", "pad_clamp", "batch3"] + tc.NEW)
def test_gather_is_the_adjoint_of_the_forward(aug, name):
    """<L x, y> = <x, L^T y> with the gather as L^T and the existing forward as L (less its offset, forward(0)).
    Bound as in test_gpu_ada.py: E32_MULTIPLE * (e32_y |y|_1 + e32_gx |x|_1)."""
    c = tc.case(name)
    g = torch.Generator().manual_seed(1)
    x = (torch.rand(c["x"].shape, generator=g) * 2 - 1) * float(c["x"].abs().max()) * 0.75
    y = torch.randn(c["x"].shape, generator=g)
    run = tc.public(aug, c, 1)
    lx = (run(x.cuda()) - run(torch.zeros_like(x).cuda())).cpu().double()
    aty = gather_adjoint(aug, c, y.cuda()).cpu().double()
    lhs, rhs = float((lx * y.double()).sum()), float((x.double() * aty).sum())
    bound = ac.E32_MULTIPLE * (c["e32_y"] * float(y.abs().sum()) + c["e32_gx"] * float(x.abs().sum()))
    print(name, "<Lx,y>", lhs, "<x,L^T y>", rhs, "difference", abs(lhs - rhs), "bound", bound,
          "relative", abs(lhs - rhs) / float(lx.norm() * y.double().norm()))
    assert abs(lhs - rhs) <= bound


@pytest.mark.parametrize("name", ["batch3", "tiles40x24", "scale0.4", "aniso45"])
def test_gather_is_bit_identical_in_either_mode(aug, name):
    from gan2shape_amd import lib
    c = tc.case(name)
    gy = c["gy"].cuda()
    runs = []
    for mode in (False, True):
        prev = lib.set_deterministic(mode)
        try:
            runs += [gather_adjoint(aug, c, gy, keep_gx2=True) for _ in range(3)]
        finally:
            lib.set_deterministic(prev)
    assert all(torch.equal(runs[0], r) for r in runs[1:])


def test_gather_writes_exact_zeros_where_the_warp_never_samples(aug):
    """scale0.4: the 52 x 68 sample positions step 0.4 source pixels about the centre of the 48 x 56 double-resolution
    image, rotated by 20 degrees in the second sample: they stay within 14.4 + 1 rows of row 23.5, so rows 0..5 and
    42..47 of gx2 receive nothing.  gx2 and the workspace enter as NaN."""
    c = tc.case("scale0.4")
    gx2 = gather_adjoint(aug, c, c["gy"].cuda(), keep_gx2=True)
    assert gx2.shape == (2, 3, 48, 56) and bool(torch.isfinite(gx2).all())
    assert bool((gx2[:, :, :6] == 0).all()) and bool((gx2[:, :, -6:] == 0).all())
    assert bool((gx2[:, :, 20:28, 24:32] != 0).all())                        # and the centre, sampled densely, does


@pytest.mark.parametrize("name", tc.names())
def test_order_2_backward_runs_in_deterministic_mode(aug, deterministic, name):
    """augment(order=2).backward() under g2s_set_deterministic: runs (order=1 refuses), bit-identical over three runs,
    within the golden bound."""
    c = tc.case(name)
    grads = []
    for _ in range(3):
        x = c["x"].cuda().requires_grad_(True)
        y = tc.public(aug, c, 2)(x)
        y.backward(c["gy"].cuda())
        grads.append(x.grad)
    assert torch.equal(grads[0], grads[1]) and torch.equal(grads[0], grads[2])
    ey, eg = float((y.detach().cpu().double() - c["y"]).abs().max()), float((grads[0].cpu().double() - c["gx"]).abs().max())
    print(name, "deterministic order 2 error / e32: y", ey / c["e32_y"], "gx", eg / c["e32_gx"])
    assert ey <= ac.E32_MULTIPLE * c["e32_y"] and eg <= ac.E32_MULTIPLE * c["e32_gx"]


@pytest.mark.parametrize("name", tc.names())
def test_order_2_with_the_mode_off_has_the_bits_of_order_1_forward(aug, name):
    """Same forward kernels: equal bits; the gradient (the scatter, float atomics) within the golden bound."""
    c = tc.case(name)
    x = c["x"].cuda().requires_grad_(True)
    y = tc.public(aug, c, 2)(x)
    assert torch.equal(y.detach(), tc.public(aug, c, 1)(c["x"].cuda()))
    gx, = torch.autograd.grad(y, x, c["gy"].cuda())
    assert float((gx.cpu().double() - c["gx"]).abs().max()) <= ac.E32_MULTIPLE * c["e32_gx"]


def _second_on_gpu(fn, c):
    x = c["x"].cuda().requires_grad_(True)
    g, q, gg = tc.second_order(fn, x, tc.weight(c).cuda())
    return g.cpu().double(), q.cpu().double(), gg.cpu().double()


def _second_ratios(got, ref):
    g, q, gg = got
    return (float((g - ref["g"]).abs().max()) / ref["e32_g"], float((q - ref["q"]).abs()) / ref["e32_q"],
            float((gg - ref["gg"]).abs().max()) / ref["e32_gg"])


@pytest.mark.parametrize("mode", [False, True], ids=["scatter", "gather"])
@pytest.mark.parametrize("name", tc.SECOND_CASES)
def test_second_order_matches_the_float64_composition(aug, name, mode):
    """g = d/dx sum(augment(x)^2 r), q = sum(g^2) and dq/dx against augment._augment_twice on the CPU in float64.
    The reference cannot serve: its grid_sample has no second derivative (make_ada_golden.py replaces its wrapper by
    F.grid_sample for that reason).  e32 per quantity: the float32 CPU run of the same composition against its float64
    run; bound SECOND_MULTIPLE x e32 (ada_twice_cases.py).  Both warp adjoints: the mode off and on."""
    from gan2shape_amd import lib
    c = tc.case(name)
    ref = tc.second_reference(aug, name)
    prev = lib.set_deterministic(mode)
    try:
        got = _second_on_gpu(tc.public(aug, c, 2), c)
    finally:
        lib.set_deterministic(prev)
    rg, rq, rgg = _second_ratios(got, ref)
    print(name, "mode", mode, "second order error / e32: g", rg, "q", rq, "dq/dx", rgg,
          "| e32", ref["e32_g"], ref["e32_q"], ref["e32_gg"])
    assert rg <= tc.SECOND_MULTIPLE and rq <= tc.SECOND_MULTIPLE and rgg <= tc.SECOND_MULTIPLE


@pytest.mark.parametrize("name", ["rot30", "batch3", "gray", "aniso45"])
def test_the_gradient_of_the_adjoint_node_is_the_linear_forward(aug, name):
    """d/d gy <_AdaAdj(gy), ggx> = L ggx = forward(ggx) - forward(0) of the existing forward: the same kernels, only
    the offset differs.  forward(0) is the offset itself, exactly; forward(ggx) rounds L ggx + offset once more than
    the node rounds L ggx, and the subtraction rounds once: 4 float32 roundings of the largest entry are allowed."""
    c = tc.case(name)
    warp, pads, cmat = tc.host_matrices(aug, c)
    warp, cmat = warp.cuda(), None if cmat is None else cmat.cuda()
    g = torch.Generator().manual_seed(7)
    ggx = torch.randn(c["x"].shape, generator=g).cuda()
    gy = c["gy"].cuda().requires_grad_(True)
    gx = aug._AdaAdj.apply(gy, warp, cmat, pads)
    got, = torch.autograd.grad(gx, gy, ggx)
    run = tc.public(aug, c, 1)
    full = run(ggx)
    want = full - run(torch.zeros_like(ggx))
    err, allowed = float((got - want).abs().max()), 4 * EPS32 * float(full.abs().max())
    print(name, "linearity error", err, "allowed", allowed)
    assert err <= allowed
    if cmat is None:
        assert torch.equal(got, full)


def test_augment_differentiable_takes_the_node_pair_on_the_gpu(aug):
    from gan2shape_amd import dtrain
    c = tc.case("batch3")
    ref = tc.second_reference(aug, "batch3")
    x = c["x"].cuda().requires_grad_(True)
    y, (G, C) = dtrain.augment_differentiable(x, 0.5, (c["G"], c["C"]))
    assert G is c["G"] and C is c["C"] and type(y.grad_fn).__name__ == "_AdaFwdBackward"
    z, _ = dtrain.augment_differentiable(x, 0.5, (c["G"], c["C"]), composed=True)
    assert z.grad_fn is not None and type(z.grad_fn).__name__ != "_AdaFwdBackward"
    node = _second_on_gpu(lambda t: dtrain.augment_differentiable(t, 0.5, (c["G"], c["C"]))[0], c)
    comp = _second_on_gpu(lambda t: dtrain.augment_differentiable(t, 0.5, (c["G"], c["C"]), composed=True)[0], c)
    dg, dq, dgg = (float((a - b).abs().max()) for a, b in zip(node, comp))
    print("node - composition / e32: g", dg / ref["e32_g"], "q", dq / ref["e32_q"], "dq/dx", dgg / ref["e32_gg"])
    assert dg <= tc.SECOND_MULTIPLE * ref["e32_g"] and dq <= tc.SECOND_MULTIPLE * ref["e32_q"]
    assert dgg <= tc.SECOND_MULTIPLE * ref["e32_gg"]
    # a CUDA tensor of another dtype has no kernels: the composition
    h, _ = dtrain.augment_differentiable(c["x"].cuda().double().requires_grad_(True), 0.5, (c["G"], c["C"]))
    assert h.dtype == torch.float64 and type(h.grad_fn).__name__ != "_AdaFwdBackward"


def _four_steps(seed):
    """One logistic step, one R1 step, one non-saturating step and one path step at G(8) / D(8), B = 4, with
    augmentation at p = 0.8, from `seed`: (losses, the final weights of D, G and g_ema)."""
    from gan2shape_amd import dtrain, gtrain
    from gan2shape_amd import stylegan2 as sg2
    from gan2shape_amd.op import conv2d_gradfix
    torch.manual_seed(seed)
    random.seed(seed)
    g = sg2.Generator(8, 32, 2, channel_multiplier=1).cuda().train()
    d = sg2.Discriminator(8, channel_multiplier=1).cuda().train()
    g_ema = copy.deepcopy(g).eval()
    dt = dtrain.DiscriminatorTrainer(d, augment=True, augment_p=0.8)
    gt = gtrain.GeneratorTrainer(g, g_ema, d, batch=4, augment=True)
    gt.ada_aug_p = dt.ada_aug_p
    real = torch.rand(4, 3, 8, 8, device="cuda") * 2 - 1
    with conv2d_gradfix.use():
        with torch.no_grad():
            fake, _ = g(gtrain.mixing_noise(4, 32, 0.9, "cuda"))
        loss = dt.step(real, fake, 0)            # i = 0: the logistic step and the R1 step
        loss.update(gt.step(0))                  # i = 0: the non-saturating step and the path step
    torch.cuda.synchronize()
    weights = [p.detach().clone() for net in (d, g, g_ema) for p in net.parameters()]
    return {k: float(v) for k, v in loss.items()}, weights


@pytest.fixture(scope="module")
def two_trainer_runs(aug):
    from gan2shape_amd import lib
    prev = lib.set_deterministic(True)
    try:
        return _four_steps(5), _four_steps(5)
    finally:
        lib.set_deterministic(prev)


def test_trainers_run_with_augmentation_in_deterministic_mode(two_trainer_runs):
    (loss, weights), _ = two_trainer_runs
    print("losses", loss)
    assert set(loss) >= {"d", "r1", "g", "path"}
    assert all(v == v and abs(v) != float("inf") for v in loss.values()), loss
    assert loss["r1"] > 0 and all(bool(torch.isfinite(w).all()) for w in weights)


def test_trainers_are_bit_identical_from_equal_seeds(two_trainer_runs):
    (loss_a, a), (loss_b, b) = two_trainer_runs
    differ = [i for i, (p, q) in enumerate(zip(a, b)) if not torch.equal(p, q)]
    print("losses", loss_a, loss_b, "parameters that differ:", differ)
    assert loss_a == loss_b and not differ
