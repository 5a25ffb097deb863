"""Symmetry flips (flip1_cfg / flip3_cfg / lam_flip) without a GPU: the package's torch-composed route (cat / flip)
in float64 against tests/golden/symmetry.npz — the flipped step 1 and step 3 composed from the reference model's own
parts (tests/golden/make_symmetry_golden.py) — and the host logic: the per-stage switches of the trainers."""
import numpy as np
import pytest
import torch

import model_cases as mc
import symmetry_cases as sc

REL = 1e-10


def _zero_grads(m):
    for p in m.parameters():
        p.grad = None


def build_cpu_model(steps, dtype=torch.float64):
    """This package's GAN2Shape on the CPU in the state of the reference model of make_symmetry_golden.py: the four
    trained nets with the seeded weights, the smooth depth net, the stand-in perceptual loss, the C oracle behind the
    rasterizer boundary (the package's own rasterizer is a HIP kernel).  No generator, discriminator or LPIPS trunk:
    steps 1 and 3 do not touch them."""
    from gan2shape_amd import networks
    from gan2shape_amd.losses import PhotometricLoss, SmoothLoss
    from gan2shape_amd.model import GAN2Shape, ViewLightSampler
    from gan2shape_amd.renderer import Renderer
    S = mc.STEP_CFG["image_size"]
    m = object.__new__(GAN2Shape)
    torch.nn.Module.__init__(m)
    m.device, m.image_size, m.debug = torch.device("cpu"), S, False
    for name, cls in (("lighting", "LightingNet"), ("viewpoint", "ViewpointNet"), ("depth", "DepthNet"),
                      ("albedo", "AlbedoNet")):
        net = getattr(networks, cls)(S)
        mc.fill_scaled(net, mc.STEP_CFG["seeds"][name])
        if name == "depth":
            mc.smooth_depth_net(net)
        setattr(m, f"{name}_net", net.to(dtype))
    m.paired_nets = m.parallel_nets = False
    m._side_streams = []
    m.max_depth, m.min_depth = 1.1, 0.9
    m.border_depth = 0.7 * m.max_depth + 0.3 * m.min_depth
    m.lam_perc, m.lam_smooth, m.lam_regular, m.lam_flip = 1, 0.01, 0.01, sc.LAM_FLIP
    m.xyz_rotation_range, m.xy_translation_range, m.z_translation_range = 60, 0.1, 0.1
    m.batch_mean = m._depth_border = None
    m.renderer = Renderer({"rot_center_depth": 1.0, "fov": 10, "tex_cube_size": 2}, S, m.min_depth, m.max_depth,
                          device="cpu")
    m.renderer.renderer = sc.OracleRasterizer(m.renderer.K.numpy(), S)
    m.renderer.K, m.renderer.inv_K = m.renderer.K.to(dtype), m.renderer.inv_K.to(dtype)
    m.view_light_sampler = ViewLightSampler(None, None, 1, "cpu",
                                            {"mean": steps["vls.vm"].tolist(), "cov": steps["vls.vc"].tolist()},
                                            {"mean": steps["vls.lm"].tolist(), "cov": steps["vls.lc"].tolist()})
    m.smooth_loss, m.photometric_loss = SmoothLoss(), PhotometricLoss()
    m.perceptual_loss = mc.fake_perceptual
    return m


@pytest.fixture(scope="module")
def cpu_case(golden):
    steps, g = golden("steps"), golden("symmetry")
    m = build_cpu_model(steps)
    image = torch.tensor(g["image"]).double()
    c2 = (torch.tensor(steps["s2.projected"]).double(), torch.tensor(steps["s2.mask"]).double())
    return m, g, image, c2


@pytest.fixture()
def float64_default():
    """The float64 run of the golden has float64 as the default dtype (its constants are built with torch.zeros)."""
    torch.set_default_dtype(torch.float64)
    yield
    torch.set_default_dtype(torch.float32)


@pytest.mark.parametrize("name", list(sc.PASSES))
def test_cpu_route_reproduces_the_float64_golden(cpu_case, float64_default, name):
    m, g, image, c2 = cpu_case
    got = sc.run_pass(m, name, image, None, c2, mc.grad_evidence, _zero_grads)
    assert float(g["lam_flip"]) == m.lam_flip
    for key, v in got.items():
        ref = g[key]
        assert v.shape == ref.shape, (key, v.shape, ref.shape)
        # losses, terms, reconstructions and `collected`: 1e-10 of the quantity's scale; the gradient evidence has gone
        # through the rasterizer's backward and four nets: 1e-8
        rel = 1e-8 if (".gnorm." in key or ".gtnorm." in key or ".gproj." in key) else REL
        err, scale = sc.distance(v, ref), float(np.max(np.abs(ref)))
        assert err <= rel * scale, (key, err, scale)
    assert abs(float(got[f"{name}.l1_flip"]) - float(got[f"{name}.l1"])) > 1e-4      # the halves are not the same thing


def test_collected_shapes_do_not_depend_on_the_flip(cpu_case, float64_default):
    m, g, image, c2 = cpu_case
    try:
        with torch.no_grad():
            _, off = m.forward_step1(image, None, None)
            m.flip1 = True
            loss_on, on = m.forward_step1(image, None, None)
            loss_off, _ = m.forward_step1(image, None, None, step1=False)        # flip3 is off: the plain pass
        assert [tuple(t.shape) for t in on[:5]] == [tuple(t.shape) for t in off[:5]] and on[5] is None and off[5] is None
        for a, b in zip(on[:5], off[:5]):       # and the B plain rows are the plain pass's
            assert torch.allclose(a, b, rtol=0, atol=1e-12)
        assert abs(float(loss_on) - float(loss_off)) > 1e-4
    finally:
        m.flip1 = False


def test_eval_ignores_the_flip(cpu_case, float64_default):
    m, g, image, c2 = cpu_case
    try:
        with torch.no_grad():
            im_off, depth_off = m.forward_step1(image, None, None, eval=True)
            m.flip1 = m.flip3 = True
            im_on, depth_on = m.forward_step1(image, None, None, eval=True)
            im_on3, _ = m.forward_step1(image, None, None, step1=False, eval=True)
        assert im_on.shape == im_off.shape == (1, 3, m.image_size, m.image_size)
        assert torch.equal(im_on, im_off) and torch.equal(depth_on, depth_off) and torch.equal(im_on3, im_off)
    finally:
        m.flip1 = m.flip3 = False


def test_decompose_is_forward_step1_behind_the_nets(cpu_case, float64_default):
    m, g, image, c2 = cpu_case          # paired_nets is False on this model: both call each net on its own
    assert m.paired_nets is False
    with torch.no_grad():
        d = m.decompose(image)
        _, c1 = m.forward_step1(image, None, None)
        view = m.viewpoint_net(image) + m.view_light_sampler.view_mean.unsqueeze(0)
        light = m.lighting_net(image) + m.view_light_sampler.light_mean.unsqueeze(0)
    for key, got, want in zip(sc.COLLECTED, d["collected"][:5], c1[:5]):
        assert torch.equal(got, want), key
    assert torch.equal(d["view"], view) and torch.equal(d["light"], light)


class RecordingModel(mc.ToyStepModel):
    """The toy step model of the trainer tests; every step call records (kind, flip1, flip3)."""

    def __init__(self, config, debug=False, device="cpu"):
        super().__init__(config, debug, device)
        self.seen = []

    def forward_step1(self, *a, **k):
        self.seen.append((1, self.flip1, self.flip3))
        return super().forward_step1(*a, **k)

    def forward_step2(self, *a, **k):
        self.seen.append((2, self.flip1, self.flip3))
        return super().forward_step2(*a, **k)

    def forward_step3(self, *a, **k):
        self.seen.append((3, self.flip1, self.flip3))
        return super().forward_step3(*a, **k)


def _fit(cfg_extra, stages):
    from gan2shape_amd.trainer import Trainer
    t = Trainer(RecordingModel, dict(mc.TOY_CFG, **cfg_extra), debug=True, device="cpu")
    t.fit(mc.toy_dataset(1), stages=stages)
    return t.model.seen


ONE_EACH = {'step1': 1, 'step2': 1, 'step3': 1}


def test_trainer_sets_the_switches_per_stage():
    seen = _fit(dict(flip1_cfg=[True, False], flip3_cfg=[False, True]), [ONE_EACH] * 2)
    assert seen == [(1, True, False), (2, True, False), (3, True, False),
                    (1, False, True), (2, False, True), (3, False, True)]


def test_short_list_repeats_its_last_entry_and_missing_key_is_off():
    seen = _fit(dict(flip1_cfg=[False, True]), [ONE_EACH] * 4)
    assert [s[1] for s in seen if s[0] == 1] == [False, True, True, True]
    assert all(s[2] is False for s in seen)                      # flip3_cfg missing: off in every stage
    seen = _fit({}, [ONE_EACH] * 2)
    assert all(s[1] is False and s[2] is False for s in seen)


def test_joint_trainer_uses_entry_zero():
    from gan2shape_amd.trainer import GeneralizingTrainer2

    class Joint(mc.ToyJointModel):
        def forward_step1(self, *a, **k):
            self.flips = (self.flip1, self.flip3)
            return super().forward_step1(*a, **k)
    t = GeneralizingTrainer2(Joint, dict(mc.TOY_JOINT_CFG, flip1_cfg=[True, False], flip3_cfg=[False, True]), device="cpu")
    t.prior_generator = lambda image, device="cpu": mc.toy_prior(image)
    t.fit(mc.toy_dataset(2), stages=mc.TOY_JOINT_STAGES, batch_size=2)
    assert t.model.flips == (True, False)


def test_model_defaults():
    from gan2shape_amd.model import GAN2Shape
    assert GAN2Shape.flip1 is False and GAN2Shape.flip3 is False and GAN2Shape.lam_flip == 0.5
