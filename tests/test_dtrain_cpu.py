"""Discriminator training without a GPU: the float64 statements of dtrain_cases.py and the CPU route of
gan2shape_amd.dtrain reproduce the reference's float64 fixture (tests/golden/dtrain.npz), the trainer's
hyper-parameters, the lazy-regularisation schedule, the state-dict round trip and `no_weight_gradients`."""
import io

import numpy as np
import pytest
import torch

import dtrain_cases as dc

REL = 1e-12


@pytest.fixture(scope="module")
def fx(golden):
    return golden("dtrain")


@pytest.fixture(scope="module")
def pkg():
    import gan2shape_amd  # noqa: F401
    from gan2shape_amd import dtrain
    from gan2shape_amd.op import conv2d_gradfix
    from gan2shape_amd.stylegan2 import Discriminator
    return dtrain, conv2d_gradfix, Discriminator


@pytest.fixture(scope="module")
def d64(pkg):
    d = pkg[2](dc.SIZE, channel_multiplier=dc.CHANNEL_MULTIPLIER).double()
    return dc.fill_weights(d), dc.draw_like(d, dc.PROBE_SEED)


def close(got, want, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    err = float(np.abs(got - want).max()) / max(float(np.abs(want).max()), 1e-300)
    print(what, "relative error", err)
    assert err <= REL, (what, err)


def check_case(fx, name, lg, rp, probe):
    close(lg["real_pred"], fx[f"{name}.real_pred"], "real_pred")
    close(lg["fake_pred"], fx[f"{name}.fake_pred"], "fake_pred")
    close(lg["loss"], fx[f"{name}.loss"], "loss")
    for key in ("real_pred", "grad_real", "per_sample", "r1"):
        close(rp[key], fx[f"{name}.r1.{key}"], "r1." + key)
    for tag, res in (("log", lg), ("r1", rp)):
        norms, proj = dc.summarize(res["grads"], probe)
        close(norms, fx[f"{name}.{tag}.norms"], tag + ".norms")
        close(proj, fx[f"{name}.{tag}.proj"], tag + ".proj")


@pytest.mark.parametrize("name", list(dc.CASES))
def test_float64_statements_reproduce_the_fixture(fx, d64, name):
    d, probe = d64
    real, fake = torch.from_numpy(fx[f"{name}.real"]).double(), torch.from_numpy(fx[f"{name}.fake"]).double()
    assert np.array_equal(fx[f"{name}.real"], dc.images(dc.CASES[name])[0])
    check_case(fx, name, dc.logistic_pass(d, real, fake), dc.r1_pass(d, real), probe)


@pytest.mark.parametrize("name", list(dc.CASES))
def test_cpu_route_of_the_losses_reproduces_the_fixture(fx, d64, pkg, name):
    dtrain = pkg[0]
    d, probe = d64
    real, fake = torch.from_numpy(fx[f"{name}.real"]).double(), torch.from_numpy(fx[f"{name}.fake"]).double()
    check_case(fx, name, dc.logistic_pass(d, real, fake, dtrain.d_logistic_loss),
               dc.r1_pass(d, real, loss_fn=dtrain.d_r1_loss), probe)


def test_mbstd_statement_is_the_discriminators_composition(pkg):
    d = pkg[2](dc.SIZE, channel_multiplier=1)
    x = torch.randn(8, 16, 4, 4, dtype=torch.float64)
    assert torch.equal(dc.mbstd(x), torch.cat([x, d._group_stddev(x)], 1))


def test_trainer_hyperparameters(pkg):
    dtrain, _, D = pkg
    t = dtrain.DiscriminatorTrainer(D(8, 1))
    c = 16 / 17
    group = t.d_optim.param_groups[0]
    assert group["lr"] == 0.002 * c and tuple(group["betas"]) == (0 ** c, 0.99 ** c)
    assert (t.r1, t.d_reg_every, t.augment, t.ada_aug_p, t.ada) == (10, 16, False, 0.0, None)
    t = dtrain.DiscriminatorTrainer(D(8, 1), lr=0.01, d_reg_every=4, augment=True, augment_p=0.3)
    assert t.d_optim.param_groups[0]["lr"] == 0.01 * 4 / 5 and t.ada_aug_p == 0.3 and t.ada is None
    t = dtrain.DiscriminatorTrainer(D(8, 1), augment=True, ada_target=0.5, ada_length=1000)
    assert (t.ada.ada_aug_target, t.ada.ada_aug_len, t.ada.update_every) == (0.5, 1000, 8)


def test_lazy_regularisation_schedule(pkg, monkeypatch):
    dtrain, _, D = pkg
    torch.manual_seed(0)
    t = dtrain.DiscriminatorTrainer(D(8, 1))
    ran = []
    orig = dtrain.d_r1_loss
    monkeypatch.setattr(dtrain, "d_r1_loss", lambda p, x: (ran.append(step[0]), orig(p, x))[1])
    step = [0]
    last = None
    for i in range(33):
        step[0] = i
        out = t.step(torch.randn(2, 3, 8, 8), torch.randn(2, 3, 8, 8), i)
        assert set(out) == {"d", "real_score", "fake_score", "r1"}
        if i in (0, 16, 32):
            assert last is None or float(out["r1"]) != last
        else:
            assert float(out["r1"]) == last         # the last R1 value is reported between its steps
        last = float(out["r1"])
    assert ran == [0, 16, 32]
    assert [i for i in range(33) if t.regularizes(i)] == [0, 16, 32]


def test_state_dict_round_trip(pkg):
    dtrain, _, D = pkg
    torch.manual_seed(1)
    a = dtrain.DiscriminatorTrainer(D(8, 1), augment=True, augment_p=0.25)
    batches = [(torch.randn(2, 3, 8, 8), torch.randn(2, 3, 8, 8)) for _ in range(3)]
    a.step(*batches[0], 0)
    buf = io.BytesIO()
    torch.save(a.state_dict(), buf)                  # as the command writes it: state_dict() itself refers to live tensors
    state = torch.load(io.BytesIO(buf.getvalue()), weights_only=True)
    assert set(state) == {"d", "d_optim", "ada_aug_p"} and state["ada_aug_p"] == 0.25
    b = dtrain.DiscriminatorTrainer(D(8, 1), augment=True, augment_p=0.25)
    b.load_state_dict(state)
    for i in (1, 2):            # neither step regularises: no augmentation draw differs between the two
        torch.manual_seed(10 + i)
        a.step(*batches[i], i)
        torch.manual_seed(10 + i)
        b.step(*batches[i], i)
    for (n, p), q in zip(a.d.named_parameters(), b.d.parameters()):
        assert torch.equal(p, q), n


def test_differentiable_augmentation_is_the_augmentation(pkg):
    dtrain = pkg[0]
    from gan2shape_amd import augment
    torch.manual_seed(3)
    x = torch.randn(2, 3, 16, 16, dtype=torch.float64)
    G = torch.inverse(augment.sample_affine(0.8, 2, 16, 16))
    C = augment.sample_color(0.8, 2)
    want, _ = augment.augment(x, 0.8, (G, C))
    xg = x.clone().requires_grad_(True)
    got, _ = dtrain.augment_differentiable(xg, 0.8, (G, C))
    assert float((got - want).abs().max()) <= 1e-12
    g, = torch.autograd.grad(got.square().sum(), xg, create_graph=True)
    g.square().sum().backward()                      # a second backward exists
    assert torch.isfinite(xg.grad).all() and float(xg.grad.abs().max()) > 0


def test_no_weight_gradients_on_the_cpu_route(pkg):
    dtrain, gradfix, D = pkg
    d = dc.fill_weights(D(8, 1).double())
    x = torch.randn(2, 3, 8, 8, dtype=torch.float64, requires_grad=True)
    assert not gradfix._NO_WEIGHT_GRADIENTS
    with gradfix.no_weight_gradients():
        assert gradfix._NO_WEIGHT_GRADIENTS
        with gradfix.no_weight_gradients(False):
            assert gradfix._NO_WEIGHT_GRADIENTS      # nested: stays disabled
    assert not gradfix._NO_WEIGHT_GRADIENTS
    pred = d(x)[0]
    loss = dtrain.d_r1_loss(pred, x)                 # CPU tensors: torch's convolutions, whose weights still train
    assert not gradfix._NO_WEIGHT_GRADIENTS
    loss.backward()
    assert all(p.grad is not None for n, p in d.named_parameters() if n != "final_linear.1.bias")
    assert float(d.convs[0][0].weight.grad.abs().max()) > 0
    with gradfix.use():
        assert gradfix.ENABLED
        assert torch.equal(d(x)[0], pred)            # the switch changes nothing for CPU tensors
    assert not gradfix.ENABLED
