"""Generator training without a GPU: this package's torch route (CPU, float64) against the reference's float64
fixture (tests/golden/gtrain.npz) to 1e-10 relative — the loss functions, g_path_regularize, accumulate and the
trainer's two steps; the `train` parser and checkpoint keys; and UP2 as the adjoint of DOWN2."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dtrain_cases as dc
import gtrain_cases as gc

REL = 1e-10


@pytest.fixture(scope="module")
def fx(golden):
    return golden("gtrain")


@pytest.fixture(scope="module")
def pkg():
    import gan2shape_amd  # noqa: F401
    from gan2shape_amd import gtrain, train
    from gan2shape_amd.stylegan2 import Discriminator, Generator
    return gtrain, train, Generator, Discriminator


def nets(pkg, dtype=torch.float64):
    _, _, G, D = pkg
    g = dc.fill_weights(G(gc.SIZE, gc.STYLE_DIM, gc.N_MLP, channel_multiplier=gc.CHANNEL_MULTIPLIER).to(dtype), gc.G_SEED)
    d = dc.fill_weights(D(gc.SIZE, channel_multiplier=gc.CHANNEL_MULTIPLIER).to(dtype), gc.D_SEED)
    return g, d.requires_grad_(False)


def close(got, want, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    err = float(np.abs(got.reshape(want.shape) - want).max())
    assert err <= REL * float(np.abs(want).max()), (what, err)


def test_fixture_is_complete(fx):
    assert list(fx["names"]) == list(gc.CASES)
    for name in gc.CASES:
        for k in ("image", "loss", "path.lengths", "path.path_mean", "path.penalty", "ns.norms", "ns.proj", "path.norms",
                  "path.proj"):
            assert f"{name}.{k}" in fx and float(fx[f"{name}.e32_{k}"]) >= 0
        lengths = fx[f"{name}.path.lengths"]
        assert lengths.min() >= 0.1 * lengths.mean()


@pytest.mark.parametrize("name", list(gc.CASES))
def test_torch_route_reproduces_the_reference(pkg, fx, name):
    gtrain = pkg[0]
    g, d = nets(pkg)
    like = torch.zeros((), dtype=torch.float64)
    probe = dc.draw_like(g, gc.PROBE_SEED)
    assert list(probe) == list(fx["params"])
    zs, maps, img = gc.inputs(name)
    inject = gc.CASES[name][2]
    ns = gc.nonsaturating_pass(g, d, gc.to(zs, like), gc.to(maps, like), inject, gtrain.g_nonsaturating_loss)
    pp = gc.path_pass(g, gc.to(zs, like), gc.to(maps, like), inject, gc.to([img], like)[0],
                      loss_fn=gtrain.g_path_regularize)
    got = {"image": ns["image"], "loss": ns["loss"], "path.lengths": pp["lengths"], "path.path_mean": pp["path_mean"],
           "path.penalty": pp["penalty"]}
    got = {k: v.numpy() for k, v in got.items()}
    got["ns.norms"], got["ns.proj"] = gc.summarize(ns["grads"], probe)
    got["path.norms"], got["path.proj"] = gc.summarize(pp["grads"], probe)
    for k, v in got.items():
        close(v, fx[f"{name}.{k}"], k)


def test_accumulate_and_noise(pkg):
    gtrain = pkg[0]
    a, b = torch.nn.Linear(5, 3).double(), torch.nn.Linear(5, 3).double()
    a2 = copy.deepcopy(a)
    gtrain.accumulate(a, b, 0.75)
    gc.accumulate(a2, b, 0.75)
    for p, q in zip(a.parameters(), a2.parameters()):
        assert torch.equal(p, q)
    assert gtrain.make_noise(3, 7, 1, "cpu").shape == (3, 7)
    two = gtrain.make_noise(3, 7, 2, "cpu")
    assert len(two) == 2 and two[0].shape == (3, 7)
    assert len(gtrain.mixing_noise(3, 7, 0.0, "cpu")) == 1 and len(gtrain.mixing_noise(3, 7, 1.0, "cpu")) == 2


def test_trainer_two_steps_on_cpu(pkg, fx):
    gtrain = pkg[0]
    g, d = nets(pkg)
    g_ema = copy.deepcopy(g)
    start = {n: p.detach().clone() for n, p in d.named_parameters()}
    like = torch.zeros((), dtype=torch.float64)
    trainer = gtrain.GeneratorTrainer(g, g_ema, d, batch=4)
    for (zs, maps, _), path_in, i in gc.trainer_inputs():
        kw = {}
        if path_in is not None:
            kw = dict(path_noise=gc.to(path_in[0], like), path_maps=gc.to(path_in[1], like),
                      image_noise=gc.to([path_in[2]], like)[0])
        out = trainer.step(i, noise=gc.to(zs, like), maps=gc.to(maps, like), **kw)
        assert all(torch.isfinite(v).item() for v in out.values())
    probe = dc.draw_like(g, gc.PROBE_SEED)
    close(gc.projections(g, probe), fx["trainer.g"], "g")
    close(gc.projections(g_ema, probe), fx["trainer.g_ema"], "g_ema")
    for n, p in d.named_parameters():
        assert torch.equal(p, start[n])


def test_train_parser_and_checkpoint_keys(pkg):
    train = pkg[1]
    args = train.build_parser().parse_args(["--size", "8", "--data", "x", "--out", "y", "--latent", "16", "--n-mlp", "1",
                                            "--channel-multiplier", "1", "--batch", "2", "--device", "cpu"])
    assert (args.g_reg_every, args.d_reg_every, args.path_batch_shrink, args.path_regularize, args.mixing, args.r1) == \
        (4, 16, 2, 2, 0.9, 10)
    with pytest.raises(SystemExit):
        train.build_parser().parse_args(["--size", "8"])
    dt, gt = train.build_trainers(args, torch.device("cpu"))
    ckpt = train.checkpoint(dt, gt)
    assert tuple(ckpt) == train.CHECKPOINT_KEYS == ("g", "d", "g_ema", "g_optim", "d_optim", "ada_aug_p")
    for a, b in zip(gt.g.parameters(), gt.g_ema.parameters()):
        assert torch.equal(a, b) and a is not b


def test_train_resumes_from_a_checkpoint(pkg, tmp_path):
    train = pkg[1]
    argv = ["--size", "8", "--data", "x", "--out", "y", "--latent", "16", "--n-mlp", "1", "--channel-multiplier", "1",
            "--batch", "2", "--device", "cpu"]
    dt, gt = train.build_trainers(train.build_parser().parse_args(argv), torch.device("cpu"))
    with torch.no_grad():
        for p in gt.g_ema.parameters():
            p.add_(1.0)                                  # g_ema apart from g
    path = str(tmp_path / "ckpt.pt")
    torch.save(train.checkpoint(dt, gt), path)
    dt2, gt2 = train.build_trainers(train.build_parser().parse_args(argv + ["--ckpt", path]), torch.device("cpu"))
    for a, b in ((gt.g, gt2.g), (gt.g_ema, gt2.g_ema), (dt.d, dt2.d)):
        for p, q in zip(a.parameters(), b.parameters()):
            assert torch.equal(p, q)
    assert train.build_parser().parse_args(argv).save_every == 10000


@pytest.mark.parametrize("k", [1, 3])
def test_up2_is_the_adjoint_of_down2(k):
    """UP2(x, w) = F.conv_transpose2d(x, w.transpose(0, 1), stride=2) is the adjoint, in x, of the stride-2
    convolution whose weight is w.transpose(0, 1) ([Cin, Cout, k, k]): stated in torch, float64."""
    g = torch.Generator().manual_seed(k)
    x = torch.randn(2, 5, 4, 4, generator=g, dtype=torch.float64)
    w = torch.randn(7, 5, k, k, generator=g, dtype=torch.float64)
    side = 2 * 4 + k - 2
    z = torch.randn(2, 7, side, side, generator=g, dtype=torch.float64, requires_grad=True)
    down = F.conv2d(z, w.transpose(0, 1), stride=2)                     # [2, 5, 4, 4]
    assert down.shape == x.shape
    adjoint, = torch.autograd.grad(down, z, x)
    up = F.conv_transpose2d(x, w.transpose(0, 1), stride=2)
    assert up.shape == adjoint.shape == (2, 7, side, side)
    assert float((up - adjoint).abs().max()) <= 1e-12 * float(up.abs().max())
