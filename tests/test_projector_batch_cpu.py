"""-m "not gpu": the batched projector's host side — project_batch on CPU tensors (layer loop + torch noise functions)
against three steps of the reference's loop at B = 2 (tests/golden/projector_batch.npz, bounds 4 x the reference's own
float32-vs-float64 distance for the same quantity), the command with --batch, batched sampling on CPU tensors, the
switch, and the argument checks of the new C entries."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import gan2shape_amd  # noqa: F401
from gan2shape_amd import dataset, generate, lib, projector, synthesis
from gan2shape_amd import stylegan2 as sg2

import projector_cases as pc
import projector_batch_cases as pb

MARGIN = 4.0     # x the reference's own float32 error


@pytest.fixture(scope="module")
def fx(golden):
    return golden("projector_batch")


def test_fixture_is_no_larger_than_the_projector_fixture():
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    assert os.path.getsize(os.path.join(here, "projector_batch.npz")) <= os.path.getsize(os.path.join(here, "projector.npz"))


def test_three_steps_of_project_batch_equal_the_reference_loop(fx):
    """Three steps at B = 2 on CPU tensors with the stand-in perceptual term; the maps and the jitter come from the
    torch.Generator stream the fixture's inputs were read from (projector_batch_cases.loop_inputs), so project_batch
    draws exactly the reference run's inputs.  The latent and every map after each step against the reference's float64
    loop, each within 4 x the reference's own float32 distance for that quantity (the fixture stores it, maximum over
    N_SEEDS inputs; step 0 runs at learning rate 0, so its latent must be exact).

    Measured: every quantity sits at the reference's own float32 distance for this input (latent 2.3e-07 and 3.1e-07
    after steps 1 and 2, maps 5.8e-08 .. 6.4e-07): on CPU tensors the modulated convolution runs in the reference's
    weight-modulation form (op/cpu_tensors.py).  In the input-scaling form of the device kernels the float32 latent
    gradient is a hundred times further from float64, and one map element whose gradients nearly cancel in Adam's ratio
    then left the bound (6.9e-06 against 2.5e-06)."""
    G = pc.fixture_generator(sg2)
    inp = pb.loop_inputs()
    percept = pb.standin_percept(inp["mask"])
    stats = (inp["latent_mean"], torch.tensor(pb.LATENT_STD))
    missed = []
    for steps_run in range(1, pb.LOOP_STEPS + 1):
        # the state after step k of a 3-step schedule: run the first k steps of it (the schedule depends on the total)
        res = _first_steps(G, percept, inp["target"], stats, steps_run)
        s = steps_run - 1
        pairs = [(f"step{s}.latent", res["latent"])] + [(f"step{s}.noise{k}", n) for k, n in enumerate(res["noise"])]
        for key, a in pairs:
            ref = torch.from_numpy(fx[f"loop.{key}"])
            assert a.shape == ref.shape, key
            e, allowed = pc.l2_rel(a, ref), MARGIN * float(fx[f"loop.ref_fp32_err.{key}"])
            print(f"[project_batch CPU, B 2] {key}: {e:.2e} / {allowed:.2e}")
            if not e <= allowed:
                missed.append((key, e, allowed))
    assert res["img"].shape == (2, 3, 16, 16) and res["history"] == []
    assert not missed, missed


def _first_steps(G, percept, target, stats, k):
    """project_batch's state after the first k steps of the LOOP_STEPS-step run: get_lr and the jitter strength take
    t = i / LOOP_STEPS, so the total stays LOOP_STEPS and the loop is cut short after step k."""
    class Stop(Exception):
        pass
    done = []
    orig = projector.noise_normalize_

    def normalize_and_count(noises):
        orig(noises)
        done.append([n.detach().clone() for n in noises])
        if len(done) == k:
            raise Stop
    seen = {}
    adam = projector._adam

    def keep_params(params, lr):
        seen["params"] = params
        return adam(params, lr)
    projector.noise_normalize_, projector._adam = normalize_and_count, keep_params
    try:
        projector.project_batch(G, percept, target, steps=pb.LOOP_STEPS, latent_stats=stats, generator=pb.loop_generator(),
                                **pb.LOOP)
    except Stop:
        pass
    finally:
        projector.noise_normalize_, projector._adam = orig, adam
    if k < pb.LOOP_STEPS:
        return {"latent": seen["params"][0].detach().clone(), "noise": done[-1]}
    return projector.project_batch(G, percept, target, steps=pb.LOOP_STEPS, latent_stats=stats,
                                   generator=pb.loop_generator(), **pb.LOOP)


def test_project_batch_of_one_equals_project_on_cpu_tensors():
    """The same seeded generator: B = 1 draws what project draws and, on CPU tensors, computes what it computes."""
    from model_cases import fake_perceptual
    G = pc.fixture_generator(sg2)
    gen = torch.Generator().manual_seed(1)
    stats = projector.mean_latent_stats(G, n=256, generator=gen)
    target, _ = G([stats[0][None] + 0.5 * torch.randn(1, 32, generator=gen)], input_is_w=True)
    for w_plus in (False, True):
        one = projector.project(G, fake_perceptual, target, steps=3, w_plus=w_plus, mse=0.1, latent_stats=stats,
                                generator=torch.Generator().manual_seed(2))
        many = projector.project_batch(G, fake_perceptual, target, steps=3, w_plus=w_plus, mse=0.1, latent_stats=stats,
                                       generator=torch.Generator().manual_seed(2))
        assert many["latent"].shape == (1,) + tuple(one["latent"].shape)
        assert torch.equal(many["latent"][0], one["latent"]) and torch.equal(many["img"], one["img"])
        assert all(torch.equal(a, b) for a, b in zip(many["noise"], one["noise"]))
    with pytest.raises(ValueError):
        projector.project_batch(G, fake_perceptual, target[0], steps=1, latent_stats=stats)


def test_command_line_with_batch_projects_three_files_in_two_groups(tmp_path, monkeypatch):
    """--batch 2 over three small PNG files (a group of two and a group of one) on a size-16 random-weight checkpoint:
    three latents/<stem>.pt files that LatentDataset loads, each with [1, 1, s, s] maps, and the three preview images."""
    from PIL import Image
    root = tmp_path / "data"
    root.mkdir()
    torch.manual_seed(0)
    G = sg2.Generator(16, 512, 8, channel_multiplier=1)
    torch.save({"g_ema": G.state_dict()}, str(tmp_path / "g.pt"))
    rng = np.random.default_rng(0)
    names = ["a.png", "b.png", "c.png"]
    for name in names:
        Image.fromarray(rng.integers(0, 255, (20, 24, 3), dtype=np.uint8)).save(str(root / name))
    (root / "list.txt").write_text("".join(n + "\n" for n in names))
    monkeypatch.chdir(tmp_path)
    calls = []
    orig = projector.project_batch
    monkeypatch.setattr(projector, "project_batch", lambda G, p, images, **kw: calls.append(images.shape[0]) or orig(G, p, images, **kw))
    paths = projector.main(["--ckpt", str(tmp_path / "g.pt"), "--size", "16", "--channel_multiplier", "1", "--step", "2",
                            "--batch", "2", "--device", "cpu"] + [str(root / n) for n in names])
    assert calls == [2, 1]
    assert paths == [str(root / "latents" / (n[0] + ".pt")) for n in names]
    ds = dataset.LatentDataset(str(root))
    assert len(ds) == 3
    for i, name in enumerate(names):
        latent = ds[i]
        assert latent.shape == (512,) and bool(torch.isfinite(latent).all())
        stored = torch.load(paths[i], weights_only=True)[name]
        assert stored["img"].shape == (3, 16, 16)
        assert [tuple(n.shape) for n in stored["noise"]] == [(1, 1, s, s) for s in pb.SIDES]
        assert os.path.exists(tmp_path / (name[0] + "-project.png"))
    a, b = (torch.load(paths[i], weights_only=True)[names[i]] for i in (0, 1))
    assert not torch.equal(a["latent"], b["latent"]) and not torch.equal(a["noise"][0], b["noise"][0])


def test_batched_sample_on_cpu_tensors_equals_the_per_sample_loop():
    """CPU tensors take the layer loop either way: the same draws give the same w and images that agree to 2e-6 of max."""
    G = pc.fixture_generator(sg2)
    draws = generate.draw(G, 3, torch.Generator().manual_seed(9))
    img_b, w_b = generate.sample(G, 3, draws=draws, batched=True)
    img_s, w_s = generate.sample(G, 3, draws=draws)
    assert torch.equal(w_b, w_s) and img_b.shape == (3, 3, 16, 16)
    assert float((img_b - img_s).abs().max()) <= 2e-6 * float(img_s.abs().max())
    args = generate.build_parser().parse_args(["--ckpt", "x", "--size", "16", "--out", "y"])
    assert args.batched is False
    assert generate.build_parser().parse_args(["--ckpt", "x", "--size", "16", "--out", "y", "--batched"]).batched is True


def test_the_switch_is_off_by_default_and_restores_itself():
    assert synthesis.PER_SAMPLE is False
    with synthesis.per_sample_noise():
        assert synthesis.PER_SAMPLE is True
        with synthesis.per_sample_noise(False):
            assert synthesis.PER_SAMPLE is False
        assert synthesis.PER_SAMPLE is True
    assert synthesis.PER_SAMPLE is False
    with pytest.raises(RuntimeError):
        with synthesis.per_sample_noise():
            raise RuntimeError("x")
    assert synthesis.PER_SAMPLE is False
    # CPU tensors are never eligible, with or without it
    G = pc.fixture_generator(sg2)
    x0 = torch.zeros(2, 4, 4, 4)
    with synthesis.per_sample_noise():
        assert not synthesis.eligible(G, x0, [torch.zeros(2, 4)], [torch.zeros(2, 1, 4, 4)])


def test_ps_entries_refuse_bad_arguments_before_any_launch():
    """Host buffers stand in for device memory: every check precedes the first launch, so nothing is launched."""
    L = lib.load()
    d = (C.c_float * 64)()
    p = C.cast(d, C.c_void_p)
    for args in ((None, p, p, p, p, 1, 1, 16), (p, None, p, p, p, 1, 1, 16), (p, p, None, p, p, 1, 1, 16),
                 (p, p, p, p, None, 1, 1, 16), (p, p, p, p, p, 0, 1, 16), (p, p, p, p, p, 1, 0, 16), (p, p, p, p, p, 1, 1, 0),
                 (p, p, p, p, p, 256, 256, 16)):
        assert L.g2s_noise_bias_act_ps(*args, 0.2, 1.0, None) == -1, args
    assert L.g2s_upfirdn2d_nba_ps(p, p, p, 6, 4, 8, 8, 4, 4, 1, 1, 1, 1, 1, 1, p, p, p, 0.2, 1.0, None) == -1   # 6 % 4
    assert L.g2s_upfirdn2d_nba_ps(p, p, p, 8, 4, 8, 8, 4, 4, 1, 1, 1, 1, 1, 1, p, None, p, 0.2, 1.0, None) == -1
    rows = (p,) * 13
    assert L.g2s_synth_bwd_rows_ps(*rows, 6, 4, 16, 0.2, 1.0, None) == -1                                       # 6 % 4
    assert L.g2s_synth_bwd_rows_ps(*((p,) * 5 + (None,) + (p,) * 7), 8, 4, 16, 0.2, 1.0, None) == -1            # gdot, no map
