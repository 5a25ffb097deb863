"""python -m gan2shape_amd.reconstruct on the CPU with the toy models, toy configs and the toy image dataset of
model_cases.py: the config merge, the schedule, the files and report of --out, that the command runs exactly the fit a
caller of `Trainer.fit` / `GeneralizingTrainer2.fit` runs, that the new `on_image_done` hook changes nothing when absent,
and `evaluate --recon-metrics`.
"""
import json
import os

import numpy as np
import pytest
import torch

import model_cases as mc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_configs")


@pytest.fixture(scope="module")
def pkg():
    import gan2shape_amd  # noqa: F401
    from gan2shape_amd import config, evaluate, reconstruct, trainer
    return {"config": config, "evaluate": evaluate, "reconstruct": reconstruct, "trainer": trainer}


def _with_results(base):
    class Model(base):
        """The toy nets plus what the --out callback and `evaluate` ask of a model: a reconstruction and a depth that
        depend on the image and on the trained parameters."""
        made = []

        def __init__(self, config, debug=False, device="cpu"):
            super().__init__(config, debug, device)
            self.device = torch.device(device)
            self.evaluated = []       # (reconstruction, depth) of every evaluate_results call
            type(self).made.append(self)

        def evaluate_results(self, image):
            with torch.no_grad():
                f = self._feat(image)
                gain = 0.8 + 0.1 * torch.tanh(self.albedo_net(f)[:, :1]).view(-1, 1, 1, 1)
                recon = (image * gain + 0.05 * torch.tanh(self.lighting_net(f)[:, :1]).view(-1, 1, 1, 1)).clamp(-1, 1)
                depth = 1.0 + 0.05 * torch.tanh(self.depth_net(f)[:, :1]).view(-1, 1, 1) * image[:, 0]
            self.evaluated.append((recon, depth))
            return recon, depth
    return Model


def _setup(tmp_path, cfg, **extra):
    """The toy image dataset under <tmp>/data/face and a one-file config; crop 8 makes the three aspect ratios 8 x 8."""
    root = tmp_path / "data" / "face"
    root.parent.mkdir()
    mc.write_toy_image_dataset(str(root))
    config = dict(cfg, root_path=str(tmp_path / "data"), crop=8, batch_size=2, **extra)
    path = tmp_path / "config.yml"
    import yaml
    path.write_text(yaml.safe_dump(config))
    return str(path), config


def _params(model):
    return {k: v.clone() for k, v in model.state_dict().items()}


def _same(a, b):
    return a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)


# ------------------------------------------------------------------------------------------- config
def test_load_config_merges_minimal_and_category(pkg):
    load_config = pkg["config"].load_config
    import yaml
    with open(os.path.join(GOLDEN, "minimal_config.yml")) as f:
        minimal = yaml.safe_load(f)
    with open(os.path.join(GOLDEN, "configs", "car.yml")) as f:
        car = yaml.safe_load(f)
    merged = load_config(category="car", config_dir=GOLDEN)
    assert merged == {**minimal, **car, "category": "car"}
    assert merged["gan_size"] == 512 and merged["image_size"] == 128 and merged["n_epochs_prior"] == 1000
    face = load_config(category="face", config_dir=GOLDEN)
    assert face["gan_size"] == 128 and face["n_proj_samples"] == 16 and face["category"] == "face"
    one = load_config(os.path.join(GOLDEN, "configs", "car.yml"))
    assert one == car and "category" not in one


def test_load_config_second_file_wins_and_missing_files_are_named(pkg, tmp_path):
    load_config = pkg["config"].load_config
    (tmp_path / "configs").mkdir()
    (tmp_path / "minimal_config.yml").write_text("image_size: 128\nprior_name: box\ncategory: wrong\n")
    (tmp_path / "configs" / "cat.yml").write_text("image_size: 64\ngan_size: 256\n")
    assert load_config(category="cat", config_dir=str(tmp_path)) == {"image_size": 64, "prior_name": "box", "gan_size": 256,
                                                                     "category": "cat"}
    with pytest.raises(FileNotFoundError, match="dog.yml"):
        load_config(category="dog", config_dir=str(tmp_path))
    with pytest.raises(FileNotFoundError, match="minimal_config.yml"):
        load_config(category="cat", config_dir=str(tmp_path / "configs"))
    with pytest.raises(FileNotFoundError, match="nowhere.yml"):
        load_config(str(tmp_path / "nowhere.yml"))


# ------------------------------------------------------------------------------------------- stages
def test_stages_parsing_and_defaults(pkg):
    r = pkg["reconstruct"]
    assert r.parse_stages("700,700,600;200,500,400") == [{'step1': 700, 'step2': 700, 'step3': 600},
                                                         {'step1': 200, 'step2': 500, 'step3': 400}]
    assert r.parse_stages(" 2, 1 ,2 ") == [{'step1': 2, 'step2': 1, 'step3': 2}]
    with pytest.raises(ValueError, match="'5x'"):
        r.parse_stages("2,1,2;1,5x,1")
    with pytest.raises(ValueError, match="stage 2.*2 fields"):
        r.parse_stages("2,1,2;1,3")
    with pytest.raises(ValueError, match="'-1'"):
        r.parse_stages("2,-1,2")
    assert r.default_stages(False) == [{'step1': 700, 'step2': 700, 'step3': 600}] + [{'step1': 200, 'step2': 500, 'step3': 400}] * 3
    assert r.default_stages(True) == [{'step1': 13, 'step2': 22, 'step3': 18}]
    a = r.build_parser().parse_args(["--images", "0", "3", "--images", "7"])
    assert a.images == [[0, 3], [7]] and a.config_file == "config.yml" and a.device == "cuda" and not a.graphs


def test_malformed_stages_and_graphs_on_the_cpu_are_refused(pkg, tmp_path, capsys):
    r = pkg["reconstruct"]
    cfg, _ = _setup(tmp_path, mc.TOY_CFG)
    out = tmp_path / "out"
    Model = _with_results(mc.ToyStepModel)
    with pytest.raises(SystemExit):
        r.main(["--config-file", cfg, "--device", "cpu", "--stages", "2,x,2", "--out", str(out)], model=Model)
    assert "'x'" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        r.main(["--config-file", cfg, "--device", "cpu", "--graphs", "--stages", "1,1,1", "--out", str(out)], model=Model)
    assert "--graphs" in capsys.readouterr().err
    assert not out.exists() and not Model.made


# ------------------------------------------------------------------------------------------- report
def test_out_directory_and_report(pkg, tmp_path, capsys):
    r = pkg["reconstruct"]
    cfg, config = _setup(tmp_path, mc.TOY_CFG)
    out = tmp_path / "out"
    Model = _with_results(mc.ToyStepModel)
    report = r.main(["--config-file", cfg, "--device", "cpu", "--seed", "3", "--images", "0", "2", "--stages", "2,1,2;1,3,1",
                     "--out", str(out)], model=Model)
    printed = capsys.readouterr().out
    assert ">>> Warning, not saving checkpoints." in printed and "using a subset" not in printed
    stems = ["img_0", "img_2"]
    assert sorted(os.listdir(out / "depth")) == [s + ".npy" for s in stems]
    assert sorted(os.listdir(out / "recon")) == sorted(s + ext for s in stems for ext in (".png", ".npy"))
    written = json.loads((out / "report.json").read_text())
    assert written == json.loads(json.dumps(report))
    assert list(written["images"]) == stems and written["total_it"] == (2 + 1 + 2 + 1 + 3 + 1) * 2
    assert written["stages"] == [{'step1': 2, 'step2': 1, 'step3': 2}, {'step1': 1, 'step2': 3, 'step3': 1}]
    assert written["config"] == config
    (model,) = Model.made
    from PIL import Image
    from gan2shape_amd.dataset import ImageLatentDataset, default_transform
    from gan2shape_amd.metrics import image_metrics
    data = ImageLatentDataset(os.path.join(config["root_path"], "face"), subset=[0, 2], transform=default_transform(8, 8))
    for i, stem in enumerate(stems):
        row = written["images"][stem]
        assert row["index"] == i and len(row["history"]) == 6 and all(h[0] == i and h[3] is not None for h in row["history"])
        image = data[i][0][None]
        recon, depth = model.evaluated[i]      # as the nets stood after this image's last stage
        d = np.load(out / "depth" / f"{stem}.npy")
        assert d.dtype == np.float32 and d.shape == (8, 8) and np.array_equal(d, depth[0].numpy())
        png = np.asarray(Image.open(out / "recon" / f"{stem}.png"))
        assert png.shape == (8, 8, 3) and np.abs(png / 127.5 - 1 - recon[0].permute(1, 2, 0).numpy()).max() <= 0.5 / 127.5 + 1e-6
        assert np.array_equal(np.load(out / "recon" / f"{stem}.npy"), recon[0].numpy())
        want = image_metrics(recon, image, data_range=2.0)
        assert row["recon"]["ssim"] is None and row["recon"]["ssim_count"] == 0 and row["recon"]["count"] == 64
        for k in ("mae", "mse", "psnr"):
            assert row["recon"][k] == float(want[k][0]) and np.isfinite(row["recon"][k])
    assert len(model.evaluated) == 2
    last = model.evaluate_results(data[1][0][None])      # the nets as the fit left them: the last image's result
    assert torch.equal(last[0], model.evaluated[1][0]) and torch.equal(last[1], model.evaluated[1][1])
    s = written["summary"]
    assert s["images"] == 2 and s["ssim_images"] == 0 and s["ssim"] == [None, None]
    assert s["psnr"][0] == pytest.approx(np.mean([written["images"][k]["recon"]["psnr"] for k in stems]))


def test_without_out_only_training_happens(pkg, tmp_path):
    r = pkg["reconstruct"]
    cfg, _ = _setup(tmp_path, mc.TOY_CFG)
    before = set(os.listdir(tmp_path))
    Model = _with_results(mc.ToyStepModel)
    assert r.main(["--config-file", cfg, "--device", "cpu", "--images", "0", "--stages", "1,1,1"], model=Model) == {"total_it": 3}
    assert set(os.listdir(tmp_path)) == before


# ------------------------------------------------------------------------------------------- trainer equivalence
@pytest.mark.parametrize("generalize", [False, True], ids=["instance", "generalize"])
def test_the_command_runs_the_fit_a_caller_runs(pkg, tmp_path, generalize, capsys):
    r, t = pkg["reconstruct"], pkg["trainer"]
    base, toy_cfg = (mc.ToyJointModel, mc.TOY_JOINT_CFG) if generalize else (mc.ToyStepModel, mc.TOY_CFG)
    cfg, config = _setup(tmp_path, toy_cfg)
    from gan2shape_amd.dataset import ImageLatentDataset, default_transform
    data = ImageLatentDataset(os.path.join(config["root_path"], "face"), subset=[0, 2], transform=default_transform(8, 8))
    stages = [{'step1': 2, 'step2': 1, 'step3': 2}, {'step1': 1, 'step2': 3, 'step3': 1}]
    Direct = _with_results(base)
    torch.manual_seed(3)
    direct = (t.GeneralizingTrainer2 if generalize else t.Trainer)(Direct, dict(config), device="cpu")
    total = direct.fit(data, stages=stages, batch_size=2)
    state = torch.get_rng_state()

    Model = _with_results(base)
    argv = ["--config-file", cfg, "--device", "cpu", "--seed", "3", "--images", "0", "--images", "2", "--stages", "2,1,2;1,3,1",
            "--out", str(tmp_path / "out")] + (["--generalize"] if generalize else [])
    report = r.main(argv, model=Model)
    printed = capsys.readouterr().out
    assert ("using a subset with a generalizing trainer" in printed) == generalize
    assert report["total_it"] == total and len(report["images"]) == 2
    assert _same(_params(direct.model), _params(Model.made[0]))
    assert torch.equal(state, torch.get_rng_state())
    assert Model.made[0].log == Direct.made[0].log
    if generalize:      # rows of a batch (step 1) and of the image (steps 2, 3), both epochs
        assert [h[2] for h in report["images"]["img_2"]["history"]] == [1, 2, 3] * toy_cfg["n_epochs_generalized"]


@pytest.mark.parametrize("generalize", [False, True], ids=["instance", "generalize"])
def test_no_callback_is_the_parent_s_fit(pkg, generalize):
    t = pkg["trainer"]
    cls, base, cfg, stages = ((t.GeneralizingTrainer2, mc.ToyJointModel, mc.TOY_JOINT_CFG, mc.TOY_JOINT_STAGES) if generalize
                              else (t.Trainer, mc.ToyStepModel, mc.TOY_CFG, mc.TOY_STAGES))
    runs = []
    for kwargs in ({}, {"on_image_done": None}, {"on_image_done": lambda index, image, trainer: seen.append((index, image.shape))}):
        seen = []
        torch.manual_seed(11)
        trainer = cls(base, dict(cfg), device="cpu")
        total = trainer.fit(mc.toy_dataset(), stages=stages, shuffle=True, **kwargs)      # shuffle: the loaders draw
        runs.append((total, _params(trainer.model), torch.get_rng_state(), trainer.model.log, trainer.history, seen))
    for other in runs[1:]:
        assert other[0] == runs[0][0] and _same(other[1], runs[0][1]) and torch.equal(other[2], runs[0][2])
        assert other[3] == runs[0][3] and other[4] == runs[0][4]
    assert runs[0][5] == [] and runs[1][5] == []
    assert sorted(runs[2][5]) == [(0, (1, 3, 8, 8)), (1, (1, 3, 8, 8))]       # once per image


# ------------------------------------------------------------------------------------------- evaluate
def test_evaluate_recon_metrics_adds_and_changes_nothing_else(pkg, tmp_path, capsys):
    evaluate = pkg["evaluate"]
    cfg, config = _setup(tmp_path, mc.TOY_CFG)
    model = _with_results(mc.ToyStepModel)(config)
    argv = ["--config", cfg, "--ckpt", "unused", "--device", "cpu", "--images", "0", "2", "--record-loss", "toy"]
    model.forward_step1 = lambda image, latent, collected, step1=True, eval=False: (image.mean() + 2.0, None)
    plain = evaluate.main(argv + ["--out", str(tmp_path / "plain")], model=model)
    plain_log = capsys.readouterr().out
    assert plain == {"images": {"img_0": {}, "img_2": {}}, "step1_loss": plain["step1_loss"]}
    assert "recon" not in (tmp_path / "plain" / "metrics.json").read_text() and "reconstructions" not in plain_log
    assert plain_log.splitlines()[0].startswith("mean = ") and len(plain_log.splitlines()) == 2

    scored = evaluate.main(argv + ["--out", str(tmp_path / "scored"), "--recon-metrics"], model=model)
    scored_log = capsys.readouterr().out
    assert json.loads((tmp_path / "scored" / "metrics.json").read_text()) == json.loads(json.dumps(scored))
    summary = scored.pop("recon_summary")
    rows = {stem: v.pop("recon") for stem, v in scored["images"].items()}
    assert scored == plain
    assert [line for line in scored_log.splitlines() if line in plain_log.splitlines()] == plain_log.splitlines()
    assert "2 reconstructions scored" in scored_log and "psnr" in scored_log
    for stem in ("img_0", "img_2"):
        assert np.array_equal(np.load(tmp_path / "plain" / "depth" / f"{stem}.npy"), np.load(tmp_path / "scored" / "depth" / f"{stem}.npy"))
        assert set(rows[stem]) == {"count", "mae", "mse", "psnr", "ssim_count", "ssim"}       # no perceptual module, no lpips
        assert rows[stem]["count"] == 64 and rows[stem]["ssim"] is None and rows[stem]["psnr"] > 0
    assert summary["images"] == 2 and summary["psnr"][0] == pytest.approx(np.mean([rows[s]["psnr"] for s in rows]))

    # a model with the perceptual module of step 1 also records it; a mask restricts the count
    model.perceptual_loss = mc.fake_perceptual

    class Mask():
        def image_mask(self, image, depth):
            d = depth[:, None].clone()
            d[..., :3] = float("nan")
            return d
    model.evaluate_results_masked = lambda image, masking_model: (lambda r, d: (r, masking_model.image_mask(image, d)))(
        *model.evaluate_results(image))
    masked = evaluate.main(argv[:-2] + ["--out", str(tmp_path / "masked"), "--recon-metrics", "--mask"], model=model,
                           masking_model=Mask())
    for stem in ("img_0", "img_2"):
        row = masked["images"][stem]["recon"]
        assert row["count"] == 8 * 5 and row["lpips"] > 0
