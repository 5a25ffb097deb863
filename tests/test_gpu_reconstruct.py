"""-m gpu: python -m gan2shape_amd.reconstruct end to end on the real model at its smallest configuration (the face
config of the existing fit tests: 128 x 128, generator of size 128, channel multiplier 1, two projected samples),
n_epochs_prior 2, --stages "2,2,2", two images — once eagerly and once with --graphs, one process each.

Everything a user would have lies in a temp dir: a random-weight StyleGAN2 checkpoint (`g_ema`, `d`), the config with
inline `view_mvn` / `light_mvn`, two images and their latents.  With --deterministic and --seed both runs must end on
identical parameters (the checkpoints of --save-ckpts, compared tensor by tensor) and identical report.json metrics, and
the report's figures must be what a direct `image_metrics` call gives on the reconstructions the command kept.
"""
import glob
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEMS = ["im_0", "im_1"]


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    import yaml
    from PIL import Image
    import bench
    import gan2shape_amd  # noqa: F401
    from gan2shape_amd.stylegan2 import Discriminator, Generator
    tmp = tmp_path_factory.mktemp("reconstruct")
    cfg = bench.face_config(n_proj=2)
    torch.manual_seed(21)
    G = Generator(cfg["gan_size"], cfg["z_dim"], 8, channel_multiplier=cfg["channel_multiplier"])
    D = Discriminator(cfg["gan_size"], channel_multiplier=cfg["channel_multiplier"])
    torch.save({"g_ema": G.state_dict(), "d": D.state_dict()}, tmp / "gan.pt")
    root = tmp / "data" / "face"
    os.makedirs(root / "latents")
    g = torch.Generator().manual_seed(22)
    for stem in STEMS:
        small = torch.randn(1, 3, 32, 32, generator=g)
        image = torch.tanh(torch.nn.functional.interpolate(small, scale_factor=4, mode="bilinear"))[0]
        Image.fromarray(((image + 1) * 127.5).round().to(torch.uint8).permute(1, 2, 0).numpy()).save(root / f"{stem}.png")
        torch.save(torch.randn(1, 512, generator=g), root / "latents" / f"{stem}.pt")
    (root / "list.txt").write_text("\n".join(s + ".png" for s in STEMS) + "\n")
    cfg.update(n_epochs_prior=2, root_path=str(tmp / "data"), gan_ckpt_path=str(tmp / "gan.pt"),
               our_nets_ckpts={"VLADE_nets": None})
    runs = {}
    for name, extra in (("eager", []), ("graphs", ["--graphs"])):
        cfg["our_nets_ckpts"]["VLADE_nets"] = str(tmp / f"ckpts_{name}")
        path = tmp / f"config_{name}.yml"
        path.write_text(yaml.safe_dump(cfg))
        argv = [sys.executable, "-m", "gan2shape_amd.reconstruct", "--config-file", str(path), "--stages", "2,2,2", "--seed", "5",
                "--deterministic", "--save-ckpts", "--out", str(tmp / f"out_{name}")] + extra
        env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
        t0 = time.perf_counter()
        done = subprocess.run(argv, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
        print(f"--- {name}: exit {done.returncode} after {time.perf_counter() - t0:.1f} s\n{done.stdout[-2000:]}\n{done.stderr[-3000:]}")
        assert done.returncode == 0, (name, done.stderr[-3000:])
        with open(tmp / f"out_{name}" / "report.json") as f:
            runs[name] = {"report": json.load(f), "out": tmp / f"out_{name}", "ckpts": tmp / f"ckpts_{name}" / "face"}
    return runs


def _checkpoints(folder):
    """{(net, image index): state dict} of the files --save-ckpts wrote (one per net and image)."""
    out = {}
    for path in sorted(glob.glob(os.path.join(folder, "*.pth"))):
        words = os.path.basename(path).split("_image_")
        ckpt = torch.load(path, map_location="cpu", weights_only=True)
        out[(words[0], int(words[1].split("_")[0]))] = ckpt
    return out


def test_report_and_files(workdir):
    for name, run in workdir.items():
        report = run["report"]
        assert list(report["images"]) == STEMS and report["total_it"] == 12 and report["graphs"] == (name == "graphs")
        assert report["stages"] == [{"step1": 2, "step2": 2, "step3": 2}]
        for i, stem in enumerate(STEMS):
            row = report["images"][stem]
            assert row["index"] == i and [h[1:3] for h in row["history"]] == [[0, 1], [0, 2], [0, 3]]
            assert all(np.isfinite(h[3]) for h in row["history"])
            d = np.load(run["out"] / "depth" / f"{stem}.npy")
            assert d.shape == (128, 128) and d.dtype == np.float32 and np.isfinite(d).all()
            assert os.path.exists(run["out"] / "recon" / f"{stem}.png")
            r = row["recon"]
            assert r["count"] == 128 * 128 and r["ssim_count"] == 118 * 118
            assert 0 < r["psnr"] < 60 and -1 <= r["ssim"] < 1 and r["mse"] > 0
        assert report["summary"]["images"] == 2 and report["summary"]["ssim_images"] == 2
        assert len(_checkpoints(run["ckpts"])) == 5 * 2


def test_eager_and_graphed_runs_end_on_the_same_bits(workdir):
    eager, graphed = workdir["eager"], workdir["graphs"]
    a, b = _checkpoints(eager["ckpts"]), _checkpoints(graphed["ckpts"])
    assert a.keys() == b.keys()
    for key in a:
        assert a[key]["total_it"] == b[key]["total_it"]
        sa, sb = a[key]["model_state_dict"], b[key]["model_state_dict"]
        assert sa.keys() == sb.keys() and all(torch.equal(sa[k], sb[k]) for k in sa), key
    for stem in STEMS:
        assert eager["report"]["images"][stem] == graphed["report"]["images"][stem]
        assert np.array_equal(np.load(eager["out"] / "depth" / f"{stem}.npy"), np.load(graphed["out"] / "depth" / f"{stem}.npy"))
    assert eager["report"]["summary"] == graphed["report"]["summary"]


def test_report_equals_a_direct_call_on_the_saved_reconstructions(workdir):
    """recon/<stem>.npy holds the float32 reconstructions the command scored; the dataset hands out the images it trained
    on: one image_metrics call on them gives the report's figures exactly (the kernel repeats bit for bit)."""
    import gan2shape_amd  # noqa: F401
    from gan2shape_amd.dataset import ImageDataset, default_transform
    from gan2shape_amd.metrics import IMAGE_KEYS, image_metrics
    for name, run in workdir.items():
        cfg = run["report"]["config"]
        data = ImageDataset(os.path.join(cfg["root_path"], "face"), transform=default_transform(cfg["image_size"]))
        images = torch.stack([data[i] for i in range(len(STEMS))]).cuda()
        recons = torch.stack([torch.from_numpy(np.load(run["out"] / "recon" / f"{s}.npy")) for s in STEMS]).cuda()
        assert recons.shape == images.shape == (2, 3, 128, 128)
        got = {k: v.cpu().numpy() for k, v in image_metrics(recons, images, data_range=2.0).items()}
        for i, stem in enumerate(STEMS):
            want = run["report"]["images"][stem]["recon"]
            print(name, stem, {k: (float(got[k][i]), want[k]) for k in IMAGE_KEYS})
            assert all(float(got[k][i]) == want[k] for k in IMAGE_KEYS)
