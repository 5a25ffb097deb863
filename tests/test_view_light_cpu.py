"""view_light on the CPU: mvn_fit's float64 route against the numpy oracle, the file format through
ViewLightSampler, estimate_view_light / fit_view_light on a toy model, and the fit_view_light command."""
import json
import os

import numpy as np
import pytest
import torch

import gan2shape_amd  # noqa: F401
import view_light_cases as vc
from gan2shape_amd import view_light
from gan2shape_amd.model import ViewLightSampler
from model_cases import toy_dataset


def _fit_arrays(fit):
    return {k: getattr(fit, k).numpy() for k in ("mean", "cov", "tril")}


def test_offset_case_tests_the_code_and_not_the_oracle():
    assert vc.offset_oracle_error() < 1e-6


@pytest.mark.parametrize("name,N,D,blocks,ld,ridge", vc.CASES, ids=vc.IDS)
def test_mvn_fit_cpu_route_against_the_oracle(name, N, D, blocks, ld, ridge):
    rows = vc.rows_of(name)[:, :D]
    fit = view_light.mvn_fit(torch.from_numpy(rows.copy()), blocks, ridge)
    assert fit.n == N and all(t.dtype == torch.float32 for t in fit[:3])
    vc.check_fit(_fit_arrays(fit), rows, blocks, ridge, name)
    vc.check_structure(fit.cov.numpy(), fit.tril.numpy(), blocks, name)


def test_mvn_fit_refusals_on_the_cpu():
    rows = torch.from_numpy(vc.rows_of("n255_d10").copy())
    with pytest.raises(ValueError, match="sum to D"):
        view_light.mvn_fit(rows, (6, 3))
    with pytest.raises(ValueError, match="sum to D"):
        view_light.mvn_fit(rows, (2, 2, 2, 2, 2))
    with pytest.raises(ValueError, match="N >= 2"):
        view_light.mvn_fit(rows[:1], (6, 4))
    with pytest.raises(ValueError, match="D <= 16"):
        view_light.mvn_fit(torch.zeros(5, 17))
    with pytest.raises(ValueError, match="float32"):
        view_light.mvn_fit(rows.double(), (6, 4))
    bad = rows.clone()
    bad[17, 3] = float("inf")
    with pytest.raises(ValueError, match="non-finite"):
        view_light.mvn_fit(bad, (6, 4))
    const = rows.clone()
    const[:, 7] = 0.25
    with pytest.raises(ValueError, match=r"column 7 \(column 1 of block 1"):
        view_light.mvn_fit(const, (6, 4))
    fit = view_light.mvn_fit(const, (6, 4), ridge=1e-6)
    assert fit.cov[7, 7].item() == pytest.approx(1e-6, rel=1e-6)


def test_saved_files_load_through_the_sampler(tmp_path):
    name, _N, D, blocks, _ld, ridge = vc.CASES[vc.IDS.index("n255_d10")]
    rows = vc.rows_of(name)
    fit = view_light.mvn_fit(torch.from_numpy(rows.copy()), blocks, ridge)
    vp, lp = str(tmp_path / "view_mvn.pth"), str(tmp_path / "light_mvn.pth")
    view_light.save_mvn(vp, *view_light.view_of(fit))
    view_light.save_mvn(lp, *view_light.light_of(fit))
    for path, dim in ((vp, 6), (lp, 4)):
        d = torch.load(path, map_location="cpu", weights_only=True)
        assert sorted(d) == ["cov", "mean"]
        assert d["mean"].dtype == torch.float32 and d["mean"].shape == (dim,) and d["mean"].device.type == "cpu"
        assert d["cov"].dtype == torch.float32 and d["cov"].shape == (dim, dim)
    sampler = ViewLightSampler(vp, lp, 1, "cpu")
    assert torch.equal(sampler.view_mean, fit.mean[:6]) and torch.equal(sampler.light_mean, fit.mean[6:])
    # the sampler factors the saved float32 covariance in float32; the fit's factor is the float64 one rounded.  Their
    # distance is held to the bound of view_light_cases on tril (the float32 composition's own error on these rows)
    bound = vc.bounds(rows, blocks, ridge)["tril"]
    for dist, sl in ((sampler.view_dist, slice(0, 6)), (sampler.light_dist, slice(6, 10))):
        err = float((dist._unbroadcasted_scale_tril.double() - fit.tril[sl, sl].double()).abs().max())
        print(f"sampler tril vs fit tril, block {sl}: {err:.3e}, bound {bound:.3e}")
        assert err <= bound
    assert sampler.sample(3, "view").shape == (3, 6) and sampler.sample(2, "light").shape == (2, 4)


def test_estimates_and_fit_on_a_toy_model():
    model = vc.toy_view_light_model(8)
    data = toy_dataset(5)                       # (image [3, 8, 8], latent, index) items
    x = torch.stack([item[0] for item in data[:3]])
    view, light = model.estimate_view_light(x)
    assert view.shape == (3, 6) and light.shape == (3, 4) and not view.requires_grad
    with torch.no_grad():
        assert torch.equal(view, model.viewpoint_net(x) + model.view_light_sampler.view_mean)
        assert torch.equal(light, model.lighting_net(x) + model.view_light_sampler.light_mean)
    singles = [model.estimate_view_light(x[i:i + 1]) for i in range(3)]
    tol = vc.batching_bound(model, torch.stack([item[0] for item in data]))
    assert torch.allclose(view, torch.cat([s[0] for s in singles]), rtol=0, atol=tol)
    assert torch.allclose(light, torch.cat([s[1] for s in singles]), rtol=0, atol=tol)

    fit, rows = view_light.fit_view_light(model, data, batch=2, ridge=1e-4)     # 5 images: batches 2, 2, 1
    per_image = torch.cat([torch.cat(model.estimate_view_light(item[0][None]), 1) for item in data])
    assert rows.shape == (5, 10) and torch.allclose(rows, per_image, rtol=0, atol=tol)
    vc.check_fit(_fit_arrays(fit), rows.numpy(), (6, 4), 1e-4, "toy model")
    _, picked = view_light.fit_view_light(model, data, batch=2, images=[4, 0, 2], ridge=1e-4)
    assert torch.allclose(picked, per_image[[4, 0, 2]], rtol=0, atol=tol)
    with pytest.raises(ValueError, match="at least 2"):
        view_light.fit_view_light(model, data, images=[1])


def _write_dataset(tmp_path, n, size=16):
    from PIL import Image
    rng = np.random.default_rng(3)
    root = tmp_path / "data" / "face"
    root.mkdir(parents=True)
    names = [f"im_{i}.png" for i in range(n)]
    for name in names:
        Image.fromarray(rng.integers(0, 256, (size, size, 3), dtype=np.uint8)).save(root / name)
    (root / "list.txt").write_text("\n".join(names) + "\n")
    cfg = tmp_path / "cfg.yml"
    cfg.write_text(f"category: face\nroot_path: {tmp_path / 'data'}\nimage_size: {size}\n")
    return cfg


def test_command_writes_the_four_files(tmp_path, capsys):
    from gan2shape_amd import fit_view_light as cmd
    from gan2shape_amd.dataset import ImageDataset, default_transform
    cfg = _write_dataset(tmp_path, 14)
    model = vc.toy_view_light_model(16)
    out = tmp_path / "out"
    argv = ["--config", str(cfg), "--ckpt", "unused", "--out", str(out), "--device", "cpu", "--batch", "4"]
    picks = [0, 2, 3, 4, 5, 7, 8, 9, 10, 11, 13, 12]            # 12 rows: enough for a 6 x 6 covariance of full rank
    assert cmd.main(argv + ["--images"] + [str(i) for i in picks], model=model) == 0
    assert sorted(os.listdir(out)) == ["estimates.npy", "light_mvn.pth", "view_light.json", "view_mvn.pth"]
    est = np.load(out / "estimates.npy")
    assert est.shape == (12, 10) and est.dtype == np.float32
    data = ImageDataset(str(tmp_path / "data" / "face"), transform=default_transform(16, None, None))
    want = torch.cat([torch.cat(model.estimate_view_light(data[i][None]), 1) for i in picks]).numpy()
    assert np.allclose(est, want, rtol=0, atol=vc.batching_bound(model, torch.stack([data[i] for i in picks])))
    report = json.loads((out / "view_light.json").read_text())
    assert set(report) == {"n", "ridge", "stems", "view_mean", "light_mean", "view_min_eig", "light_min_eig"}
    assert report["n"] == 12 and report["ridge"] == 0 and report["stems"] == [f"im_{i}" for i in picks]
    assert report["view_min_eig"] > 0 and report["light_min_eig"] > 0
    sampler = ViewLightSampler(str(out / "view_mvn.pth"), str(out / "light_mvn.pth"), 1, "cpu")
    assert np.allclose(sampler.view_mean.numpy(), est[:, :6].astype(np.float64).mean(0), rtol=0, atol=vc.EPS32)
    assert report["view_mean"] == [float(v) for v in sampler.view_mean]
    ref = vc.oracle(est, (6, 4))
    for name, sl in (("view", slice(0, 6)), ("light", slice(6, 10))):       # the files hold the blocks of the joint fit
        cov = torch.load(out / f"{name}_mvn.pth", weights_only=True)["cov"].numpy()
        assert np.abs(cov - ref["cov"][sl, sl]).max() <= 4 * vc.EPS32 * np.abs(ref["cov"]).max()


def test_command_refusals_leave_nothing(tmp_path):
    from gan2shape_amd import fit_view_light as cmd
    cfg = _write_dataset(tmp_path, 14)
    model = vc.toy_view_light_model(16)
    out = tmp_path / "out"
    base = ["--config", str(cfg), "--out", str(out), "--device", "cpu"]
    said = []
    assert cmd.main(base + ["--ckpt", "unused", "--images", "3"], model=model, log=said.append) != 0
    assert "at least 2 images" in said[-1]
    assert cmd.main(base + ["--ckpt", "a", "--ckpt", "b", "--images", "0", "1", "2"], model=model, log=said.append) != 0
    assert "2 --ckpt for 3 images" in said[-1]
    with torch.no_grad():                           # view component 4 no longer depends on the image: variance 0
        model.viewpoint_net.lin.weight[4].zero_()
        model.viewpoint_net.lin.bias[4].zero_()
    assert cmd.main(base + ["--ckpt", "unused"], model=model, log=said.append) != 0
    assert "column 4" in said[-1] and "--ridge" in said[-1]
    assert not out.exists()
    assert cmd.main(base + ["--ckpt", "unused", "--ridge", "1e-6"], model=model, log=said.append) == 0
    cov = torch.load(out / "view_mvn.pth", weights_only=True)["cov"]
    assert cov[4, 4].item() == pytest.approx(1e-6, rel=1e-6)
    est = np.load(out / "estimates.npy")
    ref = np.cov(est.astype(np.float64), rowvar=False)
    assert np.allclose(np.diag(cov.numpy()), np.diag(ref)[:6] + 1e-6, rtol=4 * vc.EPS32, atol=0)
    with pytest.raises(SystemExit):
        cmd.main(["--config", str(cfg)])            # --ckpt and --out are required
