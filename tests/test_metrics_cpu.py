"""Depth metrics without a GPU: the float64 oracle's own checks, the CPU (torch) path of
gan2shape_amd.metrics.depth_metrics against it on every case of metrics_cases.py, DepthMetrics, the C ABI's
declarations and argument checks (which precede any launch), and gan2shape_amd.evaluate end to end.

evaluate runs here on a stub model: GAN2Shape.forward_step1 rasterises through the libg2s plugin, which rejects
CPU tensors, so the real model cannot evaluate on this route.  The stub stands in for evaluate_results,
evaluate_results_masked and forward_step1; the command line, the dataset, the files written and the scoring
are the real ones.
"""
import json
import math
import os

import numpy as np
import pytest
import torch

import metrics_cases as mc


@pytest.fixture(scope="module")
def metrics():
    import gan2shape_amd  # noqa: F401
    from gan2shape_amd import metrics
    return metrics


def _oracle_of(c, **over):
    a = dict(c, **over)
    return mc.metrics64(a["pred"], a["gt"], a["mask_pred"], a["mask_gt"], a["rays"], a["erode"])


# ------------------------------------------------------------------------------------------- the oracle itself
def test_oracle_side_is_invariant_under_a_scale_of_the_prediction():
    for name in ("33x33", "8x8_raw"):
        c = mc.CASES[name]
        want = mc.oracle(name)
        got = _oracle_of(c, pred=c["pred"].astype(np.float64) * 1.37)
        np.testing.assert_array_equal(got["count"], want["count"])
        np.testing.assert_allclose(got["side"], want["side"], rtol=1e-10, atol=1e-14)
        assert not np.allclose(got["mae"], want["mae"], rtol=1e-3, equal_nan=True)


def test_oracle_mad_is_invariant_under_a_joint_scale():
    for name in ("33x33", "128x128"):
        c = mc.CASES[name]
        want = mc.oracle(name)
        got = _oracle_of(c, pred=c["pred"].astype(np.float64) * 0.83, gt=c["gt"].astype(np.float64) * 0.83)
        np.testing.assert_allclose(got["mad"], want["mad"], rtol=1e-9)
        np.testing.assert_allclose(got["side"], want["side"], rtol=1e-9, atol=1e-14)


@pytest.mark.parametrize("name", ["8x8_erode", "8x8_raw", "5x9", "5x9_raw"])
def test_oracle_agrees_with_the_per_pixel_loop(name):
    c = mc.CASES[name]
    want = mc.metrics64_loops(c["pred"], c["gt"], c["mask_pred"], c["mask_gt"], c["rays"], c["erode"])
    got = mc.oracle(name)
    for k in mc.KEYS:
        np.testing.assert_allclose(got[k], want[k], rtol=1e-11, atol=1e-15, err_msg=f"{name} {k}")


def test_cases_are_what_they_claim():
    o = mc.oracle
    assert o("3x3")["count"].tolist() == [1.0] and o("3x3")["side"][0] == 0.0 and o("3x3")["mad"][0] > 0
    assert o("8x8_erode")["count"].tolist() == [36.0] and o("8x8_raw")["count"].tolist() == [64.0]
    many = o("16x16x17")
    assert many["count"][3] == 0 and many["count"][5] == 0 and (many["count"] > 0).sum() == 15
    assert all(np.isnan(many[k][[3, 5]]).all() and not np.isnan(np.delete(many[k], [3, 5])).any() for k in mc.METRICS)
    assert all((o("p_eq_g")[k] == 0).all() for k in mc.METRICS)
    s = o("p_scaled")
    assert s["side"][0] < 1e-6 and abs(s["mae"][0] - 0.07 * mc.CASES["p_scaled"]["gt"][0, 1:-1, 1:-1].mean(dtype=np.float64)) < 1e-6
    raw, eroded = o("33x33_raw"), o("33x33")
    assert (raw["count"] > eroded["count"]).all() and (eroded["count"] > 50).all()
    assert (o("128x128")["count"] > 3000).all()
    # the real Renderer hands out the rays the cases were built with
    from gan2shape_amd.renderer.renderer import Renderer
    for H, W, S in ((33, 33, 33), (5, 9, 9), (128, 128, 128)):
        r = Renderer({"fov": 10}, S, 0.9, 1.1, device="cpu")._pixel_rays(H, W, torch.device("cpu"))[0].numpy()
        np.testing.assert_allclose(r, mc.pixel_rays(H, W), rtol=1e-5, atol=1e-7)


def test_the_bound_catches_a_dropped_erosion_ring_and_naive_fp32_moments():
    """What the bound is for.  (a) Scoring the un-eroded mask instead of the eroded one misses it on every metric's
    own scale.  (b) SIDE from fp32 E[d^2] - E[d]^2 misses it where p = 1.07 g."""
    e = mc.error_figures(dict(mc.oracle("33x33_raw"), count=mc.oracle("33x33")["count"]), mc.oracle("33x33"))
    print("un-eroded against eroded:", e)
    assert all(e[k] > mc.BOUND[k] for k in mc.METRICS)
    c = mc.CASES["p_scaled"]
    delta = np.log(c["pred"][0]) - np.log(c["gt"][0])
    assert delta.dtype == np.float32
    m = np.ones_like(delta, bool)
    m[0, :] = m[-1, :] = m[:, 0] = m[:, -1] = False
    d = delta[m]
    n = np.float32(d.size)
    var = (d * d).sum(dtype=np.float32) / n - (d.sum(dtype=np.float32) / n) ** 2
    naive = math.sqrt(max(0.0, float(var)))
    want = mc.oracle("p_scaled")["side"][0]
    e_side = abs(naive - want) / (mc.A["side"] + abs(want))
    print(f"naive fp32 SIDE {naive:.3e}, oracle {want:.3e}, e_side {e_side:.3e}, bound {mc.BOUND['side']:.3e}")
    assert e_side > mc.BOUND["side"]


# ------------------------------------------------------------------------------------------- the CPU path
@pytest.mark.parametrize("name", list(mc.CASES))
def test_cpu_path_matches_the_oracle(name, metrics):
    got = mc.run_case(metrics.depth_metrics, name)
    mc.check(got, mc.oracle(name), f"{name} torch fp32 on the CPU")
    if name == "3x3":
        assert got["side"][0] == 0.0
    if name == "p_eq_g":
        assert all((got[k] == 0).all() for k in ("mae", "mse", "side"))


def test_cpu_path_interface(metrics):
    c = mc.CASES["33x33"]
    r = mc.CaseRenderer()
    p, g, mp, mg = (torch.from_numpy(c[k]) for k in ("pred", "gt", "mask_pred", "mask_gt"))
    base = metrics.depth_metrics(p, g, mp, mg, renderer=r)
    assert set(base) == set(mc.KEYS)
    assert all(v.shape == (3,) and v.dtype == torch.float32 for v in base.values())
    wide = torch.stack([p, p], -1)[..., 0]                     # non-contiguous view
    assert not wide.is_contiguous()
    other = metrics.depth_metrics(wide, g, mp[:, None], mg[:, None].bool(), renderer=r, erode=True)
    for k in mc.KEYS:
        np.testing.assert_array_equal(base[k].numpy(), other[k].numpy())
    with pytest.raises(ValueError):
        metrics.depth_metrics(p, g[:, :-1], renderer=r)
    with pytest.raises(ValueError):
        metrics.depth_metrics(p, g, mp[:, :5], renderer=r)
    gm = metrics.gt_mask_from_depth(g)
    assert gm.dtype == torch.float32 and gm.shape == g.shape
    assert torch.equal(gm, (g < g.amax((1, 2), keepdim=True)).float()) and int((gm == 0).sum()) >= 3


def test_depth_metrics_summary(metrics):
    acc = metrics.DepthMetrics()
    many = {k: torch.from_numpy(v).float() for k, v in mc.oracle("16x16x17").items()}
    acc.update(many)
    acc.update(mc.oracle("33x33"))                                   # arrays work too; batches accumulate
    assert len(acc) == 20
    s = acc.summary()
    assert s["skipped"] == 2 and s["images"] == 18
    for k in mc.METRICS:
        v = np.concatenate([many[k].numpy().astype(np.float64), mc.oracle("33x33")[k]])
        v = v[~np.isnan(v)]
        assert len(v) == 18
        assert s[k] == (pytest.approx(np.mean(v), rel=1e-14), pytest.approx(np.std(v), rel=1e-12))
    empty = metrics.DepthMetrics().summary()
    assert empty["images"] == 0 and math.isnan(empty["mae"][0])


# ------------------------------------------------------------------------------------------- C ABI
def test_symbols_are_declared_and_exported():
    import gan2shape_amd  # noqa: F401
    from gan2shape_amd import lib
    assert {"g2s_depth_metrics", "g2s_depth_metrics_workspace_bytes"} <= set(lib.SIGNATURES)
    L = lib.load()
    assert L.g2s_abi_version() == 1
    assert L.g2s_depth_metrics_workspace_bytes(0, 8, 8) == 0
    tiles = 4 * 16
    assert L.g2s_depth_metrics_workspace_bytes(2, 128, 128) == 2 * tiles * 7 * 8
    assert L.g2s_depth_metrics_workspace_bytes(1, 3, 3) == 7 * 8


def test_bad_arguments_are_rejected_before_any_launch():
    """Every check precedes the first launch, so it runs without a GPU (the pointers are never followed)."""
    import ctypes
    import gan2shape_amd  # noqa: F401
    from gan2shape_amd import lib
    L = lib.load()
    host = (ctypes.c_double * 4096)()
    ok = ctypes.c_void_p(ctypes.addressof(host))
    need = L.g2s_depth_metrics_workspace_bytes(2, 16, 16)

    def call(pred=ok, gt=ok, rays=ok, out=ok, B=2, H=16, W=16, ws=ok, n=need):
        return L.g2s_depth_metrics(pred, gt, None, None, rays, B, H, W, 1, out, ws, n, None)
    for kw, code in (({"pred": None}, -1), ({"gt": None}, -1), ({"rays": None}, -1), ({"out": None}, -1),
                     ({"B": 0}, -1), ({"B": -3}, -1), ({"B": 65536}, -1), ({"H": 2}, -1), ({"W": 2}, -1),
                     ({"ws": None}, -3), ({"n": need - 1}, -3), ({"n": 0}, -3)):
        rc = call(**kw)
        assert rc == code and b"g2s_depth_metrics" in L.g2s_last_error(), (kw, rc, L.g2s_last_error())
        with pytest.raises(lib.G2SError):
            lib.check(rc)


# ------------------------------------------------------------------------------------------- evaluate
class StubModel():
    """What evaluate needs of GAN2Shape: a depth from the image's first channel, a loss from its mean."""

    def __init__(self, size):
        self.device = torch.device("cpu")
        self.renderer = mc.CaseRenderer(size)
        self.calls = []

    def evaluate_results(self, image):
        assert image.shape[0] == 1, "one image at a time"
        self.calls.append("evaluate_results")
        return image, 1.0 + 0.05 * image[:, 0]

    def evaluate_results_masked(self, image, masking_model):
        recon, depth = self.evaluate_results(image)
        return recon, masking_model.image_mask(image, depth)

    def forward_step1(self, image, latent, collected, step1=True, eval=False):
        assert step1 and not eval
        return image.mean() + 2.0, None


class StubMask():
    def image_mask(self, image, depth):
        d = depth[:, None].clone()
        d[..., :4] = float("nan")
        return d


def _dataset(tmp_path, size=16):
    from PIL import Image
    rng = np.random.default_rng(0)
    root = tmp_path / "data" / "face"
    root.mkdir(parents=True)
    y, x = np.meshgrid(np.linspace(0, 1, size), np.linspace(0, 1, size), indexing="ij")
    names = ["a.png", "b.png"]
    for i, name in enumerate(names):
        img = np.stack([(x + i * y) / (1 + i), y, x * y], -1) * 200 + rng.integers(0, 20, (size, size, 3))
        Image.fromarray(img.astype(np.uint8)).save(root / name)
    (root / "list.txt").write_text("\n".join(names) + "\n")
    cfg = tmp_path / "cfg.yml"
    cfg.write_text(f"category: face\nroot_path: {tmp_path / 'data'}\nimage_size: {size}\n")
    gt = tmp_path / "gt"
    gt.mkdir()
    for name in names:
        np.save(gt / (name[:-4] + ".npy"), mc.smooth_depth(rng, 1, size, size)[0])
    return cfg, gt


def test_evaluate_end_to_end_on_the_cpu(tmp_path, metrics, capsys):
    from gan2shape_amd import evaluate
    cfg, gt = _dataset(tmp_path)
    out = tmp_path / "out"
    model = StubModel(16)
    argv = ["--config", str(cfg), "--ckpt", "unused", "--gt-depth", str(gt), "--out", str(out), "--device", "cpu",
            "--record-loss", "toy"]
    result = evaluate.main(argv, model=model)
    assert model.calls == ["evaluate_results"] * 2
    written = json.loads((out / "metrics.json").read_text())
    assert written == json.loads(json.dumps(result))
    assert sorted(written["images"]) == ["a", "b"]
    for stem in ("a", "b"):
        d = np.load(out / "depth" / f"{stem}.npy")
        assert d.shape == (16, 16) and d.dtype == np.float32
        assert set(written["images"][stem]) == set(mc.KEYS) and written["images"][stem]["count"] == 14 * 14
    # the per-image values are depth_metrics of the written depths; the summary is their mean / std
    depths = np.stack([np.load(out / "depth" / f"{s}.npy") for s in ("a", "b")])
    gts = np.stack([np.load(gt / f"{s}.npy") for s in ("a", "b")])
    want = mc.metrics64(depths, gts, None, None, mc.pixel_rays(16, 16), True)
    got = {k: np.array([written["images"][s][k] for s in ("a", "b")]) for k in mc.KEYS}
    mc.check(got, want, "evaluate.main on the CPU")
    assert set(written["summary"]) == {"images", "skipped", "mae", "mse", "side", "mad"}
    assert written["summary"]["images"] == 2 and written["summary"]["skipped"] == 0
    for k in mc.METRICS:
        assert written["summary"][k] == pytest.approx([got[k].mean(), got[k].std()], rel=1e-12)
    losses = np.load(out / "step1_toy_model.npy")
    assert losses.shape == (2,) and (losses > 1).all()
    assert written["step1_loss"]["mean"] == pytest.approx(losses.mean())
    assert "mean = " in capsys.readouterr().out

    # --mask, --images, --gt-background
    out2 = tmp_path / "out2"
    masked = evaluate.main(["--config", str(cfg), "--ckpt", "unused", "--gt-depth", str(gt), "--out", str(out2),
                            "--device", "cpu", "--mask", "--images", "1", "--gt-background"],
                           model=StubModel(16), masking_model=StubMask())
    assert list(masked["images"]) == ["b"] and not os.path.exists(out2 / "depth" / "a.npy")
    d = np.load(out2 / "depth" / "b.npy")
    assert np.isnan(d[:, :4]).all() and np.isfinite(d[:, 4:]).all()
    m = (gts[1] < gts[1].max()).astype(np.float32)[None]
    want = mc.metrics64(d[None], gts[1:], None, m, mc.pixel_rays(16, 16), True)
    assert 0 < want["count"][0] <= 14 * 10
    mc.check({k: np.array([masked["images"]["b"][k]]) for k in mc.KEYS}, want, "evaluate.main --mask --gt-background")
    assert "step1_loss" not in masked and not os.path.exists(out2 / "step1_toy_model.npy")


def test_evaluate_arguments():
    from gan2shape_amd import evaluate
    with pytest.raises(SystemExit):
        evaluate.main(["--config", "x.yml"])                      # --ckpt and --out are required
    a = evaluate.build_parser().parse_args(["--config", "c", "--ckpt", "k", "--out", "o", "--images", "3", "5"])
    assert a.images == [3, 5] and not a.mask and a.gt_depth is None and a.record_loss is None
    path = evaluate.checkpoint_path_of("ck/face/depth_image_3_stage_2_100_it_now.pth")
    assert path("albedo") == os.path.join("ck/face", "albedo_image_3_stage_2_100_it_now.pth")
    assert evaluate.checkpoint_path_of("ck/{net}.pth")("lighting") == "ck/lighting.pth"
    with pytest.raises(ValueError):
        evaluate.checkpoint_path_of("ck/model.pth")
