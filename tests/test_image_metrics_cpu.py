"""gan2shape_amd.metrics.image_metrics on CPU tensors (the torch composition `_image_metrics_torch`, which is also the
specification of csrc/image_metrics.hip) and the ImageMetrics accumulator.

The float64 composition is the oracle of the kernel test; here it is checked against an independent numpy statement
of the definitions (`ssim64_direct`: every window cut out and weighted by the 2-D window) and, where scikit-image is
installed, against skimage.metrics.structural_similarity.  The float32 CPU path is then held to the bound of
image_metrics_cases.py; every test prints its figures before it asserts.
"""
import math

import numpy as np
import pytest
import torch

import image_metrics_cases as ic


@pytest.fixture(scope="module")
def metrics():
    import gan2shape_amd  # noqa: F401
    from gan2shape_amd import metrics
    return metrics


ROUNDING64 = {k: 1e-11 for k in ic.METRICS}      # float64 rounding of a few hundred terms, in units of e


@pytest.mark.parametrize("name", [n for n in ic.CASES if n != "128x128"])
def test_oracle_matches_the_window_by_window_statement(name, metrics):
    c = ic.CASES[name]
    ic.check(ic.oracle(name), ic.ssim64_direct(c["a"], c["b"], c["mask"], c["data_range"]),
             f"{name} float64 composition against the direct statement", ROUNDING64)


def test_oracle_matches_skimage_on_the_unmasked_cases(metrics):
    sk = pytest.importorskip("skimage.metrics")
    for name in ic.UNMASKED:
        c = ic.CASES[name]
        want = np.array([sk.structural_similarity(c["a"][i].astype(np.float64), c["b"][i].astype(np.float64), channel_axis=0,
                                                  gaussian_weights=True, sigma=1.5, use_sample_covariance=False,
                                                  data_range=c["data_range"]) for i in range(len(c["a"]))])
        got = ic.oracle(name)["ssim"]
        print(f"{name}: ssim {got} skimage {want}")
        np.testing.assert_allclose(got, want, rtol=1e-11, atol=1e-12)


@pytest.mark.parametrize("name", list(ic.CASES))
def test_cpu_path_matches_the_float64_oracle(name, metrics):
    got = ic.run_case(metrics.image_metrics, name)
    want = ic.oracle(name)
    ic.check(got, want, f"{name} float32 CPU path")
    if name == "11x11":
        assert got["ssim_count"][0] == 1 and got["count"][0] == 121
    if name == "10x12":
        assert (got["ssim_count"] == 0).all() and np.isnan(got["ssim"]).all() and np.isfinite(got["psnr"]).all()
    if name == "16x16x17":
        assert (got["count"][[3, 11]] == 0).all() and all(np.isnan(got[k][[3, 11]]).all() for k in ic.METRICS)
        assert got["count"][5] > 0 and got["ssim_count"][5] == 0 and np.isnan(got["ssim"][5]) and np.isfinite(got["psnr"][5])
    if name == "a_eq_b":
        assert (got["mae"] == 0).all() and (got["mse"] == 0).all() and np.isposinf(got["psnr"]).all()
        assert (got["ssim"] == 1.0).all()
    if name == "constants":       # mu_a = 0.3, mu_b = -0.2, no variance: ((2 mu_a mu_b + C1) C2) / ((mu_a^2 + mu_b^2 + C1) C2)
        c1 = (0.01 * 2.0) ** 2
        assert got["ssim"][0] == pytest.approx((2 * 0.3 * -0.2 + c1) / (0.09 + 0.04 + c1), abs=1e-4)


def test_ssim_lands_between_the_extremes():
    for name in ic.CASES:
        if name in ("a_eq_b", "constants"):
            continue
        s = ic.oracle(name)["ssim"]
        s = s[~np.isnan(s)]
        assert ((s > 0.2) & (s < 0.95)).all(), (name, s)


def test_float64_inputs_stay_float64_inside(metrics):
    a, b, m = ic._torch_args("33x47_c3", dtype=torch.float64)
    got = metrics.image_metrics(a, b, m, data_range=2.0)
    assert all(v.dtype == torch.float32 and v.shape == (2,) for v in got.values()) and set(got) == set(ic.KEYS)
    want = ic.oracle("33x47_c3")
    half_ulp = {k: 2.0 ** -24 for k in ic.METRICS}        # the float32 cast of the result, nothing else
    ic.check(ic.to_numpy(got), want, "33x47_c3 float64 CPU path", half_ulp)


def test_shapes_and_refusals(metrics):
    a, b, m = ic._torch_args("33x47_c3")
    base = metrics.image_metrics(a, b, m, data_range=2.0)
    other = metrics.image_metrics(a, b, m[:, None], data_range=2.0)                   # (B, 1, H, W) mask
    wide = torch.zeros(2, 3, 33, 94)
    wide[..., ::2] = a
    sliced = metrics.image_metrics(wide[..., ::2], b, m, data_range=2.0)            # non-contiguous
    for k in ic.KEYS:
        assert torch.equal(base[k].view(torch.int32), other[k].view(torch.int32)), k
        assert torch.equal(base[k].view(torch.int32), sliced[k].view(torch.int32)), k
    empty = metrics.image_metrics(a[:0], b[:0], m[:0], data_range=2.0)
    assert set(empty) == set(ic.KEYS) and all(v.shape == (0,) and v.dtype == torch.float32 for v in empty.values())
    with pytest.raises(ValueError, match="one shape"):
        metrics.image_metrics(a, b[:, :, :-1], data_range=2.0)
    with pytest.raises(ValueError, match="one shape"):
        metrics.image_metrics(a[0], b[0], data_range=2.0)
    with pytest.raises(ValueError, match="mask has shape"):
        metrics.image_metrics(a, b, m[:, :-1], data_range=2.0)
    with pytest.raises(ValueError, match="outside"):
        metrics.image_metrics(torch.zeros(1, 5, 12, 12), torch.zeros(1, 5, 12, 12), data_range=2.0)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="data_range"):
            metrics.image_metrics(a, b, data_range=bad)
    with pytest.raises(TypeError):
        metrics.image_metrics(a, b)                                                   # data_range has no default
    with pytest.raises(ValueError, match="one device"):
        metrics.image_metrics(a, b, m.to("meta"), data_range=2.0)


def test_summary_on_hand_made_rows(metrics):
    nan, inf = float("nan"), float("inf")
    acc = metrics.ImageMetrics()
    assert len(acc) == 0
    s = acc.summary()
    assert s["images"] == 0 and s["skipped"] == 0 and s["exact"] == 0 and s["ssim_images"] == 0
    assert all(math.isnan(x) for k in ic.METRICS for x in s[k])
    acc.update({"count": torch.tensor([10., 0.]), "mae": torch.tensor([0.1, nan]), "mse": torch.tensor([0.01, nan]),
                "psnr": torch.tensor([20., nan]), "ssim_count": torch.tensor([4., 0.]), "ssim": torch.tensor([0.5, nan])})
    acc.update({"count": np.array([5., 7.]), "mae": np.array([0.3, 0.0]), "mse": np.array([0.03, 0.0]),
                "psnr": np.array([30., inf]), "ssim_count": np.array([0., 3.]), "ssim": np.array([nan, 1.0])})
    assert len(acc) == 4
    s = acc.summary()
    assert s["images"] == 3 and s["skipped"] == 1 and s["exact"] == 1 and s["ssim_images"] == 2
    assert s["mae"] == pytest.approx((np.mean([0.1, 0.3, 0.0]), np.std([0.1, 0.3, 0.0])))
    assert s["mse"] == pytest.approx((np.mean([0.01, 0.03, 0.0]), np.std([0.01, 0.03, 0.0])))
    assert s["psnr"] == pytest.approx((25.0, 5.0))          # the infinite one is counted under "exact", not averaged
    assert s["ssim"] == pytest.approx((0.75, 0.25))
    with pytest.raises(ValueError, match="ImageMetrics.update"):
        acc.update({k: np.zeros(2 if k != "ssim" else 3) for k in ic.KEYS})
    # the depth accumulator shares the rows' code and keeps its own summary
    d = metrics.DepthMetrics()
    d.update({"count": np.array([4., 0.]), "mae": np.array([1., nan]), "mse": np.array([2., nan]),
              "side": np.array([3., nan]), "mad": np.array([nan, nan])})
    s = d.summary()
    assert s["images"] == 1 and s["skipped"] == 1 and s["mae"] == (1.0, 0.0) and math.isnan(s["mad"][0])
    with pytest.raises(ValueError, match="DepthMetrics.update"):
        d.update({"count": np.zeros(1), "mae": np.zeros(2), "mse": np.zeros(1), "side": np.zeros(1), "mad": np.zeros(1)})
