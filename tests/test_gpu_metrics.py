"""-m gpu: g2s_depth_metrics (csrc/metrics.hip) through gan2shape_amd.metrics.depth_metrics against the float64
oracle of metrics_cases.py on every case, from run to run, on non-contiguous inputs, against the CPU path, and its
argument checks.

Bound (metrics_cases.py): per metric, 4 x the largest error figure e = |got - want| / (A + |want|) that the torch
float32 composition on the CPU shows against the oracle over the same cases; count must be equal and NaN must sit
exactly where the oracle has NaN.  Each test prints the figures it measured before it asserts.
"""
import numpy as np
import pytest
import torch

import metrics_cases as mc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def g2s():
    import gan2shape_amd  # noqa: F401
    from gan2shape_amd import lib
    lib.load()
    return lib


@pytest.fixture(scope="module")
def metrics(g2s):
    from gan2shape_amd import metrics
    return metrics


def _args(name, device="cuda"):
    c = mc.CASES[name]
    return [None if c[k] is None else torch.from_numpy(c[k]).to(device) for k in ("pred", "gt", "mask_pred", "mask_gt")]


@pytest.mark.parametrize("name", list(mc.CASES))
def test_kernel_matches_the_float64_oracle(name, metrics):
    got = mc.run_case(metrics.depth_metrics, name, device="cuda")
    want = mc.oracle(name)
    mc.check(got, want, f"{name} kernel")
    if name == "3x3":
        assert got["count"][0] == 1 and got["side"][0] == 0.0
    if name == "p_eq_g":
        assert all((got[k] == 0).all() for k in mc.METRICS)
    if name == "16x16x17":
        assert got["count"][3] == 0 and got["count"][5] == 0
        assert all(np.isnan(got[k][[3, 5]]).all() for k in mc.METRICS)


def test_two_runs_are_bit_equal(metrics):
    for name in ("128x128", "33x33_raw", "16x16x17"):
        p, g, mp, mg = _args(name)
        r, erode = mc.CaseRenderer(), mc.CASES[name]["erode"]
        a = metrics.depth_metrics(p, g, mp, mg, renderer=r, erode=erode)
        for _ in range(3):
            b = metrics.depth_metrics(p, g, mp, mg, renderer=r, erode=erode)
            for k in mc.KEYS:      # bit patterns: NaN equals NaN
                assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), (name, k)


def test_non_contiguous_depth_and_channel_masks(metrics):
    p, g, mp, mg = _args("33x33")
    r = mc.CaseRenderer()
    base = metrics.depth_metrics(p, g, mp, mg, renderer=r)
    assert all(v.shape == (3,) and v.dtype == torch.float32 and v.is_cuda for v in base.values())
    wide = torch.full((3, 33, 70), float("nan"), device="cuda")
    wide[:, :, 4:70:2] = p
    sliced = wide[:, :, 4:70:2]
    tall = torch.zeros(3, 66, 33, device="cuda")
    tall[:, ::2] = g
    assert not sliced.is_contiguous() and not tall[:, ::2].is_contiguous()
    other = metrics.depth_metrics(sliced, tall[:, ::2], mp[:, None], mg[:, None], renderer=r)
    for k in mc.KEYS:
        assert torch.equal(base[k].view(torch.int32), other[k].view(torch.int32)), k
    mc.check(mc.to_numpy(other), mc.oracle("33x33"), "33x33 sliced depths, (B, 1, H, W) masks")


def test_gpu_path_matches_the_cpu_path(metrics):
    for name in ("33x33", "33x33_raw"):
        gpu = mc.run_case(metrics.depth_metrics, name, device="cuda")
        cpu = mc.run_case(metrics.depth_metrics, name, device="cpu")
        mc.check(gpu, cpu, f"{name} kernel against the CPU path")


def test_rejected_arguments_launch_nothing(g2s, metrics):
    L = g2s.load()
    name = "33x33"
    p, g, mp, mg = _args(name)
    B, H, W = p.shape
    rays = mc.CaseRenderer()._pixel_rays(H, W, torch.device("cuda")).reshape(-1, 3).contiguous()
    SENTINEL = -7.5
    out = torch.full((B, 5), SENTINEL, device="cuda")
    need = L.g2s_depth_metrics_workspace_bytes(B, H, W)
    assert need == B * 2 * 5 * 7 * 8
    ws = torch.full((need + 64,), 0x5A, dtype=torch.uint8, device="cuda")
    ptr, st = g2s.ptr, g2s.stream

    def call(pred=p, gt=g, rays_=rays, out_=out, B_=B, H_=H, W_=W, ws_=ws, n=need):
        return L.g2s_depth_metrics(ptr(pred), ptr(gt), ptr(mp), ptr(mg), ptr(rays_), B_, H_, W_, 1, ptr(out_), ptr(ws_),
                                   n, st())
    rejected = [({"pred": None}, -1), ({"gt": None}, -1), ({"rays_": None}, -1), ({"out_": None}, -1), ({"B_": 0}, -1),
                ({"B_": -1}, -1), ({"B_": 65536}, -1), ({"H_": 2}, -1), ({"W_": 2}, -1), ({"ws_": None}, -3),
                ({"n": need - 1}, -3)]
    for kw, code in rejected:
        rc = call(**kw)
        assert rc == code, (kw, rc, L.g2s_last_error())
        with pytest.raises(g2s.G2SError):
            g2s.check(rc)
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()) and bool((ws == 0x5A).all())
    # a valid call afterwards returns correct values: nothing was launched or left pending
    assert call() == 0
    torch.cuda.synchronize()
    got = {k: out[:, i].cpu().numpy().astype(np.float64) for i, k in enumerate(mc.KEYS)}
    mc.check(got, mc.oracle(name), "33x33 raw C call after the rejected ones")
    assert bool((ws[need:] == 0x5A).all())
    via_wrapper = mc.run_case(metrics.depth_metrics, name, device="cuda")
    for k in mc.KEYS:
        np.testing.assert_array_equal(got[k], via_wrapper[k])
