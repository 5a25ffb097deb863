"""-m gpu: g2s_image_metrics (csrc/image_metrics.hip) through gan2shape_amd.metrics.image_metrics against the float64
oracle of image_metrics_cases.py on every case, from run to run and in both modes of g2s_set_deterministic, on
non-contiguous inputs, against the CPU path, inside a captured graph, and its argument checks.

Bound (image_metrics_cases.py): per metric, 4 x the largest error figure e = |got - want| / (A + |want|) that the
torch float32 composition on the CPU shows against the oracle over the same cases, measured in this process; count and
ssim_count must be equal, NaN and inf must sit exactly where the oracle has them.  Each test prints the figures it
measured before it asserts.
"""
import numpy as np
import pytest
import torch

import image_metrics_cases as ic

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


def _bits_equal(x, y):
    return all(torch.equal(x[k].view(torch.int32), y[k].view(torch.int32)) for k in ic.KEYS)      # NaN equals NaN


@pytest.mark.parametrize("name", list(ic.CASES))
def test_kernel_matches_the_float64_oracle(name, metrics):
    got = ic.run_case(metrics.image_metrics, name, device="cuda")
    want = ic.oracle(name)
    ic.check(got, want, f"{name} kernel")
    if name == "11x11":
        assert got["ssim_count"][0] == 1 and got["count"][0] == 121
    if name == "10x12":
        assert (got["ssim_count"] == 0).all() and np.isnan(got["ssim"]).all() and np.isfinite(got["psnr"]).all()
    if name == "16x16x17":
        assert (got["count"][[3, 11]] == 0).all() and all(np.isnan(got[k][[3, 11]]).all() for k in ic.METRICS)
        assert got["count"][5] > 0 and got["ssim_count"][5] == 0 and np.isnan(got["ssim"][5])
    if name == "a_eq_b":
        assert (got["mae"] == 0).all() and (got["mse"] == 0).all() and np.isposinf(got["psnr"]).all()
        assert (got["ssim"] == 1.0).all()


def test_repeated_runs_and_both_deterministic_modes_are_bit_equal(g2s, metrics):
    for name in ("128x128", "two_tiles", "16x16x17"):
        a, b, m = ic._torch_args(name, "cuda")
        r = ic.CASES[name]["data_range"]
        first = metrics.image_metrics(a, b, m, data_range=r)
        for _ in range(3):
            assert _bits_equal(first, metrics.image_metrics(a, b, m, data_range=r)), name
        prev = g2s.set_deterministic(True)
        try:
            assert _bits_equal(first, metrics.image_metrics(a, b, m, data_range=r)), name
            g2s.set_deterministic(False)
            assert _bits_equal(first, metrics.image_metrics(a, b, m, data_range=r)), name
        finally:
            g2s.set_deterministic(prev)


def test_non_contiguous_images_and_channel_masks(metrics):
    a, b, m = ic._torch_args("33x47_c3", "cuda")
    base = metrics.image_metrics(a, b, m, data_range=2.0)
    assert all(v.shape == (2,) and v.dtype == torch.float32 and v.is_cuda for v in base.values())
    wide = torch.full((2, 3, 33, 100), float("nan"), device="cuda")
    wide[..., 6:100:2] = a
    tall = torch.zeros(2, 3, 66, 47, device="cuda")
    tall[:, :, ::2] = b
    sliced, strided = wide[..., 6:100:2], tall[:, :, ::2]
    assert not sliced.is_contiguous() and not strided.is_contiguous()
    other = metrics.image_metrics(sliced, strided, m[:, None], data_range=2.0)
    assert _bits_equal(base, other)
    ic.check(ic.to_numpy(other), ic.oracle("33x47_c3"), "33x47_c3 sliced images, (B, 1, H, W) mask")
    empty = metrics.image_metrics(a[:0], b[:0], data_range=2.0)
    assert all(v.shape == (0,) and v.is_cuda for v in empty.values())
    with pytest.raises(ValueError, match="one device"):
        metrics.image_metrics(a, b.cpu(), data_range=2.0)


def test_gpu_path_matches_the_cpu_path(metrics):
    for name in ("33x47_c4", "two_tiles", "constants"):
        gpu = ic.run_case(metrics.image_metrics, name, device="cuda")
        cpu = ic.run_case(metrics.image_metrics, name, device="cpu")
        ic.check(gpu, cpu, f"{name} kernel against the CPU path")


def test_rejected_arguments_launch_nothing(g2s, metrics):
    L = g2s.load()
    name = "two_tiles"
    a, b, m = ic._torch_args(name, "cuda")
    B, C, H, W = a.shape
    SENTINEL = -7.5
    out = torch.full((B, 6), SENTINEL, device="cuda")
    need = L.g2s_image_metrics_workspace_bytes(B, C, H, W)
    assert need == B * 2 * 2 * 5 * 8                      # two tiles per axis, five doubles each
    assert L.g2s_image_metrics_workspace_bytes(B, C, H - 1, W - 1) == B * 5 * 8
    assert L.g2s_image_metrics_workspace_bytes(1, 1, 3, 5) == 5 * 8      # smaller than a window: one tile, no centre
    ws = torch.full((need + 64,), 0x5A, dtype=torch.uint8, device="cuda")
    ptr, st = g2s.ptr, g2s.stream

    def call(a_=a, b_=b, out_=out, B_=B, C_=C, H_=H, W_=W, ws_=ws, n=need, L_=2.0):
        return L.g2s_image_metrics(ptr(a_), ptr(b_), ptr(m), B_, C_, H_, W_, L_, ptr(out_), ptr(ws_), n, st())
    rejected = [({"a_": None}, -1), ({"b_": None}, -1), ({"out_": None}, -1), ({"B_": 0}, -1), ({"B_": 65536}, -1),
                ({"C_": 5}, -1), ({"C_": 0}, -1), ({"H_": 0}, -1), ({"W_": 32769}, -1), ({"L_": 0.0}, -1), ({"L_": -2.0}, -1),
                ({"L_": float("nan")}, -1), ({"ws_": None}, -3), ({"n": need - 1}, -3)]
    for kw, code in rejected:
        rc = call(**kw)
        assert rc == code and b"g2s_image_metrics" in L.g2s_last_error(), (kw, rc, L.g2s_last_error())
        with pytest.raises(g2s.G2SError):
            g2s.check(rc)
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()) and bool((ws == 0x5A).all())
    # a valid call afterwards returns correct values: nothing was launched or left pending
    assert call() == 0
    torch.cuda.synchronize()
    got = {k: out[:, i].cpu().numpy().astype(np.float64) for i, k in enumerate(ic.KEYS)}
    ic.check(got, ic.oracle(name), "two_tiles raw C call after the rejected ones")
    assert bool((ws[need:] == 0x5A).all())
    via_wrapper = ic.run_case(metrics.image_metrics, name, device="cuda")
    for k in ic.KEYS:
        np.testing.assert_array_equal(got[k], via_wrapper[k])


def test_captured_call_replays_bit_equal(metrics):
    a, b, m = ic._torch_args("two_tiles", "cuda")
    eager = {k: v.clone() for k, v in metrics.image_metrics(a, b, m, data_range=2.0).items()}
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        metrics.image_metrics(a, b, m, data_range=2.0)      # warm-up: code objects
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        captured = metrics.image_metrics(a, b, m, data_range=2.0)
    for _ in range(2):
        for v in captured.values():
            v.fill_(-3.0)
        graph.replay()
        torch.cuda.synchronize()
        assert _bits_equal(eager, captured)
