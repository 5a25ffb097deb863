"""g2s_mvn_fit (csrc/mvn.hip) and view_light on the device: values against the float64 oracle within the bounds of
view_light_cases, structure, determinism, status codes, launcher refusals, canaries, and fit_view_light end to end on
the face-128 model."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

import gan2shape_amd  # noqa: F401
import view_light_cases as vc
from canary_buffers import CANARY, Buffers
from gan2shape_amd import lib, view_light

pytestmark = pytest.mark.gpu


def _launch(rows, D, blocks, ridge, shift=0):
    """One bare launch on canary views -> (dict of host arrays, status, raw bytes of the four outputs).  shift: floats
    by which the rows are moved off their 16-byte alignment."""
    bufs = Buffers()
    N, ld = rows.shape
    x = bufs.view("rows", arr=rows, shift=shift)
    mean = bufs.view("mean", like=np.empty(D))
    cov = bufs.view("cov", like=np.empty((D, D)))
    tril = bufs.view("tril", like=np.empty((D, D)))
    status = bufs.view("status", like=np.empty(1))
    view_light.mvn_fit_launch(x, N, D, ld, blocks, ridge, mean, cov, tril, status)
    torch.cuda.synchronize()
    bufs.check()
    got = {"mean": mean.cpu().numpy(), "cov": cov.cpu().numpy().reshape(D, D), "tril": tril.cpu().numpy().reshape(D, D)}
    code = int(status.view(torch.int32).item())
    raw = b"".join(t.cpu().numpy().tobytes() for t in (mean, cov, tril, status))
    return got, code, raw


@pytest.mark.parametrize("name,N,D,blocks,ld,ridge", vc.CASES, ids=vc.IDS)
def test_mvn_fit_kernel_against_the_oracle(name, N, D, blocks, ld, ridge):
    rows = vc.rows_of(name)
    got, code, raw = _launch(rows, D, blocks, ridge)
    assert code == 0
    vc.check_fit(got, rows[:, :D], blocks, ridge, name)
    vc.check_structure(got["cov"], got["tril"], blocks, name)
    _, code2, raw2 = _launch(rows, D, blocks, ridge)
    assert code2 == 0 and raw2 == raw, "two launches on the same input differ"


def test_misaligned_rows_take_the_dword_loads_to_the_same_bytes():
    """Even D, even ld and an 8-byte aligned base load pairs; one float off, the same rows load as dwords.  The
    arithmetic and its order do not change."""
    rows = vc.rows_of("n257_d10")
    _, code, raw = _launch(rows, 10, (6, 4), 0.0)
    _, code1, raw1 = _launch(rows, 10, (6, 4), 0.0, shift=1)
    assert code == 0 and code1 == 0 and raw1 == raw


def test_mvn_fit_on_the_device_equals_the_bare_launch():
    rows = vc.rows_of("n1000_d10_ld12")
    got, _, _ = _launch(rows, 10, (6, 4), 0.0)
    strided = torch.from_numpy(rows.copy()).cuda()[:, :10]          # row stride 12: no copy is made
    fit = view_light.mvn_fit(strided, (6, 4))
    assert fit.n == 1000 and fit.mean.is_cuda
    for key in ("mean", "cov", "tril"):
        assert np.array_equal(getattr(fit, key).cpu().numpy(), got[key]), key


def test_status_of_a_constant_column_and_of_a_non_finite_input():
    rows = vc.rows_of("n257_d10").copy()
    rows[:, 7] = 0.25
    got, code, _ = _launch(rows, 10, (6, 4), 0.0)
    assert code == 1 + 7
    x = rows.astype(np.float64)
    assert np.abs(got["mean"] - x.mean(0)).max() <= 4 * vc.EPS32 * np.abs(x.mean(0)).max()
    cov = np.cov(x, rowvar=False)
    assert np.abs(got["cov"] - cov).max() <= 4 * vc.EPS32 * np.abs(cov).max() and got["cov"][7, 7] == 0.0
    with pytest.raises(ValueError, match=r"column 7 \(column 1 of block 1"):
        view_light.mvn_fit(torch.from_numpy(rows).cuda(), (6, 4))
    fit = view_light.mvn_fit(torch.from_numpy(rows).cuda(), (6, 4), ridge=1e-6)
    assert fit.cov[7, 7].item() == pytest.approx(1e-6, rel=1e-6)

    rows = vc.rows_of("n257_d10").copy()
    rows[200, 3] = np.inf
    _, code, _ = _launch(rows, 10, (6, 4), 0.0)
    assert code == -1
    with pytest.raises(ValueError, match="non-finite"):
        view_light.mvn_fit(torch.from_numpy(rows).cuda(), (6, 4))


def test_launcher_refuses_bad_arguments_without_a_launch():
    L = lib.load()
    bufs = Buffers()
    x = bufs.view("rows", arr=vc.rows_of("n255_d10"))
    outs = [bufs.view(k, like=np.empty(n)) for k, n in (("mean", 17), ("cov", 17 * 17), ("tril", 17 * 17), ("status", 1))]

    def call(N, D, ld, blocks):
        arr = (C.c_int * len(blocks))(*blocks)
        return L.g2s_mvn_fit(lib.ptr(x), N, D, ld, arr, len(blocks), 0.0, *[lib.ptr(o) for o in outs], lib.stream())

    for N, D, ld, blocks, what in ((255, 0, 10, (1,), "D must be"), (255, 17, 17, (17,), "D must be"),
                                   (1, 10, 10, (6, 4), "N must be"), (255, 10, 9, (6, 4), "row stride"),
                                   (255, 10, 10, (6, 3), "blocks sum to 9"), (255, 10, 10, (6, 5), "blocks must be"),
                                   (255, 10, 10, (6, 0, 4), "blocks must be"), (255, 10, 10, (2, 2, 2, 2, 2), "blocks, got 5")):
        assert call(N, D, ld, blocks) == -1, (N, D, ld, blocks)         # G2S_ERR_INVALID
        assert what in L.g2s_last_error().decode(), (what, L.g2s_last_error().decode())
    torch.cuda.synchronize()
    bufs.check()
    assert all(bool((o == CANARY).all()) for o in outs), "a refused call wrote an output"


# ---- end to end on the face-128 model of the GPU model tests
E2E_RIDGE = 1e-4        # 6 images give a view covariance of rank 5: the ridge is what makes it a prior


@pytest.fixture(scope="module")
def face_trainer():
    import bench
    from gan2shape_amd.model import GAN2Shape
    from gan2shape_amd.trainer import Trainer
    torch.manual_seed(0)
    return Trainer(GAN2Shape, bench.face_config(n_proj=2), device="cuda")


def _toy_images(n, size):
    g = torch.Generator().manual_seed(77)
    x = torch.randn(n, 3, size // 4, size // 4, generator=g)
    return list(torch.tanh(torch.nn.functional.interpolate(x, scale_factor=4, mode="bilinear")))


def test_fit_view_light_end_to_end(face_trainer, tmp_path):
    import bench
    from gan2shape_amd.model import GAN2Shape
    from gan2shape_amd.trainer import Trainer
    model = face_trainer.model
    images = _toy_images(6, model.image_size)
    fit, rows = view_light.fit_view_light(model, images, batch=4, ridge=E2E_RIDGE)        # batches of 4 and 2
    assert rows.shape == (6, 10) and rows.is_cuda

    x = torch.stack(images)
    sampler = model.view_light_sampler
    means = torch.cat([sampler.view_mean, sampler.light_mean]).cpu()

    def cpu_rows(dtype):
        with torch.no_grad():
            nets = [copy.deepcopy(n).cpu().to(dtype) for n in (model.viewpoint_net, model.lighting_net)]
            return torch.cat([n(x.to(dtype)) for n in nets], 1) + means.to(dtype)

    r64 = cpu_rows(torch.float64)
    own = float((cpu_rows(torch.float32).double() - r64).abs().max())
    err = float((rows.cpu().double() - r64).abs().max())
    print(f"fit_view_light rows vs float64 nets: {err:.3e}; float32 CPU nets: {own:.3e}; multiple {err / own:.2f}")
    assert err <= 4 * own
    vc.check_fit({k: getattr(fit, k).cpu().numpy() for k in ("mean", "cov", "tril")}, rows.cpu().numpy(), (6, 4),
                 E2E_RIDGE, "end to end")

    # the files take the place of the inline prior in a fresh model; one step 2 runs on them
    view_light.save_mvn(str(tmp_path / "view_mvn.pth"), *view_light.view_of(fit))
    view_light.save_mvn(str(tmp_path / "light_mvn.pth"), *view_light.light_of(fit))
    cfg = bench.face_config(n_proj=2)
    del cfg["view_mvn"], cfg["light_mvn"]
    cfg.update(view_mvn_path=str(tmp_path / "view_mvn.pth"), light_mvn_path=str(tmp_path / "light_mvn.pth"))
    torch.manual_seed(0)
    fresh = Trainer(GAN2Shape, cfg, device="cuda")
    assert torch.equal(fresh.model.view_light_sampler.view_mean, fit.mean[:6])
    image, latent = bench.synthetic_sample(fresh.model, 1234, torch.device("cuda"))
    runner = bench.StepRunner(fresh, image, latent)
    assert torch.isfinite(runner.run(1)).item()
    assert torch.isfinite(runner.run(2)).item()
