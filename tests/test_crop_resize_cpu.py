"""The centre crop of step 2 on the host (op/resample.py): the band tables against the float64
fixture tests/golden/crop_resize.npz (the reference's utils.resize / utils.crop, tests/golden/make_crop_resize_golden.py),
the CPU route, the dataset transform and the configuration keys."""
import numpy as np
import pytest
import torch

import crop_resize_cases as cc

import gan2shape_amd  # noqa: F401
from gan2shape_amd import dataset, utils
from gan2shape_amd.op import resample as rs


@pytest.fixture(scope="module")
def fixture(golden):
    return golden("crop_resize")


def dense(bands):
    lo, ln, w = bands.host
    A = np.zeros((bands.n_out, bands.n_in))
    for i in range(bands.n_out):
        A[i, lo[i]:lo[i] + ln[i]] = w[i, :ln[i]]
    return A


@pytest.mark.parametrize("name", list(cc.CASES))
def test_operator_reproduces_the_float64_fixture(fixture, name):
    gan, origin, crop, image, _ = cc.CASES[name]
    x, g = cc.operands(fixture, name)
    A = rs.crop_resize_tables(gan, origin, crop, image).dense
    assert A.dtype == np.float64 and A.shape == (image, gan)
    out = np.einsum("ia,ncab,jb->ncij", A, x.numpy(), A)
    gin = np.einsum("ia,ncij,jb->ncab", A, g.numpy(), A)
    assert cc.max_err(out, fixture[f"{name}.out"]) <= 1e-12
    assert cc.max_err(gin, fixture[f"{name}.gin"]) <= 1e-12


@pytest.mark.parametrize("name", list(cc.CASES))
def test_tables_are_contiguous_bands_of_the_operator_and_its_transpose(name):
    gan, origin, crop, image, _ = cc.CASES[name]
    t = rs.crop_resize_tables(gan, origin, crop, image)
    A32 = t.dense.astype(np.float32).astype(np.float64)           # weights are rounded once from float64
    assert np.array_equal(dense(t.fwd), A32) and np.array_equal(dense(t.tr), A32.T)
    for bands, M in ((t.fwd, t.dense), (t.tr, t.dense.T)):
        lo, ln, w = bands.host
        assert w.dtype == np.float32 and w.shape == (M.shape[0], bands.K) and 1 <= bands.K <= rs.MAX_TAPS
        for i in range(M.shape[0]):
            nz = np.flatnonzero(M[i])
            assert len(nz) == ln[i] and (ln[i] == 0 or (nz[0] == lo[i] and nz[-1] == lo[i] + ln[i] - 1))
            assert not w[i, ln[i]:].any()
    assert 2 <= t.fwd.host[1].max() <= 5 and 2 <= t.tr.host[1].max() <= 4
    # the input positions nothing reads are exactly the ones the crop drops: those whose area / bilinear footprint in
    # the origin_size image lies outside the crop window
    R1 = rs.resize_matrix(gan, origin)
    m = (origin - crop) // 2
    kept = np.flatnonzero(R1[m:m + crop].any(0))
    assert np.array_equal(np.flatnonzero(t.tr.host[1]), kept)
    assert np.array_equal(np.flatnonzero(t.dense.any(0)), kept)
    if name.startswith("no_rows_dropped"):
        assert len(kept) == gan
    else:
        assert 0 < len(kept) < gan and kept[0] > 0 and kept[-1] < gan - 1
    assert rs.crop_resize_tables(gan, origin, crop, image) is t                  # cached per size tuple and device


@pytest.mark.parametrize("name", list(cc.CASES))
def test_cpu_route_is_the_torch_composition(fixture, name):
    gan, origin, crop, image, _ = cc.CASES[name]
    x, g = cc.operands(fixture, name)
    x64 = x.clone().requires_grad_(True)
    y = rs.crop_resize(x64, origin, crop, image)
    assert y.dtype == torch.float64 and cc.max_err(y.detach().numpy(), fixture[f"{name}.out"]) <= 1e-12
    gin, = torch.autograd.grad(y, x64, g)
    assert cc.max_err(gin.numpy(), fixture[f"{name}.gin"]) <= 1e-12
    x32 = x.float()
    want = utils.resize(utils.crop(utils.resize(x32, [origin, origin]), crop), [image, image])
    assert torch.equal(rs.crop_resize(x32, origin, crop, image), want)
    assert torch.equal(rs.crop_resize(x32, origin, crop, image, fused=False), want)
    assert np.array_equal(want.numpy(), fixture[f"{name}.out32"])                # the reference's float32 composition


def test_bad_crop_values_raise():
    x = torch.zeros(1, 3, 32, 32)
    for origin, crop in ((32, 0), (32, -4), (32, 33), (16, 24)):
        with pytest.raises(ValueError, match="crop"):
            rs.crop_resize(x, origin, crop, 32)
        with pytest.raises(ValueError, match="crop"):
            rs.crop_resize_tables(32, origin, crop, 32)
        with pytest.raises(ValueError, match="crop"):
            dataset.default_transform(32, crop=crop, origin_size=origin)
    with pytest.raises(ValueError, match="square"):
        rs.crop_resize(torch.zeros(1, 3, 32, 24), 32, 24, 32)
    with pytest.raises(ValueError, match="shapes"):
        rs.make_bands([0, 1], [1], np.ones((2, 1)), 4, "cpu")


def test_default_transform_with_a_crop():
    from PIL import Image
    rng = np.random.RandomState(3)
    for (w, h) in ((61, 45), (40, 77), (48, 48)):
        im = Image.fromarray(rng.randint(0, 256, size=(h, w, 3), dtype=np.uint8))
        for image_size, crop, origin in ((32, 24, 40), (32, 33, 40), (32, 32, 32), (16, 40, 40)):
            t = dataset.default_transform(image_size, crop=crop, origin_size=origin)(im)
            assert tuple(t.shape) == (3, image_size, image_size) and t.dtype == torch.float32
            # resize (smaller edge to origin_size), slice, resize
            edge = im.resize((origin, max(1, int(origin * h / w))) if w <= h else (max(1, int(origin * w / h)), origin),
                             Image.BILINEAR) if min(w, h) != origin else im
            a = np.asarray(edge)
            top, left = (a.shape[0] - crop) // 2, (a.shape[1] - crop) // 2
            cut = Image.fromarray(a[top:top + crop, left:left + crop])
            if crop != image_size:
                cut = cut.resize((image_size, image_size), Image.BILINEAR)
            want = torch.from_numpy(np.asarray(cut).copy()).permute(2, 0, 1).float().div(255)
            assert torch.equal(t, want)
        # origin_size defaults to image_size; without a crop nothing changed
        t = dataset.default_transform(32, crop=24)(im)
        assert tuple(t.shape) == (3, 32, 32)
        plain = dataset.default_transform(32)(im)
        assert min(plain.shape[1:]) == 32 and torch.equal(plain, dataset.default_transform(32, None, 40)(im))


class _Stub:
    """What GAN2Shape.gan_to_image_size reads of the model."""
    def __init__(self, crop, origin_size=None, image_size=16, fused=True):
        self.crop, self.origin_size, self.image_size, self.crop_fused = crop, origin_size, image_size, None
        self.renderer = type("R", (), {"fused": fused})()


def test_without_crop_the_model_takes_the_old_call(monkeypatch):
    from gan2shape_amd.model import GAN2Shape
    x = torch.rand(2, 3, 32, 32) * 2 - 1

    def refuse(*a, **k):
        raise AssertionError("crop_resize reached with crop absent")
    monkeypatch.setattr(rs, "crop_resize", refuse)
    seen = []
    real = utils.resize
    monkeypatch.setattr(utils, "resize", lambda im, size: seen.append(list(size)) or real(im, size))
    y = GAN2Shape.gan_to_image_size(_Stub(None), x)
    assert seen == [[16, 16]] and torch.equal(y, real(x, [16, 16]))


def test_with_crop_the_model_takes_the_composition_on_the_cpu():
    from gan2shape_amd.model import GAN2Shape
    x = torch.rand(2, 3, 32, 32) * 2 - 1
    for fused in (True, False):
        y = GAN2Shape.gan_to_image_size(_Stub(20, 24, fused=fused), x)
        assert torch.equal(y, utils.resize(utils.crop(utils.resize(x, [24, 24]), 20), [16, 16]))


def test_model_source_routes_every_gan_resize_through_the_switch():
    """The projected image of forward_step2, the frames of manipulate, and the GAN image under relative_encoding,
    which both take from _project_latent."""
    import inspect
    from gan2shape_amd.model import GAN2Shape
    for fn in (GAN2Shape.forward_step2, GAN2Shape.manipulate):
        assert inspect.getsource(fn).count("self._project_latent(") == 1
    for fn, n in ((GAN2Shape.forward_step2, 1), (GAN2Shape.manipulate, 1), (GAN2Shape._project_latent, 1)):
        src = inspect.getsource(fn)
        assert src.count("self.gan_to_image_size(") == n and "utils.resize(" not in src
