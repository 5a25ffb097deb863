"""-m gpu: upfirdn2d (csrc/upfirdn2d.hip) on every launch path against float64.

One test per group of tests/upfirdn_cases.py (the table, the paths, the reference and the bounds are described
there): forward, adjoint (autograd through op.upfirdn2d against the explicit transpose, and upfirdn2d_adjoint
bit-identical to it), f16, the two epilogues through the C entry points, and the plane loop, whose cases also show
that planes m and m + gridDim.y came out different.  Every test prints its error, e32 and their ratio."""
import numpy as np
import pytest
import torch

import upfirdn_cases as uc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def g2s():
    import gan2shape_amd  # noqa: F401
    from gan2shape_amd import lib
    return lib.load()  # fails loudly if libg2s.so is missing


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()     # a copy: the case data is read-only


def _check(name, what, got, ref, e32, bound):
    assert got.shape == ref.shape and np.isfinite(got).all(), (name, what, got.shape, ref.shape)
    err = np.abs(got.astype(np.float64) - ref)
    scale = np.abs(ref).max()
    worst = float((err / bound).max())
    print(f"{name} {what}: error {err.max() / scale:.3e} of max|ref|, e32 {e32:.3e}, ratio {err.max() / scale / e32:.2f}, "
          f"worst error / bound {worst:.2f}")
    assert worst <= 1.0, (f"{name} {what} {uc.CASE[name][2:7]}: {int((err > bound).sum())} elements over the bound, first at "
                          f"{np.unravel_index(np.argmax(err / bound), err.shape)}, {err.max() / scale / e32:.2f} x e32")


def _forward(name):
    from gan2shape_amd.op import upfirdn2d
    from gan2shape_amd.plugins import upfirdn2d_op
    _, _, shape, up, down, pad, *_ = uc.CASE[name]
    dt = uc.data(name)
    x, k = dev(dt["x"]), dev(dt["k"])
    if name not in uc.PLUGIN_ONLY:
        return upfirdn2d(x, k, up=up, down=down, pad=pad)
    major, H, W, (ux, uy), (dx, dy), p, *_ = uc.geometry(name)
    if name == "g_minor":           # [major, H, W, minor]: the plugin moves the minor dimension in front and back
        y = upfirdn2d_op.upfirdn2d(x.permute(0, 2, 3, 1).contiguous(), k, ux, uy, dx, dy, *p)
        return y.permute(0, 3, 1, 2)
    y = upfirdn2d_op.upfirdn2d(x.reshape(major, H, W, 1), k, ux, uy, dx, dy, *p)
    return y.reshape(shape[0], shape[1], y.shape[1], y.shape[2])


@pytest.mark.parametrize("name", uc.FORWARD)
def test_forward_vs_float64(g2s, name):
    dt = uc.data(name)
    y = _forward(name).cpu().numpy()
    assert y.dtype == np.float32
    _check(name, "y", y, dt["ref"], dt["e32"], uc.f32_bound(dt["ref"], dt["e32"]))


@pytest.mark.parametrize("name", uc.ADJOINT)
def test_adjoint_vs_float64_transpose(g2s, name):
    from gan2shape_amd.op import upfirdn2d
    from gan2shape_amd.op.upfirdn2d import upfirdn2d_adjoint
    _, _, shape, up, down, pad, *_ = uc.CASE[name]
    dt = uc.data(name)
    x, k, gy = dev(dt["x"]).requires_grad_(True), dev(dt["k"]), dev(dt["gy"])
    y = upfirdn2d(x, k, up=up, down=down, pad=pad)
    (gx,) = torch.autograd.grad(y, x, gy)
    _check(name, "gx", gx.cpu().numpy(), dt["ref_adj"], dt["e32_adj"], uc.f32_bound(dt["ref_adj"], dt["e32_adj"]))
    direct = upfirdn2d_adjoint(gy, k, up, down, pad, shape[2:])
    assert torch.equal(direct, gx), name


@pytest.mark.parametrize("name", uc.F16)
def test_f16_vs_float64(g2s, name):
    dt = uc.data(name)
    y = _forward(name)
    assert y.dtype == torch.float16
    _check(name, "y", y.float().cpu().numpy(), dt["ref"], dt["e32"], uc.f16_bound(dt["ref"], dt["e32"]))


def _epilogue(g2s, name):
    from gan2shape_amd import lib
    entry, alpha = uc.EPILOGUE[name]
    major, H, W, (up, _), (down, _), p, kh, kw, oh, ow = uc.geometry(name)
    dt = uc.data(name)
    x, k, bias, noise = (dev(dt[a]) for a in ("x", "k", "bias", "noise"))
    nw = dev(np.array([dt["nw"]], np.float32))
    y = torch.empty(uc.CASE[name][2][:2] + (oh, ow), device="cuda")
    fn = g2s.g2s_upfirdn2d_nba if entry == "nba" else g2s.g2s_upfirdn2d_nba_ps
    lib.check(fn(lib.ptr(x), lib.ptr(k), lib.ptr(y), major, bias.numel(), H, W, kh, kw, up, down, *p, lib.ptr(bias),
                 lib.ptr(noise), lib.ptr(nw), alpha, uc.GAIN, lib.stream()))
    return y.cpu().numpy()


@pytest.mark.parametrize("name", [n for n in uc.NBA if n not in uc.PLANE])
def test_epilogue_vs_float64(g2s, name):
    dt = uc.data(name)
    if uc.EPILOGUE[name][0] == "nba_ps":
        assert np.abs(dt["noise"][0] - dt["noise"][1]).max() > 0.1
    _check(name, "y", _epilogue(g2s, name), dt["ref"], dt["e32"], uc.f32_bound(dt["ref"], dt["e32"]))


@pytest.mark.parametrize("name", uc.PLANE)
def test_plane_loop_vs_float64(g2s, name):
    dt = uc.data(name)
    y = _epilogue(g2s, name) if name in uc.EPILOGUE else _forward(name).cpu().numpy()
    _check(name, "y", y, dt["ref"], dt["e32"], uc.f32_bound(dt["ref"], dt["e32"]))
    major, _, _, _, _, _, _, _, oh, ow = uc.geometry(name)
    gy = uc.grid_y(major, oh, ow, uc.CASE[name][6])
    assert gy < major
    planes = y.reshape(major, oh, ow)
    same = (planes[:-gy] == planes[gy:]).all(axis=(1, 2))       # a stale prefetch would repeat plane m at m + gridDim.y
    assert not same.any(), (name, np.flatnonzero(same)[:8])
