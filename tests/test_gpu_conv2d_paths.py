"""-m gpu: g2s_conv2d, g2s_conv2d_wgrad and g2s_conv2d_bwd on every launch path against float64, element by element.

The tables, the plans, the reference and the bound are those of tests/conv2d_cases.py.  The launches go through the raw
launchers of op/conv.py (_conv2d_raw, _wgrad, _conv_bwd_raw), or through the C entry points where those cannot express
the call: a gain, a bias under groups, a caller-filled output with y_is_zero = 0, a rejected geometry.  Nothing passes
ConvFunction's activation gate.  Every test prints its error, e32 and their ratio, and restores g2s_modconv_tune(-1, -1)
and the deterministic flag."""
import contextlib

import numpy as np
import pytest
import torch

import conv2d_cases as cc

pytestmark = pytest.mark.gpu

GUARD = 256         # floats on either side of an output that is the interior of a larger buffer
SENTINEL = 3.25


@pytest.fixture(scope="module")
def g2s():
    import gan2shape_amd  # noqa: F401
    from gan2shape_amd import lib
    return lib.load()  # fails loudly if libg2s.so is missing


def dev(a):
    return None if a is None else torch.from_numpy(np.array(a)).cuda()     # a copy: the case data is read-only


@contextlib.contextmanager
def tuned(L, tile=-1, sk=-1, det=False):
    from gan2shape_amd import lib
    prev = lib.set_deterministic(det)
    try:
        assert L.g2s_modconv_tune(tile, sk) == 0
        yield
    finally:
        L.g2s_modconv_tune(-1, -1)
        lib.set_deterministic(prev)


def guarded(shape, fill):
    """A tensor of `shape` that is the interior of a larger buffer: (buffer, view)."""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
    view = buf[GUARD:GUARD + n].view(shape)
    view.fill_(fill)
    return buf, view


def guards_intact(buf):
    return bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[-GUARD:] == SENTINEL).all())


def _check(name, what, path, got, ref, e32, cap, slack=0.0, ratio=cc.RATIO):
    assert got.shape == ref.shape, (name, what, got.shape, ref.shape)
    assert np.isfinite(got).all(), (name, what, "not finite", int((~np.isfinite(got)).sum()))
    err = np.abs(got.astype(np.float64) - ref)
    scale = np.abs(ref).max()
    bound = cc.bound(ref, e32, cap, ratio) + slack
    worst = float((err / np.maximum(bound, 1e-300)).max()) if err.max() > 0 else 0.0
    ratio_e32 = err.max() / scale / cc.floor_e32(e32)
    print(f"RATIO {path} {name} {what}: error {err.max() / scale:.3e} of max|ref|, e32 {e32:.3e}, ratio {ratio_e32:.2f} of {ratio:g}, "
          f"worst error / bound {worst:.2f}, worst error / cap {float((err / np.maximum(cap + slack, 1e-300)).max()):.3f}")
    assert (err <= bound).all(), (f"{name} {what} [{path}]: {int((err > bound).sum())} of {err.size} elements over the bound, "
                                  f"first at {np.unravel_index(np.argmax(err - bound), err.shape)}, {ratio_e32:.2f} x e32")


def _path(c, pl):
    return (f"{'scatter' if c.adj else 'gather'}/tile{pl['pick']}/{'split' if pl['splitk'] > 1 else 'plain'}"
            f"{'/deferred' if pl['deferred'] else ''}")


def c_conv(L, c, x, w, bias, y, y_is_zero):
    """g2s_conv2d itself; returns its code."""
    from gan2shape_amd import lib
    oh, ow = c.out_hw
    has_bias, act, alpha, gain = c.ep if c.ep is not None else (False, False, 0.0, 1.0)
    return L.g2s_conv2d(lib.ptr(x), lib.ptr(w), lib.ptr(bias if has_bias else None), lib.ptr(y), c.B, c.Cr, c.M, c.H, c.W,
                        c.k, c.s, c.p, c.adj, c.mm, oh if c.adj else 0, ow if c.adj else 0, int(act), float(alpha),
                        float(gain), int(y_is_zero), c.groups, lib.stream())


def launch_conv(L, c, x, w, bias):
    """One call as the case describes it, under the tuning state the caller has set."""
    from gan2shape_amd import lib
    from gan2shape_amd.op.conv import _conv2d_raw
    if c.ep is None:
        return _conv2d_raw(x, w, None, c.Cr, c.M, c.k, c.s, c.p, c.adj, c.mm, c.out_hw, False, 0.0, groups=c.groups)
    y = torch.empty((c.B, c.groups * c.M) + c.out_hw, dtype=torch.float32, device="cuda")
    lib.check(c_conv(L, c, x, w, bias, y, 0))
    return y


# ---------------------------------------------------------------------------------------------------- g2s_conv2d
@pytest.mark.parametrize("name", [c.name for c in cc.CONV])
def test_conv2d_vs_float64(g2s, name):
    c = cc.CONV_BY_NAME[name]
    dt = cc.conv_data(name)
    x, w, bias = dev(dt["x"]), dev(dt["w"]), dev(dt["bias"])
    with tuned(g2s, c.tile, c.sk, c.det):
        y = launch_conv(g2s, c, x, w, bias).cpu().numpy()
    _check(name, "y", _path(c, c.plan()), y, dt["ref"], dt["e32"], dt["cap"], ratio=cc.conv_ratio(c.plan()))


@pytest.mark.parametrize("name", list(cc.SWEEP))
def test_conv2d_forced_tiles_and_splits_vs_float64(g2s, name):
    """Every tile 0..4 under split-K 1, 2, 3 and one above kt_min (clipped), on one case per tap body."""
    c, _ = cc.SWEEP[name]
    dt = cc.conv_data(name)
    x, w = dev(dt["x"]), dev(dt["w"])
    for tile in cc.SWEEP_TILES:
        for sk in cc.sweep_splits(c):
            with tuned(g2s, tile, sk):
                y = launch_conv(g2s, c, x, w, None).cpu().numpy()
            _check(name, f"y tune({tile},{sk})", _path(c, c.plan(tile=tile, sk=sk)), y, dt["ref"], dt["e32"], dt["cap"])


@pytest.mark.parametrize("name", cc.PROMISE)
def test_conv2d_output_promises_and_guards(g2s, name):
    """y_is_zero = 0 on a NaN-filled y: the library clears what it adds into, every element comes back finite and
    right; y_is_zero = 1 on a zeroed y; y inside a larger buffer whose guard elements stay as they were."""
    from gan2shape_amd import lib
    c = cc.CONV_BY_NAME[name]
    dt = cc.conv_data(name)
    x, w, bias = dev(dt["x"]), dev(dt["w"]), dev(dt["bias"])
    shape = (c.B, c.groups * c.M) + c.out_hw
    for promise, fill in ((0, float("nan")), (1, 0.0)):
        buf, y = guarded(shape, fill)
        with tuned(g2s, c.tile, c.sk, c.det):
            lib.check(c_conv(g2s, c, x, w, bias, y, promise))
        _check(name, f"y y_is_zero={promise}", _path(c, c.plan()), y.cpu().numpy(), dt["ref"], dt["e32"], dt["cap"],
               ratio=cc.conv_ratio(c.plan()))
        assert guards_intact(buf), (name, promise)


@pytest.mark.parametrize("name", cc.ON_DEVICE)
def test_conv2d_plan_holds_on_the_device(g2s, name):
    """y filled with a constant and y_is_zero = 1: a class the plan calls split (float atomics) returns ref + c, one it
    calls plain overwrites (ref), holes still hold c.  This is what ties plan_conv's cls_splitk and needs-zero to the
    library's own decisions."""
    from gan2shape_amd import lib
    c = cc.CONV_BY_NAME[name]
    assert c.ep is None
    dt = cc.conv_data(name)
    const = 1.5
    pl = c.plan()
    step = c.s if c.adj else 1
    want = np.full(dt["ref"].shape, np.nan)
    for cl, atomic in zip(pl["classes"], pl["atomic"]):
        sl = (Ellipsis, slice(cl["oy0"], None, step), slice(cl["ox0"], None, step))
        want[sl] = dt["ref"][sl] + (const if atomic else 0.0)
    for oy0, ox0 in pl["holes"]:
        want[..., oy0::step, ox0::step] = const
    assert np.isfinite(want).all()
    _, y = guarded(want.shape, const)
    with tuned(g2s, c.tile, c.sk, c.det):
        lib.check(c_conv(g2s, c, dev(dt["x"]), dev(dt["w"]), None, y, 1))
    y = y.cpu().numpy()
    err = np.abs(y.astype(np.float64) - want)
    # every slice's atomic add rounds at the size of c + |ref|
    bound = cc.bound(dt["ref"], dt["e32"], dt["cap"], cc.conv_ratio(pl)) + max(pl["cls_splitk"]) * cc.EPS32 * (const + np.abs(dt["ref"]))
    off = np.abs(y.astype(np.float64) - dt["ref"])
    print(f"{name}: classes {[(cl['T'], s) for cl, s in zip(pl['classes'], pl['cls_splitk'])]} holes {pl['holes']}: "
          f"worst error / bound {float((err / bound).max()):.2f}; elements at ref + c: {int((off > 0.5 * const).sum())}")
    assert (err <= bound).all(), (name, pl["cls_splitk"], pl["holes"], int((err > bound).sum()),
                                  np.unravel_index(np.argmax(err - bound), err.shape))
    assert pl["needs_zero"] == bool(any(pl["atomic"]) or pl["holes"])


@pytest.mark.parametrize("name", cc.DETERMINISTIC)
def test_conv2d_deterministic_mode_is_the_unsplit_launch(g2s, name):
    """Under the deterministic flag a launch that would split equals the forced split-K 1 launch of the same tile bit
    for bit, twice, and meets the bound."""
    c = cc.CONV_BY_NAME[name]
    dt = cc.conv_data(name)
    x, w, bias = dev(dt["x"]), dev(dt["w"]), dev(dt["bias"])
    assert c.plan(det=False)["splitk"] > 1
    pl = c.plan(det=True)
    assert pl["splitk"] == 1
    with tuned(g2s, c.tile, c.sk, True):
        first = launch_conv(g2s, c, x, w, bias)
        second = launch_conv(g2s, c, x, w, bias)
    with tuned(g2s, pl["pick"], 1, False):
        unsplit = launch_conv(g2s, c, x, w, bias)
    assert torch.equal(first, second) and torch.equal(first, unsplit), name
    _check(name, "y deterministic", _path(c, pl) + "/det", first.cpu().numpy(), dt["ref"], dt["e32"], dt["cap"],
           ratio=cc.conv_ratio(pl))


def test_conv2d_rejects_the_5x5_stride_2_scatter_and_supported_refuses_it(g2s):
    c = cc.Conv("reject", 1, 3, 4, 6, 7, 5, 2, 2, 1)
    with pytest.raises(cc.Rejected):
        c.plan()
    x = torch.randn(1, 3, 6, 7, device="cuda")
    w = torch.randn(3, 4, 5, 5, device="cuda")
    y = torch.full((1, 4) + c.out_hw, float("nan"), device="cuda")
    with tuned(g2s):
        rc = c_conv(g2s, c, x, w, None, y, 0)
    assert rc != 0 and b"tap count" in g2s.g2s_last_error()
    torch.cuda.synchronize()
    assert bool(torch.isnan(y).all())
    from gan2shape_amd.op.conv import supported
    assert not supported(torch.nn.ConvTranspose2d(3, 4, 5, 2, 2), x) and not supported(torch.nn.Conv2d(3, 4, 5, 2, 2), x)
    assert supported(torch.nn.Conv2d(3, 4, 5, 1, 2), x) and supported(torch.nn.ConvTranspose2d(3, 4, 4, 2, 1), x)


# ---------------------------------------------------------------------------------------------- g2s_conv2d_wgrad
def _wpath(c, pl):
    return f"wgrad/{'split' if pl['split'] > 1 else 'plain'}{'/det' if c.det else ''}"


@pytest.mark.parametrize("name", [c.name for c in cc.WGRAD])
def test_wgrad_vs_float64(g2s, name):
    from gan2shape_amd.op.conv import _wgrad
    c = cc.WGRAD_BY_NAME[name]
    dt = cc.wgrad_data(name)
    with tuned(g2s, det=c.det):
        dw = _wgrad(dev(dt["A"]), dev(dt["G"]), c.k, c.s, c.p, None, c.groups).cpu().numpy()
    _check(name, "dw", _wpath(c, c.plan()), dw, dt["ref"], dt["e32"], dt["cap"], ratio=cc.wgrad_ratio(c.det))


def c_wgrad(L, c, A, G, dw, dw_is_zero):
    from gan2shape_amd import lib
    return L.g2s_conv2d_wgrad(lib.ptr(A), lib.ptr(G), lib.ptr(dw), c.B, c.Ca, c.Cg, c.PH, c.PW, c.GH, c.GW, c.k, c.s, c.p,
                              int(dw_is_zero), c.groups, lib.stream())


@pytest.mark.parametrize("name", cc.WGRAD_PROMISE)
def test_wgrad_output_promises_and_guards(g2s, name):
    from gan2shape_amd import lib
    c = cc.WGRAD_BY_NAME[name]
    dt = cc.wgrad_data(name)
    A, G = dev(dt["A"]), dev(dt["G"])
    for promise, fill in ((0, float("nan")), (1, 0.0)):
        buf, dw = guarded(dt["ref"].shape, fill)
        with tuned(g2s, det=c.det):
            lib.check(c_wgrad(g2s, c, A, G, dw, promise))
        _check(name, f"dw dw_is_zero={promise}", _wpath(c, c.plan()), dw.cpu().numpy(), dt["ref"], dt["e32"], dt["cap"],
               ratio=cc.wgrad_ratio(c.det))
        assert guards_intact(buf), (name, promise)


# ------------------------------------------------------------------------------------------------ g2s_conv2d_bwd
def _bpath(c, pl):
    return f"bwd/{'one-grid' if pl['one_grid'] else 'two-launch'}/tile{pl['pick']}/{'split' if pl['splitk'] > 1 else 'plain'}"


def _bwd_check(c, dt, gx, dw, what=""):
    pl = c.plan()
    _check(c.name, "gx" + what, _bpath(c, pl), gx.cpu().numpy(), dt["gx_ref"], dt["gx_e32"], dt["gx_cap"],
           ratio=cc.conv_ratio(pl))
    _check(c.name, "dw" + what, _bpath(c, pl) + "/" + _wpath(c.wgrad, c.wgrad.plan()), dw.cpu().numpy(), dt["dw_ref"],
           dt["dw_e32"], dt["dw_cap"], ratio=cc.wgrad_ratio(c.det))


@pytest.mark.parametrize("name", [c.name for c in cc.BWD])
def test_bwd_vs_float64(g2s, name):
    from gan2shape_amd.op.conv import _conv_bwd_raw
    c = cc.BWD_BY_NAME[name]
    dt = cc.bwd_data(name)
    with tuned(g2s, c.tile, c.sk, c.det):
        gx, dw = _conv_bwd_raw(dev(dt["gy"]), dev(dt["w"]), dev(dt["x"]), c.cin, c.cout, c.k, c.s, c.p, c.transposed,
                               None, None, c.groups)
    assert gx.shape == dt["x"].shape and dw.shape == dt["w"].shape
    _bwd_check(c, dt, gx, dw)


@pytest.mark.parametrize("name", cc.BWD_PROMISE)
def test_bwd_output_promises_and_guards(g2s, name):
    from gan2shape_amd import lib
    c = cc.BWD_BY_NAME[name]
    d, wg = c.dgrad, c.wgrad
    dt = cc.bwd_data(name)
    x, w, gy = dev(dt["x"]), dev(dt["w"]), dev(dt["gy"])
    A, G = (x, gy) if c.transposed else (gy, x)
    for promise, fill in ((0, float("nan")), (1, 0.0)):
        bx, gx = guarded(dt["x"].shape, fill)
        bw, dw = guarded(dt["w"].shape, fill)
        with tuned(g2s, c.tile, c.sk, c.det):
            lib.check(g2s.g2s_conv2d_bwd(lib.ptr(gy), lib.ptr(w), lib.ptr(gx), d.B, d.Cr, d.M, d.H, d.W, d.k, d.s, d.p, d.adj,
                                         d.mm, c.H if d.adj else 0, c.W if d.adj else 0, promise, lib.ptr(A), lib.ptr(G),
                                         lib.ptr(dw), wg.Ca, wg.Cg, wg.PH, wg.PW, wg.GH, wg.GW, promise, c.groups,
                                         lib.stream()))
        _bwd_check(c, dt, gx, dw, f" *_is_zero={promise}")
        assert guards_intact(bx) and guards_intact(bw), (name, promise)


@pytest.mark.parametrize("name", cc.BWD_DETERMINISTIC)
def test_bwd_deterministic_mode_equals_the_stand_alone_launches(g2s, name):
    from gan2shape_amd.op.conv import _conv2d_raw, _conv_bwd_raw, _wgrad
    c = cc.BWD_BY_NAME[name]
    d = c.dgrad
    dt = cc.bwd_data(name)
    x, w, gy = dev(dt["x"]), dev(dt["w"]), dev(dt["gy"])
    A, G = (x, gy) if c.transposed else (gy, x)
    pick = c.plan(det=True)["pick"]
    with tuned(g2s, c.tile, c.sk, True):
        gx, dw = _conv_bwd_raw(gy, w, x, c.cin, c.cout, c.k, c.s, c.p, c.transposed, None, None, c.groups)
        gx2, dw2 = _conv_bwd_raw(gy, w, x, c.cin, c.cout, c.k, c.s, c.p, c.transposed, None, None, c.groups)
    with tuned(g2s, pick, 1, True):
        gx_alone = _conv2d_raw(gy, w, None, d.Cr, d.M, d.k, d.s, d.p, d.adj, d.mm, (c.H, c.W), False, 0.0, groups=c.groups)
        dw_alone = _wgrad(A, G, c.k, c.s, c.p, None, c.groups)
    assert torch.equal(gx, gx2) and torch.equal(dw, dw2), name
    assert torch.equal(gx, gx_alone) and torch.equal(dw, dw_alone), name
    _check(name, "gx deterministic", "bwd/det", gx.cpu().numpy(), dt["gx_ref"], dt["gx_e32"], dt["gx_cap"],
           ratio=cc.conv_ratio(c.plan(det=True)))
    _check(name, "dw deterministic", "bwd/det/wgrad/plain/det", dw.cpu().numpy(), dt["dw_ref"], dt["dw_e32"], dt["dw_cap"],
           ratio=cc.wgrad_ratio(True))
