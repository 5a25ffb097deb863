"""-m gpu: g2s_conv3x3_wino (F(2x2)) and g2s_conv3x3_wino4 (F(4x4)) on every launch path against float64, element by element.

The tables, the plans, the reference and the bound are those of tests/wino_cases.py.  Every launch goes through the C
entry points (g2s_wino_weights + g2s_conv3x3_wino, g2s_wino4_weights + g2s_conv3x3_wino4), so that the test owns y, the
workspace and U: each is the 16-byte aligned interior of a larger buffer with sentinel guard bands, y and the workspace
start as NaN, and the workspace has exactly the floats the planned path needs (one fewer in the ws-small rows).  Every
launch runs under a time limit of its own (a watchdog that ends the process), prints its error, e32w and their ratio, and
every test restores the deterministic flag and the module globals it touched."""
import contextlib
import faulthandler

import numpy as np
import pytest
import torch

import conv2d_cases as cc
import wino_cases as wc

pytestmark = pytest.mark.gpu

GUARD = 256         # floats on either side of a buffer's interior (1 KiB: the interior keeps the allocation's alignment)
SENTINEL = 3.25
LAUNCH_SECONDS = 60
NAN = float("nan")


@pytest.fixture(scope="module")
def g2s():
    import gan2shape_amd  # noqa: F401
    from gan2shape_amd import lib
    return lib.load()  # fails loudly if libg2s.so is missing


@contextlib.contextmanager
def time_limit(seconds=LAUNCH_SECONDS):
    """A launch that does not come back ends the process with a traceback instead of holding the device."""
    faulthandler.dump_traceback_later(seconds, exit=True)
    try:
        yield
    finally:
        faulthandler.cancel_dump_traceback_later()


@contextlib.contextmanager
def deterministic(on):
    from gan2shape_amd import lib
    prev = lib.set_deterministic(on)
    try:
        yield
    finally:
        lib.set_deterministic(prev)


def dev(a):
    return None if a is None else torch.from_numpy(np.array(a)).cuda()     # a copy: the case data is read-only


def guarded(n, fill):
    """n floats that are the interior of a larger buffer: (buffer, view)."""
    buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
    view = buf[GUARD:GUARD + n]
    view.fill_(fill)
    assert view.data_ptr() % 16 == 0
    return buf, view


def guards_intact(buf):
    return bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[-GUARD:] == SENTINEL).all())


class Launch:
    """The device operands of one row; run() makes one call and returns its code."""

    def __init__(self, L, c, dt):
        from gan2shape_amd import lib
        self.L, self.c, self.lib = L, c, lib
        self.x, self.w = dev(dt["x"]), dev(dt["w"])
        self.in_scale, self.out_scale = dev(dt["in_scale"]), dev(dt["out_scale"])
        has_bias, act, has_noise = c.ep if c.ep is not None else (False, False, False)
        self.bias = dev(dt["bias"]) if has_bias else None
        self.noise = dev(dt["noise"]) if has_noise else None
        self.noise_w = torch.tensor([wc.NOISE_W], dtype=torch.float32, device="cuda") if has_noise else None
        self.act = int(act)
        floats, transform = ((L.g2s_wino4_weights_floats, L.g2s_wino4_weights) if c.kind == 4
                             else (L.g2s_wino_weights_floats, L.g2s_wino_weights))
        self.ubuf, self.U = guarded(floats(c.M, c.Cr), NAN)
        cout, cin = dt["w"].shape[:2]
        with time_limit():
            lib.check(transform(lib.ptr(self.w), lib.ptr(self.U), cout, cin, int(c.tr), lib.stream()))
            torch.cuda.synchronize()
        assert bool(torch.isfinite(self.U).all()) and guards_intact(self.ubuf), (c.name, "U")
        self.ybuf = self.y = self.wsbuf = self.ws = None

    def run(self, sk=None, y_fill=NAN, ws=None):
        """ws: None: a guarded workspace of the row's own size (or none); else (pointer, floats) of the caller's."""
        c, lib = self.c, self.lib
        sk = c.sk if sk is None else sk
        self.ybuf, y = guarded(c.y_floats, y_fill)
        self.y = y.view(c.B, c.M, c.H, c.W)
        if ws is None:
            n = c.ws_floats(sk)
            self.wsbuf, self.ws = (None, None) if n is None else guarded(n, NAN)
            ws = (lib.ptr(self.ws), 0 if n is None else n)
        entry = self.L.g2s_conv3x3_wino4 if c.kind == 4 else self.L.g2s_conv3x3_wino
        p = lib.ptr
        with time_limit():
            rc = entry(p(self.x), p(self.U), p(self.in_scale), p(self.out_scale), p(self.bias), p(self.noise), p(self.noise_w),
                       p(self.y), c.B, c.Cr, c.M, c.H, c.W, self.act, wc.ALPHA, wc.GAIN, int(sk), ws[0], ws[1], lib.stream())
            torch.cuda.synchronize()
        return rc

    def intact(self):
        return guards_intact(self.ybuf) and guards_intact(self.ubuf) and (self.wsbuf is None or guards_intact(self.wsbuf))


def _check(name, path, got, dt, slack=0.0):
    ref, e32w, cap = dt["ref"], dt["e32w"], dt["cap"]
    ratio = wc.ratio_of(path)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    assert np.isfinite(got).all(), (name, path, "not finite", int((~np.isfinite(got)).sum()),
                                    np.unravel_index(np.argmax(~np.isfinite(got)), got.shape))
    err = np.abs(got.astype(np.float64) - ref)
    scale = np.abs(ref).max()
    bound = wc.bound(ref, e32w, cap, ratio) + slack
    ratio_e32 = err.max() / scale / cc.floor_e32(e32w)
    print(f"RATIO {path} {name}: error {err.max() / scale:.3e} of max|ref|, e32w {e32w:.3e}, ratio {ratio_e32:.2f} of {ratio:g}, "
          f"worst error / bound {float((err / np.maximum(bound, 1e-300)).max()):.2f}, "
          f"worst error / cap {float((err / np.maximum(cap + slack, 1e-300)).max()):.3f}")
    assert (err <= bound).all(), (f"{name} [{path}]: {int((err > bound).sum())} of {err.size} elements over the bound, "
                                  f"first at {np.unravel_index(np.argmax(err - bound), err.shape)}, {ratio_e32:.2f} x e32w")


def _vs_float64(g2s, name):
    c = wc.BY_NAME[name]
    dt = wc.data(name)
    with deterministic(c.det):
        run = Launch(g2s, c, dt)
        run.lib.check(run.run())
    _check(name, wc.path_of(c), run.y.cpu().numpy(), dt)
    assert run.intact(), (name, "guards of y, ws or U")


@pytest.mark.parametrize("name", [c.name for c in wc.WINO])
def test_wino_vs_float64(g2s, name):
    _vs_float64(g2s, name)


@pytest.mark.parametrize("name", [c.name for c in wc.WINO4])
def test_wino4_vs_float64(g2s, name):
    _vs_float64(g2s, name)


@pytest.mark.parametrize("name", wc.ON_DEVICE)
def test_wino_plan_holds_on_the_device(g2s, name):
    """y pre-filled with a constant: the library clears y itself where partial sums meet by atomics, so every path
    returns ref.  What ties the plan to the library is the workspace: on a workspace path exactly the planned floats of
    the NaN-filled workspace change (every slice of a split-K launch; the slots of the split tiles of a stream-K one)
    and none beyond; on an atomic or whole-tile path a workspace that was passed stays untouched."""
    c = wc.BY_NAME[name]
    assert c.ep is None
    dt = wc.data(name)
    p = c.plan()
    with deterministic(c.det):
        run = Launch(g2s, c, dt)
        run.lib.check(run.run(y_fill=1.5))
    # every slice's atomic add rounds at the size of the running sum
    slack = (max(p.get("slices", 0), 1) * cc.EPS32 * np.abs(dt["ref"])) if p.get("clears_y") else 0.0
    _check(name, wc.path_of(c) + "/prefilled", run.y.cpu().numpy(), dt, slack)
    assert run.intact(), name
    if run.ws is not None:
        changed = torch.isfinite(run.ws)
        n = int(changed.sum())
        print(f"{name}: mode {p['mode']}, uses_ws {p['uses_ws']}, workspace floats changed {n} of {run.ws.numel()}, planned {p['ws_written']}")
        assert n == p["ws_written"], (name, n, p["ws_written"])
        if p["uses_ws"] and p["mode"] == "splitk":
            assert n == p["slices"] * c.y_floats == run.ws.numel()
        if not p["uses_ws"]:
            assert n == 0
    else:
        assert not p["uses_ws"], name


@pytest.mark.parametrize("name", wc.DET_FALLBACK + wc.DET_KEEPS)
def test_wino_deterministic(g2s, name):
    """Under the deterministic flag a launch whose plan would meet by atomics equals the forced whole-tile launch bit for
    bit, twice; a workspace split-K or stream-K launch repeats bit for bit; all meet the bound."""
    c = wc.BY_NAME[name]
    dt = wc.data(name)
    run = Launch(g2s, c, dt)
    with deterministic(True):
        run.lib.check(run.run())
        first = run.y.clone()
        run.lib.check(run.run())
        second = run.y.clone()
        assert run.intact(), name
    assert torch.equal(first, second), name
    p = c.plan(det=True)
    if name in wc.DET_FALLBACK:
        assert c.plan(det=False)["clears_y"] and p["det_fallback"]
        with deterministic(False):
            run.lib.check(run.run(sk=1))
        assert torch.equal(first, run.y), name
    else:
        assert p["det_keeps_ws"] and p["uses_ws"]
    _check(name, "wino/det", first.cpu().numpy(), dt)


def test_wino4_is_order_fixed(g2s):
    """No atomics on any path of the F(4x4) kernel: every partition repeats bit for bit."""
    for c in wc.WINO4:
        run = Launch(g2s, c, wc.data(c.name))
        run.lib.check(run.run())
        first = run.y.clone()
        run.lib.check(run.run())
        assert torch.equal(first, run.y) and bool(torch.isfinite(first).all()), c.name


def test_wino4_supported_table_and_rejection(g2s):
    for shape, want in wc.SUPPORTED.items():
        assert g2s.g2s_wino4_supported(*shape) == want, shape
    B, Cr, M, H, W = 1, 8, 64, 16, 16                   # 16 tiles per image
    assert wc.SUPPORTED[(B, Cr, M, H, W)] == 0
    from gan2shape_amd import lib
    for entry, shape, word in ((g2s.g2s_conv3x3_wino4, (B, Cr, M, H, W), b"not supported"),
                               (g2s.g2s_conv3x3_wino, (1, 8, 64, 1, 16), b"H, W >= 2")):
        B, Cr, M, H, W = shape
        x = torch.randn(B, Cr, H, W, device="cuda")
        U = torch.zeros(max(int(g2s.g2s_wino4_weights_floats(M, Cr)), int(g2s.g2s_wino_weights_floats(M, Cr))), device="cuda")
        ybuf, y = guarded(B * M * H * W, NAN)
        with time_limit():
            rc = entry(lib.ptr(x), lib.ptr(U), None, None, None, None, None, lib.ptr(y), B, Cr, M, H, W, 0, 0.0, 1.0, 1, None, 0,
                       lib.stream())
            torch.cuda.synchronize()
        assert rc != 0 and word in g2s.g2s_last_error(), (shape, rc, g2s.g2s_last_error())
        assert bool(torch.isnan(y).all()) and guards_intact(ybuf), shape


@pytest.mark.parametrize("name,force", wc.DISPATCH)
def test_wino_dispatch_agrees_with_entry_points(g2s, name, force):
    """modconv.py's launch site under WINO_FORCE returns, bit for bit, what the direct entry-point launch of the same
    partition with the same workspace returns: the module's launches are the ones the other tests cover."""
    from gan2shape_amd import lib
    from gan2shape_amd import modconv as mc
    c = wc.BY_NAME[name]
    dt = wc.data(name)
    sk = int(force[3:]) if isinstance(force, str) else int(force)
    run = Launch(g2s, c, dt)
    saved = (mc.WINOGRAD, mc.WINO_FORCE, mc.WINO4)
    try:
        mc.WINOGRAD, mc.WINO_FORCE, mc.WINO4 = True, force, True
        assert mc.wino_choice(run.x, run.w, mc.PLAIN, int(c.tr), int(c.ep is not None)) == force
        with time_limit():
            if c.ep is None:
                y = mc.modconv_raw(run.x, run.w, run.in_scale, run.out_scale, mc.PLAIN, int(c.tr))
            else:
                assert c.ep == (True, True, True) and not c.tr
                y = mc.modconv_nba_raw(run.x, run.w, run.in_scale, run.out_scale, run.bias, run.noise.view(1, 1, c.H, c.W),
                                       run.noise_w, wc.ALPHA, wc.GAIN)
            torch.cuda.synchronize()
    finally:
        mc.WINOGRAD, mc.WINO_FORCE, mc.WINO4 = saved
    lib.check(run.run(sk=sk, ws=lib.split_ws()))
    assert y.shape == run.y.shape and torch.equal(y, run.y), (name, force)
    assert run.intact(), name
    _check(name, "dispatch/" + wc.path_of(c), y.cpu().numpy(), dt)
