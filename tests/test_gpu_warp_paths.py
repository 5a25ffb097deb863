"""-m gpu: g2s_grid_sample_fwd / _bwd (csrc/grid_sample.hip) through the C ABI against the float64 reference of
tests/warp_cases.py (cases, reference and bounds are described there): clamp on and off, either output NULL, float
atomics and the fixed-point scatter of deterministic mode, acc_is_zero, a workspace that is not 256-byte aligned, pixels
on texels, on the limits of the grid and with no in-range corner (non-finite coordinates included).

Every tensor is a view into a canary-filled buffer: inputs must be unchanged and the canaries around the outputs (and
beyond workspace_bytes) intact.  Refusals are checked by return code, with canaries where an output would be."""
import ctypes

import numpy as np
import pytest
import torch

import warp_cases as wc
from canary_buffers import CANARY, Buffers, within

pytestmark = pytest.mark.gpu
WS_FILL = 0xA5
RATIO = {}


@pytest.fixture(scope="module")
def g2s():
    import gan2shape_amd  # noqa: F401
    from gan2shape_amd import lib
    return lib.load()  # fails loudly if libg2s.so is missing


def _note(key, r):
    RATIO[key] = max(RATIO.get(key, 0.0), r)


class Workspace:
    """`nbytes` bytes handed in 256 + off bytes into a byte buffer filled with WS_FILL (garbage for the kernel, canary
    for the test); zero=True clears the handed part, as acc_is_zero = 1 promises."""

    def __init__(self, nbytes, off=0, zero=False):
        self.raw = torch.full((nbytes + 512 + 16,), WS_FILL, dtype=torch.uint8, device="cuda")
        assert self.raw.data_ptr() % 16 == 0
        self.lo, self.hi, self.nbytes = 256 + off, 256 + off + nbytes, nbytes
        if zero:
            self.raw[self.lo:self.hi] = 0
        self.ptr = ctypes.c_void_p(self.raw.data_ptr() + self.lo)
        assert self.ptr.value % 16 == off

    def check(self, untouched=False):
        assert (self.raw[:self.lo] == WS_FILL).all() and (self.raw[self.hi:] == WS_FILL).all(), "workspace canary"
        if untouched:
            assert (self.raw == WS_FILL).all(), "workspace written although gx is NULL"


def _forward(g2s, name):
    from gan2shape_amd import lib
    c, d = wc.CASE[name], wc.inputs(name)
    B, C, ih, iw, H, W = c["shape"]
    bufs = Buffers()
    x, grid = bufs.view("x", d["x"]), bufs.view("grid", d["grid"])
    y = bufs.view("y", like=np.empty((B, C, H, W)))
    lib.check(g2s.g2s_grid_sample_fwd(lib.ptr(x), lib.ptr(grid), lib.ptr(y), B, C, ih, iw, H, W, c["clamp"], c["lo"], c["hi"],
                                      lib.stream()))
    torch.cuda.synchronize()
    bufs.check()
    return y.cpu().numpy().reshape(B, C, H, W)


def _backward(g2s, name):
    """One call; deterministic mode is the caller's to set.  (gx, ggrid) as numpy, None for a NULL output."""
    from gan2shape_amd import lib
    c, d = wc.CASE[name], wc.inputs(name)
    B, C, ih, iw, H, W = c["shape"]
    bufs = Buffers()
    gy, x, grid = bufs.view("gy", d["gy"]), bufs.view("x", d["x"]), bufs.view("grid", d["grid"])
    pre = 0.0 if c["acc_is_zero"] else 7.5          # acc_is_zero = 0: garbage the callee has to clear
    gx = bufs.view("gx", like=d["x"], fill=pre) if c["gx"] else None
    ggrid = bufs.view("ggrid", like=d["grid"]) if c["ggrid"] else None
    if not c["gx"]:
        bufs.spare("gx (NULL)", d["x"])
    if not c["ggrid"]:
        bufs.spare("ggrid (NULL)", d["grid"])
    ws = Workspace(wc.workspace_bytes(B, C, ih, iw), c["ws_off"], zero=bool(c["acc_is_zero"])) if c["det"] else None
    if ws is not None and c["gx"]:      # the round-up to 256 bytes stays inside what was handed in
        fix = (ws.ptr.value + 255) & ~255
        assert fix + B * C * ih * iw * 8 <= ws.ptr.value + ws.nbytes
    lib.check(g2s.g2s_grid_sample_bwd(lib.ptr(gy), lib.ptr(x), lib.ptr(grid), lib.ptr(gx), lib.ptr(ggrid), B, C, ih, iw, H, W,
                                      c["clamp"], c["lo"], c["hi"], ws.ptr if ws else None, ws.nbytes if ws else 0,
                                      c["acc_is_zero"], lib.stream()))
    torch.cuda.synchronize()
    bufs.check()
    if ws is not None:
        ws.check(untouched=not c["gx"])
    return (None if gx is None else gx.cpu().numpy().reshape(B, C, ih, iw),
            None if ggrid is None else ggrid.cpu().numpy().reshape(B, H, W, 2))


@pytest.mark.parametrize("name", [c["name"] for c in wc.CASES if c["entry"] == "fwd"])
def test_warp_forward(g2s, name):
    e = wc.expected(name)
    y = _forward(g2s, name)
    dead = np.broadcast_to(~e["live"][:, None], y.shape)
    c = wc.CASE[name]
    zero = min(max(0.0, c["lo"]), c["hi"]) if c["clamp"] else 0.0
    assert (y[dead] == np.float32(zero)).all(), "a pixel with no in-range corner samples 0"
    r = within(y, e["y"], e["y_bound"], "y")
    _note("y", r)
    print(f"{name} {wc.dispatch(c)}: y error / bound {r:.3f}")


@pytest.mark.parametrize("name", [c["name"] for c in wc.CASES if c["entry"] == "bwd"])
def test_warp_backward(g2s, name):
    from gan2shape_amd import lib
    c, e = wc.CASE[name], wc.expected(name)
    prev = lib.set_deterministic(c["det"])
    try:
        gx, ggrid = _backward(g2s, name)
        again = _backward(g2s, name) if c["det"] else None
    finally:
        lib.set_deterministic(prev)
    msg = [f"{name} {wc.dispatch(c)}:"]
    if c["ggrid"]:
        dead = ~e["live"]
        bad = ~(ggrid[dead] == 0)
        assert not bad.any(), ("ggrid of pixels with no in-range corner must be (0, 0)", int(bad.sum()), ggrid[dead][bad.any(-1)][:6])
        r = within(ggrid, e["ggrid"], e["ggrid_bound"], "ggrid")
        _note("ggrid", r)
        msg.append(f"ggrid {r:.3f}")
    else:
        assert ggrid is None
    if c["gx"]:
        r = within(gx, e["gx"], e["gx_bound"], "gx")
        _note("gx fixed" if c["det"] else "gx float", r)
        msg.append(f"gx {r:.3f} (m up to {int(e['m'].max())})")
    else:
        assert gx is None
    if again is not None:       # deterministic mode: bit-identical from call to call
        for a, b in zip((gx, ggrid), again):
            assert (a is None) == (b is None)
            if a is not None:
                assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    print(" ".join(msg), "error / bound")


def test_workspace_bytes(g2s):
    f = g2s.g2s_grid_sample_bwd_workspace_bytes
    for B, C, ih, iw in ((2, 3, 5, 7), (1, 1, 2, 2), (8, 3, 128, 128)):
        assert f(B, C, ih, iw) == B * C * ih * iw * 8 + 256 == wc.workspace_bytes(B, C, ih, iw)
    for args in ((0, 3, 5, 7), (2, 0, 5, 7), (2, 3, -1, 7), (2, 3, 5, 0)):
        assert f(*args) == 0


def test_warp_refusals_launch_nothing(g2s):
    """By return code: IH = 1, B = 65536, both gradients NULL, and in deterministic mode a NULL or short workspace."""
    from gan2shape_amd import lib
    name = "bwd_both_det"
    c, d = wc.CASE[name], wc.inputs(name)
    B, C, ih, iw, H, W = c["shape"]
    bufs = Buffers()
    gy, x, grid = bufs.view("gy", d["gy"]), bufs.view("x", d["x"]), bufs.view("grid", d["grid"])
    y, gx, ggrid = (bufs.spare(k, a) for k, a in (("y", d["gy"]), ("gx", d["x"]), ("ggrid", d["grid"])))
    st = lib.stream()
    P = lib.ptr

    def fwd(B_=B, ih_=ih):
        return g2s.g2s_grid_sample_fwd(P(x), P(grid), P(y), B_, C, ih_, iw, H, W, 1, -1.0, 1.0, st)

    def bwd(gx_, gg_, ws=None, nbytes=0, B_=B, ih_=ih):
        return g2s.g2s_grid_sample_bwd(P(gy), P(x), P(grid), P(gx_), P(gg_), B_, C, ih_, iw, H, W, 1, -1.0, 1.0, ws, nbytes, 0, st)

    assert fwd(ih_=1) == -1 and fwd(B_=65536) == -1
    assert bwd(gx, ggrid, ih_=1) == -1 and bwd(gx, ggrid, B_=65536) == -1
    assert bwd(None, None) == -1
    need = wc.workspace_bytes(B, C, ih, iw)
    ws = Workspace(need)
    prev = lib.set_deterministic(True)
    try:
        assert bwd(gx, ggrid, None, need) == -3              # G2S_ERR_WORKSPACE
        assert bwd(gx, ggrid, ws.ptr, need - 1) == -3
        assert bwd(None, None, ws.ptr, need) == -1
    finally:
        lib.set_deterministic(prev)
    torch.cuda.synchronize()
    bufs.check()
    ws.check(untouched=True)
    for t in (y, gx, ggrid):
        assert (t == CANARY).all()


def test_largest_error_over_bound():
    """Runs last in this file: the figures recorded in the docstring of tests/warp_cases.py."""
    print("warp: largest error / bound", {k: round(v, 3) for k, v in sorted(RATIO.items())})
    assert all(v <= 1.0 for v in RATIO.values())
