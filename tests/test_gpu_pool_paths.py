"""-m gpu: g2s_res_split_fwd / _bwd, g2s_avg_pyramid and g2s_maxpool2x2_fwd / _bwd (csrc/pool.hip) through the C ABI,
bit for bit against the numpy float32 expectations of tests/pool_cases.py (described there): ragged last workgroups,
either gradient NULL, NaNs, zeros, ties, and a max-pool just past its grid cap.

Every tensor is a view into a canary-filled buffer: inputs must be unchanged and the canaries around the outputs intact;
a NULL operand has a spare canary buffer that must stay untouched.  Refusals — shapes, NULLs and pointers that are not
aligned for the float2 / float4 accesses — are checked by return code, and nothing may have been written."""
import ctypes

import numpy as np
import pytest
import torch

import pool_cases as pc
from canary_buffers import CANARY, Buffers

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def g2s():
    import gan2shape_amd  # noqa: F401
    from gan2shape_amd import lib
    return lib.load()  # fails loudly if libg2s.so is missing


def _equal(name, key, got, cands):
    """Bit for bit with one of the candidates, element by element (NaN equals NaN)."""
    assert got.dtype == cands[0].dtype and got.shape == cands[0].shape
    if len(cands) == 1:
        np.testing.assert_array_equal(got, cands[0], err_msg=f"{name} {key}")
        return
    ok = np.zeros(got.shape, bool)
    for e in cands:
        ok |= (got == e) | (np.isnan(got) & np.isnan(e))
    first = (got == cands[0]) | (np.isnan(got) & np.isnan(cands[0]))
    print(f"{name} {key}: {int((~first).sum())} of {got.size} elements took the fma candidate")
    assert ok.all(), (name, key, int((~ok).sum()), np.argwhere(~ok)[:4].tolist(), got[~ok][:4], cands[0][~ok][:4])


def _levels(ts):
    return (ctypes.c_void_p * 4)(*[None if t is None else t.data_ptr() for t in ts])


@pytest.mark.parametrize("name", pc.NAMES)
def test_pool_path_bit_exact(g2s, name):
    from gan2shape_amd import lib
    c, d, exp = pc.CASE[name], pc.inputs(name), pc.expected(name)
    P, H, W = c["shape"]
    e, st, ptr = c["entry"], lib.stream(), lib.ptr
    bufs = Buffers()
    x = bufs.view("x", d["x"])
    half = np.empty((P, H // 2, W // 2))
    if e == "split_fwd":
        out = dict(relu_out=bufs.view("relu_out", like=d["x"]), pool_out=bufs.view("pool_out", like=half))
        rc = g2s.g2s_res_split_fwd(ptr(x), ptr(out["relu_out"]), ptr(out["pool_out"]), P, H, W, st)
    elif e == "split_bwd":
        ga, gb = bufs.view("g_relu", d["g_relu"]), bufs.view("g_pool", d["g_pool"])
        if ga is None:
            bufs.spare("g_relu (NULL)", d["x"])
        if gb is None:
            bufs.spare("g_pool (NULL)", half)
        out = dict(gx=bufs.view("gx", like=d["x"]))
        rc = g2s.g2s_res_split_bwd(ptr(x), ptr(ga), ptr(gb), ptr(out["gx"]), P, H, W, st)
    elif e == "pyramid":
        out = {f"level{l}": bufs.view(f"level{l}", like=np.empty((P, H >> (l + 1), W >> (l + 1)))) for l in range(c["levels"])}
        for l in range(c["levels"], 4):
            bufs.spare(f"level{l} (NULL)", np.empty((P, max(H >> (l + 1), 1), max(W >> (l + 1), 1))))
        rc = g2s.g2s_avg_pyramid(ptr(x), _levels([out.get(f"level{l}") for l in range(4)]), c["levels"], P, H, W, st)
    elif e == "maxpool_fwd":
        out = dict(y=bufs.view("y", like=half))
        rc = g2s.g2s_maxpool2x2_fwd(ptr(x), ptr(out["y"]), P, H, W, st)
    else:
        gy = bufs.view("gy", d["gy"])
        out = dict(gx=bufs.view("gx", like=d["x"]))
        rc = g2s.g2s_maxpool2x2_bwd(ptr(x), ptr(gy), ptr(out["gx"]), P, H, W, st)
    lib.check(rc)
    torch.cuda.synchronize()
    bufs.check()
    assert set(out) == set(exp)
    for key, cands in exp.items():
        _equal(name, key, out[key].cpu().numpy().reshape(cands[0].shape), cands)
    print(f"{name} {pc.dispatch(c)}: bit for bit")


def _untouched(bufs, *spares):
    torch.cuda.synchronize()
    bufs.check()
    for t in spares:
        assert (t == CANARY).all()


def test_res_split_refusals_write_nothing(g2s):
    """Odd H, odd W, every NULL, and x / relu_out / g_relu / gx one float off the 8 bytes their float2 accesses need."""
    from gan2shape_amd import lib
    d = pc.inputs("split_bwd_both_3x4x6")
    P, H, W = 3, 4, 6
    bufs = Buffers()
    x, ga, gb = bufs.view("x", d["x"]), bufs.view("g_relu", d["g_relu"]), bufs.view("g_pool", d["g_pool"])
    x1, ga1 = bufs.view("x+1", d["x"], shift=1), bufs.view("g_relu+1", d["g_relu"], shift=1)
    r, p, gx = bufs.spare("relu_out", d["x"]), bufs.spare("pool_out", d["g_pool"]), bufs.spare("gx", d["x"])
    ptr, st = lib.ptr, lib.stream()
    off = lambda t: ctypes.c_void_p(t.data_ptr() + 4)
    fwd, bwd = g2s.g2s_res_split_fwd, g2s.g2s_res_split_bwd
    assert x.data_ptr() % 8 == 0 and x1.data_ptr() % 8 == 4
    for h, w in ((3, 6), (4, 5), (0, 6)):
        assert fwd(ptr(x), ptr(r), ptr(p), P, h, w, st) == -1
        assert bwd(ptr(x), ptr(ga), ptr(gb), ptr(gx), P, h, w, st) == -1
    assert fwd(None, ptr(r), ptr(p), P, H, W, st) == -1 and fwd(ptr(x), None, ptr(p), P, H, W, st) == -1
    assert fwd(ptr(x), ptr(r), None, P, H, W, st) == -1 and fwd(None, None, None, P, H, W, st) == -1
    assert bwd(ptr(x), None, None, ptr(gx), P, H, W, st) == -1 and bwd(None, ptr(ga), ptr(gb), ptr(gx), P, H, W, st) == -1
    assert bwd(ptr(x), ptr(ga), ptr(gb), None, P, H, W, st) == -1 and bwd(None, None, None, None, P, H, W, st) == -1
    # alignment: refused before the launch
    assert fwd(ptr(x1), ptr(r), ptr(p), P, H, W, st) == -1
    assert fwd(ptr(x), off(r), ptr(p), P, H, W, st) == -1
    assert bwd(ptr(x1), ptr(ga), ptr(gb), ptr(gx), P, H, W, st) == -1
    assert bwd(ptr(x), ptr(ga1), ptr(gb), ptr(gx), P, H, W, st) == -1
    assert bwd(ptr(x), ptr(ga), ptr(gb), off(gx), P, H, W, st) == -1
    _untouched(bufs, r, p, gx)


def test_avg_pyramid_refusals_write_nothing(g2s):
    from gan2shape_amd import lib
    d = pc.inputs("pyramid_2x16x32_l2")
    P, H, W = 2, 16, 32
    bufs = Buffers()
    x, x1 = bufs.view("x", d["x"]), bufs.view("x+1", d["x"], shift=1)
    lv = [bufs.spare(f"level{l}", np.empty((P, H >> (l + 1), W >> (l + 1)))) for l in range(4)]
    ptr, st = lib.ptr, lib.stream()
    f = g2s.g2s_avg_pyramid
    assert f(ptr(x), _levels(lv), 0, P, H, W, st) == -1 and f(ptr(x), _levels(lv), 5, P, H, W, st) == -1
    assert f(ptr(x), _levels(lv), 3, P, 12, W, st) == -1 and f(ptr(x), _levels(lv), 2, P, H, 30, st) == -1
    assert f(ptr(x), _levels([lv[0], None, lv[2], lv[3]]), 2, P, H, W, st) == -1
    assert f(None, _levels(lv), 2, P, H, W, st) == -1 and f(ptr(x), None, 2, P, H, W, st) == -1
    assert f(ptr(x1), _levels(lv), 2, P, H, W, st) == -1                 # x is read as float2
    _untouched(bufs, *lv)


def test_maxpool_refusals_write_nothing(g2s):
    from gan2shape_amd import lib
    d = pc.inputs("maxpool_bwd_3x6x16")
    P, H, W = 3, 6, 16
    bufs = Buffers()
    x, gy = bufs.view("x", d["x"]), bufs.view("gy", d["gy"])
    x1, gy1 = bufs.view("x+1", d["x"], shift=1), bufs.view("gy+1", d["gy"], shift=1)
    y, gx = bufs.spare("y", d["gy"]), bufs.spare("gx", d["x"])
    ptr, st = lib.ptr, lib.stream()
    off = lambda t: ctypes.c_void_p(t.data_ptr() + 4)
    fwd, bwd = g2s.g2s_maxpool2x2_fwd, g2s.g2s_maxpool2x2_bwd
    for h, w in ((6, 12), (3, 16)):
        assert fwd(ptr(x), ptr(y), P, h, w, st) == -1 and bwd(ptr(x), ptr(gy), ptr(gx), P, h, w, st) == -1
    assert fwd(ptr(x1), ptr(y), P, H, W, st) == -1 and fwd(ptr(x), off(y), P, H, W, st) == -1
    assert bwd(ptr(x1), ptr(gy), ptr(gx), P, H, W, st) == -1 and bwd(ptr(x), ptr(gy1), ptr(gx), P, H, W, st) == -1
    assert bwd(ptr(x), ptr(gy), off(gx), P, H, W, st) == -1 and bwd(ptr(x), None, ptr(gx), P, H, W, st) == -1
    _untouched(bufs, y, gx)
