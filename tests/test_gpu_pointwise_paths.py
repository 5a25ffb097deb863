"""-m gpu: the pointwise entry points of csrc/fused_bias_act.hip (and g2s_noise_bias_act_ps of csrc/synth_batch.hip)
on their vector and scalar kernels, with misaligned pointers and second grid-stride turns, bit for bit against the
expectations of tests/pointwise_cases.py (described there).

The entry points are called through the C ABI: every tensor is a view into a larger, 16-byte aligned buffer filled
with a canary value — four elements in when it is to be aligned (eight for float16), one float further when it is
not — and everything outside the views must be unchanged afterwards, inputs included."""
import numpy as np
import pytest
import torch

import pointwise_cases as pc

pytestmark = pytest.mark.gpu
CANARY = 1024.0
MARGIN = 16


@pytest.fixture(scope="module")
def g2s():
    import gan2shape_amd  # noqa: F401
    from gan2shape_amd import lib
    return lib.load()  # fails loudly if libg2s.so is missing


class Buffers:
    def __init__(self, case):
        self.case, self.held = case, []

    def view(self, key, arr=None, like=None):
        """A device view holding `arr` (or uninitialised room for an output shaped like `like`), aligned or not as the
        case says for `key`; None stays None."""
        if arr is None and like is None:
            return None
        src = like if arr is None else arr
        n, dtype = src.size, torch.float16 if src.dtype == np.float16 else torch.float32
        buf = torch.full((n + 2 * MARGIN,), CANARY, dtype=dtype, device="cuda")
        assert buf.data_ptr() % 16 == 0
        off = 16 // buf.element_size() + (1 if key in self.case["mis"] else 0)
        v = buf[off:off + n]
        assert (v.data_ptr() % 16 != 0) == (key in self.case["mis"])
        if arr is not None:
            v.copy_(torch.from_numpy(np.array(arr).reshape(-1)))     # a copy: the case data is read-only
        self.held.append((key, buf, off, n, None if arr is None else buf.clone()))
        return v

    def check(self):
        for key, buf, off, n, before in self.held:
            if before is None:      # an output: the canaries around it
                assert (buf[:off] == CANARY).all() and (buf[off + n:] == CANARY).all(), f"{key}: canary overwritten"
            else:                   # an input: all of it (NaN compares as bits)
                assert torch.equal(buf.view(torch.uint8), before.view(torch.uint8)), f"{key}: input changed"


def _run(g2s, name):
    from gan2shape_amd import lib
    c, d = pc.CASE[name], pc.inputs(name)
    bufs = Buffers(c)
    e, st = c["entry"], lib.stream()
    if e == "fba":
        x, bias, ref = bufs.view("x", d["x"]), bufs.view("bias", d["bias"]), bufs.view("ref", d["ref"])
        y = bufs.view("y", like=d["x"])
        N, C, HW = c["shape"]
        rc = g2s.g2s_fused_bias_act(lib.ptr(x), lib.ptr(bias), lib.ptr(ref), lib.ptr(y), N * C * HW, HW, C, c["act"], c["grad"],
                                    pc.ALPHA, pc.SCALE, lib.G2S_F16 if c.get("f16") else lib.G2S_F32, st)
        shape = c["shape"]
    elif e in ("nba", "nba_ps"):
        x, noise, bias = bufs.view("x", d["x"]), bufs.view("noise", d["noise"]), bufs.view("bias", d["bias"])
        nw = bufs.view("nw", np.array([d["nw"]], np.float32))
        y = bufs.view("y", like=d["x"])
        fn = g2s.g2s_noise_bias_act if e == "nba" else g2s.g2s_noise_bias_act_ps
        rc = fn(lib.ptr(x), lib.ptr(noise), lib.ptr(nw), lib.ptr(bias), lib.ptr(y), 2, 3, c["hw"], pc.ALPHA, pc.SCALE, st)
        shape = d["x"].shape
    elif e == "clamp":
        x, g, y = bufs.view("x", d["x"]), bufs.view("g", d["g"]), bufs.view("y", like=d["x"])
        rc = g2s.g2s_clamp(lib.ptr(x), lib.ptr(g), lib.ptr(y), c["n"], pc.LO, pc.HI, c["backward"], st)
        shape = d["x"].shape
    else:
        a, b, bias = bufs.view("a", d["a"]), bufs.view("b", d["b"]), bufs.view("bias", d["bias"])
        y = bufs.view("y", like=d["a"])
        N, C, HW = c["shape"]
        rc = g2s.g2s_add_bias_scale(lib.ptr(a), lib.ptr(b), lib.ptr(bias), lib.ptr(y), N * C * HW, HW, C, pc.SCALE, st)
        shape = c["shape"]
    lib.check(rc)
    torch.cuda.synchronize()
    bufs.check()
    return y.cpu().numpy().reshape(shape)


@pytest.mark.parametrize("name", pc.NAMES)
def test_pointwise_path_bit_exact(g2s, name):
    c = pc.CASE[name]
    got = _run(g2s, name)
    exp = pc.expected(name)
    assert got.dtype == exp[0].dtype and got.shape == exp[0].shape
    if len(exp) == 1:
        np.testing.assert_array_equal(got, exp[0], err_msg=f"{name} {pc.dispatch(c)}")
        return
    ok = np.zeros(got.shape, bool)
    for e in exp:       # the two-rounding sum or the fma, element by element
        ok |= got == e
    print(f"{name}: {int((got != exp[0]).sum())} of {got.size} elements took the fma candidate")
    assert ok.all(), (name, pc.dispatch(c), int((~ok).sum()), np.argwhere(~ok)[:4])


def test_fused_bias_act_with_n_zero_touches_nothing(g2s):
    from gan2shape_amd import lib
    x = torch.full((64,), CANARY, device="cuda")
    y, b = x.clone(), x.clone()
    lib.check(g2s.g2s_fused_bias_act(lib.ptr(x), lib.ptr(b), None, lib.ptr(y), 0, 4, 3, 3, 0, pc.ALPHA, pc.SCALE, lib.G2S_F32,
                                     lib.stream()))
    lib.check(g2s.g2s_fused_bias_act(None, None, None, None, 0, 0, 0, 3, 0, pc.ALPHA, pc.SCALE, lib.G2S_F32, lib.stream()))
    torch.cuda.synchronize()
    for t in (x, y, b):
        assert (t == CANARY).all()
