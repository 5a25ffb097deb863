"""The case table of tests/pool_cases.py, without a GPU: the shapes reach the workgroup counts, ragged tails and second
turns they were chosen for, the inputs hold the zeros, NaNs, ties and -inf windows the cases are about, the ReLU
backward rule is torch's, and every float32 expectation is the rounding of its float64 restatement."""
import numpy as np
import pytest
import torch

import pool_cases as pc

F32 = np.float32


def test_shapes_reach_what_they_were_chosen_for():
    d = lambda n: pc.dispatch(pc.CASE[n])
    assert d("split_fwd_1x2x2") == dict(units=1, blocks=1, last=1, turns=1)
    assert d("split_fwd_3x4x6")["units"] == 18 and (6 // 2) % 2 == 1
    assert d("split_fwd_5x6x22")["units"] == 165
    assert d("split_bwd_both_4x16x18") == dict(units=288, blocks=2, last=32, turns=1)
    for s in ("1x2x2", "3x4x6", "5x6x22", "4x16x18"):
        assert {(c["g_relu"], c["g_pool"]) for c in pc.CASES if c["name"].startswith("split_bwd") and c["name"].endswith(s)} == \
            {(True, True), (False, True), (True, False)}
    assert [d(f"pyramid_2x16x32_l{l}")["units"] for l in (1, 2, 3, 4)] == [256, 64, 16, 4]
    assert d("pyramid_65x4x4_l2") == dict(units=65, blocks=2, last=1, turns=1)      # a second workgroup with one live lane
    assert d("pyramid_1x2x2_l1")["units"] == 1 and d("pyramid_3x8x24_l3")["units"] == 9
    big = d("maxpool_fwd_1x2050x4096")
    assert big == dict(units=524800, blocks=2048, last=None, turns=2) and big["units"] - 2048 * 256 == 512
    assert d("maxpool_bwd_1x2x8")["units"] == 1 and d("maxpool_bwd_3x6x16") == dict(units=18, blocks=1, last=None, turns=1)


def test_relu_backward_rule_is_torchs():
    x = torch.tensor([float("nan"), -1.0, 0.0, -0.0, 2.0], requires_grad=True)
    torch.relu(x).backward(torch.ones(5))
    assert x.grad.tolist() == [1.0, 0.0, 0.0, 0.0, 1.0]
    xn = x.detach().numpy()
    with np.errstate(invalid="ignore"):
        np.testing.assert_array_equal(np.where(xn <= 0, F32(0), F32(1)), x.grad.numpy())
    y = torch.relu(x.detach())
    assert torch.isnan(y[0]) and y[1:].tolist() == [0.0, 0.0, 0.0, 2.0]


@pytest.mark.parametrize("name", [c["name"] for c in pc.CASES if c["entry"].startswith("split")])
def test_res_split_inputs_and_expectations(name):
    c, d, e = pc.CASE[name], pc.inputs(name), pc.expected(name)
    x = d["x"]
    nan = np.isnan(x)
    assert nan.reshape(-1)[0] and (nan.sum() == 1 if x.size == 4 else nan.sum() == 3 and nan.reshape(-1)[-1])
    assert (x == 0).sum() >= 2 and np.signbit(x[x == 0]).any() and not np.signbit(x[x == 0]).all()
    x64 = x.astype(np.float64)
    if c["entry"] == "split_fwd":
        r, p = e["relu_out"][0], e["pool_out"][0]
        assert r.dtype == p.dtype == F32 and np.isnan(r[nan]).all() and (r[~nan] >= 0).all() and not np.signbit(r[x == 0]).any()
        a, b, cc, dd = pc.windows(x64)
        want = (a + b + cc + dd) / 4
        assert np.isnan(p).sum() == np.isnan(want).sum() >= 1
        ok = ~np.isnan(want)
        # three roundings of partial sums no larger than the sum of magnitudes
        mag = (np.abs(a) + np.abs(b) + np.abs(cc) + np.abs(dd)) / 4
        assert (np.abs(p.astype(np.float64) - want)[ok] <= 3 * 2.0 ** -24 * mag[ok]).all()
        return
    two, fma = e["gx"]
    np.testing.assert_array_equal(two, fma)             # the quotient by 4 is exact: the candidates coincide
    ga = d["g_relu"].astype(np.float64) if c["g_relu"] else np.zeros_like(x64)
    gb = np.repeat(np.repeat(d["g_pool"].astype(np.float64) / 4, 2, 1), 2, 2) if c["g_pool"] else np.zeros_like(x64)
    with np.errstate(invalid="ignore"):
        want = np.where(x64 <= 0, 0.0, ga) + gb
    assert np.isfinite(two).all()                        # a NaN input gives a finite gradient: g_relu + g_pool / 4
    np.testing.assert_array_equal(two, want.astype(F32))
    if c["g_relu"]:
        assert d["g_relu"].reshape(-1)[0] > 0 and (two[nan] == (ga + gb)[nan].astype(F32)).all() and (two[nan] != gb[nan].astype(F32)).all()


@pytest.mark.parametrize("name", [c["name"] for c in pc.CASES if c["entry"] == "pyramid"])
def test_pyramid_expectations(name):
    c, d, e = pc.CASE[name], pc.inputs(name), pc.expected(name)
    P, H, W = c["shape"]
    assert list(e) == [f"level{l}" for l in range(c["levels"])]
    cur = d["x"]
    for l in range(c["levels"]):
        (lv,) = e[f"level{l}"]
        assert lv.dtype == F32 and lv.shape == (P, H >> (l + 1), W >> (l + 1))
        a, b, cc, dd = pc.windows(cur.astype(np.float64))
        s1 = (a + b).astype(F32).astype(np.float64)
        s2 = (s1 + cc).astype(F32).astype(np.float64)
        np.testing.assert_array_equal(lv, ((s2 + dd).astype(F32).astype(np.float64) / 4).astype(F32))
        cur = lv
    # against the plain mean of the whole block, loosely: it is the same quantity
    S = 1 << c["levels"]
    mean = d["x"].astype(np.float64).reshape(P, H // S, S, W // S, S).mean((2, 4))
    mag = np.abs(d["x"]).astype(np.float64).reshape(P, H // S, S, W // S, S).mean((2, 4))
    assert (np.abs(cur - mean) <= 3 * c["levels"] * 2.0 ** -24 * mag).all()


@pytest.mark.parametrize("name", [c["name"] for c in pc.CASES if c["entry"].startswith("maxpool")])
def test_maxpool_inputs_and_expectations(name):
    c, d, e = pc.CASE[name], pc.inputs(name), pc.expected(name)
    x = d["x"]
    a, b, cc, dd = pc.windows(x)
    m, k = pc.winner(x)
    stack = np.stack([a, b, cc, dd])
    nan_at = np.isnan(stack)
    if c["shape"] != (1, 2, 8):
        one = nan_at.sum(0) == 1
        assert all((nan_at[i] & one).any() for i in range(4))        # a lone NaN in each position
        assert (nan_at.sum(0) == 2).any() and np.isinf(stack).all(0).any()
        with np.errstate(invalid="ignore"):
            assert ((stack == stack.max(0)).sum(0) >= 2).sum() > 4   # ties
    assert nan_at.any() and set(np.unique(k)) <= {0, 1, 2, 3}
    # the winner: a NaN if the window has one (the last of them), else the first of the maxima
    has = nan_at.any(0)
    assert np.isnan(m[has]).all() and not np.isnan(m[~has]).any()
    last_nan = 3 - np.argmax(nan_at[::-1], axis=0)
    assert (k[has] == last_nan[has]).all()
    with np.errstate(invalid="ignore"):
        first_max = np.argmax(stack == np.nanmax(stack, 0), axis=0)
    assert (k[~has] == first_max[~has]).all() and (m[~has] == stack.max(0)[~has]).all()
    t = torch.from_numpy(np.array(x))[None]
    ty, ti = torch.nn.functional.max_pool2d(t, 2, 2, return_indices=True)
    np.testing.assert_array_equal(ty[0].numpy(), m)
    if c["entry"] == "maxpool_fwd":
        np.testing.assert_array_equal(e["y"][0], m)
        return
    (gx,) = e["gx"]
    ga, gb, gc, gd = pc.windows(gx)
    np.testing.assert_array_equal(np.stack([ga, gb, gc, gd]).sum(0), d["gy"])       # one winner takes gy, three take 0
    assert ((np.stack([ga, gb, gc, gd]) != 0).sum(0) <= 1).all()
    if c["shape"][1] <= 16:       # torch's CPU backward through the saved indices agrees (small shapes)
        tx = torch.from_numpy(np.array(x))[None].requires_grad_(True)
        torch.nn.functional.max_pool2d(tx, 2, 2).backward(torch.from_numpy(np.array(d["gy"]))[None])
        np.testing.assert_array_equal(tx.grad[0].numpy(), gx)
