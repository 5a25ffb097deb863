"""The case table of tests/warp_cases.py, without a GPU: every case reaches the kernel, the clear and the grid it is
listed for; the float32 restatement of corner_of is what the module docstring says; the hand-placed pixels are there
and land where they are meant to; no clamped sample sits within its bound of a limit (but the deliberate exact ones);
the fixed point stays in range; and the kernels' float32 arithmetic agrees with the float64 reference within the bounds."""
import numpy as np
import pytest

import warp_cases as wc

F32 = np.float32


def test_every_case_takes_the_path_it_is_listed_for():
    for c in wc.CASES:
        assert wc.dispatch(c) == (c["kernel"], c["clears"], c["blocks"]), c["name"]
    have = {(c["kernel"], c["clears"]) for c in wc.CASES}
    assert have == {("fwd", None), ("bwd<float>", "gx"), ("bwd<float>", None), ("bwd<fixed>", "workspace"),
                    ("bwd<fixed>", None)}
    # deterministic mode without gx takes the float kernel and clears nothing
    assert wc.dispatch(wc.CASE["bwd_nogx_det"]) == ("bwd<float>", None, (2, 2))


def test_shapes_bounds_and_modes_are_covered():
    bwd = [c for c in wc.CASES if c["entry"] == "bwd"]
    for c in wc.CASES:
        B, C, ih, iw, H, W = c["shape"]
        assert (ih, iw) == (5, 7) and B == 2 and (H, W) in ((19, 23), (16, 16)) and C in (1, 3)
    assert wc.CASE["fwd_clamp"]["blocks"] == (2, 2) and 19 * 23 == 437 and wc.CASE["fwd_256"]["blocks"] == (1, 2)
    for group in (bwd, [c for c in wc.CASES if c["entry"] == "fwd"]):
        assert {(c["clamp"], c["lo"], c["hi"]) for c in group} >= {(0, -1.0, 1.0), (1, -1.0, 1.0), (1, float(F32(-0.3)), float(F32(0.4)))}
        assert {c["shape"][1] for c in group} == {1, 3} and {c["shape"][4] * c["shape"][5] for c in group} == {437, 256}
    for det in (False, True):
        assert {(c["gx"], c["ggrid"]) for c in bwd if c["det"] == det} == {(True, True), (False, True), (True, False)}
        assert {c["acc_is_zero"] for c in bwd if c["det"] == det} == {0, 1}
    assert {c["gy_scale"] for c in bwd if c["det"]} == {1.0, 1e5, 1e-9}
    assert [c["name"] for c in bwd if c["ws_off"]] == ["bwd_ws_offset_det"] and wc.CASE["bwd_ws_offset_det"]["ws_off"] == 4
    assert wc.workspace_bytes(2, 3, 5, 7) == 2 * 3 * 5 * 7 * 8 + 256 and wc.workspace_bytes(2, 0, 5, 7) == 0


def test_corner_restates_corner_of():
    """ix = ((g + 1) / 2) * (size - 1), floor, w0 = (f + 1) - ix, w1 = ix - f: each step is the float32 rounding of the
    exact operation on its float32 operands."""
    g = wc.inputs("fwd_noclamp")["grid"][..., 0]
    fin = np.isfinite(g) & (np.abs(g) < 1e6)
    fx, w0, w1, sane, ix = wc.corner(g, wc.IW)
    g64 = g[fin].astype(np.float64)
    a = (g64 + 1.0).astype(F32)
    b = (a.astype(np.float64) / 2.0).astype(F32)
    i = (b.astype(np.float64) * (wc.IW - 1)).astype(F32)
    np.testing.assert_array_equal(ix[fin], i)
    np.testing.assert_array_equal(fx[fin], np.floor(i.astype(np.float64)).astype(F32))
    np.testing.assert_array_equal(w0[fin], ((fx[fin].astype(np.float64) + 1.0).astype(F32).astype(np.float64) - i).astype(F32))
    np.testing.assert_array_equal(w1[fin], (i.astype(np.float64) - fx[fin]).astype(F32))
    assert sane[fin].sum() > 300 and (~sane[fin]).sum() >= 2
    # align_corners: -1 -> texel 0, +1 -> texel size - 1, weights (1, 0); 0 -> the middle texel
    fx, w0, w1, sane, ix = wc.corner(np.array([-1.0, 1.0, 0.0], F32), wc.IW)
    assert fx.tolist() == [0, 6, 3] and w0.tolist() == [1, 1, 1] and w1.tolist() == [0, 0, 0] and sane.all()
    # the edges of `sane`: floor -2 and size are in, -3 and size + 1 are out; non-finite is out
    with np.errstate(invalid="ignore"):
        fx, _, _, sane, _ = wc.corner(np.array([-1.5, 1.5, -2.0, 2.0, 1e30, np.inf, -np.inf, np.nan], F32), wc.IW)
    assert fx[:4].tolist() == [-2, 7, -3, 9] and sane.tolist() == [True, True, False, False, False, False, False, False]
    fy, _, _, sane, iy = wc.corner(np.array([-2.0, 1.5, -2.5, 2.0], F32), wc.IH)
    assert fy.tolist() == [-2, 5, -3, 6] and iy.tolist() == [-2, 5, -3, 6] and sane.tolist() == [True, True, False, False]


@pytest.mark.parametrize("name", wc.NAMES)
def test_placed_pixels_land_where_they_are_meant_to(name):
    c, d = wc.CASE[name], wc.inputs(name)
    B, C, ih, iw, H, W = c["shape"]
    g = d["grid"].reshape(B, H * W, 2)
    cs = wc.cells(name)
    n_in = np.sum([k[2] for k in cs], axis=0).reshape(B, H * W)             # in-range corners per pixel
    live = wc.expected(name)["live"].reshape(B, H * W)
    tags = {}
    for i, (px, py, tag) in enumerate(wc.placed_pixels()):
        np.testing.assert_array_equal(g[:, i], np.broadcast_to(np.array([px, py], F32), (B, 2)))
        tags.setdefault(tag, []).append(n_in[0, i])
    assert tags["corner"] == [4, 1, 2]                   # texel (0, 0); (IW - 1, IH - 1): alone; (IW - 1, 0): one column
    assert tags["texel"] == [4, 4, 4] and tags["one column"] == [2, 2] and tags["one row"] == [2, 2] and tags["one corner"] == [1]
    assert tags["sane edge"] == [0, 0, 0, 0] and tags["far"] == [0, 0, 0, 0]
    for v in ("1e30", "+inf", "-inf", "nan"):
        for ax in ("x", "y", "xy"):
            assert tags[f"{v} {ax}"] == [0]
    assert np.isnan(g[:, -1, 0]).all() and not live[:, -1].any()
    # the warp itself: most pixels have four corners, some spill
    assert (n_in == 4).sum() > 0.4 * n_in.size and (n_in == 0).sum() > len(wc.placed_pixels()) // 2
    # exact pixels: weights (1, 0, 0, 0)
    for i, (px, py, tag) in enumerate(wc.placed_pixels()):
        if tag in ("corner", "texel"):
            w = [(k[3] * k[4]).reshape(B, H * W)[0, i] for k in cs]
            assert w == [1, 0, 0, 0], (i, w)


@pytest.mark.parametrize("name", wc.NAMES)
def test_no_clamped_sample_within_its_bound_of_a_limit(name):
    c = wc.CASE[name]
    e = wc.expected(name)
    exact = wc.exact_on_limit(name)
    assert exact.sum() == 2 * c["shape"][0] * c["shape"][1]                 # the lo texel and the hi texel, per plane
    v = e["y_raw"]
    assert ((v[exact] == c["lo"]) | (v[exact] == c["hi"])).all() and (e["y"][exact] == v[exact]).all()
    if not c["clamp"]:
        return
    near = (np.abs(v - c["lo"]) <= e["y_bound"]) | (np.abs(v - c["hi"]) <= e["y_bound"])
    assert not (near & ~exact).any(), np.argwhere(near & ~exact)[:4]
    assert (v < c["lo"]).sum() >= 5 and (v > c["hi"]).sum() >= 5 and ((v > c["lo"]) & (v < c["hi"])).sum() > 100
    if c["entry"] == "bwd" and c["ggrid"]:          # the exact pixels pass the gradient
        gy = wc.inputs(name)["gy"]
        assert (gy[exact] != 0).all()


@pytest.mark.parametrize("name", wc.NAMES)
def test_float32_arithmetic_within_the_bounds_of_float64(name):
    c, e, k = wc.CASE[name], wc.expected(name), wc.emulate32(name)
    B, C, ih, iw, H, W = c["shape"]
    dead = ~e["live"]
    assert (e["y_raw"][np.broadcast_to(dead[:, None], e["y_raw"].shape)] == 0).all()
    err = np.abs(k["y"].astype(np.float64) - e["y"])
    assert np.isfinite(k["y"]).all() and (err <= e["y_bound"]).all()
    worst = {"y": float((err / np.maximum(e["y_bound"], 1e-300)).max())}
    if c["entry"] == "bwd":
        assert (e["ggrid"][dead] == 0).all() and (e["ggrid_bound"][dead] == 0).all()
        err = np.abs(k["ggrid"].astype(np.float64) - e["ggrid"])
        assert np.isfinite(k["ggrid"]).all() and (err <= e["ggrid_bound"]).all()
        worst["ggrid"] = float((err / np.maximum(e["ggrid_bound"], 1e-300)).max())
        assert e["m"].sum() == C * sum(int(x[2].sum()) for x in wc.cells(name)) and e["m"].max() > 8
        assert e["gx_abs"].max() < wc.FIX_RANGE / 2                         # the fixed point does not saturate
        assert (e["gx"][e["m"] == 0] == 0).all() and (e["gx_bound"][e["m"] == 0] == 0).all()
        if c["gy_scale"] == 1e5:
            assert e["gx_abs"].max() > 1e5
        if c["gy_scale"] == 1e-9:                                           # resolution: the 2^-41 term leads the bound
            assert (e["m"] * wc.FIX_HALF > 3 * wc.U * e["gx_abs"])[e["m"] > 0].all()
    print(name, " ".join(f"{a} {b:.3f}" for a, b in worst.items()))
