"""The case table of tests/rowops_cases.py, without a GPU: every rows_dot_scale case takes the kernel and the lane turns
it is listed for, the shapes reach the heads, idle waves, early exits and second turns they were chosen for, and the
float32 arithmetic in the kernels' order agrees with the float64 reference within the stated bounds."""
import numpy as np
import pytest

import rowops_cases as rc

F32 = np.float32


def test_rows_dot_scale_cases_take_the_kernel_they_are_listed_for():
    rds = [c for c in rc.CASES if c["entry"] == "rds"]
    for c in rds:
        assert rc.dispatch(c) == (c["kernel"], c["turns"]), c["name"]
        # the launcher's rule, from the pointers the GPU test hands in: base + 4 bytes for a name in `mis`
        ptr = {k: 4096 + (4 if k in c["mis"] else 0) for k in ("a", "b", "out")}
        if c["out"] == "b":
            ptr["out"] = ptr["b"]
        a, out = (ptr["a"] if c["a"] else 0), (ptr["out"] if c["out"] else 0)
        aligned = (not ptr["b"] & 15) and (not a or not a & 15) and (not out or not out & 15)
        assert aligned == (c["kernel"] == rc.HBT), c["name"]
    assert {c["kernel"] for c in rds} == {rc.HBT, rc.SC}
    assert {m for c in rds for m in c["mis"]} == {"a", "b", "out"}
    for shape in ((5, 7), (6, 3), (3, 1), (2, 264), (3, 1031)):
        assert any(c["shape"] == shape and c["a"] and c["dot"] and c["out"] == "sep" and c["s"] and c["inv"] and not c["mis"]
                   for c in rds), shape
    flags = {(c["a"], c["dot"], c["out"], c["s"], c["inv"]) for c in rds}
    assert (False, False, "sep", True, False) in flags and (True, True, None, False, True) in flags
    assert any(f[2] == "b" for f in flags) and any(not f[3] and f[2] for f in flags) and any(not f[4] and f[1] for f in flags)


def test_rows_dot_scale_shapes_reach_their_heads_and_turns():
    rows = lambda n: rc.rds_rows(rc.CASE[n])[1]
    r = rows("rds_5x7_full")
    assert [h for h, _, _ in r] == [0, 1, 2, 3, 0] and {n4 for _, n4, _ in r} == {1} and [t for _, _, t in r] == [3, 2, 1, 0, 3]
    # (every row of 5 x 7 keeps one float4; the rows with no float4 body are those of 6 x 3 and 3 x 1)
    assert [h for h, _, _ in rows("rds_6x3_full")] == [0, 1, 2, 3, 0, 1] and {n4 for _, n4, _ in rows("rds_6x3_full")} == {0}
    # head > n: clipped (row 1 of 3 x 1 asks for 3, row 3 of 6 x 3 asks for 3 of 3)
    assert [(4 - r_ % 4) % 4 for r_ in range(3)] == [0, 3, 2] and [h for h, _, _ in rows("rds_3x1_full")] == [0, 1, 1]
    assert rows("rds_2x264_full") == [(0, 66, 0), (0, 66, 0)]            # 64 quads, then 2 more: a second turn for two lanes
    assert rows("rds_3x1031_full") == [(0, 257, 3), (1, 257, 2), (2, 257, 1)]
    assert rows("rds_5x7_mis_a") == [(7, 0, 0)] * 5 and rows("rds_3x1031_mis_out") == [(1031, 0, 0)] * 3
    assert rc.chain(rc.CASE["rds_3x1031_full"]) == 1 + 4 * 5 + 1 + 6 and rc.chain(rc.CASE["rds_3x1031_mis_out"]) == 17 + 6
    assert rc.chain(rc.CASE["rds_3x1_full"]) == 1 + 6


def test_demod_and_channel_sum_shapes_reach_what_they_were_chosen_for():
    d = lambda n: rc.dispatch(rc.CASE[n])
    assert d("demod_fwd_2x5x3") == dict(grid=2, idle_waves=2, trips=1)
    assert d("demod_bwd_2x5x3") == dict(grid=(1, 2), wave_outputs=(1, 1, 1, 0), idle_lanes=59)      # a wave is idle
    assert d("demod_bwd_3x70x9")["grid"] == (2, 3) and d("demod_bwd_3x70x9")["wave_outputs"] == (3, 2, 2, 2)
    assert d("demod_fwd_3x70x9")["idle_waves"] == 1 and d("demod_fwd_3x70x9")["trips"] == 2     # B * Cout = 27
    assert d("demod_bwd_1x64x4")["idle_lanes"] == 0 and d("demod_fwd_2x130x7")["trips"] == 3
    assert {c["shape"] for c in rc.CASES if c["entry"] == "demod_fwd" and not c["tiny"]} == set(rc.DEMOD_SHAPES)
    for shape in rc.DEMOD_SHAPES:
        assert {c["add"] for c in rc.CASES if c["entry"] == "demod_bwd" and c["shape"] == shape} == {None, "sep", "gs"}
    # every layer of the multi call undercuts the maximum that sizes the grid somewhere
    assert d("multi_fwd") == dict(grid=(7, 3), idle_waves=(19, 7, 1))
    assert d("multi_bwd") == dict(grid=(3, 3, 3), idle_blocks=(2, 0, 1))
    cin, cout = zip(*rc.MULTI_LAYERS)
    assert cin.index(max(cin)) != cout.index(max(cout)) and len(rc.MULTI_LAYERS) < rc.MAX_LAYERS
    assert d("csum_1x3x1")["idle_lanes"] == 255 and d("csum_2x5x9") == dict(grid=5, trips=1, idle_lanes=238)
    assert d("csum_3x2x100")["trips"] == 2 and 100 < 256 < 200 + 100      # a sample boundary inside the first turn
    assert d("csum_4x7x64") == dict(grid=7, trips=1, idle_lanes=0)
    # eps leads acc in the tiny case; s is around 1 and wsq positive elsewhere
    t = rc.inputs("demod_fwd_tiny")
    acc = (t["wsq"].astype(np.float64)[None] * t["s"].astype(np.float64)[:, None] ** 2).sum(2)
    assert acc.max() < 1e-3 * rc.EPS and acc.min() > 0
    t = rc.inputs("demod_fwd_3x70x9")
    assert (t["wsq"] > 0).all() and abs(float(t["s"].mean()) - 1) < 0.1


@pytest.mark.parametrize("name", rc.NAMES)
def test_float32_arithmetic_within_the_bounds_of_float64(name):
    exp, emu = rc.expected(name), rc.emulate32(name)
    c, d = rc.CASE[name], rc.inputs(name)
    worst = 0.0
    for key, (val, bound) in exp.items():
        if bound is None:       # out = b * s: one rounding of the exact product
            assert val.dtype == F32
            s = d["s"].astype(np.float64)[:, None] if c["s"] else 1.0
            np.testing.assert_array_equal(val, (d["b"].astype(np.float64) * s).astype(F32))
            continue
        got = emu[key].astype(np.float64)
        assert got.shape == val.shape and (bound > 0).all()
        err = np.abs(got - val)
        assert (err <= bound).all(), (name, key, float((err / bound).max()))
        worst = max(worst, float((err / bound).max()))
    print(f"{name}: float32 in the kernel's order within {worst:.3f} of the bound")
