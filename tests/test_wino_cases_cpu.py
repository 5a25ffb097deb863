"""The case tables of tests/wino_cases.py, without a GPU: every row's plan (plan_wino, plan_wino4: restatements of
g2s_conv3x3_wino and g2s_conv3x3_wino4) carries the labels the row claims, the tables together reach every label of the
required sets below, SUPPORTED equals the restated gate clause by clause, the float64 reference agrees with torch's
float64 convolutions (scales and tail included), the float32 Winograd emulation lies inside the analytic cap on every
element (printed with -s), and the scales of the spans-batch rows would be caught if two samples' were exchanged."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv2d_cases as cc
import wino_cases as wc

NAMES = [c.name for c in wc.WINO + wc.WINO4]

# Every label of the F(2x2) table.  None is unreachable.
REQUIRED = (
    ["scale", "noscale", "K:full", "K:partial", "K:sub", "fast", "slow", "W-odd", "H-odd", "slow:W-even", "TW1", "TW>64",
     "M<64", "M%64", "N%64", "spans-batch", "ktiles1", "ktiles2", "ktiles3"]
    + ["whole", "persistent", "persistent:tiles%8", "splitk:ws", "splitk:atomic:no-ws", "splitk:atomic:ws-small",
       "splitk:atomic:>8", "splitk:clipped", "splitk:rounded", "streamk:forced", "streamk:library", "streamk:ws",
       "streamk:atomic:W-odd", "streamk:atomic:slots>8", "streamk:atomic:no-ws", "streamk:atomic:ws-small",
       "streamk:whole-tile-inside", "streamk:run-crosses-tiles", "det:fallback-whole", "det:keeps-ws"]
    + ["epilogue:none", "epilogue:kernel", "epilogue:reduce", "epilogue:streamk-reduce", "epilogue:deferred:bias-act",
       "epilogue:deferred:noise", "bias-only", "act-only", "bias-act", "noise", "reduce:scalar", "fwd", "transpose"])
REQUIRED4 = (
    ["scale", "noscale"] + [f"TW{t}" for t in (1, 2, 4, 8, 16, 32)] + ["blocks-per-image>1", "M128", "ktiles1", "ktiles2",
                                                                      "ktiles3", "Cr512"]
    + ["whole", "splitk:library", "splitk:forced", "splitk:clipped", "splitk:rounded", "splitk:dropped:no-ws",
       "splitk:dropped:ws-small", "splitk:dropped:>8"]
    + ["epilogue:none", "epilogue:kernel", "epilogue:reduce", "epilogue:kernel:noise", "epilogue:reduce:noise", "bias-only",
       "act-only", "bias-act", "noise", "noise-no-bias", "fwd", "transpose"])
PLACES = ("epilogue:kernel", "epilogue:reduce", "epilogue:streamk-reduce", "epilogue:deferred")


def test_every_row_reaches_what_it_claims():
    for c in wc.WINO + wc.WINO4:
        got = wc.case_labels(c)
        assert c.claims and set(c.claims) <= got, (c, sorted(set(c.claims) - got))


def test_the_tables_reach_every_required_label():
    reached = set().union(*(wc.case_labels(c) for c in wc.WINO))
    assert not [l for l in REQUIRED if l not in reached], [l for l in REQUIRED if l not in reached]
    reached4 = set().union(*(wc.case_labels(c) for c in wc.WINO4))
    assert not [l for l in REQUIRED4 if l not in reached4], [l for l in REQUIRED4 if l not in reached4]
    # every content in every place the F(2x2) epilogue can run, both templates in the kernel
    for content in ("bias-only", "act-only", "bias-act", "noise"):
        rows = [wc.case_labels(c) for c in wc.WINO if content in wc.case_labels(c)]
        for place in PLACES:
            assert any(any(l.startswith(place) for l in r) for r in rows), (content, place)
        assert any({"epilogue:kernel", "slow"} <= r for r in rows) and any({"epilogue:kernel", "fast"} <= r for r in rows)
    # every measured path has rows
    paths = {wc.path_of(c) for c in wc.WINO + wc.WINO4}
    assert paths == {"wino/whole", "wino/persistent", "wino/splitk/ws", "wino/splitk/atomic", "wino/streamk/ws",
                     "wino/streamk/atomic", "wino/det", "wino4/whole", "wino4/splitk"}, paths


def test_the_plans_at_the_points_the_rows_were_built_for():
    p = wc.BY_NAME["s_ws"].plan()
    assert (p["tiles"], p["ktiles"], p["upw"], p["grid_x"], p["slots"]) == (3, 8, 5, 5, 3) and list(p["parts"]) == [2, 3, 2]
    p = wc.BY_NAME["s_inside"].plan()
    assert (p["tiles"], p["ktiles"], p["upw"], p["grid_x"], p["slots"]) == (6, 3, 5, 4, 2) and list(p["parts"]) == [1, 2, 1, 2, 1, 1]
    # M = 130: m-tiles of 64, 64, 2 channels; 96 2x2 tiles: blocks of 256 and 128 pixels.  Tile 1 (m-tile 1, block 0) and
    # tile 3 (m-tile 0, block 1) are split in two
    assert p["ws_written"] == 2 * 64 * 256 + 2 * 64 * 128 and p["ws_written"] < p["slots"] * p["y_floats"]
    p = wc.BY_NAME["s_upw_odd"].plan()
    assert (p["ktiles"], p["upw"], p["ktiles"] % p["upw"], list(p["parts"])) == (7, 6, 1, [2, 2, 2])
    p = wc.BY_NAME["s_library"].plan()
    assert (p["tiles"], p["units"], p["upw"], p["slots"], p["mode"]) == (30, 780, 4, 8, "streamk:library") and p["units"] >= 769
    p = wc.BY_NAME["s_slots9"].plan()
    assert (p["upw"], p["slots"], p["why_atomic"]) == (2, 9, "slots>8")
    for name, tiles in (("r_fast", 512), ("r_ragged", 514)):
        p = wc.BY_NAME[name].plan()
        assert (p["mode"], p["tiles"], p["grid_x"]) == ("persistent", tiles, 256) and not p["partial_sums"]
    assert wc.BY_NAME["r_ragged"].plan()["tiles"] % 8 == 2 and ((514 + 7) // 8) % 32 != 0
    p = wc.BY_NAME["p_sk_rounded"].plan()
    assert (p["asked"], p["splitk"], p["ws_written"]) == (5, 4, 4 * p["y_floats"])
    assert wc.BY_NAME["p_sk_short"].ws_floats() == 4 * wc.BY_NAME["p_sk_short"].y_floats - 1
    p = wc.BY_NAME["d_lib_nows"].plan()
    assert p["planned"] == "streamk:library" and p["mode"] == "whole" and p["grid_x"] == 30 and not p["clears_y"]
    for name in wc.DET_FALLBACK:
        c = wc.BY_NAME[name]
        assert c.plan(det=False)["clears_y"] and not c.plan(det=True)["partial_sums"], name
    for name in wc.DET_KEEPS:
        assert wc.BY_NAME[name].plan(det=True)["uses_ws"], name
    p = wc.BY_NAME["f_cr512"].plan()
    assert (p["tiles"], p["ktiles"], p["splitk"], p["source"]) == (1, 128, 8, "library")
    p = wc.BY_NAME["f_sk_rounded3"].plan()
    assert (p["ktiles"], p["asked"], p["splitk"]) == (7, 5, 4)
    for name in wc.ON_DEVICE:
        assert wc.BY_NAME[name].ep is None, name


def test_supported_table_equals_the_restated_gate_and_covers_every_clause():
    for shape, want in wc.SUPPORTED.items():
        assert wc.supported4(*shape)[0] == want, shape
    for shape, clause in wc.SUPPORTED_CLAUSE.items():
        assert wc.SUPPORTED[shape] == 0 and wc.supported4(*shape) == (0, clause), (shape, wc.supported4(*shape))
    assert set(wc.SUPPORTED_CLAUSE.values()) == set(wc.W4_CLAUSES)
    # every rejected shape has an accepted one that differs in a single argument
    ok = [s for s, v in wc.SUPPORTED.items() if v]
    for shape, v in wc.SUPPORTED.items():
        if not v:
            assert any(sum(a != b for a, b in zip(shape, o)) == 1 for o in ok), shape
    for c in wc.WINO4:
        assert wc.supported4(c.B, c.Cr, c.M, c.H, c.W)[0] == 1, c


def _scale_check(got, ref, what):
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max(), (what, np.abs(got - ref).max(), np.abs(ref).max())


def _torch_float64(c, dt):
    x = torch.tensor(dt["x"], dtype=torch.float64)
    w = torch.tensor(dt["w"], dtype=torch.float64)
    if c.scale:
        x = x * torch.tensor(dt["in_scale"], dtype=torch.float64)[:, :, None, None]
    y = F.conv_transpose2d(x, w, padding=1) if c.tr else F.conv2d(x, w, padding=1)
    if c.scale:
        y = y * torch.tensor(dt["out_scale"], dtype=torch.float64)[:, :, None, None]
    if c.ep is not None:
        bias, act, noise = c.ep
        if noise:
            y = y + wc.NOISE_W * torch.tensor(dt["noise"], dtype=torch.float64)
        if bias:
            y = y + torch.tensor(dt["bias"], dtype=torch.float64)[None, :, None, None]
        if act:
            y = F.leaky_relu(y, wc.ALPHA) * wc.GAIN
    return y.numpy()


@pytest.mark.parametrize("name", NAMES)
def test_reference_equals_torch_float64_and_the_emulation_is_inside_the_cap(name):
    c = wc.BY_NAME[name]
    dt = wc.data(name)
    ref, cap, e32w, r32 = dt["ref"], dt["cap"], dt["e32w"], dt["r32"]
    assert ref.shape == (c.B, c.M, c.H, c.W) and dt["w"].shape == ((c.Cr, c.M, 3, 3) if c.tr else (c.M, c.Cr, 3, 3))
    _scale_check(_torch_float64(c, dt), ref, name)
    err = np.abs(r32.astype(np.float64) - ref)
    left_out = float((err > cap).mean())
    print(f"{c} [{wc.path_of(c)}]: e32w {e32w:.3e} (floored {cc.floor_e32(e32w):.3e}), float32 error / cap at most "
          f"{float((err / np.maximum(cap, 1e-300)).max()):.3f}, share of elements left out {left_out:g}")
    assert np.isfinite(ref).all() and np.isfinite(cap).all() and np.isfinite(e32w) and 0 < e32w < 1e-4, (name, e32w)
    assert left_out == 0, (name, left_out)
    if c.kind == 4:
        assert e32w > 0.5 * cc.EPS32, (name, e32w)
    # the bound is never the bare cap of an element without terms
    assert (wc.bound(ref, e32w, cap) > 0).all()


@pytest.mark.parametrize("name", [c.name for c in wc.WINO if "spans-batch" in wc.case_labels(c)])
def test_exchanged_scales_of_two_samples_miss_the_bound(name):
    c = wc.BY_NAME[name]
    dt = wc.data(name)
    for k in ("in_scale", "out_scale"):
        s = np.abs(dt[k])
        lo, hi = s[0::2].max(), s[1::2].min()
        assert max(lo, hi) / min(lo, hi) > 1.5, (name, k, lo, hi)       # the samples' scales do not overlap
    weff = wc.effective_weights(dt["w"], c.tr)
    bound = wc.bound(dt["ref"], dt["e32w"], dt["cap"])
    for k in ("in_scale", "out_scale"):
        sw = {"in_scale": dt["in_scale"], "out_scale": dt["out_scale"]}
        sw[k] = np.ascontiguousarray(np.roll(dt[k], 1, axis=0))       # sample b takes sample b - 1's
        wrong = wc.sums_reference(dt["x"], weff, sw["in_scale"], sw["out_scale"])
        if c.ep is not None:
            wrong = wc.tail(wrong, dt["bias"], dt["noise"], c.ep, np.float64)
        missed = np.abs(wrong - dt["ref"]) > bound
        assert missed.mean() > 0.9, (name, k, float(missed.mean()))


def test_the_transforms_are_winograd_and_the_data_reproducible():
    # A^T [(G g G^T) .* (B^T d B)] A is the correlation of one tile, exactly, for integer data
    rng = np.random.default_rng(5)
    for kind, m in ((2, 2), (4, 4)):
        BT, G, AT = wc.MATS[kind]
        g = rng.integers(-3, 4, (3, 3)).astype(np.float64) * 24
        d = rng.integers(-3, 4, (m + 2, m + 2)).astype(np.float64)
        y = AT @ ((G @ g @ G.T) * (BT @ d @ BT.T)) @ AT.T
        want = np.array([[(d[i:i + 3, j:j + 3] * g).sum() for j in range(m)] for i in range(m)])
        assert np.abs(y - want).max() <= 1e-9 * np.abs(want).max(), kind
    a = wc.data("t_slow")
    wc.data.cache_clear()
    b = wc.data("t_slow")
    assert a is not b and all(np.array_equal(a[k], b[k]) for k in a if isinstance(a[k], np.ndarray))
    assert not a["ref"].flags.writeable
    w = a["w"]
    assert np.abs(w - w[..., ::-1, ::-1]).max() > 0.1 * np.abs(w).max() and np.abs(w - w.transpose(0, 1, 3, 2)).max() > 0.1 * np.abs(w).max()
    assert w.dtype == np.float32 and abs(float(w.std()) * np.sqrt(9 * 6) - 1) < 0.2
    assert wc.data("x_slow")["w"].shape == (7, 70, 3, 3)
