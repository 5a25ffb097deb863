"""The case tables of tests/conv2d_cases.py, without a GPU: every row's plan (plan_conv, plan_wgrad: restatements of
conv_launch and wgrad_plan) carries the labels the row claims, the tables together reach every label of the required
sets below, the float64 references agree with torch's float64 convolutions, every float32 yardstick is positive and
inside the analytic cap (printed with -s), the data is reproducible, and op/conv.py's supported() accepts only
geometries whose three launches plan without a rejected tap count."""
import numpy as np
import pytest
import torch

import conv2d_cases as cc

CONV_NAMES = [c.name for c in cc.CONV]
WGRAD_NAMES = [c.name for c in cc.WGRAD]
BWD_NAMES = [c.name for c in cc.BWD]

# What the g2s_conv2d table has to reach.  None of the tap bodies, tiles and split forms is left out.
REQUIRED_CONV = (
    [f"gather:k{k}:s{s}" for k in range(1, 6) for s in (1, 2)] + [f"T{T}" for T in cc.TAPS_OK]
    + ["scatter:k3:s1:p1", "scatter:k4:s1:p0", "scatter:k4:s1:p3", "scatter:k5:s1:p2", "scatter:k2:s2", "scatter:k4:s2",
       "scatter:k3:s2:p0", "scatter:k3:s2:p1", "scatter:k1:s2", "holes"]
    + [f"T{T}:{w}" for T in (1, 2, 4, 9) for w in ("full", "partial", "sub")]
    + [f"{f}:k{k}:s{s}:p{p}" for f in ("gather", "scatter") for k in (3, 4) for s in (1, 2) for p in range(k)]
    + ["out:min", "out:+h", "out:+w", "early-exit", "ragged-classes"]
    + ["M<tile", "M%tile", "N<tile", "N%tile", "spans-batch", "groups:M%tile"]
    + [f"layout:adj{a}:mm{m}" for a in (0, 1) for m in (0, 1)] + [f"groups{g}" for g in (1, 2, 3, 8)]
    + ["kmax18", "kmax26", "pick:heuristic", "pick:tuned", "pick:heuristic-only", "split:heuristic", "split:tuned",
       "split:forced", "split:det", "split:unequal", "split:1", "split:n"]
    + ["epilogue:none", "epilogue:kernel", "epilogue:deferred", "needs-zero", "overwrites"])
# pick:forced, split:clipped and every tile under every split are the sweep's (test_the_sweep_...); the heuristic itself
# never picks tile 4 (64x128 comes from tuned rows at B = 9 and from g2s_modconv_tune only), so tile4 is the sweep's too
REQUIRED_HEURISTIC_TILES = ("tile0", "tile1", "tile2", "tile3")
REQUIRED_WGRAD = (
    ["Ca1", "Ca63", "Ca64", "Ca65", "N63", "N64", "N65", "K20", "K32", "K33", "K-spans-batch", "G-larger"]
    + [f"k{k}:s{s}" for k in range(1, 6) for s in (1, 2)] + [f"k3:s{s}:p{p}" for s in (1, 2) for p in range(3)]
    + ["role:conv", "role:convT", "split:1", "split:n", "split:ragged", "split:grid-full", "split:det",
       "groups1", "groups2", "groups3"])
REQUIRED_BWD = (
    [f"tile{t}" for t in range(5)] + ["bwd:one-grid", "bwd:two-launch", "kmax18", "kmax26", "layer:conv", "layer:convT",
                                       "out:+h", "out:+w", "split:1", "split:n", "split:unequal", "split:det", "groups1",
                                       "groups2", "pick:heuristic", "pick:tuned", "pick:forced"])


def test_every_conv_case_reaches_what_its_row_claims():
    for c in cc.CONV:
        got = cc.labels(c, c.plan())
        assert set(c.claims) <= got, (c, sorted(set(c.claims) - got))
        assert c.claims, c


def test_the_conv_table_reaches_every_required_label():
    reached = set().union(*(cc.labels(c, c.plan()) for c in cc.CONV))
    assert not [l for l in REQUIRED_CONV if l not in reached], [l for l in REQUIRED_CONV if l not in reached]
    heur = set().union(*(cc.labels(c, c.plan()) for c in cc.CONV if c.plan()["source"] == "heuristic"))
    assert set(REQUIRED_HEURISTIC_TILES) <= heur
    # the 128-wide picks at the smallest size that gives them: Cr = 3, M = 96, 128 x 128, B = 4 (3 for 128x64)
    c = cc.CONV_BY_NAME["heur_tile0"]
    assert cc.cdiv(c.M, 128) * cc.cdiv(c.B * 128 * 128, 128) == 512 and c.plan(fused=False)["pick"] == 0
    assert 2.0 * c.B * c.Cr * c.M * 9 * 128 * 128 < 0.4e9


def test_the_tuned_rows_are_taken_from_the_table():
    rows = cc.tuned_rows()
    assert len(rows) >= 60
    for name, want in (("tuned_tile3", (3, 6)), ("tuned_sk48", (2, 48)), ("tuned_fused", (2, 32))):
        c = cc.CONV_BY_NAME[name]
        pl = c.plan()
        assert c.B == 1 and (pl["pick"], pl["splitk"]) == want and pl["source"] == "tuned", (name, pl["pick"], pl["splitk"])
    off = cc.CONV_BY_NAME["tuned_off"].plan()
    assert (off["pick"], off["splitk"], off["source"]) == (2, 4, "heuristic-only")
    assert cc.CONV_BY_NAME["tuned_fused"].plan()["deferred"]


def test_the_classes_of_the_strided_scatter():
    # 3 x 3, stride 2: 4 / 2 / 2 / 1 taps, and pad 0 and pad 1 hand them to different residue classes
    t0 = {(c["oy0"], c["ox0"]): c["T"] for c in cc.classes(5, 7, 3, 2, 0, 1)[2]}
    t1 = {(c["oy0"], c["ox0"]): c["T"] for c in cc.classes(5, 7, 3, 2, 1, 1)[2]}
    assert t0 == {(0, 0): 4, (0, 1): 2, (1, 0): 2, (1, 1): 1} and t1 == {(0, 0): 1, (0, 1): 2, (1, 0): 2, (1, 1): 4}
    assert [c["T"] for c in cc.classes(5, 7, 2, 2, 0, 1)[2]] == [1] * 4 and [c["T"] for c in cc.classes(5, 7, 4, 2, 1, 1)[2]] == [4] * 4
    _, _, cls, holes = cc.classes(5, 7, 1, 2, 0, 1)
    assert len(cls) == 1 and holes == [(0, 1), (1, 0), (1, 1)]
    assert sorted(c["T"] for c in cc.classes(5, 7, 5, 2, 2, 1)[2]) == [4, 6, 6, 9]
    # unequal shares: 33 / 17 / 17 / 9 K tiles at split-K 8 and 4, 9 / 5 / 5 / 3 at 3
    assert cc.CONV_BY_NAME["shares_sk8"].plan()["cls_splitk"] == [2, 4, 4, 8]
    assert cc.CONV_BY_NAME["shares_sk4"].plan()["cls_splitk"] == [1, 2, 2, 4]
    assert cc.CONV_BY_NAME["shares_sk3"].plan()["cls_splitk"] == [1, 2, 2, 3]       # 2 = (3 * 5 + 4) / 9: the rounding term
    assert cc.CONV_BY_NAME["shares_sk3_p0"].plan()["cls_splitk"] == [3, 2, 2, 1]


@pytest.mark.parametrize("name", list(cc.SWEEP))
def test_the_sweep_reaches_every_tile_under_every_split_form(name):
    c, bodies = cc.SWEEP[name]
    splits = cc.sweep_splits(c)
    assert splits[:3] == (1, 2, 3) and splits[3] > 3
    seen = set()
    for tile in cc.SWEEP_TILES:
        for sk in splits:
            pl = c.plan(tile=tile, sk=sk)
            got = cc.labels(c, pl) | {f"asked{sk}"}
            assert set(bodies) <= got and pl["pick"] == tile and pl["source"] == "forced", (name, tile, sk)
            assert pl["splitk"] == min(sk, pl["kt_min"]) and (sk == splits[3]) == ("split:clipped" in got), (name, tile, sk)
            assert pl["kmax"] == (26 if "T25" in bodies else 18)
            seen |= got
    assert {f"tile{t}" for t in range(5)} | {"pick:forced", "split:forced", "split:clipped", "split:1", "split:n"} <= seen
    assert set().union(*(b for _, b in cc.SWEEP.values())) >= {f"T{T}" for T in cc.TAPS_OK}


def test_every_wgrad_case_reaches_what_its_row_claims_and_the_table_every_label():
    reached = set()
    for c in cc.WGRAD:
        got = cc.wgrad_labels(c, c.plan())
        assert c.claims and set(c.claims) <= got, (c, sorted(set(c.claims) - got), c.plan())
        reached |= got
    assert not [l for l in REQUIRED_WGRAD if l not in reached], [l for l in REQUIRED_WGRAD if l not in reached]
    pl = cc.WGRAD_BY_NAME["w_ragged"].plan()
    assert (pl["ktiles"], pl["per"], pl["split"]) == (771, 2, 386)
    pl = cc.WGRAD_BY_NAME["w_grid_full"].plan()
    assert pl["tiles"] == 768 and pl["K"] < 32 and not pl["atomic"]
    pl = cc.WGRAD_BY_NAME["w_split"].plan()
    assert pl["split"] == pl["ktiles"] == 14 and pl["atomic"]
    assert cc.WGRAD_BY_NAME["w_ca1"].PH * cc.WGRAD_BY_NAME["w_ca1"].PW == 35 and cc.WGRAD_BY_NAME["w_ca1"].B == 3


def test_every_bwd_case_reaches_what_its_row_claims_and_the_table_every_label():
    reached = set()
    for c in cc.BWD:
        pl = c.plan()
        got = cc.bwd_labels(c, pl)
        assert c.claims and set(c.claims) <= got, (c, sorted(set(c.claims) - got))
        assert pl["one_grid"] == (pl["pick"] >= 2)
        reached |= got
    assert not [l for l in REQUIRED_BWD if l not in reached], [l for l in REQUIRED_BWD if l not in reached]
    for form in ("bwd:one-grid", "bwd:two-launch"):     # either form with either kernel instance and layer kind
        rows = [cc.bwd_labels(c, c.plan()) for c in cc.BWD if form in cc.bwd_labels(c, c.plan())]
        assert {"kmax18", "kmax26", "layer:conv", "layer:convT"} <= set().union(*rows), form


def _scale_check(got, ref, what):
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max(), (what, np.abs(got - ref).max(), np.abs(ref).max())


def _yardstick(name, what, ref, cap, e32, r32):
    assert np.isfinite(ref).all() and np.isfinite(e32) and 0 < e32 < 1e-5, (name, what, e32)
    over = np.abs(r32.astype(np.float64) - ref) / np.maximum(cap, 1e-300)
    assert (np.abs(r32.astype(np.float64) - ref) <= cap).all(), (name, what, float(over.max()))
    print(f"{name} {what}: e32 {e32:.3e} (floored {cc.floor_e32(e32):.3e}), float32 error / cap at most {float(over.max()):.3f}")


@pytest.mark.parametrize("name", CONV_NAMES + list(cc.SWEEP))
def test_conv_reference_equals_torch_float64_and_the_yardstick_is_inside_the_cap(name):
    c = cc.CONV_BY_NAME[name] if name in cc.CONV_BY_NAME else cc.SWEEP[name][0]
    dt = cc.conv_data(name)
    sums = cc.conv_reference(dt["x"], dt["w"], c)
    _scale_check(cc._torch_conv_f32(dt["x"], dt["w"], c, torch.float64), sums, name)
    assert sums.shape == (c.B, c.groups * c.M) + c.out_hw
    if c.ep is not None:
        t = torch.tensor(sums)
        if c.ep[0]:
            t = t + torch.tensor(dt["bias"], dtype=torch.float64)[None, :, None, None]
        if c.ep[1]:
            t = torch.nn.functional.leaky_relu(t, c.ep[2]) * c.ep[3]
        _scale_check(t.numpy(), dt["ref"], name + " tail")
    print(c, c.plan()["pick"], c.plan()["cls_splitk"])
    _yardstick(name, "y", dt["ref"], dt["cap"], dt["e32"], dt["r32"])


@pytest.mark.parametrize("name", WGRAD_NAMES)
def test_wgrad_reference_equals_autograd_float64_and_the_yardstick_is_inside_the_cap(name):
    c = cc.WGRAD_BY_NAME[name]
    dt = cc.wgrad_data(name)
    G = np.nan_to_num(dt["G"])
    _scale_check(cc._torch_wgrad(dt["A"], G, c, torch.float64, autograd=True), dt["ref"], name)
    if c.grow:
        assert np.isnan(dt["G"][..., c.reach[0]:, :]).all() and np.isnan(dt["G"][..., :, c.reach[1]:]).all()
        assert np.isfinite(dt["G"][..., :c.reach[0], :c.reach[1]]).all()
    if not c.grow and (c.GH + 2 * c.p - c.k) // c.s + 1 == c.PH and (c.GW + 2 * c.p - c.k) // c.s + 1 == c.PW:
        # the layer itself: autograd through F.conv2d on G with its padding
        w = torch.zeros((c.groups * c.Ca, c.Cg, c.k, c.k), dtype=torch.float64, requires_grad=True)
        torch.nn.functional.conv2d(torch.tensor(G, dtype=torch.float64), w, None, c.s, c.p, 1, c.groups).backward(
            torch.tensor(dt["A"], dtype=torch.float64))
        _scale_check(w.grad.numpy(), dt["ref"], name + " layer")
    print(c, c.plan())
    _yardstick(name, "dw", dt["ref"], dt["cap"], dt["e32"], dt["r32"])


@pytest.mark.parametrize("name", BWD_NAMES)
def test_bwd_references_equal_autograd_float64(name):
    import torch.nn.functional as F
    c = cc.BWD_BY_NAME[name]
    dt = cc.bwd_data(name)
    x = torch.tensor(dt["x"], dtype=torch.float64, requires_grad=True)
    w = torch.tensor(dt["w"], dtype=torch.float64, requires_grad=True)
    y = (F.conv_transpose2d if c.transposed else F.conv2d)(x, w, None, c.s, c.p, groups=c.groups)
    assert tuple(y.shape[2:]) == (c.yh, c.yw)
    y.backward(torch.tensor(dt["gy"], dtype=torch.float64))
    _scale_check(x.grad.numpy(), dt["gx_ref"], name + " gx")
    _scale_check(w.grad.numpy(), dt["dw_ref"], name + " dw")
    print(c)
    _yardstick(name, "gx", dt["gx_ref"], dt["gx_cap"], dt["gx_e32"], dt["gx_r32"])
    _yardstick(name, "dw", dt["dw_ref"], dt["dw_cap"], dt["dw_e32"], dt["dw_r32"])


def test_case_data_is_reproducible_and_the_weights_have_no_symmetry():
    for fn, name in ((cc.conv_data, "g_k3_s1"), (cc.wgrad_data, "w_k3_s1"), (cc.bwd_data, "b_conv_t2")):
        a = fn(name)
        fn.cache_clear()
        b = fn(name)
        assert a is not b and all(np.array_equal(a[k], b[k], equal_nan=True) for k in a if isinstance(a[k], np.ndarray))
        assert not a["ref" if "ref" in a else "gx_ref"].flags.writeable
    assert cc.conv_data("g_k3_s1")["x"].tobytes() != cc.conv_data("g_k3_s2")["x"].tobytes()
    w = cc.conv_data("g_k3_s1")["w"]
    scale = np.abs(w).max()
    assert np.abs(w - w[..., ::-1, ::-1]).max() > 0.1 * scale and np.abs(w - w.transpose(0, 1, 3, 2)).max() > 0.1 * scale
    assert w.dtype == np.float32 and abs(float(w.std()) * np.sqrt(5 * 9) - 1) < 0.2


class _Mod:
    def __init__(self, k, s, p):
        self.kernel_size, self.stride, self.padding = (k, k), (s, s), (p, p)
        self.dilation, self.groups, self.padding_mode, self.output_padding = (1, 1), 1, "zeros", (0, 0)


class _Input:       # what supported() asks of x: a float32 NCHW tensor on the device
    is_cuda, dtype, shape = True, torch.float32, (1, 3, 12, 13)

    def dim(self):
        return 4


def test_supported_agrees_with_the_plans():
    """Every (k, stride, pad, transposed) supported() accepts plans its forward, data gradient and weight gradient; k = 5
    at stride 2 is the one geometry conv_launch rejects (scatter classes of 9 / 6 / 6 / 4 taps) and supported() refuses
    it for both module kinds, so that networks.py takes its torch route."""
    from gan2shape_amd.op import conv
    x = _Input()
    accepted, refused = [], []
    for k in range(1, 7):
        for s in (1, 2, 3):
            for p in range(k + 1):
                ok = conv.supported(_Mod(k, s, p), x)
                (accepted if ok else refused).append((k, s, p))
                if not ok:
                    continue
                for transposed in (False, True):
                    H, W = 12, 13
                    oh, ow = cc.out_size(H, W, k, s, p, transposed)
                    cc.plan_conv(1, 3, 4, H, W, k, s, p, transposed, not transposed)              # forward
                    cc.plan_conv(1, 4, 3, oh, ow, k, s, p, not transposed, transposed, H, W)      # data gradient
                    cc.plan_wgrad(1, 3 if transposed else 4, 4 if transposed else 3, *((H, W) if transposed else (oh, ow)), k)
    assert (5, 2, 2) in refused and (5, 1, 2) in accepted and (4, 2, 1) in accepted and (3, 2, 0) in accepted
    assert all(k <= 5 and s <= 2 and p < k for k, s, p in accepted)
    assert sorted(set(refused) - {(5, 2, p) for p in range(5)}) == sorted((k, s, p) for k, s, p in refused
                                                                          if k > 5 or s > 2 or p >= k)
    for transposed in (False, True):        # and the plans do reject what supported() now refuses
        with pytest.raises(cc.Rejected):
            oh, ow = cc.out_size(12, 13, 5, 2, 2, transposed)
            cc.plan_conv(1, 3, 4, 12, 13, 5, 2, 2, 1, 0) if transposed else cc.plan_conv(1, 4, 3, oh, ow, 5, 2, 2, 1, 0, 12, 13)
