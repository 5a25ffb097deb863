"""The case tables of tests/modconv_cases.py, without a GPU: every row's plan carries the labels the row claims and the
tables reach every label of the required sets below; the float64 reference equals torch's float64 convolutions with the
scales folded in; the float32 yardstick lies inside the analytic cap; the data is reproducible; no fp16 operand image
is subnormal, zero or infinite; the library's own g2s_modconv_needs_zero and argument validation agree with the plans;
and the bound has teeth: every mutant of modconv_cases.mutants exceeds it at least tenfold somewhere."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv2d_cases as cc
import modconv_cases as mc

F16_NAMES = [c.name for c in mc.F16]
F32_NAMES = [c.name for c in mc.F32]

REQUIRED_F16 = (
    [f"{b}:{s}" for b in mc.BODIES for s in ("scale", "noscale")]
    + ["quad:fwd", "quad:rev", "quad:is2", "quad:W4", "quad:W5+", "H!=W"]
    + ["quad:sub", "quad:full", "quad:partial", "narrow:partial", "p4:partial", "p2:partial", "p1:partial"]
    + ["tile0:forced", "tile2:heuristic", "tile2:forced", "tile0:heuristic", "pick1->2", "tile1:forced"]
    + ["M<64", "M%64", "M%128", "N%tile", "spans-batch", "ragged-classes", "early-exit"]
    + ["split:1", "split:heuristic", "split:forced", "split:forced:2", "split:forced:3", "split:clipped",
       "split:empty-slices", "split:det"]
    + ["ep:none", "ep:out_scale"] + [f"ep:{k}:{w}" for k in ("bias", "bias+act", "act") for w in ("kernel", "deferred")]
    + ["holes", "overwrites", "needs-zero"])
REQUIRED_F32 = ["noise:kernel", "noise:deferred", "thin:just-eligible", "thin:just-not", "thin:noise-keeps-mfma",
                "promise:y_is_zero", "T9:scale", "T9:noscale", "T4:scale", "T2:scale", "T1:scale", "holes", "needs-zero",
                "overwrites", "split:heuristic", "split:det", "ep:out_scale", "ep:bias:kernel", "ep:bias+act:kernel",
                "ep:bias+act:deferred"]


def test_every_row_reaches_what_it_claims_and_the_tables_every_label():
    for table, required in ((mc.F16, REQUIRED_F16), (mc.F32, REQUIRED_F32)):
        reached = set()
        for c in table:
            got = mc.labels(c, c.plan())
            assert c.claims and set(c.claims) <= got, (c, sorted(set(c.claims) - got))
            reached |= got
        claimed = set().union(*(c.claims for c in table))
        assert not [l for l in required if l not in reached], [l for l in required if l not in reached]
        assert not [l for l in required if l not in claimed], [l for l in required if l not in claimed]
    assert 35 <= len(mc.F16) <= 60 and 12 <= len(mc.F32) <= 24


def test_what_the_plans_say_about_the_named_rows():
    pl = mc.BY_NAME["heur_tile0"].plan()
    assert (pl["pick"], pl["tiles"], pl["splitk"], pl["source"]) == (0, 512, 1, "heuristic")
    pl = mc.BY_NAME["heur_1to2"].plan()
    assert pl["remapped"] and pl["pick"] == 2 and (pl["KBM"], pl["KBN"]) == (64, 64)
    assert mc.BY_NAME["heur_tile0"].Cr <= 8 and mc.BY_NAME["heur_1to2"].Cr <= 8
    # tile 1 forced: a grid for 128x64 tiles, the 128x128 instance: 2 x 3 workgroups where 2 x 2 have work
    c = mc.BY_NAME["t1_forced"]
    pl = c.plan()
    assert (pl["BM"], pl["BN"], pl["KBM"], pl["KBN"], pl["tiles"]) == (128, 64, 128, 128, 6)
    assert cc.cdiv(c.M, 128) * cc.cdiv(pl["nmax"], 128) == 4
    for tile in (3, 4):
        with pytest.raises(mc.Rejected):
            c.plan(tile=tile)
    # the split-K count comes from the fp32 kernel's K tiles, the slices from the fp16 kernel's own
    pl = mc.BY_NAME["s_heur"].plan()
    assert (pl["kt_min"], pl["splitk"], pl["ktiles16"], pl["per16"], pl["empty"]) == (17, 2, [9], [5], [[]])
    pl = mc.BY_NAME["s_heur_up"].plan()
    assert (pl["kt_min"], pl["splitk"], pl["ktiles16"]) == (17, 2, [33, 17, 17, 9]) and not any(pl["empty"])
    pl = mc.BY_NAME["s_clipped"].plan()
    assert (pl["asked"], pl["kt_min"], pl["splitk"], pl["ktiles16"], pl["empty"]) == (64, 3, 3, [2], [[2]])
    pl = mc.BY_NAME["s_empty"].plan()
    assert pl["asked"] == pl["splitk"] == 4 <= pl["kt_min"] and pl["ktiles16"] == [2] and pl["empty"] == [[2, 3]]
    pl = mc.BY_NAME["s_empty_up"].plan()
    assert pl["splitk"] == 3 == pl["kt_min"] and pl["bodies"] == ["p4", "p2", "p2", "p1"] and pl["empty"][3] == [2]
    for name in ("s_forced2", "s_forced3", "s_forced2_up", "s_forced3_up", "s_forced2_n"):
        pl = mc.BY_NAME[name].plan()
        assert pl["splitk"] == pl["asked"] > 1 and not any(pl["empty"]), name
    for name in ("s_det", "s_det_forced"):
        c = mc.BY_NAME[name]
        assert c.plan(det=False)["splitk"] > 1 and c.plan()["splitk"] == 1
    # bodies by class and width
    assert [mc.body_of(9, 4), mc.body_of(9, 3), mc.body_of(4, 3), mc.body_of(2, 9), mc.body_of(1, 1)] == ["quad", "narrow", "p4", "p2", "p1"]
    assert [mc.f16_cpt(9, True), mc.f16_cpt(9, False), mc.f16_cpt(4, False), mc.f16_cpt(2, False), mc.f16_cpt(1, False)] == [4, 8, 8, 16, 32]
    # the adjoint of the stride-1 3x3 steps through x downwards (the reversed triple), the gathers upwards
    for name, rev in (("q_rev", True), ("q_fwd", False), ("q_down", False), ("q_up_t", False)):
        taps = mc.BY_NAME[name].plan()["classes"][0]["taps"]
        assert (taps[0][1] > taps[2][1]) == rev and taps[0][0] == taps[1][0] == taps[2][0], name


@pytest.mark.parametrize("name", list(mc.SWEEP))
def test_the_sweep_reaches_every_tile_under_every_split_form(name):
    c, bodies = mc.SWEEP[name]
    splits = mc.sweep_splits(c)
    assert splits[:3] == (1, 2, 3) and splits[3] > 3
    seen = set()
    for tile in mc.SWEEP_TILES:
        for sk in splits:
            pl = c.plan(tile=tile, sk=sk)
            got = mc.labels(c, pl)
            assert set(pl["bodies"]) == set(bodies) and pl["pick"] == tile and pl["splitk"] == sk, (name, tile, sk)
            assert (sk == splits[3]) <= ("split:empty-slices" in got) and "split:clipped" not in got, (name, tile, sk)
            seen |= got
    assert {f"tile{t}:forced" for t in range(3)} | {"split:1", "split:forced:2", "split:forced:3", "split:empty-slices"} <= seen
    assert set().union(*(b for _, b in mc.SWEEP.values())) == set(mc.BODIES)


def test_no_row_of_the_tuned_table_matches_and_the_thin_rule():
    rows = mc.modconv_tuned_rows()
    assert len(rows) >= 40
    for c in mc.F32:
        assert c.H != c.W or (c.B, c.Cin, c.Cout, c.H, c.k, c.mode, c.tr) not in rows, c
    assert mc.thin_conv_eligible(1, 4, 16, 256, 256, 1, 0) and mc.thin_conv_eligible(8, 3, 128, 128, 128, 1, 0)
    for args in ((1, 4, 16, 256, 256, 3, 0), (1, 4, 16, 256, 256, 1, 1), (1, 5, 16, 256, 256, 1, 0), (1, 4, 15, 256, 256, 1, 0),
                 (1, 4, 16, 257, 257, 1, 0), (1, 4, 16, 256, 255, 1, 0)):
        assert not mc.thin_conv_eligible(*args), args
    assert mc.BY_NAME["thin_yes"].plan()["thin"] and not mc.BY_NAME["thin_yes"].plan(tile=2)["thin"]
    assert not any(mc.BY_NAME[n].plan()["thin"] for n in F32_NAMES if n != "thin_yes")


def _torch_f64(c, op, xr, wr):
    """F.conv2d / F.conv_transpose2d in float64 with the input scale folded into x and the output scale applied after."""
    x = torch.tensor(xr, dtype=torch.float64)
    w = torch.tensor(wr, dtype=torch.float64)                       # [Cout, Cin, k, k]
    if not c.adj:
        y = F.conv2d(x, w if not c.tr else w.transpose(0, 1), None, c.s, c.p)
    else:
        y = F.conv_transpose2d(x, w.transpose(0, 1) if not c.tr else w, None, c.s, c.p)
    if op["os"] is not None:
        y = y * torch.tensor(op["os"], dtype=torch.float64)[:, :, None, None]
    if c.noise:
        y = y + float(op["noise_w"][0]) * torch.tensor(op["noise"], dtype=torch.float64)
    if c.ep is not None:
        if c.ep[0]:
            y = y + torch.tensor(op["bias"], dtype=torch.float64)[None, :, None, None]
        if c.ep[1]:
            y = F.leaky_relu(y, c.ep[2]) * c.ep[3]
    return y.numpy()


@pytest.mark.parametrize("name", F16_NAMES + F32_NAMES + list(mc.SWEEP))
def test_reference_equals_torch_float64_and_the_yardstick_is_inside_the_cap(name):
    c = mc.BY_NAME[name]
    dt = mc.data(name)
    xr, wr = mc.f16_images(c, dt) if c.route == "f16" else mc.f32_images(c, dt)
    want = _torch_f64(c, dt, xr, wr)
    assert want.shape == dt["ref"].shape == (c.B, c.M) + c.out_hw, (name, want.shape, dt["ref"].shape)
    assert np.abs(want - dt["ref"]).max() <= 1e-12 * np.abs(dt["ref"]).max(), name
    assert np.isfinite(dt["ref"]).all() and 0 < dt["e32"] < 1e-5, (name, dt["e32"])
    err = np.abs(dt["r32"].astype(np.float64) - dt["ref"])
    assert (err <= dt["cap"]).all(), (name, float((err / np.maximum(dt["cap"], 1e-300)).max()))
    print(f"{c!r}: e32 {dt['e32']:.3e}, float32 error / cap at most {float((err / np.maximum(dt['cap'], 1e-300)).max()):.3f}")


def test_case_data_is_reproducible_and_the_weights_have_no_symmetry():
    a = mc.data("q_rev")
    mc.data.cache_clear()
    b = mc.data("q_rev")
    assert a is not b and all(np.array_equal(a[k], b[k]) for k in a if isinstance(a[k], np.ndarray))
    assert not a["ref"].flags.writeable and not a["x"].flags.writeable
    assert mc.data("q_rev")["x"].tobytes() != mc.data("q_fwd")["x"].tobytes()
    w = a["w"]
    assert w.dtype == np.float32 and abs(float(w.std()) - 1) < 0.2
    assert np.abs(w - w[..., ::-1]).max() > 0.1 * np.abs(w).max() and np.abs(w - w.transpose(0, 1, 3, 2)).max() > 0.1 * np.abs(w).max()
    s = mc.data("q_fwd")["s"]
    assert s.min() >= 0.4 and s.max() <= 1.6 and s.std() > 0.15


@pytest.mark.parametrize("name", F16_NAMES + list(mc.SWEEP))
def test_every_fp16_operand_image_is_a_normal_number(name):
    """The condition the fp16 rows are built to: no image is subnormal, zero by underflow or infinite, under the
    contract's rounding and under the mutants' (so that a mutant differs by the rounding alone)."""
    c = mc.BY_NAME[name]
    dt = mc.data(name)
    assert np.abs(dt["x"]).min() >= mc.FLOOR_OPERAND and np.abs(dt["w"]).min() >= mc.FLOOR_OPERAND
    images = {"contract": mc.f16_images(c, dt), "truncate": mc.f16_images(c, dt, "truncate"),
              "x before the scale": (dt["x"].astype(np.float16).astype(np.float64),)}
    for how, imgs in images.items():
        for img in imgs:
            assert np.isfinite(img).all() and np.abs(img).min() >= mc.F16_MIN_NORMAL and np.abs(img).max() <= 65504.0, (name, how)
    # the contract's images are halves, and truncation never exceeds the operand
    xr, wr = mc.f16_images(c, dt)
    assert np.array_equal(xr, xr.astype(np.float16).astype(np.float64)) and np.array_equal(wr, wr.astype(np.float16).astype(np.float64))
    xt, wt = mc.f16_images(c, dt, "truncate")
    assert np.array_equal(wt, wt.astype(np.float16).astype(np.float64)) and (np.abs(wt) <= np.abs(dt["w"])).all()
    assert np.array_equal(xt, xt.astype(np.float16).astype(np.float64)) and (np.abs(xt) <= np.abs(xr)).all()
    assert (np.abs(wr - dt["w"]) <= 2.0 ** -11 * np.abs(dt["w"])).all() and (np.abs(wt - dt["w"]) < 2.0 ** -10 * np.abs(dt["w"])).all()


@pytest.mark.parametrize("name", F16_NAMES)
def test_the_bound_has_teeth(name):
    """Every mutant a row gives rise to — unrounded operands, float16(x) * s, truncation, a lost border tap, the scale
    dropped on a partial last K tile, the last K tile omitted, the adjoint's triple not reversed — leaves the bound by a
    factor of at least 10 at some element; a row that claims a label has the mutants that target it."""
    c = mc.BY_NAME[name]
    dt = mc.data(name)
    bound = mc.case_bound(name)
    muts = mc.mutants(c, dt)
    claims = set(c.claims)
    assert {"unrounded", "truncate"} <= set(muts) and (("scale-after-round" in muts) == c.scale)
    if claims & {"quad:W4", "quad:W5+", "quad:rev"}:
        assert len([m for m in muts if m.startswith("border-tap:")]) == 4, (name, sorted(muts))
    if "quad:rev" in claims:
        assert "rev-not-swapped" in muts
    for body in mc.BODIES:
        if f"{body}:partial" in claims:
            assert f"last-tile-omitted:{body}" in muts and ((f"scale-dropped:{body}" in muts) == c.scale), (name, body, sorted(muts))
    if claims & {"split:heuristic", "split:forced", "split:forced:2", "split:forced:3", "split:clipped", "split:empty-slices", "split:det"}:
        assert any(m.startswith("last-tile-omitted:") for m in muts), (name, sorted(muts))
    for m, (_, ref) in muts.items():
        excess = np.abs(ref - dt["ref"]) / np.maximum(bound, 1e-300)
        excess = np.where((bound == 0) & (ref == dt["ref"]), 0.0, excess)
        assert excess.max() >= 10.0, (name, m, float(excess.max()))
    print(name, {m: f"{float((np.abs(r - dt['ref']) / np.maximum(bound, 1e-300)).max()):.3g}" for m, (_, r) in muts.items()})


def test_needs_zero_and_argument_validation_of_the_library():
    """g2s_modconv_needs_zero (which launches nothing) agrees with the plan of every fp32 row under the row's tuning
    state; k = 2 and an unknown mode are refused before any launch."""
    import gan2shape_amd  # noqa: F401
    from gan2shape_amd import lib
    L = lib.load()
    try:
        for c in mc.F32:
            prev = lib.set_deterministic(c.det)
            try:
                assert L.g2s_modconv_tune(c.tile, c.sk) == 0
                got = L.g2s_modconv_needs_zero(c.B, c.Cin, c.Cout, c.H, c.W, c.k, c.mode, c.tr, int(c.scale or c.oscale),
                                               int(c.fused))
            finally:
                lib.set_deterministic(prev)
            assert got == int(c.plan()["needs_zero"]), (c, got)
            assert ("needs-zero" in mc.labels(c, c.plan())) == bool(got)
        L.g2s_modconv_tune(-1, -1)
        d = (lib.C.c_float * 4)()
        for k, mode, what in ((2, 0, b"kernel size"), (3, 3, b"mode"), (3, -1, b"mode")):
            assert L.g2s_modconv_needs_zero(1, 4, 4, 8, 8, k, mode, 0, 1, 0) < 0 and what in L.g2s_last_error(), (k, mode)
            rc = L.g2s_modconv(d, d, None, None, None, None, None, d, 1, 4, 4, 8, 8, k, mode, 0, 0, 0.0, 1.0, 0, None)
            assert rc != 0 and what in L.g2s_last_error(), (k, mode)
            rc = L.g2s_modconv_f16(d, d, None, None, None, d, 1, 4, 4, 8, 8, k, mode, 0, 0, 0.0, 1.0, None)
            assert rc != 0 and what in L.g2s_last_error(), (k, mode)
    finally:
        L.g2s_modconv_tune(-1, -1)
