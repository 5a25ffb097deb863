"""The case table of tests/upfirdn_cases.py, without a GPU: every case reaches the path and the number of plane-loop
turns it is listed for, the table covers what it claims, its float64 reference agrees with the two other statements
of upfirdn2d the repository has and with its own transpose, and the float32 yardstick of every case is printed (-s)."""
import numpy as np
import pytest

import upfirdn_cases as uc
from oracle import capi


def _launch(name):
    major, _, _, up, down, _, kh, kw, oh, ow = uc.geometry(name)
    p = uc.path(up, down, kh, kw, ow)
    return p, uc.turns(major, oh, ow, p)


def _adjoint_launch(name):
    major, _, _, _, _, _, kh, kw, _, _ = uc.geometry(name)
    up, down, _, oh, ow = uc.adjoint_geometry(name)
    p = uc.path(up, down, kh, kw, ow)
    return p, uc.turns(major, oh, ow, p)


def test_every_case_takes_the_path_and_the_turns_it_is_listed_for():
    for name, group, shape, up, down, pad, path, turns, adj in uc.CASES:
        assert _launch(name) == (path, turns), name
        assert shape[0] * shape[1] >= 2, name
        _, _, _, _, _, _, _, _, oh, ow = uc.geometry(name)
        if path != "generic":
            assert oh % uc.TILE[path][1] != 0, name
        if name in uc.ADJOINT:
            assert _adjoint_launch(name)[0] == adj, (name, _adjoint_launch(name))
        else:
            assert adj is None, name


def test_edge_cases_sit_on_the_boundaries_of_launch_tiled():
    for group, down in (("d1", 1), ("d2", 2)):
        widths = {}
        for name in uc.NAMES:
            if uc.CASE[name][1] == group:
                _, H, W, _, d, _, _, _, oh, ow = uc.geometry(name)
                assert d == (down, down) and 17 <= oh <= 23 and oh % 4 != 0, name
                widths[ow] = (uc.CASE[name][6], H, W)
        assert tuple(sorted(widths)) == uc.EDGE_W
        for a, b in uc.BOUNDARY_PAIRS:
            assert widths[a][0] != widths[b][0], (a, b)
        if down == 2:       # both parities of the input size
            assert {w[1] % 2 for w in widths.values()} == {0, 1} and {w[2] % 2 for w in widths.values()} == {0, 1}
    up2 = [uc.geometry(n) for n in uc.NAMES if uc.CASE[n][1] == "up2"]
    assert {31, 33, 130} <= {g[9] for g in up2} and {g[1] % 2 for g in up2} == {0, 1}
    assert {(2, 1), (1, 2)} <= {g[5][:2] for g in up2}


def test_the_plane_loop_cases_turn_as_the_issue_of_their_grid_says():
    assert _launch("pl_t32") == ("t32", 3) and 4101 % 2048 == 5            # two full turns and a partial one
    assert _launch("pl_up2") == ("up2", 2) and _launch("pl_t160") == ("t160", 2)
    assert _launch("pl_nba") == _launch("pl_nba_ps") == ("t32", 3)
    assert _adjoint_launch("pl_t32") == ("t32", 3) and _adjoint_launch("pl_t160") == ("t160", 2)
    for name in uc.PLANE:
        major, H, W, *_ = uc.geometry(name)
        assert major * H * W * 4 < 20e6, name      # bytes of the input


@pytest.mark.parametrize("path", [p for p in uc.TILED if p != "up2"])
def test_every_tiled_path_occurs_under_both_down_values_in_every_role(path):
    fwd = {uc.geometry(n)[4][0] for n in uc.FORWARD if uc.CASE[n][6] == path}
    adj = {uc.adjoint_geometry(n)[1][0] for n in uc.ADJOINT if uc.CASE[n][8] == path}
    assert fwd == {1, 2} and adj == {1, 2}, (fwd, adj)


@pytest.mark.parametrize("path", uc.TILED)
def test_every_tiled_path_occurs_with_f16_each_epilogue_and_as_an_adjoint(path):
    assert any(uc.CASE[n][6] == path for n in uc.F16)
    assert {uc.EPILOGUE[n][0] for n in uc.NBA if uc.CASE[n][6] == path} == {"nba", "nba_ps"}
    assert any(uc.CASE[n][8] == path for n in uc.ADJOINT)
    assert any(uc.CASE[n][6] == path for n in uc.FORWARD)


def test_the_rest_of_the_table():
    assert any(uc.CASE[n][6] == "generic" for n in uc.F16)
    assert {uc.EPILOGUE[n] for n in uc.NBA} >= {(e, a) for e in ("nba", "nba_ps") for a in (0.2, 0.0)}
    for n in uc.NBA:
        assert uc.CASE[n][2][1] == 3 and uc.CASE[n][2][0] >= 2, n
    for rate in ((1, 1), (1, 2), (2, 1)):       # (up, down): the four pads on a tiled path
        pads = {uc.CASE[n][5] for n in uc.FORWARD if (uc.CASE[n][3], uc.CASE[n][4]) == rate and uc.CASE[n][6] in uc.TILED}
        assert {(1, 1), (2, 2), (2, 1)} <= pads and any(min(p) < 0 for p in pads), (rate, pads)
        assert any(uc.CASE[n][1] == "small" and (uc.CASE[n][3], uc.CASE[n][4]) == rate for n in uc.NAMES)
    k = uc.data("d1_w47")["k"]
    assert np.abs(k - k[::-1, ::-1]).max() > 1e-3 and np.abs(k - k.T).max() > 1e-3      # a flip or a transpose shows


@pytest.mark.parametrize("name", uc.NAMES)
def test_complementary_pads_give_back_the_input_size(name):
    _, H, W, *_ = uc.geometry(name)
    _, _, _, oh, ow = uc.adjoint_geometry(name)
    assert (oh, ow) == (H, W)


@pytest.mark.parametrize("name", uc.NAMES)
def test_reference_against_the_other_statements_and_float32_yardstick(name):
    """`reference` equals op/cpu_tensors.upfirdn2d in float64 to 1e-12 of scale (where that can express the case) and
    the C oracle to float32 rounding; prints the path, the turns and e32."""
    import torch
    from gan2shape_amd.op import cpu_tensors
    _, group, shape, up, down, pad, *_ = uc.CASE[name]
    dt = uc.data(name)
    x, k = dt["x"].astype(np.float64), dt["k"]
    ref = uc.reference(x, k, up, down, pad)
    scale = np.abs(ref).max()
    if name not in uc.PLUGIN_ONLY:
        got = cpu_tensors.upfirdn2d(torch.tensor(x), torch.tensor(k, dtype=torch.float64), up, down, pad).numpy()
        assert got.shape == ref.shape and np.abs(got - ref).max() <= 1e-12 * scale
    c = capi.upfirdn2d(x, k, uc._pair(up), uc._pair(down), uc._pad4(pad))
    np.testing.assert_allclose(c, ref, rtol=1e-5, atol=1e-6)
    line = f"{name} {shape} up={up} down={down} pad={pad} out={ref.shape[-2:]} path={_launch(name)} e32={dt['e32']:.3e}"
    assert np.isfinite(dt["e32"]) and 0 < dt["e32"] < 1e-6
    if name in uc.ADJOINT:
        line += f" adjoint={_adjoint_launch(name)} e32_adj={dt['e32_adj']:.3e}"
        assert 0 < dt["e32_adj"] < 1e-6
    print(line)


@pytest.mark.parametrize("name", uc.FORWARD + ["pl_t32", "pl_up2"])
def test_reference_adjoint_is_the_transpose_of_reference(name):
    _, _, shape, up, down, pad, *_ = uc.CASE[name]
    rng = np.random.default_rng(7)
    x = rng.standard_normal(shape)
    k = uc.data(name)["k"].astype(np.float64)
    y = uc.reference(x, k, up, down, pad)
    g = rng.standard_normal(y.shape)
    lhs, rhs = float((y * g).sum()), float((x * uc.reference_adjoint(g, k, up, down, pad, shape[2:])).sum())
    assert abs(lhs - rhs) <= 1e-12 * max(np.abs(y * g).sum(), 1.0)
