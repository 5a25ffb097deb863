"""The twice-differentiable route of the ADA augmentation without a GPU: `order=2` on CPU tensors (the torch
composition augment._augment_twice) against `order=1` and the reference's float64 goldens, the new golden file, the
second-order quantity of ada_twice_cases.py, and the argument checks of g2s_ada_warp_down_bwd_gather (which precede any
launch)."""
import ctypes

import pytest
import torch

import ada_cases as ac
import ada_twice_cases as tc


@pytest.fixture(scope="module")
def aug():
    import gan2shape_amd  # noqa: F401
    from gan2shape_amd import augment
    return augment


def test_the_new_fixture_holds_its_cases():
    assert [str(n) for n in tc.data()["names"]] == tc.NEW and len(tc.names()) == 11
    for name in tc.NEW:
        c = tc.case(name)
        for key in ("x", "G", "C", "pads", "gy", "y", "gx", "e32_y", "e32_gx"):
            assert f"{name}.{key}" in tc.data(), (name, key)
        assert c["x"].shape == (2, 3, 20, 28) and c["G"].shape == (2, 3, 3) and c["C"].shape == (2, 4, 4)
        assert c["y"].dtype == torch.float64 and c["gx"].dtype == torch.float64
        assert 0 < c["e32_y"] < 1e-4 and 0 < c["e32_gx"] < 1e-4
    assert tc.case("scale2.5")["pads"] == (27, 27, 19, 19)          # the clamp at size - 1 on both axes


@pytest.mark.parametrize("name", tc.NEW)
def test_torch_composition_float64_matches_the_new_golden(aug, name):
    """As test_ada_cpu.py holds the eight old cases: float64, 144 products of O(1) per pixel, below 1e-12."""
    c = tc.case(name)
    y, gx = ac.run(aug, c, c["x"].double().requires_grad_(True))
    ey, eg = float((y - c["y"]).abs().max()), float((gx - c["gx"]).abs().max())
    print(name, "float64 max abs error: y", ey, "gx", eg)
    assert y.dtype == torch.float64 and ey < 1e-12 and eg < 1e-12


@pytest.mark.parametrize("name", tc.names())
def test_order_2_equals_order_1_on_the_cpu(aug, name):
    """Two torch compositions of the same arithmetic (grid_sample against four gathers) in float64: value and first
    gradient agree to summation order, and both meet the golden."""
    c = tc.case(name)
    out = {}
    for order in (1, 2):
        x = c["x"].double().requires_grad_(True)
        y = tc.public(aug, c, order)(x)
        gx, = torch.autograd.grad(y, x, c["gy"].double())
        out[order] = (y.detach(), gx)
    dy, dg = float((out[1][0] - out[2][0]).abs().max()), float((out[1][1] - out[2][1]).abs().max())
    print(name, "order 2 - order 1: y", dy, "gx", dg)
    assert dy < 1e-12 and dg < 1e-12
    assert float((out[2][0] - c["y"]).abs().max()) < 1e-12 and float((out[2][1] - c["gx"]).abs().max()) < 1e-12


@pytest.mark.parametrize("name", tc.SECOND_CASES)
def test_second_order_on_the_cpu_is_the_composition(aug, name):
    """On a CPU tensor order=2 IS _augment_twice (dtrain keeps the name as an alias): the second-order quantity is
    finite and equal."""
    from gan2shape_amd import dtrain
    assert dtrain._augment_twice is aug._augment_twice
    c = tc.case(name)
    ref = tc.second_reference(aug, name)
    x = c["x"].double().requires_grad_(True)
    g, q, gg = tc.second_order(tc.public(aug, c, 2), x, tc.weight(c).double())
    assert bool(torch.isfinite(g).all()) and bool(torch.isfinite(q)) and bool(torch.isfinite(gg).all())
    assert float(gg.abs().max()) > 0
    scale = float(ref["gg"].abs().max())
    assert float((g - ref["g"]).abs().max()) <= 1e-12 * scale
    assert float((q - ref["q"]).abs()) <= 1e-12 * float(ref["q"].abs())
    assert float((gg - ref["gg"]).abs().max()) <= 1e-12 * scale
    assert ref["e32_g"] > 0 and ref["e32_q"] > 0 and ref["e32_gg"] > 0


def test_order_is_checked_and_float64_cuda_free_route(aug):
    c = tc.case("rot30")
    with pytest.raises(ValueError, match="order"):
        aug.augment(c["x"], 0.5, (c["G"], c["C"]), order=3)
    with pytest.raises(ValueError, match="order"):
        aug.random_apply_affine(c["x"], 1.0, c["G"], order=0)
    y, C = aug.random_apply_color(c["x"], 0.5, c["C"], order=2)
    assert torch.equal(y, aug.random_apply_color(c["x"], 0.5, c["C"])[0]) and C is c["C"]


def test_augment_differentiable_on_the_cpu_takes_the_composition_either_way(aug):
    from gan2shape_amd import dtrain
    c = tc.case("batch3")
    a, (G, C) = dtrain.augment_differentiable(c["x"], 0.5, (c["G"], c["C"]))
    b, _ = dtrain.augment_differentiable(c["x"], 0.5, (c["G"], c["C"]), composed=True)
    assert G is c["G"] and C is c["C"] and torch.equal(a, b)


def test_the_commands_take_the_deterministic_flag():
    from gan2shape_amd import dtrain, train
    args = dtrain.build_parser().parse_args(["--ckpt", "c", "--size", "8", "--data", "d", "--out", "o", "--deterministic"])
    assert args.deterministic is True
    assert dtrain.build_parser().parse_args(["--ckpt", "c", "--size", "8", "--data", "d", "--out", "o"]).deterministic is False
    assert train.build_parser().parse_args(["--size", "8", "--data", "d", "--out", "o", "--deterministic"]).deterministic is True


def test_gather_symbol_and_argument_checks(aug):
    """Every check precedes the first launch, so it runs without a GPU (the pointers are never followed); the gather
    has no deterministic refusal."""
    from gan2shape_amd import lib
    assert "g2s_ada_warp_down_bwd_gather" in lib.SIGNATURES
    L = lib.load()
    assert L.g2s_abi_version() == 1
    host = (ctypes.c_float * 64)()
    ok = ctypes.c_void_p(ctypes.addressof(host))

    def gather(gy=ok, g=ok, cm=ok, gx2=ok, ga=ok, B=2, C=3, H=16, W=12):
        return L.g2s_ada_warp_down_bwd_gather(gy, g, cm, gx2, ga, B, C, H, W, 64, 48, None)
    for kw in ({"gy": None}, {"g": None}, {"gx2": None}, {"ga": None}, {"C": 1}, {"C": 4}, {"B": 0}, {"W": -2},
               {"B": 65536, "C": 1, "cm": None}):
        rc = gather(**kw)
        assert rc == -1 and b"g2s_ada_warp_down_bwd_gather" in L.g2s_last_error(), (kw, rc, L.g2s_last_error())
        with pytest.raises(lib.G2SError):
            lib.check(rc)
