"""ADA augmentation without a GPU: the torch composition of gan2shape_amd.augment against the reference's float64
results (tests/golden/ada.npz), the host-side padding, the sampled matrices, AdaptiveAugment, and the argument
checks of the four C entries (which precede any launch)."""
import ctypes

import numpy as np
import pytest
import torch

import ada_cases as ac


@pytest.fixture(scope="module")
def aug():
    import gan2shape_amd  # noqa: F401
    from gan2shape_amd import augment
    return augment


def test_the_fixture_holds_every_case():
    assert ac.names() == ["identity16", "rot30", "aniso_shift", "flip_rot90", "pad_clamp", "batch3", "tiles40x24",
                          "gray"]
    c = ac.case("pad_clamp")
    assert c["pads"] == (15, 15, 15, 15) and c["x"].shape[2:] == (16, 16)         # the clamp at size - 1
    assert ac.case("batch3")["x"].shape == (3, 3, 20, 28) and ac.case("gray")["x"].shape[1] == 1
    assert ac.case("identity16")["pads"] == (6, 6, 6, 6)                          # the filter's pads alone
    for name in ac.names():
        c = ac.case(name)
        assert 0 < c["e32_y"] < 1e-4 and 0 < c["e32_gx"] < 1e-4


@pytest.mark.parametrize("name", ac.names())
def test_torch_composition_float64_matches_the_golden(aug, name):
    """In float64 the composition is the reference's arithmetic up to summation order: 144 products of O(1) per
    pixel at 2.2e-16 each stay below 1e-12."""
    c = ac.case(name)
    y, gx = ac.run(aug, c, c["x"].double().requires_grad_(True))
    ey, eg = float((y - c["y"]).abs().max()), float((gx - c["gx"]).abs().max())
    print(name, "float64 max abs error: y", ey, "gx", eg)
    assert y.dtype == torch.float64 and ey < 1e-12 and eg < 1e-12


@pytest.mark.parametrize("name", ac.names())
def test_torch_composition_float32_is_within_the_e32_bound(aug, name):
    c = ac.case(name)
    y, gx = ac.run(aug, c, c["x"].clone().requires_grad_(True))
    ey, eg = float((y.double() - c["y"]).abs().max()), float((gx.double() - c["gx"]).abs().max())
    print(name, "float32 error / e32: y", ey / c["e32_y"], "gx", eg / c["e32_gx"])
    assert ey <= ac.E32_MULTIPLE * c["e32_y"] and eg <= ac.E32_MULTIPLE * c["e32_gx"]


@pytest.mark.parametrize("name", ac.names())
def test_get_padding_equals_the_reference(aug, name):
    c = ac.case(name)
    H, W = c["x"].shape[2:]
    pads = aug.get_padding(c["G"], H, W, 12)
    assert tuple(int(v) for v in pads) == c["pads"]
    assert all(v.dtype == torch.int32 and v.dim() == 0 for v in pads)


@pytest.mark.parametrize("p", [0.0, 0.5, 1.0])
def test_sampled_matrices_equal_the_reference_draws(aug, p):
    d = ac.data()
    torch.manual_seed(7)
    G = aug.sample_affine(p, 4, 20, 28)
    torch.manual_seed(7)
    C = aug.sample_color(p, 4)
    assert G.shape == (4, 3, 3) and C.shape == (4, 4, 4)
    assert np.array_equal(G.numpy(), d[f"draw.affine.p{p}"])
    assert np.array_equal(C.numpy(), d[f"draw.color.p{p}"])
    if p == 0.0:
        assert torch.equal(G, torch.eye(3).expand(4, 3, 3)) and torch.equal(C, torch.eye(4).expand(4, 4, 4))


def test_augment_samples_G_then_C_like_the_reference(aug):
    """C = None with p given: the colour matrix is drawn as the reference draws it (stored with the case)."""
    c = ac.case("pad_clamp")
    torch.manual_seed(c["seed"])
    y, (G, C) = aug.augment(c["x"].double(), c["p"], (c["G"], None))
    assert G is c["G"] and torch.equal(C, c["C"])
    assert float((y - c["y"]).abs().max()) < 1e-12
    # both None: the affine draw comes first, then the colour draw
    torch.manual_seed(3)
    _, (G2, C2) = aug.augment(c["x"], 0.7, (None, None))
    torch.manual_seed(3)
    G3 = torch.inverse(aug.sample_affine(0.7, 1, 16, 16))
    C3 = aug.sample_color(0.7, 1)
    assert torch.equal(G2, G3) and torch.equal(C2, C3)


def test_random_apply_color_and_channel_check(aug):
    c = ac.case("rot30")
    y, C = aug.random_apply_color(c["x"], 0.5, c["C"])
    m = c["C"][0]
    want = (m[:3, :3] @ c["x"][0].reshape(3, -1) + m[:3, 3:]).view(3, 16, 16)
    assert C is c["C"] and torch.allclose(y[0], want, atol=1e-6)
    with pytest.raises(ValueError):
        aug.augment(ac.case("gray")["x"], 0.5, (ac.case("gray")["G"], torch.eye(4).unsqueeze(0)))


def test_adaptive_augment_follows_the_recorded_trajectory(aug):
    d = ac.data()
    target, length, every = d["tune.args"]
    ada = aug.AdaptiveAugment(float(target), int(length), int(every), "cpu")
    ps, rs = [], []
    for pred in d["tune.real_pred"]:
        ps.append(ada.tune(torch.from_numpy(pred)))
        rs.append(ada.r_t_stat)
    assert len(ps) == 40 and ps == list(d["tune.p"]) and rs == list(d["tune.r_t_stat"])
    assert max(ps) > 0.3 and ps[-1] < max(ps)            # the trajectory rises and comes back


def test_symbols_are_declared_and_exported(aug):
    from gan2shape_amd import lib
    assert {"g2s_ada_up2", "g2s_ada_up2_bwd", "g2s_ada_warp_down", "g2s_ada_warp_down_bwd"} <= set(lib.SIGNATURES)
    lib.load()


def test_bad_arguments_are_rejected_before_any_launch(aug):
    """Every check precedes the first launch, so it runs without a GPU (the pointers are never followed)."""
    from gan2shape_amd import lib
    L = lib.load()
    host = (ctypes.c_float * 64)()
    ok = ctypes.c_void_p(ctypes.addressof(host))

    def up(fn, a=ok, b=ok, B=2, C=3, H=16, W=12, pads=(3, 4, 5, 6)):
        return getattr(L, fn)(a, b, B, C, H, W, *pads, None)

    def warp(x=ok, g=ok, cm=ok, y=ok, B=2, C=3, H=16, W=12):
        return L.g2s_ada_warp_down(x, g, cm, y, B, C, H, W, 64, 48, None)

    def warp_bwd(gy=ok, g=ok, cm=ok, gx2=ok, B=2, C=3, H=16, W=12):
        return L.g2s_ada_warp_down_bwd(gy, g, cm, gx2, B, C, H, W, 64, 48, 1, None)
    for fn in ("g2s_ada_up2", "g2s_ada_up2_bwd"):
        for kw in ({"a": None}, {"b": None}, {"B": 0}, {"H": 0}, {"pads": (12, 0, 0, 0)}, {"pads": (0, 12, 0, 0)},
                   {"pads": (0, 0, 16, 0)}, {"pads": (0, 0, 0, 16)}, {"pads": (-1, 0, 0, 0)}, {"B": 65536, "C": 1}):
            rc = up(fn, **kw)
            assert rc == -1 and fn.encode() in L.g2s_last_error(), (fn, kw, rc, L.g2s_last_error())
            with pytest.raises(lib.G2SError):
                lib.check(rc)
    for call, fn in ((warp, b"g2s_ada_warp_down"), (warp_bwd, b"g2s_ada_warp_down_bwd")):
        first = "x" if call is warp else "gy"
        last = "y" if call is warp else "gx2"
        for kw in ({first: None}, {"g": None}, {last: None}, {"C": 1}, {"C": 4}, {"B": 0}, {"W": -2}):
            rc = call(**kw)
            assert rc == -1 and fn in L.g2s_last_error(), (fn, kw, rc, L.g2s_last_error())
    assert b"C == 3" in (warp(C=4), L.g2s_last_error())[1]
