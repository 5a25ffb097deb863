"""-m gpu: g2s_modconv_f16 on every body, tile and split-K form, and the scale, noise, promise and thin-dispatch paths of
g2s_modconv, against float64, element by element.

The tables, the plans, the reference and the bound are those of tests/modconv_cases.py.  Every launch goes through the C
entry points, so that a case sets every argument, under tuned(tile, sk, det), which restores g2s_modconv_tune(-1, -1) and
the deterministic flag.  The output is the interior of a guarded buffer, pre-filled with a sentinel where the plan says the
launch overwrites and with NaN where the launcher has to clear it itself.  Every test prints its largest
error / (e32 max|ref|) and error / cap."""
import numpy as np
import pytest
import torch

import conv2d_cases as cc
import modconv_cases as mc
from test_gpu_conv2d_paths import SENTINEL, dev, guarded, guards_intact, tuned

pytestmark = pytest.mark.gpu

NAN = float("nan")


@pytest.fixture(scope="module")
def g2s():
    import gan2shape_amd  # noqa: F401
    from gan2shape_amd import lib
    return lib.load()  # fails loudly if libg2s.so is missing


def _device_operands(c, dt):
    return dict(x=dev(dt["x"]), w=dev(dt["w"]), s=dev(dt["s"]), os=dev(dt["os"]),
                bias=dev(dt["bias"]) if c.ep is not None and c.ep[0] else None,
                noise=dev(dt["noise"]) if c.noise else None, noise_w=dev(dt["noise_w"]) if c.noise else None)


def call(L, c, d, y, y_is_zero=0):
    """The C entry point of the case's route; returns its code."""
    from gan2shape_amd import lib
    _, act, alpha, gain = c.ep if c.ep is not None else (False, False, 0.0, 1.0)
    if c.route == "f16":
        return L.g2s_modconv_f16(lib.ptr(d["x"]), lib.ptr(d["w"]), lib.ptr(d["s"]), lib.ptr(d["os"]), lib.ptr(d["bias"]),
                                 lib.ptr(y), c.B, c.Cin, c.Cout, c.H, c.W, c.k, c.mode, c.tr, int(act), float(alpha),
                                 float(gain), lib.stream())
    return L.g2s_modconv(lib.ptr(d["x"]), lib.ptr(d["w"]), lib.ptr(d["s"]), lib.ptr(d["os"]), lib.ptr(d["bias"]),
                         lib.ptr(d["noise"]), lib.ptr(d["noise_w"]), lib.ptr(y), c.B, c.Cin, c.Cout, c.H, c.W, c.k, c.mode,
                         c.tr, int(act), float(alpha), float(gain), int(y_is_zero), lib.stream())


def run(L, c, d, pl, tile=None, sk=None, det=None, fill=None, y_is_zero=0):
    """One launch into a guarded output: sentinel-filled where the plan overwrites, NaN-filled where the launcher clears."""
    from gan2shape_amd import lib
    if fill is None:
        fill = NAN if pl["needs_zero"] else SENTINEL
    buf, y = guarded((c.B, c.M) + c.out_hw, fill)
    with tuned(L, c.tile if tile is None else tile, c.sk if sk is None else sk, c.det if det is None else det):
        lib.check(call(L, c, d, y, y_is_zero))
    out = y.cpu().numpy()
    assert guards_intact(buf), (c.name, "guard elements overwritten")
    return out


def path_of(c, pl):
    if pl["thin"]:
        return "f32/thin"
    body = "+".join(sorted(set(pl["bodies"]))) if c.route == "f16" else "f32/" + "+".join(sorted({f"T{cl['T']}" for cl in pl["classes"]}))
    return (f"{body}/tile{pl['pick']}/{'split' if pl['splitk'] > 1 else 'det' if pl['split_source'] == 'det' else 'plain'}"
            f"{'/deferred' if pl['deferred'] else ''}")


def check(c, pl, what, got, dt):
    ref, cap, e32 = dt["ref"], dt["cap"], dt["e32"]
    assert got.shape == ref.shape, (c.name, what, got.shape, ref.shape)
    assert np.isfinite(got).all(), (c.name, what, "not finite", int((~np.isfinite(got)).sum()))
    ratio = mc.ratio_of(pl)
    err = np.abs(got.astype(np.float64) - ref)
    bound = cc.bound(ref, e32, cap, ratio)
    r_e32 = err.max() / np.abs(ref).max() / cc.floor_e32(e32)
    r_cap = float(np.where(err > 0, err / np.maximum(cap, 1e-300), 0.0).max())
    print(f"RATIO {path_of(c, pl)} {c.name} {what}: error / (e32 max|ref|) {r_e32:.2f} of {ratio:g} (e32 {e32:.3e}), "
          f"error / cap {r_cap:.3f}")
    over = err > bound
    assert not over.any(), (f"{c.name} {what} [{path_of(c, pl)}]: {int(over.sum())} of {err.size} elements over the bound, first at "
                            f"{np.unravel_index(np.argmax(err - bound), err.shape)}, {r_e32:.2f} x e32, {r_cap:.3f} x cap")


# ------------------------------------------------------------------------------------------------ g2s_modconv_f16
@pytest.mark.parametrize("name", [c.name for c in mc.F16])
def test_f16_vs_float64(g2s, name):
    c = mc.BY_NAME[name]
    dt = mc.data(name)
    d = _device_operands(c, dt)
    pl = c.plan()
    y = run(g2s, c, d, pl)
    check(c, pl, "y", y, dt)
    if c.det:       # the deterministic flag: no float atomics, two runs are bit-equal
        assert np.array_equal(y, run(g2s, c, d, pl)), name


@pytest.mark.parametrize("name", list(mc.SWEEP))
def test_f16_forced_tiles_and_splits_vs_float64(g2s, name):
    """Tiles 0, 1, 2 under split-K 1, 2, 3 and one count above the kernel's own K tiles, on one case per body."""
    c, _ = mc.SWEEP[name]
    dt = mc.data(name)
    d = _device_operands(c, dt)
    for tile in mc.SWEEP_TILES:
        for sk in mc.sweep_splits(c):
            pl = c.plan(tile=tile, sk=sk)
            check(c, pl, f"y tune({tile},{sk})", run(g2s, c, d, pl, tile=tile, sk=sk), dt)


def test_f16_refuses_tiles_3_and_4_and_the_next_call_is_right(g2s):
    c = mc.BY_NAME["q_fwd"]
    dt = mc.data(c.name)
    d = _device_operands(c, dt)
    for tile in (3, 4):
        with pytest.raises(mc.Rejected):
            c.plan(tile=tile)
        buf, y = guarded((c.B, c.M) + c.out_hw, NAN)
        with tuned(g2s, tile, -1):
            rc = call(g2s, c, d, y)
        assert rc != 0 and b"tiles 0..2" in g2s.g2s_last_error(), (tile, rc)
        torch.cuda.synchronize()
        assert bool(torch.isnan(y).all()) and guards_intact(buf), tile
        check(c, c.plan(), f"y after tile {tile} was refused", run(g2s, c, d, c.plan()), dt)


# ---------------------------------------------------------------------------------------------------- g2s_modconv
@pytest.mark.parametrize("name", [c.name for c in mc.F32])
def test_f32_vs_float64(g2s, name):
    c = mc.BY_NAME[name]
    dt = mc.data(name)
    d = _device_operands(c, dt)
    pl = c.plan()
    y = run(g2s, c, d, pl)
    check(c, pl, "y", y, dt)
    if c.det:
        assert np.array_equal(y, run(g2s, c, d, pl)), name


@pytest.mark.parametrize("name", [c.name for c in mc.F32 if c.promise])
def test_f32_y_is_zero_promise_in_both_directions(g2s, name):
    """Where g2s_modconv_needs_zero says 0 the promise is not looked at: y_is_zero = 1 on a NaN-filled output is still
    right.  Where it says 1, a zeroed output with y_is_zero = 1 and a NaN-filled one with y_is_zero = 0 agree."""
    c = mc.BY_NAME[name]
    dt = mc.data(name)
    d = _device_operands(c, dt)
    pl = c.plan()
    with tuned(g2s, c.tile, c.sk, c.det):
        needs = g2s.g2s_modconv_needs_zero(c.B, c.Cin, c.Cout, c.H, c.W, c.k, c.mode, c.tr, int(c.scale or c.oscale),
                                           int(c.fused))
    assert needs == int(pl["needs_zero"]), (name, needs)
    if not needs:
        check(c, pl, "y y_is_zero=1 on NaN", run(g2s, c, d, pl, fill=NAN, y_is_zero=1), dt)
        return
    kept = run(g2s, c, d, pl, fill=0.0, y_is_zero=1)
    cleared = run(g2s, c, d, pl, fill=NAN, y_is_zero=0)
    check(c, pl, "y y_is_zero=1 on zeros", kept, dt)
    check(c, pl, "y y_is_zero=0 on NaN", cleared, dt)
    bound = cc.bound(dt["ref"], dt["e32"], dt["cap"], mc.ratio_of(pl))
    assert (np.abs(kept.astype(np.float64) - cleared) <= bound).all(), name


THIN_ROWS = [c.name for c in mc.F32 if c.name.startswith("thin_")]


@pytest.mark.parametrize("name", THIN_ROWS)
def test_f32_thin_dispatch_boundary(g2s, name):
    """Which kernel a call takes, seen from outside: the streaming 1x1 kernel refuses an output that is not 16-byte
    aligned (before any launch), the MFMA kernel has no such requirement.  The eligible call is refused on an output
    shifted by one float; the calls one step outside the rule, and the eligible shape with a noise, run there and are right."""
    from gan2shape_amd import lib
    c = mc.BY_NAME[name]
    dt = mc.data(name)
    d = _device_operands(c, dt)
    pl = c.plan()
    n = int(np.prod(dt["ref"].shape))
    buf, _ = guarded((n + 4,), SENTINEL)
    y = buf[257:257 + n].view(dt["ref"].shape)
    assert y.data_ptr() % 16 == 4
    with tuned(g2s, c.tile, c.sk, c.det):
        rc = call(g2s, c, d, y)
    torch.cuda.synchronize()
    if pl["thin"]:
        assert rc != 0 and b"aligned" in g2s.g2s_last_error(), (name, rc)
        assert bool((buf == SENTINEL).all()), name
        # and a forced tile keeps the same call on the MFMA kernel
        plf = c.plan(tile=2, sk=1)
        assert not plf["thin"]
        with tuned(g2s, 2, 1):
            lib.check(call(g2s, c, d, y))
        check(c, plf, "y unaligned, tile 2 forced", y.cpu().numpy(), dt)
    else:
        lib.check(rc)
        check(c, pl, "y unaligned", y.cpu().numpy(), dt)
    assert bool((buf[:257] == SENTINEL).all()) and bool((buf[257 + n:] == SENTINEL).all()), name
