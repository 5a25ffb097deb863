"""-m gpu: every forward and backward variant of the depth rasterizer (csrc/raster.hip,
csrc/raster_scatter.h) against the oracle, on the case table of tests/raster_cases.py.

Forward: both tile-to-wave mappings (g2s_raster_tune 1 and 4: one tile per wave, four waves per tile),
depth / face_idx / bary bit for bit against the fp32 oracle.  Backward: g2s_raster_depth_bwd_ex on the
oracle's maps, float atomics (default) and 64-bit fixed point (deterministic), against the float64 oracle.
tests/test_raster_core_cpu.py::test_case_table_reaches_its_paths shows on the oracle alone that the cases
hold what they are there for: reversed winners, partial tiles, and in the confetti cases 192 distinct
vertices in one 8x8 tile — more than the 128 slots of the backward's LDS table, so part of the tile's sums
goes straight to global memory.

The bound.  The kernels do the fp32 oracle's arithmetic (raster_core.h) in another summation order, so they
are measured against the fp32 oracle's own distance from float64: with e32 = max|oracle_f32 - oracle_f64|
and scale = max|oracle_f64|, max|kernel - oracle_f64| <= 4 e32 + 5e-6 scale (raster_cases.Case.data).

Measured on an MI355X, max|kernel - oracle_f64| / e32 (worst topology of the case):

    case                     e32 / scale   float atomics   fixed point
    grid                     8.5e-05       1.001           1.000
    ss1                      3.6e-06       1.000           1.000
    nofill                   1.4e-05       1.000           1.000
    ragged1                  4.6e-06       1.007           1.007
    ragged2                  5.2e-06       1.006           1.006
    soup                     1.7e-06       0.964           0.964
    soup_nofill              1.8e-06       1.000           1.000
    confetti                 1.7e-06       1.000           1.000
    confetti_nofill          1.1e-06       1.000           1.000
    confetti_noflip_nofill   2.2e-06       1.000           1.000
    confetti17               1.9e-06       1.000           1.000

The ratio sits at 1: in every case the largest deviation from float64 is one vertex whose fp32 value the
kernels reproduce (the per-sample terms are the fp32 oracle's, bit for bit); the re-association moves the
last bits only.  A lost, doubled or misdirected contribution is of the order of `scale`, 1e3 to 1e6 times
e32.  `-s` prints the figures of a run.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from raster_cases import BACKGROUND, CASE, CASES, FAR  # noqa: E402


@pytest.fixture(scope="module")
def g2s():
    import gan2shape_amd  # noqa: F401
    from gan2shape_amd import lib
    lib.load()  # fails loudly if libg2s.so is missing
    assert torch.cuda.is_available()
    return gan2shape_amd


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.array(a), dtype=dtype).cuda()   # a copy: the shared reference arrays are read-only


def _K(lib, K):
    return (lib.C.c_float * 9)(*np.asarray(K, np.float32).reshape(9).tolist())


def forward(case, implicit, waves):
    """g2s_raster_depth_fwd with saved maps under g2s_raster_tune(waves).  The outputs start as
    sentinels, so a tile no wave wrote cannot pass for one an earlier launch left in the same memory."""
    from gan2shape_amd import lib
    L = lib.load()
    d = case.data()
    B, N, _ = d["verts"].shape
    S, isz, F = case.S, case.S * case.ssaa, d["faces"].shape[0]
    v = dev(d["verts"])
    f = None if implicit else dev(d["faces"], torch.int32)
    depth = torch.full((B, S, S), float("nan"), device="cuda")
    fidx = torch.full((B, isz, isz), -7, dtype=torch.int32, device="cuda")
    bary = torch.full((B, isz, isz, 3), float("nan"), device="cuda")
    ws = torch.empty(L.g2s_raster_workspace_bytes(B, N, F, S), dtype=torch.uint8, device="cuda")
    lib.check(L.g2s_raster_tune(waves))
    try:
        assert L.g2s_raster_get_tune() == waves
        lib.check(L.g2s_raster_depth_fwd(lib.ptr(v), lib.ptr(f), B, N, F, S, _K(lib, d["K"]), float(S), case.ssaa,
                                         int(case.fill_back), 0.1, FAR, lib.ptr(depth), lib.ptr(fidx),
                                         lib.ptr(bary), lib.ptr(ws), ws.numel(), lib.stream()))
        torch.cuda.synchronize()
    finally:
        lib.check(L.g2s_raster_tune(0))
    return depth.cpu().numpy(), fidx.cpu().numpy(), bary.cpu().numpy()


def backward(case, implicit, deterministic, acc_is_zero=0, g=None):
    """g2s_raster_depth_bwd_ex on the oracle's face_idx / bary (the kernel's own are the same:
    test_forward_both_variants_bit_exact).  With acc_is_zero = 0 the scatter target starts as garbage,
    which the call must clear; with 1 the caller has cleared it."""
    from gan2shape_amd import lib
    L = lib.load()
    d = case.data()
    B, N, _ = d["verts"].shape
    v = dev(d["verts"])
    f = None if implicit else dev(d["faces"], torch.int32)
    gd = dev(d["g"] if g is None else g)
    fidx, bary = dev(d["fw"]["face_idx"], torch.int32), dev(d["fw"]["bary"])
    prev = lib.set_deterministic(deterministic)
    try:
        ws, ws_bytes = None, 0
        gv = torch.full_like(v, 123.0)
        if deterministic:
            ws_bytes = L.g2s_raster_bwd_workspace_bytes(B, N)
            ws = torch.full((ws_bytes,), 0 if acc_is_zero else 0x5a, dtype=torch.uint8, device="cuda")
        elif acc_is_zero:
            gv.zero_()
        lib.check(L.g2s_raster_depth_bwd_ex(lib.ptr(v), lib.ptr(f), lib.ptr(gd), lib.ptr(fidx), lib.ptr(bary),
                                            B, N, d["faces"].shape[0], case.S, _K(lib, d["K"]), float(case.S),
                                            case.ssaa, lib.ptr(gv), lib.ptr(ws), ws_bytes, acc_is_zero,
                                            lib.stream()))
        torch.cuda.synchronize()
    finally:
        lib.set_deterministic(prev)
    return gv


def check_gradient(case, gv, what):
    d = case.data()
    err = float(np.abs(gv.cpu().numpy().astype(np.float64) - d["ref64"]).max())
    print(f"{case.name:16s} {what:24s} err {err:.3e}  err/e32 {err / d['e32'] if d['e32'] else 0:.3f}  "
          f"e32/scale {d['e32'] / d['scale'] if d['scale'] else 0:.2e}  bound {d['bound']:.3e}")
    assert np.isfinite(err) and err <= d["bound"], (case, what, err, d["e32"], d["bound"])


# ----------------------------------------------------------------------------- forward
@pytest.mark.parametrize("case", CASES, ids=repr)
def test_forward_both_variants_bit_exact(g2s, case):
    fw = case.data()["fw"]
    for implicit in case.topologies:
        outs = {w: forward(case, implicit, w) for w in (1, 4)}
        for w, (depth, fidx, bary) in outs.items():
            np.testing.assert_array_equal(fidx, fw["face_idx"], err_msg=f"waves {w} implicit {implicit}")
            np.testing.assert_array_equal(bary, fw["bary"], err_msg=f"waves {w} implicit {implicit}")
            np.testing.assert_array_equal(depth, fw["depth"], err_msg=f"waves {w} implicit {implicit}")
        for a, b in zip(outs[1], outs[4]):
            np.testing.assert_array_equal(a, b)


def test_raster_tune_refuses_other_values(g2s):
    from gan2shape_amd import lib
    L = lib.load()
    assert L.g2s_raster_get_tune() == 0
    lib.check(L.g2s_raster_tune(1))
    try:
        for bad in (2, 3, -1, 8):
            assert L.g2s_raster_tune(bad) != 0
            assert b"waves_per_tile must be 0" in L.g2s_last_error()
            assert L.g2s_raster_get_tune() == 1      # the previous setting still holds
    finally:
        lib.check(L.g2s_raster_tune(0))
    assert L.g2s_raster_get_tune() == 0


# ----------------------------------------------------------------------------- backward
@pytest.mark.parametrize("case", CASES, ids=repr)
def test_backward_against_float64(g2s, case):
    for implicit in case.topologies:
        topo = "implicit" if implicit else "explicit"
        check_gradient(case, backward(case, implicit, False), "float " + topo)
        runs = [backward(case, implicit, True) for _ in range(2)]
        check_gradient(case, runs[0], "deterministic " + topo)
        assert torch.equal(runs[0], runs[1]), (case, topo)


@pytest.mark.parametrize("name", ["confetti", "ragged2"])
def test_backward_on_a_caller_cleared_target(g2s, name):
    """acc_is_zero = 1 (the caller cleared the scatter target) against acc_is_zero = 0 (the call clears
    it): bit-equal in fixed point, both within the bound with float atomics.  confetti: the sums that
    bypass the LDS table land in the same target."""
    case = CASE[name]
    for implicit in case.topologies:
        assert torch.equal(backward(case, implicit, True, 1), backward(case, implicit, True, 0))
        check_gradient(case, backward(case, implicit, False, 1), "float, caller-cleared")
        check_gradient(case, backward(case, implicit, False, 0), "float, call clears")


@pytest.mark.parametrize("name", ["ss1", "nofill", "confetti"])
def test_autograd_wrapper_passes_ssaa_and_fill_back(g2s, name):
    from gan2shape_amd.plugins import neural_renderer as nr
    case = CASE[name]
    d = case.data()
    K = tuple(np.asarray(d["K"], np.float32).reshape(9).tolist())
    for implicit in case.topologies:
        v = dev(d["verts"]).requires_grad_(True)
        f = None if implicit else dev(d["faces"], torch.int32)
        depth = nr.RenderDepthFunction.apply(v, f, K, float(case.S), case.S, case.ssaa == 2, case.fill_back,
                                             0.1, FAR)
        (gv,) = torch.autograd.grad(depth, v, dev(d["g"]))
        np.testing.assert_array_equal(depth.detach().cpu().numpy(), d["fw"]["depth"])
        check_gradient(case, gv, "autograd " + ("implicit" if implicit else "explicit"))


def test_all_background_image(g2s):
    """Every vertex behind `far`: the faces are binned and their fragments evaluated, none is drawn.
    depth = far everywhere, face_idx = -1, and a non-zero upstream gradient gives exactly zero."""
    case = BACKGROUND
    isz = case.S * case.ssaa
    assert np.abs(case.data()["g"]).min() > 0
    for implicit in case.topologies:
        for w in (1, 4):
            depth, fidx, bary = forward(case, implicit, w)
            np.testing.assert_array_equal(depth, np.full((2, case.S, case.S), FAR, np.float32))
            np.testing.assert_array_equal(fidx, np.full((2, isz, isz), -1, np.int32))
            np.testing.assert_array_equal(bary, np.zeros((2, isz, isz, 3), np.float32))
        for deterministic in (False, True):
            assert int(torch.count_nonzero(backward(case, implicit, deterministic))) == 0
