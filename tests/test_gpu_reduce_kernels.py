"""-m gpu: csrc/geometry.hip, csrc/lpips.hip and csrc/losses.hip through the C ABI against the float64
restatement of tests/reduce_cases.py, in the default launch geometry and under g2s_set_deterministic(1)
(one workgroup strides over everything: nine of these kernels change their loops there).

Per case and mode: outputs start as NaN sentinels and the gRt / glight / loss / gsum accumulators as garbage
with acc_is_zero = 0 (the `num` / `numden` / `out` accumulators of weighted_l1_fwd* and lpips_layer_fwd as
zeros, their contract); exact-grid outputs (`Case.exact`) must EQUAL float64, every other output obeys
max|kernel - f64| <= 4 e32 + 5e-6 max|f64| (e32: the sequential-fp32 restatement's own distance from float64,
reduce_cases.Case.data); in deterministic mode a second run must repeat the first bit for bit.
tests/test_reduce_cases_cpu.py shows on the restatement alone that it reproduces the reference's fixtures and
that every case reaches what it is there for.

Measured on an MI355X: RATIO_TABLE below, appended to this docstring (`-s` prints the figures of a run, per case).
"""
import ctypes
from contextlib import contextmanager

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import reduce_cases as rc  # noqa: E402

RATIO_TABLE = """
Per operation, over its cases and outputs: the worst e32 / scale, the worst max|kernel - f64| / e32 in each mode,
and the worst max|kernel - f64| / scale.  Then every case whose ratio exceeds 1.5.

    operation (cases)            worst e32 / scale   worst ratio: default   deterministic   worst error / scale
    view_transform (3)           1.2e-07             1.823                  1.823           1.6e-07
    warp_verts (8)               1.3e-07             1.001                  1.001           1.3e-07
    inv_warp_grid (8)            3.1e-07             1.556                  1.556           3.1e-07
    normal (14)                  1.4e-06             2.006                  2.006           1.4e-06
    smooth_loss, random (16)     1.2e-07             31.222                 7.000           1.2e-07
    smooth_loss, dyadic (3)      7.4e-08             3.025                  2.500           1.2e-07
    smooth_loss, exact (6)       0.0e+00             0.000                  0.000           0.0e+00   (bounded outputs only; the rest is ==)
    shading (8)                  1.2e-07             1.477                  1.477           1.6e-07
    depth_head (7)               1.0e-06             1.215                  1.215           1.2e-06
    lpips_layer (10)             1.8e-07             2.533                  2.533           1.9e-07
    weighted_l1, exact (12)      0.0e+00             0.000                  0.000           0.0e+00   (bounded outputs only; the rest is ==)
    weighted_l1, random (8)      6.7e-08             15.000                 15.000          9.4e-08

    cases with a ratio above 1.5    e32 / scale   default   deterministic   output
    view_B64                        8.6e-08       1.823     1.823           gview
    invwarp_3x85_B1                 1.9e-07       1.556     1.556           gdepth
    smooth_3x3_N1                   2.8e-08       1.750     1.750           gp
    smooth_40x2_N1                  4.3e-08       1.763     1.763           gp
    normal_3x3_B3                   8.3e-08       2.006     2.006           gdepth
    smooth_3x3_N3                   3.5e-08       1.000     1.866           loss
    smooth_9x33_N3                  1.9e-09       31.222    1.114           loss
    smooth_2x2_N3                   1.3e-08       7.000     7.000           loss
    smooth_40x2_N3                  3.7e-08       2.995     3.305           loss
    smoothgrid_3x3_N1               4.5e-08       2.500     2.500           loss
    smoothgrid_9x33_N3              3.6e-08       3.025     1.600           loss
    lpips_1x5x1_f1                  5.5e-08       2.423     2.423           g_plain
    lpips_1x64x1088                 4.3e-08       2.533     2.533           g_plain@z0
    l1rand_1x1x4_none               5.5e-09       15.000    15.000          num
    l1rand_3x2x1028_none            7.9e-09       1.876     1.876           g3gate_x1a0

Every ratio above 1 belongs to an output whose e32 is itself within three ulp of `scale` (e32 / scale <= 2e-7):
there the sequential fp32 restatement happens to land on or next to the float64 value, and the kernel, which
writes the same expression in another association, lands an ulp or two away — the second difference as
p2 - 2 p1 + p0 and its weight inside the sum (smooth_loss), x * (1 / (norm + eps)) for x / (norm + eps)
(lpips_layer), u * (2 / (W - 1)) - 1 for u / (W - 1) * 2 - 1 (inv_warp_grid), one float4 tree for four terms
(weighted_l1: l1rand_1x1x4 is a sum of four numbers, off by one ulp).  No kernel error exceeds 1.4e-6 of scale
(normal_17x70_B3, ratio 1.0); the floor of the bound, 5e-6 scale, covers all of them, and a lost, doubled or
misdirected contribution is 1e-4 of scale or more at these shapes.  Deterministic mode changes the figures only
where it changes the summation order (smooth_loss, the reductions of the others stay within the same ulp).
"""

__doc__ += RATIO_TABLE

NAN = float("nan")


@pytest.fixture(scope="module")
def g2s():
    import gan2shape_amd  # noqa: F401
    from gan2shape_amd import lib
    lib.load()  # fails loudly if libg2s.so is missing
    assert torch.cuda.is_available()
    return lib


@contextmanager
def mode(lib, deterministic):
    prev = lib.set_deterministic(deterministic)
    try:
        yield
    finally:
        lib.set_deterministic(prev)


def dev(a):
    return torch.as_tensor(np.array(a)).cuda()   # a copy: the shared arrays are read-only


def nans(*shape):
    return torch.full(shape, NAN, device="cuda")


def garbage(*shape):
    return torch.full(shape, 123.0, device="cuda")


def zeros(*shape):
    return torch.zeros(shape, device="cuda")


class Call:
    """lib + loaded library + the two shorthands every launch uses."""

    def __init__(self, lib):
        self.lib, self.L, self.p = lib, lib.load(), lib.ptr

    def __call__(self, name, *args):
        self.lib.check(getattr(self.L, name)(*args, self.lib.stream()))


# ----------------------------------------------------------------------------- one runner per operation
def run_view(c, case, i):
    B = case.p["B"]
    view, R, t, gview = dev(i["view"]), nans(B, 3, 3), nans(B, 3), nans(B, 6)
    gR, gt = dev(i["gR"]), dev(i["gt"])
    c("g2s_view_transform_fwd", c.p(view), *rc.VIEW_SCALES, c.p(R), c.p(t), B)
    c("g2s_view_transform_bwd", c.p(view), *rc.VIEW_SCALES, c.p(gR), c.p(gt), c.p(gview), B)
    return dict(R=R, t=t, gview=gview)


def run_warp(c, case, i):
    B, H, W, inv = case.p["B"], case.p["H"], case.p["W"], case.p.get("inv")
    P = H * W
    depth, rays, R, t, cot = (dev(i[k]) for k in ("depth", "rays", "R", "t", "cot"))
    K = (ctypes.c_float * 9)(*[float(k) for k in i["K9"]])
    out = nans(B, P, 2 if inv else 3)

    def bwd(gdepth, gRt):
        if inv:
            c("g2s_inv_warp_grid_bwd", c.p(depth), c.p(rays), c.p(R), c.p(t), K, rc.RCD, c.p(cot), c.p(gdepth), c.p(gRt), B, H, W, 0)
        else:
            c("g2s_warp_verts_bwd", c.p(depth), c.p(rays), c.p(R), c.p(cot), rc.RCD, c.p(gdepth), c.p(gRt), B, P, 0)
    if inv:
        c("g2s_inv_warp_grid_fwd", c.p(depth), c.p(rays), c.p(R), c.p(t), K, rc.RCD, c.p(out), B, H, W)
    else:
        c("g2s_warp_verts_fwd", c.p(depth), c.p(rays), c.p(R), c.p(t), rc.RCD, c.p(out), B, P)
    gdepth, gRt = nans(B, P), garbage(B, 12)
    bwd(gdepth, gRt)
    # gRt == NULL: the same gdepth, and the memory right behind it — where a gRt would lie — keeps its pattern
    buf = torch.cat([nans(B * P), garbage(B * 12)])
    bwd(buf[:B * P], None)
    assert torch.equal(buf[:B * P].view(B, P), gdepth), "gdepth differs when gRt is NULL"
    assert bool((buf[B * P:] == 123.0).all()), "guard behind gdepth was written"
    return dict(out=out, gdepth=gdepth, gRt=gRt)


def run_normal(c, case, i):
    B, H, W = case.p["B"], case.p["H"], case.p["W"]
    depth, rays, cot = dev(i["depth"]), dev(i["rays"]), dev(i["cot"])
    normal, gdepth = nans(B, H, W, 3), nans(B, H, W)
    c("g2s_normal_fwd", c.p(depth), c.p(rays), c.p(normal), B, H, W)
    c("g2s_normal_bwd", c.p(depth), c.p(rays), c.p(cot), c.p(gdepth), B, H, W)
    return dict(normal=normal, gdepth=gdepth)


def run_shading(c, case, i):
    B, Bn, Ba, P = case.p["B"], case.p["Bn"], case.p["Ba"], case.p["H"] * case.p["W"]
    normal, light, albedo, gt, gd = (dev(i[k]) for k in ("normal", "light", "albedo", "gt", "gd"))
    diffuse, texture = nans(B, P), nans(B, 3, P)
    c("g2s_shading_fwd", c.p(normal), c.p(light), c.p(albedo), c.p(diffuse), c.p(texture), B, Bn, Ba, P)
    out = dict(diffuse=diffuse, texture=texture)
    for tag, g in (("", gd), ("_nogd", None)):
        gn, ga, gl = nans(B, P, 3), nans(B, 3, P), garbage(B, 4)
        c("g2s_shading_bwd", c.p(normal), c.p(light), c.p(albedo), c.p(g), c.p(gt), c.p(gn), c.p(ga), c.p(gl), B, Bn, Ba, P, 0)
        out.update({"gnormal" + tag: gn, "glight" + tag: gl, "galbedo#" + (tag or "gd"): ga})
    return out


def run_smooth(c, case, i):
    N, H, W = case.p["N"], case.p["H"], case.p["W"]
    p, loss, gp, gloss = dev(i["p"]), garbage(1), nans(N, H, W), dev(i["gloss"]).reshape(1)
    c("g2s_smooth_loss_fwd", c.p(p), c.p(loss), N, H, W, 0)
    c("g2s_smooth_loss_bwd", c.p(p), c.p(gloss), c.p(gp), N, H, W)
    return dict(loss=loss.reshape(()), gp=gp)


def run_depth_head(c, case, i, d):
    B, H, W = case.p["B"], case.p["H"], case.p["W"]
    n, h = B * H * W, rc.HEAD
    raw, cot = dev(i["raw"]), dev(i["cot"])
    mean = torch.tensor([float(d["diag"]["_mean"])], dtype=torch.float32, device="cuda")   # the caller's reduction
    out, g_raw, gsum = nans(B, H, W), nans(B, H, W), garbage(1)
    tail = (n, W, h["lo"], h["hi"], case.p["border"], h["bd"])
    c("g2s_depth_head_fwd", c.p(raw), c.p(mean), c.p(out), *tail)
    c("g2s_depth_head_bwd", c.p(raw), c.p(mean), c.p(cot), c.p(g_raw), c.p(gsum), *tail, 0)
    return dict(out=out, g_raw=g_raw, gsum=gsum.reshape(()))


def run_lpips(c, case, i):
    N, C, HW = case.p["N"], case.p["C"], case.p["HW"]
    f0, f1, w, gout, g_in = (dev(i[k]) for k in ("f0", "f1", "w", "gout", "g_in"))
    out = zeros(N)
    c("g2s_lpips_layer_fwd", c.p(f0), c.p(f1), c.p(w), c.p(out), N, C, HW)
    res = dict(out=out)
    for name, gi, gate in (("g_plain", None, 0), ("g_gate", None, 1), ("g_in", g_in, 0), ("g_in_gate", g_in, 1)):
        g0 = nans(N, C, HW)
        c("g2s_lpips_layer_bwd_ex", c.p(f0), c.p(f1), c.p(w), c.p(gout), c.p(gi), gate, c.p(g0), N, C, HW)
        res[name] = g0
    g0 = nans(N, C, HW)
    c("g2s_lpips_layer_bwd", c.p(f0), c.p(f1), c.p(w), c.p(gout), c.p(g0), N, C, HW)
    assert torch.equal(g0, res["g_plain"]), "g2s_lpips_layer_bwd != g2s_lpips_layer_bwd_ex(NULL, 0)"
    return res


def run_l1(c, case, i):
    B, C, HW = case.p["B"], case.p["C"], case.p["HW"]
    x, y, gadd, gadd2, gate_ref = (dev(i[k]) for k in ("x", "y", "gadd", "gadd2", "gate_ref"))
    w = dev(i["w"]) if "w" in i else None
    coef, g, den = (dev(i[k]).reshape(1) for k in ("coef", "g", "den"))
    add_scale, slope, gain = (float(i[k]) for k in ("add_scale", "slope", "gain"))
    sz = (B, C, HW)
    num, numden = zeros(1), zeros(2)
    c("g2s_weighted_l1_fwd", c.p(x), c.p(y), c.p(w), c.p(num), *sz)
    c("g2s_weighted_l1_fwd2", c.p(x), c.p(y), c.p(w), c.p(numden), *sz)
    res = {"num": num.reshape(()), "num#fwd2": numden[0], "den2": numden[1]}
    res["g_bwd"], res["g_bwd2"], res["g_bwd2_add"] = nans(*sz), nans(*sz), nans(*sz)
    c("g2s_weighted_l1_bwd", c.p(x), c.p(y), c.p(w), c.p(coef), c.p(res["g_bwd"]), *sz)
    c("g2s_weighted_l1_bwd2", c.p(x), c.p(y), c.p(w), c.p(g), c.p(den), None, c.p(res["g_bwd2"]), *sz)
    c("g2s_weighted_l1_bwd2", c.p(x), c.p(y), c.p(w), c.p(g), c.p(den), c.p(gadd), c.p(res["g_bwd2_add"]), *sz)
    for xo, na in rc.L1_COMBOS:      # every legal combination: x given or not, 0 / 1 / 2 joined gradients, gx / gx_gate / both
        for outs in ("gx", "gate", "both"):
            gx = nans(*sz) if outs != "gate" else None
            gq = nans(*sz) if outs != "gx" else None
            c("g2s_weighted_l1_bwd3", c.p(x if xo else None), c.p(y if xo else None), c.p(w if xo else None),
              c.p(g if xo else None), c.p(den if xo else None), c.p(gadd if na else None), c.p(gadd2 if na == 2 else None),
              add_scale, c.p(gx), c.p(gate_ref if gq is not None else None), slope, gain, c.p(gq), *sz)
            if gx is not None:
                res[f"g3_x{xo}a{na}#{outs}"] = gx
            if gq is not None:
                res[f"g3gate_x{xo}a{na}#{outs}"] = gq
    return res


RUN = dict(view=run_view, warp=run_warp, normal=run_normal, shading=run_shading, smooth=run_smooth, lpips=run_lpips, l1=run_l1)


def run(c, case):
    d = case.data()
    if case.op == "depth_head":
        return run_depth_head(c, case, d["inp"], d)
    return RUN[case.op](c, case, d["inp"])


def compare(case, got, tag, factor=1.0):
    """Every output against float64: `==` for the exact-grid ones, the bound for the rest; nothing NaN left.
    Prints the case's worst e32 / scale and worst max|kernel - f64| / e32."""
    d = case.data()
    got = case.split(d["inp"], got)
    worst = (0.0, 0.0, "-")
    for name, val in got.items():
        key = name.split("#")[0]
        ref, st = d["ref64"][key], d["stats"][key]
        v = val.detach().cpu().double().numpy().reshape(ref.shape)
        assert not np.isnan(v).any(), f"{case.name} {tag} {name}: a sentinel survived"
        if key in case.exact:
            assert np.array_equal(v, ref), f"{case.name} {tag} {name}: not equal to float64 on exact-grid inputs (max diff {np.abs(v - ref).max():.3e})"
            continue
        err = float(np.abs(v - ref).max()) if ref.size else 0.0
        if st["e32"] > 0 and err / st["e32"] > worst[1]:
            worst = (st["e32"] / max(st["scale"], 1e-300), err / st["e32"], name)
        assert err <= factor * st["bound"], (f"{case.name} {tag} {name}: max|kernel - f64| {err:.3e} > bound {factor * st['bound']:.3e} "
                                              f"(e32 {st['e32']:.3e}, scale {st['scale']:.3e})")
    print(f"[reduce] {case.name:28s} {tag:13s} e32/scale {worst[0]:.1e}  ratio {worst[1]:6.3f}  ({worst[2]})")


@pytest.mark.parametrize("deterministic", [False, True], ids=["default", "deterministic"])
@pytest.mark.parametrize("case", rc.CASES, ids=repr)
def test_kernels_against_float64(case, deterministic, g2s):
    c = Call(g2s)
    with mode(g2s, deterministic):
        got = run(c, case)
        again = run(c, case) if deterministic else None
        torch.cuda.synchronize()
    compare(case, got, "deterministic" if deterministic else "default")
    if again is not None:
        differing = [k for k in got if not torch.equal(got[k], again[k])]
        assert not differing, f"{case.name}: deterministic mode does not repeat bit for bit: {differing}"


# ----------------------------------------------------------------------------- weighted L1: what the ABI refuses
def test_weighted_l1_bwd3_refuses_illegal_combinations_and_writes_nothing(g2s):
    c = Call(g2s)
    i = rc.CASE["l1grid_2x3x4_real"].data()["inp"]
    B, C, HW = 2, 3, 4
    x, y, w, gadd, gadd2, gate_ref = (dev(i[k]) for k in ("x", "y", "w", "gadd", "gadd2", "gate_ref"))
    g, den = dev(i["g"]).reshape(1), dev(i["den"]).reshape(1)
    gx, gq = nans(B, C, HW), nans(B, C, HW)
    p = c.p

    def call(x_=x, y_=y, g_=g, den_=den, gadd_=gadd, gadd2_=gadd2, gx_=gx, ref_=gate_ref, gq_=gq, HW_=HW):
        return c.L.g2s_weighted_l1_bwd3(p(x_), p(y_), p(w), p(g_), p(den_), p(gadd_), p(gadd2_), 0.5, p(gx_), p(ref_), 0.25, 2.0,
                                        p(gq_), B, C, HW_, g2s.stream())
    illegal = dict(no_y=dict(y_=None), no_g=dict(g_=None), no_den=dict(den_=None), nothing=dict(x_=None, gadd_=None, gadd2_=None),
                   gadd2_alone=dict(gadd_=None), no_output=dict(gx_=None, gq_=None, ref_=None), gate_without_ref=dict(ref_=None),
                   ref_without_gate=dict(gq_=None), hw_not_4=dict(HW_=3), hw_zero=dict(HW_=0))
    for name, kw in illegal.items():
        assert call(**kw) != 0, f"{name}: accepted"
        torch.cuda.synchronize()
        assert bool(torch.isnan(gx).all()) and bool(torch.isnan(gq).all()), f"{name}: wrote to an output"
    assert call() == 0       # the accepted call does write
    torch.cuda.synchronize()
    assert not bool(torch.isnan(gx).any()) and not bool(torch.isnan(gq).any())


# ----------------------------------------------------------------------------- weighted L1 past the workgroup caps
@pytest.mark.parametrize("deterministic", [False, True], ids=["default", "deterministic"])
def test_weighted_l1_large_exact(deterministic, g2s):
    """(2, 9, 1024 x 1024): 4608 workgroups' worth of float4, past the 2048 cap of the forward and the 4096 cap
    of the backward, so every launch is a strided loop.  Exact-grid inputs from index arithmetic
    (reduce_cases.large_l1): the sums and every gradient element must equal the integer arithmetic."""
    c = Call(g2s)
    B, C, HW, coef = (rc.LARGE[k] for k in ("B", "C", "HW", "coef"))
    w01, x4, y4 = rc.large_l1(torch, B, C, HW)
    quarters = int(((x4 - y4).abs() * w01[:, None, :]).sum())
    den_true = C * int(w01.sum())
    assert 0 < quarters < 2 ** 24 and den_true < 2 ** 24
    x, y, w = x4.float() * 0.25, y4.float() * 0.25, w01.float()
    want = torch.sign(x4 - y4).float() * w[:, None, :] * coef
    del x4, y4, w01
    sz = (B, C, HW)
    with mode(g2s, deterministic):
        num, numden = zeros(1), zeros(2)
        c("g2s_weighted_l1_fwd", c.p(x), c.p(y), c.p(w), c.p(num), *sz)
        c("g2s_weighted_l1_fwd2", c.p(x), c.p(y), c.p(w), c.p(numden), *sz)
        assert float(num) == quarters * 0.25 and float(numden[0]) == quarters * 0.25 and float(numden[1]) == den_true, \
            (float(num), float(numden[0]), quarters * 0.25, float(numden[1]), den_true)
        k, one = torch.tensor([coef], device="cuda"), torch.ones(1, device="cuda")
        gx = nans(*sz)
        c("g2s_weighted_l1_bwd", c.p(x), c.p(y), c.p(w), c.p(k), c.p(gx), *sz)
        assert torch.equal(gx, want), "g2s_weighted_l1_bwd"
        gx.fill_(NAN)
        c("g2s_weighted_l1_bwd2", c.p(x), c.p(y), c.p(w), c.p(k), c.p(one), None, c.p(gx), *sz)
        assert torch.equal(gx, want), "g2s_weighted_l1_bwd2"
        gx.fill_(NAN)
        c("g2s_weighted_l1_bwd3", c.p(x), c.p(y), c.p(w), c.p(k), c.p(one), None, None, 1.0, c.p(gx), None, 0.25, 2.0, None, *sz)
        assert torch.equal(gx, want), "g2s_weighted_l1_bwd3"


# ----------------------------------------------------------------------------- the autograd wrappers
def _check(case, name, val, factor=1.0, ref=None):
    d = case.data()
    ref = d["ref64"][name] if ref is None else ref
    err = float(np.abs(val.detach().cpu().double().numpy().reshape(ref.shape) - ref).max())
    assert err <= factor * d["stats"][name]["bound"], f"{case.name} wrapper {name}: {err:.3e} > {factor * d['stats'][name]['bound']:.3e}"


def test_wrapper_view_transform(g2s):
    from gan2shape_amd import fused_geometry as fg
    case = rc.CASE["view_B65"]
    i = case.data()["inp"]
    view = dev(i["view"]).requires_grad_(True)
    R, t = fg.view_transform(view, *rc.VIEW_SCALES)
    assert tuple(R.shape) == (65, 3, 3) and tuple(t.shape) == (65, 1, 3)
    (gview,) = torch.autograd.grad([R, t], view, [dev(i["gR"]), dev(i["gt"]).view(65, 1, 3)])
    for name, val in (("R", R), ("t", t), ("gview", gview)):
        _check(case, name, val)


@pytest.mark.parametrize("name", ["warp_9x33_B3", "invwarp_9x33_B3"])
def test_wrapper_warps_split_gRt_and_skip_it_when_not_needed(name, g2s):
    from gan2shape_amd import fused_geometry as fg
    case = rc.CASE[name]
    d = case.data()
    i, B, H, W = d["inp"], case.p["B"], case.p["H"], case.p["W"]
    K9 = tuple(float(k) for k in i["K9"])
    rays, cot = dev(i["rays"]), dev(i["cot"])

    def go(need_rt):
        depth = dev(i["depth"]).view(B, H, W).requires_grad_(True)
        R, t = dev(i["R"]).requires_grad_(need_rt), dev(i["t"]).view(B, 1, 3).requires_grad_(need_rt)
        if case.p.get("inv"):
            y = fg.inv_warp_grid(depth, rays, R, t, K9, rc.RCD)
            assert tuple(y.shape) == (B, H, W, 2)
        else:
            y = fg.warp_verts(depth, rays, R, t, rc.RCD)
        return y, torch.autograd.grad(y, (depth, R, t) if need_rt else (depth,), cot.view(y.shape))
    y, (gd, gR, gt) = go(True)
    assert tuple(gR.shape) == (B, 3, 3) and tuple(gt.shape) == (B, 1, 3)
    _check(case, "out", y)
    _check(case, "gdepth", gd)
    _check(case, "gRt", torch.cat([gR.reshape(B, 9), gt.reshape(B, 3)], 1))
    _, (gd2,) = go(False)
    assert torch.equal(gd2, gd)


def test_wrapper_normal_and_smooth_loss(g2s):
    from gan2shape_amd import fused_geometry as fg
    case = rc.CASE["normal_9x33_B3"]
    i = case.data()["inp"]
    depth = dev(i["depth"]).requires_grad_(True)
    n = fg.normal_from_depth(depth, dev(i["rays"]))
    (gd,) = torch.autograd.grad(n, depth, dev(i["cot"]))
    _check(case, "normal", n)
    _check(case, "gdepth", gd)
    for name in ("smooth_9x33_N3", "smoothexact_xy_N2"):
        case = rc.CASE[name]
        i = case.data()["inp"]
        p = dev(i["p"]).requires_grad_(True)
        loss = fg.smooth_loss(p)
        (gp,) = torch.autograd.grad(loss, p, dev(i["gloss"]))
        _check(case, "loss", loss)
        _check(case, "gp", gp)
    p4 = dev(i["p"]).view(1, 2, 9, 33).requires_grad_(True)      # [B,C,H,W]: flattened to maps, gradient reshaped back
    (g4,) = torch.autograd.grad(fg.smooth_loss(p4), p4, dev(i["gloss"]))
    assert torch.equal(g4.view(2, 9, 33), gp)


@pytest.mark.parametrize("name", ["shading_9x33_B3", "shading_9x33_B3n1a1", "shading_9x33_B3n1a3", "shading_9x33_B1n1a1"])
def test_wrapper_shading_sums_broadcast_gradients(name, g2s):
    from gan2shape_amd import fused_geometry as fg
    case = rc.CASE[name]
    d = case.data()
    i, B, Bn, Ba, H, W = d["inp"], case.p["B"], case.p["Bn"], case.p["Ba"], case.p["H"], case.p["W"]
    normal = dev(i["normal"]).view(Bn, H, W, 3).requires_grad_(True)
    light = dev(i["light"]).requires_grad_(True)
    albedo = dev(i["albedo"]).view(Ba, 3, H, W).requires_grad_(True)
    dif, tex = fg.shading(normal, light, albedo)
    assert tuple(dif.shape) == (B, 1, H, W) and tuple(tex.shape) == (B, 3, H, W)
    gn, gl, ga = torch.autograd.grad([tex, dif], (normal, light, albedo), [dev(i["gt"]).view(B, 3, H, W), dev(i["gd"]).view(B, 1, H, W)],
                                     retain_graph=True)
    _check(case, "diffuse", dif)
    _check(case, "texture", tex)
    _check(case, "glight", gl)
    # Bn == 1 / Ba == 1: the per-b gradients summed; the bound of a sum of B tensors is B times the bound of one
    r = d["ref64"]
    _check(case, "gnormal", gn, B // Bn, r["gnormal"].reshape(B, H, W, 3).sum(0, keepdims=True) if Bn != B else None)
    _check(case, "galbedo", ga, B // Ba, r["galbedo"].reshape(B, 3, H, W).sum(0, keepdims=True) if Ba != B else None)
    (gn0,) = torch.autograd.grad(tex, normal, dev(i["gt"]).view(B, 3, H, W))     # diffuse unused: gdiffuse is None
    _check(case, "gnormal_nogd", gn0, B // Bn, r["gnormal_nogd"].reshape(B, H, W, 3).sum(0, keepdims=True) if Bn != B else None)


def test_wrapper_depth_head(g2s):
    from gan2shape_amd import fused_geometry as fg
    for name in ("head_3x32x32_border1", "head_2x3x5_border0"):
        case = rc.CASE[name]
        i, h = case.data()["inp"], rc.HEAD
        raw = dev(i["raw"]).requires_grad_(True)
        out = fg.depth_head(raw, case.p["W"], h["lo"], h["hi"], case.p["border"], h["bd"])
        (g,) = torch.autograd.grad(out, raw, dev(i["cot"]))
        # the wrapper reduces the mean itself, in fp32: its error reaches the output through tanh' <= 1 times
        # (hi - lo) / 2 = 0.1 — covered by e32, whose mean is the sequential fp32 one
        _check(case, "out", out)
        _check(case, "g_raw", g)
