"""Case table of tests/test_warp_cases_cpu.py and tests/test_gpu_warp_paths.py: g2s_grid_sample_fwd, g2s_grid_sample_bwd
and g2s_grid_sample_bwd_workspace_bytes (csrc/grid_sample.hip), called through the C ABI.  Importable without a GPU.

A case is a dict: name, entry ("fwd" / "bwd"), the shape (B, C, IH, IW, H, W), clamp and its bounds, and for the
backward: gx / ggrid (False: the pointer is NULL), det (deterministic mode), acc_is_zero, ws_off (the workspace handed
in that many bytes past 16-byte alignment) and gy_scale.  kernel / clears / blocks are what the case is meant to reach;
`dispatch` restates the launcher and the CPU test holds the two together.

The cell choice is part of the reference.  `corner` restates corner_of in numpy float32, one rounding per step and
nothing to contract (grid_sample.hip is built with -ffp-contract=off):
    ix = ((gx + 1) / 2) * (IW - 1);  fx = floor(ix);  sane = -2 <= fx <= IW (and the same for y against IH)
    x0 = sane ? (int)fx : -2;  wx0 = (fx + 1) - ix;  wx1 = ix - fx;  a corner counts when 0 <= x0 (+1) < IW, 0 <= y0 (+1) < IH
Samples and gradients are then evaluated in float64 from those float32 weights, so no test depends on which side of a
texel border a rounding falls.  A pixel with no in-range corner (ix < -1, ix > IW, 1e30, +-inf, NaN, in x, in y or in
both) has y = 0 before the clamp, adds nothing to the texture gradient and has ggrid = (0, 0): ATen's GPU kernel adds a
corner to gix / giy only inside its bounds check.

Bounds, per output element, u = 2^-24, k = additions on the longest chain of that kernel, counted from the code:
  y      k = 4: `v = 0; v += x * w` for the four corners.  (k + 2) u sum|x * wx * wy|: the two extra roundings are the
         weight product and the term's product.  The clamp moves a value towards the reference or not at all.
  ggrid  k = 4 C: four `gix -= / +=` per channel, C channels.  (k + 2) u sum|x * w * go| * (size - 1) / 2.
  gx     float atomics: (m + 2) u sum|contribution| per texel, m = that texel's number of contributions (counted by the
         reference).  Deterministic mode: m 2^-41 + 3 u sum|contribution| (2^-41: half a unit of the 2^-40 fixed point
         per contribution; 3 u: the weight product, the contribution's product, the conversion back to float), and two
         calls are bit-identical.  The fixed point saturates at 2^23: the CPU test holds sum|contribution| below it.
The clamp gate (lo <= v <= hi, on the recomputed sample) is decided by the float64 sample: the CPU test asserts that no
clamped sample lies within its bound of lo or hi, except the deliberate pixels exactly on a texel (weights 1, 0, 0, 0)
whose texel is exactly lo or hi; those pass the gradient in torch's clamp and in the kernel alike.  SEED is fixed; it
is to be redrawn until that holds whenever a case is added (the first draw held for the cases below).

Measured on an MI355X (largest error / bound over all cases): y 0.468, ggrid 0.466, gx 0.151 with float atomics and
0.405 in deterministic mode.  Before grid_sample_bwd gated gix / giy by the corner's range, every backward case with a
ggrid failed on the 26 components of the non-finite pixels (NaN from 0 * NaN); nothing else changed.
"""
import functools
import zlib

import numpy as np

U = 2.0 ** -24
FIX_HALF = 2.0 ** -41                 # half a unit of GS_FIX = 2^40
FIX_RANGE = 2.0 ** 23                 # int64 / 2^40
SEED = 20261
LANES = 256                           # grid (ceil(H * W / 256), B)
IH, IW = 5, 7
ON_TEXEL = ((3, 1), (3, 2), (3, 3))   # (x, y) of interior texels hit exactly: gx = 0, gy = -0.5, 0, 0.5
F32 = np.float32

CASES = []


def _add(name, entry, kernel, clears=None, shape=(2, 3, IH, IW, 19, 23), clamp=1, lo=-1.0, hi=1.0, **kw):
    B, H, W = shape[0], shape[4], shape[5]
    lo, hi = float(F32(lo)), float(F32(hi))             # what the kernel receives
    CASES.append(dict(dict(name=name, entry=entry, kernel=kernel, clears=clears, shape=shape, clamp=clamp, lo=lo, hi=hi,
                           blocks=(-(-H * W // LANES), B), gx=True, ggrid=True, det=False, acc_is_zero=0, ws_off=0,
                           gy_scale=1.0), **kw))


C1 = (2, 1, IH, IW, 19, 23)
S256 = (2, 3, IH, IW, 16, 16)
_add("fwd_noclamp", "fwd", "fwd", clamp=0)
_add("fwd_clamp", "fwd", "fwd")
_add("fwd_narrow", "fwd", "fwd", lo=-0.3, hi=0.4)
_add("fwd_c1_noclamp", "fwd", "fwd", shape=C1, clamp=0)
_add("fwd_c1_narrow", "fwd", "fwd", shape=C1, lo=-0.3, hi=0.4)
_add("fwd_256", "fwd", "fwd", shape=S256, lo=-0.3, hi=0.4)
for _det, _t, _k, _cl in ((False, "float", "bwd<float>", "gx"), (True, "det", "bwd<fixed>", "workspace")):
    _add(f"bwd_both_{_t}", "bwd", _k, _cl, det=_det)
    _add(f"bwd_noclamp_{_t}", "bwd", _k, _cl, det=_det, clamp=0)
    _add(f"bwd_narrow_{_t}", "bwd", _k, _cl, det=_det, lo=-0.3, hi=0.4)
    _add(f"bwd_nogx_{_t}", "bwd", "bwd<float>", None, det=_det, gx=False)       # no gx: no fixed point either
    _add(f"bwd_noggrid_{_t}", "bwd", _k, _cl, det=_det, ggrid=False, lo=-0.3, hi=0.4)
    _add(f"bwd_acczero_{_t}", "bwd", _k, None, det=_det, acc_is_zero=1)
    _add(f"bwd_c1_{_t}", "bwd", _k, _cl, det=_det, shape=C1, lo=-0.3, hi=0.4)
    _add(f"bwd_256_{_t}", "bwd", _k, _cl, det=_det, shape=S256)
_add("bwd_ws_offset_det", "bwd", "bwd<fixed>", "workspace", det=True, ws_off=4, lo=-0.3, hi=0.4)
_add("bwd_scale1e5_det", "bwd", "bwd<fixed>", "workspace", det=True, gy_scale=1e5)
_add("bwd_scale1e-9_det", "bwd", "bwd<fixed>", "workspace", det=True, gy_scale=1e-9)

NAMES = [c["name"] for c in CASES]
CASE = {c["name"]: c for c in CASES}
assert len(CASE) == len(CASES)


def workspace_bytes(B, C, ih, iw):
    """`if (B <= 0 || C <= 0 || IH <= 0 || IW <= 0) return 0; return B * C * IH * IW * sizeof(long long) + 256`"""
    return 0 if min(B, C, ih, iw) <= 0 else B * C * ih * iw * 8 + 256


def dispatch(c):
    """(kernel, what the launcher clears first, grid) of a case."""
    if c["entry"] == "fwd":
        return "fwd", None, c["blocks"]
    # `if (gx && deterministic()) { ...; if (!acc_is_zero) memset(fix); bwd<true>; fixed_to_float }
    #  else { if (gx && !acc_is_zero) memset(gx); bwd<false>(need_gx = gx != nullptr) }`
    B, H, W = c["shape"][0], c["shape"][4], c["shape"][5]
    grid = (-(-H * W // LANES), B)
    if c["gx"] and c["det"]:
        return "bwd<fixed>", (None if c["acc_is_zero"] else "workspace"), grid
    return "bwd<float>", ("gx" if c["gx"] and not c["acc_is_zero"] else None), grid


def placed_pixels():
    """(gx, gy, tag) of the hand-placed pixels, written over the first pixels of every sample."""
    inf, nan = np.inf, np.nan
    p = [(-1.0, -1.0, "corner"), (1.0, 1.0, "corner"), (1.0, -1.0, "corner")]
    p += [(2.0 * x / (IW - 1) - 1.0, 2.0 * y / (IH - 1) - 1.0, "texel") for x, y in ON_TEXEL]
    p += [(-1.2, 0.3, "one column"), (1.2, 0.3, "one column"), (0.3, -1.2, "one row"), (0.3, 1.3, "one row"),
          (-1.2, 1.3, "one corner")]
    p += [(-1.5, 0.3, "sane edge"), (1.5, 0.3, "sane edge"), (0.3, -2.0, "sane edge"), (0.3, 1.5, "sane edge")]   # fx -2, IW; fy -2, IH
    p += [(-2.0, 0.3, "far"), (2.0, 0.3, "far"), (0.3, -2.5, "far"), (0.3, 2.0, "far")]                              # fx -3, IW + 2
    for v, t in ((1e30, "1e30"), (inf, "+inf"), (-inf, "-inf"), (nan, "nan")):
        p += [(v, 0.3, t + " x"), (0.3, v, t + " y"), (v, v, t + " xy")]
    return p


@functools.lru_cache(maxsize=None)
def inputs(name):
    """x [B, C, IH, IW], grid [B, H, W, 2], gy [B, C, H, W] (backward) as read-only float32."""
    c = CASE[name]
    B, C, ih, iw, H, W = c["shape"]
    rng = np.random.default_rng([SEED, zlib.crc32(name.encode())])
    x = (0.8 * rng.standard_normal((B, C, ih, iw))).astype(F32)
    (tx, ty0), (_, ty1), _ = ON_TEXEL
    x[:, :, ty0, tx], x[:, :, ty1, tx] = c["lo"], c["hi"]          # the texels the exact pixels land on
    yy, xx = np.meshgrid(np.linspace(-1, 1, H), np.linspace(-1, 1, W), indexing="ij")
    grid = np.empty((B, H, W, 2), F32)
    for b in range(B):          # a smooth warp that spills beyond +-1
        grid[b, ..., 0] = 1.25 * xx + 0.15 * np.sin(3.0 * yy + b) + 0.02 * rng.standard_normal((H, W))
        grid[b, ..., 1] = 1.25 * yy + 0.15 * np.cos(2.0 * xx - b) + 0.02 * rng.standard_normal((H, W))
    flat = grid.reshape(B, H * W, 2)
    for i, (px, py, _) in enumerate(placed_pixels()):
        flat[:, i] = (px, py)
    flat[:, H * W - 1] = (np.nan, 0.1)                              # the last lane of the ragged workgroup
    d = dict(x=x, grid=grid, gy=None)
    if c["entry"] == "bwd":
        d["gy"] = (rng.standard_normal((B, C, H, W)) * c["gy_scale"]).astype(F32)
    for a in d.values():
        if a is not None:
            a.setflags(write=False)
    return d


def corner(g, size):
    """corner_of along one axis in numpy float32: (i0, w0, w1, in0, in1, sane, ix) for coordinates g."""
    with np.errstate(invalid="ignore", over="ignore"):
        ix = ((g.astype(F32) + F32(1.0)) / F32(2.0)) * F32(size - 1)
        fx = np.floor(ix)
        sane = (fx >= F32(-2.0)) & (fx <= F32(size))
        w0, w1 = (fx + F32(1.0)) - ix, ix - fx
    assert ix.dtype == fx.dtype == w0.dtype == w1.dtype == F32
    return fx, w0, w1, sane, ix


def cells(name):
    """The four corners of every pixel: a list of (texel y, texel x, in range, wx, wy, sign of d/dx, sign of d/dy) in
    the kernel's order nw, ne, sw, se; texel indices are 0 where the corner is out of range."""
    c, d = CASE[name], inputs(name)
    ih, iw = c["shape"][2], c["shape"][3]
    fx, wx0, wx1, sx, _ = corner(d["grid"][..., 0], iw)
    fy, wy0, wy1, sy, _ = corner(d["grid"][..., 1], ih)
    sane = sx & sy
    x0 = np.where(sane, fx, -2).astype(np.int64)
    y0 = np.where(sane, fy, -2).astype(np.int64)
    out = []
    for dy, wy, sgy in ((0, wy0, -1.0), (1, wy1, 1.0)):
        for dx, wx, sgx in ((0, wx0, -1.0), (1, wx1, 1.0)):
            ok = (x0 + dx >= 0) & (x0 + dx < iw) & (y0 + dy >= 0) & (y0 + dy < ih)
            out.append((np.where(ok, y0 + dy, 0), np.where(ok, x0 + dx, 0), ok, wx, wy, sgx, sgy))
    return out


@functools.lru_cache(maxsize=None)
def expected(name):
    """Float64 values and bounds: y_raw / y / y_bound [B, C, H, W]; for the backward gx / gx_bound / m / gx_abs
    [B, C, IH, IW] and ggrid / ggrid_bound [B, H, W, 2]; live [B, H, W]: the pixel has an in-range corner."""
    c, d = CASE[name], inputs(name)
    B, C, ih, iw, H, W = c["shape"]
    x = d["x"].astype(np.float64)
    cs = cells(name)
    bi = np.arange(B)[:, None, None]
    v, va = np.zeros((B, C, H, W)), np.zeros((B, C, H, W))
    tex, wgt = [], []
    for ty, tx, ok, wx, wy, _, _ in cs:
        t = x[bi, :, ty, tx].transpose(0, 3, 1, 2)                  # [B, C, H, W]
        w = np.where(ok, wx.astype(np.float64) * wy.astype(np.float64), 0.0)
        t = np.where(ok[:, None], t, 0.0)
        tex.append(t)
        wgt.append(w)
        v += t * w[:, None]
        va += np.abs(t * w[:, None])
    e = dict(y_raw=v, y_bound=(4 + 2) * U * va, live=np.any([k[2] for k in cs], axis=0))
    e["y"] = np.clip(v, c["lo"], c["hi"]) if c["clamp"] else v
    if c["entry"] == "fwd":
        return e
    go = d["gy"].astype(np.float64)
    if c["clamp"]:
        go = np.where((v >= c["lo"]) & (v <= c["hi"]), go, 0.0)
    gx, ga, m = np.zeros((B, C, ih, iw)), np.zeros((B, C, ih, iw)), np.zeros((B, C, ih, iw), np.int64)
    gix, giy, gixa, giya = np.zeros((B, H, W)), np.zeros((B, H, W)), np.zeros((B, H, W)), np.zeros((B, H, W))
    ci = np.arange(C)[None, :, None, None]
    for (ty, tx, ok, wx, wy, sgx, sgy), t, w in zip(cs, tex, wgt):
        idx = (np.broadcast_to(bi[:, None], go.shape), np.broadcast_to(ci, go.shape),
               np.broadcast_to(ty[:, None], go.shape), np.broadcast_to(tx[:, None], go.shape))
        okc = np.broadcast_to(ok[:, None], go.shape)
        contrib = w[:, None] * go
        np.add.at(gx, tuple(i[okc] for i in idx), contrib[okc])
        np.add.at(ga, tuple(i[okc] for i in idx), np.abs(contrib[okc]))
        np.add.at(m, tuple(i[okc] for i in idx), 1)
        wxm, wym = np.where(ok, wx.astype(np.float64), 0.0), np.where(ok, wy.astype(np.float64), 0.0)
        tx_ = (t * wym[:, None] * go).sum(1)
        ty_ = (t * wxm[:, None] * go).sum(1)
        gix += sgx * tx_
        giy += sgy * ty_
        gixa += np.abs(t * wym[:, None] * go).sum(1)
        giya += np.abs(t * wxm[:, None] * go).sum(1)
    sx, sy = float(F32(iw - 1) / F32(2.0)), float(F32(ih - 1) / F32(2.0))
    e.update(gx=gx, gx_abs=ga, m=m, gx_bound=(m * FIX_HALF + 3 * U * ga) if dispatch(c)[0] == "bwd<fixed>" else (m + 2) * U * ga,
             ggrid=np.stack([sx * gix, sy * giy], -1),
             ggrid_bound=(4 * C + 2) * U * np.stack([sx * gixa, sy * giya], -1))
    return e


def exact_on_limit(name):
    """[B, C, H, W] mask of the deliberate samples: weights exactly (1, 0, 0, 0) on a texel that is exactly lo or hi."""
    c, d = CASE[name], inputs(name)
    (ty, tx, ok, wx, wy, _, _), ne, sw, se = cells(name)
    one = ok & (wx == 1) & (wy == 1) & (ne[3] == 0) & (sw[4] == 0)
    t = d["x"][np.arange(c["shape"][0])[:, None, None], :, ty, tx].transpose(0, 3, 1, 2)
    return one[:, None] & ((t == F32(c["lo"])) | (t == F32(c["hi"])))


def emulate32(name):
    """The kernels' float32 arithmetic in their own order (forward sample and ggrid), for the CPU test."""
    c, d = CASE[name], inputs(name)
    B, C, ih, iw, H, W = c["shape"]
    cs = cells(name)
    bi = np.arange(B)[:, None, None]
    z = F32(0.0)
    with np.errstate(invalid="ignore", over="ignore"):
        ts = [np.where(ok[:, None], d["x"][bi, :, ty, tx].transpose(0, 3, 1, 2), z) for ty, tx, ok, *_ in cs]
        ws = [(wx * wy)[:, None] for _, _, _, wx, wy, _, _ in cs]
        v = np.zeros((B, C, H, W), F32)
        for (_, _, ok, *_), t, w in zip(cs, ts, ws):
            v = np.where(ok[:, None], v + t * w, v)
        y = np.where(v < F32(c["lo"]), F32(c["lo"]), np.where(v > F32(c["hi"]), F32(c["hi"]), v)) if c["clamp"] else v
        if c["entry"] == "fwd":
            return dict(y=y)
        go = d["gy"]
        if c["clamp"]:
            go = np.where((v >= F32(c["lo"])) & (v <= F32(c["hi"])), go, z)
        gix, giy = np.zeros((B, H, W), F32), np.zeros((B, H, W), F32)
        for ch in range(C):
            for (_, _, ok, wx, wy, sgx, sgy), t in zip(cs, ts):      # a corner counts only when it is in range
                gix = np.where(ok, gix + F32(sgx) * (t[:, ch] * wy * go[:, ch]), gix)
                giy = np.where(ok, giy + F32(sgy) * (t[:, ch] * wx * go[:, ch]), giy)
        gg = np.stack([(F32(iw - 1) / F32(2.0)) * gix, (F32(ih - 1) / F32(2.0)) * giy], -1)
    assert y.dtype == gg.dtype == F32
    return dict(y=y, ggrid=gg)
