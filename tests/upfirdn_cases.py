"""Case table of tests/test_upfirdn_cases_cpu.py and tests/test_gpu_upfirdn_paths.py: upfirdn2d (csrc/upfirdn2d.hip
behind g2s_upfirdn2d / _nba / _nba_ps) at shapes that reach every launch path, against a float64 restatement of the
formula in that file's header.  Importable without a GPU.

A case is (name, group, shape (N, C, H, W), up, down, pad, path, turns, adjoint path): the last three are what the
table is meant to reach and tests/test_upfirdn_cases_cpu.py holds `path` / `turns` to them.  up and down are one
rate for both axes or (x, y); pad is (before, after) for both axes or (x0, x1, y0, y1); negative pads crop.  The FIR
is the asymmetric kernel of test_upfirdn2d_vs_oracle (binomial 4 x 4 scaled by up_x * up_y, plus 0.01 N(0, 1) per
tap; 3 x 3 for the cases that say so): a symmetric one would hide a missing flip.  Inputs are seeded N(0, 1) draws
rounded to float32 (float16 for the f16 group: the reference sees the rounded values); every case has at least two
planes with different data.

The paths (`path` restates dispatch and launch_tiled, `turns` the plane loop's grid):

  generic   anything but a 4 x 4 kernel at (up, down) = (1, 1), (2, 1), (1, 2) with equal rates on both axes
  up2       (2, 1): polyphase body, 32 x 32 tiles at every width
  t32       up = 1, out_w <= 47: 32 x 32 tiles          t160   129 <= out_w <= 160: one 160-wide tile per row band,
  t64       48 <= out_w <= 95: 64 x 16                         the first 32 lanes take a second turn over x
  t128      96 <= out_w <= 128: 128 x 16                t128x  out_w > 160: several 128-wide column tiles
  plane loop: gridDim.y = min(major, max(1, 2048 / tiles)); a workgroup filters planes m, m + gridDim.y, ... and
  fetches the next plane while it filters the current one.  It turns again only when major > 2048 / tiles.

Groups:
  d1, d2    UP = 1 with DOWN = 1 / 2 at out_w = 47|48, 95|96, 128|129, 160|161 (each pair lands on two paths) and 257
            (three column tiles, the last a single column); out_h in 17..23 and no multiple of 4, so the 4-row
            strips mask rows; d2 alternates odd and even input sizes
  up2       out_w = 31 (one tile, ragged), 33 and 34 (second tile of one / two columns), 130; an odd out_w needs an
            even pad sum (out = 2 in + p0 + p1 - 3), so 31 and 33 come with pads (1, 1) and (2, 2), and (2, 1) and
            (1, 2) with 130 and 34; input heights of both parities
  pads      (1, 1), (2, 2), (2, 1) and a crop on either side, per rate, on tiled paths
  small     3 x 5 input, every rate
  generic   3 x 3 kernel; 4 x 4 at up = down = 2 and at up 3, down 2; unequal rates per axis and a minor dimension
            of 2, both through plugins/upfirdn2d_op.py (op.upfirdn2d cannot express them: forward only)
  plane     t32: one tile, 4101 planes = 2048 + 2048 + 5; up2: 2053 planes; t160: 2 tiles, 1025 planes = 1024 + 1
  f16       one case per tiled path, both DOWN values among them, and the generic kernel
  nba       g2s_upfirdn2d_nba / _nba_ps on every tiled path, channels = 3 and B = 2 (m % channels and m / channels
            both vary), alpha 0.2 and 0.0 under either entry, maps that differ per sample for _ps, and one
            three-turn case each (the bias index has to follow m across turns)

Adjoint.  Every float32 case of the `op` entry is also differentiated: _Resample.backward is the same kernel with up
and down swapped, the flipped FIR and complementary pads (negative where the forward cropped less than a kernel).
The adjoint of a DOWN = 2 case is an up2 launch, that of an up2 case a DOWN = 2 launch at the input's width; the
last column of the table is the path it takes, and the adjoints together reach every tiled path as well.

Bounds.  float32: |kernel - ref| <= min(RATIO * e32 * max|ref|, 1e-6 + 1e-5 |ref|) per element, where e32 is the
error of op/cpu_tensors.upfirdn2d (F.conv2d on the CPU: a plain float32 restatement with its own summation order)
against the float64 reference on the same inputs, as max|float32 - float64| / max|float64|, and the second term is
what test_upfirdn2d_vs_oracle uses.  For the two cases cpu_tensors cannot express (rates per axis, minor dimension)
e32 comes from `reference` run in float32.  RATIO = 4 as in groupnorm_cases.py: another summation order may cost a few
times a restatement's own error.  float16: |kernel - ref| <= 2^-11 |ref| + 2^-25 + (the float32 bound): one rounding
of the result to half, half the smallest subnormal, the float32 accumulation.  The epilogue's reference is the tail
gain * lrelu(upfirdn2d + noise_w * noise + bias[m % channels], alpha) in float64 on the float64 upfirdn2d; its e32
is the same tail in numpy float32 on cpu_tensors' float32 result.  Leaky ReLU is continuous: no element is left out.

Measured on an MI355X, largest error / (e32 * max|ref|) over the cases of a path; no case needed more than RATIO
and none was cut by the older test's term instead (f32 worst error / bound 0.76):

             forward  adjoint  epilogue                  forward  adjoint  epilogue
    t32         1.17     1.89      1.00      t128x          1.00     1.48      1.15
    t64         1.00     1.39      1.03      up2            1.68     1.98      0.93
    t128        1.46     1.27      1.00      generic        1.00     3.03         -
    t160        1.05     1.20      0.97

The 3.03 is g_u2d2's adjoint: four taps per output leave cpu_tensors' float32 at e32 = 3.5e-8, below one rounding of
the result (2^-24), and the kernel's 1.05e-7 of scale is still under one ulp.  The plane-loop cases sit at 1.05 to
1.21 (0.89 and 1.00 with the epilogue).  f16: the worst element reaches 0.94 to 0.99 of its bound on every path, as
it must: the half rounding of the result is the whole error and the bound is that rounding's own limit."""
import functools
import zlib

import numpy as np

RATIO = 4.0
FLOOR_RTOL, FLOOR_ATOL = 1e-5, 1e-6      # test_upfirdn2d_vs_oracle's bound
MAX_BLOCKS = 2048                        # launch_tiled: gy = min(major, max(1, 2048 / tiles))
TILE = dict(t32=(32, 32), up2=(32, 32), t64=(64, 16), t128=(128, 16), t128x=(128, 16), t160=(160, 16))   # TWX, TH
TILED = tuple(TILE)
GAIN = float(np.sqrt(2.0))

EDGE_W = (47, 48, 95, 96, 128, 129, 160, 161, 257)
EDGE_PATH = dict(zip(EDGE_W, ("t32", "t64", "t64", "t128", "t128", "t160", "t160", "t128x", "t128x")))
BOUNDARY_PAIRS = ((47, 48), (95, 96), (128, 129), (160, 161))
HEIGHTS = (17, 18, 19, 21, 22, 23)       # out_h of the edge cases: 17..23, no multiple of 4


def _pair(v):
    return (v, v) if isinstance(v, int) else tuple(v)


def _pad4(p):
    return (p[0], p[1], p[0], p[1]) if len(p) == 2 else tuple(p)


def out_len(n, up, down, p0, p1, taps):
    return (n * up + p0 + p1 - taps) // down + 1


def path(up, down, kh, kw, out_w):
    """The kernel g2s_upfirdn2d launches: dispatch (rates and kernel size), then launch_tiled (out_w)."""
    (ux, uy), (dx, dy) = _pair(up), _pair(down)
    # dispatch: `sq && p.kh == 4 && p.kw == 4 && up == .. && down == ..` for (1, 1), (2, 1), (1, 2), else generic
    if not (ux == uy and dx == dy and kh == 4 and kw == 4 and (ux, dx) in ((1, 1), (2, 1), (1, 2))):
        return "generic"
    if ux == 2:
        return "up2"             # launch_tiled: every `UP == 1 && ...` branch is skipped
    if 128 < out_w <= 160:       # `UP == 1 && p.out_w > 128 && p.out_w <= 160`
        return "t160"
    if out_w >= 96:              # `UP == 1 && p.out_w >= 96`: one column tile up to 128, several above 160
        return "t128" if out_w <= 128 else "t128x"
    return "t64" if out_w >= 48 else "t32"


def turns(major, out_h, out_w, path):
    """How often the plane loop of a workgroup turns (generic: its grid-stride loop)."""
    if path == "generic":
        total = major * out_h * out_w
        grid = min(-(-total // 256), 8192)       # dispatch: `std::min(cdiv(total, 256), 8192)`
        return -(-total // (grid * 256))
    twx, th = TILE[path]
    tiles = -(-out_w // twx) * -(-out_h // th)
    gy = min(major, max(1, MAX_BLOCKS // tiles))
    return -(-major // gy)


def grid_y(major, out_h, out_w, path):
    twx, th = TILE[path]
    return min(major, max(1, MAX_BLOCKS // (-(-out_w // twx) * -(-out_h // th))))


def _place(src, dst, p0y, p0x):
    """dst[..., y, x] = src[..., y - p0y, x - p0x] where that exists: pad (positive) or crop (negative)."""
    sh, sw = src.shape[-2:]
    dh, dw = dst.shape[-2:]
    y0, y1 = max(0, p0y), min(dh, sh + p0y)
    x0, x1 = max(0, p0x), min(dw, sw + p0x)
    if y1 > y0 and x1 > x0:
        dst[..., y0:y1, x0:x1] = src[..., y0 - p0y:y1 - p0y, x0 - p0x:x1 - p0x]


def reference(x, k, up, down, pad, dtype=np.float64):
    """out[.., oy, ox] = sum_{ky, kx} U[oy * down + ky - pad_y0, ox * down + kx - pad_x0] * k[kh-1-ky, kw-1-kx], U = x
    with (up - 1) zeros after every sample, 0 outside: zero insertion, pad or crop, flipped-tap FIR, decimation."""
    (ux, uy), (dx, dy), (px0, px1, py0, py1) = _pair(up), _pair(down), _pad4(pad)
    x, k = np.asarray(x, dtype), np.asarray(k, dtype)
    H, W = x.shape[-2:]
    kh, kw = k.shape
    U = np.zeros(x.shape[:-2] + (H * uy, W * ux), dtype)
    U[..., ::uy, ::ux] = x
    P = np.zeros(x.shape[:-2] + (H * uy + py0 + py1, W * ux + px0 + px1), dtype)
    _place(U, P, py0, px0)
    oh, ow = out_len(H, uy, dy, py0, py1, kh), out_len(W, ux, dx, px0, px1, kw)
    out = np.zeros(x.shape[:-2] + (oh, ow), dtype)
    for ky in range(kh):
        for kx in range(kw):
            out += P[..., ky:ky + (oh - 1) * dy + 1:dy, kx:kx + (ow - 1) * dx + 1:dx] * k[kh - 1 - ky, kw - 1 - kx]
    return out


def reference_adjoint(g, k, up, down, pad, in_hw):
    """The transpose of `reference`, step by step backwards: scatter the taps, undo the pad or crop, read the samples
    zero insertion kept."""
    (ux, uy), (dx, dy), (px0, px1, py0, py1) = _pair(up), _pair(down), _pad4(pad)
    g, k = np.asarray(g, np.float64), np.asarray(k, np.float64)
    H, W = in_hw
    kh, kw = k.shape
    oh, ow = g.shape[-2:]
    assert (oh, ow) == (out_len(H, uy, dy, py0, py1, kh), out_len(W, ux, dx, px0, px1, kw))
    GP = np.zeros(g.shape[:-2] + (H * uy + py0 + py1, W * ux + px0 + px1))
    for ky in range(kh):
        for kx in range(kw):
            GP[..., ky:ky + (oh - 1) * dy + 1:dy, kx:kx + (ow - 1) * dx + 1:dx] += g * k[kh - 1 - ky, kw - 1 - kx]
    GU = np.zeros(g.shape[:-2] + (H * uy, W * ux))
    _place(GP, GU, -py0, -px0)
    return np.ascontiguousarray(GU[..., ::uy, ::ux])


def _edge_cases():
    rows = []
    for i, w in enumerate(EDGE_W):
        oh = HEIGHTS[i % len(HEIGHTS)]
        p = EDGE_PATH[w]
        # pad (1, 1): out = in - 1; its adjoint is a (1, 1) launch at the input's width
        rows.append((f"d1_w{w}", "d1", (1, 2, oh + 1, w + 1), 1, 1, (1, 1), p, 1, path(1, 1, 4, 4, w + 1)))
        # pad (1, 1), down 2: out = in // 2 for either parity of in; its adjoint is an up2 launch
        rows.append((f"d2_w{w}", "d2", (1, 2, 2 * oh + (i + 1) % 2, 2 * w + i % 2), 1, 2, (1, 1), p, 1, "up2"))
    return rows


CASES = _edge_cases() + [
    # name, group, shape, up, down, pad, path, turns, adjoint path
    ("up2_w31", "up2", (1, 2, 9, 16), 2, 1, (1, 1), "up2", 1, "t32"),        # 17 x 31
    ("up2_w33", "up2", (1, 2, 10, 16), 2, 1, (2, 2), "up2", 1, "t32"),       # 21 x 33
    ("up2_w34", "up2", (1, 2, 11, 17), 2, 1, (1, 2), "up2", 1, "t32"),       # 22 x 34
    ("up2_w130", "up2", (1, 2, 9, 65), 2, 1, (2, 1), "up2", 1, "t64"),       # 18 x 130
    ("up2_adj_t128", "up2", (1, 2, 9, 100), 2, 1, (2, 1), "up2", 1, "t128"),     # adjoints: DOWN = 2 on the wide tiles
    ("up2_adj_t160", "up2", (1, 2, 11, 131), 2, 1, (1, 2), "up2", 1, "t160"),
    ("up2_adj_t128x", "up2", (1, 2, 9, 163), 2, 1, (2, 1), "up2", 1, "t128x"),
    ("d1_pad22", "pads", (1, 2, 20, 70), 1, 1, (2, 2), "t64", 1, "t64"),         # 21 x 71
    ("d1_pad21", "pads", (1, 2, 18, 100), 1, 1, (2, 1), "t128", 1, "t128"),      # 18 x 100
    ("d1_crop0", "pads", (1, 2, 21, 131), 1, 1, (-1, 2), "t160", 1, "t160"),     # 19 x 129
    ("d1_crop1", "pads", (1, 2, 23, 50), 1, 1, (2, -1), "t64", 1, "t64"),        # 21 x 48
    ("d1_t32_adj", "pads", (1, 2, 18, 30), 1, 1, (2, 2), "t32", 1, "t32"),       # 19 x 31; the (1, 1) adjoint on t32
    ("d2_pad22", "pads", (1, 2, 37, 101), 1, 2, (2, 2), "t64", 1, "up2"),        # 19 x 51
    ("d2_pad21", "pads", (1, 2, 35, 200), 1, 2, (2, 1), "t128", 1, "up2"),       # 18 x 100
    ("d2_crop0", "pads", (1, 2, 40, 263), 1, 2, (-1, 2), "t160", 1, "up2"),      # 19 x 131
    ("d2_crop1", "pads", (1, 2, 43, 60), 1, 2, (2, -1), "t32", 1, "up2"),        # 21 x 29
    ("up2_crop0", "pads", (1, 2, 10, 17), 2, 1, (-1, 2), "up2", 1, "t32"),       # 18 x 32
    ("up2_crop1", "pads", (1, 2, 11, 25), 2, 1, (2, -1), "up2", 1, "t32"),       # 20 x 48
    ("small_d1", "small", (1, 2, 3, 5), 1, 1, (2, 2), "t32", 1, "t32"),          # 4 x 6
    ("small_d2", "small", (1, 2, 3, 5), 1, 2, (2, 2), "t32", 1, "up2"),          # 2 x 3
    ("small_up2", "small", (1, 2, 3, 5), 2, 1, (2, 1), "up2", 1, "t32"),         # 6 x 10
    ("g_k3", "generic", (1, 2, 19, 37), 1, 1, (1, 1), "generic", 1, "generic"),
    ("g_u2d2", "generic", (1, 2, 17, 21), 2, 2, (2, 1), "generic", 1, "generic"),
    ("g_u3d2", "generic", (1, 2, 13, 15), 3, 2, (2, 3), "generic", 1, "generic"),
    ("g_rates_x", "generic", (1, 2, 18, 20), (2, 1), (1, 1), (2, 1, 1, 1), "generic", 1, None),     # up_x 2, up_y 1
    ("g_rates_y", "generic", (1, 2, 36, 20), (1, 1), (1, 2), (1, 1, 2, 1), "generic", 1, None),     # down_y 2
    ("g_minor", "generic", (2, 2, 17, 9), 1, 1, (1, 1), "generic", 1, None),     # [major 2, 17, 9, minor 2], 3 x 3
    ("pl_t32", "plane", (1, 4101, 8, 8), 1, 1, (1, 1), "t32", 3, "t32"),         # 7 x 7
    ("pl_up2", "plane", (1, 2053, 8, 8), 2, 1, (2, 1), "up2", 2, "t32"),         # 16 x 16
    ("pl_t160", "plane", (1, 1025, 20, 130), 1, 1, (1, 1), "t160", 2, "t160"),   # 19 x 129: 2 tiles, gy = 1024
    ("f16_t32", "f16", (1, 2, 18, 30), 1, 1, (1, 1), "t32", 1, None),
    ("f16_t64", "f16", (1, 2, 37, 141), 1, 2, (1, 1), "t64", 1, None),           # 18 x 70
    ("f16_t128", "f16", (1, 2, 20, 121), 1, 1, (1, 1), "t128", 1, None),
    ("f16_t160", "f16", (1, 2, 43, 300), 1, 2, (1, 1), "t160", 1, None),         # 21 x 150
    ("f16_t128x", "f16", (1, 2, 23, 201), 1, 1, (1, 1), "t128x", 1, None),
    ("f16_up2", "f16", (1, 2, 9, 20), 2, 1, (2, 1), "up2", 1, None),             # 18 x 40
    ("f16_generic", "f16", (1, 2, 13, 15), 3, 2, (2, 3), "generic", 1, None),
]

# epilogue cases: name -> (entry, alpha); shape (B, channels, H, W) with channels = 3
_NBA = [("t32", (2, 3, 18, 30), 1, 1, (1, 1)), ("t64", (2, 3, 37, 141), 1, 2, (1, 1)),
        ("t128", (2, 3, 20, 121), 1, 1, (1, 1)), ("t160", (2, 3, 43, 300), 1, 2, (1, 1)),
        ("t128x", (2, 3, 23, 201), 1, 1, (1, 1)), ("up2", (2, 3, 9, 20), 2, 1, (2, 1))]
EPILOGUE = {}
for _i, (_p, _shape, _up, _down, _pad) in enumerate(_NBA):
    for _j, _entry in enumerate(("nba", "nba_ps")):
        CASES.append((f"{_entry}_{_p}", "nba", _shape, _up, _down, _pad, _p, 1, None))
        EPILOGUE[f"{_entry}_{_p}"] = (_entry, 0.2 if (_i + _j) % 2 == 0 else 0.0)
for _entry, _alpha in (("nba", 0.2), ("nba_ps", 0.0)):
    CASES.append((f"pl_{_entry}", "nba", (1367, 3, 8, 8), 1, 1, (1, 1), "t32", 3, None))      # 4101 planes
    EPILOGUE[f"pl_{_entry}"] = (_entry, _alpha)

NAMES = [c[0] for c in CASES]
CASE = {c[0]: c for c in CASES}
assert len(CASE) == len(CASES)
PLUGIN_ONLY = ("g_rates_x", "g_rates_y", "g_minor")     # what op.upfirdn2d cannot express: forward only
K3 = ("g_k3", "g_minor")                                # 3 x 3 kernel
FORWARD = [n for n in NAMES if CASE[n][1] not in ("f16", "nba", "plane")]
ADJOINT = [n for n in NAMES if CASE[n][1] not in ("f16", "nba") and n not in PLUGIN_ONLY]
F16 = [n for n in NAMES if CASE[n][1] == "f16"]
NBA = list(EPILOGUE)
PLANE = [n for n in NAMES if CASE[n][7] > 1]


def geometry(name):
    """(major, H, W, up (x, y), down (x, y), pad (x0, x1, y0, y1), kh, kw, out_h, out_w) of a case."""
    _, _, (N, C, H, W), up, down, pad, *_ = CASE[name]
    (ux, uy), (dx, dy), p = _pair(up), _pair(down), _pad4(pad)
    kh = kw = 3 if name in K3 else 4
    return (N * C, H, W, (ux, uy), (dx, dy), p, kh, kw, out_len(H, uy, dy, p[2], p[3], kh),
            out_len(W, ux, dx, p[0], p[1], kw))


def adjoint_geometry(name):
    """The launch _Resample.backward makes: (up, down, pad (x0, x1, y0, y1), out_h, out_w) — rates swapped, what is
    left of the kernel support on either side as pads; restated, not imported."""
    _, H, W, (ux, uy), (dx, dy), (px0, _, py0, _), kh, kw, oh, ow = geometry(name)
    apad = (kw - px0 - 1, W * ux - ow * dx + px0 - ux + 1, kh - py0 - 1, H * uy - oh * dy + py0 - uy + 1)
    return (dx, dy), (ux, uy), apad, out_len(oh, dy, uy, apad[2], apad[3], kh), out_len(ow, dx, ux, apad[0], apad[1], kw)


def fir(rng, size, gain):
    b = np.array([1, 3, 3, 1] if size == 4 else [1, 2, 1], np.float32)
    k = np.outer(b, b).astype(np.float32)
    return (k / k.sum() * gain + 0.01 * rng.standard_normal((size, size)).astype(np.float32)).astype(np.float32)


def rel_err(got, want):
    return float(np.abs(np.asarray(got, np.float64) - want).max() / np.abs(want).max())


def f32_bound(ref, e32):
    """Per element: what |kernel - ref| of a float32 launch may be."""
    return np.minimum(RATIO * e32 * np.abs(ref).max(), FLOOR_ATOL + FLOOR_RTOL * np.abs(ref))


def f16_bound(ref, e32):
    return 2.0 ** -11 * np.abs(ref) + 2.0 ** -25 + f32_bound(ref, e32)


def tail(v, bias, noise, nw, alpha, gain, dtype):
    """gain * lrelu(v + nw * noise + bias[c], alpha) for v (B, C, oh, ow), noise (oh, ow) or (B, oh, ow)."""
    v, bias, noise = (np.asarray(a, dtype) for a in (v, bias, noise))
    nz = noise[:, None] if noise.ndim == 3 else noise[None, None]
    t = v + (bias[None, :, None, None] + dtype(nw) * nz)
    return np.where(t > 0, t, t * dtype(alpha)) * dtype(gain)


def _cpu_tensors_f32(x, k, up, down, pad, gy=None):
    import torch
    from gan2shape_amd.op import cpu_tensors
    xt = torch.tensor(x, dtype=torch.float32, requires_grad=gy is not None)
    y = cpu_tensors.upfirdn2d(xt, torch.tensor(k), up, down, pad)
    if gy is None:
        return y.numpy(), None
    y.backward(torch.tensor(gy))
    return y.detach().numpy(), xt.grad.numpy()


@functools.lru_cache(maxsize=None)
def data(name):
    """Everything the tests need of a case, computed once and read-only: x (float32, or float16 in the f16 group), k,
    ref (float64) and e32; gy, ref_adj and e32_adj where the case is differentiated; bias, noise, nw, alpha where it
    has an epilogue (then ref and e32 are those of the whole expression)."""
    _, group, shape, up, down, pad, *_ = CASE[name]
    major, H, W, (ux, uy), (dx, dy), pad4, kh, kw, oh, ow = geometry(name)
    rng = np.random.default_rng([20252, zlib.crc32(name.encode())])
    x = rng.standard_normal(shape).astype(np.float32)
    if group == "f16":
        x = x.astype(np.float16)
    k = fir(rng, kh, ux * uy)
    ref = reference(x, k, up, down, pad)
    out = dict(x=x, k=k)
    if name in PLUGIN_ONLY:
        r32 = reference(x.astype(np.float32), k, up, down, pad, np.float32)
    elif name in ADJOINT:
        gy = rng.standard_normal(ref.shape).astype(np.float32)
        r32, a32 = _cpu_tensors_f32(x, k, up, down, pad, gy)
        out["gy"], out["ref_adj"] = gy, reference_adjoint(gy, k, up, down, pad, (H, W))
        out["e32_adj"] = rel_err(a32, out["ref_adj"])
    else:
        r32, _ = _cpu_tensors_f32(x.astype(np.float32), k, up, down, pad)
    if name in EPILOGUE:
        entry, alpha = EPILOGUE[name]
        bias = rng.standard_normal(shape[1]).astype(np.float32)
        noise = rng.standard_normal((shape[0], oh, ow) if entry == "nba_ps" else (oh, ow)).astype(np.float32)
        nw = np.float32(0.7)
        ref = tail(ref, bias, noise, nw, alpha, GAIN, np.float64)
        r32 = tail(r32, bias, noise, nw, alpha, np.float32(GAIN), np.float32)
        out.update(bias=bias, noise=noise, nw=nw, alpha=alpha)
    out["ref"], out["e32"] = ref, rel_err(r32, ref)
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out
