"""Case table of tests/test_pool_cases_cpu.py and tests/test_gpu_pool_paths.py: g2s_res_split_fwd / _bwd,
g2s_avg_pyramid and g2s_maxpool2x2_fwd / _bwd (csrc/pool.hip), called through the C ABI.  Importable without a GPU.

A case is a dict: name, entry, shape (planes, H, W) and the entry's parameters.  `dispatch` restates the launchers'
grids; the CPU test holds them against what each shape was chosen for.

  split    g2s_res_split_fwd / _bwd: one lane per 2 x 2 window, `cdiv(windows, 256)` workgroups.  relu_out = relu(x)
           (NaN stays NaN), pool_out = ((((0 + a) + b) + c) + d) / 4 in ATen's order; backward
           gx = (x <= 0 ? 0 : g_relu) + g_pool / 4 — torch's threshold_backward, which passes the gradient where x is NaN
           (the CPU test checks the rule against torch.relu) — with both gradients, with g_relu NULL, with g_pool NULL.
           x holds exact zeros, -0.0 and NaNs.
  pyramid  g2s_avg_pyramid: one lane per (2^levels)^2 block, 64 lanes per workgroup; every level is the successive
           2 x 2 average of the one before, in the same order.  Levels above n_levels are NULL.
  maxpool  g2s_maxpool2x2_fwd / _bwd: one lane per quad (4 outputs), at most 2048 workgroups of 256 lanes:
           (1, 2050, 4096) has 524 800 quads, 512 past the cap, so some lanes take a second turn.  The winner of a
           window (a b / c d) is the first maximum in the order a, b, c, d, and a NaN beats everything before it
           (`v > best || v != v`, torch's rule); the backward writes gy at the winner and 0 elsewhere.  Ties, NaN in
           each of the four positions (and in two at once), windows of -inf.

Expected values: the same expression in numpy float32 in the kernel's order, bit for bit (NaNs compared as NaNs).  No
sum longer than the four terms of a window occurs.  One place may contract: g_pool / 4 is g_pool * 0.25 to the compiler,
and `gate + g_pool * 0.25` may become one fused multiply-add (pool.hip is built with contraction on).  `expected` gives
both candidates, the two-rounding sum and the fma evaluated through float64, and every element must equal one of them;
the quotient by 4 is exact for every normal number, so the two coincide here and the GPU test prints how many elements
differ from the first candidate.  Measured on an MI355X: 0 elements in every case; every other output has one
expectation and is bit-identical to it.  With the earlier gate `x > 0 ? g : 0` the split_bwd cases that have a g_relu
failed at the NaN inputs alone (0 where torch passes g_relu); nothing else changed.
"""
import functools
import zlib

import numpy as np

F32 = np.float32
LANES = 256
MAXPOOL_BLOCKS = 256 * 8           # `std::min<long>((quads + 255) / 256, 256 * 8)`
PYRAMID_LANES = 64

CASES = []


def _add(name, entry, shape, **kw):
    CASES.append(dict(name=name, entry=entry, shape=shape, **kw))


for _s in ((1, 2, 2), (3, 4, 6), (5, 6, 22), (4, 16, 18)):
    _t = "x".join(map(str, _s))
    _add(f"split_fwd_{_t}", "split_fwd", _s)
    for _g, _n in (((True, True), "both"), ((False, True), "norelu"), ((True, False), "nopool")):
        _add(f"split_bwd_{_n}_{_t}", "split_bwd", _s, g_relu=_g[0], g_pool=_g[1])
for _l in (1, 2, 3, 4):
    _add(f"pyramid_2x16x32_l{_l}", "pyramid", (2, 16, 32), levels=_l)
_add("pyramid_1x2x2_l1", "pyramid", (1, 2, 2), levels=1)
_add("pyramid_3x8x24_l3", "pyramid", (3, 8, 24), levels=3)
_add("pyramid_65x4x4_l2", "pyramid", (65, 4, 4), levels=2)
for _s in ((1, 2, 8), (3, 6, 16), (1, 2050, 4096)):
    _t = "x".join(map(str, _s))
    _add(f"maxpool_fwd_{_t}", "maxpool_fwd", _s)
    _add(f"maxpool_bwd_{_t}", "maxpool_bwd", _s)

NAMES = [c["name"] for c in CASES]
CASE = {c["name"]: c for c in CASES}
assert len(CASE) == len(CASES)


def _cdiv(a, b):
    return -(-a // b)


def dispatch(c):
    """dict(units, blocks, live lanes of the last workgroup, turns of the grid-stride loop)."""
    P, H, W = c["shape"]
    e = c["entry"]
    if e.startswith("split"):           # `windows = planes * (H / 2) * (W / 2); <<<cdiv(windows, 256), 256>>>`
        n = P * (H // 2) * (W // 2)
        return dict(units=n, blocks=_cdiv(n, LANES), last=n - (_cdiv(n, LANES) - 1) * LANES, turns=1)
    if e == "pyramid":                  # `blocks = planes * (H / S) * (W / S); <<<cdiv(blocks, 64), 64>>>`
        S = 1 << c["levels"]
        n = P * (H // S) * (W // S)
        return dict(units=n, blocks=_cdiv(n, PYRAMID_LANES), last=n - (_cdiv(n, PYRAMID_LANES) - 1) * PYRAMID_LANES, turns=1)
    n = P * (H // 2) * (W // 8)         # `quads = planes * (H / 2) * (W / 8); <<<min((quads + 255) / 256, 2048), 256>>>`
    blocks = min(_cdiv(n, LANES), MAXPOOL_BLOCKS)
    return dict(units=n, blocks=blocks, last=None, turns=_cdiv(n, blocks * LANES))


@functools.lru_cache(maxsize=None)
def inputs(name):
    c = CASE[name]
    P, H, W = c["shape"]
    rng = np.random.default_rng([20263, zlib.crc32(name.encode())])
    f = lambda *s: rng.standard_normal(s).astype(F32)
    e = c["entry"]
    if e.startswith("split"):
        x = f(P, H, W)
        flat = x.reshape(-1)
        flat[0] = np.nan
        if flat.size > 8:
            flat[-1] = flat[flat.size // 2] = np.nan                 # the first and the last lane, and one in between
            flat[5], flat[7] = 0.0, -0.0
        flat[1], flat[2] = 0.0, -0.0
        d = dict(x=x)
        if e == "split_bwd":
            d["g_relu"] = f(P, H, W) if c["g_relu"] else None
            if d["g_relu"] is not None:
                d["g_relu"].reshape(-1)[0] = F32(1.5)                # a positive gradient on a NaN
            d["g_pool"] = f(P, H // 2, W // 2) if c["g_pool"] else None
    elif e == "pyramid":
        d = dict(x=f(P, H, W))
    else:
        x = rng.integers(-2, 3, (P, H, W)).astype(F32)              # small integers: ties in most windows
        win = x.reshape(P, H // 2, 2, W // 2, 2)                     # [p, oy, dy, ox, dx]
        nw = (H // 2) * (W // 2)
        for k in range(4):                                           # a NaN in each of the four positions
            oy, ox = divmod((k * 5 + 1) % nw, W // 2)
            win[0, oy, k // 2, ox, k % 2] = np.nan
        oy, ox = divmod(2 % nw, W // 2)
        win[-1, oy, 0, ox, 0] = win[-1, oy, 1, ox, 1] = np.nan       # two in one window: the later one wins
        oy, ox = divmod(3 % nw, W // 2)
        win[-1, oy, :, ox, :] = -np.inf                              # all -inf: the first wins
        oy, ox = divmod(0, W // 2)
        win[-1, oy, :, ox, :] = [[-np.inf, -np.inf], [-np.inf, 1.0]]
        if H > 2:
            win[0, H // 2 - 1, :, W // 2 - 1, :] = [[2.0, np.nan], [3.0, 3.0]]      # the very last window of plane 0
        d = dict(x=x)
        if e == "maxpool_bwd":
            d["gy"] = f(P, H // 2, W // 2)
    for a in d.values():
        if a is not None:
            a.setflags(write=False)
    return d


def windows(x):
    """a, b, c, d of every 2 x 2 window (a b / c d)."""
    return x[:, 0::2, 0::2], x[:, 0::2, 1::2], x[:, 1::2, 0::2], x[:, 1::2, 1::2]


def avg(x):
    a, b, c, d = windows(x)
    return ((((F32(0.0) + a) + b) + c) + d) / F32(4.0)


def winner(x):
    """(value, index 0..3) of every window by the kernel's rule: `if (v > best || v != v) best = v`, in order."""
    a, b, c, d = windows(x)
    m, k = a.copy(), np.zeros(a.shape, np.int8)
    with np.errstate(invalid="ignore"):
        for i, v in ((1, b), (2, c), (3, d)):
            beats = (v > m) | (v != v)
            m, k = np.where(beats, v, m), np.where(beats, np.int8(i), k)
    return m, k


@functools.lru_cache(maxsize=None)
def expected(name):
    """dict of output name -> tuple of float32 candidates (one, but for gx of split_bwd: two)."""
    c, d = CASE[name], inputs(name)
    e, x = c["entry"], d["x"]
    with np.errstate(invalid="ignore"):
        if e == "split_fwd":
            relu = np.where(x > 0, x, np.where(x != x, x, F32(0.0))).astype(F32)
            return dict(relu_out=(relu,), pool_out=(avg(x),))
        if e == "split_bwd":
            ga = d["g_relu"] if c["g_relu"] else np.zeros_like(x)
            gate = np.where(x <= 0, F32(0.0), ga).astype(F32)           # torch: x <= 0 ? 0 : g — a NaN passes
            gb = d["g_pool"] if c["g_pool"] else None
            q = np.zeros_like(x) if gb is None else np.repeat(np.repeat(gb / F32(4.0), 2, 1), 2, 2)
            two = (gate + q).astype(F32)
            fma = two if gb is None else (gate.astype(np.float64) +
                                          np.repeat(np.repeat(gb.astype(np.float64) * 0.25, 2, 1), 2, 2)).astype(F32)
            return dict(gx=(two, fma))
        if e == "pyramid":
            out, cur = {}, x
            for l in range(c["levels"]):
                cur = avg(cur)
                out[f"level{l}"] = (cur,)
            return out
        m, k = winner(x)
        if e == "maxpool_fwd":
            return dict(y=(m.astype(F32),))
        gx = np.zeros_like(x)
        for i, (dy, dx) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
            gx[:, dy::2, dx::2] = np.where(k == i, d["gy"], F32(0.0))
        return dict(gx=(gx,))
