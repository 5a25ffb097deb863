"""Case table of tests/test_rowops_cases_cpu.py and tests/test_gpu_rowops_paths.py: g2s_rows_dot_scale, g2s_demod_fwd /
_bwd / _bwd_add, g2s_demod_fwd_multi / _bwd_multi and g2s_channel_sum (csrc/rowops.hip), called through the C ABI so that
the test controls the alignment of every pointer.  Importable without a GPU.  (g2s_synth_bwd_rows(_ps) has float64
tests of its own.)

A case is a dict: name, entry and the entry's parameters; `mis` names the pointers handed in one float past 16-byte
alignment.  `dispatch` restates the launcher's decision; the CPU test holds it against what the case is listed for.

  rds     g2s_rows_dot_scale on rows x n: dot[r] = (sum_i a * b) / inv[r], out = b * s[r].  One wavefront per row.
          `aligned = !(b & 15) && (!a || !(a & 15)) && (!out || !(out & 15))`: with aligned bases a scalar head of
          (4 - row * n % 4) % 4 elements (clipped to n), a float4 body, a scalar tail ("head/body/tail"); otherwise the
          whole row is the head ("scalar").  a / dot NULL (scale only), out NULL (dot only), out == b, s NULL, inv NULL.
  demod   g2s_demod_fwd / _bwd / _bwd_add on (B, Cin, Cout): demod[b, o] = 1 / sqrt(sum_i wsq[o, i] s[b, i]^2 + eps),
          g[b, i] = -s[b, i] sum_o gd[b, o] demod[b, o]^3 wsq[o, i]  (+ gs_add, separate or in place).
  multi   g2s_demod_fwd_multi / _bwd_multi: one call, B = 3, layers (Cin, Cout) = (5, 3), (130, 7), (70, 9): the grid
          is sized by maxima that every layer undercuts somewhere.  gs is pre-filled: the entry adds in place.
  csum    g2s_channel_sum on (B, C, n): out[c] = sum_{b, i} g[b, c, i], one workgroup of 256 lanes per channel.

Expected values.  out = b * s: numpy float32, bit for bit (one rounding, nothing to contract).  Every sum: the float64
evaluation of the same terms from the float32 inputs, within (k + 2) * 2^-24 * sum|term| per output element, k = the
number of additions on the longest chain of that kernel, counted from the code (`chain` below):
  rds dot     head/body/tail: 1 (head: at most 3 elements, one per lane) + 4 * ceil(n4 / 64) (per float4 of a lane: three
              additions inside `av.x * bv.x + ... + av.w * bv.w`, one onto acc) + 1 (tail) + 6 (the butterfly of
              wave_sum); scalar: ceil(n / 64) + 6.  The bound is divided by |inv[r]|.
  demod fwd   ceil(Cin / 64) (lane-strided loop) + 6 (wave_sum) + 1 (+ eps); eps is one of the terms.  The bound on acc
              goes through d/dacc (acc + eps)^-1/2 = -(acc + eps)^-3/2 / 2, evaluated at the low end of acc's interval
              (the function is convex), plus 2 ulp (2 * 2^-23 * demod) for sqrtf and the division.
  demod bwd   ceil(Cout / 4) (a wave's loop over o) + 3 (the four-way LDS join); + 1 with gs_add / in the multi entry,
              where gs_add (the pre-filled gs) is one of the terms.
  csum        ceil(B * n / 256) (lane-strided loop) + 6 (wave_sum) + 3 (the four-way LDS join).

Measured on an MI355X (largest error / bound over all cases): rds dot 0.195, demod fwd 0.179, demod bwd 0.329,
multi fwd 0.155, multi bwd 0.118, csum 0.048.
"""
import functools
import zlib

import numpy as np

U = 2.0 ** -24
EPS = 1e-8
MAX_LAYERS = 24            # G2S_DEMOD_MAX_LAYERS (include/g2s.h)
MULTI_B, MULTI_LAYERS = 3, ((5, 3), (130, 7), (70, 9))
F32 = np.float32

CASES = []


def _add(name, entry, **kw):
    CASES.append(dict(name=name, entry=entry, mis=kw.pop("mis", ()), **kw))


def _rds(name, shape, kernel, turns, a=True, dot=True, out="sep", s=True, inv=True, mis=()):
    _add(name, "rds", shape=shape, kernel=kernel, turns=turns, a=a, dot=dot, out=out, s=s, inv=inv, mis=mis)


HBT, SC = "head/body/tail", "scalar"
_rds("rds_5x7_full", (5, 7), HBT, 1)
_rds("rds_5x7_scale_only", (5, 7), HBT, 1, a=False, dot=False, inv=False)
_rds("rds_5x7_dot_only", (5, 7), HBT, 1, out=None, s=False)
_rds("rds_5x7_inplace", (5, 7), HBT, 1, out="b")
_rds("rds_5x7_no_s", (5, 7), HBT, 1, s=False)
_rds("rds_5x7_no_inv", (5, 7), HBT, 1, inv=False)
for _m in ("a", "b", "out"):
    _rds(f"rds_5x7_mis_{_m}", (5, 7), SC, 1, mis=(_m,))
_rds("rds_5x7_mis_inplace", (5, 7), SC, 1, out="b", mis=("b",))
_rds("rds_6x3_full", (6, 3), HBT, 0)
_rds("rds_6x3_mis_a", (6, 3), SC, 1, mis=("a",))
_rds("rds_3x1_full", (3, 1), HBT, 0)
_rds("rds_3x1_scale_only", (3, 1), HBT, 0, a=False, dot=False, inv=False)
_rds("rds_2x264_full", (2, 264), HBT, 2)
_rds("rds_2x264_inplace", (2, 264), HBT, 2, out="b")
_rds("rds_2x264_mis_b", (2, 264), SC, 5, mis=("b",))
_rds("rds_3x1031_full", (3, 1031), HBT, 5)
_rds("rds_3x1031_dot_only", (3, 1031), HBT, 5, out=None, s=False, inv=False)
_rds("rds_3x1031_inplace", (3, 1031), HBT, 5, out="b")
_rds("rds_3x1031_mis_out", (3, 1031), SC, 17, mis=("out",))

DEMOD_SHAPES = ((2, 5, 3), (3, 70, 9), (1, 64, 4), (2, 130, 7))
for _s in DEMOD_SHAPES + ("tiny",):
    _shape, _tiny = ((2, 70, 9), True) if _s == "tiny" else (_s, False)
    _t = "tiny" if _tiny else "x".join(map(str, _shape))
    _add(f"demod_fwd_{_t}", "demod_fwd", shape=_shape, tiny=_tiny)
    _add(f"demod_bwd_{_t}", "demod_bwd", shape=_shape, tiny=_tiny, add=None)
    _add(f"demod_bwd_add_{_t}", "demod_bwd", shape=_shape, tiny=_tiny, add="sep")
    _add(f"demod_bwd_inplace_{_t}", "demod_bwd", shape=_shape, tiny=_tiny, add="gs")
_add("multi_fwd", "multi_fwd")
_add("multi_bwd", "multi_bwd")
for _shape in ((1, 3, 1), (2, 5, 9), (3, 2, 100), (4, 7, 64)):
    _add("csum_" + "x".join(map(str, _shape)), "csum", shape=_shape)

NAMES = [c["name"] for c in CASES]
CASE = {c["name"]: c for c in CASES}
assert len(CASE) == len(CASES)


def _cdiv(a, b):
    return -(-a // b)


def rds_rows(c):
    """(head, n4, tail) per row, as rows_dot_scale splits it:
    `head = aligned_bases ? (4 - (off & 3)) & 3 : n; if (head > n) head = n; n4 = (n - head) >> 2; tail0 = head + 4 * n4`"""
    rows, n = c["shape"]
    aligned = not (set(c["mis"]) & ({"b"} | ({"a"} if c["a"] else set()) | ({"out"} if c["out"] else set())))
    out = []
    for r in range(rows):
        head = min((4 - (r * n) % 4) % 4 if aligned else n, n)
        n4 = (n - head) >> 2
        out.append((head, n4, n - head - 4 * n4))
    return aligned, out


def dispatch(c):
    """rds: (kernel, lane turns of the longest loop: of the float4 body, or of the all-scalar head); demod / multi /
    csum: the grid and what it leaves idle."""
    e = c["entry"]
    if e == "rds":
        aligned, rows = rds_rows(c)
        if aligned:
            return HBT, max(_cdiv(n4, 64) for _, n4, _ in rows)
        return SC, max(_cdiv(h, 64) for h, _, _ in rows)
    if e == "demod_fwd":
        B, Cin, Cout = c["shape"]      # `demod_fwd<<<cdiv(B * Cout, 4), 256>>>`: one wave per (b, o)
        return dict(grid=_cdiv(B * Cout, 4), idle_waves=4 * _cdiv(B * Cout, 4) - B * Cout, trips=_cdiv(Cin, 64))
    if e == "demod_bwd":
        B, Cin, Cout = c["shape"]      # `demod_bwd<<<dim3(cdiv(Cin, 64), B), 256>>>`: waves split o, lanes run along i
        return dict(grid=(_cdiv(Cin, 64), B), wave_outputs=tuple(len(range(w, Cout, 4)) for w in range(4)),
                    idle_lanes=64 * _cdiv(Cin, 64) - Cin)
    if e == "multi_fwd":               # `dim3(cdiv(B * max Cout, 4), layers)`; `if (idx >= d.B * d.Cout[l]) return`
        gx = _cdiv(MULTI_B * max(o for _, o in MULTI_LAYERS), 4)
        return dict(grid=(gx, len(MULTI_LAYERS)), idle_waves=tuple(4 * gx - MULTI_B * o for _, o in MULTI_LAYERS))
    if e == "multi_bwd":               # `dim3(cdiv(max Cin, 64), B, layers)`; `if (blockIdx.x * 64 >= d.Cin[l]) return`
        gx = _cdiv(max(i for i, _ in MULTI_LAYERS), 64)
        return dict(grid=(gx, MULTI_B, len(MULTI_LAYERS)), idle_blocks=tuple(gx - _cdiv(i, 64) for i, _ in MULTI_LAYERS))
    B, C, n = c["shape"]               # `channel_sum<<<C, 256>>>`: `for (i = threadIdx.x; i < B * n; i += 256)`
    return dict(grid=C, trips=_cdiv(B * n, 256), idle_lanes=max(0, 256 - B * n))


def chain(c, layer=None):
    """k: the additions on the longest chain (module docstring)."""
    e = c["entry"]
    if e == "rds":
        aligned, rows = rds_rows(c)
        if not aligned:
            return _cdiv(c["shape"][1], 64) + 6
        return max((1 if h else 0) + 4 * _cdiv(n4, 64) + (1 if t else 0) for h, n4, t in rows) + 6
    if e in ("demod_fwd", "multi_fwd"):
        cin = c["shape"][1] if layer is None else MULTI_LAYERS[layer][0]
        return _cdiv(cin, 64) + 6 + 1
    if e in ("demod_bwd", "multi_bwd"):
        cout = c["shape"][2] if layer is None else MULTI_LAYERS[layer][1]
        return _cdiv(cout, 4) + 3 + (1 if (layer is not None or c["add"]) else 0)
    B, C, n = c["shape"]
    return _cdiv(B * n, 256) + 6 + 3


def _demod_inputs(rng, B, Cin, Cout, tiny=False):
    f = lambda *s: rng.standard_normal(s).astype(F32)
    sc = F32(1e-6) if tiny else F32(1.0)
    wsq = ((0.05 + rng.random((Cout, Cin))) * sc).astype(F32)             # positive
    s = ((1.0 + 0.3 * f(B, Cin)) * sc).astype(F32)                         # around 1
    acc = (wsq.astype(np.float64)[None] * s.astype(np.float64)[:, None] ** 2).sum(2) + float(F32(EPS))
    return dict(wsq=wsq, s=s, demod=(1.0 / np.sqrt(acc)).astype(F32), gd=f(B, Cout), gs_add=f(B, Cin))


@functools.lru_cache(maxsize=None)
def inputs(name):
    """The float32 inputs of a case, read-only; an absent tensor is None."""
    c = CASE[name]
    rng = np.random.default_rng([20262, zlib.crc32(name.encode())])
    f = lambda *s: rng.standard_normal(s).astype(F32)
    e = c["entry"]
    if e == "rds":
        rows, n = c["shape"]
        d = dict(a=f(rows, n) if c["a"] else None, b=f(rows, n), s=f(rows) if c["s"] else None,
                 inv=(0.5 + rng.random(rows)).astype(F32) * F32(-1 if rows > 3 else 1) if c["inv"] else None)
    elif e in ("demod_fwd", "demod_bwd"):
        d = _demod_inputs(rng, *c["shape"], tiny=c["tiny"])
    elif e in ("multi_fwd", "multi_bwd"):
        d = {}
        for l, (cin, cout) in enumerate(MULTI_LAYERS):
            d.update({f"{k}{l}": v for k, v in _demod_inputs(rng, MULTI_B, cin, cout).items()})
    else:
        d = dict(g=f(*c["shape"]))
    for a in d.values():
        if a is not None:
            a.setflags(write=False)
    return d


def _demod_fwd64(wsq, s, k):
    """(demod, bound) in float64."""
    eps = float(F32(EPS))
    t = wsq.astype(np.float64)[None] * s.astype(np.float64)[:, None] ** 2          # [B, Cout, Cin]
    acc = t.sum(2) + eps
    b_acc = (k + 2) * U * (np.abs(t).sum(2) + eps)
    low = acc - b_acc
    assert (low > 0).all()
    val = 1.0 / np.sqrt(acc)
    return val, 0.5 * low ** -1.5 * b_acc + 2 * 2.0 ** -23 * val


def _demod_bwd64(wsq, s, demod, gd, add, k):
    """(gs, bound) in float64: -s[b, i] sum_o gd demod^3 wsq[o, i] (+ add)."""
    t = (gd.astype(np.float64) * demod.astype(np.float64) ** 3)[:, :, None] * wsq.astype(np.float64)[None]   # [B, Cout, Cin]
    t = -s.astype(np.float64)[:, None, :] * t
    val, mag = t.sum(1), np.abs(t).sum(1)
    if add is not None:
        val, mag = val + add.astype(np.float64), mag + np.abs(add.astype(np.float64))
    return val, (k + 2) * U * mag


@functools.lru_cache(maxsize=None)
def expected(name):
    """dict of output name -> (float64 value, bound per element); "out" -> (float32 array, None): bit for bit."""
    c, d = CASE[name], inputs(name)
    e = c["entry"]
    if e == "rds":
        r = {}
        if c["out"]:
            r["out"] = ((d["b"] * (d["s"][:, None] if c["s"] else F32(1.0))).astype(F32), None)
        if c["dot"]:
            t = d["a"].astype(np.float64) * d["b"].astype(np.float64)
            inv = d["inv"].astype(np.float64) if c["inv"] else 1.0
            r["dot"] = (t.sum(1) / inv, (chain(c) + 2) * U * np.abs(t).sum(1) / np.abs(inv))
        return r
    if e == "demod_fwd":
        return dict(demod=_demod_fwd64(d["wsq"], d["s"], chain(c)))
    if e == "demod_bwd":
        return dict(gs=_demod_bwd64(d["wsq"], d["s"], d["demod"], d["gd"], d["gs_add"] if c["add"] else None, chain(c)))
    if e == "multi_fwd":
        return {f"demod{l}": _demod_fwd64(d[f"wsq{l}"], d[f"s{l}"], chain(c, l)) for l in range(len(MULTI_LAYERS))}
    if e == "multi_bwd":
        return {f"gs{l}": _demod_bwd64(d[f"wsq{l}"], d[f"s{l}"], d[f"demod{l}"], d[f"gd{l}"], d[f"gs_add{l}"], chain(c, l))
                for l in range(len(MULTI_LAYERS))}
    g = d["g"].astype(np.float64)
    return dict(out=(g.sum((0, 2)), (chain(c) + 2) * U * np.abs(g).sum((0, 2))))


def _wave32(t, lanes=64):
    """Float32 sum over the last axis the way a wavefront takes it: lane l adds elements l, l + 64, ... in turn, then
    the butterfly of wave_sum.  lanes = 256: four such waves, joined as red[0] + red[1] + red[2] + red[3]."""
    n = t.shape[-1]
    pad = np.zeros(t.shape[:-1] + (-(-n // lanes) * lanes,), F32)
    pad[..., :n] = t
    acc = np.zeros(t.shape[:-1] + (lanes,), F32)
    for trip in range(pad.shape[-1] // lanes):
        acc = acc + pad[..., trip * lanes:(trip + 1) * lanes]
    acc = acc.reshape(t.shape[:-1] + (lanes // 64, 64))
    o = 32
    while o:
        acc = acc + acc[..., np.arange(64) ^ o]
        o >>= 1
    red = acc[..., 0]
    out = red[..., 0]
    for w in range(1, lanes // 64):
        out = out + red[..., w]
    assert out.dtype == F32
    return out


def emulate32(name):
    """The sums in float32 in the kernels' order (rows_dot_scale: in the order of its all-scalar kernel), for the CPU
    test.  dict of output name -> float32 array."""
    c, d = CASE[name], inputs(name)
    e = c["entry"]

    def fwd(wsq, s):
        return (F32(1.0) / np.sqrt(_wave32(wsq[None] * s[:, None] * s[:, None]) + F32(EPS))).astype(F32)

    def bwd(wsq, s, demod, gd, add):
        t = (gd * demod * demod * demod)[:, :, None] * wsq[None]             # [B, Cout, Cin]
        red = []
        for w in range(4):
            acc = np.zeros((t.shape[0], t.shape[2]), F32)
            for o in range(w, t.shape[1], 4):
                acc = acc + t[:, o]
            red.append(acc)
        g = -s * (((red[0] + red[1]) + red[2]) + red[3])
        return (g if add is None else add + g).astype(F32)

    if e == "rds":
        if not c["dot"]:
            return {}
        acc = _wave32(d["a"] * d["b"])
        return dict(dot=(acc / d["inv"] if c["inv"] else acc).astype(F32))
    if e == "demod_fwd":
        return dict(demod=fwd(d["wsq"], d["s"]))
    if e == "demod_bwd":
        return dict(gs=bwd(d["wsq"], d["s"], d["demod"], d["gd"], d["gs_add"] if c["add"] else None))
    if e == "multi_fwd":
        return {f"demod{l}": fwd(d[f"wsq{l}"], d[f"s{l}"]) for l in range(len(MULTI_LAYERS))}
    if e == "multi_bwd":
        return {f"gs{l}": bwd(d[f"wsq{l}"], d[f"s{l}"], d[f"demod{l}"], d[f"gd{l}"], d[f"gs_add{l}"])
                for l in range(len(MULTI_LAYERS))}
    g = d["g"]
    return dict(out=_wave32(np.ascontiguousarray(g.transpose(1, 0, 2)).reshape(g.shape[1], -1), 256))
