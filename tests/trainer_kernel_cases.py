"""Case table and float64 restatement of the small kernels of GAN training, called through the C ABI: the minibatch
stddev with its backward and double backward, the logistic head and the R1 penalty (csrc/dtrain.hip), the path-length
penalty, the non-saturating head and the parameter EMA (csrc/gtrain.hip).  Shared by
tests/test_trainer_kernel_cases_cpu.py and tests/test_gpu_trainer_kernel_paths.py; importable without a GPU.

A case is a dict: name, entry ("mbstd", "d_logistic", "g_nonsaturating", "r1", "path", "ema"), its shape, the
pointers it passes as NULL, and `data`: the key its inputs are drawn from (the NULL variants of a shape share inputs
and reference).  `inputs(name)` gives read-only float32 arrays, `expected(name)` the float64 reference, the float32
restatement, e32 and the bound of every output, `dispatch(case)` the paths the launch takes.

The restatement.  float64: dtrain_cases.mbstd / d_logistic / r1_per_sample and gtrain_cases.path_penalty /
g_nonsaturating, autograd for every backward (the stddev's double backward included).  float32: the same lines with
every reduction, in the forward and in the backward of a broadcast, as ONE sequential fp32 accumulation
(reduce_cases._seq; `Ops` here differs from reduce_cases.Ops only in that its two primitives are each other's
backward, so that the stddev can be differentiated twice).  e32 = max|f32 - f64| per output tensor.
  * The path penalty is stated with a `where` on both sides of the sqrt, so that a row of zeros has length 0 and
    gradient 0, the kernel's coef = 0 (gtrain_cases.path_penalty gives NaN there); where every length is positive the
    float64 value is gtrain_cases.path_penalty's.
  * sign(0) = sign(-0) = 0 in out[3] of the logistic head.
  * The scalars a kernel receives as float (decay, one_minus_decay) enter the reference as those float32 values.

Inputs.  Stddev: x = 0.25 randn + pattern[g], pattern = (+1, -1, +1, -1)[:G] over the members of a group; the case
takes the first seed of SEEDS for which the float64 s >= MIN_S at every element (d / s and 1 / s^3 well conditioned,
nothing masked out).  G = 1: s = sqrt(eps) everywhere, plain randn.  Exact stddev cases: dyadic x, the members of a
group equal, so d = 0 exactly; E <= 64, so that the sum of E equal values is one wave's butterfly and exact.  Heads:
3 randn with +-40, +-100, 0.0 and -0.0 planted (B = 1: 40 alone; B = 3: 40, -40 and a zero).  R1 and path: randn, one
dyadic R1 case whose every partial sum is an fp32 number.

Bounds; none is measured against the code under test.
  * exact outputs: equality with float64.
  * stddev, R1 and path outputs: max|kernel - f64| <= 4 e32 + 5e-6 max|f64| per output tensor (reduce_cases,
    raster_cases: the kernels do the arithmetic of the float32 restatement in a tree order).  The copies inside the
    stddev's out and ggout are compared bit for bit and are no part of `out.map` / `ggout.map`.
  * heads (tests/test_gpu_dtrain.py::test_loss_heads): a mean of B terms in float32 is within (B + 4) eps32 x its
    largest term; the loss of the logistic head is the sum of two such means.  A gradient sigmoid / B is within
    4 eps32 / B (exp, add, two divisions) plus one float32 subnormal: sigmoid(-100) = 3.7e-44 may flush to zero.
  * EMA (tests/test_gpu_gtrain.py::test_ema_accumulate_kernel): two products and a sum, 3 eps32 (|dst| |decay| +
    |src| |rest|) elementwise.

MEASURED: the largest error / bound per entry on an MI355X; a record, not a bound.
"""
import functools
import zlib

import numpy as np
import torch
import torch.nn.functional as F

import dtrain_cases as dc
import gtrain_cases as gc
import reduce_cases as rc
from reduce_cases import F32, F64, SEEDS

MEASURED = {
    "date": "2026-10-21", "commit": "3f5068e",       # the kernels of that commit, unchanged by these tests
    "mbstd_fwd": 0.106, "mbstd_bwd": 0.010, "mbstd_bwd2": 0.396, "d_logistic": 0.218, "r1_penalty": 0.063,
    "path_penalty": 0.097, "g_nonsaturating": 0.222, "ema_accumulate": 0.328,
}

# launch constants of csrc/dtrain.hip and csrc/gtrain.hip, restated
MB_THREADS, MB_MAXG, MB_EPS = 1024, 4, 1e-8
LH_THREADS, R1_CHUNK = 256, 4096
GH_THREADS, GH_MAXB = 1024, 1024
EM_THREADS, EM_CHUNK = 256, 8192

EPS32 = float(np.finfo(np.float32).eps)
TINY32 = float(np.finfo(np.float32).tiny)          # below it a float32 is subnormal and may be flushed
MIN_S = 0.25
PATTERN = (1.0, -1.0, 1.0, -1.0)
MEAN_PATH = 0.7
EMA_GUARD = 5                                      # canary floats before, between and after the tensors of a table
EMA_CANARY = 1024.0


def f32(v):
    return float(np.float32(v))


# ------------------------------------------------------------------------------- sequential fp32 reductions
class _Sum(torch.autograd.Function):
    """keepdim sum over `dims`, one sequential accumulation in x's dtype; its backward is _Rep."""

    @staticmethod
    def forward(ctx, x, dims):
        ctx.shape = x.shape
        return rc._seq(x, dims, keepdim=True)

    @staticmethod
    def backward(ctx, g):
        return _Rep.apply(g, ctx.shape), None


class _Rep(torch.autograd.Function):
    """expand to `shape`; its backward is _Sum over the repeated dims."""

    @staticmethod
    def forward(ctx, x, shape):
        ctx.dims = tuple(d for d in range(x.dim()) if x.shape[d] == 1 and shape[d] != 1)
        return x.expand(shape).clone()

    @staticmethod
    def backward(ctx, g):
        return (_Sum.apply(g, ctx.dims) if ctx.dims else g), None


class Ops:
    """The dtype of a restatement run and its two reduction primitives (both keep the number of dims)."""

    def __init__(self, dtype):
        self.dt, self.seq = dtype, dtype == F32

    def t(self, a, grad=False):
        return torch.tensor(np.asarray(a), dtype=self.dt).requires_grad_(grad)

    def sum(self, x, dims):
        return _Sum.apply(x, tuple(dims)) if self.seq else x.sum(tuple(dims), keepdim=True)

    def rep(self, x, shape):
        return _Rep.apply(x, tuple(shape)) if self.seq else x.expand(tuple(shape))


# ------------------------------------------------------------------------------------------- the statements
def mbstd(o, x, feat):
    """dtrain_cases.mbstd with its reductions through `o`: [B, C, H, W] -> [B, C + feat, H, W]."""
    B, C, H, W = x.shape
    G = min(B, MB_MAXG)
    M, c = B // G, C // feat
    s = x.view(G, M, feat, c, H, W)
    d = s - o.rep(o.sum(s, (0,)) / G, s.shape)
    sd = torch.sqrt(o.sum(d * d, (0,)) / G + MB_EPS)
    f = o.sum(sd, (3, 4, 5)) / (c * H * W)
    fmap = o.rep(f.view(1, M, feat, 1, 1), (G, M, feat, H, W)).reshape(B, feat, H, W)
    return torch.cat([x, fmap], 1)


def mbstd_s64(x, feat):
    """The float64 s of every element: [M, feat, C / feat, H, W]."""
    B, C, H, W = x.shape
    s = torch.tensor(np.asarray(x), dtype=F64).view(min(B, MB_MAXG), -1, feat, C // feat, H, W)
    return torch.sqrt(s.var(0, unbiased=False) + MB_EPS)


def d_logistic(o, real, fake):
    """dtrain_cases.d_logistic on [B] scores."""
    return (o.sum(F.softplus(-real), (0,)) / real.numel() + o.sum(F.softplus(fake), (0,)) / fake.numel()).view(())


def g_nonsaturating(o, fake):
    return (o.sum(F.softplus(-fake), (0,)) / fake.numel()).view(())


def mean_of(o, v):
    return (o.sum(v, (0,)) / v.numel()).view(())


def r1(o, grad):
    """dtrain_cases.r1_per_sample on [B, n] and its mean over the batch."""
    per = o.sum(grad * grad, (1,)).view(-1)
    return per, mean_of(o, per)


def path_penalty(o, grad, mean_path, decay):
    """gtrain_cases.path_penalty on [B, L, D] with a row of zeros at length 0 and gradient 0.
    -> penalty, path mean, lengths, mean length."""
    B, L, _ = grad.shape
    ms = o.sum(grad * grad, (1, 2)).view(B) / L
    pos = ms > 0
    lengths = torch.where(pos, torch.sqrt(torch.where(pos, ms, torch.ones_like(ms))), torch.zeros_like(ms))
    mean = mean_of(o, lengths)
    pm = mean_path + decay * (mean - mean_path)
    dev = lengths - o.rep(pm.view(1), (B,))
    return mean_of(o, dev * dev), pm, lengths, mean


# ---------------------------------------------------------------------------------------------- the table
CASES = []


def _add(name, entry, data=None, **kw):
    CASES.append(dict(dict(name=name, entry=entry, data=data or name, exact=False), **kw))


MBSTD_SHAPES = [(1, 4, 3, 5, 1), (2, 4, 4, 4, 2), (3, 6, 4, 4, 3), (4, 8, 4, 4, 8), (8, 64, 4, 4, 1), (12, 5, 15, 15, 1),
                (4, 2, 17, 17, 2), (4, 3, 1, 1, 1)]
MBSTD_EXACT = [(1, 4, 4, 4, 1), (2, 4, 4, 4, 2), (8, 8, 4, 4, 2)]          # G = 1, 2, 4; E = 64, 32, 64
for _s in MBSTD_SHAPES:
    _add("mbstd_%dx%dx%dx%d_f%d" % _s, "mbstd", shape=_s)
for _s in MBSTD_EXACT:
    _add("mbstd_exact_%dx%dx%dx%d_f%d" % _s, "mbstd", shape=_s, exact=True)

HEAD_NULLS = [(), ("g_real",), ("g_fake",), ("g_real", "g_fake")]
D_LOGISTIC_SHAPES = [(1, 1), (3, 260), (256, 255), (257, 600)]
for _s in D_LOGISTIC_SHAPES:
    for _n in HEAD_NULLS:
        _add("d_logistic_%dx%d" % _s + "".join("_no_" + k for k in _n), "d_logistic", "d_logistic_%dx%d" % _s, shape=_s, null=_n)
G_NONSAT_B = [1, 256, 257, 600]
for _b in G_NONSAT_B:
    for _n in ((), ("g_fake",)):
        _add(f"g_nonsaturating_{_b}" + "".join("_no_" + k for k in _n), "g_nonsaturating", f"g_nonsaturating_{_b}", shape=(_b,), null=_n)

R1_SHAPES = [(1, 1), (3, 255), (2, 4096), (2, 4097), (3, 8229), (257, 5), (300, 4100)]
R1_CHUNKS_OF = {-1: 0, 0: 0, 1: 1, 4096: 1, 4097: 2}
for _s in R1_SHAPES:
    for _n in ((), ("mean",)):
        _add("r1_%dx%d" % _s + "".join("_no_" + k for k in _n), "r1", "r1_%dx%d" % _s, shape=_s, null=_n)
_add("r1_dyadic_4x4100", "r1", shape=(4, 4100), null=(), exact=True)

PATH_SHAPES = [(1, 1, 1), (2, 3, 341), (2, 1, 1024), (3, 5, 205), (1024, 1, 3), (5, 14, 512)]
PATH_DECAYS = (0.0, 0.01)
for _s in PATH_SHAPES:
    for _dec in PATH_DECAYS:
        for _n in ((), ("dgrad",)):
            _add("path_%dx%dx%d" % _s + f"_decay{_dec}" + "".join("_no_" + k for k in _n), "path",
                 "path_%dx%dx%d" % _s + f"_decay{_dec}", shape=_s, decay=_dec, null=_n, zero="none")
_add("path_zero_row_3x5x205", "path", shape=(3, 5, 205), decay=0.01, null=(), zero="row1")
_add("path_all_zero_2x3x341", "path", shape=(2, 3, 341), decay=0.01, null=(), zero="all")

EMA_SIZES = (1, 3, 8191, 8192, 8193, 16384 + 5)
EMA_MIXED = (1, 3, 1, 8193, 17, 1, 8192, 255, 16384 + 5, 1, 8191, 4)
EMA_REST = f32(1 - 0.999)
ALIGNMENTS = {"both": (True, True), "dst_only": (True, False), "src_only": (False, True), "neither": (False, False)}
for _k, _a in ALIGNMENTS.items():
    _add(f"ema_sizes_{_k}", "ema", sizes=EMA_SIZES, aligned=(_a,) * len(EMA_SIZES), decay=0.999, rest=EMA_REST)
_MIX37 = tuple(EMA_MIXED[i % len(EMA_MIXED)] for i in range(37))
_AL37 = tuple(list(ALIGNMENTS.values())[(i + i // 4) % 4] for i in range(37))
_add("ema_table37", "ema", sizes=_MIX37, aligned=_AL37, decay=0.999, rest=EMA_REST)
_AL6 = tuple(list(ALIGNMENTS.values())[i % 4] for i in range(len(EMA_SIZES)))
_add("ema_keep", "ema", sizes=EMA_SIZES, aligned=_AL6, decay=1.0, rest=0.0, exact=True)
_add("ema_copy", "ema", sizes=EMA_SIZES, aligned=_AL6, decay=0.0, rest=1.0, exact=True)
_add("ema_rest_0.25", "ema", sizes=EMA_SIZES, aligned=_AL6, decay=0.999, rest=0.25)

NAMES = [c["name"] for c in CASES]
CASE = {c["name"]: c for c in CASES}
assert len(CASE) == len(CASES)


def by_entry(entry):
    return [c for c in CASES if c["entry"] == entry]


# ----------------------------------------------------------------------------------------------- dispatch
def _trips(n, stride):
    return -(-n // stride)


def ema_layout(c):
    """[(dst offset, src offset, n)] in floats inside two 16-byte aligned buffers, and the buffers' lengths: tensors in
    table order with EMA_GUARD floats or more between them; an aligned tensor starts on a multiple of four floats, a
    misaligned one 1, 2 or 3 floats past one (in turn)."""
    rows, at, turn = [], [EMA_GUARD, EMA_GUARD], 0
    for n, al in zip(c["sizes"], c["aligned"]):
        off = []
        for k in (0, 1):
            want = 0 if al[k] else 1 + turn % 3
            turn += not al[k]
            at[k] += (want - at[k]) % 4
            off.append(at[k])
            at[k] += n + EMA_GUARD
        rows.append((off[0], off[1], n))
    return rows, at[0], at[1]


def ema_prefix(sizes):
    """The int32 chunk prefix of gtrain._ema_table."""
    prefix = np.zeros(len(sizes) + 1, dtype=np.int32)
    prefix[1:] = np.cumsum([(n + EM_CHUNK - 1) // EM_CHUNK for n in sizes])
    return prefix


def _ema_depth(prefix, n_tensors, block):
    """(tensor, iterations of the bisection) of one block: the kernel's loop."""
    lo, hi, depth = 0, n_tensors, 0
    while hi - lo > 1:
        mid = (lo + hi) >> 1
        if prefix[mid] <= block:
            lo = mid
        else:
            hi = mid
        depth += 1
    return lo, depth


def dispatch(c):
    """The paths a case's launch takes, as a set of names (PATHS lists the ones the table has to reach)."""
    e, p = c["entry"], set()
    if e == "mbstd":
        B, C, H, W, feat = c["shape"]
        G = min(B, MB_MAXG)
        M, HW, E = B // G, H * W, (C // feat) * H * W
        p |= {f"mbstd:G={G}", f"mbstd:M={M}", f"mbstd:E trips={_trips(E, MB_THREADS)}", f"mbstd:map trips={_trips(G * HW, MB_THREADS)}"}
        p |= {"mbstd:E ragged"} if E % MB_THREADS else {"mbstd:E full"}
        p |= {"mbstd:E<64"} if E < 64 else set()
        p |= {"mbstd:H!=W"} if H != W else set()
        p |= {"mbstd:HW=1"} if HW == 1 else set()
        p |= {"mbstd:one channel per block"} if C == feat and feat > 1 else set()
        p |= {"mbstd:F>1"} if feat > 1 else set()
    elif e in ("d_logistic", "g_nonsaturating"):
        for who, n in zip(("real", "fake") if e == "d_logistic" else ("fake",), c["shape"]):
            p |= {f"{e}:{who} trips={_trips(n, LH_THREADS)}", f"{e}:{who} " + ("ragged" if n % LH_THREADS else "full")}
        if e == "d_logistic" and c["shape"][0] != c["shape"][1]:
            p.add("d_logistic:Br!=Bf")
        p |= {f"{e}:{k} NULL" for k in c["null"]} or {f"{e}:all gradients"}
    elif e == "r1":
        B, n = c["shape"]
        chunks = _trips(n, R1_CHUNK)
        last = n - (chunks - 1) * R1_CHUNK
        p |= {f"r1:chunks={min(chunks, 3)}" + ("+" if chunks >= 3 else ""), f"r1:chunk trips={_trips(min(n, R1_CHUNK), LH_THREADS)}",
              f"r1:finish trips={_trips(B, LH_THREADS)}", "r1:mean NULL" if "mean" in c["null"] else "r1:mean"}
        p |= {"r1:last chunk of one float"} if chunks > 1 and last == 1 else set()
        p |= {"r1:last chunk ragged"} if last % LH_THREADS else {"r1:last chunk full"}
    elif e == "path":
        B, L, D = c["shape"]
        n = L * D
        p |= {f"path:n trips={_trips(n, GH_THREADS)}", "path:n ragged" if n % GH_THREADS else "path:n full",
              f"path:decay={c['decay']}", "path:dgrad NULL" if "dgrad" in c["null"] else "path:dgrad"}
        p |= {f"path:n={n}"} if abs(n - GH_THREADS) <= 1 else set()
        p |= {"path:B=GH_MAXB"} if B == GH_MAXB else set()
        p |= {"path:zero " + c["zero"]} if c["zero"] != "none" else set()
    elif e == "ema":
        prefix = ema_prefix(c["sizes"])
        rows, _, _ = ema_layout(c)
        depth = 0
        for block in range(int(prefix[-1])):
            t, d = _ema_depth(prefix, len(c["sizes"]), block)
            assert prefix[t] <= block < prefix[t + 1]
            depth = max(depth, d)
            if block > prefix[t] and t > 0:
                p.add("ema:base>0 past the first tensor")
        p.add(f"ema:depth={depth}")
        for (do, so, n), al in zip(rows, c["aligned"]):
            assert (do % 4 == 0, so % 4 == 0) == tuple(al)
            p.add("ema:" + {(True, True): "vector", (True, False): "scalar, src misaligned", (False, True): "scalar, dst misaligned",
                            (False, False): "scalar, both misaligned"}[tuple(al)])
            if all(al) and n % 4:
                p.add("ema:vector with a scalar tail")
            if abs(n - EM_CHUNK) <= 1:
                p.add(f"ema:n=EM_CHUNK{n - EM_CHUNK:+d}" if n != EM_CHUNK else "ema:n=EM_CHUNK")
        if c["rest"] != f32(1 - c["decay"]):
            p.add("ema:rest unrelated to decay")
    return p


PATHS = {
    "mbstd:G=1", "mbstd:G=2", "mbstd:G=3", "mbstd:G=4", "mbstd:M=1", "mbstd:M=2", "mbstd:M=3", "mbstd:H!=W", "mbstd:HW=1",
    "mbstd:one channel per block", "mbstd:E<64", "mbstd:E full", "mbstd:E ragged", "mbstd:E trips=1", "mbstd:E trips=2",
    "mbstd:map trips=1", "mbstd:map trips=2", "mbstd:F>1",
    "d_logistic:real trips=1", "d_logistic:real trips=2", "d_logistic:fake trips=1", "d_logistic:fake trips=2",
    "d_logistic:fake trips=3", "d_logistic:real full", "d_logistic:real ragged", "d_logistic:fake ragged", "d_logistic:Br!=Bf",
    "d_logistic:g_real NULL", "d_logistic:g_fake NULL", "d_logistic:all gradients",
    "g_nonsaturating:fake trips=1", "g_nonsaturating:fake trips=2", "g_nonsaturating:fake trips=3", "g_nonsaturating:fake full",
    "g_nonsaturating:fake ragged", "g_nonsaturating:g_fake NULL", "g_nonsaturating:all gradients",
    "r1:chunks=1", "r1:chunks=2", "r1:chunks=3+", "r1:chunk trips=1", "r1:chunk trips=16", "r1:finish trips=1", "r1:finish trips=2",
    "r1:mean", "r1:mean NULL", "r1:last chunk of one float", "r1:last chunk ragged", "r1:last chunk full",
    "path:n trips=1", "path:n trips=2", "path:n trips=7", "path:n=1023", "path:n=1024", "path:n=1025", "path:n full", "path:n ragged",
    "path:decay=0.0", "path:decay=0.01", "path:dgrad", "path:dgrad NULL", "path:B=GH_MAXB", "path:zero row1", "path:zero all",
    "ema:vector", "ema:scalar, src misaligned", "ema:scalar, dst misaligned", "ema:scalar, both misaligned",
    "ema:vector with a scalar tail", "ema:n=EM_CHUNK-1", "ema:n=EM_CHUNK", "ema:n=EM_CHUNK+1", "ema:depth=3", "ema:depth=6",
    "ema:base>0 past the first tensor", "ema:rest unrelated to decay",
}


# ------------------------------------------------------------------------------------------------- inputs
def _rng(key, seed=0):
    return np.random.default_rng([seed, zlib.crc32(key.encode())])


PLANT_REAL = (40.0, -40.0, 0.0, 100.0, -100.0, -0.0)
PLANT_FAKE = (40.0, -40.0, -0.0, -100.0, 100.0, 0.0)


def _scores(rng, B, plant):
    """3 randn with the planted values: the first three at the front, the rest at the end (the last trip)."""
    v = (3 * rng.standard_normal(B)).astype(np.float32)
    for k, val in enumerate(plant[:B]):
        v[k if k < 3 else B - 1 - (k - 3)] = val
    return v


def _mbstd_inputs(c):
    B, C, H, W, feat = c["shape"]
    G = min(B, MB_MAXG)
    M = B // G
    for seed in SEEDS:
        rng = _rng(c["data"], seed)
        if c["exact"]:          # multiples of 1/8 in [-1, 1], the same for every member of a group
            x = np.broadcast_to(rng.integers(-8, 9, (1, M, C, H, W)) / 8.0, (G, M, C, H, W))
        elif G == 1:
            x = rng.standard_normal((G, M, C, H, W))
        else:
            x = 0.25 * rng.standard_normal((G, M, C, H, W)) + np.array(PATTERN[:G]).reshape(G, 1, 1, 1, 1)
        x = np.ascontiguousarray(x.reshape(B, C, H, W), dtype=np.float32)
        gout = rng.standard_normal((B, C + feat, H, W)).astype(np.float32)
        ggx = rng.standard_normal((B, C, H, W)).astype(np.float32)
        s_min = float(mbstd_s64(x, feat).min())
        if c["exact"] or G == 1 or s_min >= MIN_S:
            return dict(x=x, gout=gout, ggx=ggx), dict(seed=seed, s_min=s_min)
    raise AssertionError(f"{c['name']}: no seed of {SEEDS} keeps s >= {MIN_S} (last minimum {s_min}); enlarge PATTERN")


def _ema_inputs(c):
    rows, nd, ns = ema_layout(c)
    rng = _rng(c["data"])
    dst, src = np.full(nd, EMA_CANARY, np.float32), np.full(ns, EMA_CANARY, np.float32)
    for do, so, n in rows:
        dst[do:do + n] = rng.standard_normal(n)
        src[so:so + n] = rng.standard_normal(n)
    return dict(dst=dst, src=src), dict(rows=rows)


@functools.lru_cache(maxsize=None)
def _data(key):
    c = next(c for c in CASES if c["data"] == key)
    e, rng = c["entry"], _rng(key)
    info = {}
    if e == "mbstd":
        d, info = _mbstd_inputs(c)
    elif e == "d_logistic":
        d = dict(real=_scores(rng, c["shape"][0], PLANT_REAL), fake=_scores(rng, c["shape"][1], PLANT_FAKE))
    elif e == "g_nonsaturating":
        d = dict(fake=_scores(rng, c["shape"][0], PLANT_FAKE))
    elif e == "r1":
        B, n = c["shape"]
        g = rng.choice([-2.0, -1.0, -0.5, 0.5, 1.0, 2.0], (B, n)) if c["exact"] else rng.standard_normal((B, n))
        d = dict(grad=g.astype(np.float32))
    elif e == "path":
        B, L, D = c["shape"]
        g = rng.standard_normal((B, L, D)) * (0.5 + rng.random((B, 1, 1)))
        if c["zero"] == "row1":
            g[1] = 0.0
        elif c["zero"] == "all":
            g[:] = 0.0
        d = dict(grad=g.astype(np.float32), mean_path=np.array([MEAN_PATH], np.float32))
    else:
        d, info = _ema_inputs(c)
    for a in d.values():
        a.setflags(write=False)
    return d, info


def inputs(name):
    """Read-only float32 arrays of a case (shared by the cases of one `data` key)."""
    return _data(CASE[name]["data"])[0]


def info(name):
    """What the draw of a case recorded: the seed and the smallest float64 s (stddev), the layout rows (EMA)."""
    return _data(CASE[name]["data"])[1]


# ---------------------------------------------------------------------------------------------- references
def mbstd_run(fn, dt, i):
    """out, gx, (ggout, xg) of a stddev function in dtype `dt`: forward, backward, backward of the backward; the
    appended maps apart from the copies."""
    x = torch.tensor(i["x"], dtype=dt).requires_grad_(True)
    gout = torch.tensor(i["gout"], dtype=dt).requires_grad_(True)
    C = x.shape[1]
    out = fn(x)
    gx, = torch.autograd.grad(out, x, gout, create_graph=True)
    ggout, xg = torch.autograd.grad(gx, (gout, x), torch.tensor(i["ggx"], dtype=dt), allow_unused=True)
    xg = torch.zeros_like(x) if xg is None else xg
    return {"out.copy": out[:, :C], "out.map": out[:, C:], "gx": gx, "ggout.copy": ggout[:, :C], "ggout.map": ggout[:, C:], "xg": xg}


def _ref(c, dt, plain):
    """name -> tensor.  plain: the float64 run on the shared statements of dtrain_cases / gtrain_cases."""
    o, i, e = Ops(dt), inputs(c["name"]), c["entry"]
    if e == "mbstd":
        feat = c["shape"][4]
        return mbstd_run((lambda t: dc.mbstd(t, feat)) if plain else (lambda t: mbstd(o, t, feat)), dt, i)
    if e == "d_logistic":
        real, fake = o.t(i["real"], True), o.t(i["fake"], True)
        loss = dc.d_logistic(real, fake) if plain else d_logistic(o, real, fake)
        g_real, g_fake = torch.autograd.grad(loss, (real, fake))
        return dict(loss=loss, mean_real=mean_of(o, real), mean_fake=mean_of(o, fake), sign=torch.sign(real).sum(), g_real=g_real,
                    g_fake=g_fake)
    if e == "g_nonsaturating":
        fake = o.t(i["fake"], True)
        loss = gc.g_nonsaturating(fake) if plain else g_nonsaturating(o, fake)
        return dict(loss=loss, g_fake=torch.autograd.grad(loss, fake)[0])
    if e == "r1":
        grad = o.t(i["grad"])
        per, mean = r1(o, grad)
        if plain:
            per = dc.r1_per_sample(grad)
            mean = per.mean()
        return dict(per_sample=per, mean=mean)
    grad, m0, decay = o.t(i["grad"], True), o.t(i["mean_path"])[0], f32(c["decay"])
    if plain and c["zero"] == "none":
        pen, pm, lengths = gc.path_penalty(grad, m0, decay)
        mean = lengths.mean()
    else:
        pen, pm, lengths, mean = path_penalty(o, grad, m0, decay)
    return dict(pen=pen, pm=pm, lengths=lengths, mean=mean, dgrad=torch.autograd.grad(pen, grad)[0])


def _head_bounds(c, i, r64):
    def sp(v):
        return float(np.max(np.logaddexp(0.0, v.astype(np.float64))))
    if c["entry"] == "g_nonsaturating":
        B, = c["shape"]
        return dict(loss=(B + 4) * EPS32 * sp(-i["fake"]), g_fake=4 * EPS32 / B + TINY32)
    Br, Bf = c["shape"]
    tr, tf = (Br + 4) * EPS32, (Bf + 4) * EPS32
    return dict(loss=tr * sp(-i["real"]) + tf * sp(i["fake"]), mean_real=tr * float(np.abs(i["real"]).max()),
                mean_fake=tf * float(np.abs(i["fake"]).max()), sign=0.0, g_real=4 * EPS32 / Br + TINY32, g_fake=4 * EPS32 / Bf + TINY32)


def _ema_expected(c):
    i, rows = inputs(c["name"]), info(c["name"])["rows"]
    want, bound = i["dst"].astype(np.float64), np.zeros(i["dst"].shape)
    for do, so, n in rows:
        d, s = i["dst"][do:do + n].astype(np.float64), i["src"][so:so + n].astype(np.float64)
        want[do:do + n] = d * f32(c["decay"]) + s * f32(c["rest"])
        bound[do:do + n] = 0.0 if c["exact"] else 3 * EPS32 * (np.abs(d) * f32(c["decay"]) + np.abs(s) * f32(c["rest"]))
    return dict(ref64=dict(dst=want), ref32={}, e32={}, bound=dict(dst=bound), exact=("dst",) if c["exact"] else ())


@functools.lru_cache(maxsize=None)
def _expected(key):
    c = next(c for c in CASES if c["data"] == key)
    if c["entry"] == "ema":
        return _ema_expected(c)
    r64 = {k: v.detach().numpy() for k, v in _ref(c, F64, True).items()}
    r32 = {k: v.detach().numpy() for k, v in _ref(c, F32, False).items()}
    e32 = {k: float(np.abs(r32[k].astype(np.float64) - r64[k]).max()) for k in r64}
    if c["entry"] in ("d_logistic", "g_nonsaturating"):
        bound, exact = _head_bounds(c, inputs(c["name"]), r64), ("sign",) if c["entry"] == "d_logistic" else ()
    else:
        bound = {k: 4 * e32[k] + 5e-6 * float(np.abs(r64[k]).max()) for k in r64}
        exact = ()
        if c["entry"] == "mbstd":
            exact = ("out.copy", "ggout.copy") + (("gx", "ggout.map") if c["exact"] else ())
        elif c["entry"] == "r1" and c["exact"]:
            exact = ("per_sample", "mean")
        elif c["entry"] == "path" and c["zero"] == "all":
            exact = ("lengths", "mean", "dgrad")
    for k in exact:
        bound[k] = 0.0
    if c["entry"] == "mbstd" and c["exact"]:     # d = 0: the map is sqrt(eps) (float32 eps, sqrtf: 2 eps32); xg only finite
        bound["out.map"], bound["xg"] = 2 * EPS32 * MB_EPS ** 0.5, np.inf
    for a in list(r64.values()) + list(r32.values()):
        a.setflags(write=False)
    return dict(ref64=r64, ref32=r32, e32=e32, bound=bound, exact=exact)


def expected(name):
    """ref64 / ref32 (output -> array), e32 and bound per output, and `exact`: the outputs that must equal float64."""
    return _expected(CASE[name]["data"])
