"""Case table of tests/test_pointwise_cases_cpu.py and tests/test_gpu_pointwise_paths.py: the pointwise entry points
g2s_fused_bias_act, g2s_noise_bias_act, g2s_clamp, g2s_add_bias_scale (csrc/fused_bias_act.hip) and
g2s_noise_bias_act_ps (csrc/synth_batch.hip), called through the C ABI so that the test controls the alignment of every
pointer.  Importable without a GPU.

A case is a dict: name, entry, kernel and turns (what it is meant to reach; `dispatch` restates the launchers and the
CPU test holds the two together), reason (why it takes that kernel) and the entry's own parameters.  `mis` names the
pointers that are misaligned: views one float into a 16-byte aligned buffer.  tests/test_gpu_pointwise_paths.py puts
a canary before and after every tensor and finds them unchanged afterwards.

  fba      g2s_fused_bias_act on x (N, C, HW), bias (C): step_b = HW, size_b = C.  Vector kernel (16 bytes per lane,
           at most 2048 workgroups): float32, n % 4 == 0, no bias or step_b % 4 == 0, x and y aligned, ref aligned in
           mode (3, 1); scalar kernel (at most 4096 workgroups) otherwise.  The four modes (act, grad) = (3, 0),
           (3, 1), (3, 2), (1, 0) with and without a bias on either kernel; one case per reason for the scalar kernel
           alone (n % 4 has no bias: with one, n is a multiple of step_b); second turns: (2, 3, 349528) has
           n / 4 = 524292 > 2048 * 256 quads and a bias index that changes inside a turn and across turns,
           (2, 3, 174763) has n = 1048578 > 4096 * 256 with an odd step_b, in float32 and float16; n = 0.
  nba,     g2s_noise_bias_act / _ps on x (2, 3, HW): vector kernel when HW % 4 == 0 and x, y, noise are aligned;
  nba_ps   grid.x is capped at 64, so HW = 65556 (16389 quads > 64 * 256) and HW = 16389 take a second turn; noise
           and bias NULL where the entry allows it; one map per sample for _ps.
  clamp    g2s_clamp decides per group of four: 16-byte access where the group is whole and x, y (and g, backward)
           are aligned ("vec"; "vec+tail" when n % 4 leaves a ragged last group), element by element otherwise.
           At most CLAMP_BLOCKS = 256 * 8 workgroups of 256 lanes of 4 elements: n > 2097152 takes a second turn.
           Values exactly at lo and hi, and a NaN (forward: stays; backward: no gradient).
  abs      g2s_add_bias_scale: one decision for the launch (n % 4, hw % 4, a, y, b aligned), the same grid cap.

Expected values.  fused_bias_act: the C oracle (capi.fused_bias_act), bit for bit; float16 rounds x + bias to half
first as the kernel's storage type does, then the oracle's activation, then half again.  The others: the same
expression in numpy float32 in the kernel's order — x + nw * noise, + bias, slope, scale; (a + b) + bias, scale — one
rounding per step, compared with assert_array_equal.  One exception: x + nw * noise contracts to a fused
multiply-add where the compiler chooses to (fused_bias_act.hip and synth_batch.hip are built with contraction on), so
a noise case has two candidates, the two-rounding sum and the one-rounding fma (evaluated through float64, where the
product is exact), and every element must equal one of them bit for bit: at most one ulp of that sum, nothing else.
Measured on an MI355X: every other case is bit-identical to its single expectation; in the noise cases 11 to 23 % of
the elements differ from the two-rounding sum and equal the fma, on the vector and the scalar kernels alike.

The CPU test also holds every expectation to 2 * 2^-23 (2^-10 for float16) of the largest term of its float64
restatement times the gain: two ulp at the magnitude the roundings happen at (a sum that cancels keeps the absolute
error of its terms)."""
import functools
import zlib

import numpy as np

FBA_VEC_BLOCKS, FBA_SCALAR_BLOCKS = 2048, 4096      # launch_vec4 / g2s_fused_bias_act: std::min(cdiv(..., 256), ...)
NBA_BLOCKS_X = 64                                   # g2s_noise_bias_act(_ps): std::min(cdiv(HW4 or HW, 256), 64)
CLAMP_BLOCKS = 256 * 8                              # g2s_clamp, g2s_add_bias_scale: std::min(cdiv(quads, 256), 256 * 8)
LANES = 256
ALPHA, SCALE = 0.2, float(np.sqrt(2.0))
LO, HI = -1.0, 1.0
MODES = ((3, 0), (3, 1), (3, 2), (1, 0))
A64, S64 = float(np.float32(ALPHA)), float(np.float32(SCALE))     # what the kernels receive

CASES = []


def _add(name, entry, kernel, reason, turns=1, **kw):
    CASES.append(dict(name=name, entry=entry, kernel=kernel, reason=reason, turns=turns, mis=kw.pop("mis", ()), **kw))


for _a, _g in MODES:
    for _b in (True, False):
        _t = f"{_a}{_g}_{'bias' if _b else 'nobias'}"
        _add(f"fba_vec_{_t}", "fba", "vec", "aligned", shape=(2, 3, 20), act=_a, grad=_g, bias=_b)
        if _b:
            _add(f"fba_scalar_{_t}", "fba", "scalar", "step_b%4", shape=(2, 2, 5), act=_a, grad=_g, bias=True)
        else:
            _add(f"fba_scalar_{_t}", "fba", "scalar", "n%4", shape=(1, 3, 7), act=_a, grad=_g, bias=False)
    _add(f"fba_f16_{_a}{_g}", "fba", "scalar", "f16", shape=(2, 3, 20), act=_a, grad=_g, bias=True, f16=True)
_add("fba_mis_x", "fba", "scalar", "x misaligned", shape=(2, 3, 20), act=3, grad=0, bias=True, mis=("x",))
_add("fba_mis_y", "fba", "scalar", "y misaligned", shape=(2, 3, 20), act=3, grad=0, bias=True, mis=("y",))
_add("fba_mis_ref", "fba", "scalar", "ref misaligned", shape=(2, 3, 20), act=3, grad=1, bias=True, mis=("ref",))
_add("fba_turn_vec", "fba", "vec", "aligned", 2, shape=(2, 3, 349528), act=3, grad=0, bias=True)
_add("fba_turn_scalar", "fba", "scalar", "step_b%4", 2, shape=(2, 3, 174763), act=3, grad=0, bias=True)
_add("fba_turn_f16", "fba", "scalar", "f16", 2, shape=(2, 3, 174763), act=3, grad=0, bias=True, f16=True)

for _e in ("nba", "nba_ps"):
    _add(f"{_e}_vec", _e, "vec", "aligned", hw=1028, noise=True, bias=True)
    _add(f"{_e}_vec_nobias", _e, "vec", "aligned", hw=1028, noise=True, bias=False)
    _add(f"{_e}_scalar", _e, "scalar", "hw%4", hw=1027, noise=True, bias=True)
    _add(f"{_e}_scalar_nobias", _e, "scalar", "hw%4", hw=1027, noise=True, bias=False)
    for _m in ("x", "y", "noise"):
        _add(f"{_e}_mis_{_m}", _e, "scalar", f"{_m} misaligned", hw=1028, noise=True, bias=True, mis=(_m,))
    _add(f"{_e}_turn_vec", _e, "vec", "aligned", 2, hw=65556, noise=True, bias=True)
    _add(f"{_e}_turn_scalar", _e, "scalar", "hw%4", 2, hw=16389, noise=True, bias=True)
_add("nba_vec_nonoise", "nba", "vec", "aligned", hw=1028, noise=False, bias=True)
_add("nba_vec_neither", "nba", "vec", "aligned", hw=1028, noise=False, bias=False)
_add("nba_scalar_nonoise", "nba", "scalar", "hw%4", hw=1027, noise=False, bias=True)
_add("nba_scalar_neither", "nba", "scalar", "hw%4", hw=1027, noise=False, bias=False)

for _d, _t in ((0, "fwd"), (1, "bwd")):
    _add(f"clamp_{_t}_vec", "clamp", "vec", "aligned", n=1028, backward=_d)
    for _r in (1, 2, 3):
        _add(f"clamp_{_t}_tail{_r}", "clamp", "vec+tail", f"n%4={_r}", n=1028 + _r, backward=_d)
    for _m in ("x", "y") + (("g",) if _d else ()):
        _add(f"clamp_{_t}_mis_{_m}", "clamp", "scalar", f"{_m} misaligned", n=1028, backward=_d, mis=(_m,))
    _add(f"clamp_{_t}_turn", "clamp", "vec+tail", "n%4=3", 2, n=CLAMP_BLOCKS * LANES * 4 + 1035, backward=_d)

_add("abs_vec", "abs", "vec", "aligned", shape=(2, 3, 20), b=True, bias=True)
_add("abs_vec_nob", "abs", "vec", "aligned", shape=(2, 3, 20), b=False, bias=True)
_add("abs_vec_nobias", "abs", "vec", "aligned", shape=(2, 3, 20), b=True, bias=False)
_add("abs_ragged_hw", "abs", "scalar", "hw%4", shape=(2, 2, 5), b=True, bias=True)
_add("abs_ragged_n", "abs", "scalar", "n%4", shape=(1, 3, 7), b=True, bias=True)
_add("abs_scalar_nob", "abs", "scalar", "hw%4", shape=(2, 2, 5), b=False, bias=True)
_add("abs_scalar_nobias", "abs", "scalar", "hw%4", shape=(2, 2, 5), b=True, bias=False)
for _m in ("a", "y", "b"):
    _add(f"abs_mis_{_m}", "abs", "scalar", f"{_m} misaligned", shape=(2, 3, 20), b=True, bias=True, mis=(_m,))
_add("abs_turn_vec", "abs", "vec", "aligned", 2, shape=(2, 3, 349528), b=True, bias=True)
_add("abs_turn_scalar", "abs", "scalar", "n%4", 2, shape=(2, 3, 349529), b=True, bias=True)

NAMES = [c["name"] for c in CASES]
CASE = {c["name"]: c for c in CASES}
assert len(CASE) == len(CASES)


def _cdiv(a, b):
    return -(-a // b)


def dispatch(c):
    """(kernel, turns of its grid-stride loop) the launcher of this case's entry takes."""
    e, mis = c["entry"], set(c["mis"])
    if e == "fba":
        n, step_b = int(np.prod(c["shape"])), c["shape"][2]
        # `dtype == G2S_F32 && n % 4 == 0 && (!bias || step_b % 4 == 0) && aligned16(x) && aligned16(y) &&
        #  (mode != MODE_LRELU_GRAD || aligned16(ref))`
        vec = (not c.get("f16") and n % 4 == 0 and (not c["bias"] or step_b % 4 == 0) and not mis & {"x", "y"}
               and not ((c["act"], c["grad"]) == (3, 1) and "ref" in mis))
        if vec:
            return "vec", _cdiv(n // 4, min(_cdiv(n // 4, LANES), FBA_VEC_BLOCKS) * LANES)
        return "scalar", _cdiv(n, min(_cdiv(n, LANES), FBA_SCALAR_BLOCKS) * LANES)
    if e in ("nba", "nba_ps"):
        hw = c["hw"]
        # `HW % 4 == 0 && aligned16(x) && aligned16(y) && (!noise || aligned16(noise))`
        vec = hw % 4 == 0 and not mis & {"x", "y"} and not (c["noise"] and "noise" in mis)
        m = hw // 4 if vec else hw
        return ("vec" if vec else "scalar"), _cdiv(m, min(_cdiv(m, LANES), NBA_BLOCKS_X) * LANES)
    n = c["n"] if e == "clamp" else int(np.prod(c["shape"]))
    quads = _cdiv(n, 4)
    t = _cdiv(quads, min(_cdiv(quads, LANES), CLAMP_BLOCKS) * LANES)
    if e == "clamp":
        # per group: `i + 4 <= n && ((x + i | y + i | (dir ? g + i : x + i)) & 15) == 0`
        if mis & ({"x", "y", "g"} if c["backward"] else {"x", "y"}):
            return "scalar", t
        return ("vec" if n % 4 == 0 else "vec+tail"), t
    # abs: `(n & 3) == 0 && (hw & 3) == 0 && ((a | y | b) & 15) == 0`
    vec = n % 4 == 0 and c["shape"][2] % 4 == 0 and not mis & ({"a", "y", "b"} if c["b"] else {"a", "y"})
    return ("vec" if vec else "scalar"), t


@functools.lru_cache(maxsize=None)
def inputs(name):
    """The float32 (float16 for an f16 case) input arrays of a case, read-only; an absent tensor is None."""
    c = CASE[name]
    rng = np.random.default_rng([20253, zlib.crc32(name.encode())])
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    e = c["entry"]
    if e == "fba":
        dt = np.float16 if c.get("f16") else np.float32
        d = dict(x=f(*c["shape"]).astype(dt), bias=f(c["shape"][1]).astype(dt) if c["bias"] else None,
                 ref=f(*c["shape"]).astype(dt) if (c["act"], c["grad"]) == (3, 1) else None)
    elif e in ("nba", "nba_ps"):
        d = dict(x=f(2, 3, c["hw"]), bias=f(3) if c["bias"] else None, nw=np.float32(0.7),
                 noise=(f(2, c["hw"]) if e == "nba_ps" else f(c["hw"])) if c["noise"] else None)
    elif e == "clamp":
        x = 1.5 * f(c["n"])
        x[3], x[4], x[-1], x[-2], x[7] = LO, HI, HI, LO, np.nan
        x[1], x[2] = np.nextafter(np.float32(LO), np.float32(-2)), np.nextafter(np.float32(HI), np.float32(2))
        d = dict(x=x, g=f(c["n"]) if c["backward"] else None)
    else:
        d = dict(a=f(*c["shape"]), b=f(*c["shape"]) if c["b"] else None, bias=f(c["shape"][1]) if c["bias"] else None)
    for a in d.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return d


def _lrelu(t, alpha, scale):
    return np.where(t > 0, t, t * alpha) * scale


def _fba64(x, bias, ref, act, grad):
    """(value, largest term) of the fused_bias_act expression in float64."""
    x = x.astype(np.float64)
    b = 0.0 if bias is None else bias.astype(np.float64)[None, :, None]
    v = x + b
    if (act, grad) == (3, 0):
        o = np.where(v > 0, v, v * A64)
    elif (act, grad) == (3, 1):
        o = np.where(ref.astype(np.float64) > 0, v, v * A64)
    elif (act, grad) == (3, 2):
        o = np.zeros_like(v)
    else:
        o = v
    return o * S64, np.maximum(np.maximum(np.abs(x), np.abs(b)), np.abs(v))


@functools.lru_cache(maxsize=None)
def expected(name):
    """The candidates of a case's output: a tuple of float32 (float16) arrays; the kernel must equal one of them in
    every element (one candidate everywhere but the noise cases: see the module docstring)."""
    from oracle import capi
    c, d = CASE[name], inputs(name)
    e = c["entry"]
    f32 = np.float32
    if e == "fba":
        if not c.get("f16"):
            return (capi.fused_bias_act(d["x"], d["bias"], d["ref"], c["act"], c["grad"], ALPHA, SCALE),)
        v = d["x"].astype(f32)
        if d["bias"] is not None:       # `to_f(from_f(v + b))`: the sum lives in the storage type
            v = (v + d["bias"].astype(f32)[None, :, None]).astype(np.float16).astype(f32)
        r = None if d["ref"] is None else d["ref"].astype(f32)
        return (capi.fused_bias_act(v, None, r, c["act"], c["grad"], ALPHA, SCALE).astype(np.float16),)
    if e in ("nba", "nba_ps"):
        x, bb = d["x"], (f32(0) if d["bias"] is None else d["bias"][None, :, None])
        if d["noise"] is None:
            return (_lrelu(x + bb, f32(ALPHA), f32(SCALE)).astype(f32),)
        nz = d["noise"][:, None, :] if e == "nba_ps" else d["noise"][None, None, :]
        two = x + d["nw"] * nz                                                              # product rounded, then the sum
        fma = (np.float64(d["nw"]) * nz.astype(np.float64) + x.astype(np.float64)).astype(f32)   # one rounding
        return tuple(_lrelu(v + bb, f32(ALPHA), f32(SCALE)).astype(f32) for v in (two, fma))
    if e == "clamp":
        x = d["x"]
        with np.errstate(invalid="ignore"):
            if c["backward"]:
                return (np.where((x >= f32(LO)) & (x <= f32(HI)), d["g"], f32(0)),)
            return (np.where(x < f32(LO), f32(LO), np.where(x > f32(HI), f32(HI), x)),)
    v = d["a"] if d["b"] is None else d["a"] + d["b"]
    if d["bias"] is not None:
        v = v + d["bias"][None, :, None]
    return ((v * f32(SCALE)).astype(f32),)


def restatement64(name):
    """(float64 value, tolerance per element) of a case: 2 * eps of the largest term times the gain; None for clamp,
    which rounds nothing."""
    c, d = CASE[name], inputs(name)
    e = c["entry"]
    if e == "clamp":
        return None
    eps = 2.0 ** -10 if c.get("f16") else 2.0 ** -23
    if e == "fba":
        val, big = _fba64(d["x"], d["bias"], d["ref"], c["act"], c["grad"])
    elif e in ("nba", "nba_ps"):
        x = d["x"].astype(np.float64)
        t = 0.0
        if d["noise"] is not None:
            nz = d["noise"].astype(np.float64)
            t = np.float64(d["nw"]) * (nz[:, None, :] if e == "nba_ps" else nz[None, None, :])
        b = 0.0 if d["bias"] is None else d["bias"].astype(np.float64)[None, :, None]
        val = _lrelu(x + t + b, A64, S64)
        big = np.max([np.abs(x), np.abs(t) + 0 * x, np.abs(b) + 0 * x, np.abs(x + t), np.abs(x + t + b)], axis=0)
    else:
        a = d["a"].astype(np.float64)
        b = 0.0 if d["b"] is None else d["b"].astype(np.float64)
        bias = 0.0 if d["bias"] is None else d["bias"].astype(np.float64)[None, :, None]
        val = (a + b + bias) * S64
        big = np.max([np.abs(a), np.abs(b) + 0 * a, np.abs(bias) + 0 * a, np.abs(a + b), np.abs(a + b + bias)], axis=0)
    return val, 2 * eps * big * SCALE
