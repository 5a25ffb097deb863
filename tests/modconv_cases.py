"""Case tables of tests/test_modconv_cases_cpu.py and tests/test_gpu_modconv_paths.py: g2s_modconv_f16 (csrc/modconv_f16.hip:
the quad, narrow and polyphase bodies) and what g2s_modconv (fp32) has beyond g2s_conv2d — input / output scales, the
StyledConv tail with its noise, the y_is_zero promise and the thin 1x1 dispatch — at shapes that reach every launch path,
against a float64 reference.  Importable without a GPU.  Geometry, plans, reference and bound build on
tests/conv2d_cases.py (plan_conv, classes, conv_reference, bound, floor_e32, RATIO, RATIO_UNSPLIT, EPS32).

Operand contract of the fp16 route.  The kernel multiplies fp16_rtne(fl32(x * in_scale)) by fp16_rtne(w): the scale is
applied in float32 BEFORE the rounding, the rounding is to nearest even, products of two halves are exact in float32, the
accumulator and the epilogue (out-scale, bias, leaky-ReLU, gain) are float32.  Only the order of the float32 accumulation
is free, so the reference is float64 on the ROUNDED operands and the bound is that of the fp32 kernel's tests.

plan_f16 / plan_f32 restate modconv_launch + conv_launch on top of plan_conv(tuned=False).  fp16 route: no tuned table,
no 32x128 rule, the size rule's 128x64 becomes 64x64 (a forced tile 1 is not remapped: it launches the 128x128 instance on
a grid sized for 64-pixel tiles, whose surplus workgroups leave at the tile check), tiles 3 and 4 are rejected; the body
of a class is quad (T = 9, W >= 4), narrow (T = 9, W < 4) or p4 / p2 / p1, with 4 / 8 / 8 / 16 / 32 channels per K tile;
the split-K count is planned with the fp32 kernel's K tiles (kt_min) and slice i of a class is empty when
i * ceil(ktiles16 / splitk) >= ktiles16.  fp32 route: no row of modconv_tuned.inc matches any case (asserted), and
thin_conv_eligible is restated.

Labels (every row claims the ones it is there for; tests/test_modconv_cases_cpu.py holds rows and table to them):
  quad:scale quad:noscale narrow:.. p4:.. p2:.. p1:..   the body of a class x whether in_scale is given
  quad:fwd quad:rev quad:is2 quad:W4 quad:W5+ H!=W      quad form: ascending taps / the adjoint of the stride-1 3x3 (the
                                                        transposed PLAIN call: triple reversed in registers) / the stride-2
                                                        gather (DOWN2 forward, UP2 transposed); W = 4: both clamped load
                                                        positions xa = 0, 1 occur and the left- and right-shifted columns
                                                        are adjacent; W >= 5
  quad:sub quad:full quad:partial (and narrow: p4: ..)   Cr below one K tile of the body, a multiple, or not
  tile0:forced tile1:forced tile2:forced tile0:heuristic tile2:heuristic pick1->2
  M<64 M%64 M%128 N%tile spans-batch ragged-classes early-exit     with the kernel instance's own tile (128x128 or 64x64)
  split:1 split:heuristic split:forced split:forced:2 split:forced:3 split:clipped split:empty-slices split:det
  ep:none ep:out_scale ep:bias:kernel ep:bias:deferred ep:bias+act:kernel .. ep:act:kernel ep:act:deferred
  holes overwrites needs-zero
  fp32 only: noise:kernel noise:deferred thin:just-eligible thin:just-not thin:noise-keeps-mfma promise:y_is_zero

Operands.  Seeded N(0, 1) draws rounded to float32 (weights unscaled and without symmetry), scales 1 + 0.3 N(0, 1) clipped
to [0.4, 1.6]; every |x| and |w| below 2^-8 is moved out to +-2^-8, so that every fp16 operand image is a normal number
(tests/test_modconv_cases_cpu.py asserts it: the matrix unit's handling of half denormals is not part of this test).

Reference (float64, explicit shifted slices: conv2d_cases.conv_reference).
  fp16 route  ref = tail(out_scale * conv(float16(float32(x) * float32(s)), float16(w)))
  fp32 route  ref = tail(out_scale * conv(x * s, w) + noise_w * noise)

Bound, per element: |kernel - ref| <= min(ratio * e32 * max|ref|, cap); no element is left out (slopes are at most 1).
  e32   torch's float32 CPU evaluation of the same operation (on the rounded operands for the fp16 route) against the
        float64 reference, as a share of max|ref|, floored at half a float32 spacing (conv2d_cases.floor_e32).
  cap   gain * (n + r) * eps32 * (sum|terms| + |bias| + |noise_w * noise|): n = Cr * T of the element's class (0 in a
        hole), r the extra roundings: 1 for the scale product (fp32 route), 1 for the out-scale, 3 for bias, slope and
        gain, 2 for the noise product and its addition.
  ratio RATIO = 4 on every path; see the measurements.

Measured on an MI355X, largest error / (e32 * max|ref|) (e32 floored) and largest error / cap over the cases of a path:

    g2s_modconv_f16                   tile0 (128x128)   tile1 (forced)    tile2 (64x64)
    body        form                   ratio   /cap      ratio   /cap      ratio   /cap
    quad        plain                   0.48  0.034       0.48  0.016       0.83  0.032
    quad        split-K                 0.34  0.005       0.34  0.005       0.45  0.014
    quad        split-K, deferred tail     -      -          -      -       0.49  0.015
    quad        deterministic flag         -      -          -      -       0.72  0.004
    narrow      plain                   0.63  0.005       0.63  0.005       0.80  0.015
    narrow      split-K                 0.31  0.004       0.30  0.004       0.39  0.004
    p4+p2+p1    plain                   0.35  0.020       0.54  0.019       0.55  0.023
    p4+p2+p1    split-K                 0.25  0.009       0.25  0.009       0.60  0.021
    p4+p2+p1    split-K, deferred tail     -      -          -      -       0.55  0.018
    p1 (1x1)    plain                   0.36  0.010       0.36  0.010       1.02  0.389
    p1 (1x1)    holes, deferred tail       -      -          -      -       0.35  0.113
    p1 (1x1)    split-K                 0.36  0.010       0.36  0.010       0.36  0.010

    g2s_modconv (fp32, scales / noise)   ratio   /cap
    T9  plain (64x64)                     1.75  0.040       T1  plain (64x64, holes deferred: 1.00)   1.00  0.227
    T9  split-K                           0.58  0.002       T1  plain (32x128: the thin rule's other side)  1.00  0.267
    T9  split-K, deferred tail / noise    1.00  0.017       T4+T2+T1  plain                          0.99  0.032
    T9  deterministic flag                0.95  0.004       thin 1x1 streaming kernel                 0.91  0.231

Not measured: tile 0 and tile 1 with a deferred tail or under the deterministic flag on the fp16 route (the sweep carries no
epilogue), and the fp32 route on other tiles than the heuristic's (tests/test_gpu_conv2d_paths.py sweeps those without scales).
v_mfma_f32_32x32x16_f16 shows no rounding of its own beyond float32 accumulation: no path of the fp16 route exceeds 1.02 x e32
(the 1x1 body at Cr = 3, where e32 sits on its floor of half a spacing), so every path keeps RATIO = 4, the deterministic
flag included (the chains of these cases, at most 34 x 9 terms, are far shorter than those behind RATIO_UNSPLIT).

Two findings of these tables, both fixed with them:
  * the pipelined 1-/2-/4-tap body rounded the EXACT product x * s to a half in one step (the product and the conversion
    were selected as one v_fma_mixlo_f16) where the contract rounds fl32(x * s): heur_1to2 (10 of its 147456 scaled
    activations land on a tie of two halves in float32; 190 outputs off by up to 2371 x e32) and sw_poly under tile 0
    (2 of 3920; 391 outputs, 160 x e32 — the float64 reference with single rounding reproduces 160.03).  Small rows rarely
    hold such a value (probability 2^-14 each): heur_1to2 and heur_tile0 (17 of 262144) are the rows that pin it.
  * a bias / activation on a launch whose classes leave holes (k = 1, UP2) never reached the holes, which must hold the
    tail of 0 (p_holes_bias: 5520 of 7920 elements); conv_launch now runs that tail as the second launch.
"""
import functools
import os
import re
import zlib

import numpy as np

import conv2d_cases as cc
from conv2d_cases import EPS32, RATIO, RATIO_UNSPLIT, cdiv   # noqa: F401  (re-exported to the two test files)

PLAIN, UP2, DOWN2 = 0, 1, 2
GAIN = cc.GAIN
F16_MIN_NORMAL = 2.0 ** -14
FLOOR_OPERAND = 2.0 ** -8
THIN_PIXELS = 1 << 16
BODIES = ("quad", "narrow", "p4", "p2", "p1")


class Rejected(ValueError):
    """modconv_f16_launch's G2S_REQUIRE on the tile."""


def f16_cpt(T, quad):
    """csrc/modconv_f16.hip, f16_cpt: reduction channels per K tile."""
    return 4 if quad else 8 if T in (9, 4) else 16 if T == 2 else 32


def body_of(T, W):
    return ("quad" if W >= 4 else "narrow") if T == 9 else {4: "p4", 2: "p2", 1: "p1"}[T]


def body_cpt(body):
    return {"quad": 4, "narrow": 8, "p4": 8, "p2": 16, "p1": 32}[body]


def thin_conv_eligible(B, Cr, M, H, W, k, transpose):
    """csrc/thinconv.hip."""
    return k == 1 and not transpose and Cr <= 4 and M >= 16 and (H * W) % 4 == 0 and B * H * W >= THIN_PIXELS and B <= 65535


@functools.lru_cache(maxsize=None)
def modconv_tuned_rows():
    """The signatures of csrc/modconv_tuned.inc: (B, Cin, Cout, H, k, mode, transpose)."""
    rows = set()
    with open(os.path.join(cc.ROOT, "gan-2d-to-3d_amd", "csrc", "modconv_tuned.inc")) as f:
        for m in re.finditer(r"^\{([-\d, ]+)\}", f.read(), re.M):
            v = tuple(int(t) for t in m.group(1).split(","))
            assert len(v) == 10
            rows.add(v[:7])
    return rows


class Mod:
    """One g2s_modconv_f16 (route "f16") or g2s_modconv (route "f32") call.  Cr -> M are the channels of x and y OF THIS
    CALL (transpose: Cout -> Cin), H x W the size of x; scale / oscale: in_scale / out_scale given; ep: None or
    (bias, act, alpha, gain); noise: the StyledConv tail (fp32 route, needs ep = (True, True, ..)); tile / sk / det:
    g2s_modconv_tune and the deterministic flag; promise: a row of the y_is_zero test."""

    def __init__(self, name, B, Cr, M, H, W, k, mode, tr, scale=True, oscale=False, ep=None, noise=False, tile=-1, sk=-1,
                 det=False, route="f16", promise=False, claims=()):
        self.name, self.B, self.Cr, self.M, self.H, self.W, self.k, self.mode, self.tr = name, B, Cr, M, H, W, k, mode, int(tr)
        self.scale, self.oscale, self.ep, self.noise = bool(scale), bool(oscale), ep, bool(noise)
        self.tile, self.sk, self.det, self.route, self.promise, self.claims = tile, sk, det, route, promise, tuple(claims)
        assert k in (1, 3) and mode in (PLAIN, UP2, DOWN2) and route in ("f16", "f32")
        assert not noise or (route == "f32" and ep is not None and ep[0] and ep[1])
        # modconv_launch: the general geometry of conv_launch
        self.s = 1 if mode == PLAIN else 2
        self.p = k // 2 if mode == PLAIN else 0
        self.adj = int((mode == UP2) != bool(tr))
        self.mm = int(not tr)
        self.groups, self.eo = 1, (0, 0)
        self.Cin, self.Cout = (M, Cr) if tr else (Cr, M)        # the arguments of the C entry point

    @property
    def out_hw(self):
        return cc.out_size(self.H, self.W, self.k, self.s, self.p, self.adj)

    @property
    def fused(self):
        return self.ep is not None and (self.ep[0] or self.ep[1])

    def plan(self, tile=None, sk=None, det=None):
        args = (self.tile if tile is None else tile, self.sk if sk is None else sk, self.det if det is None else det)
        return plan_f16(self, *args) if self.route == "f16" else plan_f32(self, *args)

    def __repr__(self):
        return (f"{self.name}: {self.route} B{self.B} Cr{self.Cr} M{self.M} {self.H}x{self.W} k{self.k} mode{self.mode} "
                f"tr{self.tr} scale{int(self.scale)} oscale{int(self.oscale)} ep{self.ep} noise{int(self.noise)} "
                f"tune({self.tile},{self.sk}) det{int(self.det)}")


def _plan_conv(c, tile, sk, det):
    return cc.plan_conv(c.B, c.Cr, c.M, c.H, c.W, c.k, c.s, c.p, c.adj, c.mm, fused=c.fused or c.noise, tile=tile, splitk=sk,
                        det=det, tuned=False)


def size_rule(M, nmax, ncls):
    """conv_launch's tile heuristic before the 32x128 rule (which the fp16 route does not have)."""
    for i in range(3):
        if M > cc.CFGS[i][0] // 2 and cdiv(M, cc.CFGS[i][0]) * cdiv(nmax, cc.CFGS[i][1]) * ncls >= 512:
            return i
    return 2


def plan_f16(c, tile=-1, sk=-1, det=False):
    """modconv_launch(f16_operands) + conv_launch + modconv_f16_launch + modconv_f16_kernel for one call."""
    if tile >= 3:
        raise Rejected("fp16 operands: tiles 0..2 only")
    base = _plan_conv(c, -1, sk, det)
    rule = size_rule(c.M, base["nmax"], len(base["classes"]))
    pick = tile if tile >= 0 else 2 if rule == 1 else rule
    pl = _plan_conv(c, pick, sk, det)       # conv_launch from the tile on: grid, split-K (with the fp32 K tiles), deferral
    pl["source"] = "forced" if tile >= 0 else "heuristic"
    pl["remapped"] = tile < 0 and rule == 1
    pl["KBM"], pl["KBN"] = (64, 64) if pick == 2 else (128, 128)       # the instance modconv_f16_launch starts
    pl["bodies"] = [body_of(cl["T"], c.W) for cl in pl["classes"]]
    pl["ktiles16"] = [cdiv(c.Cr, body_cpt(b)) for b in pl["bodies"]]
    pl["per16"] = [cdiv(kt, pl["splitk"]) for kt in pl["ktiles16"]]
    pl["empty"] = [[i for i in range(pl["splitk"]) if i * per >= kt] for kt, per in zip(pl["ktiles16"], pl["per16"])]
    pl["thin"] = False
    return pl


def plan_f32(c, tile=-1, sk=-1, det=False):
    """modconv_launch + conv_launch for one g2s_modconv call; no row of modconv_tuned.inc may match (asserted by
    tests/test_modconv_cases_cpu.py), so conv_launch gets tuned_tile = tuned_splitk = -1."""
    thin = (not c.scale and not c.oscale and not c.noise and c.mode == PLAIN and tile == -1 and sk == -1
            and thin_conv_eligible(c.B, c.Cin, c.Cout, c.H, c.W, c.k, c.tr))
    pl = _plan_conv(c, tile, sk, det)
    pl["thin"] = thin
    if thin:
        pl.update(needs_zero=False, deferred=False, splitk=1, asked=1)
    pl["KBM"], pl["KBN"] = pl["BM"], pl["BN"]
    return pl


def ep_kind(c):
    if c.ep is None or not (c.ep[0] or c.ep[1]):
        return "out_scale" if c.oscale else "none"
    return "bias+act" if c.ep[0] and c.ep[1] else "bias" if c.ep[0] else "act"


def labels(c, pl):
    sc = "scale" if c.scale else "noscale"
    out = {"needs-zero" if pl["needs_zero"] else "overwrites"}
    if c.H != c.W:
        out.add("H!=W")
    if pl["holes"]:
        out.add("holes")
    kind = ep_kind(c)
    out.add(f"ep:{kind}" if kind in ("none", "out_scale") else f"ep:{kind}:{'deferred' if pl['deferred'] else 'kernel'}")
    if c.noise:
        out.add("noise:deferred" if pl["deferred"] else "noise:kernel")
    if c.promise:
        out.add("promise:y_is_zero")
    if c.route == "f32":
        elig = thin_conv_eligible(c.B, c.Cin, c.Cout, c.H, c.W, c.k, c.tr) and c.mode == PLAIN
        if pl["thin"]:
            out.add("thin:just-eligible")
        elif elig and c.noise:
            out.add("thin:noise-keeps-mfma")
        elif not elig and c.k == 1 and c.mode == PLAIN and not c.tr and not c.scale and not c.oscale and not c.noise and any(
                thin_conv_eligible(*v) for v in ((c.B, c.Cin, c.Cout + 1, c.H, c.W, 1, 0), (c.B, c.Cin - 1, c.Cout, c.H, c.W, 1, 0),
                                                 (c.B, c.Cin, c.Cout, c.H + 1, c.W, 1, 0), (c.B, c.Cin, c.Cout, c.H, c.W + 1, 1, 0),
                                                 (c.B, c.Cin, c.Cout, c.H, c.W - 1, 1, 0))):
            out.add("thin:just-not")        # one step in one argument away from the streaming kernel
        for cl in pl["classes"]:
            out.add(f"T{cl['T']}:{sc}")
    if pl["thin"]:
        return out
    # tile and ragged edges, with the tile of the instance that runs
    out.add(f"tile{pl['pick']}:{pl['source']}")
    if c.route == "f16" and pl["remapped"]:
        out.add("pick1->2")
    BM, BN = pl["KBM"], pl["KBN"]
    if c.M < 64:
        out.add("M<64")
    if c.M > 64 and c.M % 64:
        out.add("M%64")
    if BM == 128 and c.M > 128 and c.M % 128:
        out.add("M%128")
    sizes = [cl["OH"] * cl["OW"] for cl in pl["classes"]]
    if pl["nmax"] > BN and pl["nmax"] % BN:
        out.add("N%tile")
    if c.B > 1 and any(n % BN for n in sizes):
        out.add("spans-batch")
    if len(set(sizes)) > 1:
        out.add("ragged-classes")
    if any(cdiv(c.M, BM) * cdiv(c.B * n, BN) < pl["tiles"] for n in sizes):
        out.add("early-exit")
    # split-K
    if pl["splitk"] == 1:
        out.add("split:1")
    elif pl["split_source"] in ("heuristic", "forced"):
        out.add(f"split:{pl['split_source']}")
        if pl["split_source"] == "forced":
            out.add(f"split:forced:{pl['splitk']}")
    if pl["split_source"] == "det":
        out.add("split:det")
    if pl["asked"] > pl["splitk"]:
        out.add("split:clipped")
    if c.route == "f16":
        if any(pl["empty"]):
            out.add("split:empty-slices")
        for cl, body in zip(pl["classes"], pl["bodies"]):
            cpt = body_cpt(body)
            out.add(f"{body}:{sc}")
            out.add(f"{body}:" + ("sub" if c.Cr < cpt else "partial" if c.Cr % cpt else "full"))
            if body == "quad":
                out.add("quad:is2" if c.s == 2 else "quad:rev" if c.adj else "quad:fwd")
                if c.s == 1:
                    out.add("quad:W4" if c.W == 4 else "quad:W5+")
    return out


# --------------------------------------------------------------------------------------------------------- tables
BA = (True, True, 0.2, GAIN)


def _f16_cases():
    rows = []
    add = lambda *a, **kw: rows.append(Mod(*a, **kw))       # noqa: E731
    # the quad form: forward, adjoint (reversed triple), stride-2 gather, W = 4 and W >= 5, with and without the scale;
    # 6 x 7 = 42 pixels, B = 2: 84 pixels, a ragged second 64-pixel tile that holds pixels of both samples
    add("q_fwd", 2, 6, 40, 6, 7, 3, PLAIN, 0, claims=("quad:scale", "quad:fwd", "quad:W5+", "quad:partial", "H!=W", "M<64",
                                                     "N%tile", "spans-batch", "tile2:heuristic", "split:1", "ep:none", "overwrites"))
    add("q_fwd_ns", 2, 6, 40, 6, 7, 3, PLAIN, 0, scale=False, claims=("quad:noscale", "quad:fwd", "quad:partial"))
    add("q_rev", 2, 6, 40, 6, 7, 3, PLAIN, 1, claims=("quad:scale", "quad:rev", "quad:W5+", "quad:partial"))
    add("q_rev_ns", 2, 6, 40, 7, 5, 3, PLAIN, 1, scale=False, claims=("quad:noscale", "quad:rev", "quad:W5+"))
    add("q_down", 2, 6, 40, 9, 11, 3, DOWN2, 0, claims=("quad:scale", "quad:is2", "quad:partial"))
    add("q_up_t", 2, 6, 40, 9, 11, 3, UP2, 1, scale=False, claims=("quad:noscale", "quad:is2"))
    add("q_down_w4", 3, 6, 40, 7, 4, 3, DOWN2, 0, claims=("quad:is2", "H!=W"))       # one output column, xa = 0 only
    add("q_w4", 2, 6, 40, 5, 4, 3, PLAIN, 0, claims=("quad:W4", "quad:fwd", "quad:scale", "H!=W"))
    add("q_w4_rev", 2, 6, 40, 5, 4, 3, PLAIN, 1, claims=("quad:W4", "quad:rev", "quad:scale"))
    add("q_w4_sq_ns", 3, 5, 40, 4, 4, 3, PLAIN, 0, scale=False, claims=("quad:W4", "quad:noscale", "quad:partial"))
    # Cr against the 4 channels of a quad K tile
    add("q_sub", 2, 3, 40, 6, 7, 3, PLAIN, 0, claims=("quad:sub", "quad:scale"))
    add("q_full", 2, 8, 40, 6, 7, 3, PLAIN, 0, claims=("quad:full", "quad:scale"))
    add("q_partial_rev", 2, 9, 40, 6, 7, 3, PLAIN, 1, claims=("quad:partial", "quad:rev"))
    # the un-pipelined body: maps narrower than 4
    add("n_w3", 3, 11, 40, 5, 3, 3, PLAIN, 0, claims=("narrow:scale", "narrow:partial", "H!=W"))
    add("n_w3_ns", 3, 11, 40, 5, 3, 3, PLAIN, 1, scale=False, claims=("narrow:noscale", "narrow:partial"))
    add("n_w2_sub", 3, 5, 40, 6, 2, 3, PLAIN, 0, claims=("narrow:scale", "narrow:sub"))
    add("n_down", 3, 16, 40, 7, 3, 3, DOWN2, 0, claims=("narrow:scale", "narrow:full"))
    # the polyphase bodies: the 3x3 stride-2 scatter (4 / 2 / 2 / 1 taps) and the 1x1 kernels; 4 x 7 -> 9 x 15: classes of
    # 40 / 35 / 32 / 28 pixels, B = 2: 2 / 2 / 1 / 1 tiles of 64
    add("p_up", 2, 35, 40, 4, 7, 3, UP2, 0, claims=("p4:scale", "p2:scale", "p1:scale", "p4:partial", "p2:partial", "p1:partial",
                                                    "ragged-classes", "early-exit", "spans-batch", "overwrites"))
    add("p_up_ns", 2, 35, 40, 4, 7, 3, UP2, 0, scale=False, claims=("p4:noscale", "p2:noscale", "p1:noscale", "p4:partial"))
    add("p_down_t", 2, 35, 40, 4, 7, 3, DOWN2, 1, claims=("p4:scale", "p2:scale", "p1:scale", "p2:partial"))
    add("p_k1", 2, 35, 40, 6, 7, 1, PLAIN, 0, claims=("p1:scale", "p1:partial"))
    add("p_k1_t_ns", 2, 35, 40, 6, 7, 1, PLAIN, 1, scale=False, claims=("p1:noscale", "p1:partial"))
    add("p_k1_down", 2, 35, 40, 9, 11, 1, DOWN2, 0, claims=("p1:scale",))
    add("p_holes", 2, 35, 40, 5, 6, 1, UP2, 0, claims=("holes", "needs-zero", "p1:scale"))
    # a hole holds the tail of 0: gain * leaky_relu(bias); the tail runs as the second launch there
    add("p_holes_bias", 2, 35, 40, 5, 6, 1, UP2, 0, ep=BA, oscale=True, claims=("holes", "needs-zero", "ep:bias+act:deferred"))
    # tiles: forced 0 / 1 / 2, M across two row tiles (140 = 128 + 12 = 2 x 64 + 12), 3 x 54 = 162 pixels
    add("t0_forced", 3, 6, 140, 6, 9, 3, PLAIN, 0, tile=0, claims=("tile0:forced", "M%128", "N%tile", "spans-batch", "quad:scale"))
    add("t1_forced", 3, 6, 140, 6, 9, 3, PLAIN, 0, tile=1, claims=("tile1:forced", "M%128", "early-exit", "quad:scale"))
    add("t1_forced_up", 2, 35, 140, 4, 7, 3, UP2, 0, tile=1, claims=("tile1:forced", "early-exit", "p4:scale", "ragged-classes"))
    add("t2_forced", 3, 6, 140, 6, 9, 3, PLAIN, 1, tile=2, claims=("tile2:forced", "M%64", "N%tile", "quad:rev"))
    add("t0_forced_up", 2, 35, 70, 4, 7, 3, UP2, 0, tile=0, scale=False, claims=("tile0:forced", "M%64", "p4:noscale"))
    # the size rule's own 128x128 (512 tiles: B = 4, 96 channels, 128 x 128) and its 128x64 that becomes 64x64 (B = 3)
    add("heur_tile0", 4, 4, 96, 128, 128, 3, PLAIN, 0, claims=("tile0:heuristic", "quad:full", "quad:scale"))
    add("heur_1to2", 3, 3, 96, 128, 128, 1, PLAIN, 0, claims=("pick1->2", "tile2:heuristic", "p1:scale", "M%64"))
    # split-K: the heuristic's (the fp32 kernel's K tiles decide: 17 of 2 channels -> 2 slices of 5 + 4 quad tiles; the
    # 1-tap class of the polyphase form has 16 channels per fp32 K tile, so only Cr >= 256 makes the heuristic split it)
    add("s_heur", 1, 34, 40, 6, 7, 3, PLAIN, 0, claims=("split:heuristic", "needs-zero", "quad:partial", "quad:scale"))
    add("s_heur_up", 1, 260, 8, 3, 4, 3, UP2, 0, claims=("split:heuristic", "p4:partial", "p2:partial", "p1:partial", "p4:scale"))
    add("s_forced2", 2, 22, 40, 6, 7, 3, PLAIN, 0, sk=2, claims=("split:forced", "split:forced:2", "quad:partial", "needs-zero"))
    add("s_forced3", 2, 22, 40, 6, 7, 3, PLAIN, 1, sk=3, claims=("split:forced", "split:forced:3", "quad:rev"))
    add("s_forced2_up", 2, 70, 40, 4, 7, 3, UP2, 0, sk=2, claims=("split:forced:2", "p4:partial", "p2:partial", "p1:partial"))
    add("s_forced3_up", 2, 70, 40, 4, 7, 3, UP2, 0, sk=3, scale=False, claims=("split:forced:3", "p4:noscale"))
    add("s_forced2_n", 3, 20, 40, 5, 3, 3, PLAIN, 0, sk=2, claims=("split:forced:2", "narrow:partial", "narrow:scale"))
    add("s_forced2_t0", 3, 22, 140, 6, 9, 3, PLAIN, 0, sk=2, tile=0, claims=("split:forced:2", "tile0:forced", "M%128"))
    add("s_clipped", 2, 6, 40, 6, 7, 3, PLAIN, 0, sk=64, claims=("split:clipped", "split:forced:3", "split:empty-slices"))
    add("s_empty", 2, 8, 40, 6, 7, 3, PLAIN, 0, sk=4, claims=("split:empty-slices", "split:forced", "quad:full"))
    add("s_empty_up", 2, 35, 40, 4, 7, 3, UP2, 0, sk=3, claims=("split:empty-slices", "split:forced:3", "p1:partial"))
    add("s_det", 1, 34, 40, 6, 7, 3, PLAIN, 0, det=True, claims=("split:det", "split:1", "overwrites"))
    add("s_det_forced", 2, 22, 40, 6, 7, 3, PLAIN, 1, sk=3, det=True, claims=("split:det", "split:1"))
    # epilogues, in the kernel (split-K 1) and as the second launch (split-K 2)
    for nm, ep, osc in (("b", (True, False, 0.0, 1.0), False), ("ba", BA, True), ("a", (False, True, 0.2, GAIN), False),
                        ("a0", (False, True, 0.0, 1.0), True)):
        for sk in (1, 2):
            add(f"e_{nm}_sk{sk}", 2, 6, 40, 6, 7, 3, PLAIN, 0, sk=sk, ep=ep, oscale=osc,
                claims=(f"ep:{'bias+act' if nm == 'ba' else 'bias' if nm == 'b' else 'act'}:{'kernel' if sk == 1 else 'deferred'}",))
    add("e_os", 2, 6, 40, 6, 7, 3, PLAIN, 0, oscale=True, claims=("ep:out_scale", "split:1"))
    add("e_os_sk2", 2, 6, 40, 6, 7, 3, PLAIN, 1, oscale=True, sk=2, claims=("ep:out_scale", "split:forced:2"))
    add("e_ba_up", 2, 35, 40, 4, 7, 3, UP2, 0, ep=BA, oscale=True, claims=("ep:bias+act:kernel", "p4:scale"))
    add("e_ba_up_sk2", 2, 35, 40, 4, 7, 3, UP2, 0, ep=BA, oscale=True, sk=2, scale=False, claims=("ep:bias+act:deferred", "p4:noscale"))
    return rows


def _f32_cases():
    rows = []
    add = lambda *a, **kw: rows.append(Mod(*a, route="f32", **kw))      # noqa: E731
    add("m_fwd", 2, 7, 40, 6, 7, 3, PLAIN, 0, oscale=True, claims=("T9:scale", "ep:out_scale", "overwrites"))
    add("m_rev", 2, 7, 40, 6, 7, 3, PLAIN, 1, claims=("T9:scale", "ep:none"))
    add("m_rev_ns", 2, 7, 40, 6, 7, 3, PLAIN, 1, scale=False, oscale=True, claims=("T9:noscale", "ep:out_scale"))
    add("m_up", 2, 35, 40, 4, 7, 3, UP2, 0, oscale=True, ep=BA, promise=True,
        claims=("T4:scale", "T2:scale", "T1:scale", "ep:bias+act:kernel", "promise:y_is_zero", "overwrites"))
    add("m_down", 2, 7, 40, 9, 11, 3, DOWN2, 0, claims=("T9:scale",))
    add("m_up_t", 2, 7, 40, 9, 11, 3, UP2, 1, claims=("T9:scale",))
    add("m_k1_rgb", 2, 35, 3, 6, 7, 1, PLAIN, 0, ep=(True, False, 0.0, 1.0), claims=("T1:scale", "ep:bias:kernel"))
    add("m_noise", 2, 7, 40, 6, 7, 3, PLAIN, 0, oscale=True, ep=BA, noise=True, claims=("noise:kernel", "overwrites"))
    add("m_noise_sk2", 2, 7, 40, 6, 7, 3, PLAIN, 0, oscale=True, ep=BA, noise=True, sk=2, promise=True,
        claims=("noise:deferred", "needs-zero", "promise:y_is_zero"))
    add("m_noise_up", 2, 35, 40, 4, 7, 3, UP2, 0, oscale=True, ep=BA, noise=True, claims=("noise:kernel", "T4:scale"))
    add("m_noise_heur", 1, 34, 40, 6, 7, 3, PLAIN, 0, oscale=True, ep=BA, noise=True, claims=("noise:deferred", "split:heuristic"))
    add("m_heur", 1, 34, 40, 6, 7, 3, PLAIN, 0, oscale=True, promise=True,
        claims=("split:heuristic", "needs-zero", "promise:y_is_zero"))
    add("m_holes", 2, 35, 40, 5, 6, 1, UP2, 0, promise=True, claims=("holes", "needs-zero", "promise:y_is_zero", "T1:scale"))
    add("m_holes_bias", 2, 35, 40, 5, 6, 1, UP2, 0, ep=(True, False, 0.0, 1.0), promise=True,
        claims=("holes", "needs-zero", "ep:bias:deferred", "promise:y_is_zero"))
    add("m_ba_sk2", 2, 7, 40, 6, 7, 3, PLAIN, 0, oscale=True, ep=BA, sk=2, claims=("ep:bias+act:deferred", "needs-zero"))
    add("m_det", 1, 34, 40, 6, 7, 3, PLAIN, 0, oscale=True, det=True, promise=True,
        claims=("split:det", "split:1", "overwrites", "promise:y_is_zero"))
    # the thin 1x1 dispatch: 4 -> 16 channels over 256 x 256 = 2^16 pixels is the smallest eligible call; one step in
    # each argument of thin_conv_eligible leaves it; a noise keeps an eligible shape on the MFMA kernel
    add("thin_yes", 1, 4, 16, 256, 256, 1, PLAIN, 0, scale=False, ep=BA, claims=("thin:just-eligible",))
    add("thin_no_m15", 1, 4, 15, 256, 256, 1, PLAIN, 0, scale=False, ep=BA, claims=("thin:just-not",))
    add("thin_no_cr5", 1, 5, 16, 256, 256, 1, PLAIN, 0, scale=False, ep=BA, claims=("thin:just-not",))
    add("thin_no_px", 1, 4, 16, 256, 255, 1, PLAIN, 0, scale=False, ep=BA, claims=("thin:just-not",))
    add("thin_no_mod4", 1, 4, 16, 257, 257, 1, PLAIN, 0, scale=False, ep=BA, claims=("thin:just-not",))
    add("thin_noise", 1, 4, 16, 256, 256, 1, PLAIN, 0, scale=False, ep=BA, noise=True, claims=("thin:noise-keeps-mfma", "noise:kernel"))
    return rows


F16 = _f16_cases()
F32 = _f32_cases()
BY_NAME = {c.name: c for c in F16 + F32}
assert len(BY_NAME) == len(F16) + len(F32)

# forced tiles x split-K, one base case per body of the fp16 kernel (name -> the bodies it runs); the fourth split-K
# count is one above the smallest ktiles16 of the case and within the fp32 kt_min, so that it leaves empty slices
SWEEP = {
    "sw_quad": (Mod("sw_quad", 2, 14, 70, 6, 7, 3, PLAIN, 0), ("quad",)),
    "sw_quad_rev": (Mod("sw_quad_rev", 2, 14, 70, 5, 4, 3, PLAIN, 1, scale=False), ("quad",)),
    "sw_narrow": (Mod("sw_narrow", 3, 20, 70, 5, 3, 3, PLAIN, 0), ("narrow",)),
    "sw_poly": (Mod("sw_poly", 2, 70, 70, 4, 7, 3, UP2, 0), ("p4", "p2", "p1")),
    "sw_p1": (Mod("sw_p1", 2, 70, 70, 6, 7, 1, PLAIN, 0, scale=False), ("p1",)),
}
SWEEP_TILES = (0, 1, 2)
BY_NAME.update({name: c for name, (c, _) in SWEEP.items()})


def sweep_splits(c):
    return (1, 2, 3, min(c.plan(tile=2, sk=1)["ktiles16"]) + 1)


# ------------------------------------------------------------------------------------------------------ operands
def _rng(name):
    return np.random.default_rng([20261, zlib.crc32(name.encode())])


def _floored(a):
    """Every |a| below 2^-8 moved out to +-2^-8."""
    a = a.astype(np.float32)
    small = np.abs(a) < FLOOR_OPERAND
    return np.where(small, np.where(a < 0, -FLOOR_OPERAND, FLOOR_OPERAND), a).astype(np.float32)


def _scales(rng, shape):
    return np.clip(1 + 0.3 * rng.standard_normal(shape), 0.4, 1.6).astype(np.float32)


def operands(c):
    """x [B, Cr, H, W], w [Cout, Cin, k, k] (the forward layout, whatever `transpose`), s [B, Cr] or None, os [B, M] or
    None, bias [M], noise [oh, ow], noise_w [1]."""
    rng = _rng(c.name)
    oh, ow = c.out_hw
    x = _floored(rng.standard_normal((c.B, c.Cr, c.H, c.W)))
    w = _floored(rng.standard_normal((c.Cout, c.Cin, c.k, c.k)))
    s = _scales(rng, (c.B, c.Cr))
    os_ = _scales(rng, (c.B, c.M))
    bias = rng.standard_normal(c.M).astype(np.float32)
    noise = rng.standard_normal((oh, ow)).astype(np.float32)
    noise_w = np.array([0.7], np.float32)
    return dict(x=x, w=w, s=s if c.scale else None, os=os_ if c.oscale else None, bias=bias, noise=noise, noise_w=noise_w)


def truncate_f16(a):
    """float32 -> the half of no larger magnitude (normal range): the float32 with its low 13 mantissa bits cleared."""
    bits = np.ascontiguousarray(a, np.float32).view(np.uint32) & np.uint32(0xFFFFE000)
    return bits.view(np.float32)


def f16_images(c, op, how="contract"):
    """The two GEMM operands of the fp16 route as float64.  how: contract = float16(float32(x) * float32(s)) and
    float16(w), round to nearest even; the mutants: unrounded, scale-after-round (float16(x) * s), truncate (toward zero)."""
    x, w, s = op["x"], op["w"], op["s"]
    sb = None if s is None else s[:, :, None, None]
    if how == "unrounded":
        return (x.astype(np.float64) if s is None else x.astype(np.float64) * sb), w.astype(np.float64)
    if how == "scale-after-round":
        xr = x.astype(np.float16).astype(np.float64)
        return (xr if s is None else xr * sb), w.astype(np.float16).astype(np.float64)
    xs = x if s is None else x * sb                     # float32 product
    assert xs.dtype == np.float32
    if how == "truncate":
        return truncate_f16(xs).astype(np.float64), truncate_f16(w).astype(np.float64)
    assert how == "contract"
    return xs.astype(np.float16).astype(np.float64), w.astype(np.float16).astype(np.float64)


def f32_images(c, op):
    x, w, s = op["x"].astype(np.float64), op["w"].astype(np.float64), op["s"]
    return (x if s is None else x * s[:, :, None, None].astype(np.float64)), w


def n_map(c, pl):
    """Reduction length Cr * T of every output position's class; 0 in a hole."""
    n = np.zeros((pl["OHf"], pl["OWf"]))
    step = c.s if c.adj else 1
    for cl in pl["classes"]:
        n[cl["oy0"]::step, cl["ox0"]::step] = c.Cr * cl["T"]
    return n


def finish(c, op, sums, dtype=np.float64):
    """out_scale * sums, + noise_w * noise, then the tail (bias, leaky-ReLU, gain)."""
    v = np.asarray(sums, dtype)
    if op["os"] is not None:
        v = v * op["os"].astype(dtype)[:, :, None, None]
    if c.noise:
        v = v + (op["noise_w"].astype(dtype)[0] * op["noise"].astype(dtype))[None, None]
    if c.ep is not None:
        v = cc.tail(v, op["bias"], c.ep, dtype)
    return v


def reference(c, op, xr, wr):
    return finish(c, op, cc.conv_reference(xr, wr, c))


def extra_roundings(c):
    return (int(c.route == "f32" and c.scale) + int(c.oscale) + (3 if c.ep is not None and (c.ep[0] or c.ep[1]) else 0)
            + (2 if c.noise else 0))


def numbers(c, op):
    """ref, cap, e32, r32 of one case on its operands."""
    import torch
    xr, wr = f16_images(c, op) if c.route == "f16" else f32_images(c, op)
    ref = reference(c, op, xr, wr)
    terms = cc.conv_reference(np.abs(xr), np.abs(wr), c)
    if op["os"] is not None:
        terms = terms * np.abs(op["os"].astype(np.float64))[:, :, None, None]
    if c.ep is not None and c.ep[0]:
        terms = terms + np.abs(op["bias"].astype(np.float64))[None, :, None, None]
    if c.noise:
        terms = terms + np.abs(op["noise_w"].astype(np.float64)[0] * op["noise"].astype(np.float64))[None, None]
    gain = max(c.ep[3], 1.0) if c.ep is not None and c.ep[1] else 1.0
    cap = gain * (n_map(c, c.plan())[None, None] + extra_roundings(c)) * EPS32 * terms
    # torch's float32 evaluation of the same operation: the fp16 images are float32 numbers; the fp32 route's scale
    # product is a float32 product
    if c.route == "f16":
        x32, w32 = xr.astype(np.float32), wr.astype(np.float32)
    else:
        x32 = op["x"] if op["s"] is None else op["x"] * op["s"][:, :, None, None]
        w32 = op["w"]
    r32 = finish(c, op, cc._torch_conv_f32(x32, w32, c, torch.float32), np.float32)
    assert r32.dtype == np.float32
    return ref, cap, cc.rel_err(r32, ref), r32


@functools.lru_cache(maxsize=None)
def data(name):
    """The operands of a case (table or sweep) with ref, cap, e32 and r32, computed once and read-only."""
    c = BY_NAME[name]
    op = operands(c)
    ref, cap, e32, r32 = numbers(c, op)
    return cc._freeze(dict(op, ref=ref, cap=cap, e32=e32, r32=r32))


def ratio_of(pl):
    """RATIO on every path: the largest measured error is 1.75 x e32 (module docstring)."""
    return RATIO


def case_bound(name, pl=None):
    dt = data(name)
    return cc.bound(dt["ref"], dt["e32"], dt["cap"], ratio_of(pl if pl is not None else BY_NAME[name].plan()))


# ------------------------------------------------------------------------------------------------------- mutants
def _drop_channels(a, lo, axis=1):
    a = a.copy()
    idx = [slice(None)] * a.ndim
    idx[axis] = slice(lo, None)
    a[tuple(idx)] = 0.0
    return a


def _w_channel_axis(c):
    return 0 if c.tr else 1         # w is [Cout, Cin, k, k]; the reduction runs over Cout in a transposed call


def mutants(c, op):
    """name -> (labels the mutant targets, mutated reference in float64): what a subtly wrong fp16 kernel would compute.
    A mutant applies to a row that claims one of its labels (an empty tuple: every fp16 row)."""
    xr, wr = f16_images(c, op)
    pl = c.plan()
    out = {}
    for how in ("unrounded", "truncate") + (("scale-after-round",) if c.scale else ()):
        out[how] = ((), reference(c, op, *f16_images(c, op, how)))
    # a border tap of a kernel row lost in the first / last output column of the stride-1 quad form: the input column
    # that the shifted triple supplies there (0 and 1 on the left, W - 1 and W - 2 on the right)
    if "quad" in pl["bodies"] and c.s == 1:
        sums = cc.conv_reference(xr, wr, c)
        for col, src in ((0, 0), (0, 1), (c.W - 1, c.W - 1), (c.W - 1, c.W - 2)):
            only = np.zeros_like(xr)
            only[..., src] = xr[..., src]
            m = sums.copy()
            m[..., col] -= cc.conv_reference(only, wr, c)[..., col]
            out[f"border-tap:{col}<-{src}"] = (("quad:W4", "quad:W5+", "quad:rev"), finish(c, op, m))
        if c.adj:       # the adjoint's triple not reversed: the outer taps of every kernel row change places
            out["rev-not-swapped"] = (("quad:rev",), reference(c, op, xr, np.ascontiguousarray(wr[..., ::-1])))
    for body in sorted(set(pl["bodies"])):
        cpt = body_cpt(body)
        kt = cdiv(c.Cr, cpt)
        last0 = (kt - 1) * cpt      # first channel of the body's last K tile
        if c.Cr % cpt and c.Cr > cpt and c.scale:
            xs = op["x"].copy()
            xs[:, :last0] *= op["s"][:, :last0, None, None]
            out[f"scale-dropped:{body}"] = ((f"{body}:partial",), reference(c, op, xs.astype(np.float16).astype(np.float64), wr))
        if kt > 1:
            targets = (f"{body}:partial", "split:heuristic", "split:forced", "split:clipped", "split:empty-slices", "split:det")
            out[f"last-tile-omitted:{body}"] = (targets, reference(c, op, _drop_channels(xr, last0), wr))
    return out
