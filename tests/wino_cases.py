"""Case tables of tests/test_wino_cases_cpu.py and tests/test_gpu_wino_paths.py: g2s_wino_weights + g2s_conv3x3_wino
(csrc/winograd.hip, Winograd F(2x2, 3x3)) and g2s_wino4_weights + g2s_conv3x3_wino4 + g2s_wino4_supported
(csrc/winograd4.hip, F(4x4, 3x3)), with csrc/split_reduce.hip behind both, at shapes that reach every launch path,
against a float64 reference written from the formula of include/g2s.h.  Importable without a GPU.

plan_wino restates the host code of g2s_conv3x3_wino, plan_wino4 that of g2s_conv3x3_wino4, supported4 the gate
g2s_wino4_supported; `labels` / `labels4` name what a plan reaches.  Every table row carries the labels it is meant to
reach (`claims`) and tests/test_wino_cases_cpu.py holds the plans to them.

Labels of an F(2x2) launch (wino_kernel<SCALE, PARTIAL, FAST>):
  scale / noscale                in_scale (and out_scale) given or NULL
  K:full / K:partial / K:sub     Cr a multiple of the 4-channel K tile, not one, or below one tile
  fast / slow                    FAST: W even and TW = ceil(W / 2) divides 64 (two-column loads + lane exchange)
  W-odd H-odd                    a last tile column / row of one pixel;  slow:W-even: float2 stores without the exchange
  TW1                            W = 2: first and last tile column are the same lane;  TW>64: a tile row longer than a block
  M<64 M%64 N%64                 ragged channel block; B TH TW not a multiple of the 64-tile block
  spans-batch                    a 64-tile block holds tiles of two samples whose in_scale / out_scale differ by 16x
  ktiles1 ktiles2 ktiles3        reductions shorter than the pipeline prologue (U ring of three)
  whole                          one workgroup per tile, nothing to add up
  persistent (+ :tiles%8)        >= 512 whole tiles: 256 workgroups walk them (d.rr); the XCD chunks are ragged
  splitk:ws                      K slices store side by side in the workspace, split_reduce adds them
  splitk:atomic:no-ws / :ws-small / :>8     K slices meet by float atomics in a y the library clears, and why
  splitk:clipped / splitk:rounded           splitk cut to ktiles / rounded so that no slice is empty
  streamk:forced / streamk:library          equal runs of (tile, K tile) units: splitk < 0, or splitk = 0 at fill < 0.9
  streamk:ws                     runs store to slots, wino_streamk_reduce_kernel adds them
  streamk:atomic:no-ws / :W-odd / :slots>8  runs meet by float atomics, and why
  streamk:whole-tile-inside      one run holds a whole tile next to a share of a split one (parts == 1 in the reduce)
  streamk:run-crosses-tiles      a run holds units of two tiles or more
  det:fallback-whole / det:keeps-ws         the deterministic flag turns atomics into whole tiles / keeps workspace paths
  epilogue:none / kernel / reduce / streamk-reduce / deferred:bias-act / deferred:noise    where the tail runs
  bias-only act-only bias-act noise         what the tail holds;  reduce:scalar: B M H W % 4 != 0 (split_reduce's scalar branch)
  fwd / transpose                g2s_wino_weights(transpose): flipped taps, swapped channel roles

Labels of an F(4x4) launch: scale / noscale, TW1 .. TW32, blocks-per-image>1, M128, ktiles1..3, Cr512, whole,
splitk:library / forced / clipped / rounded, splitk:dropped:no-ws / :ws-small / :>8 (the launch falls back to whole
tiles), epilogue:none / kernel / reduce (+ :noise), bias-only act-only bias-act noise noise-no-bias, fwd / transpose.
SUPPORTED: (B, Cr, M, H, W) -> 0 / 1, one rejected shape per clause of g2s_wino4_supported and its nearest accepted
neighbour.

Reference.  y = gain * act(out_scale * conv3x3_pad1(in_scale * x, w) + noise_w * noise + bias) in float64 with the
shifted-slice sums of conv2d_cases.conv_reference (gain only with act, as the entry points apply it); the transposed form
through w'(i, o, ky, kx) = w(o, i, 2 - ky, 2 - kx).  Inputs are seeded N(0, 1) draws rounded to float32, weights scaled
by 1 / sqrt(9 Cr) and without symmetry, bias and noise N(0, 1), noise_w 0.7.  With B > 1 the scales of sample b carry
a factor 4^(+-1) (in_scale x 0.25 / x 4, out_scale x 4 / x 0.25, alternating): a block that takes its neighbour's scale
misses by a factor of 16.

Bound, per element: |kernel - ref| <= min(ratio * e32w * max|ref|, cap).
  e32w  error of a plain numpy float32 evaluation of the same Winograd algorithm (wino_eval: the three transforms as
        matrix products; F(2x2): 0, +-1, +-1/2, U in float32; F(4x4): the Lavin-Gray points 0, +-1, +-2, inf, U in double
        and rounded once) against the float64 reference as a share of max|ref|, floored at half a float32 spacing.
  cap   (Cr + c) eps32 |A^T| [ sum_c (|G| |g_c| |G^T|) .* (|B^T| |s d_c| |B|) ] |A| |out_scale|: wino_eval on absolute
        values with absolute matrices.  c counts the transform roundings of one product chain u v -> y, for ANY
        evaluation of a transform as a matrix product: a row with r non-zeros costs a term at most r roundings (its
        multiplication and r - 1 additions), once per axis.
          F(2x2): G rows hold <= 3 non-zeros: 6;  B^T rows 2: 4, + 1 for in_scale;  A^T rows 3: 6, + 1 for out_scale: c = 18
          F(4x4): U is rounded once: 1;  B^T rows 4: 8, + 1;  A^T rows 5: 10, + 1: c = 21  (the kernel's own chain is
          shorter: 2 fused steps per axis of B^T, 2 per axis of A^T and 3 additions where the four quadrants meet)
        The Cr term is the accumulation: a product passes at most Cr additions however the reduction is cut (a K slice or
        stream-K run holds at least one K tile, so what the slices' meeting adds, slices - 1, it saves in the chains).
        With an epilogue: max(gain, 1) (Cr + c + 3) eps32 (that sum + |bias| + |noise_w noise|), as conv2d_cases.py.
  Cases with a leaky-ReLU use the same bound on the float64 tail; no element is left out.
  ratio conv2d_cases.RATIO = 4 on every path: no path measured above 2, see the table.

Measured on an MI355X on 2026-10-20, largest error / (e32w * max|ref|) over the rows of a path (e32w floored; e32w is
1.3e-7 .. 6e-7 for F(2x2) and 2e-6 .. 1.7e-5 for F(4x4), whose constants amplify the rounding), and the largest error / cap
of any row of the path:

    g2s_conv3x3_wino    rows   ratio   error / cap        g2s_conv3x3_wino4   rows   ratio   error / cap
    whole                 43    1.59         0.021        whole                 26    1.54         0.004
    persistent             3    0.97         0.014        split-K (reduce)      14    0.95         0.002
    split-K workspace     16    1.67         0.005
    split-K atomics        7    0.81         0.002
    stream-K workspace    10    1.10         0.005
    stream-K atomics      10    1.03         0.005
    deterministic flag    20    1.16         0.005

No path is above 2, so every path gets RATIO = 4 (ratio_of); the launches of modconv.py's launch site (0.38 .. 1.06) and the
pre-filled launches of test_wino_plan_holds_on_the_device (at most 1.16) lie inside the same figures.  The cap is 50 to
500 times wider than what the kernels do: it is the backstop for elements whose terms are small, not the working bound.
"""
import functools
import zlib

import numpy as np

import conv2d_cases as cc
from conv2d_cases import EPS32, GAIN, RATIO, cdiv

ALPHA = 0.2
NOISE_W = 0.7
NCU = 256
SPLIT_REDUCE_MAX = 8
C_ROUNDINGS = {2: 18, 4: 21}

# the transforms: B^T (input), G (weights), A^T (output) of F(2x2, 3x3) and F(4x4, 3x3) (Lavin & Gray 2016, section 4)
MATS = {
    2: (np.array([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], np.float64),
        np.array([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]], np.float64),
        np.array([[1, 1, 1, 0], [0, 1, -1, -1]], np.float64)),
    4: (np.array([[4, 0, -5, 0, 1, 0], [0, -4, -4, 1, 1, 0], [0, 4, -4, -1, 1, 0], [0, -2, -1, 2, 1, 0],
                  [0, 2, -1, -2, 1, 0], [0, 4, 0, -5, 0, 1]], np.float64),
        np.array([[1 / 4, 0, 0], [-1 / 6, -1 / 6, -1 / 6], [-1 / 6, 1 / 6, -1 / 6], [1 / 24, 1 / 12, 1 / 6],
                  [1 / 24, -1 / 12, 1 / 6], [0, 0, 1]], np.float64),
        np.array([[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 0], [0, 1, 1, 4, 4, 0], [0, 1, -1, 8, -8, 1]], np.float64)),
}


# ------------------------------------------------------------------------------------------------------- plans
def plan_wino(B, Cr, M, H, W, splitk=0, ws_floats=None, det=False, has_epilogue=False):
    """What g2s_conv3x3_wino decides for one call: ws_floats None = no workspace."""
    assert B > 0 and Cr > 0 and M > 0 and H >= 2 and W >= 2
    TH, TW = cdiv(H, 2), cdiv(W, 2)
    ktiles = cdiv(Cr, 4)
    ntiles = B * TH * TW
    tiles_m = cdiv(M, 64)
    tiles = tiles_m * cdiv(ntiles, 64)
    units = tiles * ktiles
    y_floats = B * M * H * W
    asked = splitk
    have_ws = ws_floats is not None
    whole = splitk == 1 or (splitk == 0 and tiles / (cdiv(tiles, NCU) * NCU) >= 0.9)
    if whole and tiles >= 2 * NCU:
        splitk = -10000 - NCU
    upw, grid_x, use_part, streamk_part, why, slots = 0, tiles, False, False, None, 0
    clipped = rounded = False
    if splitk > 0:
        s1 = min(splitk, ktiles)
        s2 = cdiv(ktiles, cdiv(ktiles, s1))
        clipped, rounded, splitk = s1 < splitk, s2 != s1, s2
        partial_sums = splitk > 1
        mode = "splitk" if partial_sums else "whole"
        if partial_sums:
            why = ("no-ws" if not have_ws else ">8" if splitk > SPLIT_REDUCE_MAX
                   else "ws-small" if splitk * y_floats > ws_floats else None)
            use_part = why is None
    elif splitk <= -10000:
        mode, grid_x, splitk, partial_sums = "persistent", NCU, 1, False
    elif splitk < 0:
        upw = cdiv(units, min(-splitk, units))
        grid_x, splitk, partial_sums, mode = cdiv(units, upw), 1, True, "streamk:forced"
    else:
        splitk = 1
        fill = tiles / (cdiv(tiles, NCU) * NCU)
        if fill < 0.9 and cdiv(units, NCU) >= 4:
            upw = cdiv(units, NCU)
            grid_x = cdiv(units, upw)
        partial_sums = upw != 0
        mode = "streamk:library" if upw else "whole"
    if upw:
        slots = cdiv(ktiles, upw) + 1
        why = ("no-ws" if not have_ws else "W-odd" if W % 2 else "slots>8" if slots > SPLIT_REDUCE_MAX
               else "ws-small" if slots * y_floats > ws_floats else None)
        streamk_part = use_part = why is None
    det_fallback = bool(det and partial_sums and not use_part)
    planned = mode
    if det_fallback:
        splitk, grid_x, upw, partial_sums, mode = 1, tiles, 0, False, "whole"
    deferred = partial_sums and not streamk_part and has_epilogue
    slices = splitk if mode == "splitk" else slots if upw else 0
    out = dict(TH=TH, TW=TW, ktiles=ktiles, ntiles=ntiles, tiles_m=tiles_m, tiles=tiles, units=units, y_floats=y_floats,
               asked=asked, mode=mode, planned=planned, splitk=splitk, upw=upw, grid_x=grid_x, partial_sums=partial_sums,
               use_part=use_part, streamk_part=streamk_part, why_atomic=None if (use_part or not partial_sums) else why,
               why_planned=why, slots=slots, slices=slices, clipped=clipped, rounded=rounded, det_fallback=det_fallback,
               det_keeps_ws=bool(det and partial_sums and use_part), deferred=deferred,
               clears_y=partial_sums and not use_part, uses_ws=use_part,
               partial=Cr % 4 != 0, fast=TW <= 64 and 64 % TW == 0 and W % 2 == 0)
    if upw:
        parts = np.array([(t * ktiles + ktiles - 1) // upw - (t * ktiles) // upw + 1 for t in range(tiles)])
        runs = [(g * upw, min(units, (g + 1) * upw)) for g in range(grid_x)]
        inside = False
        for u0, u1 in runs:
            first, last = -(-u0 // ktiles), u1 // ktiles         # whole tiles of this run: first .. last - 1
            if last > first and (u0 % ktiles or u1 % ktiles):
                inside = True
        out.update(parts=parts, whole_tile_inside=inside,
                   run_crosses=any((u1 - 1) // ktiles > u0 // ktiles for u0, u1 in runs))
        # floats of the workspace the runs write: the outputs of every split tile, once per run that shares it
        n = np.arange(ntiles)
        r = n % (TH * TW)
        px = (1 + (2 * (r // TW) + 1 < H)) * (1 + (2 * (r % TW) + 1 < W))
        px_block = np.add.reduceat(px, np.arange(0, ntiles, 64))
        t = np.arange(tiles)
        m_count = np.minimum(64, M - 64 * (t % tiles_m))
        out["ws_written"] = int((np.where(parts > 1, parts, 0) * m_count * px_block[t // tiles_m]).sum()) if streamk_part else 0
    elif mode == "splitk":
        out["ws_written"] = splitk * y_floats if use_part else 0
    else:
        out["ws_written"] = 0
    return out


W4_CLAUSES = ("positive", "multiple", "TW", "block", "Cr512", "offsets", "weights")


def supported4(B, Cr, M, H, W):
    """g2s_wino4_supported, clause by clause: (0 / 1, the clause that rejects)."""
    if B <= 0 or Cr <= 0 or M <= 0 or H < 4 or W < 4:
        return 0, "positive"
    if H % 4 or W % 4 or M % 64 or Cr % 4:
        return 0, "multiple"
    TW = W // 4
    if TW > 32 or 32 % TW:
        return 0, "TW"
    if ((H // 4) * TW) % 32:
        return 0, "block"
    if Cr > 512:
        return 0, "Cr512"
    if B * Cr * H * W >= 1 << 29 or B * M * H * W >= 1 << 29:
        return 0, "offsets"
    if cdiv(M, 64) * cdiv(Cr, 4) * 36 * 4 * 64 >= 1 << 29:
        return 0, "weights"
    return 1, None


def plan_wino4(B, Cr, M, H, W, splitk=0, ws_floats=None):
    ok, clause = supported4(B, Cr, M, H, W)
    if not ok:
        return dict(supported=0, clause=clause)
    TH, TW = H // 4, W // 4
    ktiles = Cr // 4
    tiles = (M // 64) * cdiv(B * TH * TW, 32)
    y_floats = B * M * H * W
    asked, source = splitk, "forced"
    if splitk <= 0:
        splitk, source = 1, "library"
        if tiles < NCU:
            want = min(NCU // tiles, SPLIT_REDUCE_MAX)
            if want >= 2 and ktiles // want >= 16:
                splitk = want
    s1 = min(splitk, ktiles)
    s2 = cdiv(ktiles, cdiv(ktiles, s1))
    clipped, rounded, splitk = s1 < splitk, s2 != s1, s2
    dropped = None
    if splitk > 1:
        dropped = ("no-ws" if ws_floats is None else ">8" if splitk > SPLIT_REDUCE_MAX
                   else "ws-small" if splitk * y_floats > ws_floats else None)
    wanted = splitk
    if dropped:
        splitk = 1
    return dict(supported=1, TH=TH, TW=TW, ktiles=ktiles, tiles=tiles, y_floats=y_floats, asked=asked, source=source,
                splitk=splitk, wanted=wanted, clipped=clipped, rounded=rounded, dropped=dropped, slices=splitk if splitk > 1 else 0,
                mode="splitk" if splitk > 1 else "whole", uses_ws=splitk > 1, ws_written=splitk * y_floats if splitk > 1 else 0)


# ------------------------------------------------------------------------------------------------------- cases
class Wino:
    """One g2s_conv3x3_wino (kind 2) or g2s_conv3x3_wino4 (kind 4) call.  sk: the splitk argument; ws: "exact" (as many
    floats as the planned path needs), "short" (one fewer) or "none"; scale: in_scale and out_scale given; ep: None or
    (bias, act, noise) with leaky-ReLU 0.2 and gain sqrt(2); tr: the transposed weight transform (w is [Cr, M, 3, 3])."""

    def __init__(self, name, B, Cr, M, H, W, sk=0, ws="exact", scale=True, ep=None, tr=False, det=False, kind=2, claims=()):
        self.name, self.B, self.Cr, self.M, self.H, self.W, self.sk, self.ws = name, B, Cr, M, H, W, sk, ws
        self.scale, self.ep, self.tr, self.det, self.kind, self.claims = scale, ep, tr, det, kind, tuple(claims)
        assert ws in ("exact", "short", "none")
        assert ep is None or kind == 4 or not ep[2] or (ep[0] and ep[1])      # g2s_conv3x3_wino: a noise needs bias and act

    @property
    def y_floats(self):
        return self.B * self.M * self.H * self.W

    def _plan(self, sk, ws_floats, det):
        if self.kind == 2:
            return plan_wino(self.B, self.Cr, self.M, self.H, self.W, sk, ws_floats, det, self.ep is not None)
        return plan_wino4(self.B, self.Cr, self.M, self.H, self.W, sk, ws_floats)

    def ws_floats(self, sk=None):
        """The workspace of this row: what its path needs with room to spare taken away, one float less, or None."""
        sk = self.sk if sk is None else sk
        if self.ws == "none":
            return None
        p = self._plan(sk, 1 << 62, False)
        need = (p["wanted"] if self.kind == 4 else (p["splitk"] if p["mode"] == "splitk" else p["slots"])) * self.y_floats
        if self.kind == 4 and p["wanted"] <= 1 or self.kind == 2 and not p["partial_sums"]:
            return None
        return need - 1 if self.ws == "short" else need

    def plan(self, sk=None, det=None):
        sk = self.sk if sk is None else sk
        return self._plan(sk, self.ws_floats(sk), self.det if det is None else det)

    def __repr__(self):
        return (f"{self.name}: F({self.kind}x{self.kind}) B{self.B} Cr{self.Cr} M{self.M} {self.H}x{self.W} sk{self.sk} ws:{self.ws} "
                f"scale{int(self.scale)} ep{self.ep} tr{int(self.tr)} det{int(self.det)}")


def _content(ep):
    bias, act, noise = ep
    if noise:
        return "noise" if bias else "noise-no-bias"
    return "bias-act" if bias and act else "bias-only" if bias else "act-only"


def labels(c, p):
    out = {"scale" if c.scale else "noscale", "K:sub" if c.Cr < 4 else "K:partial" if c.Cr % 4 else "K:full",
           "fast" if p["fast"] else "slow", "transpose" if c.tr else "fwd"}
    if c.W % 2:
        out.add("W-odd")
    if c.H % 2:
        out.add("H-odd")
    if not p["fast"] and c.W % 2 == 0:
        out.add("slow:W-even")
    if p["TW"] == 1:
        out.add("TW1")
    if p["TW"] > 64:
        out.add("TW>64")
    if c.M < 64:
        out.add("M<64")
    elif c.M % 64:
        out.add("M%64")
    if p["ntiles"] % 64:
        out.add("N%64")
    if c.scale and any((b * p["TH"] * p["TW"]) % 64 for b in range(1, c.B)):
        out.add("spans-batch")
    if p["ktiles"] <= 3:
        out.add(f"ktiles{p['ktiles']}")
    mode = p["mode"]
    if mode == "whole":
        out.add("whole")
    if mode == "persistent":
        out.add("persistent")
        if p["tiles"] % 8:
            out.add("persistent:tiles%8")
    if p["planned"] == "splitk":
        out.add("splitk:ws" if p["use_part"] else f"splitk:atomic:{p['why_planned']}")
    if p["clipped"]:
        out.add("splitk:clipped")
    if p["rounded"]:
        out.add("splitk:rounded")
    if p["planned"].startswith("streamk"):
        out.add(p["planned"])
        out.add("streamk:ws" if p["streamk_part"] else f"streamk:atomic:{p['why_planned']}")
        if "parts" in p:
            if p["whole_tile_inside"]:
                out.add("streamk:whole-tile-inside")
            if p["run_crosses"]:
                out.add("streamk:run-crosses-tiles")
    if p["det_fallback"]:
        out.add("det:fallback-whole")
    if p["det_keeps_ws"]:
        out.add("det:keeps-ws")
    if c.ep is None:
        out.add("epilogue:none")
    else:
        out.add(_content(c.ep))
        if not p["partial_sums"]:
            out.add("epilogue:kernel")
        elif p["streamk_part"]:
            out.add("epilogue:streamk-reduce")
        elif p["use_part"]:
            out.add("epilogue:reduce")
        else:
            out.add("epilogue:deferred:noise" if c.ep[2] else "epilogue:deferred:bias-act")
    if p["use_part"] and not p["streamk_part"] and p["y_floats"] % 4:
        out.add("reduce:scalar")
    return out


def labels4(c, p):
    out = {"scale" if c.scale else "noscale", f"TW{p['TW']}", "transpose" if c.tr else "fwd"}
    if (p["TH"] * p["TW"]) // 32 > 1:
        out.add("blocks-per-image>1")
    if c.M == 128:
        out.add("M128")
    if p["ktiles"] <= 3:
        out.add(f"ktiles{p['ktiles']}")
    if c.Cr == 512:
        out.add("Cr512")
    if p["splitk"] == 1:
        out.add("whole")
    if p["wanted"] > 1:
        out.add(f"splitk:{p['source']}")
    if p["clipped"]:
        out.add("splitk:clipped")
    if p["rounded"]:
        out.add("splitk:rounded")
    if p["dropped"]:
        out.add(f"splitk:dropped:{p['dropped']}")
    if c.ep is None:
        out.add("epilogue:none")
    else:
        out.add(_content(c.ep))
        place = "epilogue:reduce" if p["splitk"] > 1 else "epilogue:kernel"
        out.add(place)
        if c.ep[2]:
            out.add(place + ":noise")
    return out


def case_labels(c, p=None):
    p = c.plan() if p is None else p
    return labels(c, p) if c.kind == 2 else labels4(c, p)


def path_of(c, p=None):
    """The row of the measured table a launch belongs to."""
    p = c.plan() if p is None else p
    if c.kind == 4:
        return "wino4/" + p["mode"]
    if c.det and (p["det_fallback"] or p["det_keeps_ws"]):
        return "wino/det"
    if p["mode"] in ("whole", "persistent"):
        return "wino/" + p["mode"]
    kind = "splitk" if p["mode"] == "splitk" else "streamk"
    return f"wino/{kind}/{'ws' if p['use_part'] else 'atomic'}"


EPS = {"b": (True, False, False), "a": (False, True, False), "ba": (True, True, False), "n": (True, True, True)}


def _wino_cases():
    rows = []
    add = lambda *a, **kw: rows.append(Wino(*a, **kw))      # noqa: E731
    # templates and geometry.  B2 x 3 x 4 tiles: one ragged block that holds both samples
    add("t_fast", 2, 8, 40, 6, 8, 1, claims=("scale", "K:full", "fast", "M<64", "N%64", "spans-batch", "ktiles2", "whole", "fwd", "epilogue:none"))
    add("t_fast_noscale", 2, 8, 40, 6, 8, 1, scale=False, claims=("noscale", "fast"))
    add("t_slow", 2, 6, 40, 7, 9, 1, claims=("scale", "K:partial", "slow", "W-odd", "H-odd", "spans-batch"))
    add("t_slow_noscale", 2, 6, 40, 7, 9, 1, scale=False, claims=("noscale", "K:partial", "slow"))
    add("t_sub", 2, 3, 40, 6, 8, 1, claims=("K:sub", "ktiles1", "fast"))
    add("t_sub_slow", 2, 2, 40, 7, 9, 1, scale=False, claims=("K:sub", "ktiles1", "slow", "noscale"))
    add("t_partial_fast", 2, 10, 40, 6, 8, 1, scale=False, claims=("K:partial", "fast", "noscale", "ktiles3"))
    add("g_slow_weven", 2, 8, 40, 6, 12, 1, claims=("slow:W-even", "K:full"))
    add("g_hodd_weven", 2, 8, 40, 7, 12, 1, claims=("slow:W-even", "H-odd"))
    add("g_hodd_fast", 2, 8, 40, 7, 8, 1, claims=("fast", "H-odd"))
    add("g_tw1", 3, 8, 40, 6, 2, 1, claims=("TW1", "fast", "spans-batch"))
    add("g_tw1_long", 2, 8, 40, 70, 2, 1, claims=("TW1", "fast", "spans-batch"))      # 35 tiles per sample: 2 blocks
    add("g_tw65", 1, 8, 40, 4, 130, 1, claims=("TW>64", "slow:W-even"))
    add("g_tw66_odd", 2, 5, 40, 3, 131, 1, claims=("TW>64", "W-odd", "H-odd", "K:partial", "spans-batch"))
    add("g_tw64", 1, 8, 40, 4, 128, 1, claims=("fast",))
    add("g_m70", 2, 8, 70, 6, 8, 1, claims=("M%64",))
    add("g_m130_n", 3, 8, 130, 10, 12, 1, claims=("M%64", "N%64", "spans-batch", "slow:W-even"))       # 3 x 30 tiles: 2 blocks
    add("g_m64_n64", 2, 8, 64, 8, 16, 1, claims=("fast", "whole"))                  # 2 x 32 tiles: one full block
    for Cr in (4, 8, 12, 1, 7, 9):
        add(f"k_cr{Cr}", 2, Cr, 40, 6, 8, 1, claims=(f"ktiles{cdiv(Cr, 4)}", "K:partial" if Cr % 4 else "K:full") if Cr >= 4 else ("ktiles1", "K:sub"))
        add(f"k_cr{Cr}_slow", 2, Cr, 40, 5, 7, 1, scale=False, claims=(f"ktiles{cdiv(Cr, 4)}", "slow"))
    # the library's own choice on a small launch: whole tiles
    add("p_lib_whole", 2, 32, 40, 6, 8, 0, claims=("whole",))
    # split-K: 8 K tiles
    add("p_sk_ws", 2, 32, 40, 6, 8, 4, claims=("splitk:ws", "epilogue:none"))
    add("p_sk_ws_slow", 1, 30, 70, 7, 9, 3, claims=("splitk:ws", "reduce:scalar", "W-odd", "K:partial", "M%64"))   # slices of 3, 3, 2 K tiles
    add("p_sk_nows", 2, 32, 40, 6, 8, 4, ws="none", claims=("splitk:atomic:no-ws",))
    add("p_sk_short", 2, 32, 40, 6, 8, 4, ws="short", claims=("splitk:atomic:ws-small",))
    add("p_sk_gt8", 2, 48, 40, 6, 8, 12, claims=("splitk:atomic:>8",))
    add("p_sk_8", 2, 32, 40, 6, 8, 20, claims=("splitk:clipped", "splitk:ws"))
    add("p_sk_rounded", 2, 32, 40, 6, 8, 5, claims=("splitk:rounded", "splitk:ws"))      # 5 -> per 2 -> 4
    add("p_sk_clip1", 2, 3, 40, 6, 8, 4, claims=("splitk:clipped", "whole", "ktiles1"))
    add("p_sk_scalar", 1, 8, 5, 3, 3, 2, claims=("reduce:scalar", "splitk:ws", "W-odd"))
    add("p_sk_scalar_even", 1, 8, 3, 3, 2, 2, claims=("reduce:scalar", "splitk:ws", "TW1"))            # 18 floats, float2 slots
    add("p_sk_ws_m130", 3, 12, 130, 10, 12, 3, claims=("splitk:ws", "M%64", "N%64", "ktiles3"))
    # stream-K, forced.  3 tiles x 8 K tiles over 5 runs of 5: every tile split, every run but the last crosses
    add("s_ws", 2, 32, 130, 6, 8, -5, claims=("streamk:forced", "streamk:ws", "streamk:run-crosses-tiles"))
    add("s_nows", 2, 32, 130, 6, 8, -5, ws="none", claims=("streamk:forced", "streamk:atomic:no-ws"))
    add("s_wodd", 2, 32, 130, 6, 9, -5, claims=("streamk:atomic:W-odd",))
    add("s_short", 2, 32, 130, 6, 8, -5, ws="short", claims=("streamk:atomic:ws-small",))
    add("s_slots9", 2, 64, 40, 6, 8, -8, claims=("streamk:atomic:slots>8",))                    # 16 units in runs of 2
    # 6 tiles x 3 K tiles over 4 runs of 5: tiles 0, 2, 4 whole inside runs that also hold shares of tiles 1, 3
    add("s_inside", 2, 12, 130, 12, 16, -4, claims=("streamk:whole-tile-inside", "streamk:ws", "streamk:run-crosses-tiles", "ktiles3"))
    add("s_inside_nows", 2, 12, 130, 12, 16, -4, ws="none", claims=("streamk:whole-tile-inside", "streamk:atomic:no-ws"))
    add("s_inside_slow", 3, 10, 70, 10, 12, -3, claims=("streamk:ws", "slow:W-even", "K:partial", "streamk:whole-tile-inside"))
    add("s_upw_odd", 2, 28, 130, 6, 8, -4, claims=("streamk:ws",))                              # 21 units in runs of 6: upw does not divide ktiles = 7
    # stream-K, the library's: 30 tiles x 26 K tiles = 780 units in runs of 4
    add("s_library", 2, 104, 130, 40, 32, 0, claims=("streamk:library", "streamk:ws"))
    add("s_library_nows", 2, 104, 130, 40, 32, 0, ws="none", claims=("streamk:library", "streamk:atomic:no-ws"))
    # persistent whole tiles: 2 x 256 and 2 x 257 tiles at Cr = 4
    add("r_fast", 2, 4, 66, 256, 128, 0, claims=("persistent", "fast", "M%64"))
    add("r_ragged", 2, 5, 70, 200, 163, 1, claims=("persistent", "persistent:tiles%8", "M%64", "N%64", "TW>64", "W-odd", "spans-batch"))
    # the deterministic flag
    add("d_sk_nows", 2, 32, 40, 6, 8, 4, ws="none", det=True, claims=("det:fallback-whole", "whole"))
    add("d_sk_gt8", 2, 48, 40, 6, 8, 12, det=True, claims=("det:fallback-whole",))
    add("d_s_nows", 2, 32, 130, 6, 8, -5, ws="none", det=True, claims=("det:fallback-whole",))
    add("d_s_wodd", 2, 32, 130, 6, 9, -5, det=True, claims=("det:fallback-whole", "W-odd"))
    add("d_sk_ws", 2, 32, 40, 6, 8, 4, det=True, claims=("det:keeps-ws", "splitk:ws"))
    add("d_s_ws", 2, 32, 130, 6, 8, -5, det=True, claims=("det:keeps-ws", "streamk:ws"))
    add("d_lib_nows", 2, 104, 130, 40, 32, 0, ws="none", det=True, claims=("det:fallback-whole",))
    # epilogues: what x where
    for nm, ep in EPS.items():
        add(f"e_{nm}_kernel", 2, 32, 130, 6, 8, 1, ep=ep, claims=("epilogue:kernel", _content(ep)))
        add(f"e_{nm}_kernel_slow", 2, 30, 40, 7, 9, 1, ep=ep, scale=False, claims=("epilogue:kernel", _content(ep), "slow"))
        add(f"e_{nm}_reduce", 2, 32, 130, 6, 8, 4, ep=ep, claims=("epilogue:reduce", _content(ep)))
        add(f"e_{nm}_reduce_scalar", 1, 8, 5, 3, 3, 2, ep=ep, claims=("epilogue:reduce", _content(ep), "reduce:scalar"))
        add(f"e_{nm}_streamk", 2, 12, 130, 12, 16, -4, ep=ep, claims=("epilogue:streamk-reduce", _content(ep), "streamk:whole-tile-inside"))
        add(f"e_{nm}_deferred", 2, 32, 130, 6, 8, 4, ws="none", ep=ep,
            claims=("epilogue:deferred:noise" if ep[2] else "epilogue:deferred:bias-act", _content(ep)))
        add(f"e_{nm}_deferred_streamk", 2, 12, 130, 12, 16, -4, ws="none", ep=ep,
            claims=("epilogue:deferred:noise" if ep[2] else "epilogue:deferred:bias-act", "streamk:atomic:no-ws"))
    add("e_n_persistent", 2, 4, 66, 256, 128, 1, ep=EPS["n"], claims=("persistent", "epilogue:kernel", "noise"))
    add("e_n_det", 2, 32, 130, 6, 8, 4, ws="none", ep=EPS["n"], det=True, claims=("det:fallback-whole", "epilogue:kernel", "noise"))
    # the transposed weight transform: Cr != M
    add("x_whole", 2, 12, 40, 6, 8, 1, tr=True, claims=("transpose", "whole"))
    add("x_slow", 2, 7, 70, 7, 9, 1, tr=True, claims=("transpose", "slow", "K:partial", "M%64"))
    add("x_sk_ws", 2, 32, 40, 6, 8, 4, tr=True, claims=("transpose", "splitk:ws"))
    add("x_s_ws", 2, 12, 130, 12, 16, -4, tr=True, scale=False, claims=("transpose", "streamk:ws", "noscale"))
    add("x_ep", 2, 12, 40, 6, 8, 1, tr=True, ep=EPS["ba"], claims=("transpose", "epilogue:kernel"))
    return rows


EPS4 = dict(EPS, nn=(False, False, True), na=(False, True, True))


def _wino4_cases():
    rows = []
    add = lambda *a, **kw: rows.append(Wino(*a, kind=4, **kw))      # noqa: E731
    # tile rows of 1 .. 32 tiles; one 32-tile block per image
    for i, (H, W) in enumerate(((128, 4), (64, 8), (32, 16), (16, 32), (8, 64), (4, 128))):
        add(f"f_tw{W // 4}", 2, 8, 64, H, W, 1, scale=i % 2 == 0, claims=(f"TW{W // 4}", "whole", "ktiles2", "scale" if i % 2 == 0 else "noscale", "fwd", "epilogue:none"))
    add("f_blocks2", 2, 8, 64, 32, 32, 1, claims=("blocks-per-image>1", "TW8"))
    add("f_blocks4", 1, 8, 64, 32, 64, 1, scale=False, claims=("blocks-per-image>1", "TW16"))
    add("f_m128", 2, 8, 128, 16, 32, 1, claims=("M128",))
    for Cr in (4, 8, 12, 16):
        add(f"f_cr{Cr}", 2, Cr, 64, 16, 32, 0, claims=(f"ktiles{Cr // 4}", "whole") if Cr < 16 else ("whole",))
    add("f_cr512", 1, 512, 64, 16, 32, 0, claims=("Cr512", "splitk:library", "scale"))
    add("f_cr512_whole", 2, 512, 64, 16, 32, 1, claims=("Cr512", "whole", "scale"))
    add("f_cr512_nows", 1, 512, 64, 16, 32, 0, ws="none", claims=("Cr512", "splitk:library", "splitk:dropped:no-ws", "whole"))
    add("f_sk", 2, 32, 64, 16, 32, 4, claims=("splitk:forced",))
    add("f_sk_m128", 2, 32, 128, 32, 32, 2, scale=False, claims=("splitk:forced", "M128", "blocks-per-image>1"))
    add("f_sk_clipped", 2, 32, 64, 16, 32, 20, claims=("splitk:clipped", "splitk:forced"))
    add("f_sk_rounded", 2, 32, 64, 16, 32, 5, claims=("splitk:rounded",))
    add("f_sk_rounded3", 2, 28, 64, 16, 32, 5, claims=("splitk:rounded",))              # 7 K tiles: 5 -> per 2 -> 4, the last of one
    add("f_sk_kt3", 2, 12, 64, 16, 32, 2, claims=("splitk:forced", "ktiles3"))         # slices of 2 and 1 K tiles
    add("f_sk_nows", 2, 32, 64, 16, 32, 4, ws="none", claims=("splitk:dropped:no-ws", "whole"))
    add("f_sk_short", 2, 32, 64, 16, 32, 4, ws="short", claims=("splitk:dropped:ws-small", "whole"))
    add("f_sk_gt8", 2, 48, 64, 16, 32, 12, claims=("splitk:dropped:>8", "whole"))
    for nm, ep in EPS4.items():
        noise = (":noise",) if ep[2] else ()
        add(f"f_e_{nm}_kernel", 2, 8, 64, 16, 32, 1, ep=ep, claims=("epilogue:kernel", _content(ep)) + tuple("epilogue:kernel" + n for n in noise))
        add(f"f_e_{nm}_reduce", 2, 8, 64, 16, 32, 2, ep=ep, scale=nm in ("ba", "n"), claims=("epilogue:reduce", _content(ep)) + tuple("epilogue:reduce" + n for n in noise))
    add("f_x", 2, 8, 64, 16, 32, 1, tr=True, claims=("transpose", "whole"))
    add("f_x_m128", 2, 12, 128, 16, 32, 3, tr=True, claims=("transpose", "splitk:forced", "M128"))
    add("f_x_ep", 2, 64, 128, 8, 64, 1, tr=True, ep=EPS["n"], claims=("transpose", "epilogue:kernel:noise"))
    return rows


WINO = _wino_cases()
WINO4 = _wino4_cases()
BY_NAME = {c.name: c for c in WINO + WINO4}
assert len(BY_NAME) == len(WINO) + len(WINO4)

# (B, Cr, M, H, W) -> g2s_wino4_supported: each rejected shape with the clause that rejects it, then its accepted neighbour
SUPPORTED = {
    (0, 8, 64, 16, 32): 0, (1, 0, 64, 16, 32): 0, (1, 8, 0, 16, 32): 0, (1, 8, 64, 0, 32): 0, (1, 8, 64, 16, 0): 0,
    (1, 8, 64, 16, 32): 1,
    (1, 8, 64, 18, 32): 0, (1, 8, 64, 16, 30): 0, (1, 8, 96, 16, 32): 0, (1, 6, 64, 16, 32): 0,
    (1, 8, 128, 16, 32): 1, (1, 4, 64, 16, 32): 1, (1, 8, 64, 16, 32 + 32): 1,
    (1, 8, 64, 4, 256): 0, (1, 8, 64, 4, 128): 1,            # TW = 64 > 32
    (1, 8, 64, 128, 12): 0, (1, 8, 64, 128, 16): 1,          # TW = 3 does not divide 32 (96 tiles: whole blocks)
    (1, 8, 64, 16, 16): 0, (1, 8, 64, 32, 16): 1,            # 16 tiles per image
    (2, 8, 64, 48, 32): 1, (2, 8, 64, 8, 32): 0,             # 96 / 16 tiles per image
    (1, 516, 64, 16, 32): 0, (1, 512, 64, 16, 32): 1,
    (2048, 512, 64, 32, 16): 0, (2047, 512, 64, 32, 16): 1,  # B Cr H W = 2^29
    (2048, 4, 512, 32, 16): 0, (2047, 4, 512, 32, 16): 1,    # B M H W = 2^29
    (1, 512, 29184, 16, 32): 0, (1, 512, 29120, 16, 32): 1,  # 456 x 128 blocks of U >= 2^29 floats
}
SUPPORTED_CLAUSE = {(0, 8, 64, 16, 32): "positive", (1, 8, 64, 18, 32): "multiple", (1, 8, 64, 4, 256): "TW",
                    (1, 8, 64, 128, 12): "TW", (1, 8, 64, 16, 16): "block", (1, 516, 64, 16, 32): "Cr512",
                    (2048, 512, 64, 32, 16): "offsets", (2048, 4, 512, 32, 16): "offsets", (1, 512, 29184, 16, 32): "weights"}

# the plan against the library on the device (epilogue-free rows): what happens to y and to the workspace
ON_DEVICE = ("t_fast", "p_sk_ws", "p_sk_ws_slow", "p_sk_nows", "p_sk_short", "p_sk_gt8", "p_sk_8", "p_sk_rounded", "p_sk_scalar",
             "s_ws", "s_nows", "s_wodd", "s_short", "s_slots9", "s_inside", "s_inside_slow", "s_upw_odd", "s_library",
             "d_sk_gt8", "d_s_wodd", "f_sk", "f_sk_rounded3", "f_sk_short", "f_sk_gt8", "f_cr512")
# deterministic flag: rows whose plan without the flag meets by atomics; and workspace rows that must repeat bit for bit
DET_FALLBACK = ("d_sk_nows", "d_sk_gt8", "d_s_nows", "d_s_wodd", "d_lib_nows", "e_n_det")
DET_KEEPS = ("d_sk_ws", "d_s_ws", "s_inside", "s_library", "e_n_reduce", "e_ba_streamk")
# modconv.py's launch site: (row, WINO_FORCE); the rows' shapes as module calls
DISPATCH = (("p_sk_ws", 4), ("e_n_kernel", 1), ("x_whole", 0), ("f_sk", "w4:4"), ("f_e_n_kernel", "w4:1"), ("f_x_m128", "w4:3"))


# --------------------------------------------------------------------------------------------------- reference
def effective_weights(w, tr):
    """w(m, c, ky, kx) of the map: the stored tensor [Cout, Cin, 3, 3], or for the transposed transform
    w'(i, o, ky, kx) = w(o, i, 2 - ky, 2 - kx) (include/g2s.h; conv_cases.adjoint_weights)."""
    w = np.asarray(w)
    return np.ascontiguousarray(w.transpose(1, 0, 2, 3)[:, :, ::-1, ::-1]) if tr else w


def sums_reference(x, weff, in_scale, out_scale):
    """out_scale * conv3x3_pad1(in_scale * x, w) in float64 with conv2d_cases' shifted-slice sums."""
    B, Cr, H, W = x.shape
    M = weff.shape[0]
    xs = np.asarray(x, np.float64)
    if in_scale is not None:
        xs = xs * np.asarray(in_scale, np.float64)[:, :, None, None]
    y = cc.conv_reference(xs, np.asarray(weff, np.float64), cc.Conv("ref", B, Cr, M, H, W, 3, 1, 1, 0, mm=1))
    if out_scale is not None:
        y = y * np.asarray(out_scale, np.float64)[:, :, None, None]
    return y


def tail(v, bias, noise, ep, dtype):
    """+ noise_w * noise + bias; act: gain * leaky_relu(., alpha) (the gain comes with the activation)."""
    has_bias, act, has_noise = ep
    t = np.asarray(v, dtype)
    if has_noise:
        t = t + dtype(NOISE_W) * np.asarray(noise, dtype)[None, None]
    if has_bias:
        t = t + np.asarray(bias, dtype)[None, :, None, None]
    if act:
        t = np.where(t > 0, t, t * dtype(ALPHA)) * dtype(GAIN)
    return t


def wino_eval(x, weff, in_scale, out_scale, kind, dtype, absolute=False):
    """The Winograd algorithm itself in `dtype`, the three transforms as matrix products: Y = A^T [sum_c (G g G^T) .*
    (B^T d B)] A per tile.  F(2x2): U in dtype, the scale on the input; F(4x4): U in double and rounded once, the scale
    on the transformed patch (as the kernels place them).  absolute: every matrix and operand by its absolute value."""
    m = kind
    a = m + 2
    BT, G, AT = (np.abs(t) if absolute else t for t in MATS[kind])
    fix = np.abs if absolute else (lambda v: v)
    B, Cr, H, W = x.shape
    TH, TW = cdiv(H, m), cdiv(W, m)
    ud = np.float64 if kind == 4 else dtype
    U = np.einsum("ia,mcab,jb->mcij", G.astype(ud), fix(np.asarray(weff)).astype(ud), G.astype(ud)).astype(dtype)
    xs = fix(np.asarray(x)).astype(dtype)
    s = None if in_scale is None else fix(np.asarray(in_scale)).astype(dtype)[:, :, None, None]
    if s is not None and kind == 2:
        xs = xs * s
    xp = np.zeros((B, Cr, m * TH + 2, m * TW + 2), dtype)
    xp[:, :, 1:1 + H, 1:1 + W] = xs
    P = np.empty((B, Cr, TH, TW, a, a), dtype)
    for i in range(a):
        for j in range(a):
            P[..., i, j] = xp[:, :, i:i + m * TH:m, j:j + m * TW:m]
    BT, AT = BT.astype(dtype), AT.astype(dtype)
    V = np.einsum("bctuij,kj->bctuik", np.einsum("ia,bctuaj->bctuij", BT, P), BT)
    if s is not None and kind == 4:
        V = V * s[..., None, None]
    Mm = np.einsum("mcij,bctuij->bmtuij", U, V)
    assert Mm.dtype == dtype
    Y = np.einsum("bmtupj,qj->bmtupq", np.einsum("pi,bmtuij->bmtupj", AT, Mm), AT)
    y = Y.transpose(0, 1, 2, 4, 3, 5).reshape(B, weff.shape[0], m * TH, m * TW)[:, :, :H, :W]
    if out_scale is not None:
        y = y * fix(np.asarray(out_scale)).astype(dtype)[:, :, None, None]
    return np.ascontiguousarray(y)


def inputs(c):
    rng = np.random.default_rng([20254, zlib.crc32(c.name.encode())])
    x = rng.standard_normal((c.B, c.Cr, c.H, c.W)).astype(np.float32)
    wshape = (c.Cr, c.M, 3, 3) if c.tr else (c.M, c.Cr, 3, 3)        # [Cout, Cin, 3, 3]
    w = (rng.standard_normal(wshape) / np.sqrt(9 * c.Cr)).astype(np.float32)
    in_scale = (1 + 0.3 * np.clip(rng.standard_normal((c.B, c.Cr)), -1.5, 1.5)).astype(np.float32)
    out_scale = (1 + 0.3 * np.clip(rng.standard_normal((c.B, c.M)), -1.5, 1.5)).astype(np.float32)
    f = np.where(np.arange(c.B) % 2 == 0, 0.25, 4.0).astype(np.float32)[:, None]
    in_scale, out_scale = in_scale * f, out_scale / f
    bias = rng.standard_normal(c.M).astype(np.float32)
    noise = rng.standard_normal((c.H, c.W)).astype(np.float32)
    if not c.scale:
        in_scale = out_scale = None
    return x, w, in_scale, out_scale, bias, noise


def numbers(c, x, w, in_scale, out_scale, bias, noise):
    """ref (float64, with the tail), cap, e32w and r32 (the float32 emulation) of one call on given operands."""
    weff = effective_weights(w, c.tr)
    ref = sums_reference(x, weff, in_scale, out_scale)
    r32 = wino_eval(x, weff, in_scale, out_scale, c.kind, np.float32)
    terms = wino_eval(x, weff, in_scale, out_scale, c.kind, np.float64, absolute=True)
    n = c.Cr + C_ROUNDINGS[c.kind]
    if c.ep is None:
        cap = n * EPS32 * terms
    else:
        ref = tail(ref, bias, noise, c.ep, np.float64)
        r32 = tail(r32, bias, noise, c.ep, np.float32)
        extra = np.zeros((1, 1) + ref.shape[2:])
        if c.ep[2]:
            extra = extra + NOISE_W * np.abs(noise.astype(np.float64))[None, None]
        if c.ep[0]:
            extra = extra + np.abs(bias.astype(np.float64))[None, :, None, None]
        cap = max(GAIN, 1.0) * (n + 3) * EPS32 * (terms + extra)
    return ref, cap, cc.rel_err(r32, ref), r32


@functools.lru_cache(maxsize=None)
def data(name):
    """x, w ([Cout, Cin, 3, 3]), in_scale, out_scale, bias, noise, ref, cap, e32w and r32 of a row, computed once, read-only."""
    c = BY_NAME[name]
    x, w, in_scale, out_scale, bias, noise = inputs(c)
    ref, cap, e32w, r32 = numbers(c, x, w, in_scale, out_scale, bias, noise)
    return cc._freeze(dict(x=x, w=w, in_scale=in_scale, out_scale=out_scale, bias=bias, noise=noise, ref=ref, cap=cap,
                           e32w=e32w, r32=r32))


def ratio_of(path):
    """The ratio of a path of the measured table: no path is above 2, so RATIO everywhere."""
    return RATIO


def bound(ref, e32w, cap, ratio=RATIO):
    return cc.bound(ref, e32w, cap, ratio)
