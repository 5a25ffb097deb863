"""Case tables of tests/test_conv2d_cases_cpu.py and tests/test_gpu_conv2d_paths.py: g2s_conv2d, g2s_conv2d_wgrad and
g2s_conv2d_bwd (csrc/modconv.hip: conv_launch, conv2d_impl, conv_bwd_kernel; csrc/conv_wgrad_core.h; csrc/conv_wgrad.hip)
at shapes that reach every launch path, against a float64 reference written from the formulas of include/g2s.h.
Importable without a GPU.

plan_conv restates conv_launch (and the table lookup of conv2d_impl), plan_wgrad restates wgrad_plan; `labels` /
`wgrad_labels` name what a plan reaches.  Every table row carries the labels it is meant to reach (`claims`) and
tests/test_conv2d_cases_cpu.py holds the plans to them.

Labels of a convolution launch:
  gather:k3:s2 / scatter:k3:s2 (+ :p1)   the form (adjoint = 0 / 1), kernel size, stride (and pad)
  T1 T2 T4 T9 T16 T25                    tap count of a class = the body modconv_segment instantiates; for T in 1, 2, 4, 9
                                         also T9:full / T9:partial / T9:sub: Cr a multiple of the channels per K tile
                                         (16 / T; 2 for T = 9), not one, or below one tile
  kmax18 / kmax26                        the kernel instance (26: the 5 x 5 one)
  tile0 .. tile4                         128x128, 128x64, 64x64, 32x128, 64x128 (output channels x pixels)
  pick:heuristic / tuned / forced / heuristic-only   who chose the tile: the size rule, a conv2d_tuned.inc row,
                                         g2s_modconv_tune(tile >= 0), or the size rule under tile = -2 on a tuned signature
  split:1 / split:n                      split-K after clipping to kt_min; split:heuristic / tuned / forced / det say who
                                         chose it, split:clipped that kt_min cut it, split:unequal that the classes of a
                                         strided scatter got different shares (cls_splitk)
  epilogue:none / kernel / deferred      bias / activation: none, in the kernel, or as a second launch (after split-K, and
                                         where classes leave holes, whose value is the tail of 0)
  holes                                  output positions no class writes (k = 1, stride 2 scatter)
  needs-zero / overwrites                whether the launch adds into a cleared y
  layout:adj0:mm1 ..                     adjoint x w_m_major;  groups1 ..
  M<tile M%tile N<tile N%tile            ragged tile edges; spans-batch: a pixel tile holds pixels of two samples
  ragged-classes / early-exit            classes of different sizes; a class with fewer pixel tiles than the largest
  out:min / out:+h / out:+w              adjoint output size
  bwd:one-grid / bwd:two-launch          g2s_conv2d_bwd: rider in the grid (tiles 2..4) or a second kernel (tiles 0, 1)

Labels of a weight-gradient launch: Ca1 Ca63 .. / N63 .. (N = Cg k^2) / K20 .. (K = B PH PW) where they are one of the
edge values, k3:s2, groups2, role:conv / role:convT, G-larger (G one row and column beyond the taps' reach, NaN
there), K-spans-batch (a 32-pixel K tile holds pixels of two samples), split:1 / split:n, split:ragged (the last slice
is shorter), split:grid-full (split 1 because tiles x groups >= 768), split:det.

Reference.  Gather and scatter sums with explicit shifted slices, groups and out_h / out_w; the weight gradient as
dw[a,g,ky,kx] = sum A[b,a,py,px] G[b,g,py s + ky - p, px s + kx - p].  Inputs are seeded N(0, 1) draws rounded to
float32, weights scaled by 1 / sqrt(Cr k^2) and without any symmetry.

Bound, per element: |kernel - ref| <= min(ratio * e32 * max|ref|, cap).
  e32   error of torch's float32 CPU evaluation of the same operation (F.conv2d, F.conv_transpose2d,
        torch.nn.grad.conv2d_weight) against the float64 reference as a share of max|ref|, floored at half a float32
        spacing of max|ref| (dtrain_cases.bound).
  cap   n * eps32 * sum|terms| of that element (the same reference on |x| and |w|; n the reduction length Cr k^2 or
        B PH PW): any float32 summation order meets it.  With an epilogue the cap is gain * (n + 3) * eps32 *
        (sum|terms| + |bias|): three more roundings (bias, slope, gain), and leaky-ReLU has slopes of at most 1.
  Cases with a leaky-ReLU epilogue use the same bound on the float64 tail; no element is left out.
  ratio RATIO = 4 (groupnorm_cases.py, upfirdn_cases.py), and RATIO_UNSPLIT = 8 for one path: see the measurements.

Measured on an MI355X, largest error / (e32 * max|ref|) over the cases of a path (e32 floored); the largest error / cap
of any case was 0.25 (a border element of a 3 x 3 scatter with a single term), mostly below 0.03:

    g2s_conv2d          tile0  tile1  tile2  tile3  tile4       g2s_conv2d_wgrad                g2s_conv2d_bwd      gx     dw
    gather   plain       1.10   1.45   1.13   1.10   1.10       one slice             2.14      one grid  plain   1.73   1.95
    gather   split-K     0.91   0.91   0.91   0.91   0.91       split, float atomics  2.12      one grid  split   1.56   1.94
    gather   deferred       -      -   1.08      -      -       one slice, det. flag  4.38      two launches      1.19   1.34
    scatter  plain       1.16   1.16   1.16   1.16   1.16
    scatter  split-K     0.77   0.77   1.24   0.77   0.77       deterministic flag on a launch that would split:
    scatter  deferred       -      -   0.87      -      -       gather 4.14, scatter 2.38

Split-K with float atomics needs no more than the unsplit kernel: the slices shorten every accumulation chain.  The one
path above 4 is the opposite end: under the deterministic flag a single workgroup accumulates, in one float32 chain per
output, a reduction the default mode would have cut into slices (tuned_sk48: 1152 terms, 4.14 x e32, one element of
8192 over 4; the 5 x 5 layer's weight gradient in b_k5_t2: 198 pixels, 4.38, two elements of 1500).  torch's float32
CPU convolution sums in blocks, so its e32 does not grow with the chain; both launches sit at 0.002 and 0.04 of the
analytic cap.  That path, and only it (conv_ratio: the flag decided the split-K; wgrad_ratio: the flag is set), gets
twice its measured worst, cut to 8 (dtrain_cases.MULTIPLE's largest value): RATIO_UNSPLIT.
"""
import functools
import os
import re
import zlib

import numpy as np

RATIO = 4.0
RATIO_UNSPLIT = 8.0      # launches the deterministic flag keeps from splitting: see the measurements in the docstring
EPS32 = float(np.finfo(np.float32).eps)
GAIN = float(np.sqrt(2.0))
CFGS = ((128, 128), (128, 64), (64, 64), (32, 128), (64, 128))       # conv_launch: cfgs[pick] = {BM, BN}
TAPS_OK = (1, 2, 4, 9, 16, 25)
WG_BM = WG_BN = 64
WG_BK = 32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Rejected(ValueError):
    """conv_launch's G2S_REQUIRE on the tap count of a class."""


def cdiv(a, b):
    return -(-a // b)


def cpt_of(T):
    """Reduction channels per K tile (KTile<T>::CPT; ktiles_of)."""
    return 2 if T == 9 else 1 if T == 25 else 16 // T


def ktiles_of(Cr, T):
    return cdiv(Cr, cpt_of(T))


@functools.lru_cache(maxsize=None)
def tuned_rows():
    """The rows of csrc/conv2d_tuned.inc: (B, Cr, M, H, k, stride, pad, adjoint, m_major, fused, groups) -> (tile, splitk);
    the first row of a signature wins, as in conv2d_impl."""
    rows = {}
    with open(os.path.join(ROOT, "gan-2d-to-3d_amd", "csrc", "conv2d_tuned.inc")) as f:
        for m in re.finditer(r"^\{([-\d, ]+)\}", f.read(), re.M):
            v = tuple(int(t) for t in m.group(1).split(","))
            assert len(v) == 13
            rows.setdefault(v[:11], v[11:])
    return rows


def out_size(H, W, k, s, p, adjoint, extra=(0, 0)):
    if adjoint:
        return (H - 1) * s - 2 * p + k + extra[0], (W - 1) * s - 2 * p + k + extra[1]
    return (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1


def classes(H, W, k, s, p, adjoint, out_h=0, out_w=0):
    """conv_launch's class table: (OHf, OWf, [class], [hole]); a class is a dict with T, oy0, ox0, OH, OW and taps
    [(dy, dx, weight index)], a hole the (oy0, ox0) of a residue class without taps."""
    if not adjoint:
        OHf, OWf = out_size(H, W, k, s, p, 0)
        taps = [(ky - p, kx - p, ky * k + kx) for ky in range(k) for kx in range(k)]
        return OHf, OWf, [dict(T=k * k, oy0=0, ox0=0, OH=OHf, OW=OWf, taps=taps)], []
    OHf = out_h or (H - 1) * s - 2 * p + k
    OWf = out_w or (W - 1) * s - 2 * p + k
    lo_h, lo_w = (H - 1) * s - 2 * p + k, (W - 1) * s - 2 * p + k
    assert lo_h <= OHf <= lo_h + s - 1 and lo_w <= OWf <= lo_w + s - 1
    cls, holes = [], []
    for ry in range(s):
        for rx in range(s):
            OH, OW = (OHf - ry + s - 1) // s, (OWf - rx + s - 1) // s
            taps = [((ry + p - ky) // s, (rx + p - kx) // s, ky * k + kx) for ky in range(k) for kx in range(k)
                    if (ry + p - ky) % s == 0 and (rx + p - kx) % s == 0]
            if not taps or OH <= 0 or OW <= 0:
                if OH > 0 and OW > 0:
                    holes.append((ry, rx))
                continue
            cls.append(dict(T=len(taps), oy0=ry, ox0=rx, OH=OH, OW=OW, taps=taps))
    assert cls
    return OHf, OWf, cls, holes


def plan_conv(B, Cr, M, H, W, k, s, p, adjoint, m_major, out_h=0, out_w=0, groups=1, fused=False, tile=-1, splitk=-1,
              det=False, rider=False, tuned=True):
    """What conv2d_impl + conv_launch decide for one g2s_conv2d call under g2s_modconv_tune(tile, splitk) and the
    deterministic flag `det`.  Raises Rejected for a tap count without a body.  tuned = False: conv_launch alone, without
    conv2d_impl's table (the callers of tests/modconv_cases.py, whose entry points do not read it)."""
    assert 1 <= k <= 5 and s in (1, 2) and 0 <= p < k and 1 <= groups <= 8
    OHf, OWf, cls, holes = classes(H, W, k, s, p, adjoint, out_h if adjoint else 0, out_w if adjoint else 0)
    for c in cls:
        if c["T"] not in TAPS_OK:
            raise Rejected(f"unsupported tap count {c['T']} (k={k} stride={s})")
    big = any(c["T"] == 25 for c in cls)
    nmax = max(B * c["OH"] * c["OW"] for c in cls)
    kts = [ktiles_of(Cr, c["T"]) for c in cls]
    kt_min, kt_max = min(kts), max(max(kts), 1)
    # conv2d_impl: the measured table, square inputs only
    t_tile, t_split = -1, -1
    if H == W and tuned:
        t_tile, t_split = tuned_rows().get((B, Cr, M, H, k, s, p, int(bool(adjoint)), int(bool(m_major)), int(bool(fused)),
                                            groups), (-1, -1))
    pick, source = 2, "heuristic"
    for i in range(3):
        blocks = groups * cdiv(M, CFGS[i][0]) * cdiv(nmax, CFGS[i][1]) * len(cls)
        if M > CFGS[i][0] // 2 and blocks >= 512:
            pick = i
            break
    if M <= 32 and nmax >= 1024:
        pick = 3
    if t_tile >= 0 and tile != -2:
        pick, source = t_tile, "tuned"
    else:
        if t_tile >= 0:
            source = "heuristic-only"
        t_split = -1
    if tile >= 0:
        pick, source = tile, "forced"
    BM, BN = CFGS[pick]
    tiles = groups * cdiv(M, BM) * cdiv(nmax, BN)
    sk, sk_source = 1, "heuristic"
    while tiles * len(cls) * sk < 512 and kt_min // (sk * 2) >= 8 and sk < 64:
        sk *= 2
    if t_split > 0:
        sk, sk_source = t_split, "tuned"
    if splitk > 0:
        sk, sk_source = splitk, "forced"
    if det:
        sk, sk_source = 1, "det"
    asked = sk
    sk = max(1, min(sk, kt_min))
    cls_splitk = [max(1, min(kt, (sk * kt + kt_max // 2) // kt_max)) for kt in kts]
    split = sk > 1
    return dict(OHf=OHf, OWf=OWf, classes=cls, holes=holes, big=big, kmax=26 if big else 18,
                partial=[Cr % cpt_of(c["T"]) != 0 for c in cls], ktiles=kts, kt_min=kt_min, pick=pick, source=source,
                BM=BM, BN=BN, tiles=tiles, nmax=nmax, splitk=sk, asked=asked, split_source=sk_source,
                cls_splitk=cls_splitk, atomic=[c > 1 for c in cls_splitk], deferred=(split or bool(holes)) and bool(fused),
                needs_zero=split or bool(holes), one_grid=bool(rider) and pick >= 2)


def plan_wgrad(B, Ca, Cg, PH, PW, k, groups=1, det=False):
    """wgrad_plan: tiles, split, per, atomic (and N, K, ktiles)."""
    N, K = Cg * k * k, B * PH * PW
    ktiles = cdiv(K, WG_BK)
    tiles = cdiv(Ca, WG_BM) * cdiv(N, WG_BN)
    split = max(1, min(ktiles, cdiv(768, tiles * groups)))
    if det:
        split = 1
    per = cdiv(ktiles, split)
    split = cdiv(ktiles, per)
    return dict(N=N, K=K, ktiles=ktiles, tiles=tiles, split=split, per=per, atomic=split > 1)


# --------------------------------------------------------------------------------------------------------- cases
class Conv:
    """One g2s_conv2d call.  Cr -> M channels per group; eo: (out_h, out_w) beyond the minimum (adjoint); tile / sk:
    g2s_modconv_tune; ep: None or (bias, act, alpha, gain); det: the deterministic flag."""

    def __init__(self, name, B, Cr, M, H, W, k, s, p, adj, mm=None, eo=(0, 0), groups=1, tile=-1, sk=-1, ep=None,
                 det=False, claims=()):
        self.name, self.B, self.Cr, self.M, self.H, self.W, self.k, self.s, self.p = name, B, Cr, M, H, W, k, s, p
        self.adj = int(adj)
        self.mm = int(not adj) if mm is None else int(mm)       # the layouts of nn.Conv2d / nn.ConvTranspose2d
        self.eo, self.groups, self.tile, self.sk, self.ep, self.det = tuple(eo), groups, tile, sk, ep, det
        self.claims = tuple(claims)

    @property
    def out_hw(self):
        return out_size(self.H, self.W, self.k, self.s, self.p, self.adj, self.eo)

    def plan(self, tile=None, sk=None, det=None, rider=False, fused=None):
        oh, ow = self.out_hw
        return plan_conv(self.B, self.Cr, self.M, self.H, self.W, self.k, self.s, self.p, self.adj, self.mm,
                         oh if self.adj else 0, ow if self.adj else 0, self.groups,
                         (self.ep is not None) if fused is None else fused, self.tile if tile is None else tile,
                         self.sk if sk is None else sk, self.det if det is None else det, rider)

    def __repr__(self):
        return (f"{self.name}: B{self.B} Cr{self.Cr} M{self.M} {self.H}x{self.W} k{self.k} s{self.s} p{self.p} adj{self.adj} "
                f"mm{self.mm} eo{self.eo} g{self.groups} tune({self.tile},{self.sk}) ep{self.ep} det{int(self.det)}")


def labels(c, plan):
    form = "scatter" if c.adj else "gather"
    out = {f"{form}:k{c.k}:s{c.s}", f"{form}:k{c.k}:s{c.s}:p{c.p}", f"kmax{plan['kmax']}", f"tile{plan['pick']}",
           f"pick:{plan['source']}", f"split:{'n' if plan['splitk'] > 1 else '1'}", f"split:{plan['split_source']}",
           f"layout:adj{c.adj}:mm{c.mm}", f"groups{c.groups}"}
    for cl in plan["classes"]:
        T = cl["T"]
        out.add(f"T{T}")
        if T in (1, 2, 4, 9):
            out.add(f"T{T}:" + ("sub" if c.Cr < cpt_of(T) else "partial" if c.Cr % cpt_of(T) else "full"))
    if plan["asked"] > plan["splitk"]:
        out.add("split:clipped")
    if len(set(plan["cls_splitk"])) > 1:
        out.add("split:unequal")
    out.add("epilogue:none" if c.ep is None else "epilogue:deferred" if plan["deferred"] else "epilogue:kernel")
    if plan["holes"]:
        out.add("holes")
    out.add("needs-zero" if plan["needs_zero"] else "overwrites")
    BM, BN = plan["BM"], plan["BN"]
    if c.M < BM:
        out.add("M<tile")
    elif c.M % BM:
        out.add("M%tile")
    if c.groups > 1 and c.M % BM:
        out.add("groups:M%tile")
    sizes = [cl["OH"] * cl["OW"] for cl in plan["classes"]]
    if plan["nmax"] < BN:
        out.add("N<tile")
    elif plan["nmax"] % BN:
        out.add("N%tile")
    if c.B > 1 and any(n % BN for n in sizes):
        out.add("spans-batch")
    if len(set(sizes)) > 1:
        out.add("ragged-classes")
    if any(cdiv(c.B * n, BN) < cdiv(plan["nmax"], BN) for n in sizes):
        out.add("early-exit")
    if c.adj:
        out.add("out:min" if c.eo == (0, 0) else "out:+h" if c.eo == (1, 0) else "out:+w" if c.eo == (0, 1) else "out:+hw")
    return out


def _conv_cases():
    rows = []
    add = lambda *a, **kw: rows.append(Conv(*a, **kw))      # noqa: E731
    # tap bodies: gather k = 1..5 at both strides; B = 2 on a 9 x 11 map (99 pixels at stride 1: ragged second tile)
    for k in range(1, 6):
        for s in (1, 2):
            add(f"g_k{k}_s{s}", 2, 5, 6, 9, 11, k, s, k // 2, 0, claims=(f"gather:k{k}:s{s}", f"T{k * k}", "kmax26" if k == 5 else "kmax18"))
    # scatter, stride 1
    for k, p in ((1, 0), (2, 0), (3, 1), (4, 0), (4, 3), (5, 2)):
        add(f"a_k{k}_s1_p{p}", 2, 5, 6, 9, 11, k, 1, p, 1, claims=(f"scatter:k{k}:s1:p{p}", f"T{k * k}", "out:min"))
    # scatter, stride 2: four T = 1 classes, four T = 4, 4/2/2/1 under either pad, one class and three holes
    add("a_k2_s2", 2, 5, 6, 6, 7, 2, 2, 0, 1, claims=("scatter:k2:s2", "T1"))
    add("a_k4_s2", 2, 5, 6, 6, 7, 4, 2, 1, 1, claims=("scatter:k4:s2", "T4"))
    add("a_k3_s2_p0", 2, 5, 6, 6, 7, 3, 2, 0, 1, claims=("scatter:k3:s2:p0", "T4", "T2", "T1", "ragged-classes"))
    add("a_k3_s2_p1", 2, 5, 6, 6, 7, 3, 2, 1, 1, claims=("scatter:k3:s2:p1", "T4", "T2", "T1", "ragged-classes"))
    add("a_k1_s2_holes", 2, 5, 6, 6, 7, 1, 2, 0, 1, claims=("scatter:k1:s2", "T1", "holes", "needs-zero"))
    # Cr against the channels per K tile: T = 1 (16), 2 (8), 4 (4) through the 3x3 stride-2 scatter, T = 9 (2)
    for Cr, what in ((16, "full"), (35, "partial"), (3, "sub")):
        add(f"a_k3_s2_cr{Cr}", 2, Cr, 6, 5, 7, 3, 2, 1, 1, claims=(f"T1:{what}", f"T2:{what}", f"T4:{what}"))
    for Cr, what in ((4, "full"), (7, "partial"), (1, "sub")):
        add(f"g_k3_cr{Cr}", 2, Cr, 6, 5, 7, 3, 1, 1, 0, claims=(f"T9:{what}",))
    for Cr, what in ((32, "full"), (17, "partial")):
        add(f"g_k1_cr{Cr}", 2, Cr, 6, 5, 7, 1, 1, 0, 0, claims=(f"T1:{what}",))
    add("g_k2_cr8", 2, 8, 6, 5, 7, 2, 1, 0, 0, claims=("T4:full",))
    # every pad for k = 3 and 4, both forms and strides, on a non-square map
    for k in (3, 4):
        for p in range(k):
            for s in (1, 2):
                add(f"pad_g_k{k}_s{s}_p{p}", 2, 3, 5, 8, 11, k, s, p, 0, claims=(f"gather:k{k}:s{s}:p{p}",))
                add(f"pad_a_k{k}_s{s}_p{p}", 2, 3, 5, 8, 11, k, s, p, 1, claims=(f"scatter:k{k}:s{s}:p{p}",))
    # out_h / out_w beyond the minimum at stride 2; 8 x 9 (k = 3) and 8 x 8 (k = 4) inputs: classes of 72 / 64 / 63 / 56
    # pixels and their like, so the smaller ones need fewer 64-pixel tiles (the early exit of modconv_block)
    for k in (3, 4):
        for eo, what in (((0, 0), "out:min"), ((1, 0), "out:+h"), ((0, 1), "out:+w")):
            add(f"out_k{k}_{eo[0]}{eo[1]}", 1, 5, 6, 8, 9 if k == 3 else 8, k, 2, 1, 1, eo=eo,
                claims=(what, "early-exit") if (k, eo) != (4, (0, 0)) else (what,))
    # tile edges: M around the tile heights; N below a tile, ragged, a tile over two samples (35 pixels each)
    for M in (1, 31, 33, 65, 129):
        add(f"edge_m{M}", 2, 4, M, 5, 7, 3, 1, 1, 0, claims=("M<tile" if M < 64 else "M%tile", "N%tile", "spans-batch"))
    add("edge_n_small", 1, 4, 6, 5, 7, 3, 1, 1, 0, claims=("N<tile",))
    # layouts x groups
    for adj in (0, 1):
        for mm in (0, 1):
            for g in (1, 2, 3, 8):
                add(f"lay_a{adj}m{mm}_g{g}", 2, 5, 6, 6, 7, 3, 2, 1, adj, mm=mm, groups=g,
                    claims=(f"layout:adj{adj}:mm{mm}", f"groups{g}"))
    add("grp_m70", 2, 5, 70, 6, 7, 3, 1, 1, 0, groups=2, claims=("groups2", "groups:M%tile", "M%tile"))
    add("grp_m70_adj", 2, 5, 70, 6, 7, 4, 2, 1, 1, groups=3, claims=("groups3", "groups:M%tile", "M%tile"))
    # the heuristic's own picks, and its split-K
    add("heur_tile0", 4, 3, 96, 128, 128, 3, 1, 1, 0, claims=("tile0", "pick:heuristic", "split:1"))
    add("heur_tile1", 3, 3, 96, 128, 128, 3, 1, 1, 0, claims=("tile1", "pick:heuristic"))
    add("heur_tile2", 2, 5, 40, 9, 11, 3, 1, 1, 0, claims=("tile2", "pick:heuristic"))
    add("heur_tile3", 1, 4, 8, 32, 33, 3, 1, 1, 0, claims=("tile3", "pick:heuristic"))
    add("heur_split", 1, 32, 8, 6, 7, 3, 1, 1, 0, claims=("split:n", "split:heuristic", "needs-zero"))
    # rows of conv2d_tuned.inc at B = 1: tile 3, split-K 48, a fused one; and the first again under tile = -2
    add("tuned_tile3", 1, 128, 64, 16, 16, 4, 2, 1, 1, claims=("pick:tuned", "tile3", "split:tuned", "split:n"))
    add("tuned_sk48", 1, 128, 128, 8, 8, 3, 1, 1, 0, claims=("pick:tuned", "tile2", "split:tuned", "split:n"))
    add("tuned_fused", 1, 128, 256, 16, 16, 4, 2, 1, 0, ep=(True, True, 0.2, 1.0),
        claims=("pick:tuned", "split:tuned", "epilogue:deferred"))
    add("tuned_off", 1, 128, 64, 16, 16, 4, 2, 1, 1, tile=-2, claims=("pick:heuristic-only", "tile2", "split:heuristic"))
    # 3x3 stride-2 scatter: unequal shares of the classes (Cr = 130: 33 / 17 / 17 / 9 K tiles; Cr = 35: 9 / 5 / 5 / 3)
    add("shares_sk4", 1, 130, 6, 5, 7, 3, 2, 1, 1, sk=4, claims=("split:unequal", "split:forced"))
    add("shares_sk8", 1, 130, 6, 5, 7, 3, 2, 1, 1, sk=8, claims=("split:unequal",))
    add("shares_sk3", 2, 35, 6, 5, 7, 3, 2, 1, 1, sk=3, claims=("split:unequal",))
    add("shares_sk3_p0", 2, 35, 6, 5, 7, 3, 2, 0, 1, sk=3, eo=(1, 1), claims=("split:unequal", "out:+hw"))
    # epilogues, in the kernel (split-K 1) and deferred (split-K 2), through the C entry (gain != 1, bias with groups)
    for nm, ep in (("b", (True, False, 0.0, 1.0)), ("ba0", (True, True, 0.0, 1.0)), ("ba2", (True, True, 0.2, 1.0)),
                   ("g", (False, True, 0.2, GAIN)), ("bag", (True, True, 0.2, GAIN))):
        for sk in (1, 2):
            add(f"ep_{nm}_sk{sk}", 2, 7, 40, 9, 11, 3, 1, 1, 0, sk=sk, ep=ep,
                claims=("epilogue:kernel" if sk == 1 else "epilogue:deferred",))
    for sk in (1, 2):
        add(f"ep_grp_sk{sk}", 2, 7, 6, 9, 11, 3, 1, 1, 0, sk=sk, groups=2, ep=(True, False, 0.0, 1.0),
            claims=("groups2", "epilogue:kernel" if sk == 1 else "epilogue:deferred"))
        add(f"ep_adj_sk{sk}", 2, 9, 6, 6, 7, 4, 2, 1, 1, sk=sk, groups=2, ep=(True, True, 0.2, GAIN),
            claims=("groups2", "scatter:k4:s2", "epilogue:kernel" if sk == 1 else "epilogue:deferred"))
    # the deterministic flag on launches that would split
    add("det_heur_split", 1, 32, 8, 6, 7, 3, 1, 1, 0, det=True, claims=("split:det", "split:1", "overwrites"))
    add("det_tuned", 1, 128, 128, 8, 8, 3, 1, 1, 0, det=True, claims=("split:det", "split:1", "pick:tuned"))
    add("det_shares", 1, 130, 6, 5, 7, 3, 2, 1, 1, sk=8, det=True, claims=("split:det", "split:1"))
    return rows


CONV = _conv_cases()
CONV_BY_NAME = {c.name: c for c in CONV}
assert len(CONV_BY_NAME) == len(CONV)

# forced tiles x split-K, one base case per tap body (name -> the bodies it runs); the fourth split-K value is one
# above kt_min, so that it is clipped
SWEEP = {
    "sw_T1": (Conv("sw_T1", 2, 50, 40, 9, 11, 1, 1, 0, 0), ("T1",)),
    "sw_T4": (Conv("sw_T4", 2, 14, 40, 9, 11, 2, 1, 0, 0), ("T4",)),
    "sw_T9": (Conv("sw_T9", 2, 7, 40, 9, 11, 3, 1, 1, 0), ("T9",)),
    "sw_T16": (Conv("sw_T16", 2, 4, 40, 9, 11, 4, 2, 1, 0), ("T16",)),
    "sw_T25": (Conv("sw_T25", 2, 4, 40, 9, 11, 5, 1, 2, 0), ("T25", "kmax26")),
    "sw_T9_adj": (Conv("sw_T9_adj", 2, 7, 40, 9, 11, 3, 1, 1, 1), ("T9", "scatter:k3:s1")),
    "sw_T25_adj": (Conv("sw_T25_adj", 2, 4, 40, 9, 11, 5, 1, 2, 1), ("T25", "kmax26", "scatter:k5:s1")),
    "sw_T421": (Conv("sw_T421", 2, 35, 40, 5, 7, 3, 2, 1, 1), ("T4", "T2", "T1")),
    "sw_T4x4": (Conv("sw_T4x4", 2, 14, 40, 5, 7, 4, 2, 1, 1), ("T4", "scatter:k4:s2")),
}
SWEEP_TILES = (0, 1, 2, 3, 4)


def sweep_splits(c):
    return (1, 2, 3, c.plan(tile=2, sk=1)["kt_min"] + 1)


# output promises: y_is_zero = 0 on a NaN-filled y, y_is_zero = 1 on a zeroed y, guards around y
PROMISE = ("heur_split", "shares_sk4", "a_k1_s2_holes", "g_k3_s1", "a_k3_s2_p1", "ep_ba2_sk2", "ep_grp_sk1", "out_k3_10")
# plan against library on the device (epilogue-free): y = c and y_is_zero = 1
ON_DEVICE = ("heur_split", "shares_sk3", "shares_sk3_p0", "shares_sk4", "shares_sk8", "a_k1_s2_holes", "g_k3_s1",
             "a_k3_s2_p1", "tuned_tile3", "tuned_off", "det_heur_split", "lay_a1m1_g3")
# deterministic mode against forced split-K 1 at the same tile
DETERMINISTIC = ("heur_split", "tuned_sk48", "shares_sk8", "tuned_fused", "tuned_tile3")


class Wgrad:
    """One g2s_conv2d_wgrad call: A [B, groups Ca, PH, PW], G [B, groups Cg, GH, GW].  role conv: A = gy of a Conv2d,
    G = its input of gh x gw; role convT: A = the input of a ConvTranspose2d, G = its gy; grow: G one row and column
    larger than the taps reach."""

    def __init__(self, name, B, Ca, Cg, PH, PW, k, s, p, role="conv", G_hw=None, grow=False, groups=1, det=False, claims=()):
        self.name, self.B, self.Ca, self.Cg, self.PH, self.PW, self.k, self.s, self.p = name, B, Ca, Cg, PH, PW, k, s, p
        self.role, self.grow, self.groups, self.det, self.claims = role, grow, groups, det, tuple(claims)
        reach = ((PH - 1) * s + k - p, (PW - 1) * s + k - p)        # rows / columns of G the taps can read
        if G_hw is None:
            # conv: the smallest input with this output is (PH - 1) s + k - 2p; convT: gy of exactly that size
            G_hw = ((PH - 1) * s + k - 2 * p, (PW - 1) * s + k - 2 * p)
        if grow:
            G_hw = (reach[0] + 1, reach[1] + 1)
        self.GH, self.GW = G_hw
        self.reach = reach
        assert self.GH > 0 and self.GW > 0

    def plan(self, det=None):
        return plan_wgrad(self.B, self.Ca, self.Cg, self.PH, self.PW, self.k, self.groups, self.det if det is None else det)

    def __repr__(self):
        return (f"{self.name}: B{self.B} Ca{self.Ca} Cg{self.Cg} P{self.PH}x{self.PW} G{self.GH}x{self.GW} k{self.k} "
                f"s{self.s} p{self.p} {self.role} g{self.groups} det{int(self.det)}")


def wgrad_labels(c, plan):
    out = {f"k{c.k}:s{c.s}", f"k{c.k}:s{c.s}:p{c.p}", f"groups{c.groups}", f"role:{c.role}",
           "split:n" if plan["split"] > 1 else "split:1"}
    if c.Ca in (1, 63, 64, 65):
        out.add(f"Ca{c.Ca}")
    if plan["N"] in (63, 64, 65):
        out.add(f"N{plan['N']}")
    if plan["K"] in (20, 32, 33):
        out.add(f"K{plan['K']}")
    if c.B > 1 and (c.PH * c.PW) % WG_BK:
        out.add("K-spans-batch")
    if c.grow:
        out.add("G-larger")
    if plan["split"] > 1 and plan["ktiles"] % plan["per"]:
        out.add("split:ragged")
    if c.det:
        out.add("split:det")
    elif plan["tiles"] * c.groups >= 768:
        out.add("split:grid-full")
    return out


def _wgrad_cases():
    rows = []
    add = lambda *a, **kw: rows.append(Wgrad(*a, **kw))     # noqa: E731
    for Ca in (1, 63, 64, 65):
        add(f"w_ca{Ca}", 3, Ca, 5, 5, 7, 3, 1, 1, claims=(f"Ca{Ca}", "K-spans-batch", "split:n"))
    add("w_n63", 3, 6, 7, 5, 7, 3, 1, 1, claims=("N63",))
    add("w_n64", 3, 6, 4, 5, 7, 4, 2, 1, claims=("N64",))
    add("w_n65", 3, 6, 65, 5, 7, 1, 1, 0, claims=("N65",))
    add("w_k20", 1, 6, 5, 4, 5, 3, 1, 1, claims=("K20", "split:1"))
    add("w_k32", 2, 6, 5, 4, 4, 3, 1, 1, claims=("K32", "split:1"))
    add("w_k33", 3, 6, 5, 1, 11, 3, 1, 1, claims=("K33", "split:n", "K-spans-batch"))
    for k in range(1, 6):
        for s in (1, 2):
            add(f"w_k{k}_s{s}", 3, 6, 5, 5, 7, k, s, k // 2, role="conv" if (k + s) % 2 else "convT",
                claims=(f"k{k}:s{s}", "K-spans-batch"))
    for p in (0, 2):
        for s in (1, 2):
            add(f"w_k3_s{s}_p{p}", 3, 6, 5, 5, 7, 3, s, p, claims=(f"k3:s{s}:p{p}",))
    add("w_convT", 3, 6, 5, 5, 7, 4, 2, 1, role="convT", claims=("role:convT",))
    add("w_conv_odd", 3, 6, 5, 5, 7, 4, 2, 1, G_hw=(11, 15), claims=("role:conv",))      # a stride-2 Conv2d on an odd input
    add("w_grow_s1", 3, 6, 5, 5, 7, 3, 1, 1, grow=True, claims=("G-larger",))
    add("w_grow_s2", 3, 6, 5, 5, 7, 4, 2, 1, grow=True, claims=("G-larger", "k4:s2"))
    # K = 3 x 11 x 13 = 429: 14 K tiles, split 14
    add("w_split", 3, 6, 5, 11, 13, 3, 1, 1, claims=("split:n",))
    # K = 157 x 157 = 24649: 771 K tiles on one output tile -> split 768 -> per 2 -> 386 slices, the last of one tile
    add("w_ragged", 1, 6, 5, 157, 157, 3, 1, 1, claims=("split:ragged", "split:n"))
    add("w_grid_full", 1, 512, 384, 4, 4, 4, 1, 0, role="convT", claims=("split:grid-full", "split:1"))
    add("w_det", 3, 6, 5, 11, 13, 3, 1, 1, det=True, claims=("split:det", "split:1"))
    for g in (2, 3):
        add(f"w_g{g}", 3, 6, 5, 5, 7, 3, 2, 1, groups=g, claims=(f"groups{g}",))
    add("w_g2_convT", 2, 65, 7, 5, 7, 4, 2, 1, role="convT", groups=2, claims=("groups2", "Ca65"))
    return rows


WGRAD = _wgrad_cases()
WGRAD_BY_NAME = {c.name: c for c in WGRAD}
assert len(WGRAD_BY_NAME) == len(WGRAD)
WGRAD_PROMISE = ("w_split", "w_k20", "w_g2_convT", "w_ragged")


class Bwd:
    """One g2s_conv2d_bwd call: the backward of nn.Conv2d (transposed = False) or nn.ConvTranspose2d of cin -> cout
    channels per group on an input of H x W."""

    def __init__(self, name, B, cin, cout, H, W, k, s, p, transposed, groups=1, tile=-1, sk=-1, det=False, claims=()):
        self.name, self.B, self.cin, self.cout, self.H, self.W, self.k, self.s, self.p = name, B, cin, cout, H, W, k, s, p
        self.transposed, self.groups, self.tile, self.sk, self.det, self.claims = transposed, groups, tile, sk, det, tuple(claims)
        self.yh, self.yw = out_size(H, W, k, s, p, transposed)
        # data gradient: gy -> gx; Conv2d: scatter with w [cout, cin] = [Cr][M]; ConvTranspose2d: gather, w [cin, cout] = [M][Cr]
        eo = (H - out_size(self.yh, self.yw, k, s, p, 1)[0], W - out_size(self.yh, self.yw, k, s, p, 1)[1]) if not transposed else (0, 0)
        self.dgrad = Conv(name + ".gx", B, cout, cin, self.yh, self.yw, k, s, p, not transposed, mm=transposed, eo=eo,
                          groups=groups, tile=tile, sk=sk, det=det)
        assert self.dgrad.out_hw == (H, W)
        if transposed:
            self.wgrad = Wgrad(name + ".dw", B, cin, cout, H, W, k, s, p, "convT", (self.yh, self.yw), groups=groups, det=det)
        else:
            self.wgrad = Wgrad(name + ".dw", B, cout, cin, self.yh, self.yw, k, s, p, "conv", (H, W), groups=groups, det=det)

    def plan(self, **kw):
        return self.dgrad.plan(rider=True, **kw)

    def __repr__(self):
        return f"{self.name}: {'ConvT' if self.transposed else 'Conv'} {self.dgrad!r} | {self.wgrad!r}"


def bwd_labels(c, plan):
    out = labels(c.dgrad, plan)
    out.add("bwd:one-grid" if plan["one_grid"] else "bwd:two-launch")
    out.add("layer:convT" if c.transposed else "layer:conv")
    return out


def _bwd_cases():
    rows = []
    add = lambda *a, **kw: rows.append(Bwd(*a, **kw))       # noqa: E731
    for tile in (0, 1, 2, 3, 4):
        form = "bwd:one-grid" if tile >= 2 else "bwd:two-launch"
        add(f"b_conv_t{tile}", 2, 5, 40, 9, 11, 3, 2, 1, False, tile=tile, sk=1,
            claims=(form, f"tile{tile}", "kmax18", "layer:conv", "out:min", "split:1"))
        add(f"b_convT_t{tile}", 2, 36, 6, 5, 7, 4, 2, 1, True, tile=tile, sk=3,
            claims=(form, f"tile{tile}", "kmax18", "layer:convT", "split:n"))
        add(f"b_k5_t{tile}", 2, 5, 6, 9, 11, 5, 1, 2, False, groups=2, tile=tile, sk=3,
            claims=(form, f"tile{tile}", "kmax26", "groups2", "split:n"))
    add("b_k5_convT", 2, 6, 5, 9, 11, 5, 1, 2, True, tile=3, sk=1, claims=("kmax26", "layer:convT", "bwd:one-grid"))
    add("b_odd_w", 2, 5, 6, 10, 11, 4, 2, 1, False, sk=3, claims=("out:+w", "bwd:one-grid", "pick:heuristic", "split:clipped"))
    add("b_odd_h", 2, 5, 9, 11, 10, 4, 2, 1, False, sk=2, claims=("out:+h", "split:n", "bwd:one-grid"))
    add("b_k3_shares", 2, 6, 35, 10, 12, 3, 2, 1, False, sk=3, groups=2, claims=("out:+hw", "groups2", "split:n", "split:unequal"))
    add("b_builtin", 1, 8, 32, 6, 7, 3, 1, 1, True, claims=("pick:heuristic", "split:heuristic", "split:n", "bwd:one-grid"))
    add("b_tuned", 1, 64, 128, 32, 32, 4, 2, 1, False, claims=("pick:tuned", "tile3", "split:n", "bwd:one-grid"))
    add("b_det", 1, 8, 32, 6, 7, 3, 1, 1, True, det=True, claims=("split:det", "split:1"))
    add("b_det_g2", 2, 6, 35, 10, 12, 3, 2, 1, False, groups=2, det=True, claims=("split:det", "groups2"))
    return rows


BWD = _bwd_cases()
BWD_BY_NAME = {c.name: c for c in BWD}
assert len(BWD_BY_NAME) == len(BWD)
BWD_PROMISE = ("b_conv_t2", "b_convT_t3", "b_k5_t4", "b_convT_t0", "b_builtin")
BWD_DETERMINISTIC = ("b_det", "b_det_g2", "b_conv_t3", "b_k5_t2")


# ----------------------------------------------------------------------------------------------------- reference
def weights_gmc(w, groups, M, Cr, k, m_major):
    """The launch layout ([groups][M][Cr][k][k] or [groups][Cr][M][k][k]) as [groups, M, Cr, k, k]."""
    if m_major:
        return w.reshape(groups, M, Cr, k, k)
    return w.reshape(groups, Cr, M, k, k).transpose(0, 2, 1, 3, 4)


def conv_reference(x, w, c, dtype=np.float64):
    """include/g2s.h, g2s_conv2d, term by term: adjoint = 0: y[b,m,oy,ox] = sum x[b,c,oy s + ky - p, ox s + kx - p] W(m,c,ky,kx);
    adjoint = 1: y[b,m,iy s + ky - p, ix s + kx - p] += x[b,c,iy,ix] W(m,c,ky,kx), cut to out_h x out_w."""
    B, G, Cr, M, H, W, k, s, p = c.B, c.groups, c.Cr, c.M, c.H, c.W, c.k, c.s, c.p
    x = np.asarray(x, dtype).reshape(B, G, Cr, H, W)
    wt = weights_gmc(np.asarray(w, dtype), G, M, Cr, k, c.mm)
    oh, ow = c.out_hw
    if not c.adj:
        xp = np.zeros((B, G, Cr, H + 2 * p, W + 2 * p), dtype)
        xp[..., p:p + H, p:p + W] = x
        y = np.zeros((B, G, M, oh, ow), dtype)
        for ky in range(k):
            for kx in range(k):
                y += np.einsum("gmc,bgcyx->bgmyx", wt[..., ky, kx], xp[..., ky:ky + (oh - 1) * s + 1:s, kx:kx + (ow - 1) * s + 1:s])
    else:
        full = np.zeros((B, G, M, (H - 1) * s + k + s, (W - 1) * s + k + s), dtype)
        for ky in range(k):
            for kx in range(k):
                full[..., ky:ky + (H - 1) * s + 1:s, kx:kx + (W - 1) * s + 1:s] += np.einsum("gmc,bgcyx->bgmyx", wt[..., ky, kx], x)
        y = full[..., p:p + oh, p:p + ow]
    return np.ascontiguousarray(y.reshape(B, G * M, oh, ow))


def tail(v, bias, ep, dtype):
    """The epilogue on the sums v [B, C, oh, ow]: + bias[c]; act: gain * leaky_relu(., alpha)."""
    has_bias, act, alpha, gain = ep
    t = np.asarray(v, dtype)
    if has_bias:
        t = t + np.asarray(bias, dtype)[None, :, None, None]
    if act:
        t = np.where(t > 0, t, t * dtype(alpha)) * dtype(gain)
    return t


def wgrad_reference(A, G, c, dtype=np.float64):
    """dw[a,g,ky,kx] = sum_{b,py,px} A[b,a,py,px] G[b,g,py s + ky - p, px s + kx - p], zero outside G."""
    B, Gr, Ca, Cg, PH, PW, k, s, p = c.B, c.groups, c.Ca, c.Cg, c.PH, c.PW, c.k, c.s, c.p
    A = np.asarray(A, dtype).reshape(B, Gr, Ca, PH, PW)
    Gp = padded_G(G, c, dtype).reshape(B, Gr, Cg, (PH - 1) * s + k, (PW - 1) * s + k)
    dw = np.zeros((Gr, Ca, Cg, k, k), dtype)
    for ky in range(k):
        for kx in range(k):
            dw[..., ky, kx] = np.einsum("bnayx,bngyx->nag", A, Gp[..., ky:ky + (PH - 1) * s + 1:s, kx:kx + (PW - 1) * s + 1:s])
    return dw.reshape(Gr * Ca, Cg, k, k)


def padded_G(G, c, dtype=np.float64):
    """G with p zero rows and columns in front and cut or zero-filled to the (PH - 1) s + k rows the taps reach: rows
    and columns beyond that are never read (and may hold NaN)."""
    rows, cols = (c.PH - 1) * c.s + c.k, (c.PW - 1) * c.s + c.k
    Gp = np.zeros(G.shape[:2] + (rows, cols), dtype)
    h, w = min(c.GH, rows - c.p), min(c.GW, cols - c.p)
    Gp[..., c.p:c.p + h, c.p:c.p + w] = np.asarray(G)[..., :h, :w]
    return Gp


def rel_err(got, want):
    return float(np.abs(np.asarray(got, np.float64) - want).max() / np.abs(want).max())


def floor_e32(e32):
    """Half a float32 spacing of max|ref| at the least, as dtrain_cases.bound."""
    return max(float(e32), 0.5 * EPS32)


def bound(ref, e32, cap, ratio=RATIO):
    return np.minimum(ratio * floor_e32(e32) * np.abs(ref).max(), cap)


def conv_ratio(plan):
    """RATIO, or RATIO_UNSPLIT where the deterministic flag decided the split-K (one workgroup then runs a K loop the
    default mode would have cut into slices)."""
    return RATIO_UNSPLIT if plan["split_source"] == "det" else RATIO


def wgrad_ratio(det):
    return RATIO_UNSPLIT if det else RATIO


def _torch_conv_f32(x, w, c, dtype):
    import torch
    import torch.nn.functional as F
    G, M, Cr, k = c.groups, c.M, c.Cr, c.k
    wt = weights_gmc(np.asarray(w), G, M, Cr, k, c.mm)
    xt = torch.tensor(np.asarray(x), dtype=dtype)
    if not c.adj:
        wt = torch.tensor(np.ascontiguousarray(wt.reshape(G * M, Cr, k, k)), dtype=dtype)
        return F.conv2d(xt, wt, None, c.s, c.p, 1, G).numpy()
    wt = torch.tensor(np.ascontiguousarray(wt.transpose(0, 2, 1, 3, 4).reshape(G * Cr, M, k, k)), dtype=dtype)
    return F.conv_transpose2d(xt, wt, None, c.s, c.p, c.eo, G).numpy()


def _torch_wgrad(A, G, c, dtype, autograd=False):
    import torch
    import torch.nn.functional as F
    Gp = torch.tensor(padded_G(G, c), dtype=dtype)
    At = torch.tensor(np.asarray(A), dtype=dtype)
    size = (c.groups * c.Ca, c.Cg, c.k, c.k)
    if autograd:
        w = torch.zeros(size, dtype=dtype, requires_grad=True)
        F.conv2d(Gp, w, None, c.s, 0, 1, c.groups).backward(At)
        return w.grad.numpy()
    return torch.nn.grad.conv2d_weight(Gp, size, At, c.s, 0, 1, c.groups).numpy()


def _rng(name):
    return np.random.default_rng([20253, zlib.crc32(name.encode())])


def _freeze(out):
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def _conv_data(c):
    rng = _rng(c.name.split(".")[0])
    G, M, Cr, k = c.groups, c.M, c.Cr, c.k
    x = rng.standard_normal((c.B, G * Cr, c.H, c.W)).astype(np.float32)
    wshape = (G * M, Cr, k, k) if c.mm else (G * Cr, M, k, k)
    w = (rng.standard_normal(wshape) / np.sqrt(Cr * k * k)).astype(np.float32)
    bias = rng.standard_normal(G * M).astype(np.float32)
    return x, w, bias


def conv_numbers(c, x, w, bias):
    """ref, cap and e32 of one convolution on given operands."""
    ref = conv_reference(x, w, c)
    terms = conv_reference(np.abs(x), np.abs(w), c)
    r32 = _torch_conv_f32(x, w, c, _f32())
    n = c.Cr * c.k * c.k
    if c.ep is None:
        cap = n * EPS32 * terms
    else:
        ref = tail(ref, bias, c.ep, np.float64)
        r32 = tail(r32, bias, c.ep, np.float32)
        b = np.abs(bias.astype(np.float64))[None, :, None, None] if c.ep[0] else 0.0
        cap = max(c.ep[3], 1.0) * (n + 3) * EPS32 * (terms + b)
    return ref, cap, rel_err(r32, ref), r32


def _f32():
    import torch
    return torch.float32


@functools.lru_cache(maxsize=None)
def conv_data(name):
    """x, w (launch layout), bias, ref (float64, with the epilogue), cap, e32 and r32 (torch's float32) of a g2s_conv2d case
    (table or sweep), computed once and read-only."""
    c = CONV_BY_NAME[name] if name in CONV_BY_NAME else SWEEP[name][0]
    x, w, bias = _conv_data(c)
    ref, cap, e32, r32 = conv_numbers(c, x, w, bias)
    return _freeze(dict(x=x, w=w, bias=bias, ref=ref, cap=cap, e32=e32, r32=r32))


def wgrad_numbers(c, A, G):
    ref = wgrad_reference(A, np.nan_to_num(G), c)
    terms = wgrad_reference(np.abs(A), np.abs(np.nan_to_num(G)), c)
    r32 = _torch_wgrad(A, np.nan_to_num(G), c, _f32())
    return ref, c.B * c.PH * c.PW * EPS32 * terms, rel_err(r32, ref), r32


@functools.lru_cache(maxsize=None)
def wgrad_data(name):
    """A, G (NaN beyond the taps' reach in the `grow` cases), ref, cap, e32, r32 of a g2s_conv2d_wgrad case."""
    c = WGRAD_BY_NAME[name]
    rng = _rng(name)
    A = rng.standard_normal((c.B, c.groups * c.Ca, c.PH, c.PW)).astype(np.float32)
    G = rng.standard_normal((c.B, c.groups * c.Cg, c.GH, c.GW)).astype(np.float32)
    if c.grow:
        G[..., c.reach[0]:, :] = np.nan
        G[..., :, c.reach[1]:] = np.nan
    ref, cap, e32, r32 = wgrad_numbers(c, A, G)
    return _freeze(dict(A=A, G=G, ref=ref, cap=cap, e32=e32, r32=r32))


@functools.lru_cache(maxsize=None)
def bwd_data(name):
    """x, w, gy of the layer and, for gx and dw each, ref, cap, e32, r32."""
    c = BWD_BY_NAME[name]
    rng = _rng(name)
    g, k = c.groups, c.k
    x = rng.standard_normal((c.B, g * c.cin, c.H, c.W)).astype(np.float32)
    wshape = (g * c.cin, c.cout, k, k) if c.transposed else (g * c.cout, c.cin, k, k)
    w = (rng.standard_normal(wshape) / np.sqrt(c.cin * k * k)).astype(np.float32)
    gy = rng.standard_normal((c.B, g * c.cout, c.yh, c.yw)).astype(np.float32)
    gx_ref, gx_cap, gx_e32, gx_r32 = conv_numbers(c.dgrad, gy, w, None)
    A, G = (x, gy) if c.transposed else (gy, x)
    dw_ref, dw_cap, dw_e32, dw_r32 = wgrad_numbers(c.wgrad, A, G)
    return _freeze(dict(x=x, w=w, gy=gy, gx_ref=gx_ref, gx_cap=gx_cap, gx_e32=gx_e32, gx_r32=gx_r32,
                        dw_ref=dw_ref, dw_cap=dw_cap, dw_e32=dw_e32, dw_r32=dw_r32))
