"""Cases of tests/test_gpu_hbm_twins.py: the memory-bound passes whose entries come in families — the StyledConv tail
with a shared or a per-sample noise map (in place, in the blur's store, in the backward row pass), three weighted-L1
backward entries, single- and multi-layer demodulation — held bit for bit to a recorded run of the library
(tests/golden/hbm_twins_parent.npz, written by tests/golden/make_hbm_twins_golden.py from these same calls), so that
a family can share one kernel, or stop sharing it, without a change in results.

Every kernel reached here is elementwise or one wave per row with a fixed summation order and no atomics, so its
output is a function of its inputs alone.  The shapes are the smallest that reach every path of the merged code; each
group below says which.  Inputs are seeded numpy draws; `run(L, lib)` makes every call through the exported entries
only and returns {name: device tensor}."""
import numpy as np
import torch

ALPHA, GAIN = 0.2, 2 ** 0.5

# ---- the StyledConv tail in place: (name, B, C, HW, variant)
#   vec      16-byte accesses; C = 3 is no power of two, so row / C and row % C matter
#   scalar   HW % 4 != 0
#   offset   a vector-eligible shape with x one float past alignment: the scalar path
#   inplace  y == x
#   nonoise  noise == NULL (shared entry only)
TAIL = [("vec", 2, 3, 16, ""), ("scalar", 3, 5, 25, ""), ("offset", 2, 3, 16, "offset"),
        ("inplace", 2, 3, 16, "inplace"), ("nonoise", 2, 3, 16, "nonoise")]

# ---- the blur with the tail in its store, B = 2, C = 3, pad (1, 1, 1, 1): (name, in_h, in_w, taps)
#   10 x 10   one partial 32 x 32 tile          17 x 49   64 x 16 tiles (out_w 48)
#   17 x 97   128 x 16 tiles (out_w 96)         17 x 131  the 160-wide tile: lanes take a second turn (out_w 130)
#   6 x 6 with a 3 x 3 kernel: the generic fallback
BLUR_B, BLUR_C = 2, 3
BLUR = [("10x10", 10, 10, (1, 3, 3, 1)), ("17x49", 17, 49, (1, 3, 3, 1)), ("17x97", 17, 97, (1, 3, 3, 1)),
        ("17x131", 17, 131, (1, 3, 3, 1)), ("6x6k3", 6, 6, (1, 2, 1))]

# ---- the backward row pass: (B, C, H); n = 16: 16-byte loads, n = 9: scalar.  Each with and without g2 and gdot.
ROWS = [(3, 5, 4), (2, 7, 3)]

# ---- weighted-L1 backward
WL1 = (2, 3, 8)
WL1_COMBOS = [(xo, na) for xo in (1, 0) for na in (0, 1, 2) if xo or na]     # as reduce_cases.L1_COMBOS

# ---- demodulation: (B, Cin, Cout); (2, 5, 3): one workgroup column, (3, 70, 9): two, lanes stride over Cin.
# The multi-layer entries take one B for all layers: both (Cin, Cout) as two layers of one call with B = 3.
DEMOD = [(2, 5, 3), (3, 70, 9)]
DEMOD_MULTI_B = 3
EPS = 1e-8
TAIL_NW, BLUR_NW, ROWS_NW = -0.37, -0.8, 0.6      # the noise weights (device scalars)


def _rng(*key):
    return np.random.default_rng([20240] + [int(k) for k in key])


def _f32(rng, *shape):
    return rng.standard_normal(shape).astype(np.float32)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def offset_by_one_float(t):
    """The same values at an address 4 bytes past a 16-byte boundary."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    view = buf[1:].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == 4
    return view


def taps(t):
    k = np.outer(t, t).astype(np.float32)
    return k / 16


def tail_inputs(B, C, HW):
    """x [B, C, HW], noise [B, HW], bias [C], noise weight (numpy, float32)."""
    rng = _rng(1, B, C, HW)
    x, noise, bias = _f32(rng, B, C, HW), _f32(rng, B, HW), _f32(rng, C)
    x[:, :, 1] = -bias[None, :]          # pre-activations that are exactly 0 where the map is 0
    noise[:, 1] = 0.0
    return x, noise, bias, TAIL_NW


def run_tail(L, lib, res):
    for name, B, C, HW, variant in TAIL:
        x, noise, bias, nw = tail_inputs(B, C, HW)
        nd, bd, nwd = dev(noise), dev(bias), dev([nw])
        for entry, nz in (("shared", nd[0].contiguous()), ("ps", nd)):
            if variant == "nonoise":
                if entry == "ps":
                    continue
                nz = None
            xd = dev(x)
            if variant == "offset":
                xd = offset_by_one_float(xd)
            y = xd if variant == "inplace" else torch.full((B, C, HW), float("nan"), device="cuda")
            fn = L.g2s_noise_bias_act if entry == "shared" else L.g2s_noise_bias_act_ps
            lib.check(fn(lib.ptr(xd), lib.ptr(nz), lib.ptr(nwd), lib.ptr(bd), lib.ptr(y), B, C, HW, ALPHA, GAIN,
                         lib.stream()))
            res[f"tail.{name}.{entry}"] = y


def blur_inputs(ih, iw, t):
    """x [B, C, ih, iw], taps [kh, kh], noise [B, oh, ow], bias [C], noise weight (numpy, float32)."""
    B, C = BLUR_B, BLUR_C
    rng = _rng(2, ih, iw)
    k = taps(t)
    kh = k.shape[0]
    oh, ow = ih + 2 - kh + 1, iw + 2 - kh + 1
    return _f32(rng, B, C, ih, iw), k, _f32(rng, B, oh, ow), _f32(rng, C), BLUR_NW


def plain_blur_inputs():
    """x [B, C, 10, 10] and the taps of the plain up = 2 entry."""
    return _f32(_rng(2, 0), BLUR_B, BLUR_C, 10, 10), taps((1, 3, 3, 1))


def run_blur(L, lib, res):
    B, C = BLUR_B, BLUR_C
    for name, ih, iw, t in BLUR:
        x, k, noise, bias, nw = blur_inputs(ih, iw, t)
        kh, (oh, ow) = k.shape[0], noise.shape[1:]
        xd, kd, nd, bd, nwd = dev(x), dev(k), dev(noise), dev(bias), dev([nw])
        for entry, nz in (("shared", nd[0].contiguous()), ("ps", nd)):
            y = torch.full((B, C, oh, ow), float("nan"), device="cuda")
            fn = L.g2s_upfirdn2d_nba if entry == "shared" else L.g2s_upfirdn2d_nba_ps
            lib.check(fn(lib.ptr(xd), lib.ptr(kd), lib.ptr(y), B * C, C, ih, iw, kh, kh, 1, 1, 1, 1, 1, 1, lib.ptr(bd),
                         lib.ptr(nz), lib.ptr(nwd), ALPHA, GAIN, lib.stream()))
            res[f"blur.{name}.{entry}"] = y
    # the plain entry shares the store: no tail, up = 2 (the polyphase path), float32 and float16
    x, k = plain_blur_inputs()
    kd = dev(k)
    for dname, dtype, code in (("f32", torch.float32, 0), ("f16", torch.float16, 1)):
        xd = dev(x).to(dtype)
        y = torch.full((B, C, 19, 19), float("nan"), device="cuda", dtype=dtype)
        lib.check(L.g2s_upfirdn2d(lib.ptr(xd), lib.ptr(kd), lib.ptr(y), B * C, 10, 10, 4, 4, 2, 2, 1, 1, 1, 1, 1, 1,
                                  code, lib.stream()))
        res[f"blur.plain_up2.{dname}"] = y


def rows_inputs(B, C, H):
    """x, g1, g2 [B, C, n], s1, s2, demod [B, C], noise [B, n], bias [C], noise weight (numpy, float32)."""
    n = H * H
    rng = _rng(3, B, C, H)
    x, g1, g2 = _f32(rng, B, C, n), _f32(rng, B, C, n), _f32(rng, B, C, n)
    s1, s2, demod = _f32(rng, B, C), _f32(rng, B, C), (0.5 + rng.random((B, C))).astype(np.float32)
    noise, bias = _f32(rng, B, n), _f32(rng, C)
    return x, g1, g2, s1, s2, demod, noise, bias, ROWS_NW


def run_rows(L, lib, res):
    for B, C, H in ROWS:
        n = H * H
        x, g1, g2, s1, s2, demod, noise, bias, nw = rows_inputs(B, C, H)
        xd, g1d, g2d, s1d, s2d, dmd, nd, bd, nwd = (dev(a) for a in (x, g1, g2, s1, s2, demod, noise, bias, [nw]))
        for entry, nz in (("shared", nd[0].contiguous()), ("ps", nd)):
            fn = L.g2s_synth_bwd_rows if entry == "shared" else L.g2s_synth_bwd_rows_ps
            for two in (False, True):
                for with_gdot in (False, True):
                    out = torch.full((B, C, n), float("nan"), device="cuda")
                    dot1, dot2, gdot = (torch.full((B, C), float("nan"), device="cuda") for _ in range(3))
                    lib.check(fn(lib.ptr(xd), lib.ptr(g1d), lib.ptr(s1d), lib.ptr(g2d if two else None),
                                 lib.ptr(s2d if two else None), lib.ptr(nz), lib.ptr(nwd), lib.ptr(bd), lib.ptr(dmd),
                                 lib.ptr(out), lib.ptr(dot1), lib.ptr(dot2 if two else None),
                                 lib.ptr(gdot if with_gdot else None), B * C, C, n, ALPHA, GAIN, lib.stream()))
                    key = f"rows.{B}x{C}x{H}.{entry}.g2_{int(two)}.gdot_{int(with_gdot)}"
                    res[key + ".out"], res[key + ".dot1"] = out, dot1
                    if two:
                        res[key + ".dot2"] = dot2
                    if with_gdot:
                        res[key + ".gdot"] = gdot


WL1_G, WL1_DEN, WL1_COEF, WL1_ADD_SCALE = 0.7, 3.0, 0.3, 2 ** -0.5


def wl1_inputs():
    """x, y, gadd, gadd2, gate reference [B, C, HW] and w [B, HW] (numpy, float32)."""
    B, C, HW = WL1
    rng = _rng(4)
    x, y, gadd, gadd2, ref = (_f32(rng, B, C, HW) for _ in range(5))
    y[:, :, 2] = x[:, :, 2]                      # ties: sign(0) = 0
    w = rng.random((B, HW)).astype(np.float32)
    return x, y, w, gadd, gadd2, ref


def run_wl1(L, lib, res):
    B, C, HW = WL1
    xd, yd, wd, ad, a2d, rd = (dev(a) for a in wl1_inputs())
    g, den, coef = dev([WL1_G]), dev([WL1_DEN]), dev([WL1_COEF])
    sz = (B, C, HW)
    new = lambda: torch.full(sz, float("nan"), device="cuda")      # noqa: E731
    p, st = lib.ptr, lib.stream
    for wname, wv in (("w", wd), ("now", None)):
        o = res[f"wl1.{wname}.bwd"] = new()
        lib.check(L.g2s_weighted_l1_bwd(p(xd), p(yd), p(wv), p(coef), p(o), *sz, st()))
        for aname, av in (("noadd", None), ("add", ad)):
            o = res[f"wl1.{wname}.bwd2.{aname}"] = new()
            lib.check(L.g2s_weighted_l1_bwd2(p(xd), p(yd), p(wv), p(g), p(den), p(av), p(o), *sz, st()))
        for xo, na in WL1_COMBOS:
            if not xo and wv is None:
                continue                         # w belongs to the L1 term: without x there is one combination
            for outs in ("gx", "gate", "both"):
                gx = new() if outs != "gate" else None
                gq = new() if outs != "gx" else None
                lib.check(L.g2s_weighted_l1_bwd3(
                    p(xd if xo else None), p(yd if xo else None), p(wv if xo else None), p(g if xo else None),
                    p(den if xo else None), p(ad if na else None), p(a2d if na == 2 else None), WL1_ADD_SCALE, p(gx),
                    p(rd if gq is not None else None), ALPHA, GAIN, p(gq), *sz, st()))
                if gx is not None:
                    res[f"wl1.{wname}.bwd3.x{xo}a{na}.{outs}.gx"] = gx
                if gq is not None:
                    res[f"wl1.{wname}.bwd3.x{xo}a{na}.{outs}.gate"] = gq


def demod_inputs(B, Cin, Cout):
    """wsq [Cout, Cin], s [B, Cin], gd [B, Cout], gs_add [B, Cin] (numpy, float32)."""
    rng = _rng(5, B, Cin, Cout)
    wsq = (rng.random((Cout, Cin)) + 0.1).astype(np.float32)
    return wsq, _f32(rng, B, Cin), _f32(rng, B, Cout), _f32(rng, B, Cin)


def _demod_inputs(B, Cin, Cout):
    return [dev(a) for a in demod_inputs(B, Cin, Cout)]


def run_demod(L, lib, res):
    p, st, C = lib.ptr, lib.stream, lib.C
    for B, Cin, Cout in DEMOD:
        wsq, s, gd, gs_add = _demod_inputs(B, Cin, Cout)
        key = f"demod.{B}x{Cin}x{Cout}"
        dm = res[key + ".fwd"] = torch.full((B, Cout), float("nan"), device="cuda")
        lib.check(L.g2s_demod_fwd(p(wsq), p(s), p(dm), B, Cin, Cout, EPS, st()))
        gs = res[key + ".bwd"] = torch.full((B, Cin), float("nan"), device="cuda")
        lib.check(L.g2s_demod_bwd(p(wsq), p(s), p(dm), p(gd), p(gs), B, Cin, Cout, st()))
        gs = res[key + ".bwd_add"] = torch.full((B, Cin), float("nan"), device="cuda")
        lib.check(L.g2s_demod_bwd_add(p(wsq), p(s), p(dm), p(gd), p(gs_add), p(gs), B, Cin, Cout, st()))
        gs = res[key + ".bwd_add_inplace"] = gs_add.clone()
        lib.check(L.g2s_demod_bwd_add(p(wsq), p(s), p(dm), p(gd), p(gs), p(gs), B, Cin, Cout, st()))
    B, n = DEMOD_MULTI_B, len(DEMOD)
    ins = [_demod_inputs(B, Cin, Cout) for _, Cin, Cout in DEMOD]
    dms = [torch.full((B, Cout), float("nan"), device="cuda") for _, _, Cout in DEMOD]
    gss = [i[3].clone() for i in ins]            # the multi backward adds in place
    arr = lambda ts: (C.c_void_p * n)(*[t.data_ptr() for t in ts])      # noqa: E731
    cin, cout = (C.c_int * n)(*[d[1] for d in DEMOD]), (C.c_int * n)(*[d[2] for d in DEMOD])
    wsqs, ss, gds = arr([i[0] for i in ins]), arr([i[1] for i in ins]), arr([i[2] for i in ins])
    lib.check(L.g2s_demod_fwd_multi(wsqs, ss, arr(dms), cin, cout, n, B, EPS, st()))
    lib.check(L.g2s_demod_bwd_multi(wsqs, ss, arr(dms), gds, arr(gss), cin, cout, n, B, st()))
    for l, (_, Cin, Cout) in enumerate(DEMOD):
        res[f"demod.multi.{Cin}x{Cout}.fwd"], res[f"demod.multi.{Cin}x{Cout}.bwd"] = dms[l], gss[l]


GROUPS = dict(tail=run_tail, blur=run_blur, rows=run_rows, wl1=run_wl1, demod=run_demod)


def run(L, lib):
    """Every case through the exported entries: {name: device tensor}, names prefixed by their group."""
    res = {}
    for fn in GROUPS.values():
        fn(L, lib, res)
    torch.cuda.synchronize()
    return res
