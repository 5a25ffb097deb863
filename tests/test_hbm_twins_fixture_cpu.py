"""tests/golden/hbm_twins_parent.npz against a float64 numpy restatement, on the CPU.

tests/test_gpu_hbm_twins.py holds the library to the recorded bits of one commit; a recording is only as right as the
build it came from.  Here every recorded output is computed again in float64 from the inputs of hbm_twins_cases (the
numpy draws, no device) by the formulas of include/g2s.h: the StyledConv tail, the blur with the tail in its store
(all tile shapes, the generic fallback, the plain up = 2 entry in float32 and float16), the backward row pass with
every optional output, the weighted-L1 backward entries, single- and multi-layer demodulation.

Bounds.  A float32 output is a few rounded operations per element (the blur: 16 products; the rows: sums of 9 or 16
terms; the demodulation: up to 70): every recorded float32 tensor lies within 6e-7 of max|ref| of float64, about four
times the worst measured (per group: tail 8.4e-8, blur 1.33e-7 at the 160-wide tile, rows 1.10e-7, weighted L1 9.0e-8,
demodulation 1.43e-7 at demod.3x70x9.bwd, the multi-layer entries included; the recorded float16 blur is within
0.5 ulp).  The float16 blur accumulates in float32 and rounds once: within
one float16 ulp (at the reference's magnitude) of the float64 blur of the float16-rounded input.  Scalars that reach the
kernels as float32 (noise weight, slope, gain, eps, g, den, coef, add_scale) are rounded to float32 first; the backward
demodulation is fed the recorded forward `demod`, as the kernel was."""
import numpy as np
import pytest

import hbm_twins_cases as hc

F32_BOUND = 6e-7
f32 = lambda v: float(np.float32(v))          # noqa: E731
ALPHA, GAIN = f32(hc.ALPHA), f32(hc.GAIN)


@pytest.fixture(scope="module")
def fx(golden):
    return golden("hbm_twins_parent")


def d(a):
    return np.asarray(a, np.float64)


def lrelu(v, slope=ALPHA):
    return np.where(v > 0, v, v * slope)


def upfirdn2d(x, k, up, pad):
    """x [..., H, W], zeros inserted (up), padded by `pad` on every side, correlated with the flipped taps."""
    H, W = x.shape[-2:]
    kh, kw = k.shape
    z = np.zeros(x.shape[:-2] + (H * up + 2 * pad, W * up + 2 * pad))
    z[..., pad:pad + H * up:up, pad:pad + W * up:up] = x
    oh, ow = z.shape[-2] - kh + 1, z.shape[-1] - kw + 1
    kf = k[::-1, ::-1]
    out = np.zeros(x.shape[:-2] + (oh, ow))
    for i in range(kh):
        for j in range(kw):
            out += kf[i, j] * z[..., i:i + oh, j:j + ow]
    return out


# ----------------------------------------------------------------------------- float64 restatement: {name: array}
def ref_tail():
    res = {}
    for name, B, C, HW, variant in hc.TAIL:
        x, noise, bias, nw = hc.tail_inputs(B, C, HW)
        x, noise, bias, nw = d(x), d(noise), d(bias), f32(nw)
        for entry, nz in (("shared", noise[:1]), ("ps", noise)):
            if variant == "nonoise":
                if entry == "ps":
                    continue
                nz = np.zeros((1, HW))
            res[f"tail.{name}.{entry}"] = GAIN * lrelu(x + nw * nz[:, None, :] + bias[None, :, None])
    return res


def ref_blur():
    res = {}
    for name, ih, iw, t in hc.BLUR:
        x, k, noise, bias, nw = hc.blur_inputs(ih, iw, t)
        y = upfirdn2d(d(x), d(k), 1, 1)
        for entry, nz in (("shared", d(noise)[:1]), ("ps", d(noise))):
            res[f"blur.{name}.{entry}"] = GAIN * lrelu(y + f32(nw) * nz[:, None] + d(bias)[None, :, None, None])
    x, k = hc.plain_blur_inputs()
    res["blur.plain_up2.f32"] = upfirdn2d(d(x), d(k), 2, 1)
    res["blur.plain_up2.f16"] = upfirdn2d(d(x.astype(np.float16)), d(k), 2, 1)
    return res


def ref_rows():
    res = {}
    for B, C, H in hc.ROWS:
        x, g1, g2, s1, s2, demod, noise, bias, nw = hc.rows_inputs(B, C, H)
        x, g1, g2, s1, s2, demod, noise, bias = (d(a) for a in (x, g1, g2, s1, s2, demod, noise, bias))
        gate = GAIN * np.where(x > 0, 1.0, ALPHA)
        for entry, nz in (("shared", noise[:1]), ("ps", noise)):
            yconv = np.where(x > 0, x, x / ALPHA) / GAIN - f32(nw) * nz[:, None, :] - bias[None, :, None]
            for two in (False, True):
                out = (g1 * s1[..., None] + (g2 * s2[..., None] if two else 0.0)) * gate
                for with_gdot in (False, True):
                    key = f"rows.{B}x{C}x{H}.{entry}.g2_{int(two)}.gdot_{int(with_gdot)}"
                    res[key + ".out"], res[key + ".dot1"] = out, (x * g1).sum(-1)
                    if two:
                        res[key + ".dot2"] = (x * g2).sum(-1)
                    if with_gdot:
                        res[key + ".gdot"] = (out * yconv).sum(-1) / demod
    return res


def ref_wl1():
    res = {}
    x, y, w, gadd, gadd2, ref = (d(a) for a in hc.wl1_inputs())
    g, den, coef, add_scale = f32(hc.WL1_G), f32(hc.WL1_DEN), f32(hc.WL1_COEF), f32(hc.WL1_ADD_SCALE)
    sgn = np.sign(x - y)
    gate = GAIN * np.where(ref > 0, 1.0, ALPHA)
    for wname, wv in (("w", w[:, None, :]), ("now", None)):
        sw = sgn * (1.0 if wv is None else wv)
        res[f"wl1.{wname}.bwd"] = sw * coef
        res[f"wl1.{wname}.bwd2.noadd"] = sw * g / den
        res[f"wl1.{wname}.bwd2.add"] = gadd + sw * g / den
        for xo, na in hc.WL1_COMBOS:
            if not xo and wv is None:
                continue
            gx = sw * g / den if xo else np.zeros_like(x)
            if na:
                gx = (gadd + gadd2 if na == 2 else gadd) * add_scale + gx
            for outs in ("gx", "gate", "both"):
                if outs != "gate":
                    res[f"wl1.{wname}.bwd3.x{xo}a{na}.{outs}.gx"] = gx
                if outs != "gx":
                    res[f"wl1.{wname}.bwd3.x{xo}a{na}.{outs}.gate"] = gx * gate
    return res


def _demod_bwd(wsq, s, demod, gd):
    return -s * ((gd * demod ** 3) @ wsq)


def ref_demod(fx):
    res = {}
    eps = f32(hc.EPS)
    for B, Cin, Cout in hc.DEMOD:
        wsq, s, gd, gs_add = (d(a) for a in hc.demod_inputs(B, Cin, Cout))
        key = f"demod.{B}x{Cin}x{Cout}"
        res[key + ".fwd"] = 1.0 / np.sqrt((s * s) @ wsq.T + eps)
        bwd = _demod_bwd(wsq, s, d(fx[key + ".fwd"]), gd)
        res[key + ".bwd"], res[key + ".bwd_add"], res[key + ".bwd_add_inplace"] = bwd, gs_add + bwd, gs_add + bwd
    for _, Cin, Cout in hc.DEMOD:
        wsq, s, gd, gs_add = (d(a) for a in hc.demod_inputs(hc.DEMOD_MULTI_B, Cin, Cout))
        key = f"demod.multi.{Cin}x{Cout}"
        res[key + ".fwd"] = 1.0 / np.sqrt((s * s) @ wsq.T + eps)
        res[key + ".bwd"] = gs_add + _demod_bwd(wsq, s, d(fx[key + ".fwd"]), gd)
    return res


REFS = dict(tail=lambda fx: ref_tail(), blur=lambda fx: ref_blur(), rows=lambda fx: ref_rows(),
            wl1=lambda fx: ref_wl1(), demod=ref_demod)


def test_the_restatement_covers_the_groups_of_the_gpu_test():
    assert set(REFS) == set(hc.GROUPS)


@pytest.mark.parametrize("group", list(REFS))
def test_recorded_outputs_are_float64_correct(fx, group):
    ref = REFS[group](fx)
    names = sorted(k for k in fx if k.startswith(group + "."))
    assert names and set(names) == set(ref), sorted(set(names) ^ set(ref))
    worst, bad = ("", 0.0), []
    for k in names:
        got, want = fx[k], ref[k]
        assert got.shape == want.shape, k
        err = np.abs(d(got) - want)
        if got.dtype == np.float16:
            ulp = d(np.spacing(np.abs(want).astype(np.float16)))
            r = float((err / ulp).max())
            print(f"{k}: float16, max error {r:.3f} ulp")
            if not r <= 1.0:
                bad.append(f"{k}: {r:.3f} float16 ulp")
            continue
        assert got.dtype == np.float32, k
        r = float(err.max() / np.abs(want).max())
        worst = max(worst, (k, r), key=lambda t: t[1])
        if not r <= F32_BOUND:
            bad.append(f"{k}: {r:.3e} of max|ref|")
    print(f"[{group}] {len(names)} outputs, worst float32 error {worst[1]:.3e} of max|ref| ({worst[0]})")
    assert not bad, "\n".join(bad)
