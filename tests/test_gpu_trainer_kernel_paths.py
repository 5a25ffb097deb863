"""-m gpu: g2s_mbstd_fwd / _bwd / _bwd2, g2s_d_logistic, g2s_r1_penalty (csrc/dtrain.hip), g2s_path_penalty,
g2s_g_nonsaturating and g2s_ema_accumulate (csrc/gtrain.hip) through the C ABI against the float64 reference of
tests/trainer_kernel_cases.py (cases, reference and bounds are described there): every trip count of the strided loops,
ragged tails, G and M of 1, 2 and 3, NULL gradients, Br != Bf, rows of zeros, B = GH_MAXB, the vector and scalar EMA
paths at every alignment and the bisection six levels deep.

Every tensor is a view into a canary-filled buffer: inputs must be unchanged bit for bit and the canaries around every
output intact (`partial` at exactly B * chunks floats, out[4], stats[3], lengths[B]); a spare buffer stands where a NULL
output would have been.  Every call is made twice on fresh buffers and the results must be equal bit for bit: fixed
summation order, no atomics.  Refusals are checked by return code, with canaries where an output would be."""
import numpy as np
import pytest
import torch

import trainer_kernel_cases as tk
from canary_buffers import CANARY, Buffers, within

pytestmark = pytest.mark.gpu
RATIO = {}
INVALID = -1          # G2S_ERR_INVALID


@pytest.fixture(scope="module")
def g2s():
    import gan2shape_amd  # noqa: F401
    from gan2shape_amd import lib
    return lib.load()  # fails loudly if libg2s.so is missing


def _names(entry):
    return [c["name"] for c in tk.by_entry(entry)]


def _np(t, shape):
    return t.cpu().numpy().reshape(shape)


def _twice(call):
    """The outputs of `call()` (name -> float32 array); a second call on fresh buffers gives the same bits."""
    a, b = call(), call()
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), f"{k}: two calls differ"
    return a


def _hold(name, key, got, msg):
    """Every output of `got` against the reference of case `name`; notes the largest error / bound under `key`."""
    e = tk.expected(name)
    for k, v in got.items():
        want = np.asarray(e["ref64"][k]).reshape(v.shape)
        bound = np.broadcast_to(np.asarray(e["bound"][k], np.float64), v.shape)
        r = within(np.atleast_1d(v), np.atleast_1d(want), np.atleast_1d(bound), f"{name} {k}")
        RATIO[key] = max(RATIO.get(key, 0.0), r)
        msg.append(f"{k} {'exact' if k in e['exact'] else format(r, '.3f')}")


# ---------------------------------------------------------------------------------------- minibatch stddev
def _mbstd(g2s, name):
    from gan2shape_amd import lib
    c, i = tk.CASE[name], tk.inputs(name)
    B, C, H, W, feat = c["shape"]
    P, st = lib.ptr, lib.stream()
    res = {}
    for entry in ("fwd", "bwd", "bwd2"):
        bufs = Buffers()
        x = bufs.view("x", i["x"])
        if entry == "fwd":
            out = bufs.view("out", like=i["gout"])
            lib.check(g2s.g2s_mbstd_fwd(P(x), P(out), B, C, H, W, feat, st))
        elif entry == "bwd":
            gout, gx = bufs.view("gout", i["gout"]), bufs.view("gx", like=i["x"])
            lib.check(g2s.g2s_mbstd_bwd(P(gout), P(x), P(gx), B, C, H, W, feat, st))
        else:
            ggx, gout = bufs.view("ggx", i["ggx"]), bufs.view("gout", i["gout"])
            ggout, xg = bufs.view("ggout", like=i["gout"]), bufs.view("xg", like=i["x"])
            lib.check(g2s.g2s_mbstd_bwd2(P(ggx), P(gout), P(x), P(ggout), P(xg), B, C, H, W, feat, st))
        torch.cuda.synchronize()
        bufs.check()
        if entry == "fwd":
            o = _np(out, (B, C + feat, H, W))
            res.update({"out.copy": o[:, :C].copy(), "out.map": o[:, C:].copy()})
        elif entry == "bwd":
            res["gx"] = _np(gx, (B, C, H, W))
        else:
            o = _np(ggout, (B, C + feat, H, W))
            res.update({"ggout.copy": o[:, :C].copy(), "ggout.map": o[:, C:].copy(), "xg": _np(xg, (B, C, H, W))})
    return res


@pytest.mark.parametrize("name", _names("mbstd"))
def test_minibatch_stddev_paths(g2s, name):
    c = tk.CASE[name]
    got = _twice(lambda: _mbstd(g2s, name))
    msg = [f"{name} {sorted(tk.dispatch(c))}:"]
    for key, outs in (("mbstd_fwd", ("out.copy", "out.map")), ("mbstd_bwd", ("gx",)), ("mbstd_bwd2", ("ggout.copy", "ggout.map", "xg"))):
        _hold(name, key, {k: got[k] for k in outs}, msg)
    if c["exact"]:
        assert np.isfinite(got["xg"]).all()
    print(" ".join(msg), "error / bound")


# --------------------------------------------------------------------------------------------- loss heads
def _d_logistic(g2s, name):
    from gan2shape_amd import lib
    c, i = tk.CASE[name], tk.inputs(name)
    Br, Bf = c["shape"]
    bufs = Buffers()
    real, fake, out = bufs.view("real", i["real"]), bufs.view("fake", i["fake"]), bufs.view("out", like=np.empty(4))
    grads = {}
    for k, like in (("g_real", i["real"]), ("g_fake", i["fake"])):
        grads[k] = None if k in c["null"] else bufs.view(k, like=like)
        if k in c["null"]:
            bufs.spare(k + " (NULL)", like)
    lib.check(g2s.g2s_d_logistic(lib.ptr(real), lib.ptr(fake), lib.ptr(out), lib.ptr(grads["g_real"]), lib.ptr(grads["g_fake"]),
                                 Br, Bf, lib.stream()))
    torch.cuda.synchronize()
    bufs.check()
    o = _np(out, (4,))
    res = dict(loss=o[0:1].copy(), mean_real=o[1:2].copy(), mean_fake=o[2:3].copy(), sign=o[3:4].copy())
    res.update({k: _np(v, (-1,)) for k, v in grads.items() if v is not None})
    return res


@pytest.mark.parametrize("name", _names("d_logistic"))
def test_d_logistic_paths(g2s, name):
    got = _twice(lambda: _d_logistic(g2s, name))
    assert ("g_real" in got, "g_fake" in got) == tuple(k not in tk.CASE[name]["null"] for k in ("g_real", "g_fake"))
    msg = [f"{name} {sorted(tk.dispatch(tk.CASE[name]))}:"]
    _hold(name, "d_logistic", got, msg)
    print(" ".join(msg), "error / bound")


def _g_nonsaturating(g2s, name):
    from gan2shape_amd import lib
    c, i = tk.CASE[name], tk.inputs(name)
    bufs = Buffers()
    fake, out = bufs.view("fake", i["fake"]), bufs.view("out", like=np.empty(1))
    g_fake = None if c["null"] else bufs.view("g_fake", like=i["fake"])
    if c["null"]:
        bufs.spare("g_fake (NULL)", i["fake"])
    lib.check(g2s.g2s_g_nonsaturating(lib.ptr(fake), lib.ptr(out), lib.ptr(g_fake), c["shape"][0], lib.stream()))
    torch.cuda.synchronize()
    bufs.check()
    res = dict(loss=_np(out, (1,)))
    if g_fake is not None:
        res["g_fake"] = _np(g_fake, (-1,))
    return res


@pytest.mark.parametrize("name", _names("g_nonsaturating"))
def test_g_nonsaturating_paths(g2s, name):
    got = _twice(lambda: _g_nonsaturating(g2s, name))
    assert ("g_fake" in got) == (not tk.CASE[name]["null"])
    msg = [f"{name} {sorted(tk.dispatch(tk.CASE[name]))}:"]
    _hold(name, "g_nonsaturating", got, msg)
    print(" ".join(msg), "error / bound")


def _r1(g2s, name):
    from gan2shape_amd import lib
    c, i = tk.CASE[name], tk.inputs(name)
    B, n = c["shape"]
    chunks = int(g2s.g2s_r1_penalty_chunks(n))
    assert chunks == -(-n // tk.R1_CHUNK)
    bufs = Buffers()
    grad, per = bufs.view("grad", i["grad"]), bufs.view("per_sample", like=np.empty(B))
    partial = bufs.view("partial", like=np.empty(B * chunks))
    mean = None if c["null"] else bufs.view("mean", like=np.empty(1))
    if c["null"]:
        bufs.spare("mean (NULL)", np.empty(1))
    lib.check(g2s.g2s_r1_penalty(lib.ptr(grad), lib.ptr(per), lib.ptr(mean), lib.ptr(partial), B, n, lib.stream()))
    torch.cuda.synchronize()
    bufs.check()
    res = dict(per_sample=_np(per, (B,)), partial=_np(partial, (B, chunks)))
    if mean is not None:
        res["mean"] = _np(mean, (1,))
    return res


@pytest.mark.parametrize("name", _names("r1"))
def test_r1_penalty_paths(g2s, name):
    got = _twice(lambda: _r1(g2s, name))
    partial = got.pop("partial")
    assert ("mean" in got) == (not tk.CASE[name]["null"])
    # stage 2 adds the chunks of a sample in index order: the same float32 additions here
    acc = np.zeros(partial.shape[0], np.float32)
    for k in range(partial.shape[1]):
        acc = acc + partial[:, k]
    assert np.array_equal(acc, got["per_sample"]), "per_sample is not the chunks of the workspace in index order"
    msg = [f"{name} {sorted(tk.dispatch(tk.CASE[name]))}:"]
    _hold(name, "r1_penalty", got, msg)
    print(" ".join(msg), "error / bound")


def test_r1_penalty_chunks_and_ema_chunk(g2s):
    for n, want in tk.R1_CHUNKS_OF.items():
        assert g2s.g2s_r1_penalty_chunks(n) == want
    assert g2s.g2s_ema_chunk() == tk.EM_CHUNK == 8192


def _path(g2s, name):
    from gan2shape_amd import lib
    c, i = tk.CASE[name], tk.inputs(name)
    B, L, D = c["shape"]
    bufs = Buffers()
    grad, m0 = bufs.view("grad", i["grad"]), bufs.view("mean_path", i["mean_path"])
    lengths, stats = bufs.view("lengths", like=np.empty(B)), bufs.view("stats", like=np.empty(3))
    dgrad = None if c["null"] else bufs.view("dgrad", like=i["grad"])
    if c["null"]:
        bufs.spare("dgrad (NULL)", i["grad"])
    lib.check(g2s.g2s_path_penalty(lib.ptr(grad), lib.ptr(m0), c["decay"], lib.ptr(lengths), lib.ptr(stats), lib.ptr(dgrad), B, L, D,
                                   lib.stream()))
    torch.cuda.synchronize()
    bufs.check()
    s = _np(stats, (3,))
    res = dict(pen=s[0:1].copy(), pm=s[1:2].copy(), mean=s[2:3].copy(), lengths=_np(lengths, (B,)))
    if dgrad is not None:
        res["dgrad"] = _np(dgrad, (B, L, D))
    return res


@pytest.mark.parametrize("name", _names("path"))
def test_path_penalty_paths(g2s, name):
    c = tk.CASE[name]
    got = _twice(lambda: _path(g2s, name))
    assert ("dgrad" in got) == (not c["null"])
    assert all(np.isfinite(v).all() for v in got.values())
    if c["zero"] == "row1":
        assert got["lengths"][1] == 0 and not got["dgrad"][1].any() and got["dgrad"][0].any() and got["dgrad"][2].any()
    msg = [f"{name} {sorted(tk.dispatch(c))}:"]
    _hold(name, "path_penalty", got, msg)
    print(" ".join(msg), "error / bound")


# ---------------------------------------------------------------------------------------------------- EMA
def _ema(g2s, name):
    from gan2shape_amd import lib
    c, i, rows = tk.CASE[name], tk.inputs(name), tk.info(name)["rows"]
    dst, src = torch.from_numpy(i["dst"].copy()).cuda(), torch.from_numpy(i["src"].copy()).cuda()
    assert dst.data_ptr() % 16 == 0 and src.data_ptr() % 16 == 0
    table = torch.tensor([(dst.data_ptr() + 4 * do, src.data_ptr() + 4 * so, n) for do, so, n in rows], dtype=torch.int64).cuda()
    prefix = torch.from_numpy(tk.ema_prefix(c["sizes"])).cuda()
    for (do, so, n), al in zip(rows, c["aligned"]):
        assert ((dst.data_ptr() + 4 * do) % 16 == 0, (src.data_ptr() + 4 * so) % 16 == 0) == tuple(al)
    before = [t.clone() for t in (src, table, prefix)]
    lib.check(g2s.g2s_ema_accumulate(lib.ptr(table), lib.ptr(prefix), len(rows), int(tk.ema_prefix(c["sizes"])[-1]), c["decay"],
                                     c["rest"], lib.stream()))
    torch.cuda.synchronize()
    for t, b, what in zip((src, table, prefix), before, ("src", "table", "chunk prefix")):
        assert torch.equal(t.view(torch.uint8), b.view(torch.uint8)), f"{what} changed"
    return dict(dst=dst.cpu().numpy())


@pytest.mark.parametrize("name", _names("ema"))
def test_ema_accumulate_paths(g2s, name):
    """The whole dst buffer is compared: the bound is 0 on the guard floats between the tensors."""
    c, i = tk.CASE[name], tk.inputs(name)
    got = _twice(lambda: _ema(g2s, name))
    msg = [f"{name} {sorted(tk.dispatch(c))}:"]
    _hold(name, "ema_accumulate", got, msg)
    if name == "ema_keep":
        assert np.array_equal(got["dst"].view(np.uint32), i["dst"].view(np.uint32))
    if name == "ema_rest_0.25":      # the argument is used: far from what 1 - decay would give
        do, so, n = tk.info(name)["rows"][-1]
        other = i["dst"][do:do + n].astype(np.float64) * 0.999 + i["src"][so:so + n].astype(np.float64) * 0.001
        assert np.abs(got["dst"][do:do + n] - other).max() > 0.1
    print(" ".join(msg), "error / bound")


# ---------------------------------------------------------------------------------------------- refusals
def test_refusals_launch_nothing(g2s):
    """By return code; every output is a spare canary buffer that must stay untouched."""
    from gan2shape_amd import lib
    P, st = lib.ptr, lib.stream()
    bufs = Buffers()
    B, C, H, W, feat = 4, 4, 2, 2, 2
    x, gout, ggx = (bufs.view(k, np.ones(s, np.float32)) for k, s in (("x", (8, C, H, W)), ("gout", (8, C + feat, H, W)), ("ggx", (8, C, H, W))))
    out, gx, ggout, xg = (bufs.spare(k, np.empty(s)) for k, s in (("out", (8, C + feat, H, W)), ("gx", (8, C, H, W)),
                                                                 ("ggout", (8, C + feat, H, W)), ("xg", (8, C, H, W))))
    for bad in (dict(B=6), dict(C=5), dict(F=0), dict(B=0), dict(F=3)):
        b, c, f = bad.get("B", B), bad.get("C", C), bad.get("F", feat)
        assert g2s.g2s_mbstd_fwd(P(x), P(out), b, c, H, W, f, st) == INVALID, bad
        assert g2s.g2s_mbstd_bwd(P(gout), P(x), P(gx), b, c, H, W, f, st) == INVALID, bad
        assert g2s.g2s_mbstd_bwd2(P(ggx), P(gout), P(x), P(ggout), P(xg), b, c, H, W, f, st) == INVALID, bad
    for entry, args in ((g2s.g2s_mbstd_fwd, (x, out)), (g2s.g2s_mbstd_bwd, (gout, x, gx)), (g2s.g2s_mbstd_bwd2, (ggx, gout, x, ggout, xg))):
        for k in range(len(args)):
            a = [None if j == k else P(t) for j, t in enumerate(args)]
            assert entry(*a, B, C, H, W, feat, st) == INVALID, (entry, k)

    real, fake = bufs.view("real", np.ones(4, np.float32)), bufs.view("fake", np.ones(4, np.float32))
    lout, g_real, g_fake = (bufs.spare(k, np.empty(4)) for k in ("out", "g_real", "g_fake"))
    for a in ((P(real), P(fake), P(lout), P(g_real), P(g_fake), 0, 4), (P(real), P(fake), P(lout), P(g_real), P(g_fake), 4, 0),
              (P(real), P(fake), None, P(g_real), P(g_fake), 4, 4), (None, P(fake), P(lout), P(g_real), P(g_fake), 4, 4),
              (P(real), None, P(lout), P(g_real), P(g_fake), 4, 4)):
        assert g2s.g2s_d_logistic(*a, st) == INVALID
    for a in ((P(fake), P(lout), P(g_fake), 0), (P(fake), None, P(g_fake), 4), (None, P(lout), P(g_fake), 4)):
        assert g2s.g2s_g_nonsaturating(*a, st) == INVALID

    grad = bufs.view("grad", np.ones((4, 8), np.float32))
    per, mean, partial = (bufs.spare(k, np.empty(n)) for k, n in (("per_sample", 4), ("mean", 1), ("partial", 4)))
    for a in ((P(grad), P(per), P(mean), P(partial), 4, 0), (P(grad), P(per), P(mean), P(partial), 0, 8),
              (P(grad), P(per), P(mean), P(partial), 65536, 8), (P(grad), P(per), P(mean), None, 4, 8),
              (None, P(per), P(mean), P(partial), 4, 8), (P(grad), None, P(mean), P(partial), 4, 8)):
        assert g2s.g2s_r1_penalty(*a, st) == INVALID

    m0 = bufs.view("mean_path", np.full(1, tk.MEAN_PATH, np.float32))
    lengths, stats, dgrad = (bufs.spare(k, np.empty(n)) for k, n in (("lengths", 4), ("stats", 3), ("dgrad", 32)))
    ok = (P(grad), P(m0), 0.01, P(lengths), P(stats), P(dgrad))
    for ptrs, (b, l, d) in ((ok, (0, 2, 4)), (ok, (tk.GH_MAXB + 1, 2, 4)), (ok, (4, 0, 4)), (ok, (4, 2, 0)),
                            (ok[:3] + (None,) + ok[4:], (4, 2, 4)), (ok[:4] + (None,) + ok[5:], (4, 2, 4)),
                            ((ok[0], None) + ok[2:], (4, 2, 4)), ((None,) + ok[1:], (4, 2, 4))):
        assert g2s.g2s_path_penalty(*ptrs, b, l, d, st) == INVALID, (b, l, d)

    dst, src = bufs.spare("ema dst", np.empty(8)), bufs.view("ema src", np.ones(8, np.float32))
    table = torch.tensor([(dst.data_ptr() + 64, src.data_ptr(), 4), (dst.data_ptr() + 80, src.data_ptr() + 16, 4)], dtype=torch.int64).cuda()
    prefix = torch.tensor([0, 1, 2], dtype=torch.int32).cuda()
    for a in ((None, P(prefix), 2, 2), (P(table), None, 2, 2), (P(table), P(prefix), 0, 2), (P(table), P(prefix), 2, 1)):
        assert g2s.g2s_ema_accumulate(*a, 0.5, 0.5, st) == INVALID
    torch.cuda.synchronize()
    bufs.check()
    for t in (out, gx, ggout, xg, lout, g_real, g_fake, per, mean, partial, lengths, stats, dgrad, dst):
        assert (t == CANARY).all()


def test_largest_error_over_bound():
    """Runs last in this file: the figures recorded in MEASURED of tests/trainer_kernel_cases.py."""
    print("trainer kernels: largest error / bound", {k: round(v, 3) for k, v in sorted(RATIO.items())})
    assert all(v <= 1.0 for v in RATIO.values())
