"""-m gpu: g2s_rows_dot_scale, g2s_demod_fwd / _bwd / _bwd_add, g2s_demod_fwd_multi / _bwd_multi and g2s_channel_sum
(csrc/rowops.hip) through the C ABI against the float64 reference of tests/rowops_cases.py (cases, reference and bounds
are described there): the head / body / tail kernel and the all-scalar one (a pointer one float off alignment), NULL
operands, in-place operands, idle waves and the early exits of the multi-layer grid.

Every tensor is a view into a canary-filled buffer: inputs must be unchanged and the canaries around the outputs intact;
a NULL output has a spare canary buffer that must stay untouched.  Refusals are checked by return code."""
import ctypes

import numpy as np
import pytest
import torch

import rowops_cases as rc
from canary_buffers import CANARY, Buffers, within

pytestmark = pytest.mark.gpu
RATIO = {}


@pytest.fixture(scope="module")
def g2s():
    import gan2shape_amd  # noqa: F401
    from gan2shape_amd import lib
    return lib.load()  # fails loudly if libg2s.so is missing


def _note(key, r):
    RATIO[key] = max(RATIO.get(key, 0.0), r)


def _ptrs(ts):
    return (ctypes.c_void_p * len(ts))(*[None if t is None else t.data_ptr() for t in ts])


def _ints(v):
    return (ctypes.c_int * len(v))(*v)


@pytest.mark.parametrize("name", [c["name"] for c in rc.CASES if c["entry"] == "rds"])
def test_rows_dot_scale(g2s, name):
    from gan2shape_amd import lib
    c, d, exp = rc.CASE[name], rc.inputs(name), rc.expected(name)
    rows, n = c["shape"]
    bufs = Buffers()
    sh = lambda k: 1 if k in c["mis"] else 0
    a = bufs.view("a", d["a"], shift=sh("a"))
    b = bufs.view("b", d["b"], shift=sh("b"), out=c["out"] == "b")
    s, inv = bufs.view("s", d["s"]), bufs.view("inv", d["inv"])
    out = b if c["out"] == "b" else (bufs.view("out", like=d["b"], shift=sh("out")) if c["out"] else None)
    dot = bufs.view("dot", like=np.empty(rows)) if c["dot"] else None
    if not c["out"]:
        bufs.spare("out (NULL)", d["b"])
    if not c["dot"]:
        bufs.spare("dot (NULL)", np.empty(rows))
    lib.check(g2s.g2s_rows_dot_scale(lib.ptr(a), lib.ptr(b), lib.ptr(s), lib.ptr(inv), lib.ptr(out), lib.ptr(dot), rows, n,
                                     lib.stream()))
    torch.cuda.synchronize()
    bufs.check()
    msg = f"{name} {rc.dispatch(c)}:"
    if c["out"]:
        np.testing.assert_array_equal(out.cpu().numpy().reshape(rows, n), exp["out"][0], err_msg=name)
        msg += " out bit for bit"
    if c["dot"]:
        r = within(dot.cpu().numpy(), *exp["dot"], "dot")
        _note("rds dot", r)
        msg += f" dot error / bound {r:.3f}"
    print(msg)


def test_rows_dot_scale_refusals(g2s):
    from gan2shape_amd import lib
    d = rc.inputs("rds_5x7_full")
    bufs = Buffers()
    a, b = bufs.view("a", d["a"]), bufs.view("b", d["b"])
    out, dot = bufs.spare("out", d["b"]), bufs.spare("dot", np.empty(5))
    P, st = lib.ptr, lib.stream()
    assert g2s.g2s_rows_dot_scale(P(a), P(b), None, None, None, None, 5, 7, st) == -1        # nothing to compute
    assert g2s.g2s_rows_dot_scale(None, P(b), None, None, P(out), P(dot), 5, 7, st) == -1     # dot without a
    assert g2s.g2s_rows_dot_scale(P(a), None, None, None, P(out), P(dot), 5, 7, st) == -1
    assert g2s.g2s_rows_dot_scale(P(a), P(b), None, None, P(out), P(dot), 0, 7, st) == -1
    torch.cuda.synchronize()
    bufs.check()
    assert (out == CANARY).all() and (dot == CANARY).all()


@pytest.mark.parametrize("name", [c["name"] for c in rc.CASES if c["entry"] == "demod_fwd"])
def test_demod_fwd(g2s, name):
    from gan2shape_amd import lib
    c, d, exp = rc.CASE[name], rc.inputs(name), rc.expected(name)
    B, Cin, Cout = c["shape"]
    bufs = Buffers()
    wsq, s = bufs.view("wsq", d["wsq"]), bufs.view("s", d["s"])
    demod = bufs.view("demod", like=d["demod"])
    lib.check(g2s.g2s_demod_fwd(lib.ptr(wsq), lib.ptr(s), lib.ptr(demod), B, Cin, Cout, rc.EPS, lib.stream()))
    torch.cuda.synchronize()
    bufs.check()
    r = within(demod.cpu().numpy().reshape(B, Cout), *exp["demod"], "demod")
    _note("demod fwd", r)
    print(f"{name} {rc.dispatch(c)}: demod error / bound {r:.3f}")


@pytest.mark.parametrize("name", [c["name"] for c in rc.CASES if c["entry"] == "demod_bwd"])
def test_demod_bwd(g2s, name):
    from gan2shape_amd import lib
    c, d, exp = rc.CASE[name], rc.inputs(name), rc.expected(name)
    B, Cin, Cout = c["shape"]
    bufs = Buffers()
    wsq, s, demod, gd = (bufs.view(k, d[k]) for k in ("wsq", "s", "demod", "gd"))
    P, st = lib.ptr, lib.stream()
    if c["add"] is None:
        gs = bufs.view("gs", like=d["s"])
        rcode = g2s.g2s_demod_bwd(P(wsq), P(s), P(demod), P(gd), P(gs), B, Cin, Cout, st)
    elif c["add"] == "sep":
        add, gs = bufs.view("gs_add", d["gs_add"]), bufs.view("gs", like=d["s"])
        rcode = g2s.g2s_demod_bwd_add(P(wsq), P(s), P(demod), P(gd), P(add), P(gs), B, Cin, Cout, st)
    else:
        gs = bufs.view("gs", d["gs_add"], out=True)
        rcode = g2s.g2s_demod_bwd_add(P(wsq), P(s), P(demod), P(gd), P(gs), P(gs), B, Cin, Cout, st)
    lib.check(rcode)
    torch.cuda.synchronize()
    bufs.check()
    r = within(gs.cpu().numpy().reshape(B, Cin), *exp["gs"], "gs")
    _note("demod bwd", r)
    print(f"{name} {rc.dispatch(c)}: gs error / bound {r:.3f}")


def _multi(bufs):
    d = rc.inputs("multi_bwd")
    L = range(len(rc.MULTI_LAYERS))
    t = {k: [bufs.view(f"{k}{l}", d[f"{k}{l}"]) for l in L] for k in ("wsq", "s", "demod", "gd")}
    return d, L, t


def test_demod_fwd_multi(g2s):
    from gan2shape_amd import lib
    c, exp = rc.CASE["multi_fwd"], rc.expected("multi_fwd")
    bufs = Buffers()
    d = rc.inputs("multi_fwd")
    L = range(len(rc.MULTI_LAYERS))
    wsq, s = ([bufs.view(f"{k}{l}", d[f"{k}{l}"]) for l in L] for k in ("wsq", "s"))
    demod = [bufs.view(f"demod{l}", like=d[f"demod{l}"]) for l in L]
    cin, cout = zip(*rc.MULTI_LAYERS)
    lib.check(g2s.g2s_demod_fwd_multi(_ptrs(wsq), _ptrs(s), _ptrs(demod), _ints(cin), _ints(cout), len(L), rc.MULTI_B, rc.EPS,
                                      lib.stream()))
    torch.cuda.synchronize()
    bufs.check()
    for l in L:
        r = within(demod[l].cpu().numpy().reshape(rc.MULTI_B, cout[l]), *exp[f"demod{l}"], f"demod{l}")
        _note("multi fwd", r)
        print(f"multi_fwd layer {l} {rc.MULTI_LAYERS[l]} {rc.dispatch(c)}: demod error / bound {r:.3f}")


def test_demod_bwd_multi(g2s):
    from gan2shape_amd import lib
    c, exp = rc.CASE["multi_bwd"], rc.expected("multi_bwd")
    bufs = Buffers()
    d, L, t = _multi(bufs)
    gs = [bufs.view(f"gs{l}", d[f"gs_add{l}"], out=True) for l in L]          # pre-filled: the entry adds in place
    cin, cout = zip(*rc.MULTI_LAYERS)
    lib.check(g2s.g2s_demod_bwd_multi(_ptrs(t["wsq"]), _ptrs(t["s"]), _ptrs(t["demod"]), _ptrs(t["gd"]), _ptrs(gs), _ints(cin),
                                      _ints(cout), len(L), rc.MULTI_B, lib.stream()))
    torch.cuda.synchronize()
    bufs.check()
    for l in L:
        r = within(gs[l].cpu().numpy().reshape(rc.MULTI_B, cin[l]), *exp[f"gs{l}"], f"gs{l}")
        _note("multi bwd", r)
        print(f"multi_bwd layer {l} {rc.MULTI_LAYERS[l]} {rc.dispatch(c)}: gs error / bound {r:.3f}")


def test_demod_multi_refusals(g2s):
    from gan2shape_amd import lib
    bufs = Buffers()
    d, L, t = _multi(bufs)
    gs = [bufs.view(f"gs{l}", d[f"gs_add{l}"]) for l in L]                    # inputs here: nothing may change
    cin, cout = zip(*rc.MULTI_LAYERS)
    st = lib.stream()
    big = rc.MAX_LAYERS + 1
    rep = lambda ts: _ptrs([ts[i % len(ts)] for i in range(big)])
    for layers in (0, big):
        assert g2s.g2s_demod_fwd_multi(rep(t["wsq"]), rep(t["s"]), rep(t["demod"]), _ints([cin[i % 3] for i in range(big)]),
                                       _ints([cout[i % 3] for i in range(big)]), layers, rc.MULTI_B, rc.EPS, st) == -1
        assert g2s.g2s_demod_bwd_multi(rep(t["wsq"]), rep(t["s"]), rep(t["demod"]), rep(t["gd"]), rep(gs),
                                       _ints([cin[i % 3] for i in range(big)]), _ints([cout[i % 3] for i in range(big)]),
                                       layers, rc.MULTI_B, st) == -1
    gd_null = list(t["gd"])
    gd_null[1] = None
    assert g2s.g2s_demod_bwd_multi(_ptrs(t["wsq"]), _ptrs(t["s"]), _ptrs(t["demod"]), _ptrs(gd_null), _ptrs(gs), _ints(cin),
                                   _ints(cout), len(L), rc.MULTI_B, st) == -1
    assert g2s.g2s_demod_bwd_multi(_ptrs(t["wsq"]), _ptrs(t["s"]), _ptrs(t["demod"]), None, _ptrs(gs), _ints(cin),
                                   _ints(cout), len(L), rc.MULTI_B, st) == -1
    torch.cuda.synchronize()
    bufs.check()


@pytest.mark.parametrize("name", [c["name"] for c in rc.CASES if c["entry"] == "csum"])
def test_channel_sum(g2s, name):
    from gan2shape_amd import lib
    c, d, exp = rc.CASE[name], rc.inputs(name), rc.expected(name)
    B, C, n = c["shape"]
    bufs = Buffers()
    g, out = bufs.view("g", d["g"]), bufs.view("out", like=np.empty(C))
    lib.check(g2s.g2s_channel_sum(lib.ptr(g), lib.ptr(out), B, C, n, lib.stream()))
    torch.cuda.synchronize()
    bufs.check()
    r = within(out.cpu().numpy(), *exp["out"], "out")
    _note("csum", r)
    print(f"{name} {rc.dispatch(c)}: error / bound {r:.3f}")


def test_largest_error_over_bound():
    """Runs last in this file: the figures recorded in the docstring of tests/rowops_cases.py."""
    print("rowops: largest error / bound", {k: round(v, 3) for k, v in sorted(RATIO.items())})
    assert all(v <= 1.0 for v in RATIO.values())
