"""The case table and restatement of tests/trainer_kernel_cases.py on the CPU alone: every launch path the table is
there for is reached, every conditioned case meets its condition on the float64 reference, the float64 statements agree
with finite differences, the exact cases are exact in the sequential float32 restatement too, and the zero-row path
penalty is NaN-free and equals the plain statement wherever a length is positive."""
import numpy as np
import pytest
import torch

import dtrain_cases as dc
import gtrain_cases as gc
import trainer_kernel_cases as tk
from trainer_kernel_cases import F64, Ops

DATA_KEYS = sorted({c["data"] for c in tk.CASES})
FIRST = {k: next(c for c in tk.CASES if c["data"] == k) for k in DATA_KEYS}


def _t64(a, grad=True):
    return torch.tensor(np.asarray(a), dtype=F64).requires_grad_(grad)


def _smallest(entry, n=2):
    seen = {}
    for c in tk.by_entry(entry):
        if not c["exact"] and c.get("zero", "none") == "none":
            seen.setdefault(c["shape"], c)
    return sorted(seen.values(), key=lambda c: int(np.prod(c["shape"])))[:n]


# ----------------------------------------------------------------------------- the table reaches what it is there for
def test_every_dispatch_path_is_reached():
    reached = set()
    for c in tk.CASES:
        reached |= tk.dispatch(c)
    assert not tk.PATHS - reached, sorted(tk.PATHS - reached)
    print(len(tk.CASES), "cases,", len(reached), "paths:", sorted(reached))


def test_the_table_holds_the_shapes_of_the_issue():
    def shapes(e):
        return {c["shape"] for c in tk.by_entry(e) if not c["exact"] and c.get("zero", "none") == "none"}
    assert shapes("mbstd") == {(1, 4, 3, 5, 1), (2, 4, 4, 4, 2), (3, 6, 4, 4, 3), (4, 8, 4, 4, 8), (8, 64, 4, 4, 1), (12, 5, 15, 15, 1),
                               (4, 2, 17, 17, 2), (4, 3, 1, 1, 1)}
    assert {min(c["shape"][0], 4) for c in tk.by_entry("mbstd") if c["exact"]} == {1, 2, 4}
    assert shapes("d_logistic") == {(1, 1), (3, 260), (256, 255), (257, 600)}
    for s in shapes("d_logistic"):
        assert {c["null"] for c in tk.by_entry("d_logistic") if c["shape"] == s} == {(), ("g_real",), ("g_fake",), ("g_real", "g_fake")}
    assert shapes("g_nonsaturating") == {(1,), (256,), (257,), (600,)}
    for s in shapes("g_nonsaturating"):
        assert {c["null"] for c in tk.by_entry("g_nonsaturating") if c["shape"] == s} == {(), ("g_fake",)}
    assert shapes("r1") == {(1, 1), (3, 255), (2, 4096), (2, 4097), (3, 8229), (257, 5), (300, 4100)}
    for s in shapes("r1"):
        assert {c["null"] for c in tk.by_entry("r1") if c["shape"] == s} == {(), ("mean",)}
    assert shapes("path") == {(1, 1, 1), (2, 3, 341), (2, 1, 1024), (3, 5, 205), (1024, 1, 3), (5, 14, 512)}
    for s in shapes("path"):
        assert {(c["decay"], c["null"]) for c in tk.by_entry("path") if c["shape"] == s and c["zero"] == "none"} == \
            {(d, n) for d in (0.0, 0.01) for n in ((), ("dgrad",))}
    assert {c["zero"] for c in tk.by_entry("path")} == {"none", "row1", "all"} and tk.CASE["path_zero_row_3x5x205"]["shape"][0] == 3
    assert tk.EMA_SIZES == (1, 3, 8191, 8192, 8193, 16389) and tk.EM_CHUNK == 8192
    for k, al in tk.ALIGNMENTS.items():
        c = tk.CASE[f"ema_sizes_{k}"]
        assert c["sizes"] == tk.EMA_SIZES and set(c["aligned"]) == {al} and c["rest"] == float(np.float32(1 - 0.999))
    c = tk.CASE["ema_table37"]
    assert len(c["sizes"]) == 37 and sum(n == 1 for n in c["sizes"]) >= 4 and len(set(c["aligned"])) == 4
    assert (tk.CASE["ema_keep"]["decay"], tk.CASE["ema_keep"]["rest"]) == (1.0, 0.0)
    assert (tk.CASE["ema_copy"]["decay"], tk.CASE["ema_copy"]["rest"]) == (0.0, 1.0)
    assert tk.CASE["ema_rest_0.25"]["rest"] == 0.25
    assert tk.R1_CHUNKS_OF == {n: (n + tk.R1_CHUNK - 1) // tk.R1_CHUNK if n > 0 else 0 for n in (-1, 0, 1, 4096, 4097)}


@pytest.mark.parametrize("c", tk.by_entry("ema"), ids=lambda c: c["name"])
def test_ema_layout_is_aligned_as_it_says_and_guarded(c):
    rows, nd, ns = tk.ema_layout(c)
    i = tk.inputs(c["name"])
    assert i["dst"].shape == (nd,) and i["src"].shape == (ns,)
    for k, total in ((0, nd), (1, ns)):
        end = 0
        for r, al in zip(rows, c["aligned"]):
            assert r[k] >= end + tk.EMA_GUARD and (r[k] % 4 == 0) == al[k]
            end = r[k] + r[2]
        assert total >= end + tk.EMA_GUARD
    inside = np.zeros(nd, bool)
    for do, _, n in rows:
        inside[do:do + n] = True
    assert (i["dst"][~inside] == tk.EMA_CANARY).all() and not (i["dst"][inside] == tk.EMA_CANARY).any()
    prefix = tk.ema_prefix(c["sizes"])
    assert prefix[0] == 0 and (np.diff(prefix) >= 1).all() and prefix[-1] >= len(c["sizes"])


# ----------------------------------------------------------------------------- conditions, on the float64 reference alone
@pytest.mark.parametrize("c", tk.by_entry("mbstd"), ids=lambda c: c["name"])
def test_stddev_cases_meet_their_condition(c):
    i, inf = tk.inputs(c["name"]), tk.info(c["name"])
    B, C, H, W, feat = c["shape"]
    G = min(B, tk.MB_MAXG)
    assert inf["seed"] in tk.SEEDS and B % G == 0 and C % feat == 0
    s = tk.mbstd_s64(i["x"], feat)
    members = i["x"].reshape(G, B // G, C, H, W)
    if c["exact"]:
        assert (members == members[:1]).all() and np.array_equal(i["x"] * 8, np.round(i["x"] * 8))
        assert (C // feat) * H * W <= 64 and bool((s == tk.MB_EPS ** 0.5).all())
    elif G == 1:
        assert bool((s == tk.MB_EPS ** 0.5).all())
    else:
        assert float(s.min()) >= tk.MIN_S, float(s.min())
        for g in range(G):       # well spread: every member on its side of the pattern
            assert (np.sign(members[g]) == np.sign(tk.PATTERN[g])).mean() > 0.99
    print(c["name"], "seed", inf["seed"], "smallest float64 s", inf["s_min"])


def test_head_cases_carry_the_planted_scores():
    for c in tk.by_entry("d_logistic") + tk.by_entry("g_nonsaturating"):
        i = tk.inputs(c["name"])
        for k, v in i.items():
            want = {40.0} if v.size == 1 else ({40.0, -40.0, 0.0} if v.size < 6 else {40.0, -40.0, 100.0, -100.0, 0.0})
            assert want <= set(v.tolist()), (c["name"], k)
            if v.size >= 6:
                z = v[v == 0]
                assert np.signbit(z).any() and not np.signbit(z).all()         # 0.0 and -0.0
            if v.size > tk.LH_THREADS:                                          # planted values in the last trip too
                assert np.abs(v[tk.LH_THREADS * ((v.size - 1) // tk.LH_THREADS):]).max() == 100.0
    e = tk.expected("d_logistic_257x600")
    assert float(e["ref64"]["sign"]) == float(np.sign(tk.inputs("d_logistic_257x600")["real"].astype(np.float64)).sum())


def test_dyadic_r1_case_has_exact_partial_sums():
    g = tk.inputs("r1_dyadic_4x4100")["grad"].astype(np.float64)
    assert set(np.unique(np.abs(g))) == {0.5, 1.0, 2.0} and (g > 0).any() and (g < 0).any()
    sq = g * g * 4
    assert np.array_equal(sq, np.round(sq)) and sq.sum() < 2 ** 24 and g.shape[0] == 4     # quarter units, a power-of-two batch


# ----------------------------------------------------------------------------- the float64 statements
def test_statements_through_ops_equal_the_shared_statements_in_float64():
    """What the float32 restatement restates: in float64 the lines of tk are dtrain_cases' and gtrain_cases'."""
    o = Ops(F64)
    for c in tk.by_entry("mbstd"):
        i, feat = tk.inputs(c["name"]), c["shape"][4]
        a = tk.mbstd_run(lambda t: tk.mbstd(o, t, feat), F64, i)
        b = tk.mbstd_run(lambda t: dc.mbstd(t, feat), F64, i)
        for k in a:
            np.testing.assert_allclose(a[k].detach().numpy(), b[k].detach().numpy(), rtol=1e-11, atol=1e-13, err_msg=c["name"] + k)
    for key in DATA_KEYS:
        c = FIRST[key]
        if c["entry"] in ("d_logistic", "g_nonsaturating", "r1", "path") and c.get("zero", "none") == "none":
            a, b = tk._ref(c, F64, True), tk._ref(c, F64, False)
            for k in a:
                np.testing.assert_allclose(a[k].detach().numpy(), b[k].detach().numpy(), rtol=1e-11, atol=1e-300, err_msg=key + k)


@pytest.mark.parametrize("c", _smallest("mbstd"), ids=lambda c: c["name"])
def test_stddev_statement_against_finite_differences(c):
    i, feat = tk.inputs(c["name"]), c["shape"][4]
    x, gout = _t64(i["x"]), _t64(i["gout"])
    assert torch.autograd.gradcheck(lambda t: dc.mbstd(t, feat), (x,), eps=1e-6, atol=1e-7, rtol=1e-5)

    def backward(t, g):     # bwd as a function of (x, gout): its gradients are the two outputs of bwd2
        return torch.autograd.grad(dc.mbstd(t, feat), t, g, create_graph=True)[0]
    assert torch.autograd.gradcheck(backward, (x, gout), eps=1e-6, atol=1e-6, rtol=1e-5)


@pytest.mark.parametrize("entry", ["d_logistic", "g_nonsaturating", "r1", "path"])
def test_head_statements_against_finite_differences(entry):
    for c in _smallest(entry):
        i = tk.inputs(c["name"])
        if entry == "d_logistic":
            ok = torch.autograd.gradcheck(dc.d_logistic, (_t64(i["real"]), _t64(i["fake"])), eps=1e-6, atol=1e-8, rtol=1e-6)
        elif entry == "g_nonsaturating":
            ok = torch.autograd.gradcheck(gc.g_nonsaturating, (_t64(i["fake"]),), eps=1e-6, atol=1e-8, rtol=1e-6)
        elif entry == "r1":
            ok = torch.autograd.gradcheck(lambda g: dc.r1_per_sample(g), (_t64(i["grad"]),), eps=1e-6, atol=1e-7, rtol=1e-6)
        else:
            m0 = _t64(i["mean_path"], False)[0]
            for fn in (lambda g: gc.path_penalty(g, m0, 0.01)[0], lambda g: tk.path_penalty(Ops(F64), g, m0, 0.01)[0]):
                ok = torch.autograd.gradcheck(fn, (_t64(i["grad"]),), eps=1e-6, atol=1e-7, rtol=1e-5)
                assert ok
        assert ok, c["name"]


def test_zero_row_path_statement_is_nan_free_and_equals_the_plain_one_elsewhere():
    c = tk.CASE["path_zero_row_3x5x205"]
    i = tk.inputs(c["name"])
    assert not i["grad"][1].any() and i["grad"][0].any() and i["grad"][2].any()
    m0 = _t64(i["mean_path"], False)[0]
    g = _t64(i["grad"])
    decay = tk.f32(c["decay"])                                           # the float the kernel receives
    plain = torch.autograd.grad(gc.path_penalty(g, m0, decay)[0], g)[0]
    assert bool(torch.isnan(plain[1]).all())                             # what the guard is for
    e = tk.expected(c["name"])
    for k, v in e["ref64"].items():
        assert np.isfinite(v).all() and np.isfinite(e["ref32"][k]).all(), k
    assert e["ref64"]["lengths"][1] == 0 and not e["ref64"]["dgrad"][1].any() and (e["ref64"]["lengths"][[0, 2]] > 0).all()
    pen, pm, _ = gc.path_penalty(g.detach(), m0, decay)                  # the plain values do not see the NaN gradient
    assert float(pen) == pytest.approx(float(e["ref64"]["pen"]), rel=1e-13) and float(pm) == pytest.approx(float(e["ref64"]["pm"]), rel=1e-13)
    np.testing.assert_allclose(plain[[0, 2]].numpy(), e["ref64"]["dgrad"][[0, 2]], rtol=1e-11, atol=0)
    z = tk.expected("path_all_zero_2x3x341")
    assert not z["ref64"]["dgrad"].any() and not z["ref64"]["lengths"].any() and float(z["ref64"]["pm"]) > 0
    assert all(np.isfinite(v).all() for v in z["ref64"].values())


# ----------------------------------------------------------------------------- e32, exactness
@pytest.mark.parametrize("key", DATA_KEYS)
def test_reference_is_finite_and_exact_where_it_says(key):
    c = FIRST[key]
    e, i = tk.expected(c["name"]), tk.inputs(c["name"])
    for k, v in e["ref64"].items():
        assert np.isfinite(v).all(), k
        if c["entry"] != "ema":
            assert np.isfinite(e["ref32"][k]).all() and np.isfinite(e["e32"][k]), k
        b = np.asarray(e["bound"][k])
        assert (b >= 0).all() and ((b == 0).all() or k not in e["exact"]), k
    for k in e["exact"]:     # the float64 value is an fp32 number, which the sequential fp32 sum reproduces
        r = e["ref64"][k]
        assert np.array_equal(r, r.astype(np.float32).astype(np.float64)), k
        if c["entry"] != "ema":
            assert np.array_equal(e["ref32"][k].astype(np.float64), r), k
    if c["entry"] == "mbstd":
        C = c["shape"][1]
        for r in (e["ref64"], e["ref32"]):
            assert np.array_equal(r["out.copy"], i["x"]) and np.array_equal(r["ggout.copy"], i["ggx"])
        if c["exact"]:
            for r in (e["ref64"], e["ref32"]):
                assert np.array_equal(r["gx"], i["gout"][:, :C]) and not r["ggout.map"].any() and np.isfinite(r["xg"]).all()
            # the sum of E <= 64 equal values: exact in one wave's butterfly, E roundings in the sequential restatement
            E = (C // c["shape"][4]) * c["shape"][2] * c["shape"][3]
            assert np.abs(e["ref64"]["out.map"] - tk.MB_EPS ** 0.5).max() <= 1e-18
            assert np.abs(e["ref32"]["out.map"] - tk.MB_EPS ** 0.5).max() <= (E + 2) * tk.EPS32 * tk.MB_EPS ** 0.5
    if c["name"] == "ema_keep":
        assert np.array_equal(e["ref64"]["dst"], i["dst"])
    if c["name"] == "ema_copy":
        for do, so, n in tk.info(c["name"])["rows"]:
            assert np.array_equal(e["ref64"]["dst"][do:do + n], i["src"][so:so + n])
    print(key, {k: f"{v:.3g}" for k, v in e["e32"].items()})
