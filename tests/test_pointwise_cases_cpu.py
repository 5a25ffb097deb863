"""The case table of tests/pointwise_cases.py, without a GPU: every case reaches the kernel and the number of
grid-stride turns it is listed for, every (entry point, kernel, reason) the launchers distinguish occurs, and every
float32 expectation lies within two ulp of its float64 restatement."""
import numpy as np
import pytest

import pointwise_cases as pc

REQUIRED = {
    ("fba", "vec", "aligned"), ("fba", "scalar", "n%4"), ("fba", "scalar", "step_b%4"), ("fba", "scalar", "x misaligned"),
    ("fba", "scalar", "y misaligned"), ("fba", "scalar", "ref misaligned"), ("fba", "scalar", "f16"),
    ("clamp", "vec", "aligned"), ("clamp", "vec+tail", "n%4=1"), ("clamp", "vec+tail", "n%4=2"),
    ("clamp", "vec+tail", "n%4=3"), ("clamp", "scalar", "x misaligned"), ("clamp", "scalar", "y misaligned"),
    ("clamp", "scalar", "g misaligned"),
    ("abs", "vec", "aligned"), ("abs", "scalar", "hw%4"), ("abs", "scalar", "n%4"), ("abs", "scalar", "a misaligned"),
    ("abs", "scalar", "y misaligned"), ("abs", "scalar", "b misaligned"),
} | {(e, k, r) for e in ("nba", "nba_ps") for k, r in (("vec", "aligned"), ("scalar", "hw%4"), ("scalar", "x misaligned"),
                                                        ("scalar", "y misaligned"), ("scalar", "noise misaligned"))}


def test_every_case_takes_the_kernel_and_the_turns_it_is_listed_for():
    for c in pc.CASES:
        assert pc.dispatch(c) == (c["kernel"], c["turns"]), c["name"]


def test_a_reason_is_the_only_reason():
    """Taking the reason away (aligning the pointer, the aligned shape) puts the case on the vector kernel."""
    for c in pc.CASES:
        if c["reason"].endswith("misaligned"):
            assert pc.dispatch(dict(c, mis=()))[0] == "vec", c["name"]
        if c["reason"] == "f16" and c["turns"] == 1:      # fba_turn_f16 is fba_turn_scalar's shape: an odd step_b as well
            assert pc.dispatch(dict(c, f16=False))[0] == "vec", c["name"]


def test_every_entry_kernel_and_reason_occurs():
    have = {(c["entry"], c["kernel"], c["reason"]) for c in pc.CASES}
    assert have == REQUIRED, (REQUIRED - have, have - REQUIRED)


def test_modes_nulls_and_second_turns_are_covered():
    fba = [c for c in pc.CASES if c["entry"] == "fba"]
    for kernel in ("vec", "scalar"):
        assert {(c["act"], c["grad"], c["bias"]) for c in fba if c["kernel"] == kernel and not c.get("f16")} >= \
            {(a, g, b) for a, g in pc.MODES for b in (True, False)}
    assert {(c["entry"], c["kernel"], bool(c.get("f16"))) for c in pc.CASES if c["turns"] == 2} == {
        ("fba", "vec", False), ("fba", "scalar", False), ("fba", "scalar", True), ("nba", "vec", False),
        ("nba", "scalar", False), ("nba_ps", "vec", False), ("nba_ps", "scalar", False), ("clamp", "vec+tail", False),
        ("abs", "vec", False), ("abs", "scalar", False)}
    assert pc.CASE["fba_turn_vec"]["shape"] == (2, 3, 349528) and pc.CASE["fba_turn_scalar"]["shape"] == (2, 3, 174763)
    assert {(c["noise"], c["bias"]) for c in pc.CASES if c["entry"] == "nba"} == {(a, b) for a in (True, False) for b in (True, False)}
    assert {c["bias"] for c in pc.CASES if c["entry"] == "nba_ps"} == {True, False}
    assert {(c["b"], c["bias"]) for c in pc.CASES if c["entry"] == "abs"} >= {(False, True), (True, False), (True, True)}
    assert {c["backward"] for c in pc.CASES if c["entry"] == "clamp" and c["turns"] == 2} == {0, 1}
    ps = pc.inputs("nba_ps_vec")["noise"]
    assert ps.shape == (2, 1028) and np.abs(ps[0] - ps[1]).max() > 0.1


@pytest.mark.parametrize("name", pc.NAMES)
def test_expectation_within_two_ulp_of_float64(name):
    exp = pc.expected(name)
    c = pc.CASE[name]
    assert len(exp) == (2 if c["entry"] in ("nba", "nba_ps") and c["noise"] else 1)
    r = pc.restatement64(name)
    if r is None:       # clamp: a selection, no rounding; the expectation holds only input values, lo, hi and 0
        d = pc.inputs(name)
        src = d["g"] if c["backward"] else d["x"]
        e = exp[0]
        assert e.dtype == np.float32 and ((e == src) | (e == 0) | (e == pc.LO) | (e == pc.HI) | np.isnan(e)).all()
        assert np.isnan(e).sum() == (0 if c["backward"] else 1)
        return
    val, tol = r
    worst = max(float((np.abs(e.astype(np.float64) - val) / np.maximum(tol, 1e-300)).max()) for e in exp)
    print(f"{name} {c['entry']} {pc.dispatch(c)} {c['reason']}: expectation within {2 * worst:.2f} ulp of float64")
    assert worst <= 1.0
