"""-m gpu: the four training loops against the bits of the commit that still had four hand-written loops
(tests/golden/step_runner_parent.json, written on the MI355X by tests/golden/make_step_runner_golden.py).  Short seeded
fits in deterministic mode on a non-default stream (tests/step_runner_cases.py): Trainer.fit and
GeneralizingTrainer2.fit, eager and graphs=True, bank off and on, two stages with different flips, object masks live.
The iteration count, the `history` list (losses as float bits) and the float64 sum and sum of squares of every trained
net's parameters are compared for equality: no tolerance.  All eight configurations reproduced themselves in a second
process at the recording commit."""
import json
import os

import pytest
import torch

import step_runner_cases as src

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def deterministic():
    import gan2shape_amd  # noqa: F401
    from gan2shape_amd import lib
    lib.load()
    prev = lib.set_deterministic(True)
    yield
    lib.set_deterministic(prev)


@pytest.fixture(scope="module")
def parent():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "step_runner_parent.json")) as f:
        return json.load(f)["cases"]


def test_record_holds_exactly_these_cases(parent):
    assert sorted(parent) == sorted(src.IDS)


@pytest.mark.parametrize("case", src.CASES, ids=src.IDS)
def test_fit_ends_on_the_parent_s_bits(deterministic, parent, case):
    dev = torch.device("cuda")
    torch.cuda.set_stream(torch.cuda.Stream(dev))     # captures need a non-default stream
    try:
        got = json.loads(json.dumps(src.run_case(*case)))
    finally:
        torch.cuda.set_stream(torch.cuda.default_stream(dev))
    want = parent["-".join(case)]
    print(f"[step runner] {'-'.join(case)}: total_it {got['total_it']}, history", [h[3] for h in got["history"]])
    assert got["total_it"] == want["total_it"]
    assert got["mask_calls"] == want["mask_calls"]
    assert got["history"] == want["history"], [(g, w) for g, w in zip(got["history"], want["history"]) if g != w]
    assert got["nets"] == want["nets"], {k: (got["nets"][k], want["nets"][k]) for k in want["nets"] if got["nets"][k] != want["nets"][k]}
