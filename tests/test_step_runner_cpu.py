"""The eager loops of both trainers, call by call, against the record of the commit that still had four hand-written
loops (tests/golden/step_trace_parent.json, written by tests/golden/make_step_trace_golden.py): for every step call
the kind, the hand-off it received, the flips, the object mask, len(bank) and the CPU generator's state, and the
`history` list and iteration count of the fit.  Equality, no tolerance: the stub's losses are exact constants.  Plus
the contract of graphs.EagerSteps that the trainers rest on."""
import json
import os

import pytest
import torch

import step_trace_cases as stc

import gan2shape_amd  # noqa: F401

CASES = stc.cases()


@pytest.fixture(scope="module")
def parent():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "step_trace_parent.json")) as f:
        return json.load(f)["cases"]


def test_record_holds_exactly_these_cases(parent):
    assert sorted(parent) == sorted(CASES)


@pytest.mark.parametrize("name", sorted(CASES))
def test_eager_loop_makes_the_parent_s_calls(parent, name):
    got, want = stc.run_case(*CASES[name]), parent[name]
    assert got["total_it"] == want["total_it"]
    assert got["history"] == want["history"]
    assert len(got["trace"]) == len(want["trace"])
    for k, (g, w) in enumerate(zip(got["trace"], want["trace"])):
        assert g == w, (k, g, w)
    assert got["rng_after"] == want["rng_after"]


# ---------------------------------------------------------------------------------------------- the runner itself
def stub_trainer(joint=False, **over):
    from gan2shape_amd.trainer import GeneralizingTrainer2, Trainer
    t = (GeneralizingTrainer2 if joint else Trainer)(stc.TraceModel, stc.config(**over), debug=True, device="cpu")
    t.model.trainer = t
    return t


def test_eager_steps_run_hooks_and_hand_offs():
    from gan2shape_amd.graphs import EagerJointSteps, EagerSteps, GraphedJointSteps, GraphedSteps
    assert issubclass(GraphedSteps, EagerSteps) and issubclass(GraphedJointSteps, GraphedSteps)
    assert issubclass(EagerJointSteps, EagerSteps) and not issubclass(EagerJointSteps, GraphedSteps)
    t = stub_trainer()
    image, latent = stc.data(1)[0][0][None], stc.data(1)[0][1][None]
    steps = EagerSteps(t, image, latent)
    assert steps.collected == {1: None, 2: None, 3: None} and steps.image is image and steps.latent is latent
    assert (steps.before, steps.after, steps.source) == ({}, {}, {})
    log = []
    steps.before[2] = lambda replay: log.append(("before", replay))
    steps.after[2] = lambda collected: log.append(("after", collected))
    assert steps.run_block(1, 2) == 2 and steps.run_block(3, 0) == 0
    loss = steps.run(2)
    m = t.model
    assert loss is steps.loss[2] and float(loss) == 3.0 and not loss.requires_grad
    assert steps.collected[1] is m.outputs[1] and steps.collected[2] is m.outputs[2]
    assert log == [("before", False), ("after", m.outputs[2])]
    assert [c["handoff"] for c in m.trace] == [None, None, ["output", 1]]
    # set_sample rebinds, set_source stores the hand-off of the kind in front; `source` goes before both
    other = image + 1
    steps.set_sample(other, latent)
    assert steps.image is other and steps.object_mask is None
    handoff = (torch.zeros(1),)
    steps.set_source(3, handoff)
    assert steps.collected[2] is handoff
    steps.run(3)
    assert m.trace[-1]["handoff"] == ["new", [[0.0, 1]]] and m.trace[-1]["images"] == other[:, 0, 0, 0].tolist()
    steps.source[3] = m.outputs[0]
    steps.run(3)
    assert m.trace[-1]["handoff"] == ["output", 0]


def test_eager_joint_steps_differ_in_the_optimiser_step_only():
    from gan2shape_amd.graphs import EagerJointSteps
    t = stub_trainer(joint=True)
    synced = []
    t._sync_and_step = lambda optim: synced.append(optim)
    image, latent = stc.data(1)[0][0][None], stc.data(1)[0][1][None]
    steps = EagerJointSteps(t, image, latent)
    steps.run_block(1, 1), steps.run_block(2, 2)
    assert synced == [t.optim_step1, t.optim_step2, t.optim_step2]
    assert [c["kind"] for c in t.model.trace] == [1, 2, 2]


def test_bank_hooks_on_an_eager_runner():
    from gan2shape_amd.graphs import EagerSteps
    t = stub_trainer(collect_iters=2, step3_batch=3)
    image, latent = stc.data(1)[0][0][None], stc.data(1)[0][1][None]
    steps = EagerSteps(t, image, latent)
    t._bank_hooks(steps)
    assert set(steps.after) == {2} and set(steps.before) == {3}
    steps.run_block(1, 1)
    t._bank_begin(3)
    steps.run_block(2, 3)
    assert len(t.bank) == 4
    steps.run_block(3, 2)
    a, b = (c["handoff"] for c in t.model.trace[-2:])
    assert a[0] == b[0] == "bank" and len(a[1]) == 3 and set(a[1]) | set(b[1]) <= {30.0, 31.0, 40.0, 41.0}
