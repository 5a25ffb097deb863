"""Iteration counts, `history` lists and parameter sums of the short fits of tests/step_runner_cases.py ->
tests/golden/step_runner_parent.json (run on the MI355X with a built library; only DATA is written).

    python tests/golden/make_step_runner_golden.py [--commit HASH] [--out PATH] [--check PATH]

The committed file was written ONCE, from a build of the commit named in its `commit` entry: the parent of the change
that gave the four training loops one step-block runner (graphs.EagerSteps).  tests/test_gpu_step_runner.py holds the
loops to these bits.  --check PATH compares a fresh run with an earlier record instead of writing one, and names the
configurations that do not reproduce (exit status 1).  HASH defaults to `git rev-parse HEAD`."""
import json
import os
import subprocess
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, ROOT)

import step_runner_cases as src                  # noqa: E402


def main():
    import gan2shape_amd  # noqa: F401
    from gan2shape_amd import lib
    lib.load()
    if "--commit" in sys.argv:
        commit = sys.argv[sys.argv.index("--commit") + 1]
    else:
        commit = subprocess.check_output(["git", "rev-parse", "HEAD"], cwd=ROOT, text=True).strip()
    lib.set_deterministic(True)
    torch.cuda.set_stream(torch.cuda.Stream())      # captures need a non-default stream
    cases = {name: src.run_case(*case) for name, case in zip(src.IDS, src.CASES)}
    if "--check" in sys.argv:
        with open(sys.argv[sys.argv.index("--check") + 1]) as f:
            earlier = json.load(f)["cases"]
        differing = [name for name in cases if json.loads(json.dumps(cases[name])) != earlier.get(name)]
        print("reproduced" if not differing else f"NOT reproduced: {differing}")
        sys.exit(1 if differing else 0)
    path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(HERE, "step_runner_parent.json")
    with open(path, "w") as f:      # one line per case
        f.write('{"commit": %s, "device": %s, "cases": {\n' % (json.dumps(commit), json.dumps(torch.cuda.get_device_name(0))))
        f.write(",\n".join(f"{json.dumps(name)}: {json.dumps(case, sort_keys=True)}" for name, case in cases.items()))
        f.write("\n}}\n")
    print(path, os.path.getsize(path), "bytes,", len(cases), "cases")


if __name__ == "__main__":
    main()
