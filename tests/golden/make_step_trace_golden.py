"""Call traces and `history` lists of the eager Trainer.fit and GeneralizingTrainer2.fit on the schedules of
tests/step_trace_cases.py -> tests/golden/step_trace_parent.json (CPU only; only DATA is written).

    python tests/golden/make_step_trace_golden.py [--commit HASH] [--out PATH]

The committed file was written ONCE, at the commit named in its `commit` entry: the parent of the change that gave the
four training loops one step-block runner (graphs.EagerSteps).  tests/test_step_runner_cpu.py holds the trainers to it.
HASH defaults to `git rev-parse HEAD`."""
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, ROOT)

import step_trace_cases as stc                  # noqa: E402


def main():
    import gan2shape_amd  # noqa: F401
    if "--commit" in sys.argv:
        commit = sys.argv[sys.argv.index("--commit") + 1]
    else:
        commit = subprocess.check_output(["git", "rev-parse", "HEAD"], cwd=ROOT, text=True).strip()
    cases = {name: stc.run_case(*args) for name, args in stc.cases().items()}
    path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(HERE, "step_trace_parent.json")
    with open(path, "w") as f:      # one line per case
        f.write('{"commit": %s, "cases": {\n' % json.dumps(commit))
        f.write(",\n".join(f"{json.dumps(name)}: {json.dumps(case, sort_keys=True, separators=(',', ':'))}"
                           for name, case in sorted(cases.items())))
        f.write("\n}}\n")
    print(path, os.path.getsize(path), "bytes,", len(cases), "cases,", sum(len(c["trace"]) for c in cases.values()), "calls")


if __name__ == "__main__":
    main()
