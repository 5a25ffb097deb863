"""Outputs of the library's memory-bound passes on the cases of tests/hbm_twins_cases.py ->
tests/golden/hbm_twins_parent.npz (run on the MI355X with a built library; only DATA is written: outputs, no inputs).

    python tests/golden/make_hbm_twins_golden.py [--commit HASH] [--out PATH]

The calls go through the exported entries (lib.py) only, so the same script runs on any commit that has them.  The
committed file was written ONCE, from a build of the commit named in its `commit` entry: the parent of the change that
gave the row pass, the weighted-L1 backward and the demodulation one kernel body each.  tests/test_gpu_hbm_twins.py
holds the library to these bits.  HASH defaults to `git rev-parse HEAD`."""
import os
import subprocess
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, ROOT)

import hbm_twins_cases as hc                  # noqa: E402


def main():
    import gan2shape_amd  # noqa: F401
    from gan2shape_amd import lib
    if "--commit" in sys.argv:
        commit = sys.argv[sys.argv.index("--commit") + 1]
    else:
        commit = subprocess.check_output(["git", "rev-parse", "HEAD"], cwd=ROOT, text=True).strip()
    out = {k: v.cpu().numpy() for k, v in hc.run(lib.load(), lib).items()}
    for k, v in out.items():
        assert np.isfinite(v.astype(np.float32)).all(), k
    print(len(out), "outputs,", sum(v.nbytes for v in out.values()), "bytes, device", torch.cuda.get_device_name(0))
    out["commit"] = np.array(commit)
    path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(HERE, "hbm_twins_parent.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path))


if __name__ == "__main__":
    main()
