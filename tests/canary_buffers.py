"""Device views into canary-filled buffers for the GPU tests that call the C ABI directly (test_gpu_warp_paths.py,
test_gpu_rowops_paths.py, test_gpu_pool_paths.py): a tensor is a view MARGIN floats into a larger 16-byte aligned
buffer (plus `shift` floats when it is to be misaligned); afterwards an input must be unchanged bit for bit and the
canaries around an output intact."""
import numpy as np
import torch

CANARY = 1024.0
MARGIN = 16


class Buffers:
    def __init__(self):
        self.held = []

    def view(self, key, arr=None, like=None, shift=0, fill=None, out=False):
        """A float32 device view holding `arr`, or room for an output shaped like `like` (pre-filled with `fill`, the
        canary by default).  out=True with `arr`: pre-filled with data but written by the call (an in-place operand).
        None stays None."""
        if arr is None and like is None:
            return None
        src = like if arr is None else arr
        n = int(np.prod(src.shape))
        buf = torch.full((n + 2 * MARGIN + 4,), CANARY, dtype=torch.float32, device="cuda")
        assert buf.data_ptr() % 16 == 0
        off = MARGIN + shift
        v = buf[off:off + n]
        assert v.data_ptr() % 16 == (4 * shift) % 16
        if arr is not None:
            v.copy_(torch.from_numpy(np.array(arr, np.float32).reshape(-1)))     # a copy: the case data is read-only
        elif fill is not None:
            v.fill_(fill)
        self.held.append((key, buf, off, n, None if (arr is None or out) else buf.clone()))
        return v

    def spare(self, key, like):
        """A canary buffer that is handed to nobody: where a kernel that ignored a NULL would have found its output."""
        buf = torch.full((int(np.prod(like.shape)) + 2 * MARGIN,), CANARY, dtype=torch.float32, device="cuda")
        self.held.append((key, buf, 0, 0, None))
        return buf

    def check(self):
        for key, buf, off, n, before in self.held:
            if before is None:      # an output: the canaries around it
                assert (buf[:off] == CANARY).all() and (buf[off + n:] == CANARY).all(), f"{key}: canary overwritten"
            else:                   # an input: all of it (NaN compares as bits)
                assert torch.equal(buf.view(torch.uint8), before.view(torch.uint8)), f"{key}: input changed"


def within(got, want, bound, what):
    """max error / bound; asserts |got - want| <= bound element by element (a NaN fails)."""
    got = np.asarray(got, np.float64)
    err = np.abs(got - want)
    ok = err <= bound
    assert ok.all(), (what, int((~ok).sum()), np.argwhere(~ok)[:4].tolist(), got[~ok][:4], np.asarray(want)[~ok][:4])
    nz = bound > 0
    return float((err[nz] / bound[nz]).max()) if nz.any() else 0.0
