"""-m gpu: the memory-bound passes whose entries come in families — the StyledConv tail with a shared or a per-sample
noise map (in place, in the blur's store, in the backward row pass), the three weighted-L1 backward entries, the
single- and multi-layer demodulation — bit for bit against what the library gave before the row pass, the L1 backward
and the demodulation got one kernel body each (tests/golden/hbm_twins_parent.npz, written by
tests/golden/make_hbm_twins_golden.py on the commit the file names).  These kernels are elementwise or one wave per
row in a fixed order, without atomics: there is no tolerance."""
import pytest
import torch

import hbm_twins_cases as hc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fx(golden):
    return golden("hbm_twins_parent")


@pytest.fixture(scope="module")
def got():
    import gan2shape_amd  # noqa: F401
    from gan2shape_amd import lib
    return hc.run(lib.load(), lib)


def test_every_recorded_output_is_produced_and_nothing_else(fx, got):
    assert set(got) == set(fx) - {"commit"}
    assert len(str(fx["commit"])) == 40


@pytest.mark.parametrize("group", list(hc.GROUPS))
def test_outputs_equal_the_parent_commits_bits(fx, got, group):
    names = sorted(k for k in got if k.startswith(group + "."))
    assert names
    differing = []
    for k in names:
        want = torch.from_numpy(fx[k]).cuda()
        assert got[k].shape == want.shape and got[k].dtype == want.dtype, k
        if not torch.equal(got[k], want):
            d = (got[k].float() - want.float()).abs()
            differing.append(f"{k}: {int((got[k] != want).sum())} of {want.numel()} elements, "
                             f"max |diff| {float(d.max()):.3e}")
    print(f"[{group}] {len(names)} outputs against commit {str(fx['commit'])[:7]}: {len(differing)} differ")
    assert not differing, "\n".join(differing)
