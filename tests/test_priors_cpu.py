"""-m "not gpu": what the device path of the depth priors (PriorGenerator(on_device=True), csrc/priors.hip)
leaves unchanged or promises on the host — the default is the host path, bit for bit; the device path
refuses CPU tensors; the new C entry points are declared, exported and validate before any launch; the
float64 restatement the GPU tests lean on agrees with the reference fixtures."""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch

import gan2shape_amd  # noqa: F401
from gan2shape_amd import lib, priors

import priors_cases as pc
from model_cases import PRIOR_NAMES, FakeMaskingModel

NEW_SYMBOLS = ["g2s_prior_map", "g2s_prior_smooth_workspace_bytes", "g2s_prior_smooth",
               "g2s_prior_ellipsoid_workspace_bytes", "g2s_prior_ellipsoid"]


def _golden_keys(g):
    return sorted(k for k in g if k.startswith("p."))


def test_host_path_is_the_default_and_unchanged(golden):
    """on_device defaults to False; the class then returns the same tensor whether the argument is left out or
    spelled, and what it returned before the device path existed: the reference fixtures, all eight, bit for
    bit (rtol 0).  One precondition: the fixtures' mask source (model_cases.parsing_mask) goes through torch's
    vectorised CPU sqrt, which is not correctly rounded and depends on the instruction set, so a CPU may hand
    the priors a mask a few 1e-7 from the one behind the fixtures.  Whether it does is read off `confidence`
    (far - far * mask^2: two roundings on top of the mask); on such a CPU the fixtures are held to the bound
    of test_priors_golden instead, `box` (no mask) still to rtol 0."""
    assert inspect.signature(priors.PriorGenerator.__init__).parameters["on_device"].default is False
    g = golden("model")
    keys = _golden_keys(g)
    assert len(keys) == 8
    got = {}
    for key in keys:
        _, name, size = key.split(".")
        size = int(size)
        fm = FakeMaskingModel(size)
        source = fm.confidence_mask if "confidence" in name else fm
        img = torch.zeros(1, 3, size, size)
        gen = priors.PriorGenerator(size, "face", name, masking_model=source)
        assert gen.on_device is False
        p = gen(img, device="cpu")
        q = priors.PriorGenerator(size, "face", name, masking_model=source, on_device=False)(img, device="cpu")
        assert p.device.type == "cpu" and torch.equal(p, q)
        got[key] = p.numpy()
    same_mask = np.array_equal(got["p.confidence.64"], g["p.confidence.64"])
    print("this CPU's sqrt reproduces the fixtures' mask bit for bit:", same_mask)
    np.testing.assert_array_equal(got["p.box.64"], g["p.box.64"])
    for key in keys:
        if same_mask:
            np.testing.assert_array_equal(got[key], g[key], err_msg=key)
        else:
            np.testing.assert_allclose(got[key], g[key], rtol=pc.RTOL, atol=pc.ATOL, err_msg=key)
    with pytest.raises(RuntimeError):
        priors.PriorGenerator(64, "face", "box").batch(torch.zeros(1, 3, 64, 64), device="cpu")
    with pytest.raises(TypeError):     # the device path takes no extra arguments and does not drop them silently
        priors.PriorGenerator(64, "face", "box", on_device=True)(torch.zeros(1, 3, 64, 64), "cpu", 1)


@pytest.mark.parametrize("name", PRIOR_NAMES)
def test_device_path_refuses_cpu_tensors(name):
    gen = priors.PriorGenerator(32, "face", name, on_device=True)
    img = torch.zeros(1, 3, 32, 32)
    with pytest.raises(RuntimeError, match="CUDA"):
        gen(img, device="cpu")
    with pytest.raises(RuntimeError, match="CUDA"):
        gen(img, device="cuda")            # a CPU image is refused whatever the target device
    with pytest.raises(RuntimeError, match="CUDA"):
        gen.batch([img, img], device="cuda")


def test_trainer_config_key_reaches_the_generator():
    from gan2shape_amd.trainer import Trainer
    from model_cases import TOY_CFG, ToyStepModel
    assert Trainer(ToyStepModel, dict(TOY_CFG), device="cpu").prior_generator.on_device is False
    t = Trainer(ToyStepModel, dict(TOY_CFG, prior_on_device=True), device="cpu")
    assert t.prior_generator.on_device is True


def test_new_symbols_are_declared_and_exported():
    L = lib.load()
    for name in NEW_SYMBOLS:
        assert name in lib.SIGNATURES
        assert getattr(L, name) is not None
    assert L.g2s_abi_version() == 1
    # rows + filtered map + 2 slots per pass and image; nothing for an empty batch
    need = L.g2s_prior_smooth_workspace_bytes(8, 128, 11, 3)
    assert 8 * (128 * 118 + 118 * 118) * 4 + 8 * 2 * 3 * 4 <= need <= 8 * 2 * 128 * 128 * 4 + 4096
    assert L.g2s_prior_smooth_workspace_bytes(0, 128, 11, 3) == 0
    assert L.g2s_prior_ellipsoid_workspace_bytes(5) == 5 * 16
    assert L.g2s_prior_ellipsoid_workspace_bytes(0) == 0


def test_validation_precedes_any_launch():
    """Each rejected combination returns an error and a message; B = 0 returns success.  A host buffer
    stands in for device memory: a launch would fault, a rejected call never gets that far."""
    L = lib.load()
    d = (C.c_float * 4)()
    big = 1 << 30

    def err():
        return L.g2s_last_error().decode()
    assert L.g2s_prior_smooth(d, 1, 16, 10, 3, 0.91, 1.02, d, d, big, None) == -1 and "taps" in err()    # even
    assert L.g2s_prior_smooth(d, 1, 16, 17, 3, 0.91, 1.02, d, d, big, None) == -1 and "taps" in err()    # > S
    assert L.g2s_prior_smooth(d, 1, 16, 11, -1, 0.91, 1.02, d, d, big, None) == -1 and "passes" in err()
    assert L.g2s_prior_smooth(d, 1, 16, 11, 3, 1.02, 1.02, d, d, big, None) == -1 and "near" in err()
    assert L.g2s_prior_smooth(None, 1, 16, 11, 3, 0.91, 1.02, d, d, big, None) == -1 and "NULL" in err()
    assert L.g2s_prior_smooth(d, 1, 16, 11, 3, 0.91, 1.02, None, d, big, None) == -1 and "NULL" in err()
    assert L.g2s_prior_smooth(d, 1, 16, 11, 3, 0.91, 1.02, d, None, 0, None) == -3 and "workspace" in err()
    assert L.g2s_prior_smooth(d, 1, 16, 11, 3, 0.91, 1.02, d, d, 16, None) == -3 and "workspace" in err()
    assert L.g2s_prior_smooth(d, -1, 16, 11, 3, 0.91, 1.02, d, d, big, None) == -1
    assert L.g2s_prior_map(None, 1, 16, 1, 0.7, 1.02, d, None) == -1 and "NULL" in err()
    assert L.g2s_prior_map(d, 1, 16, 2, 0.7, 1.02, None, None) == -1 and "NULL" in err()
    assert L.g2s_prior_map(d, 1, 16, 3, 0.7, 1.02, d, None) == -1 and "kind" in err()
    assert L.g2s_prior_map(d, 1, 0, 1, 0.7, 1.02, d, None) == -1
    assert L.g2s_prior_ellipsoid(None, 1, 16, 0.7, 0.4, 0.91, 1.02, d, d, big, None) == -1 and "NULL" in err()
    assert L.g2s_prior_ellipsoid(d, 1, 16, 0.7, 0.4, 1.02, 0.91, d, d, big, None) == -1 and "near" in err()
    assert L.g2s_prior_ellipsoid(d, 1, 16, 0.7, 0.0, 0.91, 1.02, d, d, big, None) == -1 and "radius" in err()
    assert L.g2s_prior_ellipsoid(d, 1, 16, 0.7, 0.4, 0.91, 1.02, d, None, 0, None) == -3 and "workspace" in err()
    # an empty batch is a no-op, NULL pointers and all
    assert L.g2s_prior_map(None, 0, 16, 1, 0.7, 1.02, None, None) == 0
    assert L.g2s_prior_smooth(None, 0, 16, 11, 3, 0.91, 1.02, None, None, 0, None) == 0
    assert L.g2s_prior_ellipsoid(None, 0, 16, 0.7, 0.4, 0.91, 1.02, None, None, 0, None) == 0


def test_float64_restatement_agrees_with_the_reference_fixtures(golden):
    """The reference's own fp32 run sits 1.7e-6 - 2.2e-6 (smoothing) and 1e-7 (ellipsoid) from the float64
    restatement: inside the bound the fixtures are held to."""
    g = golden("model")
    seen = 0
    for key in _golden_keys(g):
        _, name, size = key.split(".")
        fm = FakeMaskingModel(int(size))
        if name == "ellipsoid":
            want = pc.ellipsoid64(fm.mask[0, 0].numpy())
        elif name.startswith("smoothed_"):
            source = fm.confidence_mask if "confidence" in name else fm
            base = priors.PriorGenerator(int(size), "face", pc.SMOOTHED_FROM[name], masking_model=source)(
                None, device="cpu")[0].numpy()
            want = pc.smooth64(base)
        else:
            continue
        seen += 1
        err = np.abs(g[key][0] - want)
        print(f"{key}: reference fp32 vs float64 restatement, max abs {err.max():.3e}")
        np.testing.assert_allclose(g[key][0], want, rtol=pc.RTOL, atol=pc.ATOL, err_msg=key)
    assert seen == 5
