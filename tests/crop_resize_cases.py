"""Cases of the centre crop of step 2 (op/resample.py crop_resize, g2s_resample_sep), shared by
tests/golden/make_crop_resize_golden.py (which feeds them to the REFERENCE's utils.resize / utils.crop) and the tests
(which feed them to this package's): the images and the cotangents are pure functions of the case, so both sides see
identical operands.

A case is (gan, origin, crop, image): a [planes, gan, gan] image is resized to origin x origin, centre-cropped to
crop x crop and resized to image x image.  With the launcher's row tile of at most 12 output rows, image = 32, 16 and
128 are all heights the tile does not divide (the last tile is short), and so are the gradient launches onto
gan = 64, 32, 40 and 128.  The grid is flat (tiles x planes workgroups, no loop over planes), so there is no plane
count it could fail to divide; the cases of three planes have an odd one all the same.

Plane counts: the fixture holds, per element, a float64 and a float32 result for the image and for the gradient, and
uniform random values do not compress; the two 64-pixel cases and the 128-pixel case therefore run one plane, the
others three, which keeps the file under the repository's limit for a committed file.  Planes are independent and go
through identical code, so the per-plane checks lose nothing."""
import numpy as np
import torch

# name: (gan, origin, crop, image, planes)
CASES = {
    "down_crop_down_64_48_40_32": (64, 48, 40, 32, 1),
    "crop_up_32_32_24_32": (32, 32, 24, 32, 3),
    "crop_down_64_64_56_16": (64, 64, 56, 16, 1),
    "up_crop_down_32_48_40_32": (32, 48, 40, 32, 3),
    "odd_crop_odd_margin_64_40_33_32": (64, 40, 33, 32, 1),        # margin (40 - 33) // 2 = 3 on one side, 4 on the other
    "no_rows_dropped_24_24_24_32": (24, 24, 24, 32, 3),
    "face_128_128_112_128": (128, 128, 112, 128, 1),
    "small_40_30_21_16": (40, 30, 21, 16, 3),
}


def _seed(name):
    return sum(ord(c) * (i + 1) for i, c in enumerate(name)) % (2 ** 31)


def _uniform(seed, shape):
    # numpy's legacy RandomState: its stream is frozen, so the fixture's operands can be made again anywhere (the
    # fixture stores their sums, which the tests compare, and not the operands themselves: see the plane counts above)
    v = np.random.RandomState(seed).uniform(-1.0, 1.0, size=shape).astype(np.float32)
    return torch.from_numpy(v).double()


def image_of(name):
    """[1, planes, gan, gan] float64, uniform in [-1, 1], every value a float32."""
    gan, _, _, _, planes = CASES[name]
    return _uniform(_seed(name), (1, planes, gan, gan))


def cotangent_of(name):
    """[1, planes, image, image] float64, uniform in [-1, 1], every value a float32."""
    _, _, _, image, planes = CASES[name]
    return _uniform(_seed(name) + 1, (1, planes, image, image))


def operands(fixture, name):
    """(image, cotangent) of a case, checked against the sums the fixture recorded when it was made."""
    x, g = image_of(name), cotangent_of(name)
    want, got = fixture[f"{name}.operand_sums"], operand_sums(name)
    assert np.array_equal(got, want), f"{name}: the operands are not the ones the fixture was made from: {got} != {want}"
    return x, g


def operand_sums(name):
    """The float32 bit patterns of the image and of the cotangent, each summed as integers (exact on every machine)."""
    return np.array([t.float().numpy().view(np.uint32).sum(dtype=np.uint64) for t in (image_of(name), cotangent_of(name))])


def max_err(a, b):
    return float(np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)).max())
