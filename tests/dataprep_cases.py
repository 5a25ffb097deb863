"""Cases of the data path (prepare_data.py, dataset.DeviceBatches, csrc/dataprep.hip), shared by the CPU and the GPU
tests.  Every comparison made on them is exact equality: the resize is integer arithmetic, the batch a table lookup."""
import numpy as np

FILTERS = ("lanczos", "bilinear")

# (H, W) -> (oh, ow): down both ways; a 0/255 image; an upscale; odd sizes; only the horizontal pass; a strong
# reduction (many taps); neither pass; only-just a resize with widths that are no multiple of 16
RESIZE_SIZES = [
    ((37, 53), (16, 23)),
    ((64, 64), (16, 16)),
    ((20, 31), (40, 62)),
    ((129, 77), (32, 19)),
    ((48, 48), (48, 24)),
    ((300, 200), (24, 16)),
    ((16, 16), (16, 16)),
    ((9, 250), (8, 222)),
    ((24, 40), (12, 40)),       # only the vertical pass
]
CHECKER_SIZES = [((64, 64), (16, 16)), ((20, 31), (40, 62)), ((45, 64), (17, 24))]

# (H, W), size for resize_and_crop.  Even remainders of the longer edge (37x53: 22 - 16 = 6; 129x77: 26 - 16 = 10) and
# odd ones, whose half is rounded to even as Python's round does (37x54: 23 - 16 = 7 -> 3.5 -> 4; 40x65 at 24:
# 39 - 24 = 15 -> 7.5 -> 8; 16x27: 11 -> 5.5 -> 6; 27x16 the same downwards); portrait and landscape; one image already
# at size; one upscaled
CROP_CASES = [((37, 53), 16), ((53, 37), 16), ((37, 54), 16), ((129, 77), 16), ((40, 65), 24), ((16, 16), 16),
              ((16, 27), 16), ((27, 16), 16), ((10, 14), 20)]


def random_images(n, H, W, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (n, H, W, 3), dtype=np.uint8)


def checkerboard(n, H, W, cell=3):
    """0/255 squares of `cell` pixels (phase shifted per image and channel): Lanczos overshoots on both sides."""
    y, x = np.mgrid[0:H, 0:W]
    out = np.empty((n, H, W, 3), np.uint8)
    for i in range(n):
        for c in range(3):
            out[i, :, :, c] = 255 * ((((y + i) // cell) + ((x + c) // cell)) % 2)
    return out


def resize_cases():
    """(name, images uint8 [N, H, W, 3] factory, (oh, ow))."""
    cases = []
    for (H, W), out in RESIZE_SIZES:
        cases.append((f"random_{H}x{W}_to_{out[0]}x{out[1]}", lambda n, H=H, W=W: random_images(n, H, W, H * W), out))
    for (H, W), out in CHECKER_SIZES:
        cases.append((f"checker_{H}x{W}_to_{out[0]}x{out[1]}", lambda n, H=H, W=W: checkerboard(n, H, W), out))
    return cases


# g2s_u8_batch: (S, N, idx, flip).  S = 8, 20: the scalar kernel (20 is a multiple of 4 but not of 16); S = 64: the wide
# kernel; S = 16: the wide kernel with one chunk per row.  B = 1 and 5; mixed flips; repeated, first and last index.
BATCH_CASES = [
    (8, 5, [4, 0, 2, 2, 4], [1, 0, 1, 0, 0]),
    (8, 3, [2], [1]),
    (20, 4, [0, 3, 3, 1, 0], [0, 1, 0, 1, 1]),
    (64, 6, [5, 0, 3, 3, 5], [1, 0, 0, 1, 0]),
    (64, 2, [0], [0]),
    (64, 2, [1], [1]),
    (16, 3, [2, 2, 0, 1, 2], [1, 1, 0, 0, 1]),
]


def packed_dataset(N, S, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (N, 3, S, S), dtype=np.uint8)
