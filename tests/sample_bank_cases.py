"""Cases of the sample-bank gather shared by tests/test_sample_bank_cpu.py and tests/test_gpu_sample_bank.py.

A case is (name, S, rows, b, h, idx kind, shift): a bank of `rows` rows of [3,S,S] images and [1,S,S] masks, `b`
indices of the given kind, `h` head rows (the input image) in front of the gathered images; `shift` = 1 makes the
bank and both outputs views that start one float into their storage (no 16-byte alignment).  The sizes cover: rows
that are no multiple of 16 bytes (S = 5: 75 and 25 floats), a single row, repeats, the last rows of the bank, more
than one chunk per row (S = 128: 12288 float4 > 1024 per workgroup pass), and the dword path on a size that would
otherwise vectorise (shift)."""
import torch

CASES = [
    ("s4", 4, 3, 2, 1, "distinct", 0),
    ("s5_head", 5, 7, 3, 1, "distinct", 0),
    ("s5_nohead", 5, 7, 3, 0, "distinct", 0),
    ("one_row", 8, 1, 1, 1, "zero", 0),
    ("repeats", 8, 4, 6, 1, "repeats", 0),
    ("last_rows", 16, 24, 8, 1, "last", 0),
    ("s128", 128, 16, 8, 1, "distinct", 0),
    ("offset_views", 8, 5, 3, 1, "distinct", 1),
]
IDS = [c[0] for c in CASES]


def make_index(kind, rows, b, seed=0):
    g = torch.Generator().manual_seed(100 + seed)
    if kind == "distinct":
        return torch.randperm(rows, generator=g)[:b]
    if kind == "zero":
        return torch.zeros(b, dtype=torch.int64)
    if kind == "repeats":       # b > rows: every row at least once, some twice
        return torch.cat([torch.randperm(rows, generator=g), torch.randint(0, rows, (b - rows,), generator=g)])
    if kind == "last":
        return torch.arange(rows - b, rows).flip(0)
    raise ValueError(kind)


def make_data(S, rows, seed=0):
    """(images [rows,3,S,S], masks [rows,1,S,S], head [1,3,S,S]): every element distinct, so a row that lands in the
    wrong place, or shifted by one element, cannot compare equal."""
    n_img, n_mask = rows * 3 * S * S, rows * S * S
    images = (torch.arange(n_img, dtype=torch.float32) + 0.25).reshape(rows, 3, S, S)
    masks = -(torch.arange(n_mask, dtype=torch.float32) + 0.5).reshape(rows, 1, S, S)
    head = (torch.arange(3 * S * S, dtype=torch.float32) * -3.0 - 7.0).reshape(1, 3, S, S)
    return images, masks, head


def reference(images, masks, head, idx, h):
    """The composed route: index_select twice plus the cat."""
    sel = images.index_select(0, idx.to(torch.int64))
    batch = torch.cat([head, sel], 0) if h else sel
    return batch, masks.index_select(0, idx.to(torch.int64))
