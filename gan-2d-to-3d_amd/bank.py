"""Projected-sample bank: the samples step 3 draws from (config `collect_iters`, trainer.py).

Step 2 of GAN2Shape projects `n_proj_samples` pseudo views of the image through the GAN in every iteration; the
reference hands only the LAST iteration's batch to step 3, and the two lines of its forward_step3 that should pick a
random subset assign nothing (model.py:231-233 there).  The bank keeps the projected images and masks of the last K
step-2 iterations on the device, and every step-3 iteration draws its batch from all K * n of them with the
reference's own `torch.randperm`, made effective.

    bank = SampleBank(K, n, S, device)
    bank.put(projected, mask)                       # after a step-2 iteration; a ring of K * n rows
    idx = bank.indices(b)                           # torch.randperm(len(bank))[:b], on the CPU
    collected = bank.gather(idx, image)             # (projected_samples [b,3,S,S], masks [b,1,S,S])

`gather` is ONE launch of g2s_bank_gather (csrc/bank.hip) on the device: the selected image rows, the selected mask
rows and — with `image` — the input image as row 0 of the same buffer, so that the `torch.cat([images,
projected_samples])` which opens step 3 is already done: the result is a `HandOff`, a 2-tuple like step 2's own
hand-off whose attribute `batch` is that [1 + b, 3, S, S] buffer (`projected_samples` is its rows 1 ..).  CPU
tensors take index_select.
"""
import ctypes as C

import torch

DEFAULT_MAX_BYTES = 2 << 30


class HandOff(tuple):
    """(projected_samples, masks) with `batch`: [images; projected_samples] in one buffer, or None."""
    batch = None

    def __new__(cls, projected_samples, masks, batch=None):
        self = super().__new__(cls, (projected_samples, masks))
        self.batch = batch
        return self


def bank_bytes(collect_iters, n_proj_samples, image_size):
    """Bytes of a bank: collect_iters * n_proj_samples rows of (3 + 1) * S * S floats."""
    return int(collect_iters) * int(n_proj_samples) * 4 * int(image_size) * int(image_size) * 4


def check_bank_size(collect_iters, n_proj_samples, image_size, max_bytes=DEFAULT_MAX_BYTES):
    need = bank_bytes(collect_iters, n_proj_samples, image_size)
    if need > max_bytes:
        raise ValueError(f"sample bank too large: collect_iters={collect_iters} x n_proj_samples={n_proj_samples} rows at "
                         f"image_size={image_size} need {need} bytes, more than bank_max_bytes={max_bytes}")
    return need


class SampleBank:
    def __init__(self, collect_iters, n_proj_samples, image_size, device="cuda"):
        self.K, self.n, self.S = int(collect_iters), int(n_proj_samples), int(image_size)
        if self.K < 1 or self.n < 1 or self.S < 1:
            raise ValueError("SampleBank needs collect_iters, n_proj_samples, image_size >= 1")
        self.device = torch.device(device)
        self.capacity = self.K * self.n
        self.images = torch.zeros(self.capacity, 3, self.S, self.S, dtype=torch.float32, device=self.device)
        self.masks = torch.zeros(self.capacity, 1, self.S, self.S, dtype=torch.float32, device=self.device)
        self._next = 0      # slot (of K) the next put writes
        self._count = 0     # valid rows
        # the error word of the device-side index check (g2s_bank_gather) and whether a launch may have set it
        self._err = torch.zeros(1, dtype=torch.int32, device=self.device) if self.device.type == "cuda" else None
        self._pending = False

    def __len__(self):
        return self._count

    # ------------------------------------------------------------------ the ring
    def reset(self):
        self._report()
        self._next = self._count = 0

    def put(self, projected, mask):
        """Write the next n rows (detached inputs [n,3,S,S] and [n,1,S,S]); the ring overwrites its oldest slot."""
        self._report()
        if tuple(projected.shape) != (self.n, 3, self.S, self.S) or tuple(mask.shape) != (self.n, 1, self.S, self.S):
            raise ValueError(f"SampleBank.put: expected [{self.n},3,{self.S},{self.S}] and [{self.n},1,{self.S},{self.S}], "
                             f"got {tuple(projected.shape)} and {tuple(mask.shape)}")
        if projected.requires_grad or mask.requires_grad:
            raise ValueError("SampleBank.put takes detached tensors")
        rows = slice(self._next * self.n, (self._next + 1) * self.n)
        self.images[rows].copy_(projected)
        self.masks[rows].copy_(mask)
        self._next = (self._next + 1) % self.K
        self._count = min(self._count + self.n, self.capacity)

    # ------------------------------------------------------------------ the draw
    def indices(self, b, generator=None):
        """torch.randperm(len(bank), generator=generator)[:b] on the CPU: one draw.  b > len(bank) gives all rows,
        permuted.  The valid rows are always rows 0 .. len(bank) - 1 (the ring fills from slot 0)."""
        self._report()
        if self._count == 0:
            raise RuntimeError("SampleBank.indices: the bank is empty")
        return torch.randperm(self._count, generator=generator)[:int(b)]

    # ------------------------------------------------------------------ the gather
    def _report(self):
        """Raise for a device index the kernel had to clamp in an earlier gather (reads the error word: a sync,
        made only after a gather with a device index)."""
        if not self._pending or (self.device.type == "cuda" and torch.cuda.is_current_stream_capturing()):
            return
        self._pending = False
        bad = int(self._err.item())
        if bad:
            self._err.zero_()
            raise IndexError(f"SampleBank.gather: entry {bad - 1} of an earlier device index was outside the {self._count} "
                             "valid rows (it was clamped into the bank)")

    def _head(self, image):
        if image is None or len(image) != 1:
            return None
        if tuple(image.shape) != (1, 3, self.S, self.S) or image.dtype != torch.float32 or image.device != self.images.device:
            raise ValueError(f"SampleBank.gather: image must be float32 [1,3,{self.S},{self.S}] on {self.images.device}")
        return image.detach().contiguous()

    def gather(self, idx, image=None):
        """(projected_samples, masks) of rows `idx` (CPU or device int64 / int32, any length, repeats allowed) as a
        HandOff; with `image` [1,3,S,S] its `batch` is [image; projected_samples].  A CPU index is range-checked
        here; a device index is clamped by the kernel and reported by the next call."""
        self._report()
        if idx.dtype not in (torch.int64, torch.int32) or idx.dim() != 1 or idx.numel() < 1:
            raise ValueError("SampleBank.gather: idx must be a non-empty 1-D int64 or int32 tensor")
        if self._count == 0:
            raise RuntimeError("SampleBank.gather: the bank is empty")
        head = self._head(image)
        if not idx.is_cuda:
            if int(idx.min()) < 0 or int(idx.max()) >= self._count:
                raise IndexError(f"SampleBank.gather: index out of range for {self._count} valid rows")
        if self.device.type != "cuda":
            sel = self.images.index_select(0, idx.to(torch.int64))
            masks = self.masks.index_select(0, idx.to(torch.int64))
            if head is None:
                return HandOff(sel, masks)
            batch = torch.cat([head, sel], 0)
            return HandOff(batch[1:], masks, batch)
        if idx.is_cuda:
            self._pending = True
        else:
            idx = idx.to(self.device)
        b, h = idx.numel(), 0 if head is None else 1
        batch = torch.empty(h + b, 3, self.S, self.S, dtype=torch.float32, device=self.device)
        masks = torch.empty(b, 1, self.S, self.S, dtype=torch.float32, device=self.device)
        self.gather_into(idx, head, batch, masks)
        return HandOff(batch[h:], masks, batch if h else None)

    def gather_into(self, idx, head, batch, masks):
        """The launch itself: device `idx` [b], `head` [1,3,S,S] or None -> batch [h + b,3,S,S], masks [b,1,S,S]
        (contiguous float32 views on the bank's device).  What the graphed trainers call with static buffers."""
        from . import lib
        b, h = idx.numel(), 0 if head is None else len(head)
        lib.require_cuda(idx, head, batch, masks)
        assert idx.is_contiguous() and batch.is_contiguous() and masks.is_contiguous()
        assert tuple(batch.shape) == (h + b, 3, self.S, self.S) and tuple(masks.shape) == (b, 1, self.S, self.S)
        assert batch.dtype == masks.dtype == torch.float32 and idx.dtype in (torch.int64, torch.int32)
        assert head is None or (head.is_contiguous() and head.dtype == torch.float32)
        lib.check(lib.load().g2s_bank_gather(
            lib.ptr(self.images), lib.ptr(self.masks), C.c_int64(self._count), lib.ptr(idx),
            int(idx.dtype == torch.int64), b, lib.ptr(head), h, lib.ptr(batch), lib.ptr(masks), self.S,
            lib.ptr(self._err), lib.stream()))


class StaticHandOff:
    """The fixed buffers a captured step 3 reads (graphs.py): index [b] int64, batch [1 + b,3,S,S], masks [b,1,S,S].
    `fill` draws on the host, uploads the index and runs the gather in front of the iteration, on the current stream.
    In front of a REPLAY it also makes the draw that forward_step3 keeps from the reference (model.py: the discarded
    randperm over the hand-off's rows), which a replayed step does not reach: a seeded graphed run then consumes the
    CPU generator like the eager run and draws the same indices."""

    def __init__(self, bank, b, image):
        self.bank, self.b, self.image = bank, int(b), image
        dev, S = bank.device, bank.S
        self.idx = torch.zeros(self.b, dtype=torch.int64, device=dev)
        self.batch = torch.empty(1 + self.b, 3, S, S, dtype=torch.float32, device=dev)
        self.masks = torch.empty(self.b, 1, S, S, dtype=torch.float32, device=dev)
        self.handoff = HandOff(self.batch[1:], self.masks, self.batch)

    def fill(self, replay=False, generator=None):
        idx = self.bank.indices(self.b, generator)
        if replay:
            torch.randperm(self.b)
        if len(idx) != self.b:
            raise RuntimeError(f"a captured step 3 reads {self.b} samples; the bank holds {len(self.bank)}: collect at "
                               "least step3_batch samples in every step-2 block, or lower step3_batch")
        self.idx.copy_(idx)
        self.bank.gather_into(self.idx, self.image, self.batch, self.masks)
        return self.handoff
