"""The projected-sample bank without a GPU (config `collect_iters`, gan2shape_amd/bank.py): the ring,
the index draw, the CPU gather (index_select), and the trainers' use of the bank, driven by a stub model class with the
reference's step signatures that records what every step received."""
import pytest
import torch

import sample_bank_cases as sbc

import gan2shape_amd  # noqa: F401
from gan2shape_amd.bank import HandOff, SampleBank, bank_bytes
from gan2shape_amd.trainer import GeneralizingTrainer2, Trainer


def rows_of(k, n=2, S=4):
    """The projected images and masks of 'iteration' k: constant rows, each with its own value."""
    vals = torch.arange(n, dtype=torch.float32) + 10.0 * k
    return vals.reshape(n, 1, 1, 1).expand(n, 3, S, S).contiguous(), -vals.reshape(n, 1, 1, 1).expand(n, 1, S, S).contiguous()


# ---------------------------------------------------------------------------------------------- the ring
def test_ring_put_wrap_reset_len():
    K, n, S = 3, 2, 4
    bank = SampleBank(K, n, S, device="cpu")
    assert len(bank) == 0 and tuple(bank.images.shape) == (K * n, 3, S, S) and tuple(bank.masks.shape) == (K * n, 1, S, S)
    assert bank.images.dtype == bank.masks.dtype == torch.float32
    for k in range(1, K + 3):       # K + 2 puts: the bank holds the last K
        bank.put(*rows_of(k, n, S))
        assert len(bank) == min(k, K) * n
    held = sorted(bank.images[:len(bank), 0, 0, 0].tolist())
    want = sorted(float(v) for k in range(3, K + 3) for v in rows_of(k, n, S)[0][:, 0, 0, 0])
    assert held == want
    assert torch.equal(bank.masks[:, 0, 0, 0], -bank.images[:, 0, 0, 0])       # a mask stays with its image
    bank.reset()
    assert len(bank) == 0
    bank.put(*rows_of(9, n, S))
    assert len(bank) == n and bank.images[:n, 0, 0, 0].tolist() == [90.0, 91.0]


def test_put_refuses_wrong_shapes_and_attached_tensors():
    bank = SampleBank(2, 2, 4, device="cpu")
    img, mask = rows_of(1)
    with pytest.raises(ValueError, match="expected"):
        bank.put(img[:1], mask[:1])
    with pytest.raises(ValueError, match="detached"):
        bank.put(img.requires_grad_(True), mask)


# ---------------------------------------------------------------------------------------------- the draw
def test_indices_is_the_reference_randperm_and_one_draw():
    bank = SampleBank(3, 2, 4, device="cpu")
    for k in range(3):
        bank.put(*rows_of(k))
    torch.manual_seed(11)
    got = bank.indices(4)
    after = torch.rand(1)
    torch.manual_seed(11)
    want = torch.randperm(6)[:4]
    assert torch.equal(got, want) and got.dtype == torch.int64 and not got.is_cuda
    assert torch.equal(after, torch.rand(1))        # exactly one draw was consumed
    g = torch.Generator().manual_seed(5)
    state = torch.get_rng_state()
    got = bank.indices(2, generator=g)
    assert torch.equal(got, torch.randperm(6, generator=torch.Generator().manual_seed(5))[:2])
    assert torch.equal(state, torch.get_rng_state())        # the global generator was left alone
    everything = bank.indices(100)      # b > len: all rows, permuted
    assert sorted(everything.tolist()) == list(range(6))


def test_empty_bank_and_out_of_range_index_raise():
    bank = SampleBank(2, 2, 4, device="cpu")
    with pytest.raises(RuntimeError, match="empty"):
        bank.indices(1)
    with pytest.raises(RuntimeError, match="empty"):
        bank.gather(torch.tensor([0]))
    bank.put(*rows_of(1))
    for bad in ([2], [-1], [0, 5]):     # 2 valid rows (rows 2, 3 of the storage are not valid yet)
        with pytest.raises(IndexError, match="out of range"):
            bank.gather(torch.tensor(bad))
    with pytest.raises(ValueError, match="int64 or int32"):
        bank.gather(torch.tensor([0.0]))


# ---------------------------------------------------------------------------------------------- the gather
@pytest.mark.parametrize("case", sbc.CASES, ids=sbc.IDS)
def test_cpu_gather_equals_index_select_and_cat(case):
    _, S, rows, b, h, kind, shift = case
    images, masks, head = sbc.make_data(S, rows)
    bank = SampleBank(1, rows, S, device="cpu")
    if shift:       # the bank's tensors as views one float into their storage
        for name in ("images", "masks"):
            t = getattr(bank, name)
            setattr(bank, name, torch.zeros(t.numel() + shift)[shift:].view(t.shape))
    bank.put(images, masks)
    for dtype in (torch.int64, torch.int32):
        idx = sbc.make_index(kind, rows, b).to(dtype)
        got = bank.gather(idx, head if h else None)
        want_batch, want_masks = sbc.reference(images, masks, head, idx, h)
        assert isinstance(got, HandOff) and len(got) == 2
        projected, got_masks = got
        assert torch.equal(projected, want_batch[h:]) and torch.equal(got_masks, want_masks)
        if h:
            assert torch.equal(got.batch, want_batch)
            assert projected.data_ptr() == got.batch[1:].data_ptr()     # a view of rows 1 .., not a copy
        else:
            assert got.batch is None


# ---------------------------------------------------------------------------------------------- the trainers
S_STUB, N_STUB = 4, 2


class StubModel(torch.nn.Module):
    """The reference's step signatures; step 2 returns samples that name their iteration, and every step records
    what it was handed."""

    def __init__(self, config, debug=False):
        super().__init__()
        for name in ("albedo", "offset_encoder", "lighting", "viewpoint", "depth"):
            setattr(self, f"{name}_net", torch.nn.Linear(2, 1))
        self.step2_calls = 0
        self.step2_out = []     # the object each step-2 call returned
        self.seen3 = []         # the object each step-3 call received

    def _loss(self, net):
        return getattr(self, f"{net}_net")(torch.ones(1, 2)).sum()

    def forward_step1(self, images, latents, collected, **kw):
        normal = torch.zeros(len(images), 1)
        return self._loss("albedo"), (normal, normal, normal, normal, normal, None if len(images) == 1 else [None] * len(images))

    def forward_step2(self, image, latent, collected, n_proj_samples=8, **kw):
        self.step2_calls += 1
        out = rows_of(self.step2_calls, n_proj_samples, S_STUB)
        self.step2_out.append(out)
        self.on_step2()
        return self._loss("offset_encoder"), out

    def forward_step3(self, image, latent, collected, **kw):
        self.seen3.append(collected)
        return self._loss("depth") + self._loss("lighting") + self._loss("viewpoint") + self._loss("albedo"), None

    def on_step2(self):
        pass


def stub_config(**over):
    cfg = {"image_size": S_STUB, "category": "face", "n_proj_samples": N_STUB, "n_epochs_prior": 0, "prior_name": "ellipsoid",
           "n_epochs_generalized": 1}
    cfg.update(over)
    return cfg


def stub_data(n=1):
    g = torch.Generator().manual_seed(3)
    return [(torch.randn(3, S_STUB, S_STUB, generator=g), torch.randn(8, generator=g), i) for i in range(n)]


def loader_draws(data, batch_size=1):
    """Consume from the global CPU generator what the trainer's DataLoader does when it is iterated once."""
    from torch.utils.data import DataLoader
    for _ in DataLoader(data, batch_size=batch_size, shuffle=False):
        pass


def sample_values(k):
    """The values that mark the rows of step-2 call k (rows_of)."""
    return {float(v) for v in rows_of(k, N_STUB, S_STUB)[0][:, 0, 0, 0]}


def test_off_hands_step3_the_last_step2_object():
    assert "collect_iters" not in stub_config()
    for cfg in (stub_config(), stub_config(collect_iters=0)):
        t = Trainer(StubModel, cfg, debug=True, device="cpu")
        assert t.collect_iters == 0 and t.bank is None
        torch.manual_seed(4)
        t.fit(stub_data(), stages=[{'step1': 1, 'step2': 3, 'step3': 2}])
        after = torch.rand(1)
        torch.manual_seed(4)
        loader_draws(stub_data())
        assert torch.equal(after, torch.rand(1))        # beyond its data loader the trainer drew nothing
        m = t.model
        assert len(m.seen3) == 2 and all(c is m.step2_out[-1] for c in m.seen3)


def test_on_step3_draws_from_the_last_collect_iters_iterations():
    t = Trainer(StubModel, stub_config(collect_iters=2, step3_batch=3), debug=True, device="cpu")
    assert t.collect_iters == 2 and t.step3_batch == 3 and len(t.bank) == 0
    m = t.model
    lens = []
    m.on_step2 = lambda: lens.append(len(t.bank))       # the bank as each step-2 call finds it
    torch.manual_seed(0)
    stages = [{'step1': 1, 'step2': 5, 'step3': 4}, {'step1': 1, 'step2': 1, 'step3': 2}]
    t.fit(stub_data(), stages=stages)
    # stage 0: the bank is empty at the block's start and holds iterations 4 and 5 at its end
    assert lens[:5] == [0, 0, 0, 0, N_STUB]
    allowed = sample_values(4) | sample_values(5)
    assert len(m.seen3) == 6
    drawn = set()
    for c in m.seen3[:4]:
        projected, masks = c
        assert tuple(projected.shape) == (3, 3, S_STUB, S_STUB) and tuple(masks.shape) == (3, 1, S_STUB, S_STUB)
        vals = projected[:, 0, 0, 0].tolist()
        assert set(vals) <= allowed and len(set(vals)) == 3     # distinct rows of the bank: a permutation's head
        assert torch.equal(masks[:, 0, 0, 0], -projected[:, 0, 0, 0])
        assert (projected == projected[:, :1, :1, :1]).all()       # whole rows
        drawn |= set(vals)
    assert len(drawn) == 4      # 4 draws of 3 from 4 rows: all of them turned up (seed 0)
    # stage 1: emptied at the next step 2 (a block shorter than collect_iters keeps all of its iterations: one)
    assert lens[5] == 0
    for c in m.seen3[4:]:
        assert len(c[0]) == N_STUB and set(c[0][:, 0, 0, 0].tolist()) == sample_values(6)      # b > len: all rows
    # the image rides in front: batch = [image; projected_samples]
    image = stub_data()[0][0][None]
    for c in m.seen3:
        assert torch.equal(c.batch[:1], image) and torch.equal(c.batch[1:], c[0])


def test_on_one_extra_draw_per_step3_iteration():
    t = Trainer(StubModel, stub_config(collect_iters=1), debug=True, device="cpu")
    torch.manual_seed(4)
    t.fit(stub_data(), stages=[{'step1': 1, 'step2': 1, 'step3': 3}])
    after = torch.rand(1)
    torch.manual_seed(4)
    loader_draws(stub_data())
    picks = [torch.randperm(N_STUB)[:N_STUB] for _ in range(3)]
    assert torch.equal(after, torch.rand(1))
    for c, idx in zip(t.model.seen3, picks):
        assert torch.equal(c[0], rows_of(1, N_STUB, S_STUB)[0][idx])


def test_joint_trainer_resets_the_bank_per_image():
    t = GeneralizingTrainer2(StubModel, stub_config(collect_iters=2), debug=True, device="cpu", load_dict=None)
    t.pretrain_on_prior_all = lambda *a, **k: None      # the stub has no depth_net_forward
    m = t.model
    lens = []
    m.on_step2 = lambda: lens.append(len(t.bank))
    t.fit(stub_data(2), stages=[{'step1': 1, 'step2': 3, 'step3': 2}], batch_size=2)
    assert lens == [0, 0, N_STUB, 0, 0, N_STUB]         # emptied for the second image
    assert len(m.seen3) == 4
    for c in m.seen3[:2]:
        assert set(c[0][:, 0, 0, 0].tolist()) <= sample_values(2) | sample_values(3)
    for c in m.seen3[2:]:
        assert set(c[0][:, 0, 0, 0].tolist()) <= sample_values(5) | sample_values(6)
    off = GeneralizingTrainer2(StubModel, stub_config(), debug=True, device="cpu")
    off.pretrain_on_prior_all = lambda *a, **k: None
    off.fit(stub_data(2), stages=[{'step1': 1, 'step2': 2, 'step3': 1}], batch_size=2)
    assert off.bank is None and off.model.seen3[0] is off.model.step2_out[1] and off.model.seen3[1] is off.model.step2_out[3]


def test_memory_cap_is_refused_at_construction():
    need = bank_bytes(5, N_STUB, S_STUB)
    assert need == 5 * N_STUB * 4 * S_STUB * S_STUB * 4
    Trainer(StubModel, stub_config(collect_iters=5, bank_max_bytes=need), debug=True, device="cpu")
    with pytest.raises(ValueError) as e:
        Trainer(StubModel, stub_config(collect_iters=5, bank_max_bytes=need - 1), debug=True, device="cpu")
    msg = str(e.value)
    assert "collect_iters=5" in msg and f"n_proj_samples={N_STUB}" in msg and f"image_size={S_STUB}" in msg
    assert str(need) in msg and f"bank_max_bytes={need - 1}" in msg
    # the default cap is 2 GiB: 800 rows at 128 x 128 (210 MB) pass, 8000 rows at 256 x 256 (8.4 GB) do not
    assert bank_bytes(100, 8, 128) < 2 << 30 < bank_bytes(1000, 8, 256)
    with pytest.raises(ValueError, match="bank_max_bytes"):
        Trainer(StubModel, stub_config(collect_iters=1000, n_proj_samples=8, image_size=256), debug=True, device="cpu")
