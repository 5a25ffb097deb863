"""-m gpu: the projected-sample bank on the device (config `collect_iters`, gan2shape_amd/bank.py, csrc/bank.hip,
DESIGN.md §4.27).  A gather copies, so every comparison is torch.equal: against index_select + cat for the kernel,
against the existing hand-off path for step 3, against the eager loop for the graphed one (deterministic mode, where the
nets repeat bit for bit)."""
import collections
import ctypes as C

import numpy as np
import pytest
import torch

import model_cases as mc
import sample_bank_cases as sbc
from canary_buffers import Buffers

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def glib():
    import gan2shape_amd  # noqa: F401
    from gan2shape_amd import lib
    lib.load()
    return lib


@pytest.fixture(scope="module")
def deterministic(glib):
    prev = glib.set_deterministic(True)
    yield
    glib.set_deterministic(prev)


def raw_gather(lib, images, masks, rows, idx, head, out_img, out_mask, S, err):
    h = 0 if head is None else 1
    lib.check(lib.load().g2s_bank_gather(lib.ptr(images), lib.ptr(masks), C.c_int64(rows), lib.ptr(idx),
                                         int(idx.dtype == torch.int64), idx.numel(), lib.ptr(head), h, lib.ptr(out_img),
                                         lib.ptr(out_mask), S, lib.ptr(err), lib.stream()))


def test_symbol_is_bound(glib):
    assert "g2s_bank_gather" in glib.SIGNATURES and glib.load().g2s_bank_gather is not None


# ---------------------------------------------------------------------------------------------- exact gather
@pytest.mark.parametrize("case", sbc.CASES, ids=sbc.IDS)
def test_kernel_equals_index_select_and_cat_between_canaries(glib, case):
    _, S, rows, b, h, kind, shift = case
    images, masks, head = sbc.make_data(S, rows)
    for dtype in (torch.int64, torch.int32):
        idx = sbc.make_index(kind, rows, b).to(dtype)
        want_batch, want_masks = sbc.reference(images.cuda(), masks.cuda(), head.cuda(), idx.cuda(), h)
        bufs = Buffers()
        d_img = bufs.view("bank images", images.numpy(), shift=shift)
        d_mask = bufs.view("bank masks", masks.numpy(), shift=shift)
        d_head = bufs.view("head", head.numpy()) if h else None
        out_img = bufs.view("out images", like=np.empty((h + b, 3, S, S)), shift=shift)
        out_mask = bufs.view("out masks", like=np.empty((b, 1, S, S)), shift=shift)
        err = torch.zeros(1, dtype=torch.int32, device="cuda")
        raw_gather(glib, d_img, d_mask, rows, idx.cuda(), d_head, out_img, out_mask, S, err)
        torch.cuda.synchronize()
        assert torch.equal(out_img.view(h + b, 3, S, S), want_batch), (case, dtype)
        assert torch.equal(out_mask.view(b, 1, S, S), want_masks), (case, dtype)
        assert int(err.item()) == 0
        bufs.check()


@pytest.mark.parametrize("case", [c for c in sbc.CASES if not c[6]], ids=[c[0] for c in sbc.CASES if not c[6]])
def test_bank_gather_on_the_device(glib, case):
    """SampleBank.gather with a CPU and with a device index: the same HandOff as on the CPU."""
    from gan2shape_amd.bank import HandOff, SampleBank
    _, S, rows, b, h, kind, _ = case
    images, masks, head = sbc.make_data(S, rows)
    bank = SampleBank(1, rows, S, device="cuda")
    bank.put(images.cuda(), masks.cuda())
    idx = sbc.make_index(kind, rows, b)
    want_batch, want_masks = sbc.reference(images, masks, head, idx, h)
    for index in (idx, idx.cuda(), idx.to(torch.int32).cuda()):
        got = bank.gather(index, head.cuda() if h else None)
        assert isinstance(got, HandOff) and got[0].is_cuda
        assert torch.equal(got[0].cpu(), want_batch[h:]) and torch.equal(got[1].cpu(), want_masks)
        if h:
            assert torch.equal(got.batch.cpu(), want_batch) and got[0].data_ptr() == got.batch[1:].data_ptr()
        else:
            assert got.batch is None
    bank.reset()        # reads the error word of the device-index launches: none was set
    bank.put(images.cuda(), masks.cuda())
    with pytest.raises(IndexError, match="out of range"):
        bank.gather(torch.tensor([rows]))       # a CPU index is checked on the host


# ---------------------------------------------------------------------------------------------- device-side index check
def test_bad_device_index_is_clamped_and_reported(glib):
    """A valid launch whose index holds values outside the bank: the rows are those of the clamped index, nothing
    outside the outputs is written, and the error word names a bad entry."""
    from gan2shape_amd.bank import SampleBank
    S, rows, b = 8, 5, 4
    images, masks, head = sbc.make_data(S, rows)
    bad = torch.tensor([1, rows + 7, -3, 4])
    clamped = bad.clamp(0, rows - 1)
    want_batch, want_masks = sbc.reference(images, masks, head, clamped, 1)
    for dtype in (torch.int64, torch.int32):
        bufs = Buffers()
        d_img, d_mask = bufs.view("bank images", images.numpy()), bufs.view("bank masks", masks.numpy())
        d_head = bufs.view("head", head.numpy())
        out_img = bufs.view("out images", like=np.empty((1 + b, 3, S, S)))
        out_mask = bufs.view("out masks", like=np.empty((b, 1, S, S)))
        err = torch.zeros(1, dtype=torch.int32, device="cuda")
        raw_gather(glib, d_img, d_mask, rows, bad.to(dtype).cuda(), d_head, out_img, out_mask, S, err)
        torch.cuda.synchronize()
        assert torch.equal(out_img.view(1 + b, 3, S, S).cpu(), want_batch)
        assert torch.equal(out_mask.view(b, 1, S, S).cpu(), want_masks)
        assert int(err.item()) in (2, 3)        # 1-based position of one of the two bad entries
        bufs.check()
    # through the bank: the gather returns the clamped rows, the NEXT host-side call reports, then the bank works on
    bank = SampleBank(1, rows, S, device="cuda")
    bank.put(images.cuda(), masks.cuda())
    got = bank.gather(bad.cuda(), head.cuda())
    assert torch.equal(got.batch.cpu(), want_batch) and torch.equal(got[1].cpu(), want_masks)
    with pytest.raises(IndexError, match="clamped"):
        bank.indices(2)
    good = bank.gather(torch.tensor([0, 1]).cuda())
    assert torch.equal(good[0].cpu(), images[:2])
    bank.reset()        # nothing pending any more


# ---------------------------------------------------------------------------------------------- graph replay
def test_captured_gather_follows_the_index_buffer(glib):
    from gan2shape_amd.bank import SampleBank
    S, rows, b = 16, 12, 5
    images, masks, head = sbc.make_data(S, rows)
    bank = SampleBank(1, rows, S, device="cuda")
    bank.put(images.cuda(), masks.cuda())
    d_head = head.cuda()
    idx = torch.zeros(b, dtype=torch.int64, device="cuda")
    batch = torch.empty(1 + b, 3, S, S, device="cuda")
    out_masks = torch.empty(b, 1, S, S, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        bank.gather_into(idx, d_head, batch, out_masks)      # a launch before the capture (module load)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        bank.gather_into(idx, d_head, batch, out_masks)
    for k in range(3):
        pick = sbc.make_index("distinct", rows, b, seed=k)
        idx.copy_(pick)
        batch.fill_(-1.0), out_masks.fill_(-1.0)
        g.replay()
        eager = bank.gather(pick, d_head)
        assert torch.equal(batch, eager.batch) and torch.equal(out_masks, eager[1]), k
        assert torch.equal(batch.cpu(), sbc.reference(images, masks, head, pick, 1)[0])


# ---------------------------------------------------------------------------------------------- step 3
def build_model():
    import bench
    from gan2shape_amd.model import GAN2Shape
    cfg = bench.face_config(n_proj=mc.STEP_CFG["n_proj"])
    torch.manual_seed(0)
    m = GAN2Shape(cfg, device="cuda")
    for name in m.NETS:
        mc.fill_scaled(getattr(m, f"{name}_net"), mc.STEP_CFG["seeds"][name])
    mc.smooth_depth_net(m.depth_net)
    return m


def test_step3_on_a_bank_handoff_is_bit_identical(deterministic, golden):
    """forward_step3 fed by bank.gather(idx, image) (the prebuilt [image; samples] batch, no cat) against the same
    step fed by (imgs[idx], masks[idx]) on the existing path: same loss, same gradient of every parameter, bit for bit."""
    from gan2shape_amd.bank import SampleBank
    g = golden("steps")
    image, latent = torch.tensor(g["image"]).cuda(), torch.tensor(g["latent"]).cuda()
    m = build_model()
    S, n = mc.STEP_CFG["image_size"], mc.STEP_CFG["n_proj"]
    bank = SampleBank(2, n, S, device="cuda")
    with torch.no_grad():
        _, c1 = m.forward_step1(image, latent, None)
        for seed in (3, 4):
            torch.manual_seed(seed)
            _, c2 = m.forward_step2(image, latent, c1, n_proj_samples=n)
            bank.put(*c2)
    assert len(bank) == 2 * n and not torch.equal(bank.images[:n], bank.images[n:])
    idx = torch.tensor([2, 0, 3])
    imgs, masks = bank.images.clone(), bank.masks.clone()
    results = []
    for source in ("bank", "plain"):
        handoff = bank.gather(idx, image) if source == "bank" else (imgs[idx.cuda()], masks[idx.cuda()])
        assert (getattr(handoff, "batch", None) is not None) == (source == "bank")
        for p in m.parameters():
            p.grad = None
        loss, _ = m.forward_step3(image, latent, handoff)
        loss.backward()
        results.append((loss.detach().clone(), {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}))
    (loss_b, grads_b), (loss_p, grads_p) = results
    print(f"[sample bank] step-3 loss bank {float(loss_b):.9f} plain {float(loss_p):.9f}; {len(grads_b)} gradients")
    assert torch.equal(loss_b, loss_p), (float(loss_b), float(loss_p))
    assert grads_b.keys() == grads_p.keys() and len(grads_b) > 0
    for k in grads_b:
        assert torch.equal(grads_b[k], grads_p[k]), k
    # a `batch` that is not [image; projected_samples] around these very samples is refused, not trusted
    from gan2shape_amd.bank import HandOff
    good = bank.gather(idx, image)
    for wrong in (HandOff(good[0].clone(), good[1], good.batch), HandOff(good[0][:2], good[1][:2], good.batch)):
        with pytest.raises(ValueError, match="batch"):
            m.forward_step3(image, latent, wrong)


# ---------------------------------------------------------------------------------------------- the trainers
def make_trainer(**over):
    import bench
    from gan2shape_amd.model import GAN2Shape
    from gan2shape_amd.trainer import Trainer
    cfg = bench.face_config(n_proj=2)
    cfg.update(over)
    torch.manual_seed(0)
    t = Trainer(GAN2Shape, cfg, device=torch.device("cuda"), capturable=True)
    image, latent = bench.synthetic_sample(t.model, 1234, torch.device("cuda"))
    return t, [(image[0].cpu(), latent[0].cpu(), 0)]


def parameters_of(t):
    return {k: p.detach().clone() for k, p in t.model.named_parameters() if p.requires_grad}


def test_short_fit_graphed_equals_eager(deterministic):
    """Stages of 1 / 3 / 2 iterations with collect_iters = 2, seeded, eager and graphs=True: identical parameters."""
    dev = torch.device("cuda")
    torch.cuda.set_stream(torch.cuda.Stream(dev))     # captures need a non-default stream
    try:
        stages = [{'step1': 1, 'step2': 3, 'step3': 2}]
        out = {}
        for graphs in (False, True):
            t, data = make_trainer(collect_iters=2)
            torch.manual_seed(1)
            assert t.fit(data, stages=stages, graphs=graphs) == 6
            torch.cuda.synchronize()
            assert len(t.bank) == 4       # iterations 2 and 3 of the step-2 block
            out[graphs] = (parameters_of(t), [h[3] for h in t.history], t.bank.images.clone())
        print("[sample bank] history eager", out[False][1], "graphed", out[True][1])
        assert torch.equal(out[False][2], out[True][2])      # the banks hold the same samples
        differing = [k for k in out[False][0] if not torch.equal(out[False][0][k], out[True][0][k])]
        assert not differing, differing[:5]
    finally:
        torch.cuda.set_stream(torch.cuda.default_stream(dev))


def test_graphed_fit_replays_with_the_bank(deterministic):
    """Blocks longer than the warm-up, two stages: step-2 replays feed the bank, every step-3 iteration (warm-up or
    replay) reads static buffers that one draw and one gather filled from the bank's rows."""
    import math
    from gan2shape_amd import bank as bank_mod
    dev = torch.device("cuda")
    torch.cuda.set_stream(torch.cuda.Stream(dev))
    fill0 = bank_mod.StaticHandOff.fill
    fills = []

    def spy(self, replay=False, generator=None):
        handoff = fill0(self, replay, generator)
        rows = self.idx.cpu()
        fills.append((len(self.bank), bool(torch.equal(self.batch[1:], self.bank.images[rows.cuda()])
                                           and torch.equal(self.masks, self.bank.masks[rows.cuda()])
                                           and torch.equal(self.batch[:1], self.image))))
        return handoff
    bank_mod.StaticHandOff.fill = spy
    try:
        t, data = make_trainer(collect_iters=2, step3_batch=3)
        stages = [{'step1': 1, 'step2': 5, 'step3': 5}, {'step1': 1, 'step2': 4, 'step3': 4}]
        torch.manual_seed(1)
        assert t.fit(data, stages=stages, graphs=True) == 20
        torch.cuda.synchronize()
        assert len(fills) == 9 and all(n == 4 and ok for n, ok in fills), fills
        assert all(math.isfinite(h[3]) for h in t.history)
    finally:
        bank_mod.StaticHandOff.fill = fill0
        torch.cuda.set_stream(torch.cuda.default_stream(dev))


def test_graphed_fit_draws_the_eager_fit_s_indices(deterministic):
    """Two stages with blocks longer than the warm-up, so steps 2 and 3 are replayed and step 3 is captured: the
    seeded graphed fit draws, iteration by iteration, the indices the eager fit draws, and leaves the CPU generator
    where the eager fit leaves it (a replayed step 3 does not run forward_step3's own draw, and a capture runs it
    once more: graphs.py and bank.StaticHandOff.fill make up for both).  What the rows HOLD differs between the two
    runs once step 2 is replayed — its views and lights come from the device generator, which a replay advances
    differently, as for the plain loop — so the parameters are not compared here."""
    dev = torch.device("cuda")
    torch.cuda.set_stream(torch.cuda.Stream(dev))
    try:
        stages = [{'step1': 1, 'step2': 5, 'step3': 5}, {'step1': 1, 'step2': 4, 'step3': 4}]
        out = {}
        for graphs in (False, True):
            t, data = make_trainer(collect_iters=3, step3_batch=4)
            t.debug = True
            drawn, indices0 = [], t.bank.indices

            def indices(b, generator=None, drawn=drawn, indices0=indices0):
                idx = indices0(b, generator)
                drawn.append(idx.tolist())
                return idx
            t.bank.indices = indices
            torch.manual_seed(1)
            assert t.fit(data, stages=stages, graphs=graphs) == 20
            torch.cuda.synchronize()
            out[graphs] = (drawn, torch.rand(3))
        assert len(out[False][0]) == 9 and all(len(set(i)) == 4 and max(i) < 6 for i in out[False][0])
        assert out[True][0] == out[False][0], (out[True][0], out[False][0])
        assert torch.equal(out[True][1], out[False][1])
    finally:
        torch.cuda.set_stream(torch.cuda.default_stream(dev))


@pytest.mark.parametrize("shifts", [(0, 1), (1, 0)], ids=["mask_unaligned", "images_unaligned"])
def test_kernel_with_one_copy_vectorised_and_one_not(glib, shifts):
    """The launcher chooses the access width separately for the image copy and the mask copy: S = 8 (rows of 192 and
    64 floats) with only the masks', or only the images', buffers one float off 16-byte alignment."""
    S, rows, b = 8, 5, 3
    shift_img, shift_mask = shifts
    images, masks, head = sbc.make_data(S, rows)
    idx = sbc.make_index("distinct", rows, b)
    want_batch, want_masks = sbc.reference(images, masks, head, idx, 1)
    bufs = Buffers()
    d_img = bufs.view("bank images", images.numpy(), shift=shift_img)
    d_mask = bufs.view("bank masks", masks.numpy(), shift=shift_mask)
    d_head = bufs.view("head", head.numpy())
    out_img = bufs.view("out images", like=np.empty((1 + b, 3, S, S)), shift=shift_img)
    out_mask = bufs.view("out masks", like=np.empty((b, 1, S, S)), shift=shift_mask)
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    raw_gather(glib, d_img, d_mask, rows, idx.cuda(), d_head, out_img, out_mask, S, err)
    torch.cuda.synchronize()
    assert torch.equal(out_img.view(1 + b, 3, S, S).cpu(), want_batch)
    assert torch.equal(out_mask.view(b, 1, S, S).cpu(), want_masks)
    assert int(err.item()) == 0
    bufs.check()


@pytest.mark.parametrize("graphs", [False, True], ids=["eager", "graphed"])
def test_joint_trainer_draws_from_a_bank_per_image(deterministic, graphs):
    """GeneralizingTrainer2.fit over two images, eager and graphs=True (image 0: three warm-ups and a replay per step
    kind, image 1: replays only): every step-3 iteration reads rows of the bank, which holds the CURRENT image's last two step-2
    iterations — the samples of image 0 are gone when image 1 draws."""
    import math
    import bench
    from gan2shape_amd.model import GAN2Shape
    from gan2shape_amd.trainer import GeneralizingTrainer2
    dev = torch.device("cuda")
    torch.cuda.set_stream(torch.cuda.Stream(dev))
    try:
        cfg = bench.face_config(n_proj=2)
        cfg.update(n_epochs_prior=1, n_epochs_generalized=1, collect_iters=2)
        torch.manual_seed(0)
        t = GeneralizingTrainer2(GAN2Shape, cfg, device=dev, capturable=True)
        data = []
        for i in range(2):
            image, latent = bench.synthetic_sample(t.model, 100 + i, dev)
            data.append((image[0].cpu(), latent[0].cpu(), i))
        seen = []       # per step-3 iteration: (rows in the bank, hand-off rows all found in the bank, bank contents)

        def record(handoff, image):
            projected, masks = handoff
            held = t.bank.images[:len(t.bank)]
            found = all(any(torch.equal(projected[j], row) for row in held) for j in range(len(projected)))
            seen.append((len(t.bank), found and torch.equal(handoff.batch[:1], image), t.bank.images.clone()))
            return handoff
        # both hooks run eagerly in front of the iteration (a replayed step never passes through Python)
        from gan2shape_amd import bank as bank_mod
        fill0, draw0 = bank_mod.StaticHandOff.fill, t._bank_draw
        bank_mod.StaticHandOff.fill = lambda self, replay=False, generator=None: record(fill0(self, replay, generator), self.image)
        t._bank_draw = lambda image: record(draw0(image), image)
        try:
            assert t.fit(data, stages=[{'step1': 1, 'step2': 4, 'step3': 4}], batch_size=2, graphs=graphs) == 1 + 2 * 8
        finally:
            bank_mod.StaticHandOff.fill = fill0
        torch.cuda.synchronize()
        assert len(seen) == 8, len(seen)
        assert all(n == 4 and ok for n, ok, _ in seen), [(n, ok) for n, ok, _ in seen]
        assert not torch.equal(seen[0][2], seen[-1][2])      # image 1 drew from its own samples
        assert all(v is None or math.isfinite(v) for *_, v in t.history)
    finally:
        torch.cuda.set_stream(torch.cuda.default_stream(dev))


def kernel_names(fn):
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return collections.Counter(e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA
                               and not e.name.lower().startswith(("memcpy", "memset")))


def test_off_is_the_plain_loop(deterministic):
    """Without `collect_iters` the trainer builds no bank and Trainer.fit is the loop it was before the bank existed:
    a literal restatement of that loop, which touches nothing of the bank, ends on the same parameters bit for bit
    and launches the same kernels the same number of times."""
    from torch.utils.data import DataLoader
    from gan2shape_amd import zeropool
    stages = [{'step1': 1, 'step2': 3, 'step3': 2}]

    def plain_loop(t, data):
        for image, latent, index in DataLoader(data, batch_size=1, shuffle=False):
            image, latent = image.to(t.device), latent.to(t.device)
            for stage in range(len(stages)):
                old = None
                t._set_flips(stage)
                for step in (1, 2, 3):
                    optim, forward = getattr(t, f'optim_step{step}'), getattr(t.model, f'forward_step{step}')
                    collected = None
                    for _ in range(stages[stage][f'step{step}']):
                        optim.zero_grad()
                        loss, collected = forward(image, latent, old, n_proj_samples=t.n_proj_samples)
                        loss.backward()
                        optim.step()
                        zeropool.end()
                    old = collected

    import importlib
    fir_cache = importlib.import_module("gan2shape_amd.op.upfirdn2d")._FLIPPED
    out = {}
    for how in ("warm", "fit", "plain"):       # the first run of a process also fills lazily built workspaces
        t, data = make_trainer()
        t.debug = True      # no prior pre-training in fit: the comparison is about the step loop
        # the process-wide cache of flipped FIR kernels empties itself past 64 entries and is then refilled by
        # whichever run comes next: start both runs from an empty one
        fir_cache.clear()
        assert t.bank is None and t.collect_iters == 0
        torch.manual_seed(1)
        names = kernel_names((lambda: t.fit(data, stages=stages)) if how != "plain" else (lambda: plain_loop(t, data)))
        out[how] = (parameters_of(t), names)
    assert sum(out["fit"][1].values()) > 1000 and not any("bank_gather" in k for k in out["fit"][1])
    assert out["fit"][1] == out["plain"][1], {k: (v, out["plain"][1].get(k)) for k, v in out["fit"][1].items()
                                              if out["plain"][1].get(k) != v}
    differing = [k for k in out["fit"][0] if not torch.equal(out["fit"][0][k], out["plain"][0][k])]
    assert not differing, differing[:5]
    # and with the bank on, every step-3 iteration launches the gather once and no concatenation of the batch
    t, data = make_trainer(collect_iters=2)
    t.debug = True
    torch.manual_seed(1)
    on = kernel_names(lambda: t.fit(data, stages=stages))
    assert sum(v for k, v in on.items() if "bank_gather" in k) == 2
