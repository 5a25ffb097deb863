"""Short seeded fits of the four training loops (Trainer.fit and GeneralizingTrainer2.fit, eager and graphs=True), with
the projected-sample bank off and on, shared by tests/golden/make_step_runner_golden.py (which records them at one
commit) and tests/test_gpu_step_runner.py (which holds every later commit to the record, bit for bit).

The smallest configuration of the existing fit tests (tests/test_gpu_sample_bank.py: bench.face_config(n_proj=2), 128 x
128, blocks of 1 - 4 iterations), two stages whose symmetry flips differ, object masks live.  Callers set the
library's deterministic mode and a non-default current stream."""
import math

import torch

import model_cases as mc

LOOPS = ["image_eager", "image_graphed", "joint_eager", "joint_graphed"]
BANKS = {"bank_off": {}, "bank_on": {"collect_iters": 2}}
CASES = [(loop, bank) for loop in LOOPS for bank in BANKS]
IDS = [f"{loop}-{bank}" for loop, bank in CASES]

# per image: the second stage flips the other way (steps 1 and 3 are captured twice), its step-2 block is longer than
# the warm-up (a replay), and the second image replays every graph
STAGES = [{'step1': 1, 'step2': 3, 'step3': 2}, {'step1': 1, 'step2': 4, 'step3': 2}]
# joint (it reads stages[0] and entry 0 of the flip lists): image 0 warms up and replays once, image 1 replays only
JOINT_STAGES = [{'step1': 1, 'step2': 4, 'step3': 4}, {'step1': 1, 'step2': 3, 'step3': 2}]
FLIPS = {"flip1_cfg": [True, False], "flip3_cfg": [False, True]}


def run_case(loop, bank):
    """One fit -> {"total_it", "history" (losses as float.hex()), "nets": {name: [sum, sum of squares]} (float64, hex)}."""
    import bench
    from gan2shape_amd.model import GAN2Shape
    from gan2shape_amd.trainer import GeneralizingTrainer2, Trainer
    dev = torch.device("cuda")
    joint, graphs = loop.startswith("joint"), loop.endswith("graphed")
    cfg = bench.face_config(n_proj=2)
    cfg.update(object_mask=True, **FLIPS, **BANKS[bank])
    if joint:
        cfg.update(n_epochs_prior=1, n_epochs_generalized=1)
    calls = []

    def mask_fn(images):        # a soft ellipse that moves with every call (once per image, or once per batch)
        calls.append(len(images))
        return mc.parsing_mask(images.shape[-1], cx=0.5 + 0.04 * len(calls)).to(images.device).expand(len(images), -1, -1, -1)
    torch.manual_seed(0)
    t = (GeneralizingTrainer2 if joint else Trainer)(GAN2Shape, cfg, device=dev, capturable=True, object_mask_fn=mask_fn)
    data = []
    for i in range(2):
        image, latent = bench.synthetic_sample(t.model, 100 + i, dev)
        data.append((image[0].cpu(), latent[0].cpu(), i))
    torch.manual_seed(1)
    if joint:
        total = t.fit(data, stages=JOINT_STAGES, batch_size=2, graphs=graphs)
    else:
        total = t.fit(data, stages=STAGES, graphs=graphs)
    torch.cuda.synchronize()
    nets = {}
    for name in t.model.NETS:
        params = [p.detach().double() for p in getattr(t.model, f"{name}_net").parameters()]
        # per tensor on the device, then an exactly rounded sum of the few per-tensor values
        nets[name] = [math.fsum(float(p.sum()) for p in params).hex(), math.fsum(float((p * p).sum()) for p in params).hex()]
    history = [[list(i) if isinstance(i, tuple) else i, stage, step, None if loss is None else float(loss).hex()]
               for i, stage, step, loss in t.history]
    return {"total_it": total, "history": history, "nets": nets, "mask_calls": calls}
