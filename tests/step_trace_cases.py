"""Call traces of the two trainers' eager loops, shared by tests/golden/make_step_trace_golden.py (which records them
at one commit) and tests/test_step_runner_cpu.py (which holds every later commit to the record).

A stub model with the reference's step signatures logs, for every step call: the step kind, what it was handed
(relative to what earlier calls returned), model.flip1 / flip3, the object mask it received, len(trainer.bank) and
a hash of the CPU generator's state.  Its losses are exact constants (the call number), so the `history` rows
compare for equality on any machine; the nets still receive gradients and are stepped."""
import hashlib
import json

import torch

S, N_PROJ = 4, 2

# per-image trainer: two stages that differ, a stage without step 2 (step 3 is handed nothing), a stage without step 1
# whose single step-2 iteration leaves fewer rows in the bank than step3_batch, a stage without step 3
STAGES = [{'step1': 2, 'step2': 3, 'step3': 2}, {'step1': 1, 'step2': 0, 'step3': 1},
          {'step1': 0, 'step2': 1, 'step3': 2}, {'step1': 1, 'step2': 4, 'step3': 0}]
# joint trainer (it reads stages[0] only): one schedule per run
JOINT_STAGES = {"full": {'step1': 2, 'step2': 3, 'step3': 2}, "no_step2": {'step1': 1, 'step2': 0, 'step3': 2},
                "no_step3": {'step1': 1, 'step2': 2, 'step3': 0}, "no_step1": {'step1': 0, 'step2': 2, 'step3': 1}}
# collect_iters below (2) and above (9) the block lengths; step3_batch = 3 of the 2 * 2 rows
BANKS = {"bank_off": {}, "bank_2": {"collect_iters": 2, "step3_batch": 3}, "bank_9": {"collect_iters": 9}}
FLIPS = {"flip1_cfg": [True, False], "flip3_cfg": [False, True]}


def rows_of(k, n=N_PROJ):
    """The projected images and masks of step-2 call k: constant rows, each with its own value."""
    vals = torch.arange(n, dtype=torch.float32) + 10.0 * k
    return vals.reshape(n, 1, 1, 1).expand(n, 3, S, S).contiguous(), -vals.reshape(n, 1, 1, 1).expand(n, 1, S, S).contiguous()


def object_mask_fn(images):
    return (images[:, :1] > 0).float()


class TraceModel(torch.nn.Module):
    def __init__(self, config, debug=False):
        super().__init__()
        for name in ("albedo", "offset_encoder", "lighting", "viewpoint", "depth"):
            setattr(self, f"{name}_net", torch.nn.Linear(2, 1))
        self.trainer = None
        self.calls = 0
        self.outputs = []       # what every call returned as `collected`
        self.trace = []

    def _describe(self, collected, image):
        if collected is None:
            return None
        for j, out in enumerate(self.outputs):
            if collected is out:
                return ["output", j]
        if getattr(collected, "batch", None) is not None:      # a bank hand-off: its rows, and the image in front
            return ["bank", collected[0][:, 0, 0, 0].tolist(), bool(torch.equal(collected.batch[:1], image)),
                    bool(torch.equal(collected[1][:, 0, 0, 0], -collected[0][:, 0, 0, 0]))]
        return ["new", [t.reshape(-1)[:1].tolist() + list(t.shape) if torch.is_tensor(t) else t for t in collected]]

    def _call(self, kind, nets, images, collected, kw, out):
        self.calls += 1
        bank = self.trainer.bank
        mask = kw.get("object_mask")
        self.trace.append({
            "kind": kind, "images": images[:, 0, 0, 0].tolist(), "handoff": self._describe(collected, images),
            "flip1": getattr(self, "flip1", None), "flip3": getattr(self, "flip3", None),
            "mask": None if mask is None else [float(mask.sum())] + list(mask.shape),
            "n_proj_samples": kw.get("n_proj_samples"), "bank": None if bank is None else len(bank),
            "batch_mean": getattr(self, "batch_mean", None) is not None,
            "rng": hashlib.sha1(torch.get_rng_state().numpy().tobytes()).hexdigest()[:16]})
        self.outputs.append(out)
        # an exact loss (the call number) that still reaches every net of the step's optimiser
        return sum(getattr(self, f"{n}_net")(torch.ones(1, 2)).sum() for n in nets) * 0 + float(self.calls), out

    def forward_step1(self, images, latents, collected, **kw):
        v = torch.full((len(images), 1), float(self.calls + 1)) + torch.arange(len(images))[:, None] / 8
        out = (v, v + 100, v + 200, v + 300, v + 400, None if len(images) == 1 else [None] * len(images))
        return self._call(1, ["albedo"], images, collected, kw, out)

    def forward_step2(self, image, latent, collected, **kw):
        return self._call(2, ["offset_encoder"], image, collected, kw, rows_of(self.calls + 1, kw.get("n_proj_samples", 8)))

    def forward_step3(self, image, latent, collected, **kw):
        return self._call(3, ["depth", "lighting", "viewpoint", "albedo"], image, collected, kw, None)


def config(**over):
    cfg = {"image_size": S, "category": "face", "n_proj_samples": N_PROJ, "n_epochs_prior": 0, "prior_name": "ellipsoid",
           "n_epochs_generalized": 2}
    cfg.update(FLIPS)
    cfg.update(over)
    return cfg


def data(n):
    g = torch.Generator().manual_seed(3)
    return [(torch.randn(3, S, S, generator=g), torch.randn(8, generator=g), i) for i in range(n)]


def run_case(joint, bank, masks, stages):
    from gan2shape_amd.trainer import GeneralizingTrainer2, Trainer
    cfg = config(object_mask=masks, **BANKS[bank])
    t = (GeneralizingTrainer2 if joint else Trainer)(TraceModel, cfg, debug=True, device="cpu",
                                                     object_mask_fn=object_mask_fn if masks else None)
    t.model.trainer = t
    torch.manual_seed(7)
    if joint:
        t.pretrain_on_prior_all = lambda *a, **k: None      # the stub has no depth_net_forward
        total = t.fit(data(3), stages=[stages], batch_size=2)
    else:
        total = t.fit(data(2), stages=stages)
    # through JSON: tuples become lists, as in the committed record
    return json.loads(json.dumps({"total_it": total, "history": t.history, "trace": t.model.trace,
                                  "rng_after": hashlib.sha1(torch.get_rng_state().numpy().tobytes()).hexdigest()[:16]}))


def cases():
    """name -> arguments of run_case."""
    out = {}
    for bank in BANKS:
        for masks in (False, True):
            tail = f"{bank}-{'masks' if masks else 'no_masks'}"
            out[f"image-{tail}"] = (False, bank, masks, STAGES)
            for name, stages in JOINT_STAGES.items():
                out[f"joint-{name}-{tail}"] = (True, bank, masks, stages)
    return out
