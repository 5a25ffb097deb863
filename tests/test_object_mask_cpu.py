"""Object masks inside the steps, host side (no GPU): when the masks are live, where the trainers take them from, and
how the joint trainer deals a batch's masks out to its samples."""
import os

import pytest
import torch

import model_cases as mc


@pytest.mark.parametrize("cfg,live", [
    ({}, False),                                            # use_mask defaults to True and switches nothing on
    ({"use_mask": True}, False),
    ({"object_mask": False, "use_mask": True}, False),
    ({"object_mask": True}, True),                          # use_mask defaults to True
    ({"object_mask": True, "use_mask": True}, True),
    ({"object_mask": True, "use_mask": False}, False),      # use_mask False keeps canon_mask None
    ({"object_mask": False, "use_mask": False}, False),
])
def test_masks_are_live_only_with_both_switches(cfg, live):
    from gan2shape_amd.model import GAN2Shape
    from gan2shape_amd.trainer import object_masks_live
    assert object_masks_live(cfg) is live
    m = mc.bare_model()
    assert m.masks_live is False            # the class defaults: object_mask False, use_mask True
    m.use_mask = cfg.get("use_mask", True)                  # as GAN2Shape.__init__ reads the two keys
    m.object_mask = bool(cfg.get("object_mask", False))
    assert m.masks_live is live
    assert GAN2Shape.object_mask is False and GAN2Shape.use_mask is True


class FakeParser:
    def __init__(self):
        self.calls = []

    def image_mask(self, image, depth=None):
        self.calls.append(tuple(image.shape))
        return torch.full((image.shape[0], 1) + tuple(image.shape[-2:]), 0.25)

    def confidence_mask(self, image, depth=None):
        return self.image_mask(image) ** 2


def test_object_mask_fn_resolution_order(monkeypatch, tmp_path):
    from gan2shape_amd import parsing
    from gan2shape_amd.trainer import Trainer
    parser = FakeParser()
    # as parsing.masking_model_from_config: a model when the directory exists (no checkpoints are read here), else None
    monkeypatch.setattr(parsing, "masking_model_from_config", lambda config, device="cuda": (
        parser if os.path.isdir(config.get("parsing_ckpt_dir") or "") else None))
    S = mc.TOY_CFG["image_size"]

    def arg_fn(images):
        return torch.full((len(images), 1, S, S), 0.75)

    def masking_model(image):       # a callable as PriorGenerator takes it: one image per call
        assert len(image) == 1
        return torch.full((1, 1, S, S), 0.5)
    on = dict(mc.TOY_CFG, object_mask=True)
    images = torch.zeros(2, 3, S, S)

    def source(t):
        return float(t.object_masks(images).mean())
    # 1. the argument wins over everything
    t = Trainer(mc.ToyStepModel, dict(on, parsing_ckpt_dir=str(tmp_path)), device="cpu", object_mask_fn=arg_fn,
                masking_model=masking_model)
    assert t.object_mask_fn is arg_fn and source(t) == 0.75
    # 2. the parsing net's image_mask, when parsing_ckpt_dir resolves — also with a masking_model passed in, which
    #    stays the prior's mask source
    t = Trainer(mc.ToyStepModel, dict(on, parsing_ckpt_dir=str(tmp_path)), device="cpu", masking_model=masking_model)
    assert source(t) == 0.25 and t.prior_generator.masking_model is masking_model
    t = Trainer(mc.ToyStepModel, dict(on, parsing_ckpt_dir=str(tmp_path)), device="cpu")
    assert source(t) == 0.25 and parser.calls[-1] == (2, 3, S, S)       # batched
    # 3. a masking_model callable, image by image
    t = Trainer(mc.ToyStepModel, dict(on, parsing_ckpt_dir=str(tmp_path / "absent")), device="cpu",
                masking_model=masking_model)
    assert t.object_mask_fn is masking_model and source(t) == 0.5
    masks = t.object_masks(images)
    assert tuple(masks.shape) == (2, 1, S, S) and masks.dtype == torch.float32 and not masks.requires_grad
    # none of the three: refused at construction, and the message names the key
    for cfg in (on, dict(on, parsing_ckpt_dir=str(tmp_path / "absent"))):
        with pytest.raises(ValueError, match="parsing_ckpt_dir"):
            Trainer(mc.ToyStepModel, cfg, device="cpu")
    # with the switch off nothing is resolved, asked for or handed on
    for cfg in (dict(mc.TOY_CFG), dict(mc.TOY_CFG, use_mask=True), dict(on, use_mask=False)):
        t = Trainer(mc.ToyStepModel, cfg, device="cpu", object_mask_fn=arg_fn)
        assert t.object_mask is False and t.object_mask_fn is None and t.object_masks(images) is None
        assert t._mask_kwargs(t.object_masks(images)) == {}


class MaskRecordingModel(mc.ToyStepModel):
    """ToyStepModel that records the object_mask keyword of every step call."""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.seen = []

    def forward_step1(self, images, latents, collected, **kw):
        self.seen.append((1, "object_mask" in kw, kw.get("object_mask")))
        return super().forward_step1(images, latents, collected, **kw)

    def forward_step2(self, image, latent, collected, n_proj_samples=8, **kw):
        self.seen.append((2, "object_mask" in kw, kw.get("object_mask")))
        return super().forward_step2(image, latent, collected, n_proj_samples=n_proj_samples, **kw)

    def forward_step3(self, image, latent, collected, **kw):
        self.seen.append((3, "object_mask" in kw, kw.get("object_mask")))
        return super().forward_step3(image, latent, collected, **kw)


def _content_mask(images):
    """A mask that tells the images apart: constant, at the image's own mean."""
    return images.mean((1, 2, 3)).view(-1, 1, 1, 1).expand(-1, 1, *images.shape[-2:]).clone()


def test_fit_computes_the_mask_once_per_image_and_hands_it_to_every_step():
    from gan2shape_amd.trainer import Trainer
    calls = []

    def fn(images):
        calls.append(len(images))
        return _content_mask(images)
    data = mc.toy_dataset(2)
    t = Trainer(MaskRecordingModel, dict(mc.TOY_CFG, object_mask=True), debug=True, device="cpu", object_mask_fn=fn)
    n = t.fit(data, stages=mc.TOY_STAGES)
    assert calls == [1, 1]                                  # once per image, next to the prior pre-training
    assert len(t.model.seen) == n
    per_image = n // 2
    for i, (_kind, has, mask) in enumerate(t.model.seen):
        image = data[i // per_image][0]
        assert has and tuple(mask.shape) == (1, 1, 8, 8) and torch.allclose(mask, image.mean().expand_as(mask))
    # switch off: the keyword is never passed
    t = Trainer(MaskRecordingModel, dict(mc.TOY_CFG), debug=True, device="cpu", object_mask_fn=fn)
    t.fit(data, stages=mc.TOY_STAGES)
    assert calls == [1, 1] and all(not has for _, has, _ in t.model.seen)


class JointMaskRecordingModel(mc.ToyJointModel):
    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.seen = []

    def forward_step1(self, images, latents, collected, **kw):
        self.seen.append((1, images.clone(), kw.get("object_mask")))
        loss, c = super().forward_step1(images, latents, collected, **kw)
        # what GAN2Shape.forward_step1 hands on with the masks live: one (1,1,S,S) canonical mask per sample
        om = kw["object_mask"]
        canon = om * 2 if len(images) == 1 else list((om * 2).split(1))
        return loss, c[:5] + (canon,)

    def forward_step2(self, image, latent, collected, n_proj_samples=8, **kw):
        self.seen.append((2, image.clone(), kw.get("object_mask"), collected[5]))
        return super().forward_step2(image, latent, collected[:5] + (None,), n_proj_samples=n_proj_samples, **kw)

    def forward_step3(self, image, latent, collected, **kw):
        self.seen.append((3, image.clone(), kw.get("object_mask")))
        return super().forward_step3(image, latent, collected, **kw)


def test_joint_trainer_slices_the_masks_per_sample():
    from gan2shape_amd.trainer import GeneralizingTrainer2
    calls = []

    def fn(images):
        calls.append(len(images))
        return _content_mask(images)
    cfg = dict(mc.TOY_JOINT_CFG, object_mask=True, n_epochs_generalized=1)
    t = GeneralizingTrainer2(JointMaskRecordingModel, cfg, device="cpu", object_mask_fn=fn)
    t.prior_generator = lambda image, device="cpu": mc.toy_prior(image)
    t.fit(mc.toy_dataset(2), stages=mc.TOY_JOINT_STAGES, batch_size=2)
    assert calls == [2]                                     # once per batch
    seen = t.model.seen
    assert {s[0] for s in seen} == {1, 2, 3}
    for s in seen:
        kind, images, mask = s[0], s[1], s[2]
        B = len(images)
        assert B == (2 if kind == 1 else 1) and tuple(mask.shape) == (B, 1, 8, 8)
        assert torch.allclose(mask, _content_mask(images))              # the batch's masks, or this sample's own
        if kind == 2:                                                   # and step 1's canonical mask of this sample
            assert tuple(s[3].shape) == (1, 1, 8, 8) and torch.allclose(s[3], 2 * _content_mask(images))
