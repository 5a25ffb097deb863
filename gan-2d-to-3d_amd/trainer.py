"""Instance-wise training loop: mirror of GAN2Shape/trainer.py:13-171 (`Trainer`).

Same constructor and `fit` signature, so `Trainer(model=GAN2Shape, model_config=cfg, ...)` works as
in the reference's main.py:130-153: per image, optional prior pre-training of the depth net, then
stages x steps {1,2,3} x N iterations of zero_grad / forward_stepK / backward / Adam.step, with the
last `collected` of step K handed to step K+1.  Three persistent Adam optimisers over {A}, {E},
{L,V,D,A} (lr 1e-4, classic L2 weight decay 5e-4), a fresh Adam for every image's prior
pre-training (trainer.py:40-48,131,163-171).  The iteration itself is stated once, in graphs.EagerSteps; both
trainers run every per-image block of it through a runner's `run_block(kind, n)`, eagerly or as replayed HIP graphs.

Added (not in the reference): `rank` / `world_size` image sharding — rank r trains images
r, r+W, r+2W, ... with no collective (the per-image optimisation is independent; note that nets
are carried from image to image, so a shard equals the reference run on that rank's subset).
Plotting / wandb hooks are out of scope.
"""
import logging
import os

import torch
from torch.utils.data import DataLoader, Subset

from . import zeropool
from .graphs import EagerJointSteps, EagerSteps, GraphedJointSteps, GraphedSteps
from .priors import PriorGenerator
from .sharding import shard_indices  # noqa: F401  (re-exported)

_NO_MASK_SOURCE = ("object_mask is on but there is no source of object masks: set `parsing_ckpt_dir` to the directory of "
                   "the parsing checkpoints, or pass object_mask_fn= (or masking_model=) to the trainer")


def object_masks_live(config):
    """Whether the steps carry an object mask: config `object_mask` (default False) AND `use_mask` (default True), as
    model.GAN2Shape.masks_live."""
    return bool(config.get('object_mask', False)) and bool(config.get('use_mask', True))


class Trainer():
    def __init__(self, model, model_config, debug=False, plot_intermediate=False, log_wandb=False,
                 save_ckpts=False, load_dict=None, masking_model=None, device="cuda",
                 capturable=False, object_mask_fn=None):
        # object masks inside the steps (model.GAN2Shape.object_mask): live when config `object_mask` and `use_mask`
        # are both on; fixed for the trainer's lifetime.  Without a source of masks nothing is built.
        self.object_mask = object_masks_live(model_config)
        ckpt_dir = model_config.get('parsing_ckpt_dir')
        if self.object_mask and object_mask_fn is None and masking_model is None and not (ckpt_dir and os.path.isdir(ckpt_dir)):
            raise ValueError(_NO_MASK_SOURCE)
        try:
            self.model = model(model_config, debug, device=device)
        except TypeError:  # a model class with the reference's exact (config, debug) signature
            self.model = model(model_config, debug)
        self.device = torch.device(device)
        self.image_size = model_config.get('image_size')
        self.category = model_config.get('category')
        self.n_proj_samples = model_config.get('n_proj_samples', 8)
        self.n_epochs_prior = model_config.get('n_epochs_prior', 1000)
        self.n_workers = model_config.get('n_workers', 0)
        self.learning_rate = model_config.get('learning_rate', 1e-4)
        self.save_ckpts = save_ckpts
        self.debug = debug
        self.capturable = capturable  # Adam(capturable=True): needed to record steps in HIP graphs
        # symmetry flips (model.GAN2Shape.flip1 / flip3): one bool per stage; a missing key is all False, a list
        # shorter than the stages repeats its last entry
        self.flip1_cfg = Trainer._flip_list(model_config.get('flip1_cfg'))
        self.flip3_cfg = Trainer._flip_list(model_config.get('flip3_cfg'))
        # projected-sample bank (bank.py): `collect_iters` (absent or 0: off) step-2 iterations of every block are kept
        # on the device and every step-3 iteration draws `step3_batch` of their samples; refused here if too large
        self.collect_iters = int(model_config.get('collect_iters') or 0)
        self.step3_batch = int(model_config.get('step3_batch') or self.n_proj_samples)
        self.bank = None
        if self.collect_iters > 0:
            from .bank import DEFAULT_MAX_BYTES, SampleBank, check_bank_size
            check_bank_size(self.collect_iters, self.n_proj_samples, self.image_size,
                            int(model_config.get('bank_max_bytes', DEFAULT_MAX_BYTES)))
            self.bank = SampleBank(self.collect_iters, self.n_proj_samples, self.image_size, self.device)
        self._bank_left = 0
        prior_name = model_config.get('prior_name', 'ellipsoid')
        mask_accepts_batch = False
        want_parser_mask = self.object_mask and object_mask_fn is None
        parser = None
        if (masking_model is None or want_parser_mask) and model_config.get('parsing_ckpt_dir'):
            # config `parsing_ckpt_dir` names an existing directory: the parsing net of the category (parsing.py)
            # supplies the masks, batched; otherwise the synthetic mask stays
            from .parsing import masking_model_from_config
            parser = masking_model_from_config(model_config, device=self.device)
        # the source of the object masks: the argument, else the parsing net's image_mask, else `masking_model`
        self.object_mask_fn, self._object_mask_batched = None, True
        if self.object_mask:
            if object_mask_fn is not None:
                self.object_mask_fn = object_mask_fn
            elif parser is not None:
                self.object_mask_fn = parser.image_mask
            elif masking_model is not None:
                self.object_mask_fn, self._object_mask_batched = masking_model, False    # one image per call
            else:
                raise ValueError(_NO_MASK_SOURCE)
        if masking_model is None and parser is not None:
            masking_model = parser.confidence_mask if 'confidence' in prior_name else parser.image_mask
            mask_accepts_batch = True
        self.prior_generator = PriorGenerator(self.image_size, self.category, prior_name,
                                              masking_model=masking_model,
                                              on_device=model_config.get('prior_on_device', False),
                                              mask_accepts_batch=mask_accepts_batch)
        self.optim_step1 = Trainer.default_optimizer([self.model.albedo_net], lr=self.learning_rate,
                                                     capturable=capturable)
        self.optim_step2 = Trainer.default_optimizer([self.model.offset_encoder_net],
                                                     lr=self.learning_rate, capturable=capturable)
        self.optim_step3 = Trainer.default_optimizer([self.model.lighting_net,
                                                      self.model.viewpoint_net,
                                                      self.model.depth_net,
                                                      self.model.albedo_net], lr=self.learning_rate,
                                                     capturable=capturable)
        self.load_dict = load_dict
        if load_dict is not None:
            paths, _ = self.model.build_checkpoint_path(load_dict['base_path'],
                                                        load_dict['category'], general=True)
            self.model.load_from_checkpoint(paths[-1])
        self.history = []  # (image index, stage, step, last loss) per finished step block

    @staticmethod
    def _flip_list(value):
        if value is None:
            return []
        return [bool(v) for v in value] if isinstance(value, (list, tuple)) else [bool(value)]

    def object_masks(self, images):
        """The object masks of `images` (B,3,S,S) from the trainer's source -> (B,1,S,S) float32 on the device, no
        gradient; None when the masks are off.  Computed eagerly, once per image (fit) or per batch (the joint loop)."""
        if not self.object_mask:
            return None
        with torch.no_grad():
            fn = self.object_mask_fn
            if self._object_mask_batched or len(images) == 1:
                masks = torch.as_tensor(fn(images))
            else:
                masks = torch.cat([torch.as_tensor(fn(images[i:i + 1])).reshape(1, 1, *images.shape[-2:])
                                   for i in range(len(images))], 0)
            masks = masks.to(device=self.device, dtype=torch.float32).reshape(len(images), 1, *images.shape[-2:])
        return masks.detach().contiguous()

    def _mask_kwargs(self, masks):
        """The extra keyword of a step call: object_mask= when the masks are live, nothing otherwise (a model class
        with the reference's exact step signatures sees the call it always saw)."""
        return {} if masks is None else {'object_mask': masks}

    def _set_flips(self, stage):
        """model.flip1 / model.flip3 of stage `stage` (flip1_cfg / flip3_cfg)."""
        for name, cfg in (('flip1', self.flip1_cfg), ('flip3', self.flip3_cfg)):
            setattr(self.model, name, cfg[min(stage, len(cfg) - 1)] if cfg else False)

    # ---- the projected-sample bank (None when `collect_iters` is off: every method below is then never reached)
    def _bank_begin(self, n):
        """A step-2 block of n iterations starts: the encoder has been re-trained since the last one, so what the
        bank holds is stale."""
        self.bank.reset()
        self._bank_left = n

    def _bank_collect(self, collected):
        """After a step-2 iteration: keep its samples if it is one of the block's last `collect_iters`."""
        self._bank_left -= 1
        if self._bank_left < self.collect_iters:
            self.bank.put(collected[0].detach(), collected[1].detach())

    def _bank_draw(self, image):
        """The hand-off of one step-3 iteration: `step3_batch` samples drawn from the bank (one randperm on the CPU
        generator), gathered with the image in front."""
        return self.bank.gather(self.bank.indices(self.step3_batch), image)

    def _bank_hooks(self, steps):
        """Wire the bank into a runner (graphs.EagerSteps.after / before / source): step 2's hand-off goes into the bank
        after every iteration that collects, and in front of every step-3 iteration a draw and one gather make what it
        reads — a fresh hand-off for an eager runner (all rows of a bank that holds fewer than `step3_batch`; nothing
        of an empty one), the fill of static buffers for a graphed one."""
        steps.after[2] = self._bank_collect
        if isinstance(steps, GraphedSteps):
            from .bank import StaticHandOff
            static = StaticHandOff(self.bank, self.step3_batch, steps.image)
            steps.before[3] = static.fill
            steps.source[3] = static.handoff
        else:
            def draw(replay):
                steps.source[3] = self._bank_draw(steps.image) if len(self.bank) > 0 else None
            steps.before[3] = draw

    def fit(self, images_latents, plot_depth_map=False,
            stages=[{'step1': 1, 'step2': 1, 'step3': 1}] * 2, shuffle=False,
            rank=0, world_size=1, graphs=False, on_image_done=None, **_):
        """graphs=True replays each step kind as a HIP graph (graphs.py): same iterations, same
        order; needs Trainer(..., capturable=True) and a non-default current stream.
        on_image_done(data_index, image, trainer): called after the last stage of each image, before its checkpoint."""
        if graphs and not self.capturable:
            raise RuntimeError("graphs=True needs Trainer(..., capturable=True)")
        total_it = 0
        data = images_latents
        if world_size > 1:
            data = Subset(images_latents, shard_indices(len(images_latents), rank, world_size))
        # the original training is instance-based => batch size = 1
        dataloader = DataLoader(data, batch_size=1, shuffle=shuffle, num_workers=self.n_workers)
        steps = None
        for image, latent, data_index in dataloader:
            image, latent = image.to(self.device), latent.to(self.device)
            data_index = int(data_index[0])
            logging.info(f'Training on image {data_index}')
            if not self.debug and self.load_dict is None:
                self.pretrain_on_prior(image, data_index, plot_depth_map)
            masks = self.object_masks(image)       # once per image, eagerly: outside any capture
            if steps is None:
                steps = (GraphedSteps if graphs else EagerSteps)(self, image, latent, object_mask=masks)
                if self.bank is not None:
                    self._bank_hooks(steps)
            else:
                steps.set_sample(image, latent, masks)   # graphs read the static image / latent / mask buffers
            stage = -1 if graphs else 0     # the stage an empty schedule's checkpoint is named after
            for stage in range(len(stages)):
                self._set_flips(stage)      # a captured step depends on its flip switch: graphs are keyed by (kind, flip)
                if not graphs:      # an eager hand-off does not outlive its stage; a graph keeps reading its static buffers
                    steps.collected = {1: None, 2: None, 3: None}
                for step in [1, 2, 3]:
                    n = stages[stage][f'step{step}']
                    if self.bank is not None and step == 2:
                        self._bank_begin(n)
                    total_it += steps.run_block(step, n)
                    if n > 0 or not graphs:     # the eager loop keeps a row for an empty block
                        self.history.append((data_index, stage, step, float(steps.loss[step]) if n > 0 else None))
            if on_image_done is not None:
                on_image_done(data_index, image, self)
            if self.save_ckpts:
                self.model.save_checkpoint(data_index, stage, total_it, self.category)
        logging.info('Finished Training')
        return total_it

    def pretrain_on_prior(self, image, i_batch, plot_depth_map=False):
        """trainer.py:130-161: n_epochs_prior Adam steps of mse(depth, prior) on a fresh optimiser."""
        optim = Trainer.default_optimizer([self.model.depth_net])
        prior = self.prior_generator(image, device=self.device)
        losses = []
        for _ in range(self.n_epochs_prior):
            optim.zero_grad()
            loss, depth = self.model.depth_net_forward(image, prior)
            loss.backward()
            optim.step()
            losses.append(loss.detach())
        return [float(v) for v in torch.stack(losses).cpu()] if losses else []

    def _sync_and_step(self, optim):
        """optim.step(), preceded under data parallelism by ONE flat-bucket gradient all-reduce
        (mean) over the parameters this optimiser owns (sharding.allreduce_mean_gradients)."""
        from .sharding import allreduce_mean_gradients
        allreduce_mean_gradients([p for g in optim.param_groups for p in g['params']])
        optim.step()
        zeropool.end()

    @staticmethod
    def default_optimizer(model_list, lr=1e-4, betas=(0.9, 0.999), weight_decay=5e-4,
                          capturable=False):
        param_list = []
        for model in model_list:
            param_list += [p for p in model.parameters() if p.requires_grad]
        # GPU: the whole step as one launch of libg2s (optim.Adam on g2s_adam_step: same update rule,
        # trainer.py:163-171; device-side step counter, so it can be recorded in HIP graphs)
        if param_list and all(p.is_cuda for p in param_list):
            from gan2shape_amd.optim import Adam
            return Adam(param_list, lr=lr, betas=betas, weight_decay=weight_decay)
        return torch.optim.Adam(param_list, lr=lr, betas=betas, weight_decay=weight_decay, capturable=capturable)


class GeneralizingTrainer2(Trainer):
    """Joint training over a set of images (trainer.py:338-479, on GeneralizingTrainer :174-335):
    pre-train the depth net on every image's prior, then per epoch and per batch of images run
    step 1 on the batch and steps 2 / 3 image by image — one shared model.

    Data parallelism (added; the reference is single-process): with world_size W every batch of
    `batch_size` images is dealt round-robin to the ranks (batch_size must be a multiple of W), each
    rank runs the reference's iteration on its images, and every optimiser step is preceded by one
    flat-bucket gradient all-reduce (mean) over RCCL (`sharding.allreduce_mean_gradients`: step 1
    A, step 2 E, step 3 L+V+D+A).  Where the reference centres the depth over the whole image
    batch — prior pre-training (model.py:90) and the batched step 1 (model.py:338) —
    `get_clamped_depth` / `depth_net_forward` use the mean over ALL ranks' images
    (`sharding.global_mean`); steps 2 / 3 run image by image in the reference (trainer.py:436-452),
    so their inner step-1 pass centres each image by its own mean, on every rank as at W = 1.
    W = 1 is the reference's loop exactly.  W > 1 equals it up to the reference's own `b = 1`
    slicing in forward_step1 (model.py:96,150: only the first reconstruction of a call enters the
    losses), which then applies per rank."""

    def __init__(self, model, model_config, **kwargs):
        super().__init__(model, model_config, **kwargs)
        self.n_epochs = model_config.get('n_epochs_generalized', 1)

    def _local_batches(self, images_latents, batch_size, shuffle, rank, world_size):
        if batch_size % world_size:
            raise ValueError(f"batch_size {batch_size} must be a multiple of world_size {world_size}")
        loader = DataLoader(images_latents, batch_size=batch_size, shuffle=shuffle,
                            num_workers=self.n_workers)
        for images, latents, indices in loader:
            if len(images) % world_size:
                raise ValueError(f"{len(images_latents)} images do not fill batches of {batch_size} "
                                 f"evenly over {world_size} ranks")
            sel = slice(rank, None, world_size)
            yield images[sel].to(self.device), latents[sel].to(self.device), [int(i) for i in indices[sel]]

    def fit(self, images_latents, plot_depth_map=False,
            stages=[{'step1': 1, 'step2': 1, 'step3': 1}] * 2, batch_size=2, shuffle=False,
            rank=0, world_size=1, graphs=False, on_image_done=None, **_):
        """graphs=True: the per-image steps 2 / 3 replay as HIP graphs in two segments with the gradient
        all-reduce between them (graphs.GraphedJointSteps; needs capturable=True and a non-default current
        stream), graphs=False runs the same blocks through graphs.EagerJointSteps; the batched step 1 stays eager
        (ragged batches, and under W > 1 a collective in its forward).
        on_image_done(data_index, image, trainer): called once per image of this rank, in dataset order, after the
        last epoch (the model is shared: only then is an image's result final)."""
        from . import sharding
        # centre of the depth over the WHOLE image batch (all ranks) — only where the reference
        # itself runs a batch of images through the depth net: prior pre-training and step 1
        whole_batch = sharding.global_mean if world_size > 1 else None
        total_it = 0
        steps = None
        if graphs and not self.capturable:
            raise RuntimeError("graphs=True needs GeneralizingTrainer2(..., capturable=True)")
        self._set_flips(0)      # entry 0 of flip1_cfg / flip3_cfg, as stages[0] below
        try:
            if self.load_dict is None:
                self.model.batch_mean = whole_batch
                self.pretrain_on_prior_all(images_latents, batch_size, rank, world_size)
            for epoch in range(self.n_epochs):
                for images, latents, indices in self._local_batches(images_latents, batch_size, shuffle,
                                                                    rank, world_size):
                    loss = collected = None
                    self.model.batch_mean = whole_batch
                    masks = self.object_masks(images)       # once per batch
                    for _ in range(stages[0]['step1']):
                        self.optim_step1.zero_grad()
                        loss, collected = self.model.forward_step1(images, latents, None, **self._mask_kwargs(masks))
                        loss.backward()
                        self._sync_and_step(self.optim_step1)
                        total_it += 1
                    self.model.batch_mean = None   # steps 2 / 3: one image at a time, its own mean
                    self.history.append((tuple(indices), epoch, 1, None if loss is None else float(loss.detach())))
                    if collected is None:
                        continue
                    normals, lights_a, lights_b, albedos, depths, canon_masks = collected
                    if not isinstance(canon_masks, list):
                        canon_masks = [canon_masks]
                    for bi, index in enumerate(indices):
                        image, latent = images[bi:bi + 1], latents[bi:bi + 1]
                        mask = None if masks is None else masks[bi:bi + 1]      # this sample's mask
                        step1_collected = (normals[bi:bi + 1].detach(), lights_a[bi:bi + 1].detach(),
                                           lights_b[bi:bi + 1].detach(), albedos[bi:bi + 1].detach(),
                                           depths[bi:bi + 1].detach(), canon_masks[bi])
                        if steps is None:
                            steps = (GraphedJointSteps if graphs else EagerJointSteps)(self, image, latent, object_mask=mask)
                            if self.bank is not None:
                                self._bank_hooks(steps)
                        else:
                            steps.set_sample(image, latent, mask)
                        steps.set_source(2, step1_collected)
                        n2 = stages[0]['step2']
                        n3 = stages[0]['step3'] if n2 > 0 else 0        # no step-2 hand-off, no step 3
                        for step, n in ((2, n2), (3, n3)):
                            if self.bank is not None and step == 2:     # one bank serves all images: emptied for each
                                self._bank_begin(n)
                            total_it += steps.run_block(step, n)
                        # both rows always, read back (a synchronisation) once both blocks are queued
                        self.history += [(index, epoch, step, float(steps.loss[step]) if n > 0 else None)
                                         for step, n in ((2, n2), (3, n3))]
                if epoch % 20 == 0 and self.save_ckpts and rank == 0:
                    self.model.save_checkpoint("", epoch, total_it, self.category)
            if on_image_done is not None:      # read straight from the dataset: a DataLoader would draw a seed
                for k in range(len(images_latents)):
                    image, _latent, index = images_latents[k]
                    if world_size == 1 or (int(index) % batch_size) % world_size == rank % world_size:
                        on_image_done(int(index), image.unsqueeze(0).to(self.device), self)
        finally:
            self.model.batch_mean = None
        logging.info('Finished Training')
        return total_it

    def pretrain_on_prior_all(self, images_latents, batch_size, rank=0, world_size=1):
        """GeneralizingTrainer.pretrain_on_prior (trainer.py:296-335): one prior per image, then
        n_epochs_prior passes over the batches with a fresh Adam on the depth net."""
        optim = Trainer.default_optimizer([self.model.depth_net])
        priors = {}
        if getattr(self.prior_generator, 'on_device', False):
            # config `prior_on_device`: this rank's priors through the batched kernels, batch_size images per set of
            # launches
            mine = []
            for k in range(len(images_latents)):
                image, _, index = images_latents[k]
                if (int(index) % batch_size) % world_size == rank % world_size or world_size == 1:
                    mine.append((int(index), image))
            for at in range(0, len(mine), batch_size):
                chunk = mine[at:at + batch_size]
                images = torch.stack([image for _, image in chunk]).to(self.device)
                for (index, _), prior in zip(chunk, self.prior_generator.batch(images, device=self.device)):
                    priors[index] = prior[None]
        else:
            for image, _, index in DataLoader(images_latents, batch_size=1, shuffle=False):
                if (int(index[0]) % batch_size) % world_size == rank % world_size or world_size == 1:
                    priors[int(index[0])] = self.prior_generator(image.to(self.device), device=self.device)
        loss = None
        for _ in range(self.n_epochs_prior):
            for images, _latents, indices in self._local_batches(images_latents, batch_size, False,
                                                                 rank, world_size):
                for i in indices:
                    if i not in priors:
                        item = images_latents[i]
                        priors[i] = self.prior_generator(item[0].unsqueeze(0).to(self.device), device=self.device)
                prior = torch.stack([priors[i].reshape(self.image_size, self.image_size) for i in indices])
                optim.zero_grad()
                loss, _depth = self.model.depth_net_forward(images, prior)
                loss.backward()
                self._sync_and_step(optim)
        return None if loss is None else float(loss.detach())
