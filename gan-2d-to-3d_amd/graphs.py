"""The training iteration and its two ways of running: eagerly (EagerSteps) and as a replayed HIP graph (GraphedSteps).

One GAN2Shape iteration is zero_grad, forward_stepK, backward, Adam.step (trainer.py:99-109), with the `collected` of
step K handed to step K+1.  EagerSteps states it once, for one sample, and runs blocks of it; both trainers drive every
per-image block through `run_block(kind, n)` of one of four runners:

    EagerSteps          Trainer.fit                       launches every kernel from Python
    EagerJointSteps     GeneralizingTrainer2.fit          the same, the optimiser step behind the gradient all-reduce
    GraphedSteps        Trainer.fit(graphs=True)          captures each step kind once, then replays it
    GraphedJointSteps   GeneralizingTrainer2.fit(graphs=True)   two captured segments around the collective

Hooks (the projected-sample bank: trainer._bank_hooks; all empty otherwise), each keyed by step kind and run eagerly on
the current stream around EVERY iteration, warm-up or replay, never captured: before[kind](replay) in front of it,
after[kind](collected) behind it; source[kind] replaces the previous kind's hand-off as what the iteration reads.

Why graphs: an iteration is 1000-1500 small kernel launches; on MI355X the eager loop is host-bound (the GPU is busy
~2/3 of the wall time at batch 1).  Each step kind is therefore captured ONCE into a hipGraph (torch.cuda.CUDAGraph:
kernels of libg2s.so launch on torch's capture stream, so they are recorded like any other op) and replayed per
iteration.  A replay is exactly one iteration of the eager loop: same kernels, same order, same arithmetic; random
draws come from the graph-registered device generator, so successive replays draw fresh samples.

Constraint (PyTorch/HIP): every eager backward of these networks that precedes a capture must have
run on a non-default stream (torch.cuda.set_stream(torch.cuda.Stream()) at program start);
otherwise autograd's AccumulateGrad nodes stay bound to the legacy default stream and the capture
aborts.

Static buffers: `image`, `latent` (set_sample copies a new image in to reuse the graphs), and the `collected`
hand-offs — graph k+1 reads the output tensors of graph k in place.  With the object masks live
(model.GAN2Shape.object_mask; fixed for a trainer's lifetime, so the graph keys do not carry it) a third static
buffer holds the image's object mask: the trainer computes the mask eagerly, outside any capture, and set_sample
copies it in; the captured step 1 (and the inner step-1 pass of step 3) turns it into the canonical mask in place.
An eager runner has no buffers of its own: set_sample and set_source rebind.

Symmetry flips: a captured step 1 / step 3 depends on the model's flip switch (flip1 / flip3: twice the rows
behind the nets), so the graphs are keyed by (kind, flip) and a schedule whose stages differ captures each variant
once.  `loss[kind]` and `collected[kind]` stay the hand-off buffers of the FIRST variant captured for a kind (the
graphs of the next kind read them in place); another variant's outputs are copied into them after its replay.
"""
import torch

from . import zeropool


class EagerSteps:
    """The iterations of one sample, run eagerly: `loss[kind]` (detached) and `collected[kind]` of the latest
    iteration of each kind, the hooks, and blocks of iterations.  Touches no CUDA API of its own."""
    n_proj_kinds = (1, 2, 3)    # the step kinds that are handed n_proj_samples=

    def __init__(self, trainer, image, latent, object_mask=None):
        self.t = trainer
        self.model = trainer.model
        self.image, self.latent, self.object_mask = image, latent, object_mask
        self.loss = {}
        self.collected = {1: None, 2: None, 3: None}
        self.before, self.after, self.source = {}, {}, {}

    def set_sample(self, image, latent, object_mask=None):
        self.image, self.latent, self.object_mask = image, latent, object_mask

    def set_source(self, kind, collected):
        """Hand step `kind` this `collected` (the joint trainer hands every image its own slice of the batched step 1)."""
        self.collected[kind - 1] = collected

    def _step_kwargs(self, kind):
        kw = {'n_proj_samples': self.t.n_proj_samples} if kind in self.n_proj_kinds else {}
        if self.object_mask is not None:
            kw['object_mask'] = self.object_mask
        return kw

    def _source(self, kind):
        if kind in self.source:
            return self.source[kind]
        return {1: None, 2: self.collected[1], 3: self.collected[2]}[kind]

    def _forward_backward(self, kind, src):
        loss, collected = getattr(self.model, f'forward_step{kind}')(self.image, self.latent, src, **self._step_kwargs(kind))
        loss.backward()
        return loss, collected

    def _update(self, kind):
        getattr(self.t, f'optim_step{kind}').step()
        zeropool.end()       # the step's cleared pool serves nothing beyond the step

    def _iteration(self, kind, src):
        loss, collected = self._forward_backward(kind, src)
        self._update(kind)
        return loss, collected

    def _eager(self, kind, **zero_grad):
        """One eager iteration between its hooks -> (loss, collected)."""
        getattr(self.t, f'optim_step{kind}').zero_grad(**zero_grad)
        if kind in self.before:
            self.before[kind](False)
        loss, collected = self._iteration(kind, self._source(kind))
        if kind in self.after:
            self.after[kind](collected)
        return loss, collected

    def run(self, kind):
        """One training iteration of kind `kind`."""
        loss, self.collected[kind] = self._eager(kind)
        self.loss[kind] = loss.detach()
        return self.loss[kind]

    def run_block(self, kind, n):
        """n iterations of kind `kind` -> n."""
        for _ in range(n):
            self.run(kind)
        return n


class EagerJointSteps(EagerSteps):
    """Joint (data-parallel) iterations: the optimiser step follows the gradient all-reduce (trainer._sync_and_step)."""
    n_proj_kinds = (1, 2)       # the joint loop calls step 3 as the reference's does, without the keyword

    def _update(self, kind):
        self.t._sync_and_step(getattr(self.t, f'optim_step{kind}'))


class GraphedSteps(EagerSteps):
    def __init__(self, trainer, image, latent, warmup=3, object_mask=None):
        super().__init__(trainer, image.clone(), latent.clone(), None if object_mask is None else object_mask.detach().clone())
        self.graphs = {}
        self._outputs = {}      # (kind, flip) -> (loss, collected): the static outputs of that captured graph
        self.warmup = warmup
        # With a before hook the CPU generator decides what the step sees, so the graphed loop then consumes it exactly
        # as the eager loop does: `replay` tells the hook that the iteration's own Python (and the CPU draws in it) will
        # not run, and a capture, which runs that Python once without being an iteration, leaves the generator where it
        # was.
        for opt in (trainer.optim_step1, trainer.optim_step2, trainer.optim_step3):
            for group in opt.param_groups:
                if not group.get('capturable', False):
                    raise RuntimeError("GraphedSteps needs Adam(capturable=True): build the trainer "
                                       "with Trainer(..., capturable=True)")

    def key(self, kind):
        """(kind, flip): what a captured iteration of `kind` depends on besides the static buffers."""
        flip = {1: 'flip1', 3: 'flip3'}.get(kind)
        return kind, bool(getattr(self.model, flip, False)) if flip else False

    def captured(self, kind):
        return self.key(kind) in self.graphs

    def _publish(self, kind, loss, collected):
        """Copy a variant's outputs into the kind's hand-off buffers (no-op for the variant that owns them)."""
        with torch.no_grad():
            if loss is not self.loss[kind]:
                self.loss[kind].copy_(loss.detach())
            for dst, srct in zip(self.collected[kind] or (), collected or ()):
                if torch.is_tensor(dst) and dst is not srct:
                    dst.copy_(srct.detach())

    def capture(self, kind, warmup=None):
        """Warm up `warmup` (default: the constructor's) eager iterations on a side stream (library
        handles, lazily built caches), then capture one iteration (recorded, not executed).
        Warm-up iterations are real training iterations; callers that count iterations must count
        them (return value)."""
        warmup = self.warmup if warmup is None else int(warmup)
        if warmup < 1:
            raise ValueError("capture needs at least one eager warm-up iteration")
        optim = getattr(self.t, f'optim_step{kind}')
        src = self._source(kind)
        if kind > 1 and src is None:
            raise RuntimeError(f"capture step {kind - 1} first")
        if torch.cuda.current_stream() == torch.cuda.default_stream():
            # an eager backward on the legacy default stream binds the parameters' AccumulateGrad
            # nodes to it; capturing the same autograd graph afterwards aborts inside
            # hipStreamEndCapture (a host segfault, not an exception)
            raise RuntimeError("GraphedSteps.capture must run with a non-default current stream: call "
                               "torch.cuda.set_stream(torch.cuda.Stream()) before the first backward "
                               "of the networks (see graphs.py)")
        # warm-up (side stream) and capture (capture stream) run backward on different non-default
        # streams than the parameters' AccumulateGrad nodes were created on: expected here
        if hasattr(torch.autograd.graph, "set_warn_on_accumulate_grad_stream_mismatch"):
            torch.autograd.graph.set_warn_on_accumulate_grad_stream_mismatch(False)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(warmup):
                warm_loss, warm_collected = self._eager(kind, set_to_none=True)
        torch.cuda.current_stream().wait_stream(s)
        optim.zero_grad(set_to_none=True)
        key = self.key(kind)
        cpu_rng = torch.get_rng_state() if kind in self.before else None
        self.graphs[key], loss, collected = self._record(kind, src)
        if cpu_rng is not None:
            torch.set_rng_state(cpu_rng)
        self._outputs[key] = (loss.detach(), collected)
        if not any(k[0] == kind for k in self._outputs if k != key):   # the first variant owns the hand-off buffers
            self.loss[kind], self.collected[kind] = self._outputs[key]
        # A capture records, it does not run: the graph's static outputs (the loss, the hand-off
        # to the next step kind) are filled with the results of the last warm-up iteration, so they
        # are valid even if no replay follows (a block that asks for no more than `warmup`
        # iterations).
        self._publish(kind, warm_loss, warm_collected)
        return warmup  # iterations actually executed

    def _record(self, kind, src):
        """Capture one iteration -> (what run() replays, loss, collected)."""
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            loss, collected = self._iteration(kind, src)
        return g, loss, collected

    def run(self, kind):
        """One training iteration of kind `kind` (graph replay)."""
        key = self.key(kind)
        if kind in self.before:
            self.before[kind](True)
        self._replay(kind, key)
        self._publish(kind, *self._outputs[key])
        if kind in self.after:
            self.after[kind](self.collected[kind])
        return self.loss[kind]

    def _replay(self, kind, key):
        self.graphs[key].replay()

    def run_block(self, kind, n):
        """n iterations of kind `kind` -> n: a kind (and flip) not captured yet is, and its warm-up iterations are real
        iterations of the block, never more than it asks for; the rest are replays."""
        done = 0
        if n > 0 and not self.captured(kind):
            if kind > 1 and self.collected[kind - 1] is None:
                raise RuntimeError(f"step {kind} needs at least one step-{kind - 1} iteration first")
            done = self.capture(kind, warmup=min(self.warmup, n))
        for _ in range(n - done):
            self.run(kind)
        return n

    def set_sample(self, image, latent, object_mask=None):
        self.image.copy_(image)
        self.latent.copy_(latent)
        if (object_mask is None) != (self.object_mask is None):
            raise ValueError("the object mask is a static buffer of the captured graphs: give one with every sample, or "
                             "with none")
        if object_mask is not None:
            self.object_mask.copy_(object_mask)


class GraphedJointSteps(GraphedSteps):
    """Joint (data-parallel) training iterations as TWO captured segments with the collective between them:

        segment A   forward_stepK + backward + GradBucket.pack      (the step's gradients -> the flat bucket)
        eager       ONE all-reduce (mean) of the bucket over RCCL   (skipped by a single process)
        segment B   optimiser step reading the bucket's views       (GradBucket.bind: nothing is copied back)

    Every address is fixed (the bucket is persistent, the gradients of segment A live in the graph's pool), so
    a replayed iteration is  A.replay(); all_reduce(bucket); B.replay().  The forward itself must hold no
    collective: steps 2 / 3 always qualify (one image at a time, centred by its own mean at any W —
    GeneralizingTrainer2); step 1 qualifies when the depth centre is local (`model.batch_mean is None`: a
    single process, or one image per rank WITHOUT the whole-batch centre) and is refused otherwise — the
    trainer then runs it eagerly (sharding.global_mean is a differentiable all-reduce inside the forward)."""

    def __init__(self, trainer, image, latent, warmup=3, object_mask=None):
        super().__init__(trainer, image, latent, warmup, object_mask)
        from .sharding import bucket_of
        self.buckets = {k: bucket_of([p for g in getattr(trainer, f'optim_step{k}').param_groups for p in g['params']])
                        for k in (1, 2, 3)}
        self._static_src = {}

    def _forward_backward(self, kind, src):
        if kind == 1 and self.model.batch_mean is not None:
            raise RuntimeError("GraphedJointSteps: step 1 with a whole-batch depth centre holds a collective in its forward; run it eagerly")
        loss, collected = super()._forward_backward(kind, src)
        self.buckets[kind].pack()
        return loss, collected

    def _update(self, kind, reduce=True):
        if reduce:
            self.buckets[kind].all_reduce_mean()
        self.buckets[kind].bind()
        super()._update(kind)

    def _record(self, kind, src):
        a, b = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
        with torch.cuda.graph(a):
            loss, collected = self._forward_backward(kind, src)
        with torch.cuda.graph(b, pool=a.pool()):
            self._update(kind, reduce=False)
        return (a, b), loss, collected

    def _replay(self, kind, key):
        a, b = self.graphs[key]
        a.replay()
        self.buckets[kind].all_reduce_mean()
        b.replay()

    def set_source(self, kind, collected):
        """Copy a hand-off into the static tensors the captured graph of step `kind` reads."""
        cur = self._static_src.get(kind)
        if cur is None:
            self._static_src[kind] = cur = tuple(t.detach().clone() if torch.is_tensor(t) else t for t in collected)
            self.collected[kind - 1] = cur
            return
        with torch.no_grad():
            for dst, srct in zip(cur, collected):
                if torch.is_tensor(dst):
                    dst.copy_(srct)
