"""The Pix2Pix model family with the reference's class surface (pix2pix_model.py:11-325) on the MI355X engine.

    Pix2PixModel(train_ds, test_ds, model_name, architecture_name, lambda_l1)
    Pix2PixAugmentedModel(same)                  -- augmentation lives in the dataset (pix2pix_model.py:232-234)
    Pix2PixHistogramModel(..., lambda_l1, lambda_histogram)
    Pix2PixIndexedModel(train_ds, test_ds, model_name, architecture_name, lambda_segmentation=0.5)
    Pix2PixPaletteModel(..., lambda_l1, lambda_palette, lambda_conformance=0.0, temperature=1e-3)      -- build-added
    Pix2PixDiffAugmentModel(..., lambda_l1, policy="color,translation,cutout")                         -- build-added
    Pix2PixPaletteSnapModel(..., lambda_l1, hard=True, gradient="identity", temperature=5e-2)          -- build-added
    Pix2PixIndexedColourModel(..., lambda_segmentation=0.5, lambda_colour=100.0, lambda_histogram=0.0, hard=False, blacken=True)  -- build-added

The constructor follows the reference's (pix2pix_model.py:12-36): create_generator() / create_discriminator() with the
reference's builder signatures, `loss_object`, two Adam(0.0002, beta_1=0.5) optimizers, `checkpoint`,
`checkpoint_manager`.  train_step(batch, step, update_steps) keeps the reference's contract (one optimisation step of
both networks with gradients taken at the same pre-update weights, scalars logged at step // update_steps) and
additionally RETURNS (g_loss_tuple, d_loss_tuple) as device scalars, and tolerates summary_writer=None.

The step is FUSED: generator_loss / discriminator_loss of the classes below are evaluated by the HIP kernels inside
engine.train_step_* together with their gradients (there is no autograd tape here).  The methods exist with the
reference's signatures for standalone evaluation.  A SUBCLASS that overrides one of them cannot change the fused step:
train_step detects the override and runs the hooked step instead (hooks under torch autograd, gradients into the backward
kernels); the palette-index model takes that path only when the subclass sets `differentiable_loss_hooks = True`, and raises
otherwise instead of silently ignoring the override.
Extra keyword arguments (dtype, img_size, device, data_parallel, seed, ema_decay, ema_warmup, generator_optimizer,
discriminator_optimizer) are build-added; defaults reproduce the reference.

Optimizers (build-added): generator_optimizer= / discriminator_optimizer= (or an overridden create_optimizers())
replace the reference's two Adam(0.0002, beta_1=0.5); each may have its own rate or learning-rate schedule, betas, epsilon,
clipvalue or global_clipnorm, and its attributes stay live after construction.

Averaged generator (build-added): with `ema_decay` (e.g. 0.999) the engine keeps an exponential moving average
of the generator's weights, updated inside the Adam launch of every step.  Training is unchanged; generate(), the previews,
report_l1 / report_fid / report_palette and save_generator() then use the averaged generator (`averaged=False` asks for the live
one), and checkpoints carry the average.  With ema_decay=None (default) nothing changes and `averaged=True` raises ValueError.

Data parallelism (build-added): with `data_parallel`, every rank agrees on the same GLOBAL batch (same
dataset seed, same order) and works on its contiguous shard (parallel.shard_bounds).  The sprite datasets of dataset_utils
are told their shard (set_shard) and MATERIALISE ONLY THAT SHARE of every batch (dataset_utils.ShardedBatch carries the global
batch size and the shard's offset); any other batch source is taken as the whole global batch and sliced here.  Loss
denominators use the global batch, the dropout stream is keyed by the global sample index, gradients are summed over ranks.
Ragged global batches and ranks with an empty shard are handled.
"""
import torch

from . import _lib as L
from . import diffaugment as _diffaugment
from . import histogram as _histogram  # noqa: F401  (module parity with the reference's `import histogram`)
from . import palette as _palette
from .configuration import IMG_SIZE, MAX_PALETTE_SIZE
from .engine import Pix2PixEngine
from .networks import PatchDiscriminator, UnetGenerator
from .dataset_utils import ShardedBatch
from .parallel import shard_bounds
from .side2side_model import Checkpoint, CheckpointManager, S2SModel


class BinaryCrossentropy:
    """tf.keras.losses.BinaryCrossentropy(from_logits=True) (pix2pix_model.py:19) for standalone evaluation: mean over all
    elements of max(x,0) - x*z + log1p(exp(-|x|))."""

    def __init__(self, from_logits=True):
        if not from_logits:
            raise NotImplementedError("the reference only uses from_logits=True")

    def __call__(self, y_true, y_pred):
        x = torch.as_tensor(y_pred, dtype=torch.float32)
        z = torch.as_tensor(y_true, dtype=torch.float32).to(x.device)
        return torch.nn.functional.binary_cross_entropy_with_logits(x, z)


class CategoricalCrossentropy:
    """tf.keras.losses.CategoricalCrossentropy(from_logits=False) (pix2pix_model.py:265) for standalone evaluation.
    Keras 2.9 evaluates it on the logits cached by the softmax activation (softmax_cross_entropy_with_logits) -- that is what
    train_step's fused kernel computes (log-sum-exp form, csrc/softmax.hip) and what `logits=` selects here.  As in Keras, a
    y_pred that carries the cached logits as `y_pred._keras_logits` (the probabilities the indexed model's hooked train step hands
    its generator_loss) is evaluated on them; a tensor derived from it loses the attribute.  Handed probabilities alone, Keras'
    documented fallback applies: p /= sum p; p = clip(p, 1e-7, 1 - 1e-7); mean of -sum t log p.
    The two agree to < 1e-6 unless a target probability is below 1e-7, where the fallback is capped at -log 1e-7 = 16.1 per
    pixel and the logits form is not."""

    def __call__(self, y_true, y_pred, logits=None):
        if logits is None:
            logits = getattr(y_pred, "_keras_logits", None)
        if logits is not None:
            z = torch.as_tensor(logits, dtype=torch.float32)
            t = torch.as_tensor(y_true, dtype=torch.float32).to(z.device)
            return -(t * torch.log_softmax(z, dim=-1)).sum(-1).mean()
        p = torch.as_tensor(y_pred, dtype=torch.float32)
        t = torch.as_tensor(y_true, dtype=torch.float32).to(p.device)
        p = p / p.sum(-1, keepdim=True)
        p = p.clamp(1e-7, 1.0 - 1e-7)
        return -(t * p.log()).sum(-1).mean()


class Adam:
    """tf.keras.optimizers.Adam(learning_rate, beta_1) as the reference constructs it (pix2pix_model.py:28-29): the
    hyper-parameters live here, the moments and the step count in the engine's flat buffers (engine.ParamStore).

    Options, each optimizer its own:
      learning_rate    a float or a schedule of palette_and_histo_gan_amd.schedules (tf_compat.tf.keras.optimizers.schedules.*),
                       evaluated on the device from `iterations`
      clipvalue        every gradient element is clamped to [-clipvalue, clipvalue]
      global_clipnorm  the network's whole gradient is scaled by global_clipnorm / ||g||_2 where the norm exceeds it
                       (tf.clip_by_global_norm); `last_global_norm` is the norm of the last step, a device scalar
    Once a model has bound the optimizer, assigning learning_rate / beta_1 / beta_2 / epsilon / clipvalue / global_clipnorm writes
    through to the engine and holds from the next step on.  Per-variable `clipnorm`, `weight_decay` and `amsgrad` are not built."""

    _SETTINGS = ("learning_rate", "beta_1", "beta_2", "epsilon", "clipvalue", "global_clipnorm")

    def __init__(self, learning_rate=0.001, beta_1=0.9, beta_2=0.999, epsilon=1e-7, clipvalue=None, global_clipnorm=None, **kwargs):
        from .schedules import as_schedule
        supported = "supported: learning_rate (float or schedule), beta_1, beta_2, epsilon, clipvalue, global_clipnorm"
        for name in ("clipnorm", "weight_decay", "amsgrad"):
            if kwargs.pop(name, None):
                raise NotImplementedError(f"Adam({name}=...) is not built; {supported}")
        if kwargs:
            raise TypeError(f"Adam got unexpected keyword arguments {sorted(kwargs)}; {supported}")
        for name, v in (("clipvalue", clipvalue), ("global_clipnorm", global_clipnorm)):
            if v is not None and not float(v) > 0:
                raise ValueError(f"{name} must be positive, got {v}")
        if clipvalue is not None and global_clipnorm is not None:
            raise ValueError("clipvalue and global_clipnorm together: Keras versions disagree on their order; set one")
        as_schedule(learning_rate)
        self._store = self._engine = None
        self._values = dict(zip(self._SETTINGS, (learning_rate, beta_1, beta_2, epsilon, clipvalue, global_clipnorm)))

    def _setting(name):
        def get(self):
            return self._values[name]

        def put(self, v):
            old = self._values[name]
            self._values[name] = v
            try:
                self._push(name)
            except Exception:
                self._values[name] = old
                raise
        return property(get, put)

    learning_rate, beta_1, beta_2 = _setting("learning_rate"), _setting("beta_1"), _setting("beta_2")
    epsilon, clipvalue, global_clipnorm = _setting("epsilon"), _setting("clipvalue"), _setting("global_clipnorm")
    del _setting

    def _push(self, name=None):
        """writes one setting (None: all) into the engine's slots of this optimizer's network"""
        eng, store, v = self._engine, self._store, self._values
        if store is None:
            if name in ("clipvalue", "global_clipnorm") and v["clipvalue"] is not None and v["global_clipnorm"] is not None:
                raise ValueError("clipvalue and global_clipnorm together: Keras versions disagree on their order; set one")
            return
        if name in (None, "learning_rate"):
            eng.set_optimizer(store, learning_rate=v["learning_rate"])
        if name in (None, "beta_1", "beta_2", "epsilon"):
            eng.set_optimizer(store, beta1=v["beta_1"], beta2=v["beta_2"], eps=v["epsilon"])
        if name in (None, "clipvalue", "global_clipnorm"):
            eng.set_optimizer(store, clipping=(v["clipvalue"], v["global_clipnorm"]))

    def _bind(self, engine, store):
        self._engine, self._store = engine, store
        self._push()

    def get_config(self):
        """the settings as plain values (a schedule as its repr): what a checkpoint records"""
        return {k: (v if v is None or isinstance(v, (int, float)) else repr(v)) for k, v in self._values.items()}

    @property
    def last_global_norm(self):
        """the L2 norm of the whole gradient at this optimizer's last step, as a device scalar (no synchronisation); None without
        global_clipnorm"""
        opt = None if self._store is None else self._store.opt
        return opt.norm_dev[0] if opt is not None and opt.clipnorm_on else None

    def current_learning_rate(self):
        """the rate of the next step: the schedule at `iterations` (f64 on the host, the device's formulas)"""
        from .schedules import as_schedule
        return float(as_schedule(self._values["learning_rate"])[0](self.iterations))

    @property
    def iterations(self):
        return 0 if self._store is None else self._store.t

    def apply_gradients(self, grads_and_vars):
        """One Adam step of this optimizer's network (a custom train_step, tf_compat.tf.GradientTape): `grads_and_vars` pairs a
        gradient with every one of the network's trainable_variables.  The gradients a tape returned are views of its flat
        buffer, which Adam reads in place; other tensors are copied into a flat buffer first.  Advances `iterations` of this
        optimizer only (engine.apply_adam_store)."""
        store, eng = self._store, self._engine
        if store is None:
            raise RuntimeError("this optimizer is not bound to a network yet (a Pix2Pix*Model binds it in its constructor)")
        grads = {}
        for g, v in grads_and_vars:
            name = store.variable_name(v)
            if name is None:
                raise ValueError(f"apply_gradients: a variable of shape {tuple(getattr(v, 'shape', ()))} is not one of the "
                                 f"network this optimizer updates")
            if g is None:
                raise ValueError(f"apply_gradients: no gradient for {name} (the loss does not depend on this network)")
            if tuple(g.shape) != tuple(store.shapes[name]):
                raise ValueError(f"apply_gradients: gradient of shape {tuple(g.shape)} for {name} {tuple(store.shapes[name])}")
            grads[name] = g
        missing = [k for k in store.shapes if k not in grads]
        if missing:
            raise ValueError(f"apply_gradients steps the whole network: no gradient for {', '.join(missing)}")
        base = next(iter(grads.values()))._base
        if base is not None and base.dtype == torch.float32 and base.device == store.params.device and base.numel() == store.numel \
                and base.is_contiguous() \
                and all(g._base is base and g.is_contiguous() and g.data_ptr() == base.data_ptr() + 4 * store.offsets[k]
                        for k, g in grads.items()):
            flat = base             # the tape's own buffer
        else:
            flat = torch.zeros(store.numel, dtype=torch.float32, device=store.params.device)
            for k, g in grads.items():
                store.view(flat, k).copy_(g)
        eng.apply_adam_store(store, flat)


class Pix2PixModel(S2SModel):
    def __init__(self, train_ds, test_ds, model_name, architecture_name, lambda_l1, dtype="bf16", img_size=IMG_SIZE,
                 device="cuda:0", data_parallel=None, seed=None, ema_decay=None, ema_warmup=True, generator_optimizer=None,
                 discriminator_optimizer=None):
        super().__init__(train_ds, test_ds, model_name, architecture_name)
        if seed is None:
            from .tf_compat import global_seed      # configuration.SEED unless the notebook's tf.random.set_seed changed it
            seed = global_seed()
        self.lambda_l1 = lambda_l1
        self._dtype = {"bf16": L.BF16, "f32": L.F32}[dtype] if isinstance(dtype, str) else dtype
        self._img_size, self._device, self._seed = img_size, device, seed
        self.ema_decay, self.ema_warmup = ema_decay, bool(ema_warmup)
        self.data_parallel = data_parallel
        if data_parallel is not None and hasattr(train_ds, "set_shard"):
            train_ds.set_shard(data_parallel.rank, data_parallel.world)      # produce this rank's rows only

        self.generator = self.create_generator()
        self.discriminator = self.create_discriminator()
        self.loss_object = BinaryCrossentropy(from_logits=True)
        self.generator_optimizer, self.discriminator_optimizer = self.create_optimizers()
        if generator_optimizer is not None:
            self.generator_optimizer = generator_optimizer
        if discriminator_optimizer is not None:
            self.discriminator_optimizer = discriminator_optimizer
        if self.generator_optimizer is self.discriminator_optimizer:
            raise ValueError("the two networks need an optimizer object each (each holds its own step count and moments)")
        self.engine = self.create_engine()

        print(f"Generator: {self.generator.name} with {self.generator.count_params():,} parameters")
        print(f"Discriminator: {self.discriminator.name} with {self.discriminator.count_params():,} parameters")

        self.checkpoint = Checkpoint(generator_optimizer=self.generator_optimizer,
                                     discriminator_optimizer=self.discriminator_optimizer,
                                     generator=self.generator, discriminator=self.discriminator, engine=self.engine)
        self.checkpoint_manager = CheckpointManager(self.checkpoint, directory=self.checkpoint_dir, max_to_keep=1)
        self._hooks_checked = False
        self._custom_hooks = False

    # -- construction hooks (pix2pix_model.py:38-42) ------------------------------------------------------------
    def create_generator(self):
        return UnetGenerator(4, 4, "tanh")

    def create_discriminator(self):
        return PatchDiscriminator(4)

    def create_optimizers(self):
        """build-added: (generator optimizer, discriminator optimizer), the reference's pair (pix2pix_model.py:28-29) unless
        overridden; the constructor keywords generator_optimizer= / discriminator_optimizer= replace either"""
        return Adam(0.0002, beta_1=0.5), Adam(0.0002, beta_1=0.5)

    def create_engine(self):
        """build-added: one device engine for both networks, from the architecture the two builders recorded"""
        g, d = self.generator, self.discriminator
        if d.input_channels != g.input_channels:
            raise ValueError("the discriminator sees [target, source] images of the generator's input channel count")
        eng = Pix2PixEngine(g.input_channels, g.output_channels, g.last_activation, self._img_size, self._dtype,
                            device=self._device, seed=self._seed)
        go, do = self.generator_optimizer, self.discriminator_optimizer
        g.bind(eng, eng.G)
        d.bind(eng, eng.D)
        go._bind(eng, eng.G)        # each optimizer's settings into its network's slots (they may differ in everything)
        do._bind(eng, eng.D)
        if self.ema_decay is not None:
            eng.enable_ema(self.ema_decay, self.ema_warmup)
        if self.data_parallel is not None:
            eng.tape_refusal = ("a GradientTape step runs on one GPU (as the hooked steps): this model trains data-parallel, "
                                "its fused train_step issues the collectives")
        return eng

    # -- losses as standalone evaluations (pix2pix_model.py:44-56); train_step computes them fused ----------------
    def generator_loss(self, fake_predicted, fake_image, real_image):
        fp = torch.as_tensor(fake_predicted, dtype=torch.float32)
        adversarial_loss = self.loss_object(torch.ones_like(fp), fp)
        real = torch.as_tensor(real_image, dtype=torch.float32).to(fp.device)
        fake = torch.as_tensor(fake_image, dtype=torch.float32).to(fp.device)
        l1_loss = (real - fake).abs().mean()
        total_loss = adversarial_loss + (self.lambda_l1 * l1_loss)
        return total_loss, adversarial_loss, l1_loss

    def discriminator_loss(self, real_predicted, fake_predicted):
        rp = torch.as_tensor(real_predicted, dtype=torch.float32)
        fp = torch.as_tensor(fake_predicted, dtype=torch.float32)
        real_loss = self.loss_object(torch.ones_like(rp), rp)
        fake_loss = self.loss_object(torch.zeros_like(fp), fp)
        total_loss = fake_loss + real_loss
        return total_loss, real_loss, fake_loss

    def _weights_for(self, averaged):
        """context under which a generator call runs on the weights asked for: averaged=None is the averaged generator where the
        model keeps one and the live generator otherwise; True without an average is an error"""
        import contextlib
        on = self.engine.ema_enabled
        if averaged is None:
            averaged = on
        if averaged and not on:
            raise ValueError("averaged=True, but this model keeps no averaged generator (construct it with ema_decay=...)")
        return self.engine.averaged() if averaged else contextlib.nullcontext()

    def generate(self, batch, snap=None, averaged=None):
        """pix2pix_model.py:58-60.  `averaged` (build-added): the averaged generator (default where the model has one) or the live
        one (False).  `snap` (build-added) moves every generated pixel to the nearest colour of a palette
        (palette.snap_to_palette, f32 result, not differentiable): "target" / "source" use the palette extracted from that image
        of the batch on the device (an image with more than MAX_PALETTE_SIZE colours is returned as generated), a
        (palette (B, K, 4), sizes (B,) or None) pair is used as given; an int K in 1..256 needs no palette from elsewhere: every
        generated image is reduced to at most K colours of its own (palette.quantize: integer k-means on the image, then the snap;
        sprites of at most 128 x 128); None returns the generator's output unchanged."""
        if isinstance(snap, bool):
            raise TypeError(f'snap is None, "target", "source", a number of colours or a (palette, sizes) pair, got {snap!r}')
        source_image, target_image = batch
        with self._weights_for(averaged):
            fake_image = self.generator(source_image, training=True)
        if snap is None:
            return fake_image
        if isinstance(snap, int):
            return _palette.quantize(fake_image, colours=snap, device=fake_image.device)[0].image
        if isinstance(snap, str):
            if snap not in ("target", "source"):
                raise ValueError(f'snap is None, "target", "source" or a (palette, sizes) pair, got {snap!r}')
            palette, sizes = _palette.extract_palette_batch(target_image if snap == "target" else source_image, check=False,
                                                            device=fake_image.device)
        else:
            palette, sizes = snap
        return _palette.snap_to_palette(fake_image, palette, sizes, device=fake_image.device).image

    # -- the hot path ----------------------------------------------------------------------------------------------
    def _check_hooks(self):
        """Which train step serves this class?  The reference's own loss sets (Pix2PixModel / Pix2PixHistogramModel /
        Pix2PixIndexedModel) run fused: losses and gradients in one kernel sequence, no tape.  A subclass that OVERRIDES
        generator_loss / discriminator_loss (the hooks are part of the boundary) gets `engine.train_step_rgba_hooked`:
        the kernels run forward, the hooks are evaluated on torch tensors with autograd, their gradients enter the backward kernels.
        The palette-index model's step is fused around its softmax head and argmax: overriding ITS hooks is refused unless the
        subclass opts in with `differentiable_loss_hooks = True` (engine.train_step_indexed_hooked: unfused head, four f32
        (B,S,S,256) tensors, slower)."""
        if self._hooks_checked:
            return
        known = (Pix2PixModel, Pix2PixHistogramModel, Pix2PixIndexedModel)
        custom = []
        for hook in ("generator_loss", "discriminator_loss"):
            owner = next((c for c in type(self).__mro__ if hook in c.__dict__), None)
            if owner not in known:
                custom.append(hook)
        if custom and isinstance(self, Pix2PixIndexedModel) and not self.differentiable_loss_hooks:
            raise NotImplementedError(
                f"{type(self).__name__}.{custom[0]} overrides the reference's loss, but the palette-index train_step is one fused "
                f"sequence of HIP kernels around the softmax head and its argmax (no gradient path from the discriminator, "
                f"pix2pix_model.py:295-325): set `differentiable_loss_hooks = True` on the subclass to train through the "
                f"unfused hooked step (engine.train_step_indexed_hooked), or subclass train_step.")
        if custom and self.data_parallel is not None:
            raise NotImplementedError("overridden loss hooks run on one GPU (the hooked step issues no collectives)")
        self._custom_hooks = bool(custom)
        self._hooks_checked = True

    def _shard(self, batch, tensors):
        """(local shard of every tensor, global batch, samples in front of the shard, DataParallel or None)"""
        dp = self.data_parallel
        if isinstance(batch, ShardedBatch):       # the dataset produced this rank's rows only
            return tensors, batch.global_batch, batch.offset, dp
        Bg = len(tensors[0])
        if dp is None:
            return self._upload(tensors), Bg, 0, None
        lo, hi = shard_bounds(Bg, dp.world, dp.rank)
        return self._upload([t[lo:hi] for t in tensors]), Bg, lo, dp

    def _upload(self, tensors):
        """host batches (numpy / CPU tensors) go up on a copy stream, beside the previous step's kernels (dataset_utils.upload_async)"""
        if len(tensors[0]) == 0 or self.engine.device.type != "cuda":
            return tensors
        from .dataset_utils import upload_async
        return upload_async(tensors, self.engine.device)

    def train_step(self, batch, step, update_steps):
        """pix2pix_model.py:62-89"""
        self._check_hooks()
        source_image, real_image = batch
        (src, real), Bg, lo, dp = self._shard(batch, [source_image, real_image])
        if self._custom_hooks:
            out = self.engine.train_step_rgba_hooked(src, real, self.generator_loss, self.discriminator_loss)
        elif len(src) == 0:
            out = self.engine.train_step_empty(self.lambda_l1, dp=dp)
        else:
            out = self.engine.train_step_rgba(src, real, self.lambda_l1, global_batch=Bg, dp=dp, batch_offset=lo)
        g_loss, d_loss = (out[0], out[1], out[2]), (out[4], out[5], out[6])
        self._log(g_loss, d_loss, step, update_steps)
        return g_loss, d_loss

    def _log(self, g_loss, d_loss, step, update_steps):
        if self.summary_writer is None:
            return
        s = int(step) // int(update_steps)
        self.log_generator_loss(g_loss, s)
        self.log_discriminator_loss(d_loss, s)
        self.log_optimizers(s)

    def log_optimizers(self, step):
        """build-added: the rate of the step just taken for an optimizer with a schedule, the gradient norm (device scalar, no
        synchronisation) for one with global_clipnorm; the reference's optimizers log nothing (the same event files as before)"""
        from .schedules import LearningRateSchedule
        for tag, opt in (("generator", self.generator_optimizer), ("discriminator", self.discriminator_optimizer)):
            if isinstance(opt.learning_rate, LearningRateSchedule):
                self.summary_writer.scalar(f"{tag}/learning_rate", float(opt.learning_rate(max(opt.iterations - 1, 0))), step)
            if opt.last_global_norm is not None:
                self.summary_writer.scalar(f"{tag}/gradient_norm", opt.last_global_norm.clone(), step)

    def log_generator_loss(self, g_loss, step):
        """pix2pix_model.py:91-95"""
        total_loss, adversarial_loss, l1_loss = g_loss[:3]
        self.summary_writer.scalar("generator/total_loss", total_loss, step)
        self.summary_writer.scalar("generator/adversarial_loss", adversarial_loss, step)
        self.summary_writer.scalar("generator/l1_loss", l1_loss, step)

    def log_discriminator_loss(self, d_loss, step):
        """pix2pix_model.py:97-101"""
        total_loss, real_loss, fake_loss = d_loss
        self.summary_writer.scalar("discriminator/total_loss", total_loss, step)
        self.summary_writer.scalar("discriminator/real_loss", real_loss, step)
        self.summary_writer.scalar("discriminator/fake_loss", fake_loss, step)

    # -- evaluation helpers used by do_fit ---------------------------------------------------------------------------
    def select_examples_for_visualization(self, number_of_examples=6):
        """pix2pix_model.py:103-110"""
        num_train_examples = number_of_examples // 2
        num_test_examples = number_of_examples - num_train_examples
        train_examples = self._whole(self.train_ds).unbatch().take(num_train_examples).batch(1)
        test_examples = self._whole(self.test_ds).unbatch().take(num_test_examples).batch(1)
        return list(test_examples.as_numpy_iterator()) + list(train_examples.as_numpy_iterator())

    def evaluate_l1_batch(self, batch):
        source, target = batch[0], batch[1]
        fake = self.generate((source, target))
        return (torch.as_tensor(target, dtype=torch.float32).to(fake.device) - fake).abs().mean()


class Pix2PixAugmentedModel(Pix2PixModel):
    """pix2pix_model.py:232-234"""

    def __init__(self, train_ds, test_ds, model_name, architecture_name, lambda_l1, **kw):
        super().__init__(train_ds, test_ds, model_name, architecture_name, lambda_l1, **kw)


class Pix2PixHistogramModel(Pix2PixAugmentedModel):
    """pix2pix_model.py:237-258"""

    def __init__(self, train_ds, test_ds, model_name, architecture_name, lambda_l1, lambda_histogram, **kw):
        super().__init__(train_ds, test_ds, model_name, architecture_name, lambda_l1, **kw)
        self.lambda_histogram = lambda_histogram

    def generator_loss(self, fake_predicted, fake_image, real_image):
        real_histogram = self.engine.rgbuv_histogram(real_image)
        fake_histogram = self.engine.rgbuv_histogram(fake_image)
        histogram_loss = _histogram.hellinger_loss(real_histogram, fake_histogram)
        total_loss, adversarial_loss, l1_loss = super().generator_loss(fake_predicted, fake_image, real_image)
        total_loss = total_loss + self.lambda_histogram * histogram_loss
        return total_loss, adversarial_loss, l1_loss, histogram_loss

    def discriminator_loss(self, real_predicted, fake_predicted):
        return super().discriminator_loss(real_predicted, fake_predicted)

    def train_step(self, batch, step, update_steps):
        self._check_hooks()
        source_image, real_image = batch
        (src, real), Bg, lo, dp = self._shard(batch, [source_image, real_image])
        if self._custom_hooks:
            out = self.engine.train_step_rgba_hooked(src, real, self.generator_loss, self.discriminator_loss)
        elif len(src) == 0:
            out = self.engine.train_step_empty(self.lambda_l1, lambda_hist=self.lambda_histogram, dp=dp)
        else:
            out = self.engine.train_step_rgba(src, real, self.lambda_l1, lambda_hist=self.lambda_histogram,
                                              global_batch=Bg, dp=dp, batch_offset=lo)
        g_loss, d_loss = (out[0], out[1], out[2], out[3]), (out[4], out[5], out[6])
        self._log(g_loss, d_loss, step, update_steps)
        return g_loss, d_loss

    def log_generator_loss(self, g_loss, step):
        """pix2pix_model.py:255-258"""
        super().log_generator_loss(g_loss[:3], step)
        self.summary_writer.scalar("generator/histogram_loss", g_loss[3], step)


class Pix2PixPaletteModel(Pix2PixAugmentedModel):
    """Build-added (no counterpart in the reference): an RGBA generator held to the target sprite's palette.  generator_loss adds
    lambda_palette * the total variation between the soft palette histograms of the real and the generated image, both taken under
    the REAL image's palette (palette.soft_palette_histogram), and lambda_conformance * the generated pixels' mean weighted squared
    distance to that palette.  The palette is extracted on the device at every step (the dataset's augmentation changes the hues
    per batch) without a host sync; an image with more than MAX_PALETTE_SIZE colours contributes nothing to either term.
    The class overrides the loss hook, so by default train_step runs engine.train_step_rgba_hooked: one GPU, not replayed.
    `fused=True` computes the same loss inside the fused step instead (engine.train_step_rgba(palette=...): HIP only, replayed,
    data-parallel); generator_loss then remains a standalone evaluation, as in Pix2PixHistogramModel, and a subclass
    that overrides a loss hook has to stay with the hooked step."""

    def __init__(self, train_ds, test_ds, model_name, architecture_name, lambda_l1, lambda_palette, lambda_conformance=0.0,
                 temperature=1e-3, fused=False, **kw):
        self.fused = bool(fused)
        if self.fused:
            for hook, home in (("generator_loss", Pix2PixPaletteModel), ("discriminator_loss", Pix2PixModel)):
                owner = next(c for c in type(self).__mro__ if hook in c.__dict__)
                if owner is not home:
                    raise ValueError(f"{owner.__name__}.{hook} overrides the loss, but fused=True computes {home.__name__}'s own loss "
                                     f"in HIP kernels and never calls the hook: construct the model with fused=False (the hooked step)")
        super().__init__(train_ds, test_ds, model_name, architecture_name, lambda_l1, **kw)
        if not 0.0 < float(temperature) < float("inf"):
            raise ValueError(f"the temperature must be positive and finite, got {temperature}")
        self.lambda_palette, self.lambda_conformance, self.temperature = lambda_palette, lambda_conformance, float(temperature)

    def _check_hooks(self):
        if self.fused:          # the constructor has checked that the hooks are the class's own
            self._custom_hooks, self._hooks_checked = False, True
            return
        super()._check_hooks()

    def generator_loss(self, fake_predicted, fake_image, real_image):
        fake = torch.as_tensor(fake_image)
        real = torch.as_tensor(real_image).to(fake.device)
        palette, sizes = _palette.extract_palette_batch(real, check=False)
        real_histogram, _ = _palette.soft_palette_histogram(real, palette, sizes, self.temperature)
        fake_histogram, fake_conformance = _palette.soft_palette_histogram(fake, palette, sizes, self.temperature)
        palette_loss = _palette.palette_histogram_loss(real_histogram, fake_histogram)
        total_loss, adversarial_loss, l1_loss = super().generator_loss(fake_predicted, fake_image, real_image)
        total_loss = total_loss + self.lambda_palette * palette_loss + self.lambda_conformance * fake_conformance.mean()
        return total_loss, adversarial_loss, l1_loss, palette_loss

    def train_step(self, batch, step, update_steps):
        self._check_hooks()
        source_image, real_image = batch
        (src, real), Bg, lo, dp = self._shard(batch, [source_image, real_image])
        terms = (self.lambda_palette, self.lambda_conformance, self.temperature)
        if not self.fused:
            out = self.engine.train_step_rgba_hooked(src, real, self.generator_loss, self.discriminator_loss)
        elif len(src) == 0:
            out = self.engine.train_step_empty(self.lambda_l1, dp=dp, palette=terms)
        else:
            out = self.engine.train_step_rgba(src, real, self.lambda_l1, global_batch=Bg, dp=dp, batch_offset=lo, palette=terms)
        g_loss, d_loss = (out[0], out[1], out[2], out[3]), (out[4], out[5], out[6])
        self._log(g_loss, d_loss, step, update_steps)
        return g_loss, d_loss

    def log_generator_loss(self, g_loss, step):
        super().log_generator_loss(g_loss[:3], step)
        self.summary_writer.scalar("generator/palette_loss", g_loss[3], step)


class Pix2PixDiffAugmentModel(Pix2PixModel):
    """Build-added (no counterpart in the reference): the RGBA model with differentiable augmentation in front of the
    discriminator (diffaugment.py; DiffAugment, Zhao et al. 2020), for training sets of a few hundred pairs.  Where
    Pix2PixAugmentedModel augments the dataset -- and so changes what the generator is asked to produce -- this class leaves the
    batch alone and augments what the DISCRIMINATOR sees; the generator's gradient flows back through the augmentation.

    train_step is the reference's step (pix2pix_model.py:62-89) written for tf.GradientTape.  ONE parameter table, drawn from
    (seed, step) alone, serves the real and the fake pair, and the source image, which both pairs share, is augmented once: the two
    pairs the discriminator compares differ only in the image under judgement.  The L1 term is taken on the un-augmented images.
    `policy` is a comma-separated subset of diffaugment.POLICIES ("" trains as the plain tape step does).  Like every tape step it
    runs on one GPU and is not replayed; generate() and the report_* evaluations are inherited: augmentation never touches inference."""

    def __init__(self, train_ds, test_ds, model_name, architecture_name, lambda_l1, policy="color,translation,cutout", **kw):
        _diffaugment.policy_bits(policy)          # an unknown name fails here, not at the first step
        super().__init__(train_ds, test_ds, model_name, architecture_name, lambda_l1, **kw)
        self.policy = policy

    def augmented_step(self, source_image, real_image, step, masks=None, apply=True):
        """one step at the parameter table of `step`: (g_loss, d_loss, generator gradients, discriminator gradients), both
        gradients taken at the pre-update weights.  masks: injected dropout keep-masks instead of the device's draw; apply=False
        leaves the weights alone."""
        from .tape import GradientTape
        source_image, real_image = self._upload([source_image, real_image])
        B = len(source_image)
        p = _diffaugment.draw_parameters(B, self._img_size, self._img_size, self.policy, self._seed, int(step))
        with GradientTape(persistent=True) as tape:
            fake_image = self.generator(source_image, training=True, masks=masks)
            source_aug = _diffaugment.diff_augment(source_image, p, self.policy, device=self.engine.device)
            real_aug = _diffaugment.diff_augment(real_image, p, self.policy, device=self.engine.device)
            fake_aug = _diffaugment.diff_augment(fake_image, p, self.policy, device=self.engine.device)
            real_predicted = self.discriminator([real_aug, source_aug], training=True)
            fake_predicted = self.discriminator([fake_aug, source_aug], training=True)
            g_loss = self.generator_loss(fake_predicted, fake_image, real_image)
            d_loss = self.discriminator_loss(real_predicted, fake_predicted)
        generator_gradients = tape.gradient(g_loss[0], self.generator.trainable_variables)
        discriminator_gradients = tape.gradient(d_loss[0], self.discriminator.trainable_variables)
        if apply:
            self.generator_optimizer.apply_gradients(zip(generator_gradients, self.generator.trainable_variables))
            self.discriminator_optimizer.apply_gradients(zip(discriminator_gradients, self.discriminator.trainable_variables))
        tape.release()
        return tuple(x.detach() for x in g_loss), tuple(x.detach() for x in d_loss), generator_gradients, discriminator_gradients

    def train_step(self, batch, step, update_steps):
        source_image, real_image = batch
        g_loss, d_loss, _, _ = self.augmented_step(source_image, real_image, step)
        self._log(g_loss, d_loss, step, update_steps)
        return g_loss, d_loss


class Pix2PixPaletteSnapModel(Pix2PixModel):
    """Build-added (no counterpart in the reference): the RGBA model trained THROUGH the palette snap.  generate(snap="target")
    repairs a generated sprite after training; here the repair is part of the step: the fake image is projected onto the palette
    of the real image (palette.project_to_palette) before the discriminator judges it, so the discriminator sees what inference
    will return and the generator is trained on what survives the snap.  `hard` / `gradient` / `temperature` choose the projection:
    (True, "identity") is the snap with the straight-through gradient, (True, "soft") the snap with the soft projection's Jacobian,
    (False, "soft") the soft projection with its exact gradient.  The real image lies on its own palette and is not projected; the
    L1 term is taken on the un-projected fake image.  An image whose target has more than MAX_PALETTE_SIZE colours passes through.

    train_step is the reference's step (pix2pix_model.py:62-89) written for tf.GradientTape, as Pix2PixDiffAugmentModel's: one GPU,
    not replayed.  generate() and the report_* evaluations are inherited; generate(batch, snap="target") is the matching inference
    call."""

    def __init__(self, train_ds, test_ds, model_name, architecture_name, lambda_l1, hard=True, gradient="identity", temperature=5e-2,
                 **kw):
        _palette.check_projection_mode(hard, gradient)          # a pair without a meaning fails here, not at the first step
        if not 0.0 < float(temperature) < float("inf"):
            raise ValueError(f"the temperature must be positive and finite, got {temperature}")
        super().__init__(train_ds, test_ds, model_name, architecture_name, lambda_l1, **kw)
        self.hard, self.gradient, self.temperature = bool(hard), gradient, float(temperature)

    def projected_step(self, source_image, real_image, step, masks=None, apply=True):
        """one step: (g_loss, d_loss, generator gradients, discriminator gradients, projected fake image), both gradients taken at
        the pre-update weights.  masks: injected dropout keep-masks instead of the device's draw; apply=False leaves the weights
        alone.  (`step` is not used: the projection has no random part.)"""
        from .tape import GradientTape
        source_image, real_image = self._upload([source_image, real_image])
        palette, sizes = _palette.extract_palette_batch(real_image, check=False, device=self.engine.device)      # no host sync
        with GradientTape(persistent=True) as tape:
            fake_image = self.generator(source_image, training=True, masks=masks)
            projected_fake = _palette.project_to_palette(fake_image, palette, sizes, self.temperature, self.hard, self.gradient,
                                                         device=self.engine.device)
            real_predicted = self.discriminator([real_image, source_image], training=True)
            fake_predicted = self.discriminator([projected_fake, source_image], training=True)
            g_loss = self.generator_loss(fake_predicted, fake_image, real_image)
            d_loss = self.discriminator_loss(real_predicted, fake_predicted)
        generator_gradients = tape.gradient(g_loss[0], self.generator.trainable_variables)
        discriminator_gradients = tape.gradient(d_loss[0], self.discriminator.trainable_variables)
        if apply:
            self.generator_optimizer.apply_gradients(zip(generator_gradients, self.generator.trainable_variables))
            self.discriminator_optimizer.apply_gradients(zip(discriminator_gradients, self.discriminator.trainable_variables))
        tape.release()
        return (tuple(x.detach() for x in g_loss), tuple(x.detach() for x in d_loss), generator_gradients, discriminator_gradients,
                projected_fake.detach())

    def train_step(self, batch, step, update_steps):
        source_image, real_image = batch
        g_loss, d_loss, _, _, _ = self.projected_step(source_image, real_image, step)
        self._log(g_loss, d_loss, step, update_steps)
        return g_loss, d_loss


class Pix2PixIndexedModel(Pix2PixModel):
    """pix2pix_model.py:261-330.  A subclass that overrides generator_loss / discriminator_loss must also set
    `differentiable_loss_hooks = True`: its hooks then run under autograd beside the kernels (engine.train_step_indexed_hooked),
    at the price of the unfused head and four f32 (B,S,S,256) tensors per step."""

    differentiable_loss_hooks = False

    def __init__(self, train_ds, test_ds, model_name, architecture_name, lambda_segmentation=0.5, **kw):
        super().__init__(train_ds, test_ds, model_name, architecture_name, 0., **kw)      # lambda_l1 = 0 (:263)
        self.lambda_segmentation = lambda_segmentation
        self.segmentation_loss_object = CategoricalCrossentropy()

    def create_generator(self):
        return UnetGenerator(1, MAX_PALETTE_SIZE, "softmax")

    def create_discriminator(self):
        return PatchDiscriminator(1)

    def generator_loss(self, fake_predicted, fake_image, real_image):
        """pix2pix_model.py:273-278 (fake_image = probabilities, real_image = one-hot)"""
        segmentation_loss = self.segmentation_loss_object(real_image, fake_image)
        total_loss, adversarial_loss, l1_loss = super().generator_loss(fake_predicted, fake_image, real_image)
        total_loss = total_loss + self.lambda_segmentation * segmentation_loss
        return total_loss, adversarial_loss, l1_loss, segmentation_loss

    def discriminator_loss(self, real_predicted, fake_predicted):
        return super().discriminator_loss(real_predicted, fake_predicted)

    def generate(self, batch, averaged=None):
        """pix2pix_model.py:283-287 (`averaged`: as Pix2PixModel.generate)"""
        source_image = batch[0]
        with self._weights_for(averaged):
            return self.engine.generate_indexed(source_image)

    def debug_discriminator_patches(self, batch_of_one):
        """pix2pix_model.py:372-431: as the base class, on index images (the discriminator of this model sees indices)"""
        source, real = batch_of_one[0], batch_of_one[1]
        fake = self.generate(batch_of_one, averaged=False)          # the live pair: the discriminator was trained against it
        out = {}
        for name, img in (("real", real), ("fake", fake)):
            logits = self.discriminator([img, source], training=True)
            prob = torch.sigmoid(logits[0, :, :, 0].to(torch.float32)).cpu().numpy()
            out[name], out[name + "_mean"] = prob, float(prob.mean())
        return out

    def generate_with_probs(self, batch, averaged=None):
        """pix2pix_model.py:289-293 (`averaged`: as Pix2PixModel.generate)"""
        source_image = batch[0]
        with self._weights_for(averaged):
            return self.engine.generate_indexed(source_image, with_probs=True)

    def train_step(self, batch, step, update_steps):
        """pix2pix_model.py:295-325"""
        self._check_hooks()
        source_image, real_image, _ = batch
        (src, real), Bg, lo, dp = self._shard(batch, [source_image, real_image])
        if self._custom_hooks:
            out = self.engine.train_step_indexed_hooked(src, real, self.generator_loss, self.discriminator_loss)
        elif len(src) == 0:
            out = self.engine.train_step_empty(0.0, lambda_aux=self.lambda_segmentation, dp=dp)
        else:
            out = self.engine.train_step_indexed(src, real, self.lambda_segmentation, global_batch=Bg, dp=dp, batch_offset=lo)
        g_loss, d_loss = (out[0], out[1], out[2], out[3]), (out[4], out[5], out[6])
        self._log(g_loss, d_loss, step, update_steps)
        return g_loss, d_loss

    def log_generator_loss(self, g_loss, step):
        """pix2pix_model.py:327-330"""
        super().log_generator_loss(g_loss[:3], step)
        self.summary_writer.scalar("generator/segmentation_loss", g_loss[3], step)

    def evaluate_l1_batch(self, batch):
        fake = self.generate(batch).to(torch.float32)
        target = torch.as_tensor(batch[1], dtype=torch.float32).to(fake.device)
        return (target - fake).abs().mean()


class Pix2PixIndexedColourModel(Pix2PixIndexedModel):
    """Build-added (no counterpart in the reference): the palette-index model with losses that know what a palette slot
    LOOKS like.  The parent's generator learns from lambda_segmentation * CCE alone, to which every wrong slot costs the same -- one
    shade off or the hot-pink filler that pads the palette.  Here the probabilities are mapped through the batch's palette to an RGBA
    image (palette.palette_lookup: the expected colour, or with `hard` the argmax's colour with the straight-through gradient;
    `blacken` treats transparent slots as dataset_utils.blacken_transparent_pixels treats transparent pixels) and generator_loss adds
        lambda_colour * mean |real_rgba - fake_rgba|
        + lambda_histogram * hellinger_loss(calculate_rgbuv_histogram(real_rgba), calculate_rgbuv_histogram(fake_rgba)),
    real_rgba being the palette gather of the real indices.  At lambda_histogram == 0 the histogram term is not computed (no launch).
    train_step keeps the batch's palette on the device for the hook and otherwise is the parent's hooked step
    (differentiable_loss_hooks: engine.train_step_indexed_hooked, one GPU, not replayed); it returns and logs the two terms behind the
    parent's four (generator/colour_l1_loss, generator/histogram_loss).
    The class does NOT change what the discriminator sees: it still judges argmax indices, and the argmax still blocks every gradient
    from the discriminator to the generator.  The colour terms reach the generator through the probabilities only."""

    differentiable_loss_hooks = True

    def __init__(self, train_ds, test_ds, model_name, architecture_name, lambda_segmentation=0.5, lambda_colour=100.0,
                 lambda_histogram=0.0, hard=False, blacken=True, **kw):
        for name, value in (("lambda_colour", lambda_colour), ("lambda_histogram", lambda_histogram)):
            if not float(value) >= 0.0:
                raise ValueError(f"{name} must not be negative, got {value}")
        super().__init__(train_ds, test_ds, model_name, architecture_name, lambda_segmentation, **kw)
        self.lambda_colour, self.lambda_histogram = float(lambda_colour), float(lambda_histogram)
        self.hard, self.blacken = bool(hard), bool(blacken)
        self._step_palette = None
        self._colour_terms = None

    def generator_loss(self, fake_predicted, fake_image, real_image, palette=None):
        """fake_image = probabilities, real_image = one-hot, as the parent's; `palette` (B, 256, 4): the batch's palette for a
        standalone evaluation (train_step supplies its own batch's)."""
        palette = self._step_palette if palette is None else palette
        if palette is None:
            raise ValueError("Pix2PixIndexedColourModel.generator_loss needs the batch's palette: pass palette=, or call train_step")
        total_loss, adversarial_loss, l1_loss, segmentation_loss = super().generator_loss(fake_predicted, fake_image, real_image)
        dev = self.engine.device
        fake_rgba = _palette.palette_lookup(fake_image, palette, self.hard, self.blacken, device=dev)
        with torch.no_grad():       # a one-hot row's argmax is its index: the palette gather of the real indices, bit for bit
            real_rgba = _palette.palette_lookup(real_image, palette, True, self.blacken, device=dev)
        colour_loss = (real_rgba - fake_rgba).abs().mean()
        total_loss = total_loss + self.lambda_colour * colour_loss
        if self.lambda_histogram != 0.0:
            real_histogram = _histogram.calculate_rgbuv_histogram(real_rgba, device=dev)
            fake_histogram = _histogram.calculate_rgbuv_histogram(fake_rgba, device=dev)
            histogram_loss = _histogram.hellinger_loss(real_histogram, fake_histogram)
            total_loss = total_loss + self.lambda_histogram * histogram_loss
        else:
            histogram_loss = torch.zeros((), dtype=torch.float32, device=colour_loss.device)
        self._colour_terms = (colour_loss.detach(), histogram_loss.detach())
        return total_loss, adversarial_loss, l1_loss, segmentation_loss, colour_loss, histogram_loss

    def train_step(self, batch, step, update_steps):
        self._check_hooks()          # data parallelism is refused before anything is uploaded
        self._step_palette = torch.as_tensor(batch[2]).to(device=self.engine.device, dtype=torch.int32)
        self._colour_terms = None
        try:
            g_loss, d_loss = super().train_step(batch, step, update_steps)
        finally:
            self._step_palette = None
        return g_loss + self._colour_terms, d_loss

    def log_generator_loss(self, g_loss, step):
        super().log_generator_loss(g_loss[:4], step)
        colour_loss, histogram_loss = self._colour_terms
        self.summary_writer.scalar("generator/colour_l1_loss", colour_loss, step)
        self.summary_writer.scalar("generator/histogram_loss", histogram_loss, step)
