"""Device engine of the Pix2Pix side2side training step on MI355X.

Issues the HIP kernels of libp2pgan_hip.so in the order of the reference's train_step (pix2pix_model.py:62-89, 295-325) on the
HBM layout of buffers.py (haloed NHWC activation buffers, concat-by-slice, flat f32 parameter / gradient / Adam buffers, per-layer
weight copies for the MFMA kernels); a recorded step is packed by replay_pack.py.  PyTorch tensors are only device-memory holders
here; every arithmetic op on the path is a call into the C ABI (include/p2pgan.h).  There is no CPU fallback.
"""
from collections import OrderedDict
import ctypes as C
import math
import operator
import os

import numpy as np
import torch

from . import _lib as L
from . import histogram as _histogram
from .buffers import (HALO, DOWN_FILTERS, UP_FILTERS, NULL, DenseBuf, HaloBuf, LayerW, ParamStore, _p, _torch_dtype,  # noqa: F401
                      discriminator_param_shapes, generator_param_shapes, pad8, up32)
from .replay_pack import ReplayCall, _pack_arg, pack_replay  # noqa: F401

IN_EPS = 1e-3           # tfa InstanceNormalization default (networks.py:18,29)
LEAKY_ALPHA = 0.3       # keras LeakyReLU default (networks.py:19)
UP_DROPOUT = (True, True, True, False, False, False)
MAX_PALETTE_SIZE = 256


def _flag(text):
    return text != "0"


# The A/B switches of the engine: (attribute, environment variable or None, default, parser of the variable's text).  __init__ sets
# every attribute from this table -- nothing else in this file reads the environment -- and tests, tools and bench.py assign them
# as plain attributes ("side.x": attribute x of the weight-gradient stream helper).
# SWITCHES choose kernels, K splits and grids: a recorded step holds those choices BY VALUE, so _replay_key takes every one of them
# from this same table -- a switch added here cannot be forgotten there and let a stale recording replay the wrong kernels.
SWITCHES = (
    ("use_conv_fewout", "P2P_CONV_FEWOUT", True, _flag),        # 1..4-output heads: tap-major GEMM + shifted sum
    ("use_conv_strip", "P2P_CONV_STRIP", True, _flag),          # up6 (32 <-> 128 channels): LDS strip, weights in registers
    ("use_conv_fewin", "P2P_CONV_FEWIN", True, _flag),          # 8-channel inputs: weights in registers, strip in LDS
    ("wgemm_want", "P2P_WGEMM_WANT", 512, int),                 # workgroups wanted per 128x128-tile weight-gradient GEMM
    # f32 (parity) mode is BATCH-INVARIANT on the data path: every per-image result (activations, data gradients) is produced
    # by the same kernel variant, the same K split and the same statistics algorithm whatever the batch size, so an N-rank
    # sharded step equals the 1-rank step image by image, bit for bit, and differs only in the order of the final weight-
    # gradient sums.  (The heuristics otherwise look at the batch: a 2+2 split of a batch of 4 then rounds differently,
    # and one ReLU flip in the 1x1 .. 4x4 layers is enough to move Adam's first steps apart -- tests/test_dp_gpu.py.)
    # (__init__ turns it off for bf16)
    ("batch_invariant", "P2P_BATCH_INVARIANT", True, _flag),
    ("wgemm_pipe", "P2P_WGEMM_PIPE", True, _flag),
    ("wgemm_want_pipe", "P2P_WGEMM_WANT_PIPE", 256, int),
    # workgroups wanted per implicit-GEMM launch; 0 = by batch (_splitk): every extra K slice is another f32 slab that the
    # layer's consumers (normalisation forward / backward) read, which is what a launch-bound small batch pays for
    ("splitk_target", "P2P_SPLITK_TARGET", 0, int),
    # partial-pixel stores (the source channels of the last concat buffer, the halves of the discriminator's fake pixel) are
    # issued by the kernel that writes the rest of the pixel (0: separate stores in p2p_pack_pair, the r02 form)
    ("full_pixels", "P2P_FULL_PIXELS", True, _flag),
    ("fuse_act_bwd", "P2P_FUSE_ACT_BWD", 1, int),               # D.last data gradient + LeakyReLU backward in one launch
    # Adam emitting the operand copies of the weights it updates (one pass, p2p_adam_prep_batched): measured 0.198 ms against
    # 0.187 ms for the flat Adam + batched copy launch on c2 (the tiled kernel streams slower than the flat one): off
    ("fuse_adam", None, False, None),       # (no environment switch: tests/test_train_step_gpu.py toggles the attribute)
    ("use_head_fused", "P2P_HEAD_FUSED", True, _flag),          # indexed head: conv + softmax + CCE + argmax + gradient in one launch
    ("split_prep", "P2P_SPLIT_PREP", 1, int),                   # weight copies of the early-Adam part refreshed right behind it
    # forks that follow p2p_norm_act_bwd / p2p_act_bwd ride on that kernel's own completion signal (p2p_arm_stop_event) instead of
    # a marker packet on the main stream; 0 = every fork is an event record
    ("side.stop_event_forks", "P2P_STOP_EVENT_FORKS", True, _flag),
)
# GATES decide whether a step is recorded, replayed or elided at all, not which kernels a recorded step holds.
GATES = (
    # replay of the recorded step through ONE library call (see _REC below), at every batch size
    ("replay_max_batch", "P2P_REPLAY_MAX_BATCH", 1 << 30, int),
    ("replay_enabled", "P2P_REPLAY", True, _flag),
    # The encoder block whose output map is 1x1 under InstanceNorm (the sixth at 64x64; none from 128x128 on): over one pixel
    # x - mean(x) is exactly 0, so its output is act(beta) whatever its convolution computes, d(raw) is exactly 0, and with it
    # its kernel's and gamma's gradients and the data gradient it hands to the block above; Adam never moves the kernel
    # (DESIGN.md section 4).  The fused train steps leave that work out: 0 = issue everything; 1 = no forward / data-gradient
    # / weight-gradient GEMM of the block and its kernel out of the in-step weight-copy launch, with the entry points and the
    # launch count per entry point the step has always had (the normalisation runs on a zero "convolution result", Adam
    # still passes over the kernel and leaves it as it is); 2 = also the 1x1 normalisation kernels that read no convolution
    # result (p2p_norm_act_fwd_1x1 / _bwd_1x1) and Adam with a hole (p2p_adam_flat_dev_excl).  Bit-identical results at
    # every level (tests/test_dead_bottleneck_gpu.py).  The level in force enters the replay key as _elide.
    ("elide_dead_bottleneck", "P2P_ELIDE_DEAD", 1, int),
)


_SWITCH_VALUES = operator.attrgetter(*(attr for attr, *_ in SWITCHES))     # engine -> the switch part of its replay key


def _switch_holder(eng, attr):
    """(object, attribute name) of a table entry"""
    *path, name = attr.split(".")
    for p in path:
        eng = getattr(eng, p)
    return eng, name


_RAW_STREAM = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_STREAM_DEVICE = [None]          # device index of the process's engine (one process per GPU)


def _stream():
    """the current HIP stream as a C pointer.  Asked ~110 times per train step: the raw query (no torch.cuda.Stream object) keeps
    the host side of a batch-4 step (launch-bound: fit() at the reference's BATCH_SIZE) short."""
    if _RAW_STREAM is not None and _STREAM_DEVICE[0] is not None:
        return C.c_void_p(_RAW_STREAM(_STREAM_DEVICE[0]))
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


# Step replay.  A train step is ~105 C-ABI kernel calls and ~40 stream operations whose arguments do not change from step to step
# (persistent buffers, cached descriptors, explicit stream handles) except the batch pointers, the result pointer and the
# optimizer's hyper-parameters, which live in re-usable ctypes slots.  While _REC holds a list every call (through _rec_call) and
# every stream operation (through _op) appends itself; the list is then packed into an array of p2p_replay_call records
# (include/p2pgan.h) and Pix2PixEngine._replay() re-issues the whole step with ONE call into the library -- no interpreter between
# two launches.  Same entry points, same order, same streams: results are bit-identical.  (The reference's train_step is one traced
# tf.function, pix2pix_model.py:62: its host pays one call per step too.)
_REC = [None]
_ORIG_CALL = L.call


def _rec_call(name, *args):
    """L.call while a step is being recorded: run the entry point and remember (name, arguments)"""
    fn = getattr(L.lib(), name)
    rc = fn(*args)
    if rc != 0:
        raise L.P2PError(f"{name} failed (rc={rc}): {L.lib().p2p_last_error().decode()}")
    _REC[0].append((name, args))


def _op(name, *args):
    """a stream operation (p2p_event_record / p2p_stream_wait_event with explicit stream and event handles): run it now and,
    while a step is being recorded, remember it"""
    if getattr(L.lib(), name)(*args) != 0:
        raise L.P2PError(f"{name} failed: " + L.lib().p2p_last_error().decode())
    if _REC[0] is not None:
        _REC[0].append((name, args))


class _RecDP:
    """The data-parallel communicator while a step is being recorded: every collective runs now and is remembered, with the torch
    stream it was issued under (the backend orders a collective after the work on the CURRENT stream and wait() orders the
    current stream after the collective).  A replayed step re-issues it between two segments of the recorded call list."""

    def __init__(self, dp):
        self._dp = dp

    def _remember(self, fn):
        st = torch.cuda.current_stream()

        def go():
            with torch.cuda.stream(st):
                fn()
        _REC[0].append((None, go))

    def allreduce_async(self, t):
        self._dp.allreduce_async(t)
        self._remember(lambda: self._dp.allreduce_async(t))

    def allreduce_scalar_sum(self, t):
        self._dp.allreduce_scalar_sum(t)
        self._remember(lambda: self._dp.allreduce_scalar_sum(t))
        return t

    def wait_all(self):
        self._dp.wait_all()
        self._remember(self._dp.wait_all)

    def __getattr__(self, name):
        return getattr(self._dp, name)


# (stream ordering always uses device-only events, p2p_event_*: torch.cuda.Event.record carries a system-scope release that idled
# the main stream for ~6 us after every fork, r03; the torch fallback and its switch are gone)
_EVENT_RING, _EVENT_NEXT = [], [0]
_EVENT_RING_SIZE = 512            # far more than the stream operations of one step: an event is long consumed when its turn comes again


def _ring_event():
    """the next device-only ordering event (p2p_event_create: no timing, no system fence) of a small ring"""
    i = _EVENT_NEXT[0]
    _EVENT_NEXT[0] = (i + 1) % _EVENT_RING_SIZE
    if i >= len(_EVENT_RING):
        ev = C.c_void_p()
        L.call("p2p_event_create", C.byref(ev))
        _EVENT_RING.append(ev)
    return _EVENT_RING[i]


def _raw(stream):
    return C.c_void_p(stream.cuda_stream)


def _order(after, before):
    """work issued to stream `after` from now on waits for everything issued so far on stream `before`"""
    ev = _ring_event()
    _op("p2p_event_record", ev, _raw(before))
    _op("p2p_stream_wait_event", _raw(after), ev)


class _SideStream:
    """Fork/join helper: weight-gradient GEMMs only feed Adam, so they run on a second HIP stream concurrently with
    the data-gradient chain (the critical path of the backward pass).  fork() makes the side stream wait for
    everything issued so far on the main stream; join() makes the main stream wait for the side stream."""

    def __init__(self, device, enabled):
        self.enabled = enabled and torch.device(device).type == "cuda"
        self.stream = torch.cuda.Stream(device=device) if self.enabled else None
        self.stop_event_forks = True        # (SWITCHES)
        self._pending = None

    def prefork(self):
        """in front of the call whose LAST kernel the next fork() waits for: that kernel's dispatch will signal the fork's event"""
        # (not under stream capture: a stop event is not a graph node, the captured side branch would start without its dependency)
        if self.enabled and self.stop_event_forks and not torch.cuda.is_current_stream_capturing():
            self._pending = _ring_event()
            _op("p2p_arm_stop_event", self._pending)

    def fork(self):
        if not self.enabled:
            return
        ev, self._pending = self._pending, None
        if ev is not None:
            unclaimed = C.c_int(0)
            if L.lib().p2p_disarm_stop_event(C.byref(unclaimed)) != 0:
                raise L.P2PError(L.lib().p2p_last_error().decode())
            if not unclaimed.value:         # the kernel carries the event: only the side stream has something to do
                _op("p2p_stream_wait_event", _raw(self.stream), ev)
                return
            if _REC[0] is not None:         # (a replayed step takes the same path: it must leave nothing armed either)
                _REC[0].append(("p2p_disarm_stop_event", (None,)))
        _order(self.stream, torch.cuda.current_stream())

    def run(self):
        return torch.cuda.stream(self.stream) if self.enabled else _NullCtx()

    def join(self):
        if self.enabled:
            _order(torch.cuda.current_stream(), self.stream)


class _LightEvent:
    def __init__(self, st):
        self.ev = _ring_event()
        _op("p2p_event_record", self.ev, _raw(st))

    def wait(self, st):
        _op("p2p_stream_wait_event", _raw(st), self.ev)


def _record_event():
    """a new event recorded on the current stream (replayable)"""
    return _LightEvent(torch.cuda.current_stream())


def _wait_event(ev):
    ev.wait(torch.cuda.current_stream())


class _NullCtx:
    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False


class OptimSlots:
    """One optimizer's settings as ctypes objects the entry points receive BY ADDRESS -- a recorded step reads
    them when it is replayed, so one recording serves every value: the rate, beta_1, beta_2 (c_float, p2p_adam_tick and the four
    flat Adam entry points), the schedule (p2p_lr_schedule, p2p_adam_tick_sched), the shared fields of p2p_adam_step's argument
    struct (p2p_adam_hyper: the betas and epsilon again, the clipvalue, the decay of the average) and the clipnorm threshold.
    What changes the CALL LIST -- a schedule the device evaluates, either kind of clipping -- is in `key()`, part of the
    engine's replay key.  The device buffers of the global norm exist once global_clipnorm has been set."""

    def __init__(self, device):
        self.device = device
        self.lr, self.b1, self.b2, self.eps, self.clipnorm = C.c_float(), C.c_float(), C.c_float(), C.c_float(), C.c_float()
        self.hyper, self.sched = L.AdamHyper(), L.LrSchedule()
        self.schedule = None            # the schedule object behind `sched` (None: the plain rate `lr`)
        self.partials = self.scale_dev = self.norm_dev = None
        self.parts, self.nparts = (C.c_void_p * 1)(), (C.c_int * 1)()
        self.set_learning_rate(2e-4)
        self.set("beta1", 0.5), self.set("beta2", 0.999), self.set("eps", 1e-7)        # pix2pix_model.py:28-29

    scheduled = property(lambda self: self.schedule is not None)
    clipnorm_on = property(lambda self: self.clipnorm.value > 0)
    clipvalue_on = property(lambda self: self.hyper.clipvalue > 0)
    clipped = property(lambda self: self.clipnorm_on or self.clipvalue_on)

    def key(self):
        return self.clipnorm_on, self.clipvalue_on, self.scheduled

    def set(self, name, v):
        """beta1 / beta2 / eps: the c_float slot and the struct field"""
        getattr(self, {"beta1": "b1", "beta2": "b2", "eps": "eps"}[name]).value = v
        setattr(self.hyper, name, v)

    def set_learning_rate(self, learning_rate):
        """a float, or a schedule object of schedules.py (written into the p2p_lr_schedule slot in place)"""
        from .schedules import as_schedule
        sched, on_device = as_schedule(learning_rate)
        sched.fill(self.sched)
        self.lr.value = sched(0)
        self.schedule = sched if on_device else None

    def learning_rate_at(self, step):
        """the rate of the step that follows `step` completed ones (f64 on the host, the device's formulas)"""
        return self.schedule(step) if self.schedule is not None else float(self.lr.value)

    def set_clipping(self, clipvalue=None, global_clipnorm=None):
        for name, v in (("clipvalue", clipvalue), ("global_clipnorm", global_clipnorm)):
            if v is not None and not float(v) > 0:
                raise ValueError(f"{name} must be positive, got {v}")
        if clipvalue is not None and global_clipnorm is not None:
            raise ValueError("clipvalue and global_clipnorm together: Keras versions disagree on their order; set one")
        self.hyper.clipvalue = 0.0 if clipvalue is None else float(clipvalue)
        self.clipnorm.value = 0.0 if global_clipnorm is None else float(global_clipnorm)
        if global_clipnorm is not None and self.partials is None:
            self.partials = torch.zeros(L.SUMSQ_MAX_PARTS, dtype=torch.float32, device=self.device)
            self.scale_dev = torch.ones(1, dtype=torch.float32, device=self.device)
            self.norm_dev = torch.zeros(1, dtype=torch.float32, device=self.device)


class Pix2PixEngine:
    """One generator + one discriminator + their optimizers on one GPU."""

    def __init__(self, in_ch=4, out_ch=4, head="tanh", img_size=64, dtype=L.BF16, device="cuda:0", seed=47,
                 use_mfma=True, overlap_wgrad=True):
        assert img_size % 64 == 0 and (img_size & (img_size - 1)) == 0, "IMG_SIZE must be a power of two >= 64"
        L.lib()       # fail loudly now if the HIP library is missing
        self.in_ch, self.out_ch, self.head, self.S = in_ch, out_ch, head, img_size
        self.dtype, self.device, self.use_mfma = dtype, torch.device(device), use_mfma
        self.tdt = _torch_dtype(dtype)
        if self.device.type == "cuda":
            idx = self.device.index if self.device.index is not None else torch.cuda.current_device()
            # the event ring, the raw stream query and the step recorder are process-wide and device-bound: one process drives one
            # GPU (the data-parallel design) -- a second engine on another device is refused, not mis-ordered
            if _STREAM_DEVICE[0] is not None and _STREAM_DEVICE[0] != idx and _EVENT_RING:
                raise RuntimeError(f"this process already drives cuda:{_STREAM_DEVICE[0]}; one process per GPU (got cuda:{idx})")
            _STREAM_DEVICE[0] = idx
        self.G = ParamStore(generator_param_shapes(in_ch, out_ch), self.device)
        self.D = ParamStore(discriminator_param_shapes(in_ch), self.device)
        # one allocation [G gradients | D gradients | 16 loss slots]: under data parallelism the generator's small-tensor
        # tail, the whole discriminator gradient and the loss scalars leave in ONE all-reduce at the end of the step
        self._grad_all = torch.zeros(self.G.numel + self.D.numel + 16, dtype=torch.float32, device=self.device)
        self.G.grads = self._grad_all[:self.G.numel]
        self.D.grads = self._grad_all[self.G.numel:self.G.numel + self.D.numel]
        self.rng = np.random.default_rng(seed)
        self._slot_seed = C.c_longlong()
        self.seed = int(seed)
        self.mask_counter_dev = torch.zeros(1, dtype=torch.int64, device=self.device)    # advanced once per step on the device
        self._init_params()
        self.c6_ch = pad8(UP_FILTERS[5] + in_ch)          # [up6 32 | source | zero pad]
        self.src_ch = pad8(in_ch)
        self.dcat_ch = pad8(2 * in_ch)
        self.dz_ch = pad8(out_ch)
        self.W = {}
        self._alloc_weight_copies()
        self.plans = {}
        # Adam's hyper-parameters and the dropout seed live in ctypes slots (properties below): the entry points receive the slot
        # object, ctypes -- and a replayed step -- read it when the call is issued, so ONE recorded step serves every value of a
        # learning-rate schedule
        # learning-rate schedule.  Each network's optimizer has its own set (OptimSlots); the properties
        # lr / beta1 / beta2 / adam_eps below set both and read the generator's
        self.G.opt, self.D.opt = OptimSlots(self.device), OptimSlots(self.device)
        # moving average of the generator's masters (enable_ema): G.ema is None while it is off.  The decay
        # is a slot like lr; the warm-up flag travels by value and is part of the replay key
        self._slot_ema, self._ema_warmup = C.c_float(), 1
        self.ema_decay = 0.999
        self._ema_syncs = 0             # times G.ema was written from outside an optimizer step
        self._ema_G = self._ema_W = self._ema_table = self._ema_prepped = None      # the averaged operand copies (averaged())
        self._averaged = False          # inside averaged(): self.G / self.W are the averaged set
        self.losses =self._grad_all[self.G.numel + self.D.numel:]
        # per-workgroup partials of the loss kernels (include/p2pgan.h P2P_LOSS_BLOCKS): rows 0..2 BCE, row 3 L1 -- the
        # order of the loss slots, so one p2p_loss_partials_sum fills losses[0..3]; row 4 = discarded (generate())
        self.loss_part = torch.zeros(5 * 256, dtype=torch.float32, device=self.device)
        self.step_count = 0
        self._ticked = False
        self._adam_head_ev = None
        self.side = _SideStream(self.device, overlap_wgrad)
        self.side_hist = _SideStream(self.device, overlap_wgrad)     # third stream: histogram-loss chain
        self._dp = None             # parallel.DataParallel of the step in flight
        self._batch_offset = 0      # samples of the global batch in front of this rank's shard (keys the dropout stream)
        for attr, env, default, parse in SWITCHES + GATES:
            text = os.environ.get(env) if env else None
            obj, name = _switch_holder(self, attr)
            setattr(obj, name, default if text is None else parse(text))
        self.batch_invariant = self.batch_invariant and dtype == L.F32
        self._prep_table, self._adam_tables = {}, {}
        self._head_prepped = False
        # tape calls (tape.py): arenas of activations per call, pooled by (network, images) once a tape is released; the
        # workspaces they share per image count; the op-P copy of G.down1, prepared only when a tape needs d(source)
        self._arena_pool, self._tape_ws = {}, {}
        self._copies_version = 0
        self._down1_wn, self._down1_wn_key = None, None
        self.tape_refusal = None        # set by a model whose configuration has no tape path (data parallelism)
        self._replays, self._replay_seen = OrderedDict(), {}
        self._replay_fn = L.lib().p2p_replay
        self._slot_src, self._slot_real, self._slot_out = C.c_void_p(), C.c_void_p(), C.c_void_p()
        self._real_view = L.Tensor(None, 0, 0, 4)
        self._dead = next((i for i in range(2, len(DOWN_FILTERS) + 1) if img_size // 2 ** i == 1), None)
        self._frozen = None             # element range of the dead block's kernel in the generator's flat buffers
        if self._dead is not None:
            o = self.G.offsets[f"down{self._dead}.kernel"]
            self._frozen = (o, o + int(np.prod(self.G.shapes[f"down{self._dead}.kernel"])))
        self._frozen_ok = None          # its gradient and Adam moments are all 0 (None: not looked at since the last outside write)
        self._elide = 0                 # the level in force: non-zero only inside a fused train step
        self.refresh_weight_copies()

    def _slot_property(slot):
        def get(self):
            return getattr(self, slot).value

        def put(self, v):
            getattr(self, slot).value = v
        return property(get, put)

    seed = _slot_property("_slot_seed")
    del _slot_property

    def _both_property(name):
        """a hyper-parameter of both optimizers: reads the generator's, sets both (a store's own: store.opt)"""
        def get(self):
            return self.G.opt.learning_rate_at(self.G.t) if name == "lr" else getattr(self.G.opt.hyper, name)

        def put(self, v):
            for store in (self.G, self.D):
                store.opt.set_learning_rate(v) if name == "lr" else store.opt.set(name, v)
        return property(get, put)

    lr, beta1, beta2, adam_eps = _both_property("lr"), _both_property("beta1"), _both_property("beta2"), _both_property("eps")
    del _both_property

    @property
    def ema_decay(self):
        return self._slot_ema.value

    @ema_decay.setter
    def ema_decay(self, v):
        self._slot_ema.value = v                # the four flat entry points' argument
        self.G.opt.hyper.ema_decay = v          # p2p_adam_step's

    # ------------------------------------------------------------------ averaged generator
    @property
    def ema_enabled(self):
        return self.G.ema is not None

    def enable_ema(self, decay=0.999, warmup=True):
        """Keeps an exponential moving average of the generator's masters in G.ema (flat f32, the layout of G.params), starting as
        a copy of them: every optimizer step of the generator then updates it in the Adam launch itself
        (p2p_adam_ema_flat_dev[_excl]; p2p_ema_flat behind p2p_adam_prep_batched), e += (1 - beta_t) * (p' - e) with
        beta_t = min(decay, (1 + t) / (10 + t)) under warm-up, t = the generator's Adam iteration.  The discriminator has none."""
        if not 0.0 <= float(decay) < 1.0:
            raise ValueError(f"the decay of the average lies in [0, 1), got {decay}")
        self._require_live("enable_ema")
        self.ema_decay, self._ema_warmup = float(decay), int(bool(warmup))
        if self.G.ema is None:
            self.G.ema = torch.empty_like(self.G.params)
        self._sync_ema()

    def disable_ema(self):
        self._require_live("disable_ema")
        self.G.ema = None
        self._ema_G = self._ema_W = self._ema_table = self._ema_prepped = None

    def _sync_ema(self):
        """e := the masters (enabling, and every write of the masters from outside an optimizer step)"""
        self.G.ema.copy_(self.G.params)
        self._ema_syncs += 1

    def load_ema(self, values):
        """G.ema from a flat f32 tensor of its layout (a checkpoint's)"""
        if self.G.ema is None:
            raise RuntimeError("averaging is off (enable_ema)")
        self.G.ema.copy_(torch.as_tensor(values, dtype=torch.float32).reshape(-1))
        self._ema_syncs += 1

    def _require_live(self, what):
        if self._averaged:
            raise RuntimeError(f"{what} inside engine.averaged(): the context only serves generate / generate_indexed / a plain "
                               f"generator call; leave it before training or writing weights")

    def _prepare_averaged(self):
        """The averaged generator's parameter view and operand copies: a second ParamStore view whose `params` is G.ema, a second
        wn / wt / wd set per generator layer and the p2p_prep_task table that derives them -- built on first use, refreshed by one
        p2p_weight_prep_batched launch when G.ema has changed since (every optimizer step of the generator advances G.t)."""
        import copy
        if self._ema_G is None or self._ema_G.params is not self.G.ema:
            self._ema_G = copy.copy(self.G)
            self._ema_G.params = self.G.ema
            tdt, dev = self.tdt, self.device
            self._ema_W = dict(self.W)
            for (sid, name), lw in self.W.items():
                if sid != "G":
                    continue
                aw = LayerW(lw.cg, lw.cd, lw.hi_pad, lw.lo_pad, lw.need_g, lw.need_p)
                for kind in ("wt", "wn", "wd"):
                    t = getattr(lw, kind)
                    if t is not None:
                        setattr(aw, kind, torch.zeros(t.numel(), dtype=tdt, device=dev))
                self._ema_W[(sid, name)] = aw
            live = self.G, self.W
            self.G, self.W = self._ema_G, self._ema_W
            try:
                self._ema_table = self._task_table([s for sid, name in self.W if sid == "G" for s in self._copy_sets(sid, name)])
            finally:
                self.G, self.W = live
            self._ema_prepped = None
        version = (self.G.t, self._ema_syncs)
        if self._ema_prepped != version:
            raw, ntasks, total = self._ema_table
            if ntasks:
                L.call("p2p_weight_prep_batched", self.dtype, _p(raw), ntasks, total, _stream())
            self._ema_prepped = version

    def averaged(self):
        """Context manager: inside, generate / generate_indexed / a plain generator(source, training=True) call run on the averaged
        weights G.ema (kernels from their own operand copies; gamma, beta, bias and the f32 mode's master-as-operand from G.ema).
        Train steps, tape calls and writes of the weights raise RuntimeError inside.  Leaving restores the live set, also after an
        exception; the recorded steps hold the live buffers' addresses and never see the context."""
        import contextlib

        @contextlib.contextmanager
        def ctx():
            if self.G.ema is None:
                raise RuntimeError("averaging is off (enable_ema)")
            if self._averaged:          # nested: already there
                yield self
                return
            self._prepare_averaged()
            live = self.G, self.W
            self.G, self.W, self._averaged = self._ema_G, self._ema_W, True
            try:
                yield self
            finally:
                (self.G, self.W), self._averaged = live, False
        return ctx()

    def _adam_flat(self, store, grads, lo, hi, ex=None):
        """One flat Adam launch over the elements [lo, hi) of a store (ex: a hole, absolute elements), the generator's with its
        moving average folded in while averaging is on: the same launch count either way."""
        opt = store.opt
        bufs = (_p(store.params, lo), _p(grads, lo), _p(store.m, lo), _p(store.v, lo))
        if opt.clipped:
            # gradient clipping: the struct form of the launch, the scale p2p_clip_scale left on the device
            ema = store is self.G and store.ema is not None
            a = L.AdamArgs(bufs[0].value, bufs[1].value, bufs[2].value, bufs[3].value, _p(store.ema, lo).value if ema else None,
                           hi - lo, ex[0] - lo if ex else 0, ex[1] - lo if ex else 0, store.lr_t_dev.data_ptr(),
                           opt.scale_dev.data_ptr() if opt.clipnorm_on else None, store.t_dev.data_ptr(),
                           C.pointer(opt.hyper), self._ema_warmup if ema else 0, 0)
            L.call("p2p_adam_step", C.byref(a), _stream())
            return
        hyper = (_p(store.lr_t_dev), opt.b1, opt.b2, opt.eps, 1.0)
        if store is self.G and store.ema is not None:
            ema = (_p(store.t_dev), self._slot_ema, self._ema_warmup)
            if ex is None:
                L.call("p2p_adam_ema_flat_dev", *bufs, _p(store.ema, lo), hi - lo, *hyper, *ema, _stream())
            else:
                L.call("p2p_adam_ema_flat_dev_excl", *bufs, _p(store.ema, lo), hi - lo, ex[0] - lo, ex[1] - lo, *hyper, *ema, _stream())
        elif ex is None:
            L.call("p2p_adam_flat_dev", *bufs, hi - lo, *hyper, _stream())
        else:
            L.call("p2p_adam_flat_dev_excl", *bufs, hi - lo, ex[0] - lo, ex[1] - lo, *hyper, _stream())

    def _adam_tick(self, store):
        """t_dev += 1 and the bias-corrected step size of this step, the rate from the store's schedule where the device has one to
        evaluate (p2p_adam_tick_sched reads the step number on the device: a recorded or captured step follows the schedule)"""
        opt = store.opt
        if opt.scheduled:
            L.call("p2p_adam_tick_sched", _p(store.t_dev), _p(store.lr_t_dev), C.byref(opt.sched), opt.b1, opt.b2, _stream())
        else:
            L.call("p2p_adam_tick", _p(store.t_dev), _p(store.lr_t_dev), opt.lr, opt.b1, opt.b2, _stream())

    def _clip_scale(self, store, grads):
        """global_clipnorm: the L2 norm of the store's whole flat gradient (final by now: behind the weight-gradient stream's join
        and, data parallel, behind the all-reduce -- every rank sums the same values in the same order and gets the same scale,
        no collective) and the scale the store's Adam launches multiply by.  Two launches; the dead bottleneck's kernel is a hole
        where the step elides it."""
        opt = store.opt
        if not opt.clipnorm_on:
            return
        ex = self._frozen if (self._elide >= 2 and store is self.G) else (0, 0)
        opt.parts[0] = opt.partials.data_ptr()
        L.call("p2p_sumsq_partials", _p(grads), store.numel, ex[0], ex[1], _p(opt.partials), opt.nparts, _stream())
        L.call("p2p_clip_scale", opt.parts, opt.nparts, 1, opt.clipnorm, _p(opt.scale_dev), _p(opt.norm_dev), _stream())

    def set_optimizer(self, store, learning_rate=None, beta1=None, beta2=None, eps=None, clipping=None):
        """One optimizer's settings (store: self.G or self.D); None leaves a setting alone.  learning_rate: a float or a schedule of
        schedules.py; clipping: (clipvalue or None, global_clipnorm or None).  Values are slots and take effect at the next step,
        recorded or not; what changes the call list (clipping on / off, a schedule for the device) keys a recording of its own."""
        opt = store.opt
        if learning_rate is not None:
            opt.set_learning_rate(learning_rate)
        for name, v in (("beta1", beta1), ("beta2", beta2), ("eps", eps)):
            if v is not None:
                opt.set(name, v)
        if clipping is not None:
            if self.fuse_adam and any(c is not None for c in clipping):
                raise ValueError("gradient clipping with fuse_adam=True: p2p_adam_prep_batched takes no gradient scale")
            opt.set_clipping(*clipping)

    # ------------------------------------------------------------------ parameters
    def _init_params(self):
        """tf.random_normal_initializer(0., 0.02) kernels, zero biases, gamma=1, beta=0 (networks.py:7,24,40,54)."""
        for store in (self.G, self.D):
            vals = {}
            for k, s in store.shapes.items():
                if k.endswith(".kernel"):
                    vals[k] = self.rng.normal(0.0, 0.02, size=s).astype(np.float32)
                elif k.endswith(".gamma"):
                    vals[k] = np.ones(s, np.float32)
                else:
                    vals[k] = np.zeros(s, np.float32)
            store.load(vals)

    def _store(self, sid):
        return self.G if sid == "G" else self.D

    def _alloc_weight_copies(self):
        dev, tdt = self.device, self.tdt
        for sid, store in (("G", self.G), ("D", self.D)):
            for key in store.shapes:
                if not key.endswith(".kernel"):
                    continue
                name = key[:-7]
                _, _, cg, cd = store.shapes[key]
                hi_pad, lo_pad, need_p = cg, cd, True
                if (sid, name) == ("G", "down1"):
                    hi_pad, need_p = self.src_ch, False            # no data gradient wrt the source image
                elif (sid, name) == ("G", "last"):
                    hi_pad, lo_pad = self.c6_ch, self.dz_ch
                elif (sid, name) == ("D", "down"):
                    hi_pad = self.dcat_ch
                elif (sid, name) == ("D", "last"):
                    lo_pad = 8                                     # dlogits are stored with 8-channel pixels
                lw = LayerW(cg, cd, hi_pad, lo_pad, True, need_p)
                if self.use_mfma:
                    lw.wt = torch.zeros(16 * up32(cd) * hi_pad, dtype=tdt, device=dev)
                    if need_p and not (lw.main and self.dtype == L.F32):   # f32 main layers: the master IS wn
                        lw.wn = torch.zeros(16 * up32(cg) * lo_pad, dtype=tdt, device=dev)
                if (not self.use_mfma or not lw.main) and self.dtype != L.F32:
                    lw.wd = torch.zeros(16 * cg * cd, dtype=tdt, device=dev)
                self.W[(sid, name)] = lw

    def _in_head(self, sid, name):
        """the layer's kernel lies in front of the last gradient bucket: what _adam_head updates early"""
        lw = self.W[(sid, name)]
        head_end = self.G.buckets[-1][0] if len(self.G.buckets) >= 2 else 0
        return sid == "G" and self.G.offsets[name + ".kernel"] + 16 * lw.cg * lw.cd <= head_end

    def _copy_sets(self, sid, name):
        """a layer's weight copy sets (master, cg, cd, wn, wn rows, wn columns, wt, wt rows, wt columns): the padded operand pair
        of the MFMA kernels, then the unpadded copy of the direct kernels"""
        lw = self.W[(sid, name)]
        master = self._store(sid).p(name + ".kernel")
        sets = []
        if lw.wt is not None or lw.wn is not None:
            sets.append((master, lw.cg, lw.cd, lw.wn, up32(lw.cg), lw.lo_pad, lw.wt, up32(lw.cd), lw.hi_pad))
        if lw.wd is not None:
            sets.append((master, lw.cg, lw.cd, lw.wd, lw.cg, lw.cd, None, 0, 0))
        return sets

    def _task_table(self, specs):
        """copy sets -> device table of p2p_prep_task descriptors (raw bytes, ntasks, total blocks)"""
        if not specs:
            return None, 0, 0
        tasks = (L.PrepTask * len(specs))()
        first = 0
        for k, (master, cg, cd, wn, wn_r, wn_c, wt, wt_r, wt_c) in enumerate(specs):
            tg, td = C.c_int(0), C.c_int(0)
            nb = L.lib().p2p_weight_prep_task_blocks(cg, cd, wn_r, wn_c, wt_r, wt_c, int(wn is not None), int(wt is not None),
                                                     C.byref(tg), C.byref(td))
            t = tasks[k]
            t.w = master.value
            t.wn = wn.data_ptr() if wn is not None else None
            t.wt = wt.data_ptr() if wt is not None else None
            t.Cg, t.Cd, t.wn_rows, t.wn_cols, t.wt_rows, t.wt_cols = cg, cd, wn_r, wn_c, wt_r, wt_c
            t.tiles_g, t.tiles_d, t.first_block = tg.value, td.value, first
            first += nb
        return torch.frombuffer(bytearray(bytes(tasks)), dtype=torch.uint8).to(self.device), len(specs), first

    def _prep_tasks(self, part="all", live=False):
        """Device table of p2p_prep_task descriptors (one per weight copy set); the pointers are stable for the life
        of the engine, so it is built once.  part = "head": the generator layers whose parameters lie in front of the last
        gradient bucket (what _adam_head updates early), "rest": the others, "all": every layer, "G" / "D": one network's
        layers (the per-network optimizer step, apply_adam_store).  live: without the dead bottleneck's kernel (its master does
        not move inside a fused step; every outside writer refreshes the complete table)."""
        key = (part, "live") if live else part
        if self._prep_table.get(key) is None:
            specs = []
            for sid, name in self.W:
                in_head = self._in_head(sid, name)
                if (part == "head" and not in_head) or (part == "rest" and in_head) or (part in ("G", "D") and sid != part):
                    continue
                if live and (sid, name) == ("G", f"down{self._dead}"):
                    continue
                specs += self._copy_sets(sid, name)
            self._prep_table[key] = self._task_table(specs)
        return self._prep_table[key]

    def _adam_table(self, part):
        """Device task table of p2p_adam_prep_batched for one part of the parameters -- "G_head": the generator kernels in front
        of the last gradient bucket (what _adam_head updates early), "G_rest": the other generator kernels, "D": the
        discriminator's kernels -- each kernel listed ONCE with its first copy set; "extra": the remaining copy sets (the
        unpadded copies of the edge layers), refreshed by a plain p2p_weight_prep_batched afterwards.
        Returns (table tensor, ntasks, total blocks, elements)."""
        if part not in self._adam_tables:
            specs, n_elems = [], 0
            for (sid, name), lw in self.W.items():
                where = "D" if sid == "D" else ("G_head" if self._in_head(sid, name) else "G_rest")
                # (a kernel without copies still has to be updated: a task that writes none)
                sets = self._copy_sets(sid, name) or [(self._store(sid).p(name + ".kernel"), lw.cg, lw.cd, None, 0, 0, None, 0, 0)]
                if part == where:
                    specs.append(sets[0])
                    n_elems += 16 * lw.cg * lw.cd
                elif part == "extra":
                    specs += sets[1:]
            self._adam_tables[part] = self._task_table(specs) + (n_elems,)
        return self._adam_tables[part]

    def _adam_prep(self, part):
        """Keras Adam on the kernels of `part` and their operand copies in one launch (p2p_adam_prep_batched)."""
        raw, ntasks, total, n_elems = self._adam_table(part)
        if not ntasks:
            return
        store = self.D if part == "D" else self.G
        L.call("p2p_adam_prep_batched", self.dtype, n_elems, _p(raw), ntasks, total, _p(store.params), _p(store.grads), _p(store.m),
               _p(store.v), _p(store.lr_t_dev), store.opt.b1, store.opt.b2, store.opt.eps, _stream())

    def refresh_weight_copies(self, part="all", outside=True, optimizer_step=False):
        """Re-derives the per-layer weight copies from the f32 masters; runs after every Adam step (one launch per part).
        Everything that writes the masters from outside a train step (construction, set_params / set_weights, loading weights or a
        checkpoint) ends here with outside=True: every copy is refreshed, the dead bottleneck's included, and the next fused step
        looks at that kernel's Adam state again (_elision).  Inside a fused step that elides the block its copies are left alone.
        Code that writes G.params / G.m / G.v / G.grads directly must end here too: the engine cannot see such a write.
        With averaging on, an outside write also restarts the average from the new masters (G.ema := G.params) -- unless it is
        an optimizer step of the engine's own (apply_adam_store), whose Adam launch has just updated the average."""
        self._require_live("writing weights")
        self._copies_version += 1
        if outside:
            self._frozen_ok = None
            if self.G.ema is not None and not optimizer_step:
                self._sync_ema()
        raw, ntasks, total = self._prep_tasks(part, live=bool(self._elide))
        if ntasks:
            L.call("p2p_weight_prep_batched", self.dtype, _p(raw), ntasks, total, _stream())

    def _wn(self, sid, name):
        lw = self.W[(sid, name)]
        return _p(lw.wn) if lw.wn is not None else self._store(sid).p(name + ".kernel")

    def _wd(self, sid, name):
        lw = self.W[(sid, name)]
        return _p(lw.wd) if lw.wd is not None else self._store(sid).p(name + ".kernel")

    def _elision(self):
        """the level of elide_dead_bottleneck a fused train step may run at now: 0 where no block normalises a 1x1 map, in the
        f32 parity mode, on the direct cross-check path and with the fused Adam (they keep every launch), and unless the dead
        kernel's gradient and Adam moments are all 0 -- Adam then leaves the kernel alone bit for bit.  (A checkpoint of a
        128x128 run has the same shapes and live moments there.)  Looked at once after every outside write of the state."""
        lvl = int(self.elide_dead_bottleneck)
        if not lvl or self._dead is None or self.batch_invariant or not self.use_mfma or self.fuse_adam:
            return 0
        if self._frozen_ok is None:
            # (three reductions and a host synchronisation, once per outside refresh.  Off a GPU -- the launch census of
            # tests/step_launches.py runs this engine on device "meta", where no value can be read -- the state counts as fresh)
            lo, hi = self._frozen
            self._frozen_ok = self.device.type != "cuda" or not any(
                bool(torch.count_nonzero(t[lo:hi])) for t in (self.G.grads, self.G.m, self.G.v))
        return lvl if self._frozen_ok else 0

    def _zero_raw(self, P, N, c):
        """a dense zero [N][c] "convolution result" of the dead bottleneck: any finite value normalises to the same output"""
        z = P.get("zraw")
        if z is None:
            z = P["zraw"] = DenseBuf(N, 1, 1, c, self.tdt, self.device)
            z.t.zero_()
        return z

    def _adam_range(self, store, lo, hi):
        """Keras Adam on the elements [lo, hi) of a store's flat buffers.  At level 2 of elide_dead_bottleneck the dead kernel is a
        hole in the launch (g = m = v = 0 there: the plain launch leaves it bit for bit as it is, and reads and writes it)."""
        ex = self._frozen if (self._elide >= 2 and store is self.G) else None
        if ex is not None and lo <= ex[0] and ex[1] <= hi:
            self._adam_flat(store, store.grads, lo, hi, ex)
            return
        assert ex is None or ex[1] <= lo or hi <= ex[0], "the dead kernel straddles an Adam range"
        self._adam_flat(store, store.grads, lo, hi)

    def set_params(self, g_values=None, d_values=None):
        self._require_live("set_params")
        if g_values is not None:
            self.G.load(g_values)
        if d_values is not None:
            self.D.load(d_values)
        self.refresh_weight_copies()

    # ------------------------------------------------------------------ buffers
    def plan(self, B):
        if B in self.plans:
            return self.plans[B]
        P = {"B": B}
        self._alloc_generator(P, B)
        self._alloc_discriminator(P, 2 * B, B)
        self._alloc_workspaces(P, B)
        self.plans[B] = P
        return P

    def _alloc_generator(self, P, B):
        """the generator's activations, gradient sources and norm partials for B images"""
        S, dt, dev, tdt = self.S, self.dtype, self.device, self.tdt
        # concat buffers c1..c6: [up_k output | skip]   (networks.py:92-94); c6 = [up6 | source | zero pad]
        skips = list(reversed(DOWN_FILTERS[:-1])) + [self.in_ch]
        P["c"] = [None]
        for k in range(1, 7):
            res = S // 64 * (2 ** k)
            ch = UP_FILTERS[k - 1] + skips[k - 1] if k < 6 else self.c6_ch
            P["c"].append(HaloBuf(B, res, res, ch, dt, dev))
        r6 = S // 64
        P["a6"] = HaloBuf(B, r6, r6, 512, dt, dev)
        P["src"] = HaloBuf(B, S, S, self.src_ch, dt, dev)        # down1's input, 16-byte pixels
        # raw conv outputs, stats, dropout masks, d(raw)
        P["rd"], P["ru"], P["sd"], P["su"], P["dd"], P["du"], P["mask"] = {}, {}, {}, {}, {}, {}, {}
        for i, f in enumerate(DOWN_FILTERS, start=1):
            res = S // (2 ** i)
            if i > 1 or not self.use_mfma:
                P["rd"][i] = DenseBuf(B, res, res, f, tdt, dev)
            P["dd"][i] = HaloBuf(B, res, res, f, dt, dev)
            if i > 1:
                P["sd"][i] = torch.empty((B, f, 2), dtype=torch.float32, device=dev)
        for i, f in enumerate(UP_FILTERS, start=1):
            res = S // 64 * (2 ** i)
            P["ru"][i] = DenseBuf(B, res, res, f, tdt, dev)
            P["du"][i] = HaloBuf(B, res, res, f, dt, dev)
            P["su"][i] = torch.empty((B, f, 2), dtype=torch.float32, device=dev)
            if UP_DROPOUT[i - 1]:
                P["mask"][i] = torch.empty((B * res * res, f), dtype=torch.uint8, device=dev)
        # gradient sources: d(concat_k) for k=1..6, d(a_k) from the down path
        # d(concat k).  The source channels of concat 6 have no gradient: its buffer holds up6's 32 channels only, so the head's data
        # gradient stores whole 64-byte pixels (in a 40-channel pixel they straddle 32-byte sectors: partial writes and reads)
        P["gc"] = [None] + [DenseBuf(B, P["c"][k].h, P["c"][k].w,
                                     UP_FILTERS[5] if (k == 6 and self.full_pixels and self.use_mfma) else P["c"][k].c, tdt, dev)
                            for k in range(1, 7)]      # (the direct cross-check kernels write every input channel)
        P["ga"] = {i: DenseBuf(B, S // 2 ** i, S // 2 ** i, DOWN_FILTERS[i - 1], tdt, dev) for i in range(1, 7)}
        # dgamma/dbeta per-image partials of every InstanceNorm layer + the task table of the one batched
        # reduction that ends the backward pass: rows = {part_off, rows, cols, out_off}
        P["part_off"], tasks, off = {}, [], 0
        for name in [k[:-6] for k in self.G.shapes if k.endswith(".gamma")]:
            cch = self.G.shapes[name + ".gamma"][0]
            P["part_off"][name] = (off, off + B * cch)              # (dbeta partials, dgamma partials)
            tasks.append([off, B, cch, self.G.offsets[name + ".beta"]])
            tasks.append([off + B * cch, B, cch, self.G.offsets[name + ".gamma"]])
            off += 2 * B * cch
        P["part"] = torch.empty(off, dtype=torch.float32, device=dev)
        P["part_tasks"] = torch.tensor(tasks, dtype=torch.int32, device=dev)
        P["part_maxc"] = max(t[2] for t in tasks)
        # generator head
        P["z"] = DenseBuf(B, S, S, self.out_ch, tdt, dev)
        P["dz"] = HaloBuf(B, S, S, self.dz_ch, dt, dev)

    def _alloc_discriminator(self, P, N, B=None):
        """the discriminator's buffers for N images.  B given: the train step's layout, N = 2B -- images [0,B) = [real | source],
        [B,2B) = [fake | source] (networks.py:45) -- plus the generator path's own buffers of B images; B=None: one standalone
        call on N images (a tape call, tape.py)"""
        S, dt, dev, tdt = self.S, self.dtype, self.device, self.tdt
        h2 = S // 2
        P["dcat"] = HaloBuf(N, S, S, self.dcat_ch, dt, dev)
        P["d_act"] = HaloBuf(N, h2, h2, 64, dt, dev)
        P["logits"] = DenseBuf(N, h2, h2, 1, tdt, dev)
        P["dld"] = HaloBuf(N, h2, h2, 8, dt, dev)
        if B is not None:
            P["dlg"] = HaloBuf(B, h2, h2, 8, dt, dev)
        P["g_dact"] = DenseBuf(N, h2, h2, 64, tdt, dev)
        P["d_draw"] = HaloBuf(N, h2, h2, 64, dt, dev)
        if B is not None:
            P["d_draw_g"] = HaloBuf(B, h2, h2, 64, dt, dev)      # generator path: own buffer (D.down's wgrad may still read d_draw)
            P["g_dact_g"] = DenseBuf(B, h2, h2, 64, tdt, dev)
        # d(D.first)/d(fake): only the image's channels carry a gradient; with 4 of them the buffer is dense 4-channel pixels, so the
        # kernel that writes them stores whole pixels (in an 8-channel pixel the 8 of 16 bytes are a partial sector write)
        P["g_dcat"] = DenseBuf(N if B is None else B, S, S, 4 if (self.in_ch == 4 and self.full_pixels) else self.dcat_ch, tdt, dev)
        if not self.use_mfma:
            P["d_raw"] = DenseBuf(N, h2, h2, 64, tdt, dev)

    def _alloc_workspaces(self, P, B):
        """norm, conv-epilogue, split-K and weight-gradient workspaces (their contents live for one launch or one layer)"""
        dev = self.device
        P["nws"] = torch.empty(max(B, 2) * 16 * 1024 * 2, dtype=torch.float32, device=dev)   # norm split partials [N][16][C<=1024][2]
        P["spart"] = torch.empty(4 * 1024 * 1024, dtype=torch.float32, device=dev)    # conv-epilogue statistics [N][slots][C][2]
        # split-K / wgrad workspaces
        P["slabs"] = torch.empty(self._max_slab_elems(B), dtype=torch.float32, device=dev)
        P["wws"] = torch.empty(self._max_wgrad_ws(B) // 4 + 4, dtype=torch.float32, device=dev)

    # -- heuristics for the MFMA kernels --------------------------------------------------------------
    def _splitk(self, op, B, lh, cg, cd):
        if self.batch_invariant:
            B = 256         # the K split of the benchmarked batch, whatever the batch
        ntaps = 16 if op == L.OP_G else 4
        if lh == 1:         # 1x1 maps: p2p_igemm contracts only the taps that meet real pixels (4 / 1 per phase)
            ntaps = 4 if op == L.OP_G else 1
        ncols = cd if op == L.OP_G else cg
        cc = cg if op == L.OP_G else cd
        esz = 2 if self.dtype == L.BF16 else 4
        bn = 128 if ncols % 128 == 0 else (64 if ncols % 64 == 0 else 32)
        blocks = ((B * lh * lh + 127) // 128) * (ncols // bn) * (1 if op == L.OP_G else 4)
        # measured (profiles/r05_exp_small_batch.txt, whole step): 64 is the fastest target up to batch 16, 128 at 32, 256 from 64 on
        target = self.splitk_target or (64 if B <= 16 else (128 if B <= 32 else 256))
        sk = 1
        while blocks * sk < target and sk * 2 <= ntaps and ((ntaps // (sk * 2)) * cc * esz) % 128 == 0:
            sk *= 2
        return sk

    def _msplit(self, B, lh, cg, cd):
        """Pixel-range split of the weight-gradient GEMM.  Small output tiles (edge layers: 1-2 waves per
        workgroup, 24-48 KB of LDS) are latency-bound streams over up to 1M pixels: give the chip >= 4096 waves.
        The 128-wide tiles (4 waves, 64 KB of LDS, 2 workgroups per CU) want >= 512 workgroups."""
        bg = 128 if cg > 64 else (64 if cg > 32 else 32)
        bd = 128 if cd > 64 else (64 if cd > 32 else 32)
        nw = (bg // 32) * (bd // 32)
        nw = 4 if nw >= 4 else nw
        tiles = 16 * ((cg + bg - 1) // bg) * ((cd + bd - 1) // bd)
        want = self.wgemm_want if nw == 4 else 4096 // nw
        if self.dtype == L.BF16 and cg % 128 == 0 and cd % 128 == 0 and self.wgemm_pipe and tiles <= 448:
            # the software-pipelined kernel: 8 waves and 128 KB of LDS per workgroup (one per CU), K split once more inside it
            want = self.wgemm_want_pipe
        min_chunk = 256 if nw == 4 else 1024
        m = B * lh * lh
        ms = 1
        while tiles * ms < want and m // (ms * 2) >= min_chunk:
            ms *= 2
        return ms

    def _s2_layers(self):
        """(cg, cd, lh factor) of every stride-2 block: lh = S // div for down, S // 64 * mul for up."""
        out = []
        for i in range(2, 7):
            out.append((DOWN_FILTERS[i - 2], DOWN_FILTERS[i - 1], self.S // 2 ** i))
        cin = 512
        skips = list(reversed(DOWN_FILTERS[:-1])) + [self.in_ch]
        for i in range(1, 7):
            out.append((UP_FILTERS[i - 1], cin, self.S // 64 * 2 ** (i - 1)))
            cin = UP_FILTERS[i - 1] + skips[i - 1]
        return out

    def _max_slab_elems(self, B):
        best = 4
        for cg, cd, lh in self._s2_layers():
            best = max(best, self._splitk(L.OP_G, B, lh, cg, cd) * B * lh * lh * cd)
            best = max(best, self._splitk(L.OP_P, B, lh, cg, cd) * B * 4 * lh * lh * cg)
        return best

    def _max_wgrad_ws(self, B):
        S, best = self.S, 16
        layers = self._s2_layers() + [(self.in_ch, 64, S // 2), (self.c6_ch - (self.c6_ch - 32 - self.in_ch), self.out_ch, S)]
        for cg, cd, lh in layers:
            best = max(best, self._msplit(B, lh, cg, cd) * 16 * cg * cd * 4)
        for cg, cd, lh in ((2 * self.in_ch, 64, S // 2), (64, 1, S // 2)):
            best = max(best, self._msplit(2 * B, lh, cg, cd) * 16 * cg * cd * 4)
        # LDS-resident form: partial slabs of 16*Cg*Cd floats, at most 64 MB, plus <= 64 second-level slabs of the
        # small layers (wgrad_small.hip ws_plan / ws_sum_split)
        return max(best, (68 << 20) + 16)

    # ------------------------------------------------------------------ kernel wrappers
    def _conv(self, P, op, sid, name, N, lh, in_view, out_view, stride=2, ncols=None, bias=None, act=L.ACT_NONE,
              tmp=None, want_stats=False, slab_key=None, w_p=None):
        """op G (gathers the hi view, writes lo) or op P (gathers the lo view, writes hi).  Returns (raw_kind,
        nslabs): the result is in the output view in the activation dtype (1, 1) or in f32 split-K slabs (2, nslabs):
        the shared workspace P['slabs'], or -- with `slab_key` -- a buffer of its own that stays valid until the same
        layer runs again, returned as a third element (2, nslabs, tensor).  `ncols` limits op P to the first ncols
        output channels; `w_p`: op-P operand copy of a layer that has none in self.W (G.down1, _down1_wn)."""
        lw = self.W[(sid, name)]
        cg, cd = lw.cg, lw.cd
        hi, lo = (in_view, out_view) if op == L.OP_G else (out_view, in_view)
        if self.use_mfma and lw.main and stride == 2 and bias is None and act == L.ACT_NONE and ncols is None:
            w = _p(lw.wt) if op == L.OP_G else self._wn(sid, name)
            if self.use_conv_strip and L.lib().p2p_conv_strip_ok(op, self.dtype, N, lh, lh, cg, cd):
                slots = L.lib().p2p_conv_strip_stat_slots(op, self.dtype, N, lh, lh, cg, cd) if (want_stats and not self.batch_invariant) else 0
                if N * slots * cg * 2 > P["spart"].numel():
                    slots = 0
                L.call("p2p_conv_strip", op, self.dtype, N, lh, lh, cg, cd, C.byref(hi), C.byref(lo), w,
                       _p(P["spart"]) if slots else NULL, _stream())
                return (1, 1, slots) if slots else (1, 1)
            sk = self._splitk(op, N, lh, cg, cd)
            slots = 0
            if want_stats and sk == 1 and not self.batch_invariant:      # InstanceNorm statistics fused into the GEMM epilogue
                slots = L.lib().p2p_igemm_layer_stat_slots(op, self.dtype, N, lh, lh, cg, cd)
                if N * slots * (cd if op == L.OP_G else cg) * 2 > P["spart"].numel():
                    slots = 0
            slabs = P["slabs"]
            if sk > 1 and slab_key is not None:
                need = sk * N * (lh * lh * cd if op == L.OP_G else 4 * lh * lh * cg)
                slabs = P.setdefault("own_slabs", {}).get(slab_key)
                if slabs is None or slabs.numel() < need:
                    slabs = P["own_slabs"][slab_key] = torch.empty(need, dtype=torch.float32, device=self.device)
            L.call("p2p_igemm", op, self.dtype, N, lh, lh, cg, cd, C.byref(hi), C.byref(lo), w, sk,
                   _p(slabs) if sk > 1 else NULL, _p(P["spart"]) if slots else NULL, _stream())
            if slots:
                return (1, 1, slots)
            if sk == 1:
                return (1, 1)
            return (2, sk, slabs) if slab_key is not None else (2, sk)
        if self.use_mfma:
            if op == L.OP_G:
                cin_pad, nc, rows, w = lw.hi_pad, cd, up32(cd), _p(lw.wt)
            else:
                cin_pad, nc, rows, w = lw.lo_pad, (ncols or cg), up32(cg), w_p or self._wn(sid, name)
            if self.use_conv_fewout and L.lib().p2p_conv_fewout_ok(op, stride, self.dtype, N, lh, lh, cin_pad, nc):
                entry = "p2p_conv_fewout"
            elif self.use_conv_fewin and L.lib().p2p_conv_fewin_ok(op, stride, self.dtype, N, lh, lh, cin_pad, nc):
                entry = "p2p_conv_fewin"
            else:
                entry = "p2p_igemm_edge"
            L.call(entry, op, stride, self.dtype, N, lh, lh, cin_pad, nc, rows, C.byref(in_view),
                   C.byref(out_view), w, bias if bias is not None else NULL, act, LEAKY_ALPHA, _stream())
            return (1, 1)
        # direct (non-MFMA) cross-check path
        if act != L.ACT_NONE:
            L.call("p2p_conv_direct", op, stride, self.dtype, N, lh, lh, cg, cd, C.byref(hi), C.byref(tmp.view()),
                   self._wd(sid, name), bias if bias is not None else NULL, NULL, NULL, _stream())
            L.call("p2p_norm_act_fwd", self.dtype, N, lh, lh, cd, tmp.ptr(), 1, 1, 0, NULL, NULL, IN_EPS, act,
                   LEAKY_ALPHA, NULL, C.byref(out_view), NULL, NULL, NULL, 0, 1, _stream())
        else:
            L.call("p2p_conv_direct", op, stride, self.dtype, N, lh, lh, cg, cd, C.byref(hi), C.byref(lo),
                   self._wd(sid, name), bias if bias is not None else NULL, NULL, NULL, _stream())
        return (1, 1)

    def _fused_block(self, P, op, name, N, lh, in_view, raw_buf, act, out_view, stats):
        """Convolution + InstanceNorm + activation of one generator block in one launch (p2p_igemm_norm_act) where the shape
        qualifies (bf16, workgroups that hold whole images): returns False otherwise and the caller issues the two launches."""
        lw = self.W[("G", name)]
        if not (self.use_mfma and lw.main and L.lib().p2p_igemm_norm_act_ok(op, self.dtype, N, lh, lh, lw.cg, lw.cd)):
            return False
        hi, lo = (in_view, raw_buf.view()) if op == L.OP_G else (raw_buf.view(), in_view)
        w = _p(lw.wt) if op == L.OP_G else self._wn("G", name)
        L.call("p2p_igemm_norm_act", op, self.dtype, N, lh, lh, lw.cg, lw.cd, C.byref(hi), C.byref(lo), w,
               self.G.p(name + ".gamma"), self.G.p(name + ".beta"), IN_EPS, act, LEAKY_ALPHA, C.byref(out_view), _p(stats), _stream())
        return True

    def _c6_tail(self, P):
        """True where up6's normalisation launch also writes the source channels of the last concat buffer
        (p2p_norm_act_fwd_tail: whole 80-byte pixels from one wave) and the packers leave them alone."""
        key = ("c6_tail", self.full_pixels)
        if key not in P:
            lw, S = self.W[("G", "up6")], self.S
            fused = (not UP_DROPOUT[5]) and self.use_mfma and lw.main and \
                bool(L.lib().p2p_igemm_norm_act_ok(L.OP_P, self.dtype, P["B"], S // 2, S // 2, lw.cg, lw.cd))
            P[key] = bool(self.full_pixels and not fused and self.src_ch == 8 and P["c"][6].c == UP_FILTERS[5] + 8
                                and UP_FILTERS[5] % 8 == 0 and S * S > 16)
        return P[key]

    def _wgrad(self, P, sid, name, N, lh, hi, lo, stride=2, dbias=None, dead=False):
        """dW (and dbias) of one layer, issued on the side stream: its inputs were produced on the main stream
        before this call (fork), its outputs are only read by Adam (join in _finish_step).  dead: the gradient is identically 0
        and stays as allocated (elide_dead_bottleneck) -- only what its completion triggers is issued, if anything."""
        dp = self._dp
        nb, b = len(self.G.buckets), self.G.bucket_of[name] if sid == "G" else None
        closes = sid == "G" and self.G.bucket_last_layer[b] == name         # the last kernel gradient of its bucket
        # single GPU: every weight gradient in front of the last bucket has been issued -- Adam may start on that part of the
        # flat buffer while this stream is still busy with the last layers (see _finish_step)
        head_done = dp is None and closes and self.side.enabled and nb >= 2 and b == nb - 2
        # data parallel: every kernel gradient of this bucket has been issued on this stream -- all-reduce it now, concurrently
        # with the rest of the backward pass.  The LAST bucket completes with the last weight gradient
        # of the step and sits right in front of the small-tensor tail: both leave together in _reduce_tail (one collective
        # less on the exposed end of the step)
        reduce_now = dp is not None and closes and b != nb - 1
        if dead and not (head_done or reduce_now):
            return
        self.side.fork()
        with self.side.run():
            if not dead:
                self._wgrad_impl(P, sid, name, N, lh, hi, lo, stride, dbias)
            if head_done:
                self._adam_head_ev = _record_event()
            if reduce_now:
                lo_e, hi_e = self.G.buckets[b]
                dp.allreduce_async(self.G.grads[lo_e:hi_e])

    def _wgrad_impl(self, P, sid, name, N, lh, hi, lo, stride=2, dbias=None):
        lw = self.W[(sid, name)]
        cg, cd = lw.cg, lw.cd
        dw = self._store(sid).g(name + ".kernel")
        if not self.use_mfma:
            L.call("p2p_conv_direct", L.OP_W, stride, self.dtype, N, lh, lh, cg, cd, C.byref(hi), C.byref(lo),
                   NULL, NULL, dw, dbias if dbias is not None else NULL, _stream())
            return
        if lh >= 16:      # strips of >= 16 pixels per row: contract all 16 taps out of one LDS-resident strip
            nb = L.lib().p2p_wgrad_small_blocks(self.dtype, stride, N, lh, lh, cg, cd, hi.ld, lo.ld)
            if nb > 0 and nb * 16 * cg * cd <= P["wws"].numel():
                L.call("p2p_wgrad_small", self.dtype, stride, N, lh, lh, cg, cd, C.byref(hi), C.byref(lo), dw, _p(P["wws"]), _stream())
                if dbias is not None:
                    self._colsum(P, N, lh, cd, lo, dbias)
                return
        ms = self._msplit(N, lh, cg, cd)
        ws = _p(P["wws"]) if ms > 1 else NULL
        if lw.main and stride == 2:
            L.call("p2p_wgemm", self.dtype, N, lh, lh, cg, cd, C.byref(hi), C.byref(lo), dw, ms, ws, _stream())
        else:
            L.call("p2p_wgemm_edge", self.dtype, stride, N, lh, lh, cg, cd, C.byref(hi), C.byref(lo), dw, ms, ws, _stream())
        if dbias is not None:
            self._colsum(P, N, lh, cd, lo, dbias)

    def _colsum(self, P, N, lh, cd, lo, dbias):
        """bias gradient = column sum of the layer's output gradient (deterministic: per-workgroup partials in a workspace
        of its own -- the call runs on the weight-gradient stream)"""
        need = L.lib().p2p_view_colsum_workspace_bytes(self.dtype, N, lh, lh, cd, C.byref(lo)) // 4
        key = ("cs_ws", cd)
        ws = P.get(key)
        if ws is None or ws.numel() < need:
            ws = P[key] = torch.empty(max(need, 16), dtype=torch.float32, device=self.device)
        L.call("p2p_view_colsum", self.dtype, N, lh, lh, cd, C.byref(lo), dbias, _p(ws), _stream())

    def _nsplit(self, N, res, c, bwd=False):
        """Pixel-range splits of the InstanceNorm kernels.  Measured on MI355X (B=256): the split form re-reads the
        image from HBM in its second launch, where the one-launch form re-reads it from L2, so it only pays for the
        backward kernel (three input streams) when there would be fewer than ~1024 workgroups (4 per CU)."""
        if not bwd:
            return 0x101 if self.batch_invariant else 1
        if self.batch_invariant:
            N = 256
        groups = max(1, c // 64)
        sp = 1
        while N * groups * sp < 1024 and res * res // (sp * 2) >= 64 and sp < 16:
            sp *= 2
        # | 0x100: the two-pass forms only (the register-resident ones pick their geometry, i.e. the order of the sums, by batch)
        return sp | 0x100 if self.batch_invariant else sp

    def _norm_fwd(self, P, N, res, c, raw_buf, rk, gamma, beta, act, mask, out_view, stats, tail=None):
        """tail: view whose src_ch channels are copied behind this layer's channels in out_view (see _c6_tail)"""
        raw_kind, nslabs = rk[0], rk[1]
        raw = raw_buf.ptr() if raw_kind == 1 else _p(P["slabs"])
        slab = N * res * res * c
        entry, extra = "p2p_norm_act_fwd", ()
        if tail is not None:
            entry, extra = "p2p_norm_act_fwd_tail", (C.byref(tail), self.src_ch)
        if len(rk) == 3:      # statistics already produced by the conv epilogue: apply-only pass
            L.call(entry, self.dtype, N, res, res, c, raw, 1, 1, 0, gamma, beta, IN_EPS, act, LEAKY_ALPHA,
                   _p(mask) if mask is not None else NULL, C.byref(out_view), NULL, _p(stats),
                   _p(P["spart"]), P["spart"].numel() * 4, -rk[2], *extra, _stream())
            return
        L.call(entry, self.dtype, N, res, res, c, raw, raw_kind, nslabs, slab,
               gamma if gamma is not None else NULL, beta if beta is not None else NULL, IN_EPS, act, LEAKY_ALPHA,
               _p(mask) if mask is not None else NULL, C.byref(out_view),
               raw_buf.ptr() if raw_kind == 2 else NULL, _p(stats) if stats is not None else NULL,
               _p(P["nws"]), P["nws"].numel() * 4, self._nsplit(N, res, c), *extra, _stream())

    def _gs(self, P, buf, rk, coff=0):
        """gradient source for a conv result that went to `buf` (kind 1) or to the split-K slabs (kind 2)."""
        if rk[0] == 1:
            return buf.gsrc(coff=coff, kind=1)
        slabs = rk[2] if len(rk) == 3 else P["slabs"]
        return L.GSrc(slabs.data_ptr(), 2, rk[1], buf.n * buf.h * buf.w * buf.c, buf.c, coff)

    def _norm_bwd(self, P, name, N, res, c, raw_buf, stats, act, mask, g1, g2, draw_view, fork_follows=True):
        """(every caller but the elided bottleneck forks the layer's weight gradient right behind this call: the fork rides on the
        kernel's completion)"""
        ob, og = P["part_off"][name]
        if fork_follows:
            self.side.prefork()
        L.call("p2p_norm_act_bwd", self.dtype, N, res, res, c, raw_buf.ptr(), _p(stats), self.G.p(name + ".gamma"),
               self.G.p(name + ".beta"), act, LEAKY_ALPHA, _p(mask) if mask is not None else NULL, C.byref(g1),
               C.byref(g2) if g2 is not None else None, C.byref(draw_view), _p(P["part"], og), _p(P["part"], ob),
               _p(P["nws"]), P["nws"].numel() * 4, self._nsplit(N, res, c, bwd=True), _stream())

    def _act_bwd(self, N, res, c, act_view, g1, g2, draw_view, fork_follows=False):
        if fork_follows:
            self.side.prefork()
        L.call("p2p_act_bwd", self.dtype, N, res, res, c, C.byref(act_view), C.byref(g1),
               C.byref(g2) if g2 is not None else None, LEAKY_ALPHA, C.byref(draw_view), _stream())

    # ------------------------------------------------------------------ forward
    def _to_device(self, arr, c, B, is_int=False):
        """batch element as the reference hands it over (dataset_utils.py:209-246): dense NHWC f32 or i32."""
        t = torch.as_tensor(arr)
        t = t.to(device=self.device, dtype=torch.int32 if is_int else torch.float32).contiguous()
        if tuple(t.shape) != (B, self.S, self.S, c):
            raise ValueError(f"expected batch of shape {(B, self.S, self.S, c)}, got {tuple(t.shape)}")
        return t

    def _pack(self, P, t, view, c, ptr=None):
        """dense f32 / i32 device batch -> activation-dtype (haloed, channel-sliced) view.  `ptr`: pointer slot of the batch"""
        is_int = t.dtype == torch.int32
        L.call("p2p_pack_input", self.dtype, P["B"], self.S, self.S, c, ptr or _p(t), 1 if is_int else 0, C.byref(view), _stream())

    def _pack_multi(self, P, t, views, c, ptr=None):
        arr = (L.Tensor * len(views))(*views)
        L.call("p2p_pack_input_multi", self.dtype, P["B"], self.S, self.S, c, ptr or _p(t), 1 if t.dtype == torch.int32 else 0,
               arr, len(views), _stream())

    # -- step replay (see _REC) ------------------------------------------------------------------------------------------
    REPLAY_CACHE = 8          # recorded steps kept per engine (least recently used goes first)

    def _replay_key(self, kind, B, masks, dp, apply_update, *extra):
        """key of a replayable step, or None: device RNG masks, with the optimizer step, and nobody else instrumenting L.call
        (bench.py's per-call timing).  A data-parallel step is replayable too: its collectives are remembered between the
        segments of the call list (_RecDP); the communicator object is part of the key."""
        if (masks is not None or not apply_update or B > self.replay_max_batch or self.device.type != "cuda"
                or L.call is not _ORIG_CALL or not self.replay_enabled or torch.cuda.is_current_stream_capturing()):
            return None
        # everything the recorded calls hold BY VALUE: the switches that choose kernels and K-split / grid targets (SWITCHES) and the stream
        # the step was issued on (raw handle inside the records -- the id of the torch stream object rides along, so a recycled
        # handle value of a NEW stream does not match an old recording).  Adam's hyper-parameters and the dropout seed are NOT
        # part of the key: the records hold the address of their slots (OptimSlots), one recording serves every value.  What an
        # optimizer option changes in the call list is: per network, clipnorm on, clipvalue on, a schedule for the device.
        # Averaging changes the generator's Adam entry points: None while it is off, else the warm-up flag (held by value; the
        # decay is a slot, and the kernels read the step number from G.t_dev).
        st = torch.cuda.current_stream()
        ema = None if self.G.ema is None else int(self._ema_warmup)
        return (kind, B, _SWITCH_VALUES(self), self.use_mfma, self.side.enabled, self.side_hist.enabled,
                int(st.cuda_stream), int(st.stream_id), int(self._elide), None if dp is None else id(dp), ema,
                self.G.opt.key(), self.D.opt.key()) + extra

    def _bind_batch(self, src_t, real_t):
        """the batch tensors of this step behind the re-usable pointer slots the recorded calls hold"""
        self._slot_src.value, self._slot_real.value = src_t.data_ptr(), real_t.data_ptr()
        S = self.S
        self._real_view.ptr, self._real_view.img_stride, self._real_view.row_stride, self._real_view.ld = real_t.data_ptr(), S * S, S, 4
        self._keep_alive = (src_t, real_t)

    def _new_out(self):
        out = torch.empty(8, dtype=torch.float32, device=self.device)
        self._slot_out.value = out.data_ptr()
        return out

    def _begin_record(self, key):
        """the SECOND step of a kind is recorded (the first one allocates lazily created buffers)"""
        if key is None:
            return False
        n = self._replay_seen.get(key, 0)
        if n == 0 and len(self._replay_seen) >= 8 * self.REPLAY_CACHE:
            self._replay_seen.clear()
        self._replay_seen[key] = n + 1
        if n < 1:
            return False
        _REC[0] = []
        L.call = _rec_call
        return True

    def _end_record(self, key, ok):
        rec, _REC[0] = _REC[0], None
        L.call = _ORIG_CALL
        if ok:
            # segments: runs of C-ABI calls packed for p2p_replay, separated by the host-side operations of a data-parallel
            # step (collectives through torch.distributed, _RecDP).  A single-GPU step is one segment.
            segs, run = [], []
            for name, args in rec:
                if name is None:
                    if run:
                        segs.append(pack_replay(run))
                        run = []
                    segs.append(args)
                else:
                    run.append((name, args))
            if run:
                segs.append(pack_replay(run))
            self._replays[key] = (segs, rec)            # `rec` keeps every ctypes object alive whose address the records hold
            while len(self._replays) > self.REPLAY_CACHE:
                old, _ = self._replays.popitem(last=False)
                self._replay_seen.pop(old, None)

    def _replay(self, key, P, src_t, real_t, hist=False):
        segs, _ = self._replays[key]
        self._replays.move_to_end(key)
        self._bind_batch(src_t, real_t)
        out = self._new_out()
        for seg in segs:
            if callable(seg):
                seg()
            elif self._replay_fn(seg[0], seg[1]) != 0:
                raise L.P2PError(L.lib().p2p_last_error().decode())
        self._dp = None
        self.G.t += 1
        self.D.t += 1
        self.step_count += 1
        if hist:
            P["h_real_src"] = real_t
        return out[:7]

    def _pack_source(self, P, src_t, with_disc=False):
        """the source image feeds down1, the last skip connection (networks.py:92) and, in a train step, the second half
        of both discriminator inputs (networks.py:45): one read, up to four writes"""
        ic, B = self.in_ch, P["B"]
        views = [P["src"].view()]
        if not self._c6_tail(P):
            views.append(P["c"][6].view(coff=UP_FILTERS[5]))
        if with_disc:
            views += [P["dcat"].view(coff=ic), P["dcat"].view(coff=ic, n0=B)]
        self._pack_multi(P, src_t, views, ic, ptr=self._slot_src if src_t.data_ptr() == self._slot_src.value else None)

    def _early_side(self, P, masks, apply_update):
        """The launches of a train step that depend on nothing but device counters -- the dropout keep-masks, the mask
        counter and Adam's step counters / step sizes -- go to the weight-gradient stream at the start of the step, off
        the critical path (six ~5 us kernels plus their launch gaps)."""
        self.side.fork()
        with self.side.run():
            if masks is None:
                for i, drop in enumerate(UP_DROPOUT, start=1):
                    if drop:
                        m = P["mask"][i]
                        L.call("p2p_dropout_mask_dev", _p(m), m.numel(), self._slot_seed, _p(self.mask_counter_dev), i,
                               self._batch_offset * (m.numel() // P["B"]), _stream())
            if apply_update:
                L.call("p2p_counter_add", _p(self.mask_counter_dev), 1, _stream())
                for store in (self.G, self.D):
                    self._adam_tick(store)
                self._ticked = True
            P["early_masks"] = masks is None
            P["early_ev"] = None
            if self.side.enabled:
                P["early_ev"] = _record_event()

    def generator_forward(self, P, masks=None, head=True):
        """UnetGenerator forward up to the pre-activation head output z (networks.py:80-98).  head=False stops in front of
        the head convolution (the indexed train step fuses it with the softmax, p2p_head_softmax_cce)."""
        B, S = P["B"], self.S
        c = P["c"]
        P["rk_d"], P["rk_u"] = {}, {}
        # down path: Conv2D s2 -> [InstanceNorm] -> LeakyReLU, output written into its slice of the concat buffer
        src_view = P["src"].view()
        for i, f in enumerate(DOWN_FILTERS, start=1):
            res = S // 2 ** i
            out_view = P["a6"].view() if i == 6 else c[6 - i].view(coff=UP_FILTERS[5 - i])
            if i == 1:      # no norm (networks.py:58): LeakyReLU fused in the conv epilogue
                self._conv(P, L.OP_G, "G", "down1", B, res, src_view, out_view, act=L.ACT_LEAKY, tmp=P["rd"].get(1))
            elif self._elide and i == self._dead:       # act(beta): no convolution (elide_dead_bottleneck)
                if self._elide >= 2:
                    L.call("p2p_norm_act_fwd_1x1", self.dtype, B, f, self.G.p(f"down{i}.gamma"), self.G.p(f"down{i}.beta"),
                           L.ACT_LEAKY, LEAKY_ALPHA, NULL, C.byref(out_view), _stream())
                else:
                    self._norm_fwd(P, B, res, f, self._zero_raw(P, B, f), (1, 1), self.G.p(f"down{i}.gamma"),
                                   self.G.p(f"down{i}.beta"), L.ACT_LEAKY, None, out_view, P["sd"][i])
            elif self._fused_block(P, L.OP_G, f"down{i}", B, res, src_view, P["rd"][i], L.ACT_LEAKY, out_view, P["sd"][i]):
                pass
            else:
                rk = self._conv(P, L.OP_G, "G", f"down{i}", B, res, src_view, P["rd"][i].view(), want_stats=True)
                self._norm_fwd(P, B, res, f, P["rd"][i], rk, self.G.p(f"down{i}.gamma"), self.G.p(f"down{i}.beta"),
                               L.ACT_LEAKY, None, out_view, P["sd"][i])
            src_view = out_view
        # up path: Conv2DTranspose s2 -> InstanceNorm -> [Dropout] -> ReLU -> first slice of the concat buffer
        lo_view = P["a6"].view()
        for i, f in enumerate(UP_FILTERS, start=1):
            lh = S // 64 * 2 ** (i - 1)
            if not UP_DROPOUT[i - 1] and self._fused_block(P, L.OP_P, f"up{i}", B, lh, lo_view, P["ru"][i], L.ACT_RELU,
                                                           c[i].view(coff=0), P["su"][i]):
                lo_view = c[i].view()
                continue
            rk = self._conv(P, L.OP_P, "G", f"up{i}", B, lh, lo_view, P["ru"][i].view(), want_stats=True)
            mask = None
            if UP_DROPOUT[i - 1]:
                mask = P["mask"][i]
                if masks is not None:
                    mask.copy_(torch.as_tensor(masks[i - 1]).reshape(mask.shape).to(torch.uint8))
                elif P.get("early_masks"):      # generated on the side stream at the start of the step
                    if P.get("early_ev") is not None:
                        _wait_event(P["early_ev"])
                        P["early_ev"] = None
                else:       # Bernoulli(0.5) keep mask (networks.py:31-32), counter-based device RNG
                    L.call("p2p_dropout_mask_dev", _p(mask), mask.numel(), self._slot_seed, _p(self.mask_counter_dev), i,
                           self._batch_offset * (mask.numel() // B), _stream())
            self._norm_fwd(P, B, 2 * lh, f, P["ru"][i], rk, self.G.p(f"up{i}.gamma"), self.G.p(f"up{i}.beta"),
                           L.ACT_RELU, mask, c[i].view(coff=0), P["su"][i],
                           tail=P["src"].view() if i == 6 and self._c6_tail(P) else None)
            lo_view = c[i].view()
        # head: Conv2D(out, 4, stride 1, SAME, bias) (networks.py:75-78)
        if head:
            self._conv(P, L.OP_G, "G", "last", B, S, c[6].view(), P["z"].view(), stride=1, bias=self.G.p("last.bias"))
        P["early_masks"] = False

    def discriminator_forward(self, P, N2):
        """PatchDiscriminator on the first N2 images of dcat (networks.py:45-48)."""
        h2 = self.S // 2
        self._conv(P, L.OP_G, "D", "down", N2, h2, P["dcat"].view(), P["d_act"].view(), act=L.ACT_LEAKY, tmp=P.get("d_raw"))
        self._conv(P, L.OP_G, "D", "last", N2, h2, P["d_act"].view(), P["logits"].view(), stride=1, bias=self.D.p("last.bias"))

    def discriminator_backward(self, P, B):
        """d(D loss)/d(D weights) (pix2pix_model.py:79), then the generator's adversarial gradient through D with the
        same (pre-update) D weights down to d(fake) in g_dcat[..., :in_ch] (pix2pix_model.py:78)."""
        S, ic, h2 = self.S, self.in_ch, self.S // 2
        self._wgrad(P, "D", "last", 2 * B, h2, P["d_act"].view(), P["dld"].view(), stride=1, dbias=self.D.g("last.bias"))
        if not self._d_last_dgrad_gated(2 * B, h2, P["dld"].view(), P["d_act"].view(), P["d_draw"].view()):
            self._conv(P, L.OP_P, "D", "last", 2 * B, h2, P["dld"].view(), P["g_dact"].view(), stride=1)
            self._act_bwd(2 * B, h2, 64, P["d_act"].view(), P["g_dact"].gsrc(), None, P["d_draw"].view(), fork_follows=True)
        self._wgrad(P, "D", "down", 2 * B, h2, P["dcat"].view(), P["d_draw"].view())
        if P.get("skip_g_through_d"):
            return
        if not self._d_last_dgrad_gated(B, h2, P["dlg"].view(), P["d_act"].view(n0=B), P["d_draw_g"].view()):
            self._conv(P, L.OP_P, "D", "last", B, h2, P["dlg"].view(), P["g_dact_g"].view(), stride=1)
            self._act_bwd(B, h2, 64, P["d_act"].view(n0=B), P["g_dact_g"].gsrc(), None, P["d_draw_g"].view())
        self._conv(P, L.OP_P, "D", "down", B, h2, P["d_draw_g"].view(), P["g_dcat"].view(), ncols=ic)

    def _d_last_dgrad_gated(self, N, h2, dlogits_view, act_view, out_view):
        """d(D.last)/d(features) and the LeakyReLU backward of D.down in one launch (p2p_conv_fewin_actbwd: bit-identical to the
        two launches, the gradient tensor between them is never written); False where the few-input kernel does not apply."""
        lw = self.W[("D", "last")]
        if not (self.use_mfma and self.use_conv_fewin and self.fuse_act_bwd and
                L.lib().p2p_conv_fewin_ok(L.OP_P, 1, self.dtype, N, h2, h2, lw.lo_pad, lw.cg)):
            return False
        L.call("p2p_conv_fewin_actbwd", L.OP_P, 1, self.dtype, N, h2, h2, lw.lo_pad, lw.cg, up32(lw.cg), C.byref(dlogits_view),
               C.byref(out_view), self._wn("D", "last"), C.byref(act_view), LEAKY_ALPHA, _stream())
        return True

    def _run_step(self, kind, key_extra, P, src_t, real_t, body, masks, apply_update, hist=False):
        """One fused train step of the communicator in self._dp: replayed where a recording with its key exists, else body() is
        issued, and recorded the second time the key is seen.  The one place that puts the elision level in force and that wraps
        the communicator of a step being recorded (_RecDP): the bodies read self._dp."""
        self._require_live("a train step")
        dp = self._dp
        self._elide = self._elision()
        try:
            key = self._replay_key(kind, P["B"], masks, dp, apply_update, *key_extra)
            if key in self._replays:
                return self._replay(key, P, src_t, real_t, hist=hist)
            recording = self._begin_record(key)
            if recording and dp is not None:
                self._dp = _RecDP(dp)
            try:
                out = body()
            except BaseException:
                if recording:
                    self._end_record(key, False)
                raise
            if recording:
                self._end_record(key, True)
            return out
        finally:
            self._elide = 0         # every other path (hooked steps, tapes, generate) issues the whole network

    # ------------------------------------------------------------------ train step (RGBA models)
    def train_step_rgba(self, source, real, lambda_l1, lambda_hist=None, masks=None, global_batch=None,
                        apply_update=True, dp=None, batch_offset=0, palette=None):
        """Pix2PixModel.train_step / Pix2PixHistogramModel (pix2pix_model.py:62-89,242-250).
        Returns a device tensor [g_total, g_adv, g_l1, g_hist, d_total, d_real, d_fake] (f32).
        `palette` (build-added, not together with lambda_hist): (lambda_palette, lambda_conformance, temperature) adds
        Pix2PixPaletteModel's two loss terms to the fused step (_palette_real_early / _palette_loss); the fourth value of the
        result is then the palette loss."""
        palette = self._checked_palette_terms(palette, lambda_hist)
        B = int(source.shape[0])
        P = self.plan(B)
        Bg = global_batch or B
        self._dp, self._batch_offset = dp, int(batch_offset)
        src_t, real_t = self._to_device(source, self.in_ch, B), self._to_device(real, self.in_ch, B)
        key_extra = (float(lambda_l1), None if lambda_hist is None else float(lambda_hist), Bg, int(batch_offset))
        if palette is not None:
            key_extra += (palette,)
        return self._run_step("rgba", key_extra, P, src_t, real_t,
                              lambda: self._train_step_rgba_body(P, B, Bg, src_t, real_t, lambda_l1, lambda_hist, masks, apply_update,
                                                                 palette),
                              masks, apply_update, hist=lambda_hist is not None or palette is not None)

    def _checked_palette_terms(self, palette, lambda_hist):
        """the `palette` argument of a fused step as three floats, or None"""
        if palette is None:
            return None
        if lambda_hist is not None:
            raise ValueError("palette= and lambda_hist are mutually exclusive: a fused step carries one extra generator loss")
        if self.head != "tanh" or self.in_ch != 4 or self.out_ch != 4:
            raise ValueError("the palette loss is defined on RGBA images: a tanh head with four input and output channels")
        if len(palette) != 3:
            raise ValueError(f"palette is (lambda_palette, lambda_conformance, temperature), got {palette!r}")
        lam_pal, lam_conf, tau = (float(x) for x in palette)
        if not 0.0 < tau < float("inf"):
            raise ValueError(f"the temperature must be positive and finite, got {tau}")
        return lam_pal, lam_conf, tau

    def _train_step_rgba_body(self, P, B, Bg, src_t, real_t, lambda_l1, lambda_hist, masks, apply_update, palette=None):
        S, ic = self.S, self.in_ch
        self._bind_batch(src_t, real_t)
        whole_fake = ic == 4 and self.src_ch == 8 and self.dcat_ch == 8 and self.full_pixels and self.out_ch == 4
        if ic == 4 and self.src_ch == 8 and self.dcat_ch == 8:
            # source and target in one launch, whole 16-byte pixels (networks.py:45,92-94)
            L.call("p2p_pack_pair", self.dtype, B, S, S, self._slot_src, self._slot_real, C.byref(P["src"].view()),
                   None if self._c6_tail(P) else C.byref(P["c"][6].view(coff=UP_FILTERS[5])), C.byref(P["dcat"].view(coff=0)),
                   None if whole_fake else C.byref(P["dcat"].view(coff=0, n0=B)), _stream())
        else:
            self._pack_source(P, src_t, with_disc=True)
            self._pack(P, real_t, P["dcat"].view(coff=0), ic, ptr=self._slot_real)
        if lambda_hist is not None:
            self._hist_real_early(P, B, real_t)
        elif palette is not None:
            self._palette_real_early(P, B, real_t, palette[2])
        self._early_side(P, masks, apply_update)
        self.generator_forward(P, masks)
        real_view, fake_view = P["dcat"].view(coff=0), P["dcat"].view(coff=0, n0=B)
        inv_l1 = 1.0 / (Bg * S * S * self.out_ch)
        fake32 = NULL
        if lambda_hist is not None:
            self._hist_buffers(P, B)
            fake32 = _p(P["fake32"])
        elif palette is not None:
            fake32 = _p(P["p_fake32"])
        if whole_fake:
            # whole [fake | source] pixels (the source half comes from the real half's pixel)
            L.call("p2p_tanh_l1_fwd_pair", self.dtype, B, S, S, C.byref(P["z"].view()), C.byref(real_view), C.byref(fake_view), inv_l1,
                   _p(self.loss_part, 3 * 256), fake32, _stream())
        else:
            L.call("p2p_tanh_l1_fwd", self.dtype, B, S, S, self.out_ch, C.byref(P["z"].view()), C.byref(real_view),
                   C.byref(fake_view), inv_l1, _p(self.loss_part, 3 * 256), fake32, _stream())
        g_extra = None
        if lambda_hist is not None:
            # the histogram loss only needs `fake`: its kernels (f32 MFMA, ~1.8 ms at B=256) run on the side stream,
            # concurrently with the discriminator forward/backward, and are joined before the tanh backward
            self.side_hist.fork()
            with self.side_hist.run():
                g_extra = self._histogram_loss(P, B, Bg, lambda_hist, self._dp.allreduce_scalar_sum if self._dp is not None else None)
        elif palette is not None:
            # likewise the palette loss (vector-ALU kernels, no collective: both terms are per-image means)
            self.side_hist.fork()
            with self.side_hist.run():
                g_extra = self._palette_loss(P, B, Bg, palette)
        self.discriminator_forward(P, 2 * B)
        self._bce_logits(P, B, Bg, P["dlg"].view())
        P["skip_g_through_d"] = False
        P["head_dbias_done"] = False
        self.discriminator_backward(P, B)
        if g_extra is not None:
            self.side_hist.join()
        self._tanh_l1_bwd(P, fake_view, real_view, P["g_dcat"].gsrc(), g_extra, float(lambda_l1) * inv_l1)
        self.generator_backward(P)
        return self._finish_step(4, self._finish_args(lambda_l1, lambda_hist, palette=palette), apply_update)

    def train_step_rgba_hooked(self, source, real, generator_loss, discriminator_loss, masks=None, apply_update=True):
        """train_step (pix2pix_model.py:62-89) for a subclass that OVERRIDES the loss hooks (pix2pix_model.py:44-56,242-250 are the
        reference's own overrides; SURVEY.md B1 lists the hooks as part of the boundary).  The reference differentiates whatever the
        hooks compute with a GradientTape; here the networks are HIP kernels without a tape, but the hooks only ever see three
        tensors -- the discriminator's outputs for [real, source] and [fake, source] and the generated image -- so the tape is needed
        across the hooks alone: the kernels run forward, the hooks are evaluated on torch tensors (autograd gives d(loss)/d(logits)
        and d(loss)/d(fake)), and those gradients enter the same backward kernels the fused step uses.
          generator_loss(fake_predicted, fake_image, real_image) -> (total, adversarial, l1[, ...]);  discriminator_loss(real_predicted,
          fake_predicted) -> (total, real, fake); both written with torch operations on the tensors they are handed (f32, NHWC).
        Returns [g_total, g_adv, g_l1, g_4th or 0, d_total, d_real, d_fake].  Slower than the fused step by the hooks' own elementwise
        kernels; single GPU, not replayed (the hooks are host code)."""
        self._require_live("a train step")
        B = int(source.shape[0])
        P = self.plan(B)
        S, ic = self.S, self.in_ch
        assert self.head == "tanh", "the palette-index model has a train_step of its own"
        self._dp, self._batch_offset = None, 0
        src_t, real_t = self._to_device(source, ic, B), self._to_device(real, ic, B)
        self._bind_batch(src_t, real_t)
        self._pack_source(P, src_t, with_disc=True)
        self._pack(P, real_t, P["dcat"].view(coff=0), ic)
        self._early_side(P, masks, apply_update)
        self.generator_forward(P, masks)
        real_view, fake_view = P["dcat"].view(coff=0), P["dcat"].view(coff=0, n0=B)
        fake32 = P.get("fake32_hook")
        if fake32 is None:
            fake32 = P["fake32_hook"] = torch.empty(B * S * S * self.out_ch, dtype=torch.float32, device=self.device)
        # fake = tanh(z): the discriminator's input in the activation dtype, and the unrounded f32 copy the hooks see
        L.call("p2p_tanh_l1_fwd", self.dtype, B, S, S, self.out_ch, C.byref(P["z"].view()), C.byref(real_view), C.byref(fake_view), 0.0,
               _p(self.loss_part, 4 * 256), _p(fake32), _stream())
        self.discriminator_forward(P, 2 * B)
        d_loss, lg_d, lg_g = self._hook_discriminator(P, B, discriminator_loss)
        fake = fake32.view(B, S, S, self.out_ch).clone().requires_grad_(True)
        g_loss = generator_loss(lg_g, fake, real_t)
        g_loss[0].backward()
        self._write_dlogits(P["dld"], lg_d)
        self._write_dlogits(P["dlg"], lg_g)
        d_fake = (torch.zeros_like(fake) if fake.grad is None else fake.grad).contiguous()      # (a hook may ignore an input)
        P["hook_keep"] = (d_fake, lg_d, lg_g, fake)
        g_extra = L.GSrc(d_fake.data_ptr(), 2, 1, B * S * S * self.out_ch, self.out_ch, 0)
        P["skip_g_through_d"] = False
        P["head_dbias_done"] = False
        self.discriminator_backward(P, B)
        L.call("p2p_tanh_l1_bwd", self.dtype, B, S, S, self.out_ch, C.byref(fake_view), C.byref(real_view), C.byref(P["g_dcat"].gsrc()),
               C.byref(g_extra), 0.0, C.byref(P["dz"].view()), _stream())
        self.generator_backward(P)
        self._optimizer_tail(apply_update)
        return self._hooked_result(g_loss, d_loss)

    def _hook_discriminator(self, P, B, discriminator_loss):
        """The discriminator's loss hook of a hooked step on an f32 copy of the logits, differentiated.  Returns (d_loss, the leaf
        that carries d(loss)/d(logits), a leaf of its own with the fake half's logits for the generator's hook)."""
        h2 = self.S // 2
        logits = P["logits"].t.detach().float().view(2 * B, h2, h2, 1)
        lg_d = logits.clone().requires_grad_(True)
        d_loss = discriminator_loss(lg_d[:B], lg_d[B:])
        d_loss[0].backward()
        return d_loss, lg_d, logits[B:].clone().requires_grad_(True)

    def _write_dlogits(self, buf, lg):
        """the gradient a hook left on the logits `lg` (zero: a hook may ignore an input) into channel 0 of dld / dlg: pixels
        [g | 7 padding channels]"""
        inner = slice(HALO, HALO + self.S // 2)
        g = torch.zeros_like(lg) if lg.grad is None else lg.grad
        buf.t[:, inner, inner, 0] = g.view(lg.shape[:3]).to(self.tdt)

    def _hooked_result(self, g_loss, d_loss):
        self.step_count += 1
        vals = [g_loss[0], g_loss[1], g_loss[2], g_loss[3] if len(g_loss) > 3 else torch.zeros((), device=self.device),
                d_loss[0], d_loss[1], d_loss[2]]
        return torch.stack([v.detach().reshape(()).float() for v in vals])

    def _tanh_l1_bwd(self, P, fake_view, real_view, gsrc, extra, scale):
        """d(tanh head) into dz from the L1 term (scale), the adversarial gradient source and one more source: dz's 8-channel
        pixels [g | padding] are stored whole with full_pixels on"""
        B, S = P["B"], self.S
        args = (C.byref(fake_view), C.byref(real_view), C.byref(gsrc) if gsrc is not None else None,
                C.byref(extra) if extra is not None else None, scale, C.byref(P["dz"].view()), _stream())
        if self.full_pixels and self.out_ch == 4 and self.dz_ch == 8:
            L.call("p2p_tanh_l1_bwd_pad8", self.dtype, B, S, S, *args)
        else:
            L.call("p2p_tanh_l1_bwd", self.dtype, B, S, S, self.out_ch, *args)

    def _bce_logits(self, P, B, Bg, dlg):
        """the three BCE sums of the discriminator's logits and their gradients: dld (D's own loss) and, for the RGBA models, dlg
        (the generator's adversarial term) -- 8-channel pixels [g | padding]: whole-pixel stores with full_pixels on"""
        h2 = self.S // 2
        L.call("p2p_bce_logits_pad8" if self.full_pixels else "p2p_bce_logits", self.dtype, 2 * B, B, h2, h2,
               C.byref(P["logits"].view()), 1.0 / (Bg * h2 * h2), C.byref(P["dld"].view()), C.byref(dlg) if dlg is not None else None,
               _p(self.loss_part), _stream())

    def generator_backward(self, P):
        """Backward of UnetGenerator from dz (the gradient at the head's pre-activation)."""
        B, S = P["B"], self.S
        c, gc, ga = P["c"], P["gc"], P["ga"]
        dbias = None if P.get("head_dbias_done") else self.G.g("last.bias")      # the fused indexed head already summed it
        self._wgrad(P, "G", "last", B, S, c[6].view(), P["dz"].view(), stride=1, dbias=dbias)
        # d(concat6): only the 32 channels of up6's output are needed (the source image has no gradient)
        lw = self.W[("G", "last")]
        if (self.use_mfma and self.use_head_fused and lw.wn is not None and
                L.lib().p2p_head_dgrad_ok(self.dtype, B, S, S, lw.cd, UP_FILTERS[5], up32(lw.cg), P["dz"].c, gc[6].c)):
            # the indexed head's 256 -> 32 data gradient: strip-resident kernel of its own (K = 16 x 256, 32 outputs)
            L.call("p2p_head_dgrad", self.dtype, B, S, S, lw.cd, UP_FILTERS[5], C.byref(P["dz"].view()), _p(lw.wn), up32(lw.cg),
                   C.byref(gc[6].view()), _stream())
        else:
            self._conv(P, L.OP_P, "G", "last", B, S, P["dz"].view(), gc[6].view(), stride=1, ncols=UP_FILTERS[5])
        rk_gc = {6: (1, 1)}
        # up path, last to first
        for i in range(6, 0, -1):
            f = UP_FILTERS[i - 1]
            lh = S // 64 * 2 ** (i - 1)
            lo_buf = c[i - 1] if i > 1 else P["a6"]
            self._norm_bwd(P, f"up{i}", B, 2 * lh, f, P["ru"][i], P["su"][i], L.ACT_RELU, P["mask"].get(i),
                           self._gs(P, gc[i], rk_gc[i], 0), None, P["du"][i].view())
            self._wgrad(P, "G", f"up{i}", B, lh, P["du"][i].view(), lo_buf.view())
            out_buf = gc[i - 1] if i > 1 else ga[6]
            # split-K results stay in f32 slabs of their own: both consumers (the norm backward of up_{i-1} now, of the
            # skip partner down_{7-i} later) sum them on load -- no pass that only folds the slabs
            rk = self._conv(P, L.OP_G, "G", f"up{i}", B, lh, P["du"][i].view(), out_buf.view(), slab_key=f"up{i}.dgrad")
            if i > 1:
                rk_gc[i - 1] = rk
        # down path, last to first
        g_from_down = self._gs(P, ga[6], rk, 0)
        for i in range(6, 0, -1):
            f = DOWN_FILTERS[i - 1]
            res = S // 2 ** i
            if i == 6:
                g1, g2 = g_from_down, None
            else:
                g1 = self._gs(P, gc[6 - i], rk_gc[6 - i], UP_FILTERS[5 - i])     # skip-connection slice
                g2 = g_from_down
            if self._elide and i == self._dead:
                # only dbeta is live: d(raw) is exactly 0, so there is no weight gradient to compute (its range of the flat
                # gradient buffer has been 0 since allocation) and the block above receives its skip gradient alone
                if self._elide >= 2:
                    ob, og = P["part_off"][f"down{i}"]
                    L.call("p2p_norm_act_bwd_1x1", self.dtype, B, f, self.G.p(f"down{i}.gamma"), self.G.p(f"down{i}.beta"),
                           L.ACT_LEAKY, LEAKY_ALPHA, NULL, C.byref(g1), C.byref(g2) if g2 is not None else None,
                           _p(P["part"], og), _p(P["part"], ob), _stream())
                else:
                    self._norm_bwd(P, f"down{i}", B, res, f, self._zero_raw(P, B, f), P["sd"][i], L.ACT_LEAKY, None, g1, g2,
                                   P["dd"][i].view(), fork_follows=False)
                self._wgrad(P, "G", f"down{i}", B, res, None, None, dead=True)
                g_from_down = None
                continue
            if i > 1:
                self._norm_bwd(P, f"down{i}", B, res, f, P["rd"][i], P["sd"][i], L.ACT_LEAKY, None, g1, g2,
                               P["dd"][i].view())
                hi_view = c[7 - i].view(coff=UP_FILTERS[6 - i])
            else:
                self._act_bwd(B, res, f, c[5].view(coff=UP_FILTERS[4]), g1, g2, P["dd"][1].view(), fork_follows=True)
                hi_view = P["src"].view()
            self._wgrad(P, "G", f"down{i}", B, res, hi_view, P["dd"][i].view())
            if i > 1:
                rk = self._conv(P, L.OP_P, "G", f"down{i}", B, res, P["dd"][i].view(), ga[i - 1].view(),
                                slab_key=f"down{i}.dgrad")
                g_from_down = self._gs(P, ga[i - 1], rk, 0)
        # dgamma/dbeta sum over batch AND space: one batched reduction of every layer's
        # per-image partials into the flat gradient buffer
        self.side.fork()
        with self.side.run():       # only Adam reads these sums: off the critical path like the weight gradients
            L.call("p2p_colsum_batched", _p(P["part"]), _p(P["part_tasks"]), int(P["part_tasks"].shape[0]), P["part_maxc"],
                   _p(self.G.grads), _stream())

    def _reduce_tail(self):
        """after the backward pass: the small-tensor tail of the generator gradients (gamma/beta/bias), the whole
        discriminator gradient (36.9 KB) and the loss scalars; then wait for every bucket in flight."""
        dp = self._dp
        if dp is None:
            return
        assert self.G.buckets[-1][1] == self.G.small_range[0]
        dp.allreduce_async(self._grad_all[self.G.buckets[-1][0]:])
        dp.wait_all()
        self._dp = None

    def _optimizer_tail(self, apply_update, loss_rows=0):
        """behind the backward pass of every train step: the early part of Adam, the weight-gradient stream joined, the loss
        partials summed (fused steps: loss_rows of them) and the gradients all-reduced, then both optimizers"""
        head = self._adam_head(apply_update)
        self.side.join()
        if loss_rows:
            L.call("p2p_loss_partials_sum", _p(self.loss_part), loss_rows, _p(self.losses), _stream())
            self._reduce_tail()
        if apply_update:
            self.apply_adam(g_from=head)

    def _finish_args(self, lambda_l1, lambda_hist=None, lambda_aux=None, palette=None):
        """p2p_finish_losses' (slot of the fourth generator term or -1, slot of the L1 term, weight of L1, weight of the fourth);
        with `palette` p2p_finish_losses2' (slots of the palette, conformance and L1 terms, their three weights)"""
        if palette is not None:
            return 4, 5, 3, float(lambda_l1), palette[0], palette[1]
        if self.head == "softmax":
            # g_total = adv + 0 * l1 + lambda_seg * seg  (lambda_l1 is hard-wired to 0, pix2pix_model.py:263,273-278)
            return 5, 6, 0.0, float(lambda_aux or 0.0)
        return 4 if lambda_hist is not None else -1, 3, float(lambda_l1), float(lambda_hist) if lambda_hist is not None else 0.0

    def _finish_step(self, loss_rows, finish_args, apply_update):
        self._optimizer_tail(apply_update, loss_rows)
        return self._write_losses(finish_args)

    def _write_losses(self, finish_args):
        """the result vector of a fused step from the loss slots"""
        out = self._new_out()
        L.call("p2p_finish_losses2" if len(finish_args) == 6 else "p2p_finish_losses", _p(self.losses), *finish_args, self._slot_out,
               _stream())
        self.step_count += 1
        return out[:7]

    def train_step_empty(self, lambda_l1, lambda_hist=None, lambda_aux=None, dp=None, apply_update=True, palette=None):
        """The step of a rank whose shard of the global batch is empty (global batch smaller than the world: the ragged
        tail of an epoch, dataset_utils.py:223 has no drop_remainder): contributes zero gradients and zero loss partials,
        issues the SAME collectives in the same order as a rank with samples -- the Hellinger scalar first (histogram model),
        then the gradient buckets, then the tail with the loss slots -- and applies the same Adam update.  The palette terms
        (`palette` as for train_step_rgba) need no collective of their own: their slots are zeroed with the gradients."""
        palette = self._checked_palette_terms(palette, lambda_hist)
        self._require_live("a train step")
        self._dp = dp
        self._grad_all.zero_()
        if dp is not None:
            if lambda_hist is not None:
                if getattr(self, "_zero_scalar", None) is None:
                    self._zero_scalar = torch.zeros(1, dtype=torch.float32, device=self.device)
                self._zero_scalar.zero_()
                dp.allreduce_scalar_sum(self._zero_scalar)
            for lo_e, hi_e in self.G.buckets[:-1]:
                dp.allreduce_async(self.G.grads[lo_e:hi_e])
        self._reduce_tail()
        if apply_update:
            self.apply_adam()
        return self._write_losses(self._finish_args(lambda_l1, lambda_hist, lambda_aux, palette=palette))

    def _adam_head(self, apply_update):
        """Single-GPU steps: the main stream finishes the backward pass ~70 us before the weight-gradient stream does (the
        last layers' weight gradients are issued last).  Adam on the part of the generator's flat buffer whose gradients
        are already complete -- everything in front of the last bucket, 90 % of the parameters -- runs in that window: a
        memory-bound kernel next to the compute-bound tail of the other stream.  Returns the first element still to update.
        A generator under global_clipnorm has no early part (returns 0): its gradient scale is a function of the WHOLE gradient,
        which exists only once the last bucket and the small-tensor tail are complete (apply_adam takes the norm there), so the
        step loses this overlap.  clipvalue alone or a schedule keep it; the discriminator never had one."""
        ev, self._adam_head_ev = self._adam_head_ev, None
        if not apply_update or not self._ticked or len(self.G.buckets) < 2 or self.G.opt.clipnorm_on:
            return 0
        if self._dp is not None:
            # data parallel: the buckets in front of the last one were all-reduced asynchronously during the backward pass;
            # once those collectives are done their sums are final (the last bucket and the tail follow in _reduce_tail)
            self._dp.wait_all()
        elif ev is not None:
            _wait_event(ev)      # also orders the Adam step counters (ticked on that stream) before us
        else:
            return 0
        n = self.G.buckets[-1][0]
        if self.fuse_adam:
            self._adam_prep("G_head")          # update + operand copies in one pass over the 26 M head parameters
            self._head_prepped = True
            return n
        self._adam_range(self.G, 0, n)
        if self.split_prep:
            # their weight copies too: the data-gradient kernels that read them are done (same stream), the other stream's
            # last weight gradients do not read weight copies -- a memory-bound launch beside MFMA-bound ones instead of
            # alone at the step boundary
            self.refresh_weight_copies("head", outside=False)
            self._head_prepped = True
        return n

    def apply_adam(self, g_from=0):
        """Both optimizers step with gradients taken at the same pre-update weights (pix2pix_model.py:81-83).  `g_from`:
        first generator element not yet updated by _adam_head."""
        self._require_live("an optimizer step")
        ticked, self._ticked = self._ticked, False      # counters already advanced by _early_side of this step
        if self.fuse_adam and (self.G.opt.clipped or self.D.opt.clipped):
            raise ValueError("gradient clipping with fuse_adam=True: p2p_adam_prep_batched takes no gradient scale")
        if self.fuse_adam:
            for store in (self.G, self.D):
                store.t += 1
                if not ticked:
                    self._adam_tick(store)
            if g_from == 0:
                self._adam_prep("G_head")
            self._adam_prep("G_rest")
            self._adam_prep("D")
            for store in (self.G, self.D):       # gamma / beta / bias: the small-tensor tail of the flat buffers
                lo_e, hi_e = store.small_range
                if hi_e > lo_e:
                    L.call("p2p_adam_flat_dev", _p(store.params, lo_e), _p(store.grads, lo_e), _p(store.m, lo_e), _p(store.v, lo_e),
                           hi_e - lo_e, _p(store.lr_t_dev), store.opt.b1, store.opt.b2, store.opt.eps, 1.0, _stream())
            if self.G.ema is not None:
                # the tiled Adam kernels do not average: one pass of its own over the whole generator, behind all of them
                L.call("p2p_ema_flat", _p(self.G.ema), _p(self.G.params), self.G.numel, _p(self.G.t_dev), self._slot_ema,
                       self._ema_warmup, _stream())
            raw, ntasks, total, _ = self._adam_table("extra")
            if ntasks:
                L.call("p2p_weight_prep_batched", self.dtype, _p(raw), ntasks, total, _stream())
            if not ticked:
                L.call("p2p_counter_add", _p(self.mask_counter_dev), 1, _stream())
            self._head_prepped = False
            return
        for store in (self.G, self.D):
            store.t += 1
            if not ticked:
                self._adam_tick(store)
            self._clip_scale(store, store.grads)
            self._adam_range(store, g_from if store is self.G else 0, store.numel)
        if not ticked:
            L.call("p2p_counter_add", _p(self.mask_counter_dev), 1, _stream())
        head_done, self._head_prepped = self._head_prepped and g_from > 0, False
        self.refresh_weight_copies("rest" if head_done else "all", outside=False)

    def _histogram_loss(self, P, B, Bg, lambda_hist, hist_allreduce):
        """Pix2PixHistogramModel.generator_loss (pix2pix_model.py:242-250): Hellinger(rgbuv_hist(real), rgbuv_hist(fake)).
        Returns the gradient source lambda_hist * d(hist_loss)/d(fake) (one f32 slab).
        The loss is sqrt(sum over the GLOBAL batch)/B_global, so under data parallelism the local sum of squares is
        all-reduced between the forward and the backward kernels."""
        S = self.S
        self._hist_buffers(P, B)
        # both images are read in f32 in every mode: the real one from the f32 input batch (_hist_real_early), the fake one
        # from the unrounded copy that p2p_tanh_l1_fwd wrote (histogram.py:53-79 is f32 arithmetic)
        fake_view = L.Tensor(P["fake32"].data_ptr(), S * S, S, 4)
        assert P.get("h_real_done"), "the real histogram is taken by _hist_real_early"
        P["h_real_done"] = False
        self._hist_fwd(P, B, fake_view, P["h_fake"], points=False)
        L.call("p2p_hellinger_fwd", _p(P["h_real"]), _p(P["h_fake"]), B, _p(P["h_tot"][0]), _p(P["h_tot"][1]),
               _p(P["h_sqp"]), _p(P["h_sq"]), _stream())
        if hist_allreduce is not None:
            hist_allreduce(P["h_sq"][:1])
        # every rank holds the GLOBAL loss after the exchange; it records its B/Bg share so that the SUM all-reduce
        # of the loss scalars (like the element-mean losses) yields the global value
        L.call("p2p_hellinger_finish", _p(P["h_sq"]), (1.0 / Bg) * (B / Bg), _p(self.losses, 4), _stream())
        coef = float(lambda_hist) / (2.0 * math.sqrt(2.0) * Bg)
        L.call("p2p_rgbuv_hist_hellinger_bwd3", L.F32, B, S, S, C.byref(fake_view),
               _p(P["h_real"]), _p(P["h_fake"]), _p(P["h_tot"][0]), _p(P["h_tot"][1]), _p(P["h_sq"]), coef, _p(P["h_gh"]),
               _p(P["h_dimg"]), _stream())
        return L.GSrc(P["h_dimg"].data_ptr(), 2, 1, B * S * S * 4, 4, 0)

    def _hist_buffers(self, P, B):
        if "h_real" in P:
            return
        dev, S = self.device, self.S
        P["h_real"] = torch.empty(B * 3 * 64 * 64, dtype=torch.float32, device=dev)
        P["h_fake"] = torch.empty(B * 3 * 64 * 64, dtype=torch.float32, device=dev)
        P["h_gh"] = torch.empty(B * 3 * 64 * 64, dtype=torch.float32, device=dev)
        P["h_tot"] = torch.empty((2, B), dtype=torch.float32, device=dev)
        P["h_sq"] = torch.zeros(4, dtype=torch.float32, device=dev)
        P["h_sqp"] = torch.zeros(B, dtype=torch.float32, device=dev)      # per-image partials of the Hellinger sum
        P["h_dimg"] = torch.empty(3 * B * S * S * 4, dtype=torch.float32, device=dev)
        P["h_ws"] = torch.empty(L.lib().p2p_rgbuv_hist_fwd3_workspace_bytes(B) // 4, dtype=torch.float32, device=dev)
        P["h_points"] = torch.empty((B, self.HIST_POINT_CAP, 4), dtype=torch.float32, device=dev)
        P["h_npoints"] = torch.zeros(B, dtype=torch.int32, device=dev)
        P["fake32"] = torch.empty(B * S * S * 4, dtype=torch.float32, device=dev)      # tanh output before rounding to the activation dtype

    def _hist_real_early(self, P, B, real_t):
        """histogram of the REAL image (no dependence on the generator), read from the dense f32 input batch: issued on the
        histogram stream at the start of the step, so its f32-MFMA work overlaps the generator forward."""
        self._hist_buffers(P, B)
        S = self.S
        P["h_real_src"] = real_t           # keep the batch tensor alive until the kernel has run
        self.side_hist.fork()
        with self.side_hist.run():
            rv = self._real_view if real_t.data_ptr() == self._real_view.ptr else L.Tensor(real_t.data_ptr(), S * S, S, 4)
            self._hist_fwd(P, B, rv, P["h_real"], points=True)
        P["h_real_done"] = True

    HIST_POINT_CAP = 1024        # colour points kept per image; an image with more is contracted over its pixels

    def _hist_fwd(self, P, B, view, out, points):
        """raw RGB-uv histograms [B][3][64][64] of a dense f32 image view (histogram.py:35-81 up to the normalisation): three shared
        kernel rows per pixel with all components in one workgroup, as in the backward kernel.  points=True: the image is a palette
        sprite (the REAL image of a step) -- contract over its distinct colours.  (The per-component kernels remain in the library
        as cross-checks: tests/test_hist_indexed_gpu.py calls them directly.)"""
        S = self.S
        pts = npts = NULL
        if points:
            L.call("p2p_rgbuv_points", L.F32, B, S, S, C.byref(view), self.HIST_POINT_CAP, _p(P["h_points"]), _p(P["h_npoints"]), _stream())
            pts, npts = _p(P["h_points"]), _p(P["h_npoints"])
        L.call("p2p_rgbuv_hist_fwd3", L.F32, B, S, S, C.byref(view), pts, npts, self.HIST_POINT_CAP, _p(out), _p(P["h_ws"]), _stream())

    # -- palette loss of the fused step: Pix2PixPaletteModel.generator_loss without a torch op between two launches
    def _palette_buffers(self, P, B):
        if "p_pal" in P:
            return
        dev, S, K = self.device, self.S, MAX_PALETTE_SIZE
        P["p_pal"] = torch.zeros((B, K, 4), dtype=torch.int32, device=dev)
        P["p_sizes"] = torch.zeros(B, dtype=torch.int32, device=dev)
        P["p_hist"] = torch.empty((2, B, K), dtype=torch.float32, device=dev)       # real, fake
        P["p_conf"] = torch.empty((2, B), dtype=torch.float32, device=dev)
        P["p_ws"] = torch.empty(max(int(L.lib().p2p_soft_palette_workspace_bytes(B, S, S)) // 4, 1), dtype=torch.float32, device=dev)
        P["p_dimg"] = torch.empty(B * S * S * 4, dtype=torch.float32, device=dev)
        P["p_fake32"] = torch.empty(B * S * S * 4, dtype=torch.float32, device=dev)   # tanh output before rounding to the activation dtype

    def _palette_real_early(self, P, B, real_t, tau):
        """palette of the REAL image and its soft histogram under it (no dependence on the generator), read from the dense f32
        input batch: issued on the histogram stream at the start of the step, beside the generator forward."""
        self._palette_buffers(P, B)
        S, K = self.S, MAX_PALETTE_SIZE
        P["h_real_src"] = real_t           # keep the batch tensor alive until the kernels have run
        self.side_hist.fork()
        with self.side_hist.run():
            img = self._slot_real if real_t.data_ptr() == self._slot_real.value else _p(real_t)
            L.call("p2p_palette_extract", B, S, S, img, K, _p(P["p_pal"]), _p(P["p_sizes"]), _stream())
            L.call("p2p_soft_palette_fwd", B, S, S, img, _p(P["p_pal"]), _p(P["p_sizes"]), K, tau, _p(P["p_hist"][0]),
                   _p(P["p_conf"][0]), _p(P["p_ws"]), _stream())

    def _palette_loss(self, P, B, Bg, palette):
        """lambda_palette * TV(h_real, h_fake) + lambda_conformance * mean(conformance(fake)) under the real image's palette
        (Pix2PixPaletteModel.generator_loss).  Returns the gradient source d(both terms)/d(fake) (one f32 slab).  Both are means over
        the GLOBAL batch of per-image values: a rank writes its images' share into loss slots 4 and 5 and scales its gradient by
        1 / Bg -- no collective (unlike the Hellinger distance); an image with more than MAX_PALETTE_SIZE colours (size -1)
        contributes zero to both and to the gradient."""
        lam_pal, lam_conf, tau = palette
        S, K = self.S, MAX_PALETTE_SIZE
        fake, pal, sizes = _p(P["p_fake32"]), _p(P["p_pal"]), _p(P["p_sizes"])
        h_real, h_fake, conf_fake = _p(P["p_hist"][0]), _p(P["p_hist"][1]), _p(P["p_conf"][1])
        L.call("p2p_soft_palette_fwd", B, S, S, fake, pal, sizes, K, tau, h_fake, conf_fake, _p(P["p_ws"]), _stream())
        L.call("p2p_palette_loss", B, K, h_real, h_fake, conf_fake, sizes, 1.0 / Bg, _p(self.losses, 4), _p(self.losses, 5), _stream())
        L.call("p2p_soft_palette_tv_bwd", B, S, S, fake, pal, sizes, K, tau, h_real, h_fake, lam_pal * 0.5 / Bg, lam_conf / Bg,
               _p(P["p_dimg"]), _stream())
        return L.GSrc(P["p_dimg"].data_ptr(), 2, 1, B * S * S * 4, 4, 0)

    def rgbuv_histogram(self, image):
        """histogram.calculate_rgbuv_histogram (histogram.py:35-81) of a dense f32 (B,S,S,4) batch in [-1,1]:
        returns the normalised (B,64,64,3) f32 device tensor in the reference's layout, differentiable with respect to `image`
        (histogram.RGBuvHistogram: the loss hooks of train_step_rgba_hooked reach the generator through it)."""
        B = int(image.shape[0])
        return _histogram.rgbuv_histogram(self._to_device(image, 4, B))

    # ------------------------------------------------------------------ train step (indexed model)
    def train_step_indexed(self, source_idx, real_idx, lambda_segmentation, masks=None, global_batch=None,
                           apply_update=True, dp=None, batch_offset=0):
        """Pix2PixIndexedModel.train_step (pix2pix_model.py:295-325).  source/real: int (B,S,S,1) palette indices.
        The discriminator sees un-normalised index images and the argmax blocks every gradient from D to G, so the
        generator learns from lambda_seg * CCE only (lambda_l1 is hard-wired to 0, :263).
        Returns [g_total, g_adv, g_l1, g_seg, d_total, d_real, d_fake]."""
        assert self.head == "softmax" and self.in_ch == 1
        B = int(source_idx.shape[0])
        P = self.plan(B)
        Bg = global_batch or B
        self._dp, self._batch_offset = dp, int(batch_offset)
        src_t = self._to_device(source_idx, 1, B, is_int=True)
        real_t = self._to_device(real_idx, 1, B, is_int=True)
        return self._run_step("indexed", (float(lambda_segmentation), Bg, int(batch_offset)), P, src_t, real_t,
                              lambda: self._train_step_indexed_body(P, B, Bg, src_t, real_t, lambda_segmentation, masks, apply_update),
                              masks, apply_update)

    def _pack_indexed(self, P, B, src_t, real_t):
        S = self.S
        self._bind_batch(src_t, real_t)
        if self.full_pixels and self.in_ch == 1 and self.src_ch == 8 and self.dcat_ch == 8:
            # source and target indices in one launch, whole 16-byte pixels (networks.py:45,92-94)
            L.call("p2p_pack_pair_idx", self.dtype, B, S, S, self._slot_src, self._slot_real, C.byref(P["src"].view()),
                   None if self._c6_tail(P) else C.byref(P["c"][6].view(coff=UP_FILTERS[5])), C.byref(P["dcat"].view(coff=0)),
                   C.byref(P["dcat"].view(coff=0, n0=B)), _stream())
        else:
            self._pack_source(P, src_t, with_disc=True)
            self._pack(P, real_t, P["dcat"].view(coff=0), 1, ptr=self._slot_real)

    def _train_step_indexed_body(self, P, B, Bg, src_t, real_t, lambda_segmentation, masks, apply_update):
        S = self.S
        self._pack_indexed(P, B, src_t, real_t)
        self._early_side(P, masks, apply_update)
        fused = (self.use_mfma and self.use_head_fused and
                 L.lib().p2p_head_softmax_ok(self.dtype, B, S, S, self.c6_ch, self.out_ch))
        self.generator_forward(P, masks, head=not fused)
        real_view, fake_view = P["dcat"].view(coff=0), P["dcat"].view(coff=0, n0=B)
        inv_pix = 1.0 / (Bg * S * S)
        P["head_dbias_done"] = fused
        if fused:
            # conv + bias + softmax + CCE + argmax + gradient (+ bias gradient) in one launch: the logits are never written
            if "head_ws" not in P:
                P["head_ws"] = torch.empty(L.lib().p2p_head_softmax_workspace_bytes(B, S) // 4 + 4, dtype=torch.float32, device=self.device)
            L.call("p2p_head_softmax_cce", self.dtype, B, S, S, self.c6_ch, self.out_ch, C.byref(P["c"][6].view()),
                   _p(self.W[("G", "last")].wt), self.G.p("last.bias"), C.byref(real_view), C.byref(fake_view),
                   float(lambda_segmentation) * inv_pix, inv_pix, C.byref(P["dz"].view()), self.G.g("last.bias"),
                   _p(P["head_ws"]), _p(self.losses, 5), _stream())
        else:
            L.call("p2p_softmax_cce_argmax", self.dtype, B, S, S, self.out_ch, C.byref(P["z"].view()), C.byref(real_view),
                   C.byref(fake_view), float(lambda_segmentation) * inv_pix, inv_pix, C.byref(P["dz"].view()), NULL,
                   _p(self._softmax_part()), _p(self.losses, 5), _stream())
        self.discriminator_forward(P, 2 * B)
        self._bce_logits(P, B, Bg, None)
        P["skip_g_through_d"] = True
        self.discriminator_backward(P, B)
        self.generator_backward(P)
        return self._finish_step(3, self._finish_args(0.0, lambda_aux=lambda_segmentation), apply_update)

    def train_step_indexed_hooked(self, source_idx, real_idx, generator_loss, discriminator_loss, masks=None, apply_update=True):
        """Pix2PixIndexedModel.train_step (pix2pix_model.py:295-325) for a subclass that overrides the loss hooks (the palette-index
        counterpart of train_step_rgba_hooked).  generator_loss(fake_predicted, fake_image, real_image) is handed the discriminator's
        output for [argmax, source], the f32 softmax probabilities (B,S,S,256) and the one-hot target; discriminator_loss(real_predicted,
        fake_predicted) as in the RGBA step.  The probabilities carry their logits as `_keras_logits` (Keras caches them on a softmax
        output; pix2pix_model.CategoricalCrossentropy evaluates on them), so autograd returns d(loss)/d(probs) AND d(loss)/d(logits);
        p2p_softmax_bwd maps both to the head's pre-activation gradient.  The argmax blocks every gradient from D to G (:292,306):
        the gradient of generator_loss with respect to fake_predicted is computed and discarded.
        Unfused head, four f32 (B,S,S,256) tensors (probabilities, logits, one-hot, and the hooks' gradients): opt-in only.
        Returns [g_total, g_adv, g_l1, g_4th or 0, d_total, d_real, d_fake].  Single GPU, not replayed (the hooks are host code)."""
        assert self.head == "softmax" and self.in_ch == 1, "the RGBA models have train_step_rgba_hooked"
        self._require_live("a train step")
        B = int(source_idx.shape[0])
        P = self.plan(B)
        S, Cn = self.S, self.out_ch
        self._dp, self._batch_offset = None, 0
        src_t = self._to_device(source_idx, 1, B, is_int=True)
        real_t = self._to_device(real_idx, 1, B, is_int=True)
        self._pack_indexed(P, B, src_t, real_t)
        self._early_side(P, masks, apply_update)
        self.generator_forward(P, masks, head=True)
        real_view, fake_view = P["dcat"].view(coff=0), P["dcat"].view(coff=0, n0=B)
        bufs = P.get("hook_idx")
        if bufs is None:        # ~0.5 GB each at B = 128: kept with the plan, not allocated per step
            bufs = P["hook_idx"] = tuple(torch.empty((B, S, S, Cn), dtype=torch.float32, device=self.device) for _ in range(3))
        probs32, z32, onehot = bufs
        # softmax + argmax (written into the discriminator's fake half) + the f32 probabilities; no loss, no gradient
        L.call("p2p_softmax_cce_argmax", self.dtype, B, S, S, Cn, C.byref(P["z"].view()), C.byref(real_view), C.byref(fake_view),
               0.0, 0.0, None, _p(probs32), _p(self._softmax_part()), _p(self.losses, 14), _stream())
        L.call("p2p_unpack", self.dtype, B, S, S, Cn, C.byref(P["z"].view()), _p(z32), _stream())
        onehot.zero_()
        onehot.view(-1, Cn).scatter_(1, real_t.view(-1, 1).long(), 1.0)
        self.discriminator_forward(P, 2 * B)
        d_loss, lg_d, lg_g = self._hook_discriminator(P, B, discriminator_loss)
        probs = probs32.detach().requires_grad_(True)
        probs._keras_logits = z32.detach().requires_grad_(True)
        g_loss = generator_loss(lg_g, probs, onehot)
        g_loss[0].backward()
        grad = lambda t: None if t.grad is None else t.grad.contiguous()        # noqa: E731  (absent: zero)
        gp, gz = grad(probs), grad(probs._keras_logits)
        self._write_dlogits(P["dld"], lg_d)
        P["hook_keep"] = (gp, gz, lg_d, lg_g, probs)
        L.call("p2p_softmax_bwd", self.dtype, B, S, S, Cn, _p(probs32), NULL if gp is None else _p(gp), NULL if gz is None else _p(gz),
               1.0, C.byref(P["dz"].view()), _stream())
        P["skip_g_through_d"] = True
        P["head_dbias_done"] = False        # the plan is shared with the fused step, whose head sums the bias gradient itself
        self.discriminator_backward(P, B)
        self.generator_backward(P)
        self._optimizer_tail(apply_update)
        return self._hooked_result(g_loss, d_loss)

    def _softmax_part(self):
        """workspace of p2p_softmax_cce_argmax: one (CCE, L1) partial per workgroup (include/p2pgan.h)"""
        if getattr(self, "_sm_part", None) is None:
            self._sm_part = torch.zeros(2 * 8192, dtype=torch.float32, device=self.device)
        return self._sm_part

    def discriminate(self, target, source):
        """discriminator([target, source], training=True) (pix2pix_model.py:69-70): f32 device logits (B,S/2,S/2,1)."""
        B = int(target.shape[0])
        return self._discriminate_pair(self.plan(B), B, target, source, self.head == "softmax")

    def _discriminate_pair(self, P, N, first, second, is_int):
        """[first, second] packed into P's discriminator input, D forward, the logits unpacked: f32 (N,S/2,S/2,1)"""
        ic, h2 = self.in_ch, self.S // 2
        self._pack(P, self._to_device(first, ic, N, is_int), P["dcat"].view(coff=0), ic)
        self._pack(P, self._to_device(second, ic, N, is_int), P["dcat"].view(coff=ic), ic)
        self.discriminator_forward(P, N)
        out = torch.empty((N, h2, h2, 1), dtype=torch.float32, device=self.device)
        L.call("p2p_unpack", self.dtype, N, h2, h2, 1, C.byref(P["logits"].view()), _p(out), _stream())
        return out

    def generate_indexed(self, source_idx, masks=None, with_probs=False):
        """Pix2PixIndexedModel.generate / generate_with_probs (pix2pix_model.py:283-293): int32 (B,S,S,1) argmax indices
        (and the f32 (B,S,S,256) probabilities)."""
        assert self.head == "softmax"
        B = int(source_idx.shape[0])
        P = self.plan(B)
        S = self.S
        src_t = self._to_device(source_idx, 1, B, is_int=True)
        self._batch_offset = 0          # evaluation: the dropout stream of sample k does not depend on the last train shard
        self._pack_source(P, src_t)
        self.generator_forward(P, masks)
        fake_view = P["dcat"].view(coff=0, n0=B)
        probs = torch.empty((B, S, S, self.out_ch), dtype=torch.float32, device=self.device)
        L.call("p2p_softmax_cce_argmax", self.dtype, B, S, S, self.out_ch, C.byref(P["z"].view()), C.byref(fake_view),
               C.byref(fake_view), 0.0, 0.0, None, _p(probs), _p(self._softmax_part()), _p(self.losses, 14), _stream())
        idx = torch.empty((B * S * S,), dtype=torch.int32, device=self.device)
        L.call("p2p_argmax_lastdim", _p(probs), B * S * S, self.out_ch, _p(idx), _stream())
        idx = idx.view(B, S, S, 1)
        return (idx, probs) if with_probs else idx

    # ------------------------------------------------------------------ hipGraph replay of the whole step
    def graphed_rgba_step(self, B, lambda_l1, lambda_hist=None, global_batch=None):
        """Captures one whole train step (about 130 kernel launches on two streams) into a hipGraph and returns
        step(source, real) -> losses that copies the batch into static buffers and replays it.  Everything that
        changes from step to step (Adam's t / step size, the dropout counter) lives in device memory.  Single-GPU
        only: the gradient all-reduce stays outside graphs."""
        S, ic = self.S, self.in_ch
        self.replay_enabled = False          # the captured graph IS the replay; the host-side call list must not record capture streams
        src_s = torch.zeros((B, S, S, ic), dtype=torch.float32, device=self.device)
        real_s = torch.zeros((B, S, S, ic), dtype=torch.float32, device=self.device)
        # warm-up on a snapshot: allocates every buffer of the plan, loads every code object, then rolls the state back
        self._require_live("a train step")
        snap = [(t, t.clone()) for st in (self.G, self.D) for t in (st.params, st.m, st.v, st.t_dev, st.lr_t_dev)]
        if self.G.ema is not None:
            snap.append((self.G.ema, self.G.ema.clone()))
        snap.append((self.mask_counter_dev, self.mask_counter_dev.clone()))
        t_host = (self.G.t, self.D.t)
        side = torch.cuda.Stream(device=self.device)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            self.train_step_rgba(src_s, real_s, lambda_l1, lambda_hist, global_batch=global_batch)
        torch.cuda.current_stream().wait_stream(side)
        for t, c in snap:
            t.copy_(c)
        self.G.t, self.D.t = t_host
        self.refresh_weight_copies(outside=False)        # (the state the warm-up step started from: no second look under capture)
        torch.cuda.synchronize(self.device)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = self.train_step_rgba(src_s, real_s, lambda_l1, lambda_hist, global_batch=global_batch)
        self.G.t, self.D.t = t_host       # the capture pass only recorded; host mirrors advance per replay below

        def step(source, real):
            self._require_live("a train step")
            src_s.copy_(torch.as_tensor(source), non_blocking=True)
            real_s.copy_(torch.as_tensor(real), non_blocking=True)
            graph.replay()
            self.G.t += 1
            self.D.t += 1
            self.step_count += 1
            return out

        step.graph = graph
        return step

    # ------------------------------------------------------------------ inference-style helpers
    def generate(self, source, masks=None):
        """generator(source, training=True) (pix2pix_model.py:58-60): f32 device tensor (B,S,S,out) for the tanh
        head; dropout stays on, as in the reference."""
        if self.head != "tanh":
            raise NotImplementedError("use generate_indexed for the softmax head")
        B = int(source.shape[0])
        P = self.plan(B)
        S = self.S
        src_t = self._to_device(source, self.in_ch, B)
        self._batch_offset = 0          # evaluation: the dropout stream of sample k does not depend on the last train shard
        self._pack_source(P, src_t)
        self.generator_forward(P, masks)
        fake_view = P["dcat"].view(coff=0, n0=B)
        # tanh through the loss kernel (its L1 output lands in a scratch slot and is ignored)
        L.call("p2p_tanh_l1_fwd", self.dtype, B, S, S, self.out_ch, C.byref(P["z"].view()), C.byref(fake_view),
               C.byref(fake_view), 0.0, _p(self.loss_part, 4 * 256), NULL, _stream())
        out = torch.empty((B, S, S, self.out_ch), dtype=torch.float32, device=self.device)
        L.call("p2p_unpack", self.dtype, B, S, S, self.out_ch, C.byref(fake_view), _p(out), _stream())
        return out

    # ------------------------------------------------------------------ tape calls (tape.py: tf_compat.tf.GradientTape)
    # A custom train_step (pix2pix_model.py:62-89 is the reference's) calls the networks under a GradientTape.  Every call runs on
    # an ARENA of its own (the plan's generator or discriminator part for its image count, plus the workspaces shared by the tape
    # calls of that count), so one tape may call G twice and D three times; the VJP of a call runs the same backward kernels as
    # the fused step on that arena.  The fused and replayed steps keep their plans and never see an arena.
    def tape_arena(self, kind, N):
        """an arena for one tape call of network `kind` ("G" / "D") on N images: pooled, or allocated"""
        self._require_live("a tape call")
        pool = self._arena_pool.setdefault((kind, N), [])
        if pool:
            return pool.pop()
        P = {"B": N, "kind": kind}
        if kind == "G":
            self._alloc_generator(P, N)
            P["fake"] = DenseBuf(N, self.S, self.S, self.out_ch, self.tdt, self.device)     # tanh(z) in the activation dtype
        else:
            self._alloc_discriminator(P, N)
        ws = self._tape_ws.get(N)
        if ws is None:
            ws = {}
            self._alloc_workspaces(ws, N)
            self._tape_ws[N] = ws
        P.update(ws)
        return P

    def release_tape_arena(self, P):
        self._arena_pool[(P["kind"], P["B"])].append(P)

    def free_tape_arenas(self):
        """drops the pooled arenas and their workspaces (the memory returns to torch's allocator)"""
        self._arena_pool.clear()
        self._tape_ws.clear()

    @staticmethod
    def arena_bytes(P):
        """device bytes an arena holds besides the shared workspaces"""
        seen, total = set(), 0

        def add(t):
            nonlocal total
            if isinstance(t, (HaloBuf, DenseBuf)):
                t = t._flat if isinstance(t, HaloBuf) else t.t
            if isinstance(t, torch.Tensor) and t.data_ptr() not in seen:
                seen.add(t.data_ptr())
                total += t.numel() * t.element_size()
            elif isinstance(t, (list, tuple)):
                for x in t:
                    add(x)
            elif isinstance(t, dict):
                for x in t.values():
                    add(x)
        add({k: v for k, v in P.items() if k not in ("nws", "spart", "slabs", "wws")})
        return total

    def tape_generator_forward(self, P, source, masks=None):
        """generator(source, training=True) on arena P: the f32 (B,S,S,out) image.  Dropout: the masks are drawn at the device
        counter (offset 0), which then advances by one -- one tape step of the reference's form draws the fused step's masks."""
        B, S = P["B"], self.S
        src_t = self._to_device(source, self.in_ch, B)
        self._dp, self._batch_offset = None, 0
        self._pack_source(P, src_t)
        P["early_masks"] = False
        self.generator_forward(P, masks)
        L.call("p2p_counter_add", _p(self.mask_counter_dev), 1, _stream())
        out = torch.empty((B, S, S, self.out_ch), dtype=torch.float32, device=self.device)
        fake = P["fake"].view()
        L.call("p2p_tanh_l1_fwd", self.dtype, B, S, S, self.out_ch, C.byref(P["z"].view()), C.byref(fake), C.byref(fake), 0.0,
               _p(self.loss_part, 4 * 256), _p(out), _stream())
        return out

    def _gradient_f32(self, g, shape):
        """an upstream gradient as a dense, 16-byte aligned f32 device tensor"""
        g = g.detach().to(device=self.device, dtype=torch.float32).reshape(shape).contiguous()
        return g if g.data_ptr() % 16 == 0 else g.clone()

    def _down1_copy(self):
        """G.down1's op-P operand copy (the fused step never needs it: no gradient flows into the source image), prepared when a
        tape asks for d(source) and re-derived once the generator's weights have changed"""
        key = (self.G.t, self._copies_version)
        lw = self.W[("G", "down1")]
        if self._down1_wn is None:
            self._down1_wn = torch.zeros(16 * up32(lw.cg) * lw.lo_pad, dtype=self.tdt, device=self.device)
        if self._down1_wn_key != key:
            L.call("p2p_weight_prep_pad", self.dtype, self.G.p("down1.kernel"), lw.cg, lw.cd, _p(self._down1_wn), up32(lw.cg),
                   lw.lo_pad, None, 0, 0, _stream())
            self._down1_wn_key = key
        return _p(self._down1_wn)

    def tape_generator_backward(self, P, d_image, need_source_grad):
        """VJP of one generator call from d(image) (f32): the weight gradients into G.grads (complete once the side stream is
        joined) and, if asked, d(source) as a dense f32 (B,S,S,in) tensor.  The source feeds down1 and the last skip connection
        (concat 6 = [up6 | source], networks.py:92-94), so d(source) is G.down1 transposed into the image channels (the shape of
        D.down's data gradient) plus the source channels of the head's data gradient."""
        B, S, ic = P["B"], self.S, self.in_ch
        g = self._gradient_f32(d_image, (B, S, S, self.out_ch))
        gx = L.GSrc(g.data_ptr(), 2, 1, B * S * S * self.out_ch, self.out_ch, 0)
        fake = P["fake"].view()
        self._tanh_l1_bwd(P, fake, fake, None, gx, 0.0)
        P["head_dbias_done"] = False
        self.generator_backward(P)
        d_src = None
        if need_source_grad:
            buf = P.get("g_src")
            if buf is None:
                buf = P["g_src"] = DenseBuf(B, S, S, 4 if (ic == 4 and self.full_pixels) else self.src_ch, self.tdt, self.device)
            self._conv(P, L.OP_P, "G", "down1", B, S // 2, P["dd"][1].view(), buf.view(), ncols=ic,
                       w_p=self._down1_copy() if self.use_mfma else None)
            skip = P.get("g_c6")
            if skip is None:
                skip = P["g_c6"] = DenseBuf(B, S, S, self.c6_ch, self.tdt, self.device)
            self._conv(P, L.OP_P, "G", "last", B, S, P["dz"].view(), skip.view(), stride=1, ncols=UP_FILTERS[5] + ic)
            d_src = torch.empty((B, S, S, ic), dtype=torch.float32, device=self.device)
            d_skip = torch.empty((B, S, S, ic), dtype=torch.float32, device=self.device)
            L.call("p2p_unpack", self.dtype, B, S, S, ic, C.byref(buf.view()), _p(d_src), _stream())
            L.call("p2p_unpack", self.dtype, B, S, S, ic, C.byref(skip.view(coff=UP_FILTERS[5])), _p(d_skip), _stream())
            L.call("p2p_grad_accumulate", _p(d_src), _p(d_skip), d_src.numel(), 0, _stream())
        self.side.join()
        self._adam_head_ev = None
        P["keep"] = g
        return d_src

    def tape_discriminator_forward(self, P, first, second):
        """discriminator([first, second], training=True) on arena P: f32 logits (N,S/2,S/2,1)"""
        return self._discriminate_pair(P, P["B"], first, second, False)

    def tape_discriminator_backward(self, P, d_logits, weights, need_first, need_second):
        """VJP of one standalone discriminator call (discriminator_backward for one input pair): with `weights`, the weight
        gradients into D.grads; d(first input) / d(second input) as dense f32 (N,S,S,in) tensors where asked (else None),
        through D.down's data gradient into the image channels."""
        N, S, ic, h2 = P["B"], self.S, self.in_ch, self.S // 2
        g = self._gradient_f32(d_logits, (N, h2, h2, 1))
        L.call("p2p_pack_input", self.dtype, N, h2, h2, 1, _p(g), 0, C.byref(P["dld"].view()), _stream())     # channel 0 of 8
        dld, d_act, d_draw = P["dld"].view(), P["d_act"].view(), P["d_draw"].view()
        if weights:
            self._wgrad(P, "D", "last", N, h2, d_act, dld, stride=1, dbias=self.D.g("last.bias"))
        if not self._d_last_dgrad_gated(N, h2, dld, d_act, d_draw):
            self._conv(P, L.OP_P, "D", "last", N, h2, dld, P["g_dact"].view(), stride=1)
            self._act_bwd(N, h2, 64, d_act, P["g_dact"].gsrc(), None, d_draw, fork_follows=weights)
        if weights:
            self._wgrad(P, "D", "down", N, h2, P["dcat"].view(), d_draw)
        outs = [None, None]
        if need_first or need_second:
            nc = 2 * ic if need_second else ic
            buf = P["g_dcat"]
            if buf.c < nc:
                buf = P.get("g_dcat2")
                if buf is None:
                    buf = P["g_dcat2"] = DenseBuf(N, S, S, self.dcat_ch, self.tdt, self.device)
            self._conv(P, L.OP_P, "D", "down", N, h2, d_draw, buf.view(), ncols=nc)
            for k, want in enumerate((need_first, need_second)):
                if want:
                    outs[k] = torch.empty((N, S, S, ic), dtype=torch.float32, device=self.device)
                    L.call("p2p_unpack", self.dtype, N, S, S, ic, C.byref(buf.view(coff=k * ic)), _p(outs[k]), _stream())
        self.side.join()
        P["keep"] = g
        return outs

    def tape_collect(self, sid, dst, first):
        """the weight gradients of the backward just joined (the store's scratch `grads`) into a tape's f32 buffer: dst = grads on
        the network's first contribution, dst += grads after it"""
        store = self._store(sid)
        L.call("p2p_grad_accumulate", _p(dst), _p(store.grads), store.numel, int(bool(first)), _stream())

    def apply_adam_store(self, store, grads):
        """One optimizer's step (Adam.apply_gradients of a custom train_step): the store's own t / t_dev / lr_t_dev, Keras Adam on
        its flat buffer from `grads` (f32, the store's layout), then its layers' weight copies.  apply_adam is the fused step's
        form for both networks; the dropout counter is not advanced here (a tape's generator calls advance it)."""
        self._require_live("an optimizer step")
        store.t += 1
        self._adam_tick(store)
        self._clip_scale(store, grads)
        self._adam_flat(store, grads, 0, store.numel)
        self.refresh_weight_copies("G" if store is self.G else "D", optimizer_step=True)
