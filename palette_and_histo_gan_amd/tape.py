"""tf.GradientTape over the HIP networks, for a custom train_step (the reference's own, pix2pix_model.py:62-89, is written so):

    with tf.GradientTape(persistent=True) as tape:
        fake_image = self.generator(source_image, training=True)
        fake_predicted = self.discriminator([fake_image, source_image], training=True)
        ...
    grads = tape.gradient(g_loss[0], self.generator.trainable_variables)
    self.generator_optimizer.apply_gradients(zip(grads, self.generator.trainable_variables))

While a tape records, a network call (networks.py handles) runs forward on an arena of its own (engine.tape_arena) and returns a
differentiable f32 tensor: the loss between the calls is ordinary torch code, and torch autograd carries the gradients from one
call to the next.  Each call is one torch.autograd.Function whose backward is the engine's VJP of that call (HIP kernels);
the weights enter the graph through one anchor scalar per network, so `gradient()` asks autograd for the anchors of the
networks whose variables it was given and nothing else.  A VJP computes the weight gradients only of a network that the current
gradient() asked for, and an input gradient only where the input depends on such a network (the pruning TF does); the weight
gradients of every call of a network are summed into a tape-owned f32 buffer by p2p_grad_accumulate.  gradient() returns views
of that buffer, one per variable, in the order given, or None for every variable of a network the target does not depend on.

Single GPU (as the hooked steps), not replayed or captured; no higher-order gradients.  Outside a tape the networks behave as
before: detached values, no arena.
"""
import weakref

import torch

_RECORDING = []          # tapes inside their `with` block, innermost last


def recording():
    """the innermost tape that is recording, or None"""
    return _RECORDING[-1] if _RECORDING else None


def _deps(t):
    """the networks (engine, "G" / "D") whose tape calls a tensor depends on: walks its autograd graph back to the nearest tape
    calls (their nodes carry the set)"""
    if not isinstance(t, torch.Tensor) or not t.requires_grad or t.grad_fn is None:
        return frozenset()
    out, seen, stack = set(), set(), [t.grad_fn]
    while stack:
        node = stack.pop()
        if node is None or id(node) in seen:
            continue
        seen.add(id(node))
        d = getattr(node, "_p2p_deps", None)
        if d is not None:
            out |= d
            continue
        stack.extend(n for n, _ in node.next_functions)
    return frozenset(out)


class _Call(torch.autograd.Function):
    """one network call under a tape: inputs (anchor, x0[, x1]); the VJP is the engine's"""

    @staticmethod
    def forward(ctx, anchor, tape, eng, kind, P, masks, *xs):
        # (a weak reference: the graph a caller keeps, e.g. logged losses, must not keep the tape and its arenas alive)
        ctx.tape, ctx.eng, ctx.kind, ctx.P = weakref.ref(tape), eng, kind, P
        ctx.x_deps = [_deps(x) for x in xs]
        ctx._p2p_deps = frozenset({(eng, kind)}).union(*ctx.x_deps)
        if kind == "G":
            return eng.tape_generator_forward(P, xs[0], masks)
        return eng.tape_discriminator_forward(P, xs[0], xs[1])

    @staticmethod
    def backward(ctx, grad):
        tape = ctx.tape()
        if torch.is_grad_enabled():
            raise RuntimeError("higher-order gradients through the HIP networks are not supported (create_graph / nested tapes)")
        if tape is None or tape._released:
            raise RuntimeError("the GradientTape that recorded this call has been released: its calls cannot be differentiated")
        if not tape._wanted:
            raise RuntimeError("gradients of the HIP network calls are taken with tape.gradient(target, sources)")
        eng, kind, key = ctx.eng, ctx.kind, (ctx.eng, ctx.kind)
        weights = key in tape._wanted
        need = [ctx.needs_input_grad[6 + k] and bool(d & tape._wanted) for k, d in enumerate(ctx.x_deps)]
        if kind == "G":
            dx = [eng.tape_generator_backward(ctx.P, grad, need[0])]
        else:
            dx = eng.tape_discriminator_backward(ctx.P, grad, weights, need[0], need[1])
        d_anchor = None
        if weights:
            tape._collect(eng, kind)
            d_anchor = torch.zeros(())
        return (d_anchor, None, None, None, None, None, *dx)


def _release(arenas):
    for eng, P in arenas:
        eng.release_tape_arena(P)
    arenas.clear()


class GradientTape:
    """tf.GradientTape(persistent=False) for the HIP networks (see the module docstring)"""

    def __init__(self, persistent=False):
        self.persistent = bool(persistent)
        self._recording = False
        self._used = self._released = False
        self._anchors = {}          # (engine, "G" / "D") -> anchor scalar of that network's weights
        self._arenas = []           # (engine, arena) of every call; back to the engine's pool when the tape is released
        self._finalizer = weakref.finalize(self, _release, self._arenas)
        self._wanted = frozenset()
        self._bufs = {}

    def __enter__(self):
        if self._recording:
            raise RuntimeError("this tape is already recording")
        self._recording = True
        _RECORDING.append(self)
        return self

    def __exit__(self, *exc):
        self._recording = False
        _RECORDING.remove(self)
        return False

    # -- recording (networks.py handles) ----------------------------------------------------------------------------------
    def _check_engine(self, eng):
        if eng.head != "tanh":
            raise NotImplementedError(
                "the palette-index generator (softmax head) has no tape path: its train step is fused around the softmax and the "
                "argmax; override its loss hooks with `differentiable_loss_hooks = True` instead (engine.train_step_indexed_hooked)")
        if eng.tape_refusal:
            raise NotImplementedError(eng.tape_refusal)
        if self._released:
            raise RuntimeError("this GradientTape has been released")

    def _anchor(self, eng, kind):
        a = self._anchors.get((eng, kind))
        if a is None:
            a = self._anchors[(eng, kind)] = torch.zeros((), requires_grad=True)
        return a

    def _image(self, eng, x, what):
        if not isinstance(x, torch.Tensor):
            x = torch.as_tensor(x)
        x = x.to(device=eng.device, dtype=torch.float32)
        if x.dim() != 4 or tuple(x.shape[1:]) != (eng.S, eng.S, eng.in_ch):
            raise ValueError(f"{what}: expected a (B, {eng.S}, {eng.S}, {eng.in_ch}) batch, got {tuple(x.shape)}")
        return x

    def call_generator(self, eng, source, masks=None):
        self._check_engine(eng)
        x = self._image(eng, source, "generator input")
        P = eng.tape_arena("G", int(x.shape[0]))
        self._arenas.append((eng, P))
        return _Call.apply(self._anchor(eng, "G"), self, eng, "G", P, masks, x)

    def call_discriminator(self, eng, first, second):
        self._check_engine(eng)
        a, b = self._image(eng, first, "discriminator input 0"), self._image(eng, second, "discriminator input 1")
        if a.shape[0] != b.shape[0]:
            raise ValueError(f"discriminator inputs of {a.shape[0]} and {b.shape[0]} images")
        P = eng.tape_arena("D", int(a.shape[0]))
        self._arenas.append((eng, P))
        return _Call.apply(self._anchor(eng, "D"), self, eng, "D", P, None, a, b)

    # -- gradients ---------------------------------------------------------------------------------------------------------
    def _collect(self, eng, kind):
        key = (eng, kind)
        buf = self._bufs.get(key)
        first = buf is None
        if first:
            buf = self._bufs[key] = torch.empty(eng._store(kind).numel, dtype=torch.float32, device=eng.device)
        eng.tape_collect(kind, buf, first)

    def _variable(self, t):
        """(engine, "G" / "D", name) of a trainable variable of a network this tape has called, or None"""
        for eng, kind in self._anchors:
            name = eng._store(kind).variable_name(t)
            if name is not None:
                return eng, kind, name
        return None

    def gradient(self, target, sources):
        """d(target)/d(sources): `sources` is a network's trainable_variables list (or both networks' lists joined); returns one
        tensor per variable, in order -- views of the tape's f32 buffer of that network -- or None for every variable of a
        network the target does not depend on"""
        if self._used and not self.persistent:
            raise RuntimeError("A non-persistent GradientTape can only be used to compute one set of gradients; "
                               "use GradientTape(persistent=True)")
        if any(t._recording for t in _RECORDING if t is not self):
            raise RuntimeError("higher-order gradients through the HIP networks are not supported: gradient() was called while "
                               "another tape is recording")
        if self._released:
            raise RuntimeError("this GradientTape has been released")
        single = isinstance(sources, torch.Tensor)
        srcs = [sources] if single else list(sources)
        found = [self._variable(s) for s in srcs]
        keys = []
        for f in found:
            if f is not None and (f[0], f[1]) not in keys:
                keys.append((f[0], f[1]))
        self._used = True
        result = {}
        if keys and isinstance(target, torch.Tensor) and target.requires_grad:
            self._wanted, self._bufs = frozenset(keys), {}
            try:
                got = torch.autograd.grad(target, [self._anchors[k] for k in keys],
                                          grad_outputs=None if target.dim() == 0 else torch.ones_like(target),
                                          retain_graph=self.persistent, allow_unused=True)
            finally:
                bufs, self._wanted, self._bufs = self._bufs, frozenset(), {}
            for k, g in zip(keys, got):
                if g is not None and k in bufs:
                    result[k] = bufs[k]
        if not self.persistent:
            self.release()
        out = []
        for s, f in zip(srcs, found):
            buf = None if f is None else result.get((f[0], f[1]))
            out.append(None if buf is None else f[0]._store(f[1]).view(buf, f[2]))
        return out[0] if single else out

    def release(self):
        """gives the arenas of the recorded calls back to their engines (also when the tape is garbage-collected)"""
        self._released = True
        self._finalizer()
