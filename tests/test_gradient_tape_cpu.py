"""tape.py's bookkeeping without a GPU: a stand-in engine whose "networks" are two one-weight maps (the same entry points the
HIP engine gives the tape) -- which VJPs run with which requests, the gradients they sum, what gradient() returns, the
refusals, arena release, and what Adam.apply_gradients hands the engine."""
import gc
from collections import OrderedDict

import pytest
import torch

from palette_and_histo_gan_amd import pix2pix_model as M
from palette_and_histo_gan_amd.engine import ParamStore
from palette_and_histo_gan_amd.networks import PatchDiscriminator, UnetGenerator
from palette_and_histo_gan_amd.tf_compat import tf


class StandIn:
    """G(x) = w0 * x;  D([a, b]) = per-image sum of (v0 * a + v1 * b)"""
    head, tape_refusal, device, S, in_ch = "tanh", None, torch.device("cpu"), 4, 1

    def __init__(self):
        self.G = ParamStore(OrderedDict([("down1.kernel", (4, 4, 1, 1)), ("last.bias", (1,))]), "cpu")
        self.D = ParamStore(OrderedDict([("down.kernel", (4, 4, 2, 1))]), "cpu")
        for st in (self.G, self.D):
            st.grads = torch.zeros(st.numel)
            st.params.copy_(torch.linspace(0.5, 1.5, st.numel))
        self.log, self.pool, self.updates = [], [], []

    def _store(self, k):
        return self.G if k == "G" else self.D

    def generate(self, x, masks=None):
        return torch.as_tensor(x) * self.G.params[0]

    def discriminate(self, a, b):
        return self.tape_discriminator_forward({}, torch.as_tensor(a), torch.as_tensor(b))

    def tape_arena(self, kind, N):
        return {"kind": kind, "B": N}

    def release_tape_arena(self, P):
        self.pool.append(P)

    def tape_generator_forward(self, P, x, masks):
        P["x"] = x.clone()
        return x * self.G.params[0]

    def tape_generator_backward(self, P, g, need_source_grad):
        self.log.append(("G", need_source_grad))
        self.G.grads.zero_()
        self.G.grads[0] = (g * P["x"]).sum()
        return g * self.G.params[0] if need_source_grad else None

    def tape_discriminator_forward(self, P, a, b):
        P["a"], P["b"] = a.clone(), b.clone()
        return (a * self.D.params[0] + b * self.D.params[1]).sum(dim=(1, 2, 3), keepdim=True)

    def tape_discriminator_backward(self, P, g, weights, need_first, need_second):
        self.log.append(("D", weights, need_first, need_second))
        self.D.grads.zero_()
        self.D.grads[0], self.D.grads[1] = (g * P["a"]).sum(), (g * P["b"]).sum()
        ones = torch.ones_like(P["a"])
        return [g * self.D.params[0] * ones if need_first else None, g * self.D.params[1] * ones if need_second else None]

    def tape_collect(self, kind, dst, first):
        src = self._store(kind).grads
        dst.copy_(src) if first else dst.add_(src)

    def apply_adam_store(self, store, grads):
        store.t += 1
        self.updates.append((store, grads))


def _bind(eng):
    G = UnetGenerator(1, 1, "tanh").bind(eng, eng.G)
    Dn = PatchDiscriminator(1).bind(eng, eng.D)
    return G, Dn


def test_gradients_prune_and_sum_over_calls():
    eng = StandIn()
    G, Dn = _bind(eng)
    x = torch.randn(2, 4, 4, 1)
    with tf.GradientTape(persistent=True) as tape:
        y = G(x)
        y2 = G(y)                                   # the generator applied to its own output
        p = Dn([y2, x])
        q = Dn([x, x])
        g_loss = p.sum() + (y2 - x).abs().mean()
        d_loss = p.sum() + q.sum()
    gg = tape.gradient(g_loss, G.trainable_variables)
    # G's target: D computes no weight gradient, only d(first input); G's second call passes d(source) to the first
    assert eng.log == [("D", False, True, False), ("G", True), ("G", False)]
    eng.log.clear()
    dg = tape.gradient(d_loss, Dn.trainable_variables)
    assert eng.log == [("D", True, False, False), ("D", True, False, False)]      # no generator VJP, no input gradients
    w = eng.G.params[0].clone().requires_grad_(True)
    v = eng.D.params[:2].clone().requires_grad_(True)
    r2 = x * w * w
    rp = (r2 * v[0] + x * v[1]).sum(dim=(1, 2, 3), keepdim=True)
    rg = torch.autograd.grad(rp.sum() + (r2 - x).abs().mean(), w, retain_graph=True)[0]
    rd = torch.autograd.grad(rp.sum() + (x * v[0] + x * v[1]).sum(dim=(1, 2, 3)).sum(), v)[0]
    assert torch.allclose(gg[0].reshape(-1)[0], rg) and torch.allclose(dg[0].reshape(-1)[:2], rd)
    assert gg[0].shape == (4, 4, 1, 1) and gg[0]._base is gg[1]._base          # views of one flat tape buffer
    assert torch.equal(gg[0].reshape(-1)[1:], torch.zeros(15))                  # (the stand-in's other weights have none)
    # a target that does not depend on G: None for every variable of G
    grads = tape.gradient(q.sum(), G.trainable_variables + Dn.trainable_variables)
    assert grads[0] is None and grads[1] is None and grads[2] is not None
    del tape, y, y2, p, q, g_loss, d_loss
    gc.collect()
    assert [P["kind"] for P in eng.pool] == ["G", "G", "D", "D"]             # arenas go back when the tape is released


def test_refusals():
    eng = StandIn()
    G, Dn = _bind(eng)
    x = torch.randn(2, 4, 4, 1)
    with tf.GradientTape() as tape:
        y = G(x)
    assert y.requires_grad and not G(x).requires_grad              # outside the `with` block: not recorded
    tape.gradient(y.sum(), G.trainable_variables)
    with pytest.raises(RuntimeError, match="non-persistent"):
        tape.gradient(y.sum(), G.trainable_variables)
    with tf.GradientTape() as outer:
        with tf.GradientTape() as inner:
            y = G(x)
        with pytest.raises(RuntimeError, match="higher-order"):
            inner.gradient(y.sum(), G.trainable_variables)
    with tf.GradientTape() as tape:
        y = G(x)
    with pytest.raises(RuntimeError, match="tape.gradient"):
        y.sum().backward()
    eng.tape_refusal = "one GPU"
    with tf.GradientTape():
        with pytest.raises(NotImplementedError, match="one GPU"):
            G(x)
    eng.tape_refusal, eng.head = None, "softmax"
    with tf.GradientTape():
        with pytest.raises(NotImplementedError, match="hooked"):
            Dn([x, x])
    del outer


def test_apply_gradients_reads_the_tapes_buffer_in_place():
    eng = StandIn()
    G, Dn = _bind(eng)
    opt_g, opt_d = M.Adam(2e-4, beta_1=0.5), M.Adam(2e-4, beta_1=0.5)
    opt_g._store, opt_g._engine, opt_d._store, opt_d._engine = eng.G, eng, eng.D, eng
    x = torch.randn(2, 4, 4, 1)
    with tf.GradientTape() as tape:
        loss = Dn([G(x), x]).sum()
    grads = tape.gradient(loss, G.trainable_variables)
    opt_g.apply_gradients(zip(grads, G.trainable_variables))
    store, flat = eng.updates[-1]
    assert store is eng.G and flat.data_ptr() == grads[0]._base.data_ptr()          # no copy
    opt_g.apply_gradients(zip([g * 0.5 for g in grads], G.trainable_variables))
    store, flat = eng.updates[-1]
    assert flat.data_ptr() != grads[0]._base.data_ptr() and torch.equal(flat, 0.5 * grads[0]._base)
    assert opt_g.iterations == 2 and opt_d.iterations == 0
    with pytest.raises(ValueError, match="not one of"):
        opt_g.apply_gradients(zip(grads, Dn.trainable_variables[:1] + G.trainable_variables[1:]))
    with pytest.raises(ValueError, match="whole network"):
        opt_g.apply_gradients(zip(grads[:1], G.trainable_variables[:1]))
