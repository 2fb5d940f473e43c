"""-m gpu: tf_compat.tf.GradientTape over the HIP networks -- a custom train_step in the reference's form (pix2pix_model.py:62-89)
against the fused step, a step the loss hooks cannot express against the float64 oracle graph, the tape's semantics, the
per-network optimizer step, and the whole thing through fit()."""
import os
import types

import numpy as np
import pytest
import torch

from oracle import reference_graph as rg
from palette_and_histo_gan_amd import _lib as L
from palette_and_histo_gan_amd import dataset_utils as D
from palette_and_histo_gan_amd import engine as E
from palette_and_histo_gan_amd import pix2pix_model as M
from palette_and_histo_gan_amd.tf_compat import tf

pytestmark = pytest.mark.gpu
F64 = torch.float64
S = 64


@pytest.fixture(autouse=True)
def _in_tmp(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)          # the models write their log and checkpoint folders under the working directory


def _params(seed):
    rng = np.random.default_rng(seed)
    Gp = rg.perturb_affine(rg.init_params(rg.generator_param_shapes(4, 4), rng, F64), rng)
    Dp = rg.perturb_affine(rg.init_params(rg.discriminator_param_shapes(4), rng, F64), rng)
    return rng, Gp, Dp


def _np(p):
    return {k: v.numpy() for k, v in p.items()}


def _model(Gp, Dp, dtype="f32", seed=5, cls=M.Pix2PixModel, **kw):
    m = cls(D.synthetic_rgba_ds(4, batch_size=2), None, "front2right", "tape-test", lambda_l1=100.0, dtype=dtype, seed=seed, **kw)
    m.engine.set_params(_np(Gp), _np(Dp))
    return m


def _engine(Gp, Dp, dtype=L.F32, seed=5):
    eng = E.Pix2PixEngine(4, 4, "tanh", S, dtype, seed=seed)
    eng.set_params(_np(Gp), _np(Dp))
    return eng


def _masks(rng, B):
    return [rng.integers(0, 2, size=s).astype(np.uint8) for s in rg.dropout_mask_shapes(B, S)]


def reference_step(model, src, tgt, masks=None, apply=True):
    """pix2pix_model.py:62-89 written for the tape"""
    with tf.GradientTape(persistent=True) as tape:
        fake_image = model.generator(src, training=True, masks=masks)
        real_predicted = model.discriminator([tgt, src], training=True)
        fake_predicted = model.discriminator([fake_image, src], training=True)
        g_loss = model.generator_loss(fake_predicted, fake_image, tgt)
        d_loss = model.discriminator_loss(real_predicted, fake_predicted)
    g_grads = tape.gradient(g_loss[0], model.generator.trainable_variables)
    d_grads = tape.gradient(d_loss[0], model.discriminator.trainable_variables)
    if apply:
        model.generator_optimizer.apply_gradients(zip(g_grads, model.generator.trainable_variables))
        model.discriminator_optimizer.apply_gradients(zip(d_grads, model.discriminator.trainable_variables))
    return g_loss, d_loss, g_grads, d_grads


def _losses(g_loss, d_loss):
    return [float(x.detach()) for x in g_loss[:3]] + [0.0] + [float(x.detach()) for x in d_loss[:3]]


def _as_dict(store, grads):
    return {k: g.detach().cpu().numpy() for k, g in zip(store.shapes, grads)}


def _close(got, want, tol):
    for k in want:
        assert np.abs(got[k] - want[k]).max() <= tol * np.abs(want[k]).max() + 1e-12, (k, np.abs(got[k] - want[k]).max(),
                                                                                        np.abs(want[k]).max())


def _close_params(got, want, tol, steps):
    """parameters: within `tol` of the network's max-norm, but for a handful of entries.  Tape and fused step differ at rounding
    level (torch evaluates the loss gradients the fused kernels compute); Adam moves a weight by up to lr whatever the size of
    its gradient, so a rounding-level entry whose sign or history differs -- and after the first update an activation that flips
    -- moves by a fraction of lr (measured 3.2e-5 on down2.kernel after three B = 4 steps; tests/test_dp_gpu.py bounds the same
    effect).  Different dropout masks would move most of the generator's entries by up to lr."""
    scale = max(np.abs(w).max() for w in want.values())
    diff = np.concatenate([np.abs(got[k] - want[k]).ravel() for k in want])
    over = int((diff > tol * scale).sum())
    assert over <= 1e-5 * diff.size, (over, diff.size, scale, float(diff.max()))
    assert diff.max() <= 2 * rg.ADAM_LR * steps, float(diff.max())


def test_reference_form_step_equals_the_fused_step():
    B = 2
    rng, Gp, Dp = _params(81)
    src, tgt = rg.synthetic_rgba_batch(rng, B, S, palette_size=24)
    masks = _masks(rng, B)
    fused = _engine(Gp, Dp)
    out = fused.train_step_rgba(src, tgt, 100.0, masks=masks, apply_update=False).cpu().numpy()
    m = _model(Gp, Dp)
    g_loss, d_loss, gg, dg = reference_step(m, src, tgt, masks)
    got = _losses(g_loss, d_loss)
    for i in (0, 1, 2, 4, 5, 6):
        assert abs(got[i] - out[i]) <= 1e-6 * abs(out[i]), (i, got[i], out[i])
    assert all(g is not None for g in gg + dg)
    _close(_as_dict(m.engine.G, gg), fused.G.export(fused.G.grads), 1e-5)
    _close(_as_dict(m.engine.D, dg), fused.D.export(fused.D.grads), 1e-5)
    # after the update: the fused step with its optimizer step, from the same weights
    upd = _engine(Gp, Dp)
    upd.train_step_rgba(src, tgt, 100.0, masks=masks, apply_update=True)
    _close_params(m.engine.G.export(), upd.G.export(), 2e-5, 1)
    _close_params(m.engine.D.export(), upd.D.export(), 2e-5, 1)
    assert m.generator_optimizer.iterations == 1 and m.discriminator_optimizer.iterations == 1


def test_device_drawn_masks_follow_the_fused_steps():
    """three tape steps and three fused steps without injected masks: a tape's generator call draws at the device counter and
    advances it, apply_gradients does not -- so both draw the same masks step after step"""
    B = 4
    rng, Gp, Dp = _params(82)
    batches = [rg.synthetic_rgba_batch(rng, B, S, palette_size=24) for _ in range(3)]
    fused = _engine(Gp, Dp, seed=9)
    m = _model(Gp, Dp, seed=9)
    for src, tgt in batches:
        fused.train_step_rgba(src, tgt, 100.0)
        reference_step(m, src, tgt)
    assert int(m.engine.mask_counter_dev.item()) == int(fused.mask_counter_dev.item()) == 3
    _close_params(m.engine.G.export(), fused.G.export(), 2e-5, 3)
    _close_params(m.engine.D.export(), fused.D.export(), 2e-5, 3)


def test_cycle_step_against_the_oracle_graph(seed=90):
    """a step the loss hooks cannot express: G applied to its own output (d(source) of G, two generator arenas alive at once),
    the adversarial term on D([G(src), src]) and a discriminator term over three separate calls.  (The inputs are drawn so that
    no activation of the 1x1 .. 4x4 layers lies within f32 rounding of its kink: where one does, f32 and f64 take different
    branches and the whole image's gradient moves by ~0.5 % -- the fused step does the same, e.g. seeds 83 and 91.)"""
    B = 2
    rng, Gp, Dp = _params(seed)
    src, tgt = rg.synthetic_rgba_batch(rng, B, S, palette_size=24)
    masks = _masks(rng, B)
    bce = torch.nn.functional.binary_cross_entropy_with_logits

    def losses(G, Dn, s, t):
        f1 = G(s)
        f2 = G(f1)
        cycle = (f2 - s).abs().mean()
        fp1 = Dn([f1, s])
        adv = bce(fp1, torch.ones_like(fp1))
        g_total = adv + 10.0 * cycle + 5.0 * (t - f1).abs().mean()
        rp, fp2 = Dn([t, s]), Dn([f2, s])
        d_total = bce(rp, torch.ones_like(rp)) + bce(fp1, torch.zeros_like(fp1)) + 0.5 * bce(fp2, torch.zeros_like(fp2))
        return g_total, cycle, d_total

    m = _model(Gp, Dp)
    s_dev, t_dev = torch.tensor(src, device="cuda:0"), torch.tensor(tgt, device="cuda:0")
    with tf.GradientTape(persistent=True) as tape:
        g_total, cycle, d_total = losses(lambda x: m.generator(x, masks=masks), m.discriminator, s_dev, t_dev)
    gg = tape.gradient(g_total, m.generator.trainable_variables)
    dg = tape.gradient(d_total, m.discriminator.trainable_variables)

    Gl = {k: v.clone().requires_grad_(True) for k, v in Gp.items()}
    Dl = {k: v.clone().requires_grad_(True) for k, v in Dp.items()}
    m64 = [torch.tensor(x, dtype=F64) for x in masks]
    want = losses(lambda x: rg.unet_generator(Gl, x, m64, "tanh"), lambda ab: rg.patch_discriminator(Dl, ab[0], ab[1]),
                  torch.tensor(src, dtype=F64), torch.tensor(tgt, dtype=F64))
    for a, b in zip((g_total, cycle, d_total), want):
        assert abs(float(a.detach()) - float(b.detach())) <= 1e-5 * abs(float(b.detach())), (float(a.detach()), float(b.detach()))
    g_ref = torch.autograd.grad(want[0], list(Gl.values()), retain_graph=True)
    d_ref = torch.autograd.grad(want[2], list(Dl.values()))
    _close(_as_dict(m.engine.G, gg), {k: g.numpy() for k, g in zip(Gl, g_ref)}, 1e-4)
    _close(_as_dict(m.engine.D, dg), {k: g.numpy() for k, g in zip(Dl, d_ref)}, 1e-4)


def test_tape_semantics():
    B = 2
    rng, Gp, Dp = _params(84)
    src, tgt = rg.synthetic_rgba_batch(rng, B, S, palette_size=24)
    masks = _masks(rng, B)
    m = _model(Gp, Dp)
    G, Dn = m.generator, m.discriminator
    # outside a tape: the values of the engine's generate(), not attached to autograd, no arena
    plain = G(src, masks=masks)
    assert not plain.requires_grad and not m.engine._arena_pool
    assert torch.equal(plain, _engine(Gp, Dp).generate(src, masks=masks))
    assert not Dn([tgt, src]).requires_grad
    # a non-persistent tape gives one set of gradients
    with tf.GradientTape() as tape:
        fake = G(src, masks=masks)
        loss = (fake - torch.tensor(tgt, device="cuda:0")).abs().mean()
    assert fake.requires_grad
    assert all(g is not None for g in tape.gradient(loss, G.trainable_variables))
    with pytest.raises(RuntimeError, match="non-persistent"):
        tape.gradient(loss, G.trainable_variables)
    # a target that does not depend on G: None for every variable of G
    with tf.GradientTape() as tape:
        G(src, masks=masks)
        rp = Dn([tgt, src])
    grads = tape.gradient(rp.mean(), G.trainable_variables + Dn.trainable_variables)
    n_g = len(G.trainable_variables)
    assert all(g is None for g in grads[:n_g]) and all(g is not None for g in grads[n_g:])
    # persistent G-then-D equals two fresh single-purpose tapes, bit for bit
    _, _, gg, dg = reference_step(m, src, tgt, masks, apply=False)
    gg, dg = [g.clone() for g in gg], [g.clone() for g in dg]
    with tf.GradientTape() as t1:
        fake = G(src, masks=masks)
        g_loss = m.generator_loss(Dn([fake, src]), fake, tgt)
    gg1 = t1.gradient(g_loss[0], G.trainable_variables)
    with tf.GradientTape() as t2:
        fake = G(src, masks=masks)
        d_loss = m.discriminator_loss(Dn([tgt, src]), Dn([fake, src]))
    dg1 = t2.gradient(d_loss[0], Dn.trainable_variables)
    assert all(torch.equal(a, b) for a, b in zip(gg, gg1)) and all(torch.equal(a, b) for a, b in zip(dg, dg1))
    # higher-order gradients are refused
    with tf.GradientTape() as outer:
        with tf.GradientTape() as inner:
            fake = G(src, masks=masks)
            loss = fake.abs().mean()
        with pytest.raises(RuntimeError, match="higher-order"):
            inner.gradient(loss, G.trainable_variables)
    del outer


def test_tape_arenas_leave_the_fused_step_alone():
    B = 2
    rng, Gp, Dp = _params(85)
    src, tgt = rg.synthetic_rgba_batch(rng, B, S, palette_size=24)
    masks = _masks(rng, B)
    m = _model(Gp, Dp)
    m.engine.train_step_rgba(src, tgt, 100.0, masks=masks)          # the plan of B = 2 exists before the tape steps
    for _ in range(2):
        reference_step(m, src, tgt, masks)
    out = m.engine.train_step_rgba(src, tgt, 100.0, masks=masks, apply_update=False).cpu().numpy()
    fresh = _engine({k: torch.tensor(v) for k, v in m.engine.G.export().items()},
                    {k: torch.tensor(v) for k, v in m.engine.D.export().items()})
    for a, b in ((fresh.G, m.engine.G), (fresh.D, m.engine.D)):
        a.m.copy_(b.m)
        a.v.copy_(b.v)
        a.t_dev.copy_(b.t_dev)
        a.lr_t_dev.copy_(b.lr_t_dev)
        a.t = b.t
    fresh.mask_counter_dev.copy_(m.engine.mask_counter_dev)
    want = fresh.train_step_rgba(src, tgt, 100.0, masks=masks, apply_update=False).cpu().numpy()
    assert np.array_equal(out, want), (out, want)
    for a, b in ((m.engine.G, fresh.G), (m.engine.D, fresh.D)):
        ga, gb = a.export(a.grads), b.export(b.grads)
        assert all(np.array_equal(ga[k], gb[k]) for k in ga)


def test_apply_gradients():
    B = 2
    rng, Gp, Dp = _params(86)
    src, tgt = rg.synthetic_rgba_batch(rng, B, S, palette_size=24)
    masks = _masks(rng, B)
    m = _model(Gp, Dp)
    G = m.generator
    with tf.GradientTape() as tape:
        fake = G(src, masks=masks)
        loss = m.generator_loss(m.discriminator([fake, src]), fake, tgt)[0]
    grads = tape.gradient(loss, G.trainable_variables)
    g64 = {k: g.detach().cpu().to(F64) * 0.5 for k, g in zip(m.engine.G.shapes, grads)}
    p64 = {k: torch.tensor(v, dtype=F64) for k, v in m.engine.G.export().items()}
    d_before = m.engine.D.export()
    m.generator_optimizer.apply_gradients(zip([g * 0.5 for g in grads], G.trainable_variables))     # copied: not the tape's views
    assert m.generator_optimizer.iterations == 1 and m.discriminator_optimizer.iterations == 0
    zeros = {k: torch.zeros_like(v) for k, v in p64.items()}
    want, _, _ = rg.keras_adam(p64, g64, zeros, zeros, 1)
    got = m.engine.G.export()
    for k in want:
        w = want[k].numpy()
        assert np.abs(got[k] - w).max() <= 1e-6 * np.abs(w).max(), k
    assert all(np.array_equal(a, b) for a, b in zip(d_before.values(), m.engine.D.export().values()))
    with pytest.raises(ValueError):
        m.generator_optimizer.apply_gradients(zip(grads[:1], m.discriminator.trainable_variables[:1]))

    # bf16: the weight copies are refreshed -- generate() equals a fresh engine loaded with the exported weights, bit for bit
    m16 = _model(Gp, Dp, dtype="bf16")
    _, _, gg, dg = reference_step(m16, src, tgt, masks)
    assert m16.generator_optimizer.iterations == 1 and m16.discriminator_optimizer.iterations == 1
    fresh = E.Pix2PixEngine(4, 4, "tanh", S, L.BF16, seed=5)
    fresh.set_params(m16.engine.G.export(), m16.engine.D.export())
    assert torch.equal(m16.engine.generate(src, masks=masks), fresh.generate(src, masks=masks))
    assert torch.equal(m16.engine.discriminate(tgt, src), fresh.discriminate(tgt, src))


def _rel_devs(a, b):
    return {k: float(np.abs(a[k] - b[k]).max() / (np.abs(b[k]).max() + 1e-30)) for k in b}


def test_bf16_tape_step_within_the_fused_steps_own_deviation():
    B = 2
    rng, Gp, Dp = _params(87)
    src, tgt = rg.synthetic_rgba_batch(rng, B, S, palette_size=24)
    masks = _masks(rng, B)
    f32, f16 = _engine(Gp, Dp), _engine(Gp, Dp, dtype=L.BF16)
    o32 = f32.train_step_rgba(src, tgt, 100.0, masks=masks, apply_update=False).cpu().numpy()
    o16 = f16.train_step_rgba(src, tgt, 100.0, masks=masks, apply_update=False).cpu().numpy()
    m = _model(Gp, Dp, dtype="bf16")
    g_loss, d_loss, gg, dg = reference_step(m, src, tgt, masks, apply=False)
    got = _losses(g_loss, d_loss)
    for i in (0, 1, 2, 4, 5, 6):
        yard = abs(o16[i] - o32[i]) / abs(o32[i])
        assert abs(got[i] - o16[i]) / abs(o16[i]) <= max(1e-3, 1.5 * yard), (i, got[i], o16[i], o32[i])
    for store, grads in ((m.engine.G, gg), (m.engine.D, dg)):
        ref16 = (f16.G if store is m.engine.G else f16.D)
        ref32 = (f32.G if store is m.engine.G else f32.D)
        yard = _rel_devs(ref16.export(ref16.grads), ref32.export(ref32.grads))
        dev = _rel_devs(_as_dict(store, grads), ref16.export(ref16.grads))
        for k, e in dev.items():
            assert e <= max(1e-3, 1.5 * yard[k]), (k, e, yard[k])


class TapeStepModel(M.Pix2PixModel):
    """the reference's train_step (pix2pix_model.py:62-89) in a subclass"""

    def train_step(self, batch, step, update_steps):
        source_image, real_image = batch
        with tf.GradientTape(persistent=True) as tape:
            fake_image = self.generator(source_image, training=True)
            real_predicted = self.discriminator([real_image, source_image], training=True)
            fake_predicted = self.discriminator([fake_image, source_image], training=True)
            g_loss = self.generator_loss(fake_predicted, fake_image, real_image)
            d_loss = self.discriminator_loss(real_predicted, fake_predicted)
        generator_gradients = tape.gradient(g_loss[0], self.generator.trainable_variables)
        discriminator_gradients = tape.gradient(d_loss[0], self.discriminator.trainable_variables)
        self.generator_optimizer.apply_gradients(zip(generator_gradients, self.generator.trainable_variables))
        self.discriminator_optimizer.apply_gradients(zip(discriminator_gradients, self.discriminator.trainable_variables))
        if self.summary_writer is not None:
            self.log_generator_loss(g_loss, step // update_steps)
            self.log_discriminator_loss(d_loss, step // update_steps)
        return g_loss, d_loss


def test_a_tape_train_step_trains_through_fit():
    train = D.synthetic_rgba_ds(8, batch_size=4, palette_size=24)
    m = TapeStepModel(train, train, "front2right", "pix2pix-tape-test", lambda_l1=100.0)
    first = [float(x) for x in m.train_step(next(iter(train)), 0, 1)[0]]
    m.fit(30, 10)
    last = [float(x) for x in m.train_step(next(iter(train)), 31, 10)[0]]
    assert last[2] < 0.6 * first[2], (first, last)          # the L1 term fell
    assert m.generator_optimizer.iterations == 32 and m.discriminator_optimizer.iterations == 32
    rows = [r for r in open(m.summary_writer.path)]
    assert any("generator/l1_loss" in r for r in rows) and any("discriminator/total_loss" in r for r in rows)
    assert m.checkpoint_manager.saved and os.path.exists(m.checkpoint_manager.saved[-1])


def test_tape_calls_are_refused_where_there_is_no_tape_path():
    ids = D.synthetic_indexed_ds(4, batch_size=4)
    indexed = M.Pix2PixIndexedModel(ids, None, "front2right", "tape-test")
    src_idx = next(iter(ids))[0]
    with tf.GradientTape():
        with pytest.raises(NotImplementedError, match="hooked"):
            indexed.generator(src_idx)
    dp = types.SimpleNamespace(rank=0, world=1)
    m = M.Pix2PixModel(D.synthetic_rgba_ds(4, batch_size=2), None, "front2right", "tape-test", lambda_l1=100.0, data_parallel=dp)
    src, _ = rg.synthetic_rgba_batch(np.random.default_rng(0), 2, S)
    with tf.GradientTape():
        with pytest.raises(NotImplementedError, match="one GPU"):
            m.generator(src)
