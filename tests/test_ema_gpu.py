"""-m gpu: the averaged generator.  The recurrence uses correctly rounded f32 operations only, so every
comparison here is bit for bit: the three kernels against the NumPy float32 restatement (tests/ema_oracle.py) and against
p2p_adam_flat_dev[_excl]; whole train steps with averaging on against a twin engine without; generation under engine.averaged()
against a fresh engine that was handed G.ema as its weights; the model classes, checkpoints and export files."""
import gc

import numpy as np
import pytest
import torch

from oracle import reference_graph as rg
from palette_and_histo_gan_amd import _lib as L
from palette_and_histo_gan_amd import dataset_utils as DU
from palette_and_histo_gan_amd import engine as E
from palette_and_histo_gan_amd import keras_weights as KW
from palette_and_histo_gan_amd import pix2pix_model as M
from tests import ema_oracle as EO
from tests import gpu_util as U

pytestmark = pytest.mark.gpu
B1, B2, EPS = 0.5, 0.999, 1e-7
LR_T = 3.1e-4               # what p2p_adam_tick would leave in lr_t_dev at some step: any step size serves
DECAY = 0.999
T_VALUES = (1, 9, 10, 8990, 100_000)
NAN_BITS = 0x7FC01234       # a quiet NaN with a payload: a kernel that read or wrote it would not hand back these bits


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _same_np(t, a):
    """device f32 tensor against a NumPy float32 array, as bits"""
    return np.array_equal(t.detach().cpu().numpy().view(np.int32), np.asarray(a, np.float32).view(np.int32))


@pytest.fixture(autouse=True)
def _release_device_memory():
    """the engines of a test (two or three generators with their Adam state) go back to the allocator before the next one"""
    yield
    gc.collect()
    torch.cuda.empty_cache()


# ---------------------------------------------------------------------------------------------------------------- kernels
def _inputs(n, seed):
    g = torch.Generator(device=U.DEV)
    g.manual_seed(seed)
    r = lambda scale: torch.randn(n, generator=g, device=U.DEV, dtype=torch.float32) * scale          # noqa: E731
    p, grad, m = r(0.02), r(1e-3), r(1e-3)
    v = r(1e-3) ** 2
    e = p + r(1e-3)
    e[::7] = p[::7]          # elements where the average already equals ... the OLD p: p' - e is then Adam's own step
    return p, grad, m, v, e


def _launch(kind, bufs, n, t_dev, lr_t, hole=None, warmup=True, decay=DECAY):
    p, g, m, v, e = bufs
    four = (U.ptr(p), U.ptr(g), U.ptr(m), U.ptr(v))
    hyper = (U.ptr(lr_t), B1, B2, EPS, 1.0)
    ema = (U.ptr(t_dev), decay, int(warmup))
    if kind == "adam":
        if hole is None:
            L.call("p2p_adam_flat_dev", *four, n, *hyper, U.stream())
        else:
            L.call("p2p_adam_flat_dev_excl", *four, n, hole[0], hole[1], *hyper, U.stream())
    elif hole is None:
        L.call("p2p_adam_ema_flat_dev", *four, U.ptr(e), n, *hyper, *ema, U.stream())
    else:
        L.call("p2p_adam_ema_flat_dev_excl", *four, U.ptr(e), n, hole[0], hole[1], *hyper, *ema, U.stream())


def _check_kernels(n, inputs, t, warmup, hole=None):
    lr_t = torch.full((1,), LR_T, dtype=torch.float32, device=U.DEV)
    t_dev = torch.full((1,), t, dtype=torch.int32, device=U.DEV)
    inside = torch.zeros(n, dtype=torch.bool, device=U.DEV)
    if hole is not None:
        inside[hole[0]:hole[1]] = True
    start = [x.clone() for x in inputs]
    if hole is not None:
        for x in start:
            _bits(x)[inside] = NAN_BITS
    where = f"n {n}, t {t}, warmup {warmup}, hole {hole}"
    ref = [x.clone() for x in start]
    _launch("adam", ref, n, t_dev, lr_t, hole)
    runs = []
    for _ in range(2):          # the second, identical launch sequence must give the same bits
        new = [x.clone() for x in start]
        _launch("ema", new, n, t_dev, lr_t, hole, warmup)
        alone = start[4].clone()
        L.call("p2p_ema_flat", U.ptr(alone), U.ptr(new[0]), n, U.ptr(t_dev), DECAY, int(warmup), U.stream())
        runs.append(new + [alone])
    new, again = runs
    for what, a, b in zip(("p", "g", "m", "v", "e", "e of p2p_ema_flat"), new, again):
        assert _same(a, b), f"{what} differs between two identical launch sequences ({where})"
    for what, a, b in zip(("p", "g", "m", "v"), ref, new):
        assert _same(a, b), f"{what} differs from p2p_adam_flat_dev's ({where})"
    live = ~inside
    want = EO.ema_step(start[4].cpu().numpy(), ref[0].cpu().numpy(), t, DECAY, warmup)
    live_np = live.cpu().numpy()
    assert _same_np(new[4][live], want[live_np]), f"e differs from the float32 restatement ({where})"
    assert _same(new[5][live], new[4][live]), f"p2p_ema_flat differs from the fused form ({where})"
    if bool(live.any()):
        assert not _same(new[4][live], start[4][live]), f"the average did not move: the test shows nothing ({where})"
    for what, x in zip(("p", "g", "m", "v", "e"), new):
        assert bool((_bits(x)[inside] == NAN_BITS).all()), f"{what} was touched inside the hole ({where})"


@pytest.mark.parametrize("n", [3, 4, 1027, 8_388_608 + 1031], ids=["tail-only", "one-vector", "vectors+tail", "past-the-grid-cap"])
def test_kernels_equal_the_float32_restatement_and_the_plain_adam_bit_for_bit(n):
    """n = 8 388 608 + 1031 lies past 8192 workgroups x 256 lanes x 4 elements: the stride loop runs a second trip"""
    inputs = _inputs(n, seed=n)
    for t in T_VALUES:
        for warmup in (True, False):
            _check_kernels(n, inputs, t, warmup)


@pytest.mark.parametrize("hole", [(0, 0), (5, 5), (5, 18), (8, 16), (1, 1026), (0, 1027)], ids=str)
def test_the_hole_is_neither_read_nor_written_in_any_of_the_five_buffers(hole):
    n = 1027
    inputs = _inputs(n, seed=99)
    for t, warmup in ((9, True), (100_000, False)):
        _check_kernels(n, inputs, t, warmup, hole)


def test_misaligned_and_missing_buffers_are_refused():
    n = 64
    p, g, m, v, e = _inputs(n + 4, seed=5)
    lr_t = torch.full((1,), LR_T, dtype=torch.float32, device=U.DEV)
    t_dev = torch.ones(1, dtype=torch.int32, device=U.DEV)
    with pytest.raises(L.P2PError, match="aligned"):
        _launch("ema", (p, g, m, v, e[1:]), n, t_dev, lr_t)
    with pytest.raises(L.P2PError, match="aligned"):
        L.call("p2p_ema_flat", U.ptr(e[1:]), U.ptr(p), n, U.ptr(t_dev), DECAY, 1, U.stream())
    with pytest.raises(L.P2PError):
        L.call("p2p_ema_flat", U.ptr(e), U.ptr(p), n, None, DECAY, 1, U.stream())
    with pytest.raises(L.P2PError, match="excluded range"):
        _launch("ema", (p, g, m, v, e), n, t_dev, lr_t, hole=(8, n + 1))


# ---------------------------------------------------------------------------------------------------------------- train steps
def _rgba_batches():
    out = {}
    for b in (2, 5):
        src, tgt = rg.synthetic_rgba_batch(np.random.default_rng(48 + b), b, 64)
        out[b] = torch.as_tensor(src).to(U.DEV), torch.as_tensor(tgt).to(U.DEV)
    return out


def _twins(dtype, level, head="tanh"):
    engs = []
    for _ in range(2):
        eng = E.Pix2PixEngine(1, 256, "softmax", 64, dtype, device=U.DEV, seed=47) if head == "softmax" else \
            E.Pix2PixEngine(4, 4, "tanh", 64, dtype, device=U.DEV, seed=47)
        eng.batch_invariant = False          # (the f32 parity mode keeps every launch: off, so that the levels bite in f32 too)
        eng.elide_dead_bottleneck = level
        engs.append(eng)
    engs[1].enable_ema(DECAY, warmup=True)
    assert _same(engs[1].G.ema, engs[1].G.params) and engs[0].G.ema is None
    return engs


def _assert_twin_state(off, on, what):
    for tag in ("params", "m", "v"):
        for sid in ("G", "D"):
            a, b = getattr(getattr(off, sid), tag), getattr(getattr(on, sid), tag)
            assert _same(a, b), f"{what}: {sid}.{tag} differs between the twins"


def _step_both(off, on, step, what, decay=DECAY):
    """one step on both twins: training undisturbed, and the new average = the restatement of the old one and the twin's new p"""
    e_prev = on.G.ema.cpu().numpy()
    a, b = step(off), step(on)
    assert _same(a, b), f"{what}: losses {a.tolist()} without, {b.tolist()} with averaging"
    _assert_twin_state(off, on, what)
    assert int(on.G.t_dev[0]) == on.G.t
    want = EO.ema_step(e_prev, off.G.params.cpu().numpy(), on.G.t, decay, True)
    assert _same_np(on.G.ema, want), f"{what}: G.ema differs from the restatement at t = {on.G.t}"
    if on._frozen is not None:
        lo, hi = on._frozen
        assert _same(on.G.ema[lo:hi], on.G.params[lo:hi]), f"{what}: the dead kernel's average left the kernel"


@pytest.mark.parametrize("level", [0, 1, 2])
@pytest.mark.parametrize("dtype", [L.BF16, L.F32], ids=["bf16", "f32"])
def test_fused_steps_are_undisturbed_and_the_average_follows_the_restatement(dtype, level):
    """four steps at B = 2 (eager, recorded, replayed twice) and one at B = 5.  t changes every step, so the replayed record shows
    that the kernels read it from G.t_dev; the decay changes before the last replayed step and takes effect without a recording."""
    off, on = _twins(dtype, level)
    batches = _rgba_batches()
    for k in range(1, 5):
        decay = DECAY
        if k == 4:
            decay = on.ema_decay = 0.9
            assert len(on._replays) == 1
        _step_both(off, on, lambda e: e.train_step_rgba(*batches[2], 100.0).clone(), f"step {k}", decay)
        assert len(on._replays) == len(off._replays) == (1 if k >= 2 else 0)
    names = [n for n, _ in next(iter(on._replays.values()))[1] if n is not None]
    want = "p2p_adam_ema_flat_dev_excl" if level == 2 else "p2p_adam_ema_flat_dev"
    assert want in names and "p2p_ema_flat" not in names
    assert names.count("p2p_adam_flat_dev") == 1, "only the discriminator steps through the plain entry point"
    assert np.float32(on.ema_decay) == np.float32(0.9)
    on.ema_decay = DECAY
    _step_both(off, on, lambda e: e.train_step_rgba(*batches[5], 100.0).clone(), "step 5 (B = 5)")


def test_the_tiled_adam_path_averages_in_a_pass_of_its_own():
    off, on = _twins(L.BF16, 1)
    off.fuse_adam = on.fuse_adam = True
    src, tgt = _rgba_batches()[2]
    for k in range(1, 4):
        _step_both(off, on, lambda e: e.train_step_rgba(src, tgt, 100.0).clone(), f"fuse_adam step {k}")


def test_the_indexed_step_is_undisturbed_and_averaged():
    off, on = _twins(L.BF16, 1, head="softmax")
    src, tgt, _ = DU.synthetic_indexed_batch(np.random.default_rng([47, 0]), 2, 64, 24)
    src, tgt = torch.as_tensor(src).to(U.DEV), torch.as_tensor(tgt).to(U.DEV)
    for k in range(1, 4):
        _step_both(off, on, lambda e: e.train_step_indexed(src, tgt, 0.01).clone(), f"indexed step {k}")


def test_a_tape_step_is_undisturbed_and_averaged(tmp_path, monkeypatch):
    """Pix2PixDiffAugmentModel.train_step is a GradientTape step: both optimizers go through apply_adam_store"""
    monkeypatch.chdir(tmp_path)
    ds = DU.synthetic_rgba_ds(4, batch_size=2)
    batches = list(iter(ds))
    models = [M.Pix2PixDiffAugmentModel(ds, ds, "front2right", "ema-tape-test", 100.0, seed=47, ema_decay=d) for d in (None, DECAY)]
    off, on = (m.engine for m in models)
    for k in range(2):
        e_prev = on.G.ema.cpu().numpy()
        la, lb = (m.train_step(batches[k], k, 1) for m in models)
        assert all(float(x) == float(y) for x, y in zip(la[0] + la[1], lb[0] + lb[1]))
        _assert_twin_state(off, on, f"tape step {k + 1}")
        assert on.G.t == k + 1
        assert _same_np(on.G.ema, EO.ema_step(e_prev, off.G.params.cpu().numpy(), on.G.t, DECAY, True))
        assert not _same(on.G.ema, on.G.params)


def test_a_captured_graph_averages_at_every_replay():
    off, on = _twins(L.BF16, 1)
    src, tgt = _rgba_batches()[2]
    step = on.graphed_rgba_step(2, 100.0)
    assert on.G.t == 0 and _same(on.G.ema, on.G.params), "the warm-up step of the capture left a trace in the average"
    for k in range(1, 4):
        e_prev = on.G.ema.cpu().numpy()
        step(src, tgt)
        torch.cuda.synchronize()
        assert on.G.t == k == int(on.G.t_dev[0])
        assert _same_np(on.G.ema, EO.ema_step(e_prev, on.G.params.cpu().numpy(), k, DECAY, True)), f"replay {k}"
        assert not _same(on.G.ema, on.G.params)


# ---------------------------------------------------------------------------------------------------------------- averaged generation
def _masks(b, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 2, size=s).astype(np.uint8) for s in rg.dropout_mask_shapes(b, 64)]


@pytest.mark.parametrize("dtype", [L.BF16, L.F32], ids=["bf16", "f32"])
def test_generate_under_averaged_equals_a_fresh_engine_holding_the_average(dtype):
    off, on = _twins(dtype, 1)
    fresh = E.Pix2PixEngine(4, 4, "tanh", 64, dtype, device=U.DEV, seed=3)
    fresh.batch_invariant = False          # as the twins: the same kernel variants in f32
    src, tgt = _rgba_batches()[2]
    masks = _masks(2, 11)
    step = lambda e: e.train_step_rgba(src, tgt, 100.0).clone()          # noqa: E731
    for k in range(3):
        _step_both(off, on, step, f"step {k + 1}")
    for round_ in range(2):          # the second round follows another step: the averaged copies must be refreshed
        live_G, live_W = on.G, on.W
        with on.averaged():
            got = on.generate(src, masks=masks)
            with pytest.raises(RuntimeError, match="averaged"):
                on.train_step_rgba(src, tgt, 100.0)
            with pytest.raises(RuntimeError, match="averaged"):
                on.set_params(g_values=None)
        assert on.G is live_G and on.W is live_W and not on._averaged
        fresh.set_params(g_values=on.G.export(on.G.ema))
        want = fresh.generate(src, masks=masks)
        assert _same(got, want), f"round {round_}: generate under averaged() differs from the fresh engine"
        assert not _same(got, on.generate(src, masks=masks)), "the live generator gives the same image: the test shows nothing"
        _step_both(off, on, step, f"the step after leaving the context (round {round_})")
    with pytest.raises(ZeroDivisionError):          # an exception inside leaves the live set behind too
        with on.averaged():
            1 / 0
    assert on.G is live_G and on.W is live_W and not on._averaged
    _step_both(off, on, step, "the step after an exception inside the context")
    with pytest.raises(RuntimeError, match="averaging is off"):
        with off.averaged():
            pass


def test_generate_indexed_under_averaged_equals_a_fresh_engine_holding_the_average():
    off, on = _twins(L.BF16, 1, head="softmax")
    fresh = E.Pix2PixEngine(1, 256, "softmax", 64, L.BF16, device=U.DEV, seed=3)
    src, tgt, _ = DU.synthetic_indexed_batch(np.random.default_rng([47, 1]), 2, 64, 24)
    src, tgt = torch.as_tensor(src).to(U.DEV), torch.as_tensor(tgt).to(U.DEV)
    masks = _masks(2, 12)
    step = lambda e: e.train_step_indexed(src, tgt, 0.01).clone()          # noqa: E731
    for k in range(3):
        _step_both(off, on, step, f"step {k + 1}")
    with on.averaged():
        idx, probs = on.generate_indexed(src, masks=masks, with_probs=True)
    fresh.set_params(g_values=on.G.export(on.G.ema))
    want_idx, want_probs = fresh.generate_indexed(src, masks=masks, with_probs=True)
    assert torch.equal(idx, want_idx) and _same(probs, want_probs)
    assert not _same(probs, on.generate_indexed(src, masks=masks, with_probs=True)[1])
    _step_both(off, on, step, "the step after leaving the context")


def test_outside_writes_restart_the_average_from_the_new_weights():
    off, on = _twins(L.BF16, 1)
    src, tgt = _rgba_batches()[2]
    on.train_step_rgba(src, tgt, 100.0)
    assert not _same(on.G.ema, on.G.params)
    vals = on.G.export()
    vals["last.bias"] = vals["last.bias"] + 0.25
    on.set_params(g_values=vals)
    assert _same(on.G.ema, on.G.params)
    on.disable_ema()
    assert on.G.ema is None and not on.ema_enabled


# ---------------------------------------------------------------------------------------------------------------- models
CKPT_KEYS = {"G", "G.m", "G.v", "G.t", "D", "D.m", "D.v", "D.t", "mask_counter", "step_count"}


def test_a_model_with_ema_decay_generates_and_evaluates_with_the_averaged_generator(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    train, test = DU.synthetic_rgba_ds(8, batch_size=4), DU.synthetic_rgba_ds(4, batch_size=4, seed=3)
    model = M.Pix2PixModel(train, test, "front2right", "ema-model-test", lambda_l1=100.0, ema_decay=0.99)
    assert model.engine.ema_enabled and np.float32(model.engine.ema_decay) == np.float32(0.99)
    model.fit(6, 3)
    eng = model.engine
    assert eng.G.t == 6 and not _same(eng.G.ema, eng.G.params)
    batch = next(iter(test))
    averaged, live = model.generate(batch), model.generate(batch, averaged=False)
    assert not _same(averaged, live)
    with eng.averaged():
        assert _same(averaged, eng.generate(batch[0]))
    assert _same(live, eng.generate(batch[0])) and _same(averaged, model.generate(batch, averaged=True))
    l1_train, l1_test = model.report_l1(num_images=2)
    assert np.isfinite(float(l1_train)) and np.isfinite(float(l1_test))
    real, fake = model.select_examples_for_evaluation(1, test)
    _, fake_live = model.select_examples_for_evaluation(1, test, averaged=False)
    assert not torch.equal(fake, fake_live)
    assert model.debug_discriminator_patches(next(iter(test.unbatch().take(1).batch(1))))["fake"].shape == (32, 32)
    # export: save_generator writes the average as the generator, with the marker; generator_ema puts it beside the live one
    path = model.save_generator()
    z = np.load(path)
    assert int(z["generator_averaged"]) == 1 and not any(k.startswith("generator_ema/") for k in z.files)
    ema_vals = eng.G.export(eng.G.ema)
    for i, (k, v) in enumerate(ema_vals.items()):
        assert np.array_equal(z[f"generator/{i:03d}:{k}"], v)
    both = KW.export_model(model, str(tmp_path / "both.npz"), with_optimizer=False, which=("generator", "generator_ema"))
    zb = np.load(both)
    assert "generator_averaged" not in zb.files
    assert np.array_equal(zb["generator/000:down1.kernel"], eng.G.export()["down1.kernel"])
    assert np.array_equal(zb["generator_ema/000:down1.kernel"], ema_vals["down1.kernel"])
    live_path = model.save_generator(averaged=False)
    assert "generator_averaged" not in np.load(live_path).files
    model.save_generator()
    model.load_generator()          # the round trip: the averaged weights become the generator (and the average restarts there)
    assert all(np.array_equal(a, b) for a, b in zip(eng.G.export().values(), ema_vals.values()))
    assert _same(eng.G.ema, eng.G.params)


def test_without_ema_decay_nothing_changes_and_averaged_is_refused(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    train = DU.synthetic_rgba_ds(4, batch_size=4)
    model = M.Pix2PixModel(train, train, "front2right", "ema-off-test", lambda_l1=100.0)
    assert not model.engine.ema_enabled and model.engine.G.ema is None
    batch = next(iter(train))
    model.train_step(batch, 0, 1)
    with pytest.raises(ValueError, match="averaged"):
        model.generate(batch, averaged=True)
    with pytest.raises(ValueError, match="averaged"):
        model.save_generator(averaged=True)
    assert _same(model.generate(batch), model.generate(batch, averaged=False))
    assert set(model.checkpoint.state()) == CKPT_KEYS
    z = np.load(model.save_generator())
    names = list(model.engine.G.shapes)
    assert set(z.files) == {"format"} | {f"generator/{i:03d}:{k}" for i, k in enumerate(names)}
    z = np.load(KW.export_model(model, str(tmp_path / "all.npz")))
    assert not any("ema" in k or "averaged" in k for k in z.files)


def test_checkpoints_carry_the_average_and_cross_restore(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    train = DU.synthetic_rgba_ds(8, batch_size=4)
    batches = list(iter(train))

    def make(decay):
        return M.Pix2PixModel(train, train, "front2right", "ema-ckpt-test", lambda_l1=100.0, dtype="f32", seed=47, ema_decay=decay)
    a = make(0.99)
    for k in range(3):
        a.train_step(batches[k % 2], k, 1)
    assert set(a.checkpoint.state()) == CKPT_KEYS | {"G.ema", "ema"} and a.checkpoint.state()["ema"] == (float(np.float32(0.99)), True)
    with_avg = a.checkpoint.save(str(tmp_path / "with.pt"))
    b = make(0.99)
    b.checkpoint.restore(with_avg)
    assert _same(a.engine.G.ema, b.engine.G.ema) and _same(a.engine.G.params, b.engine.G.params)
    for m in (a, b):
        m.train_step(batches[1], 3, 1)
    assert a.engine.G.t == b.engine.G.t == 4
    assert _same(a.engine.G.params, b.engine.G.params) and _same(a.engine.G.ema, b.engine.G.ema)
    assert not _same(a.engine.G.ema, a.engine.G.params)
    # a model without an average accepts the checkpoint and ignores the keys; its own checkpoint restarts the average of a model with one
    c = make(None)
    c.checkpoint.restore(with_avg)
    assert c.engine.G.ema is None and c.engine.G.t == 3
    without = c.checkpoint.save(str(tmp_path / "without.pt"))
    assert set(torch.load(without, map_location="cpu")) == CKPT_KEYS
    b.checkpoint.restore(without)
    assert b.engine.G.t == 3 and _same(b.engine.G.params, c.engine.G.params) and _same(b.engine.G.ema, b.engine.G.params)


@pytest.mark.parametrize("kind", ["indexed", "histogram", "palette", "diffaugment", "palette-snap", "augmented"])
def test_every_model_class_accepts_ema_decay(kind, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    kw = dict(ema_decay=0.5, ema_warmup=False)
    if kind == "indexed":
        ds = DU.synthetic_indexed_ds(2, batch_size=2)
        model = M.Pix2PixIndexedModel(ds, ds, "front2right", "ema-kinds-test", **kw)
    else:
        ds = DU.synthetic_rgba_ds(2, batch_size=2, palette_size=24)
        cls, args = {"histogram": (M.Pix2PixHistogramModel, (30.0, 1.0)), "palette": (M.Pix2PixPaletteModel, (100.0, 1.0)),
                     "diffaugment": (M.Pix2PixDiffAugmentModel, (100.0,)), "palette-snap": (M.Pix2PixPaletteSnapModel, (100.0,)),
                     "augmented": (M.Pix2PixAugmentedModel, (100.0,))}[kind]
        model = cls(ds, ds, "front2right", "ema-kinds-test", *args, **kw)
    eng = model.engine
    assert eng.ema_enabled and eng.ema_decay == 0.5 and eng._ema_warmup == 0
    batch = next(iter(ds))
    e_prev = eng.G.ema.cpu().numpy()
    model.train_step(batch, 0, 1)
    assert _same_np(eng.G.ema, EO.ema_step(e_prev, eng.G.params.cpu().numpy(), 1, 0.5, False))
    out = model.generate(batch)
    assert not torch.equal(out.float(), model.generate(batch, averaged=False).float()) or kind == "indexed"
