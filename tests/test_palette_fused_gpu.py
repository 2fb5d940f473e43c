"""-m gpu: the palette loss inside the fused train step: p2p_palette_loss and p2p_soft_palette_tv_bwd on their own,
engine.train_step_rgba(palette=) against the float64 oracle graph and against the hooked step, replayed against eager launching,
with an over-full palette, sharded over two ranks, and through Pix2PixPaletteModel(fused=True).fit().

Every bound is the one the project uses for the same comparison elsewhere: 8 x the float32 restatement's deviation from float64
for a kernel (tests/test_palette_gpu.py), 1e-5 / 1e-4 of the max-norm against the oracle graph and 1e-6 / 1e-5 against the hooked
step (test_hooked_step_against_the_oracle_graph_and_the_tape, whose comment explains the temperature 5e-2), and the bounds of
tests/test_dp_gpu.py::test_two_rank_models_equal_one_rank for two ranks against one."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from oracle import reference_graph as rg
from palette_and_histo_gan_amd import _lib as L
from palette_and_histo_gan_amd import dataset_utils as D
from palette_and_histo_gan_amd import palette as P
from palette_and_histo_gan_amd import parallel as PAR
from palette_and_histo_gan_amd import pix2pix_model as M
from tests import gpu_util as U
from tests import palette_oracle as O

pytestmark = pytest.mark.gpu
F64 = torch.float64
S = 64
bce = torch.nn.functional.binary_cross_entropy_with_logits


@pytest.fixture(autouse=True)
def _in_tmp(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)          # the models write their log and checkpoint folders under the working directory


# ---------------------------------------------------------------------------------------------------- p2p_palette_loss
LOSS_CASES = {"3x40": ((3, 40), [37, -1, 40]), "2x256": ((2, 256), [2, 256]), "5x24": ((5, 24), [24, 20, 24, 1, 24]), "1x1": ((1, 1), [1])}


def _loss_tables(case):
    """f32 tables as p2p_soft_palette_fwd lays them out: rows that sum to 1 over their valid slots, every fifth slot of h_fake
    exactly h_real's (sgn = 0); NaN wherever the kernel has no business reading a value into a sum (slots past n_b, the
    conformance of an image without a palette)"""
    (B, K), sizes = LOSS_CASES[case]
    rng = np.random.default_rng(7 + B * 1000 + K)
    h_real, h_fake = np.full((B, K), np.nan, np.float32), np.full((B, K), np.nan, np.float32)
    conf = rng.uniform(0.0, 0.05, size=B).astype(np.float32)
    for b, n in enumerate(sizes):
        if n <= 0:
            conf[b] = np.nan
            continue
        for h in (h_real, h_fake):
            w = rng.random(n) ** 4
            h[b, :n] = (w / w.sum()).astype(np.float32)
        h_fake[b, 0:n:5] = h_real[b, 0:n:5]
    return h_real, h_fake, conf, np.asarray(sizes, np.int32)


def _loss_call(h_real, h_fake, conf, sizes, inv_batch):
    B, K = h_real.shape
    out = torch.full((2,), float("nan"), dtype=torch.float32, device=U.DEV)
    args = [U.dev(h_real), U.dev(h_fake), U.dev(conf), U.dev(sizes, torch.int32)]
    L.call("p2p_palette_loss", B, K, *(U.ptr(a) for a in args), inv_batch, U.ptr(out), C.c_void_p(out.data_ptr() + 4), U.stream())
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _loss_reference(h_real, h_fake, conf, sizes, inv_batch, f):
    """(inv_batch sum_b tv_b, inv_batch sum_b conf_b) with every operation in the float type f, in slot and image order"""
    K = h_real.shape[1]
    tv_sum, conf_sum = f(0), f(0)
    for b, n in enumerate(sizes):
        n = min(int(n), K)
        if n <= 0:
            continue
        s = f(0)
        for k in range(n):
            s = f(s + abs(f(h_fake[b, k]) - f(h_real[b, k])))
        tv_sum = f(tv_sum + f(0.5) * s)
        conf_sum = f(conf_sum + f(conf[b]))
    return np.array([f(inv_batch) * tv_sum, f(inv_batch) * conf_sum], np.float64)


@pytest.mark.parametrize("case", list(LOSS_CASES))
def test_palette_loss_against_float64_with_the_float32_restatement_as_yardstick(case):
    h_real, h_fake, conf, sizes = _loss_tables(case)
    B = len(sizes)
    inv_batch = float(np.float32(1.0 / (B + 2)))                          # a global batch larger than the local one
    got = _loss_call(h_real, h_fake, conf, sizes, inv_batch)
    again = _loss_call(h_real, h_fake, conf, sizes, inv_batch)
    assert np.isfinite(got).all() and got.tobytes() == again.tobytes()      # NaN-filled outputs overwritten; identical bits
    want = _loss_reference(h_real, h_fake, conf, sizes, inv_batch, np.float64)
    yard = np.abs(_loss_reference(h_real, h_fake, conf, sizes, inv_batch, np.float32) - want)
    dev = np.abs(got.astype(np.float64) - want)
    print(f"palette loss {case}: f64 {want} yardstick {yard} kernel {dev}")
    assert (want[0] > 0 or h_real.shape[1] == 1) and (h_fake == h_real).any()      # sgn = 0 slots took part (K = 1: both rows are [1])
    assert (dev <= 8 * yard).all(), (dev, yard)


def test_an_images_loss_term_does_not_depend_on_the_batch():
    h_real, h_fake, conf, sizes = _loss_tables("5x24")
    inv_batch = 0.25
    for i in range(5):
        alone = _loss_call(h_real[i:i + 1], h_fake[i:i + 1], conf[i:i + 1], sizes[i:i + 1], inv_batch)
        only = np.zeros_like(sizes)                                          # the other four images: no palette, no contribution
        only[i] = sizes[i]
        among = _loss_call(h_real, h_fake, conf, only, inv_batch)
        assert alone.tobytes() == among.tobytes(), (i, alone, among)
    # and a batch beyond one staging group of the kernel (32 images): the sum over images in ascending order, restated in float32
    rng = np.random.default_rng(3)
    rep = rng.integers(0, 5, size=70)
    big = [x[rep] for x in (h_real, h_fake, conf, sizes)]
    inv = float(np.float32(1.0 / 70))
    got = _loss_call(*big, inv).astype(np.float64)
    want = _loss_reference(*big, inv, np.float64)
    yard = np.abs(_loss_reference(*big, inv, np.float32) - want)
    assert (np.abs(got - want) <= 8 * yard).all(), (got, want, yard)


# ---------------------------------------------------------------------------------------------------- p2p_soft_palette_tv_bwd
# the four input cases of tests/test_palette_gpu.py
CASES = {"3x6x10x40": ((3, 6, 10, 40), [1, 37, 40]), "2x16x16x256": ((2, 16, 16, 256), [2, 256]),
         "2x64x64x40": ((2, 64, 64, 40), [40, 33]), "3x6x10x40-skip": ((3, 6, 10, 40), [37, -1, 40])}
PAD = 64          # sentinel floats on either side of the output (256 bytes: the output stays 16-byte aligned)


def _guarded(n):
    buf = torch.full((n + 2 * PAD,), float("nan"), dtype=torch.float32, device=U.DEV)
    buf[:PAD] = 12345.0
    buf[PAD + n:] = 12345.0
    return buf


@pytest.mark.parametrize("tau", [1e-3, 5e-2])
@pytest.mark.parametrize("case", list(CASES))
def test_tv_backward_equals_the_backward_of_the_explicit_table_bit_for_bit(case, tau):
    (B, H, W, K), sizes = CASES[case]
    img, pal, sizes, _, _ = O.noisy_palette_case(100 + len(case) + K, B, H, W, K, sizes)
    rng = np.random.default_rng(11)
    img_d, pal_d, sizes_d = U.dev(img), U.dev(pal, torch.int32), U.dev(sizes, torch.int32)
    h_fake, _ = P.soft_palette_histogram(img_d, pal_d, sizes_d, tau)
    h_real = U.dev(rng.random((B, K)).astype(np.float32) * 0.1)
    h_real[:, ::5] = h_fake[:, ::5]                                            # exactly equal slots: sgn = 0
    h_fake, h_real = h_fake.contiguous(), h_real.contiguous()
    w_tv, w_conf = 50.0 * 0.5 / 3, 20.0 / 3
    valid = torch.arange(K, device=U.DEV)[None, :] < sizes_d[:, None]
    gh = (torch.sign(h_fake - h_real) * w_tv * valid).contiguous()
    gm = torch.full((B,), w_conf, dtype=torch.float32, device=U.DEV)
    assert bool((gh == 0)[valid].any()) and bool((gh > 0).any()) and bool((gh < 0).any())
    n = B * H * W * 4
    ref, got = _guarded(n), _guarded(n)
    common = (B, H, W, U.ptr(img_d), U.ptr(pal_d), U.ptr(sizes_d), K, tau)
    L.call("p2p_soft_palette_bwd", *common, U.ptr(gh), U.ptr(gm), C.c_void_p(ref.data_ptr() + 4 * PAD), U.stream())
    L.call("p2p_soft_palette_tv_bwd", *common, U.ptr(h_real), U.ptr(h_fake), w_tv, w_conf, C.c_void_p(got.data_ptr() + 4 * PAD), U.stream())
    torch.cuda.synchronize()
    assert bool(torch.isfinite(got).all()) and bool(got[PAD:PAD + n].any())
    assert bool((got[:PAD] == 12345.0).all()) and bool((got[PAD + n:] == 12345.0).all())
    assert torch.equal(got, ref)
    for b, nb in enumerate(sizes):
        if nb <= 0:
            assert not bool(got[PAD:PAD + n].view(B, -1)[b].any())


# ---------------------------------------------------------------------------------------------------- the fused step
LAM_L1, LAM_PAL, LAM_CONF = 100.0, 50.0, 20.0
TAU_STACK = 5e-2          # tests/test_palette_gpu.py: at 1e-3 the f32 networks' 1e-6 image error alone exceeds the 1e-4 bound
TERMS = (LAM_PAL, LAM_CONF, TAU_STACK)


def _params(seed):
    rng = np.random.default_rng(seed)
    Gp = rg.perturb_affine(rg.init_params(rg.generator_param_shapes(4, 4), rng, F64), rng)
    Dp = rg.perturb_affine(rg.init_params(rg.discriminator_param_shapes(4), rng, F64), rng)
    return rng, Gp, Dp


def _model(Gp=None, Dp=None, dtype="f32", fused=True, name="palette-fused-test", **kw):
    m = M.Pix2PixPaletteModel(D.synthetic_rgba_ds(4, batch_size=2), None, "front2right", name, lambda_l1=LAM_L1,
                              lambda_palette=LAM_PAL, lambda_conformance=LAM_CONF, temperature=TAU_STACK, dtype=dtype, seed=5,
                              fused=fused, **kw)
    if Gp is not None:
        m.engine.set_params({k: v.numpy() for k, v in Gp.items()}, {k: v.numpy() for k, v in Dp.items()})
    return m


def _oracle_step(Gp, Dp, src, tgt, masks):
    """the float64 graph of one palette step: ([total, adv, l1, tv], generator gradients, discriminator gradients, palette sizes)"""
    Gl = {k: v.clone().requires_grad_(True) for k, v in Gp.items()}
    Dl = {k: v.clone().requires_grad_(True) for k, v in Dp.items()}
    s64, t64 = torch.tensor(src, dtype=F64), torch.tensor(tgt, dtype=F64)
    fake = rg.unet_generator(Gl, s64, [torch.tensor(x, dtype=F64) for x in masks], "tanh")
    rp, fp = rg.patch_discriminator(Dl, t64, s64), rg.patch_discriminator(Dl, fake, s64)
    pal, sizes = O.extract_palette(tgt)
    h_real, _ = O.soft_palette(t64, pal, sizes, TAU_STACK)
    h_fake, m_fake = O.soft_palette(fake, pal, sizes, TAU_STACK)          # an image with size -1: zero rows, zero conformance
    adv, l1, tv = bce(fp, torch.ones_like(fp)), (t64 - fake).abs().mean(), O.palette_histogram_loss(h_real, h_fake)
    total = adv + LAM_L1 * l1 + LAM_PAL * tv + LAM_CONF * m_fake.mean()   # means over the whole batch
    d_total = bce(rp, torch.ones_like(rp)) + bce(fp, torch.zeros_like(fp))
    g = torch.autograd.grad(total, list(Gl.values()), retain_graph=True)
    d = torch.autograd.grad(d_total, list(Dl.values()))
    return ([float(x.detach()) for x in (total, adv, l1, tv)], {k: x.numpy() for k, x in zip(Gl, g)},
            {k: x.numpy() for k, x in zip(Dl, d)}, sizes)


def _grads(m):
    e = m.engine
    return ({k: v.copy() for k, v in e.G.export(e.G.grads).items()}, {k: v.copy() for k, v in e.D.export(e.D.grads).items()})


def _assert_grads(got, ref, bound, what):
    worst = []
    for k, r in ref.items():
        err, top = np.abs(got[k] - r).max(), np.abs(r).max()          # down6 normalises 1 x 1 maps: its kernel's gradient is 0
        worst.append((err / (top + 1e-30), k))
        assert err <= bound * top + 1e-12, (what, k, err, top)
    print(what, "worst", sorted(worst)[-3:])


def _fused_step(m, src, tgt, masks):
    out = m.engine.train_step_rgba(src, tgt, LAM_L1, masks=masks, apply_update=False, palette=TERMS).cpu().numpy()
    return out, _grads(m)


def test_fused_step_against_the_oracle_graph_and_the_hooked_step():
    # exactly the case of test_hooked_step_against_the_oracle_graph_and_the_tape
    rng, Gp, Dp = _params(90)
    src, tgt = rg.synthetic_rgba_batch(rng, 2, S, palette_size=24)
    masks = [rng.integers(0, 2, size=s).astype(np.uint8) for s in rg.dropout_mask_shapes(2, S)]
    m = _model(Gp, Dp)
    out, (gg, gd) = _fused_step(m, src, tgt, masks)
    want, g_ref, d_ref, sizes = _oracle_step(Gp, Dp, src, tgt, masks)
    print("fused", out[:4], "oracle", want)
    assert sizes.min() >= 20 and want[3] > 0.05 and LAM_PAL * want[3] > 0.05 * want[0]
    for i in range(4):
        assert abs(out[i] - want[i]) <= 1e-5 * abs(want[i]), (i, out[i], want[i])
    _assert_grads(gg, g_ref, 1e-4, "generator vs f64")
    _assert_grads(gd, d_ref, 1e-4, "discriminator vs f64")
    # the hooked step of a second model with the same weights
    m2 = _model(Gp, Dp, fused=False)
    out2 = m2.engine.train_step_rgba_hooked(src, tgt, m2.generator_loss, m2.discriminator_loss, masks=masks, apply_update=False).cpu().numpy()
    hg, hd = _grads(m2)
    for i in range(7):
        assert abs(out[i] - out2[i]) <= 1e-6 * abs(out2[i]), (i, out[i], out2[i])
    _assert_grads(gg, hg, 1e-5, "generator vs hooked")
    _assert_grads(gd, hd, 1e-5, "discriminator vs hooked")


def test_an_image_with_an_over_full_palette_contributes_nothing():
    rng, Gp, Dp = _params(91)
    src, tgt = rg.synthetic_rgba_batch(rng, 3, S, palette_size=24)
    tgt[1] = rng.uniform(-1, 1, size=(S, S, 4)).astype(np.float32)          # thousands of colours
    masks = [rng.integers(0, 2, size=s).astype(np.uint8) for s in rg.dropout_mask_shapes(3, S)]
    m = _model(Gp, Dp)
    out, (gg, gd) = _fused_step(m, src, tgt, masks)
    want, g_ref, d_ref, sizes = _oracle_step(Gp, Dp, src, tgt, masks)
    print("fused", out[:4], "oracle", want)
    assert sizes.tolist()[1] == -1 and min(sizes[0], sizes[2]) >= 20 and want[3] > 0.01
    assert m.engine.plans[3]["p_sizes"].tolist() == sizes.tolist()
    for i in range(4):
        assert abs(out[i] - want[i]) <= 1e-5 * abs(want[i]), (i, out[i], want[i])
    _assert_grads(gg, g_ref, 1e-4, "generator vs f64")
    _assert_grads(gd, d_ref, 1e-4, "discriminator vs f64")
    assert not bool(m.engine.plans[3]["p_dimg"].view(3, -1)[1].any())        # its palette gradient: exactly 0


# ---------------------------------------------------------------------------------------------------- replay
def _state(m):
    e = m.engine
    return [getattr(s, buf).clone() for s in (e.G, e.D) for buf in ("params", "m", "v")]


@pytest.mark.parametrize("pattern", ["4,4,4,4", "4,4,2,4,4,2,4,4,2"])
def test_replayed_palette_steps_are_bit_identical_to_eager_launching(pattern):
    """the second step of a batch size is recorded, later ones go through p2p_replay: after every step weights, Adam moments and
    the loss row equal those of a model that launches call by call"""
    sizes = [int(x) for x in pattern.split(",")]
    ragged = 2 in sizes
    ds = D.synthetic_rgba_ds(10 if ragged else 16, batch_size=4, palette_size=24, seed=13)
    batches = [b for _ in range(3 if ragged else 1) for b in ds]
    assert [int(b[0].shape[0]) for b in batches] == sizes
    a, b = _model(dtype="bf16"), _model(dtype="bf16")
    a.engine.replay_enabled, b.engine.replay_enabled = True, False
    replayed, orig = [], a.engine._replay

    def counting(key, *args, **kw):
        replayed.append(t)
        return orig(key, *args, **kw)
    a.engine._replay = counting
    for t, bt in enumerate(batches):
        la, lb = (torch.stack(list(g + d)) for g, d in (m.train_step(bt, t, 1) for m in (a, b)))
        torch.cuda.synchronize()
        assert torch.equal(la, lb), (t, la, lb)
        assert bool(torch.isfinite(la).all()) and 0.0 < float(la[3]) <= 1.0
        for x, y in zip(_state(a), _state(b)):
            assert torch.equal(x, y), t
    assert replayed == ([3, 4, 6, 7, 8] if ragged else [2, 3]), replayed
    assert len(a.engine._replays) == (2 if ragged else 1) and not b.engine._replays and not a._custom_hooks


# ---------------------------------------------------------------------------------------------------- data parallel
DP_CASES = [("even", 4), ("ragged", 5), ("empty", 1)]          # (tag, global batch): 2 + 2, 3 + 2, 1 + 0 images per rank


def _dp_step(Bg, dp):
    batch = next(iter(D.synthetic_rgba_ds(Bg, batch_size=Bg, palette_size=24, seed=9)))
    m = M.Pix2PixPaletteModel(None, None, "front2right", "dp-palette-test", LAM_L1, LAM_PAL, LAM_CONF, TAU_STACK, fused=True,
                              dtype="f32", data_parallel=dp)
    g_loss, d_loss = m.train_step(batch, 0, 1)
    torch.cuda.synchronize()
    e = m.engine
    assert not m._custom_hooks
    return (np.array([float(x) for x in g_loss + d_loss]), e.G.grads.cpu().numpy().copy(), e.D.grads.cpu().numpy().copy(),
            e.G.params.cpu().numpy().copy())


def _dp_worker(rank, world, port, q, tmp):
    import faulthandler
    import sys
    faulthandler.dump_traceback_later(int(os.environ.get("P2P_TEST_DUMP_AFTER", "240")), exit=True, file=sys.stderr)       # a deadlocked rank reports where it stands
    os.chdir(tmp)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    torch.cuda.set_device(0)
    try:
        comm = PAR.DataParallel("cuda:0", backend="gloo")
        for tag, Bg in DP_CASES:
            res = _dp_step(Bg, comm)
            print(f"[rank {rank}] case {tag} done", flush=True)
            if rank == 0:
                q.put((tag,) + res)
            comm.barrier()
        comm.destroy()
    except BaseException:       # a failing rank must not leave the parent (and its sibling) waiting
        import traceback
        q.put(("error", rank, traceback.format_exc()))
        q.close()
        q.join_thread()
        os._exit(1)
    q.close()
    q.join_thread()
    os._exit(0)          # skip interpreter teardown of a process that shares the GPU with its sibling rank


@pytest.mark.timeout(1200)
def test_two_rank_fused_palette_models_equal_one_rank(tmp_path):
    world, port = 2, 29671
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_dp_worker, args=(r, world, port, q, str(tmp_path))) for r in range(world)]
    for p in procs:
        p.start()
    got = {}
    for _ in DP_CASES:
        item = q.get(timeout=600)
        if item[0] == "error":
            for p in procs:
                p.kill()
            pytest.fail(f"rank {item[1]} failed:\n{item[2]}")
        got[item[0]] = item[1:]
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0, f"rank process exited with {p.exitcode}"
    for tag, Bg in DP_CASES:
        l1, g1, d1, p1 = _dp_step(Bg, None)
        l2, g2, d2, p2 = got[tag]
        print(tag, "one rank", l1, "two ranks", l2)
        assert 0.0 < l1[3] <= 1.0
        np.testing.assert_allclose(l2, l1, rtol=5e-6, atol=1e-9, err_msg=tag)
        assert np.abs(g2 - g1).max() <= 2e-5 * np.abs(g1).max(), tag
        assert np.abs(d2 - d1).max() <= 2e-5 * np.abs(d1).max(), tag
        assert np.abs(p2 - p1).max() < 3e-5, tag       # same Adam step (rounding-level gradients may move by a fraction of lr)


# ---------------------------------------------------------------------------------------------------- fit and checkpoints
def test_a_sixteen_step_fused_fit_logs_the_palette_loss_and_saves():
    train = D.synthetic_rgba_ds(8, batch_size=4, palette_size=24)
    m = M.Pix2PixPaletteModel(train, train, "front2right", "palette-fused-fit-test", lambda_l1=100.0, lambda_palette=10.0,
                              lambda_conformance=1.0, fused=True)
    w0 = m.engine.G.params.clone()
    m.fit(16, 8)
    assert not m._custom_hooks and m.engine.G.t == 16 and not torch.equal(m.engine.G.params, w0)
    assert len(m.engine._replays) == 1                                        # the steps were replayed
    rows = [json.loads(r) for r in open(m.summary_writer.path)]
    pal = [r["value"] for r in rows if r["name"] == "generator/palette_loss"]
    print("palette loss", pal)
    assert len(pal) == 16 and all(np.isfinite(r["value"]) for r in rows) and all(0.0 <= v <= 1.0 for v in pal)
    assert m.checkpoint_manager.saved and os.path.exists(m.checkpoint_manager.saved[-1])


def test_a_restored_checkpoint_resumes_bit_exactly(tmp_path):
    batches = list(D.synthetic_rgba_ds(8, batch_size=4, palette_size=24, seed=21))
    a = _model(name="palette-fused-ckpt-a", ema_decay=0.99)
    for t in range(3):
        a.train_step(batches[t % 2], t, 1)
    path = a.checkpoint.save(str(tmp_path / "fused.pt"))
    b = _model(name="palette-fused-ckpt-b", ema_decay=0.99)
    b.checkpoint.restore(path)
    for t in (3, 4):
        la, lb = (torch.stack(list(g + d)) for g, d in (m.train_step(batches[t % 2], t, 1) for m in (a, b)))
        torch.cuda.synchronize()
        assert torch.equal(la, lb), (t, la, lb)
        for x, y in zip(_state(a), _state(b)):
            assert torch.equal(x, y), t
        assert torch.equal(a.engine.G.ema, b.engine.G.ema)
    assert a.engine.G.t == b.engine.G.t == 5
