"""-m gpu: the whole Pix2Pix train step (pix2pix_model.py:62-89) on the GPU against the CPU oracle:
losses, every gradient tensor, and the post-Adam weights over two consecutive steps."""
import numpy as np
import pytest
import torch

from oracle import reference_graph as rg
from palette_and_histo_gan_amd import _lib as L
from palette_and_histo_gan_amd import engine as E

pytestmark = pytest.mark.gpu
F64 = torch.float64


def setup_case(B, S, seed, in_ch=4, out_ch=4):
    rng = np.random.default_rng(seed)
    Gp = rg.perturb_affine(rg.init_params(rg.generator_param_shapes(in_ch, out_ch), rng, F64), rng)
    Dp = rg.perturb_affine(rg.init_params(rg.discriminator_param_shapes(in_ch), rng, F64), rng)
    src, tgt = rg.synthetic_rgba_batch(rng, B, S)
    masks = [rng.integers(0, 2, size=s).astype(np.uint8) for s in rg.dropout_mask_shapes(B, S)]
    return rng, Gp, Dp, src, tgt, masks


def to_np(p):
    return {k: v.numpy() for k, v in p.items()}


def grad_report(eng_grads, ref_grads):
    """worst (tensor, max-norm relative error) and worst (tensor, L2 relative error)"""
    worst_max, worst_l2 = ("", 0.0), ("", 0.0)
    for k, ref in ref_grads.items():
        ref = ref.numpy().astype(np.float64)
        got = eng_grads[k].astype(np.float64)
        scale = np.abs(ref).max()
        if scale == 0.0:
            emax = el2 = float(np.abs(got).max())
        else:
            emax = float(np.abs(got - ref).max() / scale)
            el2 = float(np.linalg.norm(got - ref) / np.linalg.norm(ref))
        if emax > worst_max[1]:
            worst_max = (k, emax)
        if el2 > worst_l2[1]:
            worst_l2 = (k, el2)
    return worst_max, worst_l2


def run_case(dtype, use_mfma, seed=21, B=2):
    S = 64
    rng, Gp, Dp, src, tgt, masks = setup_case(B, S, seed)
    tm = [torch.tensor(m, dtype=F64) for m in masks]
    if dtype == L.BF16:      # same graph, same bf16 storage points (oracle/reference_graph.storage_dtype)
        with rg.storage_dtype(torch.bfloat16):
            ref = rg.train_step_rgba(Gp, Dp, torch.tensor(src, dtype=F64), torch.tensor(tgt, dtype=F64), tm, lambda_l1=100.0)
    else:
        ref = rg.train_step_rgba(Gp, Dp, torch.tensor(src, dtype=F64), torch.tensor(tgt, dtype=F64), tm, lambda_l1=100.0)
    eng = E.Pix2PixEngine(4, 4, "tanh", S, dtype, use_mfma=use_mfma)
    eng.set_params(to_np(Gp), to_np(Dp))
    out = eng.train_step_rgba(src, tgt, 100.0, masks=masks, apply_update=False).cpu().numpy()
    g_ref, d_ref = ref["g_loss"], ref["d_loss"]
    want = np.array([g_ref[0], g_ref[1], g_ref[2], 0.0, d_ref[0], d_ref[1], d_ref[2]])
    print("losses got", out, "want", want)
    wg = grad_report(eng.G.export(eng.G.grads), ref["g_grads"])
    wd = grad_report(eng.D.export(eng.D.grads), ref["d_grads"])
    print("worst G grad (max-norm, L2)", wg, "worst D grad", wd)
    return out, want, wg, wd


def test_train_step_f32_mfma_matches_oracle():
    """The parity gate: f32 storage, exact-f32 MFMA.  Losses within 1e-4 relative (BASELINE.json north_star),
    every gradient tensor within 1e-4 of its max-norm."""
    out, want, wg, wd = run_case(L.F32, True)
    for i in (0, 1, 2, 4, 5, 6):
        assert abs(out[i] - want[i]) <= 1e-4 * abs(want[i]), (i, out[i], want[i])
    assert wg[0][1] < 1e-4 and wd[0][1] < 1e-4


@pytest.mark.parametrize("B", [1, 3, 5])
def test_train_step_f32_odd_batches(B):
    """batch sizes that are not powers of two: B = 1 is what the reference's evaluation feeds (`.batch(1)`, pix2pix_model.py:107-
    115), ragged tail batches of an epoch are 1..3 samples (dataset_utils.py:223 has no drop_remainder); tiles that hold four
    8x8 images or two strips are then partly empty"""
    out, want, wg, wd = run_case(L.F32, True, seed=40 + B, B=B)
    for i in (0, 1, 2, 4, 5, 6):
        assert abs(out[i] - want[i]) <= 1e-4 * abs(want[i]), (i, out[i], want[i])
    # Typical worst tensor: 5e-6.  Roughly one case in four has ONE gated element (ReLU / LeakyReLU / dropout) whose
    # pre-activation is ~1e-6 from zero and lands on the other side in f32: the f64 oracle re-run in f32 shows the very same
    # outlier (tests/diagnostics/odd_batch_errors.py; e.g. seed 61: up4.kernel 0.198 of its max-norm, 0.009 in L2, for the
    # oracle as for the engine), so the bound on every tensor is the L2 one and the max-norm bound holds for the D tensors
    assert wg[1][1] < 2e-2 and wd[0][1] < 1e-4


@pytest.mark.parametrize("B", [1, 3])
def test_train_step_bf16_odd_batches(B):
    out, want, wg, wd = run_case(L.BF16, True, seed=50 + B, B=B)
    for i in (0, 1, 2, 4, 5, 6):
        assert abs(out[i] - want[i]) <= 2e-3 * abs(want[i]), (i, out[i], want[i])
    assert wg[1][1] < 0.3 and wd[1][1] < 0.3


def test_train_step_f32_direct_kernels_match_oracle():
    """Same step through the non-MFMA kernels.  Their different summation order can flip the sign of a ReLU
    input that is ~1e-6 from zero, which moves a handful of gradient entries by O(1e-2) of the max-norm, so
    the gradient check is in the L2 norm."""
    out, want, wg, wd = run_case(L.F32, False)
    for i in (0, 1, 2, 4, 5, 6):
        assert abs(out[i] - want[i]) <= 1e-4 * abs(want[i]), (i, out[i], want[i])
    assert wg[1][1] < 2e-2 and wd[1][1] < 1e-4


@pytest.mark.parametrize("use_mfma", [True, False])
def test_train_step_bf16_matches_bf16_storage_oracle(use_mfma):
    """Throughput mode (bf16 storage, f32 accumulate) against the oracle run with the same bf16 storage points.
    Tolerances (measured, documented in DESIGN.md): losses 2e-3 relative, gradients 0.25 in the L2 norm and
    cosine > 0.97 -- the engine also stores backward intermediates (d activations) in bf16, which the
    oracle's autograd does not, and the InstanceNorm backward subtracts means of those rounded values."""
    out, want, wg, wd = run_case(L.BF16, use_mfma)
    for i in (0, 1, 2, 4, 5, 6):
        assert abs(out[i] - want[i]) <= 2e-3 * abs(want[i]), (i, out[i], want[i])
    assert wg[1][1] < 0.25 and wd[1][1] < 0.25


def test_two_adam_steps_match_oracle_f32():
    """Two consecutive steps (Adam t = 1, 2; weight copies refreshed in between).  The step-2 losses depend on every
    updated weight and must match to 1e-4.  Per-entry comparison of the weights is ill-posed for entries whose
    gradient is at rounding level (Adam moves them by ~lr * sign(g)), so the update DIRECTION of each tensor is
    compared instead (cosine of the accumulated update) plus its magnitude."""
    B, S = 2, 64
    rng, Gp, Dp, src, tgt, masks = setup_case(B, S, 22)
    eng = E.Pix2PixEngine(4, 4, "tanh", S, L.F32)
    eng.set_params(to_np(Gp), to_np(Dp))
    f32 = lambda v: v.numpy().astype(np.float32).astype(np.float64)      # what the engine's f32 masters hold
    start = dict({k: v.numpy().copy() for k, v in Gp.items()}, **{"D." + k: v.numpy().copy() for k, v in Dp.items()})
    start32 = dict({k: f32(v) for k, v in Gp.items()}, **{"D." + k: f32(v) for k, v in Dp.items()})
    gm, gv, dm, dv = (rg.zeros_like_params(Gp), rg.zeros_like_params(Gp), rg.zeros_like_params(Dp), rg.zeros_like_params(Dp))
    tm = [torch.tensor(m, dtype=F64) for m in masks]
    for t in (1, 2):
        ref = rg.train_step_rgba(Gp, Dp, torch.tensor(src, dtype=F64), torch.tensor(tgt, dtype=F64), tm, lambda_l1=100.0)
        Gp, gm, gv = rg.keras_adam(Gp, ref["g_grads"], gm, gv, t)
        Dp, dm, dv = rg.keras_adam(Dp, ref["d_grads"], dm, dv, t)
        out = eng.train_step_rgba(src, tgt, 100.0, masks=masks).cpu().numpy()
        assert abs(out[0] - ref["g_loss"][0]) < 1e-4 * abs(ref["g_loss"][0]), t
        assert abs(out[4] - ref["d_loss"][0]) < 1e-4 * abs(ref["d_loss"][0]), t
    assert eng.G.t == 2 and eng.D.t == 2
    got = dict(eng.G.export(), **{"D." + k: v for k, v in eng.D.export().items()})
    want = dict({k: v.numpy() for k, v in Gp.items()}, **{"D." + k: v.numpy() for k, v in Dp.items()})
    for k in want:
        du_ref, du_got = (want[k] - start[k]).ravel(), (got[k] - start32[k]).ravel().astype(np.float64)
        if np.abs(du_ref).max() == 0.0:          # down6.kernel / down6.gamma: dead at S=64
            assert np.abs(du_got).max() == 0.0, k
            continue
        cos = float(du_ref @ du_got / (np.linalg.norm(du_ref) * np.linalg.norm(du_got)))
        assert cos > 0.995, (k, cos)
        assert abs(np.linalg.norm(du_got) / np.linalg.norm(du_ref) - 1.0) < 1e-2, k


@pytest.mark.parametrize("dtype", [L.F32, L.BF16])
@pytest.mark.parametrize("hist", [False, True])
def test_whole_pixel_stores_equal_the_partial_ones(dtype, hist):
    """P2P_FULL_PIXELS: the source channels of the last concat buffer come from up6's normalisation launch and the fake half of
    the discriminator input is written as whole [fake | source] pixels -- same bytes in the same buffers, so three steps give
    the same weights bit for bit; only the L1 sum changes its (fixed) order."""
    B, S = 3, 64
    rng, Gp, Dp, src, tgt, masks = setup_case(B, S, seed=78)
    engines, losses = [], []
    for whole in (True, False):
        eng = E.Pix2PixEngine(4, 4, "tanh", S, dtype)
        eng.full_pixels = whole
        eng.set_params(to_np(Gp), to_np(Dp))
        for _ in range(3):
            out = eng.train_step_rgba(src, tgt, 100.0, lambda_hist=1.0 if hist else None, masks=masks)
        torch.cuda.synchronize()
        engines.append(eng)
        losses.append(out.cpu().numpy())
    a, b = engines
    assert a._c6_tail(a.plan(B)) and not b._c6_tail(b.plan(B))
    assert torch.equal(a.plan(B)["c"][6].t, b.plan(B)["c"][6].t) and torch.equal(a.plan(B)["dcat"].t, b.plan(B)["dcat"].t)
    np.testing.assert_allclose(losses[0], losses[1], rtol=3e-6)
    for sa, sb in ((a.G, b.G), (a.D, b.D)):
        for buf in ("params", "m", "v"):
            assert torch.equal(getattr(sa, buf), getattr(sb, buf)), buf


def test_whole_pixel_stores_of_the_indexed_batch_equal_the_partial_ones():
    """P2P_FULL_PIXELS, indexed model: p2p_pack_pair_idx writes whole [source 0..] / [target source 0..] / [0 source 0..] pixels
    where the generic packers stored single channels; same buffers, same weights after three steps."""
    from palette_and_histo_gan_amd import dataset_utils as DU
    B, S = 3, 64
    batches = list(DU.synthetic_indexed_ds(3 * B, batch_size=B, seed=9))
    engines, losses = [], []
    for whole in (True, False):
        eng = E.Pix2PixEngine(1, 256, "softmax", S, L.BF16, seed=8)
        eng.full_pixels = whole
        for b in batches:
            out = eng.train_step_indexed(b[0], b[1], 0.01)
        torch.cuda.synchronize()
        engines.append(eng)
        losses.append(out.cpu().numpy())
    a, b = engines
    assert torch.equal(a.plan(B)["c"][6].t, b.plan(B)["c"][6].t) and torch.equal(a.plan(B)["dcat"].t, b.plan(B)["dcat"].t)
    assert torch.equal(a.plan(B)["src"].t, b.plan(B)["src"].t)
    np.testing.assert_array_equal(losses[0], losses[1])
    for sa, sb in ((a.G, b.G), (a.D, b.D)):
        for buf in ("params", "m", "v"):
            assert torch.equal(getattr(sa, buf), getattr(sb, buf)), buf


@pytest.mark.parametrize("dtype", [L.F32, L.BF16])
def test_adam_fused_with_the_weight_copies_equals_the_two_launch_form(dtype):
    """p2p_adam_prep_batched (Adam + operand copies in one pass) against p2p_adam_flat_dev followed by
    p2p_weight_prep_batched: same masters, moments and copies after three steps (the expressions are the same; the compiler
    may contract them differently in the two kernels, hence a last-bit tolerance on the masters)."""
    B, S = 2, 64
    rng, Gp, Dp, src, tgt, masks = setup_case(B, S, seed=77)
    engines = []
    for fused in (True, False):
        eng = E.Pix2PixEngine(4, 4, "tanh", S, dtype)
        eng.fuse_adam = fused
        eng.set_params(to_np(Gp), to_np(Dp))
        for _ in range(3):
            eng.train_step_rgba(src, tgt, 100.0, masks=masks)
        torch.cuda.synchronize()
        engines.append(eng)
    a, b = engines
    for sa, sb in ((a.G, b.G), (a.D, b.D)):
        assert sa.t == sb.t == 3
        for buf in ("params", "m", "v"):
            x, y = getattr(sa, buf), getattr(sb, buf)
            assert float((x - y).abs().max()) <= 1e-6 * float(y.abs().max()), buf
    for key, lw in a.W.items():
        for name in ("wt", "wn", "wd"):
            ca, cb = getattr(lw, name), getattr(b.W[key], name)
            assert (ca is None) == (cb is None)
            if ca is not None:          # the copies follow their own masters: compare through f32 with the bf16 step as the unit
                assert float((ca.float() - cb.float()).abs().max()) <= 2 ** -7 * float(cb.float().abs().max()) + 1e-12, (key, name)
    # the copies ARE the rounded masters (layer with both orientations: up3)
    lw = a.W[("G", "up3")]
    w = a.G.view(a.G.params, "up3.kernel").reshape(16, lw.cg, lw.cd)
    if lw.wn is not None:
        assert torch.equal(lw.wn.view(16, lw.cg, lw.cd), w.to(lw.wn.dtype))
    assert torch.equal(lw.wt.view(16, lw.cd, lw.cg), w.transpose(1, 2).to(lw.wt.dtype))


@pytest.mark.parametrize("kind,B", [("baseline", 4), ("histogram", 4), ("indexed", 4), ("baseline", 256), ("histogram", 64)])
def test_host_side_step_replay_is_bit_identical_to_eager_launching(kind, B):
    """From the third step of a kind on the engine re-issues the recorded step through ONE p2p_replay call (same entry points,
    order, streams; batch pointers and result tensor behind re-usable slots) -- at every batch size since round 5, the benchmarked
    B = 256 included.  Six steps over changing batches, an evaluation call in between: weights, Adam state and every loss must
    equal the eager engine's bit for bit."""
    from palette_and_histo_gan_amd import dataset_utils as DU
    S = 64
    if kind == "indexed":
        batches = list(DU.synthetic_indexed_ds(6 * B, batch_size=B, seed=3))
    else:
        batches = list(DU.synthetic_rgba_ds(6 * B, batch_size=B, palette_size=24, seed=3))
    runs = []
    for replay in (True, False):
        eng = E.Pix2PixEngine(1, 256, "softmax", S, L.BF16, seed=5) if kind == "indexed" else E.Pix2PixEngine(4, 4, "tanh", S, L.BF16, seed=5)
        eng.replay_enabled = replay
        losses = []
        for t, b in enumerate(batches):
            if kind == "indexed":
                losses.append(eng.train_step_indexed(b[0], b[1], 0.01))
            else:
                losses.append(eng.train_step_rgba(b[0], b[1], 30.0, lambda_hist=1.0 if kind == "histogram" else None))
            if t == 3:        # an evaluation between train steps uses the same buffers and must not disturb the recorded list
                (eng.generate_indexed(b[0]) if kind == "indexed" else eng.generate(b[0]))
        torch.cuda.synchronize()
        assert len(eng._replays) == (1 if replay else 0)
        runs.append((torch.stack(losses).cpu(), eng))
    (la, a), (lb, b) = runs
    assert torch.equal(la, lb), (la - lb).abs().max()
    for sa, sb in ((a.G, b.G), (a.D, b.D)):
        assert sa.t == sb.t == len(batches) and int(sa.t_dev[0]) == len(batches)
        for buf in ("params", "m", "v"):
            assert torch.equal(getattr(sa, buf), getattr(sb, buf)), buf
    assert a.step_count == b.step_count == len(batches)
    assert int(a.mask_counter_dev[0]) == int(b.mask_counter_dev[0])


@pytest.mark.parametrize("dtype", [L.BF16, L.F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("kind", ["baseline", "indexed"])
def test_an_epochs_ragged_batch_pattern_replays_bit_identically(kind, dtype):
    """batch() has no drop_remainder (dataset_utils.py:137): 21 samples at batch 8 arrive as 8, 8, 5 every epoch.  Recordings are
    keyed by batch and plans are kept per batch, while the parameter stores, Adam state, device step counters and the dropout
    counter are shared.  Three epochs on a replaying engine and on one that launches eagerly, from the same weights and seed: the
    first step of a batch size is eager, the second one is recorded, later ones are replayed -- both B = 8 steps of the second
    epoch and every step of the third (B = 5 included) run through p2p_replay, interleaved with the other size.  Loss rows,
    parameters, Adam moments, step counters and the mask counter are bit-identical after every step."""
    from palette_and_histo_gan_amd import dataset_utils as DU
    S, epochs = 64, 3
    ds = (DU.synthetic_indexed_ds if kind == "indexed" else DU.synthetic_rgba_ds)(21, batch_size=8, seed=11)
    batches = [b for _ in range(epochs) for b in ds]
    assert [int(b[0].shape[0]) for b in batches] == [8, 8, 5] * epochs
    engs, replayed = [], []
    for replay in (True, False):
        eng = E.Pix2PixEngine(1, 256, "softmax", S, dtype, seed=5) if kind == "indexed" else E.Pix2PixEngine(4, 4, "tanh", S, dtype, seed=5)
        eng.replay_enabled = replay
        engs.append(eng)
    a, b = engs
    orig = a._replay

    def counting(key, *args, **kw):
        replayed.append(len(rows))
        return orig(key, *args, **kw)
    a._replay = counting
    rows = []
    for t, bt in enumerate(batches):
        if kind == "indexed":
            la, lb = (e.train_step_indexed(bt[0], bt[1], 0.01) for e in engs)
        else:
            la, lb = (e.train_step_rgba(bt[0], bt[1], 100.0) for e in engs)
        torch.cuda.synchronize()
        rows.append(la)
        assert torch.equal(la, lb), f"step {t + 1} (B={int(bt[0].shape[0])}): loss rows differ by {(la - lb).abs().max()}"
        for sid, sa, sb in (("G", a.G, b.G), ("D", a.D, b.D)):
            assert sa.t == sb.t == t + 1 and int(sa.t_dev[0]) == int(sb.t_dev[0]) == t + 1, f"step {t + 1}: {sid} step counters"
            for buf in ("params", "m", "v"):
                assert torch.equal(getattr(sa, buf), getattr(sb, buf)), f"step {t + 1} (B={int(bt[0].shape[0])}): {sid}.{buf}"
        assert int(a.mask_counter_dev[0]) == int(b.mask_counter_dev[0]) == t + 1, f"step {t + 1}: mask counter"
    assert replayed == [3, 4, 6, 7, 8], f"steps issued through p2p_replay (0-based): {replayed}"
    assert len(a._replays) == 2 and len(b._replays) == 0


@pytest.mark.parametrize("B,replay", [(4, True), (256, False), (256, True)])
def test_forks_on_the_kernels_own_completion_signal_order_the_streams_like_event_records(B, replay):
    """Round 5: the weight-gradient forks behind p2p_norm_act_bwd / p2p_act_bwd ride on that kernel's own completion signal
    (p2p_arm_stop_event -> hipExtLaunchKernelGGL stop event) instead of an event record between two main-stream kernels.  The side
    stream must still see the kernel's output: four steps leave exactly the weights and Adam moments of the engine that records
    every fork (a weight gradient that started early would read a half-written d(raw) tensor), eager and replayed."""
    from palette_and_histo_gan_amd import dataset_utils as DU
    batches = list(DU.synthetic_rgba_ds(4 * B, batch_size=B, palette_size=24, seed=17))
    runs = []
    for armed in (True, False):
        eng = E.Pix2PixEngine(4, 4, "tanh", 64, L.BF16, seed=3)
        eng.side.stop_event_forks = armed
        eng.replay_enabled = replay
        armed_calls, orig = [0], E._op
        try:
            def spy(name, *a):
                armed_calls[0] += name == "p2p_arm_stop_event"
                return orig(name, *a)
            E._op = spy
            losses = [eng.train_step_rgba(b[0], b[1], 100.0) for b in batches]
        finally:
            E._op = orig
        torch.cuda.synchronize()
        assert (armed_calls[0] > 0) == armed
        runs.append((torch.stack(losses).cpu(), eng))
    (la, a), (lb, b) = runs
    assert torch.equal(la, lb), (la - lb).abs().max()
    for sa, sb in ((a.G, b.G), (a.D, b.D)):
        for buf in ("params", "m", "v"):
            assert torch.equal(getattr(sa, buf), getattr(sb, buf)), buf


def test_whole_step_hipgraph_replay_equals_eager_launching():
    """engine.graphed_rgba_step captures one train step (every kernel, the forks and joins between the streams through the
    device-only events) and replays it; four steps over changing batches must leave the same weights, moments and losses as four
    eager steps, bit for bit (Adam's step count / step size and the dropout counter live in device memory)."""
    from palette_and_histo_gan_amd import dataset_utils as DU
    B, S = 4, 64
    batches = list(DU.synthetic_rgba_ds(4 * B, batch_size=B, palette_size=24, seed=11))
    runs = []
    for graphed in (True, False):
        eng = E.Pix2PixEngine(4, 4, "tanh", S, L.BF16, seed=12)
        eng.replay_enabled = False
        step = eng.graphed_rgba_step(B, 30.0) if graphed else (lambda s, r: eng.train_step_rgba(s, r, 30.0))
        losses = [step(torch.as_tensor(b[0]).cuda(), torch.as_tensor(b[1]).cuda()).clone() for b in batches]
        torch.cuda.synchronize()
        runs.append((torch.stack(losses).cpu(), eng))
    (la, a), (lb, b) = runs
    assert torch.equal(la, lb), (la - lb).abs().max()
    for sa, sb in ((a.G, b.G), (a.D, b.D)):
        assert sa.t == sb.t == len(batches) and int(sa.t_dev[0]) == int(sb.t_dev[0]) == len(batches)
        for buf in ("params", "m", "v"):
            assert torch.equal(getattr(sa, buf), getattr(sb, buf)), buf
    assert int(a.mask_counter_dev[0]) == int(b.mask_counter_dev[0])


def test_generate_is_forward_of_train_step():
    B, S = 2, 64
    rng, Gp, Dp, src, tgt, masks = setup_case(B, S, 23)
    eng = E.Pix2PixEngine(4, 4, "tanh", S, L.F32)
    eng.set_params(to_np(Gp), to_np(Dp))
    fake = eng.generate(src, masks=masks).cpu().numpy()
    ref = rg.unet_generator(Gp, torch.tensor(src, dtype=F64), [torch.tensor(m, dtype=F64) for m in masks], "tanh").numpy()
    assert np.abs(fake - ref).max() < 1e-4


def test_train_step_128x128_sprites_f32():
    """BASELINE.json config 5 geometry: IMG_SIZE = 128, the depth stays 6 so the bottleneck is 2x2 and down6 is live
    (north_star discrepancies).  Histogram model, B = 1."""
    B, S = 1, 128
    rng, Gp, Dp, src, tgt, masks = setup_case(B, S, 25)
    tm = [torch.tensor(m, dtype=F64) for m in masks]
    ref = rg.train_step_rgba(Gp, Dp, torch.tensor(src, dtype=F64), torch.tensor(tgt, dtype=F64), tm, lambda_l1=30.0, lambda_hist=1.0)
    eng = E.Pix2PixEngine(4, 4, "tanh", S, L.F32)
    eng.set_params(to_np(Gp), to_np(Dp))
    out = eng.train_step_rgba(src, tgt, 30.0, lambda_hist=1.0, masks=masks, apply_update=False).cpu().numpy()
    g, d = ref["g_loss"], ref["d_loss"]
    want = np.array([g[0], g[1], g[2], g[3], d[0], d[1], d[2]])
    for i in range(7):
        assert abs(out[i] - want[i]) <= 1e-4 * abs(want[i]), (i, out[i], want[i])
    wg = grad_report(eng.G.export(eng.G.grads), ref["g_grads"])
    wd = grad_report(eng.D.export(eng.D.grads), ref["d_grads"])
    print("worst G", wg, "worst D", wd)
    assert float(np.abs(ref["g_grads"]["down6.kernel"].numpy()).max()) > 0.0        # live at S = 128
    assert wg[1][1] < 2e-3 and wd[1][1] < 1e-4


def test_step_replay_follows_hyper_parameters_and_the_current_stream():
    """changing the learning rate or the dropout seed, or issuing the step under another torch
    stream, after a step has been recorded must give what the eager engine gives.  The hyper-parameters and the seed sit in slots
    the records point to (ONE recording serves a whole learning-rate schedule); the stream is part of the key (raw handles inside
    the records), so a step under another stream is recorded anew."""
    from palette_and_histo_gan_amd import dataset_utils as DU
    B, S = 4, 64
    batches = list(DU.synthetic_rgba_ds(32, batch_size=B, palette_size=24, seed=4))
    other = torch.cuda.Stream()
    runs = []
    for replay in (True, False):
        eng = E.Pix2PixEngine(4, 4, "tanh", S, L.BF16, seed=5)
        eng.replay_enabled = replay
        losses = []
        for t, b in enumerate(batches):
            if t == 4:
                eng.lr = 5e-4                       # picked up by p2p_adam_tick of this and the following steps
            if t == 5:
                eng.seed, eng.beta1 = 11, 0.6
            if t >= 6:                              # the last steps run under a side stream of the caller
                other.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(other):
                    losses.append(eng.train_step_rgba(b[0], b[1], 100.0))
                torch.cuda.current_stream().wait_stream(other)
            else:
                losses.append(eng.train_step_rgba(b[0], b[1], 100.0))
        torch.cuda.synchronize()
        if replay:
            assert len(eng._replays) == 2           # (default stream), (side stream): no new recording for lr / seed / beta
        runs.append((torch.stack([x.cpu() for x in losses]), eng))
    (la, a), (lb, b) = runs
    assert torch.equal(la, lb), (la - lb).abs().max()
    for sa, sb in ((a.G, b.G), (a.D, b.D)):
        for buf in ("params", "m", "v"):
            assert torch.equal(getattr(sa, buf), getattr(sb, buf)), buf
