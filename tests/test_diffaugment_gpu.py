"""-m gpu: the differentiable augmentation (csrc/diffaugment.hip behind diffaugment.diff_augment) and Pix2PixDiffAugmentModel.

Geometry (translation, cutout, identity) is held bit-exact to numpy index arithmetic, forward and backward.  The colour stage is
compared with the float64 restatement (tests/diffaugment_oracle.py); the YARDSTICK is that restatement evaluated in float32 on the
CPU for the test's own inputs, and the kernels get 8 x the yardstick's deviation (their sums are tree-shaped like torch's, in another
order).  Both figures are printed before the assertion (-s); DESIGN.md "differentiable augmentation" records them.

Every shape sees every row of ROWS (no shift, +-1, +-H/8, H - 1, >= H, int32 extremes; a box inside, over every border, outside;
s = 0, s = 1, k = 1, b = 0): the rows are dealt to the shape's batch in as many calls as it takes."""
import ctypes as C
import json
import types

import numpy as np
import pytest
import torch

from oracle import reference_graph as rg
from palette_and_histo_gan_amd import _lib as L
from palette_and_histo_gan_amd import dataset_utils as D
from palette_and_histo_gan_amd import diffaugment as A
from palette_and_histo_gan_amd import pix2pix_model as M
from tests import diffaugment_oracle as O
from tests import gpu_util as U
from tests import test_gradient_tape_gpu as T

pytestmark = pytest.mark.gpu
F64 = torch.float64
S = 64
ALL = "color,translation,cutout"
SHAPES = [(1, 8, 8, 4), (3, 16, 16, 4), (2, 8, 20, 4), (2, 64, 64, 4), (5, 128, 128, 4)]
FILL = -1.0


@pytest.fixture(autouse=True)
def _in_tmp(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)          # the models write their log and checkpoint folders under the working directory


def rows_for(H, W):
    """(color (R, 3), geometry (R, 4), ch, cw): the hand-built rows every shape is run with"""
    ch, cw = H // 2, W // 2
    big = 2 ** 31 - 1
    geometry = [
        (0, 0, H // 4, W // 4),                                   # no shift; box inside
        (1, -1, -(ch // 2), -(cw // 2)),                          # +-1; box over the top and the left border
        (-1, 1, H - ch + ch // 2, W - cw + cw // 2),              # -+1; box over the bottom and the right border
        (H // 8, -(W // 8), -(ch // 2), W // 4),                  # +-H/8; box over the top border only
        (-(H // 8), W // 8, H // 4, W - cw + 1),                  # -+H/8; box over the right border only
        (H - 1, 0, H - 1, -(cw - 1)),                             # H - 1: one row survives; box over bottom and left, one pixel deep
        (0, -(W - 1), H, 0),                                      # one column survives; box below the image: cuts nothing
        (H, 0, H // 4, W // 4),                                   # a shift of H: everything is fill
        (0, W + 3, -ch, -cw),                                     # a shift past W; box above and left of the image: cuts nothing
        (-big - 1, big, big, -big - 1),                           # int32 extremes: everything is fill, nothing overflows
    ]
    color = [(0.0, 1.0, 1.0), (0.3, 0.0, 1.2), (-0.4, 1.0, 0.6), (0.1, 1.7, 1.0), (0.0, 0.5, 1.4),
             (-0.2, 1.99, 0.5), (0.5, 0.25, 1.5), (0.2, 0.7, 0.8), (-0.5, 1.3, 1.1), (0.05, 0.0, 1.0)]
    return np.array(color, np.float32), np.array(geometry, np.int64).astype(np.int32), ch, cw


_cases = {}


def case(shape):
    """inputs of a shape, drawn once and shared (never modified): x, g, and the rows dealt into tables of B rows"""
    if shape not in _cases:
        B, H, W, _ = shape
        rng = np.random.default_rng(1000 + B * H + W)
        x = rng.uniform(-1, 1, size=shape).astype(np.float32)
        g = rng.normal(size=shape).astype(np.float32)
        color, geometry, ch, cw = rows_for(H, W)
        R = len(color)
        tables = [(color[np.arange(i, i + B) % R], geometry[np.arange(i, i + B) % R]) for i in range(0, R, B)]
        _cases[shape] = (x, g, tables, ch, cw)
    return _cases[shape]


def device_run(x, g, color, geometry, ch, cw, policy):
    """(out, dx) of one call through autograd, as numpy"""
    xt = torch.tensor(x, device=U.DEV, requires_grad=True)
    out = A.diff_augment(xt, A.AugmentParameters(color, geometry, ch, cw), policy, fill=FILL)
    out.backward(torch.tensor(g, device=U.DEV))
    return out.detach().cpu().numpy(), xt.grad.cpu().numpy()


# ---------------------------------------------------------------------------------------------------- 1. geometry, bit-exact
def np_box(H, W, y0, x0, ch, cw):
    r0, r1 = min(max(int(y0), 0), H), min(max(int(y0) + ch, 0), H)
    c0, c1 = min(max(int(x0), 0), W), min(max(int(x0) + cw, 0), W)
    return slice(r0, r1), slice(c0, c1)


def np_geometry(x, g, geometry, ch, cw, policy):
    """forward and VJP of the geometric stages by slicing"""
    on = O.stages(policy)
    B, H, W, _ = x.shape
    out, dx = np.empty_like(x), np.empty_like(x)
    for i in range(B):
        ty, tx, y0, x0 = (int(v) for v in geometry[i])
        if "translation" not in on:
            ty = tx = 0
        r0, r1, c0, c1 = min(max(ty, 0), H), min(max(H + ty, 0), H), min(max(tx, 0), W), min(max(W + tx, 0), W)      # output rows / columns with a source
        res, gi = np.full_like(x[i], FILL), g[i].copy()
        if r1 > r0 and c1 > c0:
            res[r0:r1, c0:c1] = x[i, r0 - ty:r1 - ty, c0 - tx:c1 - tx]
        if "cutout" in on:
            box = np_box(H, W, y0, x0, ch, cw)
            res[box] = FILL
            gi[box] = 0.0
        back = np.zeros_like(g[i])
        if r1 > r0 and c1 > c0:
            back[r0 - ty:r1 - ty, c0 - tx:c1 - tx] = gi[r0:r1, c0:c1]
        out[i], dx[i] = res, back
    return out, dx


@pytest.mark.parametrize("policy", ["", "translation", "cutout", "translation,cutout"])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_geometry_is_bit_exact(shape, policy):
    x, g, tables, ch, cw = case(shape)
    for color, geometry in tables:
        want, want_dx = np_geometry(x, g, geometry, ch, cw, policy)
        out, dx = device_run(x, g, color, geometry, ch, cw, policy)
        assert np.array_equal(out, want), (shape, policy, geometry.tolist())
        assert np.array_equal(dx, want_dx), (shape, policy, geometry.tolist())


# ---------------------------------------------------------------------------------------------------- 2. colour against float64
@pytest.mark.parametrize("policy", ["color", "color,translation", "color,cutout", ALL])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_colour_against_float64_with_the_float32_restatement_as_yardstick(shape, policy):
    x, g, tables, ch, cw = case(shape)
    got, ref64, ref32 = [], [], []
    for color, geometry in tables:
        got.append(device_run(x, g, color, geometry, ch, cw, policy))
        ref64.append(O.evaluate(x, g, color, geometry, ch, cw, policy, F64, FILL))
        ref32.append(O.evaluate(x, g, color, geometry, ch, cw, policy, torch.float32, FILL))
    for k, name in enumerate(("forward", "vjp")):
        r64 = np.concatenate([r[k] for r in ref64])
        top = np.abs(r64).max()
        yard = np.abs(np.concatenate([r[k] for r in ref32]) - r64).max() / top
        dev = np.abs(np.concatenate([r[k] for r in got]).astype(np.float64) - r64).max() / top
        print(f"diffaugment {shape} {policy} {name}: yardstick {yard:.3e} kernel {dev:.3e} ratio {dev / max(yard, 1e-300):.2f}")
        assert np.isfinite(dev) and dev <= 8 * yard, (name, dev, yard)
    # alpha passes through the colour stage untouched: against the geometric stages alone, bit for bit
    geo = ",".join(sorted(O.stages(policy) - {"color"}))
    for (color, geometry), (out, dx) in zip(tables, got):
        want, want_dx = np_geometry(x, g, geometry, ch, cw, geo)
        assert np.array_equal(out[..., 3], want[..., 3]) and np.array_equal(dx[..., 3], want_dx[..., 3])


# ---------------------------------------------------------------------------------------------------- 3. batch invariance
@pytest.mark.parametrize("size", [64, 128])
def test_an_image_gives_the_same_bits_alone_and_in_a_batch_and_twice(size):
    x, g, _, _, _ = case((5, 128, 128, 4))
    x, g = np.ascontiguousarray(x[:, :size, :size]), np.ascontiguousarray(g[:, :size, :size])
    color, geometry, ch, cw = rows_for(size, size)
    color, geometry = color[1:6], geometry[1:6]
    out, dx = device_run(x, g, color, geometry, ch, cw, ALL)
    out2, dx2 = device_run(x, g, color, geometry, ch, cw, ALL)
    assert np.array_equal(out, out2) and np.array_equal(dx, dx2)
    for i in range(5):
        o1, d1 = device_run(x[i:i + 1], g[i:i + 1], color[i:i + 1], geometry[i:i + 1], ch, cw, ALL)
        assert np.array_equal(o1[0], out[i]) and np.array_equal(d1[0], dx[i]), i
    # ... and wherever it sits in the batch
    perm = np.array([3, 0, 4, 2, 1])
    outp, dxp = device_run(x[perm], g[perm], color[perm], geometry[perm], ch, cw, ALL)
    assert np.array_equal(outp, out[perm]) and np.array_equal(dxp, dx[perm])


# ---------------------------------------------------------------------------------------------------- 4. through autograd
def test_autograd_runs_the_backward_entry_point():
    shape = (3, 16, 16, 4)
    x, g, tables, ch, cw = case(shape)
    B, H, W, _ = shape
    color, geometry = tables[0]          # rows 0..2: no image is wholly fill
    out, dx = device_run(x, g, color, geometry, ch, cw, ALL)
    gt, ct, qt = torch.tensor(g, device=U.DEV), torch.tensor(color, device=U.DEV), torch.tensor(geometry, device=U.DEV)
    raw = torch.full(shape, 7.0, device=U.DEV)
    ws = torch.empty(int(L.lib().p2p_diffaug_workspace_bytes(B, H, W)) // 4, device=U.DEV)
    L.call("p2p_diffaug_bwd", B, H, W, U.ptr(gt), U.ptr(ct), U.ptr(qt), ch, cw, 7, FILL, U.ptr(raw), U.ptr(ws), U.stream())
    assert np.array_equal(raw.cpu().numpy(), dx)
    # the alpha gradient is a pure gather of g; the colour gradient follows the closed form
    _, geo_dx = np_geometry(x, g, geometry, ch, cw, "translation,cutout")
    assert np.array_equal(dx[..., 3], geo_dx[..., 3])
    want = O.vjp_closed_form(torch.tensor(g, dtype=F64), color, geometry, ch, cw, ALL).numpy()
    assert np.abs(dx - want).max() <= 1e-5 * np.abs(want).max()
    # without the colour stage a source pixel whose destination is a fill (or off the image) has a zero gradient, every other pixel g
    out_g, dx_g = device_run(x, g, color, geometry, ch, cw, "translation,cutout")
    lost = geo_dx == 0
    assert lost.any() and not lost.all() and not dx_g[lost].any() and np.array_equal(dx_g, geo_dx)
    # the result is differentiable with respect to the images alone, and a chain through two augmentations works
    xt = torch.tensor(x, device=U.DEV, requires_grad=True)
    p = A.AugmentParameters(color, geometry, ch, cw)
    twice = A.diff_augment(A.diff_augment(xt, p, "color"), p, "translation,cutout")
    assert twice.requires_grad and twice.dtype == torch.float32 and tuple(twice.shape) == shape
    assert torch.equal(twice.detach().cpu(), torch.tensor(out))
    twice.backward(gt)          # (the colour stage alone adds the same gradients up at other positions, hence in another order)
    assert np.abs(xt.grad.cpu().numpy() - dx).max() <= 1e-6 * np.abs(dx).max()
    assert not A.diff_augment(torch.tensor(x, device=U.DEV), p).requires_grad
    ident = A.diff_augment(xt, p, "")
    assert torch.equal(ident, xt) and ident.requires_grad


def test_bad_arguments_of_the_entry_points_are_refused():
    x = torch.zeros((1, 8, 8, 4), device=U.DEV)
    out, ws = torch.empty_like(x), torch.empty(4, device=U.DEV)
    tab, geo = torch.zeros((1, 3), device=U.DEV), torch.zeros((1, 4), dtype=torch.int32, device=U.DEV)
    null = C.c_void_p(None)
    for args, what in (((1, 8, 8, U.ptr(x), U.ptr(tab), U.ptr(geo), 4, 4, 8, FILL, U.ptr(out), U.ptr(ws)), "policy_bits"),
                       ((1, 8, 8, U.ptr(x), U.ptr(tab), U.ptr(geo), 4, 4, 7, FILL, U.ptr(x), U.ptr(ws)), "one buffer"),
                       ((1, 8, 8, U.ptr(x), null, U.ptr(geo), 4, 4, 7, FILL, U.ptr(out), U.ptr(ws)), "color table"),
                       ((1, 8, 8, U.ptr(x), U.ptr(tab), U.ptr(geo), 4, 4, 1, FILL, U.ptr(out), null), "workspace"),
                       ((1, 8, 8, U.ptr(x), U.ptr(tab), null, 4, 4, 2, FILL, U.ptr(out), U.ptr(ws)), "geometry table"),
                       ((1, 8, 8, U.ptr(x), U.ptr(tab), U.ptr(geo), -1, 4, 4, FILL, U.ptr(out), U.ptr(ws)), "cutout box"),
                       ((0, 8, 8, U.ptr(x), U.ptr(tab), U.ptr(geo), 4, 4, 7, FILL, U.ptr(out), U.ptr(ws)), "bad shape")):
        for name in ("p2p_diffaug_fwd", "p2p_diffaug_bwd"):
            with pytest.raises(L.P2PError, match=what):
                L.call(name, *args, U.stream())
    assert L.lib().p2p_diffaug_workspace_bytes(256, 64, 64) == 256 * 4 * 4 and L.lib().p2p_diffaug_workspace_bytes(5, 8, 20) == 5 * 4
    # the tables are optional where no stage reads them
    L.call("p2p_diffaug_fwd", 1, 8, 8, U.ptr(x), null, null, 0, 0, 0, FILL, U.ptr(out), null, U.stream())
    assert torch.equal(out, x)


# ---------------------------------------------------------------------------------------------------- 5.-7. the model
def _augmented(Gp, Dp, policy, **kw):
    return T._model(Gp, Dp, cls=M.Pix2PixDiffAugmentModel, policy=policy, **kw)


def test_the_empty_policy_step_equals_the_fused_step():
    B = 2
    rng, Gp, Dp = T._params(81)
    src, tgt = rg.synthetic_rgba_batch(rng, B, S, palette_size=24)
    masks = T._masks(rng, B)
    fused = T._engine(Gp, Dp)
    out = fused.train_step_rgba(src, tgt, 100.0, masks=masks, apply_update=False).cpu().numpy()
    m = _augmented(Gp, Dp, "")
    g_loss, d_loss, gg, dg = m.augmented_step(src, tgt, 0, masks=masks, apply=False)
    got = T._losses(g_loss, d_loss)
    for i in (0, 1, 2, 4, 5, 6):
        assert abs(got[i] - out[i]) <= 1e-6 * abs(out[i]), (i, got[i], out[i])
    T._close(T._as_dict(m.engine.G, gg), fused.G.export(fused.G.grads), 1e-5)
    T._close(T._as_dict(m.engine.D, dg), fused.D.export(fused.D.grads), 1e-5)
    assert m.generator_optimizer.iterations == 0          # apply=False


ORACLE_SEED = 90
ORACLE_STEP = 0


def oracle_graph_step(Gp, Dp, src, tgt, masks, p, policy, dtype):
    """the augmented step as a graph of oracle.reference_graph networks and tests/diffaugment_oracle.py, evaluated in `dtype`:
    (losses g_total, adv, l1, d_total, d_real, d_fake as floats, generator gradients, discriminator gradients)"""
    Gl = {k: v.to(dtype).clone().requires_grad_(True) for k, v in Gp.items()}
    Dl = {k: v.to(dtype).clone().requires_grad_(True) for k, v in Dp.items()}
    s, t = torch.tensor(src, dtype=dtype), torch.tensor(tgt, dtype=dtype)
    fake = rg.unet_generator(Gl, s, [torch.tensor(x, dtype=dtype) for x in masks], "tanh")
    aug = lambda x: O.diff_augment(x, p.color.numpy(), p.geometry.numpy(), p.ch, p.cw, policy, FILL)      # noqa: E731
    source_aug = aug(s)
    real_pred = rg.patch_discriminator(Dl, aug(t), source_aug)
    fake_pred = rg.patch_discriminator(Dl, aug(fake), source_aug)
    adv, l1 = rg.bce_from_logits(fake_pred, 1), (t - fake).abs().mean()
    g_total = adv + 100.0 * l1
    d_real, d_fake = rg.bce_from_logits(real_pred, 1), rg.bce_from_logits(fake_pred, 0)
    d_total = d_fake + d_real
    g_ref = torch.autograd.grad(g_total, list(Gl.values()), retain_graph=True)
    d_ref = torch.autograd.grad(d_total, list(Dl.values()))
    losses = [float(v.detach()) for v in (g_total, adv, l1, d_total, d_real, d_fake)]
    return losses, {k: g.numpy() for k, g in zip(Gl, g_ref)}, {k: g.numpy() for k, g in zip(Dl, d_ref)}


def oracle_case(seed=ORACLE_SEED):
    rng, Gp, Dp = T._params(seed)
    src, tgt = rg.synthetic_rgba_batch(rng, 2, S, palette_size=24)
    return Gp, Dp, src, tgt, T._masks(rng, 2)


def test_the_full_policy_step_against_the_oracle_graph():
    """Weights, batch and masks are drawn at seed 90 as tests/test_gradient_tape_gpu.py::test_cycle_step_against_the_oracle_graph
    draws them, and the parameter table is the model's own for (model seed 5, step 0).  The seed was picked on the CPU: there the
    oracle graph of THIS step evaluated in float32 agrees with its float64 evaluation to 1e-5 on all six losses (measured: 8.4e-8 at
    most, and 5.4e-5 / 1.4e-6 of max-norm on the generator's / discriminator's gradients), i.e. no activation of the generator's
    1x1 .. 4x4 layers sits within f32 rounding of its kink, where the two precisions take different branches and move a whole
    image's gradient whatever the kernels do (seed 92: losses to 6e-8, yet the f32 generator gradient is 3 % off)."""
    Gp, Dp, src, tgt, masks = oracle_case()
    m = _augmented(Gp, Dp, ALL)
    g_loss, d_loss, gg, dg = m.augmented_step(src, tgt, ORACLE_STEP, masks=masks, apply=False)
    got = [float(v) for v in g_loss + d_loss]
    got_g, got_d = T._as_dict(m.engine.G, gg), T._as_dict(m.engine.D, dg)
    p = A.draw_parameters(2, S, S, ALL, seed=m._seed, step=ORACLE_STEP)
    want, g_ref, d_ref = oracle_graph_step(Gp, Dp, src, tgt, masks, p, ALL, F64)
    print("augmented step", got, "oracle", want, "table", p.color.tolist(), p.geometry.tolist())
    for a, b in zip(got, want):
        assert abs(a - b) <= 1e-5 * abs(b), (got, want)
    T._close(got_g, g_ref, 1e-4)
    T._close(got_d, d_ref, 1e-4)
    # an augmentation that silently does nothing would pass a weaker test: the generator's gradient is not the empty policy's
    m0 = _augmented(Gp, Dp, "")
    _, _, gg0, _ = m0.augmented_step(src, tgt, ORACLE_STEP, masks=masks, apply=False)
    plain = T._as_dict(m0.engine.G, gg0)
    moved = {k: np.abs(got_g[k] - plain[k]).max() / (np.abs(g_ref[k]).max() + 1e-30) for k in g_ref}
    print("generator gradient, full policy vs empty policy (of max-norm):", sorted(moved.items(), key=lambda kv: kv[1])[-3:])
    assert max(moved.values()) > 1e-4          # the tolerance of the comparison above


def _fit_model(name, train, **kw):
    return M.Pix2PixDiffAugmentModel(train, train, "front2right", name, lambda_l1=100.0, seed=5, **kw)


def test_fit_runs_logs_and_resumes_bit_exactly():
    train = D.synthetic_rgba_ds(6, batch_size=2, palette_size=24)          # three batches: a resume at step 3 starts an epoch
    whole = _fit_model("diffaug-fit-whole", train)
    w0 = whole.engine.G.params.clone()
    whole.fit(6, 3)
    assert whole.generator_optimizer.iterations == 6 and whole.discriminator_optimizer.iterations == 6
    assert not torch.equal(whole.engine.G.params, w0)
    rows = [json.loads(r) for r in open(whole.summary_writer.path)]
    for tag in ("generator/total_loss", "generator/adversarial_loss", "generator/l1_loss", "discriminator/total_loss",
                "discriminator/real_loss", "discriminator/fake_loss"):
        vals = [r["value"] for r in rows if r.get("name") == tag]
        assert len(vals) == 6 and np.isfinite(vals).all(), (tag, vals)
    # three steps, a checkpoint, and three more in a fresh model: the table of step 3 is drawn from (seed, 3) again
    first = _fit_model("diffaug-fit-first", train)
    first.fit(3, 3)
    resumed = _fit_model("diffaug-fit-resumed", train)
    resumed.checkpoint.restore(first.checkpoint_manager.latest_checkpoint)
    resumed.fit(3, 3, starting_step=3)
    assert resumed.generator_optimizer.iterations == 6
    assert torch.equal(resumed.engine.G.params, whole.engine.G.params) and torch.equal(resumed.engine.D.params, whole.engine.D.params)
    assert torch.equal(resumed.engine.G.m, whole.engine.G.m) and torch.equal(resumed.engine.D.v, whole.engine.D.v)


def test_a_data_parallel_model_refuses_the_tape_step():
    dp = types.SimpleNamespace(rank=0, world=1)
    m = M.Pix2PixDiffAugmentModel(D.synthetic_rgba_ds(4, batch_size=2), None, "front2right", "diffaug-dp-test", lambda_l1=100.0,
                                  data_parallel=dp)
    src, tgt = rg.synthetic_rgba_batch(np.random.default_rng(0), 2, S)
    with pytest.raises(NotImplementedError, match="one GPU"):
        m.train_step((src, tgt), 0, 1)
    with pytest.raises(ValueError, match="unknown augmentation"):
        M.Pix2PixDiffAugmentModel(D.synthetic_rgba_ds(4, batch_size=2), None, "front2right", "diffaug-dp-test", lambda_l1=100.0, policy="flip")
