"""-m gpu: the palette lookup (p2p_palette_lookup_fwd / _bwd in csrc/palette_lookup.hip behind palette.palette_lookup) and
Pix2PixIndexedColourModel.

The kernels are called through the C ABI on NaN-filled outputs between guard elements, every launch twice with identical bits.
The soft forward is compared with the float64 restatement (tests/palette_lookup_oracle.py); the YARDSTICK is the same sum in
float32, slots added one by one in ascending k, and the kernel gets 8 x the yardstick's deviation -- the project's margin for its
palette kernels -- with a floor of one f32 ulp of the max-norm.  Both figures are printed before the assertion (-s); DESIGN.md 6g
records them.  The hard forward and the backward are exact restatements and held to equality."""
import ctypes as C
import functools
import json
import types

import numpy as np
import pytest
import torch

from oracle import reference_graph as rg
from palette_and_histo_gan_amd import _lib as L
from palette_and_histo_gan_amd import dataset_utils as D
from palette_and_histo_gan_amd import histogram as HG
from palette_and_histo_gan_amd import palette as P
from palette_and_histo_gan_amd import pix2pix_model as M
from tests import gpu_util as U
from tests import palette_lookup_oracle as O
from tests import test_indexed_hooks_gpu as IH

pytestmark = pytest.mark.gpu
F64 = torch.float64
S, K = 64, 256
GUARD = 64                      # elements in front of and behind the output
ULP = 2.0 ** -23


@pytest.fixture(autouse=True)
def _in_tmp(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)          # the models write their log and checkpoint folders under the working directory


def _guarded(shape):
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), float("nan"), device=U.DEV)
    return buf, buf[GUARD:GUARD + n].view(shape)


def _twice(launch, shape):
    """`launch(out)` into two NaN-filled outputs between NaN guards: the guards intact, the two results bit-identical; numpy"""
    outs = []
    for _ in range(2):
        buf, out = _guarded(shape)
        launch(out)
        torch.cuda.synchronize()
        assert bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[-GUARD:]).all())
        outs.append(out.cpu().numpy())
    assert outs[0].tobytes() == outs[1].tobytes()
    return outs[0]


def _dev(x, dt=torch.float32):
    return U.dev(np.array(x), dt)          # a copy: the oracle's cases are read-only


def _forward(probs, pal, hard, blacken):
    N, H, W, _ = probs.shape
    p, q = _dev(probs), _dev(pal, torch.int32)
    return _twice(lambda out: L.call("p2p_palette_lookup_fwd", N, H, W, K, U.ptr(p), U.ptr(q), int(hard), int(blacken), U.ptr(out),
                                     U.stream()), (N, H, W, 4))


def _backward(g, pal, blacken):
    N, H, W, _ = g.shape
    u, q = _dev(g), _dev(pal, torch.int32)
    return _twice(lambda out: L.call("p2p_palette_lookup_bwd", N, H, W, K, U.ptr(u), U.ptr(q), int(blacken), U.ptr(out), U.stream()),
                  (N, H, W, K))


# ---------------------------------------------------------------------------------------------------- 1. soft forward
@pytest.mark.parametrize("s", O.SPREADS)
@pytest.mark.parametrize("name", list(O.CASES))
def test_soft_forward_against_float64_with_the_sequential_float32_sum_as_yardstick(name, s):
    probs, pal, _, _ = O.case(name, s)
    for blacken in (False, True):
        y64, yard = O.reference(name, s, blacken)
        y = _forward(probs, pal, False, blacken)
        dev = float(np.abs(y.astype(np.float64) - y64).max())
        floor = ULP * float(np.abs(y64).max())
        print(f"lookup {name} s {s} blacken {int(blacken)}: yardstick {yard:.2e} | kernel {dev:.2e} | ratio {dev / max(yard, 1e-30):.2f} | "
              f"floor {floor:.2e}")
        assert np.isfinite(y).all()          # no sentinel survives: every pixel written
        assert dev <= max(8 * yard, floor), (name, s, blacken, dev, yard)
        # an exact one-hot row returns the bits of its slot's colour
        one_hot = (probs == 1.0).any(-1)
        if one_hot.any():
            want, _ = O.hard_lookup(probs, pal, blacken)
            assert y[one_hot].tobytes() == want[one_hot].tobytes()


# ---------------------------------------------------------------------------------------------------- 2. hard forward
@pytest.mark.parametrize("name", list(O.CASES))
def test_hard_forward_equals_the_gather_bit_for_bit(name):
    probs, pal, sizes = O.hard_case(name)
    for blacken in (False, True):
        want, idx = O.hard_lookup(probs, pal, blacken)
        assert ((probs == probs.max(-1, keepdims=True)).sum(-1) > 1).any() and (idx >= sizes[:, None, None]).any()
        assert _forward(probs, pal, True, blacken).tobytes() == want.tobytes()
    # the soft cases as well: ordinary rows and exact one-hot rows
    probs, pal, _, _ = O.case(name, 12)
    assert _forward(probs, pal, True, True).tobytes() == O.hard_lookup(probs, pal, True)[0].tobytes()


# ---------------------------------------------------------------------------------------------------- 3. backward
@pytest.mark.parametrize("blacken", [False, True])
@pytest.mark.parametrize("name", list(O.CASES))
def test_backward_equals_the_float32_restatement_bit_for_bit(name, blacken):
    _, pal, g, _ = O.case(name, 4)
    got = _backward(g, pal, blacken)
    assert got.tobytes() == O.vjp32(g, pal, blacken).tobytes()          # every element: no sentinel survives


# ---------------------------------------------------------------------------------------------------- 4. batch invariance
def test_an_image_gives_the_same_bits_alone_and_inside_its_batch():
    probs, pal, g, _ = O.case("3x7x33", 4)
    hprobs, hpal, _ = O.hard_case("3x7x33")
    one = slice(1, 2)
    for blacken in (False, True):
        assert _forward(probs[one], pal[one], False, blacken).tobytes() == _forward(probs, pal, False, blacken)[one].tobytes()
        assert _forward(hprobs[one], hpal[one], True, blacken).tobytes() == _forward(hprobs, hpal, True, blacken)[one].tobytes()
        assert _backward(g[one], pal[one], blacken).tobytes() == _backward(g, pal, blacken)[one].tobytes()
    # ... and with another image's palette it does not: the palettes of the batch differ
    assert _forward(probs[one], pal[:1], False, True).tobytes() != _forward(probs[one], pal[one], False, True).tobytes()


# ---------------------------------------------------------------------------------------------------- 5. argument errors
def test_bad_arguments_are_refused_with_a_negative_code_and_a_message():
    probs, pal, g, _ = O.case("2x3x5", 4)
    N, H, W, _ = probs.shape
    p, q, u = _dev(probs), _dev(pal, torch.int32), _dev(g)
    out = torch.full((N, H, W, 4), float("nan"), device=U.DEV)
    dp = torch.full((N, H, W, K), float("nan"), device=U.DEV)
    null = C.c_void_p(0)
    fwd = [N, H, W, K, U.ptr(p), U.ptr(q), 0, 0, U.ptr(out), U.stream()]
    bwd = [N, H, W, K, U.ptr(u), U.ptr(q), 0, U.ptr(dp), U.stream()]
    for fn, good, bad in (("p2p_palette_lookup_fwd", fwd, [(3, 128, "K = 128"), (4, null, "null"), (5, null, "null"), (8, null, "null"),
                                                           (6, 2, "hard = 2"), (7, 2, "blacken = 2")]),
                          ("p2p_palette_lookup_bwd", bwd, [(3, 128, "K = 128"), (4, null, "null"), (5, null, "null"), (7, null, "null"),
                                                           (6, 2, "blacken = 2")])):
        for at, value, word in bad:
            args = list(good)
            args[at] = value
            assert getattr(L.lib(), fn)(*args) < 0, (fn, at)
            msg = L.lib().p2p_last_error().decode()
            assert fn in msg and word in msg, (fn, at, msg)
    with pytest.raises(L.P2PError, match="256"):
        L.call("p2p_palette_lookup_fwd", N, H, W, 128, U.ptr(p), U.ptr(q), 0, 0, U.ptr(out), U.stream())
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(dp).all())          # nothing ran
    assert getattr(L.lib(), "p2p_palette_lookup_fwd")(*fwd) == 0 and getattr(L.lib(), "p2p_palette_lookup_bwd")(*bwd) == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(dp).all())


# ---------------------------------------------------------------------------------------------------- 6. through autograd
def test_autograd_launches_forward_then_backward_and_feeds_the_histogram_loss(monkeypatch):
    probs, pal, g, _ = O.case("2x64x64", 4)
    called = []
    real_call = L.call
    monkeypatch.setattr(L, "call", lambda name, *a: (called.append(name), real_call(name, *a))[1])
    for hard in (False, True):
        del called[:]
        x = torch.tensor(probs, device=U.DEV, requires_grad=True)
        y = P.palette_lookup(x, pal, hard=hard, blacken=True)
        assert y.requires_grad and y.dtype == torch.float32 and tuple(y.shape) == (2, S, S, 4)
        y.backward(torch.tensor(g, device=U.DEV))
        assert called == ["p2p_palette_lookup_fwd", "p2p_palette_lookup_bwd"]
        want = O.hard_lookup(probs, pal, True)[0] if hard else None
        if hard:
            assert y.detach().cpu().numpy().tobytes() == want.tobytes()
        assert x.grad.cpu().numpy().tobytes() == O.vjp32(g, pal, True).tobytes()          # one VJP for both forwards
    monkeypatch.setattr(L, "call", real_call)
    # without a gradient nothing is saved and the result is detached; numpy inputs and other dtypes are converted
    y0 = P.palette_lookup(probs, pal)
    assert not y0.requires_grad and y0.cpu().numpy().tobytes() == _forward(probs, pal, False, False).tobytes()
    xb = torch.tensor(probs, device=U.DEV, dtype=torch.float64, requires_grad=True)
    P.palette_lookup(xb, torch.tensor(pal, dtype=torch.int64)).sum().backward()
    assert xb.grad.dtype == torch.float64 and xb.grad.shape == xb.shape and bool(torch.isfinite(xb.grad).all())
    # through a preceding torch op to a leaf, into the RGB-uv histogram and its Hellinger loss
    z = torch.tensor(np.log(np.maximum(probs, 1e-30)), device=U.DEV, requires_grad=True)
    fake = P.palette_lookup(torch.softmax(z, -1), pal, blacken=True)
    with torch.no_grad():
        real = P.palette_lookup(torch.roll(torch.tensor(probs, device=U.DEV), 1, dims=2), pal, hard=True, blacken=True)
    loss = HG.hellinger_loss(HG.calculate_rgbuv_histogram(real), HG.calculate_rgbuv_histogram(fake))
    loss.backward()
    print("hellinger loss through the lookup", float(loss.detach()), "max |dL/dlogits|", float(z.grad.abs().max()))
    assert bool(torch.isfinite(loss)) and float(loss.detach()) > 0 and bool(torch.isfinite(z.grad).all()) and bool(z.grad.any())


# ---------------------------------------------------------------------------------------------------- 7. the model
B, LAM, LAM_COLOUR, LAM_HIST = 2, 0.5, 2.0, 0.7


class HookedIndexed(M.Pix2PixIndexedModel):
    """the parent's own losses through the plain hooked step"""
    differentiable_loss_hooks = True

    def generator_loss(self, fake_predicted, fake_image, real_image):
        return super().generator_loss(fake_predicted, fake_image, real_image)


def _one_step(cls, Gp, Dp, batch, masks, **kw):
    """one train_step of a fresh f32 model at the given weights with injected dropout masks and no update; what it left behind"""
    ds = D.synthetic_indexed_ds(B, batch_size=B)
    m = cls(ds, None, "front2right", "indexed-colour-test", lambda_segmentation=LAM, dtype="f32", seed=5, **kw)
    eng = m.engine
    eng.set_params({k: v.numpy() for k, v in Gp.items()}, {k: v.numpy() for k, v in Dp.items()})
    hooked = eng.train_step_indexed_hooked
    eng.train_step_indexed_hooked = lambda src, tgt, gl, dl: hooked(src, tgt, gl, dl, masks=masks, apply_update=False)
    calls, seen = [], {}
    real_call = L.call

    def spy(name, *a):
        calls.append(name)
        real_call(name, *a)
        if name == "p2p_softmax_bwd":          # the head's pre-activation gradient, before the backward pass can touch it
            torch.cuda.synchronize()
            seen["dz"] = U.halo_to_np(eng.plan(B)["dz"])[..., :K].copy()
    L.call = spy
    try:
        g_loss, d_loss = m.train_step(batch, 0, 1)
    finally:
        L.call = real_call
    torch.cuda.synchronize()
    assert m._custom_hooks and eng.G.t == 0
    plan = eng.plan(B)
    return types.SimpleNamespace(g_loss=[float(v) for v in g_loss], d_loss=[float(v) for v in d_loss], calls=calls, dz=seen["dz"],
                                 g_grads=eng.G.grads.clone(), d_grads=eng.D.grads.clone(), probs=plan["hook_idx"][0].cpu().numpy().copy(),
                                 logits=plan["hook_idx"][1].cpu().numpy().copy(), model=m)


@functools.lru_cache(maxsize=None)
def _runs():
    rng, Gp, Dp = IH._params(71)
    src, tgt, pal = rg.synthetic_indexed_batch(rng, B, S)
    pal[:, 3] = (17, 140, 201, 0)          # a transparent slot with colour: `blacken` (the model's default) is not a no-op
    masks = [rng.integers(0, 2, size=s).astype(np.uint8) for s in rg.dropout_mask_shapes(B, S)]
    batch = (src, tgt, pal)
    step = functools.partial(_one_step, Gp=Gp, Dp=Dp, batch=batch, masks=masks)
    return types.SimpleNamespace(
        batch=batch, plain=step(HookedIndexed), colour=step(M.Pix2PixIndexedColourModel, lambda_colour=LAM_COLOUR),
        zero=step(M.Pix2PixIndexedColourModel, lambda_colour=0.0, lambda_histogram=0.0),
        hist=step(M.Pix2PixIndexedColourModel, lambda_colour=LAM_COLOUR, lambda_histogram=LAM_HIST, hard=True))


def test_the_colour_step_leaves_the_discriminator_alone_and_moves_the_generator():
    """`train_step` returns (total, adversarial, l1, segmentation, colour_l1, histogram): the adversarial, L1 and segmentation terms
    and the discriminator's three losses and gradients are those of the plain hooked step, bit for bit; the total is the plain total
    plus lambda_colour * colour_l1 (it cannot be the plain total: the term is part of it by definition)."""
    r = _runs()
    plain, colour = r.plain, r.colour
    print("plain", plain.g_loss, plain.d_loss, "colour", colour.g_loss, colour.d_loss)
    assert len(plain.g_loss) == 4 and len(colour.g_loss) == 6 and len(colour.d_loss) == 3
    assert colour.g_loss[1:4] == plain.g_loss[1:4] and colour.d_loss == plain.d_loss
    assert colour.g_loss[4] > 0 and colour.g_loss[5] == 0.0
    assert colour.g_loss[0] == float(np.float32(plain.g_loss[0]) + np.float32(LAM_COLOUR) * np.float32(colour.g_loss[4]))
    assert torch.equal(colour.d_grads, plain.d_grads) and bool(plain.d_grads.any())
    assert not torch.equal(colour.g_grads, plain.g_grads)
    moved = float((colour.g_grads - plain.g_grads).abs().max() / plain.g_grads.abs().max())
    print("generator gradient, colour vs plain step (of max-norm):", moved)
    assert moved > 1e-4
    lookups = [c for c in colour.calls if c.startswith("p2p_palette_lookup")]
    assert lookups == ["p2p_palette_lookup_fwd", "p2p_palette_lookup_fwd", "p2p_palette_lookup_bwd"]
    assert not any("hist" in c for c in colour.calls)          # lambda_histogram == 0: the histogram term is not launched
    assert not any(c.startswith("p2p_palette_lookup") for c in plain.calls)


def test_with_both_lambdas_at_zero_the_step_is_the_hooked_parents_bit_for_bit():
    r = _runs()
    assert r.zero.g_loss[:4] == r.plain.g_loss and r.zero.d_loss == r.plain.d_loss
    assert r.zero.g_loss[4] == r.colour.g_loss[4] and r.zero.g_loss[5] == 0.0          # reported, not weighted
    assert torch.equal(r.zero.g_grads, r.plain.g_grads) and torch.equal(r.zero.d_grads, r.plain.d_grads)
    assert np.array_equal(r.zero.dz, r.plain.dz) and np.array_equal(r.zero.probs, r.plain.probs)


def test_the_histogram_term_is_launched_only_when_weighted_and_reaches_the_generator():
    r = _runs()
    hist, colour = r.hist, r.colour
    print("hist", hist.g_loss)
    assert any("rgbuv" in c for c in hist.calls) and any("hellinger" in c or "rgbuv_hist" in c for c in hist.calls)
    assert hist.g_loss[5] > 0 and np.isfinite(hist.g_loss).all() and hist.g_loss[1:4] == colour.g_loss[1:4] and hist.d_loss == colour.d_loss
    assert torch.equal(hist.d_grads, colour.d_grads) and not torch.equal(hist.g_grads, colour.g_grads)
    assert bool(torch.isfinite(hist.g_grads).all())
    # hard=True: the fake image is the palette gather of the argmax
    src, tgt, pal = r.batch
    want, _ = O.hard_lookup(hist.probs, pal, True)
    real, _ = O.hard_lookup(np.eye(K, dtype=np.float32)[tgt[..., 0]], pal, True)
    l1 = float(np.abs(real.astype(np.float64) - want).mean())
    assert abs(hist.g_loss[4] - l1) <= 1e-5 * l1


def test_the_heads_gradient_is_cce_plus_softmax_vjp_plus_lookup_vjp_in_float64():
    """on the device's own probabilities and logits: dz = d(lambda_seg CCE)/dz + p (gp - <p, gp>), gp the lookup VJP of the colour
    term's image gradient; tolerance of tests/test_indexed_hooks_gpu.py for p2p_softmax_bwd in f32 (1e-6 of the pixel's max-norm)"""
    r = _runs()
    src, tgt, pal = r.batch
    p = torch.tensor(r.colour.probs, dtype=F64, requires_grad=True)
    z = torch.tensor(r.colour.logits, dtype=F64, requires_grad=True)
    onehot = torch.nn.functional.one_hot(torch.tensor(tgt[..., 0]).long(), K).to(F64)
    t = torch.tensor(O.colours(pal, True, np.float64))
    fake, real = torch.einsum("nhwk,nkc->nhwc", p, t), torch.einsum("nhwk,nkc->nhwc", onehot, t)
    margin = float((real - fake).abs().min())
    seg = -(onehot * torch.log_softmax(z, dim=-1)).sum(-1).mean()
    colour = (real - fake).abs().mean()
    (0.0 * (onehot - p).abs().mean() + LAM * seg + LAM_COLOUR * colour).backward()
    ref = (z.grad + p.detach() * (p.grad - (p.detach() * p.grad).sum(-1, keepdim=True))).numpy()
    assert abs(r.colour.g_loss[3] - float(seg)) <= 1e-5 * float(seg) and abs(r.colour.g_loss[4] - float(colour)) <= 1e-5 * float(colour)
    pix_max = np.abs(ref).max(-1, keepdims=True)
    err = np.abs(r.colour.dz.astype(np.float64) - ref)
    plain_err = np.abs(r.plain.dz.astype(np.float64) - ref)
    print(f"head gradient vs f64: worst error {float((err / pix_max).max()):.2e} of the pixel's max-norm (bound 1e-6); the plain step's head "
          f"gradient is {float((plain_err / pix_max).max()):.2e} away; min |real - fake| {margin:.2e}")
    assert margin > 1e-5          # no |.| of the colour term sits at its kink within f32 rounding
    assert float((err - 1e-6 * pix_max).max()) <= 0.0
    assert float((plain_err / pix_max).max()) > 1e-3          # the colour term is a visible part of it


# ---------------------------------------------------------------------------------------------------- 8. fit() and refusals
def test_a_four_step_fit_logs_the_two_new_terms():
    train = D.synthetic_indexed_ds(8, batch_size=4)
    m = M.Pix2PixIndexedColourModel(train, train, "front2right", "indexed-colour-fit", lambda_histogram=0.5)
    assert (m.lambda_segmentation, m.lambda_colour, m.hard, m.blacken) == (0.5, 100.0, False, True)
    w0 = m.engine.G.params.clone()
    m.fit(4, 2)
    assert m._custom_hooks and m.engine.G.t == 4 and not torch.equal(m.engine.G.params, w0)
    rows = [json.loads(r) for r in open(m.summary_writer.path)]
    for tag in ("generator/total_loss", "generator/segmentation_loss", "generator/colour_l1_loss", "generator/histogram_loss",
                "discriminator/total_loss"):
        vals = [r["value"] for r in rows if r.get("name") == tag]
        assert len(vals) == 4 and np.isfinite(vals).all() and min(vals) > 0, (tag, vals)


def test_data_parallel_and_a_missing_palette_are_refused():
    ids = D.synthetic_indexed_ds(4, batch_size=4)
    dp = types.SimpleNamespace(rank=0, world=1)
    m = M.Pix2PixIndexedColourModel(ids, ids, "front2right", "indexed-colour-dp", data_parallel=dp)
    with pytest.raises(NotImplementedError, match="one GPU"):
        m.train_step(next(iter(ids)), 0, 1)
    m = M.Pix2PixIndexedColourModel(ids, ids, "front2right", "indexed-colour-standalone")
    with pytest.raises(ValueError, match="palette"):
        m.generator_loss(torch.zeros(1, 32, 32, 1), torch.zeros(1, S, S, K), torch.zeros(1, S, S, K))
