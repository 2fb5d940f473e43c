"""-m gpu: the standalone RGB-uv histogram is differentiable (histogram.py:36-47 of the reference: "in a differentiable way").
histogram.calculate_rgbuv_histogram and Pix2PixEngine.rgbuv_histogram go through one torch.autograd.Function whose backward is
HIP (p2p_hist_normalize_bwd, then p2p_rgbuv_hist_bwd or p2p_rgbuv_hist_general_bwd); its VJP is checked against the float64
oracle under autograd, against the fused Hellinger gradient, and through the hooked train step of the histogram model."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest
import torch

from oracle import reference_graph as rg
from palette_and_histo_gan_amd import _lib as L
from palette_and_histo_gan_amd import dataset_utils as D
from palette_and_histo_gan_amd import engine as E
from palette_and_histo_gan_amd import histogram as H
from palette_and_histo_gan_amd import pix2pix_model as M
from tests import gpu_util as U

pytestmark = pytest.mark.gpu
F64 = torch.float64
GENERAL = ((64, "RBF", 0.02), (32, "inverse-quadratic", 0.05), (48, "RBF", 0.1), (16, "thresholding", 0.02),
           (128, "inverse-quadratic", 0.02), (64, "inverse-quadratic", 0.03))


def sprites(seed, B, S=64):
    rng = np.random.default_rng(seed)
    _, tgt = rg.synthetic_rgba_batch(rng, B, max(S, 64), palette_size=24)
    return tgt[:, :S, :S].copy()


def mid_range(seed, B, H_, W_, ch=4):
    """every channel in [-0.8, 0.8]: no near-black pixel, so no 1/(x + 1e-6)-steep gradient"""
    return np.random.default_rng(seed).uniform(-0.8, 0.8, size=(B, H_, W_, ch)).astype(np.float32)


def vjp(fn, img, g):
    """d <g, fn(img)> / d img of the HIP op on a f32 device leaf"""
    x = torch.tensor(img, device=U.DEV, requires_grad=True)
    out = fn(x)
    assert out.requires_grad
    (out * torch.as_tensor(g, device=U.DEV)).sum().backward()
    return x.grad.cpu().numpy()


def oracle_vjp(img, g, **kw):
    x = torch.tensor(img, dtype=F64, requires_grad=True)
    (rg.rgbuv_histogram(x, **kw) * torch.as_tensor(g, dtype=F64)).sum().backward()
    return x.grad.numpy()


def assert_close(got, ref, bound, what):
    l2 = np.linalg.norm(got - ref) / np.linalg.norm(ref)
    assert U.rel_err(got, ref) < bound and l2 < bound, (what, U.rel_err(got, ref), l2)


def upstream(seed, B, size):
    return np.random.default_rng(seed).normal(size=(B, size, size, 3)).astype(np.float32)


def test_vjp_at_the_reference_arguments_matches_the_f64_oracle():
    """<g, hist(x)> differentiated by autograd over the HIP op against the same expression over the oracle in float64: 2e-3 on
    sprites (the existing yardstick: near-black pixels put 1/(x + 1e-6) into the gradient), 1e-4 on mid-range images"""
    eng = E.Pix2PixEngine(4, 4, "tanh", 64, L.F32)
    for img, bound in ((sprites(41, 3), 2e-3), (mid_range(42, 2, 64, 64), 1e-4)):
        B = img.shape[0]
        g = upstream(43, B, 64)
        ref = oracle_vjp(img, g)
        for name, fn in (("calculate_rgbuv_histogram", H.calculate_rgbuv_histogram), ("engine.rgbuv_histogram", eng.rgbuv_histogram)):
            got = vjp(fn, img, g)
            assert got.shape == img.shape and np.count_nonzero(got[..., 3]) == 0
            assert_close(got, ref, bound, (name, bound))


@pytest.mark.parametrize("size,method,sigma", GENERAL)
def test_vjp_at_general_arguments_matches_the_f64_oracle(size, method, sigma):
    """the general backward (p2p_rgbuv_hist_general_bwd) for the six argument sets the forward is tested with"""
    for img, bound in ((sprites(44, 2), 2e-3), (mid_range(45, 2, 64, 64), 1e-4)):
        g = upstream(46, img.shape[0], size)
        got = vjp(lambda x: H.calculate_rgbuv_histogram(x, size=size, method=method, sigma=sigma), img, g)
        ref = oracle_vjp(img, g, size=size, sigma=sigma, method=method)
        assert np.count_nonzero(got[..., 3]) == 0
        assert_close(got, ref, bound, (size, method, sigma, bound))


@pytest.mark.parametrize("size,method,sigma", [(64, "inverse-quadratic", 0.02), (32, "RBF", 0.1)])
def test_vjp_of_three_channel_and_non_square_images(size, method, sigma):
    """a 3-channel input (view ld = 3), a 40 x 24 image (non-square, but 960 = 10 x 96 = 15 x 64 = 30 x 32 pixels: a whole number
    of batches in every kernel) and a 40 x 25 one (1000 = 10 x 96 + 40 = 15 x 64 + 40 = 31 x 32 + 8: a partial last batch in each),
    both backward paths; tests/test_hist_shapes_gpu.py goes through the tails class by class"""
    kw = dict(size=size, method=method, sigma=sigma)
    for img in (mid_range(47, 2, 64, 64, ch=3), mid_range(48, 2, 40, 24), mid_range(58, 2, 40, 25)):
        g = upstream(49, 2, size)
        got = vjp(lambda x: H.calculate_rgbuv_histogram(x, **kw), img, g)
        assert got.shape == img.shape
        assert_close(got, oracle_vjp(img, g, **kw), 1e-4, (img.shape, size, method))
    img = sprites(50, 2)[:, :40, :24].copy()
    g = upstream(51, 2, size)
    assert_close(vjp(lambda x: H.calculate_rgbuv_histogram(x, **kw), img, g), oracle_vjp(img, g, **kw), 2e-3, ("sprite 40x24", size))


def test_autograd_over_the_op_equals_the_fused_hellinger_gradient():
    """hellinger_loss(hist(real), hist(fake)) differentiated by torch against p2p_rgbuv_hist_hellinger_bwd3 (the fused step's
    kernels) on the same f32 images with coef = 1 / (2 sqrt2 B)"""
    B, S = 2, 64
    real = sprites(52, B)
    fake = np.clip(sprites(53, B) + np.random.default_rng(54).normal(scale=0.05, size=real.shape), -1, 1).astype(np.float32)
    x = torch.tensor(fake, device=U.DEV, requires_grad=True)
    H.hellinger_loss(H.calculate_rgbuv_histogram(real), H.calculate_rgbuv_histogram(x)).backward()
    got = x.grad.cpu().numpy()
    r_d, f_d = U.dev(real), U.dev(fake)
    vr, vf = L.Tensor(r_d.data_ptr(), S * S, S, 4), L.Tensor(f_d.data_ptr(), S * S, S, 4)
    n = B * 3 * 64 * 64
    h_r, h_f, gh = (torch.empty(n, dtype=torch.float32, device=U.DEV) for _ in range(3))
    tot = torch.empty((2, B), dtype=torch.float32, device=U.DEV)
    sq, sqp = torch.zeros(4, dtype=torch.float32, device=U.DEV), torch.zeros(B, dtype=torch.float32, device=U.DEV)
    dimg = torch.empty(B * S * S * 4, dtype=torch.float32, device=U.DEV)
    L.call("p2p_rgbuv_hist_fwd", L.F32, B, S, S, C.byref(vr), U.ptr(h_r), U.stream())
    L.call("p2p_rgbuv_hist_fwd", L.F32, B, S, S, C.byref(vf), U.ptr(h_f), U.stream())
    L.call("p2p_hellinger_fwd", U.ptr(h_r), U.ptr(h_f), B, U.ptr(tot[0]), U.ptr(tot[1]), U.ptr(sqp), U.ptr(sq), U.stream())
    L.call("p2p_rgbuv_hist_hellinger_bwd3", L.F32, B, S, S, C.byref(vf), U.ptr(h_r), U.ptr(h_f), U.ptr(tot[0]), U.ptr(tot[1]),
           U.ptr(sq), 1.0 / (2.0 * math.sqrt(2.0) * B), U.ptr(gh), U.ptr(dimg), U.stream())
    want = dimg.view(B, S, S, 4).cpu().numpy()
    assert np.linalg.norm(got - want) / np.linalg.norm(want) <= 1e-4


def _direct(img, size=64, method="inverse-quadratic", sigma=0.02):
    """the launch sequence of calculate_rgbuv_histogram before it became differentiable, issued through L.call"""
    t = U.dev(img)
    B, Hh, W, ch = t.shape
    view = L.Tensor(t.data_ptr(), Hh * W, W, ch)
    raw = torch.empty(B * 3 * size * size, dtype=torch.float32, device=U.DEV)
    if (size, method, sigma) == (64, "inverse-quadratic", 0.02):
        out = torch.empty((B, 64, 64, 3), dtype=torch.float32, device=U.DEV)
        L.call("p2p_rgbuv_hist_fwd", L.F32, B, Hh, W, C.byref(view), U.ptr(raw), U.stream())
        L.call("p2p_hist_normalize", U.ptr(raw), B, U.ptr(out), U.stream())
        return out
    L.call("p2p_rgbuv_hist_general", L.F32, B, Hh, W, C.byref(view), size, {"inverse-quadratic": 0, "RBF": 1}.get(method, 2), sigma,
           U.ptr(raw), U.stream())
    h = raw.view(B, 3, size, size).permute(0, 2, 3, 1)
    return (h / h.sum(dim=(1, 2, 3), keepdim=True)).contiguous()


def test_contract_of_the_differentiable_op():
    img = sprites(55, 2)
    eng = E.Pix2PixEngine(4, 4, "tanh", 64, L.F32)
    for kw in ({}, dict(size=32, method="RBF", sigma=0.1)):
        want = _direct(img, **kw)
        # no grad requested: exactly the values of the launch sequence above, and no autograd history
        plain = H.calculate_rgbuv_histogram(img, **kw)
        assert not plain.requires_grad and torch.equal(plain, want)
        x = torch.tensor(img, device=U.DEV, requires_grad=True)
        with torch.no_grad():
            ng = H.calculate_rgbuv_histogram(x, **kw)
        assert not ng.requires_grad and torch.equal(ng, want)
        # with grad: same values, and a gradient with the input's shape, bit-identical from one backward to the next
        out = H.calculate_rgbuv_histogram(x, **kw)
        assert out.requires_grad and torch.equal(out.detach(), want)
        g = torch.as_tensor(upstream(56, 2, out.shape[1]), device=U.DEV)
        g1, = torch.autograd.grad(out, x, g, retain_graph=True)
        g2, = torch.autograd.grad(out, x, g)
        assert g1.shape == x.shape and torch.equal(g1, g2) and torch.isfinite(g1).all()
        assert torch.count_nonzero(g1[..., 3]) == 0
    assert torch.equal(eng.rgbuv_histogram(img), _direct(img)) and not eng.rgbuv_histogram(img).requires_grad
    # channels beyond RGB get exactly zero; the gradient comes back in the caller's dtype and on the caller's device
    img5 = np.concatenate([img, img[..., :1]], -1)
    x5 = torch.tensor(img5, dtype=F64, requires_grad=True)                                   # host f64 leaf
    out = H.calculate_rgbuv_histogram(x5)
    assert out.device.type == "cuda" and out.dtype == torch.float32
    (out * torch.as_tensor(upstream(57, 2, 64), device=U.DEV)).sum().backward()
    assert x5.grad.dtype == F64 and x5.grad.device.type == "cpu" and x5.grad.shape == x5.shape
    assert torch.count_nonzero(x5.grad[..., 3:]) == 0 and torch.count_nonzero(x5.grad[..., :3]) > 0


def _params(seed):
    rng = np.random.default_rng(seed)
    Gp = rg.perturb_affine(rg.init_params(rg.generator_param_shapes(4, 4), rng, F64), rng)
    Dp = rg.perturb_affine(rg.init_params(rg.discriminator_param_shapes(4), rng, F64), rng)
    return rng, Gp, Dp


bce = torch.nn.functional.binary_cross_entropy_with_logits


def disc_ref(rp, fp):
    r, f = bce(rp, torch.ones_like(rp)), bce(fp, torch.zeros_like(fp))
    return r + f, r, f


def _grads(eng):
    return eng.G.export(eng.G.grads), eng.D.export(eng.D.grads)


def test_hooked_histogram_model_trains_on_its_histogram_term(tmp_path, monkeypatch):
    """train_step_rgba_hooked with a hook that restates Pix2PixHistogramModel.generator_loss (engine.rgbuv_histogram +
    histogram.hellinger_loss) reproduces the fused train_step_rgba(..., lambda_hist): losses 1e-5, every gradient tensor 1e-4 of
    its max-norm -- and the histogram term moves the gradients by far more than that, so the comparison cannot pass without it"""
    B, S, lam = 2, 64, 1.0
    rng, Gp, Dp = _params(81)
    src, tgt = rg.synthetic_rgba_batch(rng, B, S, palette_size=24)
    masks = [rng.integers(0, 2, size=s).astype(np.uint8) for s in rg.dropout_mask_shapes(B, S)]

    def engine():
        eng = E.Pix2PixEngine(4, 4, "tanh", S, L.F32)
        eng.set_params({k: v.numpy() for k, v in Gp.items()}, {k: v.numpy() for k, v in Dp.items()})
        return eng

    hooked = engine()

    def gen_hist(fp, fake, real):
        hist = H.hellinger_loss(hooked.rgbuv_histogram(real), hooked.rgbuv_histogram(fake))
        adv = bce(fp, torch.ones_like(fp))
        l1 = (real - fake).abs().mean()
        return adv + 100.0 * l1 + lam * hist, adv, l1, hist

    fused, plain = engine(), engine()
    out_f = fused.train_step_rgba(src, tgt, 100.0, lambda_hist=lam, masks=masks, apply_update=False).cpu().numpy()
    out_h = hooked.train_step_rgba_hooked(src, tgt, gen_hist, disc_ref, masks=masks, apply_update=False).cpu().numpy()
    plain.train_step_rgba(src, tgt, 100.0, masks=masks, apply_update=False)
    for i in range(7):
        assert abs(out_h[i] - out_f[i]) <= 1e-5 * abs(out_f[i]), (i, out_h[i], out_f[i])
    (gh_, dh_), (gf_, df_), (gp_, _) = _grads(hooked), _grads(fused), _grads(plain)
    for a, b in ((gh_, gf_), (dh_, df_)):
        for k in b:
            assert np.abs(a[k] - b[k]).max() <= 1e-4 * np.abs(b[k]).max() + 1e-12, k
    moved = max(np.abs(gf_[k] - gp_[k]).max() / (np.abs(gf_[k]).max() + 1e-30) for k in gf_)
    assert moved > 100 * 1e-4, moved

    # class level: a subclass whose generator_loss only calls super() takes the hooked step; the unsubclassed model the fused one
    monkeypatch.chdir(tmp_path)

    class Same(M.Pix2PixHistogramModel):
        def generator_loss(self, fake_predicted, fake_image, real_image):
            return super().generator_loss(fake_predicted, fake_image, real_image)

    batch = next(iter(D.synthetic_rgba_ds(B, batch_size=B, palette_size=24, seed=82)))
    runs = []
    for cls in (Same, M.Pix2PixHistogramModel):
        m = cls(None, None, "front2right", "hist-hook-test", lambda_l1=100.0, lambda_histogram=lam, dtype="f32", seed=7)
        g_loss, d_loss = m.train_step(batch, 0, 1)
        torch.cuda.synchronize()
        assert m._custom_hooks == (cls is Same)
        runs.append(([float(x) for x in g_loss + d_loss], _grads(m.engine)))
    (la, (ga, da)), (lb, (gb, db)) = runs
    for x, y in zip(la, lb):
        assert abs(x - y) <= 1e-5 * abs(y), (la, lb)
    for a, b in ((ga, gb), (da, db)):
        for k in b:
            assert np.abs(a[k] - b[k]).max() <= 1e-4 * np.abs(b[k]).max() + 1e-12, k


def test_custom_histogram_loss_matches_the_f64_oracle_under_autograd():
    """hooks: the reference's adversarial and L1 terms plus lambda * histogram.l2_loss of size-32 RBF sigma-0.1 histograms (the
    general backward), against the oracle graph differentiated in float64: losses 1e-5, gradients 1e-4 of max-norm.  Same weights,
    images and masks as the least-squares hook case of test_models_gpu.py; lambda makes the histogram term a fifth of the gradient."""
    B, S, lam = 2, 64, 1e5
    kw = dict(size=32, method="RBF", sigma=0.1)
    rng, Gp, Dp = _params(71)
    src, tgt = rg.synthetic_rgba_batch(rng, B, S, palette_size=24)
    masks = [rng.integers(0, 2, size=s).astype(np.uint8) for s in rg.dropout_mask_shapes(B, S)]

    def gen_l2(fp, fake, real, hist=H.calculate_rgbuv_histogram):
        adv = bce(fp, torch.ones_like(fp))
        l1 = (real - fake).abs().mean()
        hl = H.l2_loss(hist(real, **kw), hist(fake, **kw))
        return adv + 100.0 * l1 + lam * hl, adv, l1, hl

    eng = E.Pix2PixEngine(4, 4, "tanh", S, L.F32)
    eng.set_params({k: v.numpy() for k, v in Gp.items()}, {k: v.numpy() for k, v in Dp.items()})
    out = eng.train_step_rgba_hooked(src, tgt, gen_l2, disc_ref, masks=masks, apply_update=False).cpu().numpy()
    Gl = {k: v.clone().requires_grad_(True) for k, v in Gp.items()}
    Dl = {k: v.clone().requires_grad_(True) for k, v in Dp.items()}
    s64, t64 = torch.tensor(src, dtype=F64), torch.tensor(tgt, dtype=F64)
    fake = rg.unet_generator(Gl, s64, [torch.tensor(m, dtype=F64) for m in masks], "tanh")
    rp, fp = rg.patch_discriminator(Dl, t64, s64), rg.patch_discriminator(Dl, fake, s64)
    oracle_hist = lambda x, size, method, sigma: rg.rgbuv_histogram(x, size=size, sigma=sigma, method=method)   # noqa: E731
    g = gen_l2(fp, fake, t64, hist=oracle_hist)
    d = disc_ref(rp, fp)
    g_grads = torch.autograd.grad(g[0], list(Gl.values()), retain_graph=True, allow_unused=True)
    d_grads = torch.autograd.grad(d[0], list(Dl.values()), retain_graph=True, allow_unused=True)
    # not vacuous: without the histogram term the generator's gradient moves by far more than the tolerance
    g_plain = torch.autograd.grad(g[0] - lam * g[3], list(Gl.values()), allow_unused=True)
    assert max(float((a - b).abs().max() / a.abs().max()) for a, b in zip(g_grads, g_plain) if a is not None and a.abs().max() > 0) > 1e-2
    want = [float(x.detach()) for x in g] + [float(x.detach()) for x in d]
    for i in range(7):
        assert abs(out[i] - want[i]) <= 1e-5 * abs(want[i]), (i, out[i], want[i])
    for store, names, grads in ((eng.G, list(Gl), g_grads), (eng.D, list(Dl), d_grads)):
        got = store.export(store.grads)
        for k, gr in zip(names, grads):
            ref = np.zeros_like(got[k]) if gr is None else gr.numpy()
            assert np.abs(got[k] - ref).max() <= 1e-4 * np.abs(ref).max() + 1e-12, (k, np.abs(got[k] - ref).max(), np.abs(ref).max())


def test_overridden_histogram_model_trains_through_fit_in_bf16(tmp_path, monkeypatch):
    """the production dtype through fit(): an overridden generator_loss of the histogram model sees a differentiable histogram
    term at every step, and the reference's scalars (generator/histogram_loss among them) are logged finite"""
    monkeypatch.chdir(tmp_path)
    seen = []

    class Hooked(M.Pix2PixHistogramModel):
        def generator_loss(self, fake_predicted, fake_image, real_image):
            total, adv, l1, hist = super().generator_loss(fake_predicted, fake_image, real_image)
            seen.append(hist.requires_grad)
            return total, adv, l1, hist

    train = D.synthetic_rgba_ds(8, batch_size=4, palette_size=24)
    m = Hooked(train, train, "front2right", "hist-hook-fit-test", lambda_l1=30.0, lambda_histogram=1.0)
    m.fit(10, 5)
    assert len(seen) == 10 and all(seen) and m.engine.G.t == 10
    rows = [json.loads(r) for r in open(m.summary_writer.path)]
    names = {r["name"] for r in rows}
    assert "generator/histogram_loss" in names and "generator/total_loss" in names and "discriminator/total_loss" in names
    assert sum(1 for r in rows if r["name"] == "generator/histogram_loss") == 10
    assert all(np.isfinite(r["value"]) for r in rows), [r for r in rows if not np.isfinite(r["value"])]
    assert os.path.exists(m.summary_writer.path)
