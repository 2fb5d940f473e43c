"""-m gpu: overridable loss hooks of Pix2PixIndexedModel.  p2p_softmax_bwd (the VJP of the 256-way softmax plus a direct logits
gradient) against float64, engine.train_step_indexed_hooked against the fused step and against the f64 oracle under autograd,
the engine state it shares with the fused step, and the class-level opt-in `differentiable_loss_hooks`."""
import ctypes as C
import json
import types

import numpy as np
import pytest
import torch

from oracle import reference_graph as rg
from palette_and_histo_gan_amd import _lib as L
from palette_and_histo_gan_amd import dataset_utils as D
from palette_and_histo_gan_amd import engine as E
from palette_and_histo_gan_amd import pix2pix_model as M
from tests import gpu_util as U

pytestmark = pytest.mark.gpu
F64 = torch.float64
S, CN = 64, 256
bce = torch.nn.functional.binary_cross_entropy_with_logits


# ---------------------------------------------------------------------------------------------------- the kernel
def _logits(N, seed):
    g = torch.Generator(device=U.DEV).manual_seed(seed)
    z = torch.randn((N * S * S, CN), generator=g, device=U.DEV) * 3.0
    wide = torch.arange(0, N * S * S, 7, device=U.DEV)          # every 7th pixel: a +-30 spread, low classes underflow
    ramp = torch.linspace(-30.0, 30.0, CN, device=U.DEV)
    perm = torch.argsort(torch.rand((len(wide), CN), generator=g, device=U.DEV), dim=1)
    z[wide] = ramp[perm]
    return z.contiguous()


def _probs(z, N):
    """the library's own softmax (p2p_softmax_cce_argmax, f32, no gradient)"""
    zv = L.Tensor(z.data_ptr(), S * S, S, CN)
    idx = torch.zeros(N * S * S, dtype=torch.float32, device=U.DEV)
    tv = L.Tensor(idx.data_ptr(), S * S, S, 1)
    fake = torch.zeros_like(idx)
    fv = L.Tensor(fake.data_ptr(), S * S, S, 1)
    probs = torch.empty((N * S * S, CN), dtype=torch.float32, device=U.DEV)
    part, loss = torch.zeros(2 * 8192, dtype=torch.float32, device=U.DEV), torch.zeros(2, dtype=torch.float32, device=U.DEV)
    L.call("p2p_softmax_cce_argmax", L.F32, N, S, S, CN, C.byref(zv), C.byref(tv), C.byref(fv), 0.0, 0.0, None, U.ptr(probs),
           U.ptr(part), U.ptr(loss), U.stream())
    return probs


SENT, LD, COFF = 3.5, 272, 8          # dz view: channels 8..263 of 272-channel haloed pixels


def _launch(dtype, N, probs, gp, gz, scale):
    """dz into a NaN-prefilled interior inside a sentinel-filled halo and sentinel neighbouring channels"""
    hp = S + 2 * E.HALO
    buf = torch.full((N, hp, hp, LD), SENT, dtype=U.tdt(dtype), device=U.DEV)
    inner = slice(E.HALO, E.HALO + S)
    buf[:, inner, inner, COFF:COFF + CN] = float("nan")
    off = ((E.HALO * hp) + E.HALO) * LD + COFF
    view = L.Tensor(buf.data_ptr() + off * buf.element_size(), hp * hp, hp, LD)
    p = lambda t: None if t is None else U.ptr(t)          # noqa: E731
    L.call("p2p_softmax_bwd", dtype, N, S, S, CN, U.ptr(probs), p(gp), p(gz), scale, C.byref(view), U.stream())
    return buf


@pytest.mark.parametrize("N", [1, 3, 128])
def test_softmax_bwd_matches_float64(N):
    z = _logits(N, 11 + N)
    probs = _probs(z, N)
    g = torch.Generator(device=U.DEV).manual_seed(5 + N)
    gp = torch.randn((N * S * S, CN), generator=g, device=U.DEV)
    gz = torch.randn((N * S * S, CN), generator=g, device=U.DEV)
    scale = -0.37
    assert float(probs[::7].min()) < 1e-7 and bool(torch.isfinite(probs).all())
    p64 = probs.double()
    inner = slice(E.HALO, E.HALO + S)
    for use_gp, use_gz in ((True, False), (False, True), (True, True), (False, False)):
        ref = torch.zeros_like(p64)
        if use_gp:
            g64 = gp.double()
            ref += p64 * (g64 - (p64 * g64).sum(-1, keepdim=True))
        if use_gz:
            ref += gz.double()
        ref *= scale
        pix_max = ref.abs().amax(-1, keepdim=True)
        for dtype in (L.F32, L.BF16):
            a = _launch(dtype, N, probs, gp if use_gp else None, gz if use_gz else None, scale)
            b = _launch(dtype, N, probs, gp if use_gp else None, gz if use_gz else None, scale)
            torch.cuda.synchronize()
            what = (N, use_gp, use_gz, dtype)
            # only the view's own pixels and channels are written
            keep = torch.ones(a.shape, dtype=torch.bool, device=U.DEV)
            keep[:, inner, inner, COFF:COFF + CN] = False
            assert bool((a[keep] == SENT).all()), what
            got = a[:, inner, inner, COFF:COFF + CN].reshape(-1, CN)
            assert bool(torch.isfinite(got).all()), what
            assert torch.equal(a, b), what                     # bit-identical relaunch
            if not (use_gp or use_gz):
                assert int(torch.count_nonzero(got)) == 0, what
                continue
            err = (got.double() - ref).abs()
            if dtype == L.F32:
                bound = 1e-6 * pix_max
            else:
                bound = 2.0 ** -8 * ref.abs() + 1e-6 * pix_max
            worst = float((err - bound).max())
            assert worst <= 0.0, (what, worst, float((err / pix_max.clamp_min(1e-30)).max()))
    # C = 128: refused before any launch (the view would be written at 128 channels per pixel)
    dz128 = torch.zeros((N * S * S, 128), dtype=torch.float32, device=U.DEV)
    v128 = L.Tensor(dz128.data_ptr(), S * S, S, 128)
    assert L.lib().p2p_softmax_bwd(L.F32, N, S, S, 128, U.ptr(probs), U.ptr(gp), None, 1.0, C.byref(v128), U.stream()) < 0
    assert "256" in L.lib().p2p_last_error().decode()
    with pytest.raises(L.P2PError, match="256"):
        L.call("p2p_softmax_bwd", L.F32, N, S, S, 128, U.ptr(probs), None, U.ptr(gz), 1.0, C.byref(v128), U.stream())
    assert int(torch.count_nonzero(dz128)) == 0


# ---------------------------------------------------------------------------------------------------- the hooked step
def _params(seed):
    """the indexed model's weights (as tests/test_hist_indexed_gpu.py draws them: the index inputs are un-normalised, 0..255,
    so the first-layer kernels are scaled down)"""
    rng = np.random.default_rng(seed)
    Gp = rg.perturb_affine(rg.init_params(rg.generator_param_shapes(1, CN), rng, F64), rng)
    Dp = rg.perturb_affine(rg.init_params(rg.discriminator_param_shapes(1), rng, F64), rng)
    Gp["down1.kernel"] *= 0.05
    Dp["down.kernel"] *= 0.05
    return rng, Gp, Dp


def _batch(rng, B):
    src, tgt, _pal = rg.synthetic_indexed_batch(rng, B, S)
    masks = [rng.integers(0, 2, size=s).astype(np.uint8) for s in rg.dropout_mask_shapes(B, S)]
    return src, tgt, masks


def _engine(dtype, Gp, Dp):
    eng = E.Pix2PixEngine(1, CN, "softmax", S, dtype)
    eng.set_params({k: v.numpy() for k, v in Gp.items()}, {k: v.numpy() for k, v in Dp.items()})
    return eng


def restated_hooks(lam):
    """Pix2PixIndexedModel's own formulas (pix2pix_model.py:44-56,273-278) in torch, the CCE through `_keras_logits`"""
    cce = M.CategoricalCrossentropy()

    def gen(fp, probs, onehot):
        adv = bce(fp, torch.ones_like(fp))
        l1 = (onehot - probs).abs().mean()
        seg = cce(onehot, probs)
        return adv + 0.0 * l1 + lam * seg, adv, l1, seg

    def disc(rp, fp):
        r, f = bce(rp, torch.ones_like(rp)), bce(fp, torch.zeros_like(fp))
        return r + f, r, f

    return gen, disc


def test_restated_reference_hooks_reproduce_the_fused_step():
    B, lam = 2, 0.5
    rng, Gp, Dp = _params(71)
    src, tgt, masks = _batch(rng, B)
    gen, disc = restated_hooks(lam)
    fused, hooked = _engine(L.F32, Gp, Dp), _engine(L.F32, Gp, Dp)
    out_f = fused.train_step_indexed(src, tgt, lam, masks=masks, apply_update=False).cpu().numpy()
    out_h = hooked.train_step_indexed_hooked(src, tgt, gen, disc, masks=masks, apply_update=False).cpu().numpy()
    print("fused", out_f, "hooked", out_h)
    for i in range(7):
        assert abs(out_h[i] - out_f[i]) <= 1e-6 * abs(out_f[i]), (i, out_h[i], out_f[i])
    for a, b in ((hooked.G, fused.G), (hooked.D, fused.D)):
        ga, gb = a.export(a.grads), b.export(b.grads)
        for k in ga:
            assert np.abs(ga[k] - gb[k]).max() <= 1e-5 * np.abs(gb[k]).max() + 1e-12, (k, np.abs(ga[k] - gb[k]).max(), np.abs(gb[k]).max())


GAMMA, LAM_LS, EPS_LS = 2.0, 0.5, 0.1


def focal_hooks():
    """focal loss on the probabilities (gamma 2: d/d probs) + lambda * label-smoothed CCE on the cached logits (d/d logits);
    least-squares GAN discriminator"""
    def gen(fp, probs, onehot):
        adv = ((fp - 1.0) ** 2).mean()
        pt = (probs * onehot).sum(-1)
        focal = (-((1.0 - pt) ** GAMMA) * pt.clamp_min(1e-30).log()).mean()
        smooth = onehot * (1.0 - EPS_LS) + EPS_LS / CN
        ls = -(smooth * torch.log_softmax(probs._keras_logits, dim=-1)).sum(-1).mean()
        return adv + focal + LAM_LS * ls, adv, focal, ls

    def disc(rp, fp):
        r, f = ((rp - 1.0) ** 2).mean(), (fp ** 2).mean()
        return 0.5 * (r + f), r, f

    return gen, disc


def _oracle(Gp, Dp, src, tgt, masks, gen, disc):
    Gl = {k: v.clone().requires_grad_(True) for k, v in Gp.items()}
    Dl = {k: v.clone().requires_grad_(True) for k, v in Dp.items()}
    s64, t64 = torch.tensor(src, dtype=F64), torch.tensor(tgt, dtype=F64)
    logits = rg.unet_generator(Gl, s64, [torch.tensor(m, dtype=F64) for m in masks], "logits")
    probs = torch.softmax(logits, dim=-1)
    probs._keras_logits = logits
    fake_idx = torch.argmax(probs, dim=-1, keepdim=True).to(F64)
    rp, fp = rg.patch_discriminator(Dl, t64, s64), rg.patch_discriminator(Dl, fake_idx, s64)
    onehot = torch.nn.functional.one_hot(torch.tensor(tgt[..., 0]).long(), CN).to(F64)
    g, d = gen(fp, probs, onehot), disc(rp, fp)
    g_grads = torch.autograd.grad(g[0], list(Gl.values()), retain_graph=True, allow_unused=True)
    d_grads = torch.autograd.grad(d[0], list(Dl.values()), allow_unused=True)
    zg = lambda gr, x: torch.zeros_like(x) if gr is None else gr          # noqa: E731
    return ([float(x.detach()) for x in g] + [float(x.detach()) for x in d],
            {k: zg(gr, Gl[k]).numpy() for k, gr in zip(Gl, g_grads)}, {k: zg(gr, Dl[k]).numpy() for k, gr in zip(Dl, d_grads)})


def test_focal_and_label_smoothed_hooks_match_the_f64_oracle_under_autograd():
    """losses 1e-5 of the oracle's; every gradient tensor within 1e-4 of its max-norm, or within 1.5 x the fused step's own error
    against rg.train_step_indexed on the same weights and batch where that is larger (f32 mode: the un-normalised index inputs put
    the generator's first layers ~5e-4 of max-norm from the f64 graph in the fused step too, tests/test_hist_indexed_gpu.py)"""
    B, lam = 2, 0.5
    rng, Gp, Dp = _params(71)
    src, tgt, masks = _batch(rng, B)
    gen, disc = focal_hooks()
    eng = _engine(L.F32, Gp, Dp)
    out = eng.train_step_indexed_hooked(src, tgt, gen, disc, masks=masks, apply_update=False).cpu().numpy()
    want, g_ref, d_ref = _oracle(Gp, Dp, src, tgt, masks, gen, disc)
    print("hooked", out, "oracle", want)
    for i in range(7):
        assert abs(out[i] - want[i]) <= 1e-5 * abs(want[i]), (i, out[i], want[i])
    fused = _engine(L.F32, Gp, Dp)
    fused.train_step_indexed(src, tgt, lam, masks=masks, apply_update=False)
    yard = rg.train_step_indexed(Gp, Dp, torch.tensor(src), torch.tensor(tgt), [torch.tensor(m, dtype=F64) for m in masks], lam)
    rel = lambda a, r: float(np.abs(a - r).max() / (np.abs(r).max() + 1e-30))          # noqa: E731
    worst = []
    for store, ref, fstore, fref in ((eng.G, g_ref, fused.G, yard["g_grads"]), (eng.D, d_ref, fused.D, yard["d_grads"])):
        got, fgot = store.export(store.grads), fstore.export(fstore.grads)
        for k in ref:
            eh, ef = rel(got[k], ref[k]), rel(fgot[k], fref[k].numpy())
            worst.append((eh, k, ef))
            assert eh <= max(1e-4, 1.5 * ef), (k, eh, ef)
    print("worst (hooked, tensor, fused)", sorted(worst)[-3:])


def test_bf16_hooked_step_against_the_oracle_with_the_fused_step_as_yardstick():
    B, lam = 4, 0.5
    rng, Gp, Dp = _params(73)
    src, tgt, masks = _batch(rng, B)
    with rg.storage_dtype(torch.bfloat16):
        ref = rg.train_step_indexed(Gp, Dp, torch.tensor(src), torch.tensor(tgt), [torch.tensor(m, dtype=F64) for m in masks], lam)
    gen, disc = restated_hooks(lam)
    fused, hooked = _engine(L.BF16, Gp, Dp), _engine(L.BF16, Gp, Dp)
    fused.train_step_indexed(src, tgt, lam, masks=masks, apply_update=False)
    out = hooked.train_step_indexed_hooked(src, tgt, gen, disc, masks=masks, apply_update=False).cpu().numpy()
    assert np.isfinite(out).all()
    gf, gh = fused.G.export(fused.G.grads), hooked.G.export(hooked.G.grads)
    worst = []
    for k, r in ref["g_grads"].items():
        r = r.numpy()
        n = np.linalg.norm(r)
        if n == 0.0:        # down6 normalises 1 x 1 maps: no gradient reaches its kernel in the oracle
            continue
        ef, eh = np.linalg.norm(gf[k] - r) / n, np.linalg.norm(gh[k] - r) / n
        worst.append((eh - 1.5 * ef, k, eh, ef))
        assert eh <= 1.5 * ef + 1e-3, (k, eh, ef)
    print("worst (margin, tensor, hooked, fused)", max(worst))


def test_fused_step_after_a_hooked_step_is_bit_identical_to_a_fresh_one():
    """the hooked step shares the plan (dz, dld, the head's bias-gradient flag) with the fused one: fused -> hooked -> fused on one
    engine ends exactly where a fresh engine's fused step does (bf16: the fused head sums last.bias itself)"""
    B, lam = 4, 0.5
    rng, Gp, Dp = _params(74)
    src, tgt, masks = _batch(rng, B)
    gen, disc = focal_hooks()
    one, fresh = _engine(L.BF16, Gp, Dp), _engine(L.BF16, Gp, Dp)
    one.train_step_indexed(src, tgt, lam, masks=masks, apply_update=False)
    one.train_step_indexed_hooked(src, tgt, gen, disc, masks=masks, apply_update=False)
    hooked_bias = one.G.export(one.G.grads)["last.bias"].copy()
    out_a = one.train_step_indexed(src, tgt, lam, masks=masks, apply_update=False)
    out_b = fresh.train_step_indexed(src, tgt, lam, masks=masks, apply_update=False)
    torch.cuda.synchronize()
    assert torch.equal(out_a, out_b), (out_a, out_b)
    assert torch.equal(one.G.grads, fresh.G.grads) and torch.equal(one.D.grads, fresh.D.grads)
    ga, gb = one.G.export(one.G.grads), fresh.G.export(fresh.G.grads)
    assert np.array_equal(ga["last.bias"], gb["last.bias"]) and not np.array_equal(hooked_bias, gb["last.bias"])


# ---------------------------------------------------------------------------------------------------- the class level
class FocalIndexed(M.Pix2PixIndexedModel):
    differentiable_loss_hooks = True
    seen = []

    def generator_loss(self, fake_predicted, fake_image, real_image):
        FocalIndexed.seen.append((fake_image.requires_grad, hasattr(fake_image, "_keras_logits"), tuple(fake_image.shape),
                                  bool(((real_image == 0) | (real_image == 1)).all()) and bool((real_image.sum(-1) == 1).all())))
        adv = self.loss_object(torch.ones_like(fake_predicted), fake_predicted)
        pt = (fake_image * real_image).sum(-1)
        seg = (-((1.0 - pt) ** GAMMA) * pt.clamp_min(1e-30).log()).mean()
        l1 = (real_image - fake_image).abs().mean()
        return adv + self.lambda_segmentation * seg, adv, l1, seg


def test_opted_in_subclass_trains_through_fit_in_bf16(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    FocalIndexed.seen.clear()
    train = D.synthetic_indexed_ds(8, batch_size=4)
    m = FocalIndexed(train, train, "front2right", "indexed-hook-fit-test", lambda_segmentation=0.5)
    w0 = m.engine.G.params.clone()
    m.fit(10, 5)
    assert m._custom_hooks and m.engine.G.t == 10
    assert len(FocalIndexed.seen) == 10 and all(s == (True, True, (4, 64, 64, CN), True) for s in FocalIndexed.seen), FocalIndexed.seen
    assert not torch.equal(m.engine.G.params, w0)
    rows = [json.loads(r) for r in open(m.summary_writer.path)]
    seg = [r["value"] for r in rows if r["name"] == "generator/segmentation_loss"]
    print("segmentation loss", seg)
    assert len(seg) == 10 and all(np.isfinite(r["value"]) for r in rows)
    assert seg[-1] < 0.9 * seg[0], seg          # measured: 5.69 -> 4.83 (0.85x) in 10 steps


def test_hooks_without_the_opt_in_or_with_data_parallel_are_refused(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    ids = D.synthetic_indexed_ds(4, batch_size=4)

    class NoOptIn(FocalIndexed):
        differentiable_loss_hooks = False

    with pytest.raises(NotImplementedError, match="fused"):
        NoOptIn(ids, ids, "front2right", "indexed-hook-test").train_step(next(iter(ids)), 0, 1)
    dp = types.SimpleNamespace(rank=0, world=1)
    m = FocalIndexed(ids, ids, "front2right", "indexed-hook-test", data_parallel=dp)
    with pytest.raises(NotImplementedError, match="one GPU"):
        m.train_step(next(iter(ids)), 0, 1)
