"""Not-gpu: the ill-conditioned cases of tests/numeric_edges.py can fail, and their caps hold -- from NumPy alone.

For every InstanceNorm case and dtype:
  * a float32 two-pass restatement stays within half of the rstd bound, of the output tolerance and of the constant-channel bound
    (a bf16 store takes its own half ulp on top), and within half of the mean bound on the maps the lane-group form serves (<= 16
    pixels).  On larger maps a plain float32 sum of 256 +- 1 values carries about one ulp of 256 into the mean: up to 0.59 of the
    bound -- inside it, not inside half of it; the shifted sums that serve those maps stay within half (mean) / the whole (rstd);
  * a float32 plain-sum restatement (E[x^2] - E[x]^2, what nobody must be able to put back unnoticed) exceeds the rstd bound >= 10x on
    the offset and the variance << eps regimes -- but for bf16 at 2x2 pixels, where plain sums are exact;
  * the kink exclusion of the backward check stays <= 0.1 %, the builders are deterministic, the bf16 regimes survive their rounding,
    and the cases together reach every statistics-computing arm of the norm launchers.
The slot-pooled form, the conv operands and the fused block have self-tests of their own below."""
import numpy as np
import pytest

from oracle import np_restatement as npr
from palette_and_histo_gan_amd import _lib as L
from tests import gpu_util as U
from tests import numeric_edges as NE

CASES = [pytest.param(c, d, id=f"{c.id}-{'f32' if d == L.F32 else 'bf16'}") for d in NE.DTYPES for c in NE.NORM_CASES]


def _by_regime(e, c):
    """{regime: max of e [n, c] over the regime's channels}"""
    return {r: float(e[:, [ch for ch in range(c) if NE.regime(ch) == r]].max()) for r in range(6) if r < c}


@pytest.mark.parametrize("case,dtype", CASES)
def test_two_pass_float32_meets_the_bounds_and_plain_sums_do_not(case, dtype):
    x, gamma, beta, mask = NE.norm_input(case, dtype)
    again = NE.norm_input(case, dtype)
    assert all(np.array_equal(a, b) for a, b in zip((x, gamma, beta), again[:3]))
    assert (mask is None) == (again[3] is None) and (mask is None or np.array_equal(mask, again[3]))
    assert np.array_equal(x, U.q(x, dtype))

    hw = case.h * case.h
    mu, rs = NE.two_pass_f32(x)
    e_mu, e_rs = NE.stat_errors(mu, rs, x)
    e_mu_s, e_rs_s = NE.stat_errors(*NE.shifted_f32(x), x)
    # rs: two-pass sums within half the bound, shifted sums (the register-resident and workgroup forms) within it.  mu: the restatement of
    # the form that serves the map within half -- two-pass on <= 16 pixels (the lane-group form), shifted sums above; a plain f32
    # sum of >= 64 values of 256 +- 1 carries about one ulp of 256, 0.6 of the bound: within the bound, not within half of it
    assert e_rs.max() <= 0.5 and e_rs_s.max() <= 1.0, (_by_regime(e_rs, case.c), _by_regime(e_rs_s, case.c))
    assert e_mu.max() <= 1.0 and e_mu_s.max() <= 0.5 and (hw > 16 or e_mu.max() <= 0.5), (e_mu.max(), e_mu_s.max())

    _, e_plain = NE.stat_errors(*NE.plain_f32(x), x)
    worst = _by_regime(e_plain, case.c)
    if dtype == L.BF16 and hw <= 4:
        # four bf16 values: their f32 sum and sum of squares (8-bit significands, 16-bit squares) are exact, so plain sums are as
        # good as any algorithm here -- the one shape where nothing can tell them apart
        assert max(worst.values()) <= 0.5
    else:
        assert worst[1] >= 10 and worst[3] >= 10, worst
    print(f"\n{case.id}: rs error / bound  two-pass {e_rs.max():.2f}  shifted {e_rs_s.max():.2f}  plain sums " +
          " ".join(f"R{r} {v:.3g}x" for r, v in worst.items()))

    # apply pass from its own statistics, and the constant channels
    ref = NE.apply64(x, mu, rs, gamma, beta, case.act, mask)
    out = NE.apply_f32(x, mu, rs, gamma, beta, case.act, mask)
    assert NE.plane_err(out, ref) <= 0.5 * NE.OUT_TOL[dtype]
    out = U.q(out, dtype).astype(np.float64)           # the bf16 store alone takes up to 2^-8 of the 6e-3
    assert NE.plane_err(out, ref) <= NE.OUT_TOL[dtype]
    const = [ch for ch in range(case.c) if NE.regime(ch) in NE.CONSTANT]
    dev = np.abs(out - NE.constant_ref(x, beta, case.act, mask))[..., const]
    bound = NE.constant_out_bound(x, gamma, beta, case.act, mask, dtype)[..., const]
    assert (dev <= (0.5 if dtype == L.F32 else 1.0) * bound).all(), float((dev / bound).max())
    assert (np.abs(beta[const]) >= 0.05).all()

    # the backward reference alone respects the cap on undecided activation gates
    mean, rs64, _ = NE.stats64(x)
    dy1, dy2 = NE.grad_sources(case, dtype)
    dy = dy1[..., 8:].astype(np.float64) + (dy2.astype(np.float64).sum(0) if case.gslabs else dy2)
    dx, dgamma, dbeta, kink = NE.backward64(x, mean, rs64, gamma, beta, case.act, mask, dy)
    assert kink.mean() <= NE.KINK_SHARE and np.isfinite(dx).all()


@pytest.mark.parametrize("case,dtype", [p for p in CASES if p.values[0].slots])
def test_pooled_slots_meet_the_bounds_and_need_their_cross_term(case, dtype):
    """the slot partials made for the apply-only form: pooled by the parallel-variance rule in float32 they meet half the bounds;
    without the cnt (mi - mall)^2 term the pooled variance loses the spread BETWEEN the slots"""
    x = NE.norm_input(case, dtype)[0]
    hw = case.h * case.h
    sp = NE.slot_partials(x, case.slots)
    mean, rs64 = NE.pooled64(sp, hw)
    e_mu, e_rs = NE.given_stat_errors(*NE.pooled_f32(sp, hw), mean, rs64, x)
    assert e_mu.max() <= 1.0 and e_rs.max() <= 0.5, (e_mu.max(), _by_regime(e_rs, case.c))      # mu: 16 slot means of 256 added one by one
    _, e_drop = NE.given_stat_errors(*NE.pooled_f32(sp, hw, cross_term=False), mean, rs64, x)
    worst = _by_regime(e_drop, case.c)
    assert worst[0] >= 10 and worst[1] >= 10 and worst[2] >= 10, worst
    # and the stored slots describe the data: within twice the bounds of the data's own moments (see numeric_edges.pooled64)
    e_mu, e_rs = NE.stat_errors(mean, rs64, x)
    assert e_mu.max() <= 2.0 and e_rs.max() <= 2.0, (e_mu.max(), e_rs.max())


def _stored(op, a, w, dtype):
    import torch
    from oracle import reference_graph as rg
    conv = rg.conv4x4_s2 if op == L.OP_G else rg.convT4x4_s2
    return U.q(conv(torch.tensor(a, dtype=torch.float64), torch.tensor(w, dtype=torch.float64)).numpy(), dtype)


@pytest.mark.parametrize("dtype", NE.DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("op,n,lh,cg,cd", NE.IGEMM_CASES)
def test_conv_operands_reach_their_ratio(dtype, op, n, lh, cg, cd):
    """positive operands whose stored convolution result has mean / std ~ 64 (f32) / 16 (bf16); float32 two-pass statistics of it
    stay within half the bounds"""
    a, w, ratio = NE.conv_operands(op, n, lh, lh, cg, cd, dtype, NE.CONV_RATIO[dtype])
    assert abs(ratio / NE.CONV_RATIO[dtype] - 1) < 0.1 and a.min() > 0 and w.min() > 0
    assert all(np.array_equal(p, q) for p, q in zip((a, w), NE.conv_operands(op, n, lh, lh, cg, cd, dtype, NE.CONV_RATIO[dtype])[:2]))
    x = _stored(op, a, w, dtype)
    e_mu, e_rs = NE.given_stat_errors(*NE.two_pass_f32(x), *NE.stats64(x)[:2], x)
    assert e_mu.max() <= 0.5 and e_rs.max() <= 0.5


@pytest.mark.parametrize("op,n,lh,cg,cd,act", NE.FUSED_CASES)
def test_the_fused_block_case_tells_plain_sums_by_its_statistics_not_by_the_graph(op, n, lh, cg, cd, act):
    """The graph comparison cannot tell: a convolution result on a bf16 rounding boundary falls either way with the order of the f32
    sum, one bf16 ulp of a value 64 std from 0 is 0.25 std, and that moves the float32 CPU graph by ~0.1 of the output whatever
    its statistics are -- with plain sums the deviation is the same number.  What does tell is the check of the statistics against
    the block's own stored result: two-pass float32 within half the bounds, plain sums >= 10x outside."""
    a, w, ratio = NE.conv_operands(op, n, lh, lh, cg, cd, L.BF16, NE.FUSED_RATIO, scale=NE.FUSED_SCALE)
    assert abs(ratio / NE.FUSED_RATIO - 1) < 0.1
    ncols = cd if op == L.OP_G else cg
    rng = np.random.default_rng(8)
    gamma, beta = (1 + 0.2 * rng.normal(size=ncols)).astype(np.float32), (0.2 * rng.normal(size=ncols)).astype(np.float32)
    ref, dev32 = NE.fused_graphs(op, a, w, gamma, beta, act)
    _, dev_plain = NE.fused_graphs(op, a, w, gamma, beta, act, NE.plain_f32)
    x = _stored(op, a, w, L.BF16)
    mean, rs, _ = NE.stats64(x)
    e_mu, e_rs = NE.given_stat_errors(*NE.two_pass_f32(x), mean, rs, x)
    _, e_plain = NE.given_stat_errors(*NE.plain_f32(x), mean, rs, x)
    print(f"\nfused {'GP'[op]}: float32 CPU graph deviation {dev32:.3f}, with plain sums {dev_plain:.3f}; rs error / bound two-pass "
          f"{e_rs.max():.2f} plain sums {e_plain.max():.0f}x")
    assert dev32 > NE.OUT_TOL[L.BF16] and dev_plain < 10 * max(NE.OUT_TOL[L.BF16], 3 * dev32)
    assert e_mu.max() <= 0.5 and e_rs.max() <= 0.5 and e_plain.max() >= 10


def test_bf16_regimes_survive_their_rounding():
    case = NE.NormCase(2, 16, 12, L.ACT_RELU, False)
    x = NE.norm_input(case, L.BF16)[0].astype(np.float64)
    for ch in range(case.c):
        mean, std, _ = NE.REGIMES[L.BF16][NE.regime(ch)]
        got = x[..., ch].std(axis=(1, 2))
        if std:
            assert (got >= 0.5 * std).all(), (ch, got)
            assert (np.abs(np.abs(x[..., ch].mean(axis=(1, 2))) - mean) <= max(0.5 * mean, 3 * std)).all()
        else:
            assert (got == 0).all()
    assert (x[1, :, :, 1] < 0).all() and (x[0, :, :, 1] > 0).all()          # the offset's sign alternates between images
    assert x[0, 0, 0, 2] == 40.0


def test_the_backward_closed_form_is_np_restatements():
    rng = np.random.default_rng(3)
    x, dy = rng.normal(size=(2, 4, 4, 6)) + 3, rng.normal(size=(2, 4, 4, 6))
    gamma, beta = 1 + 0.1 * rng.normal(size=6), np.full(6, 1e3)           # every gate open: LeakyReLU's slope 1
    mean, rs, _ = NE.stats64(x)
    dx, dgamma, dbeta, kink = NE.backward64(x, mean, rs, gamma, beta, L.ACT_LEAKY, None, dy)
    want = npr.instance_norm_backward(x, gamma, dy, eps=NE.EPS)
    for a, b in zip((dx, dgamma, dbeta), want):
        np.testing.assert_allclose(a, b, rtol=1e-12, atol=1e-12)
    assert not kink.any()
    np.testing.assert_allclose(NE.apply64(x, mean, rs, gamma, beta, L.ACT_NONE, None), npr.instance_norm(x, gamma, beta, NE.EPS), rtol=1e-12)


@pytest.mark.parametrize("nslabs", [1, 2, 3, 4, 5, 7, 16])
def test_power_of_two_slabs_sum_to_the_input_bit_for_bit(nslabs):
    x = NE.norm_input(NE.NormCase(2, 4, 16, L.ACT_RELU, False), L.F32)[0]
    slabs = NE.pow2_slabs(x, nslabs)
    acc = np.zeros_like(x)
    for s in slabs:
        acc = acc + s
    assert slabs.dtype == np.float32 and len(slabs) == nslabs and np.array_equal(acc, x)


def test_the_cases_reach_every_statistics_computing_arm():
    want_f, want_b = NE.statistics_arms()
    got = [NE.norm_routes(c, d) for d in NE.DTYPES for c in NE.NORM_CASES]
    assert want_f <= {f for f, _ in got}, sorted(want_f - {f for f, _ in got})
    assert want_b <= {b for _, b in got}, sorted(want_b - {b for _, b in got})
    assert len(want_f) == 13 and len(want_b) == 12          # small and reg x 4 pixel counts, each x 2 loaders; vec0, vec1+2 (, vec3)


def test_loss_adam_and_colour_builders():
    for dtype in NE.DTYPES:
        x = NE.bce_logits(dtype).astype(np.float64)
        half = x.shape[0] // 2
        for e in NE.BCE_EDGES:
            q = float(U.q(np.array([e]), dtype)[0])
            assert (x[:half] == q).sum() >= 2 and (x[half:] == q).sum() >= 2, e
        assert np.isfinite(NE.bce64(x, 1.0)).all() and NE.bce64(np.array([-3e4]), 1.0)[0] == 3e4
        z, pos = NE.tanh_field(dtype)
        assert all((z.reshape(-1)[p] == U.q(np.array([e]), dtype)[0]).all() for e, p in zip(NE.TANH_EDGES, pos))
    g = NE.adam_gradients()
    assert np.array_equal(g, NE.adam_gradients()) and NE.ADAM_N % 4
    mags = np.abs(g[:, 128:NE.ADAM_N // 4 * 4].reshape(3, -1, 4))
    assert ((mags.max(-1) >= 1) & (mags.min(-1) <= 1e-18)).mean() > 0.5           # most 16-byte vectors mix large and tiny entries
    assert not g[:, :64].any() and g[0, 64:128].all() and not g[1:, 64:128].any()
    ref = NE.adam_reference(np.ones(NE.ADAM_N), g)
    assert all(np.isfinite(v).all() for step in ref for v in step)
    for size, tiles in ((32, 1), (64, 4)):
        img, want = NE.points_batch(size)
        assert np.array_equal(img, NE.points_batch(size)[0]) and want.tolist() == [64, -1, tiles, -1]
        per_tile = [[len(np.unique(t[:, :3], axis=0)) for t in im.reshape(tiles, 1024, 4)] for im in img]
        assert per_tile[0] == [64 // tiles] * tiles and sum(per_tile[1]) == 65 and per_tile[2] == [1] * tiles
        assert per_tile[3] == [1024] * tiles and (img[2, ..., :3] == -1).all() and np.abs(img).max() <= 1
