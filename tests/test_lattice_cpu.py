"""tests/lattice.py without a GPU: the generated operands are dtype values, f32 accumulation of a lattice launch is exact in any
order (the premise of the zero-tolerance GPU checks, as far as a host can show it), the alphabets keep the sums where bf16 tells
every integer apart, and one dropped product of a K = 4096 contraction always changes the expected bits -- which the Gaussian
operands with the 6e-3 max-norm criterion of tests/step_launches.OUT_TOL notice for a minority of them (printed)."""
import numpy as np
import pytest
import torch

from palette_and_histo_gan_amd import _lib as L
from tests import lattice as LT
from tests import step_launches as SL

BF, F = L.BF16, L.F32
K_CLASSES = [64, LT.max_k(0), LT.max_k(0) + 1, LT.max_k(1), LT.max_k(1) + 1, LT.max_k(2), 16384]


def test_alphabet_bounds():
    """3 sigma <= 256 up to max_k(k) and not beyond; f32 outputs always draw from the widest alphabet"""
    for k in range(len(LT.ALPHABETS)):
        assert 3 * LT.sigma(LT.max_k(k), k) <= 256 < 3 * LT.sigma(LT.max_k(k) + 1, k), k
        assert LT.alphabet_index(LT.max_k(k), True) == k
        assert LT.alphabet_index(LT.max_k(k) + 1, True) == min(k + 1, len(LT.ALPHABETS) - 1)
        assert LT.alphabet_index(LT.max_k(k) + 1, False) == 0
    print("\n  longest K per alphabet pair:", [LT.max_k(k) for k in range(len(LT.ALPHABETS))])
    with pytest.raises(AssertionError):
        LT.operands(np.random.default_rng(0), (4,), "x", 2 ** 21, F, False)        # 2^21 * 9 >= 2^24


@pytest.mark.parametrize("K", K_CLASSES)
def test_every_value_survives_bf16(K):
    rng = np.random.default_rng(K)
    steps = set()
    for seed in range(12):
        for role in ("x", "w"):
            for out_bf16 in (True, False):
                v, step = LT.operands(rng, (50, 7), role, K, BF, out_bf16)
                steps.add((role, step))
                assert v.dtype == np.float32
                assert np.array_equal(torch.as_tensor(v).to(torch.bfloat16).float().numpy(), v)
                assert np.array_equal(SL.bf16_round(v), v)
                ints = LT.to_int(v, step)
                xs, ws = LT.ALPHABETS[LT.alphabet_index(K, out_bf16)]
                assert set(np.unique(ints)) <= set(xs if role == "x" else ws)
                if role == "x":
                    assert (ints != 0).all()                      # a dropped term cannot hide behind a zero activation
        o = LT.other_channels(rng, (5, 3), 8.0)
        assert np.array_equal(SL.bf16_round(o), o) and set(np.unique(np.abs(o))) == {512.0}
    assert len({s for r, s in steps if r == "x"}) > 1 and len({s for r, s in steps if r == "w"}) > 2        # the exponent varies


def _three_orders(terms):
    """terms [M, K] (float32 products) summed in f32: forward, reversed, and in blocks of 32 with the partials summed last"""
    M, K = terms.shape
    fwd, rev = np.zeros(M, np.float32), np.zeros(M, np.float32)
    for k in range(K):
        fwd = fwd + terms[:, k]
        rev = rev + terms[:, K - 1 - k]
    pad = (-K) % 32
    t = np.concatenate([terms, np.zeros((M, pad), np.float32)], axis=1).reshape(M, -1, 32)
    part = np.zeros(t.shape[:2], np.float32)
    for k in range(32):
        part = part + t[:, :, k]
    blk = np.zeros(M, np.float32)
    for b in range(part.shape[1]):
        blk = blk + part[:, b]
    assert fwd.dtype == rev.dtype == blk.dtype == np.float32
    return fwd, rev, blk


def _products(a, b):
    """elementwise products in f32, asserted exact"""
    p = a.astype(np.float32) * b.astype(np.float32)
    assert np.array_equal(p.astype(np.float64), a.astype(np.float64) * b.astype(np.float64))
    return p


def _terms_g(hi, w, s):
    n, H, W_, cg = hi.shape
    lh, lw, cd = H // s, W_ // s, w.shape[3]
    hp = np.pad(hi, ((0, 0), (1, 2), (1, 2), (0, 0)))
    t = [_products(hp[:, kh:kh + s * lh:s, kw:kw + s * lw:s, :, None], w[kh, kw][None, None, None]) for kh in range(4) for kw in range(4)]
    return np.stack(t, axis=-1).transpose(0, 1, 2, 4, 3, 5).reshape(n * lh * lw * cd, cg * 16)       # [n,y,x,d | g,tap]


def _terms_p(lo, w, s):
    n, lh, lw, cd = lo.shape
    cg = w.shape[2]
    t = np.zeros((n, s * lh + 3, s * lw + 3, cg, 16, cd), np.float32)
    for kh in range(4):
        for kw in range(4):
            t[:, kh:kh + s * lh:s, kw:kw + s * lw:s, :, 4 * kh + kw, :] = _products(lo[:, :, :, None, :], w[kh, kw][None, None, None])
    return t[:, 1:1 + s * lh, 1:1 + s * lw].reshape(n * s * lh * s * lw * cg, 16 * cd)


def _terms_w(hi, lo, s):
    n, lh, lw, cd = lo.shape
    cg = hi.shape[3]
    hp = np.pad(hi, ((0, 0), (1, 2), (1, 2), (0, 0)))
    t = [_products(hp[:, kh:kh + s * lh:s, kw:kw + s * lw:s, :, None], lo[:, :, :, None, :]) for kh in range(4) for kw in range(4)]
    return np.stack(t, axis=0).reshape(16, n * lh * lw, cg * cd).transpose(0, 2, 1).reshape(16 * cg * cd, n * lh * lw)


@pytest.mark.parametrize("dtype,out_bf16", [(BF, True), (BF, False), (F, False)])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_f32_accumulation_is_exact_in_any_order(seed, dtype, out_bf16):
    """seeded launches of op G, op P (both strides) and op W: the f32 sum of the products, forward, reversed and blocked by 32,
    is the float64 result of step_launches.conv_* bit for bit"""
    rng = np.random.default_rng([seed, int(out_bf16), dtype])
    for s, n, lh, cg, cd in ((2, 2, 4, 24, 5), (1, 3, 3, 9, 4)):
        Kg, Kp, Kw = 16 * cg, (4 if s == 2 else 16) * cd, n * lh * lh
        hi, _ = LT.operands(rng, (n, s * lh, s * lh, cg), "x", max(Kg, Kw), dtype, out_bf16)
        lo, _ = LT.operands(rng, (n, lh, lh, cd), "x", max(Kp, Kw), dtype, out_bf16)
        w, _ = LT.operands(rng, (4, 4, cg, cd), "w", max(Kg, Kp), dtype, out_bf16)
        for terms, ref in ((_terms_g(hi, w, s), SL.conv_g(hi, w, s)), (_terms_p(lo, w, s), SL.conv_p(lo, w, s)),
                           (_terms_w(hi, lo, s), SL.conv_w(hi, lo, s))):
            ref = ref.reshape(-1)
            assert terms.shape[0] == ref.size
            assert np.abs(ref).max() > 0
            for got in _three_orders(terms):
                assert np.array_equal(got.astype(np.float64), ref)
            assert np.array_equal(LT.expected(ref, F), ref.astype(np.float32))


def _sums(rng, K, M=512, D=8):
    """integer sums of M * D outputs of a length-K contraction on lattice operands for a bf16 output"""
    x, sx = LT.operands(rng, (M, K), "x", K, BF, True)
    w, sw = LT.operands(rng, (K, D), "w", K, BF, True)
    return LT.to_int(x.astype(np.float64) @ w.astype(np.float64), sx * sw)


@pytest.mark.parametrize("k", range(len(LT.ALPHABETS)))
def test_sums_stay_where_bf16_tells_integers_apart(k):
    K = LT.max_k(k)
    share = LT.sensitive_share(_sums(np.random.default_rng(K), K))
    print(f"\n  alphabet pair {k} at its longest K = {K}: sensitive share {share:.4f}")
    assert share >= 0.99


def test_expected_epilogue():
    """bias, LeakyReLU, ReLU and the act-backward gate in f32, then one rounding (two for the gate: it acts on the stored value)"""
    s = np.array([-300.0, -255.0, -3.0, 0.0, 2.0, 257.0, 300.0])
    a = float(np.float32(0.3))
    assert np.array_equal(LT.expected(s, F), s.astype(np.float32))
    assert np.array_equal(LT.expected(s, BF), np.array([-300, -255, -3, 0, 2, 256, 300], np.float32))
    want = np.where(s + 1 > 0, s + 1, np.float32(a) * (s + 1).astype(np.float32)).astype(np.float32)
    assert np.array_equal(LT.expected(s, F, bias=np.float32(1.0), act=L.ACT_LEAKY, alpha=a), want)
    assert np.array_equal(LT.expected(s, BF, bias=np.float32(1.0), act=L.ACT_LEAKY, alpha=a), SL.bf16_round(want))
    assert np.array_equal(LT.expected(s, F, act=L.ACT_RELU), np.maximum(s, 0).astype(np.float32))
    gate = np.array([1.0, -1.0, 1.0, -1.0, -1.0, -1.0, 1.0])
    g = LT.expected(s, BF, alpha=a, gate=gate)
    assert np.array_equal(g, SL.bf16_round(SL.bf16_round(s.astype(np.float32)) * np.where(gate > 0, np.float32(1), np.float32(a))))
    assert LT.describe_mismatches(g, g, 1.0, ("i",)) == ""
    bad = g.copy()
    bad[2] += 2.0
    assert "1 of 7" in LT.describe_mismatches(bad, g, 0.5, ("i",)) and "(i 2: +4)" in LT.describe_mismatches(bad, g, 0.5, ("i",))
    bad[3] = np.nan
    assert len(LT.mismatches(bad, g)) == 2 and len(LT.mismatches(-g, g)) == 6           # (-0 == +0)


def test_one_dropped_product_always_changes_the_bits():
    """op G, K = 4096 (256 input channels), bf16 output: one non-zero product removed from each of 1000 seeded outputs.  The
    expected bits change at every output whose sum is within +-256 (but for a clean +-256 moved to +-257, a tie that rounds back:
    counted and printed).  For the record, the same perturbation on Gaussian operands under the 6e-3 max-norm criterion."""
    K, M = 4096, 1000
    rng = np.random.default_rng(4096)
    x, sx = LT.operands(rng, (M, K), "x", K, BF, True)
    w, sw = LT.operands(rng, (K,), "w", K, BF, True)
    step = sx * sw
    prod = x.astype(np.float64) * w.astype(np.float64)
    clean = prod.sum(axis=1)
    drop = np.array([rng.choice(np.flatnonzero(prod[i])) for i in range(M)])
    broken = clean - prod[np.arange(M), drop]
    ci, bi = LT.to_int(clean, step), LT.to_int(broken, step)
    assert (ci != bi).all()
    inside = np.abs(ci) <= LT.SENSITIVE
    tie = inside & (np.abs(ci) == 256) & (np.abs(bi) == 257)
    changed = LT.expected(clean, BF) != LT.expected(broken, BF)
    assert changed[inside & ~tie].all()
    # the Gaussian operands of _conv_family, one image of M outputs: max |error| / max |reference| >= 6e-3 ?
    gx = SL.bf16_round(rng.normal(size=(M, K)).astype(np.float32)).astype(np.float64)
    gw = SL.bf16_round(rng.normal(scale=1.0 / np.sqrt(K), size=K).astype(np.float32)).astype(np.float64)
    gp = gx * gw
    ref = gp.sum(axis=1)
    got = SL.bf16_round((ref - gp[np.arange(M), drop]).astype(np.float32)).astype(np.float64)
    rounding = np.abs(SL.bf16_round(ref.astype(np.float32)) - ref).max() / np.abs(ref).max()
    flagged = np.abs(got - ref) / np.abs(ref).max() >= SL.OUT_TOL[BF]
    print(f"\n  K = {K}, {M} outputs, one product dropped from each: lattice {int(changed.sum())} of {M} detected "
          f"({int(inside.sum())} within +-256, all of them detected, {int(tie.sum())} ties at 256 | 257; share within +-256 "
          f"{LT.sensitive_share(ci):.4f}); Gaussian operands, 6e-3 of the maximum: {int(flagged.sum())} of {M} detected "
          f"(clean bf16 rounding alone uses {rounding / SL.OUT_TOL[BF]:.0%} of the tolerance)")
    assert LT.sensitive_share(ci) >= 0.99
