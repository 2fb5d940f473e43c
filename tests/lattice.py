"""Integer-lattice operands for the contraction kernels: inputs on which a launch's result is known bit for bit.  Host only.

Every contraction kernel multiplies activation-dtype values and accumulates in f32 (mfma_f32_32x32x16_bf16 / 32x32x2f32, plain FMAs
in conv_direct.hip).  With operands that are small integers times a power of two
- every product is an integer times the LATTICE STEP (the product of the two tensors' powers of two), exact in f32;
- every partial sum of a contraction is an integer below 2^24 times that step, so the f32 accumulator is exact in ANY summation
  order, split-K, msplit or tile shape;
- the stored result is the exact sum in f32, and its round-to-nearest-even (step_launches.bf16_round) in bf16.
No tolerance is involved, and every route of a layer is comparable with every other through the reference.  bfloat16 has 8
significant bits: every integer in [-256, 256] is a bf16 value of its own, so while the integer sum stays in that range one wrong,
lost or foreign term always changes the stored bits (the one exception is a clean +-256 that a wrong term moves to +-257, which
ties back to +-256).  The alphabets are chosen from the contraction length so that three standard deviations of the sum stay
within 256 (sensitive_share measures what a case really gets).

The exact sums come from step_launches.conv_g / conv_p / conv_w: float64, exact on these values.
"""
import numpy as np

from palette_and_histo_gan_amd import _lib as L
from tests import step_launches as SL

# (activation alphabet, weight alphabet), widest first.  Activations are never 0 (a dropped term cannot hide behind a zero
# activation), weights may be.
ALPHABETS = (((-3, -2, -1, 1, 2, 3), (-2, -1, 0, 1, 2)),
             ((-2, -1, 1, 2), (-1, 0, 1)),
             ((-1, 1), (-1, 0, 1)))
SENSITIVE = 256             # |integer| up to which every integer is a bf16 value of its own
ACT_EXP = (0, 3)            # activations: times 2^a, a in 0 .. 3
W_EXP = (0, 6)              # weights: times 2^-b, b in 0 .. 6 (so that the exponent path is not trivially 1.0)
OTHER = 64                  # magnitude (in steps of the tensor) of the channels of a pixel that a launch must not read


def _var(alphabet):
    a = np.asarray(alphabet, np.float64)
    return float((a ** 2).mean() - a.mean() ** 2)


def sigma(K, k):
    """standard deviation of the integer sum of K products of alphabet pair k (independent uniform draws)"""
    return float(np.sqrt(K * _var(ALPHABETS[k][0]) * _var(ALPHABETS[k][1])))


def max_k(k):
    """the longest contraction for which alphabet pair k keeps 3 sigma of the integer sum within SENSITIVE"""
    return int((SENSITIVE / 3.0) ** 2 / (_var(ALPHABETS[k][0]) * _var(ALPHABETS[k][1])))


def alphabet_index(K, out_is_bf16):
    """the widest alphabet pair with 3 sigma <= 256 at contraction length K for a bf16 output (the narrowest one beyond the last
    bound); always the widest one for an f32 output, where the sum only has to stay below 2^24"""
    if not out_is_bf16:
        return 0
    for k in range(len(ALPHABETS)):
        if 3.0 * sigma(K, k) <= SENSITIVE:
            return k
    return len(ALPHABETS) - 1


def operands(rng, shape, role, K, dtype, out_is_bf16):
    """(values, step): float32 values = integers * step, step a power of two drawn per tensor.
    role "x": an activation or a gradient (never 0, step 2^a); role "w": a weight (may be 0, step 2^-b).
    K: the longest contraction length of the launch (op G: 16 * cin; op P: 4 * cd at stride 2, 16 * cd at stride 1; op W:
    N * LH * LW).  out_is_bf16: the launch stores the contraction in bf16 (False: the f32 dtype, every op W, split-K slabs, column
    sums)."""
    assert role in ("x", "w"), role
    k = alphabet_index(K, out_is_bf16)
    xs, ws = ALPHABETS[k]
    # the largest possible |integer sum|: K products of two activations (op W) or of an activation and a weight
    assert K * max(np.abs(xs)) ** 2 < 2 ** 24, f"a sum of {K} products can reach 2^24: the f32 accumulator is no longer exact"
    if role == "x":
        ints = rng.choice(np.asarray(xs, np.int64), size=shape)
        step = 2.0 ** int(rng.integers(ACT_EXP[0], ACT_EXP[1] + 1))
    else:
        ints = rng.choice(np.asarray(ws, np.int64), size=shape)
        step = 2.0 ** -int(rng.integers(W_EXP[0], W_EXP[1] + 1))
    vals = (ints * step).astype(np.float32)
    if dtype == L.BF16:
        assert np.array_equal(SL.bf16_round(vals), vals), "a lattice value is no bf16 value"
    return vals, float(step)


def small_ints(rng, shape, step, lim=3):
    """integers in [-lim, lim] times step, float32: biases, shifts"""
    return (rng.integers(-lim, lim + 1, size=shape) * step).astype(np.float32)


def other_channels(rng, shape, step):
    """+-OTHER * step: what the channels around an input view hold.  A kernel that reads one shows up as a multiple of 64 steps"""
    return (rng.choice(np.asarray((-OTHER, OTHER), np.int64), size=shape) * step).astype(np.float32)


def _round(v, dtype):
    return SL.bf16_round(v) if dtype == L.BF16 else np.asarray(v, np.float32)


def expected(sum_exact, dtype, bias=None, act=0, alpha=0.0, gate=None):
    """The values the kernel must store: the exact sum as f32, plus the bias in f32 (a multiple of the lattice step: exact), the
    activation in f32 -- v > 0 ? v : f32(alpha) * v is one f32 multiply and rounds once, identically on both sides -- then the
    rounding to the dtype.  gate (p2p_conv_fewin_actbwd): the LeakyReLU backward factor (gate > 0 ? 1 : f32(alpha)) is applied to
    the ROUNDED result and the product is rounded again, as p2p_act_bwd applies it to the stored tensor."""
    s64 = np.asarray(sum_exact, np.float64)
    v = s64.astype(np.float32)
    assert np.array_equal(v.astype(np.float64), s64), "the exact sum is no f32 value: not a lattice launch"
    if bias is not None:
        v = v + np.asarray(bias, np.float32)
    if act == L.ACT_LEAKY:
        v = np.where(v > 0, v, np.float32(alpha) * v).astype(np.float32)
    elif act == L.ACT_RELU:
        v = np.maximum(v, np.float32(0.0))
    v = _round(v, dtype)
    if gate is not None:
        v = _round(v * np.where(np.asarray(gate) > 0, np.float32(1.0), np.float32(alpha)).astype(np.float32), dtype)
    return v


def to_int(x, step):
    """values on a lattice -> their integers (asserts that they are on it)"""
    q = np.asarray(x, np.float64) / step
    r = np.rint(q)
    assert np.array_equal(q, r), "a value is no integer multiple of the lattice step"
    return r.astype(np.int64)


def sensitive_share(sum_int):
    """the share of elements whose integer sum lies in [-256, 256], where one wrong term always changes the bf16 bits"""
    s = np.abs(np.asarray(sum_int, np.float64))
    return float((s <= SENSITIVE).mean())


def mismatches(got, want):
    """indices (rows of np.argwhere) of the elements that are not the expected value; +0 and -0 count as equal, a NaN never does"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    return np.argwhere(~(got == want))


def describe_mismatches(got, want, step, names, limit=10):
    """'' when every element is the expected one; else the count and the first `limit` positions with got - want in lattice steps
    (the delta is the lost or foreign term's value, its position says which tap, chunk or strip)"""
    bad = mismatches(got, want)
    if not len(bad):
        return ""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    rows = []
    for idx in bad[:limit]:
        idx = tuple(int(i) for i in idx)
        rows.append("(" + ", ".join(f"{n} {i}" for n, i in zip(names, idx)) + f": {(got[idx] - want[idx]) / step:+g})")
    return f"{len(bad)} of {got.size} elements differ; first (got - want in lattice steps): " + " ".join(rows)
