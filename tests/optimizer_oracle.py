"""NumPy restatements of the optimizer options for tests/test_optimizer_cpu.py and tests/test_optimizer_gpu.py:
the learning-rate schedules in float64 (the host side of palette_and_histo_gan_amd/schedules.py), the global gradient norm in
float32 in the documented order of p2p_sumsq_partials / p2p_clip_scale (include/p2pgan.h), the clip scale, and the clipped Adam
element in float32 with every rounding spelled out (csrc/optim.hip adam_update, no contraction).
"""
import math

import numpy as np

from palette_and_histo_gan_amd import schedules as SCH

F32, F64 = np.float32, np.float64
MAX_PARTS, BLOCK, WAVE = 1024, 256, 64          # P2P_SUMSQ_MAX_PARTS, threads per workgroup, lanes per wave


# ---------------------------------------------------------------------------------------------------------------- schedules
def lr_t(schedule, t, b1, b2):
    """the step size p2p_adam_tick[_sched] leaves in lr_t_dev after the increment to t: the schedule at t - 1 (Keras evaluates it
    at `iterations` before the increment) times the bias correction, in float64, rounded once to float32.  schedule: a float or
    a schedule object (a float reaches the kernel as a float32, a schedule's numbers as float64); b1, b2: rounded to float32 as
    the kernel receives them."""
    lr = float(F32(schedule)) if isinstance(schedule, (int, float, F32)) else SCH.as_schedule(schedule)[0](t - 1)
    b1, b2 = float(F32(b1)), float(F32(b2))
    return F32(lr * math.sqrt(1.0 - math.pow(b2, t)) / (1.0 - math.pow(b1, t)))


def ulps(a, b):
    """distance of two float32 values in units in the last place (same sign, finite)"""
    ia, ib = (int(np.asarray(x, F32).view(np.int32)) for x in (a, b))
    return abs(ia - ib)


# ---------------------------------------------------------------------------------------------------------------- global norm
def sumsq_grid(n):
    """(whole vectors V, workgroups NB, sweeps of the grid-stride loop) of p2p_sumsq_partials for n elements"""
    V = n // 4
    NB = min(max(-(-V // BLOCK), 1), MAX_PARTS)
    return V, NB, -(-V // (NB * BLOCK))


def wave_tree(a):
    """the wave tree over the last axis (64 lanes): for off = 32 .. 1, lane l += lane l + off; lane 0's value"""
    a = np.array(a, F32)
    off = WAVE // 2
    while off:
        a = a[..., :off] + a[..., off:2 * off]
        off //= 2
    return a[..., 0]


def sumsq_partials(g, ex_lo=0, ex_hi=0):
    """float32 partials [NB] of p2p_sumsq_partials: thread q walks the vectors q, q + 256 NB, ... and their components in order
    with one accumulator (acc = acc + g * g, both rounded), thread 0 adds the n % 4 tail, wave tree, ((w0 + w1) + w2) + w3"""
    g = np.array(g, F32).reshape(-1)
    n = g.size
    g[ex_lo:ex_hi] = 0.0
    V, NB, sweeps = sumsq_grid(n)
    T = NB * BLOCK
    with np.errstate(over="ignore", invalid="ignore"):
        sq = np.zeros(max(sweeps, 1) * T * 4, F32)
        sq[:V * 4] = g[:V * 4] * g[:V * 4]
        sq = sq.reshape(max(sweeps, 1), T, 4)
        acc = np.zeros(T, F32)
        for s in range(sweeps):
            for k in range(4):
                acc = acc + sq[s, :, k]
        for j in range(V * 4, n):
            acc[0] = acc[0] + g[j] * g[j]
        w = wave_tree(acc.reshape(NB, BLOCK // WAVE, WAVE))
        return ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]


def global_sumsq(partials_list):
    """float32 sum of p2p_clip_scale: the partials of every buffer concatenated, lane l sums the entries l, l + 64, ... in rising
    order, wave tree"""
    c = np.concatenate([np.asarray(p, F32).reshape(-1) for p in partials_list])
    rows = -(-c.size // WAVE)
    padded = np.zeros(rows * WAVE, F32)
    padded[:c.size] = c
    acc = np.zeros(WAVE, F32)
    with np.errstate(over="ignore", invalid="ignore"):
        for r in padded.reshape(rows, WAVE):
            acc = acc + r
        return wave_tree(acc)


def global_norm(partials_list):
    """float32 norm of p2p_clip_scale: the square root of global_sumsq, correctly rounded"""
    with np.errstate(invalid="ignore"):
        return np.sqrt(global_sumsq(partials_list))


def clip_scale(norm, clipnorm):
    """float32: clipnorm / norm above the threshold, exactly 1 at and below it, NaN for a non-finite norm"""
    norm, clipnorm = F32(norm), F32(clipnorm)
    if not np.isfinite(norm):
        return F32(np.nan)
    return clipnorm / norm if norm > clipnorm else F32(1.0)


def sumsq_error_bound(n, nbuf=1):
    """relative bound of the float32 sum of squares against the exact one: every square is rounded once and then passes through
    at most (longest serial chain + tree depth) rounded additions of non-negative terms, each within 2^-24 relative.
    chain: 4 per sweep and the tail in a thread, then the lane's share of the partials; tree: 6 levels of the wave tree, the 3
    additions over a workgroup's waves, 6 levels of the final tree.  (+ 2: the square's own rounding and the usual slack of the
    first-order bound.)"""
    V, NB, sweeps = sumsq_grid(n)
    chain = 4 * sweeps + n % 4 + -(-NB * nbuf // WAVE)
    depth = 6 + 3 + 6
    return chain, depth, (chain + depth + 2) * 2.0 ** -24


# ---------------------------------------------------------------------------------------------------------------- Adam element
def fma32(a, b, c):
    """float32 fused multiply-add with ONE rounding: the product is exact in float64, the float64 sum is rounded to odd (TwoSum
    gives the sign of what the sum lost), and the final rounding to float32 is then the rounding of the exact value"""
    a, b, c = (np.asarray(x, F32).astype(F64) for x in (a, b, c))
    with np.errstate(over="ignore", invalid="ignore"):
        p = a * b
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
        other = np.nextafter(s, np.where(err > 0, np.inf, -np.inf))
        even = (s.view(np.int64) & 1) == 0
        s = np.where((err != 0) & even & np.isfinite(s), other, s)
        return s.astype(F32)


def adam_element(p, g, m, v, lr_t, b1, b2, eps, gscale=1.0, clipvalue=0.0):
    """(p', m', v') of csrc/optim.hip adam_update behind p2p_adam_step's gradient options, float32 throughout:
    g = fmin(fmax(g, -c), c) where c > 0; gg = g * gscale; m' = fma(1 - b1, gg, b1 * m); v' = fma(b2, v, ((1 - b2) * gg) * gg);
    p' = p - (lr_t * m') / (sqrt(v') + eps)"""
    p, g, m, v = (np.asarray(x, F32) for x in (p, g, m, v))
    lr_t, b1, b2, eps, gscale, c = (F32(x) for x in (lr_t, b1, b2, eps, gscale, clipvalue))
    with np.errstate(over="ignore", invalid="ignore", divide="ignore", under="ignore"):
        if c > 0:
            g = np.fmin(np.fmax(g, -c), c)
        gg = g * gscale
        m1 = fma32(F32(1.0) - b1, gg, b1 * m)
        v1 = fma32(b2, v, ((F32(1.0) - b2) * gg) * gg)
        p1 = p - (lr_t * m1) / (np.sqrt(v1) + eps)
    return p1, m1, v1


def adam_flat(p, g, m, v, lr_t, b1, b2, eps, gscale=1.0, clipvalue=0.0, hole=None, chunk=1 << 22):
    """adam_element over flat buffers in chunks (float64 temporaries of fma32), the elements of `hole` left alone"""
    out = [np.array(x, F32) for x in (p, m, v)]
    for lo in range(0, out[0].size, chunk):
        sl = slice(lo, min(lo + chunk, out[0].size))
        p1, m1, v1 = adam_element(out[0][sl], np.asarray(g, F32)[sl], out[1][sl], out[2][sl], lr_t, b1, b2, eps, gscale, clipvalue)
        out[0][sl], out[1][sl], out[2][sl] = p1, m1, v1
    if hole is not None and hole[1] > hole[0]:
        for o, x in zip(out, (p, m, v)):
            o[hole[0]:hole[1]] = np.asarray(x, F32)[hole[0]:hole[1]]
    return out[0], out[1], out[2]


def ema_element(e, p, t, decay, warmup):
    """csrc/optim.hip ema_update: e + (1 - beta_t) * (p - e), beta_t = warmup ? min(decay, (1 + t) / (10 + t)) : decay"""
    beta = F32(decay)
    if warmup:
        beta = min(beta, (F32(1.0) + F32(t)) / (F32(10.0) + F32(t)))
    omb = F32(1.0) - beta
    e, p = np.asarray(e, F32), np.asarray(p, F32)
    return e + omb * (p - e)
