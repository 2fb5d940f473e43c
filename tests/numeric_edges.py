"""Case builders, float64 references, float32 restatements and bounds of the ill-conditioned-input tests
(tests/test_numeric_edges_cpu.py proves from NumPy that the cases can fail; tests/test_numeric_edges_gpu.py runs the kernels).

A. InstanceNorm.  Every kernel test elsewhere feeds the normalisations mean / std = 0.15, where an unshifted E[x^2] - E[x]^2 passes.
   Here every channel takes one of six regimes (channel mod 6, so one 4- or 8-channel vector always mixes them), the sign of the
   offset alternates between images, and the values are rounded through the activation dtype before any reference sees them:

       regime                          f32                      bf16
       0 control                       mean 0.3, std 2          same
       1 offset                        mean 256, std 1          mean 32, std 1
       2 offset + outlier first pixel  regime 1, x[n,0,0,c] = mean + 8 std   (the shifted forms shift by the first pixel)
       3 variance << eps               mean 100, std 1e-3       mean 1, std 2^-6
       4 constant                      5.1                      same
       5 constant                      200                      same

   Bounds (none of them taken from what a kernel returns):
     mu:  |mu - mean64| <= 2^-22 max|x| of the (image, channel)
     rs:  |rs - rs64| / rs64 <= 2^-22 (4 + k^2),  k = (x0 - mean64) / std64 (0 on a constant channel): the first-order cancellation
          error of sums shifted by x0, with a factor 2 of margin
     out: against act(drop(gamma (x - mu_k) rs_k + beta)) in f64 from the kernel's OWN statistics (the line above established that
          they are right; using them removes the ulp(mean) * rs term no f32 algorithm avoids), OUT_TOL per (image, channel) plane
          relative to the plane's reference, floored at PLANE_FLOOR of the tensor's maximum
     constant channels: |out - act(drop(beta))| <= keep * 4 ulp_f32(|x|) |gamma| / sqrt(eps)  (+ the output rounding in bf16)
B. losses at saturation, C. Adam on degenerate gradients, D. colour-point list edges: builders only, the references are the
   oracle's.
"""
import math

import numpy as np

from oracle import np_restatement as npr
from palette_and_histo_gan_amd import _lib as L
from tests import gpu_util as U
from tests.step_launches import OUT_TOL, act as act_np

EPS = 1e-3
ALPHA = 0.3
REGIMES = {       # (mean, std, outlier of the first pixel in stds)
    L.F32: ((0.3, 2.0, 0.0), (256.0, 1.0, 0.0), (256.0, 1.0, 8.0), (100.0, 1e-3, 0.0), (5.1, 0.0, 0.0), (200.0, 0.0, 0.0)),
    L.BF16: ((0.3, 2.0, 0.0), (32.0, 1.0, 0.0), (32.0, 1.0, 8.0), (1.0, 2.0 ** -6, 0.0), (5.1, 0.0, 0.0), (200.0, 0.0, 0.0)),
}
CONSTANT = (4, 5)
# A plane that ReLU and dropout leave (nearly) empty has no scale of its own.  Its elements still carry the f32 rounding of the
# pre-activation's terms, ~3 * 2^-24 of the tensor's magnitude: against OUT_TOL[f32] = 2e-5 that needs a floor >= 1e-2 of it.
PLANE_FLOOR = 1e-2
KINK = 1e-5            # elements whose pre-activation is within KINK * max|pre-activation| of 0 are left out of the backward checks
KINK_SHARE = 1e-3      # ... at most this share of a tensor
BWD_TOL = {L.F32: 1e-4, L.BF16: 1e-2}     # d(raw), of the max-norm (tests/test_kernels_gpu.py::test_norm_act_fwd_bwd)
PART_TOL = 1e-4                           # dgamma / dbeta


def regime(c):
    return c % 6


# ------------------------------------------------------------------------------------------------------------------ A: cases
class NormCase:
    """One p2p_norm_act_fwd / _bwd launch: n images of h x h x c; nslabs > 0: the forward reads f32 split-K slabs (raw_kind 2);
    slots > 0: the statistics come as conv-epilogue slots (nsplit = -slots); gslabs: the backward's second gradient source is five
    f32 slabs (else a second activation-dtype tensor)."""

    def __init__(self, n, h, c, act, mask, nsplit=1, nslabs=0, slots=0, gslabs=True):
        self.n, self.h, self.c, self.act, self.mask, self.nsplit, self.nslabs, self.slots, self.gslabs = \
            n, h, c, act, mask, nsplit, nslabs, slots, gslabs

    @property
    def id(self):
        s = f"{self.n}x{self.h}x{self.h}x{self.c}"
        if self.nsplit != 1:
            s += f"-ns{self.nsplit:#x}"
        if self.nslabs:
            s += f"-slabs{self.nslabs}"
        if self.slots:
            s += f"-slots{self.slots}"
        return s + ("-g2slabs" if self.gslabs else "-g2dense")


LK, RL = L.ACT_LEAKY, L.ACT_RELU
NORM_CASES = [
    # the lane-group form (<= 16 pixels): exact two-pass sums
    NormCase(2, 2, 8, RL, False, gslabs=False), NormCase(2, 4, 64, LK, False), NormCase(3, 3, 16, LK, True),
    NormCase(2, 4, 64, LK, False, nslabs=16, gslabs=False), NormCase(3, 2, 256, RL, True, nslabs=7),
    # the register-resident form at 1, 2, 4, 8 pixels per thread, dense and slab-fed
    NormCase(3, 8, 32, RL, True), NormCase(3, 8, 32, RL, True, gslabs=False),
    NormCase(2, 16, 128, RL, False, nsplit=0x202), NormCase(2, 16, 128, RL, False, nsplit=0x202, gslabs=False),
    NormCase(2, 32, 64, LK, False, nsplit=0x204), NormCase(2, 32, 64, LK, False, nsplit=0x204, gslabs=False),
    NormCase(3, 8, 256, RL, True, nsplit=0x201), NormCase(3, 8, 256, RL, True, nsplit=0x201, gslabs=False),
    NormCase(2, 8, 256, LK, False, nslabs=5), NormCase(3, 16, 128, LK, True, nslabs=4), NormCase(2, 32, 64, LK, False, nslabs=2),
    NormCase(2, 16, 128, LK, False, nsplit=0x202, nslabs=3), NormCase(2, 32, 64, RL, False, nsplit=0x204, nslabs=3),
    NormCase(3, 8, 256, LK, True, nsplit=0x201, nslabs=3),
    # the workgroup forms: one pass, statistics pass + apply pass over a pixel split, both also slab-fed
    NormCase(2, 16, 128, RL, False, nsplit=0x102), NormCase(2, 16, 128, RL, False, nsplit=0x101, gslabs=False),
    NormCase(2, 64, 32, LK, False, nsplit=4), NormCase(2, 64, 32, LK, False, nsplit=4, nslabs=3),
    # apply-only over statistics slots (the slots are made from the same input, see slot_partials)
    NormCase(2, 8, 32, RL, True, slots=4), NormCase(2, 16, 64, LK, False, slots=8), NormCase(2, 64, 32, RL, False, slots=16),
]
DTYPES = (L.F32, L.BF16)


def norm_input(case, dtype, seed=41):
    """(x, gamma, beta, mask): x [n,h,h,c] rounded through dtype (float32 array); |beta| >= 0.05 on the constant channels"""
    rng = np.random.default_rng([seed, case.n, case.h, case.c, dtype])
    n, h, c = case.n, case.h, case.c
    xi = rng.normal(size=(n, h, h, c))
    x = np.empty((n, h, h, c))
    for ch in range(c):
        mean, std, outlier = REGIMES[dtype][regime(ch)]
        for i in range(n):
            m = mean if i % 2 == 0 else -mean
            x[i, :, :, ch] = m + std * xi[i, :, :, ch]
            if outlier:
                x[i, 0, 0, ch] = m + outlier * std
    gamma = (1 + 0.2 * rng.normal(size=c)).astype(np.float32)
    beta = (0.2 * rng.normal(size=c)).astype(np.float32)
    small = np.abs(beta) < 0.05
    beta[small] = np.where(beta[small] < 0, -0.05, 0.05).astype(np.float32)
    mask = rng.integers(0, 2, size=(n, h, h, c)).astype(np.uint8) if case.mask else None
    return U.q(x, dtype), gamma, beta, mask


def grad_sources(case, dtype, seed=43):
    """(dy1 [n,h,h,c+8] in dtype: the source sits behind 8 other channels, dy2): dy2 = five f32 slabs [5,n,h,h,c] or one more
    tensor in dtype [n,h,h,c]"""
    rng = np.random.default_rng([seed, case.n, case.h, case.c, dtype])
    n, h, c = case.n, case.h, case.c
    dy1 = U.q(rng.normal(size=(n, h, h, c + 8)), dtype)
    dy2 = rng.normal(size=(5, n, h, h, c)).astype(np.float32) if case.gslabs else U.q(rng.normal(size=(n, h, h, c)), dtype)
    return dy1, dy2


def pow2_slabs(x, nslabs):
    """f32 slabs that are exact power-of-two fractions of x, smallest first (2^-(k-1), 2^-(k-1), 2^-(k-2), ... 1/2): every partial
    sum in slab order is a power-of-two multiple of x, so the f32 sum is x bit for bit"""
    x = np.asarray(x, np.float32)
    if nslabs == 1:
        return x[None].copy()
    f = [2.0 ** -(nslabs - 1)] + [2.0 ** -(nslabs - 1 - max(k - 1, 0)) for k in range(1, nslabs)]
    assert abs(sum(f) - 1.0) == 0.0
    return np.stack([x * np.float32(v) for v in f])


def slot_partials(x, slots):
    """what a conv epilogue leaves for x [n,h,h,c]: (mean, centred sum of squares) of `slots` equal groups of consecutive pixels,
    f32 [n,slots,c,2], computed in f64 (the pooled result does not depend on which pixels share a slot)"""
    n, h, _, c = x.shape
    g = np.asarray(x, np.float64).reshape(n, slots, h * h // slots, c)
    mean = g.mean(axis=2)
    m2 = ((g - mean[:, :, None, :]) ** 2).sum(axis=2)
    return np.stack([mean, m2], axis=-1).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------------ A: references
def stats64(x):
    """per (image, channel) in f64: mean, rs = 1 / sqrt(var + eps), k = (x0 - mean) / std (0 where the channel is constant)"""
    x = np.asarray(x, np.float64)
    mean = x.mean(axis=(1, 2))
    var = ((x - mean[:, None, None, :]) ** 2).mean(axis=(1, 2))
    std = np.sqrt(var)
    k = np.divide(x[:, 0, 0, :] - mean, std, out=np.zeros_like(mean), where=std > 0)
    return mean, 1.0 / np.sqrt(var + EPS), k


def mu_bound(x):
    return 2.0 ** -22 * np.abs(np.asarray(x, np.float64)).max(axis=(1, 2))


def rs_bound(k):
    return 2.0 ** -22 * (4.0 + k * k)


def stat_errors(mu, rs, x):
    """(mu error / its bound, relative rs error / its bound), each [n, c]"""
    mean, rs64, k = stats64(x)
    e_mu = np.abs(np.asarray(mu, np.float64) - mean) / mu_bound(x)
    e_rs = np.abs(np.asarray(rs, np.float64) - rs64) / rs64 / rs_bound(k)
    return e_mu, e_rs


def pre_activation(x, mu, rs, gamma, beta):
    x, mu, rs = (np.asarray(v, np.float64) for v in (x, mu, rs))
    return (x - mu[:, None, None, :]) * rs[:, None, None, :] * np.asarray(gamma, np.float64) + np.asarray(beta, np.float64)


def apply64(x, mu, rs, gamma, beta, act, mask):
    """act(drop(gamma (x - mu) rs + beta)) in f64 from the given statistics [n, c]"""
    y = pre_activation(x, mu, rs, gamma, beta)
    if mask is not None:
        y = y * mask * 2.0
    return act_np(y, act, ALPHA)


def plane_err(got, ref):
    """max over (image, channel) planes of max|got - ref| / max(max|ref| of the plane, PLANE_FLOOR * max|ref| of the tensor)"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    scale = np.maximum(np.abs(ref).max(axis=(1, 2)), PLANE_FLOOR * np.abs(ref).max())
    return float((np.abs(got - ref).max(axis=(1, 2)) / scale).max())


def ulp32(v):
    return np.spacing(np.abs(np.asarray(v, np.float32))).astype(np.float64)


def constant_out_bound(x, gamma, beta, act, mask, dtype):
    """[n,h,h,c]: the bound on |out - act(drop(beta))| (meaningful on the constant channels).  The dropout keep factor 2 scales the
    deviation with the value; a bf16 output adds its own rounding, half an ulp (at most 2^-8) of a value within the bound of the reference."""
    keep = 2.0 if mask is not None else 1.0
    b = keep * 4.0 * ulp32(x) * np.abs(np.asarray(gamma, np.float64)) / math.sqrt(EPS)
    if dtype == L.BF16:
        ref = np.abs(constant_ref(x, beta, act, mask))
        b = b + 2.0 ** -8 * (ref + b)
    return b


def constant_ref(x, beta, act, mask):
    y = np.broadcast_to(np.asarray(beta, np.float64), np.shape(x)).copy()
    if mask is not None:
        y = y * mask * 2.0
    return act_np(y, act, ALPHA)


def backward64(x, mu, rs, gamma, beta, act, mask, dy):
    """closed form of np_restatement.instance_norm_backward behind dropout and the activation, in f64, from the given statistics
    [n, c] -> (d(raw) [n,h,h,c], dgamma [c], dbeta [c], kink [n,h,h,c] bool: elements whose activation gate is undecided)"""
    x, mu, rs, dy = (np.asarray(v, np.float64) for v in (x, mu, rs, dy))
    gamma = np.asarray(gamma, np.float64)
    xh = (x - mu[:, None, None, :]) * rs[:, None, None, :]
    pre = xh * gamma + np.asarray(beta, np.float64)
    keep = mask * 2.0 if mask is not None else 1.0
    a = pre * keep
    slope = np.where(a > 0, 1.0, ALPHA if act == L.ACT_LEAKY else 0.0)
    d = dy * slope * keep
    dbeta, dgamma = d.sum(axis=(0, 1, 2)), (d * xh).sum(axis=(0, 1, 2))
    m1, m2 = d.mean(axis=(1, 2), keepdims=True), (d * xh).mean(axis=(1, 2), keepdims=True)
    dx = gamma * rs[:, None, None, :] * (d - m1 - xh * m2)
    kink = (np.abs(pre) <= KINK * np.abs(pre).max()) & (np.asarray(keep) > 0)
    return dx, dgamma, dbeta, kink


# ------------------------------------------------------------------------------------------------------------------ A: float32 restatements
def _f32(x):
    return np.asarray(x, np.float32)


def _tree_sum(a):
    """float32 sum over the pixels of a [n,h,w,c] by a balanced binary tree (zero-padded to a power of two): the order of a wave's
    butterfly, and of a workgroup's tree reduction over per-lane partial sums"""
    a = _f32(a).reshape(a.shape[0], -1, a.shape[-1])
    size = 1
    while size < a.shape[1]:
        size *= 2
    a = np.concatenate([a, np.zeros((a.shape[0], size - a.shape[1], a.shape[2]), np.float32)], axis=1)
    while a.shape[1] > 1:
        a = a[:, 0::2] + a[:, 1::2]
    return a[:, 0]


def two_pass_f32(x):
    """(mu, rs) [n, c] by exact two-pass sums, every operation float32"""
    x = _f32(x)
    hw = np.float32(x.shape[1] * x.shape[2])
    mu = _tree_sum(x) / hw
    d = x - mu[:, None, None, :]
    var = _tree_sum(d * d) / hw
    return mu, np.float32(1) / np.sqrt(var + np.float32(EPS))


def shifted_f32(x, clamp=True):
    """sums shifted by the first pixel, var = max(t2 / HW - m^2, 0) (the register-resident and workgroup forms)"""
    x = _f32(x)
    hw = np.float32(x.shape[1] * x.shape[2])
    sh = x[:, 0, 0, :]
    d = x - sh[:, None, None, :]
    m = _tree_sum(d) / hw
    var = _tree_sum(d * d) / hw - m * m
    if clamp:
        var = np.maximum(var, np.float32(0))
    return sh + m, np.float32(1) / np.sqrt(var + np.float32(EPS))


def plain_f32(x):
    """unshifted E[x^2] - E[x]^2: what the bounds must catch"""
    x = _f32(x)
    hw = np.float32(x.shape[1] * x.shape[2])
    m = _tree_sum(x) / hw
    var = np.maximum(_tree_sum(x * x) / hw - m * m, np.float32(0))
    return m, np.float32(1) / np.sqrt(var + np.float32(EPS))


def pooled64(sp, hw):
    """(mean, rs) [n, c] the slot partials [n,slots,c,2] AS STORED (f32) describe, pooled in f64: what the apply-only form is asked to
    reproduce.  (An f32 slot mean carries half an ulp of the mean; at mean / std = 256 that alone moves rs by about the whole rs
    bound against the data's own moments, whatever pools the slots.)"""
    sp = np.asarray(sp, np.float64)
    slots = sp.shape[1]
    mall = sp[..., 0].mean(axis=1)
    m2 = sp[..., 1].sum(axis=1) + (hw / slots) * ((sp[..., 0] - mall[:, None, :]) ** 2).sum(axis=1)
    return mall, 1.0 / np.sqrt(m2 / hw + EPS)


def given_stat_errors(mu, rs, mean, rs64, x):
    """stat_errors against given f64 statistics (k = 0: no shift to be far from)"""
    e_mu = np.abs(np.asarray(mu, np.float64) - mean) / mu_bound(x)
    e_rs = np.abs(np.asarray(rs, np.float64) - rs64) / rs64 / rs_bound(0.0)
    return e_mu, e_rs


def pooled_f32(sp, hw, cross_term=True):
    """the parallel-variance pooling of slot partials [n,slots,c,2] in float32 (cross_term False: the cnt (mi - mall)^2 term dropped)"""
    sp = _f32(sp)
    slots = sp.shape[1]
    mall = sp[..., 0].sum(axis=1, dtype=np.float32) / np.float32(slots)
    cnt = np.float32(hw / slots)
    m2 = sp[..., 1].sum(axis=1, dtype=np.float32)
    if cross_term:
        dm = sp[..., 0] - mall[:, None, :]
        m2 = m2 + (cnt * dm * dm).sum(axis=1, dtype=np.float32)
    return mall, np.float32(1) / np.sqrt(m2 / np.float32(hw) + np.float32(EPS))


def apply_f32(x, mu, rs, gamma, beta, act, mask):
    x, mu, rs = _f32(x), _f32(mu), _f32(rs)
    y = (x - mu[:, None, None, :]) * rs[:, None, None, :] * _f32(gamma) + _f32(beta)
    if mask is not None:
        y = y * (mask.astype(np.float32) * np.float32(2))
    return act_np(y, act, np.float32(ALPHA))


# ------------------------------------------------------------------------------------------------------------------ A: routes
_FAKE = 1 << 20


def norm_routes(case, dtype):
    """(forward arm, backward arm) of the case: the launchers' own decision functions, nothing started (needs no GPU)"""
    import ctypes as C
    lib = L.lib()
    n, h, c = case.n, case.h, case.c
    p = C.c_void_p(_FAKE)
    out = L.Tensor(_FAKE, (h + 4) * (h + 4), h + 4, c + 8)
    ws_bytes = n * 16 * c * 2 * 4
    nsplit = -case.slots if case.slots else case.nsplit
    fwd = lib.p2p_norm_act_fwd_route(dtype, n, h, h, c, p, 2 if case.nslabs else 1, max(case.nslabs, 1), n * h * h * c, p, p, C.byref(out),
                                     p if case.nslabs else None, p, p, ws_bytes, nsplit, None, 0)
    g1 = L.GSrc(_FAKE, 1, 1, 0, c + 8, 8)
    g2 = L.GSrc(_FAKE, 2, 5, n * h * h * c, c, 0) if case.gslabs else L.GSrc(_FAKE, 1, 1, 0, c, 0)
    draw = L.Tensor(_FAKE, (h + 4) * (h + 4), h + 4, c)
    bwd = lib.p2p_norm_act_bwd_route(dtype, n, h, h, c, p, p, p, p, C.byref(g1), C.byref(g2), C.byref(draw), p, p, p, ws_bytes,
                                     case.nsplit)
    assert fwd >= 0 and bwd >= 0, (case.id, fwd, bwd)
    return fwd & 0xff, bwd & 0xff


def statistics_arms():
    """every arm of P2P_NORM_FWD_ARMS / P2P_NORM_BWD_ARMS but the scalar kernel (C % 8 != 0: no layer of the networks) and those
    tests/test_switch_routes_cpu.py names UNREACHED"""
    from tests import switch_routes as R
    from tests.test_switch_routes_cpu import UNREACHED
    arms = R.header_arms()
    return tuple({a for a in arms[k] if a & 7 != 0 and (k, a) not in UNREACHED} for k in ("norm_fwd", "norm_bwd"))


# ------------------------------------------------------------------------------------------------------------------ A: conv epilogues
CONV_RATIO = {L.F32: 64.0, L.BF16: 16.0}
# (op, n, lh, cg, cd): the smallest shapes of test_igemm_fused_instance_norm_statistics whose epilogue offers slots at n <= 3
IGEMM_CASES = [(L.OP_G, 2, 8, 64, 128), (L.OP_P, 2, 8, 64, 128), (L.OP_G, 3, 16, 32, 64), (L.OP_P, 2, 32, 32, 128)]
STRIP_CASE = (L.OP_P, 2, 32, 32, 128)
# the block-resident fused kernel (bf16): with operands of mean ~1 the variance at mean / std = 16 is 4e-3, next to eps = 1e-3, and
# eps damps every error of it: plain f32 sums stay within 3-4x the rs bound.  Weights scaled by 32 (exact in bf16) lift the
# variance off eps, and mean / std = 64 (the issue allows up to 256) makes plain sums miss the bound >= 100x
FUSED_CASES = [(L.OP_P, 2, 16, 64, 96, L.ACT_RELU), (L.OP_G, 3, 8, 64, 256, L.ACT_LEAKY)]
FUSED_RATIO, FUSED_SCALE = 64.0, 32.0
# the same kernel's slot epilogue through p2p_igemm (op, n, lh, cg, cd): 8-wide maps (4 images per tile, ragged at n = 3), 16-wide,
# and 32-wide (strips of an image: several slots)
BRIG_CASES = [(L.OP_P, 3, 8, 64, 64), (L.OP_P, 2, 16, 64, 96), (L.OP_G, 2, 16, 64, 256), (L.OP_P, 2, 32, 64, 32)]
BORDER_TAP = 2.0 ** -8


def conv_operands(op, n, lh, lw, cg, cd, dtype, ratio, seed=47, scale=1.0):
    """(hi or lo input, w [4,4,cg,cd]) of a stride-2 block with POSITIVE operands whose output has mean / std ~ ratio per (image,
    channel).  Inputs (1 + a |zeta_yx|)(1 + 0.1 |xi|), weights b_i b_j (1 + 0.1 xi) / K with b = (2^-8, 1, 1, 2^-8): the outer taps
    are the ones a border pixel loses to the zero padding, so the border does not set the spread; the weight noise is shared by all
    pixels of a channel, so the per-pixel amplitude a sets it.  a is solved on the f64 graph (the caller passes the graph's
    conv) by bisection.  scale (a power of two) multiplies the weights: the output's mean, about 1.1, times scale.  Returns
    (input, w, the ratio reached)."""
    import torch
    from oracle import reference_graph as rg
    rng = np.random.default_rng([seed, op, n, lh, cg, cd, dtype])
    shape = (n, 2 * lh, 2 * lw, cg) if op == L.OP_G else (n, lh, lw, cd)
    zeta, xi = np.abs(rng.normal(size=shape[:3] + (1,))), np.abs(rng.normal(size=shape))
    b = np.array([BORDER_TAP, 1.0, 1.0, BORDER_TAP])
    k = 4 * (cg if op == L.OP_G else cd)
    w = U.q(b[:, None, None, None] * b[None, :, None, None] * (1 + 0.1 * rng.normal(size=(4, 4, cg, cd))) * (scale / k), dtype)
    conv = rg.conv4x4_s2 if op == L.OP_G else rg.convT4x4_s2
    wt = torch.tensor(w, dtype=torch.float64)

    def build(a):
        x = U.q((1 + a * zeta) * (1 + 0.1 * xi), dtype)
        y = conv(torch.tensor(x, dtype=torch.float64), wt).numpy()
        return x, float(np.median(np.abs(y.mean(axis=(1, 2))) / y.std(axis=(1, 2))))

    lo_a, hi_a = 1e-3, 4.0
    for _ in range(24):                    # the ratio falls as a grows: bisection in log a
        a = math.sqrt(lo_a * hi_a)
        x, r = build(a)
        if abs(r / ratio - 1) < 0.05:
            break
        lo_a, hi_a = (a, hi_a) if r > ratio else (lo_a, a)
    return x, w, r


def fused_graphs(op, a, w, gamma, beta, act, stats32=None):
    """the block conv -> bf16 store -> InstanceNorm -> activation on the operands of conv_operands: (the f64 graph's output, the
    max-norm deviation from it of the same graph evaluated by torch in float32 on the CPU and stored as bf16).  stats32: the float32
    statistics of the second graph (two_pass_f32; the CPU self-test passes plain_f32)."""
    import torch
    from oracle import reference_graph as rg
    conv = rg.conv4x4_s2 if op == L.OP_G else rg.convT4x4_s2
    x64 = U.q(conv(torch.tensor(a, dtype=torch.float64), torch.tensor(w, dtype=torch.float64)).numpy(), L.BF16)
    mean, rs, _ = stats64(x64)
    ref = apply64(x64, mean, rs, gamma, beta, act, None)
    x32 = U.q(conv(torch.tensor(a, dtype=torch.float32), torch.tensor(w, dtype=torch.float32)).numpy(), L.BF16)
    mu32, rs32 = (stats32 or two_pass_f32)(x32)
    out32 = U.q(apply_f32(x32, mu32, rs32, gamma, beta, act, None), L.BF16)
    return ref, U.rel_err(out32, ref)


# ------------------------------------------------------------------------------------------------------------------ B: losses
BCE_EDGES = (0.0, 1e-4, -1e-4, 20.0, -20.0, 88.0, -88.0, 104.0, -104.0, 3e4, -3e4)
TANH_EDGES = (0.0, 1e-3, -1e-3, 10.0, -10.0, 20.0, -20.0, 90.0, -90.0, 1e4, -1e4)


def embed(field, edges, rng, copies):
    """field with `copies` of every edge value written at seeded distinct positions (in place on a copy); returns it and the flat
    positions [len(edges), copies]"""
    out = np.array(field, np.float64)
    pos = rng.permutation(out.size)[:len(edges) * copies].reshape(len(edges), copies)
    flat = out.reshape(-1)
    for e, p in zip(edges, pos):
        flat[p] = e
    return out, pos


def bce_logits(dtype, n2=6, h=8, seed=51):
    """[n2,h,h,1] N(0, 3) logits with every BCE_EDGES value in both halves (real: images < n2 / 2, fake: the rest)"""
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(n2, h, h, 1)) * 3
    half = n2 // 2 * h * h
    a, _ = embed(x.reshape(-1)[:half], BCE_EDGES, rng, 2)
    b, _ = embed(x.reshape(-1)[half:], BCE_EDGES, rng, 2)
    return U.q(np.concatenate([a, b]).reshape(n2, h, h, 1), dtype)


def tanh_field(dtype, n=3, s=16, c=4, seed=52):
    """z [n,s,s,c] ~ N(0, 1) with every TANH_EDGES value 8 times, and their flat positions"""
    rng = np.random.default_rng(seed)
    z, pos = embed(rng.normal(size=(n, s, s, c)), TANH_EDGES, rng, 8)
    return U.q(z, dtype), pos


def bce64(x, z):
    """np_restatement.bce_from_logits without the mean: per-element, f64"""
    x = np.asarray(x, np.float64)
    return np.maximum(x, 0) - x * z + np.log1p(np.exp(-np.abs(x)))


def sigmoid64(x):
    x = np.asarray(x, np.float64)
    e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


# ------------------------------------------------------------------------------------------------------------------ C: Adam
ADAM_EDGES = np.array([0.0, 1e-30, -1e-30, 1e-18, -1e-18, 1.0, -1.0, 1e15, -1e15], np.float32)
ADAM_N = 1031            # not a multiple of the 4-float vector
ADAM_HOLE = (301, 402)   # unaligned at both ends


def adam_gradients(seed=53):
    """three gradient vectors [3, ADAM_N] drawn from ADAM_EDGES, neighbours independent (every 16-byte vector mixes magnitudes).
    Elements [0, 64): g = 0 in all three steps.  Elements [64, 128): non-zero in step 1, 0 afterwards."""
    rng = np.random.default_rng(seed)
    g = ADAM_EDGES[rng.integers(0, len(ADAM_EDGES), size=(3, ADAM_N))]
    g[:, :64] = 0.0
    g[0, 64:128] = ADAM_EDGES[1 + rng.integers(0, len(ADAM_EDGES) - 1, size=64)]
    g[1:, 64:128] = 0.0
    return g


def adam_reference(p0, g, steps=3, lr=2e-4, b1=0.5, b2=0.999, eps=1e-7):
    """[(p, m, v)] after each step, np_restatement.keras_adam_step in f64 from zero moments"""
    p, m, v = np.asarray(p0, np.float64), np.zeros(len(p0)), np.zeros(len(p0))
    out = []
    for t in range(1, steps + 1):
        p, m, v = npr.keras_adam_step(p, np.asarray(g[t - 1], np.float64), m, v, t, lr, b1, b2, eps)
        out.append((p, m, v))
    return out


F32_TINY = float(np.finfo(np.float32).tiny)       # a moment below the smallest normal float32 may be flushed to 0


# ------------------------------------------------------------------------------------------------------------------ D: colour points
def _colours(rng, k):
    """k distinct RGB colours in [-1, 1], multiples of 1/64 (exact in f32)"""
    idx = rng.permutation(129 ** 3)[:k]
    return np.stack([idx % 129, idx // 129 % 129, idx // 129 // 129], axis=1).astype(np.float32) / 64.0 - 1.0


def _image_of(colours, tile_pixels, rng):
    """tile_pixels pixels that show every one of the colours at least once"""
    k = len(colours)
    idx = np.concatenate([np.arange(k), rng.integers(0, k, size=tile_pixels - k)])
    return colours[rng.permutation(idx)]


def points_batch(size, seed=54):
    """four size x size RGBA images (alpha 1) and the npoints a list of capacity 64 must report.  The list is built per tile of
    1024 consecutive pixels and tiles are not merged:
      32x32 (one tile):   exactly 64 colours -> 64;  65 colours -> -1;  one colour, all -1 -> 1;  every pixel its own -> -1
      64x64 (four tiles): 16 colours per tile (disjoint) -> 64;  16, 16, 16, 17 -> -1;  one colour -> 4;  every pixel its own -> -1"""
    rng = np.random.default_rng([seed, size])
    tiles = size * size // 1024
    per_tile = 64 // tiles
    imgs, want = [], []
    for extra in (0, 1):
        cols = _colours(rng, 64 + extra)
        parts = [_image_of(cols[t * per_tile:(t + 1) * per_tile + (extra if t == tiles - 1 else 0)], 1024, rng) for t in range(tiles)]
        imgs.append(np.concatenate(parts))
        want.append(64 if not extra else -1)
    imgs.append(np.full((size * size, 3), -1.0, np.float32))
    want.append(tiles)
    imgs.append(_colours(rng, size * size))
    want.append(-1)
    rgb = np.stack(imgs).reshape(4, size, size, 3)
    return np.concatenate([rgb, np.ones((4, size, size, 1), np.float32)], axis=-1).astype(np.float32), np.array(want, np.int32)
