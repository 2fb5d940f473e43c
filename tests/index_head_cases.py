"""Case builders and float64 references of the palette-index head tests: inputs on which the argmax is known exactly.  Host only
(tests/test_index_head_cases_cpu.py proves from NumPy that the cases can fail; tests/test_index_head_gpu.py runs the kernels).

A. Softmax kernels (p2p_softmax_cce_argmax, p2p_argmax_lastdim): quarter-step logits z = k / 4, k a uniform integer in [-32, 32].
   Every value is exact in f32 and in bf16.  Equal logits give bit-equal probabilities and the runner-up of a pixel is at most
   exp(-0.25) of its top, so the kernel's argmax of exp(z - max) / sum must be the FIRST MAXIMUM OF z on every pixel: no pixel is
   excluded.  With C = 256 draws from 65 values about 92 % of the pixels attain their maximum at least twice (72 % at C = 100,
   42 % at C = 65 -- the share of a case is the case's own property, tied_share; a tie needs two classes, so C = 1 has none).

B. Fused head (p2p_head_softmax_cce): integer-lattice operands (tests/lattice.py, ALPHABETS[0]) with the powers of two fixed per
   case.  x in (-3..3 without 0) * sx and w in (-2..2) * sw on the 33 real channels of the 40-channel pixel (pad channels and their
   weights zero), the bias an integer in [-3, 3] times the logit step sx * sw.  K = 16 * 33 = 528 products of at most 6 steps:
   every partial sum is far below 2^24 steps, so the f32 logits are exact in any order and step_launches.conv_g (float64) gives them
   bit for bit.  Distinct logits differ by at least one step (>= 2^-4), far beyond the error of a fast exponential, so the argmax
   is again the first maximum of the exact logits on every pixel.  The integer logits have a standard deviation of 70 steps inside an image
   (sqrt(528 * 14/3 * 2)) and about 65 over these short images, whose border pixels sum fewer taps:
     moderate    step 2^-4 / 2^-3: standard deviation about 4.1 / 7.6
     saturated   step 1: most random targets sit more than 104 below the maximum, where exp(z_t - max) is 0 in f32 and a
                 -log(p_t) form of the loss returns inf
     duplicated  weight column and bias of channel c copied from channel map(c): every pixel ties exactly between the members of
                 a class group, and the lowest member must win.  One map per exchange level of the fused kernel, whose lane holds
                 channel 128 cw + 4 h + 32 i + (e & 3) + 8 (e >> 2):  c & ~1 in-lane (e), c & ~4 lane ^ 32 (h), c & ~32 next channel
                 tile (i), c & 127 partner wave through LDS (cw), c & 63 a four-way tie across the tiles and the waves.
   Targets: t = (37 * pixel index) mod 256.  37 is odd, so every class is a target within any 256 consecutive pixels and the walk
   visits every lane position of the kernel's target match.

The wrong kernels at the end restate three plausible defects; the CPU test asserts that each of them disagrees with the reference
on the tie cases (the saturated case for the loss), which is how the cases prove that they can fail.
"""
import functools

import numpy as np

from tests import lattice as LT
from tests import step_launches as SL

K_LIM = 32                 # z = k / 4, k in [-K_LIM, K_LIM]
TARGET_STRIDE = 37
EXP_UNDERFLOW = -104.0     # exp(d) == 0 in f32 below this (2^-150 = exp(-103.97))

# (N, H, W) of the softmax tests: a single pixel (one 16-lane group or wave busy), part of a wave, one pixel over a 16-pixel
# workgroup, a column of 67 pixels (several workgroups, the last one partly idle), a ragged batch of three images
SOFTMAX_SHAPES = ((1, 1, 1), (1, 1, 3), (1, 1, 17), (1, 67, 1), (3, 5, 7))


# ------------------------------------------------------------------------------------------------------------------ A: softmax
def targets(n, h, w, c=256):
    """t = (37 * pixel index) mod c, int64 [n, h, w]"""
    return ((TARGET_STRIDE * np.arange(n * h * w, dtype=np.int64)) % c).reshape(n, h, w)


TIE_CLASSES = 100          # from this class count on a case is a TIE CASE: redrawn until it has the two properties below
TIE_SHARE, SPLIT_SHARE = 0.5, 0.1


@functools.lru_cache(maxsize=None)
def quarter_logits(n, h, w, c, seed=0):
    """float32 [n, h, w, c] of k / 4 (read-only: shared between the tests of a shape).  A tie case (c >= TIE_CLASSES) is drawn
    again, deterministically, until at least half of its pixels attain their maximum twice and at least a tenth of them attain
    it in both halves of the classes (a case of one or three pixels does not have that by itself; the large ones have it at the
    first draw)"""
    for attempt in range(64):
        rng = np.random.default_rng([seed, n, h, w, c, attempt])
        z = (rng.integers(-K_LIM, K_LIM + 1, size=(n, h, w, c)) / 4.0).astype(np.float32)
        if c < TIE_CLASSES or (tied_share(z) >= TIE_SHARE and split_tie_share(z) >= SPLIT_SHARE):
            z.setflags(write=False)
            return z
    raise AssertionError(f"no tie case of shape {(n, h, w, c)} in 64 draws")


def split_tie_share(z):
    """the share of pixels whose maximum is attained in the lower AND in the upper half of the classes"""
    z = np.asarray(z)
    top = z == z.max(-1, keepdims=True)
    half = (z.shape[-1] + 1) // 2
    return float((top[..., :half].any(-1) & top[..., half:].any(-1)).mean())


def first_max(z):
    """tf.argmax semantics: the lowest index among the maxima of the last axis"""
    return np.argmax(np.asarray(z), axis=-1).astype(np.int64)


def tied_share(z):
    """the share of pixels whose maximum is attained at least twice"""
    z = np.asarray(z)
    return float(((z == z.max(-1, keepdims=True)).sum(-1) >= 2).mean())


def softmax_ref(z, t, grad_scale, want_probs=True):
    """float64 reference of the softmax kernels on logits z [.., C] and targets t [..]:
    idx (first maximum of z), cce = log sum exp(z - max) - (z_t - max) and l1 = sum_c |onehot - p| per pixel, p, and
    dz = grad_scale * (p - onehot)"""
    z = np.asarray(z, np.float64)
    t = np.asarray(t, np.int64)
    d = z - z.max(-1, keepdims=True)
    e = np.exp(d)
    s = e.sum(-1, keepdims=True)
    p = e / s
    onehot = np.zeros_like(p)
    np.put_along_axis(onehot, t[..., None], 1.0, -1)
    out = {"idx": first_max(z), "cce": np.log(s[..., 0]) - np.take_along_axis(d, t[..., None], -1)[..., 0],
           "l1": np.abs(onehot - p).sum(-1), "dz": grad_scale * (p - onehot)}
    if want_probs:
        out["p"] = p
    return out


def losses(ref, inv_count, c):
    """(loss_out[0], loss_out[1]) of a launch from the per-pixel terms of softmax_ref"""
    return inv_count * float(ref["cce"].sum()), inv_count / c * float(ref["l1"].sum())


# ------------------------------------------------------------------------------------------------------------------ B: fused head
HEAD_W, HEAD_CIN, HEAD_CPAD, HEAD_NCLS = 64, 33, 40, 256
DUP_MAPS = {"inlane": lambda c: c & ~1, "lane32": lambda c: c & ~4, "tile": lambda c: c & ~32, "wave": lambda c: c & 127,
            "fourway": lambda c: c & 63}
# the class bit(s) that tell the members of a group apart: a tie-break that prefers the half with the bit SET is wrong there
DUP_BITS = {"inlane": (1,), "lane32": (4,), "tile": (32,), "wave": (128,), "fourway": (64, 128)}


class HeadCase:
    """one p2p_head_softmax_cce launch: n images of h x 64; sx = 2^ax (activations), sw = 2^-bw (weights), dup: a key of DUP_MAPS"""

    def __init__(self, name, n, h, ax, bw, dup=None, seed=0):
        self.name, self.n, self.h, self.ax, self.bw, self.dup, self.seed = name, n, h, ax, bw, dup, seed
        self.sx, self.sw = 2.0 ** ax, 2.0 ** -bw
        self.step = self.sx * self.sw

    @property
    def id(self):
        return f"{self.name}-n{self.n}-h{self.h}"


HEAD_CASES = ([HeadCase("moderate", 1, 4, 1, 4, seed=1), HeadCase("moderate", 2, 8, 0, 4, seed=2), HeadCase("moderate", 3, 12, 2, 6, seed=3),
               HeadCase("saturated", 2, 8, 2, 2, seed=4)] +
              [HeadCase("dup_" + k, 2, 8, 0, 4, dup=k, seed=5 + i) for i, k in enumerate(DUP_MAPS)])


@functools.lru_cache(maxsize=None)
def head_operands(case):
    """(x [n,h,64,33], w [4,4,33,256] HWIO, bias [256], z float64 [n,h,64,256], t int64 [n,h,64]); everything read-only.
    z = conv_g(x, w) + bias is asserted to be on the lattice and exact in f32."""
    rng = np.random.default_rng([case.seed, case.n, case.h])
    xs, ws = LT.ALPHABETS[0]
    x = (rng.choice(np.asarray(xs, np.int64), size=(case.n, case.h, HEAD_W, HEAD_CIN)) * case.sx).astype(np.float32)
    w = (rng.choice(np.asarray(ws, np.int64), size=(4, 4, HEAD_CIN, HEAD_NCLS)) * case.sw).astype(np.float32)
    bias = LT.small_ints(rng, HEAD_NCLS, case.step)
    if case.dup:
        src = DUP_MAPS[case.dup](np.arange(HEAD_NCLS))
        w, bias = np.ascontiguousarray(w[..., src]), bias[src].copy()
    for v in (x, w):
        assert np.array_equal(SL.bf16_round(v), v), "a lattice value is no bf16 value"
    z = SL.conv_g(x, w, 1) + bias.astype(np.float64)
    zi = LT.to_int(z, case.step)                    # (asserts that every logit is on the lattice)
    assert 16 * HEAD_CIN * 6 + 3 < 2 ** 24 and np.abs(zi).max() < 2 ** 24
    assert np.array_equal(z.astype(np.float32).astype(np.float64), z), "an exact logit is no f32 value"
    t = targets(case.n, case.h, HEAD_W, HEAD_NCLS)
    for v in (x, w, bias, z, t):
        v.setflags(write=False)
    return x, w, bias, z, t


def saturated_share(z, t):
    """the share of pixels whose target logit is more than 104 below the maximum: exp(z_t - max) is 0 in f32"""
    z = np.asarray(z, np.float64)
    zt = np.take_along_axis(z, np.asarray(t, np.int64)[..., None], -1)[..., 0]
    return float((zt - z.max(-1) < EXP_UNDERFLOW).mean())


# ------------------------------------------------------------------------------------------------------------------ wrong kernels
def argmax_ties_highest(z):
    """'>=' for '>': the highest index among the maxima"""
    z = np.asarray(z)
    return (z.shape[-1] - 1 - np.argmax(z[..., ::-1], axis=-1)).astype(np.int64)


def argmax_upper_half_preferred(z, bit=None):
    """the lowest index within each half, but on a tie BETWEEN the halves the upper one wins (a dropped 'oi < besti' or a '>=' in
    one exchange level).  The halves are the classes with `bit` clear / set; default: the lower and the upper half of the classes"""
    z = np.asarray(z, np.float64)
    c = np.arange(z.shape[-1])
    upper = (c & bit) != 0 if bit is not None else c >= (z.shape[-1] + 1) // 2
    if not upper.any():
        return first_max(z)
    lo, hi = np.where(upper, -np.inf, z), np.where(upper, z, -np.inf)
    i0, i1 = np.argmax(lo, -1), np.argmax(hi, -1)
    return np.where(hi.max(-1) >= lo.max(-1), i1, i0).astype(np.int64)


def softmax_f32(z):
    """exp(z - max) / sum restated in float32 (the form both kernels evaluate)"""
    z = np.asarray(z, np.float32)
    e = np.exp(z - z.max(-1, keepdims=True), dtype=np.float32)
    return (e / e.sum(-1, keepdims=True, dtype=np.float32)).astype(np.float32)


def cce_from_probability_f32(z, t):
    """-log(p_t) from the f32 probability: inf where p_t underflowed (the form the kernels must NOT use)"""
    pt = np.take_along_axis(softmax_f32(z), np.asarray(t, np.int64)[..., None], -1)[..., 0]
    with np.errstate(divide="ignore"):
        return -np.log(pt.astype(np.float32))
