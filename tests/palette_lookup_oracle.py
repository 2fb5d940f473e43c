"""Numpy restatement of the palette lookup (include/p2pgan.h p2p_palette_lookup_fwd / _bwd) and the inputs its tests
share: no torch, no GPU.

    t_k = palette_k / 127.5 - 1 per channel; with `blacken` the RGB of a slot whose alpha is 0 counts as 0
    soft    out_p = sum_k probs_pk t_k
    hard    out_p = t_argmax_k probs_pk, ties to the lowest k
    VJP     dprobs_pk = ((g_p0 t_k0 + g_p1 t_k1) + g_p2 t_k2) + g_p3 t_k3

`lookup64` is the reference (float64 throughout), `lookup32` the YARDSTICK: the same sum in float32, slots added one by one in
ascending k.  `lookup32_butterfly` restates the order the kernel uses (four FMAs per lane and channel, then a 64-lane xor butterfly)
to show where that order sits against the yardstick; it emulates an f32 FMA through float64, which double-rounds in rare cases, so
it is printed and never asserted bit for bit.  `hard_lookup` and `vjp32` are exact restatements: the kernels must match them bit
for bit."""
import functools

import numpy as np

K = 256
FILLER = (255, 0, 220, 255)                 # the reference's INVALID_INDEX_COLOR pads every palette to 256 rows
CASES = {"1x1x1": (1, 1, 1), "2x3x5": (2, 3, 5), "3x7x33": (3, 7, 33), "2x64x64": (2, 64, 64)}
SPREADS = (1, 4, 12)                        # standard deviation of the logits behind the probabilities
F32 = np.float32


def colours(palette, blacken, dtype=F32):
    """t (N, K, 4) in `dtype`: one division and one subtraction, each rounded to `dtype`"""
    pal = np.array(palette, dtype=np.int64)
    if blacken:
        pal[pal[..., 3] == 0, :3] = 0
    return (pal.astype(dtype) / dtype(127.5) - dtype(1.0)).astype(dtype)


def lookup64(probs, palette, blacken):
    return np.einsum("nhwk,nkc->nhwc", np.asarray(probs, np.float64), colours(palette, blacken, np.float64))


def lookup32(probs, palette, blacken):
    """float32, slots added in ascending k, every product and every sum rounded on its own"""
    p, t = np.asarray(probs, F32), colours(palette, blacken)
    acc = np.zeros(p.shape[:3] + (4,), F32)
    for k in range(K):
        acc = acc + p[..., k, None] * t[:, None, None, k, :]
    return acc


def _fma32(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F32)


def lookup32_butterfly(probs, palette, blacken):
    """the kernel's order: lane l takes slots 4l .. 4l+3 (four FMAs from 0), then lanes are added pairwise at xor offsets 32 .. 1"""
    p, t = np.asarray(probs, F32), colours(palette, blacken)
    N, H, W, _ = p.shape
    lanes = np.zeros((N, H, W, 64, 4), F32)
    for s in range(4):
        lanes = _fma32(p[..., s::4, None], t[:, None, None, s::4, :], lanes)
    o = 32
    while o:
        idx = np.arange(64) ^ o
        lanes = lanes + lanes[..., idx, :]
        o >>= 1
    return lanes[..., 0, :]


def hard_lookup(probs, palette, blacken):
    """(colours of the argmax, the argmax): np.argmax returns the first of equal maxima"""
    idx = np.argmax(np.asarray(probs, F32), axis=-1)
    t = colours(palette, blacken)
    n = np.arange(t.shape[0])[:, None, None]
    return t[n, idx], idx


def vjp32(g, palette, blacken):
    g, t = np.asarray(g, F32), colours(palette, blacken)
    tk = t[:, None, None, :, :]                                     # (N, 1, 1, K, 4)
    gp = g[..., None, :]                                            # (N, H, W, 1, 4)
    return ((gp[..., 0] * tk[..., 0] + gp[..., 1] * tk[..., 1]) + gp[..., 2] * tk[..., 2]) + gp[..., 3] * tk[..., 3]


def vjp64(g, palette, blacken):
    return np.einsum("nhwc,nkc->nhwk", np.asarray(g, np.float64), colours(palette, blacken, np.float64))


# ---------------------------------------------------------------------------------------------------- inputs
def palettes(rng, N):
    """(palette int32 (N, K, 4), number of real colours per image): 5..40 real colours, then the filler.  Slot 0 is transparent black
    as in the indexed pipeline; two more real slots are transparent with RGB that is NOT 0 (only `blacken` makes them black)."""
    pal = np.tile(np.array(FILLER, np.int32), (N, K, 1))
    sizes = rng.integers(5, 41, size=N)
    for n, m in enumerate(sizes):
        pal[n, :m, :3] = rng.integers(0, 256, size=(m, 3))
        pal[n, :m, 3] = 255
        pal[n, 0] = 0
        pal[n, 2] = (200, 30, 90, 0)
        pal[n, m - 1] = (7, 250, 1, 0)
    return pal, sizes


def _softmax_rows(rng, shape, s, sizes):
    z = rng.normal(0.0, s, size=shape + (K,))
    flat = z.reshape(shape[0], -1, K)
    for n in range(shape[0]):
        third = np.arange(1, flat.shape[1], 3)                      # every third pixel: its mass on one filler slot
        flat[n, third, rng.integers(sizes[n], K, size=len(third))] += 3.0 * s + 4.0
    z -= z.max(-1, keepdims=True)
    e = np.exp(z)
    return (e / e.sum(-1, keepdims=True)).astype(F32)


@functools.lru_cache(maxsize=None)
def case(name, s):
    """(probs f32 (N, H, W, K), palette, g f32 (N, H, W, 4), sizes) of the soft tests: softmax of N(0, s^2) logits over all 256
    slots, every third pixel with most of its mass on a filler slot, every fifth an exact one-hot row (any slot, filler included)"""
    N, H, W = CASES[name]
    rng = np.random.default_rng(1000 * s + 7 * N + H * W)
    pal, sizes = palettes(rng, N)
    probs = _softmax_rows(rng, (N, H, W), s, sizes)
    flat = probs.reshape(N, H * W, K)
    for n in range(N):
        fifth = np.arange(4, H * W, 5)
        hot = np.zeros((len(fifth), K), F32)
        hot[np.arange(len(fifth)), rng.integers(0, K, size=len(fifth))] = 1.0
        flat[n, fifth] = hot
    g = rng.normal(size=(N, H, W, 4)).astype(F32)
    for a in (probs, pal, g):
        a.setflags(write=False)
    return probs, pal, g, sizes


@functools.lru_cache(maxsize=None)
def hard_case(name):
    """(probs, palette, sizes) of the hard tests: rows at s = 4 with engineered ties in front of every image -- two equal maxima on
    filler slots (in different lanes of the kernel), all 256 equal, the maximum in the last slot, two equal maxima inside one lane's
    four slots, two equal maxima on real slots 64 lanes' width apart.  The single pixel of 1x1x1 is the first of them: a tie whose
    argmax is a filler slot."""
    N, H, W = CASES[name]
    rng = np.random.default_rng(77 + 7 * N + H * W)
    pal, sizes = palettes(rng, N)
    probs = _softmax_rows(rng, (N, H, W), 4, sizes)
    flat = probs.reshape(N, H * W, K)
    rows = np.tile(np.full(K, 0.5 / (K - 2), F32), (5, 1))
    rows[0, [130, 201]] = 0.25                                      # -> 130 (filler: at most 40 slots are real)
    rows[1, :] = F32(1.0 / K)                                       # -> 0
    rows[2, :] = 0.001
    rows[2, K - 1] = 0.745                                          # -> 255
    rows[3, [9, 10]] = 0.25                                         # -> 9 (lane 2 holds slots 8 .. 11)
    rows[4, [3, 1]] = 0.25                                          # -> 1
    rows[4, 131] = 0.25                                             # three equal maxima: 1, 3 and a filler slot
    for n in range(N):
        m = min(5, H * W)
        flat[n, :m] = rows[:m]
    for a in (probs, pal):
        a.setflags(write=False)
    return probs, pal, sizes


@functools.lru_cache(maxsize=None)
def reference(name, s, blacken):
    """(float64 forward, float32 yardstick: max |lookup32 - lookup64|) of a soft case, computed once"""
    probs, pal, _, _ = case(name, s)
    y64 = lookup64(probs, pal, blacken)
    yard = float(np.abs(lookup32(probs, pal, blacken).astype(np.float64) - y64).max())
    y64.setflags(write=False)
    return y64, yard
