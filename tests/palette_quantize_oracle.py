"""Helper of tests/test_palette_quantize_*.py: p2p_palette_quantize (the comment in include/p2pgan.h) restated by brute
force in numpy -- int64 everywhere, np.unique for the colour set, argmin / argmax over explicit distance tables -- with a trace of
what every pass met, and the inputs the CPU and GPU tests share."""
import collections

import numpy as np

from tests import palette_snap_oracle as SO

Quantized = collections.namedtuple("Quantized", "palette size iters trace")


def pack(colours):
    """r + 256 g + 65536 b + 2^24 a of (n, 4) colours, int64"""
    c = np.asarray(colours, np.int64).reshape(-1, 4)
    return c[:, 0] + 256 * c[:, 1] + 65536 * c[:, 2] + (1 << 24) * c[:, 3]


def unpack(keys):
    k = np.asarray(keys, np.int64)
    return np.stack([k & 255, (k >> 8) & 255, (k >> 16) & 255, k >> 24], axis=-1)


def _dist(q, C):
    """(pixels, slots) table of D(q_p, C_k)"""
    return ((q[:, None, :] - C[None, :, :]) ** 2).sum(-1)


def quantize_image(img, colours, iterations, init=None, K=256):
    """One image (H, W, 4) float32 -> Quantized(palette (K, 4) int32, size, iters, trace).  `init` is None or (rows (K', 4), size).
    trace: {"exact": bool, "farthest_tie": [bool per selection step], "passes": [{"counts": n_k, "pixel_tie": bool}, ...]}"""
    assert 1 <= colours <= K <= 256 and 0 <= iterations <= 64
    q = SO.quantise(np.asarray(img, np.float32).reshape(-1, 4))          # (HW, 4) int64
    keys = pack(q)
    U = np.unique(keys)
    palette = np.zeros((K, 4), np.int32)
    trace = {"exact": len(U) <= colours, "farthest_tie": [], "passes": []}
    if len(U) <= colours:
        palette[:len(U)] = unpack(U)
        return Quantized(palette, len(U), 0, trace)
    n0 = 0
    if init is not None:
        rows, size = init
        n0 = min(max(int(size), 0), K)
    if n0 > 0:
        n = min(n0, colours)
        C = np.asarray(rows, np.int64)[:n] & 255
    else:
        n = colours
        C = np.zeros((n, 4), np.int64)
        C[0] = unpack(U[0])
        m = None
        for j in range(1, n):
            d = _dist(q, C[j - 1:j])[:, 0]
            m = d if m is None else np.minimum(m, d)
            top = int(m.max())
            assert top > 0
            cands = np.unique(keys[m == top])
            trace["farthest_tie"].append(len(cands) > 1)
            C[j] = unpack(cands[0])
    iters = 0
    for t in range(1, iterations + 1):
        D = _dist(q, C)
        a = D.argmin(axis=1)                                              # the lowest index among equals
        best = D[np.arange(len(a)), a]
        counts = np.bincount(a, minlength=n)
        trace["passes"].append({"counts": counts.tolist(), "pixel_tie": bool(((D == best[:, None]).sum(1) > 1).any())})
        new = C.copy()
        for k in range(n):
            if counts[k]:
                S = q[a == k].sum(0)
                new[k] = (2 * S + counts[k]) // (2 * counts[k])
        iters = t
        same = np.array_equal(new, C)
        C = new
        if same:
            break
    out = np.unique(pack(C))
    palette[:len(out)] = unpack(out)
    return Quantized(palette, len(out), iters, trace)


def quantize(img, colours, iterations, init_palette=None, init_sizes=None, K=256):
    """A batch (B, H, W, 4) -> (palette (B, K, 4) int32, sizes (B,) int32, iters (B,) int32, [trace per image])"""
    img = np.asarray(img, np.float32)
    res = []
    for b in range(img.shape[0]):
        init = None if init_palette is None else (init_palette[b], K if init_sizes is None else init_sizes[b])
        res.append(quantize_image(img[b], colours, iterations, init, K))
    return (np.stack([r.palette for r in res]), np.array([r.size for r in res], np.int32), np.array([r.iters for r in res], np.int32),
            [r.trace for r in res])


# ------------------------------------------------------------------------------------------------------------ shared inputs
def lattice_image(seed, levels, step, shape=(4, 4)):
    """pixels on a small colour lattice: channel values integers(0, levels) * step"""
    rng = np.random.default_rng(seed)
    return SO.normalise(rng.integers(0, levels, size=(*shape, 4)) * step)


def small_values_image(seed=4):
    """a 4 x 4 image of values in +-0.2: 8-bit values near 128"""
    return np.random.default_rng(seed).uniform(-0.2, 0.2, size=(4, 4, 4)).astype(np.float32)


EMPTY_SLOT_INIT = np.array([[0, 0, 0, 0], [128] * 4, [128] * 4, [255] * 4], np.int32)


def noise_image(seed, H, W):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, size=(H, W, 4)).astype(np.float32)


def sprite_like_image(seed, S=64, colours=12, sigma=0.03, transparent=0.8):
    """`colours` - 1 random opaque colours on a transparent-black ground that covers `transparent` of the image, every channel of
    every pixel with N(0, sigma) noise, clipped to [-1, 1]; returns (image, the true colours (colours, 4))"""
    rng = np.random.default_rng(seed)
    true = rng.integers(0, 256, size=(colours, 4))
    true[:, 3] = 255
    true[0] = 0
    idx = np.where(rng.random((S, S)) < transparent, 0, rng.integers(1, colours, size=(S, S)))
    img = SO.normalise(true[idx]) + rng.normal(0.0, sigma, size=(S, S, 4))
    return np.clip(img, -1.0, 1.0).astype(np.float32), true


def edge_batch():
    """(3, 7, 9, 4): an all-NaN image; uniform noise (the one image with starting slots in `init`); an image with the extremes +-1 / +-inf / 3.0 among coarse noise"""
    rng = np.random.default_rng(21)
    img = rng.uniform(-1.0, 1.0, size=(3, 7, 9, 4)).astype(np.float32)
    img[0] = np.nan
    flat = img[2].reshape(-1, 4)
    flat[0], flat[1], flat[2] = 1.0, -1.0, [3.0, -3.0, np.inf, -np.inf]
    flat[3] = [-1.0, 1.0, -1.0, 1.0]
    init = rng.integers(0, 256, size=(3, 5, 4)).astype(np.int32)
    return img, init, np.array([0, 5, -1], np.int32)
