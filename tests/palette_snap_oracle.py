"""Helper of tests/test_palette_snap_*.py: the palette snap of DESIGN.md "palette snap" by brute force in numpy (int64 differences,
argmin over the valid rows -- numpy's argmin returns the lowest index among equals), the packed key the kernel minimises, and the
engineered edge case the CPU and GPU tests share."""
import collections

import numpy as np

BIAS = 520200          # 2 * 4 * 255^2: keeps |c|^2 - 2 q.c + BIAS >= 0
Snap = collections.namedtuple("Snap", "index image distance counts off_palette distance_sum")


def quantise(img):
    """clamp(floor((v * 0.5 + 0.5) * 255 + 0.5), 0, 255) with every step in float32; NaN gives 0 (the kernel's fmaxf(NaN, 0))"""
    f = np.float32
    img = np.asarray(img, f)
    with np.errstate(invalid="ignore"):
        q = np.floor((img * f(0.5) + f(0.5)) * f(255) + f(0.5))
        q = np.where(np.isnan(q), f(0), q)
        return np.clip(q, 0, 255).astype(np.int64)


def normalise(c):
    """c / 127.5f - 1.0f as two float32 operations (the dataset's normalisation)"""
    return np.asarray(c).astype(np.float32) / np.float32(127.5) - np.float32(1.0)


def snap(img, palette, sizes=None):
    """img (B,H,W,4) float32, palette (B,K,4) ints 0..255, sizes (B,) ints or None -> Snap of numpy arrays"""
    img = np.asarray(img, np.float32)
    pal = np.asarray(palette, np.int64)
    B, H, W, _ = img.shape
    K = pal.shape[1]
    sizes = [K] * B if sizes is None else [int(s) for s in sizes]
    q = quantise(img)
    index = np.full((B, H, W), -1, np.int32)
    dist = np.zeros((B, H, W), np.int32)
    image = img.copy()
    counts = np.zeros((B, K), np.int32)
    off, dsum = np.zeros(B, np.int64), np.zeros(B, np.int64)
    for b in range(B):
        n = min(max(sizes[b], 0), K)
        if n == 0:
            continue
        D = ((q[b].reshape(-1, 1, 4) - pal[b, :n].reshape(1, n, 4)) ** 2).sum(-1)          # (HW, n) int64
        idx = D.argmin(axis=1)
        d = D[np.arange(len(idx)), idx]
        index[b] = idx.reshape(H, W)
        dist[b] = d.reshape(H, W)
        image[b] = normalise(pal[b][idx]).reshape(H, W, 4)
        counts[b] = np.bincount(idx, minlength=K)
        off[b], dsum[b] = (d > 0).sum(), d.sum()
    return Snap(index, image, dist, counts, off, dsum)


def packed_key_snap(q, pal):
    """(index, dist) of ONE quantised pixel q (4,) against pal (n, 4) through the kernel's packed key:
    word_k = ((|c_k|^2 + BIAS) << 8) | k,  key_k = word_k - (q.c_k << 9),  min over k in uint32 arithmetic."""
    q, pal = np.asarray(q, np.uint64), np.asarray(pal, np.uint64)
    word = (((pal * pal).sum(-1) + np.uint64(BIAS)) << np.uint64(8)) | np.arange(len(pal), dtype=np.uint64)
    assert word.max() < 2 ** 32
    key = (word - ((pal * q).sum(-1) << np.uint64(9))) & np.uint64(0xFFFFFFFF)          # the kernel's 32-bit wrap-around
    best = int(key.min())
    return best & 255, (best >> 8) - BIAS + int((q * q).sum())


def engineered_case():
    """(img (1,33,7,4), palette (1,256,4), sizes [256]): a palette with duplicate rows and engineered ties, pixels at 0 and 255 in
    every channel, one NaN pixel, noisy pixels elsewhere"""
    rng = np.random.default_rng(77)
    pal = rng.integers(0, 256, size=(1, 256, 4)).astype(np.int32)
    pal[0, 0] = [0, 0, 0, 0]
    pal[0, 1] = [255, 255, 255, 255]
    pal[0, 5] = pal[0, 3]                                  # duplicates: the lower slot wins
    pal[0, 200] = pal[0, 100]
    pal[0, 255] = pal[0, 0]
    pal[0, 10], pal[0, 11] = [100, 50, 50, 255], [104, 50, 50, 255]          # 102 is equidistant: slot 10
    pal[0, 21], pal[0, 20] = [30, 60, 90, 255], [30, 64, 90, 255]            # the same tie with the nearer-in-order slot second: 20
    pal[0, 30], pal[0, 31] = [10, 200, 10, 255], [12, 202, 10, 255]          # (11, 201) is 2 from both and (10, 202), (12, 200) too
    img = normalise(pal[0][rng.integers(0, 256, size=(33, 7))])[None]
    noisy = rng.random((1, 33, 7, 1)) < 0.5
    img = np.clip(img + noisy * rng.normal(0.0, 0.05, size=img.shape), -1.0, 1.0).astype(np.float32)
    flat = img.reshape(-1, 4)
    flat[0] = normalise([102, 50, 50, 255])
    flat[1] = normalise([30, 62, 90, 255])
    flat[2] = normalise([11, 201, 10, 255])
    flat[3] = -1.0                                         # 0 in every channel
    flat[4] = 1.0                                          # 255 in every channel
    flat[5] = np.nan                                       # quantises to 0, 0, 0, 0
    flat[6] = [-1.0, 1.0, -1.0, 1.0]
    flat[7] = [3.0, -3.0, np.inf, -np.inf]                 # clamped
    flat[230] = normalise(pal[0, 5])                       # a duplicate's colour: slot 3
    return img, pal, np.array([256], np.int32)
